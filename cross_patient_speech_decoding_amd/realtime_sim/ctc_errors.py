"""Edit-operation alignment on the device: the Levenshtein alignment of decoded against target sequences
(csrc/xps_edit_align.hip), i.e. which errors make up a PER -- hits, substitutions, deletions and insertions,
the map between the two sequences and the phoneme confusion matrix of a CTC decoder, whose decoded and target sequences
differ in length.  Integers throughout, in the table and tie rule of include/xps.h.  There is no CPU fallback; the shape,
length and label checks run before any device call."""
import torch

from .._dev import ptr, stream, workspace
from .._lib import call, lib
from ._ctc_host import EDIT_MAX_PRED, EDIT_MAX_TARGET, at, integer_tokens, labels_in_range, lengths, runs_within

MAX_WORKSPACE_BYTES = 1 << 30
OPS = ('hit', 'substitution', 'deletion', 'insertion')


class EditAlignment:
    """What edit_align returns (device tensors): distance (B,) int64, the edit distance of each pair; hits, substitutions,
    deletions, insertions (B,) int64 (hits + substitutions + deletions = the target's length, hits + substitutions +
    insertions = the prediction's, substitutions + deletions + insertions = distance); target_to_pred (B, L) int32, the
    index of the prediction token aligned to target token j, -1 for a deleted one, -2 past the target's length;
    pred_to_target (B, P) int32, the index of the target token aligned to prediction token i, -1 for an inserted one, -2 past
    the prediction's length; confusion (K + 1, K + 1) int64 over the whole batch, None without n_classes: row = target class,
    row K = no target (insertions), column = predicted class, column K = nothing (deletions), cell (K, K) always 0.
    pred (B, P), pred_lengths, targets (B, L) and target_lengths, int64, are the device copies the launch read."""

    def __init__(self, distance, counts, target_to_pred, pred_to_target, confusion, pred, pred_lengths, targets,
                 target_lengths):
        self.distance, self.counts = distance, counts
        self.hits, self.substitutions, self.deletions, self.insertions = counts.unbind(1)
        self.target_to_pred, self.pred_to_target, self.confusion = target_to_pred, pred_to_target, confusion
        self.pred, self.pred_lengths, self.targets, self.target_lengths = pred, pred_lengths, targets, target_lengths

    def per(self):
        """Phoneme error rate in percent, a 0-dim float64 device tensor: per_device's own expression on the same integers,
        so the two are equal bit for bit."""
        total = self.target_lengths.sum().double()
        return self.distance.sum().double() / total * 100

    def rates(self):
        """(3,) float64 device tensor: the substitutions, deletions and insertions of the batch, each as a share of its
        target tokens; the three add up to per() / 100 (up to rounding)."""
        total = self.target_lengths.sum().double()
        return self.counts[:, 1:].sum(0).double() / total

    def target_ops(self):
        """(B, L) int64 device tensor, what happened to each target token: 0 hit, 1 substitution, 2 deletion, -1 past the
        target's length.  From the map and the tokens."""
        m = self.target_to_pred.long()
        if self.pred.shape[1] == 0:
            sub = torch.zeros_like(m)
        else:
            got = torch.gather(self.pred, 1, m.clamp(min=0))
            sub = (got != self.targets).long()
        ops = torch.where(m == -1, torch.full_like(m, 2), sub)
        return torch.where(m == -2, torch.full_like(m, -1), ops)

    def position_error_rate(self):
        """(L,) float64 device tensor: of the targets that have a token at position j, the share whose token was substituted
        or deleted -- the per-position error of the three-phoneme tasks; NaN at a position no target reaches."""
        ops = self.target_ops()
        return (ops > 0).sum(0).double() / (ops >= 0).sum(0).double()

    def confusion_by(self, class_map):
        """Fold the (K + 1, K + 1) phoneme confusion into coarser classes: class_map (K,) integers, the class 0..G-1 of each
        label -> (G + 1, G + 1) int64 device tensor, G = max(class_map) + 1, with the insertion row and the deletion column
        kept as row / column G.  For the articulator classes of alignment_utils._PHON_TO_ARTIC (1-based phonemes to 1-based
        articulators) and 0-based labels p = phoneme - 1:
        class_map = [_PHON_TO_ARTIC[p + 1] - 1 for p in range(9)]; a label that is no phoneme (a blank) gets a class of its
        own."""
        if self.confusion is None:
            raise ValueError('confusion was not computed: pass n_classes to edit_align')
        K = self.confusion.shape[0] - 1
        cm = torch.as_tensor(class_map).detach().cpu().reshape(-1)
        if cm.is_floating_point() or cm.dtype == torch.bool:
            raise ValueError(f'class_map of dtype {cm.dtype}: expected integers')
        if cm.numel() != K:
            raise ValueError(f'class_map of {cm.numel()} entries for {K} classes')
        if int(cm.min()) < 0:
            raise ValueError('class_map holds a negative class')
        G = int(cm.max()) + 1
        idx = torch.cat([cm.to(torch.int64), torch.tensor([G])]).to(self.confusion.device)
        rows = torch.zeros(G + 1, K + 1, dtype=torch.int64, device=self.confusion.device).index_add_(0, idx, self.confusion)
        return torch.zeros(G + 1, G + 1, dtype=torch.int64, device=rows.device).index_add_(1, idx, rows)

    def pairs(self, b):
        """Pair b's alignment as a host list of (op, target_token, pred_token) from the start of the sequences to their
        end, op one of 'hit', 'substitution', 'deletion', 'insertion', the absent token None; between two aligned tokens the
        deletions are listed before the insertions.  For inspection: it copies the pair to the host."""
        m, n = int(self.pred_lengths[b]), int(self.target_lengths[b])
        a, t = self.pred[b, :m].tolist(), self.targets[b, :n].tolist()
        p2t = self.pred_to_target[b, :m].tolist()
        out, i, j = [], 0, 0
        while i < m or j < n:
            nxt = next((q for q in range(i, m) if p2t[q] >= 0), m)          # the next aligned prediction token
            stop = p2t[nxt] if nxt < m else n
            out += [(OPS[2], t[q], None) for q in range(j, stop)]
            out += [(OPS[3], None, a[q]) for q in range(i, nxt)]
            if nxt < m:
                out.append((OPS[0] if a[nxt] == t[stop] else OPS[1], t[stop], a[nxt]))
            i, j = nxt + 1, stop + 1
        return out


def workspace_runs(B, P, L, max_workspace_bytes):
    """Cut B pairs into runs [(start, stop), ...] whose backpointer workspace, P * L bytes per pair, stays within
    max_workspace_bytes; as few runs as that allows, of even size.  A single pair above the limit raises ValueError."""
    return runs_within(B, max(int(P), 0) * max(int(L), 0), max_workspace_bytes, f'one pair of up to {P} against {L} tokens')


def _check(pred, pred_lengths, targets, target_lengths, n_classes, max_workspace_bytes):
    """Every shape, length and label check of edit_align, on the host.  Returns (pred, targets, pred_lengths, target_lengths
    (host int64), runs)."""
    pred, targets = integer_tokens(pred, 'pred', 'two axes, (B, P)'), integer_tokens(targets, 'targets', 'two axes, (B, L)')
    if pred.size(0) != targets.size(0):
        raise ValueError(f'{pred.size(0)} predictions for {targets.size(0)} targets')
    B, P, L = pred.size(0), pred.size(1), targets.size(1)
    if P > EDIT_MAX_PRED or L > EDIT_MAX_TARGET:
        raise ValueError(f'edit alignment of up to {P} against {L} tokens: the kernel supports {EDIT_MAX_PRED} against '
                         f'{EDIT_MAX_TARGET}')
    if pred_lengths is None:
        raise ValueError('pred_lengths is needed: the padding of a decode carries no length')
    pl = lengths(pred_lengths, B, P, 'pred_lengths')
    tl = torch.full((B,), L, dtype=torch.int64) if target_lengths is None else lengths(target_lengths, B, L, 'target_lengths')
    if n_classes is not None:
        K = int(n_classes)
        if K < 1:
            raise ValueError(f'n_classes {n_classes}: a confusion matrix needs at least one class')
        labels_in_range(pred.detach().cpu().to(torch.int64), pl, K, 'prediction')
        labels_in_range(targets.detach().cpu().to(torch.int64), tl, K, 'target')
    return pred, targets, pl, tl, workspace_runs(B, P, L, max_workspace_bytes)


def edit_align(pred, pred_lengths, targets, target_lengths, n_classes=None, max_workspace_bytes=MAX_WORKSPACE_BYTES):
    """Levenshtein alignment of B padded pairs -> EditAlignment.  pred (B, P), an integer device tensor, and targets (B, L),
    integers (moved to pred's device), with their lengths (B,) (target_lengths None: all L); what lies past a length is
    never read (the -1 padding of greedy_decode_device is fine).
    n_classes = K asks for the (K + 1, K + 1) confusion matrix of the batch; every token within its length must then lie in
    0..K-1.  Shapes, lengths and labels are checked here, on the host (lengths, and with n_classes the tokens, are copied to
    the host for it, which waits for them); every check raises ValueError before any device call, and host tensors raise
    RuntimeError: there is no CPU fallback.
    max_workspace_bytes: the kernel keeps one backpointer byte per cell of each pair's table, P * L bytes per pair (64 MB
    for 2048 pairs at P = 512, L = 64; 470 KB at the training shape, 47 against 5), so the batch is cut into runs of pairs
    that stay within this limit, one launch per run on the same workspace, the confusion matrix accumulating across the
    runs; the results do not depend on the cut.  A single pair above the limit raises ValueError."""
    pred, targets, pl, tl, runs = _check(pred, pred_lengths, targets, target_lengths, n_classes, max_workspace_bytes)
    if not pred.is_cuda:
        raise RuntimeError('cross_patient_speech_decoding_amd: edit_align needs device tensors (no CPU fallback)')
    dev = pred.device
    B, P, L = pred.size(0), pred.size(1), targets.size(1)
    pred = pred.to(torch.int64).contiguous()
    targets = targets.to(dev, torch.int64).contiguous()
    pl_d, tl_d = pl.to(dev), tl.to(dev)
    dist = torch.empty(B, dtype=torch.int64, device=dev)
    counts = torch.empty(B, 4, dtype=torch.int64, device=dev)
    t2p = torch.empty(B, L, dtype=torch.int32, device=dev)
    p2t = torch.empty(B, P, dtype=torch.int32, device=dev)
    K = 0 if n_classes is None else int(n_classes)
    conf = None if n_classes is None else torch.zeros(K + 1, K + 1, dtype=torch.int64, device=dev)
    ws_bytes = max([int(lib().xps_edit_align_workspace(b1 - b0, P, L)) for b0, b1 in runs], default=0)
    ws = workspace(ws_bytes, dev)
    for b0, b1 in runs:
        call('xps_edit_align', at(pred, b0, P), P, at(pl_d, b0, 1), at(targets, b0, L), L, at(tl_d, b0, 1), b1 - b0, P, L, K,
             at(dist, b0, 1), at(counts, b0, 4), at(t2p, b0, L), at(p2t, b0, P), ptr(conf), ws.data_ptr(), ws_bytes,
             stream(dev))
    return EditAlignment(dist, counts, t2p, p2t, conf, pred, pl_d, targets, tl_d)
