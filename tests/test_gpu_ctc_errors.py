"""Edit-operation alignment on the MI355X (csrc/xps_edit_align.hip, realtime_sim/ctc_errors.py) against the numpy
restatement of the header's contract (tests/ctc_errors_ref.py, itself tied to a brute force in
tests/test_ctc_errors_host.py): the distance, the four counts, both maps and the confusion matrix EXACTLY equal on every
route of the kernel, then the C entry point's memory discipline and refusals and the two hooks.  Every quantity is an
integer: no tolerance appears."""
import functools

import numpy as np
import pytest
import torch

from ctc_errors_ref import edit_align_ref
from guarded_buf import SENT, Buf

pytestmark = pytest.mark.gpu


def _rt():
    from cross_patient_speech_decoding_amd import realtime_sim
    return realtime_sim


def _lib():
    from cross_patient_speech_decoding_amd._lib import lib
    return lib()


def _stream():
    from cross_patient_speech_decoding_amd._dev import stream
    return stream()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).cuda()


def _equal(ea, ref, what=''):
    """EditAlignment == edit_align_ref's tuple, exactly, and the count identities."""
    dist, counts, t2p, p2t, conf = ref
    assert ea.distance.dtype == torch.int64 and ea.counts.dtype == torch.int64
    assert ea.target_to_pred.dtype == torch.int32 and ea.pred_to_target.dtype == torch.int32
    assert np.array_equal(ea.distance.cpu().numpy(), dist), what
    assert np.array_equal(ea.counts.cpu().numpy(), counts), what
    assert np.array_equal(ea.target_to_pred.cpu().numpy(), t2p), what
    assert np.array_equal(ea.pred_to_target.cpu().numpy(), p2t), what
    for k, name in enumerate(('hits', 'substitutions', 'deletions', 'insertions')):
        assert np.array_equal(getattr(ea, name).cpu().numpy(), counts[:, k]), what
    if conf is None:
        assert ea.confusion is None
    else:
        assert ea.confusion.dtype == torch.int64 and np.array_equal(ea.confusion.cpu().numpy(), conf), what


def _run_and_compare(pred, pl, tgt, tl, K, what=''):
    """edit_align on the device == the restatement, and dist == xps_edit_distance_i64 on the same tensors."""
    rt = _rt()
    ref = edit_align_ref(pred, pl, tgt, tl, n_classes=K)
    p_d, t_d = _dev(pred), _dev(tgt)
    ea = rt.edit_align(p_d, pl, t_d, tl, n_classes=K)
    _equal(ea, ref, what)
    assert torch.equal(ea.distance, rt.edit_distance_device(p_d, pl, t_d, tl)), what
    c = ref[1]
    assert np.array_equal(c[:, 0] + c[:, 1] + c[:, 2], np.asarray(tl)) and np.array_equal(c[:, 0] + c[:, 1] + c[:, 3], np.asarray(pl))
    assert np.array_equal(c[:, 1] + c[:, 2] + c[:, 3], ref[0])
    return ea, ref


# ---- the ragged batch of the issue: B = 7, not a multiple of the 4 pairs per block -------------------------------------------
def _ragged(K):
    """(m, n) = (0, 0), (0, 3), (3, 0), (4, 4) equal, (4, 4) with no common symbol, (5, 2) over a one-symbol alphabet (every
    alignment ties), (1, 1).  The padding holds the valid label x: past a length it must change nothing."""
    x, y = K - 1, 0
    pred = np.array([[x] * 5, [x] * 5, [y, x, y, x, x], [y, x, x, y, x], [y, y, y, y, x], [x] * 5, [y, x, x, x, x]], np.int64)
    tgt = np.array([[x] * 4, [x, y, x, x], [x] * 4, [y, x, x, y], [x, x, x, x], [x, x, y, y], [x, y, y, y]], np.int64)
    return pred, [0, 0, 3, 4, 4, 5, 1], tgt, [0, 3, 0, 4, 4, 2, 1]


@pytest.mark.parametrize('K', [2, 11])
def test_ragged_batch_equals_restatement(K):
    pred, pl, tgt, tl = _ragged(K)
    ea, ref = _run_and_compare(pred, pl, tgt, tl, K)
    assert ref[0].tolist() == [0, 3, 3, 0, 4, 3, 1]
    assert ref[1].tolist() == [[0, 0, 0, 0], [0, 0, 3, 0], [0, 0, 0, 3], [4, 0, 0, 0], [0, 4, 0, 0], [2, 0, 0, 3], [0, 1, 0, 0]]
    # the one-symbol pair: the diagonal wins every tie, so the LAST two prediction tokens are the hits
    assert ref[2][5].tolist() == [3, 4, -2, -2] and ref[3][5].tolist() == [-1, -1, -1, 0, 1]
    assert ea.pairs(5) == [('insertion', None, K - 1)] * 3 + [('hit', K - 1, K - 1)] * 2
    assert ea.pairs(0) == [] and ea.pairs(1) == [('deletion', t, None) for t in tgt[1, :3].tolist()]
    assert ea.target_ops().tolist()[4] == [1, 1, 1, 1] and ea.target_ops().tolist()[1] == [2, 2, 2, -1]
    per = ea.per()
    assert per.dtype == torch.float64 and per.dim() == 0
    assert torch.equal(per, _rt().per_device(_dev(pred), pl, _dev(tgt), tl))
    assert ea.position_error_rate().tolist() == [3 / 5, 1 / 2, 2 / 3, 1 / 2]
    assert ea.rates().tolist() == [5 / 14, 3 / 14, 6 / 14]


# ---- route and chunk edges -----------------------------------------------------------------------------------------------------
def _random_pairs(rng, B, P, L, pl, tl, n_symbols):
    pred = rng.integers(0, n_symbols, (B, P))
    tgt = rng.integers(0, n_symbols, (B, L))
    return pred, np.asarray(pl), tgt, np.asarray(tl)


M_EDGES = [1, 63, 64, 65, 129]


@pytest.mark.parametrize('n', [63, 64, 65, 256, 257])
def test_chunk_and_route_edges(n):
    """Targets of n tokens padded to L = n (n = 64 | 65 and 256 | 257 are the edges of the 1-, 4- and 16-chunk routes, 63 | 64
    | 65 those of a chunk's lanes) against predictions of m = 1, 63, 64, 65, 129 tokens (the 64-token loads of the prediction);
    3 symbols, so ties are everywhere; the last pair repeats the target as its prediction."""
    rng = np.random.default_rng(n)
    pred, pl, tgt, tl = _random_pairs(rng, 6, 129, n, M_EDGES + [min(n, 129)], [n] * 5 + [n], 3)
    pred[5, :min(n, 129)] = tgt[5, :min(n, 129)]
    tl = tl.copy()
    tl[1] = n - 1                                                        # one target shorter than the padded extent
    _, ref = _run_and_compare(pred, pl, tgt, tl, 3, f'n = {n}')
    assert ref[0][5] == max(n - 129, 0)


def test_the_cap_1024_targets():
    rng = np.random.default_rng(1024)
    pred, pl, tgt, tl = _random_pairs(rng, 2, 64, 1024, [64, 37], [1024, 1000], 4)
    pred[0] = tgt[0, 500:564]                                            # 64 hits somewhere in the middle, 960 deletions
    _, ref = _run_and_compare(pred, pl, tgt, tl, 4)
    assert ref[0][0] == 960 and ref[1][0].tolist() == [64, 0, 960, 0]


@pytest.mark.parametrize('P,L', [(47, 5), (64, 64), (820, 5)])
def test_short_targets_and_the_same_pairs_in_wider_rows(P, L):
    """Targets far shorter than a wave (47 x 5 is the training shape; 59 of the 64 lanes hold no column), three workgroups with
    ragged lengths, and the same pairs again in rows padded by 800 more columns: a pair's results do not depend on the
    padded extent."""
    rng = np.random.default_rng(P * L)
    B = 9                                                                # three blocks, the last with one pair
    pl = [P, P - 1, 1, 0, P, P // 2, P, 3, P]
    tl = [L, L, L, L, 0, L - 1, 1, L, L]
    pred, pl, tgt, tl = _random_pairs(rng, B, P, L, pl, tl, 3)
    _, ref = _run_and_compare(pred, pl, tgt, tl, 3, f'P = {P}, L = {L}')
    wide = np.concatenate([pred, rng.integers(0, 3, (B, 800))], 1)
    ea = _rt().edit_align(_dev(wide), pl, _dev(tgt), tl, n_classes=3)
    assert np.array_equal(ea.pred_to_target.cpu().numpy()[:, :P], ref[3]) and bool((ea.pred_to_target[:, P:] == -2).all())
    assert np.array_equal(ea.target_to_pred.cpu().numpy(), ref[2]) and np.array_equal(ea.counts.cpu().numpy(), ref[1])
    assert np.array_equal(ea.confusion.cpu().numpy(), ref[4])


# ---- the C entry point: one guarded buffer, strides, NULL outputs, determinism, refusals ---------------------------------------
class _Launch:
    """dist, counts, tgt_to_pred, pred_to_tgt, confusion and the workspace in ONE guarded buffer of 32-bit words, gaps
    between them; the confusion matrix starts at zero (the kernel adds into it), everything else at the sentinel."""
    GAP = 16
    NAMES = ('dist', 'counts', 't2p', 'p2t', 'conf', 'ws')

    def __init__(self, B, P, L, K):
        self.B, self.P, self.L, self.K = B, P, L, K
        self.ws_bytes = int(_lib().xps_edit_align_workspace(B, P, L))
        sizes = [2 * B, 8 * B, B * L, B * P, 2 * (K + 1) ** 2, (self.ws_bytes + 3) // 4]
        self.off, n = [], 0
        for s in sizes:
            n += n % 2                                                   # 8-byte alignment (the int64 outputs)
            self.off.append(n)
            n += s + self.GAP
        self.sizes = sizes
        self.buf = Buf(n)
        self.live = np.zeros(n, bool)
        for o, s in zip(self.off, sizes):
            self.live[o:o + s] = True
        self.buf.view().view(torch.int32)[self.off[4]:self.off[4] + sizes[4]] = 0

    def ptr(self, name):
        return self.buf.ptr + 4 * self.off[self.NAMES.index(name)]

    def words(self):
        return self.buf.view().view(torch.int32).cpu().numpy()

    def part(self, name):
        i = self.NAMES.index(name)
        return self.words()[self.off[i]:self.off[i] + self.sizes[i]]

    def outputs(self):
        B, P, L, K = self.B, self.P, self.L, self.K
        return (self.part('dist').view(np.int64), self.part('counts').view(np.int64).reshape(B, 4),
                self.part('t2p').reshape(B, L), self.part('p2t').reshape(B, P),
                self.part('conf').view(np.int64).reshape(K + 1, K + 1))

    def run(self, pred, pl, tgt, tl, /, **kw):
        """One call of xps_edit_align on tensors; a keyword replaces the argument of that name."""
        a = dict(pred=pred.data_ptr(), pstride=pred.stride(0), pl=pl.data_ptr(), tgt=tgt.data_ptr(), tstride=tgt.stride(0),
                 tl=tl.data_ptr(), B=self.B, P=self.P, L=self.L, K=self.K, dist=self.ptr('dist'), counts=self.ptr('counts'),
                 t2p=self.ptr('t2p'), p2t=self.ptr('p2t'), conf=self.ptr('conf'), ws=self.ptr('ws'), ws_bytes=self.ws_bytes)
        a.update(kw)
        rc = _lib().xps_edit_align(a['pred'], a['pstride'], a['pl'], a['tgt'], a['tstride'], a['tl'], a['B'], a['P'], a['L'],
                                   a['K'], a['dist'], a['counts'], a['t2p'], a['p2t'], a['conf'], a['ws'], a['ws_bytes'],
                                   _stream())
        torch.cuda.synchronize()
        return rc


@functools.lru_cache(maxsize=None)
def _guarded_case(P, L):
    """B = 6 pairs over K = 5 classes in PITCHED rows (stride = extent + 3 / + 2) whose padding, past each length and past
    the extents, holds valid labels; two length entries lie above the extents and one below zero: they are clamped."""
    rng = np.random.default_rng(100 * P + L)
    B, K = 6, 5
    pred, tgt = rng.integers(0, K, (B, P + 3)), rng.integers(0, K, (B, L + 2))
    pl = np.array([P, P + 50, max(P // 2, 1), 0, 2, P])
    tl = np.array([L, L - 1, 2 ** 40, 3, -7, 1])
    ref = edit_align_ref(pred, pl, tgt, tl, P=P, L=L, n_classes=K)
    m, n = np.clip(pl, 0, P), np.clip(tl, 0, L)
    return pred, pl, tgt, tl, ref, (B, K), m, n


GUARDED_SHAPES = [(12, 7), (70, 66)]           # one chunk of target columns and two


@pytest.mark.parametrize('P,L', GUARDED_SHAPES)
def test_guarded_buffers_strides_clamping_and_determinism(P, L):
    pred, pl, tgt, tl, ref, (B, K), m, n = _guarded_case(P, L)
    dev = [_dev(a) for a in (pred, pl, tgt, tl)]
    before = [t.clone() for t in dev]
    # xps_edit_distance_i64 runs the row pass of a function that also holds the alignment's stores: dist, B int64 in the
    # middle of a guarded buffer, is all it may write
    gap = _Launch.GAP
    dbuf = Buf(2 * B + 2 * gap)
    assert _lib().xps_edit_distance_i64(dev[0].data_ptr(), P + 3, dev[1].data_ptr(), dev[2].data_ptr(), L + 2,
                                        dev[3].data_ptr(), B, P, L, dbuf.ptr + 4 * gap, _stream()) == 0
    torch.cuda.synchronize()
    assert dbuf.guards_intact(), 'xps_edit_distance_i64 wrote a guard row'
    dwords = dbuf.view().view(torch.int32).cpu().numpy()
    assert (dwords[:gap] == np.int32(SENT)).all() and (dwords[gap + 2 * B:] == np.int32(SENT)).all(), \
        'xps_edit_distance_i64 wrote outside dist'
    dist_kernel = torch.from_numpy(dwords[gap:gap + 2 * B].view(np.int64).copy())
    assert np.array_equal(dist_kernel.numpy(), ref[0])
    for t, b4 in zip(dev, before):
        assert torch.equal(t, b4), 'xps_edit_distance_i64 wrote an input'
    runs = []
    for _ in range(2):
        la = _Launch(B, P, L, K)
        assert la.run(*dev) == 0
        assert la.buf.guards_intact(), 'a guard row was written'
        w = la.words()
        assert (w[~la.live] == np.int32(SENT)).all(), 'a gap between the buffers was written'
        for got, want in zip(la.outputs(), ref):                        # every element of every output is written: the
            assert np.array_equal(got, want)                            # restatement holds no sentinel
        assert np.array_equal(la.outputs()[0], dist_kernel.cpu().numpy())
        # the workspace: one byte per cell; only 1 <= i <= m, 1 <= j <= n of a pair may be written, and what is written
        # is a backpointer
        ws = la.part('ws').view(np.uint8)
        sent = np.frombuffer(np.full(len(ws) // 4, SENT, np.int32).tobytes(), np.uint8)
        cells, sentinel = ws[:B * P * L].reshape(B, P, L), sent[:B * P * L].reshape(B, P, L)
        allowed = np.zeros((B, P, L), bool)
        for b in range(B):
            allowed[b, :m[b], :n[b]] = True
        assert np.array_equal(cells[~allowed], sentinel[~allowed]), 'a workspace cell outside a pair\'s table was written'
        changed = cells != sentinel
        assert (cells[changed] <= 3).all()
        assert changed[allowed].all(), 'a live backpointer was not written'
        assert np.array_equal(ws[B * P * L:], sent[B * P * L:])
        runs.append(w.copy())
    assert np.array_equal(runs[0], runs[1]), 'two launches differ'
    for t, b4 in zip(dev, before):
        assert torch.equal(t, b4), 'an input was written'


@pytest.mark.parametrize('P,L', GUARDED_SHAPES)
@pytest.mark.parametrize('skip', ['counts', 't2p', 'p2t', 'conf', 'all'])
def test_each_optional_output_may_be_null(skip, P, L):
    pred, pl, tgt, tl, ref, (B, K), _, _ = _guarded_case(P, L)
    dev = [_dev(a) for a in (pred, pl, tgt, tl)]
    names = ('counts', 't2p', 'p2t', 'conf') if skip == 'all' else (skip,)
    la = _Launch(B, P, L, K)
    assert la.run(*dev, **{k: None for k in names}) == 0
    assert la.buf.guards_intact() and (la.words()[~la.live] == np.int32(SENT)).all()
    for name, got, want in zip(('dist', 'counts', 't2p', 'p2t', 'conf'), la.outputs(), ref):
        if name == 'conf' and name in names:
            assert (got == 0).all(), 'a skipped confusion matrix was added into'
        elif name in names:
            assert (la.part(name) == np.int32(SENT)).all(), f'the skipped output {name} was written'
        else:
            assert np.array_equal(got, want), name
    if skip == 'all':                                                    # dist alone: no backpointers are kept at all
        assert (la.part('ws') == np.int32(SENT)).all()


@pytest.mark.parametrize('K', [2, 11, 89, 90])
def test_confusion_matrix_margins_and_accumulation(K):
    """Rows are target classes (row K: the insertions), columns predicted classes (column K: the deletions): the row sums
    are the target histogram, the column sums the prediction histogram, the trace the hits, (K, K) is 0; a second launch
    into the same matrix doubles it.  K = 89 | 90 are the two sides of the workgroup's LDS bins ((K + 1)^2 <= 8192 cells)."""
    rng = np.random.default_rng(K)
    B, P, L = 37, 47, 5
    pl, tl = rng.integers(0, P + 1, B), rng.integers(0, L + 1, B)
    pred, pl, tgt, tl = _random_pairs(rng, B, P, L, pl, tl, K)
    ref = edit_align_ref(pred, pl, tgt, tl, n_classes=K)
    dev = [_dev(a) for a in (pred, pl, tgt, tl)]
    la = _Launch(B, P, L, K)
    assert la.run(*dev) == 0
    conf = la.outputs()[4].copy()
    assert np.array_equal(conf, ref[4])
    live_t = np.arange(L)[None, :] < tl[:, None]
    live_p = np.arange(P)[None, :] < pl[:, None]
    assert np.array_equal(conf[:K].sum(1), np.bincount(tgt[live_t], minlength=K))
    assert np.array_equal(conf[:, :K].sum(0), np.bincount(pred[live_p], minlength=K))
    counts = la.outputs()[1]
    assert np.trace(conf) == counts[:, 0].sum() and conf[K, K] == 0
    assert conf[K].sum() == counts[:, 3].sum() and conf[:, K].sum() == counts[:, 2].sum()
    assert conf[:K, :K].sum() - np.trace(conf) == counts[:, 1].sum()
    assert la.run(*dev) == 0
    assert np.array_equal(la.outputs()[4], 2 * conf)
    assert la.buf.guards_intact()


def test_a_batch_cut_into_runs_equals_the_uncut_batch(monkeypatch):
    rt = _rt()
    from cross_patient_speech_decoding_amd.realtime_sim import ctc_errors
    rng = np.random.default_rng(21)
    for P, L in [(47, 5), (70, 66)]:
        B, K = 23, 6
        pl, tl = rng.integers(0, P + 1, B), rng.integers(0, L + 1, B)
        pred, pl, tgt, tl = _random_pairs(rng, B, P, L, pl, tl, K)
        p_d, t_d = _dev(pred), _dev(tgt)
        whole = rt.edit_align(p_d, pl, t_d, tl, n_classes=K)
        seen = []
        real = ctc_errors.call
        monkeypatch.setattr(ctc_errors, 'call', lambda fn, *a: (seen.append((fn, a[6])), real(fn, *a))[1])
        cut = rt.edit_align(p_d, pl, t_d, tl, n_classes=K, max_workspace_bytes=5 * P * L)
        monkeypatch.setattr(ctc_errors, 'call', real)
        assert seen == [('xps_edit_align', 5)] * 4 + [('xps_edit_align', 3)]
        for name in ('distance', 'counts', 'target_to_pred', 'pred_to_target', 'confusion'):
            assert torch.equal(getattr(cut, name), getattr(whole, name)), name
        _equal(cut, edit_align_ref(pred, pl, tgt, tl, n_classes=K))


REFUSALS = [
    (dict(B=-1), 'bad argument'),
    (dict(P=65537, pstride=70000), 'sequence lengths outside the supported range'),
    (dict(L=1025, tstride=2000), 'sequence lengths outside the supported range'),
    (dict(P=-1), 'sequence lengths outside the supported range'),
    (dict(L=-1), 'sequence lengths outside the supported range'),
    (dict(pstride=11), 'row stride shorter than the padded length'),
    (dict(tstride=6), 'row stride shorter than the padded length'),
    (dict(K=0), 'a confusion matrix needs at least one class'),
    (dict(K=-3), 'a confusion matrix needs at least one class'),
    (dict(pred=None), 'null argument'),
    (dict(tgt=None), 'null argument'),
    (dict(pl=None), 'null argument'),
    (dict(tl=None), 'null argument'),
    (dict(dist=None), 'null argument'),
    (dict(ws=None), 'workspace too small'),
    (dict(ws_short=1), 'workspace too small'),
]


@pytest.mark.parametrize('i', range(len(REFUSALS)))
def test_abi_refusals(i):
    kw, text = dict(REFUSALS[i][0]), REFUSALS[i][1]
    pred, pl, tgt, tl, _, (B, K), _, _ = _guarded_case(12, 7)
    dev = [_dev(a) for a in (pred, pl, tgt, tl)]
    la = _Launch(B, 12, 7, K)
    if 'ws_short' in kw:
        kw = dict(ws_bytes=la.ws_bytes - kw['ws_short'])
    assert la.run(*dev, **kw) == -1                                      # XPS_E_INVALID
    msg = _lib().xps_last_error().decode()
    assert msg == f'xps_edit_align: {text}', msg
    w = la.words()
    assert la.buf.guards_intact() and (w[~la.live] == np.int32(SENT)).all()
    assert all((la.part(nm) == np.int32(SENT)).all() for nm in ('dist', 'counts', 't2p', 'p2t', 'ws')), 'a refused call wrote'
    assert (la.part('conf') == 0).all(), 'a refused call added into the confusion matrix'


def test_no_classes_are_needed_without_a_confusion_matrix_and_empty_batches():
    pred, pl, tgt, tl, ref, (B, K), _, _ = _guarded_case(12, 7)
    dev = [_dev(a) for a in (pred, pl, tgt, tl)]
    la = _Launch(B, 12, 7, K)
    assert la.run(*dev, K=0, conf=None) == 0
    assert np.array_equal(la.outputs()[1], ref[1]) and (la.outputs()[4] == 0).all()
    lib = _lib()
    assert lib.xps_edit_align_workspace(3, 5, 2) >= 3 * 5 * 2
    assert lib.xps_edit_align_workspace(0, 5, 2) >= 1 and lib.xps_edit_align_workspace(3, 0, 2) >= 1
    rt = _rt()
    ea = rt.edit_align(torch.zeros(0, 5, dtype=torch.int64, device='cuda'), [], torch.zeros(0, 2, dtype=torch.int64, device='cuda'),
                       [], n_classes=3)
    assert ea.distance.shape == (0,) and ea.target_to_pred.shape == (0, 2) and ea.confusion.tolist() == [[0] * 4] * 4
    ea = rt.edit_align(torch.zeros(2, 0, dtype=torch.int64, device='cuda'), [0, 0], torch.ones(2, 3, dtype=torch.int64, device='cuda'),
                       [3, 1], n_classes=2)                              # no prediction at all: every target token is deleted
    assert ea.distance.tolist() == [3, 1] and ea.counts.tolist() == [[0, 0, 3, 0], [0, 0, 1, 0]]
    assert ea.target_to_pred.tolist() == [[-1, -1, -1], [-1, -2, -2]] and ea.pred_to_target.shape == (2, 0)
    assert ea.confusion.tolist() == [[0, 0, 0], [0, 0, 4], [0, 0, 0]] and ea.target_ops().tolist() == [[2, 2, 2], [2, -1, -1]]
    with pytest.raises(RuntimeError, match='edit_align needs device tensors'):
        rt.edit_align(torch.zeros(1, 2, dtype=torch.int64), [2], torch.zeros(1, 2, dtype=torch.int64), [2])


# ---- the model and the session replay ------------------------------------------------------------------------------------------
def test_model_decode_errors_equals_per_device_of_its_own_greedy_decode():
    rt = _rt()
    torch.manual_seed(0)
    win, stride, Cin, ncls = 6, 4, 2, 5
    m = rt.RealtimeRNNModel(win * Cin, 8, 1, ncls, dropout=0.0, win_size=win, stride=stride).cuda()
    with torch.no_grad():
        m.classifier.fc.bias.zero_()                                     # the initial bias (+2 blank, -2 the others) decodes
        m.classifier.fc.weight.mul_(4.0)                                 # nothing: an untrained model that emits tokens
    m.train()
    x = torch.randn(5, 46, Cin, device='cuda') * 3
    tg = torch.tensor([[1, 2, 0], [3, 3, 4], [2, 0, 0], [4, 1, 2], [1, 1, 1]])
    tl = [2, 3, 1, 3, 0]
    ea = m.decode_errors(x, tg, target_lengths=tl)
    assert m.training                                                    # the mode is put back
    m.eval()
    with torch.no_grad():
        lp = torch.log_softmax(m.forward(x), dim=2)
    tokens, lengths = rt.greedy_decode_device(lp, blank=m.blank)
    assert int(lengths.max()) >= 1
    assert torch.equal(ea.per(), rt.per_device(tokens, lengths, tg.cuda(), tl))
    assert ea.confusion.shape == (ncls + 1, ncls + 1)
    want = rt.edit_align(tokens, lengths, tg.cuda(), tl, n_classes=ncls)
    for name in ('distance', 'counts', 'target_to_pred', 'pred_to_target', 'confusion'):
        assert torch.equal(getattr(ea, name), getattr(want, name)), name
    _equal(ea, edit_align_ref(tokens.cpu().numpy(), lengths.cpu().numpy(), tg.numpy(), tl, n_classes=ncls))
    # target_lengths None: all of targets' columns; input_lengths: the windows past a trial's length decode as blank
    full = m.decode_errors(x, tg)
    assert full.target_lengths.tolist() == [3] * 5
    short = m.decode_errors(x, tg, target_lengths=tl, input_lengths=[46, 46, 22, 46, 5])
    n_win = [m.n_windows(46), m.n_windows(46), (22 - win) // stride + 1, m.n_windows(46), 0]
    for b, w in enumerate(n_win):
        tb, lb = rt.greedy_decode_device(lp[b:b + 1, :w], blank=m.blank)
        assert short.pred[b, :int(lb)].tolist() == tb[0, :int(lb)].tolist() and int(short.pred_lengths[b]) == int(lb)


def test_session_result_errors_equals_edit_align():
    rt = _rt()
    tokens = torch.tensor([[1, 2, 3, -1, -1], [4, -1, -1, -1, -1], [-1, -1, -1, -1, -1], [2, 2, 1, 0, 3]], device='cuda')
    lengths = torch.tensor([3, 1, 0, 5], device='cuda')
    res = rt.SessionResult(None, tokens, lengths, None, None)
    tg = torch.tensor([[1, 3, 0], [4, 4, 0], [2, 0, 0], [2, 1, 3]])
    tl = [2, 2, 1, 3]
    got = res.errors(tg, target_lengths=tl, n_classes=5)
    want = rt.edit_align(tokens, lengths, tg.cuda(), tl, n_classes=5)
    for name in ('distance', 'counts', 'target_to_pred', 'pred_to_target', 'confusion'):
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    _equal(got, edit_align_ref(tokens.cpu().numpy(), lengths.cpu().numpy(), tg.numpy(), tl, n_classes=5))
    assert got.distance.tolist() == [1, 1, 1, 2]
    assert res.errors(tg, target_lengths=tl).confusion is None
    assert res.errors(tg).target_lengths.tolist() == [3] * 4
