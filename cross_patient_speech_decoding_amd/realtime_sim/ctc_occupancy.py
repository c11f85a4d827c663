"""CTC posterior occupancies on the device: the forward-backward posteriors of a KNOWN target sequence through the network's
frame scores (csrc/xps_ctc_occupancy.hip), i.e. how sure the model is that a phoneme was emitted at, or
started at, a frame -- where forced_align reports the one best path.  Float64 in the log domain, in the operation order of
include/xps.h.  There is no CPU fallback; the shape and range checks (forced_align's own) run before any device call."""
import torch

from .._dev import ptr, stream, workspace
from .._lib import call, lib
from ._ctc_host import at, check_lattice_inputs, frame_times, lattice_on_device, runs_within

WANT = ('token_occ', 'onset', 'class_occ')
MAX_WORKSPACE_BYTES = 1 << 30


class CTCOccupancy:
    """What posterior_align returns (device tensors, float64 unless said otherwise): log_z (B,), the log of the summed path
    scores (-nll for log-probabilities); feasible (B,) bool, log_z > -inf; token_occ (B, T, Lmax), the posterior that frame t
    emits token j; onset (B, T, Lmax), the posterior that token j starts at frame t (sums to 1 over t); class_occ (B, T, C),
    the posterior that frame t emits class c (rows sum to 1) -- each of the three None when not asked for;
    expected_frames (B, Lmax), the expected number of frames of token j; onset_mean (B, Lmax), the expected onset frame, NaN
    where there is no token.  Frames past a sequence's length and tokens past its target's length are 0; an infeasible
    sequence has every posterior 0 and onset_mean NaN.  targets (B, Lmax) int64 and target_lengths (B,) int64 are the device
    copies the launch read; blank the blank label."""

    def __init__(self, log_z, token_occ, onset, class_occ, expected_frames, onset_mean, targets, target_lengths, blank):
        self.log_z, self.token_occ, self.onset, self.class_occ = log_z, token_occ, onset, class_occ
        self.expected_frames, self.onset_mean = expected_frames, onset_mean
        self.targets, self.target_lengths, self.blank = targets, target_lengths, int(blank)
        self.feasible = log_z > -float('inf')

    def _need(self, name):
        v = getattr(self, name)
        if v is None:
            raise ValueError(f"{name} was not computed: ask for it with want=(..., '{name}')")
        return v

    def onset_times(self, frame_time):
        """Onset posteriors against a per-frame time vector: frame_time (T,), the time of each frame (window_end_times for
        the realtime model's windows) -> (mean, sd) (B, Lmax) tensors of frame_time's dtype on the device: the mean and the
        standard deviation of each token's onset time under `onset`; NaN where there is no token."""
        onset = self._need('onset')
        ft = frame_times(frame_time, onset.shape[1], onset.device)
        w = onset.to(ft.dtype)
        mean = (w * ft[None, :, None]).sum(1)
        var = (w * (ft[None, :, None] - mean[:, None, :]) ** 2).sum(1)
        none = torch.isnan(self.onset_mean)
        nan = torch.full_like(mean, float('nan'))
        return torch.where(none, nan, mean), torch.where(none, nan, var.clamp(min=0).sqrt())

    def peak(self):
        """(B, Lmax): the largest posterior any frame gives token j, a per-token confidence (0 where there is no token)."""
        occ = self._need('token_occ')
        if occ.shape[1] == 0:
            return occ.new_zeros(occ.shape[0], occ.shape[2])
        return occ.max(dim=1).values

    def posteriorgram(self):
        """(B, T, C): class_occ, the posterior over classes frame by frame given the target."""
        return self._need('class_occ')


def workspace_runs(B, T, Lmax, max_workspace_bytes):
    """Cut B sequences into runs [(start, stop), ...] whose alpha workspace, T * (2 Lmax + 1) * 8 bytes per sequence, stays
    within max_workspace_bytes; as few runs as that allows, of even size.  A single sequence above the limit raises
    ValueError."""
    return runs_within(B, max(int(T), 0) * (2 * int(Lmax) + 1) * 8, max_workspace_bytes,
                       f'one sequence of {T} frames and {Lmax} labels')


def posterior_align(scores, targets, input_lengths=None, target_lengths=None, blank=0, time_major=False,
                    want=WANT, max_workspace_bytes=MAX_WORKSPACE_BYTES):
    """Forward-backward posteriors of each sequence's target through its scores -> CTCOccupancy.  scores, targets and the
    lengths are forced_align's arguments with forced_align's checks (every one raises ValueError before any device call);
    no softmax is applied: logits and their log-softmax have the same posteriors, log_z is -nll only for log-probabilities.
    want: which of 'token_occ', 'onset', 'class_occ' to compute (the others are None; log_z, expected_frames and onset_mean
    always are).
    max_workspace_bytes: the kernel keeps alpha for every (sequence, frame, state), T * (2 Lmax + 1) * 8 bytes per sequence
    (1 GB at B = 2048, T = 512, L = 64), so the batch is cut into runs of sequences that stay within this limit, one launch
    per run on the same workspace; the results do not depend on the cut.  The default, 1 GiB, is well under one percent of
    the MI355X's memory and still leaves a run of a thousand sequences at T = 512, L = 64 (several workgroups for each of
    the 256 CUs, which is what hides the recursion's latency); the training shape (47 windows, 5 labels) needs 8.5 MB for
    2048 sequences.  A single sequence above the limit raises ValueError."""
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in WANT]
    if unknown:
        raise ValueError(f'want holds {unknown[0]!r}: expected a subset of {WANT}')
    scores, targets, il, tl, T, B, Cn = check_lattice_inputs(scores, targets, input_lengths, target_lengths, blank, time_major)
    Lmax = targets.size(1)
    runs = workspace_runs(B, T, Lmax, max_workspace_bytes)
    d = lattice_on_device(scores, targets, il, tl, time_major, 'posterior_align')
    dev = d.device

    def out(*shape):
        return torch.empty(*shape, dtype=torch.float64, device=dev)
    log_z, ef, om = out(B), out(B, Lmax), out(B, Lmax)
    tok = out(B, T, Lmax) if 'token_occ' in want else None
    ons = out(B, T, Lmax) if 'onset' in want else None
    cls = out(B, T, Cn) if 'class_occ' in want else None
    ws_bytes = max([int(lib().xps_ctc_occupancy_workspace(b1 - b0, T, Lmax)) for b0, b1 in runs], default=0)
    ws = workspace(ws_bytes, dev)
    for b0, b1 in runs:
        call('xps_ctc_occupancy', at(d.scores, b0, d.stride_b), d.is_f32, d.stride_t, d.stride_b, T, b1 - b0, Cn, Lmax,
             at(d.targets, b0, Lmax), Lmax, at(d.input_lengths, b0, 1), at(d.target_lengths, b0, 1), int(blank),
             at(log_z, b0, 1), at(tok, b0, T * Lmax), at(ons, b0, T * Lmax), at(cls, b0, T * Cn), at(ef, b0, Lmax),
             at(om, b0, Lmax), ptr(ws), ws_bytes, stream(dev))
    return CTCOccupancy(log_z, tok, ons, cls, ef, om, d.targets, d.target_lengths, blank)
