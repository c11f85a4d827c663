"""CTC forced alignment on the device: the Viterbi best path of a KNOWN target sequence through the network's frame scores
(csrc/xps_ctc_align.hip), i.e. when each phoneme was emitted.  One launch for the batch, float64
additions and comparisons only, so the result is bit for bit the recursion of include/xps.h.  There is no CPU fallback;
the shape and range checks run before any device call."""
import torch

from .._dev import ptr, stream, workspace
from .._lib import call, lib
from ._ctc_host import TARGET_MAX, check_lattice_inputs, frame_times, lattice_on_device  # noqa: F401


class CTCAlignment:
    """What forced_align returns (device tensors): states (B, T) int32, the extended-state index of each frame (even: the
    blank before / after token s // 2, odd: token s // 2), -1 from the sequence's end on and everywhere in an infeasible
    sequence; token_start / token_end (B, Lmax) int32, the first frame and one past the last frame of each target token,
    -1 past the target's length; score (B,) float64, the sum of the path's scores (its log-probability for
    log-probabilities); feasible (B,) bool, score > -inf.  targets (B, Lmax) int64 and target_lengths (B,) int64 are the
    device copies the launch read; blank the blank label."""

    def __init__(self, states, token_start, token_end, score, targets, target_lengths, blank):
        self.states, self.token_start, self.token_end, self.score = states, token_start, token_end, score
        self.targets, self.target_lengths, self.blank = targets, target_lengths, int(blank)
        self.feasible = score > -float('inf')

    def frame_labels(self):
        """(B, T) int64 device tensor: the label emitted at each frame, blank included, -1 past the end."""
        s = self.states.long()
        if self.targets.shape[1] == 0:
            lab = torch.full_like(s, self.blank)
        else:
            tok = torch.gather(self.targets, 1, (s.clamp(min=0) // 2).clamp(max=self.targets.shape[1] - 1))
            lab = torch.where(s % 2 == 1, tok, torch.full_like(s, self.blank))
        return torch.where(s < 0, torch.full_like(s, -1), lab)

    def spans(self, b):
        """[(label, start, end), ...] of sequence b's tokens (host integers; empty when infeasible): frames start .. end - 1."""
        n = int(self.target_lengths[b])
        if not bool(self.feasible[b]):
            return []
        rows = torch.stack([self.targets[b, :n], self.token_start[b, :n].long(), self.token_end[b, :n].long()], 1).tolist()
        return [tuple(r) for r in rows]

    def times(self, frame_time):
        """Spans mapped through a per-frame time vector: frame_time (T,), the time of each frame (window_end_times for the
        realtime model's windows) -> (onset, offset) (B, Lmax) tensors of frame_time's dtype on the device, onset the time of
        a token's first frame and offset the time of its LAST frame (end - 1); NaN where there is no span."""
        ft = frame_times(frame_time, self.states.shape[1], self.states.device)
        none = self.token_start < 0
        if ft.numel() == 0:
            nan = torch.full(self.token_start.shape, float('nan'), dtype=ft.dtype, device=ft.device)
            return nan, nan.clone()
        onset = ft[self.token_start.long().clamp(min=0)]
        offset = ft[(self.token_end.long() - 1).clamp(min=0)]
        nan = torch.full_like(onset, float('nan'))
        return torch.where(none, nan, onset), torch.where(none, nan, offset)


def window_end_times(n_windows, win_size, stride, step_s):
    """(n_windows,) float64: the time at which the LAST input row of window w has arrived, rows arriving every step_s seconds
    (row r is complete at (r + 1) * step_s).  The rows of window w are RealtimeRNNModel.reformat_time_windows' own index
    expression, arange(n_windows) * stride + arange(win_size)."""
    if n_windows < 0 or win_size < 1 or stride < 1:
        raise ValueError(f'n_windows {n_windows}, win_size {win_size}, stride {stride}: need >= 0, >= 1, >= 1')
    idx = (torch.arange(n_windows) * stride)[:, None] + torch.arange(win_size)
    return (idx[:, -1] + 1).double() * float(step_s)


def forced_align(scores, targets, input_lengths=None, target_lengths=None, blank=0, time_major=False):
    """Best CTC path of each sequence's target through its scores -> CTCAlignment.  scores (B, T, C), or (T, B, C) with
    time_major: float32 / float64 scores of any kind (no softmax is applied: a per-frame constant shifts every path
    alike, so logits and their log-softmax have the same best path up to rounding; pass log-probabilities for a
    log-probability score), host or device; a device tensor with contiguous classes is read in place whatever its strides over the first two axes.
    targets (B, Lmax) integers padded, with target_lengths (B,) (None: all Lmax), or a list of B 1-D sequences;
    input_lengths (B,) (None: all T).  Lengths and labels are checked here, on the host (a device tensor of targets or
    lengths is copied to the host for it, which waits for it); every check raises ValueError before any device call."""
    scores, targets, il, tl, T, B, Cn = check_lattice_inputs(scores, targets, input_lengths, target_lengths, blank, time_major)
    d = lattice_on_device(scores, targets, il, tl, time_major, 'forced_align')
    dev, Lmax = d.device, targets.size(1)
    states = torch.empty(B, T, dtype=torch.int32, device=dev)
    t0 = torch.empty(B, Lmax, dtype=torch.int32, device=dev)
    t1 = torch.empty(B, Lmax, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float64, device=dev)
    ws_bytes = int(lib().xps_ctc_align_workspace(B, T, Lmax))
    ws = workspace(ws_bytes, dev)
    call('xps_ctc_align', d.scores.data_ptr(), d.is_f32, d.stride_t, d.stride_b, T, B, Cn, Lmax, d.targets.data_ptr(), Lmax,
         ptr(d.input_lengths), d.target_lengths.data_ptr(), int(blank), states.data_ptr(), t0.data_ptr(), t1.data_ptr(),
         score.data_ptr(), ws.data_ptr(), ws_bytes, stream(dev))
    return CTCAlignment(states, t0, t1, score, d.targets, d.target_lengths, blank)
