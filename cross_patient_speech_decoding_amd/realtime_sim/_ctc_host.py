"""The host front end shared by forced_align (ctc_align.py), posterior_align (ctc_occupancy.py), edit_align (ctc_errors.py)
and edit_distance_device: the checks that raise ValueError before any device call, the move of a checked batch to the
device, the run cutter of the workspace limits and the pointer arithmetic of a run.  Private: the public names live in
the modules that use these."""
from collections import namedtuple

import numpy as np
import torch

from .._dev import current_device

TARGET_MAX = 511                              # 2 * L + 1 <= 1023 states, the CTC kernels' cap (CTC_MAXS, csrc/xps_ctc_lattice.h)
EDIT_MAX_PRED, EDIT_MAX_TARGET = 65536, 1024  # xps_edit_distance_supported (include/xps.h)


def lengths(v, B, top, what):
    if v is None:
        return None
    v = torch.as_tensor(v)
    host = v.detach().cpu().to(torch.int64).reshape(-1)
    if host.numel() != B:
        raise ValueError(f'{host.numel()} {what} for {B} sequences')
    if B and (int(host.min()) < 0 or int(host.max()) > top):
        raise ValueError(f'{what} outside 0..{top}')
    return host


def integer_tokens(v, what, axes_text):
    v = torch.as_tensor(v)
    if v.dim() != 2:
        raise ValueError(f'{what} of shape {tuple(v.shape)}: expected {axes_text}')
    if v.is_floating_point() or v.dtype == torch.bool:
        raise ValueError(f'{what} of dtype {v.dtype}: expected integers')
    return v


def labels_in_range(host, lens, K, what):
    """host (B, width) int64 host tensor, lens (B,) host tensor or an integer: every label within its length lies in 0..K-1."""
    width = host.size(1)
    if host.size(0) and width:
        live = torch.arange(width)[None, :] < (lens[:, None] if torch.is_tensor(lens) else lens)
        bad = live & ((host < 0) | (host >= K))
        if bool(bad.any()):
            b, j = (int(v) for v in bad.nonzero()[0])
            raise ValueError(f'{what} {b} holds the label {int(host[b, j])} at position {j}: outside 0..{K - 1}')


def runs_within(B, bytes_per_item, max_workspace_bytes, describe):
    """Cut B items into runs [(start, stop), ...] whose workspace, bytes_per_item each, stays within max_workspace_bytes; as
    few runs as that allows, of even size.  A single item above the limit raises ValueError, naming it by `describe`."""
    per, limit = int(bytes_per_item), int(max_workspace_bytes)
    if B <= 0:
        return []
    if per > limit:
        raise ValueError(f'{describe} needs {per} bytes of workspace: above max_workspace_bytes = {limit}')
    most = B if per == 0 else min(B, limit // per)
    n = -(-B // -(-B // most))                      # the fewest runs, then evened out: no short last launch
    return [(s, min(s + n, B)) for s in range(0, B, n)]


def check_lattice_inputs(scores, targets, input_lengths, target_lengths, blank, time_major):
    """Every shape and range check of forced_align, on the host.  Returns (scores, targets (B, Lmax) int64 host or device
    tensor, input_lengths, target_lengths (host int64 or None), T, B, C)."""
    scores = torch.as_tensor(scores)
    if scores.dim() != 3:
        raise ValueError(f'scores of shape {tuple(scores.shape)}: expected three axes')
    (T, B) = (scores.size(0), scores.size(1)) if time_major else (scores.size(1), scores.size(0))
    Cn = scores.size(2)
    if Cn < 1:
        raise ValueError('forced alignment needs at least one class')
    if not 0 <= int(blank) < Cn:
        raise ValueError(f'blank {blank} outside 0..{Cn - 1}')
    if isinstance(targets, (list, tuple)) and not (len(targets) and all(np.ndim(t) == 0 for t in targets)):
        rows = [torch.as_tensor(t).detach().cpu().to(torch.int64) for t in targets]
        if any(r.dim() != 1 for r in rows):
            raise ValueError('a list of targets holds 1-D sequences')
        if target_lengths is not None:
            raise ValueError('a list of targets carries its own lengths: target_lengths must be None')
        if len(rows) != B:
            raise ValueError(f'{len(rows)} targets for {B} sequences')
        Lmax = max([r.numel() for r in rows], default=0)
        target_lengths = torch.tensor([r.numel() for r in rows], dtype=torch.int64)
        targets = torch.zeros(B, Lmax, dtype=torch.int64)
        for b, r in enumerate(rows):
            targets[b, :r.numel()] = r
    else:
        targets = integer_tokens(targets, 'targets', '(B, Lmax) or a list of 1-D sequences')
        if targets.size(0) != B:
            raise ValueError(f'{targets.size(0)} targets for {B} sequences')
    Lmax = targets.size(1)
    if Lmax > TARGET_MAX:
        raise ValueError(f'targets of {Lmax} labels: the alignment kernel holds at most {TARGET_MAX}')
    il = lengths(input_lengths, B, T, 'input_lengths')
    tl = lengths(target_lengths, B, Lmax, 'target_lengths')
    labels_in_range(targets.detach().cpu().to(torch.int64), Lmax if tl is None else tl, Cn, 'target')
    return scores, targets, il, tl, T, B, Cn


DeviceLattice = namedtuple('DeviceLattice', 'device scores is_f32 stride_t stride_b targets input_lengths target_lengths')


def lattice_on_device(scores, targets, il, tl, time_major, who):
    """A checked batch (check_lattice_inputs) as the kernels read it: float32 / float64 scores with contiguous classes on
    the device (in place where they already are) with their strides over frames and sequences, targets (B, Lmax) int64
    contiguous, input_lengths (B,) int64 or None, target_lengths (B,) int64 (all Lmax when tl is None)."""
    dev = scores.device if scores.is_cuda else current_device(who)
    if scores.dtype not in (torch.float32, torch.float64):
        scores = scores.float() if scores.is_floating_point() else scores.double()
    scores = scores.to(dev)
    if scores.size(2) > 1 and scores.stride(2) != 1:
        scores = scores.contiguous()
    st, sb = (scores.stride(0), scores.stride(1)) if time_major else (scores.stride(1), scores.stride(0))
    B, Lmax = targets.size(0), targets.size(1)
    tg = targets.to(dev, torch.int64).contiguous()
    il_d = None if il is None else il.to(dev)
    tl_d = torch.full((B,), Lmax, dtype=torch.int64, device=dev) if tl is None else tl.to(dev)
    return DeviceLattice(dev, scores, int(scores.dtype == torch.float32), int(st), int(sb), tg, il_d, tl_d)


def at(tensor, b0, row):
    """Address of row-group b0 of a contiguous tensor whose items per sequence number `row`; None in, None out."""
    return None if tensor is None else tensor.data_ptr() + tensor.element_size() * b0 * row


def frame_times(frame_time, T, device):
    """frame_time as a flat floating-point tensor of T entries on the device (integers become float64)."""
    ft = torch.as_tensor(frame_time)
    if not ft.is_floating_point():
        ft = ft.double()
    ft = ft.to(device).reshape(-1)
    if ft.numel() != T:
        raise ValueError(f'{ft.numel()} frame times for {T} frames')
    return ft
