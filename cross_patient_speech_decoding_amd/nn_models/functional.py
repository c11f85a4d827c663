"""torch.autograd bindings of the HIP kernels (libxps.so) for the seq2seq GRU path.

Every function here enqueues HIP kernels through the C ABI on the current torch stream;
torch supplies device memory, streams and autograd bookkeeping only.  There is no CPU
fallback: a non-CUDA tensor raises.

Internal activation layout is TIME-MAJOR: (T, B, features).
"""
import ctypes as C
from typing import NamedTuple

import torch

from .._dev import need_gpu as _need_gpu, ptr as _ptr, ptr_array as _ptr_array, stream as _stream, workspace as _ws  # noqa: F401
from .. import _switches
from .._lib import TnProblem, call, lib, rowmap

_f32 = torch.float32

GEMM_PRECISIONS = {'fp32': 0, 'bf16x3': 1}


def set_gemm_precision(name):
    """Product precision of the matrix kernels (GEMMs and the fused GRU recurrence): 'bf16x3' (default: operands split
    hi + lo in bf16, three bf16 MFMAs per product, fp32 accumulate: ~2^-16 relative product error, logits within 2e-6
    of the reference goldens) or 'fp32' (fp32 MFMA, exact fp32 fma chains).  Process-wide; also XPS_GEMM_PRECISION."""
    if name not in GEMM_PRECISIONS:
        raise ValueError(f"gemm precision must be one of {sorted(GEMM_PRECISIONS)}")
    call('xps_set_gemm_precision', GEMM_PRECISIONS[name])


def get_gemm_precision():
    mode = lib().xps_get_gemm_precision()
    return {v: k for k, v in GEMM_PRECISIONS.items()}[mode]


_memo_values = {}


def _memo(key, compute):
    """compute() once per key, for answers that depend on nothing but the key and the switches: every _switches.set forgets
    everything (as does _memo.clear()), and each use names in its key the library state that has a setter of its own
    (precision, cluster mode, BPTT grid).  Bounded: beyond 4096 keys nothing more is kept."""
    v = _memo_values.get(key)
    if v is None:
        v = compute()
        if len(_memo_values) < 4096:
            _memo_values[key] = v
    return v


_memo.clear = _memo_values.clear
_switches.on_change(_memo_values.clear)


# --------------------------------------------------------------------------- #
# raw GEMM wrappers                                                            #
# --------------------------------------------------------------------------- #
def gemm_nt(A, B, out, M, N, K, bias=None, ra=None, rb=None, rc=None, accumulate=False):
    """out[m][n] (+)= sum_k A[m][k] B[n][k] + bias[n]."""
    ra = ra or rowmap(K)
    rb = rb or rowmap(K)
    rc = rc or rowmap(N)
    call('xps_gemm_nt_f32', _ptr(A), C.byref(ra), _ptr(B), C.byref(rb), _ptr(out), C.byref(rc),
         _ptr(bias), M, N, K, int(accumulate), _stream())
    return out


def gemm_nn(A, B, out, M, N, K, ra=None, rb=None, rc=None, accumulate=False):
    """out[m][n] (+)= sum_k A[m][k] B[k][n]."""
    ra = ra or rowmap(K)
    rb = rb or rowmap(N)
    rc = rc or rowmap(N)
    call('xps_gemm_nn_f32', _ptr(A), C.byref(ra), _ptr(B), C.byref(rb), _ptr(out), C.byref(rc),
         M, N, K, int(accumulate), _stream())
    return out


def gemm_tn(A, B, out, M, N, K, ra=None, rb=None, rc=None, accumulate=False):
    """out[m][n] (+)= sum_k A[k][m] B[k][n]   (deterministic split-K)."""
    ra = ra or rowmap(M)
    rb = rb or rowmap(N)
    rc = rc or rowmap(N)
    nbytes = lib().xps_gemm_tn_f32_workspace(M, N, K)
    ws = _ws(nbytes, out.device)
    call('xps_gemm_tn_f32', _ptr(A), C.byref(ra), _ptr(B), C.byref(rb), _ptr(out), C.byref(rc),
         M, N, K, int(accumulate), _ptr(ws), nbytes, _stream())
    return out


def tn_problem(A, B, out, M, N, K, ra=None, rb=None, rc=None, colsum_out=None, accumulate=False,
               accumulate_colsum=False):
    """One weight-gradient problem  out (+)= A^T B  (A: K x M, B: K x N) [+ colsum_out (+)= column sums of A].
    ``accumulate`` makes both destinations accumulate; ``accumulate_colsum`` the column sums alone."""
    return TnProblem(_ptr(A), _ptr(B), _ptr(out), _ptr(colsum_out), ra or rowmap(M), rb or rowmap(N),
                     rc or rowmap(N), M, N, K, int(bool(accumulate)) | (2 if accumulate_colsum else 0))


def gemm_tn_grouped(problems, device, stream=None):
    """All problems in ONE split-K launch + ONE reduce launch (deterministic).  stream: raw HIP stream handle to launch
    on (default: torch's current stream); returns the workspace tensors (the caller of a foreign-stream launch keeps them
    alive until that stream has been joined)."""
    st = _stream() if stream is None else stream
    keep = []
    for i in range(0, len(problems), 12):
        chunk = problems[i:i + 12]
        arr = (TnProblem * len(chunk))(*chunk)
        key = ('tn_ws', *[(q.M, q.N, q.K, bool(q.colsum_a)) for q in chunk])   # the slab layout depends on the shapes only
        nbytes = _memo(key, lambda: lib().xps_gemm_tn_grouped_f32_workspace(arr, len(chunk)))
        ws = _ws(nbytes, device)
        call('xps_gemm_tn_grouped_f32', arr, len(chunk), _ptr(ws), nbytes, st)
        keep.append(ws)
    return keep


# Weight-gradient GEMMs are off the critical path of the backward pass (nothing downstream reads them until
# the optimiser step), while the recurrence kernels that ARE on it leave ~40 % of the MFMA pipe idle and the
# element-wise kernels all of it.  They are therefore launched on a second HIP stream and co-scheduled with
# whatever the main stream runs next; the main stream re-joins when the autograd engine finishes the pass.
# Only done when the results land straight in .grad buffers (DIRECT_GRAD): nothing on the main stream may
# consume them before the join.  Deterministic: stream order does not change any reduction order.
# XPS_OVERLAP_WGRAD=0: everything on the main stream.
_side_streams = {}
_side_pending = set()


def _low_priority_stream(idx):
    """Side stream BELOW the default priority (torch only offers default / high): when a CU frees up, kernels of
    the critical path are dispatched first; measured without it, tiny main-stream kernels queued up to 100 us
    behind the side stream's GEMM blocks."""
    if _switches.get('XPS_SIDE_PRIORITY') == 'default':       # (diagnostic: tools/graph_probe.py -- what a hipGraph replay does to the side work)
        return torch.cuda.Stream(device=idx)
    handle = C.c_void_p()
    with torch.cuda.device(idx):
        call('xps_stream_create_low_priority', C.byref(handle))
    return torch.cuda.ExternalStream(handle.value, device=idx)


_side_keep = []        # operands / workspaces of launches on the side stream: referenced until the main stream has joined


def _join_side_streams():
    for dev_index in list(_side_pending):
        torch.cuda.current_stream(dev_index).wait_stream(_side_streams[dev_index])
    _side_pending.clear()
    # everything the side stream read may be released now: later allocations are ordered behind the join on the main stream
    _side_keep.clear()


def _launch_weight_grads(fn, device, tensors, direct):
    """fn(stream) enqueues weight-gradient kernels reading `tensors` on the raw HIP stream it is given (None: the current
    stream) and returns the temporaries it allocated.  Runs it on the side stream when allowed.  The kernels take the
    stream as a C-ABI argument, so torch's current stream is never switched (the context manager and one
    record_stream per operand cost ~30 us of host time per call site; the operands are kept alive until the join)."""
    if not (_switches.get('XPS_OVERLAP_WGRAD') and direct):
        fn(None)
        return
    idx = device.index if device.index is not None else torch.cuda.current_device()
    side = _side_streams.get(idx)
    if side is None:
        side = _side_streams[idx] = _low_priority_stream(idx)
    side.wait_stream(torch.cuda.current_stream(idx))
    keep = fn(side.cuda_stream)
    _side_keep.append((tensors, keep))
    if idx not in _side_pending:
        if not _side_pending:
            torch.autograd.Variable._execution_engine.queue_callback(_join_side_streams)
        _side_pending.add(idx)


# When a parameter already owns a contiguous .grad buffer (FlatAdamW points every .grad into ONE flat
# buffer), weight gradients are accumulated straight into it by the GEMM epilogue and autograd gets
# None: no temporary, no extra add kernel per parameter.
DIRECT_GRAD = True


def _grad_target(param, shape, device):
    g = getattr(param, 'grad', None) if DIRECT_GRAD else None
    if g is not None and g.is_contiguous() and tuple(g.shape) == tuple(shape) and g.dtype == _f32 and g.is_cuda:
        return g, True, None
    t = torch.empty(shape, dtype=_f32, device=device)
    return t, False, t


def _grad_targets(w, w_shape, b, b_shape, device):
    """_grad_target of a weight and of its bias, which one grouped-TN problem writes under ONE accumulate flag: both straight
    into .grad, else both into temporaries.  Returns dw, db, accumulate, rw, rb (rw / rb: what autograd gets)."""
    dw, acc_w, rw = _grad_target(w, w_shape, device)
    db, acc_b, rb = _grad_target(b, b_shape, device)
    if acc_w != acc_b:
        dw = rw = torch.empty(w_shape, dtype=_f32, device=device)
        db = rb = torch.empty(b_shape, dtype=_f32, device=device)
        acc_w = False
    return dw, db, acc_w, rw, rb


def colsum(X, rows, cols, out=None, out_sq=None, ldx=None, accumulate=False):
    out = out if out is not None else torch.empty(cols, dtype=_f32, device=X.device)
    nbytes = lib().xps_colsum_f32_workspace(rows, cols)
    ws = _ws(nbytes, X.device)
    call('xps_colsum_f32', _ptr(X), ldx or cols, rows, cols, _ptr(out), _ptr(out_sq), int(accumulate),
         _ptr(ws), nbytes, _stream())
    return out


def transpose(src, rows, cols):
    dst = torch.empty(cols, rows, dtype=_f32, device=src.device)
    call('xps_transpose_f32', _ptr(src), _ptr(dst), rows, cols, _stream())
    return dst


# --------------------------------------------------------------------------- #
# Linear                                                                       #
# --------------------------------------------------------------------------- #
class LinearFn(torch.autograd.Function):
    """y = x W^T + b on the fp32 MFMA (nn.Linear / the input projections of nn.GRU)."""

    @staticmethod
    def forward(ctx, x, w, b):
        _need_gpu(x, w, b)
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        wc = w.contiguous()
        M, K = x2.shape
        N = wc.shape[0]
        y = torch.empty(M, N, dtype=_f32, device=x.device)
        gemm_nt(x2, wc, y, M, N, K, bias=b)
        ctx.save_for_backward(x2, wc)
        ctx.params = (w, b)
        ctx.xshape = x.shape
        ctx.x_param = x if isinstance(x, torch.nn.Parameter) and x.dim() == 2 else None    # e.g. an embedding table
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, wc = ctx.saved_tensors
        w, b = ctx.params
        M, K = x2.shape
        N = wc.shape[0]
        dy2 = dy.reshape(M, N).contiguous()
        dx = rw = rb = None
        if ctx.needs_input_grad[0]:
            gx, acc_x, _ = _grad_target(ctx.x_param, (M, K), dy.device) if ctx.x_param is not None else (None, False, None)
            if acc_x:
                gemm_nn(dy2, wc, gx, M, K, N, accumulate=True)
            else:
                dx = torch.empty(M, K, dtype=_f32, device=dy.device)
                gemm_nn(dy2, wc, dx, M, K, N)
                dx = dx.view(ctx.xshape)
        need_w, need_b = ctx.needs_input_grad[1], b is not None and ctx.needs_input_grad[2]
        if need_w or need_b:
            if need_b:
                dw, db, acc_w, rw, rb = _grad_targets(w, (N, K), b, (N,), dy.device)
            else:
                (dw, acc_w, rw), db = _grad_target(w, (N, K), dy.device), None
            prob = [tn_problem(dy2, x2, dw, N, K, M, colsum_out=db, accumulate=acc_w)]
            _launch_weight_grads(lambda st: gemm_tn_grouped(prob, dy.device, st), dy.device, (dy2, x2),
                                 rw is None and (rb is None or not need_b))
            if not need_w:
                rw = None
        return dx, rw, rb


def linear(x, w, b=None):
    return LinearFn.apply(x, w, b)


# --------------------------------------------------------------------------- #
# GRU                                                                          #
# --------------------------------------------------------------------------- #
def _gru_ws_bytes(fn, T, B, H, ndir):
    """Workspace size of the recurrence entry points (depends on the shape, the cluster mode and the BPTT grid only)."""
    key = (fn, T, B, H, ndir, lib().xps_get_gru_cluster_mode(), lib().xps_get_gru_bptt_grid())
    return _memo(key, lambda: getattr(lib(), fn)(T, B, H, ndir))


# The cluster-persistent recurrence (256 < H <= 512) bounds every in-kernel wait; a wait that gave up stores 1 into ONE small
# persistent word per device (xps_gru_set_status_word).  Nothing is read during a step: check_gru_status() is called where the
# host synchronises anyway (the Trainer: when it reads the epoch's loss, and at the end of fit / validate / test / predict).
_gru_status_word = {}


def _gru_status_register(device):
    idx = device.index if device.index is not None else torch.cuda.current_device()
    w = _gru_status_word.get(idx)
    if w is None:
        w = _gru_status_word[idx] = torch.zeros(1, dtype=torch.int32, device=torch.device('cuda', idx))
        with torch.cuda.device(idx):
            call('xps_gru_set_status_word', w.data_ptr())
    return w


def check_gru_status():
    """Synchronising check of the per-device hand-off status words (set by a cluster-recurrence launch whose in-kernel wait
    timed out since the last call)."""
    bad = [idx for idx, w in _gru_status_word.items() if int(w.item()) != 0]
    for idx in bad:
        _gru_status_word[idx].zero_()
    if bad:
        raise RuntimeError(f'xps_gru_seq: an in-kernel hand-off of the cluster-persistent GRU recurrence timed out on device(s) {bad} '
                           '(the GPU is shared with another persistent launch?); the results since the last check are invalid.  '
                           'XPS_GRU_CLUSTER=steps runs the same kernels without in-kernel hand-offs')


def set_gru_cluster_mode(name):
    """'persistent' (default), 'steps' (same kernels, one step per launch) or 'off' (per-step GEMM kernels) for 128 < H <= 512."""
    modes = {'off': 0, 'steps': 1, 'persistent': 2}
    if name not in modes:
        raise ValueError(f'gru cluster mode must be one of {sorted(modes)}')
    call('xps_set_gru_cluster_mode', modes[name])


def fused_dropout_supported(T, B, H, ndir):
    """The recurrence kernels of this shape apply the inter-layer dropout themselves (XPS_FUSED_DROPOUT=0: never)."""
    return _memo(('fused_drop', T, B, H, ndir), lambda: bool(_switches.get('XPS_FUSED_DROPOUT'))
                 and bool(lib().xps_gru_seq_fused_dropout_supported(T, B, H, ndir)))


def split4_supported(T, B, H, ndir):
    """The BPTT kernels of this shape can write dgi / dghn as XPS_FMT_SPLIT4 groups (include/xps.h) in the current precision
    mode: their readers (weight-gradient and input-gradient GEMMs) then stage them without conversion arithmetic, same bits.
    XPS_SPLIT4=0: never."""
    key = ('split4', T, B, H, ndir, lib().xps_get_gemm_precision(), lib().xps_get_gru_cluster_mode())
    return _memo(key, lambda: bool(_switches.get('XPS_SPLIT4')) and bool(lib().xps_gru_seq_bwd_split4_supported(T, B, H, ndir)))


def split4_wanted(T, B, H, ndir):
    """Policy on top of split4_supported: pre-split dgi / dghn pay where the 256-tile kernels (compile-time operand formats)
    read them -- the cluster-recurrence shapes, 256 < H <= 512.  At H = 64 / 128 every reader is a 128-tile kernel whose
    split4-capable instantiation carries run-time format flags in its k loop: measured neutral there, while keeping the flags
    out of the fp32-operand instantiation is worth 2.4 % of the cfg-2 step."""
    return H > 256 and split4_supported(T, B, H, ndir)


def _launch_form(B, H):
    """The saved-gates buffer is private between the forward and the BPTT kernels and its layout depends on the launch form
    (member-major on the cluster path, row-major on the single-workgroup path: csrc/xps_gru_cluster.hip).  The form that wrote
    `saved` travels with the forward -- on the autograd ctx, and as `saved.launch_form` for callers of _gru_forward -- so that a
    mode change between forward and backward is an error instead of silently wrong gradients."""
    return (lib().xps_get_gru_cluster_mode() != 0, B, H)


def _check_form(was, B, H):
    now = _launch_form(B, H)
    if was is not None and was != now:
        raise RuntimeError(f'GRU backward: the saved gates were written with cluster path {"on" if was[0] else "off"} (B, H = {was[1:]}) '
                           f'but the backward runs with it {"on" if now[0] else "off"} (B, H = {now[1:]}): the launch form '
                           '(set_gru_cluster_mode / XPS_GRU_CLUSTER) must not change between a forward and its backward')


def _gru_forward(gi, w_hh, b_hh, h0, T, B, H, ndir, save, drop=None):
    dev = gi.device
    y_ext = torch.empty(T + 2, B, ndir * H, dtype=_f32, device=dev)
    saved = torch.empty(ndir, T, B, 4 * H, dtype=_f32, device=dev) if save else None
    if save:
        saved.launch_form = _launch_form(B, H)
    nbytes = _gru_ws_bytes('xps_gru_seq_fwd_f32_workspace', T, B, H, ndir)
    ws = _ws(nbytes, dev)
    if nbytes > 16:
        _gru_status_register(dev)
    if drop is not None:
        # inter-layer dropout fused into the recurrence kernel: a second output y_drop = y * keep / (1 - p)
        y_drop = torch.empty(T, B, ndir * H, dtype=_f32, device=dev)
        call('xps_gru_seq_fwd_drop_f32', _ptr(gi), _ptr_array(w_hh), _ptr_array(b_hh), _ptr(h0), _ptr(y_ext),
             _ptr(saved), T, B, H, ndir, _ptr(y_drop), float(drop[0]), int(drop[1]), _ptr(ws), nbytes, _stream())
        return y_ext, saved, y_drop
    call('xps_gru_seq_fwd_f32', _ptr(gi), _ptr_array(w_hh), _ptr_array(b_hh), _ptr(h0), _ptr(y_ext),
         _ptr(saved), T, B, H, ndir, _ptr(ws), nbytes, _stream())
    return y_ext, saved


def hprev_split_wanted(T, B, H, ndir, split4=None):
    """The weight-gradient group of a large layer (256 < H <= 512, bf16x3 mode: where dgi / dghn are XPS_FMT_SPLIT4 operands and the
    256-tile kernels run) reads h_prev from an XPS_FMT_SPLIT4 image of the state sequence, made by one pass on the stream that
    carries the group: with BOTH operands split the dW_hh products take the LDS-DMA k loop (csrc/xps_gemm_dma.h) -- the group of
    configs[3]'s layer 1 1.07-1.2 ms -> 0.95 ms (tools/bench_wgrad_group.py) for a 0.37-GB pass.  XPS_HPREV_SPLIT=0: never.
    split4: split4_wanted of this shape, where the caller has it (gru_layer_plan)."""
    return ((split4_wanted(T, B, H, ndir) if split4 is None else split4) and (ndir * H) % 4 == 0 and T * B >= 4096 and H % 256 == 0
            and bool(_switches.get('XPS_HPREV_SPLIT')) and bool(_switches.get('XPS_GEMM_DMA')))


def fwd_ysplit_wanted(T, B, H, ndir, hprev=None):
    """The forward recurrence launch writes the XPS_FMT_SPLIT4 image of y_ext that the weight-gradient group reads h_prev from
    (hprev_split_wanted) where the launch can use that image AS its in-kernel exchange buffer (xps_gru_seq_fwd_image_exchange_supported:
    H = 512, no pad trials): the image replaces the ring buffer's stores, and the xps_split4_f32 pass over y_ext in the backward
    (65 us and 0.34 GB per layer at configs[3]'s shape) is gone.  XPS_FWD_YSPLIT=0: the pass.  hprev: hprev_split_wanted of this
    shape, where the caller has it."""
    return (bool(_switches.get('XPS_FWD_YSPLIT')) and (hprev_split_wanted(T, B, H, ndir) if hprev is None else hprev)
            and bool(lib().xps_gru_seq_fwd_image_exchange_supported(T, B, H, ndir)))


def fwd_images_wanted(T, B, H, ndir, hprev=None):
    """OPT-IN (XPS_FWD_IMAGES=1): the forward launch ALSO writes the image of dropout(y) for a layer whose dropped output feeds the
    next layer's GEMMs (layer_output_split4_ok) -- and, off the image-exchange shapes, the image of y_ext as an extra store --
    instead of xps_split4_f32 passes over the finished tensors.  Bit-identical (tests/test_gpu_split4.py), measured level (round 4,
    serial profile: split4 passes 192 -> 0 us, forward kernels 1359 -> 1541 us per step; headline 6.60 vs 6.61 ms): an extra 1-KiB
    store instruction per gate wave and round goes through the per-CU vector-memory pipe that paces the cluster kernels,
    at the price the separate pass pays at HBM speed.  Not the default.  hprev: as in fwd_ysplit_wanted."""
    return (bool(_switches.get('XPS_FWD_IMAGES')) and (hprev_split_wanted(T, B, H, ndir) if hprev is None else hprev)
            and bool(lib().xps_gru_seq_fwd_images_supported(T, B, H, ndir)))


def _gru_forward_images(gi, w_hh, b_hh, T, B, H, ndir, save, want_dropped, drop):
    """_gru_forward (no h0) + the images: returns y_ext, saved, y_split (T + 2, B, ndir*H), y_drop_split (T, B, ndir*H) or None."""
    dev = gi.device
    y_ext = torch.empty(T + 2, B, ndir * H, dtype=_f32, device=dev)
    y_split = torch.empty(T + 2, B, ndir * H, dtype=_f32, device=dev) if save else None
    yd_split = torch.empty(T, B, ndir * H, dtype=_f32, device=dev) if want_dropped else None
    saved = torch.empty(ndir, T, B, 4 * H, dtype=_f32, device=dev) if save else None
    if save:
        saved.launch_form = _launch_form(B, H)
    nbytes = _gru_ws_bytes('xps_gru_seq_fwd_f32_workspace', T, B, H, ndir)
    ws = _ws(nbytes, dev)
    _gru_status_register(dev)
    call('xps_gru_seq_fwd_images_f32', _ptr(gi), _ptr_array(w_hh), _ptr_array(b_hh), None, _ptr(y_ext), _ptr(saved), T, B, H, ndir,
         _ptr(y_split), _ptr(yd_split), float(drop[0]) if (drop and want_dropped) else 0.0, int(drop[1]) if (drop and want_dropped) else 0,
         _ptr(ws), nbytes, _stream())
    return y_ext, saved, y_split, yd_split


def gru_forward_training_form(gi, w_hh, b_hh, T, B, H, ndir):
    """The forward recurrence launch a training step of this shape issues (probes in bench.py / tools/): with the image of y_ext as
    its exchange buffer where fwd_ysplit_wanted, else the plain launch.  Returns (y_ext, saved)."""
    if fwd_ysplit_wanted(T, B, H, ndir):
        return _gru_forward_images(gi, w_hh, b_hh, T, B, H, ndir, True, False, None)[:2]
    return _gru_forward(gi, w_hh, b_hh, None, T, B, H, ndir, True)


def _gru_backward(dy, dhn, y_ext, saved, w_hh, T, B, H, ndir, need_dh0, drop=None, split4=False, form=None):
    """BPTT kernel.  dy (T,B,ndir*H) or None, dhn (ndir,B,H) or None.  Returns dgi (ndir,T,B,3H),
    dghn (ndir,T,B,H), dh0 (ndir,B,H) or None.  split4 (only where split4_supported): dgi / dghn hold XPS_FMT_SPLIT4
    groups -- GEMM operands to be described with rowmap(..., fmt=1), not fp32 values.  form: the _launch_form of the forward
    that wrote `saved` (default: what _gru_forward left on `saved`, if anything)."""
    dev = y_ext.device
    _check_form(form if form is not None else getattr(saved, 'launch_form', None), B, H)
    if dy is not None and not dy.is_contiguous():
        dy = dy.contiguous()
    if dhn is not None and not dhn.is_contiguous():
        dhn = dhn.contiguous()
    if dy is None and dhn is None:
        dhn = torch.zeros(ndir, B, H, dtype=_f32, device=dev)
    if len(w_hh) > 1:           # both directions in one launch
        w_t = [torch.empty(H, 3 * H, dtype=_f32, device=dev) for _ in w_hh]
        call('xps_transpose_batched_f32', _ptr_array(w_hh), _ptr_array(w_t), len(w_hh), 3 * H, H, _stream())
    else:
        w_t = [transpose(w, 3 * H, H) for w in w_hh]
    dgi = torch.empty(ndir, T, B, 3 * H, dtype=_f32, device=dev)
    dghn = torch.empty(ndir, T, B, H, dtype=_f32, device=dev)
    dh0 = torch.empty(ndir, B, H, dtype=_f32, device=dev) if need_dh0 else None
    nbytes = _gru_ws_bytes('xps_gru_seq_bwd_f32_workspace', T, B, H, ndir)
    ws = _ws(nbytes, dev)
    _gru_status_register(dev)
    if split4:
        fused = drop is not None and dy is not None
        call('xps_gru_seq_bwd_split4_f32', _ptr(dy), _ptr(dhn), _ptr(y_ext), _ptr(saved), _ptr_array(w_hh), _ptr_array(w_t), _ptr(dgi),
             _ptr(dghn), _ptr(dh0), T, B, H, ndir, float(drop[0]) if fused else 0.0, int(drop[1]) if fused else 0, _ptr(ws), nbytes,
             _stream())
        return dgi, dghn, dh0
    if drop is not None and dy is not None:
        # dy is the gradient w.r.t. the dropped output of the forward kernel: the decisions are re-made while it is loaded
        call('xps_gru_seq_bwd_drop_f32', _ptr(dy), _ptr(dhn), _ptr(y_ext), _ptr(saved), _ptr_array(w_hh), _ptr_array(w_t), _ptr(dgi),
             _ptr(dghn), _ptr(dh0), T, B, H, ndir, float(drop[0]), int(drop[1]), _ptr(ws), nbytes, _stream())
        return dgi, dghn, dh0
    call('xps_gru_seq_bwd_f32', _ptr(dy), _ptr(dhn), _ptr(y_ext), _ptr(saved), _ptr_array(w_hh), _ptr_array(w_t), _ptr(dgi),
         _ptr(dghn), _ptr(dh0), T, B, H, ndir, _ptr(ws), nbytes, _stream())
    return dgi, dghn, dh0


def _recurrent_grad_problems(dgi, dghn, y_ext, w_hh_params, b_hh_params, T, B, H, ndir, fmt=0, y_fmt=0):
    """dW_hh = dgh^T h_prev and db_hh = colsum(dgh) as grouped-TN problems.  h_prev(t) are slots of
    y_ext (forward: slots 0..T-1, reverse: slots 2..T+1); the r,z rows of dgh are dgi's, the n rows dghn.
    fmt = 1: dgi / dghn are XPS_FMT_SPLIT4 operands (_gru_backward(split4=True)); y_fmt = 1: so is `y_ext` (a split4 image of
    the state sequence: hprev_split_wanted)."""
    dev = y_ext.device
    ldy = ndir * H
    probs, rets = [], []
    for d in range(ndir):
        dw, db, acc_w, rw, rb = _grad_targets(w_hh_params[d], (3 * H, H), b_hh_params[d], (3 * H,), dev)
        first_slot = 0 if d == 0 else 2
        hprev = y_ext.view(-1)[first_slot * B * ldy + d * H:]
        probs.append(tn_problem(dgi[d], hprev, dw, 2 * H, H, T * B, ra=rowmap(3 * H, fmt=fmt), rb=rowmap(ldy, fmt=y_fmt), rc=rowmap(H),
                                colsum_out=db, accumulate=acc_w))
        probs.append(tn_problem(dghn[d], hprev, dw[2 * H:], H, H, T * B, ra=rowmap(H, fmt=fmt), rb=rowmap(ldy, fmt=y_fmt), rc=rowmap(H),
                                colsum_out=db[2 * H:], accumulate=acc_w))
        rets.append((rw, rb))
    return probs, rets


class GRURecurFn(torch.autograd.Function):
    """Fused GRU recurrence given the input projections gi (ndir, T, B, 3H).
    Returns y_ext (T+2, B, ndir*H): slot t+1 = h_t (see include/xps.h)."""

    @staticmethod
    def forward(ctx, gi, h0, ndir, *wb):
        _need_gpu(gi, h0, *wb)
        w_hh = [w.contiguous() for w in wb[:ndir]]
        b_hh = [b.contiguous() for b in wb[ndir:]]
        gi = gi.contiguous()
        _, T, B, H3 = gi.shape
        H = H3 // 3
        h0c = None if h0 is None else h0.contiguous()
        save = any(ctx.needs_input_grad)
        y_ext, saved = _gru_forward(gi, w_hh, b_hh, h0c, T, B, H, ndir, save)
        if save:
            ctx.save_for_backward(y_ext, saved, *w_hh)
            ctx.form = saved.launch_form
        ctx.params = wb
        ctx.dims = (T, B, H, ndir)
        ctx.has_h0 = h0 is not None
        return y_ext

    @staticmethod
    def backward(ctx, dy_ext):
        y_ext, saved, *w_hh = ctx.saved_tensors
        T, B, H, ndir = ctx.dims
        need_dh0 = ctx.has_h0 and ctx.needs_input_grad[1]
        dgi, dghn, dh0 = _gru_backward(dy_ext[1:T + 1], None, y_ext, saved, w_hh, T, B, H, ndir, need_dh0, form=ctx.form)
        if need_dh0:                                   # gradient that arrived directly on the h0 slots of y_ext
            dh0[0] += dy_ext[0, :, :H]
            if ndir == 2:
                dh0[1] += dy_ext[T + 1, :, H:]
        probs, rets = _recurrent_grad_problems(dgi, dghn, y_ext, ctx.params[:ndir], ctx.params[ndir:], T, B, H, ndir)
        gemm_tn_grouped(probs, y_ext.device)
        return (dgi, dh0, None, *[r[0] for r in rets], *[r[1] for r in rets])


HN_NONE, HN_STACK, HN_SUM = 0, 1, 2


FMT_X_SPLIT4, FMT_Y_SPLIT4 = 1, 2


def split4_mode():
    """XPS_FMT_SPLIT4 operands are in use: bf16x3 product mode and not switched off (XPS_SPLIT4=0)."""
    return lib().xps_get_gemm_precision() == 1 and bool(_switches.get('XPS_SPLIT4'))


def layer_output_split4_ok(T, B, H, ndir, drop_p):
    """A GRU layer whose dropped output is read by the NEXT layer's GEMMs only (input projection, dW_ih) can write it as
    XPS_FMT_SPLIT4 groups in the dropout pass it runs anyway (shapes whose recurrence kernels do not fuse the dropout; H > 256:
    where the 256-tile kernels read it, see split4_wanted)."""
    return bool(drop_p and drop_p > 0.0 and split4_mode() and H > 256 and (ndir * H) % 4 == 0
                and not fused_dropout_supported(T, B, H, ndir))


def _presplit_weights_ok(rows, In, H3):
    """Pre-splitting W_ih (one small launch per matrix and forward pass) pays when the projection / input-gradient GEMMs
    that read it are large (configs[3] layer 1: 40960 x 1536 x 1024); XPS_SPLIT4_WEIGHTS=0: never."""
    return (split4_mode() and In % 4 == 0 and rows >= 4096 and In * H3 >= _switches.get('XPS_SPLIT4_WEIGHTS_MIN')
            and bool(_switches.get('XPS_SPLIT4_WEIGHTS')))


def skinny_dx_wanted(rows, In, K):
    """OPT-IN (XPS_SKINNY_DX=1): the input gradient of a large layer with few input channels on the LDS-DMA loop through a
    zero-padded weight image (xps_split4_pad_f32).  Measured on configs[3] layer 0 (40960 x 100 x 3072, round 4, rocprofv3):
    261 us against 213 us for the 64-row edge tiles -- one 256-row tile per CU streams its 3 MB of dgi AND 3 MB of padded
    weight rows through the same ~25 GB/s per-CU LDS ingest, on 160 of 256 CUs; the edge tiles re-use the weight tile from L1 /
    L2 three blocks per CU.  Same bits either way (tests/test_gpu_gemm_big.py); not the default."""
    return (bool(_switches.get('XPS_SKINNY_DX')) and split4_mode() and In % 4 == 0 and In < 256 and rows % 256 == 0
            and rows >= 96 * 256 and K % 32 == 0 and K >= 512 and bool(_switches.get('XPS_GEMM_DMA')))


def split4_pad(w, ldo):
    """XPS_FMT_SPLIT4 image of the 2-D matrix w with leading dimension ldo (zero beyond w's columns)."""
    w = w.contiguous()
    out = torch.empty(w.shape[0], ldo, dtype=_f32, device=w.device)
    call('xps_split4_pad_f32', _ptr(w), w.shape[1], w.shape[0], w.shape[1], _ptr(out), ldo, _stream())
    return out


def split4(x, drop_p=0.0, seed=0):
    """XPS_FMT_SPLIT4 image of dropout(x) (drop_p = 0: of x): a GEMM input operand for rowmap(..., fmt=1), not fp32 values."""
    out = torch.empty_like(x)
    call('xps_split4_f32', _ptr(x), _ptr(out), x.numel(), float(drop_p), int(seed), _stream())
    return out


class GruPlan(NamedTuple):
    """Everything that is decided for one GRULayerFmtFn call: made once by gru_layer_plan in the forward, obeyed by the backward."""
    cluster_on: bool        # launch form of the recurrence (_launch_form)
    precision: int          # xps_get_gemm_precision() the formats below were chosen under
    drop_fused: bool        # the recurrence kernels apply the inter-layer dropout (else: a separate pass each way)
    x_fmt: int              # x holds XPS_FMT_SPLIT4 groups (FMT_X_SPLIT4)
    w_fmt: int              # W_ih is split once per forward pass (_presplit_weights_ok)
    y_out_split: bool       # the dropped output is written as XPS_FMT_SPLIT4 groups (FMT_Y_SPLIT4)
    fwd_images: bool        # fwd_images_wanted
    fwd_ysplit: bool        # fwd_ysplit_wanted
    want_dropped: bool      # the forward launch also writes the image of the dropped output
    bwd_split4: int         # dgi / dghn as XPS_FMT_SPLIT4 operands (split4_wanted): they only feed GEMMs, same bits
    y_fmt: int              # dW_hh reads h_prev from a split4 image of the state sequence (hprev_split_wanted)
    skinny_dx: bool         # skinny_dx_wanted


def gru_layer_plan(T, B, In, H, ndir, drop_p, fmt):
    """The GruPlan of one layer call under the library state and the switches (_switches) of this moment."""
    has_drop = bool(drop_p and drop_p > 0.0)
    drop_fused = bool(has_drop and fused_dropout_supported(T, B, H, ndir))
    y_out_split = bool(fmt & FMT_Y_SPLIT4)
    if y_out_split and (not has_drop or drop_fused):
        raise ValueError('FMT_Y_SPLIT4: only with a separate dropout pass (see layer_output_split4_ok)')
    w_fmt = 1 if _presplit_weights_ok(T * B, In, 3 * H) else 0
    split4 = bool(split4_wanted(T, B, H, ndir))
    hprev = bool(hprev_split_wanted(T, B, H, ndir, split4))
    fwd_images = bool(fwd_images_wanted(T, B, H, ndir, hprev))
    return GruPlan(cluster_on=lib().xps_get_gru_cluster_mode() != 0, precision=lib().xps_get_gemm_precision(), drop_fused=drop_fused,
                   x_fmt=1 if (fmt & FMT_X_SPLIT4) else 0, w_fmt=w_fmt, y_out_split=y_out_split, fwd_images=fwd_images,
                   fwd_ysplit=bool(fwd_ysplit_wanted(T, B, H, ndir, hprev)), want_dropped=fwd_images and y_out_split,
                   bwd_split4=int(split4), y_fmt=int(hprev),
                   skinny_dx=bool(split4 and not w_fmt and skinny_dx_wanted(T * B, In, 3 * H)))


class GRULayerFmtFn(torch.autograd.Function):
    """One (bi)directional GRU layer over a time-major input x (T, B, In):
    input projection GEMMs for all steps + fused recurrence; backward = BPTT kernel + ONE grouped
    launch for all six weight/bias gradients.  weights: per direction (w_ih, w_hh, b_ih, b_hh).
    Returns (y (T, B, ndir*H), hn).  hn_mode selects what hn is: HN_STACK (ndir, B, H) final state of each
    direction; HN_SUM (B, H) their sum (what the seq2seq encoder hands to the decoder: one strided add, and
    the backward gets ONE (B, H) gradient for both directions); HN_NONE: None (inner layers)."""

    @staticmethod
    def forward(ctx, x, ndir, hn_mode, drop_p, fmt, *wb):
        """drop_p > 0: the layer's output goes through inverted dropout (torch.nn.GRU's inter-layer dropout), fused into the
        recurrence kernels where they support it (fused_dropout_supported), else a separate pass; hn stays undropped.
        fmt: FMT_X_SPLIT4 -- x holds XPS_FMT_SPLIT4 groups (the previous layer wrote them); FMT_Y_SPLIT4 -- write the
        dropped output that way (only where layer_output_split4_ok): such a tensor is a GEMM operand, not fp32 values."""
        ctx.set_materialize_grads(False)
        _need_gpu(x, *wb)
        x = x.contiguous()
        T, B, In = x.shape
        w_ih = [wb[4 * d + 0].contiguous() for d in range(ndir)]
        w_hh = [wb[4 * d + 1].contiguous() for d in range(ndir)]
        b_ih = [wb[4 * d + 2].contiguous() for d in range(ndir)]
        b_hh = [wb[4 * d + 3].contiguous() for d in range(ndir)]
        H = w_hh[0].shape[1]
        plan = ctx.plan = gru_layer_plan(T, B, In, H, ndir, drop_p, fmt)
        gi = torch.empty(ndir, T, B, 3 * H, dtype=_f32, device=x.device)
        # large layers: W_ih split once per forward pass (its readers: this projection and the backward's input gradient)
        if plan.w_fmt:
            w_ih = [split4(w) for w in w_ih]
        ra, rb, rc = rowmap(In, fmt=plan.x_fmt), rowmap(In, fmt=plan.w_fmt), rowmap(3 * H)          # all directions in ONE launch
        call('xps_gemm_nt_multi_f32', _ptr(x), C.byref(ra), _ptr_array(w_ih), C.byref(rb), _ptr_array([gi[d] for d in range(ndir)]),
             C.byref(rc), _ptr_array(b_ih), ndir, T * B, 3 * H, In, _stream())
        save = any(ctx.needs_input_grad)
        drop = None
        y_drop = None
        if drop_p and drop_p > 0.0:
            drop = (float(drop_p), next_dropout_seed())
        ctx.drop = drop
        y_split = None
        if (save and (plan.fwd_images or plan.fwd_ysplit)) or plan.want_dropped:
            # the recurrence kernel's epilogue writes the split4 images of y_ext (h_prev of dW_hh) and of the dropped output
            y_ext, saved, y_split, y_drop = _gru_forward_images(gi, w_hh, b_hh, T, B, H, ndir, save, plan.want_dropped, drop)
        elif plan.drop_fused:
            y_ext, saved, y_drop = _gru_forward(gi, w_hh, b_hh, None, T, B, H, ndir, save, drop)
        else:
            y_ext, saved = _gru_forward(gi, w_hh, b_hh, None, T, B, H, ndir, save)
        if save:                                # (y_split: there iff plan.fwd_images or plan.fwd_ysplit)
            ctx.save_for_backward(x, y_ext, saved, *w_ih, *w_hh, *([y_split] if y_split is not None else []))
        ctx.params = wb
        ctx.dims = (T, B, H, ndir, In, hn_mode)
        # y: per-step outputs (a view of y_ext: slots 1..T); hn: final hidden state of each direction
        # (forward: t = T-1, reverse: t = 0), returned separately so that a consumer of the final state
        # only (the seq2seq encoder) sends back a small gradient instead of a zero-padded (T, B, .) one
        y = y_ext[1:T + 1]
        if y_drop is not None:
            y = y_drop
        elif drop is not None:                  # shapes without the fused path: the same decisions in a separate pass
            out = torch.empty(T, B, ndir * H, dtype=_f32, device=x.device)
            if plan.y_out_split:                # same decisions and values, written as the hi / lo split the next layer's GEMMs stage
                call('xps_split4_f32', _ptr(y), _ptr(out), out.numel(), drop[0], drop[1], _stream())
            else:
                call('xps_dropout_f32', _ptr(y), _ptr(out), None, out.numel(), drop[0], drop[1], _stream())
            y = out
        if hn_mode == HN_NONE:
            hn = None
        elif hn_mode == HN_SUM:
            hn = y_ext[T, :, :H] + y_ext[1, :, H:] if ndir == 2 else y_ext[T, :, :H].clone()
        else:
            hn = torch.stack([y_ext[T, :, :H]] + ([y_ext[1, :, H:]] if ndir == 2 else []), dim=0)
        return y, hn

    @staticmethod
    def backward(ctx, dy, dhn):
        T, B, H, ndir, In, hn_mode = ctx.dims
        if dhn is not None and hn_mode == HN_SUM:          # the same (B, H) gradient reaches both directions
            dhn = dhn.unsqueeze(0).expand(ndir, B, H).contiguous()
        plan = ctx.plan
        if lib().xps_get_gemm_precision() != plan.precision:
            names = {v: k for k, v in GEMM_PRECISIONS.items()}
            raise RuntimeError(f'GRU backward: the forward chose its operand formats in {names[plan.precision]} mode but the backward '
                               f'runs in {names[lib().xps_get_gemm_precision()]} mode: the product precision (set_gemm_precision / '
                               'XPS_GEMM_PRECISION) must not change between a forward and its backward')
        x, y_ext, saved, *w = ctx.saved_tensors
        y_split = w.pop() if (plan.fwd_images or plan.fwd_ysplit) else None
        w_ih, w_hh = w[:ndir], w[ndir:]
        fmt, y_fmt, x_fmt, w_fmt = plan.bwd_split4, plan.y_fmt, plan.x_fmt, plan.w_fmt
        wb = ctx.params
        if ctx.drop is not None and dy is not None and not plan.drop_fused:
            dyc = dy.contiguous()
            dyd = torch.empty_like(dyc)
            call('xps_dropout_f32', _ptr(dyc), _ptr(dyd), None, dyc.numel(), ctx.drop[0], ctx.drop[1], _stream())
            dy = dyd
        dgi, dghn, _ = _gru_backward(dy, dhn, y_ext, saved, w_hh, T, B, H, ndir, False, ctx.drop if plan.drop_fused else None,
                                     split4=bool(fmt), form=(plan.cluster_on, B, H))
        dev = x.device
        # weight gradients first: on the side stream they depend on the recurrence kernel only, so they start
        # together with the input-gradient GEMM below instead of after it (and are out of the way earlier)
        have_img = y_split is not None                                 # written by the forward kernel (an image: only where y_fmt)
        y_src = (y_split if have_img else torch.empty_like(y_ext)) if y_fmt else y_ext   # (else filled on the group's stream: below)
        probs, rets_hh = _recurrent_grad_problems(dgi, dghn, y_src, [wb[4 * d + 1] for d in range(ndir)],
                                                  [wb[4 * d + 3] for d in range(ndir)], T, B, H, ndir, fmt, y_fmt)
        rets_ih = []
        for d in range(ndir):
            dw, db, acc_w, rw, rb = _grad_targets(wb[4 * d + 0], (3 * H, In), wb[4 * d + 2], (3 * H,), dev)
            probs.append(tn_problem(dgi[d], x, dw, 3 * H, In, T * B, ra=rowmap(3 * H, fmt=fmt), rb=rowmap(In, fmt=x_fmt),
                                    colsum_out=db, accumulate=acc_w))
            rets_ih.append((rw, rb))
        direct = all(r[0] is None and r[1] is None for r in rets_ih + rets_hh)
        def launch_group(st):
            if y_fmt and not have_img:
                call('xps_split4_f32', _ptr(y_ext), _ptr(y_src), y_ext.numel(), 0.0, 0, _stream() if st is None else st)
            return gemm_tn_grouped(probs, dev, st)
        _launch_weight_grads(launch_group, dev, (dgi, dghn, x, y_ext, y_src), direct)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(T, B, In, dtype=_f32, device=dev)
            if plan.skinny_dx:
                # few input channels (configs[3] layer 0: In = 100): dx = dgi W_ih is bound by the read of dgi (503 MB), not by the
                # matrix pipe -- W_ih as a zero-padded 256-column split4 image, so that the product takes ONE 256-wide tile per 256
                # rows on the LDS-DMA loop (gemm_big_kernel<.., 5>) instead of 64-row edge tiles; measured SLOWER (261 vs 213 us): opt-in, see skinny_dx_wanted
                w_ih = [split4_pad(w, 256) for w in w_ih]
                w_fmt, ldw = 1, 256
            else:
                ldw = In
            if ndir == 2:       # both directions summed in registers: one launch, no accumulate pass over dx
                ra, rb, rc = rowmap(3 * H, fmt=fmt), rowmap(ldw, fmt=w_fmt), rowmap(In)
                call('xps_gemm_nn2_f32', _ptr(dgi[0]), _ptr(w_ih[0]), 3 * H, _ptr(dgi[1]), _ptr(w_ih[1]), 3 * H,
                     C.byref(ra), C.byref(rb), _ptr(dx), C.byref(rc), T * B, In, 0, _stream())
            else:
                gemm_nn(dgi[0], w_ih[0], dx, T * B, In, 3 * H, ra=rowmap(3 * H, fmt=fmt), rb=rowmap(ldw, fmt=w_fmt))
        grads = []
        for d in range(ndir):
            grads += [rets_ih[d][0], rets_hh[d][0], rets_ih[d][1], rets_hh[d][1]]
        return (dx, None, None, None, None, *grads)


class GRULayerDropFn(torch.autograd.Function):
    """GRULayerFmtFn on plain fp32 tensors: (x, ndir, hn_mode, drop_p, *weights)."""

    @staticmethod
    def forward(ctx, x, ndir, hn_mode, drop_p, *wb):
        return GRULayerFmtFn.forward(ctx, x, ndir, hn_mode, drop_p, 0, *wb)

    @staticmethod
    def backward(ctx, dy, dhn):
        g = GRULayerFmtFn.backward(ctx, dy, dhn)
        return g[:4] + g[5:]


class GRULayerFn(torch.autograd.Function):
    """GRULayerDropFn without the inter-layer dropout: (x, ndir, hn_mode, *weights)."""

    @staticmethod
    def forward(ctx, x, ndir, hn_mode, *wb):
        return GRULayerDropFn.forward(ctx, x, ndir, hn_mode, 0.0, *wb)

    @staticmethod
    def backward(ctx, dy, dhn):
        g = GRULayerDropFn.backward(ctx, dy, dhn)
        return g[:3] + g[4:]


# --------------------------------------------------------------------------- #
# TemporalConv: Conv1d -> BatchNorm1d -> [ReLU] -> Dropout                      #
# --------------------------------------------------------------------------- #
POST_SYNCBN_HOOKS = []
def _dp_world(group):
    """World size of `group` when torch.distributed is up, else 1.  The data-parallel paths (SyncBN exchanges, gradient
    all-reduce) run iff _dp_enabled(group)."""
    import torch.distributed as dist
    if group is not None and dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group)
    return 1


def _dp_enabled(group):
    """Production rule: more than one rank.  (The one-rank RCCL rehearsals -- tests/dp_worker.py --device nccl1,
    bench.py with XPS_BENCH_FORCE_DP=1 -- replace THIS function from the outside to exercise the same code on a one-GPU box.)"""
    return _dp_world(group) > 1


def _dist_sum_(t, group):
    """In-place sum over the ranks of `group` when the data-parallel paths are on; returns whether it ran."""
    if _dp_enabled(group):
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return True
    return False


def _global_rows(rows, group, device, global_trials, Tp):
    """SyncBN denominator = rows summed over ranks.  When the caller knows the global trial count of this
    batch (the trainer does: it shards the batch itself) no communication is needed; otherwise one small
    host-synchronising all-reduce."""
    if global_trials is not None:
        return float(global_trials) * Tp
    cnt = torch.tensor([float(rows)], dtype=torch.float64, device=device)
    _dist_sum_(cnt, group)
    return float(cnt.item())


class TemporalConvFn(torch.autograd.Function):
    """x (B, T, C) -> (T', B, F) time-major.  The strided convolution is ONE GEMM over
    window rows of x (row map: trial stride T*C, window stride s*C, K = k*C contiguous)
    with the bias fused; BatchNorm batch statistics are a deterministic two-stage column
    reduction (all-reduced over `group` = SyncBN when data-parallel)."""

    @staticmethod
    def forward(ctx, x, conv_w, conv_b, gamma, beta, running_mean, running_var, stride, training,
                relu, drop_mask, drop_scale, momentum, eps, group, global_trials=None, num_batches_tracked=None):
        _need_gpu(x, conv_w)
        x = x.contiguous()
        B, T, Cin = x.shape
        F, _, k = conv_w.shape
        Tp = (T - k) // stride + 1
        if Tp < 1:
            raise ValueError('TemporalConv: sequence shorter than the kernel')
        w2 = conv_w.permute(0, 2, 1).contiguous().view(F, k * Cin)      # (F, k*C): K index = kk*C + c
        rows = Tp * B
        y = torch.empty(Tp, B, F, dtype=_f32, device=x.device)
        ra = rowmap(stride * Cin, rpg=Tp, gs=T * Cin)       # window row m = (b, t')
        rc = rowmap(B * F, rpg=Tp, gs=F)                    # -> time-major row (t', b)
        gemm_nt(x, w2, y, rows, F, k * Cin, bias=conv_b, ra=ra, rc=rc)
        out = torch.empty_like(y)
        if training:
            # two passes (BatchNorm statistics): sum y, then sum (y - mean)^2 about the global mean
            stats = torch.empty(2 * F, dtype=_f32, device=x.device)
            nbytes = lib().xps_colsum_f32_workspace(rows, F)
            ws = _ws(nbytes, x.device)
            call('xps_colsum_f32', _ptr(y), F, rows, F, _ptr(stats), None, 0, _ptr(ws), nbytes, _stream())
            count = float(rows)
            if _dist_sum_(stats[:F], group):
                count = _global_rows(rows, group, x.device, global_trials, Tp)
            call('xps_bn_centered_sumsq_f32', _ptr(y), rows, F, _ptr(stats), count, _ptr(stats[F:]), _ptr(ws), nbytes,
                 _stream())
            _dist_sum_(stats[F:], group)
            mean = torch.empty(F, dtype=_f32, device=x.device)
            rstd = torch.empty(F, dtype=_f32, device=x.device)
            call('xps_bn_finalize_apply_f32', _ptr(y), _ptr(stats), count, _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd),
                 _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), momentum, eps, _ptr(drop_mask), drop_scale,
                 _ptr(out), rows, F, int(relu), _stream())
            ctx.save_for_backward(x, w2, y, out, mean, rstd, gamma, drop_mask)
            ctx.cfg = (B, T, Cin, F, k, stride, Tp, relu, drop_scale, count, group)
            ctx.conv_w = conv_w
            ctx.conv_b = conv_b
            ctx.bn_params = (gamma, beta)
        else:
            call('xps_bn_apply_eval_f32', _ptr(y), _ptr(running_mean), _ptr(running_var), eps, _ptr(gamma),
                 _ptr(beta), _ptr(out), rows, F, int(relu), _stream())
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w2, y, out, mean, rstd, gamma, drop_mask = ctx.saved_tensors
        B, T, Cin, F, k, stride, Tp, relu, drop_scale, count, group = ctx.cfg
        rows = Tp * B
        dev = x.device
        dout = dout.contiguous()
        sums = torch.empty(2 * F, dtype=_f32, device=dev)
        nbytes = lib().xps_bn_bwd_workspace(rows, F)
        ws = _ws(nbytes, dev)
        # BatchNorm parameter gradients = the LOCAL sums: added straight into the .grad buffers by the reduction
        # kernel when they exist (no clone, no add launches), else handed to autograd as slices
        g_beta, acc_beta, _ = _grad_target(ctx.bn_params[1], (F,), dev)
        g_gamma, acc_gamma, _ = _grad_target(ctx.bn_params[0], (F,), dev)
        direct_bn = acc_beta and acc_gamma
        dp = _dp_enabled(group)
        call('xps_bn_bwd_reduce_f32', _ptr(dout), _ptr(out), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(drop_mask),
             drop_scale, int(relu), _ptr(sums), _ptr(g_beta) if direct_bn else None, _ptr(g_gamma) if direct_bn else None,
             rows, F, _ptr(ws), nbytes, _stream())
        dbeta = dgamma = None
        if not direct_bn:
            local = sums.clone() if dp else sums
            dbeta, dgamma = local[:F], local[F:]
        if dp:                                  # SyncBN: the dy formula needs the global sums
            _dist_sum_(sums, group)
            # every gradient downstream of this layer is enqueued by now: a data-parallel optimiser may start
            # reducing them (AFTER the statistics exchange above, so that it never queues behind a large one)
            for hook in list(POST_SYNCBN_HOOKS):
                hook()
        dy = torch.empty_like(y)
        call('xps_bn_bwd_apply_f32', _ptr(dout), _ptr(out), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma),
             _ptr(drop_mask), drop_scale, int(relu), _ptr(sums), count, _ptr(dy), rows, F, _stream())
        # dW2[f][kk*C + c] = sum_m dy[m][f] * window[m][kk*C + c], m = (b, t'); conv-bias gradient = the
        # column sums of dy, produced by the same launch
        dconv_b, acc_cb, r_cb = _grad_target(ctx.conv_b, (F,), dev) if ctx.conv_b is not None else (None, False, None)
        if dconv_b is None:
            dconv_b = r_cb = torch.empty(F, dtype=_f32, device=dev)
        dw2 = torch.empty(F, k * Cin, dtype=_f32, device=dev)
        # contraction rows in (t', b) order: dy is then a plain contiguous matrix and the window rows of x form
        # groups of B rows (stride T*C) per t' (stride s*C) -- k-tiles never straddle a group when 16 | B, which
        # keeps both operands on the unguarded load path
        gemm_tn_grouped([tn_problem(dy, x, dw2, F, k * Cin, rows, ra=rowmap(F),
                                    rb=rowmap(T * Cin, rpg=B, gs=stride * Cin), colsum_out=dconv_b,
                                    accumulate_colsum=acc_cb)], dev)
        gw, acc_w, _ = _grad_target(ctx.conv_w, (F, Cin, k), dev)
        if acc_w:                               # un-permute and accumulate in one pass, straight into .grad
            gw.add_(dw2.view(F, k, Cin).permute(0, 2, 1))
            dconv_w = None
        else:
            dconv_w = dw2.view(F, k, Cin).permute(0, 2, 1).contiguous()
        return (None, dconv_w, r_cb, dgamma, dbeta) + (None,) * 12


# --------------------------------------------------------------------------- #
# decoder glue, dropout, loss                                                   #
# --------------------------------------------------------------------------- #
def decoder_supported(H, C, L):
    return bool(lib().xps_decoder_supported(int(H), int(C), int(L)))


class DecoderFn(torch.autograd.Function):
    """All decode steps of a one-layer GRU decoder in ONE launch (xps_decoder_fwd_f32) and one
    backward launch + one grouped weight-gradient launch.  Returns logits (B, L, C)."""

    @staticmethod
    def forward(ctx, table, h0, w_hh, b_hh, w_fc, b_fc, teacher, flags, start_token, L):
        ctx.set_materialize_grads(False)               # no zero tensor for the (integer) tokens output
        _need_gpu(table, h0, w_hh, w_fc)
        table, h0c = table.contiguous(), h0.contiguous()
        w_hh_c, b_hh_c, w_fc_c, b_fc_c = w_hh.contiguous(), b_hh.contiguous(), w_fc.contiguous(), b_fc.contiguous()
        B, H = h0c.shape
        C = w_fc_c.shape[0]
        ntok = table.shape[0]
        dev = h0c.device
        save = any(ctx.needs_input_grad)
        logits = torch.empty(B, L, C, dtype=_f32, device=dev)
        tokens = torch.empty(L, B, dtype=torch.int64, device=dev)
        hs = torch.empty(L + 1, B, H, dtype=_f32, device=dev)
        saved = torch.empty(L, B, 4 * H, dtype=_f32, device=dev) if save else None
        if teacher is not None:
            teacher = teacher.contiguous()
            if tuple(teacher.shape) != (B, L):
                raise ValueError('teacher tokens must be (batch, seq_length)')
        call('xps_decoder_fwd_f32', _ptr(table), _ptr(w_hh_c), _ptr(b_hh_c), _ptr(h0c), _ptr(w_fc_c), _ptr(b_fc_c),
             _ptr(teacher), _ptr(flags) if teacher is not None else None, _ptr(logits), _ptr(tokens), _ptr(hs),
             _ptr(saved), B, H, C, L, ntok, int(start_token), _stream())
        if save:
            ctx.save_for_backward(tokens, hs, saved, w_hh_c, w_fc_c)
        ctx.params = (w_hh, b_hh, w_fc, b_fc)
        ctx.dims = (B, H, C, L, ntok)
        ctx.mark_non_differentiable(tokens)
        return logits, tokens

    @staticmethod
    def backward(ctx, dlogits, _dtok):
        tokens, hs, saved, w_hh_c, w_fc_c = ctx.saved_tensors
        B, H, C, L, ntok = ctx.dims
        w_hh, b_hh, w_fc, b_fc = ctx.params
        dev = hs.device
        if dlogits is None:
            return (None,) * 10
        dlogits = dlogits.contiguous()
        w_t = transpose(w_hh_c, 3 * H, H)
        dgi = torch.empty(L, B, 3 * H, dtype=_f32, device=dev)
        dghn = torch.empty(L, B, H, dtype=_f32, device=dev)
        dh0 = torch.empty(B, H, dtype=_f32, device=dev)
        call('xps_decoder_bwd_f32', _ptr(dlogits), _ptr(hs), _ptr(saved), _ptr(w_t), _ptr(w_fc_c), _ptr(dgi), _ptr(dghn),
             _ptr(dh0), B, H, C, L, _stream())
        dtable, r_wh, r_bh, r_wf, r_bf = _decoder_weight_grads(dlogits, dgi, dghn, hs, tokens, ctx.params, B, H, C, L, ntok)
        return dtable, dh0, r_wh, r_bh, r_wf, r_bf, None, None, None, None


def _decoder_weight_grads(dlogits, dgi, dghn, hs, tokens, params, B, H, C, L, ntok):
    """Shared tail of the decoder backward passes: W_hh / b_hh from (dgi, dghn) x h_prev = hs[0:L], W_fc / b_fc from
    dlogits x hs[1:L+1] in ONE grouped launch over all steps, and d table[tok] += dgi over all (step, trial) rows."""
    w_hh, b_hh, w_fc, b_fc = params
    dev = hs.device
    dwh, acc_h, r_wh = _grad_target(w_hh, (3 * H, H), dev)
    dbh, acc_bh, r_bh = _grad_target(b_hh, (3 * H,), dev)
    dwf, acc_f, r_wf = _grad_target(w_fc, (C, H), dev)
    dbf, acc_bf, r_bf = _grad_target(b_fc, (C,), dev)
    if not (acc_h == acc_bh and acc_f == acc_bf):
        dwh, dbh = torch.empty(3 * H, H, dtype=_f32, device=dev), torch.empty(3 * H, dtype=_f32, device=dev)
        dwf, dbf = torch.empty(C, H, dtype=_f32, device=dev), torch.empty(C, dtype=_f32, device=dev)
        acc_h = acc_f = False
        r_wh, r_bh, r_wf, r_bf = dwh, dbh, dwf, dbf
    hprev = hs                                   # rows (s, b): hs[s]
    hnext = hs.view(-1)[B * H:]                  # rows (s, b): hs[s + 1]
    probs = [
        tn_problem(dgi, hprev, dwh, 2 * H, H, L * B, ra=rowmap(3 * H), rb=rowmap(H), rc=rowmap(H),
                   colsum_out=dbh, accumulate=acc_h),
        tn_problem(dghn, hprev, dwh[2 * H:], H, H, L * B, ra=rowmap(H), rb=rowmap(H), rc=rowmap(H),
                   colsum_out=dbh[2 * H:], accumulate=acc_h),
        # dlogits is (B, L, C): row (s, b) lives at b*L*C + s*C
        tn_problem(dlogits, hnext, dwf, C, H, L * B, ra=rowmap(L * C, rpg=B, gs=C), rb=rowmap(H), rc=rowmap(H),
                   colsum_out=dbf, accumulate=acc_f),
    ]
    _launch_weight_grads(lambda st: gemm_tn_grouped(probs, dev, st), dev, (dgi, dghn, hs, dlogits),
                         r_wh is None and r_bh is None and r_wf is None and r_bf is None)
    dtable = torch.empty(ntok, 3 * H, dtype=_f32, device=dev)
    nbytes = lib().xps_scatter_rows_f32_workspace(L * B, 3 * H, ntok)
    ws = _ws(nbytes, dev)
    call('xps_scatter_rows_f32', _ptr(dgi), _ptr(tokens), _ptr(dtable), L * B, 3 * H, ntok, 0, _ptr(ws), nbytes,
         _stream())
    return dtable, r_wh, r_bh, r_wf, r_bf


class DecoderWideFn(torch.autograd.Function):
    """One-layer GRU decoder (nn_models/models.py:719-761, decode loop :285-301) for hidden sizes the one-launch kernel of
    DecoderFn does not hold in a workgroup (H = 500 / 512 of the north-star shape).  Forward: per step the token-projection
    gather, ONE recurrence step (the generic / cluster GRU entry point on a sliding 3-slot window of one state buffer, so that
    the L steps leave ONE (L + 2)-slot state sequence and ONE saved-gates sequence behind), the output Linear written straight
    into its (step, trial) rows, the next-token choice on the device.  Backward: the tokens are known, so the L steps are ONE
    BPTT launch (dy = dlogits W_fc for all steps from one GEMM), ONE grouped weight-gradient launch over all steps and one
    scatter for the token table -- instead of L times {recurrence backward, two weight-gradient launches + reduces, scatter,
    transposes and autograd's adds / fills}: 85 -> 35 launches, 0.94 -> ~0.45 ms per configs[3] step."""

    @staticmethod
    def forward(ctx, table, h0, w_hh, b_hh, w_fc, b_fc, teacher, flags, start_token, L):
        ctx.set_materialize_grads(False)
        _need_gpu(table, h0, w_hh, w_fc)
        table, h0c = table.contiguous(), h0.contiguous()
        w_hh_c, b_hh_c, w_fc_c, b_fc_c = w_hh.contiguous(), b_hh.contiguous(), w_fc.contiguous(), b_fc.contiguous()
        B, H = h0c.shape
        C = w_fc_c.shape[0]
        ntok = table.shape[0]
        dev = h0c.device
        save = any(ctx.needs_input_grad)
        if teacher is not None:
            teacher = teacher.contiguous()
            if tuple(teacher.shape) != (B, L):
                raise ValueError('teacher tokens must be (batch, seq_length)')
        steps = torch.empty(L, B, C, dtype=_f32, device=dev)             # logits by (step, trial)
        tokens = torch.empty(L, B, dtype=torch.int64, device=dev)
        tokens[0].fill_(int(start_token))
        hs = torch.empty(L + 2, B, H, dtype=_f32, device=dev)            # y_ext layout of a T = L sequence: slot s = h_{s-1}
        saved = torch.empty(1, L, B, 4 * H, dtype=_f32, device=dev) if save else None
        ctx.form = _launch_form(B, H)                                     # (L one-step forwards and one T = L backward share it)
        gi = torch.empty(B, 3 * H, dtype=_f32, device=dev)
        nbytes = _gru_ws_bytes('xps_gru_seq_fwd_f32_workspace', 1, B, H, 1)
        _gru_status_register(dev)
        w_arr, b_arr = _ptr_array([w_hh_c]), _ptr_array([b_hh_c])
        rc = rowmap(C)
        fused_select = C <= 16                          # logits + next token + its table row in one launch
        for s in range(L):
            if s == 0 or not fused_select:
                call('xps_gather_rows_f32', _ptr(table), _ptr(tokens[s]), _ptr(gi), B, 3 * H, ntok, _stream())
            ws = _ws(nbytes, dev)
            # one step on the window hs[s : s + 3]: slot 0 <- h0 (= hs[s] itself at s > 0), slot 1 <- h_s, slot 2 <- 0 (rewritten
            # by the next step)
            call('xps_gru_seq_fwd_f32', _ptr(gi), w_arr, b_arr, _ptr(h0c if s == 0 else hs[s]), _ptr(hs[s:]),
                 _ptr(saved[0, s]) if save else None, 1, B, H, 1, _ptr(ws), nbytes, _stream())
            tstride = teacher.stride(0) if teacher is not None else 0
            if fused_select:
                last = s + 1 == L
                call('xps_decoder_select_f32', _ptr(hs[s + 1]), _ptr(w_fc_c), _ptr(b_fc_c), _ptr(steps[s]),
                     _ptr(teacher[:, s]) if (teacher is not None and not last) else None, tstride,
                     _ptr(flags[s:s + 1]) if (teacher is not None and not last) else None, _ptr(table),
                     None if last else _ptr(tokens[s + 1]), None if last else _ptr(gi), B, H, C, ntok, _stream())
                continue
            gemm_nt(hs[s + 1], w_fc_c, steps[s], B, C, H, bias=b_fc_c, rc=rc)
            if s + 1 < L:
                call('xps_next_token', _ptr(steps[s]), C, _ptr(teacher[:, s]) if teacher is not None else None, tstride,
                     _ptr(flags[s:s + 1]) if teacher is not None else None, _ptr(tokens[s + 1]), B, _stream())
        logits = steps.permute(1, 0, 2).contiguous()
        if save:
            ctx.save_for_backward(tokens, hs, saved, w_hh_c, w_fc_c)
        ctx.params = (w_hh, b_hh, w_fc, b_fc)
        ctx.dims = (B, H, C, L, ntok)
        ctx.mark_non_differentiable(tokens)
        return logits, tokens

    @staticmethod
    def backward(ctx, dlogits, _dtok):
        tokens, hs, saved, w_hh_c, w_fc_c = ctx.saved_tensors
        B, H, C, L, ntok = ctx.dims
        dev = hs.device
        if dlogits is None:
            return (None,) * 10
        dlogits = dlogits.contiguous()
        # dy[s, b, :] = dlogits[b, s, :] W_fc for all steps at once (rows (s, b) of dlogits at b*L*C + s*C)
        dy = torch.empty(L, B, H, dtype=_f32, device=dev)
        gemm_nn(dlogits, w_fc_c, dy, L * B, H, C, ra=rowmap(L * C, rpg=B, gs=C))
        dgi, dghn, dh0 = _gru_backward(dy, None, hs, saved, [w_hh_c], L, B, H, 1, True, form=ctx.form)
        dtable, r_wh, r_bh, r_wf, r_bf = _decoder_weight_grads(dlogits, dgi[0], dghn[0], hs, tokens, ctx.params, B, H, C, L, ntok)
        return dtable, dh0[0], r_wh, r_bh, r_wf, r_bf, None, None, None, None


class GatherRowsFn(torch.autograd.Function):
    """out[b] = table[idx[b]] (nn.Embedding lookups / per-token input projections)."""

    @staticmethod
    def forward(ctx, table, idx):
        _need_gpu(table, idx)
        table = table.contiguous()
        idx = idx.contiguous()
        n_rows, cols = table.shape
        out = torch.empty(idx.shape[0], cols, dtype=_f32, device=table.device)
        call('xps_gather_rows_f32', _ptr(table), _ptr(idx), _ptr(out), idx.shape[0], cols, n_rows, _stream())
        ctx.save_for_backward(idx)
        ctx.shape = (n_rows, cols)
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        n_rows, cols = ctx.shape
        dout = dout.contiguous()
        dt = torch.empty(n_rows, cols, dtype=_f32, device=dout.device)
        nbytes = lib().xps_scatter_rows_f32_workspace(idx.shape[0], cols, n_rows)
        ws = _ws(nbytes, dout.device)
        call('xps_scatter_rows_f32', _ptr(dout), _ptr(idx), _ptr(dt), idx.shape[0], cols, n_rows, 0, _ptr(ws), nbytes,
             _stream())
        return dt, None


def gather_rows(table, idx):
    return GatherRowsFn.apply(table, idx)


def next_token(logits, teacher, use_teacher):
    """argmax (first max) or the teacher token, chosen by a DEVICE flag -> no host sync."""
    B, Cn = logits.shape
    nxt = torch.empty(B, dtype=torch.int64, device=logits.device)
    tstride = teacher.stride(0) if teacher is not None else 0
    call('xps_next_token', _ptr(logits.contiguous()), Cn, _ptr(teacher), tstride, _ptr(use_teacher), _ptr(nxt),
         B, _stream())
    return nxt


class MaskScaleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, scale):
        x = x.contiguous()
        out = torch.empty_like(x)
        call('xps_mask_scale_f32', _ptr(x), _ptr(mask), scale, _ptr(out), x.numel(), _stream())
        ctx.save_for_backward(mask)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, dout):
        (mask,) = ctx.saved_tensors
        dout = dout.contiguous()
        dx = torch.empty_like(dout)
        call('xps_mask_scale_f32', _ptr(dout), _ptr(mask), ctx.scale, _ptr(dx), dout.numel(), _stream())
        return dx, None, None


_DROP_COUNTER = [0]


def next_dropout_seed():
    """64-bit seed for one dropout site: drawn from torch's CPU generator on first use (so
    torch.manual_seed governs the run), then advanced by a fixed odd stride per call."""
    if _DROP_COUNTER[0] == 0:
        _DROP_COUNTER[0] = int(torch.randint(1, 2 ** 62, (1,)).item()) | 1
    _DROP_COUNTER[0] = (_DROP_COUNTER[0] + 0x9E3779B97F4A7C15) % (2 ** 64)
    return _DROP_COUNTER[0]


def dropout_mask(shape, p, device):
    """{0,1} float mask with P(0) = p from the in-kernel counter-based generator (one pass, no torch RNG
    kernels)."""
    mask = torch.empty(shape, dtype=_f32, device=device)
    call('xps_dropout_f32', None, None, _ptr(mask), mask.numel(), float(p), next_dropout_seed(), _stream())
    return mask


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        x = x.contiguous()
        out = torch.empty_like(x)
        # no mask tensor: the decisions are a pure function of (seed, element index); the backward pass regenerates
        # them with the same call on the incoming gradient (one pass less over a (T', B, 2H) tensor each way)
        ctx.seed, ctx.p = next_dropout_seed(), float(p)
        call('xps_dropout_f32', _ptr(x), _ptr(out), None, x.numel(), ctx.p, ctx.seed, _stream())
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        dx = torch.empty_like(dout)
        call('xps_dropout_f32', _ptr(dout), _ptr(dx), None, dout.numel(), ctx.p, ctx.seed, _stream())
        return dx, None


def dropout(x, p, training):
    """Inverted dropout, mask generation and multiply fused in one HIP pass."""
    if not training or p <= 0.0:
        return x
    return DropoutFn.apply(x, p)


_unit_grads = {}


def unit_gradient(device):
    """A resident scalar 1.0 on `device`: pass it to ``loss.backward(...)`` (autograd would otherwise launch a fill per step).
    CrossEntropyFn recognises it and returns the gradient it computed in the forward launch without another kernel."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    t = _unit_grads.get(key)
    if t is None:
        t = _unit_grads[key] = torch.ones((), dtype=_f32, device=device)
    return t


_ce_ws = {}


def _ce_workspace(rows, device, query='xps_cross_entropy_loss_grad_f32_workspace'):
    """Zero-initialised partial-sum / ticket buffer of the fused cross-entropy launch and of the one-launch classification
    step (`query`: the size query of the entry point), one per (device, stream): both kernels leave the ticket at zero, so
    the buffer is reused by every step."""
    nbytes = getattr(lib(), query)(rows)
    key = (device.index, _stream())
    t = _ce_ws.get(key)
    if t is None or t.numel() < nbytes:
        t = _ce_ws[key] = torch.zeros(max(int(nbytes), 4096), dtype=torch.uint8, device=device)
    return t, nbytes


class CrossEntropyFn(torch.autograd.Function):
    """mean CE over rows (nn.CrossEntropyLoss defaults), deterministic reduction; loss and gradient in ONE launch."""

    @staticmethod
    def forward(ctx, logits, target):
        _need_gpu(logits, target)
        logits = logits.contiguous()
        target = target.contiguous()
        rows, Cn = logits.shape
        row_loss = torch.empty(rows, dtype=_f32, device=logits.device)
        loss = torch.empty(1, dtype=_f32, device=logits.device)
        need = ctx.needs_input_grad[0]
        dl = torch.empty_like(logits) if need else None
        ws, nbytes = _ce_workspace(rows, logits.device)
        call('xps_cross_entropy_loss_grad_f32', _ptr(logits), _ptr(target), _ptr(row_loss), _ptr(loss), _ptr(dl), _ptr(ws),
             ws.numel(), rows, Cn, _stream())
        ctx.unit = dl
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        dl = ctx.unit
        key = (gout.device.type, gout.device.index)
        one = _unit_grads.get(key)
        if one is not None and gout.data_ptr() == one.data_ptr():
            return dl, None                              # d loss / d loss = the resident 1.0: nothing to scale
        return dl * gout.to(_f32), None


def cross_entropy(logits, target):
    return CrossEntropyFn.apply(logits, target)


class ClassifyLossAccFn(torch.autograd.Function):
    """The classification step of the single-label models in ONE launch: mean cross-entropy (the bits of CrossEntropyFn) with
    its gradient, the confusion matrix of argmax(logits) against the target, and accuracy = trace / rows.  Returns
    (loss, acc, cmat); only loss carries a gradient."""

    @staticmethod
    def forward(ctx, logits, target, num_classes):
        _need_gpu(logits, target)
        logits = logits.contiguous()
        target = target.contiguous()
        rows, Cn = logits.shape
        if Cn != num_classes:
            raise ValueError(f'classify_loss_acc: logits have {Cn} columns, num_classes = {num_classes}')
        if target.dtype != torch.int64 or target.shape != (rows,):
            raise ValueError('classify_loss_acc: target must be an int64 vector with one class per row')
        dev = logits.device
        row_loss = torch.empty(rows, dtype=_f32, device=dev)
        loss = torch.empty(1, dtype=_f32, device=dev)
        acc = torch.empty(1, dtype=_f32, device=dev)
        cmat = torch.empty(Cn, Cn, dtype=torch.int64, device=dev)        # zeroed by the kernel
        dl = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        ws, _ = _ce_workspace(rows, dev, 'xps_classify_loss_acc_f32_workspace')
        call('xps_classify_loss_acc_f32', _ptr(logits), _ptr(target), _ptr(row_loss), _ptr(loss), _ptr(dl), _ptr(cmat), _ptr(acc),
             _ptr(ws), ws.numel(), rows, Cn, _stream())
        ctx.unit = dl
        acc = acc.view(())
        ctx.mark_non_differentiable(acc, cmat)
        return loss.view(()), acc, cmat

    @staticmethod
    def backward(ctx, gout, _gacc, _gcmat):
        dl = ctx.unit
        key = (gout.device.type, gout.device.index)
        one = _unit_grads.get(key)
        if one is not None and gout.data_ptr() == one.data_ptr():
            return dl, None, None                        # d loss / d loss = the resident 1.0: nothing to scale
        return dl * gout.to(_f32), None, None


def classify_loss_acc(logits, target, num_classes):
    """(loss, acc, cmat) of (rows, num_classes) logits against int64 targets (rows,), one launch (ClassifyLossAccFn)."""
    return ClassifyLossAccFn.apply(logits, target, num_classes)


class TimeMaxFn(torch.autograd.Function):
    """Max over time of a time-major (T, B, F) tensor -> (B, F); torch.max(z, dim=0)'s values under its CPU tie / NaN rule
    (first maximum wins, a NaN counts as the maximum), and the int32 time index of each.  The saved index routes the gradient: the backward writes
    every element of dz once (no memset, no atomics)."""

    @staticmethod
    def forward(ctx, z):
        _need_gpu(z)
        if z.dim() != 3 or z.dtype != _f32:
            raise ValueError('time_max: expected a float32 (T, B, F) tensor')
        z = z.contiguous()
        T, B, F = z.shape
        if T < 1 or B < 1 or F < 1:
            raise ValueError('time_max: empty tensor')
        out = torch.empty(B, F, dtype=_f32, device=z.device)
        arg = torch.empty(B, F, dtype=torch.int32, device=z.device)
        call('xps_time_max_fwd_f32', _ptr(z), _ptr(out), _ptr(arg), T, B, F, _stream())
        ctx.save_for_backward(arg)
        ctx.T = T
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, dout, _darg):
        arg, = ctx.saved_tensors
        B, F = arg.shape
        dout = dout.contiguous()
        dz = torch.empty(ctx.T, B, F, dtype=_f32, device=dout.device)
        call('xps_time_max_bwd_f32', _ptr(dout), _ptr(arg), _ptr(dz), ctx.T, B, F, _stream())
        return dz


def time_max(z, return_indices=False):
    """max over the time axis of a time-major (T, B, F) tensor -> (B, F) (TimeMaxFn); return_indices: also the int32 time
    index of each maximum."""
    out, arg = TimeMaxFn.apply(z)
    return (out, arg) if return_indices else out


class CTCLossFn(torch.autograd.Function):
    """nn.CTCLoss(blank, reduction='mean', zero_infinity) on TIME-major raw scores (T, B, C): log-softmax, alpha,
    beta and the gradient with respect to the scores in one launch (xps_ctc_loss_f32)."""

    @staticmethod
    def forward(ctx, logits, targets, input_lengths, target_lengths, blank, zero_infinity):
        _need_gpu(logits)
        if targets.dim() != 2:
            raise ValueError('targets must be a padded (batch, max_target_length) tensor')
        logits = logits.contiguous()
        T, B, Cn = logits.shape
        dev = logits.device
        if not input_lengths.is_cuda and int(input_lengths.max()) > T:         # torch's own check (host lengths only)
            raise RuntimeError(f'Expected input_lengths to have value at most {T}, but got value '
                               f'{int(input_lengths.max())}')
        if not target_lengths.is_cuda and target_lengths.numel() and int(target_lengths.max()) > targets.shape[1]:
            raise RuntimeError(f'Expected tensor to have size at least {int(target_lengths.max())} at dimension 1, but '
                               f'got size {tuple(targets.shape)}')          # torch's own check (host lengths only)
        tg = targets.to(device=dev, dtype=torch.int64).contiguous()
        il = input_lengths.to(device=dev, dtype=torch.int64).contiguous()
        tl = target_lengths.to(device=dev, dtype=torch.int64).contiguous()
        Lmax = tg.shape[1]
        nll = torch.empty(B, dtype=_f32, device=dev)
        loss = torch.empty(1, dtype=_f32, device=dev)
        need = ctx.needs_input_grad[0]
        dl = torch.empty_like(logits) if need else None
        nbytes = lib().xps_ctc_loss_f32_workspace(T, B, Lmax)
        ws = _ws(nbytes, dev)
        call('xps_ctc_loss_f32', _ptr(logits), _ptr(tg), tg.stride(0), _ptr(il), _ptr(tl), T, B, Cn, Lmax, int(blank),
             int(bool(zero_infinity)), _ptr(nll), _ptr(loss), _ptr(dl), _ptr(ws), nbytes, _stream())
        if need:
            ctx.save_for_backward(dl)
        ctx.nll = nll
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        (dl,) = ctx.saved_tensors
        return dl * gout, None, None, None, None, None


def ctc_loss(logits_tm, targets, input_lengths, target_lengths, blank=0, zero_infinity=True):
    if not torch.is_grad_enabled():         # needs_input_grad ignores no_grad: detached, the kernel gets no gradient buffer
        logits_tm = logits_tm.detach()
    return CTCLossFn.apply(logits_tm, targets, input_lengths, target_lengths, blank, zero_infinity)


class WindowLinearFn(torch.autograd.Function):
    """Input projection of right-aligned sliding windows without materialising them: row (b, w) of the
    (B*nw, win*C) window matrix is the contiguous win*C floats at x[b, w*stride] (row map), the result is
    TIME-major (nw, B, N).  x is data (no gradient); dW / db = one grouped TN launch over the same row map."""

    @staticmethod
    def forward(ctx, x, w, b, win, stride):
        _need_gpu(x, w)
        x = x.contiguous()
        B, T, Cc = x.shape
        nw = (T - win) // stride + 1
        K = win * Cc
        wc = w.contiguous()
        N = wc.shape[0]
        if wc.shape[1] != K:
            raise ValueError(f'weight expects {wc.shape[1]} inputs, windows have win_size * channels = {K}')
        out = torch.empty(nw, B, N, dtype=_f32, device=x.device)
        gemm_nt(x, wc, out, nw * B, N, K, bias=b, ra=rowmap(stride * Cc, rpg=nw, gs=T * Cc),
                rc=rowmap(B * N, rpg=nw, gs=N))
        ctx.save_for_backward(x)
        ctx.params = (w, b)
        ctx.dims = (B, T, Cc, nw, K, N, stride)
        return out

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        w, b = ctx.params
        B, T, Cc, nw, K, N, stride = ctx.dims
        dev = x.device
        dout = dout.contiguous()
        if b is not None:
            dw, db, acc_w, rw, rb = _grad_targets(w, (N, K), b, (N,), dev)
        else:
            (dw, acc_w, rw), db, rb = _grad_target(w, (N, K), dev), None, None
        # contraction rows in (w, b) order: dout is plain, the window rows of x are groups of B rows per window
        gemm_tn_grouped([tn_problem(dout, x, dw, N, K, nw * B, ra=rowmap(N),
                                    rb=rowmap(T * Cc, rpg=B, gs=stride * Cc), colsum_out=db, accumulate=acc_w)], dev)
        return None, rw, rb, None, None


# --------------------------------------------------------------------------- #
# Transformer encoder layer                                    #
# --------------------------------------------------------------------------- #
ATTENTION_MAX_HEAD_DIM = 128
LAYER_NORM_MAX_WIDTH = 1024


def check_attention_shape(d_model, n_head):
    """ValueError outside the envelope of the attention kernels: n_head must divide d_model, head dimension <= 128."""
    if n_head < 1 or d_model < 1 or d_model % n_head != 0:
        raise ValueError(f'self_attention: n_head = {n_head} does not divide d_model = {d_model}')
    if d_model // n_head > ATTENTION_MAX_HEAD_DIM:
        raise ValueError(f'self_attention: head dimension {d_model // n_head} > {ATTENTION_MAX_HEAD_DIM} is outside the kernels\' '
                         'envelope (there is no fallback)')


class SelfAttentionFn(torch.autograd.Function):
    """Fused multi-head self-attention on the packed in-projection output, time-major rows (xps_attention_fwd_f32 / _bwd_f32)."""

    @staticmethod
    def forward(ctx, qkv, B, S, n_head, p, seed):
        _need_gpu(qkv)
        if qkv.dtype != _f32 or qkv.numel() == 0 or qkv.shape[-1] % 3 != 0:
            raise ValueError('self_attention: expected a float32 (S * B, 3 * d_model) tensor')
        D = qkv.shape[-1] // 3
        check_attention_shape(D, n_head)
        if B < 1 or S < 1 or qkv.numel() != S * B * 3 * D:
            raise ValueError(f'self_attention: {tuple(qkv.shape)} is not S * B = {S} * {B} rows of 3 * d_model')
        dh = D // n_head
        if not lib().xps_attention_supported(B, S, n_head, dh):
            raise ValueError(f'self_attention: shape B = {B}, S = {S}, heads = {n_head}, head dimension = {dh} is outside the '
                             'kernels\' envelope (there is no fallback)')
        qkv = qkv.contiguous()
        out = torch.empty(*qkv.shape[:-1], D, dtype=_f32, device=qkv.device)
        lse = torch.empty(B, n_head, S, dtype=_f32, device=qkv.device)
        call('xps_attention_fwd_f32', _ptr(qkv), _ptr(out), _ptr(lse), B, S, n_head, dh, float(p), int(seed), _stream())
        ctx.save_for_backward(qkv, out, lse)
        ctx.cfg = (B, S, n_head, dh, float(p), int(seed))
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        B, S, n_head, dh, p, seed = ctx.cfg
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        nbytes = _memo(('attn_bwd_ws', B, S, n_head, dh), lambda: lib().xps_attention_bwd_f32_workspace(B, S, n_head, dh))
        ws = _ws(nbytes, qkv.device)
        call('xps_attention_bwd_f32', _ptr(dout), _ptr(qkv), _ptr(out), _ptr(lse), _ptr(dqkv), B, S, n_head, dh, p, seed, _ptr(ws),
             nbytes, _stream())
        return dqkv, None, None, None, None, None


def self_attention(qkv, B, S, n_head, p=0.0, training=False):
    """Multi-head self-attention of S * B time-major rows (row s * B + b) of packed q | k | v, each d_model wide with head h at
    columns h * dh: softmax((q / sqrt(dh)) k^T) v per (trial, head), heads concatenated -> (S * B, d_model).  Dropout with
    rate p acts on the probabilities when training (one seed from next_dropout_seed, decision index
    ((b * n_head + head) * S + query) * S + key).  No attention or key-padding masks."""
    drop = bool(training and p > 0.0)
    return SelfAttentionFn.apply(qkv, int(B), int(S), int(n_head), float(p) if drop else 0.0, next_dropout_seed() if drop else 0)


class AddLayerNormFn(torch.autograd.Function):
    """y = LayerNorm(x + dropout(r)) * weight + bias (xps_add_layer_norm_fwd_f32 / _bwd_f32)."""

    @staticmethod
    def forward(ctx, x, r, weight, bias, eps, p, seed):
        _need_gpu(x, r, weight, bias)
        if x.shape != r.shape or x.dtype != _f32 or r.dtype != _f32:
            raise ValueError('add_layer_norm: x and r must be float32 tensors of one shape')
        D = x.shape[-1]
        if D < 1 or D > LAYER_NORM_MAX_WIDTH or x.numel() == 0:
            raise ValueError(f'add_layer_norm: width {D} is outside the kernel\'s envelope (1 .. {LAYER_NORM_MAX_WIDTH}; there is no '
                             'fallback)')
        if tuple(weight.shape) != (D,) or tuple(bias.shape) != (D,):
            raise ValueError('add_layer_norm: weight and bias must have the width of x')
        x, r = x.contiguous(), r.contiguous()
        w, bs = weight.contiguous(), bias.contiguous()
        rows = x.numel() // D
        y = torch.empty_like(x)
        mean = torch.empty(rows, dtype=_f32, device=x.device)
        rstd = torch.empty(rows, dtype=_f32, device=x.device)
        call('xps_add_layer_norm_fwd_f32', _ptr(x), _ptr(r), _ptr(w), _ptr(bs), _ptr(y), _ptr(mean), _ptr(rstd), rows, D, float(eps),
             float(p), int(seed), _stream())
        ctx.save_for_backward(x, r, w, mean, rstd)
        ctx.cfg = (rows, D, float(p), int(seed))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, r, w, mean, rstd = ctx.saved_tensors
        rows, D, p, seed = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dr = torch.empty_like(x) if p > 0.0 else dx          # without dropout both branches get the same gradient: one buffer
        dw = torch.empty(D, dtype=_f32, device=x.device)
        db = torch.empty(D, dtype=_f32, device=x.device)
        nbytes = _memo(('add_ln_bwd_ws', rows, D), lambda: lib().xps_add_layer_norm_bwd_f32_workspace(rows, D))
        ws = _ws(nbytes, x.device)
        call('xps_add_layer_norm_bwd_f32', _ptr(dy), _ptr(x), _ptr(r), _ptr(w), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dr), _ptr(dw),
             _ptr(db), rows, D, p, seed, _ptr(ws), nbytes, _stream())
        return dx, dr, dw, db, None, None, None


def add_layer_norm(x, r, weight, bias, eps=1e-5, p=0.0, training=False):
    """LayerNorm(x + dropout(r)) * weight + bias over the last axis (biased variance, nn.LayerNorm): the residual add, the
    dropout of the branch r (rate p when training; decision index = flat element index) and the normalisation in one kernel."""
    drop = bool(training and p > 0.0)
    return AddLayerNormFn.apply(x, r, weight, bias, float(eps), float(p) if drop else 0.0, next_dropout_seed() if drop else 0)


class ReluDropoutFn(torch.autograd.Function):
    """out = dropout(relu(x)) in one pass; the saved output is the backward's gate (xps_relu_dropout_fwd_f32 / _bwd_f32)."""

    @staticmethod
    def forward(ctx, x, p, seed):
        _need_gpu(x)
        x = x.contiguous()
        out = torch.empty_like(x)
        call('xps_relu_dropout_fwd_f32', _ptr(x), _ptr(out), x.numel(), float(p), int(seed), _stream())
        ctx.save_for_backward(out)
        ctx.p = float(p)
        return out

    @staticmethod
    def backward(ctx, dout):
        out, = ctx.saved_tensors
        dout = dout.contiguous()
        dx = torch.empty_like(out)
        call('xps_relu_dropout_bwd_f32', _ptr(dout), _ptr(out), _ptr(dx), out.numel(), ctx.p, _stream())
        return dx, None, None


def relu_dropout(x, p=0.0, training=False):
    """dropout(relu(x)) (the feed-forward block of the encoder layer), one seed from next_dropout_seed when training with p > 0."""
    drop = bool(training and p > 0.0)
    return ReluDropoutFn.apply(x, float(p) if drop else 0.0, next_dropout_seed() if drop else 0)


class AddPositionalFn(torch.autograd.Function):
    """z + table[s] written TIME-major (S, B, D); z is (S, B, D), or (B, S, D) with batch_major.  Backward: the identity."""

    @staticmethod
    def forward(ctx, z, table, batch_major):
        _need_gpu(z, table)
        if z.dim() != 3 or z.dtype != _f32 or z.numel() == 0:
            raise ValueError('add_positional: expected a non-empty float32 3-D tensor')
        B, S, D = (z.shape[0], z.shape[1], z.shape[2]) if batch_major else (z.shape[1], z.shape[0], z.shape[2])
        table = table.reshape(-1, table.shape[-1])
        if table.shape[1] != D or table.shape[0] < S or table.dtype != _f32:
            raise ValueError(f'add_positional: table {tuple(table.shape)} does not cover {S} steps of width {D}')
        z, table = z.contiguous(), table.contiguous()
        out = torch.empty(S, B, D, dtype=_f32, device=z.device)
        call('xps_add_positional_f32', _ptr(z), _ptr(table), _ptr(out), S, B, D, int(bool(batch_major)), _stream())
        ctx.batch_major = bool(batch_major)
        return out

    @staticmethod
    def backward(ctx, dout):
        return (dout.permute(1, 0, 2) if ctx.batch_major else dout), None, None


def add_positional(z, table, batch_major=False):
    """Time-major (S, B, D) sum of z and the first S rows of the (>= S, D) positional table (a leading axis of 1 is accepted);
    z is time-major (S, B, D), or batch-major (B, S, D) with batch_major=True (the transposition rides on the add)."""
    return AddPositionalFn.apply(z, table, batch_major)


class TimeMeanFn(torch.autograd.Function):
    """Mean over time of a time-major (T, B, F) tensor -> (B, F); the sibling of TimeMaxFn."""

    @staticmethod
    def forward(ctx, z):
        _need_gpu(z)
        if z.dim() != 3 or z.dtype != _f32:
            raise ValueError('time_mean: expected a float32 (T, B, F) tensor')
        z = z.contiguous()
        T, B, F = z.shape
        if T < 1 or B < 1 or F < 1:
            raise ValueError('time_mean: empty tensor')
        out = torch.empty(B, F, dtype=_f32, device=z.device)
        call('xps_time_mean_fwd_f32', _ptr(z), _ptr(out), T, B, F, _stream())
        ctx.T = T
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous()
        B, F = dout.shape
        dz = torch.empty(ctx.T, B, F, dtype=_f32, device=dout.device)
        call('xps_time_mean_bwd_f32', _ptr(dout), _ptr(dz), ctx.T, B, F, _stream())
        return dz


def time_mean(z):
    """mean over the time axis of a time-major (T, B, F) tensor -> (B, F) (TimeMeanFn)."""
    return TimeMeanFn.apply(z)


# --------------------------------------------------------------------------- #
# optimiser                                                                    #
# --------------------------------------------------------------------------- #
def grad_sumsq(flat_grad, out=None):
    out = out if out is not None else torch.empty(1, dtype=_f32, device=flat_grad.device)
    nbytes = lib().xps_sumsq_f32_workspace(flat_grad.numel())
    ws = _ws(nbytes, flat_grad.device)
    call('xps_sumsq_f32', _ptr(flat_grad), flat_grad.numel(), _ptr(out), _ptr(ws), nbytes, _stream())
    return out


def clip_adamw_step(p, g, m, v, sumsq, max_norm, lr, beta1, beta2, eps, weight_decay, step):
    """global-norm partials + fused clip / AdamW (the final fold of the norm happens inside the update kernel)."""
    nbytes = lib().xps_sumsq_f32_workspace(g.numel())
    ws = _ws(nbytes, g.device)
    call('xps_clip_adamw_f32', _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(sumsq), float(max_norm or 0.0),
         float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step), _ptr(ws), nbytes, _stream())


def adamw_step(p, g, m, v, sumsq, max_norm, lr, beta1, beta2, eps, weight_decay, step):
    call('xps_adamw_f32', _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(sumsq), float(max_norm or 0.0),
         float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), int(step), _stream())
