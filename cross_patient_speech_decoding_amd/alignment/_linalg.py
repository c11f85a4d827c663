"""Device linear algebra for the aligners, on top of the C ABI (include/xps.h).

Everything heavy — per-condition means, centred Gram / cross-covariance accumulation on the
f64 MFMA, Jacobi eigen/singular decompositions, batched transform apply — runs in libxps.so.
Host numpy only sorts / normalises / sign-fixes the small (d x d) results and builds index
lists; there is no CPU fallback for the kernels.
"""

import numpy as np
import torch

from .. import _switches
from .._dev import current_device, ptr, stream, workspace
from .._lib import call, lib

F64 = torch.float64
EPS = float(np.finfo(np.float64).eps)


def device():
    """The current device; raises where there is none (no CPU fallback)."""
    return current_device('cross_patient_speech_decoding_amd.alignment')


def to_device(x):
    """numpy / torch (float32 or float64; anything else -> float64) -> contiguous device tensor."""
    if isinstance(x, torch.Tensor):
        t = x
    else:
        x = np.asarray(x)
        if x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(F64)
    return t.to(device()).contiguous()


def like_input(out, X):
    """Transforms return what they were given: a DEVICE tensor for a device-resident input (no PCIe round trip: the next
    stage -- pooling, the DataModule, the model -- consumes it in HBM), otherwise the reference's float64 ndarray."""
    if isinstance(X, torch.Tensor) and X.is_cuda:
        return out
    return out.cpu().numpy()


def _is32(t):
    return int(t.dtype == torch.float32)


def _rows(t):
    """`t` as the kernels read a matrix: element (i, j) at data_ptr + i * stride(0) + j.  A row-strided view (a block of columns
    of a wider matrix) already is that and is passed as it is, with its stride(0) as the leading dimension; a view whose last
    stride is not 1 (a transpose, every second column) is copied."""
    return t if t.stride(-1) == 1 else t.contiguous()


def _vec(t):
    return None if t is None else t.contiguous()


# ------------------------------------------------------------------------------------ k1
def condition_index(keys):
    """Sorted unique string keys + CSR (order, start) of the trials of each condition, trials in
    original order inside a condition (numpy boolean-mask order)."""
    uniq, inv = np.unique(np.asarray(keys), return_inverse=True)
    order = np.argsort(inv, kind='stable').astype(np.int32)
    start = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(uniq)))]).astype(np.int32)
    return uniq, order, start


def cnd_avg_device(data_d, order, start):
    """data_d (N, ...) float32/float64 device tensor -> (n_cond, ...) float64 device tensor."""
    n_cond = len(start) - 1
    row_len = int(np.prod(data_d.shape[1:])) if data_d.dim() > 1 else 1
    out = torch.empty((n_cond,) + tuple(data_d.shape[1:]), dtype=F64, device=data_d.device)
    o = torch.from_numpy(order).to(data_d.device)
    s = torch.from_numpy(start).to(data_d.device)
    fn = 'xps_cnd_avg_f32' if data_d.dtype == torch.float32 else 'xps_cnd_avg_f64'
    call(fn, data_d.data_ptr(), o.data_ptr(), s.data_ptr(), out.data_ptr(), n_cond, row_len, stream())
    return out


# ------------------------------------------------------------------------------------ k2
def col_mean(X):
    """Column means (float64) of an (n, d) device matrix."""
    X = _rows(X)
    n, d = X.shape
    out = torch.empty(d, dtype=F64, device=X.device)
    nb = lib().xps_colsum_f64_workspace(n, d)
    ws = workspace(nb, device())
    call('xps_colsum_f64', X.data_ptr(), _is32(X), X.stride(0), n, d, out.data_ptr(), ws.data_ptr(), nb, stream())
    return out / n


def xcov(A, B=None, mean_a=None, mean_b=None):
    """(A - mean_a)^T (B - mean_b) in float64 on the f64 MFMA.  A (n, da), B (n, db) device."""
    B = A if B is None else B
    if B is A and mean_b is None:
        mean_b = mean_a
    Ar = _rows(A)
    A, B = Ar, (Ar if B is A else _rows(B))
    mean_a, mean_b = _vec(mean_a), _vec(mean_b)
    n, da = A.shape
    db = B.shape[1]
    C = torch.empty(da, db, dtype=F64, device=A.device)
    nb = lib().xps_xcov_f64_workspace(n, da, db)
    ws = workspace(nb, device())
    call('xps_xcov_f64', A.data_ptr(), _is32(A), A.stride(0), ptr(mean_a),
         B.data_ptr(), _is32(B), B.stride(0), ptr(mean_b),
         C.data_ptr(), db, n, da, db, ws.data_ptr(), nb, stream())
    return C


def dgemm(A, B, ta=False, tb=False):
    """op(A) @ op(B) for small float64 device matrices."""
    A, B = _rows(A), _rows(B)
    M = A.shape[1] if ta else A.shape[0]
    K = A.shape[0] if ta else A.shape[1]
    N = B.shape[0] if tb else B.shape[1]
    C = torch.empty(M, N, dtype=F64, device=A.device)
    if K >= 512 and ((M + 63) // 64) * ((N + 63) // 64) <= 64:
        # few output tiles, long contraction (the skinny products of the subspace iteration): split-K slabs + one reduce
        nb = lib().xps_dgemm_splitk_workspace(M, N, K)
        ws = workspace(nb, device())
        call('xps_dgemm_splitk', A.data_ptr(), A.stride(0), int(ta), B.data_ptr(), B.stride(0), int(tb), C.data_ptr(), N,
             M, N, K, ws.data_ptr(), nb, stream())
        return C
    call('xps_dgemm_small', A.data_ptr(), A.stride(0), int(ta), B.data_ptr(), B.stride(0), int(tb), C.data_ptr(), N,
         M, N, K, stream())
    return C


def cheb_filter(Cd, A, deg, c, e, sigma1):
    """Y_deg of the scaled Chebyshev recurrence on the block A (n x m) with the symmetric operator Cd -- `deg` products
    enqueued by ONE library call (xps_cheb_filter_f64: per product a split-K launch + a reduce that applies the three-term update)."""
    A, Cd = A.contiguous(), _rows(Cd)
    n, m = A.shape
    out = torch.empty_like(A)
    nb = lib().xps_cheb_filter_f64_workspace(n, m)
    ws = workspace(nb, device())
    call('xps_cheb_filter_f64', Cd.data_ptr(), Cd.stride(0), n, A.data_ptr(), m, int(deg), float(c), float(e), float(sigma1),
         out.data_ptr(), ws.data_ptr(), nb, stream())
    return out


def apply(X, W, mean=None, out_f32=False):
    """(X - mean) @ W over all rows of X (..., d_in) -> (..., d_out).  W float64 (d_in, d_out)."""
    W, mean = _rows(W), _vec(mean)
    X2 = _rows(X.reshape(-1, X.shape[-1]))
    n, d_in = X2.shape
    d_out = W.shape[1]
    Y = torch.empty(n, d_out, dtype=torch.float32 if out_f32 else F64, device=X.device)
    call('xps_apply_f64', X2.data_ptr(), _is32(X2), X2.stride(0), ptr(mean),
         W.data_ptr(), W.stride(0), Y.data_ptr(), int(out_f32), d_out, n, d_in, d_out, stream())
    return Y.view(*X.shape[:-1], d_out)


# ------------------------------------------------------------------------------------ k3 / k5
def _jacobi_tol(m_rows, n_cols):
    """Converged = every pair orthogonal to rounding level; the largest |cos| over n^2/2 pairs of length-m columns cannot
    be pushed below a few eps * sqrt(m), so the bound grows slowly with the size."""
    return max(1e-14, 4.0 * EPS * np.sqrt(max(m_rows, n_cols)) * np.log2(max(n_cols, 2)))


def _jacobi(Wc, n_cols, m_rows, max_sweeps=40, tol=None, want_v=True):
    """Wc: (n_cols, m_rows) float64 device tensor = column-major (m x n) matrix.  Rotates in place;
    returns V (n_cols x n_cols as rows = columns of V, i.e. V^T in row-major terms), or None when
    ``want_v`` is False (rotations not accumulated: half the work).

    Small problems (n <= 128 and the matrix within one workgroup's LDS) are decomposed by ONE launch that
    runs every sweep and the convergence test on the device; larger ones by one launch per round."""
    if tol is None:
        tol = _jacobi_tol(m_rows, n_cols)
    Vc = torch.empty(n_cols, n_cols, dtype=F64, device=Wc.device) if want_v else None
    if lib().xps_jacobi_small_supported(m_rows, n_cols, int(want_v)):
        call('xps_jacobi_small_f64', Wc.data_ptr(), Wc.stride(0), 0, ptr(Vc), n_cols, 0,
             m_rows, n_cols, 1, max_sweeps, tol, None, None, stream())
        return Vc
    if want_v:
        Vc.copy_(torch.eye(n_cols, dtype=F64, device=Wc.device))
    off = torch.zeros(1, dtype=F64, device=Wc.device)
    done = 0
    while done < max_sweeps:
        k = 5 if done == 0 else 1
        call('xps_jacobi_sweeps_f64', Wc.data_ptr(), Wc.stride(0), ptr(Vc), n_cols, m_rows,
             n_cols, k, off.data_ptr(), None, 0, stream())
        done += k
        if off.item() <= tol:
            break
    return Vc


def jacobi_batched(Wb, want_v=True, max_sweeps=40, tol=None):
    """Wb: (batch, n, m) float64 device tensor, each [b] a column-major m x n matrix; all decomposed by one
    launch (one workgroup per matrix).  Returns Vb (batch, n, n) or None."""
    batch, n, m = Wb.shape
    if tol is None:
        tol = _jacobi_tol(m, n)
    if not lib().xps_jacobi_small_supported(m, n, int(want_v)):
        raise ValueError(f'jacobi_batched: {m} x {n} does not fit the single-workgroup kernel')
    Vb = torch.empty(batch, n, n, dtype=F64, device=Wb.device) if want_v else None
    call('xps_jacobi_small_f64', Wb.data_ptr(), Wb.stride(1), Wb.stride(0), ptr(Vb), n,
         n * n, m, n, batch, max_sweeps, tol, None, None, stream())
    return Vb


RAGGED_GROUP = 4        # single sweeps enqueued blind between two downloads of `frozen`
_PACK_ALIGN = 64        # doubles: every packed matrix starts on a 512-byte boundary (the kernel's column loads start aligned)


def _packed_offsets(lengths):
    """Element offsets (and, last, the total) of buffers of `lengths` doubles packed one after another, each aligned."""
    offs = [0]
    for ln in lengths:
        offs.append(offs[-1] + -(-int(ln) // _PACK_ALIGN) * _PACK_ALIGN)
    return offs


def _jacobi_ragged_packed(buf, offs, shapes, max_sweeps=40, tol=None):
    """The driver of jacobi_ragged on matrices already inside the flat float64 device buffer `buf`: matrix b is column-major
    m x n with leading dimension ld at element offs[b], shapes[b] = (m, n, ld).  Rotates in place; returns the sweeps each
    matrix ran (int32 ndarray)."""
    batch = len(shapes)
    if batch == 0:
        return np.zeros(0, dtype=np.int32)
    w_off = np.asarray(offs, dtype=np.int64)
    ms, ns, lds = (np.asarray([sh[k] for sh in shapes], dtype=dt) for k, dt in ((0, np.int32), (1, np.int32), (2, np.int64)))
    tols = np.array([_jacobi_tol(m, n) for m, n in zip(ms, ns)] if tol is None else np.broadcast_to(tol, (batch,)),
                    dtype=np.float64)
    dev = buf.device
    tol_d = torch.from_numpy(tols).to(dev)
    off_d = torch.zeros(batch, dtype=F64, device=dev)
    state = torch.zeros(2, batch, dtype=torch.int32, device=dev)              # frozen | sweeps_done
    nb = int(lib().xps_jacobi_sweeps_batched_f64_workspace(batch))
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=dev)

    def sweeps(k):
        call('xps_jacobi_sweeps_batched_f64', buf.data_ptr(), buf.numel(), w_off.ctypes.data, lds.ctypes.data, ms.ctypes.data,
             ns.ctypes.data, batch, k, 1, tol_d.data_ptr(), off_d.data_ptr(), state[0].data_ptr(), state[1].data_ptr(),
             ws.data_ptr(), nb, stream())

    # _jacobi's schedule per matrix -- 5 sweeps, then 1 at a time, checked after every call -- with the checks on the device:
    # a matrix freezes at the sweep where _jacobi would have stopped it, and `frozen` comes down once per group of calls
    done = 0
    if max_sweeps > 0:
        sweeps(5)
        done = 5
    while done < max_sweeps:
        k = min(max(RAGGED_GROUP, 1), max_sweeps - done)
        for _ in range(k):
            sweeps(1)
        done += k
        if bool(state[0].cpu().numpy().all()):
            break
    return state[1].cpu().numpy()


def jacobi_ragged(mats, max_sweeps=40, tol=None):
    """One-sided Jacobi (no V) of a RAGGED batch: mats is a list of 2-D float64 device tensors, mats[b] of shape (n_b, m_b) a
    column-major m_b x n_b matrix with xps_jacobi_batched_supported(m_b, n_b).  The matrices are packed into one device
    buffer and every sweep covers the whole batch (one launch per block round); each matrix stops at the sweep where _jacobi
    would have stopped it alone, with the same bits.  The number of host synchronisations depends on the sweeps the slowest
    matrix needs, not on the batch.  ``tol``: None (per matrix, _jacobi's formula), a scalar or one value per matrix.
    Returns (rotated, sweeps_done): views into the packed buffer and an int32 ndarray."""
    for t in mats:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.dtype == F64):
            raise ValueError('jacobi_ragged: 2-D float64 device matrices are needed')
        if not lib().xps_jacobi_batched_supported(t.shape[1], t.shape[0]):
            raise ValueError(f'jacobi_ragged: {t.shape[1]} x {t.shape[0]} is not a shape of the block kernel')
    offs = _packed_offsets([t.numel() for t in mats])
    buf = torch.empty(int(offs[-1]), dtype=F64, device=device())
    views = [buf[o:o + t.numel()].view(t.shape) for o, t in zip(offs, mats)]
    for v, t in zip(views, mats):
        v.copy_(t)
    done = _jacobi_ragged_packed(buf, offs[:-1], [(t.shape[1], t.shape[0], t.shape[1]) for t in mats], max_sweeps, tol)
    return views, done


def chol_whiten_blocks(Gd, offs, scale, shift, LHS=None):
    """Upper-triangular whitening factors S_b = L_b^-T of the diagonal blocks A_b = scale * G_bb + shift * I = L_b L_b^T of the
    device matrix Gd (D x D), written into a block-diagonal D x D device matrix S (S^T blockdiag(A_b) S = I); A_b is also written
    over the diagonal blocks of ``LHS`` when given.  One launch when the blocks have one size.  Returns S, or None when a block is
    too large for the LDS-resident kernel or is not positive definite (the caller then takes the eigendecomposition route)."""
    D = Gd.shape[0]
    sizes = [int(offs[b + 1] - offs[b]) for b in range(len(offs) - 1)]
    if not all(lib().xps_chol_whiten_supported(n) for n in sizes):
        return None
    S = torch.zeros_like(Gd)
    info = torch.zeros(len(sizes), dtype=torch.int32, device=Gd.device)
    ld = Gd.stride(0)
    groups = [(0, len(sizes))] if len(set(sizes)) == 1 else [(b, 1) for b in range(len(sizes))]
    for b0, cnt in groups:
        n, o = sizes[b0], int(offs[b0])
        step = n * (ld + 1) * 8
        call('xps_chol_whiten_f64', Gd.data_ptr() + o * (ld + 1) * 8, ld, n * (ld + 1), float(scale), float(shift),
             None if LHS is None else LHS.data_ptr() + o * (LHS.stride(0) + 1) * 8, 0 if LHS is None else LHS.stride(0),
             0 if LHS is None else n * (LHS.stride(0) + 1), S.data_ptr() + o * (S.stride(0) + 1) * 8, S.stride(0),
             n * (S.stride(0) + 1), n, cnt, info.data_ptr() + 4 * b0, stream())
    if int(info.abs().max().item()) != 0:
        return None
    return S


def _svd_tail(W, V):
    """(U, s, Vt) from the rotated matrix of a one-sided Jacobi SVD, W (n, m) with row j = u_j * s_j, and the rotations V (n, n)
    with row j = v_j: the norms, a stable descending order, and U with zero columns where a singular value is zero."""
    s = np.linalg.norm(W, axis=1)
    order = np.argsort(-s, kind='stable')
    s, W, V = s[order], W[order], V[order]
    U = np.zeros_like(W)
    nz = s > 0
    U[nz] = W[nz] / s[nz, None]
    return U.T, s, V


def svd(A):
    """Thin SVD of a small float64 device matrix by one-sided Jacobi: A = U diag(s) Vt, s descending.
    Returns numpy (U, s, Vt)."""
    A = A.to(F64)
    m, n = A.shape
    if m < n:
        U, s, Vt = svd(A.t().contiguous())
        return Vt.T, s, U.T
    Wc = A.t().contiguous().clone()                 # row j = column j of A
    Vc = _jacobi(Wc, n, m)
    return _svd_tail(Wc.cpu().numpy(), Vc.cpu().numpy())


# Eigenvectors without accumulated rotations.  After the one-sided Jacobi W = C V = V diag(w), so for a
# positive-definite C the eigenvectors are the normalised columns of W (half the work, and for n = 128 the
# whole problem then fits one workgroup's LDS).  The direction of column j carries a relative error of about
# eps * w_max / w_j, so every PSD matrix is first shifted by sigma = 2^-10 * (Gershgorin bound of w_max):
# same eigenvectors, spectrum within a factor 2^10 -> direction error <= ~2e-13, and the eigenvalues w - sigma
# keep the absolute accuracy eps * w_max of a LAPACK eigensolver (the reference's numpy / sklearn calls).
_SHIFT = 2.0 ** -10


def _eig_from_w(W, sigma):
    w = np.linalg.norm(W, axis=1)
    if len(w) == 0 or not np.all(w > 0.5 * _SHIFT * w.max()):
        return None
    order = np.argsort(-w, kind='stable')
    return np.maximum(w[order] - sigma, 0.0), (W[order] / w[order, None]).T


def _shift_of(C):
    g = float(C.abs().sum(dim=-1).max().item())
    return g * _SHIFT if g > 0 else 1.0


def eigh_psd(C, well_conditioned=False):
    """Eigendecomposition of a symmetric PSD float64 device matrix (Jacobi): returns numpy
    (w descending, V with eigenvectors in columns).  ``well_conditioned``: the caller guarantees a spectrum
    bounded away from zero (regularised / already shifted matrices): no extra shift is applied."""
    C = C.to(F64)
    n = C.shape[0]
    sigma = 0.0 if well_conditioned else _shift_of(C)
    Wc = C.contiguous().clone()
    if sigma:
        Wc.diagonal().add_(sigma)
    _jacobi(Wc, n, n, want_v=False)
    res = _eig_from_w(Wc.cpu().numpy(), sigma)
    if res is not None:
        return res
    if well_conditioned:                             # the caller's promise did not hold: shift after all
        return eigh_psd(C, False)
    Wc = C.contiguous().clone()                      # not PSD (negative eigenvalue beyond the shift): accumulate V
    Vc = _jacobi(Wc, n, n)
    W = Wc.cpu().numpy()
    V = Vc.cpu().numpy()
    w = np.linalg.norm(W, axis=1)
    order = np.argsort(-w, kind='stable')
    return w[order], V[order].T


def _shifted_stack(Cs, well_conditioned):
    """(Wb, sig): the (batch, n, n) device stack C + sigma I of a batch and its shifts.  An ndarray stack is shifted on the host
    and uploaded once; a list (device tensors allowed) is stacked and shifted on the device."""
    if isinstance(Cs, np.ndarray):
        g = np.abs(Cs).sum(axis=-1).max(axis=-1)
        sig = np.zeros(len(Cs)) if well_conditioned else np.where(g > 0, g * _SHIFT, 1.0)
        return to_device(Cs + sig[:, None, None] * np.eye(Cs.shape[-1])), sig
    Wb = torch.stack([to_device(c).to(F64) for c in Cs]).contiguous()
    sig = [0.0 if well_conditioned else _shift_of(W) for W in Wb]
    for W, sg in zip(Wb, sig):
        if sg:
            W.diagonal().add_(sg)
    return Wb, sig


def route_sizes(sizes, small_ok, ragged_ok):
    """Where eigh_psd_batched sends square matrices of the orders `sizes` (pure numpy: no device): ``(small, ragged, alone)``
    with `small` a dict order -> indices for one jacobi_batched launch each (orders with small_ok(n)), `ragged` the indices
    of the ONE jacobi_ragged call (ragged_ok(n)) and `alone` the indices that eigh_psd takes one at a time.  Indices ascend."""
    small, ragged, alone = {}, [], []
    for i, n in enumerate(sizes):
        if small_ok(int(n)):
            small.setdefault(int(n), []).append(i)
        elif ragged_ok(int(n)):
            ragged.append(i)
        else:
            alone.append(i)
    return small, ragged, alone


def _shifts_of(mats, well_conditioned):
    """_shift_of of every device matrix of `mats` -- the same torch expression per matrix, so the same bits -- with ONE
    download for all of them."""
    if well_conditioned or not mats:
        return [0.0] * len(mats)
    g = torch.stack([C.abs().sum(dim=-1).max() for C in mats]).cpu().numpy()
    return [float(x) * _SHIFT if float(x) > 0 else 1.0 for x in g]


def _small_stack(Cs, idx, well_conditioned):
    """(Wb, sig) of the matrices Cs[i], i in idx -- one size of the one-workgroup kernel.  ndarrays, in a stack or in a list,
    are shifted on the host as an ndarray stack is (one rule, whether or not the batch has other sizes in it); a list of one
    shape that holds device matrices as _shifted_stack shifts it; device matrices out of a list of mixed sizes as eigh_psd
    shifts each of them alone."""
    if all(isinstance(Cs[i], np.ndarray) for i in idx):
        return _shifted_stack(np.stack([np.asarray(Cs[i], dtype=np.float64) for i in idx]), well_conditioned)
    if len(idx) == len(Cs):
        return _shifted_stack(Cs, well_conditioned)
    mats = [to_device(Cs[i]).to(F64) for i in idx]
    sig = _shifts_of(mats, well_conditioned)
    Wb = torch.stack(mats).contiguous()
    for W, sg in zip(Wb, sig):
        if sg:
            W.diagonal().add_(sg)
    return Wb, sig


def _eigh_ragged(Cs, idx, well_conditioned):
    """_eig_from_w results (None where rejected) of the matrices Cs[i], i in idx, through ONE jacobi_ragged call.  Every
    matrix is what eigh_psd would have worked on, bit for bit: its shift is eigh_psd's torch expression evaluated per matrix
    on the device; the scalars of the whole batch come down in one download."""
    ns = [int(Cs[i].shape[0]) for i in idx]
    offs = _packed_offsets([n * n for n in ns])
    if isinstance(Cs, np.ndarray) or all(isinstance(Cs[i], np.ndarray) for i in idx):
        host = np.zeros(int(offs[-1]))
        for o, n, i in zip(offs, ns, idx):
            host[o:o + n * n] = np.asarray(Cs[i], dtype=np.float64).reshape(-1)
        buf = to_device(host)                                              # one upload
        views = [buf[o:o + n * n].view(n, n) for o, n in zip(offs, ns)]
        seen = views
    else:
        buf = torch.empty(int(offs[-1]), dtype=F64, device=device())
        views = [buf[o:o + n * n].view(n, n) for o, n in zip(offs, ns)]
        seen = [to_device(Cs[i]).to(F64) for i in idx]                     # what eigh_psd takes its shift from
        for v, c in zip(views, seen):
            v.copy_(c)
    sig = _shifts_of(seen, well_conditioned)
    for v, sg in zip(views, sig):
        if sg:
            v.diagonal().add_(sg)
    _jacobi_ragged_packed(buf, offs[:-1], [(n, n, n) for n in ns])
    host = buf.cpu().numpy()
    return [_eig_from_w(host[o:o + n * n].reshape(n, n), sg) for o, n, sg in zip(offs, ns, sig)]


def eigh_psd_batched(Cs, well_conditioned=False, one_at_a_time=False):
    """eigh_psd of a batch of PSD matrices of any mix of sizes: a list of (w descending, V) in input order.  Cs is a
    (batch, n, n) float64 ndarray or a list of matrices (ndarrays or device tensors).  Sizes of the one-workgroup kernel take
    ONE jacobi_batched launch and one download per distinct size; sizes of the block kernel (up to 1024) take ONE jacobi_ragged
    call together -- a fixed number of host synchronisations, whatever the batch; anything larger goes through eigh_psd.  A
    matrix that is not PSD beyond its shift falls back to eigh_psd on its own.  ``one_at_a_time``: every matrix beyond the
    one-workgroup kernel goes through eigh_psd instead; the results are the same bit for bit."""
    if isinstance(Cs, np.ndarray):
        Cs = np.ascontiguousarray(Cs, dtype=np.float64)
    L = lib()
    small, ragged, _ = route_sizes([c.shape[0] for c in Cs], lambda n: bool(L.xps_jacobi_small_supported(n, n, 0)),
                                   lambda n: not one_at_a_time and bool(L.xps_jacobi_batched_supported(n, n)))
    res = [None] * len(Cs)
    for idx in small.values():
        Wb, sig = _small_stack(Cs, idx, well_conditioned)
        jacobi_batched(Wb, want_v=False)
        for i, W, sg in zip(idx, Wb.cpu().numpy(), sig):
            res[i] = _eig_from_w(W, sg)
    if ragged:
        for i, r in zip(ragged, _eigh_ragged(Cs, ragged, well_conditioned)):
            res[i] = r
    return [r if r is not None else eigh_psd(to_device(Cs[i]), well_conditioned) for i, r in enumerate(res)]


def _eigh_sym_top_full(C, k):
    """All eigenpairs by one-sided Jacobi on the shifted matrix, the first k returned (small n, or k close to n)."""
    n = C.shape[0]
    mu = float(C.abs().sum(dim=1).max().item())
    Cs = C + (2.0 * mu) * torch.eye(n, dtype=F64, device=C.device)
    w, V = eigh_psd(Cs, well_conditioned=True)
    return (w - 2.0 * mu)[:k], V[:, :k]


_SUBSPACE_START = {}


def _subspace_start(n, m, dev):
    """Deterministic full-rank start block (the same for every call of a shape: fits are reproducible run to run)."""
    key = (n, m, str(dev))
    if key not in _SUBSPACE_START:
        if len(_SUBSPACE_START) > 16:
            _SUBSPACE_START.clear()
        _SUBSPACE_START[key] = torch.from_numpy(np.random.default_rng(20240229).standard_normal((n, m))).to(dev)
    return _SUBSPACE_START[key]


def _lanczos_bounds(C, steps=24):
    """(lo, hi) enclosing the spectrum of the symmetric device matrix C from `steps` Lanczos steps (no
    reorthogonalisation: only the two extreme Ritz values are used): extreme Ritz value -/+ its residual bound
    |beta_j s_j|, widened by 2 % of the width.  The recurrence runs on the device without synchronising; the
    steps x steps tridiagonal matrix is diagonalised by the small device Jacobi."""
    C = _rows(C)
    n = C.shape[0]
    steps = min(steps, n)
    dev = C.device
    v = torch.sin(0.7 * torch.arange(1, n + 1, dtype=F64, device=dev)) + 0.01      # (xps_lanczos_f64 starts from v / ||v||)
    ab_d = torch.empty(2 * steps, dtype=F64, device=dev)
    nb = lib().xps_lanczos_f64_workspace(n)
    ws = workspace(nb, device())
    # (the whole recurrence is enqueued by one library call: 2 launches per step; the Python loop paid ~10 launches per step)
    call('xps_lanczos_f64', C.data_ptr(), C.stride(0), n, steps, v.data_ptr(), ab_d.data_ptr(), ab_d.data_ptr() + 8 * steps,
         ws.data_ptr(), nb, stream())
    ab = ab_d.cpu().numpy()
    a, b = ab[:steps], ab[steps:]
    if not np.isfinite(ab).all():
        return None
    T = np.diag(a) + np.diag(b[:-1], 1) + np.diag(b[:-1], -1)
    shift = float(np.abs(T).sum(axis=1).max()) * 1.5 + 1e-300           # Gershgorin: T + shift I is positive definite
    th, S = eigh_psd(to_device(T + shift * np.eye(steps)), well_conditioned=True)
    th = th - shift                                                      # descending
    hi = th[0] + abs(b[-1] * S[-1, 0])
    lo = th[-1] - abs(b[-1] * S[-1, -1])
    pad = 0.02 * (hi - lo)
    return lo - pad, hi + pad


def _orthonormal_columns_cholqr3(Y):
    """Orthonormal basis of the column span of Y (n x m, m << n) by SHIFTED CHOLESKY QR in three passes (Fukaya, Kannan,
    Nakatsukasa, Yamamoto, Yanagisawa 2020) on the column-normalised block: pass 1 factors G + s I with
    s = 11 (n m + m (m + 1)) eps ||G|| (a factor exists whatever the condition number; it brings the block to a condition of
    ~sqrt(1 / eps) at worst), passes 2 and 3 are plain Cholesky QR.  Per pass: Gram matrix and the triangular solve as f64 MFMA
    products on the device, the m x m (<= 48 x 48) factor on the host.  ~0.4 ms against ~1.3 ms for the one-sided Jacobi on the
    tall block (three workgroups busy).  None when a factorisation fails or the result is not orthonormal (-> the Jacobi route)."""
    n, m = Y.shape
    s = torch.linalg.vector_norm(Y, dim=0)
    smin, smax = (float(x) for x in torch.stack([s.min(), s.max()]).cpu())
    if not np.isfinite(smax) or smin <= 0.0:
        return None
    A = (Y / s).contiguous()
    for p in range(3):
        G = dgemm(A, A, ta=True).cpu().numpy()
        G = 0.5 * (G + G.T)
        if not np.isfinite(G).all():
            return None
        if p == 0:
            G = G + (11.0 * (n * m + m * (m + 1)) * EPS * float(np.linalg.norm(G, 2))) * np.eye(m)
        try:
            Linv = np.linalg.inv(np.linalg.cholesky(G))
        except np.linalg.LinAlgError:
            return None
        A = dgemm(A, to_device(np.ascontiguousarray(Linv.T)))
    G = dgemm(A, A, ta=True).cpu().numpy()
    if not np.isfinite(G).all() or np.abs(G - np.eye(m)).max() > 1e-12:
        return None
    return A


def _orthonormal_columns(Y):
    """Orthonormal basis of the column span of Y (n x m device matrix, m << n).  Shifted Cholesky QR (above) where it
    succeeds; else -- and always with XPS_TOPK_ORTHO=jacobi -- one-sided Jacobi on Y itself (no Gram matrix: a filtered block
    whose columns differ in size by 1e7 keeps its small directions).  None if rank was lost."""
    if _switches.get('XPS_TOPK_ORTHO') != 'jacobi':
        Q = _orthonormal_columns_cholqr3(Y)
        if Q is not None:
            return Q
    Wt = Y.t().contiguous()
    m, n = Wt.shape
    _jacobi(Wt, m, n, want_v=False)
    s = torch.linalg.vector_norm(Wt, dim=1)
    smin, smax = (float(x) for x in torch.stack([s.min(), s.max()]).cpu())
    if not np.isfinite(smax) or smin <= smax * 1e-13:
        return None
    return (Wt / s[:, None]).t().contiguous()


def _reorthonormalise(A):
    """Orthonormal basis of the span of an ALREADY nearly orthonormal block (the purge of the locked directions moved it by
    rounding errors only): Cholesky QR -- Gram matrix on the device (f64 MFMA), its 45 x 45 Cholesky factor on the host, one
    product -- instead of a second one-sided Jacobi on the tall block (~1 ms each).  The Gram matrix of such a block is
    within rounding of the identity, so squaring the condition number costs nothing; anything else takes the robust route."""
    G = dgemm(A, A, ta=True).cpu().numpy()
    G = 0.5 * (G + G.T)
    if not np.isfinite(G).all() or np.abs(G - np.eye(G.shape[0])).max() > 1e-3:
        return _orthonormal_columns(A)
    Linv = np.linalg.inv(np.linalg.cholesky(G))                    # G = L L^T  ->  A L^-T is orthonormal
    return dgemm(A, to_device(np.ascontiguousarray(Linv.T)))


def eigh_sym_top(C, k, tol=2e-14, max_outer=40, max_degree=40, stats=None):
    """Top-k (algebraically largest) eigenpairs of a symmetric, possibly indefinite, float64 device matrix:
    numpy (w descending, V with eigenvectors in columns).

    The MCCA fit (AlignMCCA.py) needs n_components (10-30) of D = 512-1024 pairs; a full Jacobi diagonalisation
    spends its time on the D - k pairs nobody reads (76 of the 130 ms of an 8-view fit).  Here: Chebyshev-filtered
    subspace iteration with locking on a block of m = k + buffer vectors.  Per outer step the active block is
    multiplied `degree` times by the (deflated) matrix -- f64 MFMA GEMMs; the three-term recurrence damps the interval
    [lower spectrum bound, smallest Ritz value of the block] and is scaled so that the largest active Ritz value maps
    to 1 (Zhou & Saad) -- then orthonormalised (one-sided Jacobi on the tall block) and Rayleigh-Ritz-projected (small
    device Jacobi).  Leading pairs whose residual ||C v - theta v|| <= tol * ||C|| are locked: they leave the block
    and the operator moves their eigenvalues to the lower bound (C - L (Theta - lo) L^T), so that a well separated
    group of large eigenvalues (the shared latents of MCCA: 15 against a bulk below 2.1) does not cap the degree that
    the pairs inside the bulk need.  The degree adapts to an amplification of <= 2e7 per outer step across the block.
    Small problems (n <= 640) and wide requests (block over 128 columns or over n / 3) take the full decomposition,
    and so does any run that loses rank or does not converge.  ``stats``: receives iteration counts."""
    C = C.to(F64).contiguous()
    n = C.shape[0]
    k = min(k, n)
    m = k + max(8, (k + 1) // 2)
    # the full Jacobi costs ~73 ms x (n / 1024)^3, the subspace iteration 9-35 ms almost independent of n: worth it above ~640
    if n <= 640 or m > 128 or 3 * m > n or not lib().xps_jacobi_small_supported(m, m, 0):
        return _eigh_sym_top_full(C, k)
    dev = C.device
    bounds = _lanczos_bounds(C)
    if bounds is None or not bounds[1] > bounds[0]:
        return _eigh_sym_top_full(C, k)
    lo, hi = bounds
    scale = max(abs(lo), abs(hi))
    L, tl = None, np.zeros(0)                          # locked vectors (n x l device) and their eigenvalues
    Cd = C                                             # deflated operator C - L (Theta - lo) L^T, rebuilt when pairs lock

    def op(X):
        return dgemm(Cd, X)

    def purge(X):                                      # remove what rounding re-introduced of the locked directions
        return X if L is None else X - dgemm(L, dgemm(L, X, ta=True))

    A = _orthonormal_columns(op(op(_subspace_start(n, m, dev))))
    theta, nprod = None, 2
    for outer in range(max_outer):
        if A is None:
            break
        if theta is not None:
            b = float(theta[-1])
            e, c = 0.5 * (b - lo), 0.5 * (b + lo)
            xtop = (float(theta[0]) - c) / e
            if not (e > 0 and xtop > 1.0):
                break
            deg = int(np.log(2e7) / np.arccosh(xtop))
            deg = max(2, min(max_degree, deg))
            sigma1 = e / (float(theta[0]) - c)
            Y = cheb_filter(Cd, A, deg, c, e, sigma1)       # (the whole recurrence: one library call, 2 launches per product)
            nprod += deg
            if outer > 12 or nprod > 260:              # a spectrum this method is not made for: stop paying for it
                break
            A = _orthonormal_columns(purge(Y))
            if A is None:
                break
            if L is not None:
                A = _reorthonormalise(purge(A))
                if A is None:
                    break
        # Rayleigh-Ritz of the (deflated) operator on the active block; H + shift is positive definite
        CA = op(A)
        nprod += 1
        Hm = dgemm(A, CA, ta=True)
        shift = (hi - lo) - lo
        w, Z = eigh_psd(0.5 * (Hm + Hm.t()) + shift * torch.eye(A.shape[1], dtype=F64, device=dev), well_conditioned=True)
        theta = w - shift
        Zd = to_device(np.ascontiguousarray(Z))
        A = dgemm(A, Zd)
        R = dgemm(CA, Zd) - A * torch.from_numpy(theta).to(dev)
        res = torch.linalg.vector_norm(R, dim=0).cpu().numpy()
        if theta[-1] < lo:                             # the lower bound was not one: widen it (the filter stays safe)
            lo = float(theta[-1]) - 0.05 * (hi - lo)
        have = 0 if L is None else L.shape[1]
        nl = 0
        while nl < len(theta) and have + nl < k and res[nl] <= tol * scale:
            nl += 1
        if stats is not None:
            stats.update(outer=outer + 1, products=nprod, locked=have + nl)
        if nl:
            Ln = A[:, :nl].contiguous()
            Cd = Cd - dgemm(Ln * torch.from_numpy(theta[:nl] - lo).to(dev), Ln, tb=True)
            L = Ln if L is None else torch.cat([L, Ln], dim=1).contiguous()
            tl = np.concatenate([tl, theta[:nl]])
            A, theta = A[:, nl:].contiguous(), theta[nl:]
        if L is not None and L.shape[1] >= k:
            order = np.argsort(-tl, kind='stable')     # (locking is in Ritz order; equal within rounding at worst)
            return tl[order][:k], L.cpu().numpy()[:, order][:, :k]
        if A.shape[1] < 2:
            break
    if stats is not None:
        stats['fallback'] = True
    return _eigh_sym_top_full(C, k)                    # rank loss / no convergence: the safe path


def svd_tall_device(A, mean=None):
    """Thin SVD of a tall (n x d, n >= d) device matrix by one-sided Jacobi ON THE MATRIX ITSELF (no Gram matrix: singular
    values keep their relative accuracy, so the numerical rank can follow LAPACK's rule and ill-conditioned data do not lose
    half their digits).  ``mean``: column means subtracted first (apply kernel).  Returns (Wt, s, V): Wt (d x n) device
    tensor whose row j is u_j * s_j, s (numpy, descending) and V (numpy, columns = right singular vectors), rows / columns
    in the same (descending) order."""
    A = A if A.dim() == 2 else A.reshape(-1, A.shape[-1])
    n, d = A.shape
    eye = torch.eye(d, dtype=F64, device=A.device)
    Ac = apply(A, eye, mean)                          # centred float64 copy: (A - mean) I on the apply kernel
    Wt = Ac.t().contiguous()                          # row j = column j
    Vc = _jacobi(Wt, d, n)
    s = torch.linalg.vector_norm(Wt, dim=1).cpu().numpy()
    order = np.argsort(-s, kind='stable')
    idx = torch.as_tensor(order, device=A.device)
    return Wt[idx].contiguous(), s[order], Vc.cpu().numpy()[order].T


def rank_from_singular_values(s, shape):
    """numpy.linalg.matrix_rank semantics (the reference's AlignCCA.py:263-264): s > s_max * max(shape) * eps."""
    if len(s) == 0 or s[0] <= 0:
        return 0
    return int((s > s[0] * max(shape) * EPS).sum())


def rank_from_gram_eigs(w, n_rows):
    """Numerical rank of an (n_rows x d) matrix from the eigenvalues of its Gram matrix.

    LAPACK's matrix_rank (used by the reference, AlignCCA.py:263-264) thresholds singular values
    at s_max * max(shape) * eps.  A Gram-based method cannot resolve singular values below
    sqrt(eps)-ish of s_max, so the threshold here is on the eigenvalues: w > w_max * max(shape) *
    eps (i.e. s > s_max * sqrt(max(shape) * eps)).  The two rules agree unless the condition number
    of the data lies between ~1e5 and ~1e10 (documented in DESIGN.md)."""
    if len(w) == 0 or w[0] <= 0:
        return 0
    tol = w[0] * max(n_rows, len(w)) * EPS
    return int((w > tol).sum())


def pinv_small(M):
    """numpy.linalg.pinv semantics (rcond = 1e-15 on singular values) through the Jacobi SVD."""
    U, s, Vt = svd(to_device(M))
    cutoff = 1e-15 * (s.max() if len(s) else 0.0)
    inv = np.where(s > cutoff, 1.0 / np.where(s > cutoff, s, 1.0), 0.0)
    return dgemm(to_device(Vt.T * inv), to_device(U), tb=True).cpu().numpy()


# ------------------------------------------------------------------------------------ fold-batched tables
# The grouped kernels (csrc/xps_fold_align.hip) read device tables of int64 words and trust them: every extent is checked
# here, against the tensors themselves, before a table is uploaded.
XCOV_WORDS, APPLY_WORDS, CNDAVG_WORDS, GRAM_WORDS = 20, 12, 8, 8  # XPS_*_WORDS of include/xps.h
XCOV_SPLIT_ROWS, XCOV_MAX_SPLITS = 256, 64


def xcov_grouped_splits(rows):
    """K splits of a grouped cross-moment problem of `rows` rows: one per 256 rows, at most 64 (so more than 256 rows take
    the split-K route).  A function of the problem's own shape alone: a problem gives the same bits in any table."""
    return int(max(1, min(XCOV_MAX_SPLITS, -(-int(rows) // XCOV_SPLIT_ROWS))))


def _tile_table(counts):
    """The int32 table of a grouped launch, one row {problem, mt, nt[, split]} per workgroup.  counts[i]: problem i's numbers of
    row tiles, column tiles [and splits].  Problems in order; within a problem the last index runs fastest."""
    counts = np.asarray(counts, dtype=np.int64)
    per = counts.prod(axis=1)
    rest = np.arange(per.sum()) - np.repeat(np.cumsum(per) - per, per)       # position of a workgroup inside its problem
    cols = []
    for c in np.repeat(counts, per, axis=0).T[::-1]:
        cols.append(rest % c)
        rest = rest // c
    return np.ascontiguousarray(np.stack([np.repeat(np.arange(len(per)), per)] + cols[::-1], axis=1), dtype=np.int32)


def _check_matrix(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 2 and t.dtype in (torch.float32, F64)
            and (t.shape[1] == 1 or t.stride(1) == 1) and t.stride(0) >= t.shape[1]):
        raise ValueError(f'{what}: a 2-D float32 / float64 device matrix with contiguous rows is needed')


def _check_vector(v, n, what):
    if v is None:
        return 0
    if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == F64 and v.dim() == 1 and v.is_contiguous()
            and v.shape[0] == n):
        raise ValueError(f'{what}: a contiguous float64 device vector of {n} elements is needed')
    return v.data_ptr()


def xcov_grouped(problems):
    """problems: list of (A, B, blk_a, blk_b, blk_len, c_a, c_b): A (n_a, da) and B (n_b, db) device matrices (float32 or
    float64), blk_a / blk_b integer sequences of equal length (first row of each block), c_a / c_b float64 device vectors or
    None.  One xps_xcov_grouped_f64 call.  Returns (out, offsets): `out` a flat float64 device tensor, problem i at
    out[offsets[i]:offsets[i + 1]] as [C (da x db) | s_a | s_b | count]."""
    dev = device()
    n = len(problems)
    tab = np.zeros((n, XCOV_WORDS), dtype=np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    blks, tiles, nblk_tot, slab_tot = [], [], 0, 0
    for i, (A, B, ba, bb, blk_len, ca, cb) in enumerate(problems):
        _check_matrix(A, 'xcov_grouped A')
        _check_matrix(B, 'xcov_grouped B')
        ba, bb = np.asarray(ba, dtype=np.int64).reshape(-1), np.asarray(bb, dtype=np.int64).reshape(-1)
        blk_len = int(blk_len)
        if len(ba) != len(bb) or blk_len < 1:
            raise ValueError('xcov_grouped: the two block lists differ in length, or blk_len < 1')
        if len(ba) and (ba.min() < 0 or bb.min() < 0 or ba.max() + blk_len > A.shape[0] or bb.max() + blk_len > B.shape[0]):
            raise ValueError('xcov_grouped: a row block reaches outside its matrix')
        da, db = A.shape[1], B.shape[1]
        rows = len(ba) * blk_len
        if rows >= 2 ** 31:
            raise ValueError('xcov_grouped: row count must fit in int32')
        splits = xcov_grouped_splits(rows)
        kchunk = -(-max(-(-rows // splits), 1) // 16) * 16
        ln = da * db + da + db
        tab[i] = [A.data_ptr(), B.data_ptr(), A.stride(0), B.stride(0), _is32(A), _is32(B),
                  _check_vector(ca, da, 'xcov_grouped c_a'), _check_vector(cb, db, 'xcov_grouped c_b'),
                  nblk_tot, nblk_tot + len(ba), len(ba), blk_len, da, db, offs[i], slab_tot, splits, kchunk, 0, 0]
        offs[i + 1] = offs[i] + ln + 1
        blks += [ba, bb]
        nblk_tot += 2 * len(ba)
        slab_tot += splits * ln
        tiles.append((-(-da // 64), -(-db // 64), splits))
    out = torch.empty(int(offs[-1]), dtype=F64, device=dev)
    if n == 0:
        return out, offs
    slabs = torch.empty(max(slab_tot, 1), dtype=F64, device=dev)
    words = torch.empty(n * XCOV_WORDS + max(nblk_tot, 1), dtype=torch.int64, device=dev)
    base = words.data_ptr() + 8 * n * XCOV_WORDS
    tab[:, 8] = base + 8 * tab[:, 8]
    tab[:, 9] = base + 8 * tab[:, 9]
    tab[:, 14] = out.data_ptr() + 8 * tab[:, 14]
    tab[:, 15] = slabs.data_ptr() + 8 * tab[:, 15]
    host = np.concatenate([tab.reshape(-1)] + blks + ([np.zeros(1, dtype=np.int64)] if nblk_tot == 0 else []))
    words.copy_(torch.from_numpy(host))
    tiles = _tile_table(tiles)
    tiles_d = torch.from_numpy(tiles).to(dev)
    call('xps_xcov_grouped_f64', words.data_ptr(), n, tiles_d.data_ptr(), len(tiles),
         int((offs[1:] - offs[:-1]).max()), stream())
    return out, offs


def loo_sum(inp, n_out):
    """inp (G, len) float64 device -> (n_out, len): out[f] = sum of inp[g] over g != f in ascending g (plain adds from 0)."""
    if not (inp.is_cuda and inp.dtype == F64 and inp.dim() == 2 and inp.is_contiguous() and 0 <= n_out <= inp.shape[0]):
        raise ValueError('loo_sum: a contiguous (G, len) float64 device tensor and n_out <= G are needed')
    out = torch.empty(n_out, inp.shape[1], dtype=F64, device=inp.device)
    call('xps_loo_sum_f64', inp.data_ptr(), out.data_ptr(), inp.shape[0], n_out, inp.shape[1], stream())
    return out


def apply_grouped(entries):
    """entries: list of (X, mean, W, out): out[:] = (X - mean) @ W for every entry in ONE launch.  X (rows, d_in) float32 /
    float64, mean a float64 vector or None, W (d_in, d_out) float64, out (rows, d_out) float32 / float64 -- device matrices
    with contiguous rows (slices of larger tensors are fine: each is addressed by its own pointer and row stride)."""
    n = len(entries)
    if n == 0:
        return
    tab = np.zeros((n, APPLY_WORDS), dtype=np.int64)
    tiles = []
    for i, (X, mean, W, out) in enumerate(entries):
        for t, what in ((X, 'X'), (W, 'W'), (out, 'out')):
            _check_matrix(t, 'apply_grouped ' + what)
        rows, d_in = X.shape
        d_out = W.shape[1]
        if W.dtype != F64 or W.shape[0] != d_in or tuple(out.shape) != (rows, d_out) or rows >= 2 ** 31:
            raise ValueError('apply_grouped: shapes of X, W and out do not fit together (W must be float64)')
        tab[i] = [X.data_ptr(), _is32(X), X.stride(0), rows, _check_vector(mean, d_in, 'apply_grouped mean'), W.data_ptr(),
                  W.stride(0), d_in, d_out, out.data_ptr(), out.stride(0), _is32(out)]
        tiles.append((-(-rows // 64), -(-d_out // 64)))
    dev = device()
    tiles = _tile_table(tiles)
    tab_d = torch.from_numpy(tab.reshape(-1)).to(dev)
    tiles_d = torch.from_numpy(tiles).to(dev)
    call('xps_apply_grouped_f64', tab_d.data_ptr(), n, tiles_d.data_ptr(), len(tiles), stream())


def gram_tiles(rows):
    """The int32 tile table of a grouped Gram launch (pure numpy): one row {problem, ti, tj} for every 64 x 64 tile with tj <= ti of
    every problem, problems in order, ti ascending and tj ascending inside it.  rows[p]: problem p's row count."""
    out = []
    for p, n in enumerate(rows):
        ti, tj = np.tril_indices(-(-int(n) // 64))
        out.append(np.stack([np.full(len(ti), p), ti, tj], axis=1))
    return np.ascontiguousarray(np.concatenate(out) if out else np.zeros((0, 3)), dtype=np.int32)


def gram_grouped(problems):
    """problems: list of (V, G): G[:] = V @ V.T for every problem in ONE xps_gram_grouped_f64 launch.  V (n, D) float32 / float64,
    G (n, n) float64 -- device matrices with contiguous rows (slices of larger tensors are fine); n and D differ per problem and
    may be 0.  Every G is symmetric bit for bit.  Returns the host tables of the call, which the caller keeps until it has
    synchronised with the stream (the library checks them once more and copies them on the stream)."""
    n = len(problems)
    if n == 0:
        return None
    tab = np.zeros((n, GRAM_WORDS), dtype=np.int64)
    for i, (V, G) in enumerate(problems):
        _check_matrix(V, 'gram_grouped V')
        _check_matrix(G, 'gram_grouped G')
        rows, D = V.shape
        if G.dtype != F64 or tuple(G.shape) != (rows, rows) or rows >= 2 ** 31 - 64 or D >= 2 ** 31 - 16:
            raise ValueError('gram_grouped: G must be the float64 (n, n) matrix of the (n, D) matrix V')
        tab[i, :7] = [V.data_ptr(), _is32(V), V.stride(0), rows, D, G.data_ptr(), G.stride(0)]
    tab, tiles = np.ascontiguousarray(tab.reshape(-1)), gram_tiles(tab[:, 3])
    nb = int(lib().xps_gram_grouped_f64_workspace(n, len(tiles)))
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=device())
    call('xps_gram_grouped_f64', tab.ctypes.data, n, tiles.ctypes.data, len(tiles), ws.data_ptr(), nb, stream())
    return tab, tiles, ws


RBF_WORDS, VAR_WORDS = 8, 8                                 # XPS_RBF_GROUPED_WORDS, XPS_VAR_GROUPED_WORDS of include/xps.h


def rbf_tiles(rows):
    """The int32 tile table of a grouped rbf launch (pure numpy): one row {problem, ti, tj} for every 64 x 64 tile of every problem,
    problems in order, tj fastest.  rows[p]: problem p's row count."""
    t = [-(-int(n) // 64) for n in rows]
    return _tile_table([(c, c) for c in t]) if t else np.zeros((0, 3), dtype=np.int32)


def rbf_grouped(problems):
    """problems: list of (G, gamma, K): K[i][j] = exp(-gamma (G[i][i] + G[j][j] - 2 G[i][j])) for every problem in ONE
    xps_rbf_grouped_from_gram_f64 launch -- xps_rbf_from_gram_f64's bits with the diagonal of G as norms.  G, K (n, n) float64
    device matrices with contiguous rows (slices of larger tensors are fine); several problems may share a G; no K may overlap a
    G of the call.  Returns the host tables of the call, which the caller keeps until it has synchronised with the stream."""
    n = len(problems)
    if n == 0:
        return None
    tab = np.zeros((n, RBF_WORDS), dtype=np.int64)
    for i, (G, gamma, K) in enumerate(problems):
        _check_matrix(G, 'rbf_grouped G')
        _check_matrix(K, 'rbf_grouped K')
        rows = G.shape[0]
        gamma = float(gamma)
        if G.dtype != F64 or K.dtype != F64 or tuple(G.shape) != (rows, rows) or tuple(K.shape) != (rows, rows) or rows >= 2 ** 31 - 64:
            raise ValueError('rbf_grouped: G and K must be float64 (n, n) matrices of one size')
        if not (np.isfinite(gamma) and gamma >= 0):
            raise ValueError(f'rbf_grouped: gamma must be finite and non-negative; got {gamma}')
        tab[i, :6] = [G.data_ptr(), G.stride(0), rows, np.float64(gamma).view(np.int64), K.data_ptr(), K.stride(0)]
    tab, tiles = np.ascontiguousarray(tab.reshape(-1)), rbf_tiles(tab[:, 2])
    nb = int(lib().xps_rbf_grouped_from_gram_f64_workspace(n, len(tiles)))
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=device())
    call('xps_rbf_grouped_from_gram_f64', tab.ctypes.data, n, tiles.ctypes.data, len(tiles), ws.data_ptr(), nb, stream())
    return tab, tiles, ws


def var_grouped(blocks):
    """blocks: list of (V, first, rows): the population variance (numpy's ``.var()``) of all elements of V[first:first + rows], for
    every block in ONE xps_var_grouped_f64 launch, float64 in two passes.  V (n, D) float32 / float64 device matrices with contiguous
    rows.  Returns the float64 device vector of the variances (0 for an empty block) and the host table of the call, which the caller
    keeps until it has synchronised with the stream (downloading the vector does)."""
    n = len(blocks)
    out = torch.empty(n, dtype=F64, device=device())
    if n == 0:
        return out, None
    tab = np.zeros((n, VAR_WORDS), dtype=np.int64)
    for i, (V, first, rows) in enumerate(blocks):
        _check_matrix(V, 'var_grouped V')
        first, rows = int(first), int(rows)
        if first < 0 or rows < 0 or first + rows > V.shape[0] or V.shape[0] >= 2 ** 31 or V.shape[1] >= 2 ** 31:
            raise ValueError('var_grouped: the rows first .. first + rows - 1 must lie inside V')
        tab[i, :6] = [V.data_ptr(), _is32(V), V.stride(0), first, rows, V.shape[1]]
    tab = np.ascontiguousarray(tab.reshape(-1))
    nb = int(lib().xps_var_grouped_f64_workspace(n))
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=device())
    call('xps_var_grouped_f64', tab.ctypes.data, n, out.data_ptr(), ws.data_ptr(), nb, stream())
    return out, (tab, ws)


def cnd_avg_folds(segments):
    """segments: list of (src, out, trials): out[:] = mean over t in `trials` (in that order, float64 adds) of src[t].
    src (n, ...) and out (...) contiguous float64 device tensors, trials an integer sequence.  ONE launch."""
    n = len(segments)
    if n == 0:
        return
    tab = np.zeros((n, CNDAVG_WORDS), dtype=np.int64)
    lists, pos = [], 0
    for i, (src, out, trials) in enumerate(segments):
        row_len = int(np.prod(src.shape[1:]))
        tr = np.asarray(trials, dtype=np.int64).reshape(-1)
        if not (src.is_cuda and out.is_cuda and src.dtype == F64 and out.dtype == F64 and src.is_contiguous()
                and out.is_contiguous() and out.numel() == row_len):
            raise ValueError('cnd_avg_folds: contiguous float64 device tensors with out.numel() == one row of src are needed')
        if len(tr) and (tr.min() < 0 or tr.max() >= src.shape[0]):
            raise ValueError('cnd_avg_folds: a trial index reaches outside src')
        tab[i, :5] = [src.data_ptr(), row_len, out.data_ptr(), pos, pos + len(tr)]
        lists.append(tr.astype(np.int32))
        pos += len(tr)
    dev = device()
    tab_d = torch.from_numpy(tab.reshape(-1)).to(dev)
    tr_d = torch.from_numpy(np.concatenate(lists + [np.zeros(1, dtype=np.int32)])).to(dev)
    for s0 in range(0, n, 65535):                    # (the kernel's grid limit; a fit has folds x conditions segments)
        cnt = min(65535, n - s0)
        call('xps_cnd_avg_folds_f64', tab_d.data_ptr() + 8 * CNDAVG_WORDS * s0, cnt, tr_d.data_ptr(),
             int(tab[s0:s0 + cnt, 1].max()), stream())


PREFIX_WORDS, PREFIX_TILE = 8, 16                            # XPS_PREFIX_KERNELS_WORDS of include/xps.h; the kernel's tile


def gram_center_folds(G, folds):
    """G (N, N) float64 device Gram matrix of all rows about one centre; folds: list of (training rows, held-out rows).  ONE
    xps_gram_center_folds_f64 call.  Returns (Kc, offsets): fold f's (n_all_f, n_tr_f) matrix -- the Gram matrix of its rows
    (training rows first) about the mean of its training rows -- is Kc[offsets[f]:offsets[f + 1]].view(n_all_f, n_tr_f)."""
    _check_matrix(G, 'gram_center_folds G')
    N = G.shape[0]
    if G.dtype != F64 or G.shape[1] != N or N < 1:
        raise ValueError('gram_center_folds: a square float64 device matrix is needed')
    lists, fold_off, n_train, offs = [], [0], [], [0]
    for tr, te in folds:
        tr, te = np.asarray(tr, dtype=np.int64).reshape(-1), np.asarray(te, dtype=np.int64).reshape(-1)
        both = np.concatenate([tr, te])
        if len(tr) < 1 or both.min() < 0 or both.max() >= N:
            raise ValueError('gram_center_folds: a fold without training rows, or a row index outside the Gram matrix')
        lists.append(both.astype(np.int32))
        fold_off.append(fold_off[-1] + len(both))
        n_train.append(len(tr))
        offs.append(offs[-1] + len(both) * len(tr))
    if fold_off[-1] >= 2 ** 31:
        raise ValueError('gram_center_folds: the row lists must fit int32 offsets')
    dev = G.device
    Kc = torch.empty(offs[-1], dtype=F64, device=dev)
    if not lists:
        return Kc, np.asarray(offs, dtype=np.int64)
    rows_d = torch.from_numpy(np.concatenate(lists)).to(dev)
    fold_off_h, n_train_h = np.asarray(fold_off, dtype=np.int32), np.asarray(n_train, dtype=np.int32)      # host arrays of the call
    nb = int(lib().xps_gram_center_folds_f64_workspace(len(lists), fold_off[-1]))
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=dev)
    call('xps_gram_center_folds_f64', G.data_ptr(), G.stride(0), N, rows_d.data_ptr(), fold_off_h.ctypes.data, n_train_h.ctypes.data,
         len(lists), Kc.data_ptr(), ws.data_ptr(), nb, stream())
    return Kc, np.asarray(offs, dtype=np.int64)


def prefix_kernels(problems, rbf, K):
    """problems: list of (Z, cuts): Z an (n, R) float64 device matrix with contiguous rows, cuts a list of (r, outputs) with r
    ascending in 1..R and outputs a list of (gamma, dest): the n x n linear (rbf=False) or rbf kernel matrix of Z[:, :r] is
    written at element dest of the flat float64 device buffer K.  ONE xps_prefix_kernels_f64 call.  Returns the host tables of
    the call, which the caller keeps until it has synchronised with the stream (the library copies them on the stream)."""
    if not (isinstance(K, torch.Tensor) and K.is_cuda and K.dtype == F64 and K.dim() == 1 and K.is_contiguous()):
        raise ValueError('prefix_kernels: K must be a flat contiguous float64 device buffer')
    P = len(problems)
    if P == 0:
        return None
    tab = np.zeros((P, PREFIX_WORDS), dtype=np.int64)
    cuts, cut_out, gammas, dest, tiles = [], [0], [], [], []
    for p, (Z, cut_list) in enumerate(problems):
        _check_matrix(Z, 'prefix_kernels Z')
        n, R = Z.shape
        if Z.dtype != F64 or n < 1 or R < 1 or not cut_list:
            raise ValueError('prefix_kernels: a float64 score matrix with rows, columns and at least one cut is needed')
        tab[p] = [Z.data_ptr(), Z.stride(0), n, R, len(cuts), len(cuts) + len(cut_list), 0, 0]
        prev = 0
        for r, outs in cut_list:
            if not prev < int(r) <= R:
                raise ValueError('prefix_kernels: cuts must ascend within 1..R')
            prev = int(r)
            cuts.append(prev)
            for gamma, d in outs:
                if not (0 <= float(gamma) < np.inf and 0 <= int(d) and int(d) + n * n <= K.numel()):
                    raise ValueError('prefix_kernels: a gamma is negative or not finite, or an output reaches outside K')
                gammas.append(float(gamma))
                dest.append(int(d))
            cut_out.append(len(dest))
        tiles.append((-(-n // PREFIX_TILE), -(-n // PREFIX_TILE)))
    host = (np.ascontiguousarray(tab.reshape(-1)), np.asarray(cuts, dtype=np.int32), np.asarray(cut_out, dtype=np.int32),
            np.asarray(gammas + [0.0], dtype=np.float64), np.asarray(dest + [0], dtype=np.int64), _tile_table(tiles))
    n_out, n_tiles = len(dest), len(host[5])
    nb = int(lib().xps_prefix_kernels_f64_workspace(P, len(cuts), n_out, n_tiles))
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=K.device)
    call('xps_prefix_kernels_f64', host[0].ctypes.data, P, host[1].ctypes.data, host[2].ctypes.data, len(cuts), host[3].ctypes.data,
         host[4].ctypes.data, n_out, host[5].ctypes.data, n_tiles, int(bool(rbf)), K.data_ptr(), K.numel(), ws.data_ptr(), nb, stream())
    return host + (ws,)


def svd_batched(Ks):
    """Thin SVDs of equally shaped small float64 matrices given as ONE (batch, m, n) ndarray, all by one jacobi_batched
    launch: a list of numpy (U, s, Vt) as `svd` returns.  Shapes beyond the one-workgroup kernel take `svd` one by one."""
    Ks = np.ascontiguousarray(Ks, dtype=np.float64)
    b, m, n = Ks.shape
    if m < n:
        return [(Vt.T, s, U.T) for U, s, Vt in svd_batched(np.ascontiguousarray(Ks.transpose(0, 2, 1)))]
    if not lib().xps_jacobi_small_supported(m, n, 1):
        return [svd(to_device(K)) for K in Ks]
    Wb = to_device(np.ascontiguousarray(Ks.transpose(0, 2, 1)))         # [b] row j = column j of K[b]
    Vb = jacobi_batched(Wb, want_v=True)
    return [_svd_tail(W, V) for W, V in zip(Wb.cpu().numpy(), Vb.cpu().numpy())]


# ------------------------------------------------------------------------------------ label-grouped sums (csrc/xps_cluster.hip)
CLUSTER_MAX_CLASSES = 64                                     # XPS_CLUSTER_MAX_CLASSES of include/xps.h


def _check_label_sets(labels_t, k, what):
    """(n, R) of the transposed label array of a call: labels_t[j][r] uint8 on the device, contiguous; 2 <= k <= 64.  The values
    are the caller's to check before the upload (nothing is read here); the kernels skip a label >= k."""
    if not (isinstance(labels_t, torch.Tensor) and labels_t.is_cuda and labels_t.dtype == torch.uint8 and labels_t.dim() == 2
            and labels_t.is_contiguous() and labels_t.shape[0] >= 1 and labels_t.shape[1] >= 1):
        raise ValueError(f'{what}: labels_t must be a contiguous (n, R) uint8 device tensor with n >= 1 and R >= 1')
    if not (isinstance(k, (int, np.integer)) and 2 <= k <= CLUSTER_MAX_CLASSES):
        raise ValueError(f'{what}: 2 <= k <= {CLUSTER_MAX_CLASSES} classes are needed; got {k!r}')
    return int(labels_t.shape[0]), int(labels_t.shape[1])


def _check_f64(t, shape, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == F64 and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
        raise ValueError(f'{what}: a contiguous float64 device tensor of shape {tuple(shape)} is needed')


def _check_gram(G, n, what):
    _check_matrix(G, what + ' G')
    if G.dtype != F64 or tuple(G.shape) != (n, n):
        raise ValueError(f'{what}: G must be the float64 ({n}, {n}) Gram matrix of the labelled rows')


def _class_counts(counts, n, R, k, what):
    """The (R, k) int32 host table of class counts: every count in [0, n], every set adding up to n."""
    c = np.asarray(counts)
    if c.shape != (R, k) or c.dtype.kind not in 'iu' or (c < 0).any() or (c.sum(axis=1) != n).any():
        raise ValueError(f'{what}: counts must be ({R}, {k}) non-negative integers that add up to n = {n} in every label set')
    return np.ascontiguousarray(c, dtype=np.int32)


def label_row_sums(G, labels_t, k, mode):
    """S (R, n, k) float64: S[r][i][q] = sum over j with labels_t[j][r] == q, j ascending, of G[i][j] (mode 0) or of the euclidean
    distance sqrt(max(G[i][i] + G[j][j] - 2 G[i][j], 0)), exactly 0 for j == i (mode 1).  G (n, n) float64 device matrix with
    contiguous rows; labels_t (n, R) uint8 device, values in [0, k).  ONE xps_label_row_sums_f64 launch for all R label sets."""
    n, R = _check_label_sets(labels_t, k, 'label_row_sums')
    _check_gram(G, n, 'label_row_sums')
    if mode not in (0, 1):
        raise ValueError(f'label_row_sums: mode must be 0 (Gram entries) or 1 (euclidean distances); got {mode!r}')
    S = torch.empty(R, n, int(k), dtype=F64, device=G.device)
    call('xps_label_row_sums_f64', G.data_ptr(), G.stride(0), labels_t.data_ptr(), n, R, int(k), int(mode), S.data_ptr(), stream())
    return S


def label_col_sums(V, labels_t, k):
    """M (R, k, w) float64: M[r][p][c] = sum over i with labels_t[i][r] == p, i ascending, of V[r][i][c].  V: (R, n, w) contiguous
    float64 device tensor, or (n, w): one table shared by every label set.  ONE xps_label_col_sums_f64 launch."""
    n, R = _check_label_sets(labels_t, k, 'label_col_sums')
    if not (isinstance(V, torch.Tensor) and V.dim() in (2, 3) and V.shape[-1] >= 1):
        raise ValueError('label_col_sums: V must be an (R, n, w) or (n, w) float64 device tensor with w >= 1')
    w = int(V.shape[-1])
    _check_f64(V, (R, n, w) if V.dim() == 3 else (n, w), 'label_col_sums V')
    M = torch.empty(R, int(k), w, dtype=F64, device=V.device)
    call('xps_label_col_sums_f64', V.data_ptr(), n * w if V.dim() == 3 else 0, labels_t.data_ptr(), n, R, int(k), w, M.data_ptr(),
         stream())
    return M


def silhouette_from_sums(S, counts, labels_t):
    """sklearn's silhouette rules on the mode-1 sums S (R, n, k) of label_row_sums: returns (sil, stats, keep) with sil (R, n) the
    silhouette of every sample under every label set, stats (R, 3) = (mean, mean of the positive values -- NaN when there are
    none --, number of positive values) and `keep` the host table and workspace of the call, which the caller holds until it has
    synchronised with the stream.  counts: (R, k) integer HOST array of class counts (an empty class is skipped)."""
    if not (isinstance(S, torch.Tensor) and S.dim() == 3):
        raise ValueError('silhouette_from_sums: S must be the (R, n, k) tensor of label_row_sums')
    k = int(S.shape[2])
    n, R = _check_label_sets(labels_t, k, 'silhouette_from_sums')
    _check_f64(S, (R, n, k), 'silhouette_from_sums S')
    counts = _class_counts(counts, n, R, k, 'silhouette_from_sums')
    sil = torch.empty(R, n, dtype=F64, device=S.device)
    stats = torch.empty(R, 3, dtype=F64, device=S.device)
    nb = int(lib().xps_silhouette_from_sums_f64_workspace(R, k))
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=S.device)
    call('xps_silhouette_from_sums_f64', S.data_ptr(), counts.ctypes.data, labels_t.data_ptr(), n, R, k, sil.data_ptr(),
         stats.data_ptr(), ws.data_ptr(), nb, stream())
    return sil, stats, (counts, ws)


def centroid_dist_from_sums(G, S0, M, counts, labels_t):
    """dist (R, n) float64: the distance of every sample to the centroid of its own class under every label set, from the Gram
    matrix G, the mode-0 sums S0 (R, n, k) and their class-block sums M (R, k, k) = label_col_sums(S0).  Returns (dist, keep);
    `keep` as in silhouette_from_sums."""
    if not (isinstance(S0, torch.Tensor) and S0.dim() == 3):
        raise ValueError('centroid_dist_from_sums: S0 must be the (R, n, k) tensor of label_row_sums')
    k = int(S0.shape[2])
    n, R = _check_label_sets(labels_t, k, 'centroid_dist_from_sums')
    _check_gram(G, n, 'centroid_dist_from_sums')
    _check_f64(S0, (R, n, k), 'centroid_dist_from_sums S0')
    _check_f64(M, (R, k, k), 'centroid_dist_from_sums M')
    counts = _class_counts(counts, n, R, k, 'centroid_dist_from_sums')
    dist = torch.empty(R, n, dtype=F64, device=S0.device)
    nb = int(lib().xps_centroid_dist_from_sums_f64_workspace(R, k))
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=S0.device)
    call('xps_centroid_dist_from_sums_f64', G.data_ptr(), G.stride(0), S0.data_ptr(), M.data_ptr(), counts.ctypes.data,
         labels_t.data_ptr(), n, R, k, dist.data_ptr(), ws.data_ptr(), nb, stream())
    return dist, (counts, ws)


# ------------------------------------------------------------------------------------ exact t-SNE (csrc/xps_tsne.hip)
TSNE_WORDS, TSNE_TILE_ROWS, TSNE_MAX_SAMPLES = 16, 4, 4096   # XPS_TSNE_WORDS, XPS_TSNE_TILE_ROWS, XPS_TSNE_MAX_SAMPLES of include/xps.h
TSNE_STATE_HEAD, TSNE_STATE_ARRAYS = 8, 15                   # XPS_TSNE_STATE_HEAD, XPS_TSNE_STATE_ARRAYS
# the words of a problem (include/xps.h)
(TS_N, TS_NC, TS_G, TS_LDG, TS_D2, TS_C, TS_P, TS_BETA, TS_STEPS, TS_ROWSUM, TS_YIN, TS_YOUT, TS_STATE, TS_ITBEGIN,
 TS_LR) = range(15)


def tsne_tiles(rows):
    """The int32 tile table of a t-SNE launch (pure numpy): {problem, row tile} for every tile of TSNE_TILE_ROWS rows of every problem, the problems
    in order and the tiles of a problem ascending.  rows[p]: problem p's row count."""
    out = [np.stack([np.full(-(-int(n) // TSNE_TILE_ROWS), p), np.arange(-(-int(n) // TSNE_TILE_ROWS))], axis=1)
           for p, n in enumerate(rows)]
    return np.ascontiguousarray(np.concatenate(out) if out else np.zeros((0, 2)), dtype=np.int32)


def tsne_table(problems):
    """The int64 problem table of a t-SNE launch from one dict per problem: n, nc and the device tensors / scalars the entry reads
    (G, D2, C, P, beta, steps, rowsum, Y_in, Y_out, state, it_begin, lr).  Checks every tensor against n before its address is
    taken; an entry refuses a word it needs and finds 0."""
    tab = np.zeros((len(problems), TSNE_WORDS), dtype=np.int64)
    for row, pr in zip(tab, problems):
        n, nc = int(pr['n']), int(pr.get('nc', 2))
        if not 2 <= n <= TSNE_MAX_SAMPLES or nc not in (1, 2):
            raise ValueError(f't-SNE: 2 <= n <= {TSNE_MAX_SAMPLES} samples and 1 or 2 components are needed; got n = {n}, nc = {nc}')
        row[TS_N], row[TS_NC] = n, nc
        shapes = dict(D2=((n, n), torch.float32), C=((n, n), F64), P=((n, n), F64), beta=((n,), F64), steps=((n,), torch.int32),
                      rowsum=((n,), F64), Y_in=((n, nc), F64), Y_out=((n, nc), F64),
                      state=((2 * (TSNE_STATE_HEAD + TSNE_STATE_ARRAYS * n),), F64))
        words = dict(D2=TS_D2, C=TS_C, P=TS_P, beta=TS_BETA, steps=TS_STEPS, rowsum=TS_ROWSUM, Y_in=TS_YIN, Y_out=TS_YOUT,
                     state=TS_STATE)
        for key, (shape, dtype) in shapes.items():
            t = pr.get(key)
            if t is None:
                continue
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError(f't-SNE: {key} must be a contiguous {dtype} device tensor of shape {shape}')
            row[words[key]] = t.data_ptr()
        if pr.get('G') is not None:
            _check_gram(pr['G'], n, 't-SNE')
            row[TS_G], row[TS_LDG] = pr['G'].data_ptr(), pr['G'].stride(0)
        row[TS_ITBEGIN] = int(pr.get('it_begin', 0))
        row[TS_LR] = np.float64(pr.get('lr', 0.0)).view(np.int64)
    return np.ascontiguousarray(tab.reshape(-1))


def _tsne_call(name, problems, *args):
    """One t-SNE entry for a list of problem dicts.  Returns the host tables and the workspace of the call, which the caller keeps
    until it has synchronised with the stream."""
    tab = tsne_table(problems)
    tiles = tsne_tiles([pr['n'] for pr in problems])
    nb = int(getattr(lib(), name + '_workspace')(len(problems), len(tiles)))
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=device())
    call(name, tab.ctypes.data, len(problems), tiles.ctypes.data, len(tiles), *args, ws.data_ptr(), nb, stream())
    return tab, tiles, ws


def tsne_state(n, dev):
    """The descent state of a problem of n samples: two halves of 8 + 15 n doubles (include/xps.h)."""
    return torch.empty(2 * (TSNE_STATE_HEAD + TSNE_STATE_ARRAYS * int(n)), dtype=F64, device=dev)


def tsne_sqdist(problems):
    """D2 = float32(max((G_ii + G_jj) - 2 G_ij, 0)), zero diagonal, for every problem dict (n, G, D2): ONE launch."""
    return _tsne_call('xps_tsne_sqdist_f32', problems)


def tsne_affinities(problems, perplexity):
    """sklearn's perplexity search and joint probabilities for every problem dict (n, D2, C, P, beta, steps, rowsum): TWO launches."""
    return _tsne_call('xps_tsne_affinities_f64', problems, float(perplexity))


def tsne_descent(problems, n_launches, max_iter, momentum, exaggeration, n_iter_without_progress, min_grad_norm):
    """One phase of sklearn's _gradient_descent for every problem dict (n, nc, P, Y_in, Y_out, state, it_begin, lr): a priming
    launch and n_launches iteration launches, enqueued without a host synchronisation.  The result lies in state half
    n_launches & 1."""
    return _tsne_call('xps_tsne_descent_f64', problems, int(n_launches), int(max_iter), float(momentum), float(exaggeration),
                      int(n_iter_without_progress), float(min_grad_norm))


# ------------------------------------------------------------------------------------ RDM analysis (csrc/xps_rsa.hip)
RSA_STD_WORDS, RSA_RDM_WORDS, RSA_PAIR_WORDS = 8, 8, 12      # XPS_RSA_STD_WORDS, XPS_RSA_RDM_WORDS, XPS_RSA_PAIR_WORDS of include/xps.h
RSA_MAX_CONDITIONS = 1024                                    # XPS_RSA_MAX_CONDITIONS
# the words of a pair (include/xps.h)
CP_A, CP_LDA, CP_NA, CP_IA, CP_B, CP_LDB, CP_NB, CP_IB, CP_M, CP_TABLE, CP_ROW = range(11)


def _check_f64_matrix(t, what):
    _check_matrix(t, what)
    if t.dtype != F64:
        raise ValueError(f'{what}: a float64 device matrix is needed')


def _rows_call(name, tab, words):
    """One row-per-workgroup call of csrc/xps_rsa.hip on the host table `tab`; returns what the caller keeps until it has
    synchronised with the stream."""
    tab = np.ascontiguousarray(tab.reshape(-1))
    n = len(tab) // words
    if n > 65535:
        raise ValueError(f'{name}: {n} problems; at most 65535 go into one call')
    nb = int(getattr(lib(), name + '_workspace')(n))
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=device())
    call(name, tab.ctypes.data, n, ws.data_ptr(), nb, stream())
    return tab, ws


def row_standardize_grouped(problems):
    """problems: list of (X, Z): every row of Z becomes (x - mean) / |x - mean| of the row x of X (scipy.stats.pearsonr's
    arithmetic; NaN for a constant row), for every problem in ONE xps_row_standardize_grouped_f64 launch.  X, Z (rows, D) float64
    device matrices with contiguous rows, D >= 1; Z may be X.  Returns the host table and workspace of the call."""
    if not problems:
        return None
    tab = np.zeros((len(problems), RSA_STD_WORDS), dtype=np.int64)
    for i, (X, Z) in enumerate(problems):
        _check_f64_matrix(X, 'row_standardize_grouped X')
        _check_f64_matrix(Z, 'row_standardize_grouped Z')
        if tuple(Z.shape) != tuple(X.shape) or X.shape[1] < 1 or X.shape[0] >= 2 ** 31 or X.shape[1] >= 2 ** 31:
            raise ValueError('row_standardize_grouped: X and Z must be (rows, D) matrices of one shape with D >= 1')
        tab[i, :6] = [X.data_ptr(), X.stride(0), X.shape[0], X.shape[1], Z.data_ptr(), Z.stride(0)]
    return _rows_call('xps_row_standardize_grouped_f64', tab, RSA_STD_WORDS)


def rdm_from_corr_grouped(problems):
    """problems: list of (C, out): out[i][j] = 1 - clip(C[i][j], -1, 1), NaN kept, the diagonal exactly 0 unless it is NaN, for every
    problem in ONE xps_rdm_from_corr_grouped_f64 launch.  C, out (n, n) float64 device matrices with contiguous rows; out may be C.
    Returns the host table and workspace of the call."""
    if not problems:
        return None
    tab = np.zeros((len(problems), RSA_RDM_WORDS), dtype=np.int64)
    for i, (Cm, out) in enumerate(problems):
        _check_f64_matrix(Cm, 'rdm_from_corr_grouped C')
        _check_f64_matrix(out, 'rdm_from_corr_grouped out')
        n = Cm.shape[0]
        if tuple(Cm.shape) != (n, n) or tuple(out.shape) != (n, n) or n >= 2 ** 31:
            raise ValueError('rdm_from_corr_grouped: C and out must be square matrices of one size')
        tab[i, :5] = [Cm.data_ptr(), Cm.stride(0), n, out.data_ptr(), out.stride(0)]
    return _rows_call('xps_rdm_from_corr_grouped_f64', tab, RSA_RDM_WORDS)


def rdm_compare_perm(pairs, idx, tables, perms, R, cosine=False):
    """The centred triangle products of pairs of RDMs under R relabellings of the second one: ONE xps_rdm_compare_perm_f64 call (two
    launches).  pairs: list of (A, ia, B, ib, m, table): A, B square float64 device matrices with contiguous rows, ia / ib the
    offsets in `idx` (int32 host array) of the m indices of the shared conditions in A / B, `table` the row of `tables` (int64
    (n_tables, 2) host array of {offset in `perms`, m}) that holds the pair's (R + 1, m) int32 permutations, row 0 the identity.
    Returns (stats (n_pairs, 4) = {mean_x, mean_y, sxx, syy}, cross (n_pairs, R + 1), keep): device tensors in pair order, and the
    host tables and workspace of the call, which the caller keeps until it has synchronised with the stream.  The library checks
    every index and every permutation before it launches."""
    n, R = len(pairs), int(R)
    idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
    perms = np.ascontiguousarray(perms, dtype=np.int32).reshape(-1)
    tables = np.ascontiguousarray(tables, dtype=np.int64).reshape(-1, 2)
    if R < 0:
        raise ValueError(f'rdm_compare_perm: R must be non-negative; got {R}')
    tab = np.zeros((n, RSA_PAIR_WORDS), dtype=np.int64)
    for q, (A, ia, B, ib, m, table) in enumerate(pairs):
        _check_f64_matrix(A, 'rdm_compare_perm A')
        _check_f64_matrix(B, 'rdm_compare_perm B')
        if A.shape[0] != A.shape[1] or B.shape[0] != B.shape[1] or A.shape[0] < 1 or B.shape[0] < 1:
            raise ValueError('rdm_compare_perm: A and B must be square matrices')
        if not 2 <= int(m) <= RSA_MAX_CONDITIONS:
            raise ValueError(f'rdm_compare_perm: {int(m)} shared conditions; 2 to XPS_RSA_MAX_CONDITIONS = {RSA_MAX_CONDITIONS} are supported')
        tab[q, :11] = [A.data_ptr(), A.stride(0), A.shape[0], ia, B.data_ptr(), B.stride(0), B.shape[0], ib, m, table, q]
    dev = device()
    stats = torch.empty(n, 4, dtype=F64, device=dev)
    cross = torch.empty(n, R + 1, dtype=F64, device=dev)
    if n == 0:
        return stats, cross, None
    tab = np.ascontiguousarray(tab.reshape(-1))
    nb = int(lib().xps_rdm_compare_perm_f64_workspace(n, len(tables), len(idx), len(perms)))
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=dev)
    call('xps_rdm_compare_perm_f64', tab.ctypes.data, n, tables.ctypes.data, len(tables), idx.ctypes.data, len(idx), perms.ctypes.data,
         len(perms), R, int(bool(cosine)), stats.data_ptr(), cross.data_ptr(), n, ws.data_ptr(), nb, stream())
    return stats, cross, (tab, tables, idx, perms, ws)


# ------------------------------------------------------------------------------------ TME surrogates (csrc/xps_tme.hip)
TME_KRON_WORDS, TME_MAX_AXIS = 20, 1024                      # XPS_TME_KRON_WORDS, XPS_TME_MAX_AXIS of include/xps.h
# the words of a problem (include/xps.h)
(KP_K0, KP_K1, KP_K2, KP_L0, KP_L1, KP_L2, KP_W1_0, KP_W1_1, KP_W1_2, KP_W2_0, KP_W2_1, KP_W2_2, KP_P01, KP_LD01, KP_P02, KP_LD02,
 KP_P12, KP_LD12, KP_SCAL) = range(19)


def _check_f64_vector(v, n, what):
    if not (isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == F64 and v.dim() == 1 and v.is_contiguous() and v.shape[0] == n):
        raise ValueError(f'{what}: a contiguous float64 device vector of {n} elements is needed')
    return v.data_ptr()


def tme_kron_pass(problems):
    """problems: list of dicts with the float64 device tensors l (three multiplier vectors of k0, k1, k2 elements), w1 and w2
    (three vectors each: the single-axis marginals of W = 1 / (l0_i + l1_j + l2_k) and of W^2), p01 (k0, k1), p02 (k0, k2), p12
    (k1, k2) (the pairwise marginals of W^2; matrices with contiguous rows) and scal (2: sum log D, the number of axis-0 slabs with a
    D <= 0).  ONE xps_tme_kron_pass_f64 call for all problems.  Returns the host table and workspace of the call, which the
    caller keeps until it has synchronised with the stream."""
    n = len(problems)
    if n == 0:
        return None
    if n > 65535:
        raise ValueError(f'tme_kron_pass: {n} problems; at most 65535 go into one call')
    tab = np.zeros((n, TME_KRON_WORDS), dtype=np.int64)
    for row, pr in zip(tab, problems):
        k = [int(v.shape[0]) if isinstance(v, torch.Tensor) and v.dim() == 1 else -1 for v in pr['l']]
        if len(k) != 3 or not all(1 <= x <= TME_MAX_AXIS for x in k):
            raise ValueError(f'tme_kron_pass: three multiplier vectors of 1 .. XPS_TME_MAX_AXIS = {TME_MAX_AXIS} elements are needed')
        row[KP_K0:KP_K0 + 3] = k
        for r in range(3):
            row[KP_L0 + r] = _check_f64_vector(pr['l'][r], k[r], 'tme_kron_pass l')
            row[KP_W1_0 + r] = _check_f64_vector(pr['w1'][r], k[r], 'tme_kron_pass w1')
            row[KP_W2_0 + r] = _check_f64_vector(pr['w2'][r], k[r], 'tme_kron_pass w2')
        for key, word, shape in (('p01', KP_P01, (k[0], k[1])), ('p02', KP_P02, (k[0], k[2])), ('p12', KP_P12, (k[1], k[2]))):
            _check_f64_matrix(pr[key], 'tme_kron_pass ' + key)
            if tuple(pr[key].shape) != shape:
                raise ValueError(f'tme_kron_pass: {key} must have shape {shape}')
            row[word], row[word + 1] = pr[key].data_ptr(), max(pr[key].stride(0), shape[1])
        row[KP_SCAL] = _check_f64_vector(pr['scal'], 2, 'tme_kron_pass scal')
    tab = np.ascontiguousarray(tab.reshape(-1))
    nb = int(lib().xps_tme_kron_pass_f64_workspace(n))
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=device())
    call('xps_tme_kron_pass_f64', tab.ctypes.data, n, ws.data_ptr(), nb, stream())
    return tab, ws


def tme_core_scale(z, ls, out=None):
    """core = z * sqrt(W), W_ijk = 1 / (l0_i + l1_j + l2_k), for z (S, k0, k1, k2): a float64 device tensor whose rows (the last
    axis) are contiguous and evenly spaced (a contiguous tensor, or one padded along its last axis).  out: the same kind of
    tensor (default: a new contiguous one; may be z).  ONE launch."""
    if not (isinstance(z, torch.Tensor) and z.is_cuda and z.dtype == F64 and z.dim() == 4):
        raise ValueError('tme_core_scale: z must be an (S, k0, k1, k2) float64 device tensor')
    S, k0, k1, k2 = (int(v) for v in z.shape)
    if not all(1 <= x <= TME_MAX_AXIS for x in (k0, k1, k2)):
        raise ValueError(f'tme_core_scale: every box size must lie in 1 .. XPS_TME_MAX_AXIS = {TME_MAX_AXIS}')
    out = torch.empty((S, k0, k1, k2), dtype=F64, device=z.device) if out is None else out
    lds = []
    for t, what in ((z, 'z'), (out, 'out')):
        ld = max(int(t.stride(2)), k2) if isinstance(t, torch.Tensor) and t.dim() == 4 else 0
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == F64 and tuple(t.shape) == (S, k0, k1, k2)
                and (k2 == 1 or t.stride(3) == 1) and (k1 == 1 or t.stride(2) == ld) and (k0 == 1 or t.stride(1) == k1 * ld)
                and (S <= 1 or t.stride(0) == k0 * k1 * ld)):
            raise ValueError(f'tme_core_scale: {what} must be a float64 device tensor of shape {(S, k0, k1, k2)} with evenly spaced rows')
        lds.append(ld)
    ptrs = [_check_f64_vector(v, k, 'tme_core_scale l') for v, k in zip(ls, (k0, k1, k2))]
    call('xps_tme_core_scale_f64', z.data_ptr(), lds[0], ptrs[0], ptrs[1], ptrs[2], k0, k1, k2, S, out.data_ptr(), lds[1], stream())
    return out


def tme_mode_product(A, B, C, b_kcontig=False, add=None):
    """C[b] = A[b] @ op(B[b]) + add for every member b of a batch in ONE xps_tme_mode_product_f64 launch.  A (M, K) or (batch, M, K),
    B (K, N) or (batch, K, N) -- with b_kcontig (N, K) or (batch, N, K), multiplied as its transpose --, add (M, N) or None, C
    (batch, M, N) float64 or float32: device tensors with contiguous rows; a 2-D operand is shared by the batch.  The batch axis
    of an operand may have any non-negative stride."""
    def mat(t, what, dtypes=(F64,)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in dtypes and t.dim() in (2, 3) and t.shape[-1] >= 1
                and (t.shape[-1] == 1 or t.stride(-1) == 1) and t.stride(-2) >= 0):
            raise ValueError(f'tme_mode_product: {what} must be a 2-D or 3-D device tensor with contiguous rows')
        return max(int(t.stride(-2)), int(t.shape[-1])), (int(t.stride(0)) if t.dim() == 3 else 0)
    lda, sa = mat(A, 'A')
    ldb, sb = mat(B, 'B')
    if C.dim() != 3:
        raise ValueError('tme_mode_product: C must be (batch, M, N)')
    ldc, sc = mat(C, 'C', (F64, torch.float32))
    batch, M, N = (int(v) for v in C.shape)
    K = int(A.shape[-1])
    if (tuple(A.shape[-2:]) != (M, K) or tuple(B.shape[-2:]) != ((N, K) if b_kcontig else (K, N))
            or any(t.dim() == 3 and t.shape[0] != batch for t in (A, B)) or sa < 0 or sb < 0 or K < 1):
        raise ValueError('tme_mode_product: the shapes of A, B and C do not fit together')
    if batch > 1 and sc < (M - 1) * ldc + N:
        raise ValueError('tme_mode_product: the outputs of two batch members overlap')
    ldadd = 0
    if add is not None:
        ldadd, _ = mat(add, 'add')
        if add.dim() != 2 or tuple(add.shape) != (M, N):
            raise ValueError('tme_mode_product: add must be (M, N)')
    call('xps_tme_mode_product_f64', A.data_ptr(), lda, sa, B.data_ptr(), ldb, sb, int(bool(b_kcontig)), ptr(add), ldadd, C.data_ptr(),
         _is32(C), ldc, sc, M, N, K, batch, stream())
    return C
