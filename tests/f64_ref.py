"""Plain numpy references for the float64 GEMM family of csrc/xps_align.hip (tests/test_gpu_f64_kernels.py compares the kernels
with them; tests/test_f64_ref_host.py checks the references themselves on the CPU).

Two references:

* exact -- operands hold small integers (-8..8, stored as float64 or float32), means are multiples of 0.5.  Every centred
  element is then a multiple of 0.5 of size <= 12, every product a multiple of 0.25 of size <= 144 and every partial sum of up
  to 2^20 of them a multiple of 0.25 below 2^28: all of them are float64 numbers, no addition rounds, and ANY summation order
  (BLAS blocks, 64-wide MFMA tiles, split-K slabs) gives the same bits.  The expected result is numpy's product.
* long double -- operands are standard-normal reals, centred in float64 with one rounding as the kernel centres them, multiplied
  in np.longdouble.  A length-K dot product summed in float64 in any order is within gamma_K |a|.|b| of the true one; (K + 2) u
  with u = 2^-53 covers gamma_K = K u / (1 - K u) for every K used here and the error of the long-double reference itself.

The split rules of the library are restated here (slab_layout) so that the tests can say which slab layout a shape was chosen
for; the host test checks the restatement against the library's own workspace queries.
"""
import numpy as np

U = 2.0 ** -53                      # unit roundoff of float64
U32 = 2.0 ** -24                    # ... of float32
DK = 16                             # contraction tile of gemm_f64_kernel
CS_ROWS = 512                       # rows per partial of the column sums


def have_long_double():
    return bool(np.finfo(np.longdouble).eps < 2.0 ** -60)


LONG_DOUBLE_REASON = 'np.longdouble is no wider than float64 here: no reference more precise than the kernel'


# ------------------------------------------------------------------------------------------------ data
def int_matrix(rng, shape, dtype=np.float64):
    """Uniform integers in -8..8 stored in `dtype`."""
    return rng.integers(-8, 9, size=shape).astype(dtype)


def half_vector(rng, d):
    """Multiples of 0.5 in -4..4 (the means of the exact reference)."""
    return rng.integers(-8, 9, size=d) * 0.5


def real_matrix(rng, shape, dtype=np.float64):
    return rng.standard_normal(shape).astype(dtype)


def padded(a, pad, fill):
    """`a` (rows x cols) in the leading columns of a (rows + 1) x (cols + pad) array filled with `fill`; returns the big array
    (the extra row keeps the buffer non-empty for a 0 x cols operand)."""
    big = np.full((a.shape[0] + 1, a.shape[1] + pad), fill, dtype=a.dtype)
    big[:a.shape[0], :a.shape[1]] = a
    return big


# ------------------------------------------------------------------------------------------------ references
def centred(a, mean=None):
    """fl(a - mean) in float64: the one rounding the kernel makes while it stages an operand (float32 widens exactly)."""
    a = np.asarray(a).astype(np.float64)
    return a if mean is None else a - np.asarray(mean, dtype=np.float64)


def op(a, t):
    return a.T if t else a


def exact_product(a, b):
    """Product of integer-valued (multiples of 0.5) float64 operands: exact in any summation order, see the module docstring."""
    return np.ascontiguousarray(a) @ np.ascontiguousarray(b)


def int64_product(a, b, scale=2):
    """The same product in int64 (operands scaled to integers first): the cross-check of the exactness argument."""
    ai, bi = np.rint(a * scale).astype(np.int64), np.rint(b * scale).astype(np.int64)
    assert np.array_equal(ai, a * scale) and np.array_equal(bi, b * scale)
    return (ai @ bi).astype(np.float64) / (scale * scale)


def long_product(a, b):
    return np.asarray(a, dtype=np.longdouble) @ np.asarray(b, dtype=np.longdouble)


def dot_bound(a, b):
    """(K + 2) u |a| |b|, elementwise: any-order float64 dot products of length K against the long-double product."""
    K = a.shape[1]
    return (K + 2) * U * (np.abs(a) @ np.abs(b))


def assert_within(c, ref, bound, what=''):
    """|c - ref| <= bound elementwise, the difference taken in long double."""
    err = np.abs(np.asarray(c, dtype=np.longdouble) - ref)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(err - bound), err.shape)
        raise AssertionError(f'{what}: {int(bad.sum())} of {err.size} elements outside the bound; worst at {i}: '
                             f'error {float(err[i]):.3e}, bound {float(np.asarray(bound)[i]):.3e}')
    with np.errstate(divide='ignore', invalid='ignore'):
        used = np.where(bound > 0, err / bound, 0.0)
    return float(used.max()) if used.size else 0.0


# ------------------------------------------------------------------------------------------------ the library's split rules
def cdiv(a, b):
    return -(-a // b)


def dgemm_splits(M, N, K):
    tiles = cdiv(M, 64) * cdiv(N, 64)
    return max(1, min(cdiv(256, tiles), cdiv(K, 4 * DK), 64))


def xcov_splits(n, da, db):
    tiles = cdiv(da, 64) * cdiv(db, 64)
    return max(1, min(cdiv(1024, tiles), cdiv(n, 256), 512))


def slab_layout(K, splits):
    """(slabs, non-empty slabs, length of the last non-empty slab) of a contraction of length K cut into `splits` chunks of
    cdiv(K, splits) rounded up to the contraction tile."""
    kchunk = cdiv(cdiv(K, splits), DK) * DK
    lens = [max(0, min(K, (z + 1) * kchunk) - z * kchunk) for z in range(splits)]
    full = [x for x in lens if x > 0]
    return splits, len(full), full[-1]


# ------------------------------------------------------------------------------------------------ recurrences
def cheb_scalars(deg, c, e, sigma1):
    """(alpha_j, beta_j, gamma_j) of every product, in float64 as the host code of xps_cheb_filter_f64 computes them."""
    out, sigma = [], sigma1
    for j in range(deg):
        if j == 0:
            alpha, gamma = sigma1 / e, 0.0
        else:
            sigma2 = 1.0 / (2.0 / sigma1 - sigma)
            alpha, gamma, sigma = 2.0 * sigma2 / e, -sigma * sigma2, sigma2
        out.append((alpha, -c * alpha, gamma))
    return out


def cheb_recurrence(C, A, deg, c, e, sigma1, dtype):
    """[Y_1 .. Y_deg] of Y_{j+1} = alpha (C Y_j) + beta Y_j + gamma Y_{j-1} in `dtype` (the scalars are the float64 ones)."""
    C, Y, Vp, out = C.astype(dtype), A.astype(dtype), None, []
    for alpha, beta, gamma in cheb_scalars(deg, c, e, sigma1):
        nxt = dtype(alpha) * (C @ Y) + dtype(beta) * Y
        if Vp is not None:
            nxt = nxt + dtype(gamma) * Vp
        Vp, Y = Y, nxt
        out.append(nxt)
    return out


def lanczos_recurrence(C, v0, steps, dtype):
    """(alpha, beta) of `steps` Lanczos steps without reorthogonalisation from v0 / ||v0||, in `dtype`."""
    C, v = C.astype(dtype), v0.astype(dtype)
    v = v / np.sqrt(v @ v)
    vp, bprev = np.zeros_like(v), dtype(0)
    alpha, beta = np.zeros(steps, dtype=dtype), np.zeros(steps, dtype=dtype)
    for j in range(steps):
        w = C @ v - bprev * vp
        a = w @ v
        w = w - a * v
        b = np.sqrt(w @ w)
        vp, v, bprev = v, w / b, b
        alpha[j], beta[j] = a, b
    return alpha, beta
