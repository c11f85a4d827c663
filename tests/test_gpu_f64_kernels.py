"""The float64 GEMM family of csrc/xps_align.hip on the MI355X, entry point by entry point through the C ABI:
gemm_f64_kernel<AK, BK> behind xps_dgemm_small / xps_dgemm_splitk / xps_xcov_f64 / xps_apply_f64 / xps_cheb_filter_f64 /
xps_lanczos_f64, and the column sums beside it (xps_colsum_f64).

Two references (tests/f64_ref.py): integer-valued operands, for which every summation order gives the same bits
(assert_array_equal), and standard-normal operands against a long-double product with the textbook bound
(K + 2) 2^-53 |A| |B|.  Conventions of every test: operands live in buffers whose rows are longer than the matrix (leading
dimension = row length + 3) with NaN in the padding, so an element read from outside the matrix poisons the result; outputs are
pre-filled with a sentinel that padding columns and the rows beyond the matrix must keep; workspaces are pre-filled with NaN
bits, so a slab that is read without having been written shows.
"""
import functools

import numpy as np
import pytest

import f64_ref as R

pytestmark = pytest.mark.gpu
needs_long_double = pytest.mark.skipif(not R.have_long_double(), reason=R.LONG_DOUBLE_REASON)

SENT = -77.125                       # no multiple of 0.25: no exact result can equal it (and float32 holds it)
PAD = 3


# ------------------------------------------------------------------------------------------------ device helpers
def torch_():
    import torch
    return torch


def device():
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    return LA.device()


def dev(a):
    return torch_().from_numpy(np.ascontiguousarray(a)).to(device())


def sentinel(shape, f32=False):
    torch = torch_()
    return torch.full(shape, SENT, dtype=torch.float32 if f32 else torch.float64, device=device())


def nan_workspace(nbytes):
    """A workspace of `nbytes` (what the library is told) whose doubles are all NaN, followed by 4 KiB of the same: a read
    just past the end, a row of 130 partial sums for instance, finds NaN too instead of whatever lies there."""
    torch = torch_()
    return torch.full((int(nbytes) + 4096,), 255, dtype=torch.uint8, device=device())


def run(name, *args):
    torch = torch_()
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import call
    call(name, *args, _dev.stream())
    torch.cuda.synchronize()


def lib():
    from cross_patient_speech_decoding_amd._lib import lib as _l
    return _l()


def read_block(Cd, rows, cols):
    """The rows x cols result of a sentinel-filled output buffer; everything else must still be the sentinel."""
    C = Cd.cpu().numpy()
    assert (C[:rows, cols:] == SENT).all(), 'padding columns were written'
    assert (C[rows:] == SENT).all(), 'rows beyond the matrix were written'
    return np.ascontiguousarray(C[:rows, :cols])


def frozen(a):
    a.setflags(write=False)
    return a


@pytest.fixture(scope='module', autouse=True)
def drop_cached_references():
    """The shared inputs and references (xcov_data, cheb_problem) live as long as this module's tests."""
    yield
    xcov_data.cache_clear()
    cheb_problem.cache_clear()


# ------------------------------------------------------------------------------------------------ 1. xps_dgemm_small / splitk
def gemm_operands(seed, M, N, K, ta, tb, real):
    rng = np.random.default_rng(seed)
    gen = R.real_matrix if real else R.int_matrix
    return gen(rng, (K, M) if ta else (M, K)), gen(rng, (N, K) if tb else (K, N))


def run_dgemm(entry, A, B, ta, tb, M, N, K):
    Ap, Bp = R.padded(A, PAD, np.nan), R.padded(B, PAD, np.nan)
    Ad, Bd, Cd = dev(Ap), dev(Bp), sentinel((M + 2, N + PAD))
    if entry == 'small':
        run('xps_dgemm_small', Ad.data_ptr(), Ap.shape[1], int(ta), Bd.data_ptr(), Bp.shape[1], int(tb), Cd.data_ptr(), N + PAD,
            M, N, K)
    else:
        nb = lib().xps_dgemm_splitk_workspace(M, N, K)
        ws = nan_workspace(nb)
        run('xps_dgemm_splitk', Ad.data_ptr(), Ap.shape[1], int(ta), Bd.data_ptr(), Bp.shape[1], int(tb), Cd.data_ptr(), N + PAD,
            M, N, K, ws.data_ptr(), nb)
    return read_block(Cd, M, N)


def check_dgemm(entry, M, N, K, ta, tb, long_double, seed):
    A, B = gemm_operands(seed, M, N, K, ta, tb, real=False)
    ref = R.exact_product(R.op(A, ta), R.op(B, tb))
    assert ref.shape == (M, N) and not (ref == SENT).any()
    C = run_dgemm(entry, A, B, ta, tb, M, N, K)
    np.testing.assert_array_equal(C, ref)
    if M * N * K <= 70 * 70 * 520:                                      # the exactness argument itself, on the small shapes
        np.testing.assert_array_equal(ref, R.int64_product(R.op(A, ta), R.op(B, tb)))
    if K == 0:
        assert not C.any(), 'an empty contraction is a zero matrix'
    if long_double:
        if not R.have_long_double():
            pytest.skip(R.LONG_DOUBLE_REASON)
        A, B = gemm_operands(seed + 1, M, N, K, ta, tb, real=True)
        a, b = R.op(A, ta), R.op(B, tb)
        C = run_dgemm(entry, A, B, ta, tb, M, N, K)
        used = R.assert_within(C, R.long_product(a, b), R.dot_bound(a, b), f'{entry} {M}x{N}x{K} ta={ta} tb={tb}')
        print(f'{entry} ({M}, {N}, {K}) ta={ta} tb={tb}: {100 * used:.3f} % of the bound')
    return C


_MS = (1, 63, 64, 65, 130)
_KS = (0, 1, 3, 15, 16, 17, 100)


def small_cases():
    """40 of the 4 x 5 x 5 x 7 combinations: for every (ta, tb) each M and each N twice and each K at least once, (M, N) pairs
    that differ between the variants; every third case also runs the long-double reference."""
    out = []
    for v, (ta, tb) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        for i in range(10):
            M, N, K = _MS[i % 5], _MS[(2 * i + v + i // 5) % 5], _KS[(i + 2 * v) % 7]
            out.append(pytest.param(M, N, K, ta, tb, (i + v) % 3 == 0, id=f'{M}x{N}x{K}-ta{ta}-tb{tb}'))
    return out


def test_small_cases_cover_the_grid():
    cases = [p.values for p in small_cases()]
    assert len(cases) == 40 and len(set(cases)) == 40
    for v in [(0, 0), (0, 1), (1, 0), (1, 1)]:
        mine = [c for c in cases if (c[3], c[4]) == v]
        assert {c[0] for c in mine} == set(_MS) and {c[1] for c in mine} == set(_MS) and {c[2] for c in mine} == set(_KS)
    assert 12 <= sum(c[5] for c in cases) <= 15


@pytest.mark.parametrize('M,N,K,ta,tb,long_double', small_cases())
def test_dgemm_small(M, N, K, ta, tb, long_double):
    check_dgemm('small', M, N, K, ta, tb, long_double, seed=1000 * M + 10 * N + K)


# Split-K shapes (M, N, K) and the slab layout each was chosen for (f64_ref.slab_layout; tests/test_f64_ref_host.py pins them):
#   (45, 45, 1025)   17 slabs of 64, the last holds ONE contraction element
#   (64, 64, 4100)   64 slabs of 80: 52 hold data (the last 20 elements), 12 are EMPTY and must be written as zeros
#   (130, 70, 513)   9 slabs of 64, the last holds one element; 3 x 2 output tiles with edge tiles in both directions
#   (700, 1, 700)    the Lanczos product: N = 1, 11 slabs of 64, the last holds 60, 11 row tiles
_SPLITK = [(45, 45, 1025, True), (64, 64, 4100, False), (130, 70, 513, True), (700, 1, 700, False)]


@pytest.mark.parametrize('ta,tb', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('M,N,K,long_double', _SPLITK)
def test_dgemm_splitk(M, N, K, long_double, ta, tb):
    seed = 1000 * M + 10 * N + K
    C1 = check_dgemm('splitk', M, N, K, ta, tb, long_double, seed)
    A, B = gemm_operands(seed + 1, M, N, K, ta, tb, real=True)          # real data: a changed order would change the bits
    one, two = run_dgemm('splitk', A, B, ta, tb, M, N, K), run_dgemm('splitk', A, B, ta, tb, M, N, K)
    np.testing.assert_array_equal(one, two)
    assert np.isfinite(one).all() and np.isfinite(C1).all()


def test_dgemm_splitk_honours_its_workspace_query():
    from cross_patient_speech_decoding_amd import _dev
    M, N, K = 45, 45, 1025
    A, B = gemm_operands(1, M, N, K, 0, 0, real=False)
    Ad, Bd, Cd = dev(A), dev(B), sentinel((M, N))
    nb = lib().xps_dgemm_splitk_workspace(M, N, K)
    assert nb == R.dgemm_splits(M, N, K) * M * N * 8 + 16
    ws = nan_workspace(nb)
    rc = lib().xps_dgemm_splitk(Ad.data_ptr(), K, 0, Bd.data_ptr(), N, 0, Cd.data_ptr(), N, M, N, K, ws.data_ptr(), nb - 1,
                                _dev.stream())
    torch_().cuda.synchronize()
    assert rc == -3                                                      # XPS_E_WORKSPACE
    assert (Cd.cpu().numpy() == SENT).all()
    rc = lib().xps_dgemm_splitk(Ad.data_ptr(), K, 0, Bd.data_ptr(), N, 0, Cd.data_ptr(), N, M, N, K, ws.data_ptr(), nb,
                                _dev.stream())
    torch_().cuda.synchronize()
    assert rc == 0
    np.testing.assert_array_equal(Cd.cpu().numpy(), A @ B)


@pytest.mark.parametrize('M,N,K,entry', [(40, 30, 600, 'xps_dgemm_splitk'),      # K >= 512, one output tile
                                         (40, 30, 100, 'xps_dgemm_small'),       # short contraction
                                         (520, 520, 512, 'xps_dgemm_small')])    # K >= 512 but 81 tiles fill the chip already
def test_linalg_dgemm_routing(monkeypatch, M, N, K, entry):
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    names, real = [], LA.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(LA, 'call', recording)
    for ta, tb in [(False, False), (True, False), (False, True), (True, True)]:
        A, B = gemm_operands(M + K, M, N, K, ta, tb, real=False)
        del names[:]
        C = LA.dgemm(dev(A), dev(B), ta=ta, tb=tb)
        assert names == [entry]
        np.testing.assert_array_equal(C.cpu().numpy(), R.exact_product(R.op(A, ta), R.op(B, tb)))


# ------------------------------------------------------------------------------------------------ 2. xps_xcov_f64
@functools.lru_cache(maxsize=None)
def xcov_data(n, d, kind, which):
    """(float64 matrix, its float32 twin, a mean vector): integers / halves (kind 'int') or standard normals ('real')."""
    rng = np.random.default_rng(7919 * n + 31 * d + (which == 'b') + 500 * (kind == 'real'))
    if kind == 'int':
        X, mean = R.int_matrix(rng, (n, d)), R.half_vector(rng, d)
    else:
        X, mean = R.real_matrix(rng, (n, d)), rng.standard_normal(d)
    return frozen(X), frozen(X.astype(np.float32)), frozen(mean)


def run_xcov(A, mean_a, B, mean_b, same):
    n, da = A.shape
    db = B.shape[1]
    Ad = dev(R.padded(A, PAD, np.nan))
    Bd = Ad if same else dev(R.padded(B, PAD + 1, np.nan))
    ma, mb = (None if m is None else dev(m) for m in (mean_a, mean_b))
    Cd = sentinel((da + 1, db + PAD))
    nb = lib().xps_xcov_f64_workspace(n, da, db)
    ws = nan_workspace(nb)
    run('xps_xcov_f64', Ad.data_ptr(), int(A.dtype == np.float32), da + PAD, None if ma is None else ma.data_ptr(),
        Bd.data_ptr(), int(B.dtype == np.float32), Bd.shape[1], None if mb is None else mb.data_ptr(),
        Cd.data_ptr(), db + PAD, n, da, db, ws.data_ptr(), nb)
    return read_block(Cd, da, db)


def xcov_case(n, da, db, kind, a32, b32, use_ma, use_mb, same):
    A64, A32, ma = xcov_data(n, da, kind, 'a')
    B64, B32, mb = (A64, A32, ma) if same else xcov_data(n, db, kind, 'b')
    A, B = (A32 if a32 else A64), (B32 if b32 else B64)
    ma, mb = (ma if use_ma else None), (mb if use_mb else None)
    return A, ma, B, mb, R.centred(A, ma).T, R.centred(B, mb)


def xcov_combos():
    out = [(a32, b32, ma, mb, False) for a32 in (0, 1) for b32 in (0, 1) for ma in (0, 1) for mb in (0, 1)]
    return out + [(f32, f32, m, m, True) for f32 in (0, 1) for m in (0, 1)]


# (257, 5, 7): 2 slabs of 144 rows, the second holds 113; (4097, 30, 30): 17 slabs of 256 rows, the last holds ONE row
@pytest.mark.parametrize('a32,b32,use_ma,use_mb,same', xcov_combos())
@pytest.mark.parametrize('n,da,db', [(257, 5, 7), (4097, 30, 30)])
def test_xcov_small_shapes(n, da, db, a32, b32, use_ma, use_mb, same):
    db = da if same else db
    A, ma, B, mb, at, b = xcov_case(n, da, db, 'int', a32, b32, use_ma, use_mb, same)
    ref = R.exact_product(at, b)
    assert not (ref == SENT).any()
    np.testing.assert_array_equal(run_xcov(A, ma, B, mb, same), ref)
    if n == 257:
        np.testing.assert_array_equal(ref, R.int64_product(at, b))
    if not R.have_long_double():
        pytest.skip(R.LONG_DOUBLE_REASON)
    A, ma, B, mb, at, b = xcov_case(n, da, db, 'real', a32, b32, use_ma, use_mb, same)
    R.assert_within(run_xcov(A, ma, B, mb, same), R.long_product(at, b), R.dot_bound(at, b), f'xcov {n} x {da} x {db}')


# (9000, 200, 130): 4 x 3 output tiles with edge tiles, 36 slabs of 256 rows, the last holds 40;
# (16400, 256, 256): 64 slabs of 272 rows of which 61 hold data (the last 80 rows) and 3 are EMPTY
@pytest.mark.parametrize('f32', [0, 1])
@pytest.mark.parametrize('n,da,db', [(9000, 200, 130), (16400, 256, 256)])
def test_xcov_large_shapes(n, da, db, f32):
    A, ma, B, mb, at, b = xcov_case(n, da, db, 'int', f32, f32, 1, 1, False)
    np.testing.assert_array_equal(run_xcov(A, ma, B, mb, False), R.exact_product(at, b))


# ------------------------------------------------------------------------------------------------ 3. xps_apply_f64
def run_apply(X, mean, W, out_f32):
    n, d_in = X.shape
    d_out = W.shape[1]
    Xd, Wd = dev(R.padded(X, PAD, np.nan)), dev(R.padded(W, 2, np.nan))
    md = None if mean is None else dev(mean)
    Yd = sentinel((n + 1, d_out + PAD), f32=out_f32)
    run('xps_apply_f64', Xd.data_ptr(), int(X.dtype == np.float32), d_in + PAD, None if md is None else md.data_ptr(),
        Wd.data_ptr(), d_out + 2, Yd.data_ptr(), int(out_f32), d_out + PAD, n, d_in, d_out)
    Y = read_block(Yd, n, d_out)
    assert Y.dtype == (np.float32 if out_f32 else np.float64)
    return Y


@pytest.mark.parametrize('d_out', [1, 30, 65])
@pytest.mark.parametrize('d_in', [1, 17, 128])
@pytest.mark.parametrize('n', [1, 65, 1000])
def test_apply(n, d_in, d_out):
    rng = np.random.default_rng(10000 * n + 100 * d_in + d_out)
    ints = (R.int_matrix(rng, (n, d_in)), R.half_vector(rng, d_in), R.int_matrix(rng, (d_in, d_out)))
    reals = (R.real_matrix(rng, (n, d_in)), rng.standard_normal(d_in), R.real_matrix(rng, (d_in, d_out)))
    worst = 0.0
    for x32 in (0, 1):
        for use_mean in (0, 1):
            X, mean, W = ints
            X = X.astype(np.float32) if x32 else X
            mean = mean if use_mean else None
            ref = R.exact_product(R.centred(X, mean), W)
            assert not (ref == SENT).any()
            np.testing.assert_array_equal(run_apply(X, mean, W, False), ref)
            y32 = run_apply(X, mean, W, True)
            np.testing.assert_array_equal(y32, ref.astype(np.float32))
            if not R.have_long_double():
                continue
            X, mean, W = reals
            X = X.astype(np.float32) if x32 else X
            mean = mean if use_mean else None
            xc = R.centred(X, mean)
            ref, bound = R.long_product(xc, W), R.dot_bound(xc, W)
            what = f'apply {n} x {d_in} x {d_out} x32={x32} mean={use_mean}'
            worst = max(worst, R.assert_within(run_apply(X, mean, W, False), ref, bound, what))
            R.assert_within(run_apply(X, mean, W, True), ref, bound + R.U32 * np.abs(ref), what + ' float32 out')
    print(f'apply ({n}, {d_in}, {d_out}): at most {100 * worst:.3f} % of the bound')


# ------------------------------------------------------------------------------------------------ 4. xps_colsum_f64
_COLSUM_LD = 130 + PAD
# rows -> number of 512-row partials: the unrolled-by-8 loop of colsum64_stage2 is entered by group q of 16 when q + 112 < partials
_COLSUM_N = {1: 1, 300: 1, 8192: 16, 8193: 17, 57344: 112, 57345: 113, 65536: 128, 65636: 129, 123387: 241}


@pytest.fixture(scope='module')
def colsum_bases():
    """One integer and one real (max rows) x (130 + 3) matrix in both dtypes, uploaded once; every case reads a corner of them."""
    rng = np.random.default_rng(512)
    n = max(_COLSUM_N)
    out = {}
    for kind, X in (('int', R.int_matrix(rng, (n, _COLSUM_LD))), ('real', R.real_matrix(rng, (n, _COLSUM_LD)))):
        X32 = X.astype(np.float32)
        out[kind, 0] = (frozen(X), dev(X))
        out[kind, 1] = (frozen(X32), dev(X32))
    yield out
    out.clear()


def run_colsum(Xd, f32, n, d):
    out = sentinel((d + 2,))
    nb = lib().xps_colsum_f64_workspace(n, d)
    ws = nan_workspace(nb)
    run('xps_colsum_f64', Xd.data_ptr(), f32, _COLSUM_LD, n, d, out.data_ptr(), ws.data_ptr(), nb)
    o = out.cpu().numpy()
    assert (o[d:] == SENT).all()
    return o[:d]


@pytest.mark.parametrize('f32', [0, 1])
@pytest.mark.parametrize('d', [1, 64, 65, 130])
@pytest.mark.parametrize('n', sorted(_COLSUM_N))
def test_colsum(colsum_bases, n, d, f32):
    assert R.cdiv(n, R.CS_ROWS) == _COLSUM_N[n]
    X, Xd = colsum_bases['int', f32]
    ref = X[:n, :d].sum(axis=0, dtype=np.float64)                       # integers below 2^53: exact in any order
    assert not (ref == SENT).any()
    np.testing.assert_array_equal(run_colsum(Xd, f32, n, d), ref)
    if not R.have_long_double():
        pytest.skip(R.LONG_DOUBLE_REASON)
    X, Xd = colsum_bases['real', f32]
    ref = X[:n, :d].sum(axis=0, dtype=np.longdouble)
    bound = n * R.U * np.abs(X[:n, :d]).sum(axis=0, dtype=np.longdouble)
    R.assert_within(run_colsum(Xd, f32, n, d), ref, bound, f'colsum {n} x {d}')


# ------------------------------------------------------------------------------------------------ 5. recurrences
_CHEB = dict(c=-0.55, e=1.55, sigma1=1.55 / 2.45)    # damps [-2.1, 1.0], the top Ritz value 1.9 maps to 1: spectrum of C in [-2, 2]
_DEGS = (2, 5, 20)


def sym_matrix(rng, n):
    G = rng.standard_normal((n, n))
    return (G + G.T) / np.sqrt(2.0 * n)              # Wigner: spectrum in about [-2, 2]


@functools.lru_cache(maxsize=None)
def cheb_problem(n, m):
    """C, A and the recurrence to the largest degree in long double and in plain float64 (Y_deg does not depend on how many
    products follow it, so one run serves every degree)."""
    rng = np.random.default_rng(100 * n + m)
    C, A = sym_matrix(rng, n), rng.standard_normal((n, m))
    deg = max(_DEGS)
    yld = R.cheb_recurrence(C, A, deg, dtype=np.longdouble, **_CHEB) if R.have_long_double() else None
    return frozen(C), frozen(A), yld, R.cheb_recurrence(C, A, deg, dtype=np.float64, **_CHEB)


def run_cheb(C, A, deg, alias=False):
    n, m = A.shape
    Cd, Ad = dev(R.padded(C, PAD, np.nan)), dev(A)
    out = sentinel((n + 1, m))
    nb = lib().xps_cheb_filter_f64_workspace(n, m)
    ws = nan_workspace(nb)
    run('xps_cheb_filter_f64', Cd.data_ptr(), n + PAD, n, Ad.data_ptr(), m, deg, _CHEB['c'], _CHEB['e'], _CHEB['sigma1'],
        Ad.data_ptr() if alias else out.data_ptr(), ws.data_ptr(), nb)
    return read_block(out, n, m)


@needs_long_double
@pytest.mark.parametrize('m', [1, 12, 70])
@pytest.mark.parametrize('n', [65, 700])
def test_cheb_filter_degree_one(n, m):
    """Y_1 = alpha (C A) + (-c alpha) A: a dot product of length n, two scalings and one addition, so
    |Y - R| <= (n + 4) 2^-53 (|alpha| |C| |A| + |c alpha| |A|)."""
    C, A, yld, _ = cheb_problem(n, m)
    (alpha, beta, _g), = R.cheb_scalars(1, **_CHEB)
    ref = np.longdouble(alpha) * R.long_product(C, A) + np.longdouble(beta) * A.astype(np.longdouble)
    assert np.array_equal(ref, yld[0])
    bound = (n + 4) * R.U * (abs(alpha) * (np.abs(C) @ np.abs(A)) + abs(beta) * np.abs(A))
    used = R.assert_within(run_cheb(C, A, 1), ref, bound, f'cheb deg 1 {n} x {m}')
    print(f'cheb ({n}, {m}) deg 1: {100 * used:.3f} % of the bound')


@needs_long_double
@pytest.mark.parametrize('deg', _DEGS)
@pytest.mark.parametrize('m', [1, 12, 70])
@pytest.mark.parametrize('n', [65, 700])
def test_cheb_filter_recurrence(n, m, deg):
    """Y_deg against the same recurrence in long double; allowed: 8 x the largest elementwise error of the plain float64 numpy
    recurrence against that long-double result (the 8 covers another summation order: 64-wide tiles and slabs).
    Observed ratio (device error / numpy error) on the MI355X: 0.29 .. 1.62 over the 18 cases (errors 4e-17 .. 6e-16)."""
    C, A, yld, y64 = cheb_problem(n, m)
    ref = yld[deg - 1]
    err_np = float(np.abs(y64[deg - 1] - ref).max())
    err = float(np.abs(run_cheb(C, A, deg).astype(np.longdouble) - ref).max())
    print(f'cheb ({n}, {m}) deg {deg}: device error {err:.3e}, numpy float64 error {err_np:.3e}, ratio {err / err_np:.2f}')
    assert err <= 8.0 * err_np


def test_cheb_filter_refuses_out_equal_to_input():
    from cross_patient_speech_decoding_amd._lib import XpsError
    rng = np.random.default_rng(3)
    C, A = sym_matrix(rng, 65), rng.standard_normal((65, 12))
    with pytest.raises(XpsError, match='bad argument'):
        run_cheb(C, A, 2, alias=True)


def run_lanczos(C, v0, steps):
    n = C.shape[0]
    Cd, vd = dev(R.padded(C, PAD, np.nan)), dev(v0)
    ab = sentinel((2, steps + 1))
    nb = lib().xps_lanczos_f64_workspace(n)
    ws = nan_workspace(nb)
    run('xps_lanczos_f64', Cd.data_ptr(), n + PAD, n, steps, vd.data_ptr(), ab.data_ptr(), ab.data_ptr() + 8 * (steps + 1),
        ws.data_ptr(), nb)
    assert np.array_equal(vd.cpu().numpy(), v0), 'the start vector is an input'
    ab = ab.cpu().numpy()
    assert (ab[:, steps] == SENT).all()
    return ab[0, :steps], ab[1, :steps]


@needs_long_double
@pytest.mark.parametrize('steps', [1, 4])
@pytest.mark.parametrize('n', [5, 700])
def test_lanczos(n, steps):
    """alpha, beta against the same recurrence in long double, from a unit start vector and from 3 x that vector (the entry
    point starts from v0 / ||v0||); allowed: 8 x the largest error of the plain float64 numpy recurrence.
    Observed ratio (device error / numpy error) on the MI355X: 0.27 .. 2.63 over the 4 cases x 2 lengths (errors 3e-17 .. 3e-16)."""
    rng = np.random.default_rng(10 * n + steps)
    C, v0 = sym_matrix(rng, n), rng.standard_normal(n)
    v0 = v0 / np.linalg.norm(v0)
    ald, bld = R.lanczos_recurrence(C, v0, steps, np.longdouble)
    a64, b64 = R.lanczos_recurrence(C, v0, steps, np.float64)
    err_np = float(max(np.abs(a64 - ald).max(), np.abs(b64 - bld).max()))
    for scale in (1.0, 3.0):
        a, b = run_lanczos(C, scale * v0, steps)
        err = float(max(np.abs(a - ald).max(), np.abs(b - bld).max()))
        print(f'lanczos n={n} steps={steps} |v0|={scale}: device error {err:.3e}, numpy float64 error {err_np:.3e}, '
              f'ratio {err / err_np:.2f}')
        assert err <= 8.0 * err_np, f'start vector of length {scale}'


# ------------------------------------------------------------------------------------------------ 6. wrapper strides
def view_of(M, kind):
    """A device view that holds the matrix M without being contiguous."""
    torch = torch_()
    r, c = M.shape
    if kind == 'T':                                                      # .T of the transposed copy: strides (1, r)
        v = dev(M.T).T
    elif kind == 'step2':                                                # every second column of a matrix twice as wide
        big = torch.full((r, 2 * c), float('nan'), dtype=dev(M).dtype, device=device())
        big[:, ::2] = dev(M)
        v = big[:, ::2]
    else:                                                                # 'rows': the leading columns of a wider matrix
        big = torch.full((r, c + 5), float('nan'), dtype=dev(M).dtype, device=device())
        big[:, :c] = dev(M)
        v = big[:, :c]
    assert tuple(v.shape) == (r, c) and (not v.is_contiguous() or r == 1 or c == 1)
    assert torch.equal(v, dev(M))
    return v


def vec_view_of(m, kind):
    if kind != 'step2':
        return dev(m)
    big = torch_().full((2 * len(m),), float('nan'), dtype=torch_().float64, device=device())
    big[::2] = dev(m)
    return big[::2]


@pytest.fixture
def recorded(monkeypatch):
    """The (name, args) of every library call the alignment wrappers make."""
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    calls, real = [], LA.call

    def recording(name, *args):
        calls.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(LA, 'call', recording)
    return calls


def assert_passed_in_place(calls, name, view, ptr_at, ld_at):
    """The row-strided view itself went to the library: its pointer and its row stride, no copy."""
    (args,) = [a for nm, a in calls if nm == name]
    assert args[ptr_at] == view.data_ptr() and args[ld_at] == view.stride(0) and view.stride(0) > view.shape[1]


KINDS = ['T', 'step2', 'rows']


@pytest.mark.parametrize('kind', KINDS)
def test_wrapper_col_mean_strided(recorded, kind):
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    X = R.real_matrix(np.random.default_rng(1), (1300, 65), np.float32)
    want = LA.col_mean(dev(X))
    np.testing.assert_allclose(want.cpu().numpy(), X.astype(np.float64).mean(axis=0), rtol=0, atol=1e-13)
    del recorded[:]
    v = view_of(X, kind)
    assert torch_().equal(LA.col_mean(v), want)
    if kind == 'rows':
        assert_passed_in_place(recorded, 'xps_colsum_f64', v, 0, 2)


@pytest.mark.parametrize('kind', KINDS)
def test_wrapper_xcov_strided(recorded, kind):
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    rng = np.random.default_rng(2)
    A, B = R.real_matrix(rng, (600, 30), np.float32), R.real_matrix(rng, (600, 20))
    ma, mb = rng.standard_normal(30), rng.standard_normal(20)
    want = LA.xcov(dev(A), dev(B), dev(ma), dev(mb))
    np.testing.assert_allclose(want.cpu().numpy(), R.centred(A, ma).T @ R.centred(B, mb), rtol=0, atol=1e-10)
    want_gram = LA.xcov(dev(A), mean_a=dev(ma))
    del recorded[:]
    va, vb = view_of(A, kind), view_of(B, kind)
    assert torch_().equal(LA.xcov(va, vb, vec_view_of(ma, kind), vec_view_of(mb, kind)), want)
    if kind == 'rows':
        assert_passed_in_place(recorded, 'xps_xcov_f64', va, 0, 2)
        assert_passed_in_place(recorded, 'xps_xcov_f64', vb, 4, 6)
    assert torch_().equal(LA.xcov(va, mean_a=vec_view_of(ma, kind)), want_gram)


@pytest.mark.parametrize('kind', KINDS)
def test_wrapper_apply_strided(recorded, kind):
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    rng = np.random.default_rng(3)
    X, W, mean = R.real_matrix(rng, (300, 17), np.float32), R.real_matrix(rng, (17, 9)), rng.standard_normal(17)
    want = LA.apply(dev(X), dev(W), dev(mean))
    np.testing.assert_allclose(want.cpu().numpy(), R.centred(X, mean) @ W, rtol=0, atol=1e-12)
    del recorded[:]
    vx, vw = view_of(X, kind), view_of(W, kind)
    assert torch_().equal(LA.apply(vx, vw, vec_view_of(mean, kind)), want)
    if kind == 'rows':
        assert_passed_in_place(recorded, 'xps_apply_f64', vx, 0, 2)
        assert_passed_in_place(recorded, 'xps_apply_f64', vw, 4, 5)


@pytest.mark.parametrize('kind', KINDS)
def test_wrapper_cheb_filter_strided(recorded, kind):
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    rng = np.random.default_rng(4)
    C, A = sym_matrix(rng, 130), rng.standard_normal((130, 12))
    want = LA.cheb_filter(dev(C), dev(A), 3, **_CHEB)
    np.testing.assert_allclose(want.cpu().numpy(), R.cheb_recurrence(C, A, 3, dtype=np.float64, **_CHEB)[-1], rtol=0, atol=1e-11)
    del recorded[:]
    vc = view_of(C, kind)
    assert torch_().equal(LA.cheb_filter(vc, view_of(A, kind), 3, **_CHEB), want)
    if kind == 'rows':
        assert_passed_in_place(recorded, 'xps_cheb_filter_f64', vc, 0, 1)


@pytest.mark.parametrize('kind', KINDS)
def test_wrapper_lanczos_bounds_strided(recorded, kind):
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    C = sym_matrix(np.random.default_rng(5), 130)
    want = LA._lanczos_bounds(dev(C))
    w = np.linalg.eigvalsh(C)                                            # (a sanity check of `want`, not an accuracy test)
    slack = 0.1 * (w[-1] - w[0])
    assert want[0] < w[0] + slack and w[-1] - slack < want[1] and want[1] - want[0] < 1.5 * (w[-1] - w[0])
    del recorded[:]
    vc = view_of(C, kind)
    assert LA._lanczos_bounds(vc) == want
    if kind == 'rows':
        assert_passed_in_place(recorded, 'xps_lanczos_f64', vc, 0, 1)


@pytest.mark.parametrize('K,entry', [(100, 'xps_dgemm_small'), (600, 'xps_dgemm_splitk')])
@pytest.mark.parametrize('kind', KINDS)
def test_wrapper_dgemm_strided(recorded, kind, K, entry):
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    for ta, tb in [(False, False), (True, True)]:
        A, B = gemm_operands(K, 40, 30, K, ta, tb, real=True)
        want = LA.dgemm(dev(A), dev(B), ta=ta, tb=tb)
        np.testing.assert_allclose(want.cpu().numpy(), R.op(A, ta) @ R.op(B, tb), rtol=0, atol=1e-11)
        del recorded[:]
        va, vb = view_of(A, kind), view_of(B, kind)
        assert torch_().equal(LA.dgemm(va, vb, ta=ta, tb=tb), want)
        if kind == 'rows':
            assert_passed_in_place(recorded, entry, va, 0, 1)
            assert_passed_in_place(recorded, entry, vb, 3, 4)
