"""The references of tests/f64_ref.py, checked on the CPU: the exactness argument against int64, the long-double bound
against a plain float64 product, the restated split rules against the library's workspace queries (host code), and the slab
layouts the GPU tests name."""
import numpy as np
import pytest

import f64_ref as R
from cross_patient_speech_decoding_amd import _build, _lib

needs_long_double = pytest.mark.skipif(not R.have_long_double(), reason=R.LONG_DOUBLE_REASON)


@pytest.fixture(scope='module')
def lib():
    _build.build(verbose=False)
    return _lib.lib()


def test_long_double_is_wider_than_float64():
    if not R.have_long_double():
        pytest.skip(R.LONG_DOUBLE_REASON)
    assert np.finfo(np.longdouble).eps < 2.0 ** -60


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('M,K,N', [(5, 257, 7), (65, 1100, 30), (130, 17, 130)])
def test_exact_product_equals_int64_in_any_order(M, K, N, dtype):
    rng = np.random.default_rng(M * K + N)
    a = R.centred(R.int_matrix(rng, (M, K), dtype), R.half_vector(rng, K))
    b = R.centred(R.int_matrix(rng, (K, N), dtype), R.half_vector(rng, N))
    ref = R.int64_product(a, b)
    np.testing.assert_array_equal(R.exact_product(a, b), ref)
    # another order: split-K slabs of 16 summed last to first, and a reversed contraction
    slabs = [a[:, k:k + 16] @ b[k:k + 16] for k in range(0, K, 16)]
    np.testing.assert_array_equal(sum(reversed(slabs)), ref)
    np.testing.assert_array_equal(a[:, ::-1] @ b[::-1], ref)
    np.testing.assert_array_equal(np.asarray(R.long_product(a, b), dtype=np.float64), ref)


@needs_long_double
def test_float64_product_stays_inside_the_long_double_bound():
    rng = np.random.default_rng(7)
    a = R.centred(R.real_matrix(rng, (130, 1100)), rng.standard_normal(1100))
    b = R.real_matrix(rng, (1100, 130))
    ref, bound = R.long_product(a, b), R.dot_bound(a, b)
    used = R.assert_within(a @ b, ref, bound, 'numpy float64 product')
    assert 0.0 < used < 0.05, used                   # a float64 product uses a small part of the worst-case bound
    wrong = a @ b
    wrong[3, 5] += 2.0 * bound[3, 5]                 # and the check sees an element that leaves it
    with pytest.raises(AssertionError, match='outside the bound'):
        R.assert_within(wrong, ref, bound)
    c32 = (a @ b).astype(np.float32)                 # float32 output: one more rounding
    R.assert_within(c32, ref, bound + R.U32 * np.abs(ref), 'float32 output')


@needs_long_double
def test_a_dropped_contraction_element_leaves_the_bound():
    rng = np.random.default_rng(8)
    a, b = R.real_matrix(rng, (64, 100)), R.real_matrix(rng, (100, 64))
    with pytest.raises(AssertionError, match='outside the bound'):
        R.assert_within(a[:, :-1] @ b[:-1], R.long_product(a, b), R.dot_bound(a, b))


def test_split_rules_restate_the_library(lib):
    for M, N, K in [(45, 45, 1025), (64, 64, 4100), (130, 70, 513), (700, 1, 700), (1, 1, 1), (1024, 45, 1024), (700, 70, 700),
                    (65, 12, 65), (4096, 4096, 100000)]:
        assert lib.xps_dgemm_splitk_workspace(M, N, K) == R.dgemm_splits(M, N, K) * M * N * 8 + 16, (M, N, K)
    for n, da, db in [(257, 5, 7), (4097, 30, 30), (9000, 200, 130), (16400, 256, 256), (1, 1, 1), (409600, 128, 128),
                      (10 ** 6, 8, 8)]:
        assert lib.xps_xcov_f64_workspace(n, da, db) == R.xcov_splits(n, da, db) * da * db * 8 + 16, (n, da, db)
    for n, d in [(1, 1), (512, 3), (513, 64), (123387, 130)]:
        assert lib.xps_colsum_f64_workspace(n, d) == R.cdiv(n, R.CS_ROWS) * d * 8 + 16


def test_slab_layouts_the_gpu_tests_are_chosen_for():
    """(slabs, non-empty, length of the last non-empty one)"""
    assert R.slab_layout(16400, R.xcov_splits(16400, 256, 256)) == (64, 61, 80)
    assert R.slab_layout(4097, R.xcov_splits(4097, 30, 30)) == (17, 17, 1)
    assert R.slab_layout(9000, R.xcov_splits(9000, 200, 130)) == (36, 36, 40)
    assert R.slab_layout(257, R.xcov_splits(257, 5, 7)) == (2, 2, 113)
    assert R.slab_layout(4100, R.dgemm_splits(64, 64, 4100)) == (64, 52, 20)
    assert R.slab_layout(1025, R.dgemm_splits(45, 45, 1025)) == (17, 17, 1)
    assert R.slab_layout(513, R.dgemm_splits(130, 70, 513)) == (9, 9, 1)
    assert R.slab_layout(700, R.dgemm_splits(700, 1, 700)) == (11, 11, 60)


@needs_long_double
def test_recurrences_in_float64_follow_the_long_double_ones():
    rng = np.random.default_rng(9)
    n = 65
    G = rng.standard_normal((n, n))
    C = (G + G.T) / np.sqrt(2.0 * n)
    A = rng.standard_normal((n, 12))
    y64 = R.cheb_recurrence(C, A, 5, -0.85, 1.35, 0.45, np.float64)
    yld = R.cheb_recurrence(C, A, 5, -0.85, 1.35, 0.45, np.longdouble)
    for a, b in zip(y64, yld):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, float(np.abs(b).max()))
    v0 = rng.standard_normal(n)
    a64, b64 = R.lanczos_recurrence(C, v0, 4, np.float64)
    ald, bld = R.lanczos_recurrence(C, 3.0 * v0, 4, np.longdouble)          # the start is normalised: its length is immaterial
    assert np.abs(a64 - ald).max() <= 1e-12 and np.abs(b64 - bld).max() <= 1e-12
    T = np.diag(a64) + np.diag(b64[:-1], 1) + np.diag(b64[:-1], -1)         # Ritz values lie inside the spectrum
    w = np.linalg.eigvalsh(C)
    th = np.linalg.eigvalsh(T)
    assert w[0] - 1e-12 <= th[0] and th[-1] <= w[-1] + 1e-12
