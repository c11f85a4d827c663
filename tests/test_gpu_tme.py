"""surrogates/tme.py on the MI355X against tests/tme_ref.py: the fit (kept ranks, the residual recomputed in long double from the
returned multipliers, the covariance they imply against Sigma_r of the data), the sampling map on a given z within the chained
elementwise bar, the mean tensor, reproducibility (seed, chunking, fit_many against fit) and one statistical sanity test."""
import functools

import numpy as np
import pytest

import tme_ref as TR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
TOL = 1e-9

# The statistical test's bound.  tests/tme_ref.py's surrogate_cov_deviation(random_tensor((6, 5, 4), 11), 4096, seed) -- the host
# restatement with numpy's default_rng(seed) -- gave, over seed = 0 .. 19, relative Frobenius deviations of the mean of
# S_(r) S_(r)^T from Sigma_r between 0.0060 and 0.020792502486893977 (the largest over the three axes).  The device draws are other
# numbers from the same law, so the bound is twice the largest value seen.
STAT_BOUND = 2 * 0.020792502486893977


def torch_():
    import torch
    return torch


def SUR():
    from cross_patient_speech_decoding_amd import surrogates
    return surrogates


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def data(shape, f32=False):
    X = TR.random_tensor(shape, 1)
    return X.astype(np.float32) if f32 else X


CASES = [(s, c, False) for s, c in TR.FITS] + [((6, 8, 4), True, True)]


def case_id(case):
    return TR.fit_name(case[0], case[1]) + ('_f32' if case[2] else '')


@functools.lru_cache(maxsize=None)
def fitted(shape, center, f32):
    return SUR().TME(center=center).fit(data(shape, f32))


@functools.lru_cache(maxsize=None)
def host_fit(shape, center, f32):
    return TR.fit(data(shape, f32).astype(np.float64), center_=center)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_fit_keeps_the_ranks_converges_and_implies_the_data_covariances(case):
    shape, center, f32 = case
    m, ref = fitted(*case), host_fit(*case)
    X = data(shape, f32).astype(np.float64)                              # float32 input is widened
    assert list(m.kept_) == ref['kept'] and m.shape_ == shape
    assert [len(v) for v in m.eigvals_] == ref['kept'] and [q.shape for q in m.eigvecs_] == [(n, k) for n, k in zip(shape, m.kept_)]
    L = max(TR.terms(m.kept_)['w'])
    res = TR.residual(m.eigvals_, m.multipliers_)                         # long double, from what the fit returned
    assert res <= TOL + (L + 4) * U and m.residual_ <= TOL and 1 <= m.n_iter_ <= 40
    marg = TR.marginals(m.multipliers_)
    assert not marg['bad']
    worst = 0.0
    for r in range(3):
        # tol, plus the bar of the eigh_psd_batched tests (|V^T C V - diag(w)| <= 1e-10 w_0 elementwise: n 1e-10 in Frobenius norm)
        dev = TR.rel_fro(TR.implied_cov(m.eigvecs_[r], np.asarray(marg['w1'][r], dtype=np.float64)), TR.sigma(ref['R'], r))
        assert dev <= TOL + shape[r] * 1e-10, f'axis {r}: {dev:.3e}'
        worst = max(worst, dev)
        assert abs(m.eigvals_[r].sum() - m.total_) <= 1e-12 * m.total_
        assert np.abs(m.eigvecs_[r].T @ m.eigvecs_[r] - np.eye(m.kept_[r])).max() <= 1e-11
    assert abs(m.total_ - ref['total']) <= 1e-12 * ref['total']
    if center:
        # the mean tensor: three pairwise means of n <= 66 terms ((log2 n + 2) u <= 9 u each), three subtractions and X - R
        assert np.abs(m.mean_.cpu().numpy() - ref['M']).max() <= 32 * U * np.abs(X).max()
    else:
        assert m.mean_ is None
    print(f'{case_id(case)}: kept {m.kept_}, residual {res:.2e} after {m.n_iter_} launches, implied covariance off by {worst:.2e}')


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_sampling_a_given_z_is_the_restatements_map_within_the_chained_bar(case):
    shape, center, f32 = case
    m = fitted(*case)
    S = 2
    z = np.random.default_rng(3).standard_normal((S,) + tuple(m.kept_))
    M = np.zeros(shape) if m.mean_ is None else m.mean_.cpu().numpy()
    got = m.sample(S, z=z)
    assert tuple(got.shape) == (S,) + shape and got.dtype == torch_().float64 and got.is_cuda
    want, bar = TR.sample_map(z, m.multipliers_, m.eigvecs_, M)
    err = np.abs(got.cpu().numpy().astype(LD) - want)
    assert (err <= bar).all(), f'off by {float((err / bar).max()):.2f} bars'
    assert float(bar.max()) < 1e-9 * float(np.abs(want).max())
    # z = 0: the mean tensor of the data, exactly as the fit holds it
    zero = m.sample(1, z=np.zeros((1,) + tuple(m.kept_)))[0].cpu().numpy()
    assert np.array_equal(bits(zero), bits(M))
    # chunk budgets: one surrogate per chunk and all in one chunk, the same bits; a device z as well
    one = m.sample(S, z=torch_().from_numpy(z).cuda(), max_bytes=1)
    assert np.array_equal(bits(one.cpu().numpy()), bits(got.cpu().numpy()))
    print(f'{case_id(case)}: largest fraction of the bar {float((err / bar).max()):.2e}')


def test_the_same_seed_gives_the_same_bits_in_any_chunking_and_float32_is_the_rounded_float64():
    torch = torch_()
    m = fitted((6, 8, 4), True, False)
    a = m.sample(5, random_state=7)
    b = m.sample(5, random_state=7, max_bytes=1)
    c = m.sample(5, random_state=7, max_bytes=3 * 8 * (5 * 7 * 3 + 5 * 7 * 4 + 5 * 8 * 4))        # chunks of 3 and 2
    d = m.sample(5, random_state=8)
    assert torch.equal(a, b) and torch.equal(a, c) and not torch.equal(a, d)
    assert torch.equal(m.sample(3, random_state=7), a[:3])               # one draw per surrogate, in order
    f = m.sample(5, random_state=7, dtype=torch.float32)
    assert f.dtype == torch.float32 and torch.equal(f, a.to(torch.float32))
    g = SUR().tme_surrogates(data((6, 8, 4)), 5, random_state=7)
    assert torch.equal(g, a)
    assert torch.isfinite(a).all() and float(a.std()) > 0


def test_fit_many_is_three_fits_bit_for_bit():
    cases = [((6, 8, 4), True), ((66, 10, 34), True), ((6, 4, 6), True)]
    many = SUR().fit_many([data(s) for s, _ in cases])
    for m, (s, c) in zip(many, cases):
        one = fitted(s, c, False)
        assert m.kept_ == one.kept_ and m.n_iter_ == one.n_iter_ and m.residual_ == one.residual_ and m.total_ == one.total_
        for r in range(3):
            assert np.array_equal(bits(m.multipliers_[r]), bits(one.multipliers_[r]))
            assert np.array_equal(bits(m.eigvals_[r]), bits(one.eigvals_[r])) and np.array_equal(bits(m.eigvecs_[r]), bits(one.eigvecs_[r]))
        assert torch_().equal(m.mean_, one.mean_)


def test_an_unpreserved_axis_implies_a_multiple_of_the_identity():
    X = TR.random_tensor((6, 5, 4), 3)
    m = SUR().TME(preserve=(1,)).fit(X)
    ref = TR.fit(X, preserve=(1,))
    assert list(m.kept_) == ref['kept'] == [6, 4, 4]
    marg = TR.marginals(m.multipliers_)
    for r in (0, 2):
        assert np.array_equal(m.eigvecs_[r], np.eye(X.shape[r]))
        implied = TR.implied_cov(m.eigvecs_[r], np.asarray(marg['w1'][r], dtype=np.float64))
        assert TR.rel_fro(implied, np.eye(X.shape[r]) * m.total_ / X.shape[r]) <= TOL + (20 + 4) * U
    implied = TR.implied_cov(m.eigvecs_[1], np.asarray(marg['w1'][1], dtype=np.float64))
    assert TR.rel_fro(implied, TR.sigma(ref['R'], 1)) <= TOL + 5 * 1e-10
    S = m.sample(2, random_state=1)
    assert tuple(S.shape) == (2, 6, 5, 4)


def test_the_mean_covariances_of_4096_surrogates_are_the_datas():
    X = TR.random_tensor((6, 5, 4), 11)
    m = SUR().TME().fit(X)
    S = (m.sample(4096, random_state=2024) - m.mean_).cpu().numpy()
    R, _ = TR.center(X)
    worst = 0.0
    for r in range(3):
        A = np.moveaxis(S, r + 1, 1).reshape(4096, X.shape[r], -1)
        worst = max(worst, TR.rel_fro(np.einsum('sab,scb->ac', A, A) / 4096, TR.sigma(R, r)))
    print(f'largest relative Frobenius deviation {worst:.4f}, bound {STAT_BOUND:.4f}')
    assert worst <= STAT_BOUND
    # no stray mean: an element is a combination of the core with orthonormal weights, so its variance is at most max W and the
    # mean of 4096 of them lies within 6 standard deviations of zero
    assert np.abs(S.mean(axis=0)).max() <= 6 * np.sqrt(TR.weights(m.multipliers_).max() / 4096)


def test_a_fit_that_runs_out_of_iterations_raises_with_the_residual():
    with pytest.raises(RuntimeError, match=r'did not converge: largest relative residual \d\.\d{3}e[-+]\d\d after 2 iterations'):
        SUR().TME(max_iter=2).fit(data((6, 8, 4)))
