"""surrogates/tme.py and its restatement without a device: tests/tme_ref.py's solver on every shape the GPU tests use, on an
ill-conditioned spectrum and with unpreserved axes; the covariance its multipliers imply against Sigma_r of the data; the kept
ranks; the host half of the package's Newton iteration fed with the restatement's long-double sums; the new prototypes; and every
argument refusal of the wrappers, raised before the device is looked for."""
import ctypes as C

import numpy as np
import pytest
import torch

import tme_ref as TR
import cross_patient_speech_decoding_amd as pkg
from cross_patient_speech_decoding_amd import _lib, surrogates
from cross_patient_speech_decoding_amd.alignment import _linalg as LA
from cross_patient_speech_decoding_amd.surrogates import tme

F64 = lambda v: np.asarray(v, dtype=np.float64)                          # noqa: E731


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Any look for the device fails the test: the refusals come first."""
    def boom(*a, **k):
        raise AssertionError('the device was looked for')
    monkeypatch.setattr(LA, 'device', boom)
    monkeypatch.setattr(LA, 'to_device', boom)


def check_fit(f, X, preserve=(0, 1, 2)):
    """The restatement's fit: converged to 1e-10, and Q_r diag(marginal) Q_r^T = Sigma_r to 1e-9 for every preserved axis; an
    unpreserved axis implies a multiple of the identity."""
    assert f['residual'] <= 1e-10 and TR.residual(f['lams'], f['ls']) <= 1.1e-10
    m = TR.marginals(f['ls'])
    assert not m['bad']
    for r in range(3):
        implied = TR.implied_cov(f['Qs'][r], F64(m['w1'][r]))
        if r in preserve:
            assert TR.rel_fro(implied, TR.sigma(f['R'], r)) <= 1e-9
        else:
            assert TR.rel_fro(implied, np.eye(X.shape[r]) * f['total'] / X.shape[r]) <= 1e-9
    for r in range(3):                                                   # the three constraint sets share their trace
        assert abs(f['lams'][r].sum() - f['total']) <= 1e-12 * f['total']


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('shape,center', TR.FITS, ids=[TR.fit_name(*c) for c in TR.FITS])
def test_the_restatement_converges_and_implies_the_data_covariances(shape, center):
    X = TR.random_tensor(shape, 1)
    f = TR.fit(X, center_=center)
    check_fit(f, X)
    if center:
        assert f['kept'] == [n - 1 for n in shape]                       # centring makes one eigenvalue per axis zero
        assert max(np.abs(f['R'].mean(axis=a)).max() for a in range(3)) <= 1e-13 * np.abs(X).max()
    print(f'{TR.fit_name(shape, center)}: kept {f["kept"]}, residual {f["residual"]:.2e} in {f["n_iter"]} evaluations')


def test_the_kept_boxes_are_the_boxes_of_the_kernel_tests():
    boxes = {tuple(TR.fit(TR.random_tensor(s, 1), center_=c)['kept']) for s, c in TR.FITS}
    assert boxes >= set(TR.BOXES)
    assert TR.fit(TR.random_tensor((1, 4, 6), 1), center_=False)['kept'] == [1, 4, 4]        # a short axis is rank deficient


def test_a_decayed_spectrum_of_condition_1e8_converges():
    X = TR.random_tensor((8, 7, 12), 2, decay=4.5)
    f = TR.fit(X, eig_tol=1e-14)
    assert f['lams'][2][0] / f['lams'][2][-1] >= 1e8
    check_fit(f, X)


@pytest.mark.parametrize('preserve', [(1,), (0, 2), (0, 1)])
def test_unpreserved_axes_get_the_identity_and_a_uniform_spectrum(preserve):
    X = TR.random_tensor((6, 5, 4), 3)
    f = TR.fit(X, preserve=preserve)
    for r in range(3):
        if r not in preserve:
            assert f['kept'][r] == X.shape[r] and np.array_equal(f['Qs'][r], np.eye(X.shape[r]))
            assert np.array_equal(f['lams'][r], np.full(X.shape[r], f['total'] / X.shape[r]))
    check_fit(f, X, preserve)


def test_exact_rational_sums_agree_with_the_long_double_sums():
    rng = np.random.default_rng(5)
    ls = [rng.integers(1, 9, size=n) for n in (3, 4, 2)]
    exact, ld = TR.exact_marginals(ls), TR.marginals([F64(v) for v in ls])
    for key in ('p01', 'p02', 'p12'):
        assert np.abs(exact[key] - ld[key]).max() <= 8 * 2.0 ** -64 * np.abs(exact[key]).max()
    for r in range(3):
        assert np.abs(exact['w1'][r] - ld['w1'][r]).max() <= 16 * 2.0 ** -64 * np.abs(exact['w1'][r]).max()
        assert np.abs(exact['w2'][r] - ld['w2'][r]).max() <= 16 * 2.0 ** -64 * np.abs(exact['w2'][r]).max()
    assert TR.terms((3, 4, 2)) == dict(w=[8, 6, 12], p01=2, p02=4, p12=3, sumlog=24)
    assert TR.marginals([F64([1.0]), F64([-3.0, 1.0]), F64([1.0])])['bad']


def test_the_sampling_map_is_the_kronecker_product_of_the_bases():
    rng = np.random.default_rng(6)
    k, n = (2, 3, 2), (3, 4, 3)
    Qs = [np.linalg.qr(rng.standard_normal((n[r], n[r])))[0][:, :k[r]] for r in range(3)]
    ls = [rng.uniform(0.5, 2.0, size=k[r]) for r in range(3)]
    z = rng.standard_normal((2,) + k)
    M = rng.standard_normal(n)
    S, bar = TR.sample_map(z, ls, Qs, M)
    kron = np.kron(np.kron(Qs[0], Qs[1]), Qs[2])
    for s in range(2):
        want = kron @ (z[s] * np.sqrt(TR.weights(ls))).reshape(-1) + M.reshape(-1)
        assert np.abs(F64(S[s]).reshape(-1) - want).max() <= 1e-14
    assert bar.shape == S.shape and (bar > 0).all() and bar.max() < 1e-13
    S0, _ = TR.sample_map(np.zeros_like(z), ls, Qs, M)
    assert np.array_equal(F64(S0[0]), M)                                 # z = 0: the mean tensor


# ------------------------------------------------------------------------------------------------ the package's host half
def test_keep_and_scale_is_the_restatements():
    rng = np.random.default_rng(7)
    ws = [np.sort(rng.uniform(0.1, 5.0, size=n))[::-1] for n in (6, 5, 4)]
    ws[1][-2:] = [1e-11 * ws[1][0], 0.0]
    for preserve in ((0, 1, 2), (1,), (0, 2)):
        a, b = tme.keep_and_scale(ws, (6, 5, 4), 7.5, preserve, 1e-10), TR.keep_and_scale(ws, (6, 5, 4), 7.5, preserve, 1e-10)
        assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    assert tme.keep_and_scale(ws, (6, 5, 4), 7.5, (0, 1, 2), 1e-10)[0] == [6, 3, 4]


@pytest.mark.parametrize('shape,center', [TR.FITS[0], TR.FITS[3], TR.FITS[4]], ids=lambda v: str(v))
def test_the_host_half_of_the_newton_iteration_converges_on_exact_sums(shape, center):
    """tme._Newton fed with the restatement's long-double sums in place of the kernel's."""
    X = TR.random_tensor(shape, 1)
    R, _ = TR.center(X, center)
    total = float((R * R).sum())
    kept, lams = tme.keep_and_scale([TR.eig_desc(TR.sigma(R, r))[0] for r in range(3)], shape, total, (0, 1, 2), 1e-10)
    s = tme._Newton(lams, 1e-9, 100)
    while not s.done:
        l = s.propose()
        m = TR.marginals(s.split(l))
        s.receive(l, np.concatenate([F64(v) for v in m['w1']]), np.concatenate([F64(v) for v in m['w2']]), F64(m['p01']),
                  F64(m['p02']), F64(m['p12']), float(m['sumlog']), float(m['bad']))
    assert s.n_iter <= 25 and s.cur['res'] <= 1e-9 and TR.residual(lams, s.split(s.l_eval)) <= 1e-9 + 1e-12
    assert all((v > 0).all() for v in s.split(s.cur['l']))               # the balanced gauge keeps every multiplier positive


def test_a_fit_that_cannot_converge_raises_with_the_residual():
    s = tme._Newton([np.array([1.0, 2.0]), np.array([3.0]), np.array([3.0])], 1e-9, 2)
    with pytest.raises(RuntimeError, match=r'did not converge: largest relative residual \d\.\d{3}e[-+]\d\d after 2 iterations'):
        while not s.done:
            l = s.propose()
            m = TR.marginals(s.split(l))
            s.receive(l, np.concatenate([F64(v) for v in m['w1']]), np.concatenate([F64(v) for v in m['w2']]), F64(m['p01']),
                      F64(m['p02']), F64(m['p12']), float(m['sumlog']), float(m['bad']))


def test_surrogates_per_chunk_counts_the_temporaries():
    assert tme.surrogates_per_chunk((6, 5, 4), (5, 4, 3), 8 * (60 + 80 + 100) * 3 + 7) == 3
    assert tme.surrogates_per_chunk((6, 5, 4), (5, 4, 3), 1) == 1


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_every_refusal_comes_before_the_device():
    X = TR.random_tensor((4, 3, 5), 0)
    assert pkg.TME is tme.TME is surrogates.TME and pkg.fit_many is tme.fit_many and pkg.tme_surrogates is tme.tme_surrogates
    for bad, text in ((X[0], '3-D tensor'), (X[None], '3-D tensor'), (torch.zeros(3, 4), '3-D tensor'),
                      (np.zeros((3, 0, 2)), 'empty axis'), (np.zeros((2, 1025, 2), dtype=np.float32), 'at most XPS_TME_MAX_AXIS = 1024'),
                      (np.where(X > 2.5, np.nan, X), 'not finite'), (np.where(X > 2.5, np.inf, X), 'not finite'),
                      (torch.full((2, 2, 2), float('nan')), 'not finite'), (np.ones((2, 2, 2), dtype=np.int64), 'float32 or float64'),
                      (torch.ones(2, 2, 2, dtype=torch.float16), 'float32 or float64')):
        for fn in (lambda x: tme.TME().fit(x), lambda x: tme.fit_many([X, x]), lambda x: tme.tme_surrogates(x, 2)):
            with pytest.raises(ValueError, match=text):
                fn(bad)
    for kw, text in ((dict(preserve=()), 'at least one axis'), (dict(preserve=(0, 3)), 'axes out of 0, 1, 2'),
                     (dict(preserve=(-1,)), 'axes out of 0, 1, 2'), (dict(preserve=(1.0,)), 'axes out of 0, 1, 2'),
                     (dict(preserve=2), 'sequence of axes'), (dict(eig_tol=0.0), 'eig_tol must lie in'), (dict(tol=1.5), 'tol must lie in'),
                     (dict(max_iter=0), 'max_iter must be an integer >= 1'), (dict(max_iter=2.5), 'max_iter must be an integer >= 1')):
        for fn in (lambda **k: tme.TME(**k).fit(X), lambda **k: tme.fit_many([X], **k), lambda **k: tme.tme_surrogates(X, 2, **k)):
            with pytest.raises(ValueError, match=text):
                fn(**kw)
    for n in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match='n must be an integer >= 1'):
            tme.tme_surrogates(X, n)
    with pytest.raises(RuntimeError, match=r'^Must call fit\(\) before sampling\.$'):
        tme.TME().sample(3)
    assert tme.fit_many([]) == []
    with pytest.raises(AssertionError, match='the device was looked for'):                 # a good call gets as far as the device
        tme.TME().fit(X)

    m = tme.TME()                                                        # a fitted model, as far as sample()'s checks read it
    m.shape_, m.kept_, m.mean_ = (4, 3, 5), (3, 2, 4), None
    m.eigvecs_, m.multipliers_ = [np.eye(n)[:, :k] for n, k in zip(m.shape_, m.kept_)], [np.ones(k) for k in m.kept_]
    for args, kw, text in (((0,), {}, 'n must be an integer >= 1'), ((2,), dict(z=np.zeros((2, 3, 2, 5))), r'z must have shape \(2, 3, 2, 4\)'),
                           ((2,), dict(z=torch.zeros(1, 3, 2, 4)), r'z must have shape \(2, 3, 2, 4\)'),
                           ((2,), dict(z=np.zeros((3, 2, 4))), r'z must have shape \(2, 3, 2, 4\)'),
                           ((2,), dict(dtype=torch.float16), 'dtype must be torch.float32 or torch.float64'),
                           ((2,), dict(max_bytes=0), 'max_bytes must be an integer >= 1'),
                           ((2,), dict(random_state='seed'), 'random_state must be None or an int')):
        with pytest.raises(ValueError, match=text):
            m.sample(*args, **kw)
    with pytest.raises(AssertionError, match='the device was looked for'):
        m.sample(2, z=np.zeros((2, 3, 2, 4)))


def test_the_device_wrappers_refuse_bad_tensors_without_a_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(LA, 'call', lambda name, *a: calls.append(name))
    v, Mx = torch.zeros(3, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64)      # host tensors: refused as they are
    pr = dict(l=[v, v, v], w1=[v, v, v], w2=[v, v, v], p01=Mx, p02=Mx, p12=Mx, scal=v[:2])
    with pytest.raises(ValueError, match='device vector'):
        LA.tme_kron_pass([pr])
    with pytest.raises(ValueError, match='three multiplier vectors'):
        LA.tme_kron_pass([dict(pr, l=[v, v])])
    with pytest.raises(ValueError, match='float64 device tensor'):
        LA.tme_core_scale(torch.zeros(1, 3, 3, 3, dtype=torch.float64), [v, v, v])
    with pytest.raises(ValueError, match='contiguous rows'):
        LA.tme_mode_product(Mx, Mx, torch.zeros(1, 3, 3, dtype=torch.float64))
    assert LA.tme_kron_pass([]) is None and calls == []


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_header_declares_the_entries_and_the_constants_match():
    sigs = _lib.SIGNATURES
    v, i, i64, sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
    assert sigs['xps_tme_kron_pass_f64'] == (i, [v, i, v, sz, v]) and sigs['xps_tme_kron_pass_f64_workspace'] == (sz, [i])
    assert sigs['xps_tme_core_scale_f64'] == (i, [v, i64, v, v, v, i, i, i, i64, v, i64, v])
    assert sigs['xps_tme_mode_product_f64'] == (i, [v, i64, i64, v, i64, i64, i, v, i64, v, i, i64, i64, i64, i, i, i64, v])
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name, value in (('XPS_TME_KRON_WORDS', LA.TME_KRON_WORDS), ('XPS_TME_MAX_AXIS', LA.TME_MAX_AXIS)):
        assert f'#define {name} {value}\n' in header
    assert LA.KP_SCAL < LA.TME_KRON_WORDS and tme.MAX_AXIS == 1024
