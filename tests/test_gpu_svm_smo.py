"""svm_smo_kernel (csrc/xps_svm.hip) on the MI355X, through the C ABI, against the float64 restatement of its rules and the
long-double certificate of tests/svm_ref.py.  The problems, the assertions and the proof that they bite (every rule of the kernel
changed once, and rejected) are in svm_ref.py / test_svm_ref_host.py; this file launches the kernel.

Every launch: outputs preset to NaN (iters to -7) between guard elements; K with a leading dimension above its width, and NaN in
the padding AND in every row and column that is not a point of the launch, so a wrong row, column or leading dimension reads NaN;
idx scattered and non-monotone; off[0] > 0, so a kernel that ignores the offset writes into a guard.

Which assertion catches which fault (the host test shows each on the committed problems):
  i choice, j choice        iters / alpha / the prefixes max_iter = 1, 2, 3, 5, 8 against the restatement (positive definite problems)
  both tie rules            'seven' and 'edges' bit for bit (i tie across the wave edge 63 | 64, j tie across the stride edge 255 | 256)
  stop rule                 iters against the restatement; the recomputed KKT gap <= eps + drift; one more iteration stops too
  TAU guard                 'tau' bit for bit (quad < 0); the singular problems take the quad <= 0 path 11 times under the certificate
  each clipping branch      0 <= alpha <= cb exactly (all eight are taken on the positive definite and on the singular problems)
  gradient update           the KKT gap and rho of the gradient recomputed from alpha, n = 65 .. 513: a stale G[t] at a wave or
                            a block-stride edge misses them by orders of magnitude
  rho, free mean / midpoint rho against calculate_rho on the recomputed gradient; problems with and without free points
  idx / ldk / kbase         NaN everywhere outside the points of the launch; multi-matrix launch against the single-matrix one

Measured on the MI355X (worst over the committed problems; the bounds are those of svm_ref.check_*):
  KKT gap of the recomputed gradient    below eps on all 47 problems: the largest excess over eps is -1.7e-06 (bound: + drift)
  rho against the recomputed gradient   <= 4.6e-13 (513-1-lin_sing-large-3, C = 1e3, drift 6.0e-11); <= 2.2e-14 on every other problem
  alpha against the restatement         <= 3.4e-13 (257-85-rbf-large-4: 1005 iterations, s_case 3.1e-13, tolerance 3.6e-09);
                                        <= 1.4e-15 on every other problem; the largest error / tolerance is 0.033
  rho against the restatement           <= 2.5e-14 (the same problem); <= 2.3e-16 on every other problem
  s_case                                0 to 3.1e-13 (4.5e-15 without 257-85-rbf-large-4)
  iterations, supports, prefixes        those of the restatement on all 29 positive definite problems
  front end (3 pairs, 58 to 107 iterations): alpha <= 6.7e-16, rho <= 5.3e-17 against tolerances of 9.8e-13 to 3.5e-12
"""
import functools
import types

import numpy as np
import pytest

import svm_ref as R

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 5
FIGURES = []


def dev():
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    return LA.device()


@functools.lru_cache(maxsize=None)
def on_device(kernel):
    import torch
    return torch.from_numpy(np.array(R.world(kernel))).to(dev())


def masked(K, rows):
    """K (a world's name or a host matrix) on the device with NaN in every row and column outside ``rows`` (and in the padding,
    where K has it already)."""
    import torch
    Kd = on_device(K) if isinstance(K, str) else torch.from_numpy(np.array(K)).to(dev())
    ix = torch.from_numpy(np.unique(rows).astype(np.int64)).to(Kd.device)
    out = torch.full_like(Kd, NAN)
    out[ix[:, None], ix[None, :]] = Kd[ix[:, None], ix[None, :]]
    return out


def launch(K_d, problems, max_iter=R.MAX_ITER, entry='xps_svm_smo_f64', kbase=None, kld=None):
    """One launch of ``problems`` (each with idx, npos, cb) on the device matrix K_d.  Returns per problem (alpha, rho, iters), after
    asserting that nothing outside the outputs of the launch was written."""
    import torch
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import call
    d = K_d.device
    P = len(problems)
    sizes = [len(p.idx) for p in problems]
    off = GUARD + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)           # off[0] = GUARD: the buffers start before the launch's part
    total = int(off[-1]) + GUARD
    idx = np.zeros(total, dtype=np.int32)
    cb = np.full(total, NAN)
    for p, o in zip(problems, off):
        idx[o:o + len(p.idx)], cb[o:o + len(p.idx)] = p.idx, p.cb
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)                   # noqa: E731
    idx_d, off_d, npos_d, cb_d = up(idx), up(off), up(np.array([p.npos for p in problems] + [0], dtype=np.int32)), up(cb)
    alpha = torch.full((total,), NAN, dtype=torch.float64, device=d)
    rho = torch.full((P + 2 * GUARD,), NAN, dtype=torch.float64, device=d)
    iters = torch.full((P + 2 * GUARD,), -7, dtype=torch.int32, device=d)
    tail = (idx_d.data_ptr(), off_d.data_ptr(), npos_d.data_ptr(), P, max(sizes + [1]), cb_d.data_ptr(), R.EPS, int(max_iter),
            alpha.data_ptr(), rho[GUARD:].data_ptr(), iters[GUARD:].data_ptr(), _dev.stream())
    if kbase is None:
        call(entry, K_d.data_ptr(), K_d.stride(0), *tail)
    else:
        call(entry, K_d.data_ptr(), kbase.data_ptr(), kld.data_ptr(), *tail)
    torch.cuda.synchronize()
    alpha, rho, iters = alpha.cpu().numpy(), rho.cpu().numpy(), iters.cpu().numpy()
    assert np.isnan(alpha[:GUARD]).all() and np.isnan(alpha[off[-1]:]).all(), 'alpha was written outside [off[0], off[P])'
    assert np.isnan(rho[:GUARD]).all() and np.isnan(rho[GUARD + P:]).all(), 'rho was written outside its P elements'
    assert (iters[:GUARD] == -7).all() and (iters[GUARD + P:] == -7).all(), 'iters was written outside its P elements'
    return [(alpha[off[q]:off[q + 1]].copy(), float(rho[GUARD + q]), int(iters[GUARD + q])) for q in range(P)]


@functools.lru_cache(maxsize=None)
def single(spec, max_iter=R.MAX_ITER):
    """A committed problem alone in its launch (computed once; the grouped launches are compared with it)."""
    p = R.problem(spec)
    return launch(masked(spec[2], p.idx), [p], max_iter)[0]


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope='module', autouse=True)
def report():
    yield
    if FIGURES:
        w = lambda k: max((f[k] for f in FIGURES if k in f), default=float('nan'))    # noqa: E731
        print(f'\nworst over {len(FIGURES)} problems: KKT excess over eps {w("excess"):.3e}; rho against the recomputed gradient '
              f'{w("rho_cert"):.3e}; against the restatement alpha {w("alpha_err"):.3e}, rho {w("rho_err"):.3e}; s_case {w("s_case"):.3e}; '
              f'largest error / tolerance {max((max(f["alpha_err"], f["rho_err"]) / f["tol"] for f in FIGURES if f.get("tol")), default=0):.3f}')


# ================================================================================================ the committed problems
@pytest.mark.parametrize('spec', R.CASES, ids=R.case_name)
def test_kernel_meets_the_certificate_and_the_restatement(spec):
    p = R.problem(spec)
    out = R.check_problem(p, lambda m: single(spec, m))
    FIGURES.append(out)
    print('  '.join(f'{k} {v:.3e}' if isinstance(v, float) else f'{k} {v}' for k, v in out.items()))


@pytest.mark.parametrize('name', sorted(R.TIES))
def test_tie_rules_and_tau_guard_bit_for_bit(name):
    p = R.tie_problem(name)
    R.check_tie(p, lambda m: launch(masked(p.K, p.idx), [p], m)[0])


@pytest.mark.parametrize('kernel', R.KERNELS)
def test_many_problems_in_one_launch_equal_one_launch_each_bit_for_bit(kernel):
    specs = [s for s in R.CASES if s[2] == kernel]
    ps = [R.problem(s) for s in specs]
    assert len({p.n for p in ps}) >= 6
    got = launch(masked(kernel, np.concatenate([p.idx for p in ps])), ps)
    again = launch(masked(kernel, np.concatenate([p.idx for p in ps])), ps)
    for s, g, h in zip(specs, got, again):
        alpha, rho, iters = single(s)
        assert iters == g[2] == h[2], R.case_name(s)
        np.testing.assert_array_equal(bits(g[0]), bits(alpha), err_msg=R.case_name(s))
        np.testing.assert_array_equal(bits(h[0]), bits(alpha), err_msg=R.case_name(s))
        assert bits(g[1]) == bits(rho) == bits(h[1]), R.case_name(s)


def test_multi_matrix_entry_gives_the_bits_of_the_single_matrix_entry():
    import torch
    specs = [(65, 21, 'rbf', 'mixed', 0), (257, 85, 'lin_pd', 'mixed', 0), (255, 85, 'lin_sing', 'mixed', 6), (3, 2, 'rbf', 'small', 0)]
    ps = [R.problem(s) for s in specs]
    mats = [masked(s[2], p.idx) for s, p in zip(specs, ps)]
    lead = torch.full((7,), NAN, dtype=torch.float64, device=mats[0].device)          # no matrix starts at element 0
    buf = torch.cat([lead] + [m.reshape(-1) for m in mats])
    base = np.cumsum([7] + [m.numel() for m in mats[:-1]]).astype(np.int64)
    order = [2, 0, 3, 1]                                                              # the problems do not follow their matrices
    kbase = torch.from_numpy(base[order]).to(buf.device)
    kld = torch.from_numpy(np.array([mats[q].stride(0) for q in order], dtype=np.int64)).to(buf.device)
    got = launch(buf, [ps[q] for q in order], entry='xps_svm_smo_multi_f64', kbase=kbase, kld=kld)
    for q, g in zip(order, got):
        alpha, rho, iters = single(specs[q])
        assert iters == g[2] and bits(g[1]) == bits(rho)
        np.testing.assert_array_equal(bits(g[0]), bits(alpha))


def test_no_problem_writes_nothing():
    p = R.problem((3, 2, 'rbf', 'small', 0))
    assert launch(masked(p.K, p.idx), []) == []


# ================================================================================================ through the front end
def test_svc_fit_is_the_restatement_pair_by_pair():
    """decoders.SVC on three classes with class weights and integer sample weights: n_iter_, the dual coefficients and the intercepts
    of every pair are those of the restatement on the pair problem that _ovo poses (sklearn's signs: the lower class positive,
    intercept_ = -rho), and every pair passes the certificate."""
    import torch
    from cross_patient_speech_decoding_amd import decoders
    from cross_patient_speech_decoding_amd.decoders import _ovo
    f = R.frontend_problem()
    svc = decoders.SVC(C=f.C, kernel='rbf', gamma=f.gamma, tol=f.tol, class_weight=f.class_weight).fit(f.X, f.y, sample_weight=f.w)
    X, y, w = f.X[f.keep], f.y[f.keep], f.w[f.keep]
    classes, yi = np.unique(y, return_inverse=True)
    prob = _ovo.pair_problems(yi, np.arange(len(y)), _ovo.class_weights(f.class_weight, classes, yi), w)
    cb_all = _ovo.bounds(f.C, prob)
    off = np.concatenate([[0], np.cumsum(prob['sizes'])])
    Xd = torch.from_numpy(np.ascontiguousarray(X)).to(dev())
    sq = _ovo.row_sq_norms(Xd)
    K = _ovo.kernel_matrix('rbf', f.gamma, Xd, sq, Xd, sq).cpu().numpy()              # the matrix the fit solved on, bit for bit
    assert np.abs(K - R.rbf_kernel(X, f.gamma)).max() <= 1e-13
    coef = svc.dual_coef_pairs_.cpu().numpy()
    assert coef.shape == (3, len(y)) and len(svc.n_iter_) == 3 and list(svc.classes_) == [3, 7, 9]
    for q, (idx, npos, cb) in enumerate(f.pairs):
        sl = slice(off[q], off[q + 1])
        np.testing.assert_array_equal(prob['idx'][sl], idx)                           # _ovo poses the problem the host test examined
        np.testing.assert_array_equal(cb_all[sl], cb)
        assert prob['npos'][q] == npos
        p = types.SimpleNamespace(name=f'pair {q}', K=K, idx=idx, npos=npos, cb=cb, n=len(idx), max_k=1.0)
        a, b = R.smo_ref(K, idx, npos, cb, f.tol, R.MAX_ITER), R.smo_ref(K, idx, npos, cb, f.tol, R.MAX_ITER, R.LD)
        assert a.trace == b.trace and (a.margins[1:, :2] >= R.MARGIN).all() and (a.margins[:, 2] >= R.MARGIN).all()
        s_case = max(float(np.abs(a.alpha - b.alpha).max()), float(abs(a.rho - b.rho)))
        tol = R.tolerance(p, s_case, a.iters)
        y_pair = np.where(np.arange(len(idx)) < npos, 1.0, -1.0)
        alpha = y_pair * coef[q, idx]
        rest = np.delete(coef[q], idx)
        ea, er = float(np.abs(alpha - a.alpha).max()), float(abs(-svc.intercept_[q] - a.rho))
        print(f'pair {q}: {a.iters} iterations, alpha error {ea:.3e}, rho error {er:.3e}, tolerance {tol:.3e}, s_case {s_case:.3e}')
        assert int(svc.n_iter_[q]) == a.iters
        assert (rest == 0).all() and R.support(alpha, cb) == R.support(a.alpha, cb)
        assert ea <= tol and er <= tol
        R.check_certificate(p, alpha, -float(svc.intercept_[q]), a.iters)
