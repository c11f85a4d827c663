"""tests/svm_ref.py without a device: the restatement of the SMO kernel against closed forms, exact-arithmetic tie problems and libsvm;
the assertions of tests/test_gpu_svm_smo.py fed with wrong variants of the restatement, each of which they must reject; and the
preconditions of the trajectory cases (the float64 and the long-double restatement walk the same path, with a selection margin of
1e-9 at every choice after the structural tie of the first)."""
import numpy as np
import pytest

import svm_ref as R

PD = [s for s in R.CASES if R.problem(s).pd]


def restatement(p, mutant=None, cap=R.MAX_ITER):
    """``solve`` of check_problem / check_tie by (a variant of) the restatement.  ``cap``: a wrong variant need not converge."""
    def solve(max_iter):
        r = R.smo_ref(p.K, p.idx, p.npos, p.cb, R.EPS, min(max_iter, cap), mutant=mutant)
        return r.alpha, r.rho, r.iters
    return solve


# ================================================================================================ closed forms
@pytest.mark.parametrize('dtype', [np.float64, R.LD])
@pytest.mark.parametrize('C,free', [(10.0, True), (0.3, False)])
def test_two_points_closed_form(C, free, dtype):
    K = np.array([[2.0, 0.5, np.nan], [0.5, 1.5, np.nan]])
    want = min(C, 2 / (2.0 + 1.5 - 2 * 0.5))                              # 0.8 free, 0.3 clipped
    assert (want < C) == free
    r = R.smo_ref(K, [0, 1], 1, np.full(2, C), 1e-3, 100, dtype)
    assert r.iters == 1 and r.trace == [(0, 1)] and r.alpha.dtype == dtype
    np.testing.assert_allclose(r.alpha.astype(np.float64), [want, want], rtol=1e-15)
    G = np.array([-1 + want * (2.0 - 0.5), -1 + want * (1.5 - 0.5)])    # G = Q alpha - 1 with Q = [[2, -.5], [-.5, 1.5]]
    rho = (G[0] - G[1]) / 2                                               # free: the mean of y G; clipped: ub = -G_2, lb = G_1: the midpoint
    assert r.nfree == (2 if free else 0)
    assert abs(float(r.rho) - rho) <= 1e-15
    c = R.certificate(K, [0, 1], 1, np.full(2, C), r.alpha.astype(np.float64), float(r.rho))
    assert c.below == c.above == 0 and c.sum_y_alpha == 0 and c.rho_err <= 1e-15 and c.nfree == r.nfree
    assert abs(c.objective - (want * want * (2.0 + 1.5 - 1.0) / 2 - 2 * want)) <= 1e-15
    assert (abs(c.kkt_gap) <= 1e-15) if free else (c.kkt_gap < 0)


def test_seven_point_ties_in_exact_arithmetic():
    p = R.tie_problem('seven')
    r = R.smo_ref(p.K, p.idx, p.npos, p.cb, R.EPS, 100)
    assert r.trace == [(2, 6), (1, 5)] and r.iters == 2
    assert r.alpha.tolist() == [0, .25, .25, 0, 0, .25, .25] and r.rho == 1.0
    one = R.smo_ref(p.K, p.idx, p.npos, p.cb, R.EPS, 1)
    assert one.iters == 1 and one.alpha.tolist() == [0, 0, .25, 0, 0, 0, .25]
    assert r.margins[0, 0] == 0 and r.margins[0, 1] == 0                  # both choices of the first step ARE ties


def test_edge_and_tau_problems_in_exact_arithmetic():
    p = R.tie_problem('edges')
    r = R.smo_ref(p.K, p.idx, p.npos, p.cb, R.EPS, 100)
    assert r.trace == [(64, 256), (63, 255)] and np.flatnonzero(r.alpha).tolist() == [63, 64, 255, 256] and r.rho == 1.0
    assert (r.alpha[[63, 64, 255, 256]] == .25).all() and r.margins[0, 0] == 0 and r.margins[0, 1] == 0
    p = R.tie_problem('tau')
    r = R.smo_ref(p.K, p.idx, p.npos, p.cb, R.EPS, 100)
    assert r.trace == [(1, 2), (0, 3)] and r.tau_steps == 1 and r.alpha.tolist() == [.25] * 4 and r.rho == -0.5 and r.nfree == 0
    for name in R.TIES:                                                   # long double computes the same numbers: nothing is rounded
        p = R.tie_problem(name)
        a, b = R.smo_ref(p.K, p.idx, p.npos, p.cb, R.EPS, 100), R.smo_ref(p.K, p.idx, p.npos, p.cb, R.EPS, 100, R.LD)
        assert a.trace == b.trace == p.trace and (a.alpha == b.alpha).all() and a.rho == b.rho


# ================================================================================================ against libsvm
@pytest.mark.parametrize('spec', [(63, 21, 'lin_pd', 'large', 0), (255, 85, 'rbf', 'small', 1), (256, 85, 'rbf', 'mixed', 4),
                                  (513, 171, 'lin_sing', 'small', 10), (255, 85, 'lin_sing', 'mixed', 6)], ids=R.case_name)
def test_dual_objective_equals_libsvm(spec):
    """Two eps-KKT points of one convex problem: the objectives differ by at most eps * sum(cb).  The alphas are NOT compared: on
    a singular kernel they legitimately differ."""
    svm = pytest.importorskip('sklearn.svm')
    assert spec in R.CASES
    p, ref = R.problem(spec), R.reference(spec)
    keep = p.cb > 0                                                       # libsvm drops the points of zero weight
    C = R.BOUNDS[spec[3]]
    sub = p.idx[keep]
    y = np.where(np.arange(p.n) < p.npos, 1, -1)[keep]
    sk = svm.SVC(kernel='precomputed', C=C, tol=R.EPS).fit(p.K[np.ix_(sub, sub)], y, sample_weight=p.cb[keep] / C)
    alpha = np.zeros(p.n)
    alpha[np.flatnonzero(keep)[sk.support_]] = np.abs(sk.dual_coef_[0])
    mine = R.certificate(p.K, p.idx, p.npos, p.cb, ref.alpha, ref.rho)
    theirs = R.certificate(p.K, p.idx, p.npos, p.cb, alpha, -sk.intercept_[0])       # the decision is positive for y = +1
    print(f'{p.name}: objective {mine.objective!r} (libsvm {theirs.objective!r}), iterations {ref.iters} ({int(sk.n_iter_[0])}), '
          f'KKT gap {mine.kkt_gap:.3e} ({theirs.kkt_gap:.3e}), max |alpha - libsvm| {np.abs(alpha - ref.alpha).max():.3e}')
    assert abs(mine.objective - theirs.objective) <= R.EPS * p.cb.sum()
    R.check_certificate(p, ref.alpha, ref.rho, ref.iters)
    # libsvm's certificate: its Q rows are float32, so its gradient carries 2^-24 |K| per unit of alpha
    slack = 2.0 ** -24 * p.max_k * alpha.sum()
    assert theirs.below == 0 and theirs.above == 0 and theirs.sum_y_alpha <= 1e-9 * p.cb.max()
    assert theirs.kkt_gap <= R.EPS + slack and theirs.rho_err <= R.EPS + slack


# ================================================================================================ the assertions bite
def test_the_restatement_passes_every_assertion_of_the_gpu_test():
    for name in R.TIES:
        p = R.tie_problem(name)
        R.check_tie(p, restatement(p))
    worst = dict(excess=-np.inf, alpha_err=0.0, rho_err=0.0, s_case=0.0)
    for spec in R.CASES:
        p = R.problem(spec)
        out = R.check_problem(p, restatement(p))
        assert out.get('alpha_err', 0.0) == 0.0 and out.get('rho_err', 0.0) == 0.0
        worst = {k: max(v, out.get(k, v)) for k, v in worst.items()}
    print(f'the restatement itself: KKT excess over eps {worst["excess"]:.3e}, s_case {worst["s_case"]:.3e}')


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_a_wrong_rule_is_rejected_on_the_committed_problems(mutant):
    """A kernel with this fault would fail the GPU test: the same assertions, the same problems."""
    caught = []
    for name in R.TIES:
        p = R.tie_problem(name)
        try:
            R.check_tie(p, restatement(p, mutant, 3000))
        except AssertionError as e:
            caught.append(str(e))
    for spec in sorted(R.CASES, key=lambda s: R.reference(s).iters):
        if caught:
            break
        p = R.problem(spec)
        try:
            R.check_problem(p, restatement(p, mutant, 3000))
        except AssertionError as e:
            caught.append(str(e))
    print(f'{mutant}: {caught}')
    assert caught, f'no assertion notices {mutant}'


# ================================================================================================ what the cases cover
def test_the_committed_problems_cover_the_envelope():
    refs = {s: R.reference(s) for s in R.CASES}
    assert len(set(R.CASES)) == len(R.CASES) and 35 <= len(R.CASES) <= 50
    assert {s[0] for s in R.CASES} == set(R.SIZES)
    for n in R.SIZES:
        assert {s[1] for s in R.CASES if s[0] == n} >= ({1} if n == 2 else {1, 2} if n == 3 else {1, n // 3, n - 1})
    for kernel in R.KERNELS:
        assert {s[3] for s in R.CASES if s[2] == kernel} == set(R.BOUNDS)
    assert all(r.iters <= 2500 for r in refs.values())                   # every problem converges in a few thousand iterations
    for pd in (True, False):
        hit = np.sum([refs[s].branches for s in R.CASES if R.problem(s).pd == pd], axis=0)
        assert (hit > 0).all(), f'clipping branches taken (pd = {pd}): {hit}'
    assert sum(refs[s].tau_steps for s in R.CASES) >= 5                   # the quad <= 0 path, on the singular problems
    assert all(refs[s].tau_steps == 0 for s in PD)
    for pd in (True, False):                                              # both branches of calculate_rho
        assert {refs[s].nfree == 0 for s in R.CASES if R.problem(s).pd == pd} == {True, False}
    mixed = [R.problem(s) for s in R.CASES if s[3] == 'mixed']
    assert sum((p.cb == 0).any() and len(set(p.cb[p.cb > 0])) == 2 for p in mixed) >= 8      # zero bounds beside unequal C_i, C_j
    for s in R.CASES:
        p = R.problem(s)
        assert len(set(p.idx.tolist())) == p.n and (p.n < 63 or ((np.diff(p.idx) < 0).any() and (np.diff(p.idx) > 0).any()))


@pytest.mark.parametrize('spec', PD, ids=R.case_name)
def test_trajectory_preconditions(spec):
    """No case is skipped: the seeds in CASES are those for which this holds."""
    for m in (R.MAX_ITER,) + R.PREFIXES:
        a, b = R.reference(spec, m), R.reference(spec, m, R.LD)
        assert a.trace == b.trace and a.iters == b.iters
        assert R.support(a.alpha, R.problem(spec).cb) == R.support(b.alpha.astype(np.float64), R.problem(spec).cb)
    a = R.reference(spec)
    margins = a.margins
    # the first i and the first j choose among all G = -1: the rule decides, and both sides compute it exactly
    later = margins[1:, :2]
    print(f'{R.case_name(spec)}: {a.iters} iterations, least margin i {later[:, 0].min(initial=np.inf):.2e}, j {later[:, 1].min(initial=np.inf):.2e}, '
          f'stop {margins[:, 2].min(initial=np.inf):.2e}, s_case {R.sensitivity(spec):.2e}')
    assert (later >= R.MARGIN).all() and (margins[:, 2] >= R.MARGIN).all()


def test_the_front_end_problem_meets_the_preconditions():
    f = R.frontend_problem()
    K = R.rbf_kernel(f.X[f.keep], f.gamma)
    for q, (idx, npos, cb) in enumerate(f.pairs):
        a, b = R.smo_ref(K, idx, npos, cb, f.tol, R.MAX_ITER), R.smo_ref(K, idx, npos, cb, f.tol, R.MAX_ITER, R.LD)
        assert a.trace == b.trace and 8 < a.iters < 2500
        assert (a.margins[1:, :2] >= R.MARGIN).all() and (a.margins[:, 2] >= R.MARGIN).all()
        assert len(set(cb.tolist())) > 2                                  # class weights times integer sample weights
    assert len(f.pairs) == 3 and not f.keep.all()
