"""tests/tsne_ref.py, the restatement the GPU t-SNE tests compare against, held to sklearn itself on the CPU: the perplexity search
and the joint probabilities against ``_utils._binary_search_perplexity`` / ``_t_sne._joint_probabilities`` on the same float32
distances, gradient and error against ``_t_sne._kl_divergence``, ten iterations and a 5 + 5 phase change against
``_t_sne._gradient_descent``, and ``n_iter_`` of a frozen problem against ``TSNE(method='exact')``.  No device is touched.

sklearn adds in numpy's / BLAS's order, so a comparison allows the restatement's bar (the kernels' order) plus the same bar
with m u for a sum of m terms (any order)."""
import numpy as np
import pytest
from scipy.spatial.distance import squareform
from sklearn.manifold import TSNE, _t_sne, _utils

import tsne_ref as TR

CASES = TR.cases()
NAMES = sorted(CASES)
_cache = {}


def affinities(name):
    """(d2 float32, Search, P) of a case, computed once and left unchanged."""
    if name not in _cache:
        X, perp = CASES[name]
        d2 = TR.sqdist_f32(X)
        sr = TR.search(d2, perp)
        _cache[name] = (d2, sr, TR.joint(sr.C, sr.rowsum))
    return _cache[name]


def any_order(n):
    return TR.sum_bar(n, 'any') / TR.sum_bar(n)


def test_wave_sum_is_the_lane_strided_butterfly():
    rng = np.random.default_rng(0)
    for m in (1, 5, 64, 65, 130, 200):
        t = rng.standard_normal(m)
        lanes = [0.0] * 64
        for j in range(m):
            lanes[j % 64] = lanes[j % 64] + t[j]
        for o in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
        assert TR.wave_sum(t) == lanes[0] and len(set(lanes)) == 1
    assert TR.wave_sum(rng.standard_normal((3, 70))).shape == (3,)


@pytest.mark.parametrize('name', NAMES)
def test_search_and_joint_probabilities_are_sklearns(name):
    X, perp = CASES[name]
    d2, sr, P = affinities(name)
    n = len(d2)
    C_sk = _utils._binary_search_perplexity(d2, perp, 0)
    decided = ~sr.undecided
    assert sr.undecided.sum() <= 0.02 * n
    bar = sr.C_bar * (1.0 + any_order(n))
    err = np.abs(sr.C - C_sk)[decided]
    print(f'{name}: C off by {err.max():.2e}; smallest search margin {sr.margin.min():.2e}, largest entropy bar '
          f'{sr.entropy_bar.max():.2e}; undecided rows {int(sr.undecided.sum())}; exhausted {int((sr.steps == 100).sum())}')
    assert (err <= bar[decided]).all()
    P_sk = squareform(_t_sne._joint_probabilities(d2.astype(np.float64), perp, 0))
    assert np.isfinite(P).all() and np.array_equal(P, P.T) and (np.diag(P) == 0).all()
    both = decided[:, None] & decided[None, :]
    pbar = TR.joint_bar(sr) * (1.0 + any_order(n))
    assert (np.abs(P - P_sk)[both] <= pbar[both]).all(), np.abs(P - P_sk)[both].max()
    clamped = (sr.C + sr.C.T) / (2 * sr.rowsum.sum()) < TR.EPS / 2
    np.fill_diagonal(clamped, False)
    assert (P[clamped] == TR.EPS).all()


def test_the_degenerate_case_takes_the_zero_sum_branch_and_exhausts_13_rows():
    d2, sr, P = affinities('n130_D10_degenerate')
    exhausted = np.nonzero(sr.steps == 100)[0]
    # row 7 (every exp underflows) and the twelve identical rows (eleven neighbours at distance 0: entropy >= log 11 > log 5)
    assert list(exhausted) == [7] + list(range(20, 32))
    # row 7 walks along float64's underflow boundary (its exps are subnormal where the perplexity would be met): reported, not held
    assert list(np.nonzero(sr.undecided)[0]) == [7]
    assert np.isfinite(P).all() and (P[7, np.arange(130) != 7] < 1e3 * TR.EPS).all()


@pytest.mark.parametrize('name', NAMES)
def test_the_long_double_twin_takes_the_same_steps(name):
    d2, sr, _ = affinities(name)
    ld = TR.search(d2, CASES[name][1], TR.LD)
    decided = ~sr.undecided
    assert np.array_equal(ld.steps[decided], sr.steps[decided])
    assert (np.abs(np.asarray(ld.C, np.float64) - sr.C)[decided] <= sr.C_bar[decided]).all()


@pytest.mark.parametrize('nc', [1, 2])
@pytest.mark.parametrize('exag', [1.0, 12.0])
@pytest.mark.parametrize('name', NAMES)
def test_gradient_and_error_are_sklearns_kl_divergence(name, exag, nc):
    _, _, P = affinities(name)
    n = len(P)
    rng = np.random.default_rng(3)
    Y = rng.standard_normal((n, nc)) * 2.0
    pt = TR.partials(P, Y, True)
    Z, grad, err = TR.objective(pt, exag)
    bars = TR.partials_bars(P, Y)
    _, dg, derr = TR.objective_bars(pt, bars, exag)
    kl, g_sk = _t_sne._kl_divergence(Y.ravel().copy(), squareform(P) * exag, 1, n, nc)
    g_sk = g_sk.reshape(n, nc)
    scale = 1.0 + any_order(n)
    assert (np.abs(grad[:, :nc] - g_sk) <= dg[:, :nc] * scale).all(), (np.abs(grad[:, :nc] - g_sk) / dg[:, :nc]).max()
    assert abs(err - kl) <= derr * scale, (err, kl, derr)
    # the long-double twin lies within the bar itself
    ptl = TR.partials(P, Y, True, TR.LD)
    Zl, gl, el = TR.objective(ptl, exag, TR.LD)
    assert (np.abs(np.asarray(gl, np.float64) - grad) <= dg).all() and abs(float(el) - err) <= derr


def _sklearn_descent(P, Y0, nc, lr, plan):
    """plan: [(it, max_iter, momentum, exaggeration)] -> the embedding after every phase."""
    n = len(P)
    p, out = Y0.ravel().copy(), []
    for it, max_iter, momentum, exag in plan:
        p, _, last = _t_sne._gradient_descent(_t_sne._kl_divergence, p, it=it, max_iter=max_iter, n_iter_check=50,
                                              momentum=momentum, learning_rate=lr, min_grad_norm=1e-7,
                                              args=[squareform(P) * exag, 1, n, nc], kwargs={})
        assert last == max_iter - 1
        out.append(p.reshape(n, nc).copy())
    return out


@pytest.mark.parametrize('nc', [1, 2])
@pytest.mark.parametrize('name', NAMES)
def test_ten_iterations_and_a_phase_change_are_sklearns_gradient_descent(name, nc):
    _, _, P = affinities(name)
    n = len(P)
    lr = max(n / 12.0 / 4.0, 50.0)
    Y0 = TR.random_init(n, nc, 7)
    for plan in ([(0, 10, 0.5, 12.0)], [(0, 5, 0.5, 12.0), (5, 10, 0.8, 1.0)]):
        runs = {}
        for dt in (np.float64, TR.LD):
            traj, Yin, und = [], Y0, []
            for it, max_iter, momentum, exag in plan:
                ph = TR.Descent(P, Yin, nc, it, max_iter, momentum, exag, lr, dtype=dt, track=dt is np.float64).run(max_iter - it)
                assert ph.done and ph.it == max_iter - 1
                traj, Yin, und = traj + ph.trajectory, ph.Y_out, und + ph.undecided
            runs[dt] = traj
            if dt is np.float64:
                frac = np.mean([u.mean() for u in und])
                assert frac == 0.0, f'{frac:.3%} of the gains elements are too close to call'
        bars = TR.trajectory_bars(runs[np.float64], runs[TR.LD])
        ends = np.cumsum([m - i for i, m, _, _ in plan]) - 1
        for Y_sk, t in zip(_sklearn_descent(P, Y0, nc, lr, plan), ends):
            gap = np.abs(runs[np.float64][t] - Y_sk).max()
            assert gap <= bars[t], (t, gap, bars[t])


def test_a_frozen_problem_stops_at_the_first_check_of_each_phase_as_sklearn_does():
    X, perp = CASES['n64_D10']
    _, _, P = affinities('n64_D10')
    init = np.full((64, 2), 0.25)
    sk = TSNE(method='exact', init=init.copy(), perplexity=perp).fit(X.astype(np.float64))
    Y, kl, n_iter = TR.fit(P, init, 2)
    assert sk.n_iter_ == 99 and n_iter == sk.n_iter_
    assert np.array_equal(Y, init) and np.array_equal(sk.embedding_, init)
    pt = TR.partials(P, init, True)
    _, _, derr = TR.objective_bars(pt, TR.partials_bars(P, init), 1.0)
    assert abs(kl - sk.kl_divergence_) <= derr * (1.0 + any_order(64))
