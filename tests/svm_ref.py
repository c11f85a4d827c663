"""A plain numpy restatement of the SMO kernel of csrc/xps_svm.hip (svm_smo_kernel: libsvm's Solver without shrinking), a certificate
that judges a solution from alpha alone, the committed problems the GPU test runs, and the assertions it makes on them.  Nothing here
imports the package; the host test (test_svm_ref_host.py) feeds the same assertions with wrong variants of the restatement, the GPU
test (test_gpu_svm_smo.py) feeds them with the kernel.

A problem: points idx[0..n) of a kernel matrix K, the first npos of them y = +1, the others y = -1, per-point bound cb.  It solves
min alpha' Q alpha / 2 - sum alpha, 0 <= alpha <= cb, y' alpha = 0 with Q = y y' K.  The rules, each once (Fan, Chen & Lin 2005):

  i      the maximum of -y G over I_up  = {y = +1, alpha < cb} + {y = -1, alpha > 0}
  j      the maximum of grad_diff^2 / quad over I_low = {y = +1, alpha > 0} + {y = -1, alpha < cb} with grad_diff = Gmax + y_t G_t > 0,
         quad = K_ii + K_tt - 2 y_i y_t K_it, quad <= 0 -> TAU = 1e-12
  ties   to the LARGER index, in both
  stop   Gmax + Gmax2 < eps (Gmax2: the maximum of y G over I_low) or no j
  step   libsvm's two-variable update, clipped to the box in eight branches (numbered 0..7 in ``_step``)
  G      G_t += y_i y_t K_it d alpha_i + y_j y_t K_jt d alpha_j, element by element: no sums
  rho    calculate_rho: the mean of y G over the free points; none free: (ub + lb) / 2

u = 2^-52 below is the spacing of float64 at 1."""
import functools
import types

import numpy as np

LD = np.longdouble
U = 2.0 ** -52
TAU = 1e-12
NEG = -1e300
EPS = 1e-3                                                   # the tolerance of every committed problem (sklearn's default tol)
MAX_ITER = 20000                                             # nothing committed needs more than a few thousand
PREFIXES = (1, 2, 3, 5, 8)
MARGIN = 1e-9                                                # the least selection margin of a trajectory case (host test)


# ------------------------------------------------------------------------------------------------ the restatement
def _pick(v, mask, smaller):
    """(index, relative gap to the second best) of the maximum of v over mask; ties to the larger index (``smaller``: a mutant)."""
    c = np.flatnonzero(mask)
    if not len(c):
        return -1, np.inf
    vals = v[c]
    best = vals.max()
    w = c[vals == best]
    k = int(w[0] if smaller else w[-1])
    rest = vals[c != k]
    if not len(rest):
        return k, np.inf
    second = rest.max()
    scale = max(abs(float(best)), abs(float(second)), 1e-300)
    return k, float(best - second) / scale


def _step(yi, yj, Gi, Gj, ai, aj, Ci, Cj, quad, drop, equal_c):
    """libsvm's clipped two-variable update; returns (alpha_i, alpha_j, branches taken).  ``drop``: the branch a mutant leaves out;
    ``equal_c``: a mutant that clips as if C_i == C_j."""
    hit = []

    def take(b):
        hit.append(b)
        return b != drop
    zero = ai * 0
    if yi != yj:
        delta = (-Gi - Gj) / quad
        diff = ai - aj
        ai, aj = ai + delta, aj + delta
        if diff > 0:
            if aj < 0 and take(0):
                aj, ai = zero, diff
        elif ai < 0 and take(1):
            ai, aj = zero, -diff
        if diff > (zero if equal_c else Ci - Cj):
            if ai > Ci and take(2):
                ai, aj = Ci, Ci - diff
        elif aj > Cj and take(3):
            aj, ai = Cj, Cj + diff
    else:
        delta = (Gi - Gj) / quad
        tot = ai + aj
        ai, aj = ai - delta, aj + delta
        if tot > Ci:
            if ai > Ci and take(4):
                ai, aj = Ci, tot - Ci
        elif aj < 0 and take(5):
            aj, ai = zero, tot
        if tot > (Ci if equal_c else Cj):
            if aj > Cj and take(6):
                aj, ai = Cj, tot - Cj
        elif ai < 0 and take(7):
            ai, aj = zero, tot
    return ai, aj, hit


def calculate_rho(alpha, G, cb, pos, always_free_mean=False):
    """libsvm's calculate_rho; returns (rho, number of free points)."""
    yG = np.where(pos, G, -G)
    upper = alpha >= cb
    lower = ~upper & (alpha <= 0)
    free = ~upper & ~lower
    to_ub = (upper & ~pos) | (lower & pos)
    to_lb = (upper & pos) | (lower & ~pos)
    ub = yG[to_ub].min() if to_ub.any() else alpha.dtype.type(-NEG)
    lb = yG[to_lb].max() if to_lb.any() else alpha.dtype.type(NEG)
    nfree = int(free.sum())
    if nfree > 0 or always_free_mean:
        with np.errstate(all='ignore'):
            return yG[free].sum() / alpha.dtype.type(nfree), nfree
    return (ub + lb) / 2, nfree


MUTANTS = ('first_order_j', 'ties_smaller', 'no_gmax2', 'equal_c', 'rho_free_mean', 'no_tau', 'stale_256', 'stale_wave') + tuple(
    f'drop_clip{b}' for b in range(8))


def smo_ref(K, idx, npos, cb, eps, max_iter, dtype=np.float64, mutant=None, alpha0=None, G0=None):
    """The kernel's iteration in ``dtype``.  Returns alpha, rho, iters, trace [(i, j)], margins (one row per selection that led to a
    step: the relative gap of the i choice, of the j choice, |Gmax + Gmax2 - eps|; for the selection that stopped the run, whose
    choices decide nothing, (inf, inf, |Gmax + Gmax2 - eps|)), nfree, ``branches`` (how often each clipping branch was taken) and
    ``tau_steps`` (the steps whose quad was <= 0).
    ``mutant``: one rule changed (MUTANTS), for the host test only.  ``alpha0`` / ``G0``: the state to start from (default 0 / -1)."""
    assert mutant is None or mutant in MUTANTS
    idx = np.asarray(idx)
    n = len(idx)
    Ks = np.asarray(K)[np.ix_(idx, idx)].astype(dtype)
    cb = np.asarray(cb).astype(dtype)
    t_ = np.arange(n)
    pos = t_ < npos
    y = np.where(pos, 1, -1).astype(dtype)
    diag = Ks.diagonal().copy()
    alpha = np.zeros(n, dtype) if alpha0 is None else np.asarray(alpha0).astype(dtype)
    G = -np.ones(n, dtype) if G0 is None else np.asarray(G0).astype(dtype)
    smaller = mutant == 'ties_smaller'
    drop = int(mutant[-1]) if mutant and mutant.startswith('drop_clip') else -1
    trace, margins, branches, tau_steps = [], [], [0] * 8, 0
    it = 0
    while it < max_iter:
        v = np.where(pos, -G, G)
        i, gap_i = _pick(v, np.where(pos, alpha < cb, alpha > 0), smaller)
        if i < 0:
            break
        Gmax, yi = v[i], y[i]
        low = np.where(pos, alpha > 0, alpha < cb)
        yG = np.where(pos, G, -G)
        Gmax2 = yG[low].max() if low.any() else dtype(NEG)
        grad_diff = Gmax + yG
        Qi = yi * y * Ks[i]
        quad = np.where(pos, diag[i] + diag - 2.0 * yi * Qi, diag[i] + diag + 2.0 * yi * Qi)
        cand = low & (grad_diff > 0)
        with np.errstate(all='ignore'):
            gain = grad_diff * grad_diff / (quad if mutant == 'no_tau' else np.where(quad > 0, quad, dtype(TAU)))
        j, gap_j = _pick(yG if mutant == 'first_order_j' else gain, cand, smaller)
        stop_margin = abs(float(Gmax + Gmax2) - eps)
        if (Gmax < eps if mutant == 'no_gmax2' else Gmax + Gmax2 < eps) or j < 0:
            margins.append((np.inf, np.inf, stop_margin))
            break
        margins.append((gap_i, gap_j, stop_margin))
        trace.append((i, j))
        yj = y[j]
        q = diag[i] + diag[j] + 2.0 * (yi * yj * Ks[i, j]) if yi != yj else diag[i] + diag[j] - 2.0 * (yi * yj * Ks[i, j])
        if q <= 0:
            tau_steps += 1
            if mutant != 'no_tau':
                q = dtype(TAU)
        with np.errstate(all='ignore'):
            ai, aj, hit = _step(yi, yj, G[i], G[j], alpha[i], alpha[j], cb[i], cb[j], q, drop, mutant == 'equal_c')
        for b in hit:
            branches[b] += 1
        dai, daj = ai - alpha[i], aj - alpha[j]
        alpha[i], alpha[j] = ai, aj
        with np.errstate(all='ignore'):
            dG = yi * y * Ks[i] * dai + yj * y * Ks[j] * daj
        if mutant == 'stale_256':
            dG[256:] = 0
        if mutant == 'stale_wave':
            dG[64::64] = 0
        G += dG
        it += 1
    rho, nfree = calculate_rho(alpha, G, cb, pos, mutant == 'rho_free_mean')
    return types.SimpleNamespace(alpha=alpha, rho=rho, iters=it, trace=trace, margins=np.array(margins, dtype=np.float64).reshape(-1, 3),
                                 nfree=nfree, branches=branches, tau_steps=tau_steps, G=G)


# ------------------------------------------------------------------------------------------------ the certificate
def certificate(K, idx, npos, cb, alpha, rho):
    """Judges (alpha, rho) in long double from alpha alone: G = Q alpha - 1 recomputed, the number of alpha < 0 and of alpha > cb,
    |sum y alpha|, the KKT gap max_{I_up}(-y G) - min_{I_low}(-y G) (-inf where a set is empty), calculate_rho on the recomputed G
    and its distance to ``rho``, the number of free points and the dual objective."""
    idx = np.asarray(idx)
    n = len(idx)
    Ks = np.asarray(K)[np.ix_(idx, idx)].astype(LD)
    a, cb = np.asarray(alpha).astype(LD), np.asarray(cb).astype(LD)
    pos = np.arange(n) < npos
    y = np.where(pos, 1, -1).astype(LD)
    Qa = y * (Ks @ (y * a))
    G = Qa - 1
    up = np.where(pos, a < cb, a > 0)
    low = np.where(pos, a > 0, a < cb)
    myG = -y * G
    gap = float(myG[up].max() - myG[low].min()) if up.any() and low.any() else -np.inf
    rho_c, nfree = calculate_rho(a, G, cb, pos)
    return types.SimpleNamespace(G=G, below=int((a < 0).sum()), above=int((a > cb).sum()), sum_y_alpha=float(abs((y * a).sum())),
                                 kkt_gap=gap, rho=rho_c, rho_err=float(abs(LD(rho) - rho_c)), nfree=nfree,
                                 objective=float(a @ Qa / 2 - a.sum()))


# ------------------------------------------------------------------------------------------------ the committed problems
# One world of 2 x HALF points per kernel: rows [0, HALF) are class A (shifted by SHIFT[kernel] along the first axis), rows [HALF, 2 HALF)
# class B.  A problem draws its npos positives from A and the others from B, in a scattered order.  'rbf': 5 features, strictly
# positive definite.  'lin_pd': linear with D_PD >= every n features: positive definite.  'lin_sing': linear with 3 features: singular
# from n = 4 on; the second half of each class repeats the first half, and the first TWINS points of B are the first TWINS points of A,
# so a problem holds duplicated rows within a class and across the classes (quad = 0 with grad_diff > 0: the TAU path).
HALF, PAD, D_PD, TWINS = 520, 3, 520, 64
SHIFT = {'rbf': 2.5, 'lin_pd': 1.5, 'lin_sing': 3.0}
KERNELS = ('rbf', 'lin_pd', 'lin_sing')
BOUNDS = {'small': 0.1, 'large': 1e3, 'mixed': 0.5}          # uniform C; 'mixed': C * integers(0, 3) per point
SIZES = (2, 3, 63, 64, 65, 255, 256, 257, 513)

# (n, npos, kernel, bounds, seed).  Every size with npos in {1, n / 3, n - 1}, the three kernels and the three bounds, thinned; the
# seeds are those for which the preconditions of test_svm_ref_host.py hold and, for 'mixed', something moves.  From n = 63 on
# npos = 1 comes with the singular kernel only, which is held to the certificate and not to the trajectory: with one positive point,
# I_up is that point plus the few negatives with alpha > 0, an unclipped step leaves -y G of its two points EQUAL up to rounding, and
# as nothing else in so small a set lies above them, the next i is decided by the last bit (margins of 0 to 2e-16 for each of 40
# seeds of four such problems): no arithmetic fixes the trajectory there.  The rule chooses j by the gain, not by the value, so
# npos = n - 1 has no such tie.  The singular kernel with the large C and n / 3 positives from n = 255 on does not converge in 20000
# iterations and is left out: every committed problem takes 0 to 1005 iterations in the restatement.
CASES = (
    (2, 1, 'rbf', 'small', 0), (2, 1, 'rbf', 'large', 0), (2, 1, 'lin_pd', 'mixed', 0), (2, 1, 'lin_sing', 'small', 0),
    (3, 1, 'rbf', 'mixed', 0), (3, 2, 'rbf', 'small', 0), (3, 2, 'lin_sing', 'large', 0), (3, 1, 'lin_pd', 'small', 0),
    (63, 1, 'lin_sing', 'small', 0), (63, 21, 'lin_pd', 'large', 0), (63, 62, 'rbf', 'mixed', 1), (63, 21, 'lin_sing', 'mixed', 0),
    (63, 1, 'lin_sing', 'large', 0), (63, 62, 'lin_pd', 'small', 0),
    (64, 21, 'rbf', 'large', 0), (64, 63, 'lin_pd', 'small', 0), (64, 1, 'lin_sing', 'mixed', 0), (64, 63, 'lin_sing', 'large', 0),
    (64, 63, 'rbf', 'mixed', 1),
    (65, 21, 'rbf', 'mixed', 0), (65, 64, 'rbf', 'large', 0), (65, 1, 'lin_sing', 'small', 0), (65, 21, 'lin_pd', 'small', 0),
    (65, 64, 'lin_sing', 'mixed', 4),
    (255, 85, 'rbf', 'small', 1), (255, 254, 'lin_pd', 'mixed', 3), (255, 1, 'lin_sing', 'large', 0), (255, 254, 'rbf', 'large', 1),
    (255, 85, 'lin_sing', 'mixed', 6),
    (256, 85, 'lin_pd', 'large', 0), (256, 255, 'rbf', 'small', 1), (256, 1, 'lin_sing', 'mixed', 0), (256, 85, 'rbf', 'mixed', 4),
    (257, 85, 'rbf', 'large', 4), (257, 1, 'lin_sing', 'small', 0), (257, 256, 'lin_sing', 'small', 0), (257, 85, 'lin_pd', 'mixed', 0),
    (257, 256, 'rbf', 'large', 0), (257, 85, 'rbf', 'small', 0),
    (513, 171, 'rbf', 'mixed', 5), (513, 512, 'lin_pd', 'large', 0), (513, 1, 'lin_sing', 'large', 1), (513, 1, 'lin_sing', 'large', 3), (513, 171, 'lin_sing', 'small', 10),
    (513, 171, 'lin_pd', 'small', 0), (513, 512, 'rbf', 'small', 0), (513, 171, 'lin_sing', 'mixed', 0),
)


def case_name(spec):
    return '-'.join(str(s) for s in spec)


@functools.lru_cache(maxsize=None)
def world(kernel):
    """The kernel matrix of a world, (2 HALF, 2 HALF + PAD) with NaN in the padding columns.  Not to be written to."""
    rng = np.random.default_rng(KERNELS.index(kernel) + 40)
    d = {'rbf': 5, 'lin_pd': D_PD, 'lin_sing': 3}[kernel]
    X = rng.standard_normal((2 * HALF, d))
    if kernel == 'lin_pd':
        X /= np.sqrt(d)
    if kernel == 'lin_sing':
        q = HALF // 2
        X[q:HALF] = X[:q]
        X[HALF + q:] = X[HALF:HALF + q]
    X[:HALF, 0] += SHIFT[kernel]
    if kernel == 'lin_sing':
        X[HALF:HALF + TWINS] = X[:TWINS]
    G = X @ X.T
    if kernel == 'rbf':
        sq = np.diagonal(G)
        G = np.exp(-0.3 * np.maximum(sq[:, None] + sq[None, :] - 2 * G, 0))
    K = np.full((2 * HALF, 2 * HALF + PAD), np.nan)
    K[:, :2 * HALF] = (G + G.T) / 2
    K.setflags(write=False)
    return K


@functools.lru_cache(maxsize=None)
def problem(spec):
    """The problem of a CASES entry: K (its world), idx (scattered and non-monotone), npos, cb, pd (positive definite: a trajectory
    case) and max_k = max |K| over its points."""
    n, npos, kernel, bounds, seed = spec
    rng = np.random.default_rng([n, npos, KERNELS.index(kernel), sorted(BOUNDS).index(bounds), seed])
    K = world(kernel)
    if kernel == 'lin_sing':                                 # rows r and r + HALF / 2 of a class are the same point: draw both
        def draw(m, base):
            first = rng.permutation(HALF // 2)[:(m + 1) // 2]
            return rng.permutation(np.concatenate([first, first[:m // 2] + HALF // 2])) + base
    else:
        def draw(m, base):
            return rng.permutation(HALF)[:m] + base
    idx = np.concatenate([draw(npos, 0), draw(n - npos, HALF)]).astype(np.int32)
    C = BOUNDS[bounds]
    cb = C * rng.integers(0, 3, n).astype(np.float64) if bounds == 'mixed' else np.full(n, C)
    cb.setflags(write=False)
    return types.SimpleNamespace(spec=spec, name=case_name(spec), K=K, idx=idx, npos=npos, cb=cb, pd=kernel != 'lin_sing', n=n,
                                 max_k=float(np.abs(K[np.ix_(idx, idx)]).max()))


@functools.lru_cache(maxsize=None)
def reference(spec, max_iter=MAX_ITER, dtype=np.float64):
    """The restatement on a committed problem, computed once and shared; not to be written to."""
    p = problem(spec)
    return smo_ref(p.K, p.idx, p.npos, p.cb, EPS, max_iter, dtype)


def sensitivity(spec, max_iter=MAX_ITER):
    """s_case: how far the float64 and the long-double restatement of a problem are apart, in alpha and in rho."""
    a, b = reference(spec, max_iter), reference(spec, max_iter, LD)
    return max(float(np.abs(a.alpha - b.alpha).max()), float(abs(a.rho - b.rho)))


# The exact-arithmetic problems: linear kernel on points with coordinates 0 and 2, cb = 0.25.  Every quantity is a small dyadic number
# (or is clipped to one), so the restatement and the kernel compute the same bits whatever the order of their operations.
#   'seven'  3 positives at (2, 0), 4 negatives at (0, 0): every choice of the first step is a tie
#   'edges'  65 positives at (2, 0): the i tie crosses the wave edge 63 | 64; negatives at (0, 0) only at t = 255 and t = 256: the j tie
#            crosses the block-stride edge; the other negatives up to t = 257 at (0, 2), a lower gain
#   'tau'    positives (0, 0) and (2, 0), negatives (2, 0) and (0, 2), and K between the twins t = 1, 2 is 4 + 2^-20, as a Gram matrix
#            summed in another order may give: quad = -2^-19 < 0, so only the TAU guard lets the twin be chosen (and clipped)
# name -> (coordinates of the positives, of the negatives, trace)
TIES = {'seven': ([(2, 0)] * 3, [(0, 0)] * 4, [(2, 6), (1, 5)]),
        'edges': ([(2, 0)] * 65, [(0, 2)] * 190 + [(0, 0)] * 2 + [(0, 2)], [(64, 256), (63, 255)]),
        'tau': ([(0, 0), (2, 0)], [(2, 0), (0, 2)], [(1, 2), (0, 3)])}


@functools.lru_cache(maxsize=None)
def tie_problem(name):
    plus, minus, trace = TIES[name]
    X = np.array(plus + minus, dtype=np.float64)
    n, npos = len(X), len(plus)
    G = X @ X.T
    if name == 'tau':
        G[1, 2] = G[2, 1] = 4 + 2.0 ** -20
    N = n + 5
    idx = np.sort(np.random.default_rng(n).permutation(N)[:n]).astype(np.int32)[::-1].copy()     # descending: point t is row idx[t]
    K = np.full((N, N + PAD), np.nan)
    K[np.ix_(idx, idx)] = G
    K.setflags(write=False)
    cb = np.full(n, 0.25)
    cb.setflags(write=False)
    return types.SimpleNamespace(name=name, K=K, idx=idx, npos=npos, cb=cb, n=n, trace=trace, pd=False, max_k=float(G.max()))


# The problem of the front-end test: three classes (labels out of order in the rows), class weights, integer sample weights (the
# zeros are dropped by the fit), rbf.  ``pairs``: libsvm's one-vs-one problems over the KEPT rows, the lower class positive, members
# in row order: (idx, npos, cb) with cb = (C * class weight) * sample weight.
def rbf_kernel(X, gamma):
    G = X @ X.T
    sq = np.diagonal(G)
    return np.exp(-gamma * (sq[:, None] + sq[None, :] - 2 * G))


@functools.lru_cache(maxsize=None)
def frontend_problem(seed=0):
    rng = np.random.default_rng(seed + 900)
    labels, per = np.array([3, 7, 9]), (33, 28, 37)
    y = rng.permutation(np.repeat(labels, per))
    centres = 1.2 * rng.standard_normal((3, 5))
    X = rng.standard_normal((len(y), 5)) + centres[np.searchsorted(labels, y)]
    w = rng.integers(0, 4, len(y)).astype(np.float64)
    class_weight = {3: 1.0, 7: 2.0, 9: 0.5}
    C, keep = 1.5, w > 0
    yk, wk = y[keep], w[keep]
    pairs = []
    for a in range(3):
        for b in range(a + 1, 3):
            ia, ib = np.flatnonzero(yk == labels[a]), np.flatnonzero(yk == labels[b])
            idx = np.concatenate([ia, ib])
            cw = np.concatenate([np.full(len(ia), class_weight[labels[a]]), np.full(len(ib), class_weight[labels[b]])])
            pairs.append((idx.astype(np.int32), len(ia), (C * cw) * wk[idx]))
    return types.SimpleNamespace(X=X, y=y, w=w, class_weight=class_weight, C=C, gamma=0.3, tol=EPS, keep=keep, pairs=pairs)


# ------------------------------------------------------------------------------------------------ the assertions
def check_feasible(p, alpha):
    """The box, exactly: clipping ASSIGNS the bounds, so there is no tolerance; a zero bound never moves."""
    assert np.isfinite(alpha).all(), f'{p.name}: alpha is not finite'
    assert (alpha >= 0).all() and (alpha <= p.cb).all(), f'{p.name}: alpha leaves the box'
    assert (alpha[p.cb == 0] == 0).all(), f'{p.name}: a point with a zero bound moved'


def check_certificate(p, alpha, rho, iters, max_iter=MAX_ITER, eps=EPS):
    """What holds for every problem whatever the trajectory.  Returns (KKT excess over eps, |rho - rho of the certificate|, drift)."""
    check_feasible(p, alpha)
    assert 0 <= iters <= max_iter, f'{p.name}: iters {iters}'
    assert np.isfinite(rho), f'{p.name}: rho {rho}'
    c = certificate(p.K, p.idx, p.npos, p.cb, alpha, rho)
    cmax = float(p.cb.max())
    assert c.below == 0 and c.above == 0
    # the pair update conserves y' alpha up to one rounding of each of the two alphas per iteration
    assert c.sum_y_alpha <= 4 * iters * U * cmax, f'{p.name}: |sum y alpha| {c.sum_y_alpha:.3e} after {iters} iterations'
    # every iteration adds two products of a few roundings each to every G[t]
    drift = 8 * iters * U * p.max_k * cmax
    assert c.rho_err <= drift, f'{p.name}: rho {rho!r} against {float(c.rho)!r} of the recomputed gradient, drift {drift:.3e}'
    excess = c.kkt_gap - eps
    if iters < max_iter:
        assert excess <= drift, f'{p.name}: KKT gap {c.kkt_gap:.6e} exceeds eps by {excess:.3e}, drift {drift:.3e}'
        # the stop was genuine: one more iteration from the kernel's alpha and the recomputed gradient stops as well
        more = smo_ref(p.K, p.idx, p.npos, p.cb, eps, 1, alpha0=alpha, G0=c.G.astype(np.float64))
        assert more.iters == 0 or more.margins[0, 2] < drift, f'{p.name}: the run stopped {more.margins[0, 2]:.3e} above eps'
    return excess, c.rho_err, drift


def tolerance(p, s_case, iters):
    """The trajectory tolerance: 16 x the larger of the reference's own sensitivity and one rounding of the largest bound per iteration."""
    return 16 * max(s_case, iters * U * float(p.cb.max()))


def support(alpha, cb):
    return np.flatnonzero(alpha > 0).tolist(), np.flatnonzero(alpha == cb).tolist()


def check_trajectory(p, alpha, rho, iters, max_iter=MAX_ITER):
    """A positive definite committed problem against the restatement.  Returns (alpha error, rho error, s_case, tolerance)."""
    ref = reference(p.spec, max_iter)
    assert iters == ref.iters, f'{p.name}: {iters} iterations, the restatement takes {ref.iters}'
    assert support(alpha, p.cb) == support(ref.alpha, p.cb), f'{p.name}: the support differs'
    s_case = sensitivity(p.spec, max_iter)
    tol = tolerance(p, s_case, iters)
    ea, er = float(np.abs(alpha - ref.alpha).max()), float(abs(rho - ref.rho))
    assert ea <= tol, f'{p.name}: alpha is {ea:.3e} from the restatement, tolerance {tol:.3e} (s_case {s_case:.3e})'
    assert er <= tol, f'{p.name}: rho is {er:.3e} from the restatement, tolerance {tol:.3e} (s_case {s_case:.3e})'
    return ea, er, s_case, tol


def check_prefix(p, m, alpha, rho, iters):
    """The state after ``m`` iterations of a trajectory case (every committed one takes more than m or is compared at its end)."""
    ref = reference(p.spec, m)
    assert iters == ref.iters == min(m, reference(p.spec).iters), f'{p.name}: {iters} iterations at max_iter = {m}'
    check_feasible(p, alpha)
    tol = tolerance(p, sensitivity(p.spec, m), iters)
    ea, er = float(np.abs(alpha - ref.alpha).max()), float(abs(rho - ref.rho))
    assert ea <= tol, f'{p.name}: alpha after {m} iterations is {ea:.3e} from the restatement, tolerance {tol:.3e}'
    assert er <= tol, f'{p.name}: rho after {m} iterations is {er:.3e} from the restatement, tolerance {tol:.3e}'
    c = certificate(p.K, p.idx, p.npos, p.cb, alpha, rho)                  # rho follows calculate_rho on the current gradient
    assert c.rho_err <= 8 * iters * U * p.max_k * float(p.cb.max()), f'{p.name}: rho after {m} iterations: {c.rho_err:.3e}'
    if m == 1 and iters == 1:
        # all G = -1: i is the last positive that can move (npos - 1 unless its bound is zero), j one negative
        moved = np.flatnonzero(alpha).tolist()
        last = int(np.flatnonzero(p.cb[:p.npos] > 0)[-1])
        assert len(moved) == 2 and moved[0] == last and moved[1] >= p.npos, f'{p.name}: the first step moved {moved}'
    return ea, er


def check_problem(p, solve):
    """Every assertion the GPU test makes on a committed problem.  ``solve(max_iter) -> (alpha, rho, iters)``: the kernel there, a
    variant of the restatement in the host test.  Returns the figures to print."""
    alpha, rho, iters = solve(MAX_ITER)
    assert iters < MAX_ITER, f'{p.name}: did not converge'
    out = dict(name=p.name, iters=iters)
    out['excess'], out['rho_cert'], out['drift'] = check_certificate(p, alpha, rho, iters)
    if p.pd:
        out['alpha_err'], out['rho_err'], out['s_case'], out['tol'] = check_trajectory(p, alpha, rho, iters)
        for m in PREFIXES:
            ea, er = check_prefix(p, m, *solve(m))
            out['alpha_err'], out['rho_err'] = max(out['alpha_err'], ea), max(out['rho_err'], er)
    return out


def check_tie(p, solve):
    """An exact-arithmetic tie problem: the bits of the restatement, at the end and after one iteration."""
    for m in (MAX_ITER, 1):
        ref = smo_ref(p.K, p.idx, p.npos, p.cb, EPS, m)
        assert ref.trace == p.trace[:m]
        alpha, rho, iters = solve(m)
        assert iters == ref.iters, f'{p.name}: {iters} iterations, the restatement takes {ref.iters}'
        assert np.array_equal(np.asarray(alpha).view(np.int64), ref.alpha.view(np.int64)), f'{p.name}: alpha {np.flatnonzero(alpha)}'
        assert np.float64(rho).view(np.int64) == np.float64(ref.rho).view(np.int64), f'{p.name}: rho {rho!r}, exact {ref.rho!r}'
