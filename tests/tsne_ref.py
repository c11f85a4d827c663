"""Restatement of the exact t-SNE contract of include/xps.h (csrc/xps_tsne.hip) in numpy, for tests/test_gpu_tsne_kernels.py and
tests/test_gpu_tsne.py (tests/test_tsne_ref_host.py holds the restatement itself to sklearn on the CPU).

Every function takes a ``dtype``: np.float64 rounds where the kernels round and adds in their order -- lane l of a wave takes
its terms l, l + 64, ... in ascending order, the 64 partial sums meet in the xor butterfly 32, 16, .., 1 (``wave_sum``) --;
np.longdouble is the twin the error bars are measured against.  Also here: the fixed-seed cases and the bars, derived from each
case's data (nothing is a number chosen in advance):

* u = 2^-53; exp and log are taken at 2 ulps; a sum of m terms in the stated order carries ``sum_bar(m)`` = (ceil(m / 64) + 6) u
  relative to the sum of the |terms| (a lane's chain of ceil(m / 64) additions, six butterfly levels).
* exp(-d2 beta): the product is rounded once, so the value moves by (|d2 beta| + 2) u relative; one more u is spare; and by two
  subnormal spacings absolutely (2^-1073), which only counts in a row whose whole sum is subnormal.
* the force sums a, b carry an ABSOLUTE bar against their sum of |terms| (taken in long double by the caller): a term
  (P w) d[c] has four roundings in w = 1 / (1 + d0^2 + d1^2), two products; (w w) d[c] doubles w's.
* discrete decisions too close to call are REPORTED, not bounded: a search row is undecided if at any step
  | |entropy - log perplexity| - 1e-5 | < 1e3 x the entropy's bar (a row that walks along float64's underflow boundary has a
  subnormal sum and a bar of order 1: the long-double twin, with its wider exponent, takes another path there), or if a sum is
  exactly 0 while a term sits within one unit of the underflow boundary (-d2 beta > -746); a gains element if
  0 < |update grad| < 1e3 x its bar.
"""
import numpy as np

import cluster_ref as CR

LD = np.longdouble
U = 2.0 ** -53
EPS = 2.220446049250313e-16
TOL = float(np.float32(1e-5))              # the .pyx keeps both constants in a C float
EPS_SUM = float(np.float32(1e-8))
DBL_MAX = float(np.finfo(np.float64).max)
TINY = 2.0 ** -1074                        # float64's smallest subnormal: the absolute floor of an exp's error
_LANES = np.arange(64)


def sum_bar(m, order='wave'):
    """Relative error of a sum of m terms against the sum of their magnitudes: the kernels' order, or any order (m u)."""
    return ((-(-int(m) // 64) + 6) if order == 'wave' else int(m)) * U


def wave_sum(t):
    """Sum over the last axis in the kernels' order, in t's dtype."""
    t = np.asarray(t)
    m = t.shape[-1]
    rounds = -(-m // 64)
    pad = np.zeros(t.shape[:-1] + (rounds * 64 - m,), dtype=t.dtype)
    t = np.concatenate([t, pad], axis=-1).reshape(t.shape[:-1] + (rounds, 64))
    acc = np.zeros(t.shape[:-2] + (64,), dtype=t.dtype)
    for r in range(rounds):
        acc = acc + t[..., r, :]
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., _LANES ^ o]
    return acc[..., 0]


# ------------------------------------------------------------------------------------------------ cases
def _blobs(n, D, k, seed, dtype=np.float64):
    return CR.make_case(n, D, k, seed, dtype)[0]


def cases():
    """name -> (X, perplexity): the smallest shapes at which the kernels can go wrong."""
    deg = _blobs(130, 10, 5, 25)
    deg[7] = 1e3                 # every exp of the row underflows: the sum == 0 -> 1e-8 branch
    deg[20:32] = 25.0            # twelve identical rows away from the blobs (a row with THEM as nearest neighbours would exhaust too)
    return {
        'n5_D3': (_blobs(5, 3, 2, 21), 2.0),
        'n64_D10': (_blobs(64, 10, 4, 22), 30.0),
        'n65_D17_f32': (_blobs(65, 17, 3, 23, np.float32), 5.0),
        'n130_D100': (_blobs(130, 100, 9, 24), 30.0),
        'n130_D10_degenerate': (deg, 5.0),
    }


def random_init(n, nc, seed):
    """sklearn's init='random' draws, widened."""
    return (1e-4 * np.random.RandomState(seed).standard_normal((n, nc)).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ steps 1 - 3
def sqdist_f32(X):
    """Step 1 in numpy: the Gram matrix of the centred rows (numpy's dot order), d2 = max((G_ii + G_jj) - 2 G_ij, 0) -> float32."""
    Xc = CR.centred(X)
    G = Xc @ Xc.T
    g = np.diag(G)
    d = np.maximum((g[:, None] + g[None, :]) - 2.0 * G, 0.0)
    np.fill_diagonal(d, 0.0)
    return d.astype(np.float32)


def sqdist_bar(X):
    """Absolute bar (n, n) of the float32 d2 against the long-double direct differences: cluster_ref's Gram bound
    (D + 6) u (|x_i| + |x_j|)^2 plus one float32 rounding of the value."""
    Xc = CR.centred(X)
    nrm = np.sqrt((Xc * Xc).sum(axis=1))
    d2 = np.asarray(CR.sq_dists(X), dtype=np.float64)
    gram = (Xc.shape[1] + 6) * U * (nrm[:, None] + nrm[None, :]) ** 2
    return gram + 2.0 ** -24 * (d2 + gram)


class Search:
    """C, beta, steps, rowsum of the perplexity search; C_bar (absolute), undecided (rows), margin (the smallest
    | |diff| - 1e-5 | of a row over its steps) and entropy_bar (the largest of a row)."""


def search(d2, perplexity, dtype=np.float64):
    d2 = np.asarray(d2)
    assert d2.dtype == np.float32
    n = len(d2)
    d = d2.astype(dtype)
    off = ~np.eye(n, dtype=bool)
    desired = dtype(np.log(np.float64(np.float32(perplexity))))
    beta, bmin, bmax = np.ones(n, dtype), np.full(n, -np.inf, dtype), np.full(n, np.inf, dtype)
    beta_used, sum_used = np.ones(n, dtype), np.ones(n, dtype)
    steps, active = np.zeros(n, np.int32), np.ones(n, bool)
    margin, ent_bar, undecided = np.full(n, np.inf), np.zeros(n), np.zeros(n, bool)
    sb = sum_bar(n)
    with np.errstate(under='ignore', over='ignore', invalid='ignore', divide='ignore'):
        for l in range(100):
            idx = np.nonzero(active)[0]
            if not len(idx):
                break
            b = beta[idx]
            arg = -d[idx] * b[:, None]
            e = np.where(off[idx], np.exp(arg), dtype(0))
            raw = wave_sum(e)
            s = np.where(raw == 0, dtype(EPS_SUM), raw)
            p = e / s[:, None]
            sd = wave_sum(d[idx] * p)
            ent = np.log(s) + b * sd
            diff = ent - desired
            # the entropy's bar, in float64
            a64 = arg.astype(np.float64)
            e64, s64, p64, d64, b64 = (np.asarray(a, np.float64) for a in (e, s, p, d[idx], b))
            abs_e = np.where(off[idx], e64 * (np.abs(a64) + 3.0) * U + 2 * TINY, 0.0)
            rel_s = abs_e.sum(axis=1) / s64 + sb
            dp = d64 * p64
            d_p = abs_e / s64[:, None] + p64 * (rel_s[:, None] + U)
            bar = (rel_s + 2 * U * np.abs(np.log(s64)) + b64 * ((d64 * d_p).sum(axis=1) + (sb + U) * dp.sum(axis=1))
                   + U * np.abs(b64 * np.asarray(sd, np.float64)) + 2 * U * np.abs(np.asarray(ent, np.float64)))
            gap = np.abs(np.abs(np.asarray(diff, np.float64)) - TOL)
            margin[idx] = np.minimum(margin[idx], gap)
            ent_bar[idx] = np.maximum(ent_bar[idx], bar)
            undecided[idx] |= gap < 1e3 * bar
            # sum == 0 is a decision too: too close to call where a term sits on the underflow boundary
            undecided[idx] |= (np.asarray(raw, np.float64) == 0) & (np.where(off[idx], a64, -np.inf).max(axis=1) > -746.0)
            steps[idx] = l + 1
            beta_used[idx], sum_used[idx] = b, s
            stop = np.abs(diff) <= TOL
            up = diff > 0
            nb = np.where(up, np.where(np.isinf(bmax[idx]), b * 2, (b + bmax[idx]) / 2),
                          np.where(np.isinf(bmin[idx]), b / 2, (b + bmin[idx]) / 2))
            go = ~stop
            bmin[idx] = np.where(go & up, b, bmin[idx])
            bmax[idx] = np.where(go & ~up, b, bmax[idx])
            beta[idx] = np.where(go, nb, b)
            active[idx[stop]] = False
        arg = -d * beta_used[:, None]
        C = np.where(off, np.exp(arg) / sum_used[:, None], dtype(0))
        C64, s64 = np.asarray(C, np.float64), np.asarray(sum_used, np.float64)
        abs_e = np.where(off, C64 * s64[:, None] * (np.abs(arg.astype(np.float64)) + 3.0) * U + 2 * TINY, 0.0)
        rel_s = abs_e.sum(axis=1) / s64 + sb
        C_bar = abs_e / s64[:, None] + C64 * (rel_s[:, None] + U)
    out = Search()
    out.C, out.beta, out.steps, out.rowsum = C, beta, steps, wave_sum(C)
    out.C_bar = C_bar
    out.undecided, out.margin, out.entropy_bar = undecided, margin, ent_bar
    return out


def joint(C, rowsum):
    """Step 3: P = max((C + C^T) / S, eps), S = max(2 sum_i rowsum_i, eps), zero diagonal."""
    dtype = C.dtype.type
    S = dtype(2) * wave_sum(rowsum)
    S = S if S > EPS else dtype(EPS)
    P = np.maximum((C + C.T) / S, dtype(EPS))
    np.fill_diagonal(P, 0)
    return P


def joint_bar(sr):
    """Absolute bar (n, n) of P from the search's bars: the two C's, S (2 n^2 terms through two levels of sums), the division."""
    C = np.asarray(sr.C, np.float64)
    n = len(C)
    S = 2.0 * float(np.asarray(sr.rowsum, np.float64).sum())
    rel_S = sr.C_bar.sum() / C.sum() + 2 * sum_bar(n) + U
    return (sr.C_bar + sr.C_bar.T) / S + ((C + C.T) / S) * (rel_S + 2 * U)


# ------------------------------------------------------------------------------------------------ steps 4 - 6
def _y2(Y, dtype):
    Y = np.asarray(Y, dtype=dtype).reshape(len(Y), -1)
    return np.concatenate([Y, np.zeros((len(Y), 2 - Y.shape[1]), dtype)], axis=1)      # component 1 of a one-component problem is 0


class Partials:
    """s (n,), a, b (n, 2), e1, e2 (n,) or None; min_w: the smallest w_ij (for the clamp assertion)."""


def partials(P, Y, want_err, dtype=np.float64):
    Y = _y2(Y, dtype)
    n = len(Y)
    P = np.asarray(P, dtype=dtype)
    off = ~np.eye(n, dtype=bool)
    d0 = Y[:, None, 0] - Y[None, :, 0]
    d1 = Y[:, None, 1] - Y[None, :, 1]
    q = 1 + (d0 * d0 + d1 * d1)
    w = np.where(off, 1 / q, dtype(0))
    pw, w2 = P * w, w * w
    out = Partials()
    out.s = wave_sum(w)
    out.a = np.stack([wave_sum(pw * d0), wave_sum(pw * d1)], axis=1)
    out.b = np.stack([wave_sum(w2 * d0), wave_sum(w2 * d1)], axis=1)
    out.e1 = out.e2 = None
    if want_err:
        with np.errstate(divide='ignore', invalid='ignore'):
            out.e1 = wave_sum(np.where(off, P * np.log(np.where(off, P * q, 1)), dtype(0)))
        out.e2 = wave_sum(np.where(off, P, dtype(0)))
    out.min_w = float(w[off].min())
    return out


def partials_bars(P, Y):
    """Absolute bars of the float64 partial sums, from sums of |terms| taken in long double: dict s, a, b, e1, e2."""
    Y = _y2(Y, LD)
    n = len(Y)
    P = np.asarray(P, dtype=LD)
    off = ~np.eye(n, dtype=bool)
    d0, d1 = Y[:, None, 0] - Y[None, :, 0], Y[:, None, 1] - Y[None, :, 1]
    q = 1 + (d0 * d0 + d1 * d1)
    w = np.where(off, 1 / q, LD(0))
    sb = sum_bar(n)
    f = lambda x: np.asarray(x, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        lg = np.where(off, np.log(np.where(off, P * q, 1)), LD(0))
    return dict(
        s=f((sb + 4 * U) * w.sum(axis=1)),
        a=f((sb + 6 * U) * np.stack([(P * w * np.abs(d0)).sum(axis=1), (P * w * np.abs(d1)).sum(axis=1)], axis=1)),
        b=f((sb + 10 * U) * np.stack([(w * w * np.abs(d0)).sum(axis=1), (w * w * np.abs(d1)).sum(axis=1)], axis=1)),
        e1=f(sb * (P * np.abs(lg)).sum(axis=1) + (P * (5 * U + 3 * U * np.abs(lg))).sum(axis=1)),
        e2=f(sb * np.where(off, P, 0).sum(axis=1)))


def objective(pt, exag, dtype=np.float64):
    """(Z, grad (n, 2), error or NaN) from the partial sums, as a launch forms them."""
    Z = wave_sum(pt.s)
    assert pt.min_w / float(Z) > EPS, 'sklearn\'s clamp Q = max(w / Z, eps) would be active: outside the contract'
    rz = 1 / Z
    grad = 4 * (dtype(exag) * pt.a - rz * pt.b)
    err = dtype(np.nan)
    if pt.e1 is not None:
        err = dtype(exag) * (wave_sum(pt.e1) + np.log(dtype(exag) * Z) * wave_sum(pt.e2))
    return Z, grad, err


def objective_bars(pt, bars, exag):
    """Absolute bars of (Z, grad, error) as objective() forms them from partial sums that carry ``bars``."""
    n = len(pt.s)
    sb = sum_bar(n)
    s64 = np.asarray(pt.s, np.float64)
    Z = float(s64.sum())
    dZ = float(bars['s'].sum()) + sb * Z
    b64, a64 = np.abs(np.asarray(pt.b, np.float64)), np.abs(np.asarray(pt.a, np.float64))
    dg = 4.0 * (exag * bars['a'] + bars['b'] / Z + b64 / Z * (dZ / Z + 2 * U) + 2 * U * (exag * a64 + b64 / Z))
    dg = dg + U * 4.0 * (exag * a64 + b64 / Z)
    derr = None
    if pt.e1 is not None:
        e1, e2 = np.asarray(pt.e1, np.float64), np.asarray(pt.e2, np.float64)
        E1, E2, lz = float(e1.sum()), float(e2.sum()), float(np.log(exag * Z))
        derr = exag * (float(bars['e1'].sum()) + sb * float(np.abs(e1).sum()) + abs(lz) * (float(bars['e2'].sum()) + sb * E2)
                       + E2 * (dZ / Z + 3 * U + 2 * U * abs(lz)) + 3 * U * (abs(E1) + abs(lz) * E2))
    return dZ, dg, derr


class Descent:
    """One phase of _gradient_descent as xps_tsne_descent_f64 runs it: prime(), then step() per launch.  Fields: Y (n, 2),
    update, gains, grad, it (the next iteration; sklearn's `it` once done), error, best_error, best_it, done, Z, norm, Y_out;
    trajectory: Y after every launch; undecided: per launch, the gains elements too close to call (needs P_abs bars: a float64
    run only)."""

    def __init__(self, P, Y_in, nc, it_begin, max_iter, momentum, exag, lr, n_iter_without_progress=300, min_grad_norm=1e-7,
                 dtype=np.float64, track=False):
        self.dtype, self.P, self.nc, self.max_iter = dtype, np.asarray(P, dtype=dtype), nc, int(max_iter)
        self.momentum, self.exag, self.lr = dtype(momentum), exag, dtype(lr)
        self.niwp, self.mgn, self.track = n_iter_without_progress, min_grad_norm, track
        self.Y = _y2(Y_in, dtype)
        n = len(self.Y)
        self.update, self.gains, self.grad = np.zeros((n, 2), dtype), np.ones((n, 2), dtype), np.zeros((n, 2), dtype)
        self.it = self.best_it = int(it_begin)
        self.error = self.best_error = dtype(DBL_MAX)
        self.done, self.Z, self.norm, self.Y_out = False, dtype(0), dtype(0), None
        self.trajectory, self.undecided = [], []
        self.pt = partials(self.P, self.Y, self._wants(self.it), dtype)

    def _wants(self, it):
        return (it + 1) % 50 == 0 or it == self.max_iter - 1

    def step(self):
        if self.done:
            return
        dt, it, nc = self.dtype, self.it, self.nc
        Z, g, err = objective(self.pt, self.exag, dt)
        g[:, nc:] = 0
        if self.track:
            _, dg, _ = objective_bars(self.pt, partials_bars(self.P, self.Y), self.exag)
            ug = np.abs(np.asarray(self.update * g, np.float64))
            bar = np.abs(np.asarray(self.update, np.float64)) * dg + U * ug
            self.undecided.append(((ug > 0) & (ug < 1e3 * bar))[:, :nc])
        inc = self.update * g < 0
        ga = np.where(inc, self.gains + dt(0.2), self.gains * dt(0.8))
        ga = np.where(ga < dt(0.01), dt(0.01), ga)
        ga[:, nc:] = 1
        self.update = self.momentum * self.update - self.lr * (g * ga)
        self.Y = self.Y + self.update
        self.gains, self.grad, self.Z, self.error = ga, g, Z, err
        check, last = (it + 1) % 50 == 0, it == self.max_iter - 1
        if check:
            sc = g * ga
            self.norm = np.sqrt(wave_sum(sc[:, 0] * sc[:, 0] + sc[:, 1] * sc[:, 1]))
            if err < self.best_error:
                self.best_error, self.best_it = err, it
            elif it - self.best_it > self.niwp:
                self.done = True
            if self.norm <= self.mgn:
                self.done = True
        if last:
            self.done = True
        self.trajectory.append(self.Y[:, :nc].copy())
        if self.done:
            self.Y_out = self.Y[:, :nc].copy()
            return
        self.it = it + 1
        self.pt = partials(self.P, self.Y, self._wants(self.it), dt)

    def run(self, n_launches):
        for _ in range(n_launches):
            self.step()
        return self


def fit(P, Y0, nc, max_iter=1000, early_exaggeration=12.0, lr=None, n_iter_without_progress=300, min_grad_norm=1e-7,
        dtype=np.float64, explore=250):
    """Both phases as _tsne runs them -> (Y, kl_divergence, n_iter)."""
    n = len(P)
    lr = max(n / early_exaggeration / 4.0, 50.0) if lr is None else lr
    ph = Descent(P, Y0, nc, 0, explore, 0.5, early_exaggeration, lr, explore, min_grad_norm, dtype).run(explore)
    if ph.it + 1 < max_iter:
        ph = Descent(P, ph.Y_out, nc, ph.it + 1, max_iter, 0.8, 1.0, lr, n_iter_without_progress, min_grad_norm, dtype)
        ph.run(max_iter)
    return ph.Y_out, float(ph.error), ph.it


def trajectory_bars(traj64, trajld):
    """The bar at launch t of a pointwise comparison along a trajectory: 8 x the largest gap between the restatement's float64
    and long-double runs at t, at least 64 u x the embedding's largest |coordinate|."""
    out = []
    for a, b in zip(traj64, trajld):
        gap = float(np.abs(np.asarray(a, LD) - b).max())
        out.append(max(8.0 * gap, 64 * U * float(np.abs(a).max())))
    return out
