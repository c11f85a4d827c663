"""A plain numpy / long-double restatement of the tensor maximum entropy surrogates of surrogates/tme.py (Elsayed &
Cunningham 2017), with the error bars the GPU tests hold the kernels to.  Nothing here imports the package.

X (n0, n1, n2) -> R = X with the mean along every axis removed (M = X - R), Sigma_r = R_(r) R_(r)^T of the three unfoldings,
their eigenpairs in descending order, the pairs with lam > eig_tol lam_max kept and rescaled to the trace |R|_F^2, and the
multipliers l_r of the maximum entropy distribution: W_ijk = 1 / (l0_i + l1_j + l2_k) with every single-axis marginal of W equal to
lam_r.  A surrogate is M + (z sqrt(W)) x_0 Q_0 x_1 Q_1 x_2 Q_2.

Sums over the box are taken in long double (64-bit mantissa on x86: u_ld = 2^-64, so a sum of L <= 2^21 positive terms is exact to
2^-43 u-units of float64: far below every bar here).  u = 2^-53."""
import itertools

import numpy as np

U = 2.0 ** -53
LD = np.longdouble

# kept boxes the kernels are tested on, and the full-size tensors of the fits: (shape, center) -> kept
BOXES = [(1, 4, 4), (2, 2, 2), (5, 7, 3), (65, 9, 33), (64, 64, 4)]
FITS = [((1, 4, 6), False), ((6, 4, 6), True), ((3, 3, 3), True), ((6, 8, 4), True), ((66, 10, 34), True), ((65, 65, 5), True),
        ((65, 9, 33), True)]


def fit_name(shape, center):
    return 'x'.join(str(n) for n in shape) + ('' if center else '_raw')


# ------------------------------------------------------------------------------------------------ data side
def center(X, do=True):
    """(R, M): R = X with the mean along axis 0, then 1, then 2 removed (the three commute); M = X - R."""
    X = np.asarray(X, dtype=np.float64)
    R = X.copy()
    if do:
        for ax in range(3):
            R = R - R.mean(axis=ax, keepdims=True)
    return R, X - R


def unfold(T, r):
    """The mode-r unfolding (n_r, product of the others), the others in ascending axis order."""
    T = np.asarray(T)
    return np.moveaxis(T, r, 0).reshape(T.shape[r], -1)


def sigma(R, r):
    A = unfold(R, r)
    return A @ A.T


def eig_desc(S):
    w, V = np.linalg.eigh(S)
    return w[::-1].copy(), V[:, ::-1].copy()


def keep_and_scale(ws, shape, total, preserve=(0, 1, 2), eig_tol=1e-10):
    """(kept, lams): per axis the number of eigenpairs with lam > eig_tol lam_max and their eigenvalues rescaled to add up to
    `total`; an axis outside `preserve` keeps all n_r with the uniform spectrum total / n_r.  ws[r]: descending eigenvalues."""
    kept, lams = [], []
    for r in range(3):
        if r not in preserve:
            kept.append(int(shape[r]))
            lams.append(np.full(shape[r], total / shape[r]))
            continue
        w = np.asarray(ws[r], dtype=np.float64)
        k = int((w > eig_tol * w[0]).sum())
        kept.append(k)
        lams.append(w[:k] * (total / w[:k].sum()))
    return kept, lams


def random_tensor(shape, seed, decay=None):
    """normal + 1 with unequal axis scales; decay: axis-2 scales 10^(-decay j / (n2 - 1)) (a spectrum of condition 10^(2 decay))."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal(shape) + 1.0
    for ax in range(3):
        s = 1.0 + np.arange(shape[ax]) / max(shape[ax] - 1, 1)
        if decay is not None and ax == 2:
            s = 10.0 ** (-decay * np.arange(shape[ax]) / max(shape[ax] - 1, 1))
        X = X * np.expand_dims(s, tuple(a for a in range(3) if a != ax))
    return X


# ------------------------------------------------------------------------------------------------ the box
def box(ls):
    """D_ijk = l0_i + l1_j + l2_k in long double."""
    l0, l1, l2 = (np.asarray(v, dtype=LD) for v in ls)
    return l0[:, None, None] + l1[None, :, None] + l2[None, None, :]


def marginals(ls):
    """Every output of the Kronecker-sum pass in long double: w1[r], w2[r] (single marginals of W and W^2), p01, p02, p12 (pairwise
    marginals of W^2), sumlog, abslog (sum |log D|), bad (any D <= 0)."""
    D = box(ls)
    others = [(1, 2), (0, 2), (0, 1)]
    with np.errstate(invalid='ignore', divide='ignore'):                 # (a box with a D <= 0 is asked for its flag)
        W = 1 / D
        W2 = W * W
        lg = np.log(D)
    return dict(w1=[W.sum(axis=o) for o in others], w2=[W2.sum(axis=o) for o in others], p01=W2.sum(axis=2), p02=W2.sum(axis=1),
                p12=W2.sum(axis=0), sumlog=lg.sum(), abslog=np.abs(lg).sum(), bad=bool((~(D > 0)).any()))


def exact_marginals(ls):
    """The same sums for INTEGER multipliers as exact rationals (fractions), returned as long doubles of the exact values."""
    from fractions import Fraction
    l0, l1, l2 = ([int(v) for v in l] for l in ls)
    k = (len(l0), len(l1), len(l2))
    W = np.empty(k, dtype=object)
    for i, j, q in itertools.product(*(range(n) for n in k)):
        W[i, j, q] = Fraction(1, l0[i] + l1[j] + l2[q])
    W2 = W * W
    others = [(1, 2), (0, 2), (0, 1)]

    def ld(a):
        a = np.asarray(a, dtype=object)
        out = np.empty(a.shape, dtype=LD)
        for idx in np.ndindex(a.shape):
            f = a[idx]
            out[idx] = LD(f.numerator) / LD(f.denominator)
        return out
    return dict(w1=[ld(W.sum(axis=o)) for o in others], w2=[ld(W2.sum(axis=o)) for o in others], p01=ld(W2.sum(axis=2)),
                p02=ld(W2.sum(axis=1)), p12=ld(W2.sum(axis=0)))


def terms(k):
    """The number of terms L of every output of the pass for a box k: w1 / w2 of axis r, p01, p02, p12, sumlog."""
    k0, k1, k2 = k
    return dict(w=[k1 * k2, k0 * k2, k0 * k1], p01=k2, p02=k1, p12=k0, sumlog=k0 * k1 * k2)


def residual(lams, ls):
    """max |marginal - lam| / lam over every axis and kept index, the marginals in long double."""
    m = marginals(ls)
    return float(max(np.max(np.abs(m['w1'][r] - np.asarray(lams[r], dtype=LD)) / np.asarray(lams[r], dtype=LD)) for r in range(3)))


# ------------------------------------------------------------------------------------------------ the solver
def start(lams):
    k = [len(v) for v in lams]
    n = float(np.prod(k))
    return [(n / k[r]) / (3.0 * np.asarray(lams[r], dtype=np.float64)) for r in range(3)]


def balance(l, cuts):
    """The same D in the gauge where the smallest multiplier of every axis is the same (a third of the smallest D): the shifts
    l0 + a, l1 + b, l2 - a - b leave D, and with equal traces F, unchanged, and keep every multiplier positive while D > 0."""
    mins = [l[cuts[r]:cuts[r + 1]].min() for r in range(3)]
    out = l.copy()
    for r in range(3):
        out[cuts[r]:cuts[r + 1]] += sum(mins) / 3.0 - mins[r]
    return out


def accepts(new, cur):
    """A step is taken if F decreases, or if F is flat to rounding and the largest relative residual decreases."""
    if not (np.isfinite(new['F']) and np.isfinite(new['res'])):
        return False
    return new['F'] < cur['F'] or (new['F'] <= cur['F'] + 1e-13 * cur['scale'] and new['res'] < cur['res'])


def solve(lams, tol=1e-10, max_iter=200):
    """Levenberg-Marquardt Newton in theta = log l on F(l) = sum_r lam_r . l_r - sum log D -> (ls, residual, iterations).  The
    marginals of every evaluation are long-double sums; the linear algebra is float64.  Raises when it does not converge."""
    lams = [np.asarray(v, dtype=np.float64) for v in lams]
    k = [len(v) for v in lams]
    cuts = np.cumsum([0] + k)
    lam = np.concatenate(lams)

    def evaluate(theta):
        l = np.exp(theta)
        ls = [l[cuts[r]:cuts[r + 1]] for r in range(3)]
        m = marginals(ls)
        w1 = np.concatenate([np.asarray(v, dtype=np.float64) for v in m['w1']])
        H = np.diag(np.concatenate([np.asarray(v, dtype=np.float64) for v in m['w2']]))
        H[cuts[0]:cuts[1], cuts[1]:cuts[2]] = m['p01']
        H[cuts[0]:cuts[1], cuts[2]:cuts[3]] = m['p02']
        H[cuts[1]:cuts[2], cuts[2]:cuts[3]] = m['p12']
        H = np.triu(H) + np.triu(H, 1).T
        g = lam - w1
        return dict(l=l, F=float(lam @ l - float(m['sumlog'])), scale=float(abs(lam @ l) + abs(float(m['sumlog']))),
                    res=float(np.max(np.abs(g) / lam)), g=g, H=H)

    theta = np.log(np.concatenate(start(lams)))
    cur, mu = evaluate(theta), 1e-2
    for it in range(1, max_iter + 1):
        if cur['res'] <= tol:
            return [cur['l'][cuts[r]:cuts[r + 1]] for r in range(3)], cur['res'], it
        l = cur['l']
        Ht = l[:, None] * cur['H'] * l[None, :] + np.diag(cur['g'] * l)
        try:
            step = np.linalg.solve(Ht + np.diag(mu * np.abs(np.diag(Ht))), -(cur['g'] * l))
        except np.linalg.LinAlgError:
            mu *= 4.0
            continue
        with np.errstate(over='ignore', invalid='ignore'):
            new = evaluate(theta + step)
        if accepts(new, cur):
            theta, cur, mu = np.log(balance(new['l'], cuts)), new, max(mu / 8.0, 1e-12)
            cur['l'] = np.exp(theta)
        else:
            mu *= 4.0
    raise RuntimeError(f'tme_ref.solve: residual {cur["res"]:.3e} after {max_iter} iterations')


# ------------------------------------------------------------------------------------------------ the sampling map
def weights(ls):
    return np.asarray(1 / box(ls), dtype=np.float64)


def core_of(z, ls):
    """z sqrt(W) in long double; z (..., k0, k1, k2)."""
    return np.asarray(z, dtype=LD) * np.sqrt(1 / box(ls))


def mode_product(T, Q, axis):
    """T x_axis Q: the axis of T (length k) is contracted with the columns of Q (n, k); the result has length n there."""
    out = np.tensordot(np.asarray(Q, dtype=T.dtype), T, axes=([1], [axis]))
    return np.moveaxis(out, 0, axis)


def sample_map(z, ls, Qs, M):
    """(surrogates, bar): M + core x_0 Q_0 x_1 Q_1 x_2 Q_2 for z (S, k0, k1, k2) in long double, and the elementwise bar
    (k0 + k1 + k2 + 8) u (|Q_0| x |Q_1| x |Q_2|) |core| + u |M| of three chained float64 products of lengths k2, k1, k0, the
    scaling of the core (3 roundings) and the final addition."""
    core = core_of(z, ls)
    out, mag = core, np.abs(core)
    for r in range(3):
        out = mode_product(out, np.asarray(Qs[r], dtype=LD), r + 1)
        mag = mode_product(mag, np.abs(np.asarray(Qs[r], dtype=LD)), r + 1)
    k = core.shape[1:]
    out = out + np.asarray(M, dtype=LD)
    bar = (sum(k) + 8) * U * mag + U * np.abs(np.asarray(M, dtype=LD))
    return out, bar


def implied_cov(Q, marg):
    Q = np.asarray(Q, dtype=np.float64)
    return (Q * np.asarray(marg, dtype=np.float64)) @ Q.T


def rel_fro(A, B):
    return float(np.linalg.norm(np.asarray(A, dtype=np.float64) - np.asarray(B, dtype=np.float64)) / np.linalg.norm(B))


def fit(X, preserve=(0, 1, 2), center_=True, eig_tol=1e-10, tol=1e-10):
    """The whole fit on the host -> dict(R, M, kept, lams, Qs, ls, residual, n_iter, total)."""
    R, M = center(X, center_)
    total = float((R * R).sum())
    ws, Vs = [], []
    for r in range(3):
        w, V = eig_desc(sigma(R, r))
        ws.append(w)
        Vs.append(V)
    kept, lams = keep_and_scale(ws, R.shape, total, preserve, eig_tol)
    Qs = [Vs[r][:, :kept[r]] if r in preserve else np.eye(R.shape[r]) for r in range(3)]
    ls, res, it = solve(lams, tol)
    return dict(R=R, M=M, kept=kept, lams=lams, Qs=Qs, ls=ls, residual=res, n_iter=it, total=total)


def surrogate_cov_deviation(X, n_sur, seed):
    """The largest relative Frobenius deviation, over the three axes, of the mean over n_sur host surrogates of S_(r) S_(r)^T
    (S without its mean tensor) from Sigma_r: the statistical test's yardstick, drawn with numpy's generator."""
    f = fit(X)
    z = np.random.default_rng(seed).standard_normal((n_sur,) + tuple(f['kept']))
    core = z * np.sqrt(weights(f['ls']))
    S = core
    for r in range(3):
        S = mode_product(S, f['Qs'][r], r + 1)
    worst = 0.0
    for r in range(3):
        A = np.moveaxis(S, r + 1, 1).reshape(n_sur, X.shape[r], -1)
        worst = max(worst, rel_fro(np.einsum('sab,scb->ac', A, A) / n_sur, sigma(f['R'], r)))
    return worst
