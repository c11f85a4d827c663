"""Tensor maximum entropy surrogates on the MI355X (Elsayed & Cunningham 2017): random ``(n0, n1, n2)`` tensors --
here ``(trials, T, channels)`` -- that keep a data tensor's mean and its covariance across each of the three axes, and nothing
else.  They are the control of the reference's cross-patient figures (``tme_corrs``, ``surr_recon``, ``cca_tme``, "Surrogate data
(unaligned)"), which reads them from a pickle that no program of the reference writes.

``X`` is centred along every axis (``R``; the mean tensor ``M = X - R`` is added back to every surrogate); ``Sigma_r = R_(r) R_(r)^T``
of the three unfoldings are formed by ONE ragged Gram launch and diagonalised by ``eigh_psd_batched``; the eigenpairs above
``eig_tol`` are kept and rescaled to the common trace.  The maximum entropy distribution with these marginals is Gaussian with
covariance ``(Q_0 x Q_1 x Q_2) diag(W) (...)^T``, ``W_ijk = 1 / (l0_i + l1_j + l2_k)``; its multipliers solve "every single-axis
marginal of W equals lam_r".  They are found by a damped Newton iteration in ``log l`` whose sums over the box -- the marginals
of W and W^2, ``sum log D`` -- are ONE ragged library call per iteration for every tensor still iterating
(``xps_tme_kron_pass_f64``); the host solves the (k0 + k1 + k2)-square linear system in float64.  A surrogate is
``M + (z sqrt(W)) x_0 Q_0 x_1 Q_1 x_2 Q_2`` with ``z`` standard normal: one scaling launch and three batched mode products per
chunk of surrogates, everything float64 and deterministic (the same bits for any chunking).  There is no CPU fallback; argument
errors are raised before the device is looked for.
"""
import numpy as np
import torch

from ..alignment import _linalg as LA

MAX_AXIS = LA.TME_MAX_AXIS
MU_START, MU_MIN, MU_MAX = 1e-2, 1e-12, 1e12
F_FLAT = 1e-13                                                            # F counts as flat within this fraction of its two terms


# ------------------------------------------------------------------------------------------------ arguments (no device)
def _check_options(preserve, center, eig_tol, tol, max_iter, what):
    try:
        axes = tuple(preserve)
    except TypeError:
        raise ValueError(f'{what}: preserve must be a sequence of axes out of 0, 1, 2; got {preserve!r}') from None
    if len(axes) == 0:
        raise ValueError(f'{what}: preserve must name at least one axis')
    for a in axes:
        if not (isinstance(a, (int, np.integer)) and not isinstance(a, bool) and 0 <= a <= 2):
            raise ValueError(f'{what}: preserve must hold axes out of 0, 1, 2; got {a!r}')
    for name, v in (('eig_tol', eig_tol), ('tol', tol)):
        if not (isinstance(v, (int, float, np.floating)) and 0 < v < 1):
            raise ValueError(f'{what}: {name} must lie in (0, 1); got {v!r}')
    if not (isinstance(max_iter, (int, np.integer)) and max_iter >= 1):
        raise ValueError(f'{what}: max_iter must be an integer >= 1; got {max_iter!r}')
    return tuple(sorted({int(a) for a in axes})), bool(center), float(eig_tol), float(tol), int(max_iter)


def _check_tensor(X, what):
    """The shape of a data tensor; refuses what is not 3-D, an empty or too long axis, a dtype that is not floating point and
    any value that is not finite (a device tensor is looked at on the device)."""
    if not isinstance(X, torch.Tensor):
        X = np.asarray(X)
        if X.dtype not in (np.float32, np.float64):
            raise ValueError(f'{what}: X must be float32 or float64; got {X.dtype}')
    elif X.dtype not in (torch.float32, torch.float64):
        raise ValueError(f'{what}: X must be float32 or float64; got {X.dtype}')
    if X.ndim != 3:
        raise ValueError(f'{what}: X must be a 3-D tensor (n0, n1, n2); got {X.ndim} dimensions')
    shape = tuple(int(n) for n in X.shape)
    if min(shape) < 1:
        raise ValueError(f'{what}: X has an empty axis: shape {shape}')
    if max(shape) > MAX_AXIS:
        raise ValueError(f'{what}: an axis of {max(shape)} elements; at most XPS_TME_MAX_AXIS = {MAX_AXIS} are supported')
    finite = bool(torch.isfinite(X).all()) if isinstance(X, torch.Tensor) else bool(np.isfinite(X).all())
    if not finite:
        raise ValueError(f'{what}: X holds values that are not finite')
    return X, shape


def _check_count(n, what):
    if not (isinstance(n, (int, np.integer)) and not isinstance(n, bool) and n >= 1):
        raise ValueError(f'{what}: n must be an integer >= 1; got {n!r}')
    return int(n)


def keep_and_scale(ws, shape, total, preserve, eig_tol):
    """(kept, lams): for every axis the number of eigenpairs with lam > eig_tol lam_max and their eigenvalues rescaled so that they
    add up to ``total`` = |R|_F^2 (the three constraint sets are consistent only if their traces agree); an axis outside
    ``preserve`` keeps all n_r with the uniform spectrum total / n_r.  ws[r]: the descending eigenvalues of Sigma_r (None for an
    axis that is not preserved).  Pure numpy."""
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


# ------------------------------------------------------------------------------------------------ the Newton iteration (host half)
class _Newton:
    """The host half of one tensor's fit: Levenberg-Marquardt Newton in theta = log l on the convex
    F(l) = sum_r lam_r . l_r - sum log D.  ``propose()`` gives the multipliers to evaluate, ``receive()`` takes the device sums at
    them.  After every accepted step the multipliers are moved, at unchanged D, to the gauge where the smallest one of every axis
    is the same (a third of the smallest D): all stay positive, which log l needs."""

    def __init__(self, lams, tol, max_iter):
        self.k = [len(v) for v in lams]
        self.cuts = np.cumsum([0] + self.k)
        self.lam = np.concatenate([np.asarray(v, dtype=np.float64) for v in lams])
        n = float(np.prod(self.k))
        self.theta = np.log(np.concatenate([(n / self.k[r]) / (3.0 * np.asarray(lams[r], dtype=np.float64)) for r in range(3)]))
        self.tol, self.max_iter = tol, max_iter
        self.cur, self.mu, self.n_iter, self.trial = None, MU_START, 0, None
        self.done = False

    def split(self, v):
        return [v[self.cuts[r]:self.cuts[r + 1]] for r in range(3)]

    def propose(self):
        """The next point in l, or None when no step can be formed (singular system: the damping grows and the next call tries
        again; a damping beyond MU_MAX ends the fit)."""
        while True:
            if self.cur is None:
                self.trial = self.theta
                break
            l, g, H = self.cur['l'], self.cur['g'], self.cur['H']
            Ht = l[:, None] * H * l[None, :] + np.diag(g * l)
            try:
                step = np.linalg.solve(Ht + np.diag(self.mu * np.abs(np.diag(Ht))), -(g * l))
            except np.linalg.LinAlgError:
                step = None
            if step is not None and np.isfinite(step).all():
                self.trial = self.theta + step
                break
            self.mu *= 4.0
            if self.mu > MU_MAX:
                self.fail()
        with np.errstate(over='ignore'):
            return np.exp(self.trial)

    def fail(self):
        res = float('nan') if self.cur is None else self.cur['res']
        raise RuntimeError(f'TME: the fit did not converge: largest relative residual {res:.3e} after {self.n_iter} iterations '
                           f'(tol = {self.tol:.1e}, max_iter = {self.max_iter})')

    def receive(self, l, w1, w2, p01, p02, p12, sumlog, bad):
        """The sums of the pass at the proposed l (host float64 arrays)."""
        self.n_iter += 1
        c = self.cuts
        H = np.diag(w2)
        H[c[0]:c[1], c[1]:c[2]] = p01
        H[c[0]:c[1], c[2]:c[3]] = p02
        H[c[1]:c[2], c[2]:c[3]] = p12
        H = np.triu(H) + np.triu(H, 1).T
        g = self.lam - w1
        with np.errstate(invalid='ignore', over='ignore'):
            lin = float(self.lam @ l)
            new = dict(l=l, F=lin - sumlog, scale=abs(lin) + abs(sumlog), res=float(np.max(np.abs(g) / self.lam)), g=g, H=H)
        ok = bad == 0 and np.isfinite(new['F']) and np.isfinite(new['res']) and np.isfinite(H).all()
        if ok and (self.cur is None or new['F'] < self.cur['F']
                   or (new['F'] <= self.cur['F'] + F_FLAT * self.cur['scale'] and new['res'] < self.cur['res'])):
            self.cur, self.mu = new, max(self.mu / 8.0, MU_MIN)
            self.l_eval = l
            mins = [v.min() for v in self.split(l)]                      # the balanced gauge: D as it was
            bal = l.copy()
            for r in range(3):
                bal[c[r]:c[r + 1]] += sum(mins) / 3.0 - mins[r]
            self.theta = np.log(bal)
            new['l'] = bal
        else:
            if self.cur is None:
                raise RuntimeError('TME: the starting point of the fit is not finite; the spectra of the data are out of range')
            self.mu *= 4.0
        if self.cur['res'] <= self.tol:
            self.done = True
        elif self.n_iter >= self.max_iter or self.mu > MU_MAX:
            self.fail()


def _run_newton(solvers):
    """Every solver to convergence: one ragged pass per iteration for all that are still iterating.  Per iteration the multipliers
    go up in ONE upload and the sums come down in ONE download: per tensor k0 + k1 + k2 doubles up and
    2 (k0 + k1 + k2) + k0 k1 + k0 k2 + k1 k2 + 2 doubles down."""
    dev = LA.device()
    while True:
        active = [s for s in solvers if not s.done]
        if not active:
            return
        ls = [s.propose() for s in active]
        sizes = []
        for s in active:
            k0, k1, k2 = s.k
            sizes.append([k0, k1, k2, k0, k1, k2, k0 * k1, k0 * k2, k1 * k2, 2])
        cuts_in = np.cumsum([0] + [len(l) for l in ls])
        l_d = torch.from_numpy(np.concatenate(ls)).to(dev)
        cuts_out = np.cumsum([0] + [n for sz in sizes for n in sz])
        out = torch.empty(int(cuts_out[-1]), dtype=LA.F64, device=dev)
        problems, pos = [], 0
        for s, sz, c0 in zip(active, sizes, cuts_in):
            k0, k1, k2 = s.k
            v = [out[cuts_out[pos + i]:cuts_out[pos + i + 1]] for i in range(10)]
            pos += 10
            off = np.cumsum([0, k0, k1, k2])
            problems.append(dict(l=[l_d[c0 + off[r]:c0 + off[r + 1]] for r in range(3)], w1=v[0:3], w2=v[3:6], p01=v[6].view(k0, k1),
                                 p02=v[7].view(k0, k2), p12=v[8].view(k1, k2), scal=v[9]))
        keep = LA.tme_kron_pass(problems)
        host = out.cpu().numpy()                                         # (synchronises with the stream: `keep` may go)
        pos = 0
        for s, l in zip(active, ls):
            k0, k1, k2 = s.k
            v = [host[cuts_out[pos + i]:cuts_out[pos + i + 1]] for i in range(10)]
            pos += 10
            s.receive(l, np.concatenate(v[0:3]), np.concatenate(v[3:6]), v[6].reshape(k0, k1), v[7].reshape(k0, k2),
                      v[8].reshape(k1, k2), float(v[9][0]), float(v[9][1]))
        del keep


# ------------------------------------------------------------------------------------------------ the estimator
class TME:
    """Tensor maximum entropy surrogates of one data tensor.

    preserve: the axes whose covariance the surrogates keep (an axis that is not named gets the identity basis and a uniform
    spectrum).  center: remove (and give back to every surrogate) the mean along every axis.  eig_tol: eigenpairs of Sigma_r
    with lam <= eig_tol lam_max are dropped (centring makes one eigenvalue per axis zero; a short axis is rank deficient).  tol:
    the fit is converged when max |marginal - lam| / lam <= tol; after max_iter evaluations it raises, with the residual.

    Fitted: shape_, mean_ (device tensor M), total_ (|R|_F^2), eigvals_ (three float64 arrays: the kept, rescaled lam_r), eigvecs_
    (three (n_r, k_r) arrays Q_r), kept_ (k_0, k_1, k_2), multipliers_ (three arrays l_r; determined up to shifts between the axes
    that leave D unchanged), residual_, n_iter_ (evaluations of the box, one ragged launch each)."""

    def __init__(self, preserve=(0, 1, 2), center=True, eig_tol=1e-10, tol=1e-9, max_iter=100):
        self.preserve, self.center, self.eig_tol, self.tol, self.max_iter = preserve, center, eig_tol, tol, max_iter

    def fit(self, X):
        _fit_models([self], [X])
        return self

    def sample(self, n, random_state=None, z=None, dtype=None, max_bytes=2 ** 30):
        """``n`` surrogates as an (n, n0, n1, n2) device tensor (float64; dtype=torch.float32 stores float32 from the last
        product's epilogue).  z: an (n, k0, k1, k2) array or tensor that replaces the draw; otherwise every surrogate takes one
        ``torch.randn`` call on the device from a ``torch.Generator`` seeded with ``random_state`` (None: a seed is drawn from
        torch's global host generator, so ``torch.manual_seed`` still reproduces the run), so the same seed gives the same bits in any chunking.  max_bytes: the budget of the
        temporaries of a chunk of surrogates (at least one surrogate per chunk)."""
        what = 'TME.sample'
        if not hasattr(self, 'multipliers_'):
            raise RuntimeError('Must call fit() before sampling.')
        n = _check_count(n, what)
        if dtype not in (None, torch.float32, torch.float64):
            raise ValueError(f'{what}: dtype must be torch.float32 or torch.float64; got {dtype!r}')
        if not (isinstance(max_bytes, (int, np.integer)) and max_bytes >= 1):
            raise ValueError(f'{what}: max_bytes must be an integer >= 1; got {max_bytes!r}')
        if random_state is not None and not (isinstance(random_state, (int, np.integer)) and not isinstance(random_state, bool)):
            raise ValueError(f'{what}: random_state must be None or an int; got {random_state!r}')
        k = tuple(self.kept_)
        if z is not None:
            zshape = tuple(z.shape) if hasattr(z, 'shape') else np.shape(z)
            if zshape != (n,) + k:
                raise ValueError(f'{what}: z must have shape {(n,) + k}; got {zshape}')
        dev = LA.device()
        n0, n1, n2 = self.shape_
        k0, k1, k2 = k
        if not hasattr(self, '_dev'):                                    # Q_r and l_r on the device, once
            self._dev = ([LA.to_device(np.ascontiguousarray(q)) for q in self.eigvecs_],
                         [LA.to_device(np.ascontiguousarray(v)) for v in self.multipliers_])
        Qs, ls = self._dev
        out = torch.empty((n, n0, n1, n2), dtype=dtype or LA.F64, device=dev)
        step = surrogates_per_chunk(self.shape_, k, max_bytes)
        gen = None
        if z is None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(torch.randint(0, 2 ** 62, (1,)).item()) if random_state is None else int(random_state))
        else:
            z = LA.to_device(z).to(LA.F64)
        M2 = None if self.mean_ is None else self.mean_.view(n0, n1 * n2)
        for s0 in range(0, n, step):
            S = min(step, n - s0)
            if z is None:
                core = torch.empty((S, k0, k1, k2), dtype=LA.F64, device=dev)
                for s in range(S):                                       # one draw per surrogate: the chunking leaves no trace
                    core[s] = torch.randn((k0, k1, k2), dtype=LA.F64, device=dev, generator=gen)
                LA.tme_core_scale(core, ls, out=core)
            else:
                core = LA.tme_core_scale(z[s0:s0 + S].contiguous(), ls)
            t1 = torch.empty((1, S * k0 * k1, n2), dtype=LA.F64, device=dev)
            LA.tme_mode_product(core.view(S * k0 * k1, k2), Qs[2], t1, b_kcontig=True)           # rows (s, i, j) times Q_2^T
            t2 = torch.empty((S * k0, n1, n2), dtype=LA.F64, device=dev)
            LA.tme_mode_product(Qs[1], t1.view(S * k0, k1, n2), t2)                            # Q_1 times every slice (s, i)
            LA.tme_mode_product(Qs[0], t2.view(S, k0, n1 * n2), out[s0:s0 + S].view(S, n0, n1 * n2), add=M2)
        return out


def surrogates_per_chunk(shape, kept, max_bytes):
    """Surrogates whose temporaries (the core and the results of the first two mode products, float64) fit max_bytes; at least 1."""
    n0, n1, n2 = shape
    k0, k1, k2 = kept
    per = 8 * (k0 * k1 * k2 + k0 * k1 * n2 + k0 * n1 * n2)
    return int(max(1, int(max_bytes) // per))


def _fit_models(models, Xs):
    what = 'TME.fit'
    opts = [_check_options(m.preserve, m.center, m.eig_tol, m.tol, m.max_iter, what) for m in models]
    checked = [_check_tensor(X, what) for X in Xs]                       # every refusal before the device
    if not models:
        return
    dev = LA.device()
    Rs, Ms, grams, owner = [], [], [], []
    for i, ((X, shape), (preserve, center, _, _, _)) in enumerate(zip(checked, opts)):
        Xd = LA.to_device(X).to(LA.F64)
        R = Xd
        if center:
            for ax in range(3):
                R = R - R.mean(dim=ax, keepdim=True)
        Rs.append(R)
        Ms.append((Xd - R).contiguous() if center else None)
        for r in preserve:                                               # the unfoldings: one permuted copy of R per axis and fit
            if shape[r] == 1:                                            # Sigma_r is the 1 x 1 matrix |R|_F^2: nothing to diagonalise
                continue
            V =R.movedim(r, 0).reshape(shape[r], -1).contiguous()
            grams.append((V, torch.empty(shape[r], shape[r], dtype=LA.F64, device=dev)))
            owner.append((i, r))
    keep = LA.gram_grouped(grams)                                        # every Sigma_r of every tensor: ONE launch
    totals = torch.stack([(R * R).sum() for R in Rs]).cpu().numpy()      # (synchronises: `keep` may go)
    del keep
    eigs = LA.eigh_psd_batched([G for _, G in grams])
    ws = [[None] * 3 for _ in models]
    Vs = [[None] * 3 for _ in models]
    for (i, r), (w, V) in zip(owner, eigs):
        ws[i][r], Vs[i][r] = w, V
    solvers = []
    for i, (m, (X, shape), (preserve, center, eig_tol, tol, max_iter)) in enumerate(zip(models, checked, opts)):
        total = float(totals[i])
        if not (total > 0 and np.isfinite(total)):
            raise ValueError(f'{what}: the {"centred " if center else ""}tensor is zero: there is no covariance to keep')
        for r in preserve:
            if shape[r] == 1:
                ws[i][r], Vs[i][r] = np.array([total]), np.ones((1, 1))
        kept, lams = keep_and_scale(ws[i], shape, total, preserve, eig_tol)
        m.shape_, m.total_, m.kept_, m.eigvals_ = shape, total, tuple(kept), lams
        m.eigvecs_ = [np.ascontiguousarray(Vs[i][r][:, :kept[r]]) if r in preserve else np.eye(shape[r]) for r in range(3)]
        m.mean_ = Ms[i]
        for attr in ('multipliers_', '_dev'):
            if hasattr(m, attr):
                delattr(m, attr)
        solvers.append(_Newton(lams, tol, max_iter))
    _run_newton(solvers)
    for m, s in zip(models, solvers):
        m.multipliers_ = [v.copy() for v in s.split(s.l_eval)]
        m.residual_, m.n_iter_ = s.cur['res'], s.n_iter


def fit_many(Xs, preserve=(0, 1, 2), center=True, eig_tol=1e-10, tol=1e-9, max_iter=100):
    """A fitted TME for every tensor of ``Xs`` (tensors of different shapes: all patients): ONE Gram launch for every Sigma_r, one
    batched eigendecomposition, and every Newton iteration ONE ragged launch for all tensors that have not converged.  Each
    model is bit for bit what ``TME(...).fit(X)`` gives alone."""
    models = [TME(preserve, center, eig_tol, tol, max_iter) for _ in Xs]
    _fit_models(models, list(Xs))
    return models


def tme_surrogates(X, n, preserve=(0, 1, 2), center=True, eig_tol=1e-10, tol=1e-9, max_iter=100, random_state=None, dtype=None,
                   max_bytes=2 ** 30):
    """``n`` surrogates of ``X`` in one call: ``TME(...).fit(X).sample(n, ...)``.  -> (n, n0, n1, n2) device tensor."""
    _check_count(n, 'tme_surrogates')
    return TME(preserve, center, eig_tol, tol, max_iter).fit(X).sample(n, random_state=random_state, dtype=dtype, max_bytes=max_bytes)
