"""Fold-batched PCA -> CCA alignment: every fold of a k-fold split as ONE device problem.

``process_aligner`` (nn_models/data_utils/datamodules.py) fits, per fold, 1 + P PCAs and P pairwise CCAs.  For splits
whose test sets partition the trials (KFold / StratifiedKFold) all of that is shared structure:

  * the held-out groups partition the target's trials, so a fold's covariance is a sum of the OTHER groups' moment
    matrices  M_g = sum (x - c)(x - c)^T,  s_g = sum (x - c)  about one provisional centre c (the all-trial mean):
        S_f = sum_{g != f} M_g,  t_f = sum_{g != f} s_g,  mean_f = c + t_f / n_f,  cov_f = (S_f - t_f t_f^T / n_f) / (n_f - 1);
  * the pooled patients' PCAs and condition means do not depend on the fold: they are computed once;
  * a fold's condition means are means over its training trials of Z_f = (X - mean_f) W_f;
  * the P x k CCA problems are independent d x d problems once C_aa, C_bb, C_ab exist.

Launch list of one ``fit_folds`` (k folds, P pooled patients; no Python loop over folds issues device calls except the
Jacobi launches -- one per distinct matrix size -- and the chunks of ``max_bytes``):
  per pooled patient (once)   PCA (colsum, xcov; ONE Jacobi call for all patients), transform, condition means
  1  xps_colsum_f64           provisional centre
  2  xps_xcov_grouped_f64     group moments, one problem per trial group
  3  xps_loo_sum_f64          fold sums
  4  Jacobi                   k fold covariances in one launch (above 128 channels: one ragged batch)
  5  xps_apply_grouped_f64    Z_f for every fold + the training rows of every fold's pooled tensor (float32)
  6  xps_cnd_avg_folds_f64    every fold's condition means
  7  xps_xcov_grouped_f64     C_aa, C_bb, C_ab of every (fold, patient)
  8  Jacobi                   C_aa / C_bb by size, then the whitened K matrices by shape
  9  xps_apply_grouped_f64    every (fold, patient) aligned block into its slab of the fold's pooled tensor
With ``append_heldout=True`` every fold's pooled tensor has the fold's held-out trials after the pooled rows; they are more
entries of launch 5 (the fold's own mean and components), so the list above does not grow.
The O(d^2) glue (whitening factors, M_a, M_b, the maps) is host numpy, as in ``AlignCCA._cca_device``.
``fit_folds_multi`` fits a list of ``n_components`` values: launches 1-4 and the pooled patients' eigendecompositions once
(nothing in them looks at ``n_components``), then launches 5-9 once with the folds of every distinct set of component counts
side by side -- a (value, fold) pair is just another fold to them.

Only ``AlignCCA``'s defaults (type='class', return_space='b_to_a') are supported.
"""
import numpy as np
import torch

from . import _linalg as LA
from .AlignCCA import _cca_device, cca_tail
from .alignment_utils import _cnd_avg_device, label2str
from .pca import PCA, count_components, eig_many, sign_rule

SPECTRUM_LIMIT = 1e10          # above it rank_from_gram_eigs and LAPACK's rank rule may disagree: the problem takes _cca_device


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, 'detach') else np.asarray(x)


def _csr(inv, n):
    """CSR (order, start) of the members of each of n classes, members in their original order."""
    order = np.argsort(inv, kind='stable').astype(np.int64)
    start = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=n))]).astype(np.int64)
    return order, start


def _runs(idx):
    """[(first trial, count, position)]: `idx` cut into runs of consecutive trials."""
    if len(idx) == 0:
        return []
    first = np.concatenate([[0], np.flatnonzero(np.diff(idx) != 1) + 1])
    count = np.diff(np.concatenate([first, [len(idx)]]))
    return [(int(idx[a]), int(c), int(a)) for a, c in zip(first, count)]


class FoldPlan:
    """Index tables of a fold-batched fit (pure numpy).

    n_trials, n_folds, n_groups   n_groups = n_folds, + 1 when some trials are in no test set (never held out)
    splits                        [(train, test)] int64 arrays as given
    group_of_trial                (N,) fold whose test set holds the trial (n_folds for an uncovered trial)
    group_order, group_start      CSR: the trials of group g are group_order[group_start[g]:group_start[g + 1]], ascending
    cond_keys[f]                  sorted unique condition keys (label2str) of fold f's training trials
    cond_order[f], cond_start[f]  CSR over cond_keys[f]: ORIGINAL trial indices, in `train` order inside a condition
    pool_keys[p]                  sorted unique condition keys of pooled patient p
    shared[f][p]                  (i_a, i_b) of np.intersect1d(cond_keys[f], pool_keys[p], return_indices=True)
    train_runs[f]                 [(first trial, count, destination row)]: `train` cut into runs of consecutive trials
    """


def fold_plan(y_align, pool_align_labels, splits):
    """Validate `splits` and build the index tables (no device needed).  `splits` must be (train, test) pairs with
    pairwise disjoint test sets and every train set the complement of its test set in range(N), as KFold /
    StratifiedKFold produce; anything else raises ValueError (keep the per-fold path for those)."""
    keys = label2str(y_align)
    N = len(keys)
    plan = FoldPlan()
    plan.n_trials = N
    plan.splits = [(np.asarray(_np(tr), dtype=np.int64).reshape(-1), np.asarray(_np(te), dtype=np.int64).reshape(-1))
                   for tr, te in splits]
    plan.n_folds = F = len(plan.splits)
    if F < 1:
        raise ValueError('fold_plan: no splits given')
    group = np.full(N, F, dtype=np.int64)
    for f, (tr, te) in enumerate(plan.splits):
        if len(te) and (te.min() < 0 or te.max() >= N) or len(tr) and (tr.min() < 0 or tr.max() >= N):
            raise ValueError(f'fold_plan: fold {f} has a trial index outside range({N})')
        if len(np.unique(te)) != len(te) or (group[te] != F).any():
            raise ValueError(f'fold_plan: the test set of fold {f} overlaps another test set (or repeats a trial); '
                             'the fold-batched path needs pairwise disjoint test sets')
        group[te] = f
        comp = np.setdiff1d(np.arange(N), te)
        if len(tr) != len(comp) or not np.array_equal(np.sort(tr), comp):
            raise ValueError(f'fold_plan: the train set of fold {f} is not the complement of its test set in range({N})')
        if len(tr) == 0:
            raise ValueError(f'fold_plan: fold {f} has no training trials')
    plan.group_of_trial = group
    plan.n_groups = G = F + int((group == F).any())
    plan.group_order, plan.group_start = _csr(group, G)
    plan.pool_keys = [np.unique(label2str(ya)) for ya in pool_align_labels]
    plan.cond_keys, plan.cond_order, plan.cond_start, plan.shared, plan.train_runs = [], [], [], [], []
    for tr, _ in plan.splits:
        uniq, inv = np.unique(keys[tr], return_inverse=True)
        order, start = _csr(np.asarray(inv).reshape(-1), len(uniq))
        plan.cond_keys.append(uniq)
        plan.cond_order.append(tr[order])
        plan.cond_start.append(start)
        plan.shared.append([tuple(np.intersect1d(uniq, pk, assume_unique=True, return_indices=True)[1:])
                            for pk in plan.pool_keys])
        plan.train_runs.append(_runs(tr))
    return plan


class _FoldProjector:
    """What ``process_aligner`` returns as its fitted target PCA, for one fold: mean_, components_, n_components_ and
    ``transform`` (device apply, like alignment.PCA)."""

    def __init__(self, fa, f):
        self.mean_, self.components_, self.n_components_ = fa.pca_mean_[f], fa.pca_components_[f], fa.n_components_[f]
        self.explained_variance_ = fa.explained_variance_[f]
        self._mean_d, self._W_d = fa._mean_d[f], fa._W_d[f]

    def transform_device(self, Xd, out_f32=False):
        return LA.apply(Xd, self._W_d, self._mean_d, out_f32=out_f32)

    def transform(self, X):
        return LA.like_input(self.transform_device(LA.to_device(X)), X)


class FoldAlignment:
    """Result of ``fit_folds``.  Per fold f: pca_mean_[f], pca_components_[f], n_components_[f], explained_variance_[f],
    explained_variance_ratio_all_[f] (the whole curve); per pooled patient p: M_a_[f][p], M_b_[f][p], canon_corrs_[f][p] and
    the device map maps_[f][p] = M_b pinv(M_a); fallbacks_ = [(f, p)] sent through the per-problem ``_cca_device``."""

    def train_pool(self, f):
        """Pooled float32 device tensor of fold f: the target's training trials in `train` order, then each aligned
        pooled patient in order -- ``process_aligner``'s X_pool."""
        return self._pool[f]

    def pool_with_heldout(self, f):
        """(rows, held-out trials) of a fit with ``append_heldout=True``: the float32 device tensor whose first rows are
        ``train_pool(f)`` and whose last len(held-out) rows are the fold's held-out target trials in fold f's latent space
        (``project(f, held-out)``, bit for bit), and the original indices of those trials, in the order of the rows."""
        if self._pool_all is None:
            raise ValueError('pool_with_heldout: the folds were fitted without append_heldout=True')
        return self._pool_all[f], self.plan.splits[f][1]

    def project(self, f, idx):
        """Target trials `idx` in fold f's latent space, float32 device tensor (len(idx), T, n_components_[f])."""
        idx = torch.as_tensor(np.asarray(_np(idx), dtype=np.int64), device=self._X.device)
        return LA.apply(self._X[idx], self._W_d[f], self._mean_d[f], out_f32=True)

    def projector(self, f):
        return _FoldProjector(self, f)


def _fold_chunks(bytes_per_fold, max_bytes):
    chunks, cur, tot = [], [], 0
    for f, b in enumerate(bytes_per_fold):
        if cur and tot + b > max_bytes:
            chunks.append(cur)
            cur, tot = [], 0
        cur.append(f)
        tot += b
    if cur:
        chunks.append(cur)
    return chunks


def _by_shape(mats):
    groups = {}
    for i, m in enumerate(mats):
        groups.setdefault(m.shape, []).append(i)
    return groups


def _solve_cca(probs):
    """probs: list of dicts with Caa, Cbb, Cab (centred sums) and n rows.  Fills M_a, M_b, S, map (host) or marks
    'fallback'.  Jacobi launches: one per distinct C size, one per distinct K shape."""
    mats = [p['Caa'] for p in probs] + [p['Cbb'] for p in probs]
    eig = [None] * len(mats)
    for shape, idx in _by_shape(mats).items():
        for i, r in zip(idx, LA.eigh_psd_batched(np.stack([mats[i] for i in idx]))):
            eig[i] = r
    ready = []
    for j, p in enumerate(probs):
        (wa, Va), (wb, Vb) = eig[j], eig[len(probs) + j]
        if not (wa[-1] > 0 and wb[-1] > 0 and wa[0] <= SPECTRUM_LIMIT * wa[-1] and wb[0] <= SPECTRUM_LIMIT * wb[-1]):
            p['fallback'] = True
            continue
        ra, rb = LA.rank_from_gram_eigs(wa, p['n']), LA.rank_from_gram_eigs(wb, p['n'])
        p['Wa'], p['Wb'] = Va[:, :ra] / np.sqrt(wa[:ra]), Vb[:, :rb] / np.sqrt(wb[:rb])
        p['K'] = p['Wa'].T @ p['Cab'] @ p['Wb']
        ready.append(p)
    for shape, idx in _by_shape([p['K'] for p in ready]).items():
        for i, (U, S, Vt) in zip(idx, LA.svd_batched(np.stack([ready[i]['K'] for i in idx]))):
            p = ready[i]
            p['M_a'], p['M_b'], p['S'] = cca_tail(p['Wa'], p['Wb'], U, S, Vt)
            p['map'] = p['M_b'] @ np.linalg.pinv(p['M_a'])


class _Shared:
    """What a fold-batched fit computes before ``n_components`` is looked at (launches 1-4 and the pooled patients' covariances
    and eigendecompositions): ``fit_folds_multi`` computes it once for all its values."""


def _ratio_curve(w):
    """(clipped spectrum, its explained-variance-ratio curve): alignment.PCA's rule on the covariance side."""
    w = np.clip(w, 0.0, None)
    total = w.sum()
    return w, (w / total if total > 0 else np.zeros_like(w))


def resolve_counts(n_components, fold_spectra, fold_rows, n_channels, pool_spectra, pool_shapes):
    """The component counts one ``n_components`` value resolves to (host only): (the target's count in every fold, the count of
    every pooled patient), two tuples.  ``fold_spectra[f]`` / ``pool_spectra[p]``: the descending covariance spectra;
    ``fold_rows[f]``: the rows (trials x time) of fold f's training set; ``pool_shapes[p]``: (rows, channels) of patient p.  Two
    values with equal tuples give the same fit."""
    folds = tuple(count_components(n_components, _ratio_curve(w)[1], int(n), n_channels) for w, n in zip(fold_spectra, fold_rows))
    pools = tuple(count_components(n_components, _ratio_curve(w)[1], int(n), int(d)) for w, (n, d) in zip(pool_spectra, pool_shapes))
    return folds, pools


def distinct_counts(n_components_list, fold_spectra, fold_rows, n_channels, pool_spectra, pool_shapes):
    """(index, firsts): ``index[i]`` numbers the distinct fit entry i of the list resolves to (``resolve_counts``), in order of first
    appearance, and ``firsts[j]`` is the position in the list of the first entry of fit j (host only)."""
    seen, index, firsts = {}, [], []
    for i, nc in enumerate(n_components_list):
        key = resolve_counts(nc, fold_spectra, fold_rows, n_channels, pool_spectra, pool_shapes)
        if key not in seen:
            seen[key] = len(firsts)
            firsts.append(i)
        index.append(seen[key])
    return index, firsts


def fit_folds(X, y_align, pool_data, splits, n_components=0.95, max_bytes=2 ** 30, append_heldout=False):
    """Fit the target PCA and the P pairwise CCA alignments of EVERY fold of `splits` at once.

    X (N, T, C) float32 / float64 tensor or ndarray; y_align the target's alignment labels; pool_data the list of
    (x, y, y_align) the data modules take; splits as ``fold_plan`` requires.  Folds are processed in chunks whose
    per-fold device arrays (Z_f and the pooled tensor) stay within `max_bytes`.  ``append_heldout``: every fold's pooled tensor is
    allocated with room for the fold's held-out trials after the pooled rows and launch 5 fills them (``pool_with_heldout``);
    ``train_pool`` and everything else are what they are without it.  Returns a ``FoldAlignment``."""
    return _finish(_prepare(X, y_align, pool_data, splits), [n_components], max_bytes, append_heldout)[0]


def fit_folds_multi(X, y_align, pool_data, splits, n_components_list, max_bytes=2 ** 30, append_heldout=False):
    """``[fit_folds(..., n_components=v) for v in n_components_list]``, value for value and bit for bit, with the work that does
    not depend on ``n_components`` done once for the list: the group moments, the fold covariances and every eigendecomposition of
    a covariance (launches 1-4 and the pooled patients' PCAs).  Entries that resolve to the same component counts -- the same
    target count in every fold and the same count for every pooled patient (``resolve_counts``) -- are ONE ``FoldAlignment``
    object.  Launches 5-9 run once per chunk of ``max_bytes`` with the folds of all distinct objects side by side (a (value, fold)
    pair is just another fold to them), and a pooled patient's PCA scores once per distinct component count."""
    sh = _prepare(X, y_align, pool_data, splits)
    n_components_list = list(n_components_list)
    index, firsts = distinct_counts(n_components_list, [w for w, _ in sh.fold_eig], sh.n_f, sh.C, [e[0] for e, _, _, _ in sh.pool_eig],
                                    [(n, d) for _, _, n, d in sh.pool_eig])
    fits = _finish(sh, [n_components_list[i] for i in firsts], max_bytes, append_heldout)
    return [fits[j] for j in index]


def _prepare(X, y_align, pool_data, splits):
    Xd = LA.to_device(X)
    if Xd.dim() != 3:
        raise ValueError('fit_folds: X must be (trials, time, channels)')
    N, T, C = Xd.shape
    X2 = Xd.view(N * T, C)
    plan = fold_plan(_np(y_align), [_np(ya) for _, _, ya in pool_data], splits)
    if plan.n_trials != N:
        raise ValueError('fit_folds: y_align and X differ in their number of trials')
    F, G = plan.n_folds, plan.n_groups

    # pooled patients: covariance and eigendecomposition once
    pool_d = [LA.to_device(x) for x, _, _ in pool_data]
    for xd in pool_d:
        if xd.dim() != 3 or xd.shape[1] != T:
            raise ValueError('fit_folds: every pooled patient must be (trials, T, channels) with the target\'s T')
    pool_eig = eig_many([xd.reshape(-1, xd.shape[-1]) for xd in pool_d])

    # 1-3: group moments about the all-trial mean -> fold sums
    c_d = LA.col_mean(X2)
    moments, offs = LA.xcov_grouped([(X2, X2, plan.group_order[plan.group_start[g]:plan.group_start[g + 1]] * T,
                                      plan.group_order[plan.group_start[g]:plan.group_start[g + 1]] * T, T, c_d, c_d)
                                     for g in range(G)])
    sums = LA.loo_sum(moments.view(G, -1), F).cpu().numpy()
    c = c_d.cpu().numpy()
    n_f = sums[:, -1]
    t_f = sums[:, C * C:C * C + C]
    S_f = sums[:, :C * C].reshape(F, C, C)
    covs = (S_f - t_f[:, :, None] * t_f[:, None, :] / n_f[:, None, None]) / (n_f - 1)[:, None, None]
    covs = 0.5 * (covs + covs.transpose(0, 2, 1))
    means = c[None, :] + t_f / n_f[:, None]

    # 4: the k fold eigendecompositions
    sh = _Shared()
    sh.Xd, sh.X2, sh.plan, sh.pool_data, sh.pool_d, sh.pool_eig = Xd, X2, plan, pool_data, pool_d, pool_eig
    sh.N, sh.T, sh.C, sh.n_f, sh.means = N, T, C, n_f, means
    sh.fold_eig = list(LA.eigh_psd_batched(covs))
    sh.pool_cache = {}
    return sh


def _cut(sh, n_components):
    """What one ``n_components`` value cuts from the shared spectra (host rules, one upload): the FoldAlignment with its fold PCAs,
    and per pooled patient the scores Zp and condition means Bp of its PCA -- computed once per (patient, component count)."""
    plan, C, n_f, means = sh.plan, sh.C, sh.n_f, sh.means
    F = plan.n_folds
    Zp, Bp = [], []
    for p, ((e, mean, n, d), xd, (_, _, ya), pk) in enumerate(zip(sh.pool_eig, sh.pool_d, sh.pool_data, plan.pool_keys)):
        k = count_components(n_components, _ratio_curve(e[0])[1], n, d)
        if (p, k) not in sh.pool_cache:
            pca = PCA(n_components=n_components)._fit_from_eig(e, mean, n, d)
            assert pca.n_components_ == k
            z = pca.transform_device(xd)
            uniq, b = _cnd_avg_device(z, label2str(_np(ya)))
            assert np.array_equal(uniq, pk)
            sh.pool_cache[p, k] = (z.reshape(-1, z.shape[-1]), b.reshape(-1, b.shape[-1]))
        Zp.append(sh.pool_cache[p, k][0])
        Bp.append(sh.pool_cache[p, k][1])

    fa = FoldAlignment()
    fa.plan, fa._X = plan, sh.Xd
    fa.pca_mean_, fa.pca_components_, fa.n_components_, fa.explained_variance_ = [], [], [], []
    fa.explained_variance_ratio_all_ = []
    for f, (w, V) in enumerate(sh.fold_eig):
        # alignment.PCA's rules on the covariance side: ratio curve w / sum(w), its component count, sklearn's sign rule
        w, ratio = _ratio_curve(w)
        k = count_components(n_components, ratio, int(n_f[f]), C)
        comps = V.T[:k].copy()
        fa.pca_mean_.append(means[f].copy())
        fa.pca_components_.append(comps * sign_rule(comps, 1)[:, None])
        fa.n_components_.append(k)
        fa.explained_variance_.append(w[:k])
        fa.explained_variance_ratio_all_.append(ratio)
    kf = fa.n_components_
    flat = LA.to_device(np.concatenate([np.concatenate([fa.pca_mean_[f], fa.pca_components_[f].T.reshape(-1)])
                                        for f in range(F)]))
    fa._mean_d, fa._W_d, o = [], [], 0
    for f in range(F):
        fa._mean_d.append(flat[o:o + C])
        fa._W_d.append(flat[o + C:o + C + C * kf[f]].view(C, kf[f]))
        o += C + C * kf[f]
    return fa, Zp, Bp


def _finish(sh, values, max_bytes, append_heldout):
    """Everything of a fit that depends on ``n_components``, for a list of values at once: the cuts of the spectra (``_cut``) and
    launches 5-9, to which a (value, fold) pair is just another fold.  Returns one FoldAlignment per value."""
    Xd, X2, plan, N, T = sh.Xd, sh.X2, sh.plan, sh.N, sh.T
    F, P = plan.n_folds, len(sh.pool_data)
    pool_n = [xd.shape[0] for xd in sh.pool_d]
    n_train = [len(tr) for tr, _ in plan.splits]
    pool_rows = [n + sum(pool_n) for n in n_train]
    held_rows = [len(te) if append_heldout else 0 for _, te in plan.splits]
    fas, Zps, Bps = [], [], []
    for v in values:
        fa, Zp, Bp = _cut(sh, v)
        fa._pool = [None] * F
        fa._pool_all = [None] * F if append_heldout else None
        fa.M_a_ = [[None] * P for _ in range(F)]
        fa.M_b_ = [[None] * P for _ in range(F)]
        fa.canon_corrs_ = [[None] * P for _ in range(F)]
        fa.maps_ = [[None] * P for _ in range(F)]
        fa.fallbacks_ = []
        fas.append(fa)
        Zps.append(Zp)
        Bps.append(Bp)
    jobs = [(e, f) for e in range(len(values)) for f in range(F)]              # a job: fold f under value e
    kj = {(e, f): fas[e].n_components_[f] for e, f in jobs}
    per_job = [N * T * kj[j] * 8 + (pool_rows[j[1]] + held_rows[j[1]]) * T * kj[j] * 4 for j in jobs]
    for chunk in _fold_chunks(per_job, max_bytes):
        chunk = [jobs[i] for i in chunk]
        # 5: Z_f and the target rows of the pooled tensors
        Z, entries = {}, []
        for e, f in chunk:
            fa, k = fas[e], kj[e, f]
            Z[e, f] = torch.empty(N * T, k, dtype=LA.F64, device=Xd.device)
            whole = torch.empty(pool_rows[f] + held_rows[f], T, k, dtype=torch.float32, device=Xd.device)
            fa._pool[f] = whole[:pool_rows[f]]
            entries.append((X2, fa._mean_d[f], fa._W_d[f], Z[e, f]))
            p2 = whole.view(-1, k)
            runs = plan.train_runs[f]
            if append_heldout:
                fa._pool_all[f] = whole
                runs = runs + [(a, cnt, pool_rows[f] + dst) for a, cnt, dst in _runs(plan.splits[f][1])]
            entries += [(X2[a * T:(a + cnt) * T], fa._mean_d[f], fa._W_d[f], p2[dst * T:(dst + cnt) * T]) for a, cnt, dst in runs]
        LA.apply_grouped(entries)
        # 6: condition means of every fold
        A, segs = {}, []
        for e, f in chunk:
            nc, k = len(plan.cond_keys[f]), kj[e, f]
            A[e, f] = torch.empty(nc, T, k, dtype=LA.F64, device=Xd.device)
            Zv = Z[e, f].view(N, T * k)
            st, od = plan.cond_start[f], plan.cond_order[f]
            segs += [(Zv, A[e, f][ci], od[st[ci]:st[ci + 1]]) for ci in range(nc)]
        LA.cnd_avg_folds(segs)
        # 7: C_aa, C_bb, C_ab of every (fold, patient) with at least as many rows as columns
        probs, table = [], []
        for e, f in chunk:
            k, Bp = kj[e, f], Bps[e]
            A2 = A[e, f].view(-1, k)
            for p in range(P):
                i_a, i_b = plan.shared[f][p]
                rows = len(i_a) * T
                pr = {'e': e, 'f': f, 'p': p, 'n': rows}
                probs.append(pr)
                if rows < max(k, Bp[p].shape[1]):
                    pr['fallback'] = True
                    continue
                ba, bb = i_a * T, i_b * T
                table += [(A2, A2, ba, ba, T, None, None), (Bp[p], Bp[p], bb, bb, T, None, None),
                          (A2, Bp[p], ba, bb, T, None, None)]
        out, offs = LA.xcov_grouped(table)
        out = out.cpu().numpy()
        j = 0
        for pr in probs:
            if pr.get('fallback'):
                continue
            k, dp = kj[pr['e'], pr['f']], Bps[pr['e']][pr['p']].shape[1]
            for name in ('Caa', 'Cbb', 'Cab'):
                blk = out[offs[j]:offs[j + 1]]
                j += 1
                da = k if name != 'Cbb' else dp
                db = k if name == 'Caa' else dp
                Cm, sa, sb = blk[:da * db].reshape(da, db), blk[da * db:da * db + da], blk[da * db + da:da * db + da + db]
                Cm = Cm - np.outer(sa, sb) / blk[-1]
                pr[name] = Cm if name == 'Cab' else 0.5 * (Cm + Cm.T)
        # 8: the d x d problems
        _solve_cca([pr for pr in probs if not pr.get('fallback')])
        for pr in probs:
            e, f, p = pr['e'], pr['f'], pr['p']
            fa, k, Bp = fas[e], kj[e, f], Bps[e]
            if pr.get('fallback'):
                # rank-deficient or badly conditioned: the per-problem route on the same L matrices
                i_a, i_b = plan.shared[f][p]
                dev = Xd.device
                La = A[e, f][torch.from_numpy(i_a).to(dev)].reshape(-1, k)
                Lb = Bp[p].view(-1, T, Bp[p].shape[1])[torch.from_numpy(i_b).to(dev)].reshape(-1, Bp[p].shape[1])
                pr['M_a'], pr['M_b'], pr['S'] = _cca_device(La, Lb)
                pr['map'] = LA.dgemm(LA.to_device(pr['M_b']), LA.to_device(LA.pinv_small(pr['M_a']))).cpu().numpy()
                fa.fallbacks_.append((f, p))
            fa.M_a_[f][p], fa.M_b_[f][p], fa.canon_corrs_[f][p] = pr['M_a'], pr['M_b'], pr['S']
        # 9: every aligned block into its slab
        flat = LA.to_device(np.concatenate([np.ascontiguousarray(pr['map']).reshape(-1) for pr in probs])) if probs else None
        entries, o = [], 0
        for pr in probs:
            e, f, p = pr['e'], pr['f'], pr['p']
            fa, k = fas[e], kj[e, f]
            dp = Bps[e][p].shape[1]
            fa.maps_[f][p] = flat[o:o + dp * k].view(dp, k)
            o += dp * k
            r0 = (n_train[f] + sum(pool_n[:p])) * T
            entries.append((Zps[e][p], None, fa.maps_[f][p], fa._pool[f].view(-1, k)[r0:r0 + pool_n[p] * T]))
        LA.apply_grouped(entries)
        del Z, A
    return fas
