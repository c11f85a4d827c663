"""Cross-validated search over ``C`` and ``gamma`` of a ``decoders.SVC``, resident on the MI355X.

The reference chooses its decoders by nested cross-validation: every outer fold searches ``C`` in 1e-3..1e5 and ``gamma`` in
1e-4..1e3 of ``make_pipeline(DimRedReshape(PCA), SVC(kernel='rbf', class_weight='balanced'))``, 25 candidates (5 at a time) on 20
inner folds (scripts/aligned_decode_svm_ncv.py:398-402,422-425 and the ``*_subsample.py`` scripts).  ``GridSearchCV`` around
``decoders.SVC`` runs that as one fit per (candidate, fold): an upload, a Gram matrix of nearly the same points, an SMO launch of
k (k - 1) / 2 workgroups, a coefficient assembly, a decision product, a download and a host vote, 500 times per search.  But every
fold's training set is a sub-block of one kernel matrix, every ``gamma`` is an element-wise map of one Gram matrix, every ``C`` is
only another bound vector, and the held-out rows of a fold are rows of the same matrix.  ``SVCSearchCV`` uses that:

per view     (one feature matrix: for a bare ``SVC`` the whole X, the folds being index lists into it; for a pipeline the
             transformed training rows of one (outer parameters, fold) followed by its transformed held-out rows)
             one upload, one Gram product, for rbf one ``xps_rbf_multi_from_gram_f64`` over the view's distinct gamma values;
per chunk    (all models = (candidate, fold) pairs whose kernel matrices fit ``max_kernel_bytes``)
             ONE ``xps_svm_smo_multi_f64`` over all class-pair problems of all models, ONE ``xps_svm_cv_score_f64``, one download
             of the confusion tables and predictions.

Scores, ranks and ``cv_results_`` are assembled on the host from the confusion tables.  The per-fold rules are ``SVC.fit``'s
applied to the fold's training rows (``gamma='scale'``, ``class_weight='balanced'``, class members in original order, libsvm's pair
order, fewer pairs for a fold that lost a class), posed by the builder ``SVC.fit`` uses and solved by the same driver
(decoders/_ovo.py).  There is no CPU fallback.

``batch_pca=True`` takes the ``DimRedReshape(PCA)`` step in front of the SVC into the device problem as well.
With more features than rows a fold's PCA lives on the sample side: the centred Gram matrix of any training set is a sub-block,
centred again, of ONE Gram matrix of all flattened trials (``xps_gram_center_folds_f64``); one eigendecomposition per fold,
Kc_tr,tr = U L U^T, serves every ``n_components`` (they differ in where the spectrum is cut); Z = Kc U_R L_R^-1/2 holds the PCA
scores of the fold's training and held-out rows (``xps_apply_grouped_f64``), the view of a candidate with r components is the
column prefix Z[:, :r], and ``xps_prefix_kernels_f64`` writes the kernel matrices of every prefix and every gamma of a chunk from
one pass over Z.  sklearn's sign rule only flips columns, which neither kernel sees, and ``gamma='scale'`` is n_tr / sum_{i<r} L_i
because the score columns have zero mean and squared norms L_i."""
import numpy as np
import torch
from scipy.stats import rankdata
from sklearn.base import BaseEstimator, clone
from sklearn.model_selection import ParameterGrid, check_cv
from sklearn.pipeline import Pipeline

from .._dev import stream
from .._lib import call, lib
from ..alignment import _linalg as LA
from ..alignment.pca import PCA, PCA_SPECTRUM_LIMIT, count_components, gram_ratio
from ..decomposition.DimRedReshape import DimRedReshape
from . import _ovo
from .svm import SVC

BATCHED = ('C', 'gamma')                    # the SVC parameters that are batched on the device; every other key is an outer key
SCORINGS = (None, 'accuracy', 'balanced_accuracy')


def check_class_count(k):
    """The class counts every cross-validated driver takes: sklearn's refusal of one class, the scoring kernel's of more than 64."""
    if k < 2:
        raise ValueError('The number of classes has to be greater than one; got 1 class')
    if k > 64:
        raise ValueError(f'the scoring kernel takes 2..64 classes; got {k}')


# ------------------------------------------------------------------------------------------------ candidates (host)
def expand_candidates(param_grid, candidates):
    """The list of candidate dicts: ``ParameterGrid(param_grid)`` in its order, or the explicit ``candidates`` as given."""
    if (param_grid is None) == (candidates is None):
        raise ValueError('give exactly one of param_grid and candidates')
    out = [dict(c) for c in candidates] if candidates is not None else list(ParameterGrid(param_grid))
    if not out:
        raise ValueError('no candidates to search')
    return out


def svc_of(estimator):
    """(the searched SVC, the prefix of its parameters, the earlier pipeline steps or None)."""
    if isinstance(estimator, SVC):
        return estimator, '', None
    if isinstance(estimator, Pipeline) and estimator.steps and isinstance(estimator.steps[-1][1], SVC):
        name, svc = estimator.steps[-1]
        return svc, name + '__', (list(estimator.steps[:-1]) or None)
    raise TypeError('estimator must be a decoders.SVC or a sklearn Pipeline whose last step is a decoders.SVC (the search runs on the '
                    f'device; there is no CPU fallback); got {type(estimator).__name__}')


def split_params(estimator, params):
    """One candidate -> (batched, outer): ``batched`` holds ``C`` / ``gamma`` under their bare names, ``outer`` every other key as
    it was given.  A key that addresses another parameter of the SVC (or replaces the SVC step) raises ``ValueError``, and so does a
    key the estimator does not have."""
    svc, prefix, _ = svc_of(estimator)
    svc_names = set(svc.get_params(deep=False))
    known = estimator.get_params(deep=True)
    batched, outer = {}, {}
    for key, val in params.items():
        if key not in known:
            raise ValueError(f'Invalid parameter {key!r} for estimator {estimator}.')
        if prefix and key == prefix[:-2]:
            raise ValueError(f'{key!r} replaces the searched SVC: only its C and gamma can be searched')
        name = key[len(prefix):] if key.startswith(prefix) else None
        if name in BATCHED:
            batched[name] = val
        elif name is not None and (prefix or name in svc_names):
            raise ValueError(f'{key!r} addresses the SVC parameter {name!r}: the device search batches C and gamma only; set the '
                             'others on the estimator')
        else:
            outer[key] = val
    return batched, outer


def pca_step_of(estimator):
    """(name, step) of the ``DimRedReshape(PCA)`` in front of the SVC, the only pipeline ``batch_pca=True`` takes."""
    if not (isinstance(estimator, Pipeline) and len(estimator.steps) == 2 and isinstance(estimator.steps[0][1], DimRedReshape)
            and isinstance(estimator.steps[1][1], SVC)):
        raise ValueError('batch_pca=True needs a Pipeline of exactly DimRedReshape(dim_red) and a decoders.SVC')
    red = estimator.steps[0][1].dim_red
    if not (isinstance(red, type) and issubclass(red, PCA)):
        raise ValueError(f'batch_pca=True needs DimRedReshape over alignment.PCA or a subclass of it; got {red!r}')
    return estimator.steps[0]


def split_params_pca(estimator, params):
    """``split_params`` with ``<dimredreshape>__n_components`` batched too (as ``n_components``); any other outer key raises."""
    name, _ = pca_step_of(estimator)
    batched, outer = split_params(estimator, params)
    key = name + '__n_components'
    if key in outer:
        batched['n_components'] = outer.pop(key)
    if outer:
        raise ValueError(f'batch_pca=True batches {key!r}, C and gamma only; got {sorted(outer)}')
    return batched, outer


def pca_cut(L, n_components, n_tr, d):
    """(r, batched) of one (fold, ``n_components``) from the fold's Gram-side spectrum L (descending, n_tr values): r by the PCA
    class's rule (None for ``n_components=None``); batched when 1 <= r <= min(n_tr - 1, d) and L[r - 1] >= L[0] /
    PCA_SPECTRUM_LIMIT, else the pair takes the per-(outer, fold) view path."""
    if n_components is None:
        return None, False
    L = np.clip(np.asarray(L, dtype=np.float64), 0.0, None)
    r = count_components(n_components, gram_ratio(L, n_tr, d), n_tr, d)
    return r, bool(1 <= r <= min(n_tr - 1, d) and L[0] > 0 and L[r - 1] >= L[0] / PCA_SPECTRUM_LIMIT)


def pca_gamma(kernel, gamma, L, r, n_tr):
    """``_ovo.gamma_value`` on the r leading PCA scores of a fold's n_tr training rows, from the spectrum alone: the score columns
    have zero mean and squared norms L_i, so ``'scale'`` = 1 / (r * var) = n_tr / sum_{i<r} L_i; ``'auto'`` = 1 / r."""
    if kernel == 'rbf' and isinstance(gamma, str) and gamma in ('scale', 'auto'):
        total = float(np.clip(np.asarray(L[:r], dtype=np.float64), 0.0, None).sum())
        return (n_tr / total if total != 0 else 1.0) if gamma == 'scale' else 1.0 / r
    return _ovo.gamma_value(kernel, gamma, None)


def _same_outer(a, b):
    if a.keys() != b.keys():
        return False
    try:
        return all(a[key] is b[key] or bool(a[key] == b[key]) for key in a)
    except (TypeError, ValueError):
        return False


# ------------------------------------------------------------------------------------------------ the plan (host)
class Plan:
    """Host description of a search: ``views`` (feature matrices), ``matrices`` ((view, gamma value) per kernel matrix, the matrices
    of a view adjacent) and ``models`` (one dict per (candidate, fold): cand, fold, matrix, C, problems, test_pos, ytest)."""

    def __init__(self):
        self.views, self.matrices, self.models = [], [], []
        self._matrix_of = {}
        self.pca = None                                         # build_plan_pca: a matrix's view is then ('pca', fold, r) or an index

    def rows(self, view):
        return self.pca['n_all'][view[1]] if isinstance(view, tuple) else self.views[view].shape[0]

    def matrix(self, view, gamma):
        key = (view, float(gamma))
        if key not in self._matrix_of:
            self._matrix_of[key] = len(self.matrices)
            self.matrices.append(key)
        return self._matrix_of[key]

    def matrix_bytes(self):
        return [8 * self.rows(v) ** 2 for v, _ in self.matrices]


def _fold_problems(svc, yi, classes, tr, train_pos):
    """SVC.fit's rules on THIS fold's rows: its classes, its 'balanced' weights; pair_a / pair_b as indices into ``classes``."""
    cls, yi_tr = np.unique(yi[tr], return_inverse=True)
    problems = _ovo.pair_problems(yi_tr, train_pos, _ovo.class_weights(svc.class_weight, classes[cls], yi_tr))
    problems['pair_a'], problems['pair_b'] = (cls[problems[key]].astype(np.int32) for key in ('pair_a', 'pair_b'))
    return problems


def _fit_view(estimator, outer, X, yi, classes, tr, te):
    """What Pipeline.fit / predict do with the steps before the last, for one (outer combination, fold): the transformed
    training rows followed by the transformed held-out rows, and the training rows alone."""
    steps = [step for _, step in clone(estimator).set_params(**outer).steps[:-1] if step is not None and step != 'passthrough']
    Ztr, Zte = X[tr], X[te]
    for step in steps:
        Ztr = step.fit_transform(Ztr, classes[yi[tr]]) if hasattr(step, 'fit_transform') else step.fit(Ztr, classes[yi[tr]]).transform(Ztr)
        Zte = step.transform(Zte) if len(te) else Zte
    Ztr = np.asarray(Ztr, dtype=np.float64)
    Zte = np.asarray(Zte, dtype=np.float64) if len(te) else np.empty((0, Ztr.shape[1]))
    if Ztr.ndim != 2 or Zte.shape[1] != Ztr.shape[1]:
        raise ValueError('the pipeline steps before the SVC must produce (n_samples, n_features)')
    return np.ascontiguousarray(np.vstack([Ztr, Zte])), Ztr


def build_plan(estimator, split_candidates, X, yi, classes, splits, plan=None, only=None):
    """Views, kernel matrices and models of a search (host; a pipeline's earlier steps are fitted here, once per (outer
    combination, fold)).  ``split_candidates``: ``split_params`` of every candidate; ``yi``: class indices of y into ``classes``.
    ``plan`` / ``only`` (build_plan_pca): append to this plan, and only the (candidate, fold) pairs of ``only``."""
    svc, _, pre = svc_of(estimator)
    plan = Plan() if plan is None else plan
    gamma_cache = {}

    def add_models(view, fold, cands, Ztr, train_pos, test_pos, tr, te):
        problems = _fold_problems(svc, yi, classes, tr, train_pos)
        for c in cands:
            batched = split_candidates[c][0]
            spec = batched.get('gamma', svc.gamma)
            key = (view, fold, spec if isinstance(spec, str) else float(spec))
            if key not in gamma_cache:                          # SVC.fit's rule on the features handed to THIS fold's fit
                gamma_cache[key] = _ovo.gamma_value(svc.kernel, spec, Ztr)
            plan.models.append(dict(cand=c, fold=fold, matrix=plan.matrix(view, gamma_cache[key]), C=float(batched.get('C', svc.C)),
                                    problems=problems, test_pos=np.asarray(test_pos, dtype=np.int32), ytest=yi[te].astype(np.int32)))

    if pre is None:
        Z = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        if Z.ndim != 2:
            raise ValueError('X must be (n_samples, n_features)')
        for _, outer in split_candidates:
            if outer:
                raise ValueError(f'Invalid parameters {sorted(outer)} for a bare SVC')
        plan.views.append(Z)
        for f, (tr, te) in enumerate(splits):
            add_models(0, f, range(len(split_candidates)), Z[tr], tr, te, tr, te)
        return plan
    outers = []                                                 # distinct outer combinations, in order of first appearance
    for c, (_, outer) in enumerate(split_candidates):
        for known, members in outers:
            if _same_outer(known, outer):
                members.append(c)
                break
        else:
            outers.append((outer, [c]))
    for outer, members in outers:
        for f, (tr, te) in enumerate(splits):
            wanted = members if only is None else [c for c in members if (c, f) in only]
            if not wanted:
                continue
            view, Ztr = _fit_view(estimator, outer, X, yi, classes, tr, te)
            plan.views.append(view)
            add_models(len(plan.views) - 1, f, wanted, Ztr, np.arange(len(tr)), len(tr) + np.arange(len(te)), tr, te)
    return plan


def build_plan_pca(estimator, split_candidates, X, yi, classes, splits):
    """The plan of a ``batch_pca=True`` search.  Device: one upload of X, the column mean, one Gram product, one centring launch
    for all folds, ONE eigh_psd_batched call (one launch per distinct training size the one-workgroup Jacobi takes, one ragged
    batch for the larger ones) and one grouped apply for the scores Z_f of every fold.
    Host: per (fold, n_components) the cut r and whether it is batched (``pca_cut``), gamma from the spectrum (``pca_gamma``).  A
    batched (fold, r, gamma) is a kernel matrix whose view is ``('pca', fold, r)``; the other (candidate, fold) pairs go through
    ``build_plan``'s views inside the same plan.  ``split_candidates``: ``split_params_pca`` of every candidate."""
    svc = svc_of(estimator)[0]
    name, red = pca_step_of(estimator)
    if X.ndim < 2:
        raise ValueError('X must be (n_samples, ...)')
    Xd = LA.to_device(X.reshape(X.shape[0], -1))
    d = Xd.shape[1]
    Xc = Xd.to(LA.F64) - LA.col_mean(Xd)                        # about ONE provisional centre, the all-trial mean
    G = LA.dgemm(Xc, Xc, tb=True)
    Kc, offs = LA.gram_center_folds(G, splits)
    Kc_h = Kc.cpu().numpy()
    nf = len(splits)
    n_tr = [len(tr) for tr, _ in splits]
    n_all = [len(tr) + len(te) for tr, te in splits]
    blocks = [Kc_h[offs[f]:offs[f + 1]].reshape(n_all[f], n_tr[f])[:n_tr[f]] for f in range(nf)]
    eig = LA.eigh_psd_batched([0.5 * (blocks[f] + blocks[f].T) for f in range(nf)])     # folds differ in size by one: one call
    plan = Plan()
    ncs = [b.get('n_components', red.n_components) for b, _ in split_candidates]
    comps = np.zeros((len(ncs), nf), dtype=np.int64)
    cuts, fallbacks, only = [], [], set()
    for f in range(nf):
        cuts.append({})
        for c, nc in enumerate(ncs):
            if nc not in cuts[f]:
                cuts[f][nc] = pca_cut(eig[f][0], nc, n_tr[f], d)
                if not cuts[f][nc][1]:
                    fallbacks.append((f, nc))
            if not cuts[f][nc][1]:
                only.add((c, f))
    R = [max([r for r, ok in cuts[f].values() if ok], default=0) for f in range(nf)]
    W_h = [eig[f][1][:, :R[f]] / np.sqrt(eig[f][0][:R[f]]) for f in range(nf)]                  # U_R L_R^-1/2
    w_off = np.concatenate([[0], np.cumsum([w.size for w in W_h])])
    z_off = np.concatenate([[0], np.cumsum([n_all[f] * R[f] for f in range(nf)])])
    Wbuf = LA.to_device(np.concatenate([w.ravel() for w in W_h] + [np.zeros(1)]))
    Zbuf = torch.empty(int(z_off[-1]) + 1, dtype=torch.float64, device=Xd.device)
    Z = [Zbuf[z_off[f]:z_off[f + 1]].view(n_all[f], R[f]) if R[f] else None for f in range(nf)]
    LA.apply_grouped([(Kc[offs[f]:offs[f + 1]].view(n_all[f], n_tr[f]), None, Wbuf[w_off[f]:w_off[f + 1]].view(n_tr[f], R[f]), Z[f])
                      for f in range(nf) if R[f]])
    plan.pca = dict(n_all=n_all, Z=Z, spectra=[e[0] for e in eig])
    for f, (tr, te) in enumerate(splits):
        problems = _fold_problems(svc, yi, classes, tr, np.arange(n_tr[f]))
        for c, (batched, _) in enumerate(split_candidates):
            r, ok = cuts[f][ncs[c]]
            if not ok:
                continue
            comps[c, f] = r
            gamma = pca_gamma(svc.kernel, batched.get('gamma', svc.gamma), eig[f][0], r, n_tr[f])
            plan.models.append(dict(cand=c, fold=f, matrix=plan.matrix(('pca', f, r), gamma), C=float(batched.get('C', svc.C)),
                                    problems=problems, test_pos=(n_tr[f] + np.arange(len(te))).astype(np.int32),
                                    ytest=yi[te].astype(np.int32)))
    if only:                                                    # the pairs that are not batched: the per-(outer, fold) views
        key = name + '__n_components'
        first = len(plan.models)
        build_plan(estimator, [({k: v for k, v in b.items() if k != 'n_components'}, {key: b['n_components']} if 'n_components' in b else {})
                               for b, _ in split_candidates], X, yi, classes, splits, plan=plan, only=only)
        for mod in plan.models[first:]:
            comps[mod['cand'], mod['fold']] = plan.views[plan.matrices[mod['matrix']][0]].shape[1]
    plan.pca.update(n_components=comps, fallbacks=fallbacks)
    return plan


def cut_chunks(matrix_bytes, max_bytes):
    """Consecutive runs of kernel matrices whose bytes stay within ``max_bytes``: a list of lists of matrix indices that covers
    every matrix exactly once, in order.  A single matrix beyond the limit raises."""
    chunks, cur, used = [], [], 0
    for m, b in enumerate(matrix_bytes):
        if b > max_bytes:
            raise ValueError(f'one kernel matrix takes {b} bytes: max_kernel_bytes={max_bytes} is too small')
        if cur and used + b > max_bytes:
            chunks.append(cur)
            cur, used = [], 0
        cur.append(m)
        used += b
    if cur:
        chunks.append(cur)
    return chunks


# ------------------------------------------------------------------------------------------------ scores (host)
def scores_from_confusion(conf, scoring):
    """conf (..., k, k) int, rows = true class -> the score of each table.  ``'accuracy'``: trace / count.
    ``'balanced_accuracy'``: sklearn's definition, the mean recall over the classes that have held-out rows."""
    conf = np.asarray(conf)
    flat = conf.reshape(-1, conf.shape[-2], conf.shape[-1])
    out = np.empty(len(flat))
    for i, table in enumerate(flat):
        with np.errstate(divide='ignore', invalid='ignore'):
            if scoring == 'balanced_accuracy':
                per_class = np.diag(table) / table.sum(axis=1)
                per_class = per_class[~np.isnan(per_class)]
                out[i] = np.mean(per_class) if len(per_class) else np.nan
            else:
                out[i] = np.float64(np.trace(table)) / np.float64(table.sum())
    return out.reshape(conf.shape[:-2])


def assemble_results(candidates, scores):
    """sklearn's ``cv_results_`` (the test-score part) from the (n_candidates, n_splits) score table: per-split scores, mean, std,
    and ``rank_test_score`` by ``rankdata(-mean, method='min')`` with NaN means ranked last, as ``GridSearchCV`` does."""
    scores = np.asarray(scores, dtype=np.float64)
    res = {}
    names = []
    for cand in candidates:
        names += [name for name in cand if name not in names]
    for name in sorted(names):
        col = np.ma.MaskedArray(np.empty(len(candidates), dtype=object), mask=True)
        for i, cand in enumerate(candidates):
            if name in cand:
                col[i] = cand[name]
        res[f'param_{name}'] = col
    res['params'] = [dict(c) for c in candidates]
    for f in range(scores.shape[1]):
        res[f'split{f}_test_score'] = scores[:, f].copy()
    means = np.average(scores, axis=1)
    res['mean_test_score'] = means
    res['std_test_score'] = np.sqrt(np.average((scores - means[:, None]) ** 2, axis=1))
    if np.isnan(means).all():
        rank = np.ones_like(means, dtype=np.int32)
    else:
        rank = rankdata(-np.nan_to_num(means, nan=np.nanmin(means) - 1), method='min').astype(np.int32, copy=False)
    res['rank_test_score'] = rank
    return res


# ------------------------------------------------------------------------------------------------ the device
def _cat(dicts, key):
    return np.concatenate([d[key] for d in dicts])


def solve_and_score(Kbuf, models, mn, mbase, tol, svc_max_iter, k):
    """The models (dicts with problems, C, test_pos, ytest) whose kernel matrices lie in the flat buffer ``Kbuf``, model s's a square
    matrix of mn[s] rows at element mbase[s]: three uploads (index lists, matrix offsets and leading dimensions, bounds), ONE
    ``xps_svm_smo_multi_f64`` over all class-pair problems, ONE ``xps_svm_cv_score_f64`` and one download.  Returns
    (conf (S, k, k), pred, tst_off): model s's predictions of its held-out rows are pred[tst_off[s]:tst_off[s + 1]]."""
    dev = Kbuf.device
    S = len(models)
    probs = [mod['problems'] for mod in models]
    nprob = np.array([len(p['npos']) for p in probs], dtype=np.int64)
    mn, mbase = np.asarray(mn, dtype=np.int64), np.asarray(mbase, dtype=np.int64)
    sizes_q = _cat(probs, 'sizes')
    off = np.concatenate([[0], np.cumsum(sizes_q)])
    tst_off = np.concatenate([[0], np.cumsum([len(mod['test_pos']) for mod in models])])
    mod_off = np.concatenate([[0], np.cumsum(nprob)])
    if max(off[-1], tst_off[-1]) > np.iinfo(np.int32).max:
        raise ValueError('the chunk holds more training points than int32 offsets address: lower max_kernel_bytes')
    Q, T = int(mod_off[-1]), int(tst_off[-1])
    idx_d, off_d, npos_d, pa_d, pb_d, tst_d, yt_d, mn_d = _ovo.upload_int32(
        [_cat(probs, 'idx'), off, _cat(probs, 'npos'), _cat(probs, 'pair_a'), _cat(probs, 'pair_b'), _cat(models, 'test_pos'),
         _cat(models, 'ytest'), mn], dev)
    longs_d = torch.from_numpy(np.concatenate([np.repeat(mbase, nprob), np.repeat(mn, nprob), mbase, mn])).to(dev)
    kbase_d, kld_d, mbase_d, mld_d = longs_d[:Q], longs_d[Q:2 * Q], longs_d[2 * Q:2 * Q + S], longs_d[2 * Q + S:]
    cb = np.concatenate([_ovo.bounds(mod['C'], mod['problems']) for mod in models])
    alpha, rho, _ = _ovo.smo(Kbuf, idx_d, off_d, npos_d, int(sizes_q.max()), cb, tol, svc_max_iter, kbase_d, kld_d)
    out = torch.empty(S * k * k + max(T, 1), dtype=torch.int32, device=dev)                     # conf, then pred: one download
    ws_bytes = int(lib().xps_svm_cv_score_f64_workspace(S))
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    mod_off_h, tst_off_h = mod_off.astype(np.int32), tst_off.astype(np.int32)                   # host arrays of the call
    call('xps_svm_cv_score_f64', Kbuf.data_ptr(), mbase_d.data_ptr(), mld_d.data_ptr(), mn_d.data_ptr(), idx_d.data_ptr(), off_d.data_ptr(),
         npos_d.data_ptr(), alpha.data_ptr(), rho.data_ptr(), pa_d.data_ptr(), pb_d.data_ptr(), mod_off_h.ctypes.data, tst_d.data_ptr(),
         yt_d.data_ptr(), tst_off_h.ctypes.data, S, k, out.data_ptr() + 4 * S * k * k, out.data_ptr(), None, 0, ws.data_ptr(), ws_bytes,
         stream())
    host = out.cpu().numpy()                                    # (synchronises: the host offset arrays were read before this returns)
    return host[:S * k * k].reshape(S, k, k), host[S * k * k:S * k * k + T], tst_off


def _run_chunk(plan, mats, kernel, tol, svc_max_iter, k):
    """Kernel matrices ``mats`` (adjacent per view) and all their models: per view an upload, a Gram product and, for rbf, one
    multi-gamma launch; then one SMO launch, one scoring launch and one download.  Returns (models, conf (S, k, k), pred, tst_off)."""
    dev = LA.device()
    sizes = [plan.rows(plan.matrices[m][0]) ** 2 for m in mats]
    base = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    Kbuf = torch.empty(int(base[-1]), dtype=torch.float64, device=dev)
    slot = {m: i for i, m in enumerate(mats)}
    i = 0
    prefixes = {}                                               # fold -> {cut r: [(gamma, first element in Kbuf)]} of the batched PCA
    while i < len(mats):                                        # one pass per view of the chunk
        v = plan.matrices[mats[i]][0]
        if isinstance(v, tuple):
            prefixes.setdefault(v[1], {}).setdefault(v[2], []).append((plan.matrices[mats[i]][1], int(base[i])))
            i += 1
            continue
        j = i
        while j < len(mats) and plan.matrices[mats[j]][0] == v:
            j += 1
        Zd = torch.from_numpy(plan.views[v]).to(dev)
        n = Zd.shape[0]
        G = LA.dgemm(Zd, Zd, tb=True)
        if kernel == 'rbf':
            sq = _ovo.row_sq_norms(Zd)
            gammas = torch.tensor([plan.matrices[m][1] for m in mats[i:j]], dtype=torch.float64).to(dev)
            call('xps_rbf_multi_from_gram_f64', G.data_ptr(), G.stride(0), sq.data_ptr(), sq.data_ptr(), n, n, gammas.data_ptr(), j - i,
                 Kbuf.data_ptr() + 8 * int(base[i]), n, n * n, stream())
        else:
            Kbuf[int(base[i]):int(base[i]) + n * n].copy_(G.view(-1))
        i = j
    # every (fold, cut, gamma) matrix of the chunk from ONE launch; its host tables live until the download below
    tables = LA.prefix_kernels([(plan.pca['Z'][f], sorted(cuts.items())) for f, cuts in prefixes.items()], kernel == 'rbf', Kbuf)  # noqa: F841
    models = [mod for mod in plan.models if mod['matrix'] in slot]
    models.sort(key=lambda mod: slot[mod['matrix']])            # (stable: plan order inside a matrix)
    mn = [plan.rows(plan.matrices[mod['matrix']][0]) for mod in models]
    mbase = [base[slot[mod['matrix']]] for mod in models]
    return (models,) + solve_and_score(Kbuf, models, mn, mbase, tol, svc_max_iter, k)


class SearchTail:
    """What a fitted search is, whatever it searched: the ``scoring`` refusal, sklearn's result attributes from the confusion
    tables, and ``predict`` / ``score`` through the refitted ``best_estimator_`` (each class refits in its own ``fit``)."""

    def _check_scoring(self):
        if self.scoring not in SCORINGS:
            raise ValueError(f"scoring must be None, 'accuracy' or 'balanced_accuracy'; got {self.scoring!r}")

    def _set_results(self, candidates, conf, test_predictions, classes):
        """conf (n_candidates, n_splits, k, k), rows = true class; test_predictions: per split (test_idx, labels (n_candidates,
        len(test_idx)))."""
        self.cv_results_ = assemble_results(candidates, scores_from_confusion(conf, self.scoring))
        self.cv_confusion_ = conf
        self.cv_test_predictions_ = test_predictions
        self.n_splits_ = conf.shape[1]
        self.classes_ = classes
        self.best_index_ = int(self.cv_results_['rank_test_score'].argmin())
        self.best_params_ = self.cv_results_['params'][self.best_index_]
        self.best_score_ = float(self.cv_results_['mean_test_score'][self.best_index_])

    def _best(self):
        if not hasattr(self, 'best_estimator_'):
            raise AttributeError(f'this {type(self).__name__} has no best_estimator_: it was not fitted, or refit=False')
        return self.best_estimator_

    def predict(self, X):
        return self._best().predict(X)

    def score(self, X, y):
        return self._best().score(X, y)


class SVCSearchCV(SearchTail, BaseEstimator):
    """``GridSearchCV`` for ``decoders.SVC`` (bare, or the last step of a sklearn ``Pipeline``) with all folds and all ``C`` /
    ``gamma`` candidates trained and scored as one device problem per chunk.

    ``param_grid`` (a dict or list of dicts, expanded by ``ParameterGrid``) or ``candidates`` (an explicit list of parameter dicts:
    what a Bayesian or random search hands over); ``cv``: an int (``StratifiedKFold``), a splitter or an iterable of (train, test),
    which need not partition the rows; ``scoring``: ``None`` / ``'accuracy'`` or ``'balanced_accuracy'``.  Keys other than the SVC's
    ``C`` and ``gamma`` are outer keys: the earlier pipeline steps are fitted once per (outer combination, fold).  A key addressing
    another SVC parameter raises ``ValueError``; ``sample_weight`` and other fit parameters, ``return_train_score`` and a
    non-default ``error_score`` raise ``NotImplementedError``.

    After ``fit``: ``cv_results_``, ``best_index_``, ``best_params_``, ``best_score_``, ``n_splits_``, ``classes_``,
    ``cv_test_predictions_`` (per split: ``(test_idx, labels (n_candidates, len(test_idx)))``), ``cv_confusion_`` (n_candidates,
    n_splits, k, k; rows = true class) and, with ``refit``, ``best_estimator_`` = ``clone(estimator).set_params(**best_params_)
    .fit(X, y)``, to which ``predict`` / ``decision_function`` / ``score`` delegate.

    ``batch_pca=True`` (the estimator must be a Pipeline of exactly ``DimRedReshape(alignment.PCA or a subclass)`` and a
    ``decoders.SVC``): ``<dimredreshape>__n_components`` is batched beside ``C`` and ``gamma`` -- one Gram matrix of the flattened
    trials serves all folds, one eigendecomposition per fold all component counts -- and any other outer key raises
    ``ValueError``.  Adds ``pca_n_components_`` (n_candidates x n_splits) and ``pca_fallbacks_``, the (fold, n_components) pairs
    that took the per-fold fit instead (``None``, a cut at or beyond the training rows' rank, or below the spectrum limit)."""

    def __init__(self, estimator, param_grid=None, *, candidates=None, cv=5, scoring=None, refit=True, max_kernel_bytes=2 ** 30,
                 return_train_score=False, error_score=np.nan, batch_pca=False):
        self.estimator = estimator
        self.param_grid = param_grid
        self.candidates = candidates
        self.cv = cv
        self.scoring = scoring
        self.refit = refit
        self.max_kernel_bytes = max_kernel_bytes
        self.return_train_score = return_train_score
        self.error_score = error_score
        self.batch_pca = batch_pca

    def _check_settings(self):
        svc, _, _ = svc_of(self.estimator)
        svc._check_settings()
        self._check_scoring()
        if self.return_train_score:
            raise NotImplementedError('return_train_score is not implemented on the HIP path')
        if not (isinstance(self.error_score, float) and np.isnan(self.error_score)):
            raise NotImplementedError('error_score is not implemented on the HIP path: a failing fit raises')
        return svc

    def fit(self, X, y, **fit_params):
        if fit_params:
            raise NotImplementedError(f'fit parameters ({sorted(fit_params)}) are not implemented on the HIP path')
        svc = self._check_settings()
        candidates = expand_candidates(self.param_grid, self.candidates)
        split_candidates = [(split_params_pca if self.batch_pca else split_params)(self.estimator, c) for c in candidates]
        X, y = np.asarray(X), np.asarray(y)
        if y.ndim != 1 or X.shape[0] != y.shape[0]:
            raise ValueError('X must have one row per element of y (n_samples,)')
        classes, yi = np.unique(y, return_inverse=True)
        k = len(classes)
        check_class_count(k)
        cv = check_cv(self.cv, y, classifier=True)
        splits = [(np.asarray(tr), np.asarray(te)) for tr, te in cv.split(X, y)]
        if not splits:
            raise ValueError('cv yields no split')
        plan = (build_plan_pca if self.batch_pca else build_plan)(self.estimator, split_candidates, X, yi, classes, splits)
        # ---- the device: no loop over candidates or folds below, only over views (uploads) and chunks
        conf = np.zeros((len(candidates), len(splits), k, k), dtype=np.int32)
        labels = [np.empty((len(candidates), len(te)), dtype=classes.dtype) for _, te in splits]
        for mats in cut_chunks(plan.matrix_bytes(), int(self.max_kernel_bytes)):
            models, conf_c, pred_c, tst_off = _run_chunk(plan, mats, svc.kernel, svc.tol, svc.max_iter, k)
            for s, mod in enumerate(models):
                conf[mod['cand'], mod['fold']] = conf_c[s]
                labels[mod['fold']][mod['cand']] = classes[pred_c[tst_off[s]:tst_off[s + 1]]]
        self._set_results(candidates, conf, [(te, lab) for (_, te), lab in zip(splits, labels)], classes)
        if self.batch_pca:
            self.pca_n_components_, self.pca_fallbacks_ = plan.pca['n_components'], plan.pca['fallbacks']
        if self.refit:
            self.best_estimator_ = clone(self.estimator).set_params(**self.best_params_).fit(X, y)
        return self

    def decision_function(self, X):
        return self._best().decision_function(X)
