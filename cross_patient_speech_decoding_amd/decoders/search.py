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
(decoders/_ovo.py).  There is no CPU fallback."""
import numpy as np
import torch
from scipy.stats import rankdata
from sklearn.base import BaseEstimator, clone
from sklearn.model_selection import ParameterGrid, check_cv
from sklearn.pipeline import Pipeline

from .._dev import stream
from .._lib import call, lib
from ..alignment import _linalg as LA
from . import _ovo
from .svm import SVC

BATCHED = ('C', 'gamma')                    # the SVC parameters that are batched on the device; every other key is an outer key
SCORINGS = (None, 'accuracy', 'balanced_accuracy')


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

    def matrix(self, view, gamma):
        key = (view, float(gamma))
        if key not in self._matrix_of:
            self._matrix_of[key] = len(self.matrices)
            self.matrices.append(key)
        return self._matrix_of[key]

    def matrix_bytes(self):
        return [8 * self.views[v].shape[0] ** 2 for v, _ in self.matrices]


def build_plan(estimator, split_candidates, X, yi, classes, splits):
    """Views, kernel matrices and models of a search (host; a pipeline's earlier steps are fitted here, once per (outer
    combination, fold)).  ``split_candidates``: ``split_params`` of every candidate; ``yi``: class indices of y into ``classes``."""
    svc, _, pre = svc_of(estimator)
    plan = Plan()
    gamma_cache = {}

    def add_models(view, fold, cands, Ztr, train_pos, test_pos, tr, te):
        cls, yi_tr = np.unique(yi[tr], return_inverse=True)   # SVC.fit's rules on THIS fold's rows: its classes, its 'balanced' weights
        problems = _ovo.pair_problems(yi_tr, train_pos, _ovo.class_weights(svc.class_weight, classes[cls], yi_tr))
        problems['pair_a'], problems['pair_b'] = (cls[problems[key]].astype(np.int32) for key in ('pair_a', 'pair_b'))
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
            steps = [step for _, step in clone(estimator).set_params(**outer).steps[:-1] if step is not None and step != 'passthrough']
            Ztr, Zte = X[tr], X[te]
            for step in steps:                                  # what Pipeline.fit / predict do with the steps before the last
                Ztr = step.fit_transform(Ztr, classes[yi[tr]]) if hasattr(step, 'fit_transform') else step.fit(Ztr, classes[yi[tr]]).transform(Ztr)
                Zte = step.transform(Zte) if len(te) else Zte
            Ztr = np.asarray(Ztr, dtype=np.float64)
            Zte = np.asarray(Zte, dtype=np.float64) if len(te) else np.empty((0, Ztr.shape[1]))
            if Ztr.ndim != 2 or Zte.shape[1] != Ztr.shape[1]:
                raise ValueError('the pipeline steps before the SVC must produce (n_samples, n_features)')
            plan.views.append(np.ascontiguousarray(np.vstack([Ztr, Zte])))
            add_models(len(plan.views) - 1, f, members, Ztr, np.arange(len(tr)), len(tr) + np.arange(len(te)), tr, te)
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


def _run_chunk(plan, mats, kernel, tol, svc_max_iter, k):
    """Kernel matrices ``mats`` (adjacent per view) and all their models: per view an upload, a Gram product and, for rbf, one
    multi-gamma launch; then one SMO launch, one scoring launch and one download.  Returns (models, conf (S, k, k), pred, tst_off)."""
    dev = LA.device()
    sizes = [plan.views[plan.matrices[m][0]].shape[0] ** 2 for m in mats]
    base = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    Kbuf = torch.empty(int(base[-1]), dtype=torch.float64, device=dev)
    slot = {m: i for i, m in enumerate(mats)}
    i = 0
    while i < len(mats):                                        # one pass per view of the chunk
        v = plan.matrices[mats[i]][0]
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
    models = [mod for mod in plan.models if mod['matrix'] in slot]
    models.sort(key=lambda mod: slot[mod['matrix']])            # (stable: plan order inside a matrix)
    S = len(models)
    probs = [mod['problems'] for mod in models]
    nprob = np.array([len(p['npos']) for p in probs], dtype=np.int64)
    mn = np.array([plan.views[plan.matrices[mod['matrix']][0]].shape[0] for mod in models], dtype=np.int64)
    mbase = np.array([base[slot[mod['matrix']]] for mod in models], dtype=np.int64)
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
    return models, host[:S * k * k].reshape(S, k, k), host[S * k * k:S * k * k + T], tst_off


class SVCSearchCV(BaseEstimator):
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
    .fit(X, y)``, to which ``predict`` / ``decision_function`` / ``score`` delegate."""

    def __init__(self, estimator, param_grid=None, *, candidates=None, cv=5, scoring=None, refit=True, max_kernel_bytes=2 ** 30,
                 return_train_score=False, error_score=np.nan):
        self.estimator = estimator
        self.param_grid = param_grid
        self.candidates = candidates
        self.cv = cv
        self.scoring = scoring
        self.refit = refit
        self.max_kernel_bytes = max_kernel_bytes
        self.return_train_score = return_train_score
        self.error_score = error_score

    def _check_settings(self):
        svc, _, _ = svc_of(self.estimator)
        svc._check_settings()
        if self.scoring not in SCORINGS:
            raise ValueError(f"scoring must be None, 'accuracy' or 'balanced_accuracy'; got {self.scoring!r}")
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
        split_candidates = [split_params(self.estimator, c) for c in candidates]
        X, y = np.asarray(X), np.asarray(y)
        if y.ndim != 1 or X.shape[0] != y.shape[0]:
            raise ValueError('X must have one row per element of y (n_samples,)')
        classes, yi = np.unique(y, return_inverse=True)
        k = len(classes)
        if k < 2:
            raise ValueError('The number of classes has to be greater than one; got 1 class')
        if k > 64:
            raise ValueError(f'the scoring kernel takes 2..64 classes; got {k}')
        cv = check_cv(self.cv, y, classifier=True)
        splits = [(np.asarray(tr), np.asarray(te)) for tr, te in cv.split(X, y)]
        if not splits:
            raise ValueError('cv yields no split')
        plan = build_plan(self.estimator, split_candidates, X, yi, classes, splits)
        # ---- the device: no loop over candidates or folds below, only over views (uploads) and chunks
        conf = np.zeros((len(candidates), len(splits), k, k), dtype=np.int32)
        labels = [np.empty((len(candidates), len(te)), dtype=classes.dtype) for _, te in splits]
        for mats in cut_chunks(plan.matrix_bytes(), int(self.max_kernel_bytes)):
            models, conf_c, pred_c, tst_off = _run_chunk(plan, mats, svc.kernel, svc.tol, svc.max_iter, k)
            for s, mod in enumerate(models):
                conf[mod['cand'], mod['fold']] = conf_c[s]
                labels[mod['fold']][mod['cand']] = classes[pred_c[tst_off[s]:tst_off[s + 1]]]
        scores = scores_from_confusion(conf, self.scoring)
        self.cv_results_ = assemble_results(candidates, scores)
        self.cv_confusion_ = conf
        self.cv_test_predictions_ = [(te, lab) for (_, te), lab in zip(splits, labels)]
        self.n_splits_ = len(splits)
        self.classes_ = classes
        self.best_index_ = int(self.cv_results_['rank_test_score'].argmin())
        self.best_params_ = self.cv_results_['params'][self.best_index_]
        self.best_score_ = float(self.cv_results_['mean_test_score'][self.best_index_])
        if self.refit:
            self.best_estimator_ = clone(self.estimator).set_params(**self.best_params_).fit(X, y)
        return self

    # ------------------------------------------------------------------ the refitted estimator
    def _best(self):
        if not hasattr(self, 'best_estimator_'):
            raise AttributeError('this SVCSearchCV has no best_estimator_: it was not fitted, or refit=False')
        return self.best_estimator_

    def predict(self, X):
        return self._best().predict(X)

    def decision_function(self, X):
        return self._best().decision_function(X)

    def score(self, X, y):
        return self._best().score(X, y)
