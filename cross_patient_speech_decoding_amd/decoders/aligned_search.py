"""Cross-validated search over ``n_comp``, ``C`` and ``gamma`` of an aligned decoder, resident on the MI355X.

The reference's nested-CV experiment chooses the settings of ``crossPtDecoder_sepAlign(pool, SVC, AlignCCA)`` with
``BayesSearchCV(model, param_grid, cv=cv, n_points=5, refit=False).fit(X, y, y_align=...)`` (scripts/aligned_decode_svm_ncv.py:
388-413): per (candidate, fold) a PCA of the target's training trials, a CCA alignment of every pooled patient, pooling, an SVC fit
and a prediction.  ``cross_val_decode`` runs all folds of ONE candidate as one device problem; ``AlignedSVCSearchCV`` puts the
candidates beside the folds:

per partition  (a run of splits whose test sets partition the trials: one repeat of a repeated k-fold)
               ``alignment.fit_folds_multi`` over the candidates' ``n_comp`` values with the held-out trials appended (the moments,
               covariances and eigendecompositions once; launches 5-9 of ``fit_folds`` once, with the folds of every distinct set
               of component counts side by side);
               a VIEW per distinct (alignment, fold): the rows of ``pool_with_heldout(f)``, with ``fold_decode.fold_layout``'s
               class-pair problems, weights and bootstrap draws for the view's own feature count;
               ONE ``xps_var_grouped_f64`` and one download for all views some candidate asks ``gamma='scale'`` of;
per chunk      (kernel matrices, and for rbf the Gram matrices of their views, within ``max_kernel_bytes``)
               ONE ``xps_gram_grouped_f64`` over the chunk's views,
               rbf only: ONE ``xps_rbf_grouped_from_gram_f64`` over the chunk's distinct (view, gamma value) matrices,
               ONE ``search.solve_and_score`` with one model per (candidate, fold, estimator): three uploads, ONE
               ``xps_svm_smo_multi_f64``, ONE ``xps_svm_cv_score_f64``, one download.

Candidates that differ only in ``C`` share a kernel matrix, candidates that differ only in ``gamma`` share a Gram matrix, and the
launch count does not depend on the number of candidates.  The ensemble vote and the per-split confusion table of a bagged model are
taken on the host from the one download.  There is no CPU fallback."""
import numpy as np
import torch
from sklearn.base import BaseEstimator, clone
from sklearn.model_selection import check_cv

from ..alignment import _linalg as LA
from ..alignment.fold_align import fit_folds_multi
from . import _ovo
from .fold_decode import _Features, check_model, confusion, cut_partitions, fold_layout, host_vote
from .search import SCORINGS, assemble_results, cut_chunks, expand_candidates, scores_from_confusion, solve_and_score

BATCHED = ('C', 'gamma')                    # the SVC parameters a candidate may set, beside the wrapper's n_comp


# ------------------------------------------------------------------------------------------------ candidates (host)
def decoder_prefix(ensemble):
    """The prefix of the searched SVC's parameters in the wrapper's ``get_params``: a bare SVC or the estimator of an ensemble."""
    return 'decoder__' if ensemble is None else 'decoder__estimator__'


def supported_keys(ensemble):
    return ['n_comp'] + [decoder_prefix(ensemble) + name for name in BATCHED]


def split_params(model, params):
    """One candidate -> a dict with the keys it sets among ``n_comp``, ``C``, ``gamma`` (bare names).  A key that is no parameter of
    the model raises sklearn's "Invalid parameter" ``ValueError``; a parameter the search does not batch raises a ``ValueError``
    that names the supported keys."""
    _, ens = check_model(model)
    known = model.get_params(deep=True)
    keys = supported_keys(ens)
    out = {}
    for key, val in params.items():
        if key not in known:
            raise ValueError(f'Invalid parameter {key!r} for estimator {type(model).__name__}. Valid parameters are: {sorted(known)!r}.')
        if key not in keys:
            raise ValueError(f'{key!r} is a parameter of the model that AlignedSVCSearchCV does not search; the supported keys are {keys}: '
                             'set the others on the model')
        out[key.rsplit('__', 1)[-1]] = val
    if 'C' in out and not float(out['C']) > 0:
        raise ValueError(f"C must be positive; got {out['C']!r}")
    return out


def gamma_spec(kernel, spec):
    """How a candidate's gamma enters the plan: None for a linear kernel (accepted, without effect, as in sklearn), the string for
    'scale' / 'auto', else the float."""
    if kernel != 'rbf':
        return None
    return spec if isinstance(spec, str) else float(spec)


# ------------------------------------------------------------------------------------------------ the plan (host)
class AlignedPlan:
    """Host description of one partition of the search.  ``views``: the distinct (alignment, fold) pairs; ``matrices``: (view,
    gamma value or None for linear) per kernel matrix, the matrices of a view adjacent; ``models``: one dict per (candidate, fold):
    cand, fold, view, matrix, C.  ``rows[v]``: the rows of view v's matrices."""

    def matrix_bytes(self):
        return [8 * self.rows[v] ** 2 for v, _ in self.matrices]


def scale_views(settings, align_of, n_folds, kernel):
    """The (alignment, fold) pairs some candidate asks ``gamma='scale'`` of, in view order (host only)."""
    if kernel != 'rbf':
        return []
    wanted = sorted({align_of[c] for c, st in enumerate(settings) if st['gamma'] == 'scale'})
    return [(a, f) for a in wanted for f in range(n_folds)]


def build_plan(settings, align_of, rows_of, kernel, gamma_of):
    """``settings[c]``: candidate c's resolved dict(C=..., gamma=...) (``gamma_spec``); ``align_of[c]``: the index of its alignment
    among the distinct ones; ``rows_of[a][f]``: the rows of fold f's pooled tensor under alignment a; ``gamma_of(a, f, spec)``: the
    gamma value ``SVC.fit`` resolves on that fold's training rows.  Pure host code: no device is needed."""
    plan = AlignedPlan()
    plan.views, plan.rows, plan.matrices, plan.models = [], [], [], []
    for a in sorted(set(align_of)):
        members = [c for c in range(len(settings)) if align_of[c] == a]
        for f, rows in enumerate(rows_of[a]):
            v = len(plan.views)
            plan.views.append((a, f))
            plan.rows.append(int(rows))
            matrix_of = {}
            for c in members:
                g = None if kernel != 'rbf' else float(gamma_of(a, f, settings[c]['gamma']))
                if g not in matrix_of:
                    matrix_of[g] = len(plan.matrices)
                    plan.matrices.append((v, g))
                plan.models.append(dict(cand=c, fold=f, view=v, matrix=matrix_of[g], C=float(settings[c]['C'])))
    return plan


def chunk_bytes(plan, mats, rbf):
    """The device bytes of a chunk: its kernel matrices and, for rbf, one Gram matrix per view that has a matrix in it."""
    own = sum(8 * plan.rows[plan.matrices[m][0]] ** 2 for m in mats)
    return own + (sum(8 * plan.rows[v] ** 2 for v in {plan.matrices[m][0] for m in mats}) if rbf else 0)


def cut_plan_chunks(plan, rbf, max_bytes):
    """Consecutive runs of kernel matrices whose ``chunk_bytes`` stay within ``max_bytes`` (a run of one matrix is always taken, so
    for rbf a chunk may hold one matrix and its Gram beyond the limit).  A single matrix above the limit raises ``cut_chunks``'
    ``ValueError``."""
    cut_chunks(plan.matrix_bytes(), max_bytes)                  # (raises for a matrix that can never fit)
    chunks, cur = [], []
    for m in range(len(plan.matrices)):
        if cur and chunk_bytes(plan, cur + [m], rbf) > max_bytes:
            chunks.append(cur)
            cur = []
        cur.append(m)
    if cur:
        chunks.append(cur)
    return chunks


# ------------------------------------------------------------------------------------------------ the device
def _run_chunk(plan, mats, V, layouts, rbf, svc, k):
    """The kernel matrices ``mats`` and all their models.  V[v]: view v's (rows, features) float32 device matrix; layouts[v]:
    its ``fold_layout``.  Returns [(model, (E, held-out rows) predictions, (E, k, k) confusion tables)]."""
    dev = LA.device()
    base = np.concatenate([[0], np.cumsum([plan.rows[plan.matrices[m][0]] ** 2 for m in mats])]).astype(np.int64)
    Kbuf = torch.empty(int(base[-1]), dtype=LA.F64, device=dev)
    K = {m: Kbuf[base[i]:base[i + 1]].view(plan.rows[plan.matrices[m][0]], -1) for i, m in enumerate(mats)}
    if rbf:
        views = sorted({plan.matrices[m][0] for m in mats})
        gbase = np.concatenate([[0], np.cumsum([plan.rows[v] ** 2 for v in views])]).astype(np.int64)
        Gbuf = torch.empty(int(gbase[-1]), dtype=LA.F64, device=dev)
        G = {v: Gbuf[gbase[i]:gbase[i + 1]].view(plan.rows[v], plan.rows[v]) for i, v in enumerate(views)}
        t_gram = LA.gram_grouped([(V[v], G[v]) for v in views])                                   # noqa: F841  (host tables: alive
        t_rbf = LA.rbf_grouped([(G[plan.matrices[m][0]], plan.matrices[m][1], K[m]) for m in mats])  # noqa: F841  until the download)
    else:
        t_gram = LA.gram_grouped([(V[plan.matrices[m][0]], K[m]) for m in mats])                  # noqa: F841
    slot = {m: i for i, m in enumerate(mats)}
    owners, models, mn, mbase = [], [], [], []
    for mod in plan.models:
        if mod['matrix'] not in slot:
            continue
        lay = layouts[mod['view']]
        owners.append(mod)
        for p in lay['problems']:
            models.append(dict(problems=p, C=mod['C'], test_pos=lay['test_pos'], ytest=lay['ytest']))
            mn.append(plan.rows[mod['view']])
            mbase.append(base[slot[mod['matrix']]])
    conf, pred, tst_off = solve_and_score(Kbuf, models, mn, mbase, svc.tol, svc.max_iter, k)
    out, s = [], 0
    for mod in owners:
        E = len(layouts[mod['view']]['problems'])
        out.append((mod, np.stack([pred[tst_off[s + e]:tst_off[s + e + 1]] for e in range(E)]), conf[s:s + E]))
        s += E
    return out


class AlignedSVCSearchCV(BaseEstimator):
    """``GridSearchCV`` / the evaluation step of a ``BayesSearchCV`` for a ``crossPtDecoder_sepAlign`` over ``n_comp`` and the SVC's
    ``C`` and ``gamma``, with all folds and all candidates aligned, trained and scored as one device problem per chunk.

    ``model``: what ``cross_val_decode`` takes -- ``aligner=AlignCCA``, ``dim_red=alignment.PCA`` and a ``decoders.SVC`` or a
    ``decoders.BaggingClassifier(decoders.SVC(...))`` as its decoder.  ``param_grid`` (expanded by ``ParameterGrid``) or
    ``candidates`` (an explicit list of parameter dicts: what a Bayesian or random search hands over) with the keys ``n_comp`` (an
    int or a variance fraction) and ``decoder__C`` / ``decoder__gamma`` (bare SVC) or ``decoder__estimator__C`` /
    ``decoder__estimator__gamma`` (bagged); ``gamma`` on a linear kernel is accepted and has no effect.  ``cv`` through
    ``check_cv(cv, y, classifier=True)``, its splits being runs of partitions of the trials; ``scoring``: ``None`` / ``'accuracy'``
    or ``'balanced_accuracy'``, a split's score coming from its own confusion table.

    After ``fit(X, y, y_align=None)``: ``cv_results_``, ``best_index_``, ``best_params_``, ``best_score_``, ``n_splits_``,
    ``classes_``, ``cv_test_predictions_`` (per split: ``(test_idx, labels (n_candidates, len(test_idx)))``), ``cv_confusion_``
    (n_candidates, n_splits, k, k; rows = true class), ``n_components_`` (n_candidates, n_splits: the target's component counts)
    and, with ``refit``, ``best_estimator_`` = ``clone(model).set_params(**best_params_).fit(X, y, y_align=y_align)``, to which
    ``predict`` / ``score`` delegate."""

    def __init__(self, model, param_grid=None, *, candidates=None, cv=5, scoring=None, refit=True, max_kernel_bytes=2 ** 30):
        self.model = model
        self.param_grid = param_grid
        self.candidates = candidates
        self.cv = cv
        self.scoring = scoring
        self.refit = refit
        self.max_kernel_bytes = max_kernel_bytes

    def fit(self, X, y, y_align=None):
        model = self.model
        svc, ens = check_model(model)
        if self.scoring not in SCORINGS:
            raise ValueError(f"scoring must be None, 'accuracy' or 'balanced_accuracy'; got {self.scoring!r}")
        candidates = expand_candidates(self.param_grid, self.candidates)
        split = [split_params(model, c) for c in candidates]
        rbf = svc.kernel == 'rbf'
        settings = [dict(C=float(s.get('C', svc.C)), gamma=gamma_spec(svc.kernel, s.get('gamma', svc.gamma))) for s in split]
        n_comps = [s.get('n_comp', model.n_comp) for s in split]
        y = np.asarray(y)
        if y.ndim != 1:
            raise ValueError('y must be (n_trials,)')
        N = len(y)
        y_al = y if y_align is None else y_align
        pool = list(model.cross_pt_data)
        ys = [np.asarray(yc) for _, yc, _ in pool]
        classes = np.unique(np.hstack([y] + ys))
        k = len(classes)
        if k < 2:
            raise ValueError('The number of classes has to be greater than one; got 1 class')
        if k > 64:
            raise ValueError(f'the scoring kernel takes 2..64 classes; got {k}')
        yi_tar = np.searchsorted(classes, y).astype(np.int32)
        yi_pool = np.searchsorted(classes, np.hstack(ys)).astype(np.int32) if ys else np.zeros(0, dtype=np.int32)
        parts = cut_partitions(check_cv(self.cv, y, classifier=True).split(np.zeros(N), y), N)
        n_cand, n_splits = len(candidates), sum(len(p) for p in parts)
        conf = np.zeros((n_cand, n_splits, k, k), dtype=np.int64)
        comps = np.zeros((n_cand, n_splits), dtype=np.int64)
        tests, labels = [], []
        Xd = LA.to_device(X)                                       # one upload for all partitions
        s0 = 0
        for part in parts:
            fas = fit_folds_multi(Xd, y_al, pool, part, n_comps, max_bytes=int(self.max_kernel_bytes), append_heldout=True)
            distinct, align_of = [], []
            for fa in fas:                                         # (equal component counts are one object)
                if not any(fa is d for d in distinct):
                    distinct.append(fa)
                align_of.append(next(i for i, d in enumerate(distinct) if d is fa))
            F = len(part)
            rows_of = [[fa.pool_with_heldout(f)[0].shape[0] for f in range(F)] for fa in distinct]
            # the views: their rows on the device and what a clone fitted on the fold poses
            V, layouts = {}, {}
            for a, fa in enumerate(distinct):
                for f, (tr, te) in enumerate(fa.plan.splits):
                    Vf, _ = fa.pool_with_heldout(f)
                    d = Vf.shape[1] * Vf.shape[2]
                    V[a, f] = Vf.view(Vf.shape[0], d)
                    layouts[a, f] = fold_layout(svc, ens, classes, yi_tar, yi_pool, tr, te, model.tar_in_train, d)
                    assert layouts[a, f]['rows'] == Vf.shape[0]
            # gamma='scale': ONE variance launch and one download for every view that needs it
            wanted = scale_views(settings, align_of, F, svc.kernel)
            var_d, tables = LA.var_grouped([(V[v], layouts[v]['first'], layouts[v]['last'] - layouts[v]['first']) for v in wanted])
            var = dict(zip(wanted, var_d.cpu().numpy())) if wanted else {}
            del tables

            def gamma_of(a, f, spec):                              # SVC.fit's rule on the rows handed to THIS fold's fit
                lay = layouts[a, f]
                return _ovo.gamma_value(svc.kernel, spec, _Features(lay['last'] - lay['first'], V[a, f].shape[1], var.get((a, f))))
            plan = build_plan(settings, align_of, rows_of, svc.kernel, gamma_of)
            Vv, Lv = [V[v] for v in plan.views], [layouts[v] for v in plan.views]
            part_labels = [np.empty((n_cand, len(te)), dtype=classes.dtype) for _, te in part]
            for mats in cut_plan_chunks(plan, rbf, int(self.max_kernel_bytes)):
                for mod, pred, conf_e in _run_chunk(plan, mats, Vv, Lv, rbf, svc, k):
                    c, f = mod['cand'], mod['fold']
                    if ens is None:
                        winner, table = pred[0], conf_e[0]
                    else:
                        winner = host_vote(pred, k)[1]
                        table = confusion(Lv[mod['view']]['ytest'], winner, k)
                    conf[c, s0 + f] = table
                    part_labels[f][c] = classes[winner]
            for c in range(n_cand):
                comps[c, s0:s0 + F] = fas[c].n_components_
            tests += [np.asarray(te) for _, te in part]
            labels += part_labels
            s0 += F
        scores = scores_from_confusion(conf, self.scoring)
        self.cv_results_ = assemble_results(candidates, scores)
        self.cv_confusion_ = conf
        self.n_components_ = comps
        self.cv_test_predictions_ = list(zip(tests, labels))
        self.n_splits_ = n_splits
        self.classes_ = classes
        self.best_index_ = int(self.cv_results_['rank_test_score'].argmin())
        self.best_params_ = self.cv_results_['params'][self.best_index_]
        self.best_score_ = float(self.cv_results_['mean_test_score'][self.best_index_])
        if self.refit:
            self.best_estimator_ = clone(model).set_params(**self.best_params_)
            self.best_estimator_.fit(X, y, y_align=y_align)
        return self

    # ------------------------------------------------------------------ the refitted model
    def _best(self):
        if not hasattr(self, 'best_estimator_'):
            raise AttributeError('this AlignedSVCSearchCV has no best_estimator_: it was not fitted, or refit=False')
        return self.best_estimator_

    def predict(self, X):
        return self._best().predict(X)

    def score(self, X, y):
        return self._best().score(X, y)
