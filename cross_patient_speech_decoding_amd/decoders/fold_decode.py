"""Cross-validated aligned SVM decoding with every fold as one device problem.

The reference's config-1 experiment (scripts/aligned_decode_svm.py) scores an iteration by running, per fold of a k-fold split,
``crossPtDecoder_sepAlign(...).fit(X[tr], y[tr], y_align=...).predict(X[te])`` -- a PCA of the target's training trials, a CCA
alignment of every pooled patient, pooling, a (bagged) SVC fit and a prediction -- and taking the balanced accuracy over all
held-out predictions.  This module holds the ONE engine that runs such folds without the loop, for any number of candidate
settings (``n_comp``, ``C``, ``gamma``) side by side (``run_partition``), and its one-candidate user, ``cross_val_decode``;
``aligned_search.AlignedSVCSearchCV`` is the many-candidate user.

per partition  (a run of splits whose test sets partition the trials: one repeat of a repeated k-fold)
               ``alignment.fit_folds_multi`` over the candidates' ``n_comp`` values (one value: ``fit_folds`` bit for bit) with the
               held-out trials appended to every fold's pooled float32 tensor;
               a VIEW per distinct (alignment, fold): the rows of ``pool_with_heldout(f)``, with ``fold_layout``'s class-pair
               problems, weights and bootstrap draws for the view's own feature count;
               ONE ``xps_var_grouped_f64`` and one download for all views some candidate asks ``gamma='scale'`` of;
               the host plan (``build_plan``): kernel matrices = distinct (view, gamma value), models = (candidate, fold);
per chunk      (kernel matrices, and for rbf the Gram matrices of their views, within the byte limit: ``cut_plan_chunks``)
               ONE ``xps_gram_grouped_f64`` over the chunk's views (training rows first, held-out rows last),
               rbf only: ONE ``xps_rbf_grouped_from_gram_f64`` over the chunk's matrices, norms from the Gram diagonal,
               ONE ``search.solve_and_score`` with one model per (candidate, fold, estimator): three uploads, ONE
               ``xps_svm_smo_multi_f64``, ONE ``xps_svm_cv_score_f64``, ONE download of the confusion tables and predictions.

The host builds the class-pair problems of every (fold, estimator) with the rules a clone fitted on that fold applies
(decoders/_ovo.py: this fold's classes, ``'balanced'`` weights, ``gamma='scale'``, sklearn's bootstrap draws for the fold's own row
and feature counts) and takes the ensemble vote from the one download.  The launch count depends neither on the number of folds
nor on the number of candidates.  There is no CPU fallback."""
import copy
import numbers

import numpy as np
import torch
from sklearn.model_selection import check_cv
from sklearn.pipeline import Pipeline

from ..alignment import AlignCCA
from ..alignment import _linalg as LA
from ..alignment.fold_align import fit_folds_multi
from ..alignment.pca import PCA
from . import _ovo
from .bagging import BaggingClassifier, bagging_sample_indices, sample_weights
from .cross_pt_decoders import crossPtDecoder_sepAlign
from .search import check_class_count, cut_chunks, scores_from_confusion, solve_and_score
from .svm import SVC

SUPPORTED = ('cross_val_decode takes a crossPtDecoder_sepAlign with aligner=AlignCCA (its defaults), dim_red=alignment.PCA and a '
             'decoders.SVC or decoders.BaggingClassifier(decoders.SVC(...)) as its decoder')


# ------------------------------------------------------------------------------------------------ host
def check_model(model):
    """(svc, ensemble or None) of a supported model; ``TypeError`` naming what is supported for every other wrapper class, aligner,
    reduction or decoder, ``NotImplementedError`` for a pipeline decoder and for the settings the SVC / the ensemble refuse."""
    if type(model) is not crossPtDecoder_sepAlign:
        raise TypeError(f'{SUPPORTED}; got {type(model).__name__}')
    if model.aligner is not AlignCCA:
        raise TypeError(f'{SUPPORTED}; got the aligner {model.aligner!r}')
    if model.dim_red is not PCA:
        raise TypeError(f'{SUPPORTED}; got the reduction {model.dim_red!r}')
    dec = model.decoder
    if isinstance(dec, Pipeline):
        raise NotImplementedError('a pipeline decoder (e.g. a DimRedReshape step in front of the SVC) is not implemented in '
                                  'cross_val_decode')
    if isinstance(dec, SVC):
        dec._check_settings()
        return dec, None
    if isinstance(dec, BaggingClassifier):
        dec._check_settings()
        return dec.estimator, dec
    raise TypeError(f'{SUPPORTED}; got the decoder {type(dec).__name__}')


def cut_partitions(splits, n):
    """``splits`` cut into consecutive partitions: runs of (train, test) pairs whose test sets are pairwise disjoint and cover
    range(n), as ``KFold`` / ``StratifiedKFold`` produce once and ``RepeatedStratifiedKFold`` once per repeat.  Anything else
    raises ``ValueError`` (a train set that is not the complement of its test set is refused by ``alignment.fold_plan``)."""
    if n < 1:
        raise ValueError('cut_partitions: no trials')
    parts, cur, seen = [], [], np.zeros(n, dtype=bool)
    for s, (tr, te) in enumerate(splits):
        tr, te = (np.asarray(a, dtype=np.int64).reshape(-1) for a in (tr, te))
        if len(te) and (te.min() < 0 or te.max() >= n):
            raise ValueError(f'cut_partitions: split {s} has a test index outside range({n})')
        if len(np.unique(te)) != len(te) or seen[te].any():
            raise ValueError(f'cut_partitions: the test set of split {s} overlaps an earlier one before the trials were covered; '
                             'the splits must be runs of k-fold partitions of the trials')
        seen[te] = True
        cur.append((tr, te))
        if seen.all():
            parts.append(cur)
            cur, seen = [], np.zeros(n, dtype=bool)
    if cur:
        raise ValueError('cut_partitions: the last splits do not cover the trials; the splits must be runs of k-fold partitions')
    if not parts:
        raise ValueError('cv yields no split')
    return parts


def decode_setup(model, y, y_align, cv):
    """What every cross-validated run of a checked model starts from (host only): ``y`` as an array, the alignment labels (``y``
    for None), the pool, ``classes`` (the union of the target's and the pooled patients' labels, 2..64 of them), the class indices
    of the target's trials and of the pooled rows, and the partitions of ``check_cv(cv, y, classifier=True)``."""
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError('y must be (n_trials,)')
    N = len(y)
    pool = list(model.cross_pt_data)
    ys = [np.asarray(yc) for _, yc, _ in pool]
    classes = np.unique(np.hstack([y] + ys))
    check_class_count(len(classes))
    yi_tar = np.searchsorted(classes, y).astype(np.int32)
    yi_pool = np.searchsorted(classes, np.hstack(ys)).astype(np.int32) if ys else np.zeros(0, dtype=np.int32)
    parts = cut_partitions(check_cv(cv, y, classifier=True).split(np.zeros(N), y), N)
    return y, (y if y_align is None else y_align), pool, classes, yi_tar, yi_pool, parts


def fold_problems(svc, ensemble, classes, labels, positions, n_features):
    """The class-pair problems of one fold, per estimator, as a clone of the decoder fitted on the fold's training rows poses them.
    ``labels``: the index into ``classes`` of every training row; ``positions``: its row in the fold's kernel matrix.  The fold's
    own classes and class weights (``SVC.fit`` / ``BaggingClassifier.fit``: from all training rows of the fold), for an ensemble
    sklearn's draws for ``len(labels)`` rows and ``n_features`` features and the multiplicities as sample weights; pair_a / pair_b
    are indices into ``classes``.  Returns (problems, samples): one ``_ovo.pair_problems`` dict per estimator (one for a bare SVC)
    and the draws (an empty list for a bare SVC)."""
    labels, positions = np.asarray(labels), np.asarray(positions)
    cls, yi = np.unique(labels, return_inverse=True)
    if len(cls) < 2:
        raise ValueError(f'The number of classes has to be greater than one; got {len(cls)} class')
    cw = _ovo.class_weights(svc.class_weight, classes[cls], yi)
    if ensemble is None:
        samples, weights = [], [None]
    else:
        rs = ensemble.random_state                             # (a clone per fold starts a RandomState instance from the same state)
        rs = rs if rs is None or isinstance(rs, numbers.Integral) else copy.deepcopy(rs)
        samples = bagging_sample_indices(rs, int(ensemble.n_estimators), len(yi), n_features, ensemble.max_samples, ensemble.bootstrap)
        weights = sample_weights(samples, np.ones(len(yi)), ensemble.bootstrap)
    problems = []
    for w in weights:
        p = _ovo.pair_problems(yi, positions, cw, w)
        p['pair_a'], p['pair_b'] = (cls[p[key]].astype(np.int32) for key in ('pair_a', 'pair_b'))
        problems.append(p)
    return problems, samples


def fold_layout(svc, ensemble, classes, yi_tar, yi_pool, tr, te, tar_in_train, n_features):
    """One fold as the device sees it (host only).  Its matrix holds the target's training trials ``tr``, then the pooled patients'
    rows, then the held-out trials ``te``; the training rows are rows first..last - 1 (``tar_in_train=False`` leaves the target's
    out of every index list), the held-out rows follow at ``test_pos``.  ``yi_tar`` / ``yi_pool``: class indices of the target's
    trials and of the pooled rows.  Returns a dict: rows, first, last, problems, samples (``fold_problems``), test_pos, ytest."""
    tr, te = np.asarray(tr), np.asarray(te)
    first, last = (0 if tar_in_train else len(tr)), len(tr) + len(yi_pool)
    problems, samples = fold_problems(svc, ensemble, classes, np.concatenate([yi_tar[tr], yi_pool])[first:], np.arange(first, last),
                                      n_features)
    return dict(rows=last + len(te), first=first, last=last, problems=problems, samples=samples,
                test_pos=(last + np.arange(len(te))).astype(np.int32), ytest=np.asarray(yi_tar[te], dtype=np.int32))


def host_vote(pred, k):
    """pred (E, m): each estimator's predicted class index per row -> (votes (m, k) int32, winner (m,)): the estimators counted per
    class and the first maximum (``bag_vote_kernel``'s rule and sklearn's).  An index outside [0, k) casts no vote."""
    pred = np.asarray(pred).reshape(len(pred), -1)
    votes = np.zeros((pred.shape[1], k), dtype=np.int32)
    for row in pred:
        ok = np.flatnonzero((row >= 0) & (row < k))
        np.add.at(votes, (ok, row[ok]), 1)
    return votes, votes.argmax(axis=1)


def confusion(y_true, y_pred, k):
    """(k, k) int table of class indices, rows = true class."""
    conf = np.zeros((k, k), dtype=np.int64)
    np.add.at(conf, (np.asarray(y_true), np.asarray(y_pred)), 1)
    return conf


class _Features:
    """What ``_ovo.gamma_value`` reads of the matrix handed to a fit -- its shape and the variance of its elements -- for rows that
    stay on the device."""

    def __init__(self, rows, cols, var):
        self.shape, self._var = (rows, cols), var

    def var(self):
        return self._var


class FoldDecode:
    """Result of ``cross_val_decode`` over R partitions of N trials and k classes: ``classes_`` (the union of the target's and the
    pooled patients' labels), ``y_pred_`` (R, N) labels in trial order, ``votes_`` (R, N, k) int32 estimator counts per class,
    ``fold_of_trial_`` (R, N), ``confusion_`` (R, k, k; rows = true class) over a partition's held-out rows, ``accuracy_`` and
    ``balanced_accuracy_`` (R,) (sklearn's rule over all held-out predictions of a partition, as the script scores an iteration),
    ``estimators_samples_[r][f]`` (the bootstrap draws of fold f's ensemble; empty for a bare SVC) and ``alignment_`` (the R
    ``FoldAlignment`` objects)."""


# ------------------------------------------------------------------------------------------------ the plan (host)
def gamma_spec(kernel, spec):
    """How a candidate's gamma enters the plan: None for a linear kernel (accepted, without effect, as in sklearn), the string for
    'scale' / 'auto', else the float."""
    if kernel != 'rbf':
        return None
    return spec if isinstance(spec, str) else float(spec)


class AlignedPlan:
    """Host description of one partition.  ``views``: the distinct (alignment, fold) pairs; ``matrices``: (view, gamma value or
    None for linear) per kernel matrix, the matrices of a view adjacent; ``models``: one dict per (candidate, fold): cand, fold,
    view, matrix, C.  ``rows[v]``: the rows of view v's matrices."""

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


def run_partition(Xd, y_align, pool, svc, ens, tar_in_train, classes, yi_tar, yi_pool, part, settings, n_comps, max_bytes):
    """One partition of the trials for any number of candidates: all folds of all candidates aligned, trained and scored as one
    device problem per chunk of ``max_bytes``.  ``Xd``: the device tensor of X (N, T, C); ``y_align`` / ``pool``: what
    ``fit_folds_multi`` takes; ``svc``, ``ens``: ``check_model``'s pair; ``classes``, ``yi_tar``, ``yi_pool``: ``decode_setup``'s;
    ``part``: the partition's (train, test) splits; candidate c is ``settings[c]`` = dict(C=..., gamma=``gamma_spec``) on
    ``n_comps[c]``.  Returns (the ``FoldAlignment`` of every candidate -- equal component counts are one object --, a list of
    (candidate, fold, (E, held-out rows) predicted class indices, (E, k, k) confusion tables, the fold's ``fold_layout``) covering
    every (candidate, fold) once)."""
    k, rbf, F = len(classes), svc.kernel == 'rbf', len(part)
    fas = fit_folds_multi(Xd, y_align, pool, part, n_comps, max_bytes=int(max_bytes), append_heldout=True)
    distinct, align_of = [], []
    for fa in fas:                                             # (equal component counts are one object)
        if not any(fa is d for d in distinct):
            distinct.append(fa)
        align_of.append(next(i for i, d in enumerate(distinct) if d is fa))
    # the views: their rows on the device and what a clone fitted on the fold poses
    V, layouts = {}, {}
    for a, fa in enumerate(distinct):
        for f, (tr, te) in enumerate(fa.plan.splits):
            Vf, _ = fa.pool_with_heldout(f)
            d = Vf.shape[1] * Vf.shape[2]
            V[a, f] = Vf.view(Vf.shape[0], d)
            layouts[a, f] = fold_layout(svc, ens, classes, yi_tar, yi_pool, tr, te, tar_in_train, d)
            assert layouts[a, f]['rows'] == Vf.shape[0]
    # gamma='scale': ONE variance launch and one download for every view that needs it
    wanted = scale_views(settings, align_of, F, svc.kernel)
    var_d, tables = LA.var_grouped([(V[v], layouts[v]['first'], layouts[v]['last'] - layouts[v]['first']) for v in wanted])
    var = dict(zip(wanted, var_d.cpu().numpy())) if wanted else {}
    del tables

    def gamma_of(a, f, spec):                                  # SVC.fit's rule on the rows handed to THIS fold's fit
        lay = layouts[a, f]
        return _ovo.gamma_value(svc.kernel, spec, _Features(lay['last'] - lay['first'], V[a, f].shape[1], var.get((a, f))))
    plan = build_plan(settings, align_of, [[layouts[a, f]['rows'] for f in range(F)] for a in range(len(distinct))], svc.kernel, gamma_of)
    Vv, Lv = [V[v] for v in plan.views], [layouts[v] for v in plan.views]
    out = []
    for mats in cut_plan_chunks(plan, rbf, int(max_bytes)):
        out += [(mod['cand'], mod['fold'], pred, conf, Lv[mod['view']]) for mod, pred, conf in _run_chunk(plan, mats, Vv, Lv, rbf, svc, k)]
    return fas, out


def cross_val_decode(model, X, y, y_align=None, cv=5, max_bytes=2 ** 30):
    """Held-out predictions of ``clone(model).fit(X[tr], y[tr], y_align=y_align[tr]).predict(X[te])`` for every split of ``cv``,
    with all folds of a partition aligned, trained and scored as one device problem per chunk of ``max_bytes`` of kernel
    matrices and, for rbf, their Gram matrices (``cut_plan_chunks``): ``run_partition`` with one candidate, the model's own ``C``,
    ``gamma`` and ``n_comp``.

    ``model``: a ``crossPtDecoder_sepAlign`` with ``aligner=AlignCCA``, ``dim_red=alignment.PCA`` and a ``decoders.SVC`` or a
    ``decoders.BaggingClassifier(decoders.SVC(...))`` (kernel linear or rbf); ``tar_in_train`` is honoured.  X (N, T, C); ``y`` the
    decode labels (N,); ``y_align`` the alignment labels (None: ``y``); ``cv`` through ``check_cv(cv, y, classifier=True)``, its
    splits being runs of partitions of the trials (``cut_partitions``).  Returns a ``FoldDecode``."""
    svc, ens = check_model(model)
    y, y_align, pool, classes, yi_tar, yi_pool, parts = decode_setup(model, y, y_align, cv)
    settings = [dict(C=float(svc.C), gamma=gamma_spec(svc.kernel, svc.gamma))]
    R, N, k = len(parts), len(y), len(classes)
    res = FoldDecode()
    res.classes_ = classes
    res.votes_ = np.zeros((R, N, k), dtype=np.int32)
    res.fold_of_trial_ = np.zeros((R, N), dtype=np.int64)
    res.confusion_ = np.zeros((R, k, k), dtype=np.int64)
    res.estimators_samples_, res.alignment_ = [], []
    pred_idx = np.zeros((R, N), dtype=np.int64)
    Xd = LA.to_device(X)                                       # one upload for all partitions
    for r, part in enumerate(parts):
        fas, results = run_partition(Xd, y_align, pool, svc, ens, model.tar_in_train, classes, yi_tar, yi_pool, part, settings,
                                     [model.n_comp], max_bytes)
        samples = [None] * len(part)
        for _, f, pred, conf, layout in results:
            te = part[f][1]
            res.votes_[r, te], pred_idx[r, te] = host_vote(pred, k)
            res.fold_of_trial_[r, te] = f
            if ens is None:
                res.confusion_[r] += conf[0]
            samples[f] = layout['samples']
        if ens is not None:
            res.confusion_[r] = confusion(yi_tar, pred_idx[r], k)
        res.estimators_samples_.append(samples)
        res.alignment_.append(fas[0])
    res.y_pred_ = classes[pred_idx]
    res.accuracy_ = scores_from_confusion(res.confusion_, 'accuracy')
    res.balanced_accuracy_ = scores_from_confusion(res.confusion_, 'balanced_accuracy')
    return res
