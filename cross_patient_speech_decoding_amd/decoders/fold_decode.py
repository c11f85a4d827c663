"""Cross-validated aligned SVM decoding with every fold as one device problem.

The reference's config-1 experiment (scripts/aligned_decode_svm.py) scores an iteration by running, per fold of a k-fold split,
``crossPtDecoder_sepAlign(...).fit(X[tr], y[tr], y_align=...).predict(X[te])`` -- a PCA of the target's training trials, a CCA
alignment of every pooled patient, pooling, a (bagged) SVC fit and a prediction -- and taking the balanced accuracy over all
held-out predictions.  ``cross_val_decode`` runs the same experiment without the loop:

per partition  (a run of splits whose test sets partition the trials: one repeat of a repeated k-fold)
               ``alignment.fit_folds`` with the held-out trials appended to every fold's pooled float32 tensor; for rbf with
               ``gamma='scale'`` the variance of every fold's training rows (one small reduction per fold, ONE download);
per chunk      (folds whose kernel matrices fit ``max_bytes``)
               ONE ``xps_gram_grouped_f64`` (every fold's Gram matrix of its own rows, training rows first, held-out rows last),
               rbf only: per fold one ``xps_rbf_from_gram_f64`` with norms from the Gram diagonal (F small launches),
               three uploads, ONE ``xps_svm_smo_multi_f64``, ONE ``xps_svm_cv_score_f64`` with one model per (fold, estimator),
               ONE download of the confusion tables and predictions (``search.solve_and_score``).

The host builds the class-pair problems of every (fold, estimator) with the rules a clone fitted on that fold applies
(decoders/_ovo.py: this fold's classes, ``'balanced'`` weights, ``gamma='scale'``, sklearn's bootstrap draws for the fold's own row
and feature counts) and takes the ensemble vote from the one download.  There is no CPU fallback."""
import copy
import numbers

import numpy as np
import torch
from sklearn.model_selection import check_cv
from sklearn.pipeline import Pipeline

from .._dev import stream
from .._lib import call
from ..alignment import AlignCCA
from ..alignment import _linalg as LA
from ..alignment.fold_align import fit_folds
from ..alignment.pca import PCA
from . import _ovo
from .bagging import BaggingClassifier, bagging_sample_indices, sample_weights
from .cross_pt_decoders import crossPtDecoder_sepAlign
from .search import cut_chunks, scores_from_confusion, solve_and_score
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


# ------------------------------------------------------------------------------------------------ the device
def _train_variances(folds):
    """Population variance of the elements of every fold's training rows, float64 on the device: one reduction per fold, ONE
    download."""
    return torch.stack([fd['V'][fd['first']:fd['last']].to(LA.F64).var(unbiased=False) for fd in folds]).cpu().numpy()


def _run_chunk(folds, svc, k):
    """The folds of one chunk: their kernel matrices in one buffer, one model per (fold, estimator).  Returns per fold the
    (E, held-out rows) predictions and the (E, k, k) confusion tables."""
    dev = LA.device()
    base = np.concatenate([[0], np.cumsum([fd['rows'] ** 2 for fd in folds])]).astype(np.int64)
    Kbuf = torch.empty(int(base[-1]), dtype=LA.F64, device=dev)
    mats = [Kbuf[base[i]:base[i + 1]].view(fd['rows'], fd['rows']) for i, fd in enumerate(folds)]
    if svc.kernel == 'rbf':
        Gbuf = torch.empty_like(Kbuf)
        grams = [Gbuf[base[i]:base[i + 1]].view(fd['rows'], fd['rows']) for i, fd in enumerate(folds)]
    else:
        grams = mats
    tables = LA.gram_grouped([(fd['V'], G) for fd, G in zip(folds, grams)])  # noqa: F841  (host tables: alive until the download)
    if svc.kernel == 'rbf':
        for fd, G, K in zip(folds, grams, mats):               # the rbf map: F small launches
            sq = torch.diagonal(G).contiguous()                # |x_i|^2: the Gram diagonal (libsvm: dot(x_i, x_i))
            call('xps_rbf_from_gram_f64', G.data_ptr(), G.stride(0), sq.data_ptr(), sq.data_ptr(), fd['rows'], fd['rows'],
                 float(fd['gamma']), K.data_ptr(), K.stride(0), stream())
    models, mn, mbase = [], [], []
    for i, fd in enumerate(folds):
        for p in fd['problems']:
            models.append(dict(problems=p, C=float(svc.C), test_pos=fd['test_pos'], ytest=fd['ytest']))
            mn.append(fd['rows'])
            mbase.append(base[i])
    conf, pred, tst_off = solve_and_score(Kbuf, models, mn, mbase, svc.tol, svc.max_iter, k)
    out, s = [], 0
    for fd in folds:
        E = len(fd['problems'])
        out.append((np.stack([pred[tst_off[s + e]:tst_off[s + e + 1]] for e in range(E)]), conf[s:s + E]))
        s += E
    return out


def cross_val_decode(model, X, y, y_align=None, cv=5, max_bytes=2 ** 30):
    """Held-out predictions of ``clone(model).fit(X[tr], y[tr], y_align=y_align[tr]).predict(X[te])`` for every split of ``cv``,
    with all folds of a partition aligned, trained and scored as one device problem per chunk of ``max_bytes`` of kernel
    matrices (for rbf a Gram buffer of the same size lies beside them).

    ``model``: a ``crossPtDecoder_sepAlign`` with ``aligner=AlignCCA``, ``dim_red=alignment.PCA`` and a ``decoders.SVC`` or a
    ``decoders.BaggingClassifier(decoders.SVC(...))`` (kernel linear or rbf); ``tar_in_train`` is honoured.  X (N, T, C); ``y`` the
    decode labels (N,); ``y_align`` the alignment labels (None: ``y``); ``cv`` through ``check_cv(cv, y, classifier=True)``, its
    splits being runs of partitions of the trials (``cut_partitions``).  Returns a ``FoldDecode``."""
    svc, ens = check_model(model)
    y = np.asarray(y)
    if y.ndim != 1:
        raise ValueError('y must be (n_trials,)')
    N = len(y)
    y_align = y if y_align is None else y_align
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
    parts = cut_partitions(check_cv(cv, y, classifier=True).split(np.zeros(N), y), N)
    R = len(parts)
    res = FoldDecode()
    res.classes_ = classes
    res.votes_ = np.zeros((R, N, k), dtype=np.int32)
    res.fold_of_trial_ = np.zeros((R, N), dtype=np.int64)
    res.confusion_ = np.zeros((R, k, k), dtype=np.int64)
    res.estimators_samples_, res.alignment_ = [], []
    pred_idx = np.zeros((R, N), dtype=np.int64)
    Xd = LA.to_device(X)                                       # one upload for all partitions
    for r, part in enumerate(parts):
        fa = fit_folds(Xd, y_align, pool, part, n_components=model.n_comp, max_bytes=max_bytes, append_heldout=True)
        folds = []
        for f, (tr, te) in enumerate(fa.plan.splits):
            V, _ = fa.pool_with_heldout(f)
            d = V.shape[1] * V.shape[2]
            fd = fold_layout(svc, ens, classes, yi_tar, yi_pool, tr, te, model.tar_in_train, d)
            assert fd['rows'] == V.shape[0]
            folds.append(dict(fd, V=V.view(fd['rows'], d), d=d))
        if svc.kernel == 'rbf':
            var = _train_variances(folds) if isinstance(svc.gamma, str) and svc.gamma == 'scale' else [None] * len(folds)
            for fd, v in zip(folds, var):                      # SVC.fit's rule on the rows handed to THIS fold's fit
                fd['gamma'] = _ovo.gamma_value(svc.kernel, svc.gamma, _Features(fd['last'] - fd['first'], fd['d'], v))
        for chunk in cut_chunks([8 * fd['rows'] ** 2 for fd in folds], int(max_bytes)):
            for f, (pred, conf) in zip(chunk, _run_chunk([folds[f] for f in chunk], svc, k)):
                te = fa.plan.splits[f][1]
                res.votes_[r, te], pred_idx[r, te] = host_vote(pred, k)
                res.fold_of_trial_[r, te] = f
                if ens is None:
                    res.confusion_[r] += conf[0]
        if ens is not None:
            res.confusion_[r] = confusion(yi_tar, pred_idx[r], k)
        res.estimators_samples_.append([fd['samples'] for fd in folds])
        res.alignment_.append(fa)
    res.y_pred_ = classes[pred_idx]
    res.accuracy_ = scores_from_confusion(res.confusion_, 'accuracy')
    res.balanced_accuracy_ = scores_from_confusion(res.confusion_, 'balanced_accuracy')
    return res
