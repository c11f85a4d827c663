"""Cross-validated search over ``n_comp``, ``C`` and ``gamma`` of an aligned decoder, resident on the MI355X.

The reference's nested-CV experiment chooses the settings of ``crossPtDecoder_sepAlign(pool, SVC, AlignCCA)`` with
``BayesSearchCV(model, param_grid, cv=cv, n_points=5, refit=False).fit(X, y, y_align=...)`` (scripts/aligned_decode_svm_ncv.py:
388-413): per (candidate, fold) a PCA of the target's training trials, a CCA alignment of every pooled patient, pooling, an SVC fit
and a prediction.  ``fold_decode.run_partition`` runs all folds of any number of candidates as one device problem per chunk (its
module docstring lists the launches); ``cross_val_decode`` hands it one candidate, ``AlignedSVCSearchCV`` all of them: this module
is the candidate handling and the results.

Per partition ``alignment.fit_folds_multi`` does the moments, covariances and eigendecompositions once for all ``n_comp`` values
and launches 5-9 of ``fit_folds`` once, with the folds of every distinct set of component counts side by side.  Candidates that
differ only in ``C`` share a kernel matrix, candidates that differ only in ``gamma`` share a Gram matrix, and the launch count does
not depend on the number of candidates.  The ensemble vote and the per-split confusion table of a bagged model are taken on the
host from the one download.  There is no CPU fallback."""
import numpy as np
from sklearn.base import BaseEstimator, clone

from ..alignment import _linalg as LA
from .fold_decode import AlignedPlan, build_plan, chunk_bytes, cut_plan_chunks, scale_views  # noqa: F401  (the plan's earlier home)
from .fold_decode import check_model, confusion, decode_setup, gamma_spec, host_vote, run_partition
from .search import SearchTail, expand_candidates

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


class AlignedSVCSearchCV(SearchTail, BaseEstimator):
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
        self._check_scoring()
        candidates = expand_candidates(self.param_grid, self.candidates)
        split = [split_params(model, c) for c in candidates]
        settings = [dict(C=float(s.get('C', svc.C)), gamma=gamma_spec(svc.kernel, s.get('gamma', svc.gamma))) for s in split]
        n_comps = [s.get('n_comp', model.n_comp) for s in split]
        y, y_al, pool, classes, yi_tar, yi_pool, parts = decode_setup(model, y, y_align, self.cv)
        k, n_cand, n_splits = len(classes), len(candidates), sum(len(p) for p in parts)
        conf = np.zeros((n_cand, n_splits, k, k), dtype=np.int64)
        comps = np.zeros((n_cand, n_splits), dtype=np.int64)
        tests, labels = [], []
        Xd = LA.to_device(X)                                       # one upload for all partitions
        s0 = 0
        for part in parts:
            fas, results = run_partition(Xd, y_al, pool, svc, ens, model.tar_in_train, classes, yi_tar, yi_pool, part, settings, n_comps,
                                         self.max_kernel_bytes)
            part_labels = [np.empty((n_cand, len(te)), dtype=classes.dtype) for _, te in part]
            for c, f, pred, conf_e, layout in results:
                if ens is None:
                    winner, table = pred[0], conf_e[0]
                else:
                    winner = host_vote(pred, k)[1]
                    table = confusion(layout['ytest'], winner, k)
                conf[c, s0 + f] = table
                part_labels[f][c] = classes[winner]
            for c in range(n_cand):
                comps[c, s0:s0 + len(part)] = fas[c].n_components_
            tests += [np.asarray(te) for _, te in part]
            labels += part_labels
            s0 += len(part)
        self._set_results(candidates, conf, list(zip(tests, labels)), classes)
        self.n_components_ = comps
        if self.refit:
            self.best_estimator_ = clone(model).set_params(**self.best_params_)
            self.best_estimator_.fit(X, y, y_align=y_align)
        return self

