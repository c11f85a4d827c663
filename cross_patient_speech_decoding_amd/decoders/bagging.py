"""Bagged SVC ensemble resident on the MI355X -- the whole decoder of BASELINE config 1.

The reference's config-1 decoder is ``BaggingClassifier(estimator=SVC(kernel='linear'), n_estimators=10)``
(scripts/aligned_decode_svm.py:262-263); the nested-CV and sub-sampling scripts search ``baggingclassifier__n_estimators`` over
10..100 and ``baggingclassifier__estimator__C`` / ``__gamma`` for the RBF decoder (scripts/aligned_decode_svm_ncv.py:151-159).
sklearn's ``BaggingClassifier`` around ``decoders.SVC`` runs that as E separate fits: E uploads of X, E Gram matrices of nearly
the same points, E SMO launches, E downloads, and a host loop over the estimators at predict.  sklearn hands every bagged
estimator the WHOLE X with ``sample_weight`` = the bootstrap multiplicities, so every estimator's kernel matrix is a sub-block
of one n x n matrix, and ``gamma='scale'`` / ``class_weight='balanced'`` (computed from the whole X / y) are the same for all of
them.  ``BaggingClassifier`` below uses that:

fit      one upload of X, one Gram product (one ``xps_rbf_from_gram_f64`` for rbf), ONE ``xps_svm_smo_f64`` launch over all
         Q = sum_e P_e class-pair problems (index lists into the one kernel matrix), one ``xps_bag_coef_scatter_f64`` to the dense
         (Q, n) coefficient matrix, for ``kernel='linear'`` one GEMM to the (Q, d) weight vectors;
predict  one upload of the test rows, one decision product (linear: X W^T; rbf: K(test, train), then K coef^T), one
         ``xps_bag_vote_f64`` launch, download of ``pred`` and ``votes``.

The bootstrap samples are sklearn's, draw for draw (``bagging_sample_indices``), so for the same ``random_state`` the ensemble is
the one sklearn's bagging would train.  Each estimator's problems are posed by the builder ``SVC.fit`` uses, and all are solved by
the same driver (decoders/_ovo.py).  There is no CPU fallback."""
import numbers

import numpy as np
import torch
from sklearn.base import BaseEstimator, ClassifierMixin
from sklearn.utils import check_random_state
from sklearn.utils.random import sample_without_replacement

from .._dev import stream
from .._lib import call, lib  # noqa: F401  (lib: stubbed with call by the host tests that allow no device work before a refusal)
from ..alignment import _linalg as LA
from . import _ovo
from .svm import SVC

MAX_INT = np.iinfo(np.int32).max            # sklearn.ensemble._bagging.MAX_INT


def n_draws(max_samples, n_samples):
    """sklearn's ``_max_samples``: an int is taken as it is, a float is ``int(max_samples * n_samples)``."""
    n_draw = max_samples if isinstance(max_samples, numbers.Integral) else int(max_samples * n_samples)
    if n_draw > n_samples:
        raise ValueError('max_samples must be <= n_samples')
    if n_draw < 1:
        raise ValueError('max_samples must draw at least one sample')
    return int(n_draw)


def bagging_sample_indices(random_state, n_estimators, n_samples, n_features, max_samples=1.0, bootstrap=True):
    """The sample indices sklearn's ``BaggingClassifier`` (1.7) draws for its estimators, as ``estimators_samples_`` lists them
    (host only).  One seed per estimator from ``random_state``; a ``RandomState`` per seed; ``_generate_bagging_indices`` draws the
    FEATURE indices first (``max_features=1.0``, no feature bootstrap: ``sample_without_replacement`` of all features -- the same
    call is made here and its result thrown away, so whatever it takes from the generator is taken), then the samples: ``randint``
    with replacement, or ``sample_without_replacement``."""
    n_draw = n_draws(max_samples, n_samples)
    seeds = check_random_state(random_state).randint(MAX_INT, size=n_estimators)
    out = []
    for seed in seeds:
        rs = np.random.RandomState(seed)
        sample_without_replacement(n_features, n_features, random_state=rs)
        if bootstrap:
            out.append(rs.randint(0, n_samples, n_draw))
        else:
            out.append(sample_without_replacement(n_samples, n_draw, random_state=rs))
    return out


def sample_weights(samples, base_w, bootstrap=True):
    """The ``sample_weight`` sklearn's bagging hands to each estimator's fit (host only): ``base_w`` times the multiplicity of a row
    in the estimator's draws, or, without replacement, ``base_w`` on the drawn rows and zero elsewhere."""
    n = len(base_w)
    if bootstrap:
        return [base_w * np.bincount(s, minlength=n) for s in samples]
    weights = []
    for s in samples:
        mask = np.zeros(n, dtype=bool)
        mask[s] = True
        weights.append(np.where(mask, base_w, 0.0))
    return weights


class BaggingClassifier(ClassifierMixin, BaseEstimator):
    """``sklearn.ensemble.BaggingClassifier`` for ``estimator=decoders.SVC(...)``, trained and evaluated as ONE device problem.

    Constructor, ``get_params`` / ``set_params`` (``estimator__C``, ``n_estimators``, ...) / ``clone`` and the pipeline step name
    (``baggingclassifier``) are sklearn's.  ``estimator`` must be a ``decoders.SVC`` (``TypeError`` otherwise, ``None`` included);
    ``max_features != 1.0``, ``bootstrap_features``, ``oob_score`` and ``warm_start`` raise ``NotImplementedError``; ``n_jobs`` and
    ``verbose`` are accepted and ignored.  The estimator's own unsupported settings raise as ``SVC.fit`` raises them.

    Attributes after ``fit``: ``classes_``, ``n_classes_``, ``n_features_in_``, ``estimators_samples_`` (sklearn's draws),
    ``n_iter_`` (a list of E arrays: the SMO iterations of each estimator's class pairs).  ``predict_proba`` is ``votes /
    n_estimators`` (sklearn's voting fallback for an estimator without ``predict_proba``); ``predict`` is the first maximum.
    ``estimators_`` and ``decision_function`` are NOT provided: the estimators exist only as rows of one coefficient matrix, and
    sklearn's own ``decision_function`` fails on an ensemble whose bootstrap lost a class."""

    def __init__(self, estimator=None, n_estimators=10, *, max_samples=1.0, max_features=1.0, bootstrap=True, bootstrap_features=False,
                 oob_score=False, warm_start=False, n_jobs=None, random_state=None, verbose=0):
        self.estimator = estimator
        self.n_estimators = n_estimators
        self.max_samples = max_samples
        self.max_features = max_features
        self.bootstrap = bootstrap
        self.bootstrap_features = bootstrap_features
        self.oob_score = oob_score
        self.warm_start = warm_start
        self.n_jobs = n_jobs
        self.random_state = random_state
        self.verbose = verbose

    # ------------------------------------------------------------------ fit
    def _check_settings(self):
        if not isinstance(self.estimator, SVC):
            raise TypeError(f'estimator must be a decoders.SVC instance (the ensemble runs on the device; there is no CPU fallback); '
                            f'got {type(self.estimator).__name__}')
        if not (isinstance(self.max_features, float) and self.max_features == 1.0):
            raise NotImplementedError('max_features other than 1.0 is not implemented on the HIP path')
        for name in ('bootstrap_features', 'oob_score', 'warm_start'):
            if getattr(self, name):
                raise NotImplementedError(f'{name} is not implemented on the HIP path')
        if not isinstance(self.n_estimators, numbers.Integral) or self.n_estimators < 1:
            raise ValueError('n_estimators must be a positive integer')
        self.estimator._check_settings()

    def fit(self, X, y, sample_weight=None):
        self._check_settings()
        est = self.estimator
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        y = np.asarray(y)
        if X.ndim != 2 or y.ndim != 1 or X.shape[0] != y.shape[0]:
            raise ValueError('X must be (n_samples, n_features) and y (n_samples,)')
        n, d = X.shape
        E = int(self.n_estimators)
        if E * 2016 > np.iinfo(np.int32).max:
            raise ValueError('n_estimators is too large')
        base_w = np.ones(n) if sample_weight is None else np.asarray(sample_weight, dtype=np.float64)
        if base_w.shape != (n,) or (base_w < 0).any():
            raise ValueError('sample_weight must be a non-negative (n_samples,) vector')
        classes, yi = np.unique(y, return_inverse=True)
        k = len(classes)
        if k < 2:
            raise ValueError('The number of classes has to be greater than one; got 1 class')
        if k > 64:
            raise ValueError(f'the vote kernel takes 2..64 classes; got {k}')
        # the draws (host), then the weights sklearn would hand to each estimator's fit
        samples = bagging_sample_indices(self.random_state, E, n, d, self.max_samples, self.bootstrap)
        weights = sample_weights(samples, base_w, self.bootstrap)
        # everything that SVC.fit derives from the X / y it is handed is derived from the WHOLE X / y, as under sklearn's bagging
        gamma = _ovo.gamma_value(est.kernel, est.gamma, X)
        cw = _ovo.class_weights(est.class_weight, classes, yi)
        probs = [_ovo.pair_problems(yi, np.arange(n), cw, w) for w in weights]      # estimator-major; one estimator's as SVC.fit's
        idx, npos, pair_a, pair_b, sizes = (np.concatenate([p[key] for p in probs]) for key in ('idx', 'npos', 'pair_a', 'pair_b', 'sizes'))
        off = np.concatenate([[0], np.cumsum(sizes)])
        est_off = np.concatenate([[0], np.cumsum([len(p['npos']) for p in probs])])
        cb = np.concatenate([_ovo.bounds(est.C, p) for p in probs])
        # ---- the device: nothing below loops over estimators
        dev = LA.device()
        Xd = torch.from_numpy(X).to(dev)
        G = LA.dgemm(Xd, Xd, tb=True)
        sq = torch.diagonal(G).contiguous() if est.kernel == 'rbf' else None           # |x_i|^2: the Gram diagonal (libsvm: dot(x_i, x_i))
        K = _ovo.kernel_from_gram(est.kernel, gamma, G, sq, sq)
        idx_d, off_d, npos_d, pa_d, pb_d, eo_d = _ovo.upload_int32([idx, off, npos, pair_a, pair_b, est_off], dev)
        alpha, rho, iters = _ovo.smo(K, idx_d, off_d, npos_d, int(sizes.max()), cb, est.tol, est.max_iter)
        coef = _ovo.coef_scatter(alpha, idx_d, off_d, npos_d, n)
        if est.kernel == 'linear':
            self._W, self._coef = LA.dgemm(coef, Xd), None  # (Q, d) weight vectors; the coefficients are not needed again
            self._Xd = None
        else:
            self._W, self._coef = None, coef
            self._Xd = Xd
        self._kernel, self._gamma, self._sq, self._rho = est.kernel, gamma, sq, rho
        self._pair_a, self._pair_b, self._est_off = pa_d, pb_d, eo_d        # (views of the one int32 upload)
        self._E, self._samples = E, samples
        self.classes_ = classes
        self.n_classes_ = k
        self.n_features_in_ = d
        iters_h = iters.cpu().numpy()
        self.n_iter_ = [iters_h[a:b] for a, b in zip(est_off[:-1], est_off[1:])]
        return self

    @property
    def estimators_samples_(self):
        """The drawn sample indices of each estimator, as sklearn's property of the same name lists them."""
        return list(self._samples)

    # ------------------------------------------------------------------ decisions
    def _decision_product(self, X):
        """(m, Q) raw decision values on the device (rho not yet subtracted): one upload, one product."""
        if not hasattr(self, '_rho'):
            raise RuntimeError('this BaggingClassifier is not fitted yet')
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        if X.ndim != 2 or X.shape[1] != self.n_features_in_:
            raise ValueError(f'X must be (n_samples, {self.n_features_in_})')
        Xd = torch.from_numpy(X).to(LA.device())
        if self._W is not None:
            return LA.dgemm(Xd, self._W, tb=True)
        Kx = _ovo.kernel_matrix(self._kernel, self._gamma, Xd, _ovo.row_sq_norms(Xd), self._Xd, self._sq)      # (m, n)
        return LA.dgemm(Kx, self._coef, tb=True)

    def _pair_decisions(self, X):
        """Decision values minus rho of all Q problems, (m, Q) on the host: estimator-major, libsvm's pair order inside each."""
        return (self._decision_product(X) - self._rho[None, :]).cpu().numpy()

    def _vote(self, X):
        dec = self._decision_product(X)
        m = dec.shape[0]
        votes = torch.empty(m, self.n_classes_, dtype=torch.int32, device=dec.device)
        pred = torch.empty(m, dtype=torch.int32, device=dec.device)
        call('xps_bag_vote_f64', dec.data_ptr(), dec.stride(0), self._rho.data_ptr(), self._pair_a.data_ptr(), self._pair_b.data_ptr(),
             self._est_off.data_ptr(), m, self._E, self.n_classes_, votes.data_ptr(), pred.data_ptr(), stream())
        return pred.cpu().numpy(), votes.cpu().numpy()

    def predict(self, X):
        return self.classes_.take(self._vote(X)[0])

    def predict_proba(self, X):
        return self._vote(X)[1] / float(self._E)
