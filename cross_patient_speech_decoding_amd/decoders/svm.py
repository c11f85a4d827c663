"""Support-vector classifier on the MI355X -- the decoder of BASELINE config 1 (cross-patient SVM decode).

The reference hands the pooled, aligned features to ``sklearn.svm.SVC``: ``SVC(kernel='linear')`` inside a ``BaggingClassifier``
(scripts/aligned_decode_svm.py:262-263) and ``SVC(kernel='rbf', class_weight='balanced')`` behind ``DimRedReshape`` in the
nested-CV and sub-sampling scripts (scripts/aligned_decode_svm_ncv.py:313-321, scripts/aligned_decode_*_subsample.py:249-261);
decoders/cross_pt_decoders.py:29-38 only call ``decoder.fit / predict / score``.  ``SVC`` below is a drop-in for that estimator
(constructor arguments, ``fit`` / ``predict`` / ``decision_function`` / ``score`` / ``classes_`` / ``get_params`` / ``set_params`` /
``clone``), so it can be bagged, grid-searched, put into a pipeline and wrapped by ``crossPtDecoder_*`` unchanged.  It solves what
libsvm solves: one C-SVC per class pair (classes ascending, the lower class positive), SMO with the second-order working-set rule,
tolerance ``tol`` on the maximal KKT violation, libsvm's ``rho``; per-point upper bound C * class_weight * sample_weight; the
prediction is libsvm's one-vs-one vote (ties: the lowest class).  On the device: the Gram matrix X X^T (f64 MFMA), for
``kernel='rbf'`` exp(-gamma ||x - y||^2) from it (csrc/xps_svm.hip, libsvm's formula), ALL pair problems in one launch, the
decision values as f64 GEMMs.  What a fit resolves from its data, how it poses the pair problems and how it launches them is
shared with the bagged ensemble and the grid search: decoders/_ovo.py.  There is no CPU fallback."""
import numpy as np
import torch
from sklearn.base import BaseEstimator, ClassifierMixin

from ..alignment import _linalg as LA
from . import _ovo
from ._ovo import class_weights as _class_weights  # noqa: F401  (imported from here by the tests)


def _ovr_from_ovo(dec, n_classes):
    """sklearn.utils.multiclass._ovr_decision_function(dec < 0, -dec, n_classes): votes plus the monotonically squashed sum of
    the pairwise confidences -- what SVC.decision_function returns for decision_function_shape='ovr'."""
    predictions, confidences = dec < 0, -dec
    m = dec.shape[0]
    votes = np.zeros((m, n_classes))
    sums = np.zeros((m, n_classes))
    k = 0
    for i in range(n_classes):
        for j in range(i + 1, n_classes):
            sums[:, i] -= confidences[:, k]
            sums[:, j] += confidences[:, k]
            votes[predictions[:, k] == 0, i] += 1
            votes[predictions[:, k] == 1, j] += 1
            k += 1
    return votes + sums / (3 * (np.abs(sums) + 1))


class SVC(ClassifierMixin, BaseEstimator):
    """C-support vector classification, ``kernel='linear'`` or ``'rbf'`` (sklearn.svm.SVC semantics for these)."""

    def __init__(self, C=1.0, kernel='rbf', gamma='scale', tol=1e-3, max_iter=-1, decision_function_shape='ovr', break_ties=False,
                 class_weight=None, random_state=None):
        self.C = C
        self.kernel = kernel
        self.gamma = gamma
        self.tol = tol
        self.max_iter = max_iter
        self.decision_function_shape = decision_function_shape
        self.break_ties = break_ties
        self.class_weight = class_weight
        self.random_state = random_state

    def _check_settings(self):
        """The settings the HIP path does not implement are refused (by ``fit``, and by the bagged ensemble on its estimator)."""
        if self.kernel not in ('linear', 'rbf'):
            raise NotImplementedError("the HIP SVC implements kernel='linear' and kernel='rbf' (what the reference's decoders use)")
        if self.break_ties:
            raise NotImplementedError('break_ties is not implemented on the HIP path')
        if self.decision_function_shape not in ('ovr', 'ovo'):
            raise ValueError("decision_function_shape must be 'ovr' or 'ovo'")

    def _gamma_value(self, X):
        return _ovo.gamma_value(self.kernel, self.gamma, X)

    # ------------------------------------------------------------------ fit
    def fit(self, X, y, sample_weight=None):
        self._check_settings()
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        y = np.asarray(y)
        if X.ndim != 2 or X.shape[0] != y.shape[0]:
            raise ValueError('X must be (n_samples, n_features) and y (n_samples,)')
        self._gamma = self._gamma_value(X)
        classes, yi_all = np.unique(y, return_inverse=True)
        cw = _ovo.class_weights(self.class_weight, classes, yi_all)
        self.class_weight_ = cw
        # sample weights (BaggingClassifier passes the bootstrap multiplicities): per-point bound C * class weight * w; zero-weight
        # points are dropped before training, as sklearn's libsvm does
        w = np.ones(X.shape[0]) if sample_weight is None else np.asarray(sample_weight, dtype=np.float64)
        if w.shape != (X.shape[0],) or (w < 0).any():
            raise ValueError('sample_weight must be a non-negative (n_samples,) vector')
        keep = w > 0
        X, y, w = X[keep], y[keep], w[keep]
        self.classes_, yi = np.unique(y, return_inverse=True)
        if len(self.classes_) != len(classes):               # a class lost all its weight: its weight entry goes with it
            cw = cw[np.isin(classes, self.classes_)]
        k = len(self.classes_)
        n = X.shape[0]
        p = _ovo.pair_problems(yi, np.arange(n), cw, w)
        off = np.concatenate([[0], np.cumsum(p['sizes'])])
        dev = LA.device()
        Xd = torch.from_numpy(X).to(dev)
        self._sq = _ovo.row_sq_norms(Xd) if self.kernel == 'rbf' else None
        K = _ovo.kernel_matrix(self.kernel, self._gamma, Xd, self._sq, Xd, self._sq)
        idx_d, off_d, npos_d = _ovo.upload_int32([p['idx'], off, p['npos']], dev)
        alpha, rho, iters = _ovo.smo(K, idx_d, off_d, npos_d, int(p['sizes'].max()), _ovo.bounds(self.C, p), self.tol, self.max_iter)
        coef = _ovo.coef_scatter(alpha, idx_d, off_d, npos_d, n)    # signed dual coefficients of every pair, dense (P, n)
        self._Xd = Xd
        self._rho = rho
        self._pairs = list(zip(p['pair_a'].tolist(), p['pair_b'].tolist()))
        self.n_iter_ = iters.cpu().numpy()
        self.dual_coef_pairs_ = coef                                # (kept on the device; sklearn's dual_coef_ packs it differently)
        self.n_features_in_ = X.shape[1]
        flip = -1.0 if k == 2 else 1.0                              # sklearn flips coef_ / intercept_ / the decision of a binary problem
        if self.kernel == 'linear':
            self._W = LA.dgemm(coef, Xd)                            # (P, d) weight vectors: W = coef X (f64 GEMM)
            self.coef_ = flip * self._W.cpu().numpy()
        self.intercept_ = flip * -rho.cpu().numpy()
        return self

    # ------------------------------------------------------------------ decisions
    def _pair_decisions(self, X):
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        Xd = torch.from_numpy(X).to(LA.device())
        if self.kernel == 'linear':
            return (LA.dgemm(Xd, self._W, tb=True) - self._rho[None, :]).cpu().numpy()     # (m, P)
        Kx = _ovo.kernel_matrix(self.kernel, self._gamma, Xd, _ovo.row_sq_norms(Xd), self._Xd, self._sq)      # (m, n)
        return (LA.dgemm(Kx, self.dual_coef_pairs_, tb=True) - self._rho[None, :]).cpu().numpy()

    def decision_function(self, X):
        """sklearn's layout: two classes: a vector, positive for ``classes_[1]``; more: ``decision_function_shape='ovo'`` the
        one-vs-one values (m, P), columns in libsvm's pair order (0 v 1, 0 v 2, ..., k-2 v k-1), ``'ovr'`` (the default) the (m, k)
        vote-plus-confidence scores sklearn derives from them."""
        dec = self._pair_decisions(X)
        k = len(self.classes_)
        if k == 2:
            return -dec[:, 0]
        if self.decision_function_shape == 'ovr':
            return _ovr_from_ovo(dec, k)
        return dec

    def predict(self, X):
        dec = self._pair_decisions(X)
        k = len(self.classes_)
        votes = np.zeros((dec.shape[0], k), dtype=np.int64)
        for p_, (a, b) in enumerate(self._pairs):
            pos = dec[:, p_] > 0
            votes[pos, a] += 1
            votes[~pos, b] += 1
        return self.classes_[np.argmax(votes, axis=1)]             # first maximum: libsvm's tie rule
