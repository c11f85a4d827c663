"""PCA on the MI355X with scikit-learn's conventions (the reference calls
``sklearn.decomposition.PCA`` at nn_models/data_utils/datamodules.py:542-548 and
alignment/JointPCA.py:199).

covariance (xps_xcov_f64, f64 MFMA) -> Jacobi eigendecomposition (xps_jacobi_*) -> sklearn's sign
rule (largest-|.| entry of each component positive) and component-count rule for a variance
fraction (``searchsorted(cumsum(ratio), n, side='right') + 1``) -> transform = (X - mean) W on the
device (xps_apply_f64).  This is exactly what sklearn's 'covariance_eigh' solver computes; where
sklearn would pick its unseeded randomized solver this class returns the exact answer instead.

``solver='gram'`` is the same PCA from the sample side, for wide data (the flattened trials behind ``DimRedReshape``: 144 rows of
22 200 features, whose covariance would be a 3.9 GB matrix): centred rows -> G = Xc Xc^T (n x n, f64 MFMA GEMM) -> Jacobi ->
explained variance L / (n - 1), components (Xc^T U_k) L_k^-1/2 by one device product.  The direction of a component with
eigenvalue L_i carries an error of about eps * L_0 / L_i, so a kept component below L_0 / PCA_SPECTRUM_LIMIT is refused.
``solver='auto'`` takes the Gram side when there are more features than rows; ``GramPCA`` is the class whose default that is.
"""
import numpy as np

from . import _linalg as LA

SOLVERS = ('covariance', 'gram', 'auto')
PCA_SPECTRUM_LIMIT = 1e6            # a kept Gram-side component needs L_i >= L_0 / this: direction error eps * L_0 / L_i <= ~1e-10


def count_components(n_components, ratio, n, d):
    """The class's component-count rule: ``ratio`` is the explained-variance-ratio curve of the fit, (n, d) the shape of X."""
    if n_components is None:
        k = min(n, d)
    elif 0 < n_components < 1:
        k = int(np.searchsorted(np.cumsum(ratio), n_components, side='right') + 1)
    else:
        k = int(n_components)
    return max(1, min(k, d))


def sign_rule(M, axis):
    """sklearn's sign rule: the factors (+1 / -1) that make the entry of largest magnitude along ``axis`` of every vector of M
    positive -- the first such entry on a tie; a zero entry counts as +1.  M is 2-D: axis 0 for vectors in columns, 1 for rows."""
    M = np.asarray(M)
    idx = np.argmax(np.abs(M), axis=axis)
    other = np.arange(len(idx))
    signs = np.sign(M[idx, other] if axis == 0 else M[other, idx])
    signs[signs == 0] = 1
    return signs


def gram_ratio(L, n, d):
    """The ratio curve of a Gram-side spectrum L (descending): over the min(n, d) leading eigenvalues, clipped at 0."""
    L = np.clip(np.asarray(L, dtype=np.float64)[:min(n, d)], 0.0, None)
    total = L.sum()
    return L / total if total > 0 else np.zeros_like(L)


class PCA:
    def __init__(self, n_components=None, solver='covariance', **_ignored):
        self.n_components = n_components
        self.solver = solver

    def get_params(self, deep=True):
        return {'n_components': self.n_components, 'solver': self.solver}

    def set_params(self, **params):
        for k, v in params.items():
            setattr(self, k, v)
        return self

    def fit(self, X, y=None):
        Xd = LA.to_device(X)
        Xd = Xd.reshape(-1, Xd.shape[-1])
        n, d = Xd.shape
        if self.solver not in SOLVERS:
            raise ValueError(f'solver must be one of {SOLVERS}; got {self.solver!r}')
        mean = LA.col_mean(Xd)
        if self.solver == 'gram' or (self.solver == 'auto' and d > n):
            return self._fit_gram(Xd, mean)
        cov = LA.xcov(Xd, None, mean) / (n - 1)
        return self._fit_from_eig(LA.eigh_psd(cov), mean, n, d)

    def _fit_from_eig(self, eig, mean, n, d):
        """The covariance solver's tail: (w, V) of the covariance of n rows of d features -> the fitted attributes."""
        w, V = eig
        w = np.clip(w, 0.0, None)
        comps = V.T.copy()
        total = w.sum()
        ratio = w / total if total > 0 else np.zeros_like(w)
        k = count_components(self.n_components, ratio, n, d)
        return self._set_fitted(mean, comps[:k], w[:k], ratio[:k], np.sqrt(w[:k] * (n - 1)), n)

    def _fit_gram(self, Xd, mean):
        n, d = Xd.shape
        Xc = Xd.to(LA.F64) - mean
        G = LA.dgemm(Xc, Xc, tb=True)
        w, U = LA.eigh_psd(0.5 * (G + G.t()))
        w = np.clip(w, 0.0, None)
        ratio = gram_ratio(w, n, d)
        k = min(count_components(self.n_components, ratio, n, d), n)
        if not w[k - 1] >= w[0] / PCA_SPECTRUM_LIMIT or w[k - 1] <= 0:
            raise ValueError(f"component {k - 1} of the {k} kept has the eigenvalue {w[k - 1]:.3e} against {w[0]:.3e} of the first: "
                             f"below 1 / {PCA_SPECTRUM_LIMIT:g} of it the Gram side (solver='gram') cannot resolve its direction.  "
                             "Ask for fewer components or use solver='covariance'")
        Wk = LA.to_device(np.ascontiguousarray(U[:, :k] / np.sqrt(w[:k])))
        comps = LA.dgemm(Wk, Xc, ta=True).cpu().numpy()           # (Xc^T U_k) L_k^-1/2 as rows: one device product
        return self._set_fitted(mean, comps, w[:k] / (n - 1), ratio[:k], np.sqrt(w[:k]), n)

    def _set_fitted(self, mean, comps, variance, ratio, singular_values, n):
        """The fitted attributes of either solver; comps (k, d) rows = components, their signs still the solver's."""
        self.mean_ = mean.cpu().numpy()
        self.components_ = comps * sign_rule(comps, 1)[:, None]
        self.explained_variance_ = variance
        self.explained_variance_ratio_ = ratio
        self.singular_values_ = singular_values
        self.n_components_, self.n_features_in_ = comps.shape
        self.n_samples_ = n
        self._mean_d = mean
        self._W_d = LA.to_device(np.ascontiguousarray(self.components_.T))
        return self

    def _check(self):
        if not hasattr(self, 'components_'):
            raise RuntimeError('This PCA instance is not fitted yet.')

    def transform_device(self, Xd, out_f32=False):
        self._check()
        return LA.apply(Xd, self._W_d, self._mean_d, out_f32=out_f32)

    def transform(self, X):
        self._check()
        return LA.like_input(self.transform_device(LA.to_device(X)), X)

    def fit_transform(self, X, y=None):
        return self.fit(X).transform(X)

    def inverse_transform(self, Z):
        self._check()
        Zd = LA.to_device(Z)
        W = LA.to_device(np.ascontiguousarray(self.components_))
        return (LA.apply(Zd, W) + self._mean_d).cpu().numpy()


def fit_many(Xs, n_components=None, solver='covariance'):
    """``PCA(n_components).fit(x)`` for every x of Xs -- inputs of any mix of widths -- with ONE eigh_psd_batched call over all
    the covariances: column mean and covariance per input as in ``PCA.fit``, then widths of the one-workgroup Jacobi share one
    launch per width and the wider ones share one ragged call.  Returns the fitted ``PCA`` objects, attribute for attribute
    what the separate fits give, bit for bit.  Only the covariance solver is batched."""
    if solver != 'covariance':
        raise ValueError(f"fit_many batches the covariance solver only; got solver={solver!r}")
    return [PCA(n_components=n_components, solver=solver)._fit_from_eig(e, mean, n, d) for e, mean, n, d in eig_many(Xs)]


def eig_many(Xs):
    """The part of ``fit_many`` that does not look at ``n_components``: per input (eig, mean, n, d) -- the eigendecomposition of its
    covariance, its column mean (device) and its shape -- with ONE eigh_psd_batched call.  ``PCA(v)._fit_from_eig(eig, mean, n, d)``
    is then the fit for any ``v``, so one decomposition serves a list of component counts (alignment.fit_folds_multi)."""
    means, covs, shapes = [], [], []
    for x in Xs:
        Xd = LA.to_device(x)
        Xd = Xd.reshape(-1, Xd.shape[-1])
        n, d = Xd.shape
        mean = LA.col_mean(Xd)
        means.append(mean)
        covs.append(LA.xcov(Xd, None, mean) / (n - 1))
        shapes.append((n, d))
    eigs = list(LA.eigh_psd_batched(covs)) if covs else []
    return [(e, mean, n, d) for e, mean, (n, d) in zip(eigs, means, shapes)]


class GramPCA(PCA):
    """``PCA`` whose default solver is ``'auto'``: ``DimRedReshape`` builds its reducer as ``dim_red(n_components=...)``, so the class
    itself carries the choice -- ``DimRedReshape(GramPCA)`` runs at the width of the flattened trials."""

    def __init__(self, n_components=None, solver='auto', **_ignored):
        super().__init__(n_components=n_components, solver=solver)
