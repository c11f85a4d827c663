"""Exact t-SNE on the MI355X behind sklearn's estimator surface: ``Silhouette (t-SNE)`` of the reference's figure analyses
(``fig_2`` / ``supp_fig_5`` / ``supp_fig_6_7``: ``get_cluster_scores(TSNE(n_components=2, perplexity=30).fit_transform(pt_time_pca),
labels, silhouette_scorer)``, per patient, unaligned and aligned, per iteration).

sklearn's recipe (``_t_sne.py`` / ``_utils.pyx``; restated in include/xps.h) with the EXACT gradient: squared
distances from one Gram matrix rounded to float32, the perplexity search, the joint probabilities, and ``_gradient_descent`` in
its two phases.  ``fit_transform_many`` puts data sets of different n and D into ONE device problem: one Gram launch, one distance
launch, two affinity launches and one launch per iteration for all of them, with two host synchronisations per fit whatever the
batch and ``max_iter``.  Float64 throughout (float32 input is widened), no atomics, fixed summation order: a data set gives the
same bits alone and inside any batch.  There is no CPU fallback; argument errors are raised before the device is looked for.
"""
import numpy as np
import torch
from sklearn.base import BaseEstimator
from sklearn.utils import check_random_state

from ..alignment import _linalg as LA
from ..alignment.metrics import _shape_of
from ..alignment.pca import PCA, fit_many

MAX_SAMPLES = LA.TSNE_MAX_SAMPLES
EXPLORATION_ITER = 250            # sklearn's _EXPLORATION_MAX_ITER: the phase with early exaggeration and momentum 0.5


def _download(parts):
    """ONE host synchronisation: the device tensors of ``parts`` as float64 ndarrays."""
    host = torch.cat([p.reshape(-1).to(LA.F64) for p in parts]).cpu().numpy()
    cuts = np.cumsum([0] + [p.numel() for p in parts])
    return [host[a:b].reshape(tuple(p.shape)) for p, a, b in zip(parts, cuts[:-1], cuts[1:])]


def _finite(X):
    return bool(torch.isfinite(X).all()) if isinstance(X, torch.Tensor) else bool(np.isfinite(np.asarray(X, dtype=np.float64)).all())


class TSNE(BaseEstimator):
    """sklearn.manifold.TSNE (1.7) with the exact gradient on the device.  Names and defaults are sklearn's, except ``method``:
    'exact' is the default and the only one ('barnes_hut' is refused).

    Fitted: embedding_ (n, n_components) float64, kl_divergence_, n_iter_, learning_rate_, n_features_in_, sigma_ (n,) =
    1 / sqrt(beta_i) of the perplexity search; after fit_transform_many the lists embeddings_, kl_divergences_, n_iters_,
    sigmas_ (and learning_rates_)."""

    def __init__(self, n_components=2, *, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', max_iter=1000,
                 n_iter_without_progress=300, min_grad_norm=1e-7, metric='euclidean', init='pca', verbose=0, random_state=None,
                 method='exact'):
        self.n_components = n_components
        self.perplexity = perplexity
        self.early_exaggeration = early_exaggeration
        self.learning_rate = learning_rate
        self.max_iter = max_iter
        self.n_iter_without_progress = n_iter_without_progress
        self.min_grad_norm = min_grad_norm
        self.metric = metric
        self.init = init
        self.verbose = verbose
        self.random_state = random_state
        self.method = method

    # -------------------------------------------------------------------------------------------- arguments (no device)
    def _check_params(self):
        if self.method != 'exact':
            raise ValueError(f"TSNE: method={self.method!r}: this estimator computes the exact gradient on the device; "
                             "method='barnes_hut' is not implemented (use method='exact', the default here)")
        if self.n_components not in (1, 2):
            raise ValueError(f'TSNE: n_components={self.n_components!r}: 1 or 2 are supported (both have one degree of freedom; '
                             'the reference notebooks use 2)')
        if self.metric not in ('euclidean', 'precomputed'):
            raise ValueError(f"TSNE: metric={self.metric!r}: 'euclidean' and 'precomputed' are supported")
        if not (isinstance(self.max_iter, (int, np.integer)) and self.max_iter >= 250):
            raise ValueError(f"The 'max_iter' parameter of TSNE must be an int in the range [250, inf). Got {self.max_iter!r} instead.")
        if not (isinstance(self.perplexity, (int, float, np.number)) and self.perplexity > 0):
            raise ValueError(f"The 'perplexity' parameter of TSNE must be a float in the range (0.0, inf). Got {self.perplexity!r} instead.")
        if not (isinstance(self.early_exaggeration, (int, float, np.number)) and self.early_exaggeration >= 1):
            raise ValueError("The 'early_exaggeration' parameter of TSNE must be a float in the range [1.0, inf). "
                             f'Got {self.early_exaggeration!r} instead.')
        if not (self.learning_rate == 'auto' if isinstance(self.learning_rate, str)
                else isinstance(self.learning_rate, (int, float, np.number)) and self.learning_rate > 0):
            raise ValueError("The 'learning_rate' parameter of TSNE must be a str among {'auto'} or a float in the range (0.0, inf). "
                             f'Got {self.learning_rate!r} instead.')
        if not (isinstance(self.n_iter_without_progress, (int, np.integer)) and self.n_iter_without_progress >= -1):
            raise ValueError("The 'n_iter_without_progress' parameter of TSNE must be an int in the range [-1, inf). "
                             f'Got {self.n_iter_without_progress!r} instead.')
        if not (isinstance(self.min_grad_norm, (int, float, np.number)) and self.min_grad_norm >= 0):
            raise ValueError(f"The 'min_grad_norm' parameter of TSNE must be a float in the range [0.0, inf). Got {self.min_grad_norm!r} instead.")
        if isinstance(self.init, str):
            if self.init not in ('pca', 'random'):
                raise ValueError("The 'init' parameter of TSNE must be a str among {'pca', 'random'} or an instance of 'numpy.ndarray'. "
                                 f'Got {self.init!r} instead.')
            if self.init == 'pca' and self.metric == 'precomputed':
                raise ValueError('The parameter init="pca" cannot be used with metric="precomputed".')
        elif not isinstance(self.init, np.ndarray):
            raise ValueError("The 'init' parameter of TSNE must be a str among {'pca', 'random'} or an instance of 'numpy.ndarray'. "
                             f'Got {type(self.init).__name__} instead.')

    def _check_data(self, X):
        n, D = _shape_of(X, 'TSNE')
        if self.perplexity >= n:
            raise ValueError(f'perplexity ({self.perplexity}) must be less than n_samples ({n})')
        if n > MAX_SAMPLES:
            raise ValueError(f'TSNE: {n} samples; at most XPS_TSNE_MAX_SAMPLES = {MAX_SAMPLES} are supported (the embedding of a '
                             'problem lives in LDS, its probabilities are n^2 doubles)')
        if not _finite(X):
            raise ValueError('Input X contains NaN or infinity.')
        if self.metric == 'precomputed':
            X = X if isinstance(X, torch.Tensor) else np.asarray(X)
            if X.ndim != 2 or X.shape[0] != X.shape[1]:
                raise ValueError('X should be a square distance matrix')
            if bool((X < 0).any()):
                raise ValueError("Negative values in data passed to TSNE.fit(). With metric='precomputed', X should contain positive distances..")       # sklearn's text, its two periods included
        return n, D

    def _inits(self, shapes, inits):
        """The host part of the initialisation: one float64 (n, nc) array per data set, or None where PCA makes it on the device."""
        nc = self.n_components
        if inits is None:
            inits = [self.init] * len(shapes)
        elif len(inits) != len(shapes):
            raise ValueError(f'TSNE: {len(inits)} inits for {len(shapes)} data sets')
        rng, out = None, []
        for (n, _), init in zip(shapes, inits):
            if isinstance(init, str):
                if init == 'pca':
                    if self.metric == 'precomputed':
                        raise ValueError('The parameter init="pca" cannot be used with metric="precomputed".')
                    out.append(None)
                    continue
                if init != 'random':
                    raise ValueError(f"TSNE: init={init!r}: 'pca', 'random' or an ndarray")
                rng = check_random_state(self.random_state) if rng is None else rng      # sklearn's draws, one data set after the other
                out.append((1e-4 * rng.standard_normal(size=(n, nc)).astype(np.float32)).astype(np.float64))
                continue
            init = np.asarray(init)
            if init.shape != (n, nc):
                raise ValueError(f'TSNE: init has the shape {init.shape}; ({n}, {nc}) is needed')
            if not np.isfinite(init).all():
                raise ValueError('TSNE: init contains NaN or infinity.')
            out.append(np.ascontiguousarray(init, dtype=np.float64))
        return out

    def _learning_rate(self, n):
        if isinstance(self.learning_rate, str):
            return float(np.maximum(n / self.early_exaggeration / 4, 50))
        return float(self.learning_rate)

    # -------------------------------------------------------------------------------------------- the device pass
    def fit_transform_many(self, Xs, inits=None):
        """The embeddings of the data sets Xs (each (n, ...), numpy or torch; n and D differ) as ONE device problem.  inits: one
        per data set ('pca', 'random' or an (n, n_components) ndarray); default: ``self.init`` for each.  Returns the list of
        float64 ndarrays; sets embeddings_, kl_divergences_, n_iters_, sigmas_, learning_rates_."""
        self._check_params()
        Xs = list(Xs)
        if not Xs:
            raise ValueError('TSNE: no data set')
        shapes = [self._check_data(X) for X in Xs]
        host_inits = self._inits(shapes, inits)                                         # every refusal before the device
        nc, max_iter = int(self.n_components), int(self.max_iter)
        lrs = [self._learning_rate(n) for n, _ in shapes]

        dev = LA.device()
        keep, probs = [], []
        for X, (n, _) in zip(Xs, shapes):
            pr = dict(n=n, nc=nc, D2=torch.empty(n, n, dtype=torch.float32, device=dev))
            for key in ('C', 'P'):
                pr[key] = torch.empty(n, n, dtype=LA.F64, device=dev)
            pr['beta'], pr['rowsum'] = torch.empty(n, dtype=LA.F64, device=dev), torch.empty(n, dtype=LA.F64, device=dev)
            pr['steps'] = torch.empty(n, dtype=torch.int32, device=dev)
            pr['X'] = LA.to_device(X).reshape(n, -1)
            probs.append(pr)
        if self.metric == 'precomputed':
            for pr in probs:
                D = pr['X'].to(LA.F64)
                pr['D2'] = (D * D).to(torch.float32).contiguous()                       # sklearn: distances **= 2, then astype(float32)
        else:
            for pr in probs:
                Xc = pr['X'].to(LA.F64) - LA.col_mean(pr['X'])
                pr['Xc'], pr['G'] = Xc, torch.empty(pr['n'], pr['n'], dtype=LA.F64, device=dev)
            keep.append(LA.gram_grouped([(pr['Xc'], pr['G']) for pr in probs]))
            keep.append(LA.tsne_sqdist(probs))
        keep.append(LA.tsne_affinities(probs, self.perplexity))

        pca_idx = [i for i, y in enumerate(host_inits) if y is None]
        if pca_idx:
            small = [i for i in pca_idx if shapes[i][1] <= shapes[i][0]]
            fitted = dict(zip(small, fit_many([probs[i]['X'] for i in small], n_components=nc))) if small else {}
            for i in pca_idx:
                pca = fitted[i] if i in fitted else PCA(n_components=nc, solver='gram').fit(probs[i]['X'])
                if pca.n_components_ != nc:
                    raise ValueError(f"TSNE: init='pca' found {pca.n_components_} components for n_components = {nc}")
                Y = pca.transform_device(probs[i]['X']).to(torch.float32)               # sklearn: .astype(np.float32)
                Y = Y / Y[:, 0].std(unbiased=False) * np.float32(1e-4)
                probs[i]['Y'] = Y.to(LA.F64).contiguous()
        for pr, y, lr in zip(probs, host_inits, lrs):
            if y is not None:
                pr['Y'] = torch.from_numpy(y).to(dev)
            pr['Y_in'] = pr['Y_out'] = pr['Y']                                          # a phase reads Y_in whole before it writes Y_out
            pr['state'], pr['lr'], pr['it_begin'] = LA.tsne_state(pr['n'], dev), lr, 0

        # phase 1: early exaggeration, momentum 0.5, n_iter_without_progress = 250
        keep.append(LA.tsne_descent(probs, EXPLORATION_ITER, EXPLORATION_ITER, 0.5, self.early_exaggeration, EXPLORATION_ITER,
                                    self.min_grad_norm))
        half = (LA.TSNE_STATE_HEAD + LA.TSNE_STATE_ARRAYS * np.array([pr['n'] for pr in probs])) * (EXPLORATION_ITER & 1)
        heads = _download([pr['state'][h:h + LA.TSNE_STATE_HEAD] for pr, h in zip(probs, half)])       # synchronisation 1
        its = [int(h[0]) for h in heads]
        errors = [float(h[1]) for h in heads]
        again = [i for i, it in enumerate(its) if it + 1 < max_iter]                    # sklearn: it < 250 or max_iter > 250
        n_launches = 0
        if again:
            for i in again:
                probs[i]['it_begin'] = its[i] + 1
            n_launches = max(max_iter - probs[i]['it_begin'] for i in again)
            keep.append(LA.tsne_descent([probs[i] for i in again], n_launches, max_iter, 0.8, 1.0, max(int(self.n_iter_without_progress), 0),
                                        self.min_grad_norm))
        parts = [pr['Y'] for pr in probs] + [pr['beta'] for pr in probs]
        for i in again:
            h = (LA.TSNE_STATE_HEAD + LA.TSNE_STATE_ARRAYS * probs[i]['n']) * (n_launches & 1)
            parts.append(probs[i]['state'][h:h + LA.TSNE_STATE_HEAD])
        host = _download(parts)                                                         # synchronisation 2
        m = len(probs)
        for i, h in zip(again, host[2 * m:]):
            its[i], errors[i] = int(h[0]), float(h[1])
        del keep
        self.embeddings_ = [np.ascontiguousarray(y) for y in host[:m]]
        with np.errstate(divide='ignore'):
            self.sigmas_ = [1.0 / np.sqrt(b) for b in host[m:2 * m]]
        self.kl_divergences_, self.n_iters_, self.learning_rates_ = errors, its, lrs
        self.n_features_ins_ = [D for _, D in shapes]
        if self.verbose:
            for i, (kl, it) in enumerate(zip(errors, its)):
                print(f'[t-SNE] data set {i}: KL divergence after {it + 1} iterations: {kl:f}')
        return self.embeddings_

    def fit_transform(self, X, y=None):
        """The embedding of X (n, ...): float64 ndarray (n, n_components).  The one-problem case of fit_transform_many."""
        Y = self.fit_transform_many([X])[0]
        self.embedding_ = Y
        self.kl_divergence_, self.n_iter_ = self.kl_divergences_[0], self.n_iters_[0]
        self.learning_rate_, self.sigma_, self.n_features_in_ = self.learning_rates_[0], self.sigmas_[0], self.n_features_ins_[0]
        return Y

    def fit(self, X, y=None):
        self.fit_transform(X)
        return self
