"""Alignment-quality measures on the MI355X: the cluster separability scores of the reference's figure analyses
(``supp_fig_5`` / ``supp_fig_6_7``: sklearn's ``silhouette_samples``, ``calinski_harabasz_score`` and ``davies_bouldin_score``,
the notebooks' ``silhouette_scorer`` and their shuffled-label control) and the reference's ``alignment/metrics.py``
(``pt_corr`` :41, ``pt_corr_multi`` :12).

Every score of every label vector is a label-grouped sum over ONE n x n Gram matrix G of the centred data: the
distances are sqrt(G_ii + G_jj - 2 G_ij), the class-block sums of G give the dispersions and the centroid distances.  So a
permutation null of R shuffles costs one Gram product and a fixed number of launches per chunk of label sets
(csrc/xps_cluster.hip); only k x k tables, k-vectors, the three silhouette statistics and the silhouettes themselves come down.
Everything is float64 (float32 input is widened) and deterministic: a label set gives the same bits alone, among shuffles and in
any chunking.  There is no CPU fallback; argument errors are raised before the device is looked for.
"""
import numpy as np
import torch
from scipy import special

from . import _linalg as LA
from .alignment_utils import label2str

MAX_CLASSES = LA.CLUSTER_MAX_CLASSES
SCORES = ('silhouette', 'silhouette_pos', 'calinski_harabasz', 'davies_bouldin')


# ------------------------------------------------------------------------------------------------ arguments (no device)
def _shape_of(X, what):
    """(n, D) of X (n, ...) flattened; numpy or torch, checked without touching the device."""
    shape = tuple(X.shape) if isinstance(X, torch.Tensor) else np.shape(X)
    if len(shape) < 1 or shape[0] < 1:
        raise ValueError(f'{what}: X must be (n_samples, ...)')
    D = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    if D < 1:
        raise ValueError(f'{what}: X has no features')
    return int(shape[0]), D


def _label_vector(labels, n, what):
    """1-D labels as they are; 2-D label sequences as their strings (label2str, as the aligners read them)."""
    if hasattr(labels, 'detach'):
        labels = labels.detach().cpu().numpy()
    labels = np.asarray(labels)
    if labels.ndim > 1:
        labels = label2str(labels)
    if labels.ndim != 1 or len(labels) != n:
        raise ValueError(f'{what}: a label vector has {labels.shape[0] if labels.ndim else 0} entries for {n} samples')
    return labels


def _codes(labels, n, what):
    """(codes, k): the class index of every sample in np.unique's order.  2 <= k <= n - 1 as sklearn demands; k <= 64."""
    uniq, codes = np.unique(labels, return_inverse=True)
    k = len(uniq)
    if not 2 <= k <= n - 1:
        raise ValueError(f'{what}: number of labels is {k}; valid values are 2 to n_samples - 1 (inclusive)')
    if k > MAX_CLASSES:
        raise ValueError(f'{what}: {k} classes; at most {MAX_CLASSES} are supported')
    return np.asarray(codes).reshape(-1).astype(np.uint8), k


def _generator(random_state):
    """None: numpy's global generator (np.random.seed(s) reproduces the notebooks' np.random.permutation); an int seeds a
    RandomState; a RandomState or Generator is used as it is."""
    if random_state is None:
        return np.random
    if isinstance(random_state, (int, np.integer)):
        return np.random.RandomState(int(random_state))
    if hasattr(random_state, 'permutation'):
        return random_state
    raise ValueError(f'random_state must be None, an int or a numpy generator; got {random_state!r}')


# ------------------------------------------------------------------------------------------------ host formulas (k x k tables)
def _ch_db(M, dg, intra_sum, counts, ks, n):
    """Calinski-Harabasz and Davies-Bouldin of every label set from its downloaded tables: M (R, k, k) class-block sums of G,
    dg (R, k) per-class sums of the diagonal of G, intra_sum (R, k) per-class sums of the own-centroid distances, counts (R, k),
    ks (R,) the number of classes of each set.  The sums over classes are taken class by class in ascending order and every
    other step is elementwise, so a set's bits do not depend on the sets beside it (an empty class adds +0.0)."""
    R, k = counts.shape
    cnt = counts.astype(np.float64)
    full = cnt > 0
    safe = np.where(full, cnt, 1.0)
    Md = M[:, np.arange(k), np.arange(k)]
    trace, between = np.zeros(R), np.zeros(R)
    for q in range(k):
        trace = trace + dg[:, q]
        between = between + np.where(full[:, q], Md[:, q] / safe[:, q], 0.0)       # sum_q n_q |c_q|^2: the data is centred
    within = trace - between
    with np.errstate(divide='ignore', invalid='ignore'):
        ch = np.where(within > 0.0, between * (n - ks) / (within * (ks - 1.0)), 1.0)           # sklearn: 1.0 for no dispersion

        intra = np.where(full, intra_sum / safe, 0.0)
        c2 = Md / (safe * safe)
        cd2 = c2[:, :, None] + c2[:, None, :] - 2.0 * M / (safe[:, :, None] * safe[:, None, :])
        pair = full[:, :, None] & full[:, None, :] & ~np.eye(k, dtype=bool)[None]
        cd = np.where(pair, np.sqrt(np.maximum(cd2, 0.0)), 0.0)
        # sklearn's two zero-division cases: every cluster a point, or every centroid the same point -> 0.0
        degenerate = (np.abs(intra) <= 1e-8).all(axis=1) | (np.abs(cd) <= 1e-8).all(axis=(1, 2))
        ratio = np.where(cd > 0.0, (intra[:, :, None] + intra[:, None, :]) / np.where(cd > 0.0, cd, 1.0), 0.0)
        worst = ratio.max(axis=2)
        total = np.zeros(R)
        for p in range(k):
            total = total + worst[:, p]
        db = np.where(degenerate, 0.0, total / ks)
    return ch, db


class ClusterScores:
    """Scores of 1 + n_shuffles (+ extra) label sets of the same samples.  Set 0 is the given labels, sets 1..n_shuffles their
    permutations in the order they were drawn, then the ``label_sets``.

    silhouette_samples_ (sets, n); silhouette_, silhouette_pos_ (the mean of the positive silhouettes: the notebooks'
    ``silhouette_scorer``; NaN when none is positive), calinski_harabasz_, davies_bouldin_ (sets,); p_value_: per score name
    (1 + #{shuffle at least as extreme as set 0}) / (1 + n_shuffles), smaller counting as more extreme for Davies-Bouldin;
    labels_: the label vectors in set order; n_shuffles."""

    def __init__(self, sil, stats, ch, db, labels, n_shuffles):
        self.silhouette_samples_ = sil
        self.silhouette_ = np.ascontiguousarray(stats[:, 0])
        self.silhouette_pos_ = np.ascontiguousarray(stats[:, 1])
        self.calinski_harabasz_ = ch
        self.davies_bouldin_ = db
        self.labels_ = labels
        self.n_shuffles = int(n_shuffles)
        self.p_value_ = {name: permutation_p_value(getattr(self, name + '_'), self.n_shuffles, smaller=(name == 'davies_bouldin'))
                         for name in SCORES}


def permutation_p_value(values, n_shuffles, smaller=False):
    """(1 + #{r in 1..n_shuffles: values[r] at least as extreme as values[0]}) / (1 + n_shuffles); a NaN never counts."""
    null = np.asarray(values)[1:1 + n_shuffles]
    hits = (null <= values[0]) if smaller else (null >= values[0])
    return (1.0 + float(np.count_nonzero(hits))) / (1.0 + n_shuffles)


def bytes_per_set(n, k):
    """Device bytes one label set adds to a chunk: two (n, k) sum tables, the silhouettes, the centroid distances, the k x k and
    k tables, the three statistics and the labels."""
    return 8 * (2 * n * k + 2 * n + k * k + 2 * k + 3) + n


def sets_per_chunk(n, k, max_bytes):
    """Label sets whose device tables fit max_bytes; at least one."""
    return int(max(1, int(max_bytes) // bytes_per_set(n, k)))


# ------------------------------------------------------------------------------------------------ the device pass
def cluster_scores(X, labels, n_shuffles=0, random_state=None, label_sets=None, max_bytes=2 ** 28):
    """Silhouette, Calinski-Harabasz and Davies-Bouldin scores of X (n, ...) under ``labels``, under ``n_shuffles`` permutations
    of them (``rng.permutation(labels)`` drawn in order on the host) and under every extra vector of ``label_sets`` (each with
    its own classes), from ONE Gram matrix.  X: numpy or device tensor, float32 or float64.  -> ClusterScores."""
    what = 'cluster_scores'
    n, _ = _shape_of(X, what)
    if not (isinstance(n_shuffles, (int, np.integer)) and n_shuffles >= 0):
        raise ValueError(f'{what}: n_shuffles must be a non-negative integer; got {n_shuffles!r}')
    if not (isinstance(max_bytes, (int, np.integer)) and max_bytes >= 1):
        raise ValueError(f'{what}: max_bytes must be a positive integer; got {max_bytes!r}')
    rng = _generator(random_state)
    base = _label_vector(labels, n, what)
    extra = [_label_vector(ls, n, what + ' label_sets') for ls in ([] if label_sets is None else label_sets)]
    coded = [_codes(v, n, what) for v in [base] + extra]                 # every refusal before the first draw and the device
    vectors = [base] + [rng.permutation(base) for _ in range(int(n_shuffles))] + extra
    uniq = np.unique(base)
    coded = [coded[0]] + [(np.searchsorted(uniq, v).astype(np.uint8), coded[0][1]) for v in vectors[1:1 + n_shuffles]] + coded[1:]
    sets = len(coded)
    ks = np.array([k for _, k in coded], dtype=np.float64)
    k = int(ks.max())
    codes = np.stack([c for c, _ in coded], axis=1)                      # (n, sets): the kernels' transposed layout
    counts = np.stack([np.bincount(c, minlength=k) for c, _ in coded]).astype(np.int32)

    dev = LA.device()
    Xd = LA.to_device(X).reshape(n, -1)                                  # one upload
    Xc = Xd.to(LA.F64) - LA.col_mean(Xd)                                 # about the grand mean
    G = torch.empty(n, n, dtype=LA.F64, device=dev)
    keep = [LA.gram_grouped([(Xc, G)])]                                  # host tables: alive until the last download
    diag = G.diagonal().contiguous().view(n, 1)

    sil = np.empty((sets, n))
    stats, ch, db = np.empty((sets, 3)), np.empty(sets), np.empty(sets)
    step = sets_per_chunk(n, k, max_bytes)
    for s0 in range(0, sets, step):
        s1 = min(sets, s0 + step)
        Rc = s1 - s0
        lt = torch.from_numpy(np.ascontiguousarray(codes[:, s0:s1])).to(dev)
        cnt = counts[s0:s1]
        S0 = LA.label_row_sums(G, lt, k, 0)
        S1 = LA.label_row_sums(G, lt, k, 1)
        sil_d, stats_d, t_sil = LA.silhouette_from_sums(S1, cnt, lt)
        M = LA.label_col_sums(S0, lt, k)
        dg = LA.label_col_sums(diag, lt, k)
        dist, t_dist = LA.centroid_dist_from_sums(G, S0, M, cnt, lt)
        intra = LA.label_col_sums(dist.view(Rc, n, 1), lt, k)
        keep += [t_sil, t_dist]
        parts = [sil_d, stats_d, M, dg, intra]
        host = torch.cat([p.reshape(-1) for p in parts]).cpu().numpy()   # one download
        cuts = np.cumsum([0] + [p.numel() for p in parts])
        sil[s0:s1] = host[cuts[0]:cuts[1]].reshape(Rc, n)
        stats[s0:s1] = host[cuts[1]:cuts[2]].reshape(Rc, 3)
        ch[s0:s1], db[s0:s1] = _ch_db(host[cuts[2]:cuts[3]].reshape(Rc, k, k), host[cuts[3]:cuts[4]].reshape(Rc, k),
                                      host[cuts[4]:cuts[5]].reshape(Rc, k), cnt, ks[s0:s1], n)
    return ClusterScores(sil, stats, ch, db, vectors, n_shuffles)


def silhouette_samples(X, labels):
    """sklearn.metrics.silhouette_samples(X, labels) (euclidean): float64 ndarray (n,)."""
    return cluster_scores(X, labels).silhouette_samples_[0]


def silhouette_score(X, labels):
    """sklearn.metrics.silhouette_score(X, labels) (euclidean, all samples): the mean silhouette."""
    return cluster_scores(X, labels).silhouette_[0]


def silhouette_scorer(X, labels):
    """The notebooks' reduction (supp_fig_5): the mean of the positive silhouettes; NaN when none is positive."""
    return cluster_scores(X, labels).silhouette_pos_[0]


def calinski_harabasz_score(X, labels):
    """sklearn.metrics.calinski_harabasz_score(X, labels)."""
    return cluster_scores(X, labels).calinski_harabasz_[0]


def davies_bouldin_score(X, labels):
    """sklearn.metrics.davies_bouldin_score(X, labels)."""
    return cluster_scores(X, labels).davies_bouldin_[0]


# ------------------------------------------------------------------------------------------------ pt_corr
def _pearson_p(r, length):
    """scipy.stats.pearsonr's two-sided p-value: r is beta(L / 2 - 1, L / 2 - 1) on (-1, 1) under the null."""
    if length == 2:
        return np.where(np.isnan(r), np.nan, 1.0)
    ab = length / 2.0 - 1.0
    return 2.0 * special.betaincc(ab, ab, (np.abs(r) + 1.0) / 2.0)


def _pt_corr_many(target, others, p_vals, what):
    shape = tuple(target.shape) if hasattr(target, 'shape') else np.shape(target)
    if len(shape) < 1 or shape[0] < 1:
        raise ValueError(f'{what}: target must be (n_conditions, ...)')
    n_c = int(shape[0])
    L = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    if L < 2:
        raise ValueError(f'{what}: a condition needs at least 2 values')
    for o in others:
        if tuple(o.shape if hasattr(o, 'shape') else np.shape(o)) != shape:
            raise ValueError(f'{what}: target and to_corr must have the same shape')
    if not others:
        return [], []
    # columns = flattened conditions: the target's, then every comparison set's -> one centred covariance pass for all of them
    Z = torch.cat([LA.to_device(a).to(LA.F64).reshape(n_c, L) for a in [target] + list(others)]).t().contiguous()
    C = LA.xcov(Z, None, LA.col_mean(Z))
    cols = torch.arange(n_c, device=C.device)
    pick = [C.diagonal()] + [C[cols, cols + (i + 1) * n_c] for i in range(len(others))]
    host = torch.cat(pick).cpu().numpy()
    var, cxy = host[:n_c * (len(others) + 1)].reshape(-1, n_c), host[n_c * (len(others) + 1):].reshape(-1, n_c)
    rs, ps = [], []
    with np.errstate(divide='ignore', invalid='ignore'):
        for i in range(len(others)):
            r = cxy[i] / (np.sqrt(var[0]) * np.sqrt(var[i + 1]))        # scipy: (xm / |xm|) . (ym / |ym|), clipped
            r = np.where(np.isnan(r), np.nan, np.clip(r, -1.0, 1.0))
            r = np.round(r) if L == 2 else r
            rs.append(r)
            ps.append(_pearson_p(r, L) if p_vals else None)
    return rs, ps


def pt_corr(target, to_corr, p_vals=False):
    """Per-condition Pearson r between two datasets of one shape (n_conditions, ...), each condition flattened
    (scipy.stats.pearsonr's recipe in float64).  -> ndarray (n_conditions,), or (r, p-values) with ``p_vals``."""
    rs, ps = _pt_corr_many(target, [to_corr], p_vals, 'pt_corr')
    return (rs[0], ps[0]) if p_vals else rs[0]


def pt_corr_multi(target, to_corr_list, p_vals=False):
    """pt_corr of ``target`` against every dataset of ``to_corr_list``: a list of ndarrays, or (list of r, list of p-values)
    with ``p_vals``.  All comparison sets share one device pass over ``target``."""
    rs, ps = _pt_corr_many(target, list(to_corr_list), p_vals, 'pt_corr_multi')
    return (rs, ps) if p_vals else rs
