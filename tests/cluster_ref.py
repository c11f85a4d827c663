"""Restatement of the cluster separability scores in np.longdouble, for tests/test_gpu_cluster_kernels.py and
tests/test_gpu_cluster_scores.py (tests/test_cluster_ref_host.py checks the restatement itself against sklearn on the CPU).

The squared distances are direct differences sum (x_i - x_j)^2 -- no Gram trick --, the grouped sums and sklearn's rules follow:
silhouette a = own-class sum / (count - 1), b = smallest other-class mean, s = (b - a) / max(a, b), 0 for a sample alone in its
class; Calinski-Harabasz and Davies-Bouldin from the class centroids.  Also here: the fixed-seed cases of the GPU tests, and the
error bars those tests hold the device route to, derived from the data of each case (nothing is a number chosen in advance):

* a distance taken through the Gram matrix, d^2 = G_ii + G_jj - 2 G_ij with G from length-D float64 dot products, carries an
  absolute error of (D + 6) u (|x_i|^2 + |x_j|^2 + 2 |x_i| |x_j|) at most (three dot products of gamma_D, two additions, the
  centring rounding of each operand), i.e. a relative error of d of eps_ij = (D + 6) u (|x_i| + |x_j|)^2 / (2 d_ij^2);
  eps = max over pairs.  A class mean of distances then carries eps + n u (an ascending sum of at most n terms), a and b one
  division more, and s = (b - a) / max(a, b) moves by at most 2 (relative error of a + that of b) <= 4 (eps + n u).
* Calinski-Harabasz and Davies-Bouldin come from sums of Gram entries of relative size (D + n) u (a dot product, then at most n
  additions per level).  The within-cluster dispersion is a difference of two such sums of size sum G_ii, so its relative error
  is amplified by kappa = sum G_ii / within; squared centroid distances and squared own-centroid distances are differences of
  terms of the size of the class's mean |x|^2, amplified by that size over the smallest of them.  8 (D + n) u kappa covers the
  quotient of two such quantities with the constant of the three-term expressions.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ cases
def make_case(n, D, k, seed, dtype=np.float64, counts=None, names=None, spread=1.0):
    """Gaussian class means (std `spread`) plus unit noise; labels cover every class (`counts`: explicit class sizes)."""
    rng = np.random.default_rng(seed)
    if counts is None:
        codes = np.arange(n) % k
    else:
        assert sum(counts) == n and len(counts) == k
        codes = np.repeat(np.arange(k), counts)
    codes = rng.permutation(codes)
    X = (spread * rng.standard_normal((k, D))[codes] + rng.standard_normal((n, D))).astype(dtype)
    labels = codes if names is None else np.asarray(names)[codes]
    return X, labels


# name -> (X, labels): the cases of tests/test_gpu_cluster_scores.py
def cases():
    return {
        'n130_D100_k9': make_case(130, 100, 9, 11),
        'n65_D17_k3_f32': make_case(65, 17, 3, 12, np.float32),
        'n64_D6000_k9_f32': make_case(64, 6000, 9, 13, np.float32, spread=0.25),
        'n12_D5_k4_singleton': make_case(12, 5, 4, 14, counts=[1, 3, 4, 4], spread=2.0),
        'n40_D8_k5_strings': make_case(40, 8, 5, 15, names=['ba', 'da', 'ga', 'pa', 'ta'], spread=1.5),
    }


def shuffles(labels, R, seed):
    """R permutations of `labels` as cluster_scores draws them from RandomState(seed)."""
    rng = np.random.RandomState(seed)
    return [rng.permutation(labels) for _ in range(R)]


# ------------------------------------------------------------------------------------------------ the restatement
def sq_dists(X):
    """(n, n) long-double matrix of sum_d (x_i - x_j)^2 from direct differences, row by row."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1).astype(LD)
    out = np.zeros((len(X), len(X)), dtype=LD)
    for i in range(len(X)):
        diff = X - X[i]
        out[i] = (diff * diff).sum(axis=1)
    return out


def codes_of(labels):
    uniq, codes = np.unique(labels, return_inverse=True)
    return np.asarray(codes).reshape(-1), len(uniq)


def grouped_row_sums(F, codes, k):
    """S[i][q] = sum over j with codes[j] == q of F[i][j], in F's dtype (long double for the references)."""
    return np.stack([F[:, codes == q].sum(axis=1) for q in range(k)], axis=1)


def silhouette_samples(X, labels, d2=None):
    """sklearn's rules in long double.  d2: sq_dists(X) if already known."""
    codes, k = codes_of(labels)
    d = np.sqrt(sq_dists(X) if d2 is None else d2)
    n = len(codes)
    cnt = np.bincount(codes, minlength=k)
    S = grouped_row_sums(d, codes, k)
    s = np.zeros(n, dtype=LD)
    for i in range(n):
        y = codes[i]
        if cnt[y] == 1:
            continue
        a = S[i, y] / (cnt[y] - 1)
        b = min(S[i, q] / cnt[q] for q in range(k) if q != y and cnt[q] > 0)
        big = max(a, b)
        s[i] = (b - a) / big if big > 0 else 0
    return s


def positive_mean(s):
    pos = s[s > 0]
    return pos.sum() / len(pos) if len(pos) else LD('nan')


def _centroids(X, codes, k):
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1).astype(LD)
    cen = np.stack([X[codes == q].sum(axis=0) / (codes == q).sum() for q in range(k)])
    return X, cen


def calinski_harabasz(X, labels):
    codes, k = codes_of(labels)
    X, cen = _centroids(X, codes, k)
    n = len(X)
    mean = X.sum(axis=0) / n
    cnt = np.bincount(codes, minlength=k)
    extra = sum(cnt[q] * ((cen[q] - mean) ** 2).sum() for q in range(k))
    intra = sum(((X[codes == q] - cen[q]) ** 2).sum() for q in range(k))
    return LD(1.0) if intra == 0 else extra * (n - k) / (intra * (k - 1))


def davies_bouldin(X, labels):
    codes, k = codes_of(labels)
    X, cen = _centroids(X, codes, k)
    intra = np.array([np.sqrt(((X[codes == q] - cen[q]) ** 2).sum(axis=1)).sum() / (codes == q).sum() for q in range(k)], dtype=LD)
    cd = np.sqrt(((cen[:, None, :] - cen[None, :, :]) ** 2).sum(axis=2))
    if np.allclose(intra.astype(np.float64), 0) or np.allclose(cd.astype(np.float64), 0):
        return LD(0.0)
    cd[cd == 0] = np.inf
    scores = ((intra[:, None] + intra[None, :]) / cd).max(axis=1)
    return scores.sum() / k


# ------------------------------------------------------------------------------------------------ conditioning and the bars
def centred(X):
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    return X - X.mean(axis=0)


def conditioning(X, d2=None):
    """min_{i != j} d^2_ij / max_i |x_i|^2 of the centred data: the GPU cases demand >= 1e-3."""
    Xc = centred(X)
    d2 = np.asarray(sq_dists(X) if d2 is None else d2, dtype=np.float64)
    off = d2[~np.eye(len(Xc), dtype=bool)]
    return float(off.min() / (Xc * Xc).sum(axis=1).max())


def silhouette_bar(X, d2=None, centre=True):
    """4 (eps + n u), eps the largest relative error of a distance taken through the Gram matrix of X (centred first unless
    ``centre`` is False: sklearn works on the data as given)."""
    Xc = centred(X) if centre else np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    n, D = Xc.shape
    nrm = np.sqrt((Xc * Xc).sum(axis=1))
    d2 = np.asarray(sq_dists(X) if d2 is None else d2, dtype=np.float64)
    off = ~np.eye(n, dtype=bool)
    eps = ((D + 6) * U * (nrm[:, None] + nrm[None, :]) ** 2 / (2.0 * np.where(off, d2, 1.0)))[off].max()
    return 4.0 * (eps + n * U)


def dispersion_bars(X, labels, centre=True):
    """(bar of Calinski-Harabasz, bar of Davies-Bouldin), both relative: 8 (D + n) u kappa.  kappa = sum |x_i|^2 / within-cluster
    dispersion; Davies-Bouldin also takes the largest class mean of |x|^2 over the smallest squared centroid distance and over
    the smallest squared own-centroid mean (classes of one sample have an own-centroid distance of exactly 0 on every route and
    are left out of that minimum)."""
    Xc = centred(X) if centre else np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    n, D = Xc.shape
    codes, k = codes_of(labels)
    cnt = np.bincount(codes, minlength=k)
    cen = np.stack([Xc[codes == q].mean(axis=0) for q in range(k)])
    own2 = ((Xc - cen[codes]) ** 2).sum(axis=1)
    x2 = (Xc * Xc).sum(axis=1)
    kappa = x2.sum() / own2.sum()
    m2 = max(x2[codes == q].mean() for q in range(k))
    cd2 = ((cen[:, None, :] - cen[None, :, :]) ** 2).sum(axis=2)[~np.eye(k, dtype=bool)].min()
    intra = np.array([np.sqrt(own2[codes == q]).mean() for q in range(k)])
    kappa_db = max(kappa, m2 / cd2, m2 / (intra[cnt > 1] ** 2).min())
    return 8.0 * (D + n) * U * kappa, 8.0 * (D + n) * U * kappa_db


def sklearn_singleton_slack(X, labels):
    """Absolute error sklearn's own davies_bouldin_score may carry when a class has ONE sample: it takes the distance of that
    sample to itself as sqrt(max(|x|^2 - 2 x.x + |x|^2, 0)), and the rounding of up to (D + 2) u 4 |x|^2 under the root leaves
    delta = 2 |x| sqrt((D + 2) u) where the exact value is 0; every ratio (intra_p + intra_q) / cd_pq then moves by at most
    delta / min cd, and so does their mean.  0 without such a class (the restatement and the device route give exactly 0 there)."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    codes, k = codes_of(labels)
    cnt = np.bincount(codes, minlength=k)
    if not (cnt == 1).any():
        return 0.0
    cen = np.stack([X[codes == q].mean(axis=0) for q in range(k)])
    cd = np.sqrt(((cen[:, None, :] - cen[None, :, :]) ** 2).sum(axis=2))[~np.eye(k, dtype=bool)].min()
    x = max(np.sqrt((X[codes == q] ** 2).sum()) for q in range(k) if cnt[q] == 1)
    return 2.0 * x * np.sqrt((X.shape[1] + 2) * U) / cd


# ------------------------------------------------------------------------------------------------ the Gram route in numpy
def gram_tables(X, label_sets, k):
    """What the device pass downloads, made with numpy float64 on the host (any summation order): (counts, M, dg, intra_sum) for
    the label sets given as code vectors.  The host test feeds them to alignment.metrics._ch_db."""
    Xc = centred(X)
    G = Xc @ Xc.T
    dg_all = np.diag(G)
    counts, M, dg, intra = [], [], [], []
    for codes in label_sets:
        cnt = np.bincount(codes, minlength=k)
        S0 = grouped_row_sums(G, codes, k)
        Mr = np.stack([S0[codes == p].sum(axis=0) if cnt[p] else np.zeros(k) for p in range(k)])
        safe = np.where(cnt > 0, cnt, 1)
        dist = np.sqrt(np.maximum(dg_all - 2 * S0[np.arange(len(codes)), codes] / safe[codes] + np.diag(Mr)[codes] / safe[codes] ** 2, 0))
        counts.append(cnt)
        M.append(Mr)
        dg.append(np.bincount(codes, weights=dg_all, minlength=k))
        intra.append(np.bincount(codes, weights=dist, minlength=k))
    return np.stack(counts).astype(np.int32), np.stack(M), np.stack(dg), np.stack(intra)


def gram_silhouettes(X, codes, k):
    """Silhouettes through the Gram matrix in numpy float64: the device route's arithmetic in another summation order."""
    Xc = centred(X)
    G = Xc @ Xc.T
    g = np.diag(G)
    d = np.sqrt(np.maximum((g[:, None] + g[None, :]) - 2.0 * G, 0.0))
    np.fill_diagonal(d, 0.0)
    cnt = np.bincount(codes, minlength=k)
    S = grouped_row_sums(d, codes, k)
    n = len(codes)
    s = np.zeros(n)
    for i in range(n):
        y = codes[i]
        if cnt[y] > 1:
            a = S[i, y] / (cnt[y] - 1)
            b = min(S[i, q] / cnt[q] for q in range(k) if q != y and cnt[q] > 0)
            s[i] = (b - a) / max(a, b) if max(a, b) > 0 else 0.0
    return s
