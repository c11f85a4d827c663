"""Restatement of the representational dissimilarity analysis in np.longdouble, for tests/test_gpu_rsa_kernels.py and
tests/test_gpu_rsa.py (tests/test_rsa_ref_host.py checks the restatement itself against scipy and the golden fixture on the CPU).

The condition averages are numpy's own ``np.mean(data[labels == c], axis=0)`` in the data's dtype, widened (the reference's
``cnd_avg``; the device route reproduces those sums).  From there everything is long double: per-row Pearson correlation as
scipy.stats.pearsonr takes it -- deviations from the mean, divided by their norm, dotted --, the RDM 1 - clip(r) with a zero
diagonal, the comparison of two RDMs over the upper triangles (np.triu_indices order, k = 1) of the shared conditions, and the
permuted comparison through ``B[np.ix_(ib[p], ib[p])]``.  Also here: the fixed-seed cases of the GPU tests and the error bars
they hold the device route to.  With u = 2^-53:

* r_ij of two rows of length D.  The device standardises z = d / |d| with d = x - mean, then takes the float64 dot product
  z_i . z_j on the f64 MFMA.  First-order terms, relative to |z_i| |z_j| = 1: the dot product of D terms, D u; each |d|^2 is a
  sum of D squares in some fixed order, at most (D + 2) u, halved by the root, for both rows (D + 2) u; the roundings of
  x - mean, of the division and of the root, 3 u per row.  That is (2 D + 8) u.  The rounded mean shifts every deviation of a
  row by the same s_i, |s_i| <= u |mean| + (a second-pass remainder far below it) <= u |x_i| / sqrt(D); a common shift moves z_i
  by s_i sqrt(D) / |d_i| <= u kappa_i along the constant direction, to which z_j is orthogonal but for its own shift of
  u kappa_j: the effect on r is u^2 D-free and of second order, but each shift also perturbs what the first-order terms act
  on by the factor (1 + u kappa).  So 4 (D + 6) u kappa_i kappa_j >= (2 D + 8) u (1 + u kappa_i)(1 + u kappa_j) + u^2 kappa_i
  kappa_j covers it with kappa = |x| / |x - mean| >= 1; an input average that is off by one rounding (a mean taken as a
  quotient or as a product with 1 / n) adds 2 u kappa_i kappa_j at most and is inside the same bar.  The long-double
  restatement's own rounding is 2^-11 of all that.  scipy.stats.pearsonr works in float64 with the same operations (its sums
  are numpy's pairwise ones), so it carries a bar of the same form and may differ from the device by the sum of the two.
* The comparison of two triangles of length L = m (m - 1) / 2: the same count with L for D -- the cross sum L u, the two sums
  of squares (L + 2) u together after the roots, the deviations, the root and the host's quotient 6 u -- is (2 L + 8) u; the
  single-pass triangle mean is off by at most L u mean|x| <= sqrt(L) u |x|, a common shift again, entering at second order
  (L^2 u^2 kappa_x kappa_y, below 1e-20 for every m up to 1024) because the device uses one mean in the statistics and in the
  cross products.  4 (L + 8) u kappa_x kappa_y covers it; the cosine method has no mean: kappa = 1.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


# ------------------------------------------------------------------------------------------------ condition averages
def label_strings(labels):
    """The reference's label2str: 1-D labels as str, 2-D label sequences as the joined digits of a row."""
    labels = np.asarray(labels)
    if labels.ndim > 1:
        return np.array([''.join(str(v) for v in row) for row in labels])
    return labels.astype(str)


def cnd_means(data, labels):
    """(condition averages (n_c, D) float64, unique label strings): np.mean over the trials of a condition in the data's dtype."""
    data = np.asarray(data)
    X = data.reshape(len(data), -1)
    keys = label_strings(labels)
    uniq = np.unique(keys)
    ca = np.zeros((len(uniq), X.shape[1]))
    for i, c in enumerate(uniq):
        ca[i] = np.mean(X[keys == c], axis=0)
    return ca, uniq


# ------------------------------------------------------------------------------------------------ RDM
def pearson_rows(CA):
    """(n_c, n_c) long-double Pearson correlations of the rows of CA; NaN in the row and column of a constant row."""
    X = np.asarray(CA).astype(LD)
    d = X - X.mean(axis=1, keepdims=True)
    norm = np.sqrt((d * d).sum(axis=1, keepdims=True))
    const = (np.asarray(CA) == np.asarray(CA)[:, :1]).all(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        z = d / norm
    z[const] = np.nan
    return z @ z.T


def rdm_ref(CA):
    """1 - clip(r, -1, 1) in long double with the diagonal 0 where it is not NaN."""
    r = pearson_rows(CA)
    out = 1 - np.where(np.isnan(r), r, np.clip(r, -1, 1))
    i = np.arange(len(out))
    out[i, i] = np.where(np.isnan(out[i, i]), np.nan, 0)
    return out


def kappa(X):
    """|x| / |x - mean| of every row (long double); inf for a constant row."""
    X = np.atleast_2d(np.asarray(X)).astype(LD)
    d = X - X.mean(axis=1, keepdims=True)
    with np.errstate(divide='ignore'):
        return np.sqrt((X * X).sum(axis=1)) / np.sqrt((d * d).sum(axis=1))


def corr_bar(CA):
    """(n_c, n_c) bars 4 (D + 6) u kappa_i kappa_j on every r_ij (and so on every RDM entry)."""
    k = kappa(CA).astype(np.float64)
    return 4.0 * (np.shape(CA)[1] + 6) * U * k[:, None] * k[None, :]


# ------------------------------------------------------------------------------------------------ comparison
def triangle(M, idx):
    """The upper triangle k = 1, in np.triu_indices order, of M restricted to the rows and columns idx."""
    idx = np.asarray(idx)
    return np.asarray(M)[np.ix_(idx, idx)][np.triu_indices(len(idx), k=1)]


def similarity(x, y, method='pearson'):
    """Long-double Pearson correlation (cosine: no centring) of two vectors, clipped; NaN for a zero norm."""
    x, y = np.asarray(x).astype(LD), np.asarray(y).astype(LD)
    if method == 'pearson':
        x, y = x - x.mean(), y - y.mean()
    with np.errstate(divide='ignore', invalid='ignore'):
        r = (x * y).sum() / (np.sqrt((x * x).sum()) * np.sqrt((y * y).sum()))
    return r if np.isnan(r) else np.clip(r, -1, 1)


def compare_ref(A, ia, B, ib, p=None, method='pearson'):
    """The comparison of A over ia with B over ib[p] (p: a permutation of the shared conditions; None: the identity)."""
    ib = np.asarray(ib) if p is None else np.asarray(ib)[np.asarray(p)]
    return similarity(triangle(A, ia), triangle(B, ib), method)


def compare_bar(x, y, method='pearson'):
    """4 (L + 8) u kappa_x kappa_y for two triangles of length L; kappa = 1 for the cosine method."""
    kx, ky = (1.0, 1.0) if method == 'cosine' else (float(kappa(x)[0]), float(kappa(y)[0]))
    return 4.0 * (len(x) + 8) * U * kx * ky


def shared_indices(labels_a, labels_b):
    """(shared labels, indices in labels_a, indices in labels_b): np.intersect1d and the notebooks' label_to_index lookup."""
    shared = np.intersect1d(labels_a, labels_b)
    la, lb = {v: i for i, v in enumerate(labels_a)}, {v: i for i, v in enumerate(labels_b)}
    return shared, np.array([la[s] for s in shared]), np.array([lb[s] for s in shared])


def permutation_tables(ms, R, rng):
    """The draws of compare_rdms_many restated: ascending distinct m, R times rng.permutation(m) each, row 0 the identity."""
    return {m: np.stack([np.arange(m)] + [rng.permutation(m) for _ in range(R)]) for m in sorted(set(int(m) for m in ms))}


# ------------------------------------------------------------------------------------------------ cases
def make_patient(n, T, d, conditions, seed, dtype=np.float64, sequences=False):
    """A latent space (n, T, d) of the form normal + 3 with a condition structure, and its labels: integers drawn from
    `conditions` (every one present), or two-digit label sequences (n, 2) when `sequences`."""
    rng = np.random.default_rng(seed)
    conditions = np.asarray(conditions)
    codes = rng.permutation(np.arange(n) % len(conditions))
    means = rng.standard_normal((len(conditions), T, d))
    X = (means[codes] + rng.standard_normal((n, T, d)) + 3.0).astype(dtype)
    labels = conditions[codes]
    if sequences:
        labels = np.stack([labels // 10, labels % 10], axis=1)
    return X, labels


def cases():
    """name -> (data, labels).  The patients share most but not all conditions; one has float32 data, one label sequences."""
    return {
        'a_n130_T5_d4_k9': make_patient(130, 5, 4, np.arange(1, 10), 11),
        'b_n65_T5_d4_k7_f32': make_patient(65, 5, 4, np.array([1, 2, 3, 5, 6, 8, 9]), 12, dtype=np.float32),
        'c_n97_T3_d7_k9': make_patient(97, 3, 7, np.arange(3, 12), 13),
        'd_n40_T2_d3_seq': make_patient(40, 2, 3, np.array([12, 13, 21, 23, 31, 32]), 14, sequences=True),
        'e_n48_T2_d3_seq_f32': make_patient(48, 2, 3, np.array([12, 13, 21, 23, 32, 33]), 15, dtype=np.float32, sequences=True),
    }
