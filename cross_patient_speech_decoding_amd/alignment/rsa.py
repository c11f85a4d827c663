"""Representational dissimilarity analysis on the MI355X: the reference's figure notebooks' ``calc_rdm_corr``, ``compare_rdms``,
``subset_rdm`` and ``cos_sim`` (``figure_analyses/fig_2.ipynb``, ``fig_6.ipynb``) behind their own names, and the batched forms
that make a Mantel permutation null over a whole sweep affordable.

An RDM is ``1 - r`` between the condition averages of a latent space.  On the device the averages are standardised row by row
(``(x - mean) / |x - mean|``: ``scipy.stats.pearsonr``'s arithmetic) and ONE ragged Gram launch yields every ``r_ij`` of every data
set.  Two RDMs are compared by the Pearson correlation (or the cosine) of their upper triangles over the shared conditions; a
Mantel null relabels the conditions of the second matrix.  All comparisons of a chunk, with all their permutations, are one
library call; only the four statistics of a pair and its R + 1 cross products come down, and the quotient is taken on the host.
Everything is float64 (float32 input is widened after its condition averages, which keep ``np.mean``'s dtype semantics) and
deterministic: a pair gives the same bits alone, among other pairs and in any chunking.  There is no CPU fallback; argument
errors are raised before the device is looked for and before any permutation is drawn.
"""
import numpy as np
import torch

from . import _linalg as LA
from .alignment_utils import label2str
from .metrics import _generator, _label_vector, permutation_p_value

MAX_CONDITIONS = LA.RSA_MAX_CONDITIONS
METHODS = ('pearson', 'cosine')
_TOO_SHORT = '`x` and `y` must have length at least 2.'          # scipy.stats.pearsonr's refusal, word for word


# ------------------------------------------------------------------------------------------------ host helpers (the notebooks')
def subset_rdm(rdm, labels, shared_labels):
    """The rows and columns of ``rdm`` (whose conditions are ``labels``) that belong to ``shared_labels``, in their order.  A shared
    label that ``labels`` does not hold is dropped, as in the notebooks.  Host indexing."""
    keep = _positions(labels, shared_labels)
    return np.asarray(rdm)[keep[:, None], keep[None, :]]


def cos_sim(a, b):
    """The cosine of the angle between two vectors: their dot product over the product of their euclidean lengths."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return (a @ b) / (np.sqrt(a @ a) * np.sqrt(b @ b))


def _positions(labels, wanted):
    """int32 positions in ``labels`` of every label of ``wanted`` that ``labels`` holds, in ``wanted``'s order (a label that
    occurs twice counts at its last position); the others are left out."""
    where = dict(zip(list(labels), range(len(labels))))
    return np.array([where[w] for w in wanted if w in where], dtype=np.int32)


def _shared_indices(labels_a, labels_b):
    """(shared labels, their positions in labels_a, in labels_b): np.intersect1d, then the lookup of subset_rdm."""
    shared = np.intersect1d(labels_a, labels_b)
    return shared, _positions(labels_a, shared), _positions(labels_b, shared)


def permutation_tables(ms, n_permutations, random_state=None):
    """{m: (n_permutations + 1, m) int32 table} for the distinct numbers of shared conditions in ``ms``: row 0 the identity, then
    ``rng.permutation(m)`` drawn in order, table by table in ascending m.  All pairs of one m share their table."""
    rng = _generator(random_state)
    tables = {}
    for m in sorted({int(m) for m in ms}):
        rows = [np.arange(m)] + [rng.permutation(m) for _ in range(int(n_permutations))]
        tables[m] = np.ascontiguousarray(np.stack(rows), dtype=np.int32)
    return tables


def _similarity(cross, sxx, syy):
    """cross / (sqrt(sxx) sqrt(syy)) clipped to [-1, 1], NaN kept: elementwise float64 on the host."""
    with np.errstate(divide='ignore', invalid='ignore'):
        r = cross / (np.sqrt(sxx) * np.sqrt(syy))
    return np.where(np.isnan(r), np.nan, np.clip(r, -1.0, 1.0))


def pairs_per_chunk(n_permutations, max_bytes):
    """Pairs whose (R + 1) cross products and four statistics fit max_bytes; at least one."""
    return int(max(1, int(max_bytes) // (8 * (int(n_permutations) + 5))))


# ------------------------------------------------------------------------------------------------ arguments (no device)
def _data_shape(data, what):
    shape = tuple(data.shape) if hasattr(data, 'shape') else np.shape(data)
    if len(shape) not in (2, 3) or shape[0] < 1:
        raise ValueError(f'{what}: data must be (n_trials, T, d) or (n_trials, D)')
    D = int(np.prod(shape[1:]))
    if D < 2:
        raise ValueError(_TOO_SHORT)
    return int(shape[0]), D


def _check_count(value, name, what, least=0):
    if not (isinstance(value, (int, np.integer)) and value >= least):
        raise ValueError(f'{what}: {name} must be an integer >= {least}; got {value!r}')
    return int(value)


def _check_method(method, what):
    if method not in METHODS:
        raise ValueError(f"{what}: method must be 'pearson' or 'cosine'; got {method!r}")
    return method == 'cosine'


def _rdm_arguments(datas, labels_list, what):
    """[(n, D, label strings)] of every data set; every refusal of calc_rdm_corr_many."""
    datas, labels_list = list(datas), list(labels_list)
    if len(datas) != len(labels_list):
        raise ValueError(f'{what}: {len(datas)} data sets and {len(labels_list)} label vectors')
    out = []
    for data, labels in zip(datas, labels_list):
        n, D = _data_shape(data, what)
        out.append((n, D, label2str(_label_vector(labels, n, what))))    # strings: '10' sorts before '2', as in the reference
    return datas, out


# ------------------------------------------------------------------------------------------------ RDMs
def _rdms_device(datas, described):
    """[(rdm device tensor (n_c, n_c), unique labels)] of every data set: the condition averages (one launch for all float64 data
    sets, one per float32 data set), ONE standardise launch, ONE Gram launch, ONE 1 - r launch."""
    dev = LA.device()
    index = [LA.condition_index(keys) for _, _, keys in described]
    avgs, segments = [], []
    for data, (n, D, _), (uniq, order, start) in zip(datas, described, index):
        Xd = LA.to_device(data).reshape(n, D)
        if Xd.dtype == torch.float32:                                    # np.mean's float32 sums, stored as float64
            avgs.append(LA.cnd_avg_device(Xd, order, start))
            continue
        ca = torch.empty(len(uniq), D, dtype=LA.F64, device=dev)
        segments += [(Xd, ca[c], order[start[c]:start[c + 1]]) for c in range(len(uniq))]
        avgs.append(ca)
    LA.cnd_avg_folds(segments)
    Z = [torch.empty_like(ca) for ca in avgs]
    G = [torch.empty(len(ca), len(ca), dtype=LA.F64, device=dev) for ca in avgs]
    keep = [LA.row_standardize_grouped(list(zip(avgs, Z))), LA.gram_grouped(list(zip(Z, G))),
            LA.rdm_from_corr_grouped([(g, g) for g in G])]
    return [(g, uniq) for g, (uniq, _, _) in zip(G, index)], keep


def _download(tensors):
    """The tensors as float64 ndarrays through ONE download (which also synchronises with the stream)."""
    if not tensors:
        return []
    host = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy()
    cuts = np.cumsum([0] + [t.numel() for t in tensors])
    return [host[cuts[i]:cuts[i + 1]].reshape(tuple(t.shape)) for i, t in enumerate(tensors)]


def calc_rdm_corr_many(datas, labels_list):
    """``calc_rdm_corr`` of every (data, labels) of the two lists as ONE device problem: data sets of different n_trials, numbers of
    conditions and D.  -> list of (rdm, unique_labels), bit for bit what ``calc_rdm_corr`` gives for each alone."""
    datas, described = _rdm_arguments(datas, labels_list, 'calc_rdm_corr_many')
    if not datas:
        return []
    rdms, keep = _rdms_device(datas, described)
    host = _download([g for g, _ in rdms])
    return [(h, uniq) for h, (_, uniq) in zip(host, rdms)]


def calc_rdm_corr(data, labels):
    """The notebooks' ``calc_rdm_corr``: ``rdm[i][j] = 1 - pearsonr(ca[i], ca[j])`` between the condition averages ``ca`` of
    ``data`` ((n_trials, T, d) or (n_trials, D), numpy or torch) under ``labels`` (1-D, or 2-D label sequences read through
    ``label2str``).  -> (rdm float64 ndarray (n_c, n_c), unique_labels = np.unique of the label strings: the row order).

    The diagonal is exactly 0.0; the notebooks' is ``1 - pearsonr(x, x)``, which is 0 or a few ulps of 1 (up to 3 2^-53 in the golden
    fixture).  A condition whose average
    is constant gives NaN in its row and column (diagonal included), as scipy does.  ``D = T d < 2`` raises scipy's ValueError."""
    return calc_rdm_corr_many([data], [labels])[0]


# ------------------------------------------------------------------------------------------------ comparisons
class RDMComparison:
    """Comparisons of pairs of RDMs.  similarity_ (n_pairs,): the Pearson correlation (or cosine) of the two upper triangles over
    the shared conditions; null_ (n_pairs, R): the same with the conditions of the second matrix relabelled by permutation r;
    p_value_ (n_pairs,): (1 + #{null >= similarity}) / (1 + R); n_shared_ (n_pairs,); shared_labels_: per pair; n_permutations."""

    def __init__(self, values, n_shared, shared_labels, n_permutations):
        self.n_permutations = int(n_permutations)
        self.similarity_ = np.ascontiguousarray(values[:, 0])
        self.null_ = np.ascontiguousarray(values[:, 1:])
        self.p_value_ = np.array([permutation_p_value(v, self.n_permutations) for v in values], dtype=np.float64)
        self.n_shared_ = n_shared
        self.shared_labels_ = shared_labels


def _matrix_size(rdm, labels, what):
    shape = tuple(rdm.shape) if hasattr(rdm, 'shape') else np.shape(rdm)
    if len(shape) != 2 or shape[0] != shape[1] or shape[0] < 1:
        raise ValueError(f'{what}: an RDM must be a square matrix; got shape {shape}')
    if np.ndim(labels) != 1 or len(labels) != shape[0]:
        raise ValueError(f'{what}: an RDM of {shape[0]} conditions needs {shape[0]} labels')
    return int(shape[0])


def _rdm_to_device(rdm):
    t = LA.to_device(rdm).to(LA.F64)
    return t if t.stride(-1) == 1 else t.contiguous()


def compare_rdms_many(rdms, labels, pairs, method='pearson', n_permutations=0, random_state=None, max_bytes=2 ** 28):
    """``compare_rdms(rdms[a], labels[a], rdms[b], labels[b])`` for every (a, b) of ``pairs`` with a Mantel null of
    ``n_permutations`` relabellings each, as ONE device problem per chunk of pairs (``max_bytes`` over the R + 5 doubles a pair brings
    down: its R + 1 cross products and four statistics).  rdms: device or host matrices.  Permutation r relabels the shared
    conditions of the SECOND matrix: ``y = B[ib[p[u]]][ib[p[v]]]``.  With ``n_permutations > 0`` a second matrix must be symmetric
    bit for bit, as ``calc_rdm_corr`` makes it: the mean and the sum of squares of its triangle are taken once, for the identity,
    and belong to a relabelled triangle only then.  A host matrix that is not is refused (matrices made by scipy loops differ
    from their transposes in the last bits: pass ``(M + M.T) / 2``); a device matrix is the caller's to keep symmetric, and an
    asymmetric one gets null values normalised by the identity's statistics.  The permutations are drawn on the host, one table of R per distinct number
    m of shared conditions in ascending m, each by ``rng.permutation(m)`` in order; pairs of equal m share their table
    (``random_state=None`` draws from numpy's global generator).  -> RDMComparison."""
    what = 'compare_rdms_many'
    cosine = _check_method(method, what)
    R = _check_count(n_permutations, 'n_permutations', what)
    _check_count(max_bytes, 'max_bytes', what, least=1)
    rdms, labels, pairs = list(rdms), [np.asarray(v) for v in labels], [tuple(p) for p in pairs]
    if len(rdms) != len(labels):
        raise ValueError(f'{what}: {len(rdms)} RDMs and {len(labels)} label vectors')
    for rdm, v in zip(rdms, labels):
        _matrix_size(rdm, v, what)
    lists = []
    for p in pairs:
        if len(p) != 2 or not all(isinstance(i, (int, np.integer)) and 0 <= i < len(rdms) for i in p):
            raise ValueError(f'{what}: a pair must be two indices into rdms; got {p!r}')
        shared, ia, ib = _shared_indices(labels[p[0]], labels[p[1]])
        if len(shared) < 3:                                               # fewer than 2 triangle entries
            raise ValueError(_TOO_SHORT)
        if len(shared) > MAX_CONDITIONS:
            raise ValueError(f'{what}: {len(shared)} shared conditions; at most XPS_RSA_MAX_CONDITIONS = {MAX_CONDITIONS} are supported')
        lists.append((shared, ia, ib))
    if R > 0:                                                             # the null takes mean_y and syy once, from the identity
        for b in sorted({p[1] for p in pairs}):
            M = rdms[b]
            if not isinstance(M, torch.Tensor) or not M.is_cuda:
                M = np.asarray(M.detach().numpy() if isinstance(M, torch.Tensor) else M)
                if not np.array_equal(M, M.T, equal_nan=M.dtype.kind == 'f'):
                    raise ValueError(f'{what}: rdms[{b}] is not symmetric bit for bit, which a permutation null of the second '
                                     'matrix needs (a relabelling then keeps the mean and the spread of its triangle); '
                                     'pass (M + M.T) / 2')
    rng = _generator(random_state)                                       # every refusal before the first draw and the device
    tables = permutation_tables([len(s) for s, _, _ in lists], R, rng)

    values = np.empty((len(pairs), R + 1))
    if pairs:
        LA.device()
        on_device = {i: _rdm_to_device(rdms[i]) for i in sorted({i for p in pairs for i in p})}
        step = pairs_per_chunk(R, max_bytes)
        for q0 in range(0, len(pairs), step):
            chunk = range(q0, min(len(pairs), q0 + step))
            ms = sorted({len(lists[q][0]) for q in chunk})
            offs = np.cumsum([0] + [tables[m].size for m in ms])
            desc = np.array([[offs[t], m] for t, m in enumerate(ms)], dtype=np.int64)
            perms = np.concatenate([tables[m].reshape(-1) for m in ms])
            idx = np.concatenate([v for q in chunk for v in lists[q][1:]])
            entries, pos = [], 0
            for q in chunk:
                m = len(lists[q][0])
                entries.append((on_device[pairs[q][0]], pos, on_device[pairs[q][1]], pos + m, m, ms.index(m)))
                pos += 2 * m
            stats_d, cross_d, keep = LA.rdm_compare_perm(entries, idx, desc, perms, R, cosine)
            stats, cross = _download([stats_d, cross_d])
            values[chunk.start:chunk.stop] = _similarity(cross, stats[:, 2:3], stats[:, 3:4])
    return RDMComparison(values, np.array([len(s) for s, _, _ in lists], dtype=np.int64), [s for s, _, _ in lists], R)


def compare_rdms(rdm1, labels1, rdm2, labels2, method='pearson'):
    """The notebooks' ``compare_rdms``: the Pearson correlation of the upper triangles (``k = 1``, ``np.triu_indices`` order) of
    the two RDMs over their shared labels (``np.intersect1d``).  ``method='cosine'``: the notebooks' commented-out ``cos_sim``
    variant.  Fewer than 3 shared conditions leave fewer than 2 triangle entries and raise scipy's ValueError.  -> float."""
    return float(compare_rdms_many([rdm1, rdm2], [labels1, labels2], [(0, 1)], method=method).similarity_[0])


class RDMAlignment:
    """``rdm_alignment_scores``'s result.  rdm_target_, labels_target_: the target's RDM and its conditions; rdms_, labels_: one per
    other patient; comparison_: the RDMComparison of each with the target (pair i = target against other i); similarity_,
    p_value_: its fields; mean_similarity_: the notebooks' ``np.mean`` over the other patients."""

    def __init__(self, target, others, comparison):
        self.rdm_target_, self.labels_target_ = target
        self.rdms_ = [r for r, _ in others]
        self.labels_ = [u for _, u in others]
        self.comparison_ = comparison
        self.similarity_ = comparison.similarity_
        self.p_value_ = comparison.p_value_
        self.mean_similarity_ = float(np.mean(comparison.similarity_)) if len(others) else float('nan')


def rdm_alignment_scores(target, target_labels, others, others_labels, method='pearson', n_permutations=0, random_state=None,
                         max_bytes=2 ** 28):
    """The notebooks' inner block: the RDM of the target patient's latent space, the RDM of every other (aligned) patient's, and
    the comparison of each with the target's -- ``calc_rdm_corr_many`` and ``compare_rdms_many`` on RDMs that stay on the device
    in between.  -> RDMAlignment."""
    what = 'rdm_alignment_scores'
    _check_method(method, what)
    R = _check_count(n_permutations, 'n_permutations', what)
    _check_count(max_bytes, 'max_bytes', what, least=1)
    _generator(random_state)
    datas, described = _rdm_arguments([target] + list(others), [target_labels] + list(others_labels), what)
    conditions = [np.unique(keys) for _, _, keys in described]
    for other in conditions[1:]:                                          # compare_rdms_many's refusals, before the device
        m = len(np.intersect1d(conditions[0], other))
        if m < 3:
            raise ValueError(_TOO_SHORT)
        if m > MAX_CONDITIONS:
            raise ValueError(f'{what}: {m} shared conditions; at most XPS_RSA_MAX_CONDITIONS = {MAX_CONDITIONS} are supported')
    rdms, keep = _rdms_device(datas, described)
    cmp_ = compare_rdms_many([g for g, _ in rdms], [u for _, u in rdms], [(0, i) for i in range(1, len(rdms))], method=method,
                             n_permutations=R, random_state=random_state, max_bytes=max_bytes)
    host = _download([g for g, _ in rdms])
    both = [(h, u) for h, (_, u) in zip(host, rdms)]
    return RDMAlignment(both[0], both[1:], cmp_)
