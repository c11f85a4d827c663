"""What ``SVC`` (svm.py), ``BaggingClassifier`` (bagging.py) and ``SVCSearchCV`` (search.py) share, each rule once: the settings a
fit resolves from its data, the one-vs-one problems of one fit and their bounds, the single int32 upload, the kernel matrix, the
batched SMO launch and the signed coefficient matrix.  The three agree bit for bit on what a problem is because they pose it here."""
import numpy as np
import torch

from .._dev import stream
from .._lib import call, lib
from ..alignment import _linalg as LA


# ------------------------------------------------------------------------------------------------ settings (host)
def gamma_value(kernel, gamma, X):
    """sklearn's ``gamma`` of an rbf SVC fitted on X (0.0 for every other kernel)."""
    if kernel != 'rbf':
        return 0.0
    if isinstance(gamma, str):
        if gamma == 'scale':                                # sklearn: 1 / (n_features * X.var()) of the X handed to fit
            var = float(X.var())
            return 1.0 / (X.shape[1] * var) if var != 0 else 1.0
        if gamma == 'auto':
            return 1.0 / X.shape[1]
        raise ValueError(f"When 'gamma' is a string, it should be either 'scale' or 'auto'. Got '{gamma}' instead.")
    if gamma < 0:
        raise ValueError('gamma must be non-negative')
    return float(gamma)


def class_weights(class_weight, classes, yi):
    """sklearn.utils.class_weight.compute_class_weight on the y handed to fit (``yi``: its class indices)."""
    if class_weight is None:
        return np.ones(len(classes))
    if isinstance(class_weight, str):
        if class_weight != 'balanced':
            raise ValueError("class_weight must be 'balanced', a dict or None")
        return len(yi) / (len(classes) * np.bincount(yi, minlength=len(classes)).astype(np.float64))
    return np.array([float(class_weight.get(c, 1.0)) for c in classes])


# ------------------------------------------------------------------------------------------------ problems (host)
def pair_problems(yi, positions, cw, sample_weight=None):
    """The class-pair problems of ONE fit.  ``yi``: the class index of every row handed to the fit; ``positions``: the row of each in
    the kernel matrix; ``cw``: the weight of every class; ``sample_weight``: per row (None: ones).  Zero-weight rows are dropped, as
    sklearn's libsvm does; the members of a class keep their original order (libsvm groups so); the pairs follow libsvm's order
    with the lower class positive; a class that lost all its rows takes its pairs with it, and fewer than two classes left raise
    sklearn's ``ValueError``.  Returns ``idx`` (int32 kernel-matrix rows, problem after problem, the positive class first), ``sizes``
    and ``npos`` per problem, ``pair_a`` / ``pair_b`` (indices into ``cw``) and, per point, ``weight`` (of its class) and ``sample_weight``."""
    yi, positions, cw = np.asarray(yi), np.asarray(positions), np.asarray(cw, dtype=np.float64)
    w = np.ones(len(yi)) if sample_weight is None else np.asarray(sample_weight, dtype=np.float64)
    kept = np.flatnonzero(w > 0)
    members = [kept[yi[kept] == c] for c in range(len(cw))]
    present = [c for c, m in enumerate(members) if len(m)]
    if len(present) < 2:
        raise ValueError(f'The number of classes has to be greater than one; got {len(present)} class')
    rows, sizes, npos, pair_a, pair_b = [], [], [], [], []
    for i, a in enumerate(present):
        for b in present[i + 1:]:
            rows += [members[a], members[b]]
            sizes.append(len(members[a]) + len(members[b]))
            npos.append(len(members[a]))
            pair_a.append(a)
            pair_b.append(b)
    rows = np.concatenate(rows)
    return dict(idx=positions[rows].astype(np.int32), sizes=np.asarray(sizes, dtype=np.int64), npos=np.asarray(npos, dtype=np.int32),
                pair_a=np.asarray(pair_a, dtype=np.int32), pair_b=np.asarray(pair_b, dtype=np.int32), weight=cw[yi[rows]],
                sample_weight=w[rows])


def bounds(C, problems):
    """The per-point upper bound of ``pair_problems``' points: (C * class weight) * sample weight, in this order."""
    return (float(C) * problems['weight']) * problems['sample_weight']


# ------------------------------------------------------------------------------------------------ the device
def upload_int32(arrays, dev):
    """Integer arrays -> one int32 host array -> ONE upload; a device view per array (the views share the storage and keep it alive)."""
    cuts = np.cumsum([0] + [len(a) for a in arrays])
    buf = torch.from_numpy(np.concatenate(arrays).astype(np.int32)).to(dev)
    return [buf[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def row_sq_norms(Ad, chunk=2048):
    """|a_i|^2 as the diagonal of the Gram matrix of the rows (f64 MFMA GEMM, in chunks of rows; no element-wise host math)."""
    return torch.cat([torch.diagonal(LA.dgemm(Ad[i:i + chunk], Ad[i:i + chunk], tb=True)) for i in range(0, Ad.shape[0], chunk)]).contiguous()


def kernel_from_gram(kernel, gamma, G, na, nb):
    """K from the Gram matrix G = A B^T: linear: G itself; rbf: exp(-gamma (|a|^2 + |b|^2 - 2 a.b)), libsvm's formula."""
    if kernel == 'linear':
        return G
    K = torch.empty_like(G)
    call('xps_rbf_from_gram_f64', G.data_ptr(), G.stride(0), na.data_ptr(), nb.data_ptr(), G.shape[0], G.shape[1], float(gamma),
         K.data_ptr(), K.stride(0), stream())
    return K


def kernel_matrix(kernel, gamma, Ad, na, Bd, nb):
    """K(A, B) on the device: the Gram matrix by the f64 MFMA GEMM, then ``kernel_from_gram`` (``na`` / ``nb`` are read for rbf only)."""
    return kernel_from_gram(kernel, gamma, LA.dgemm(Ad, Bd, tb=True), na, nb)


def smo(K, idx_d, off_d, npos_d, max_pts, cb, tol, max_iter, kbase=None, kld=None):
    """All problems in ONE launch: problem p is the points ``idx_d[off_d[p]:off_d[p + 1]]``, the first ``npos_d[p]`` of them positive,
    with the host bounds ``cb``; ``max_pts``: the size of the largest.  ``K`` is the one kernel matrix of all problems, or, with
    ``kbase`` / ``kld`` (int64 per problem), a buffer in which problem p's matrix starts at ``kbase[p]`` with the leading dimension
    ``kld[p]``.  ``max_iter``: the SVC's (-1: libsvm has no limit; here one nothing reaches).  Returns (alpha, rho, iterations)."""
    limit = int(lib().xps_svm_smo_f64_max_points())
    if max_pts > limit:
        raise ValueError(f'a class pair has {max_pts} samples; the LDS-resident solver takes {limit}')
    max_iter = int(max_iter) if max_iter and max_iter > 0 else max(10_000_000, 100 * max_pts)
    Q, dev = len(npos_d), K.device
    cb_d = torch.from_numpy(cb).to(dev)
    alpha = torch.empty(len(idx_d), dtype=torch.float64, device=dev)
    rho = torch.empty(Q, dtype=torch.float64, device=dev)
    iters = torch.empty(Q, dtype=torch.int32, device=dev)
    tail = (idx_d.data_ptr(), off_d.data_ptr(), npos_d.data_ptr(), Q, max_pts, cb_d.data_ptr(), float(tol), max_iter, alpha.data_ptr(),
            rho.data_ptr(), iters.data_ptr(), stream())
    if kbase is None:
        call('xps_svm_smo_f64', K.data_ptr(), K.stride(0), *tail)
    else:
        call('xps_svm_smo_multi_f64', K.data_ptr(), kbase.data_ptr(), kld.data_ptr(), *tail)
    return alpha, rho, iters


def coef_scatter(alpha, idx_d, off_d, npos_d, n):
    """The signed dual coefficients of every problem as a dense (Q, n) matrix: +alpha at the positive points of a problem, -alpha
    at its negative ones, zeros elsewhere (one launch; every element is written)."""
    Q = len(npos_d)
    coef = torch.empty(Q, n, dtype=torch.float64, device=alpha.device)
    call('xps_bag_coef_scatter_f64', alpha.data_ptr(), idx_d.data_ptr(), off_d.data_ptr(), npos_d.data_ptr(), Q, n, coef.data_ptr(),
         coef.stride(0), stream())
    return coef
