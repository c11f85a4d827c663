"""The fold-batched PCA in front of the SVC search on the MI355X: the two kernels of csrc/xps_pca_folds.hip through the C ABI
(long-double restatements, bit-identity of repeats and of every prefix with a single-cut call, every refusal), alignment.PCA's
Gram-side solver against numpy's SVD, and SVCSearchCV(batch_pca=True) against sklearn's PCA + libsvm fold by fold and against the
default route."""
import functools
import sys

import numpy as np
import pytest
from sklearn.base import clone
from sklearn.decomposition import PCA as SkPCA
from sklearn.metrics import accuracy_score, balanced_accuracy_score
from sklearn.model_selection import ParameterGrid, StratifiedKFold
from sklearn.pipeline import make_pipeline
from sklearn.svm import SVC as SkSVC

pytestmark = pytest.mark.gpu

NAN = float('nan')
U = 2.0 ** -53
LD = np.longdouble


def dev_tensor(a):
    import torch
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    return torch.from_numpy(np.ascontiguousarray(a)).to(LA.device())


def xps_call(name, *args):
    import torch
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import call
    try:
        call(name, *args, _dev.stream())
    finally:
        torch.cuda.synchronize()


def ptr(t):
    return None if t is None else t.data_ptr()


# ================================================================================================ 1. xps_gram_center_folds_f64
def center_case(N, ldg, folds, seed):
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((N, 7)) + 0.5
    G = np.full((N, ldg), NAN)
    G[:, :N] = F @ F.T + 0.01 * rng.standard_normal((N, N))              # (not symmetric: the kernel must not assume it)
    return G, [(np.asarray(tr), np.asarray(te)) for tr, te in folds]


def center_ref(G, N, folds):
    """Kc[a][b] = G[r_a][r_b] - m[a] - m[b] + mm in long double."""
    out = []
    Gl = G[:, :N].astype(LD)
    for tr, te in folds:
        rows = np.concatenate([tr, te]).astype(np.int64)
        sub = Gl[np.ix_(rows, tr)]
        m = sub.sum(axis=1) / LD(len(tr))
        mm = m[:len(tr)].sum() / LD(len(tr))
        out.append(sub - m[:, None] - m[None, :len(tr)] + mm)
    return out


def run_center(Gh, Nh, folds, **override):
    import torch
    from cross_patient_speech_decoding_amd._lib import lib
    rows = np.concatenate([np.concatenate([tr, te]) for tr, te in folds]).astype(np.int32)
    fold_off = np.concatenate([[0], np.cumsum([len(tr) + len(te) for tr, te in folds])]).astype(np.int32)      # host arrays
    n_train = np.array([len(tr) for tr, _ in folds], dtype=np.int32)
    sizes = [(len(tr) + len(te)) * len(tr) for tr, te in folds]
    G_d, rows_d = dev_tensor(Gh), dev_tensor(rows)
    Kc = torch.full((sum(sizes) + 5,), NAN, dtype=torch.float64, device=G_d.device)
    nb = int(lib().xps_gram_center_folds_f64_workspace(len(folds), int(fold_off[-1])))
    ws = torch.zeros(nb // 8 + 1, dtype=torch.int64, device=G_d.device)
    args = dict(G=ptr(G_d), ldg=Gh.shape[1], N=Nh, rows=ptr(rows_d), fold_off=fold_off.ctypes.data, n_train=n_train.ctypes.data,
                n_folds=len(folds), Kc=ptr(Kc), ws=ptr(ws), ws_bytes=nb)
    for key, val in override.items():
        args[key] = val.ctypes.data if isinstance(val, np.ndarray) else val
    xps_call('xps_gram_center_folds_f64', *args.values())
    host = Kc.cpu().numpy()
    assert np.isnan(host[sum(sizes):]).all()                              # nothing is written past the last fold
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    return [host[cuts[f]:cuts[f + 1]].reshape(len(tr) + len(te), len(tr)) for f, (tr, te) in enumerate(folds)]


def center_cases():
    perm = np.random.default_rng(3).permutation(67)
    parts = [perm[:23], perm[23:45], perm[45:]]                           # three folds of unequal size: 44 / 45 / 45 training rows
    rest = lambda i: np.concatenate([parts[j] for j in range(3) if j != i])
    desc = np.sort(perm)[::-1]
    return {'one row': (1, 1, [([0], [])]),
            'five rows, two folds': (5, 5, [([0, 1, 2], [3, 4]), ([3, 4], [0, 1, 2])]),
            '67 rows, padded': (67, 72, [(rest(0), parts[0]), (rest(1), parts[1]), (rest(2), parts[2]),
                                         (perm, np.zeros(0, dtype=np.int64)),              # a fold without held-out rows
                                         (desc[:40], desc[40:])])}                         # rows in descending order


@pytest.mark.parametrize('case', list(center_cases()))
def test_centring_kernel_is_within_its_bound_of_long_double_and_repeats_bit_for_bit(case):
    """|Kc - ref| <= (2 n_tr + 8) 2^-53 max|G|: two n_tr-term sums and four additions."""
    N, ldg, folds = center_cases()[case]
    G, folds = center_case(N, ldg, folds, 7 + N)
    got = run_center(G, N, folds)
    again = run_center(G, N, folds)
    gmax = np.abs(G[:, :N]).max()
    share = 0.0
    for (tr, te), a, b, ref in zip(folds, got, again, center_ref(G, N, folds)):
        assert np.isfinite(a).all()                                       # (the NaN padding of G was not read)
        np.testing.assert_array_equal(a.view(np.int64), b.view(np.int64))
        bound = (2 * len(tr) + 8) * U * gmax
        err = float(np.abs(a.astype(LD) - ref).max())
        share = max(share, err / bound)
        assert err <= bound
    print(f'{case}: largest error / bound = {share:.3f}')


def test_centring_kernel_refuses_bad_arguments():
    from cross_patient_speech_decoding_amd._lib import XpsError
    N, ldg, folds = center_cases()['five rows, two folds']
    G, folds = center_case(N, ldg, folds, 1)
    run_center(G, N, folds)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    for key in ('G', 'rows', 'fold_off', 'n_train', 'Kc', 'ws'):
        with pytest.raises(XpsError, match='null argument'):
            run_center(G, N, folds, **{key: None})
    for change in (dict(N=0), dict(ldg=4), dict(n_folds=-1), dict(n_folds=65536)):
        with pytest.raises(XpsError, match='bad parameter'):
            run_center(G, N, folds, **change)
    for bad in (i32(0, 5, 4), i32(0, -1, 10)):
        with pytest.raises(XpsError, match='fold_off must ascend'):
            run_center(G, N, folds, fold_off=bad)
    with pytest.raises(XpsError, match='start at 0'):
        run_center(G, N, folds, fold_off=i32(1, 5, 10))
    for bad in (i32(0, 2), i32(3, 6), i32(-1, 2)):
        with pytest.raises(XpsError, match='n_train'):
            run_center(G, N, folds, n_train=bad)
    with pytest.raises(XpsError, match='workspace'):
        run_center(G, N, folds, ws_bytes=8)
    for where, value in ((0, -1), (4, 5), (9, 2 ** 31 - 1), (5, -2 ** 31)):   # an index outside [0, N): refused, nothing read
        bad = [(tr.copy(), te.copy()) for tr, te in folds]
        flat = [bad[0][0], bad[0][1], bad[1][0], bad[1][1]]
        pos = where
        for part in flat:
            if pos < len(part):
                part[pos] = value
                break
            pos -= len(part)
        with pytest.raises(XpsError, match=r'outside \[0, N\)'):
            run_center(G, N, bad)


# ================================================================================================ 2. xps_prefix_kernels_f64
R_MAX = 40
GAMMAS = [0.0, 0.37, 2.5e-3]
CUT_LISTS = [(1,), (1, 2, 3), (4, 17, 40)]
SIZES = [1, 5, 33, 67]


@functools.lru_cache(maxsize=None)
def score_matrices():
    rng = np.random.default_rng(17)
    return {n: rng.standard_normal((n, R_MAX)) * np.linspace(3.0, 0.2, R_MAX) for n in SIZES}


def run_prefix(cases, mode, gap=3, **override):
    """cases: list of (Z (n, R) ndarray, ldz, cuts, gammas): every cut gets one output per gamma.  Returns {(p, r, g): matrix}.
    The outputs lie `gap` doubles apart in a NaN-filled buffer: what lies between them must stay NaN."""
    import torch
    from cross_patient_speech_decoding_amd._lib import lib
    tab = np.zeros((len(cases), 8), dtype=np.int64)
    cuts, cut_out, gammas, dest, tiles, keep, where = [], [0], [], [], [], [], {}
    pos = gap
    for p, (Z, ldz, cut_list, gs) in enumerate(cases):
        n, R = Z.shape
        Zp = np.full((n, ldz), NAN)
        Zp[:, :R] = Z
        keep.append(dev_tensor(Zp))
        tab[p, :6] = [ptr(keep[-1]), ldz, n, R, len(cuts), len(cuts) + len(cut_list)]
        for r in cut_list:
            cuts.append(r)
            for g in gs:
                where[p, r, g] = (pos, n)
                gammas.append(g)
                dest.append(pos)
                pos += n * n + gap
            cut_out.append(len(dest))
        nt = -(-n // 16)
        tiles += [(p, a, b) for a in range(nt) for b in range(nt)]
    h = dict(problems=tab.reshape(-1), cuts=np.array(cuts, dtype=np.int32), cut_out=np.array(cut_out, dtype=np.int32),
             gammas=np.array(gammas, dtype=np.float64), dest=np.array(dest, dtype=np.int64), tiles=np.array(tiles, dtype=np.int32).reshape(-1))
    h.update({k: v for k, v in override.items() if isinstance(v, np.ndarray)})
    K = torch.full((pos,), NAN, dtype=torch.float64, device=keep[0].device)
    n_tiles = len(h['tiles']) // 3
    nb = int(lib().xps_prefix_kernels_f64_workspace(len(cases), len(cuts), len(dest), n_tiles))
    ws = torch.zeros(nb // 8 + 1, dtype=torch.int64, device=K.device)
    args = dict(problems=h['problems'].ctypes.data, n_problems=len(cases), cuts=h['cuts'].ctypes.data, cut_out=h['cut_out'].ctypes.data,
                n_cuts=len(cuts), gammas=h['gammas'].ctypes.data, dest=h['dest'].ctypes.data, n_out=len(dest), tiles=h['tiles'].ctypes.data,
                n_tiles=n_tiles, rbf=int(mode), K=ptr(K), k_len=pos, ws=ptr(ws), ws_bytes=nb)
    args.update({k: v for k, v in override.items() if not isinstance(v, np.ndarray)})
    xps_call('xps_prefix_kernels_f64', *args.values())
    host = K.cpu().numpy()
    written = np.zeros(pos, dtype=bool)
    out = {}
    for key, (o, n) in where.items():
        out[key] = host[o:o + n * n].reshape(n, n)
        written[o:o + n * n] = True
    assert np.isnan(host[~written]).all() and np.isfinite(host[written]).all()
    return out


@pytest.mark.parametrize('rbf', [0, 1])
@pytest.mark.parametrize('cut_list', CUT_LISTS)
def test_prefix_kernel_snapshots_equal_single_cut_calls_and_stay_within_their_bounds(cut_list, rbf):
    """Four problems of different n in one launch, ldz > R.  Every snapshot equals, bit for bit, a call that has the single cut r on the
    first r columns alone.  Linear: |acc - ref| <= (r + 1) 2^-53 sum_k |z_ik z_jk| (an r-term chain of FMAs).  Rbf: the distance
    d = na + nb - 2 g is built from three such chains and two more roundings (2 g is exact), so |d^ - d| <= E_d = (r + 4) 2^-53 (S_ii +
    S_jj + 2 S_ij) with S_ab = sum_k |z_ak z_bk|; the product with gamma rounds once, E_t = gamma E_d + 2^-53 gamma (|d| + E_d); and
    |K^ - K| <= K expm1(E_t) + 2 ulp(K) for exp."""
    Zs = score_matrices()
    gs = GAMMAS if rbf else [0.0]
    got = run_prefix([(Zs[n], R_MAX + 3, cut_list, gs) for n in SIZES], rbf)
    share = 0.0
    for r in cut_list:
        single = run_prefix([(np.ascontiguousarray(Zs[n][:, :r]), r, (r,), gs) for n in SIZES], rbf)
        for p, n in enumerate(SIZES):
            Zl = Zs[n][:, :r].astype(LD)
            ref = Zl @ Zl.T
            S = np.abs(Zl) @ np.abs(Zl).T
            for g in gs:
                K = got[p, r, g]
                np.testing.assert_array_equal(K.view(np.int64), single[p, r, g].view(np.int64))
                np.testing.assert_array_equal(K, K.T)                     # (a commutative product in both chains)
                if not rbf:
                    bound = (r + 1) * U * S
                    err = np.abs(K.astype(LD) - ref)
                else:
                    sq = np.diag(ref)
                    d = sq[:, None] + sq[None, :] - 2 * ref
                    diag = np.diag(S)
                    E_d = (r + 4) * U * (diag[:, None] + diag[None, :] + 2 * S)
                    E_t = g * E_d + U * g * (np.abs(d) + E_d)
                    Kref = np.exp(-LD(g) * d)
                    bound = Kref * np.expm1(E_t) + 2 * 2.0 ** -52 * Kref
                    err = np.abs(K.astype(LD) - Kref)
                    np.testing.assert_array_equal(np.diag(K), np.ones(n))  # the diagonal is exactly 1
                    if g == 0.0:
                        np.testing.assert_array_equal(K, np.ones((n, n)))
                assert (err <= bound).all()
                share = max(share, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    print(f'cuts {cut_list}, rbf={rbf}: largest error / bound = {share:.3f}')


def test_prefix_kernel_refuses_bad_arguments():
    from cross_patient_speech_decoding_amd._lib import XpsError
    Z = score_matrices()[5]
    good = [(Z, R_MAX + 3, (1, 2, 3), [0.5]), (score_matrices()[33], R_MAX, (4, 17, 40), [0.5])]
    base = run_prefix(good, 1)
    assert len(base) == 6
    i32 = lambda *v: np.array(v, dtype=np.int32)
    for key in ('problems', 'cuts', 'cut_out', 'gammas', 'dest', 'tiles', 'K', 'ws'):
        with pytest.raises(XpsError, match='null argument'):
            run_prefix(good, 1, **{key: None})
    for change in (dict(rbf=2), dict(n_cuts=-1), dict(n_out=-1), dict(n_tiles=-1), dict(k_len=-1)):
        with pytest.raises(XpsError, match='bad parameter'):
            run_prefix(good, 1, **change)
    with pytest.raises(XpsError, match='workspace'):
        run_prefix(good, 1, ws_bytes=16)
    for cuts, why in ((i32(1, 3, 2, 4, 17, 40), 'cuts must ascend'), (i32(1, 2, 2, 4, 17, 40), 'cuts must ascend'),
                      (i32(0, 2, 3, 4, 17, 40), 'a cut of 0'), (i32(1, 2, 3, 4, 17, 41), 'beyond R'), (i32(-1, 2, 3, 4, 17, 40), 'a cut of 0')):
        with pytest.raises(XpsError, match=why):
            run_prefix(good, 1, cuts=cuts)
    for co, why in ((i32(0, 1, 3, 2, 4, 5, 6), 'cut_out must ascend'), (i32(1, 1, 2, 3, 4, 5, 6), 'from 0 to n_out'),
                    (i32(0, 1, 2, 3, 4, 5, 7), 'from 0 to n_out')):
        with pytest.raises(XpsError, match=why):
            run_prefix(good, 1, cut_out=co)

    def table(words):
        tab = np.zeros((2, 8), dtype=np.int64)
        keep = [dev_tensor(np.ones((5, R_MAX + 3))), dev_tensor(np.ones((33, R_MAX)))]
        tab[0, :6] = [ptr(keep[0]), R_MAX + 3, 5, R_MAX, 0, 3]
        tab[1, :6] = [ptr(keep[1]), R_MAX, 33, R_MAX, 3, 6]
        for (p, w), v in words.items():
            tab[p, w] = v
        return tab.reshape(-1), keep
    for words, why in (({(0, 2): 0}, 'n must be'), ({(1, 2): -3}, 'n must be'), ({(0, 3): 0}, 'R < 1'), ({(0, 1): R_MAX - 1}, 'ldz < R'),
                       ({(1, 0): 0}, 'null score matrix'), ({(0, 5): 0}, 'none empty'), ({(1, 4): 2}, 'follow each other'),
                       ({(1, 5): 7}, 'follow each other'), ({(1, 5): 5}, 'belong to no problem'), ({(1, 2): 34}, 'outside K')):
        tab, keep = table(words)
        with pytest.raises(XpsError, match=why):
            run_prefix(good, 1, problems=tab)
    dest = np.array([3, 31, 59, 87, 1179, 2271], dtype=np.int64)
    for o, v in ((0, -1), (5, 2275), (2, 2 ** 40)):
        bad = dest.copy()
        bad[o] = v
        with pytest.raises(XpsError, match='outside K'):
            run_prefix(good, 1, dest=bad)
    for g in (-0.5, np.inf, NAN):
        with pytest.raises(XpsError, match='gamma'):
            run_prefix(good, 1, gammas=np.array([0.5, 0.5, g, 0.5, 0.5, 0.5]))
    tiles = np.array([(0, 0, 0)] + [(1, a, b) for a in range(3) for b in range(3)], dtype=np.int32)
    for t, v, why in ((0, (2, 0, 0), 'names no problem'), (0, (-1, 0, 0), 'names no problem'), (0, (0, 1, 0), 'outside its problem'),
                      (3, (1, 0, 3), 'outside its problem'), (3, (1, -1, 0), 'outside its problem')):
        bad = tiles.copy()
        bad[t] = v
        with pytest.raises(XpsError, match=why):
            run_prefix(good, 1, tiles=bad.reshape(-1))


# ================================================================================================ 3. alignment.PCA(solver='gram')
def svd_pca(X):
    Xc = X.astype(np.float64) - X.astype(np.float64).mean(axis=0)
    _, s, Vt = np.linalg.svd(Xc, full_matrices=False)
    ratio = s ** 2 / (s ** 2).sum()
    return Xc, s, Vt, ratio


@functools.lru_cache(maxsize=None)
def pca_data(wide):
    if wide:                                                              # the reference notebook's shape, float32
        from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
        X = make_patient(2, 144, T=200, C=111)[0].reshape(144, -1)
        assert X.shape == (144, 22200) and X.dtype == np.float32
    else:
        rng = np.random.default_rng(5)
        X = (rng.standard_normal((40, 9)) * np.linspace(4, 1, 9)) @ rng.standard_normal((9, 300)) + 0.3 * rng.standard_normal((40, 300)) + 2.0
    return (X,) + svd_pca(X)


@pytest.mark.parametrize('wide', [False, True])
def test_gram_solver_equals_numpys_svd_of_the_centred_matrix(wide):
    import cross_patient_speech_decoding_amd.alignment as A
    X, Xc, s, Vt, ratio = pca_data(wide)
    n = X.shape[0]
    for frac in (0.5, 0.8, 0.95):
        k = int(np.searchsorted(np.cumsum(ratio), frac, side='right') + 1)
        margin = np.abs(np.cumsum(ratio) - frac).min()
        assert margin > 1e-9                                              # (a condition on the input: the rule has room)
        p = A.PCA(frac, solver='gram').fit(X)
        assert p.n_components_ == k and p.components_.shape == (k, X.shape[1])
        flip = np.sign((p.components_ * Vt[:k]).sum(axis=1))
        comp_err = np.abs(p.components_ * flip[:, None] - Vt[:k]).max() / np.abs(Vt[:k]).max()
        want = Xc @ Vt[:k].T
        T = p.transform(X)
        t_err = np.abs(T * flip - want).max() / np.abs(want).max()
        print(f'wide={wide} frac={frac}: k={k}, margin {margin:.2e}, components {comp_err:.2e}, transform {t_err:.2e}, L_k/L_0 {(s[k - 1] / s[0]) ** 2:.2e}')
        assert comp_err <= 1e-8 and t_err <= 1e-8
        np.testing.assert_allclose(p.explained_variance_, s[:k] ** 2 / (n - 1), rtol=1e-9)
        np.testing.assert_allclose(p.explained_variance_ratio_, ratio[:k], rtol=1e-9)
        np.testing.assert_allclose(p.singular_values_, s[:k], rtol=1e-9)
        idx = np.argmax(np.abs(p.components_), axis=1)
        assert (p.components_[np.arange(k), idx] > 0).all()               # the class's sign rule
        if frac == 0.5:
            back = p.inverse_transform(T)
            assert back.shape == X.shape and p.n_features_in_ == X.shape[1] and p.n_samples_ == n
            auto = A.GramPCA(frac).fit(X)                                 # 'auto' takes the Gram side when d > n: the same bits
            np.testing.assert_array_equal(auto.components_, p.components_)


def test_auto_is_the_covariance_solver_bit_for_bit_when_there_are_no_more_features_than_rows():
    import cross_patient_speech_decoding_amd.alignment as A
    rng = np.random.default_rng(6)
    for n, d in ((50, 20), (20, 20)):
        X = rng.standard_normal((n, d)) * np.linspace(3, 0.5, d) + 1.0
        a, b, c = A.GramPCA(0.9).fit(X), A.PCA(0.9).fit(X), A.PCA(0.9, solver='covariance').fit(X)
        for other in (a, c):
            assert other.n_components_ == b.n_components_
            for name in ('components_', 'explained_variance_', 'explained_variance_ratio_', 'singular_values_', 'mean_'):
                np.testing.assert_array_equal(getattr(other, name), getattr(b, name))
            np.testing.assert_array_equal(other.transform(X), b.transform(X))
    with pytest.raises(ValueError, match='solver must be'):
        A.PCA(2, solver='svd').fit(X)


def test_gram_solver_refuses_a_kept_component_below_the_spectrum_limit():
    import cross_patient_speech_decoding_amd.alignment as A
    from cross_patient_speech_decoding_amd.decomposition import DimRedReshape
    X = pca_data(False)[0]
    for est in (A.PCA(None, solver='gram'), A.GramPCA(), A.GramPCA(40)):    # n_components=None on wide data: the last direction has L = 0
        with pytest.raises(ValueError, match="fewer components or use solver='covariance'"):
            est.fit(X)
    assert A.GramPCA(39).fit(X).n_components_ == 39                       # n - 1 directions of 40 centred rows are there
    assert clone(A.PCA(3, solver='gram')).solver == 'gram'
    step = DimRedReshape(A.GramPCA, n_components=4).fit(X.reshape(40, 30, 10))
    assert step.transformer.solver == 'auto' and step.transform(X.reshape(40, 30, 10)).shape == (40, 4)


# ================================================================================================ 4. the search
TOL = 1e-6
SETTINGS = dict(kernel='rbf', class_weight='balanced', tol=TOL)
NC = 'dimredreshape__n_components'
RECIPES = {'A': dict(patient=(0, 60), shape=dict(T=10, C=8, n_cond=12, k=4), folds=3, margin=7.4e-4,
                     grid={NC: [0.3, 0.5, 0.8, 0.95, 5], 'svc__C': [1, 100], 'svc__gamma': ['scale', 0.01]}),
           'B': dict(patient=(1, 180), shape=dict(T=6, C=40, n_cond=24, k=6), folds=4, margin=3.8e-5,
                     grid={NC: [0.5, 0.9], 'svc__C': [1, 10], 'svc__gamma': ['scale']})}


def pipeline(dim_red=None):
    import cross_patient_speech_decoding_amd.alignment as A
    from cross_patient_speech_decoding_amd.decoders import SVC
    from cross_patient_speech_decoding_amd.decomposition import DimRedReshape
    return make_pipeline(DimRedReshape(dim_red or A.GramPCA), SVC(**SETTINGS))


def recipe_data(name):
    from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
    rec = RECIPES[name]
    X, y_full = make_patient(*rec['patient'], **rec['shape'])
    return X, y_full[:, 0], StratifiedKFold(rec['folds'])


def sklearn_folds(X, y, splits, cands):
    """Per fold sklearn's PCA(svd_solver='full') per n_components, per (candidate, fold) libsvm on its features: predictions, robust
    rows, component counts, the kernel matrices of [training rows; held-out rows] and the margin of the variance-fraction rule."""
    F = X.reshape(len(X), -1).astype(np.float64)
    pred, robust, comps, kernels, feats = {}, {}, {}, {}, {}
    margin = np.inf
    for f, (tr, te) in enumerate(splits):
        cs = np.cumsum(SkPCA(svd_solver='full').fit(F[tr]).explained_variance_ratio_)
        for c, cand in enumerate(cands):
            nc = cand[NC]
            if (nc, f) not in feats:
                sk = SkPCA(n_components=nc, svd_solver='full').fit(F[tr])
                feats[nc, f] = (sk.transform(F[tr]), sk.transform(F[te]), sk.n_components_)
                if nc < 1:
                    margin = min(margin, float(np.abs(cs - nc).min()))
            Ztr, Zte, comps[c, f] = feats[nc, f]
            svc = SkSVC(decision_function_shape='ovo', C=cand['svc__C'], gamma=cand['svc__gamma'], **SETTINGS).fit(Ztr, y[tr])
            pred[c, f] = svc.predict(Zte)
            robust[c, f] = (np.abs(svc.decision_function(Zte).reshape(len(te), -1)) >= 1e-3).all(axis=1)
            Z = np.vstack([Ztr, Zte])
            sq = (Z * Z).sum(axis=1)
            kernels[c, f] = np.exp(-svc._gamma * (sq[:, None] + sq[None, :] - 2 * Z @ Z.T))
    return pred, robust, comps, kernels, margin


@functools.lru_cache(maxsize=None)
def searched(name):
    """The fused search, the default route and sklearn fold by fold on one recipe: computed once, shared (read-only)."""
    from cross_patient_speech_decoding_amd.decoders import SVCSearchCV
    X, y, cv = recipe_data(name)
    grid = RECIPES[name]['grid']
    cands = list(ParameterGrid(grid))
    splits = list(cv.split(X, y))
    fused = SVCSearchCV(pipeline(), grid, cv=cv, refit=False, batch_pca=True).fit(X, y)
    default = SVCSearchCV(pipeline(), grid, cv=cv, refit=False).fit(X, y)
    sk_pred, robust, comps, kernels, margin = sklearn_folds(X, y, splits, cands)
    return dict(X=X, y=y, cv=cv, grid=grid, cands=cands, splits=splits, fused=fused, default=default, sk_pred=sk_pred, robust=robust,
                comps=comps, kernels=kernels, margin=margin)


@pytest.mark.parametrize('name', ['A', 'B'])
def test_search_cuts_every_fold_where_sklearns_pca_does(name):
    s = searched(name)
    fused = s['fused']
    print(f'recipe {name}: margin of the variance-fraction rule {s["margin"]:.3e}')
    assert s['margin'] >= RECIPES[name]['margin'] * 0.99                  # a condition on the input (7.4e-4 / 3.8e-5, two digits given)
    assert fused.pca_n_components_.shape == (len(s['cands']), len(s['splits'])) and fused.pca_fallbacks_ == []
    for (c, f), k in s['comps'].items():
        assert fused.pca_n_components_[c, f] == k
    assert not hasattr(s['default'], 'pca_n_components_')


@pytest.mark.parametrize('name', ['A', 'B'])
def test_search_kernel_matrices_equal_those_of_sklearns_pca_features(name):
    """The matrices of the plan, rebuilt through the same wrappers the search calls, against exp(-gamma |z_i - z_j|^2) of sklearn's
    PCA features with sklearn's own gamma: within 1e-10 of the largest entry (float64 numpy reaches 7e-14; the smallest L_r / L_0
    is 1.4e-2; a wrong centre or cut errs by 1e-3 or more)."""
    import torch
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    from cross_patient_speech_decoding_amd.decoders import search as S
    s = searched(name)
    X, y = s['X'], s['y']
    classes, yi = np.unique(y, return_inverse=True)
    pipe = pipeline()
    plan = S.build_plan_pca(pipe, [S.split_params_pca(pipe, c) for c in s['cands']], X, yi, classes, s['splits'])
    sizes = [plan.rows(v) ** 2 for v, _ in plan.matrices]
    base = np.concatenate([[0], np.cumsum(sizes)])
    K = torch.full((int(base[-1]),), NAN, dtype=torch.float64, device=LA.device())
    per_fold = {}
    for m, (view, gamma) in enumerate(plan.matrices):
        assert view[0] == 'pca'
        per_fold.setdefault(view[1], {}).setdefault(view[2], []).append((gamma, int(base[m])))
    tables = LA.prefix_kernels([(plan.pca['Z'][f], sorted(cuts.items())) for f, cuts in per_fold.items()], True, K)
    host = K.cpu().numpy()
    assert tables is not None and np.isfinite(host).all()
    worst = 0.0
    for mod in plan.models:
        n = plan.rows(plan.matrices[mod['matrix']][0])
        got = host[base[mod['matrix']]:base[mod['matrix'] + 1]].reshape(n, n)
        want = s['kernels'][mod['cand'], mod['fold']]
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print(f'recipe {name}: largest kernel-matrix difference / largest entry = {worst:.2e}')
    assert len(plan.models) == len(s['cands']) * len(s['splits']) and worst <= 1e-10


@pytest.mark.parametrize('name', ['A', 'B'])
def test_search_predicts_as_the_default_route_and_as_sklearn_on_every_robust_row(name):
    s = searched(name)
    fused, default = s['fused'], s['default']
    total = weak = 0
    for f, (te, labels) in enumerate(fused.cv_test_predictions_):
        np.testing.assert_array_equal(te, s['splits'][f][1])
        for c in range(len(s['cands'])):
            ok = s['robust'][c, f]
            np.testing.assert_array_equal(labels[c][ok], s['sk_pred'][c, f][ok])
            np.testing.assert_array_equal(labels[c][ok], default.cv_test_predictions_[f][1][c][ok])
            total += len(ok)
            weak += int((~ok).sum())
    print(f'recipe {name}: {weak} of {total} rows are not robust')
    assert weak / total <= 0.03                                           # a condition on the input, not a tolerance
    assert fused.cv_results_['params'] == default.cv_results_['params'] == s['cands']
    assert fused.best_params_ == default.best_params_


@pytest.mark.parametrize('name', ['A', 'B'])
def test_search_scores_are_sklearns_metrics_of_its_own_predictions(name):
    from cross_patient_speech_decoding_amd.decoders import search as S
    s = searched(name)
    fused, y = s['fused'], s['y']
    bal = S.scores_from_confusion(fused.cv_confusion_, 'balanced_accuracy')
    for f, (te, labels) in enumerate(fused.cv_test_predictions_):
        for c in range(len(s['cands'])):
            assert fused.cv_results_[f'split{f}_test_score'][c] == accuracy_score(y[te], labels[c])
            assert bal[c, f] == balanced_accuracy_score(y[te], labels[c])
    table = np.array([fused.cv_results_[f'split{f}_test_score'] for f in range(len(s['splits']))]).T
    again = S.assemble_results(s['cands'], table)
    for key in ('mean_test_score', 'std_test_score', 'rank_test_score'):
        np.testing.assert_array_equal(fused.cv_results_[key], again[key])
    assert fused.best_params_ == s['cands'][fused.best_index_] and fused.best_score_ == again['mean_test_score'][fused.best_index_]


def same_results(a, b):
    np.testing.assert_array_equal(a.cv_confusion_, b.cv_confusion_)
    for (_, x), (_, z) in zip(a.cv_test_predictions_, b.cv_test_predictions_):
        np.testing.assert_array_equal(x, z)
    for key in ('mean_test_score', 'std_test_score', 'rank_test_score'):
        np.testing.assert_array_equal(a.cv_results_[key], b.cv_results_[key])
    np.testing.assert_array_equal(a.pca_n_components_, b.pca_n_components_)
    assert a.best_params_ == b.best_params_


def test_a_shift_of_the_data_changes_no_robust_prediction():
    from cross_patient_speech_decoding_amd.decoders import SVCSearchCV
    s = searched('A')
    shifted = SVCSearchCV(pipeline(), s['grid'], cv=s['cv'], refit=False, batch_pca=True).fit(s['X'].astype(np.float64) + 50.0, s['y'])
    np.testing.assert_array_equal(shifted.pca_n_components_, s['fused'].pca_n_components_)
    for f, (_, labels) in enumerate(shifted.cv_test_predictions_):
        for c in range(len(s['cands'])):
            ok = s['robust'][c, f]
            np.testing.assert_array_equal(labels[c][ok], s['fused'].cv_test_predictions_[f][1][c][ok])


def test_two_runs_and_four_chunks_give_the_same_bits(monkeypatch):
    from cross_patient_speech_decoding_amd.decoders import SVCSearchCV
    from cross_patient_speech_decoding_amd.decoders import search as S
    s = searched('A')
    chunks = []
    real = S._run_chunk
    monkeypatch.setattr(S, '_run_chunk', lambda plan, mats, *a: (chunks.append(list(mats)), real(plan, mats, *a))[1])
    again = SVCSearchCV(pipeline(), s['grid'], cv=s['cv'], refit=False, batch_pca=True).fit(s['X'], s['y'])
    same_results(again, s['fused'])
    assert len(chunks) == 1
    n_mats = len(chunks[0])
    del chunks[:]
    per_chunk = -(-n_mats // 4)
    cut = SVCSearchCV(pipeline(), s['grid'], cv=s['cv'], refit=False, batch_pca=True, max_kernel_bytes=per_chunk * 8 * 60 * 60).fit(s['X'], s['y'])
    assert len(chunks) == 4 and sorted(m for ch in chunks for m in ch) == list(range(n_mats))
    same_results(cut, s['fused'])


def test_a_cut_beyond_the_rank_takes_the_per_fold_fit_inside_the_same_plan():
    import cross_patient_speech_decoding_amd.alignment as A
    from cross_patient_speech_decoding_amd.decoders import SVCSearchCV
    rng = np.random.default_rng(8)
    y = np.arange(30) % 3
    X = ((rng.standard_normal((30, 3)) + np.eye(3)[y] * 2.0) @ rng.standard_normal((3, 80))).reshape(30, 8, 10)     # exactly rank 3
    cands = [{NC: 10, 'svc__C': 1.0, 'svc__gamma': 'scale'}, {NC: 2, 'svc__C': 1.0, 'svc__gamma': 'scale'},
             {NC: None, 'svc__C': 10.0, 'svc__gamma': 0.05}]
    cv = StratifiedKFold(3)
    fused = SVCSearchCV(pipeline(A.PCA), candidates=cands, cv=cv, refit=False, batch_pca=True).fit(X, y)
    default = SVCSearchCV(pipeline(A.PCA), candidates=cands, cv=cv, refit=False).fit(X, y)
    assert fused.pca_fallbacks_ == [(0, 10), (0, None), (1, 10), (1, None), (2, 10), (2, None)]
    np.testing.assert_array_equal(fused.pca_n_components_, [[10] * 3, [2] * 3, [20] * 3])
    for (_, a), (_, b) in zip(fused.cv_test_predictions_, default.cv_test_predictions_):
        np.testing.assert_array_equal(a[[0, 2]], b[[0, 2]])                # the per-fold fits: the default route's predictions exactly
    np.testing.assert_array_equal(fused.cv_confusion_[[0, 2]], default.cv_confusion_[[0, 2]])


def test_one_launch_of_each_kernel_whatever_the_number_of_folds_and_candidates(monkeypatch):
    from collections import Counter
    from cross_patient_speech_decoding_amd import _lib
    from cross_patient_speech_decoding_amd.decoders import SVCSearchCV
    counts = Counter()
    real = _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    for mod in list(sys.modules.values()):                               # every module that bound `call` by name
        if getattr(mod, '__name__', '').startswith('cross_patient_speech_decoding_amd') and getattr(mod, 'call', None) is real:
            monkeypatch.setattr(mod, 'call', counting)
    X, y, _ = recipe_data('A')
    wider = {NC: [0.3, 0.5, 0.8, 0.95, 5], 'svc__C': [0.1, 1, 10, 100], 'svc__gamma': ['scale', 0.01]}
    for folds, grid in ((3, RECIPES['A']['grid']), (6, wider)):
        counts.clear()
        search = SVCSearchCV(pipeline(), grid, cv=folds, refit=False, batch_pca=True).fit(X, y)
        assert search.cv_confusion_.shape[:2] == (len(ParameterGrid(grid)), folds) and len(ParameterGrid(grid)) == (20 if folds == 3 else 40)
        for entry in ('xps_gram_center_folds_f64', 'xps_apply_grouped_f64', 'xps_prefix_kernels_f64', 'xps_svm_smo_multi_f64',
                      'xps_svm_cv_score_f64', 'xps_colsum_f64'):
            assert counts[entry] == 1, (entry, dict(counts))
        assert counts['xps_rbf_multi_from_gram_f64'] == 0 and counts['xps_xcov_f64'] == 0 and counts['xps_apply_f64'] == 0, dict(counts)
        assert counts['xps_dgemm_small'] + counts['xps_dgemm_splitk'] == 1, dict(counts)       # the one Gram product
        print(folds, dict(counts))


def test_refit_with_grampca_predicts_like_the_cloned_pipeline_fitted_by_hand():
    from cross_patient_speech_decoding_amd.decoders import SVCSearchCV
    X, y, cv = recipe_data('A')
    grid = {NC: [0.5, 5], 'svc__C': [1, 100], 'svc__gamma': ['scale']}
    search = SVCSearchCV(pipeline(), grid, cv=cv, batch_pca=True).fit(X, y)
    by_hand = clone(pipeline()).set_params(**search.best_params_).fit(X, y)
    Xnew = recipe_data('A')[0][::-1] * 1.01
    np.testing.assert_array_equal(search.predict(Xnew), by_hand.predict(Xnew))
    np.testing.assert_array_equal(search.decision_function(Xnew), by_hand.decision_function(Xnew))
    assert search.score(X, y) == by_hand.score(X, y)
