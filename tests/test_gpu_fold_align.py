"""Fold-batched PCA -> CCA alignment (alignment.fit_folds, process_aligner_folds, batched_folds=True) on the device.

Expected values: ``oracle.align_oracle.process_aligner`` per fold, fed the same values as float64 on that fold's training
rows; projections through the sklearn PCA it returns.  Bars (the project's, tests/test_gpu_alignment.py): component counts
equal, pooled tensors and projections within 1e-6 * max|expected|, canonical correlations within 1e-8, labels equal.  Each
fold's cumulative-variance curve must stay 1e-6 away from 0.95 at the chosen count (asserted), else the count is ambiguous.
The four grouped kernels are also checked on their own against float64 numpy.  T = 20 throughout."""
import functools

import numpy as np
import pytest
import torch
from sklearn.model_selection import KFold

pytestmark = pytest.mark.gpu

from oracle import align_oracle as ao  # noqa: E402
from cross_patient_speech_decoding_amd.utils.synthetic import make_patient  # noqa: E402

T = 20
CASES = {                      # N, channel counts (target first), n_cond, folds, dtype the device gets
    'A': (48, [24, 20, 24, 17], 12, 4, np.float32),
    'B': (60, [33, 20, 40, 17], 40, 5, np.float64),
    'C': (40, [130, 24], 10, 4, np.float32),
}


def A():
    import cross_patient_speech_decoding_amd.alignment as a
    return a


def LA():
    from cross_patient_speech_decoding_amd.alignment import _linalg
    return _linalg


def DM():
    from cross_patient_speech_decoding_amd.nn_models.data_utils import datamodules
    return datamodules


@functools.lru_cache(maxsize=None)
def _inputs(name):
    N, Cs, n_cond, k, dtype = CASES[name]
    pats = [make_patient(p, N + 3 * p, T=T, C=c, n_cond=n_cond, k=6, noise=0.5) for p, c in enumerate(Cs)]
    X, y = pats[0]
    pool = [(x, yy, yy) for x, yy in pats[1:]]
    splits = list(KFold(k, shuffle=True, random_state=0).split(X))
    return X, y, pool, splits, dtype


def _oracle_fold(X, y, pool, tr):
    """oracle process_aligner on one fold's training rows (float64 values) + its canonical correlations and the margin of
    the 0.95 rule on the target's curve."""
    X64 = X.astype(np.float64)
    pool64 = [(x.astype(np.float64), yy, ya) for x, yy, ya in pool]
    X_pool, y_pool, tar = ao.process_aligner(X64[tr], y[tr], y[tr], pool64)
    cum = np.cumsum(tar.explained_variance_ratio_)
    margin = min(cum[-1] - 0.95, 0.95 - cum[-2]) if len(cum) > 1 else cum[-1] - 0.95
    tar_dr = tar.transform(X64[tr].reshape(-1, X.shape[-1])).reshape(len(tr), T, -1)
    corrs = []
    for x, _, ya in pool64:
        _, z = ao.pca_fit(x.reshape(-1, x.shape[-1]), 0.95)
        corrs.append(ao.AlignCCAOracle().fit(tar_dr, z.reshape(x.shape[0], T, -1), y[tr], ya).canon_corrs)
    return X_pool, y_pool, tar, corrs, margin


@functools.lru_cache(maxsize=None)
def _expected(name):
    X, y, pool, splits, _ = _inputs(name)
    return [_oracle_fold(X, y, pool, tr) for tr, _ in splits]


@functools.lru_cache(maxsize=None)
def _fitted(name):
    X, y, pool, splits, dtype = _inputs(name)
    return A().fit_folds(X.astype(dtype), y, [(x.astype(dtype), yy, ya) for x, yy, ya in pool], splits)


def _lost_conditions(name):
    X, y, pool, splits, _ = _inputs(name)
    keys = ao.label_keys(y)
    return [len(np.unique(keys)) - len(np.unique(keys[tr])) for tr, _ in splits]


def test_the_cases_are_what_they_claim():
    assert _lost_conditions('A') == [0, 0, 0, 0]                       # no fold loses a condition
    assert all(4 <= n <= 6 for n in _lost_conditions('B'))              # every fold loses 4 to 6
    assert sorted(_lost_conditions('C')) == [0, 0, 0, 1]               # one fold loses one
    assert not LA().lib().xps_jacobi_small_supported(130, 130, 0)       # case C's target is wider than the one-workgroup Jacobi


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_fold_matches_the_oracle(name):
    X, y, pool, splits, dtype = _inputs(name)
    fa, exp = _fitted(name), _expected(name)
    assert fa.fallbacks_ == []
    for f, ((tr, te), (X_pool, y_pool, tar, corrs, margin)) in enumerate(zip(splits, exp)):
        print(f'case {name} fold {f}: margin of the 0.95 rule {margin:.3e}, n_components {tar.n_components_}')
        assert margin >= 1e-6, (f, margin)
        assert fa.n_components_[f] == tar.n_components_
        assert fa.pca_components_[f].shape == tar.components_.shape and fa.pca_mean_[f].shape == tar.mean_.shape
        got = fa.train_pool(f)
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == X_pool.shape
        err = np.abs(got.cpu().numpy().astype(np.float64) - X_pool).max() / np.abs(X_pool).max()
        proj = tar.transform(X[te].astype(np.float64).reshape(-1, X.shape[-1])).reshape(len(te), T, -1)
        gp = fa.project(f, te)
        assert gp.dtype == torch.float32 and tuple(gp.shape) == proj.shape
        perr = np.abs(gp.cpu().numpy().astype(np.float64) - proj).max() / np.abs(proj).max()
        cerr = max(np.abs(fa.canon_corrs_[f][p] - corrs[p]).max() for p in range(len(pool)))
        print(f'   pooled rel err {err:.2e}, projection rel err {perr:.2e}, canon_corrs err {cerr:.2e}')
        assert err <= 1e-6, (f, err)
        assert perr <= 1e-6, (f, perr)
        for p in range(len(pool)):
            assert fa.canon_corrs_[f][p].shape == corrs[p].shape
        assert cerr <= 1e-8, (f, cerr)
        assert fa.M_a_[f][0].shape[0] == tar.n_components_ and tuple(fa.maps_[f][0].shape)[1] == tar.n_components_


@pytest.mark.parametrize('name', ['A', 'B'])
def test_process_aligner_folds_pool_and_labels(name):
    X, y, pool, splits, dtype = _inputs(name)
    out = DM().process_aligner_folds(X.astype(dtype), y, None, [(x.astype(dtype), yy, ya) for x, yy, ya in pool], splits)
    assert len(out) == len(splits)
    for (tr, te), (Xp, yp, proj), (X_pool, y_pool, tar, _, _) in zip(splits, out, _expected(name)):
        assert yp.dtype == torch.int64 and np.array_equal(yp.numpy(), y_pool)
        assert np.abs(Xp.cpu().numpy() - X_pool).max() <= 1e-6 * np.abs(X_pool).max()
        z = proj.transform(X[te].astype(dtype).reshape(-1, X.shape[-1]))
        ref = tar.transform(X[te].astype(np.float64).reshape(-1, X.shape[-1]))
        assert np.abs(z - ref).max() <= 1e-6 * np.abs(ref).max()


def test_equal_trial_counts_keep_the_hstack_quirk():
    """(N, L) labels with the same N in every patient hstack to (N, L * P) in process_aligner; the folds path keeps that."""
    X, y, pool, splits, dtype = _inputs('A')
    n_tr = len(splits[0][0])
    assert all(len(tr) == n_tr for tr, _ in splits)
    pool_eq = [(x[:n_tr], yy[:n_tr], ya[:n_tr]) for x, yy, ya in pool[:1]]
    out = DM().process_aligner_folds(X, y, y, pool_eq, splits)
    for (tr, _), (Xp, yp, _) in zip(splits, out):
        _, y_pool, _ = ao.process_aligner(X[tr].astype(np.float64), y[tr], y[tr], [(x.astype(np.float64), yy, ya) for x, yy, ya in pool_eq])
        assert y_pool.shape == (n_tr, 6) and np.array_equal(yp.numpy(), y_pool)


def test_two_fits_are_bit_identical():
    X, y, pool, splits, dtype = _inputs('A')
    a, b = A().fit_folds(X, y, pool, splits), A().fit_folds(X, y, pool, splits)
    for f in range(len(splits)):
        assert torch.equal(a.train_pool(f), b.train_pool(f))
        assert np.array_equal(a.pca_components_[f], b.pca_components_[f])


def test_chunking_by_max_bytes_changes_nothing():
    X, y, pool, splits, dtype = _inputs('A')
    a, b = _fitted('A'), A().fit_folds(X, y, pool, splits, max_bytes=1)          # one fold per chunk
    for f in range(len(splits)):
        assert torch.equal(a.train_pool(f), b.train_pool(f))


# ------------------------------------------------------------------ fallback
def _fallback_inputs():
    """Case A's target (24 channels) and two pooled patients of 24 channels, every PCA keeping all 24 components; the second
    pooled patient shares ONE condition with the target: 20 rows meet 24 columns."""
    X, y, _, splits, _ = _inputs('A')
    (x1, y1), (x2, y2) = (make_patient(p, 48 + 3 * p, T=T, C=24, n_cond=12, k=6, noise=0.5) for p in (1, 2))
    keys, k2 = ao.label_keys(y), ao.label_keys(y2)
    keep = [c for c in np.unique(k2) if all(c in keys[tr] for tr, _ in splits)][0]
    ya2 = np.where((k2 == keep)[:, None], y2, y2 + 10)                  # every other condition gets labels the target lacks
    return X, y, [(x1, y1, y1), (x2, y2, ya2)], splits


def test_single_shared_condition_takes_the_per_problem_path():
    X, y, pool, splits = _fallback_inputs()
    keys = ao.label_keys(y)
    for tr, _ in splits:
        assert len(np.intersect1d(np.unique(keys[tr]), np.unique(ao.label_keys(pool[1][2])))) == 1     # 20 rows
    fa = A().fit_folds(X, y, pool, splits, n_components=24)
    assert fa.n_components_ == [24] * len(splits)
    assert sorted(fa.fallbacks_) == [(f, 1) for f in range(len(splits))]
    X64, pool64 = X.astype(np.float64), [(x.astype(np.float64), yy, ya) for x, yy, ya in pool]
    rng = np.random.default_rng(7)
    Xq = X64 * (1 + 1e-12 * rng.standard_normal(X64.shape))
    poolq = [(x * (1 + 1e-12 * rng.standard_normal(x.shape)), yy, ya) for x, yy, ya in pool64]
    for f, (tr, te) in enumerate(splits):
        got = fa.train_pool(f).cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        own, _, _ = DM().process_aligner(X[tr], y[tr], y[tr], pool, A().AlignCCA, n_components=24)
        own = own.numpy().astype(np.float64)
        lo = len(tr) + pool[0][0].shape[0]
        assert got.shape == own.shape
        assert np.abs(got[lo:] - own[lo:]).max() <= 1e-6 * np.abs(own[lo:]).max()
        assert np.abs(got[:lo] - own[:lo]).max() <= 1e-6 * np.abs(own[:lo]).max()       # the other blocks: batched vs per-fold
        ref, _, _ = ao.process_aligner(X64[tr], y[tr], y[tr], pool64, n_components=24)
        refq, _, _ = ao.process_aligner(Xq[tr], y[tr], y[tr], poolq, n_components=24)
        scale = np.abs(ref[lo:]).max()
        sens = np.abs(ref[lo:].astype(np.float64) - refq[lo:]).max() / scale
        err = np.abs(got[lo:] - ref[lo:]).max() / scale
        print(f'fold {f}: oracle against itself under a 1e-12 relative perturbation {sens:.2e}, device against oracle {err:.2e}')
        # measured (oracle alone, CPU): it moves by 3.7e-9 to 9.5e-9 of the block's largest entry under the perturbation, the
        # float32 rounding of its output; 100 x that stays below the floor, so the bar is 1e-6 in every fold
        assert err <= max(1e-6, 100 * sens), (f, err, sens)


# ------------------------------------------------------------------ the kernels on their own
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _xcov_ref(Am, Bm, ba, bb, blk_len, ca, cb):
    ra = np.concatenate([np.arange(s, s + blk_len) for s in ba]).astype(int) if len(ba) else np.zeros(0, dtype=int)
    rb = np.concatenate([np.arange(s, s + blk_len) for s in bb]).astype(int) if len(bb) else np.zeros(0, dtype=int)
    a = Am[ra].astype(np.float64) - (0 if ca is None else ca)
    b = Bm[rb].astype(np.float64) - (0 if cb is None else cb)
    return a.T @ b, a.sum(0), b.sum(0), float(len(ra))


def test_xcov_grouped_against_numpy_and_bit_identical():
    la = LA()
    rng = np.random.default_rng(11)
    M17 = rng.standard_normal((300, 17)).astype(np.float32)
    M33 = rng.standard_normal((320, 33))
    M130 = rng.standard_normal((100, 130)).astype(np.float32)
    wide = rng.standard_normal((90, 40))                                  # row-strided view: 33 of 40 columns
    c17, c33, c130 = rng.standard_normal(17), rng.standard_normal(33), rng.standard_normal(130)
    long_blocks = rng.permutation(14)[:14] * 20                           # 14 blocks x 20 rows = 280 rows > 256: split-K, 2 slabs
    assert la.xcov_grouped_splits(280) == 2 and la.xcov_grouped_splits(256) == 1 and la.xcov_grouped_splits(0) == 1
    host = [
        (M17, M33, [0, 40, 20], [300, 0, 20], 20, c17, c33),              # d_a != d_b, fp32 x fp64, unordered blocks
        (M130, M130, [0, 80, 20, 40], [0, 80, 20, 40], 20, c130, c130),   # 130 columns: 3 x 3 tiles, Gram
        (M33, M17, [5], [7], 20, None, None),                             # one block, no centres
        (M17, M33, [], [], 20, c17, c33),                                 # zero blocks
        (M17, M17, long_blocks, long_blocks[::-1].copy(), 20, c17, None), # long: the split-K route
        (wide[:, :33], M130, [0, 60, 30], [3, 77, 40], 7, c33, c130),      # strided rows, block length 7, 33 x 130
        (M130, M130, [0, 20, 40, 60, 80], [0, 20, 40, 60, 80], 20, c130, c130),   # rows 0..99 in order, one split: = xps_xcov_f64
    ]
    dev_m = {id(m): _dev(m) for m in (M17, M33, M130)}
    wide_d = _dev(wide)

    def dv(m):
        return wide_d[:, :33] if m.base is wide else dev_m[id(m)]
    probs = [(dv(a), dv(b), ba, bb, bl, None if ca is None else _dev(ca), None if cb is None else _dev(cb))
             for a, b, ba, bb, bl, ca, cb in host]
    out1, offs = la.xcov_grouped(probs)
    out2, _ = la.xcov_grouped(probs)
    assert torch.equal(out1, out2)                                        # fixed-order slab reduce
    out = out1.cpu().numpy()
    for i, (a, b, ba, bb, bl, ca, cb) in enumerate(host):
        Cr, sa, sb, cnt = _xcov_ref(a, b, ba, bb, bl, ca, cb)
        da, db = Cr.shape
        blk = out[offs[i]:offs[i + 1]]
        assert len(blk) == da * db + da + db + 1 and blk[-1] == cnt
        scale = max(np.abs(Cr).max(), 1e-300)
        assert np.abs(blk[:da * db].reshape(da, db) - Cr).max() <= 1e-12 * scale, i
        s_scale = max(np.abs(sa).max(), np.abs(sb).max(), 1e-300)
        assert np.abs(blk[da * db:da * db + da] - sa).max() <= 1e-12 * s_scale, i
        assert np.abs(blk[da * db + da:-1] - sb).max() <= 1e-12 * s_scale, i
        if cnt == 0:
            assert not blk.any()
    # the whole matrix in order as one problem = xps_xcov_f64, bit for bit (the same 16-row steps over the same rows, one split)
    c130_d = _dev(c130)
    whole = la.xcov(dev_m[id(M130)], dev_m[id(M130)], c130_d, c130_d).cpu().numpy()
    np.testing.assert_array_equal(out[offs[6]:offs[6] + 130 * 130].reshape(130, 130), whole)
    with pytest.raises(ValueError, match='outside its matrix'):
        la.xcov_grouped([(dev_m[id(M17)], dev_m[id(M33)], [290], [0], 20, None, None)])


@pytest.mark.parametrize('G,n_out', [(2, 2), (20, 20), (5, 4)])
def test_loo_sum_equals_the_ascending_numpy_loop(G, n_out):
    rng = np.random.default_rng(G)
    x = rng.standard_normal((G, 1000)) * 10.0 ** rng.integers(-8, 8, (G, 1000))
    out = LA().loo_sum(_dev(x), n_out).cpu().numpy()
    for f in range(n_out):
        acc = np.zeros(1000)
        for g in range(G):
            if g != f:
                acc += x[g]
        np.testing.assert_array_equal(out[f], acc)


def test_apply_grouped_against_numpy():
    la = LA()
    rng = np.random.default_rng(5)
    specs = [(70, 33, 1, np.float32, np.float64, True), (130, 17, 5, np.float64, np.float32, False),
             (1, 40, 17, np.float32, np.float32, True), (65, 130, 70, np.float64, np.float64, True)]
    host, entries, outs = [], [], []
    big = torch.full((300, 80), 7.0, dtype=torch.float32, device='cuda')      # slabs of a wider tensor: neighbours stay untouched
    for i, (rows, d_in, d_out, xt, ot, with_mean) in enumerate(specs):
        X = rng.standard_normal((rows, d_in)).astype(xt)
        W = rng.standard_normal((d_in, d_out))
        mean = rng.standard_normal(d_in) if with_mean else None
        if i == 2:
            out = big[10:11, 3:20]
        else:
            out = torch.zeros(rows, d_out, dtype=torch.float32 if ot == np.float32 else torch.float64, device='cuda')
        host.append((X, W, mean))
        outs.append(out)
        entries.append((_dev(X), None if mean is None else _dev(mean), _dev(W), out))
    la.apply_grouped(entries)
    for (X, W, mean), out, spec in zip(host, outs, specs):
        ref = (X.astype(np.float64) - (0 if mean is None else mean)) @ W
        got = out.cpu().numpy()
        if spec[4] == np.float32:
            # the float32 rounding of the float64 result: at most one float32 ulp apart where the float64 values differ in rounding
            assert got.dtype == np.float32
            assert np.abs(got.astype(np.float64) - ref).max() <= 2.0 ** -24 * np.abs(ref).max() * (1 + 1e-6)
            near = np.abs(ref - ref.astype(np.float32)) < 0.49 * np.spacing(np.abs(ref).astype(np.float32))
            np.testing.assert_array_equal(got[near], ref.astype(np.float32)[near])
        else:
            assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    rest = big.clone()
    rest[10:11, 3:20] = 7.0
    assert bool((rest == 7.0).all())
    for (X, W, mean), e in zip(host[:1], entries[:1]):                    # one entry alone = xps_apply_f64, bit for bit
        assert torch.equal(outs[0], la.apply(e[0], e[2], e[1]))


def test_cnd_avg_folds_against_numpy():
    la = LA()
    rng = np.random.default_rng(9)
    Z0, Z1 = rng.standard_normal((12, T, 5)), rng.standard_normal((12, T, 7))     # two folds, ragged widths
    cond = np.array([0, 1, 2, 0, 1, 0, 3, 0, 1, 0, 1, 0])
    fold_tr = [np.array([0, 1, 2, 3, 4, 5, 7, 8, 9]), np.array([0, 1, 3, 4, 5, 6, 7, 10, 11])]
    # fold 0: condition 2 has ONE remaining trial and condition 3 is absent; fold 1: condition 3 present, condition 2 absent
    segs, refs = [], []
    for Z, tr in zip((Z0, Z1), fold_tr):
        Zd = _dev(Z)
        for c in np.unique(cond[tr]):
            trials = tr[cond[tr] == c]
            out = torch.empty(T, Z.shape[-1], dtype=torch.float64, device='cuda')
            segs.append((Zd, out, trials))
            refs.append(Z[trials].sum(0) / len(trials))
    assert [len(s[2]) for s in segs][:3] == [5, 3, 1] and len(segs) == 6
    la.cnd_avg_folds(segs)
    for (_, out, _), ref in zip(segs, refs):
        assert np.abs(out.cpu().numpy() - ref).max() <= 1e-13 * np.abs(ref).max()
    with pytest.raises(ValueError, match='outside src'):
        la.cnd_avg_folds([(segs[0][0], segs[0][1], [12])])


def test_svd_batched_against_numpy():
    rng = np.random.default_rng(2)
    for shape in ((6, 9, 9), (5, 12, 7), (4, 7, 12)):
        Ks = rng.standard_normal(shape)
        for K, (U, s, Vt) in zip(Ks, LA().svd_batched(Ks)):
            np.testing.assert_allclose(s, np.linalg.svd(K, compute_uv=False), atol=1e-12)
            np.testing.assert_allclose((U * s) @ Vt, K, atol=1e-12)


# ------------------------------------------------------------------ data module
def test_data_module_batched_folds_matches_the_default_path():
    X, y, pool, splits, _ = _inputs('A')
    dm = DM()
    mods = []
    for batched in (False, True):
        m = dm.AlignedMicroValDataModule(X, y, y, pool, A().AlignCCA, folds=4, val_size=0.2, augmentations=None,
                                         batched_folds=batched)
        np.random.seed(0)
        m.setup()
        mods.append(m)
    for k in range(4):
        a, b = mods[0]._folds[k], mods[1]._folds[k]
        for name in dm._FoldModule.FOLD_KEYS:
            assert a[name] is not None and b[name] is not None and a[name].shape == b[name].shape, name
            if name.endswith('labels'):
                assert torch.equal(a[name], b[name]), name
            else:
                assert a[name].dtype == b[name].dtype == torch.float32
                assert (a[name] - b[name]).abs().max().item() <= 1e-6 * a[name].abs().max().item(), (k, name)


def test_data_module_batched_folds_refuses_what_it_does_not_support():
    X, y, pool, _, _ = _inputs('A')
    dm, a = DM(), A()
    with pytest.raises(ValueError, match='batched_folds'):
        dm.AlignedMicroDataModule(X, y, y, pool, a.AlignCCA, folds=4, batched_folds=True)               # aligns after the split
    with pytest.raises(ValueError, match='batched_folds'):
        dm.AlignedMicroValDataModule(X, y, y, pool, a.AlignMCCA, folds=4, batched_folds=True)
    with pytest.raises(ValueError, match='batched_folds'):
        dm.AlignedMicroValDataModule(X, y, y, pool, lambda: a.AlignCCA(type='trial'), folds=4, batched_folds=True)
    with pytest.raises(ValueError, match='batched_folds'):
        dm.AlignedMicroValDataModule(X, y, y, pool, a.AlignCCA, folds=4, multiview=True, batched_folds=True)
    with pytest.raises(ValueError, match='batched_folds'):
        dm.AlignedMicroValDataModule(X, y, y, pool, a.AlignCCA, folds=4, process_group=object(), batched_folds=True)
    dm.AlignedMicroValDataModule(X, y, y, pool, a.AlignCCA, folds=4)                                    # the default is untouched
