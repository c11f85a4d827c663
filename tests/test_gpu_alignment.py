"""GPU parity of the alignment path (cnd_avg, CCA, MCCA, joint PCA, PCA) through the C ABI:
against the golden vectors produced by the reference's own alignment package, against the CPU
oracle on seeded inputs, and — at BASELINE full size — through size-independent properties.
Tolerances: canon_corrs <= 1e-8, transform outputs <= 1e-6 relative, condition
means bit-exact."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import align_oracle as ao  # noqa: E402
from oracle import mcca_oracle as mo  # noqa: E402


def A():
    import cross_patient_speech_decoding_amd.alignment as a
    return a


def LA():
    from cross_patient_speech_decoding_amd.alignment import _linalg
    return _linalg


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def _match_up_to_sign(M, ref, tol):
    assert M.shape == ref.shape
    for j in range(M.shape[1]):
        e = min(np.abs(M[:, j] - ref[:, j]).max(), np.abs(M[:, j] + ref[:, j]).max())
        assert e <= tol * max(1.0, np.abs(ref[:, j]).max()), (j, e)


# ------------------------------------------------------------------ condition means
def test_cnd_avg_bit_exact_vs_reference_golden(golden_dir):
    g = _load(golden_dir, 'align_labels.npz')
    a = A()
    avg1 = a.cnd_avg(g['X1'], a.label2str(g['y1']))
    avg3 = a.cnd_avg(g['X3'], a.label2str(g['y3']))
    assert avg1.dtype == np.float64 and avg3.dtype == np.float64
    np.testing.assert_array_equal(avg1, g['avg1'])           # float64 input
    np.testing.assert_array_equal(avg3, g['avg3'])           # float32 input: f32 sum, f32 divide, f64 store
    out = a.extract_group_conditions([g['gXa'], g['gXb'], g['gXc']], [g['gya'], g['gyb'], g['gyc']])
    for i in range(3):
        np.testing.assert_array_equal(out[i], g[f'g{i}'])


def test_cnd_avg_ragged_and_large():
    rng = np.random.default_rng(0)
    a = A()
    # ragged: one condition with a single trial, one with many; float32
    y = np.array([5] * 1 + [7] * 300 + [10] * 13)
    X = rng.standard_normal((len(y), 9, 5)).astype(np.float32)
    perm = rng.permutation(len(y))
    X, y = X[perm], y[perm]
    np.testing.assert_array_equal(a.cnd_avg(X, a.label2str(y)), ao.cnd_avg(X, ao.label_keys(y)))
    # north-star sized slice: 2048 trials x 200 x 128 float32 (210 MB), 64 conditions
    y = rng.integers(0, 64, 2048)
    X = rng.standard_normal((2048, 200, 128), dtype=np.float32)
    got = a.cnd_avg(X, a.label2str(y))
    sel = [0, 17, 63]
    keys = ao.label_keys(y)
    uniq = np.unique(keys)
    for c in sel:
        np.testing.assert_array_equal(got[c], np.mean(X[keys == uniq[c]], axis=0).astype(np.float64))
    # property: count-weighted mean of condition means == grand mean
    counts = np.array([(keys == u).sum() for u in uniq])
    np.testing.assert_allclose((got * counts[:, None, None]).sum(0) / len(y), X.mean(0, dtype=np.float64), atol=2e-5)


# ------------------------------------------------------------------ CCA
@pytest.mark.parametrize('case', ['full', 'uneq', 'rdef'])
def test_align_cca_vs_reference_golden(golden_dir, case):
    g = _load(golden_dir, 'align_cca.npz')
    Xa, ya, Xb, yb = (g[f'{case}_{k}'] for k in ('Xa', 'ya', 'Xb', 'yb'))
    al = A().AlignCCA(return_space='shared')
    assert al.fit(Xa, Xb, ya, yb) is None
    assert al.M_a.dtype == np.float64 and isinstance(al.canon_corrs, np.ndarray)
    if case == 'rdef':
        _check_rank_deficient(al, g, Xa, ya, Xb, yb)
        return
    np.testing.assert_allclose(al.canon_corrs, g[f'{case}_S'], rtol=0, atol=1e-8)
    if case != 'rdef':
        _match_up_to_sign(al.M_a, g[f'{case}_M_a'], 1e-7)
        _match_up_to_sign(al.M_b, g[f'{case}_M_b'], 1e-7)
        ta, tb = al.transform([Xa, Xb])
        _match_up_to_sign(ta.reshape(-1, ta.shape[-1]), g[f'{case}_shared_ta'].reshape(-1, ta.shape[-1]), 1e-6)
        _match_up_to_sign(tb.reshape(-1, tb.shape[-1]), g[f'{case}_shared_tb'].reshape(-1, tb.shape[-1]), 1e-6)
    else:
        assert al.M_b.shape == g['rdef_M_b'].shape == (7, 6)        # rank truncation reproduced
    for space, X in (('b_to_a', Xb), ('a_to_b', Xa)):
        al.return_space = space
        al._maps = {}
        out = al.transform(X)
        ref = g[f'{case}_{space}_t']
        assert out.shape == ref.shape and out.dtype == np.float64
        rel = np.abs(out - ref).max() / np.abs(ref).max()
        assert rel <= 1e-6, (space, rel)


def _check_rank_deficient(al, g, Xa, ya, Xb, yb):
    """View B has an exactly dependent channel (rank 6 of 7).  The reference's answer is then NOT
    a function of the data alone: Householder QR of a rank-deficient matrix completes Q with a
    direction built from rounding noise (AlignCCA.py:269-270), and that column enters the SVD
    of Q_a^T Q_b (:273) with a chance correlation ~ 1/sqrt(n_samples).  The HIP path computes the
    exact CCA on the rank-truncated space instead.  What must agree: the rank truncation
    (shapes), and the values up to that chance-correlation term; what the HIP result must satisfy
    exactly: the CCA optimality conditions."""
    assert al.M_a.shape == g['rdef_M_a'].shape and al.M_b.shape == g['rdef_M_b'].shape == (7, 6)
    # How far may the values be from the golden?  Not further than the reference is from ITSELF: the fixture holds the
    # reference's own outputs for this input perturbed by relative noise of 1e-16 (below one ulp): its canonical
    # correlations move by 0.03 .. 0.10 and its transforms by 18 .. 77 % (rdef_ref_selfdiff_*).  That spread -- not a
    # tolerance picked to pass -- is the bound.
    assert g['rdef_ref_selfdiff_S'].min() > 1e-3 and g['rdef_ref_selfdiff_T'].min() > 1e-2     # the golden is ill-defined at this level
    assert np.abs(al.canon_corrs - g['rdef_S']).max() <= g['rdef_ref_selfdiff_S'].max()
    La, Lb = ao.shared_class_dynamics(Xa, Xb, ya, yb)
    La, Lb = La - La.mean(0), Lb - Lb.mean(0)
    Pa, Pb = La @ al.M_a, Lb @ al.M_b
    np.testing.assert_allclose(Pa.T @ Pa, np.eye(6), atol=1e-9)          # orthonormal canonical variates
    np.testing.assert_allclose(Pb.T @ Pb, np.eye(6), atol=1e-9)
    np.testing.assert_allclose(Pa.T @ Pb, np.diag(al.canon_corrs), atol=1e-9)   # diagonal = canonical corrs
    # and they are the correlations scipy's exact subspace-angle computation gives on the true range spaces
    import scipy.linalg
    Lb_r = Lb[:, :6]                                                      # drop the dependent channel
    ang = scipy.linalg.subspace_angles(La, Lb_r)
    np.testing.assert_allclose(np.sort(np.cos(ang))[::-1][:6], al.canon_corrs, atol=1e-9)
    al.return_space = 'b_to_a'
    out = al.transform(Xb)
    ref = g['rdef_b_to_a_t']
    assert out.shape == ref.shape
    assert np.abs(out - ref).max() / np.abs(ref).max() <= g['rdef_ref_selfdiff_T'].max()


@pytest.mark.parametrize('case,tol_s,tol_t', [('illc7', 1e-8, 1e-6), ('illc9', 1e-7, 1e-5)])
def test_align_cca_ill_conditioned_full_rank_vs_reference_golden(golden_dir, case, tol_s, tol_t):
    """Views with condition numbers 2e7 / 6e8 (channel scales spanning 7 / 9 decades), full rank by LAPACK's rule on the
    singular values (reference AlignCCA.py:263-264: tolerance s_max * max(shape) * eps ~ 4e-14).  A Gram-side method sees
    eigenvalue ratios of 1e-15 / 1e-18 there (below ITS tolerance: it would drop channels and return other shapes) and loses
    half the digits; the device path takes the SVD of the centred data themselves, keeps every channel like the reference and
    matches it at the bounds of the well-conditioned cases (illc7) / at eps * cond (illc9)."""
    g = _load(golden_dir, 'align_cca.npz')
    Xa, ya, Xb, yb = (g[f'{case}_{k}'] for k in ('Xa', 'ya', 'Xb', 'yb'))
    al = A().AlignCCA(return_space='b_to_a')
    al.fit(Xa, Xb, ya, yb)
    assert al.M_a.shape == g[f'{case}_M_a'].shape == (8, 7) and al.M_b.shape == g[f'{case}_M_b'].shape == (7, 7)   # no channel dropped
    np.testing.assert_allclose(al.canon_corrs, g[f'{case}_S'], rtol=0, atol=tol_s)
    for space, X in (('b_to_a', Xb), ('a_to_b', Xa)):
        al.return_space = space
        al._maps = {}
        out = al.transform(X)
        ref = g[f'{case}_{space}_t']
        # per channel: the channels differ by up to nine decades in scale
        scale = np.abs(ref).reshape(-1, ref.shape[-1]).max(axis=0)
        rel = (np.abs(out - ref).reshape(-1, ref.shape[-1]).max(axis=0) / scale).max()
        assert rel <= tol_t, (space, rel)


def test_cca_align_function_and_inplace_centering(golden_dir):
    g = _load(golden_dir, 'align_cca.npz')
    La, Lb = g['raw_La'].copy(), g['raw_Lb'].copy()
    Ma, Mb, S = A().CCA_align(La, Lb)
    np.testing.assert_allclose(S, g['raw_S'], atol=1e-8)
    _match_up_to_sign(Ma, g['raw_Ma'], 1e-7)
    _match_up_to_sign(Mb, g['raw_Mb'], 1e-7)
    np.testing.assert_allclose(La, g['raw_La'] - g['raw_La'].mean(1, keepdims=True), atol=1e-14)   # mutated like the reference


def test_cca_errors_and_torch_input(golden_dir):
    a = A()
    with pytest.raises(RuntimeError, match=r'Must call fit\(\) before transforming data\.'):
        a.AlignCCA().transform(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError, match='type must be "class" or "trial".'):
        a.AlignCCA(type='bogus').fit(np.zeros((4, 3, 2)), np.zeros((4, 3, 2)), np.arange(4), np.arange(4))
    g = _load(golden_dir, 'align_cca.npz')
    al = a.AlignCCA()
    al.fit(g['full_Xa'], g['full_Xb'], g['full_ya'], g['full_yb'])
    out_t = al.transform(torch.from_numpy(g['full_Xb']))         # tensors arrive in realtime_datamodule.py:891
    np.testing.assert_allclose(out_t, g['full_b_to_a_t'], rtol=0, atol=1e-6 * np.abs(g['full_b_to_a_t']).max())


def test_cca_float32_large_seeded_vs_oracle():
    """PCA-sized latent dims, float32 inputs, 64 conditions x 200 steps (n = 12800 samples)."""
    from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
    Xa, ya = make_patient(0, 512, T=200, C=40)
    Xb, yb = make_patient(1, 480, T=200, C=33)
    ref = ao.AlignCCAOracle().fit(Xa, Xb, ya, yb)
    al = A().AlignCCA()
    al.fit(Xa, Xb, ya, yb)
    np.testing.assert_allclose(al.canon_corrs, ref.canon_corrs, atol=1e-8)
    out, exp = al.transform(Xb), ref.transform(Xb)
    assert np.abs(out - exp).max() / np.abs(exp).max() <= 1e-6


# ------------------------------------------------------------------ PCA / joint PCA
def test_pca_vs_sklearn():
    rng = np.random.default_rng(5)
    X = (rng.standard_normal((6000, 6)) @ rng.standard_normal((6, 24)) + 0.3 * rng.standard_normal((6000, 24)))
    for dtype, tol in ((np.float64, 1e-9), (np.float32, 2e-5)):
        Xd = X.astype(dtype)
        p, Z = ao.pca_fit(Xd, 0.95)
        q = A().PCA(n_components=0.95)
        Zq = q.fit_transform(Xd)
        assert q.n_components_ == p.n_components_
        np.testing.assert_allclose(q.components_, p.components_, atol=tol * 10)
        np.testing.assert_allclose(q.explained_variance_, p.explained_variance_, rtol=max(tol, 1e-9) * 10)
        np.testing.assert_allclose(Zq, Z, atol=tol * 100)
    q = A().PCA(n_components=5).fit(X)
    assert q.components_.shape == (5, 24)


def test_joint_pca_vs_reference_golden(golden_dir):
    g = _load(golden_dir, 'align_jointpca.npz')
    Xs, ys = [g[f'X{i}'] for i in range(3)], [g[f'y{i}'] for i in range(3)]
    jp = A().JointPCA(n_components=4)
    t = jp.fit_transform(Xs, ys)
    assert isinstance(jp.transforms, tuple) and len(jp.transforms) == 3
    for i in range(3):
        np.testing.assert_allclose(jp.transforms[i], g[f'W{i}'], rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(t[i], g[f't{i}'], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(jp.transform(Xs[1], idx=1), g['t1_single'], rtol=1e-6, atol=1e-7)
    with pytest.raises(IndexError, match='Input idx is greater than the number of learned'):
        jp.transform(Xs[0], idx=3)
    with pytest.raises(RuntimeError, match='Must call fit'):
        A().JointPCA().transform(Xs)


# ------------------------------------------------------------------ MCCA (parity unpinned vs mvlearn)
def _mcca_data(seed=9):
    rng = np.random.default_rng(seed)
    seqs = np.array([[a, b, 2] for a in (1, 2, 3, 4) for b in (1, 2)])
    Z = np.cumsum(rng.standard_normal((8, 12, 3)), axis=1)
    feats, labs = [], []
    for n, C in ((40, 6), (36, 8), (44, 5)):
        c = np.concatenate([np.arange(8), rng.integers(0, 8, n - 8)])
        feats.append(Z[c] @ rng.standard_normal((3, C)) + 0.2 * rng.standard_normal((n, 12, C)))
        labs.append(seqs[c])
    return feats, labs


@pytest.mark.parametrize('pca_var', [1, 0.9])
def test_align_mcca_vs_oracle_and_properties(pca_var):
    feats, labs = _mcca_data()
    ref = mo.get_mcca_transforms(feats, labs, n_components=3, regs=0.5, pca_var=pca_var)
    al = A().AlignMCCA(n_components=3, regs=0.5, pca_var=pca_var)
    out = al.fit_transform(feats, labs)
    assert len(al.mcca.loadings_) == 3
    np.testing.assert_allclose(al.mcca.evals_, ref.evals_, rtol=1e-9, atol=1e-10)
    for i in range(3):
        np.testing.assert_allclose(al.mcca.loadings_[i], ref.loadings_[i], rtol=1e-6, atol=1e-8)
        exp = mo.mcca_transform(ref, feats[i], i)
        assert out[i].shape == exp.shape
        np.testing.assert_allclose(out[i], exp, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(al.transform(feats[i], idx=i), exp, rtol=1e-6, atol=1e-8)
    if pca_var == 1:
        # generalised-eigen residual and RHS-orthonormality of the device solution
        views = [a.reshape(-1, a.shape[-1]) for a in ao.extract_group_conditions(feats, labs)]
        views = [v - v.mean(0) for v in views]
        LHS, RHS = mo.mcca_gevp_blocks(views, 0.5)
        V = np.vstack(al.mcca.loadings_)
        np.testing.assert_allclose(LHS @ V, RHS @ V * al.mcca.evals_, atol=1e-8 * np.abs(LHS).max())
        np.testing.assert_allclose(V.T @ RHS @ V, np.eye(3), atol=1e-9)
    with pytest.raises(IndexError, match='Input idx is greater than the number of learned'):
        al.transform(feats[0], idx=3)
    with pytest.raises(RuntimeError, match='Must call fit'):
        A().AlignMCCA().transform(feats)


_north_star_views = {}


@pytest.mark.parametrize('sizes', [[128] * 8, [30, 30, 17, 136, 1], [64]])
def test_cholesky_whitening_factors_of_the_view_blocks_vs_numpy(sizes):
    """xps_chol_whiten_f64 (the RHS reduction of the MCCA pencil, AlignMCCA._gevp): S_b = L_b^-T of A_b = scale G_bb + shift I,
    against numpy's Cholesky factor; the regularised blocks written over LHS; a block that is not positive definite is refused."""
    la = LA()
    rng = np.random.default_rng(len(sizes))
    offs = np.concatenate([[0], np.cumsum(sizes)])
    D = int(offs[-1])
    Z = rng.standard_normal((max(sizes) // 2 + 3, D))             # rank deficient blocks: only the shift makes them definite
    G = Z.T @ Z
    Gd = torch.from_numpy(G).cuda()
    LHS = Gd.clone()
    S = la.chol_whiten_blocks(Gd, offs, 0.5, 0.5, LHS)
    assert S is not None
    S, L2 = S.cpu().numpy(), LHS.cpu().numpy()
    want_S, want_L = np.zeros_like(G), G.copy()
    for b, n in enumerate(sizes):
        sl = slice(offs[b], offs[b + 1])
        Ab = 0.5 * G[sl, sl] + 0.5 * np.eye(n)
        want_L[sl, sl] = Ab
        want_S[sl, sl] = np.linalg.inv(np.linalg.cholesky(Ab)).T
    np.testing.assert_array_equal(L2, want_L)
    np.testing.assert_allclose(S, want_S, rtol=0, atol=1e-13 * np.abs(want_S).max())
    W = S.T @ want_L @ S                                            # off-diagonal blocks untouched, diagonal blocks whitened
    for b in range(len(sizes)):
        sl = slice(offs[b], offs[b + 1])
        np.testing.assert_allclose(W[sl, sl], np.eye(sizes[b]), atol=1e-12)
    assert la.chol_whiten_blocks(Gd, offs, 1.0, -1e-3 * np.abs(G).max(), None) is None     # the largest block is rank deficient
    assert la.chol_whiten_blocks(torch.eye(137, dtype=torch.float64).cuda(), np.array([0, 137]), 1.0, 0.0) is None   # > one workgroup's LDS


def test_mcca_fit_is_deterministic():
    """Two fits of the same 8 views at the north-star size (D = 1024, k = 30: Chebyshev subspace iteration with locking, split-K
    products with a fixed-order reduce, Cholesky whitening) give the same bits: eigenvalues, loadings, transforms."""
    feats, labs = _north_star_mcca_inputs()
    a = A().AlignMCCA(n_components=30, regs=0.5)
    oa = a.fit_transform(feats, labs)
    b = A().AlignMCCA(n_components=30, regs=0.5)
    ob = b.fit_transform(feats, labs)
    np.testing.assert_array_equal(a.mcca.evals_, b.mcca.evals_)
    for x, y in zip(a.mcca.loadings_, b.mcca.loadings_):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(oa, ob):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


def test_mcca_cholesky_and_eigendecomposition_whitening_give_the_same_transforms():
    """The two reductions of the pencil (Cholesky factors, default; symmetric R_b^-1/2 by Jacobi, XPS_MCCA_WHITEN=eig) give the same
    eigenvalues and loadings to rounding."""
    from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
    pats = [make_patient(p, 96, T=40, C=32) for p in range(4)]
    feats, labs = [p[0] for p in pats], [p[1] for p in pats]
    a = A().AlignMCCA(n_components=10, regs=0.5)
    a.fit(feats, labs)
    from cross_patient_speech_decoding_amd import _switches
    b = A().AlignMCCA(n_components=10, regs=0.5)
    with _switches.override(XPS_MCCA_WHITEN='eig'):
        b.fit(feats, labs)
    np.testing.assert_allclose(a.mcca.evals_, b.mcca.evals_, rtol=1e-11, atol=1e-12)
    for la_, lb_ in zip(a.mcca.loadings_, b.mcca.loadings_):
        np.testing.assert_allclose(la_, lb_, rtol=0, atol=1e-9 * np.abs(lb_).max())


def _north_star_mcca_inputs():
    """Eight north-star patients (C = 128 channels, T = 200 samples, 64 shared conditions): 192 trials each --
    the condition-averaged views are the full 64 x 200 = 12 800 rows x 128 channels of the north-star fit (D = 1024);
    the trial count only sets how much noise the averages keep."""
    if not _north_star_views:
        from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
        pats = [make_patient(p, 192, T=200, C=128, n_cond=64) for p in range(8)]
        _north_star_views['d'] = ([x for x, _ in pats], [y for _, y in pats])
    return _north_star_views['d']


@pytest.mark.parametrize('pca_var', [1, 0.8])
def test_align_mcca_north_star_size_vs_oracle(pca_var):
    """north_star's "per-patient cross-covariance accumulation plus generalized eigensolve for MCCA" END TO END at its own
    size: 8 views x 128 channels, 64 shared conditions x 200 samples (12 800 x 1024), AlignMCCA(n_components=30, regs=0.5)
    as scripts/aligned_decode_svm_ncv.py:180-185 builds it, pca_var 1 and 0.8 (signal ranks from the raw data,
    alignment/AlignMCCA.py:146-150), against oracle/mcca_oracle.py (scipy.linalg.eigh on the 1024 x 1024 pencil): eigenvalues
    1e-9, loadings and transforms of every view 1e-6 up to the sign of a component, generalised-eigen residual and
    RHS-orthonormality of the device solution, and the block rows an 8-rank fit computes (one view per rank)
    assembled to the bits of the single-process Gram matrix and to the oracle's LHS.  Reference call site:
    alignment/AlignMCCA.py:140-154 (the third-party arithmetic itself stays parity-unpinned: DESIGN section 2)."""
    from cross_patient_speech_decoding_amd.alignment.AlignMCCA import DeviceMCCA
    la = LA()
    feats, labs = _north_star_mcca_inputs()
    k = 30
    ref = mo.get_mcca_transforms(feats, labs, n_components=k, regs=0.5, pca_var=pca_var)
    al = A().AlignMCCA(n_components=k, regs=0.5, pca_var=pca_var)
    out = al.fit_transform(feats, labs)
    assert len(al.mcca.loadings_) == 8 and al.mcca.block_rows_computed_ == list(range(8))
    if pca_var != 1:
        assert al.mcca.signal_ranks == ref.signal_ranks and max(ref.signal_ranks) < 30
    np.testing.assert_allclose(al.mcca.evals_, ref.evals_, rtol=1e-9, atol=1e-10)
    gaps = np.abs(np.diff(ref.evals_)) / np.abs(ref.evals_).max()
    assert gaps.min() > 2e-7, gaps.min()                 # (the comparison of eigenVECTORS below presumes simple eigenvalues)
    for i in range(8):
        assert al.mcca.loadings_[i].shape == (128, k)
        _match_up_to_sign(al.mcca.loadings_[i], ref.loadings_[i], 1e-6)
        np.testing.assert_allclose(al.mcca.means_[i], ref.means_[i], rtol=1e-12, atol=1e-12)
    # one sign per component for the whole solution (the sign rule acts on the common scores)
    V, Vr = np.vstack(al.mcca.loadings_), np.vstack(ref.loadings_)
    sg = np.sign((V * Vr).sum(0))
    assert np.abs(V * sg - Vr).max() <= 1e-6 * np.abs(Vr).max()
    for i in (0, 3, 7):
        exp = mo.mcca_transform(ref, feats[i][:16], i) * sg
        got = np.asarray(al.transform(feats[i][:16], idx=i))
        assert got.shape == (16, 200, k) and out[i].shape == (192, 200, k)
        assert np.abs(got - exp).max() <= 1e-6 * max(1.0, np.abs(exp).max())
        np.testing.assert_array_equal(np.asarray(out[i][:16]), got)
    # the pencil of the oracle, and the block rows of an 8-rank layout (rank r owns view r: ITS xps_xcov_f64 launches only)
    views = [a.reshape(-1, a.shape[-1]) for a in ao.extract_group_conditions(feats, labs)]
    assert views[0].shape == (12800, 128)
    cent = [v - v.mean(0) for v in views]
    Zc = np.concatenate(cent, axis=1)
    Gref = Zc.T @ Zc
    Vd = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in views]
    offs = np.arange(9) * 128
    Z = torch.cat(Vd, dim=1).contiguous()
    mean = torch.cat([la.col_mean(v) for v in Vd])
    rows = [None] * 8
    for r in range(8):
        own = DeviceMCCA.own_block_rows(Vd, Z, mean, offs, 8, r)
        assert [j for j, b in enumerate(own) if b is not None] == [r]
        rows[r] = own[r].cpu().numpy()
    G8 = np.concatenate(rows, axis=0)
    np.testing.assert_array_equal(G8, al.mcca.gram_)                         # 8-rank assembly == single-process matrix, bit for bit
    assert np.abs(G8 - Gref).max() <= 1e-10 * np.abs(Gref).max()
    assert np.abs(G8 - G8.T).max() <= 1e-10 * np.abs(Gref).max()
    if pca_var == 1:
        LHS, RHS = mo.mcca_gevp_blocks(cent, 0.5)
        np.testing.assert_allclose(LHS @ V, RHS @ V * al.mcca.evals_, atol=1e-8 * np.abs(LHS).max())
        np.testing.assert_allclose(V.T @ RHS @ V, np.eye(k), atol=1e-9)


def test_n_components_var_bug_compatible():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((500, 7, 6)) * np.array([5, 3, 2, 1, 0.5, 0.1])
    from cross_patient_speech_decoding_amd.alignment.AlignMCCA import n_components_var
    assert n_components_var(X, 0.8) == mo.n_components_var(X.reshape(-1, 6), 0.8)


# ------------------------------------------------------------------ kernels at BASELINE size
def test_xcov_and_jacobi_full_size_properties():
    la = LA()
    rng = np.random.default_rng(1)
    n, d = 409600, 128                               # one north-star patient: 2048 x 200 rows x 128 ch
    X = torch.from_numpy(rng.standard_normal((n, d), dtype=np.float32) @ np.diag(np.linspace(0.2, 3, d)).astype(np.float32))
    Xd = X.cuda()
    mean = la.col_mean(Xd)
    np.testing.assert_allclose(mean.cpu().numpy(), X.double().mean(0).numpy(), atol=1e-12)
    C = la.xcov(Xd, None, mean).cpu().numpy()
    ref = np.cov(X.double().numpy().T) * (n - 1)
    assert np.abs(C - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.abs(C - C.T).max() <= 1e-9 * np.abs(C).max()
    # determinism (split-K slabs, no atomics)
    assert np.array_equal(C, la.xcov(Xd, None, mean).cpu().numpy())
    w, V = la.eigh_psd(torch.from_numpy(C).cuda())
    wr = np.linalg.eigvalsh(ref)[::-1]
    np.testing.assert_allclose(w, wr, rtol=1e-10)
    np.testing.assert_allclose(V.T @ V, np.eye(d), atol=1e-12)
    np.testing.assert_allclose(V.T @ C @ V, np.diag(w), atol=1e-9 * w[0])


def test_jacobi_eigh_d1024_and_svd():
    la = LA()
    rng = np.random.default_rng(2)
    D = 1024                                         # north-star MCCA: 8 views x 128 channels
    Bm = rng.standard_normal((D, 300))
    C = Bm @ Bm.T + 0.5 * np.eye(D)
    w, V = la.eigh_psd(torch.from_numpy(C).cuda())
    np.testing.assert_allclose(w, np.linalg.eigvalsh(C)[::-1], rtol=1e-10)
    assert np.abs(V.T @ C @ V - np.diag(w)).max() <= 1e-9 * w[0]
    M = rng.standard_normal((37, 52))
    U, s, Vt = la.svd(torch.from_numpy(M).cuda())
    np.testing.assert_allclose(s, np.linalg.svd(M, compute_uv=False), rtol=1e-12)
    np.testing.assert_allclose((U * s) @ Vt, M, atol=1e-12)
    np.testing.assert_allclose(la.pinv_small(M), np.linalg.pinv(M), atol=1e-12)


@pytest.mark.parametrize('n', [1, 2, 7, 31, 96, 97, 128, 130])
def test_jacobi_single_workgroup_kernel(n):
    """The one-launch Jacobi (W, and V when it fits, in LDS): eigenpairs of PSD matrices incl. rank-deficient
    ones (V in LDS for n <= 96, V in global memory above), odd sizes, and the batched entry point -- given a list and given one
    (5, n, n) ndarray.  n = 130 is one past the one-workgroup kernel: the batch then takes one matrix at a time."""
    la = LA()
    rng = np.random.default_rng(n)
    Bm = rng.standard_normal((n, max(n // 2, 1)))             # rank n/2: the null space needs accumulated V
    C = Bm @ Bm.T
    w, V = la.eigh_psd(torch.from_numpy(C).cuda())
    wr = np.linalg.eigvalsh(C)[::-1]
    np.testing.assert_allclose(w, wr, atol=1e-10 * max(wr[0], 1e-300))
    np.testing.assert_allclose(V.T @ V, np.eye(n), atol=1e-12)
    np.testing.assert_allclose(V.T @ C @ V, np.diag(w), atol=1e-10 * max(wr[0], 1e-300))
    # well-conditioned shortcut (no accumulated rotations) and the batch of 5 matrices in one launch
    Cs = [Bm @ Bm.T * (1 + i) + 0.5 * np.eye(n) for i in range(5)]
    for batch in (Cs, np.stack(Cs)):
        for (w, V), Ci in zip(la.eigh_psd_batched(batch, well_conditioned=True), Cs):
            np.testing.assert_allclose(w, np.linalg.eigvalsh(Ci)[::-1], rtol=1e-11)
            np.testing.assert_allclose(V.T @ V, np.eye(n), atol=1e-11)
            np.testing.assert_allclose(V.T @ Ci @ V, np.diag(w), atol=1e-10 * w[0])


def test_eigh_sym_top_indefinite_matrix():
    la = LA()
    rng = np.random.default_rng(3)
    for n, k in ((200, 30), (64, 5)):
        A = rng.standard_normal((n, n))
        C = A + A.T                                            # indefinite
        w, V = la.eigh_sym_top(torch.from_numpy(C).cuda(), k)
        wr, Vr = np.linalg.eigh(C)
        np.testing.assert_allclose(w, wr[::-1][:k], atol=1e-10 * np.abs(wr).max())
        assert np.abs(C @ V - V * w).max() <= 1e-10 * np.abs(wr).max()


@pytest.mark.parametrize('n,k,kind', [(768, 10, 'mcca'), (1024, 30, 'mcca'), (800, 20, 'random'), (704, 12, 'clustered')])
def test_eigh_sym_top_subspace_iteration(n, k, kind):
    """Large n, few pairs: the Chebyshev-filtered subspace iteration (not the full Jacobi) must give the pairs LAPACK gives --
    MCCA-like spectra (a few large generalised correlations over a bulk, negative tail), a random indefinite matrix (small
    gaps) and a cluster of equal eigenvalues straddling position k."""
    la = LA()
    rng = np.random.default_rng(n + k)
    if kind == 'mcca':
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        lam = np.concatenate([np.linspace(6.5, 2.0, k + 5), rng.uniform(-1.0, 1.2, n - k - 5)])
        C = (Q * lam) @ Q.T
    elif kind == 'random':
        A = rng.standard_normal((n, n))
        C = A + A.T
    else:
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        lam = np.concatenate([np.linspace(9.0, 5.0, k - 3), np.full(6, 4.0), rng.uniform(-2.0, 3.0, n - k - 3)])
        C = (Q * lam) @ Q.T
    C = 0.5 * (C + C.T)
    st = {}
    w, V = la.eigh_sym_top(torch.from_numpy(C).cuda(), k, stats=st)
    assert 'outer' in st and not st.get('fallback'), f'the subspace path did not run / converge: {st}'
    wr = np.linalg.eigvalsh(C)[::-1]
    scale = np.abs(wr).max()
    np.testing.assert_allclose(w, wr[:k], atol=1e-11 * scale)
    assert np.abs(C @ V - V * w).max() <= 1e-11 * scale
    np.testing.assert_allclose(V.T @ V, np.eye(k), atol=1e-11)
    w2, V2 = la.eigh_sym_top(torch.from_numpy(C).cuda(), k)
    assert np.array_equal(w, w2) and np.array_equal(V, V2)          # reproducible run to run


def test_device_resident_inputs_stay_on_the_device(golden_dir):
    """A device tensor in -> a device tensor out (no PCIe round trip between alignment stages), same values as the ndarray path."""
    g = _load(golden_dir, 'align_cca.npz')
    Xa, ya, Xb, yb = (g[f'full_{k}'] for k in ('Xa', 'ya', 'Xb', 'yb'))
    al = A().AlignCCA()
    al.fit(torch.from_numpy(Xa).cuda(), torch.from_numpy(Xb).cuda(), ya, yb)
    out_d = al.transform(torch.from_numpy(Xb).cuda())
    assert isinstance(out_d, torch.Tensor) and out_d.is_cuda and out_d.dtype == torch.float64
    out_h = al.transform(Xb)
    assert isinstance(out_h, np.ndarray)
    np.testing.assert_array_equal(out_d.cpu().numpy(), out_h)
    rel = np.abs(out_h - g['full_b_to_a_t']).max() / np.abs(g['full_b_to_a_t']).max()
    assert rel <= 1e-6
    pca = A().PCA(0.95)
    Z = pca.fit(torch.from_numpy(Xa).cuda().reshape(-1, Xa.shape[-1])).transform(torch.from_numpy(Xa).cuda().reshape(-1, Xa.shape[-1]))
    assert Z.is_cuda
    np.testing.assert_array_equal(Z.cpu().numpy(), pca.transform(Xa.reshape(-1, Xa.shape[-1])))
    m = A().AlignMCCA(n_components=3, regs=0.5)
    m.fit([torch.from_numpy(Xa).cuda(), torch.from_numpy(Xb).cuda()], [ya, yb])
    t = m.transform(torch.from_numpy(Xb).cuda(), idx=1)
    assert t.is_cuda and tuple(t.shape) == Xb.shape[:2] + (3,)
    np.testing.assert_array_equal(t.cpu().numpy(), m.transform(Xb, idx=1))
