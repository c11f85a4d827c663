"""SVCSearchCV(batch_pca=True) and alignment.PCA(solver=...), the host side (no GPU): the cut r and the gamma of a fold from its
Gram-side spectrum against sklearn's PCA fitted on the fold, the batched-or-fallback decision at its edges, key splitting and every
refusal, and the algebra the device path rests on -- Kc and Z restated in numpy -- against sklearn's transform."""
import numpy as np
import pytest
from sklearn.base import clone
from sklearn.decomposition import PCA as SkPCA
from sklearn.model_selection import StratifiedKFold
from sklearn.pipeline import make_pipeline

import cross_patient_speech_decoding_amd.alignment as A
from cross_patient_speech_decoding_amd.alignment import pca as P
from cross_patient_speech_decoding_amd.decoders import SVC, SVCSearchCV, _ovo
from cross_patient_speech_decoding_amd.decoders import search as S
from cross_patient_speech_decoding_amd.decomposition import DimRedReshape, NoCenterPCA
from cross_patient_speech_decoding_amd.utils.synthetic import make_patient

NCS = [0.3, 0.5, 0.8, 0.95, 5]


def recipe_a(shift=0.0):
    X, y_full = make_patient(0, 60, T=10, C=8, n_cond=12, k=4)
    F = X.reshape(60, -1).astype(np.float64) + shift
    y = y_full[:, 0]
    return F, y, list(StratifiedKFold(3).split(F, y))


def fold_algebra(F, tr, te):
    """The device path's algebra in float64 numpy: G about the all-trial mean, Kc of the fold's rows (training rows first) about the
    mean of its training rows, the spectrum of its training block, and the scores Z = Kc U L^-1/2 of all its rows."""
    Fc = F - F.mean(axis=0)
    G = Fc @ Fc.T
    rows = np.concatenate([tr, te])
    n_tr = len(tr)
    m = G[np.ix_(rows, tr)].sum(axis=1) / n_tr
    mm = m[:n_tr].sum() / n_tr
    Kc = G[np.ix_(rows, tr)] - m[:, None] - m[None, :n_tr] + mm
    L, U = np.linalg.eigh(0.5 * (Kc[:n_tr] + Kc[:n_tr].T))
    L, U = L[::-1], U[:, ::-1]
    return Kc, L, U


@pytest.mark.parametrize('shift', [0.0, 50.0])
def test_cut_and_gamma_from_the_spectrum_equal_sklearns_pca_fitted_on_the_fold(shift):
    F, y, splits = recipe_a(shift)
    d = F.shape[1]
    for tr, te in splits:
        _, L, _ = fold_algebra(F, tr, te)
        for nc in NCS:
            sk = SkPCA(n_components=nc, svd_solver='full').fit(F[tr])
            r, batched = S.pca_cut(L, nc, len(tr), d)
            assert r == sk.n_components_ and batched
            Ztr = sk.transform(F[tr])
            want = _ovo.gamma_value('rbf', 'scale', Ztr)
            got = S.pca_gamma('rbf', 'scale', L, r, len(tr))
            assert abs(got - want) <= 1e-9 * want
            assert S.pca_gamma('rbf', 'auto', L, r, len(tr)) == _ovo.gamma_value('rbf', 'auto', Ztr) == 1.0 / r
            assert S.pca_gamma('rbf', 0.01, L, r, len(tr)) == 0.01
            assert S.pca_gamma('linear', 'scale', L, r, len(tr)) == 0.0
    with pytest.raises(ValueError, match='scale'):
        S.pca_gamma('rbf', 'nope', L, 2, len(tr))
    with pytest.raises(ValueError, match='non-negative'):
        S.pca_gamma('rbf', -1.0, L, 2, len(tr))


def test_a_pair_is_batched_up_to_the_rank_of_the_training_rows_and_the_spectrum_limit():
    L = np.array([10.0, 5.0, 2.0, 1.0, 0.5, 0.0])                         # six training rows: rank five
    assert S.pca_cut(L, 5, 6, 40) == (5, True)                           # r = n_tr - 1
    assert S.pca_cut(L, 6, 6, 40) == (6, False)                          # r = n_tr
    assert S.pca_cut(L, None, 6, 40) == (None, False)
    assert S.pca_cut(L, 4, 6, 3) == (3, True)                            # the class's rule clamps r to the feature count
    assert S.pca_cut(L, 0.5, 6, 40) == (1, True)                         # 10 / 18.5 = 0.54 > 0.5
    assert S.pca_cut(L, 0.6, 6, 40) == (2, True)                         # 15 / 18.5 = 0.81 > 0.6
    assert P.PCA_SPECTRUM_LIMIT == 1e6 and A.PCA_SPECTRUM_LIMIT == 1e6
    edge = np.array([1e6, 1.0, 0.5, 0.0])
    assert S.pca_cut(edge, 2, 4, 40) == (2, True)                        # exactly L_0 / limit
    assert S.pca_cut(edge, 3, 4, 40) == (3, False)                       # below it
    assert S.pca_cut(np.array([1e6, np.nextafter(1.0, 0.0), 0.0]), 2, 3, 40) == (2, False)
    assert S.pca_cut(np.zeros(4), 1, 4, 40) == (1, False)                # constant rows: nothing to cut
    assert S.pca_cut(np.array([3.0, 1.0, -1e-17]), 2, 3, 40) == (2, True)    # a rounded-off zero below 0 is clipped


def test_the_component_count_rule_is_one_function():
    ratio = np.array([0.5, 0.3, 0.15, 0.05])
    assert [P.count_components(nc, ratio, 9, 4) for nc in (None, 0.5, 0.79, 0.8, 0.99, 3, 7)] == [4, 2, 2, 3, 4, 3, 4]
    np.testing.assert_array_equal(P.gram_ratio([6.0, 2.0, -1.0, 0.0], 4, 9), [0.75, 0.25, 0.0, 0.0])
    np.testing.assert_array_equal(P.gram_ratio([6.0, 2.0, 1.0], 3, 2), [0.75, 0.25])       # min(n, d) leading values
    np.testing.assert_array_equal(P.gram_ratio([0.0, 0.0], 2, 5), [0.0, 0.0])


def test_the_sign_rule_is_one_function():
    #             largest |.| negative   exact tie: first wins   all zero
    M = np.array([[1.0,                  -2.0,                   0.0],
                  [-3.0,                 2.0,                    0.0],
                  [2.0,                  -2.0,                   0.0]])
    np.testing.assert_array_equal(P.sign_rule(M, 0), [-1.0, -1.0, 1.0])          # down the columns
    np.testing.assert_array_equal(P.sign_rule(M.T.copy(), 1), [-1.0, -1.0, 1.0])   # the same vectors as rows
    np.testing.assert_array_equal(P.sign_rule(np.array([[2.0, -2.0, 1.0]]), 1), [1.0])     # the tie the other way round
    signed = M * P.sign_rule(M, 0)
    assert signed[1, 0] == 3.0 and signed[0, 1] == 2.0 and not signed[:, 2].any()


def test_keys_are_split_with_n_components_batched_and_everything_else_refused():
    pipe = make_pipeline(DimRedReshape(A.PCA), SVC(kernel='rbf'))
    got = S.split_params_pca(pipe, {'svc__C': 5, 'svc__gamma': 0.2, 'dimredreshape__n_components': 0.9})
    assert got == ({'C': 5, 'gamma': 0.2, 'n_components': 0.9}, {})
    assert S.split_params_pca(pipe, {'svc__C': 5}) == ({'C': 5}, {})
    assert S.split_params_pca(pipe, {'dimredreshape__n_components': None}) == ({'n_components': None}, {})
    named = type(pipe)([('reduce', DimRedReshape(A.GramPCA)), ('clf', SVC())])
    assert S.split_params_pca(named, {'reduce__n_components': 3, 'clf__gamma': 'auto'}) == ({'gamma': 'auto', 'n_components': 3}, {})
    for other in ({'dimredreshape__dim_red': A.GramPCA}, {'dimredreshape': DimRedReshape(A.PCA)}):
        with pytest.raises(ValueError, match='C and gamma only'):
            S.split_params_pca(pipe, {**other, 'svc__C': 1})
    with pytest.raises(ValueError, match='C and gamma only'):
        S.split_params_pca(pipe, {'svc__kernel': 'linear'})
    with pytest.raises(ValueError, match='Invalid parameter'):
        S.split_params_pca(pipe, {'n_components': 3})
    assert S.split_params(pipe, {'dimredreshape__n_components': 0.9}) == ({}, {'dimredreshape__n_components': 0.9})   # the default route


def test_batch_pca_refuses_every_other_estimator_before_it_touches_the_device():
    X, y = np.zeros((12, 3, 2)), np.arange(12) % 2
    grid = {'svc__C': [1.0]}
    bad = [SVC(),
           make_pipeline(DimRedReshape(SkPCA), SVC()),
           make_pipeline(DimRedReshape(NoCenterPCA), SVC()),
           make_pipeline(DimRedReshape(A.PCA(3)), SVC()),                 # an instance, not the class DimRedReshape builds from
           make_pipeline(DimRedReshape(A.PCA), DimRedReshape(A.PCA), SVC()),
           make_pipeline(A.PCA(), SVC())]
    for est in bad:
        with pytest.raises(ValueError, match='batch_pca=True needs'):
            SVCSearchCV(est, grid if not isinstance(est, SVC) else {'C': [1.0]}, cv=2, batch_pca=True).fit(X, y)
    for ok in (A.PCA, A.GramPCA):
        assert S.pca_step_of(make_pipeline(DimRedReshape(ok), SVC()))[0] == 'dimredreshape'
    search = SVCSearchCV(make_pipeline(DimRedReshape(A.GramPCA), SVC()), grid, batch_pca=True)
    assert search.get_params()['batch_pca'] is True and clone(search).batch_pca is True
    assert SVCSearchCV(SVC(), {'C': [1.0]}).batch_pca is False            # the default is today's path


def test_pca_carries_its_solver_through_get_params_and_clone():
    assert A.PCA(0.5).get_params() == {'n_components': 0.5, 'solver': 'covariance'}
    assert A.GramPCA(0.5).get_params() == {'n_components': 0.5, 'solver': 'auto'}
    assert issubclass(A.GramPCA, A.PCA)
    for est in (A.PCA(3, solver='gram'), A.GramPCA(0.9), A.GramPCA(2, solver='covariance')):
        twin = clone(est)
        assert type(twin) is type(est) and twin.get_params() == est.get_params()
    assert DimRedReshape(A.GramPCA, n_components=0.8).dim_red(n_components=0.8).solver == 'auto'


@pytest.mark.parametrize('shift', [0.0, 50.0])
def test_the_numpy_restatement_of_kc_and_z_gives_sklearns_scores_of_training_and_held_out_rows(shift):
    F, y, splits = recipe_a(shift)
    for tr, te in splits:
        Kc, L, U = fold_algebra(F, tr, te)
        R = 12
        Z = Kc @ (U[:, :R] / np.sqrt(L[:R]))
        sk = SkPCA(n_components=R, svd_solver='full').fit(F[tr])
        want = sk.transform(F[np.concatenate([tr, te])])
        flip = np.sign((Z[:len(tr)] * want[:len(tr)]).sum(axis=0))
        assert np.abs(Z * flip - want).max() <= 1e-9 * np.abs(want).max()
        np.testing.assert_allclose(L[:R] / (len(tr) - 1), sk.explained_variance_, rtol=1e-10)
        np.testing.assert_allclose((Z[:len(tr)] ** 2).sum(axis=0), L[:R], rtol=1e-10)         # squared norms L_i ...
        assert np.abs(Z[:len(tr)].sum(axis=0)).max() <= 1e-9 * np.sqrt(L[0])                    # ... and zero mean: the 'scale' identity
        for r in (1, 5, R):                                               # a prefix of the columns is the PCA with fewer components
            D2 = ((want[:, None, :r] - want[None, :, :r]) ** 2).sum(axis=2)
            Zr = Z[:, :r]
            sq = (Zr * Zr).sum(axis=1)
            assert np.abs(sq[:, None] + sq[None, :] - 2 * Zr @ Zr.T - D2).max() <= 1e-9 * D2.max()
