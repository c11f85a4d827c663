"""decoders.AlignedSVCSearchCV, the host side (no GPU): key splitting and its refusals for a bare and a bagged SVC, the dedupe of
``n_comp`` values that resolve to the same component counts (synthetic spectra), the planner's sharing of kernel matrices across
``C`` and of Gram matrices across ``gamma``, the chunk byte accounting, and the surface of the class."""
import numpy as np
import pytest
from sklearn.pipeline import make_pipeline

from cross_patient_speech_decoding_amd import alignment as A
from cross_patient_speech_decoding_amd import decoders as D
from cross_patient_speech_decoding_amd.alignment import PCA, AlignCCA, AlignMCCA
from cross_patient_speech_decoding_amd.alignment import fold_align as FA
from cross_patient_speech_decoding_amd.alignment._linalg import rbf_tiles
from cross_patient_speech_decoding_amd.decoders import aligned_search as AS
from cross_patient_speech_decoding_amd.decomposition import DimRedReshape


def _pool():
    rng = np.random.default_rng(0)
    return [(rng.standard_normal((9, 4, 6)), np.arange(9) % 3, np.arange(9) % 3)]


def _bare(**kw):
    return D.crossPtDecoder_sepAlign(_pool(), D.SVC(**kw), AlignCCA)


def _bagged(**kw):
    return D.crossPtDecoder_sepAlign(_pool(), D.BaggingClassifier(D.SVC(**kw), n_estimators=4, random_state=0), AlignCCA)


# ------------------------------------------------------------------------------------------------ keys
def test_exports():
    assert D.AlignedSVCSearchCV is AS.AlignedSVCSearchCV
    assert A.fit_folds_multi is FA.fit_folds_multi


def test_key_splitting_for_a_bare_and_a_bagged_svc():
    assert AS.split_params(_bare(), {'n_comp': 0.9, 'decoder__C': 10, 'decoder__gamma': 'scale'}) == {'n_comp': 0.9, 'C': 10, 'gamma': 'scale'}
    assert AS.split_params(_bare(), {}) == {}
    assert AS.split_params(_bagged(), {'decoder__estimator__C': 2.0, 'decoder__estimator__gamma': 1e-3, 'n_comp': 5}) == {
        'C': 2.0, 'gamma': 1e-3, 'n_comp': 5}
    assert AS.supported_keys(None) == ['n_comp', 'decoder__C', 'decoder__gamma']
    assert AS.supported_keys(object()) == ['n_comp', 'decoder__estimator__C', 'decoder__estimator__gamma']
    # gamma on a linear kernel is accepted and has no effect
    assert AS.split_params(_bare(kernel='linear'), {'decoder__gamma': 0.5}) == {'gamma': 0.5}
    assert AS.gamma_spec('linear', 0.5) is None and AS.gamma_spec('linear', 'scale') is None
    assert AS.gamma_spec('rbf', 'scale') == 'scale' and AS.gamma_spec('rbf', 1) == 1.0 and isinstance(AS.gamma_spec('rbf', 1), float)


@pytest.mark.parametrize('key', ['decoder__tol', 'decoder__kernel', 'decoder', 'tar_in_train', 'aligner', 'decoder__class_weight'])
def test_a_parameter_the_search_does_not_batch_names_the_supported_keys(key):
    with pytest.raises(ValueError, match=r"supported keys are \['n_comp', 'decoder__C', 'decoder__gamma'\]"):
        AS.split_params(_bare(), {key: 1})


@pytest.mark.parametrize('key', ['decoder__n_estimators', 'decoder__estimator', 'decoder__estimator__tol', 'decoder__max_samples'])
def test_the_same_for_a_bagged_svc(key):
    with pytest.raises(ValueError, match=r"supported keys are \['n_comp', 'decoder__estimator__C', 'decoder__estimator__gamma'\]"):
        AS.split_params(_bagged(), {key: 1})


def test_keys_that_are_no_parameters_raise_sklearns_error():
    for model, key in ((_bare(), 'decoder__estimator__C'), (_bagged(), 'decoder__C'), (_bare(), 'C'), (_bare(), 'n_components'),
                       (_bare(), 'decoder__dimredreshape__n_components')):
        with pytest.raises(ValueError, match='Invalid parameter'):
            AS.split_params(model, {key: 1})
        with pytest.raises(ValueError, match='Invalid parameter'):              # (and sklearn says the same of the model itself)
            model.set_params(**{key: 1})
    with pytest.raises(ValueError, match='C must be positive'):
        AS.split_params(_bare(), {'decoder__C': 0})


def test_the_model_is_checked_as_cross_val_decode_checks_it():
    X, y = np.zeros((12, 4, 5)), np.arange(12) % 3
    for model in (D.crossPtDecoder_sepDimRed(_pool(), D.SVC()), D.crossPtDecoder_sepAlign(_pool(), D.SVC(), AlignMCCA), D.SVC()):
        with pytest.raises(TypeError, match='decoders.SVC'):
            D.AlignedSVCSearchCV(model, {'n_comp': [3]}).fit(X, y)
    pipe = make_pipeline(DimRedReshape(PCA), D.SVC())
    with pytest.raises(NotImplementedError, match='pipeline'):
        D.AlignedSVCSearchCV(D.crossPtDecoder_sepAlign(_pool(), pipe, AlignCCA), {'n_comp': [3]}).fit(X, y)
    with pytest.raises(NotImplementedError, match='kernel'):
        D.AlignedSVCSearchCV(_bare(kernel='poly'), {'n_comp': [3]}).fit(X, y)
    with pytest.raises(ValueError, match='scoring'):
        D.AlignedSVCSearchCV(_bare(), {'n_comp': [3]}, scoring='f1').fit(X, y)
    with pytest.raises(ValueError, match='exactly one'):
        D.AlignedSVCSearchCV(_bare()).fit(X, y)
    with pytest.raises(ValueError, match='exactly one'):
        D.AlignedSVCSearchCV(_bare(), {'n_comp': [3]}, candidates=[{'n_comp': 3}]).fit(X, y)
    with pytest.raises(ValueError, match='supported keys'):
        D.AlignedSVCSearchCV(_bare(), candidates=[{'n_comp': 3}, {'decoder__tol': 1e-3}]).fit(X, y)
    with pytest.raises(ValueError, match='n_trials'):
        D.AlignedSVCSearchCV(_bare(), {'n_comp': [3]}).fit(X, np.stack([y, y], axis=1))


def test_predict_and_score_without_refit_raise_an_attribute_error_naming_best_estimator():
    search = D.AlignedSVCSearchCV(_bare(), {'n_comp': [3]}, refit=False)
    for use in (lambda: search.predict(np.zeros((2, 4, 5))), lambda: search.score(np.zeros((2, 4, 5)), [0, 1])):
        with pytest.raises(AttributeError, match='best_estimator_'):
            use()
    params = search.get_params(deep=False)
    assert sorted(params) == ['candidates', 'cv', 'max_kernel_bytes', 'model', 'param_grid', 'refit', 'scoring']
    assert params['cv'] == 5 and params['max_kernel_bytes'] == 2 ** 30 and params['scoring'] is None


# ------------------------------------------------------------------------------------------------ dedupe of n_comp
def _spectra():
    """Two folds of 6 channels and two pooled patients (5 and 4 channels) with geometric spectra: cumulative ratios are known."""
    fold = [np.array([32.0, 16, 8, 4, 2, 1]), np.array([32.0, 16, 8, 4, 2, 2])]         # sums 63 and 64
    pool = [np.array([16.0, 8, 4, 2, 1]), np.array([8.0, 4, 2, 2])]                     # sums 31 and 16
    return fold, [200, 190], 6, pool, [(300, 5), (260, 4)]


def test_resolve_counts_applies_the_pca_rule_to_every_spectrum():
    fold, rows, C, pool, shapes = _spectra()
    # 0.8: fold 0 cumulative 32/63 = .508, 48/63 = .762, 56/63 = .889 -> 3; fold 1: .5, .75, .875 -> 3; pools 16/31, 24/31 = .774, 28/31 -> 3; .5, .75, .875 -> 3
    assert FA.resolve_counts(0.8, fold, rows, C, pool, shapes) == ((3, 3), (3, 3))
    assert FA.resolve_counts(0.76, fold, rows, C, pool, shapes) == ((2, 3), (2, 3))
    assert FA.resolve_counts(4, fold, rows, C, pool, shapes) == ((4, 4), (4, 4))
    assert FA.resolve_counts(5, fold, rows, C, pool, shapes) == ((5, 5), (5, 4))        # an int is capped at the channels
    assert FA.resolve_counts(None, fold, rows, C, pool, shapes) == ((6, 6), (5, 4))
    # negative eigenvalues of a Jacobi run are clipped before the ratio is taken, as alignment.PCA does
    assert FA.resolve_counts(0.8, [np.array([32.0, 16, 8, 4, 2, -1e-18])] * 2, rows, C, pool, shapes)[0] == (3, 3)


def test_values_that_resolve_to_the_same_counts_are_one_fit():
    fold, rows, C, pool, shapes = _spectra()
    values = [0.8, 0.95, 3, 0.8, 0.85, 0.76, 0.97]
    counts = [FA.resolve_counts(v, fold, rows, C, pool, shapes) for v in values]
    assert counts[0] == counts[2] == counts[3] == counts[4] and counts[1] != counts[0] and counts[5] != counts[0]
    index, firsts = FA.distinct_counts(values, fold, rows, C, pool, shapes)
    assert firsts == [0, 1, 5] + ([6] if counts[6] != counts[1] else [])
    assert index[:6] == [0, 1, 0, 0, 0, 2]
    for i, j in enumerate(index):
        assert counts[firsts[j]] == counts[i]
    # the pooled patients' counts belong to the key: equal fold counts alone do not share a fit
    a = FA.resolve_counts(4, fold, rows, C, pool, shapes)
    b = FA.resolve_counts(4, fold, rows, C, [pool[0][:3], pool[1]], [(300, 3), (260, 4)])
    assert a[0] == b[0] and a != b
    assert FA.distinct_counts([], fold, rows, C, pool, shapes) == ([], [])


# ------------------------------------------------------------------------------------------------ the planner
def _settings(grid):
    return [dict(C=float(C), gamma=AS.gamma_spec('rbf', g)) for C, g in grid]


def _gamma_of(a, f, spec):
    return 0.01 * (1 + a) + 0.001 * f if spec == 'scale' else spec


ROWS = [[100, 101, 99], [100, 101, 99]]                            # rows_of[alignment][fold]


def test_matrices_are_shared_across_C_and_grams_across_gamma():
    grid = [(C, g) for C in (1, 10, 100) for g in ('scale', 1e-4)]
    settings = _settings(grid) * 2                                  # 12 candidates: the 6 settings on alignment 0, then on alignment 1
    align_of = [0] * 6 + [1] * 6
    plan = AS.build_plan(settings, align_of, ROWS, 'rbf', _gamma_of)
    assert plan.views == [(a, f) for a in (0, 1) for f in range(3)] and plan.rows == ROWS[0] + ROWS[1]
    assert len(plan.matrices) == 6 * 2 and len(plan.models) == 12 * 3
    for v in range(6):                                              # two gammas per view, adjacent
        assert [view for view, _ in plan.matrices[2 * v:2 * v + 2]] == [v, v]
        a, f = plan.views[v]
        assert [g for _, g in plan.matrices[2 * v:2 * v + 2]] == [_gamma_of(a, f, 'scale'), 1e-4]
    for mod in plan.models:
        a, f = plan.views[mod['view']]
        assert align_of[mod['cand']] == a and mod['fold'] == f and plan.matrices[mod['matrix']][0] == mod['view']
        assert mod['C'] == settings[mod['cand']]['C']
        assert plan.matrices[mod['matrix']][1] == _gamma_of(a, f, settings[mod['cand']]['gamma'])
    for m in range(len(plan.matrices)):                             # three values of C on every matrix
        assert sorted(mod['C'] for mod in plan.models if mod['matrix'] == m) == [1.0, 10.0, 100.0]
    assert sorted((mod['cand'], mod['fold']) for mod in plan.models) == [(c, f) for c in range(12) for f in range(3)]
    assert AS.scale_views(settings, align_of, 3, 'rbf') == plan.views
    assert AS.scale_views(settings[1::2], [0, 0, 0, 1, 1, 1], 3, 'rbf') == []
    assert AS.scale_views(_settings([(1, 'scale'), (1, 0.1)]), [1, 0], 3, 'rbf') == [(1, 0), (1, 1), (1, 2)]
    assert AS.scale_views(settings, align_of, 3, 'linear') == []
    # two spellings of one value are one matrix
    same = AS.build_plan(_settings([(1, 0.5), (2, 0.5), (3, 1 / 2)]), [0, 0, 0], [[10]], 'rbf', _gamma_of)
    assert same.matrices == [(0, 0.5)] and [mod['matrix'] for mod in same.models] == [0, 0, 0]


def test_a_linear_kernel_has_one_matrix_per_view_whatever_gamma_says():
    settings = [dict(C=1.0, gamma=AS.gamma_spec('linear', g)) for g in ('scale', 0.1, 5)]
    plan = AS.build_plan(settings, [0, 0, 1], ROWS, 'linear', None)
    assert plan.matrices == [(v, None) for v in range(6)]
    assert [(mod['cand'], mod['view']) for mod in plan.models] == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 3), (2, 4), (2, 5)]


def test_chunk_bytes_count_a_views_gram_while_any_of_its_matrices_is_in_the_chunk():
    settings = _settings([(1, 0.1), (1, 0.2), (1, 0.3)])
    plan = AS.build_plan(settings, [0, 0, 0], [[10, 20]], 'rbf', _gamma_of)
    assert plan.matrices == [(0, 0.1), (0, 0.2), (0, 0.3), (1, 0.1), (1, 0.2), (1, 0.3)]
    small, large = 8 * 10 ** 2, 8 * 20 ** 2
    assert plan.matrix_bytes() == [small] * 3 + [large] * 3
    assert AS.chunk_bytes(plan, [0, 1, 2], True) == 4 * small and AS.chunk_bytes(plan, [0, 1, 2], False) == 3 * small
    assert AS.chunk_bytes(plan, [2, 3], True) == 2 * small + 2 * large and AS.chunk_bytes(plan, [3, 4], True) == 3 * large
    assert AS.cut_plan_chunks(plan, True, 2 ** 30) == [[0, 1, 2, 3, 4, 5]]
    assert AS.cut_plan_chunks(plan, True, 4 * small + 4 * large) == [[0, 1, 2, 3, 4, 5]]
    assert AS.cut_plan_chunks(plan, True, 4 * small + 4 * large - 1) == [[0, 1, 2, 3, 4], [5]]
    assert AS.cut_plan_chunks(plan, True, 3 * large) == [[0, 1, 2, 3], [4, 5]]        # (4 small + 2 large = 3 large: it just fits)
    assert AS.cut_plan_chunks(plan, True, 3 * large - 1) == [[0, 1, 2], [3], [4], [5]]  # (two large and their Gram: 3 large)
    assert AS.cut_plan_chunks(plan, False, 3 * large) == [[0, 1, 2, 3, 4], [5]]
    assert AS.cut_plan_chunks(plan, True, large) == [[0, 1, 2], [3], [4], [5]]        # one matrix and its Gram are always taken
    assert AS.cut_plan_chunks(plan, False, large) == [[0, 1, 2], [3], [4], [5]]
    for rbf in (True, False):
        with pytest.raises(ValueError, match=f'max_kernel_bytes={large - 1} is too small'):
            AS.cut_plan_chunks(plan, rbf, large - 1)
        chunks = AS.cut_plan_chunks(plan, rbf, 2 * large)
        assert [m for ch in chunks for m in ch] == list(range(6))


def test_rbf_tiles_list_every_tile_of_every_problem():
    t = rbf_tiles([130, 0, 64, 1])
    assert t.dtype == np.int32
    assert t.tolist() == [[0, i, j] for i in range(3) for j in range(3)] + [[2, 0, 0], [3, 0, 0]]
    assert rbf_tiles([]).shape == (0, 3) and rbf_tiles([0]).shape == (0, 3)
