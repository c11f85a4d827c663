"""decoders.SVCSearchCV, the host side (no GPU): candidate expansion and key splitting, the per-fold problem builder against a
restatement of decoders.SVC.fit's construction, scores from confusion tables against sklearn.metrics, the cv_results_ assembly
against GridSearchCV fed the same scores, and the chunk cutter."""
import numpy as np
import pytest
from sklearn.decomposition import PCA
from sklearn.metrics import accuracy_score, balanced_accuracy_score
from sklearn.model_selection import GridSearchCV, ParameterGrid, PredefinedSplit, StratifiedKFold
from sklearn.pipeline import make_pipeline
from sklearn.svm import SVC as SkSVC

from cross_patient_speech_decoding_amd.decoders import SVC, SVCSearchCV
from cross_patient_speech_decoding_amd.decoders import search as S
from cross_patient_speech_decoding_amd.decoders.svm import _class_weights
from cross_patient_speech_decoding_amd.decomposition import DimRedReshape


# ------------------------------------------------------------------------------------------------ candidates and keys
def test_candidates_are_parameter_grids_in_its_order_or_the_explicit_list():
    grid = [{'C': [10, 0.1, 1], 'gamma': ['scale', 0.5]}, {'C': [3.0]}]
    assert S.expand_candidates(grid, None) == list(ParameterGrid(grid))
    explicit = [{'gamma': 0.5, 'C': 2}, {'C': 1}, {'gamma': 0.5, 'C': 2}]
    assert S.expand_candidates(None, explicit) == explicit
    assert S.expand_candidates(None, iter(explicit)) == explicit
    for bad in ((None, None), (grid, explicit)):
        with pytest.raises(ValueError, match='exactly one'):
            S.expand_candidates(*bad)
    with pytest.raises(ValueError, match='no candidates'):
        S.expand_candidates(None, [])


def test_keys_are_split_into_batched_and_outer():
    bare = SVC(kernel='rbf')
    assert S.split_params(bare, {'C': 2.0, 'gamma': 'scale'}) == ({'C': 2.0, 'gamma': 'scale'}, {})
    assert S.split_params(bare, {'gamma': 0.1}) == ({'gamma': 0.1}, {})
    assert S.split_params(bare, {}) == ({}, {})
    pipe = make_pipeline(DimRedReshape(PCA), SVC(kernel='rbf'))
    got = S.split_params(pipe, {'svc__C': 5, 'svc__gamma': 0.2, 'dimredreshape__n_components': 0.9})
    assert got == ({'C': 5, 'gamma': 0.2}, {'dimredreshape__n_components': 0.9})
    assert S.split_params(pipe, {'dimredreshape__dim_red': PCA}) == ({}, {'dimredreshape__dim_red': PCA})
    svc, prefix, pre = S.svc_of(pipe)
    assert svc is pipe.steps[-1][1] and prefix == 'svc__' and [name for name, _ in pre] == ['dimredreshape']
    assert S.svc_of(bare) == (bare, '', None)


@pytest.mark.parametrize('key', ['kernel', 'tol', 'class_weight', 'max_iter', 'decision_function_shape'])
def test_other_svc_keys_are_refused(key):
    with pytest.raises(ValueError, match='C and gamma only'):
        S.split_params(SVC(), {'C': 1.0, key: SVC().get_params()[key]})
    pipe = make_pipeline(DimRedReshape(PCA), SVC())
    with pytest.raises(ValueError, match='C and gamma only'):
        S.split_params(pipe, {'svc__' + key: SVC().get_params()[key]})


def test_unknown_keys_wrong_estimators_and_unsupported_settings_are_refused():
    pipe = make_pipeline(DimRedReshape(PCA), SVC())
    with pytest.raises(ValueError, match='Invalid parameter'):
        S.split_params(SVC(), {'nope': 1})
    with pytest.raises(ValueError, match='Invalid parameter'):
        S.split_params(pipe, {'C': 1})                                    # a bare key does not address a pipeline's SVC
    with pytest.raises(ValueError, match='replaces the searched SVC'):
        S.split_params(pipe, {'svc': SVC()})
    for est in (SkSVC(), make_pipeline(DimRedReshape(PCA), SkSVC()), None):
        with pytest.raises(TypeError, match='decoders.SVC'):
            S.svc_of(est)
    X, y = np.zeros((6, 2)), np.array([0, 1] * 3)
    with pytest.raises(NotImplementedError, match='fit parameters'):
        SVCSearchCV(SVC(), {'C': [1]}).fit(X, y, sample_weight=np.ones(6))
    with pytest.raises(NotImplementedError, match='return_train_score'):
        SVCSearchCV(SVC(), {'C': [1]}, return_train_score=True).fit(X, y)
    with pytest.raises(NotImplementedError, match='error_score'):
        SVCSearchCV(SVC(), {'C': [1]}, error_score=0.0).fit(X, y)
    with pytest.raises(NotImplementedError, match='kernel'):
        SVCSearchCV(SVC(kernel='poly'), {'C': [1]}).fit(X, y)
    with pytest.raises(ValueError, match='scoring'):
        SVCSearchCV(SVC(), {'C': [1]}, scoring='f1').fit(X, y)
    with pytest.raises(ValueError, match='C and gamma only'):
        SVCSearchCV(SVC(), {'C': [1], 'tol': [1e-3]}).fit(X, y)


def test_both_searches_share_one_tail():
    """``search.SearchTail``: the same ``scoring`` refusal, the ``AttributeError`` naming the concrete class, ``decision_function``
    on ``SVCSearchCV`` alone, and the class-count refusals of ``check_class_count``."""
    from cross_patient_speech_decoding_amd.alignment import AlignCCA
    from cross_patient_speech_decoding_amd.decoders import AlignedSVCSearchCV, crossPtDecoder_sepAlign
    pool = [(np.zeros((9, 4, 6)), np.arange(9) % 3, np.arange(9) % 3)]
    plain = SVCSearchCV(SVC(), {'C': [1]}, scoring='f1', refit=False)
    aligned = AlignedSVCSearchCV(crossPtDecoder_sepAlign(pool, SVC(), AlignCCA), {'n_comp': [3]}, scoring='f1', refit=False)
    assert isinstance(plain, S.SearchTail) and isinstance(aligned, S.SearchTail)
    assert type(plain).predict is type(aligned).predict is S.SearchTail.predict and type(plain).score is type(aligned).score
    message = r"^scoring must be None, 'accuracy' or 'balanced_accuracy'; got 'f1'$"
    with pytest.raises(ValueError, match=message):
        plain.fit(np.zeros((6, 2)), np.array([0, 1] * 3))
    with pytest.raises(ValueError, match=message):
        aligned.fit(np.zeros((12, 4, 5)), np.arange(12) % 3)
    for search, X in ((plain, np.zeros((2, 2))), (aligned, np.zeros((2, 4, 5)))):
        name = type(search).__name__
        for use in (lambda: search.predict(X), lambda: search.score(X, [0, 1])):
            with pytest.raises(AttributeError, match=f'^this {name} has no best_estimator_: it was not fitted, or refit=False$'):
                use()
    with pytest.raises(AttributeError, match='^this SVCSearchCV has no best_estimator_'):
        plain.decision_function(np.zeros((2, 2)))
    assert not hasattr(aligned, 'decision_function')
    with pytest.raises(ValueError, match='^The number of classes has to be greater than one; got 1 class$'):
        S.check_class_count(1)
    with pytest.raises(ValueError, match=r'^the scoring kernel takes 2\.\.64 classes; got 65$'):
        S.check_class_count(65)
    assert S.check_class_count(2) is None and S.check_class_count(64) is None
    with pytest.raises(ValueError, match=r'^the scoring kernel takes 2\.\.64 classes; got 65$'):
        SVCSearchCV(SVC(), {'C': [1]}).fit(np.zeros((130, 2)), np.arange(130) % 65)


# ------------------------------------------------------------------------------------------------ the problem builder
def svc_fit_construction(svc, X, y):
    """What decoders.SVC.fit builds from the X / y it is handed (no sample weights): the lines of its fit, restated."""
    gamma = svc._gamma_value(X)
    classes, yi = np.unique(y, return_inverse=True)
    cw = _class_weights(svc.class_weight, classes, yi)
    k = len(classes)
    if k < 2:
        raise ValueError('The number of classes has to be greater than one; got 1 class')
    members = [np.flatnonzero(yi == c).astype(np.int32) for c in range(k)]
    idx, off, npos, pairs = [], [0], [], []
    for a in range(k):
        for b in range(a + 1, k):
            idx += [members[a], members[b]]
            off.append(off[-1] + len(members[a]) + len(members[b]))
            npos.append(len(members[a]))
            pairs.append((classes[a], classes[b]))
    idx = np.concatenate(idx)
    cb = float(svc.C) * cw[yi[idx]] * np.ones(len(y))[idx]
    return gamma, idx, np.asarray(off), np.asarray(npos), pairs, cb


def search_data(sizes=(30, 28, 2), d=5, seed=3):
    rng = np.random.default_rng(seed)
    y = np.repeat([1, 4, 7][:len(sizes)], sizes)
    X = rng.standard_normal((len(y), d)) + y[:, None] * 0.3
    perm = rng.permutation(len(y))
    return X[perm], y[perm]


@pytest.mark.parametrize('class_weight', [None, 'balanced', {4: 2.5}])
def test_problem_builder_matches_svc_fit_fold_by_fold(class_weight):
    """Class sizes 30 / 28 / 2 on 4 unstratified folds: at least one fold loses the class of two points."""
    X, y = search_data()
    classes, yi = np.unique(y, return_inverse=True)
    rng = np.random.default_rng(0)
    order = np.concatenate([np.flatnonzero(y == 7), rng.permutation(np.flatnonzero(y != 7))])    # the first fold holds out all of class 7
    splits =[(np.sort(np.setdiff1d(order, part))[::-1].copy(), np.sort(part)) for part in np.array_split(order, 4)]   # train descending
    est = SVC(kernel='rbf', class_weight=class_weight, C=1.0)
    cands = [{'C': 0.5, 'gamma': 'scale'}, {'C': 4.0, 'gamma': 0.25}, {'C': 4.0, 'gamma': 'scale'}, {'gamma': 'auto'}]
    plan = S.build_plan(est, [S.split_params(est, c) for c in cands], X, yi, classes, splits)
    assert len(plan.views) == 1 and plan.views[0].shape == X.shape
    assert len(plan.models) == len(cands) * len(splits)
    lost = 0
    for mod in plan.models:
        tr, te = splits[mod['fold']]
        cand = cands[mod['cand']]
        gamma, idx, off, npos, pairs, cb = svc_fit_construction(SVC(kernel='rbf', class_weight=class_weight).set_params(**cand), X[tr], y[tr])
        p = mod['problems']
        lost += len(pairs) < 3
        np.testing.assert_array_equal(p['idx'], tr[idx])                  # training indices mapped into the view (the whole X)
        assert p['idx'].dtype == np.int32
        np.testing.assert_array_equal(np.concatenate([[0], np.cumsum(p['sizes'])]), off)
        np.testing.assert_array_equal(p['npos'], npos)
        assert [(classes[a], classes[b]) for a, b in zip(p['pair_a'], p['pair_b'])] == pairs
        assert (p['pair_a'] < p['pair_b']).all()
        np.testing.assert_array_equal(mod['C'] * p['weight'], cb)         # bit for bit
        assert plan.matrices[mod['matrix']] == (0, gamma)                 # the fold's own 'scale' / 'auto' / number
        np.testing.assert_array_equal(mod['test_pos'], te)
        np.testing.assert_array_equal(classes[mod['ytest']], y[te])
    assert lost >= len(cands)                                             # a fold that lost a class was among them
    n_scale = len({plan.matrices[m['matrix']][1] for m in plan.models if cands[m['cand']].get('gamma') == 'scale'})
    assert n_scale == len(splits)                                         # gamma='scale' is per fold; C does not add matrices
    assert len(plan.matrices) == len(splits) + 2 and plan.matrix_bytes() == [8 * len(y) ** 2] * len(plan.matrices)


def test_a_single_class_fold_raises_sklearns_error():
    X, y = search_data()
    classes, yi = np.unique(y, return_inverse=True)
    one = np.flatnonzero(y == 1)
    splits = [(one, np.flatnonzero(y != 1))]
    est = SVC(kernel='linear')
    with pytest.raises(ValueError, match='The number of classes has to be greater than one; got 1 class'):
        S.build_plan(est, [S.split_params(est, {'C': 1.0})], X, yi, classes, splits)
    with pytest.raises(ValueError, match='greater than one'):
        SVCSearchCV(est, {'C': [1.0]}, cv=splits).fit(X, y)
    with pytest.raises(ValueError, match='greater than one'):
        SVCSearchCV(est, {'C': [1.0]}, cv=2).fit(X[one], y[one])


def test_pipeline_views_hold_the_transformed_training_rows_then_the_held_out_rows():
    """A host-only pipeline (sklearn's PCA behind DimRedReshape): one view per (outer combination, fold), the earlier steps fitted
    once for each, the training indices mapped to 0 .. n_train - 1 and the held-out rows behind them."""
    rng = np.random.default_rng(2)
    y = np.arange(40) % 3
    X = rng.standard_normal((40, 4, 2)) + y[:, None, None]
    classes, yi = np.unique(y, return_inverse=True)
    splits = list(StratifiedKFold(3).split(X, y))
    pipe = make_pipeline(DimRedReshape(PCA), SVC(kernel='rbf', class_weight='balanced'))
    cands = list(ParameterGrid({'svc__C': [1, 10], 'svc__gamma': ['scale', 0.1], 'dimredreshape__n_components': [2, 5]}))
    fits = []
    real = DimRedReshape.fit

    def counting(self, X, y=None):
        fits.append(self.n_components)
        return real(self, X, y)
    DimRedReshape.fit = counting
    try:
        plan = S.build_plan(pipe, [S.split_params(pipe, c) for c in cands], X, yi, classes, splits)
    finally:
        DimRedReshape.fit = real
    assert sorted(fits) == [2] * 3 + [5] * 3                             # once per (outer combination, fold), not per C / gamma
    assert len(plan.views) == 6 and len(plan.models) == len(cands) * 3
    assert not hasattr(pipe.steps[0][1], 'transformer')                   # the searched estimator itself is not fitted
    for mod in plan.models:
        cand = cands[mod['cand']]
        tr, te = splits[mod['fold']]
        v, gamma = plan.matrices[mod['matrix']]
        step = DimRedReshape(PCA, n_components=cand['dimredreshape__n_components']).fit(X[tr])
        Ztr, Zte = step.transform(X[tr]), step.transform(X[te])
        np.testing.assert_array_equal(plan.views[v], np.vstack([Ztr, Zte]))
        ref = svc_fit_construction(SVC(kernel='rbf', class_weight='balanced', C=cand['svc__C'], gamma=cand['svc__gamma']), Ztr, y[tr])
        assert gamma == ref[0]
        np.testing.assert_array_equal(mod['problems']['idx'], ref[1])     # X[train] order: the view's first rows
        np.testing.assert_array_equal(mod['C'] * mod['problems']['weight'], ref[5])
        np.testing.assert_array_equal(mod['test_pos'], len(tr) + np.arange(len(te)))


# ------------------------------------------------------------------------------------------------ scores
def test_scores_from_confusion_tables_equal_sklearn_metrics():
    rng = np.random.default_rng(7)
    k = 4
    cases = []
    for trial in range(6):
        yt = rng.integers(0, k, 37)
        yp = rng.integers(0, k, 37)
        if trial == 0:
            yt[yt == 2] = 3                                               # class 2 has no held-out row but is predicted
            assert (yp == 2).any()
        if trial == 1:
            yp = yt.copy()
        cases.append((yt, yp))
    conf = np.zeros((len(cases), k, k), dtype=np.int32)
    for i, (yt, yp) in enumerate(cases):
        np.add.at(conf[i], (yt, yp), 1)
    assert conf[0, 2].sum() == 0
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                                   # sklearn warns about the predicted class without true rows
        want_acc = np.array([accuracy_score(yt, yp) for yt, yp in cases])
        want_bal = np.array([balanced_accuracy_score(yt, yp) for yt, yp in cases])
    np.testing.assert_array_equal(S.scores_from_confusion(conf, None), want_acc)
    np.testing.assert_array_equal(S.scores_from_confusion(conf, 'accuracy'), want_acc)
    np.testing.assert_array_equal(S.scores_from_confusion(conf, 'balanced_accuracy'), want_bal)
    assert S.scores_from_confusion(conf.reshape(2, 3, k, k), 'balanced_accuracy').shape == (2, 3)
    assert np.isnan(S.scores_from_confusion(np.zeros((1, k, k), dtype=np.int32), 'accuracy')).all()


def test_results_assembly_and_ranks_equal_gridsearchcv_fed_the_same_scores():
    """GridSearchCV over sklearn's SVC with a scorer that looks the score up in the injected table (ties between candidates, the
    first of the best kept), against assemble_results on that table."""
    n_splits = 3
    grid = {'C': [0.1, 1.0, 10.0, 100.0], 'gamma': [0.5, 'scale']}
    cands = list(ParameterGrid(grid))
    table = np.array([[0.5, 0.75, 0.25], [0.75, 0.5, 0.625], [0.625, 0.625, 0.625], [0.125, 0.25, 0.5],
                      [0.75, 0.625, 0.5], [0.5, 0.5, 0.5], [0.25, 0.5, 0.75], [0.0, 1.0, 0.5]])
    assert len(table) == len(cands)
    X = np.arange(12, dtype=np.float64)[:, None] + np.array([[0.0, 1.0]])
    y = np.arange(12) % 2
    fold_of = np.arange(12) % n_splits

    def scorer(est, Xf, yf):
        c = cands.index({'C': est.C, 'gamma': est.gamma})
        return table[c, fold_of[int(Xf[0, 0])]]
    gs = GridSearchCV(SkSVC(), grid, cv=PredefinedSplit(fold_of), scoring=scorer, refit=False).fit(X, y)
    res = S.assemble_results(cands, table)
    for f in range(n_splits):
        np.testing.assert_array_equal(res[f'split{f}_test_score'], gs.cv_results_[f'split{f}_test_score'])
    for key in ('mean_test_score', 'std_test_score', 'rank_test_score'):
        np.testing.assert_array_equal(res[key], gs.cv_results_[key])
    assert res['params'] == gs.cv_results_['params']
    for name in ('param_C', 'param_gamma'):
        assert list(res[name]) == list(gs.cv_results_[name]) and not np.ma.getmaskarray(res[name]).any()
    assert (res['rank_test_score'] == 1).sum() == 3                       # three candidates tie for the best mean (0.625)
    assert int(res['rank_test_score'].argmin()) == gs.best_index_ == 1
    uneven = S.assemble_results([{'C': 1}, {'gamma': 2}], np.array([[np.nan, 1.0], [0.5, 0.5]]))
    assert list(np.ma.getmaskarray(uneven['param_C'])) == [False, True] and list(uneven['rank_test_score']) == [2, 1]


# ------------------------------------------------------------------------------------------------ chunks
@pytest.mark.parametrize('sizes,limit', [([8] * 10, 24), ([8, 16, 8, 24, 8, 8], 24), ([5], 5), ([3, 3, 3], 100), ([7, 7, 7], 7)])
def test_chunks_stay_within_the_limit_and_cover_every_matrix_once(sizes, limit):
    chunks = S.cut_chunks(sizes, limit)
    assert [m for chunk in chunks for m in chunk] == list(range(len(sizes)))
    assert all(chunk and sum(sizes[m] for m in chunk) <= limit for chunk in chunks)
    for a, b in zip(chunks[:-1], chunks[1:]):                              # greedy: the next matrix would not have fitted
        assert sum(sizes[m] for m in a) + sizes[b[0]] > limit


def test_a_matrix_beyond_the_limit_is_refused():
    with pytest.raises(ValueError, match='max_kernel_bytes'):
        S.cut_chunks([8, 32, 8], 24)
    assert S.cut_chunks([], 24) == []
