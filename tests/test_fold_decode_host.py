"""decoders.cross_val_decode, the host side (no GPU): the partition cutter, the (fold, estimator) problem builder against a per-fold
restatement of SVC.fit's / BaggingClassifier.fit's construction, the host vote against a numpy restatement, the scores against
sklearn.metrics, every refusal (those of the front matter through both entry points that share it), and the one-candidate plan
cross_val_decode hands the partition engine."""
import numpy as np
import pytest
from sklearn.decomposition import PCA as SkPCA
from sklearn.ensemble import BaggingClassifier as SkBagging
from sklearn.metrics import accuracy_score, balanced_accuracy_score
from sklearn.model_selection import KFold, RepeatedStratifiedKFold, ShuffleSplit, StratifiedKFold
from sklearn.pipeline import make_pipeline
from sklearn.svm import SVC as SkSVC
from sklearn.utils.class_weight import compute_class_weight

from cross_patient_speech_decoding_amd import decoders as D
from cross_patient_speech_decoding_amd.alignment import PCA, AlignCCA, AlignMCCA, JointPCA
from cross_patient_speech_decoding_amd.alignment._linalg import gram_tiles
from cross_patient_speech_decoding_amd.decoders import _ovo
from cross_patient_speech_decoding_amd.decoders import fold_decode as FD
from cross_patient_speech_decoding_amd.decoders.bagging import bagging_sample_indices
from cross_patient_speech_decoding_amd.decoders.search import scores_from_confusion
from cross_patient_speech_decoding_amd.decomposition import DimRedReshape


# ------------------------------------------------------------------------------------------------ partitions
def test_repeated_stratified_k_fold_gives_one_partition_per_repeat():
    y = np.arange(30) % 3
    splits = list(RepeatedStratifiedKFold(n_splits=3, n_repeats=2, random_state=0).split(np.zeros(30), y))
    parts = FD.cut_partitions(splits, 30)
    assert [len(p) for p in parts] == [3, 3]
    flat = [s for p in parts for s in p]
    for (tr, te), (tr0, te0) in zip(flat, splits):
        assert np.array_equal(tr, tr0) and np.array_equal(te, te0)
    for p in parts:
        assert np.array_equal(np.sort(np.concatenate([te for _, te in p])), np.arange(30))
    assert [len(p) for p in FD.cut_partitions(KFold(5).split(np.zeros(30)), 30)] == [5]


def test_splits_that_do_not_partition_are_refused():
    with pytest.raises(ValueError, match='overlaps'):
        FD.cut_partitions(ShuffleSplit(4, test_size=0.5, random_state=0).split(np.zeros(30)), 30)
    kf = list(KFold(5).split(np.zeros(30)))
    with pytest.raises(ValueError, match='do not cover'):
        FD.cut_partitions(kf[:4], 30)
    with pytest.raises(ValueError, match='do not cover'):
        FD.cut_partitions(kf + kf[:2], 30)
    with pytest.raises(ValueError, match='outside range'):
        FD.cut_partitions([(np.arange(5), np.array([30]))], 30)
    with pytest.raises(ValueError, match='no split'):
        FD.cut_partitions([], 30)


def test_gram_tiles_list_the_lower_triangle_of_every_problem():
    t = gram_tiles([130, 0, 64, 1])
    assert t.dtype == np.int32
    assert t.tolist() == [[0, 0, 0], [0, 1, 0], [0, 1, 1], [0, 2, 0], [0, 2, 1], [0, 2, 2], [2, 0, 0], [3, 0, 0]]
    assert gram_tiles([]).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ the problem builder
def _restated(labels, positions, class_weight, C, weights=None):
    """SVC.fit's construction on the rows handed to one fit, restated: sklearn's classes and 'balanced' weights from ALL rows handed
    over, zero-weight rows dropped, members in original order, libsvm's pair order, the lower class positive; bound = C * class
    weight * sample weight.  Returns per problem (class a, class b, kernel-matrix rows, npos, bounds) with classes as labels."""
    labels, positions = np.asarray(labels), np.asarray(positions)
    classes = np.unique(labels)
    cw = compute_class_weight(class_weight, classes=classes, y=labels)
    w = np.ones(len(labels)) if weights is None else np.asarray(weights, dtype=np.float64)
    out = []
    for i, a in enumerate(classes):
        for j, b in enumerate(classes):
            if j <= i:
                continue
            ma, mb = np.flatnonzero((labels == a) & (w > 0)), np.flatnonzero((labels == b) & (w > 0))
            if len(ma) == 0 or len(mb) == 0:
                continue
            rows = np.concatenate([ma, mb])
            bound = np.concatenate([(C * cw[i]) * w[ma], (C * cw[j]) * w[mb]])
            out.append((a, b, positions[rows], len(ma), bound))
    return out


def _assert_same(problems, C, restated, classes):
    off = np.concatenate([[0], np.cumsum(problems['sizes'])])
    assert len(problems['npos']) == len(restated)
    cb = _ovo.bounds(C, problems)
    for q, (a, b, rows, npos, bound) in enumerate(restated):
        assert classes[problems['pair_a'][q]] == a and classes[problems['pair_b'][q]] == b
        assert np.array_equal(problems['idx'][off[q]:off[q + 1]], rows)
        assert problems['npos'][q] == npos
        assert np.array_equal(cb[off[q]:off[q + 1]], bound)


CLASSES = np.array([2, 3, 5, 7, 11])                         # the union over the target and the pooled patients


def _fold_inputs(seed=0):
    rng = np.random.default_rng(seed)
    y_tar = CLASSES[rng.integers(0, 4, 40)]                   # the target never shows class 11
    y_pool = CLASSES[np.concatenate([rng.integers(0, 4, 24), [4]])]     # class 11: one pooled row
    tr, te = np.setdiff1d(np.arange(40), np.arange(3, 40, 4)), np.arange(3, 40, 4)
    return y_tar, y_pool, tr, te


def test_a_bare_svc_fold_is_svc_fits_construction_on_the_folds_rows():
    y_tar, y_pool, tr, te = _fold_inputs()
    svc = D.SVC(kernel='linear', C=2.5, class_weight='balanced')
    fd = FD.fold_layout(svc, None, CLASSES, np.searchsorted(CLASSES, y_tar), np.searchsorted(CLASSES, y_pool), tr, te, True, 60)
    n_all = len(tr) + len(y_pool)
    assert (fd['first'], fd['last'], fd['rows']) == (0, n_all, n_all + len(te)) and fd['samples'] == [] and len(fd['problems']) == 1
    assert np.array_equal(fd['test_pos'], n_all + np.arange(len(te))) and np.array_equal(CLASSES[fd['ytest']], y_tar[te])
    _assert_same(fd['problems'][0], 2.5, _restated(np.concatenate([y_tar[tr], y_pool]), np.arange(n_all), 'balanced', 2.5), CLASSES)


def test_tar_in_train_false_leaves_the_targets_rows_out_of_every_index_list():
    y_tar, y_pool, tr, te = _fold_inputs()
    svc = D.SVC(kernel='rbf', class_weight='balanced')
    fd = FD.fold_layout(svc, None, CLASSES, np.searchsorted(CLASSES, y_tar), np.searchsorted(CLASSES, y_pool), tr, te, False, 60)
    lo, hi = len(tr), len(tr) + len(y_pool)
    assert (fd['first'], fd['last'], fd['rows']) == (lo, hi, hi + len(te))
    idx = fd['problems'][0]['idx']
    assert idx.min() >= lo and idx.max() < hi
    assert np.array_equal(fd['test_pos'], hi + np.arange(len(te)))                 # the held-out rows stay where they are
    _assert_same(fd['problems'][0], 1.0, _restated(y_pool, np.arange(lo, hi), 'balanced', 1.0), CLASSES)


def test_balanced_weights_are_each_folds_own():
    y_tar, y_pool, _, _ = _fold_inputs(3)
    svc = D.SVC(kernel='linear', class_weight='balanced')
    yi_tar, yi_pool = np.searchsorted(CLASSES, y_tar), np.searchsorted(CLASSES, y_pool)
    seen = []
    for tr, te in StratifiedKFold(4, shuffle=True, random_state=1).split(np.zeros(40), y_tar):
        fd = FD.fold_layout(svc, None, CLASSES, yi_tar, yi_pool, tr, te, True, 60)
        labels = np.concatenate([y_tar[tr], y_pool])
        _assert_same(fd['problems'][0], 1.0, _restated(labels, np.arange(len(labels)), 'balanced', 1.0), CLASSES)
        seen.append(tuple(np.bincount(np.searchsorted(CLASSES, labels), minlength=5)))
    assert len(set(seen)) > 1                                                      # the folds do differ in their class counts


def test_a_bagged_fold_is_bagging_fits_construction_and_a_bootstrap_may_lose_a_class():
    y_tar, y_pool, tr, te = _fold_inputs()
    labels = np.concatenate([y_tar[tr], y_pool])
    assert (labels == 11).sum() == 1                                               # one row: a bootstrap loses it 1 time in e
    ens = D.BaggingClassifier(D.SVC(kernel='linear', C=0.5, class_weight='balanced'), n_estimators=10, random_state=0)
    d = 60
    fd = FD.fold_layout(ens.estimator, ens, CLASSES, np.searchsorted(CLASSES, y_tar), np.searchsorted(CLASSES, y_pool), tr, te, True, d)
    draws = bagging_sample_indices(0, 10, len(labels), d)                          # a clone fitted on this fold: its rows, its features
    assert len(fd['samples']) == 10 and all(np.array_equal(a, b) for a, b in zip(fd['samples'], draws))
    lost = 0
    for p, s in zip(fd['problems'], draws):
        w = np.bincount(s, minlength=len(labels)).astype(np.float64)
        restated = _restated(labels, np.arange(len(labels)), 'balanced', 0.5, w)
        _assert_same(p, 0.5, restated, CLASSES)
        present = np.unique(labels[w > 0])
        lost += len(present) < len(np.unique(labels))
        assert len(p['npos']) == len(present) * (len(present) - 1) // 2
    assert lost >= 1
    # another row count draws differently: the draws are this fold's own
    other = [s[:len(labels)] for s in bagging_sample_indices(0, 10, len(labels) + 1, d)]
    assert not all(np.array_equal(a, b) for a, b in zip(draws, other))


def test_a_fold_with_one_class_raises_sklearns_error():
    with pytest.raises(ValueError, match='greater than one'):
        FD.fold_problems(D.SVC(), None, CLASSES, np.zeros(5, dtype=int), np.arange(5), 4)


# ------------------------------------------------------------------------------------------------ vote and scores
def _vote_restated(pred, k):
    votes = np.zeros((pred.shape[1], k), dtype=np.int64)
    for e in range(pred.shape[0]):
        for r in range(pred.shape[1]):
            if 0 <= pred[e, r] < k:
                votes[r, pred[e, r]] += 1
    win = np.array([[c for c in range(k) if v[c] == v.max()][0] for v in votes])
    return votes, win


def test_host_vote_counts_estimators_and_ties_go_to_the_lowest_class():
    pred = np.array([[3, 1, 2, 0], [1, 1, 0, 0], [3, 2, 2, 4], [1, 2, 0, 4]])     # row 0: 3 and 1 tie -> 1; row 1: 1, 2 tie -> 1
    votes, win = FD.host_vote(pred, 5)
    assert votes.dtype == np.int32 and votes.sum(axis=1).tolist() == [4, 4, 4, 4]
    assert win.tolist() == [1, 1, 0, 0]
    rng = np.random.default_rng(0)
    pred = rng.integers(0, 6, (10, 200))
    pred[3] = rng.integers(0, 2, 200)                                              # an estimator that lacks classes 2..5
    pred[7, ::9] = -1                                                              # a row outside the matrix casts no vote
    votes, win = FD.host_vote(pred, 6)
    v0, w0 = _vote_restated(pred, 6)
    assert np.array_equal(votes, v0) and np.array_equal(win, w0)
    one, w1 = FD.host_vote(pred[:1], 6)                                            # a bare SVC: E = 1
    assert np.array_equal(w1, pred[0]) and one.sum(axis=1).tolist() == [1] * 200


def test_scores_equal_sklearn_metrics():
    rng = np.random.default_rng(4)
    y_true = rng.integers(0, 4, 150)                                               # class 4 of 5 has no held-out row
    y_pred = np.where(rng.random(150) < 0.7, y_true, rng.integers(0, 5, 150))
    conf = FD.confusion(y_true, y_pred, 5)
    assert conf.sum() == 150 and conf[4].sum() == 0
    assert scores_from_confusion(conf, 'accuracy') == accuracy_score(y_true, y_pred)
    with pytest.warns(UserWarning):
        ref = balanced_accuracy_score(y_true, y_pred)
    assert scores_from_confusion(conf, 'balanced_accuracy') == ref


# ------------------------------------------------------------------------------------------------ refusals
def _pool():
    rng = np.random.default_rng(0)
    return [(rng.standard_normal((12, 4, 6)), np.arange(12) % 3, np.arange(12) % 3)]


def _data():
    rng = np.random.default_rng(1)
    return rng.standard_normal((12, 4, 5)), np.arange(12) % 3


def test_exports():
    assert D.cross_val_decode is FD.cross_val_decode and D.FoldDecode is FD.FoldDecode


@pytest.mark.parametrize('model', [
    D.crossPtDecoder_sepDimRed(_pool(), D.SVC()),
    D.crossPtDecoder_jointDimRed(_pool(), D.SVC(), JointPCA),
    D.crossPtDecoder_mcca(_pool(), D.SVC(), AlignMCCA),
    D.crossPtDecoder_sepAlign(_pool(), D.SVC(), AlignMCCA),
    D.crossPtDecoder_sepAlign(_pool(), D.SVC(), lambda: AlignCCA(type='trial')),
    D.crossPtDecoder_sepAlign(_pool(), D.SVC(), AlignCCA, dim_red=SkPCA),
    D.crossPtDecoder_sepAlign(_pool(), SkSVC(kernel='linear'), AlignCCA),
    D.crossPtDecoder_sepAlign(_pool(), SkBagging(D.SVC()), AlignCCA),
    D.crossPtDecoder_sepAlign(_pool(), D.BaggingClassifier(SkSVC()), AlignCCA),
    D.SVC(),
], ids=['sepDimRed', 'jointDimRed', 'mcca', 'AlignMCCA', 'AlignCCA-trial', 'sklearn-PCA', 'sklearn-SVC', 'sklearn-bagging',
        'bagged-sklearn-SVC', 'no-wrapper'])
def test_everything_else_is_a_type_error_that_names_what_is_supported(model):
    X, y = _data()
    with pytest.raises(TypeError, match='decoders.SVC'):
        D.cross_val_decode(model, X, y)


def test_pipelines_and_unsupported_settings_are_not_implemented():
    X, y = _data()
    pipe = make_pipeline(DimRedReshape(PCA), D.SVC())
    with pytest.raises(NotImplementedError, match='pipeline'):
        D.cross_val_decode(D.crossPtDecoder_sepAlign(_pool(), pipe, AlignCCA), X, y)
    with pytest.raises(NotImplementedError, match='kernel'):
        D.cross_val_decode(D.crossPtDecoder_sepAlign(_pool(), D.SVC(kernel='poly'), AlignCCA), X, y)
    with pytest.raises(NotImplementedError, match='oob_score'):
        D.cross_val_decode(D.crossPtDecoder_sepAlign(_pool(), D.BaggingClassifier(D.SVC(), oob_score=True), AlignCCA), X, y)
    with pytest.raises(ValueError, match='n_trials'):
        D.cross_val_decode(D.crossPtDecoder_sepAlign(_pool(), D.SVC(), AlignCCA), X, np.stack([y, y], axis=1))


def _one_class_pool():
    return [(np.zeros((12, 4, 6)), np.zeros(12, dtype=int), np.zeros(12, dtype=int))]


@pytest.mark.parametrize('pool, y, message', [
    (_pool(), np.stack([np.arange(12) % 3] * 2, axis=1), r'^y must be \(n_trials,\)$'),
    (_one_class_pool(), np.zeros(12, dtype=int), '^The number of classes has to be greater than one; got 1 class$'),
    (_pool(), np.arange(130) % 65, r'^the scoring kernel takes 2\.\.64 classes; got 65$'),
], ids=['2-D y', 'one class', '65 classes'])
def test_both_entry_points_refuse_the_same_things_with_the_same_messages(pool, y, message):
    """The one front matter (``decode_setup``, ``search.check_class_count``), before anything touches the device."""
    X = np.zeros((len(y), 4, 5))
    model = D.crossPtDecoder_sepAlign(pool, D.SVC(), AlignCCA)
    with pytest.raises(ValueError, match=message):
        D.cross_val_decode(model, X, y)
    with pytest.raises(ValueError, match=message):
        D.AlignedSVCSearchCV(model, {'n_comp': [3]}).fit(X, y)
    with pytest.raises(ValueError, match=message):
        FD.decode_setup(model, y, None, 5)


def test_the_front_matter_of_a_run():
    y = np.array([5, 3, 7] * 4)
    pool = [(np.zeros((4, 4, 6)), np.array([3, 11, 3, 5]), None)]
    model = D.crossPtDecoder_sepAlign(pool, D.SVC(), AlignCCA)
    y_out, y_al, pool_out, classes, yi_tar, yi_pool, parts = FD.decode_setup(model, list(y), None, StratifiedKFold(3))
    assert np.array_equal(y_out, y) and y_al is y_out and len(pool_out) == 1
    assert classes.tolist() == [3, 5, 7, 11]                                      # the union: the target never shows 11
    assert yi_tar.dtype == np.int32 and np.array_equal(classes[yi_tar], y)
    assert yi_pool.dtype == np.int32 and yi_pool.tolist() == [0, 3, 0, 1]
    assert [len(p) for p in parts] == [3]
    marker = object()
    assert FD.decode_setup(model, y, marker, StratifiedKFold(3))[1] is marker
    assert len(FD.decode_setup(model, y, None, RepeatedStratifiedKFold(n_splits=2, n_repeats=3, random_state=0))[6]) == 3


# ------------------------------------------------------------------------------------------------ the one-candidate plan
@pytest.mark.parametrize('kernel, gamma', [('rbf', 'scale'), ('rbf', 0.25), ('linear', 'scale')], ids=['rbf-scale', 'rbf-float', 'linear'])
def test_one_candidate_is_one_view_one_matrix_and_one_model_per_fold(kernel, gamma):
    """What cross_val_decode hands the engine: one setting on one alignment."""
    settings = [dict(C=2.0, gamma=FD.gamma_spec(kernel, gamma))]
    rows = [225, 226, 225, 224]
    plan = FD.build_plan(settings, [0], [rows], kernel, lambda a, f, spec: 0.5 + f if spec == 'scale' else spec)
    value = {('rbf', 'scale'): lambda f: 0.5 + f, ('rbf', 0.25): lambda f: 0.25, ('linear', 'scale'): lambda f: None}[kernel, gamma]
    assert plan.views == [(0, f) for f in range(4)] and plan.rows == rows
    assert plan.matrices == [(f, value(f)) for f in range(4)]
    assert plan.models == [dict(cand=0, fold=f, view=f, matrix=f, C=2.0) for f in range(4)]
    assert plan.matrix_bytes() == [8 * n ** 2 for n in rows]
    assert FD.scale_views(settings, [0], 4, kernel) == ([(0, f) for f in range(4)] if (kernel, gamma) == ('rbf', 'scale') else [])
    rbf = kernel == 'rbf'
    assert FD.cut_plan_chunks(plan, rbf, 2 ** 30) == [[0, 1, 2, 3]]
    assert FD.cut_plan_chunks(plan, rbf, 8 * 226 ** 2) == [[0], [1], [2], [3]]    # for rbf each with its Gram beside it
    assert len(FD.cut_plan_chunks(plan, rbf, 2 * 8 * 226 ** 2)) == (4 if rbf else 2)
    with pytest.raises(ValueError, match='too small'):
        FD.cut_plan_chunks(plan, rbf, 8 * 226 ** 2 - 1)


def test_supported_models_pass_the_check():
    svc = D.SVC(kernel='rbf', class_weight='balanced')
    assert FD.check_model(D.crossPtDecoder_sepAlign(_pool(), svc, AlignCCA, tar_in_train=False)) == (svc, None)
    ens = D.BaggingClassifier(D.SVC(kernel='linear'), n_estimators=10)
    assert FD.check_model(D.crossPtDecoder_sepAlign(_pool(), ens, AlignCCA)) == (ens.estimator, ens)
