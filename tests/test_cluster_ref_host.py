"""tests/cluster_ref.py against sklearn on the CPU, the conditions the GPU tests of the cluster scores rely on for every
fixed-seed case they use, the host half of alignment/metrics.py (the k x k formulas on numpy-made tables, the p-values) and the
argument refusals of its public functions, none of which needs a device."""
import numpy as np
import pytest
from scipy import stats
from sklearn import metrics as SK

import cluster_ref as CR
from cross_patient_speech_decoding_amd.alignment import metrics as MT

CASES = CR.cases()
SHUFFLES, SEED = 65, 5                                        # what tests/test_gpu_cluster_scores.py draws per case


@pytest.fixture(scope='module')
def d2():
    return {name: CR.sq_dists(X) for name, (X, _) in CASES.items()}


def label_sets(name):
    return [CASES[name][1]] + CR.shuffles(CASES[name][1], SHUFFLES, SEED)


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_restatement_agrees_with_sklearn(name, d2):
    X, labels = CASES[name]
    X64 = X.astype(np.float64).reshape(len(X), -1)
    for y in label_sets(name)[:3]:
        s = CR.silhouette_samples(X64, y, d2[name])
        err = np.abs(SK.silhouette_samples(X64, y) - s).max()
        bar = CR.silhouette_bar(X64, d2[name], centre=False)
        print(f'{name}: silhouettes sklearn vs long double {float(err):.2e} (bar {bar:.2e})')
        assert err <= bar
        ch_bar, db_bar = CR.dispersion_bars(X64, y, centre=False)
        ch, db = CR.calinski_harabasz(X64, y), CR.davies_bouldin(X64, y)
        assert abs(SK.calinski_harabasz_score(X64, y) - ch) <= ch_bar * abs(ch)
        assert abs(SK.davies_bouldin_score(X64, y) - db) <= db_bar * abs(db) + CR.sklearn_singleton_slack(X64, y)
        pos = np.asarray(s, dtype=np.float64)
        assert abs(CR.positive_mean(s) - pos[pos > 0].mean()) <= 1e-15


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_gpu_case_is_well_conditioned_and_has_positive_silhouettes(name, d2):
    X, labels = CASES[name]
    assert CR.conditioning(X, d2[name]) >= 1e-3
    sets = label_sets(name)
    s0 = CR.silhouette_samples(X, sets[0], d2[name])
    share = float((s0 > 0).mean())
    shuffled = [float((CR.silhouette_samples(X, y, d2[name]) > 0).mean()) for y in sets[1:9]]
    print(f'{name}: positive share {share:.2f} on the labels, {min(shuffled):.2f}..{max(shuffled):.2f} shuffled')
    assert share >= 0.25
    assert max(shuffled) > 0


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_gram_route_in_numpy_stays_within_the_bars(name, d2):
    """The device route's arithmetic in numpy (another summation order) and the library's own host formulas on its tables."""
    X, labels = CASES[name]
    sets = label_sets(name)[:6]
    k = CR.codes_of(labels)[1]
    coded = [CR.codes_of(y)[0] for y in sets]
    bar = CR.silhouette_bar(X, d2[name])
    for y, c in zip(sets, coded):
        assert np.abs(CR.gram_silhouettes(X, c, k) - CR.silhouette_samples(X, y, d2[name])).max() <= bar
    counts, M, dg, intra = CR.gram_tables(X, coded, k)
    ch, db = MT._ch_db(M, dg, intra, counts, np.full(len(sets), float(k)), len(X))
    for r, y in enumerate(sets):
        ch_bar, db_bar = CR.dispersion_bars(X, y)
        ch_ref, db_ref = CR.calinski_harabasz(X, y), CR.davies_bouldin(X, y)
        assert abs(ch[r] - ch_ref) <= ch_bar * abs(ch_ref)
        assert abs(db[r] - db_ref) <= db_bar * abs(db_ref)
    # a set scored alone, and with more (empty) classes beside it, gives the same bits
    one = MT._ch_db(M[2:3], dg[2:3], intra[2:3], counts[2:3], np.array([float(k)]), len(X))
    assert one[0][0] == ch[2] and one[1][0] == db[2]
    pad = [np.concatenate([a, np.zeros(a.shape[:-1] + (2,), a.dtype)], axis=-1) for a in (counts, dg, intra)]
    Mp = np.zeros((len(sets), k + 2, k + 2))
    Mp[:, :k, :k] = M
    wide = MT._ch_db(Mp, pad[1], pad[2], pad[0], np.full(len(sets), float(k)), len(X))
    assert np.array_equal(wide[0], ch) and np.array_equal(wide[1], db)


def test_davies_bouldin_zero_division_cases_return_what_sklearn_returns():
    points = np.array([[0.0, 0.0], [0.0, 0.0], [4.0, 2.0], [4.0, 2.0], [4.0, 2.0]])       # every cluster a point
    same_centroid = np.array([[-1.0], [1.0], [-2.0], [2.0]])                              # both centroids at 0
    for X, y in ((points, np.array([0, 0, 1, 1, 1])), (same_centroid, np.array([0, 0, 1, 1]))):
        counts, M, dg, intra = CR.gram_tables(X, [y], 2)
        _, db = MT._ch_db(M, dg, intra, counts, np.array([2.0]), len(X))
        assert db[0] == SK.davies_bouldin_score(X, y) == 0.0
    counts, M, dg, intra = CR.gram_tables(points, [np.array([0, 0, 1, 1, 1])], 2)
    ch, _ = MT._ch_db(M, dg, intra, counts, np.array([2.0]), 5)
    assert ch[0] == SK.calinski_harabasz_score(points, np.array([0, 0, 1, 1, 1])) == 1.0


def test_p_values_follow_the_host_formula():
    v = np.array([0.5, 0.6, 0.5, 0.1, np.nan, 0.9])
    assert MT.permutation_p_value(v, 4) == (1 + 2) / 5                    # 0.6, 0.5; the NaN never counts; 0.9 is no shuffle
    assert MT.permutation_p_value(v, 4, smaller=True) == (1 + 2) / 5      # 0.5, 0.1
    assert MT.permutation_p_value(v, 0) == 1.0
    assert MT.sets_per_chunk(100, 9, 1) == 1 and MT.sets_per_chunk(100, 9, 2 ** 28) > 1000


def test_pearson_p_values_are_scipys():
    rng = np.random.default_rng(0)
    for L in (2, 5, 30):
        x, y = rng.standard_normal(L), rng.standard_normal(L)
        res = stats.pearsonr(x, y)
        assert MT._pearson_p(np.array([res.statistic]), L)[0] == res.pvalue


def test_argument_refusals_need_no_device(monkeypatch):
    def no_device():
        raise AssertionError('the device was looked for before the arguments were checked')
    monkeypatch.setattr(MT.LA, 'device', no_device)
    monkeypatch.setattr(MT.LA, 'to_device', lambda x: no_device())
    X = np.zeros((10, 3))
    y = np.arange(10) % 3
    for fn in (MT.silhouette_samples, MT.silhouette_score, MT.silhouette_scorer, MT.calinski_harabasz_score,
               MT.davies_bouldin_score, MT.cluster_scores):
        with pytest.raises(ValueError, match='number of labels is 1'):
            fn(X, np.zeros(10, dtype=int))
        with pytest.raises(ValueError, match='number of labels is 10'):
            fn(X, np.arange(10))
        with pytest.raises(ValueError, match='10 entries for 9 samples'):
            fn(X[:9], y)
    with pytest.raises(ValueError, match='65 classes'):
        MT.cluster_scores(np.zeros((130, 2)), np.arange(130) % 65)
    with pytest.raises(ValueError, match='label_sets.*9 entries for 10 samples'):
        MT.cluster_scores(X, y, label_sets=[y, y[:9]])
    with pytest.raises(ValueError, match='number of labels is 1'):
        MT.cluster_scores(X, y, label_sets=[np.zeros(10)])
    for bad in (-1, 1.5, None):
        with pytest.raises(ValueError, match='n_shuffles'):
            MT.cluster_scores(X, y, n_shuffles=bad)
    with pytest.raises(ValueError, match='max_bytes'):
        MT.cluster_scores(X, y, max_bytes=0)
    with pytest.raises(ValueError, match='random_state'):
        MT.cluster_scores(X, y, random_state='seed')
    with pytest.raises(ValueError, match='same shape'):
        MT.pt_corr(np.zeros((7, 5, 6)), np.zeros((7, 5, 5)))
    with pytest.raises(ValueError, match='same shape'):
        MT.pt_corr_multi(np.zeros((7, 5, 6)), [np.zeros((7, 5, 6)), np.zeros((6, 5, 6))], p_vals=True)
    with pytest.raises(ValueError, match='at least 2 values'):
        MT.pt_corr(np.zeros((7, 1)), np.zeros((7, 1)))
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError):
        MT.cluster_scores(X, y, n_shuffles=3, label_sets=[y[:9]])
    assert np.array_equal(np.random.get_state()[1], state)                 # a refused call draws nothing


def test_without_a_device_the_functions_raise_the_packages_error():
    import torch
    if torch.cuda.is_available():
        return
    X, y = CASES['n12_D5_k4_singleton']
    with pytest.raises(RuntimeError, match='needs the MI355X'):
        MT.cluster_scores(X, y, n_shuffles=2, random_state=0)
    with pytest.raises(RuntimeError, match='needs the MI355X'):
        MT.pt_corr(np.ones((7, 5, 6)), np.ones((7, 5, 6)))
    import cross_patient_speech_decoding_amd.alignment as A
    assert A.metrics is MT and A.cluster_scores is MT.cluster_scores and A.pt_corr is MT.pt_corr
