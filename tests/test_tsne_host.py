"""manifold.TSNE without a device: every argument refusal and its text (raised before the device is looked for), the learning
rate rule, the random init's draws, get_params / set_params / clone, the tile and problem tables, and the new prototypes."""
import ctypes as C

import numpy as np
import pytest
import torch
from sklearn.base import clone
from sklearn.manifold import TSNE as SkTSNE

from cross_patient_speech_decoding_amd import _lib, manifold
from cross_patient_speech_decoding_amd.alignment import _linalg as LA
from cross_patient_speech_decoding_amd.manifold import TSNE

X = np.random.default_rng(0).standard_normal((40, 6))


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Any look for the device fails the test: the refusals come first."""
    def boom(*a, **k):
        raise AssertionError('the device was looked for')
    monkeypatch.setattr(LA, 'device', boom)
    monkeypatch.setattr(LA, 'to_device', boom)


def test_names_and_defaults_are_sklearns_except_method():
    ours, theirs = TSNE().get_params(), SkTSNE().get_params()
    assert ours.pop('method') == 'exact' and theirs.pop('method') == 'barnes_hut'
    for key, value in ours.items():
        assert theirs[key] == value, key
    assert manifold.TSNE is TSNE
    t = TSNE(1, perplexity=5.0, init='random', random_state=3)
    c = clone(t)
    assert c is not t and c.get_params() == t.get_params() and c.n_components == 1
    assert t.set_params(max_iter=300) is t and t.max_iter == 300


@pytest.mark.parametrize('kw, text', [
    (dict(method='barnes_hut'), r"exact gradient.*'barnes_hut' is not implemented"),
    (dict(n_components=3), r'n_components=3: 1 or 2 are supported.*notebooks use 2'),
    (dict(n_components=0), r'1 or 2 are supported'),
    (dict(perplexity=40), r'perplexity \(40\) must be less than n_samples \(40\)'),
    (dict(max_iter=249), r"The 'max_iter' parameter of TSNE must be an int in the range \[250, inf\)\. Got 249 instead\."),
    (dict(metric='cosine'), r"metric='cosine': 'euclidean' and 'precomputed' are supported"),
    (dict(init='spectral'), r"The 'init' parameter of TSNE must be a str among \{'pca', 'random'\}"),
    (dict(init=np.zeros((40, 3))), r'init has the shape \(40, 3\); \(40, 2\) is needed'),
    (dict(init=np.zeros((39, 2))), r'init has the shape \(39, 2\); \(40, 2\) is needed'),
    (dict(init=[[0.0, 0.0]] * 40), r"The 'init' parameter of TSNE"),
    (dict(learning_rate='fast'), r"The 'learning_rate' parameter of TSNE"),
    (dict(learning_rate=0.0), r"The 'learning_rate' parameter of TSNE"),
    (dict(early_exaggeration=0.5), r"The 'early_exaggeration' parameter of TSNE"),
    (dict(perplexity=0.0), r"The 'perplexity' parameter of TSNE"),
    (dict(min_grad_norm=-1.0), r"The 'min_grad_norm' parameter of TSNE"),
    (dict(n_iter_without_progress=-2), r"The 'n_iter_without_progress' parameter of TSNE"),
])
def test_argument_refusals_come_before_the_device(kw, text):
    with pytest.raises(ValueError, match=text):
        TSNE(**kw).fit(X)
    with pytest.raises(ValueError, match=text):
        TSNE(**kw).fit_transform_many([X, X])


def test_data_refusals_come_before_the_device():
    bad = X.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match='Input X contains NaN or infinity'):
        TSNE().fit(bad)
    with pytest.raises(ValueError, match='Input X contains NaN or infinity'):
        TSNE().fit(torch.from_numpy(bad))
    bad[3, 2] = np.inf
    with pytest.raises(ValueError, match='Input X contains NaN or infinity'):
        TSNE().fit_transform_many([X, bad])
    with pytest.raises(ValueError, match=r'4097 samples; at most XPS_TSNE_MAX_SAMPLES = 4096'):
        TSNE().fit(np.zeros((4097, 2)))
    with pytest.raises(ValueError, match='no data set'):
        TSNE().fit_transform_many([])
    with pytest.raises(ValueError, match='1 inits for 2 data sets'):
        TSNE().fit_transform_many([X, X], inits=['random'])
    with pytest.raises(ValueError, match=r'init contains NaN or infinity'):
        TSNE(init=np.full((40, 2), np.nan)).fit(X)
    D = np.abs(X @ X.T)
    with pytest.raises(ValueError, match='The parameter init="pca" cannot be used with metric="precomputed"'):
        TSNE(metric='precomputed').fit(D)
    with pytest.raises(ValueError, match='cannot be used with metric="precomputed"'):
        TSNE(metric='precomputed', init='random').fit_transform_many([D], inits=['pca'])
    with pytest.raises(ValueError, match='X should be a square distance matrix'):
        TSNE(metric='precomputed', init='random').fit(X)
    D[2, 5] = -1.0
    with pytest.raises(ValueError, match="With metric='precomputed', X should contain positive distances"):
        TSNE(metric='precomputed', init='random').fit(D)
    # sklearn's wording where sklearn has one
    for kw, data in ((dict(perplexity=40), X), (dict(max_iter=249), X), (dict(metric='precomputed'), np.abs(X @ X.T)),
                     (dict(metric='precomputed', init='random'), D)):
        with pytest.raises(ValueError) as theirs:
            SkTSNE(method='exact', **kw).fit(data)
        with pytest.raises(ValueError) as ours:
            TSNE(**kw).fit(data)
        assert str(ours.value) == str(theirs.value)


def test_learning_rate_is_sklearns_auto_rule():
    assert TSNE()._learning_rate(130) == 50.0
    assert TSNE()._learning_rate(4800) == 4800 / 12.0 / 4
    assert TSNE(early_exaggeration=4.0)._learning_rate(1600) == 100.0
    assert TSNE(learning_rate=200)._learning_rate(10) == 200.0


def test_random_inits_are_sklearns_draws_one_data_set_after_the_other():
    ts = TSNE(init='random', random_state=5)
    got = ts._inits([(7, 3), (4, 9)], None)
    rng = np.random.RandomState(5)
    for y, n in zip(got, (7, 4)):
        want = 1e-4 * rng.standard_normal(size=(n, 2)).astype(np.float32)
        assert y.dtype == np.float64 and np.array_equal(y, want.astype(np.float64))
    given = np.arange(8, dtype=np.float32).reshape(4, 2)
    mixed = TSNE(init='random', random_state=5)._inits([(4, 1), (7, 3), (6, 2)], [given, 'random', 'pca'])
    assert mixed[0].dtype == np.float64 and np.array_equal(mixed[0], given) and mixed[2] is None
    assert np.array_equal(mixed[1], got[0])                              # a given init consumes no draws
    one = TSNE(1, init='random', random_state=5)._inits([(7, 3)], None)[0]
    assert one.shape == (7, 1)


def test_tables_and_prototypes():
    tiles = LA.tsne_tiles([5, 8, 9])
    assert tiles.dtype == np.int32 and tiles.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [2, 0], [2, 1], [2, 2]]
    tab = LA.tsne_table([dict(n=5, nc=1, it_begin=7, lr=50.0)]).reshape(1, LA.TSNE_WORDS)
    assert tab[0, LA.TS_N] == 5 and tab[0, LA.TS_NC] == 1 and tab[0, LA.TS_ITBEGIN] == 7
    assert tab[0, LA.TS_LR:LA.TS_LR + 1].view(np.float64)[0] == 50.0 and tab[0, LA.TS_P] == 0
    for bad in (dict(n=1), dict(n=4097), dict(n=5, nc=3)):
        with pytest.raises(ValueError, match='2 <= n <= 4096 samples and 1 or 2 components'):
            LA.tsne_table([bad])
    with pytest.raises(ValueError, match='P must be a contiguous'):
        LA.tsne_table([dict(n=5, P=torch.zeros(5, 5))])
    i, i64, sz, vp, d = C.c_int, C.c_int64, C.c_size_t, C.c_void_p, C.c_double
    head = [vp, i, vp, i]
    assert _lib.SIGNATURES['xps_tsne_state_bytes'] == (sz, [i])
    for name in ('sqdist_f32', 'affinities_f64', 'descent_f64'):
        assert _lib.SIGNATURES[f'xps_tsne_{name}_workspace'] == (sz, [i, i])
    assert _lib.SIGNATURES['xps_tsne_sqdist_f32'] == (i, head + [vp, sz, vp])
    assert _lib.SIGNATURES['xps_tsne_affinities_f64'] == (i, head + [d, vp, sz, vp])
    assert _lib.SIGNATURES['xps_tsne_descent_f64'] == (i, head + [i, i, d, d, i, d, vp, sz, vp])
    src = open(_lib.HEADER_PATH).read()
    for macro, value in (('XPS_TSNE_WORDS', LA.TSNE_WORDS), ('XPS_TSNE_TILE_ROWS', LA.TSNE_TILE_ROWS),
                         ('XPS_TSNE_MAX_SAMPLES', LA.TSNE_MAX_SAMPLES), ('XPS_TSNE_STATE_HEAD', LA.TSNE_STATE_HEAD),
                         ('XPS_TSNE_STATE_ARRAYS', LA.TSNE_STATE_ARRAYS)):
        assert f'#define {macro} {value}\n' in src
