"""decoders.BaggingClassifier without a device: sklearn's bootstrap draws reproduced exactly, the estimator plumbing
(clone / get_params / set_params / pipeline step name) and the refusals that must happen before any device work."""
import numpy as np
import pytest
from sklearn.base import clone
from sklearn.dummy import DummyClassifier
from sklearn.ensemble import BaggingClassifier as SkBagging
from sklearn.pipeline import make_pipeline
from sklearn.preprocessing import StandardScaler

from cross_patient_speech_decoding_amd.decoders import SVC, BaggingClassifier
from cross_patient_speech_decoding_amd.decoders.bagging import bagging_sample_indices, n_draws

N_FEATURES = 7


@pytest.mark.parametrize('seed_kind', ['int', 'RandomState'])
@pytest.mark.parametrize('n,E,max_samples,bootstrap', [(37, 5, 1.0, True), (64, 70, 0.5, True), (50, 3, 20, False)])
def test_sample_indices_equal_sklearn_draw_for_draw(n, E, max_samples, bootstrap, seed_kind):
    """sklearn's draws, in sklearn's order: one seed per estimator, the feature draw, then the sample draw."""
    X = np.random.default_rng(n).standard_normal((n, N_FEATURES))
    y = np.arange(n) % 3

    def seed():
        return 1234 + n if seed_kind == 'int' else np.random.RandomState(99 + n)
    ref = SkBagging(DummyClassifier(), n_estimators=E, max_samples=max_samples, bootstrap=bootstrap, random_state=seed()).fit(X, y)
    got = bagging_sample_indices(seed(), E, n, N_FEATURES, max_samples, bootstrap)
    want = ref.estimators_samples_
    assert len(got) == len(want) == E
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert all(len(a) == ref._max_samples for a in got)
    if not bootstrap:
        assert all(len(np.unique(a)) == len(a) for a in got)


def test_number_of_draws_follows_sklearn():
    assert n_draws(1.0, 37) == 37 and n_draws(0.5, 65) == 32 and n_draws(20, 50) == 20 and n_draws(0.3, 60) == 18
    with pytest.raises(ValueError, match='max_samples must be <= n_samples'):
        n_draws(51, 50)


def test_params_clone_and_pipeline_name():
    bag = BaggingClassifier(SVC(kernel='linear', C=0.5), n_estimators=10, max_samples=0.8, random_state=3, n_jobs=4, verbose=1)
    twin = clone(bag)
    assert twin is not bag and twin.estimator is not bag.estimator
    p = twin.get_params(deep=True)
    assert p['n_estimators'] == 10 and p['max_samples'] == 0.8 and p['random_state'] == 3 and p['n_jobs'] == 4 and p['verbose'] == 1
    assert p['estimator__C'] == 0.5 and p['estimator__kernel'] == 'linear'
    assert p['bootstrap'] is True and p['bootstrap_features'] is False and p['oob_score'] is False and p['warm_start'] is False
    assert p['max_features'] == 1.0
    twin.set_params(estimator__C=2.0, n_estimators=40)
    assert twin.estimator.C == 2.0 and twin.n_estimators == 40
    assert bag.estimator.C == 0.5 and bag.n_estimators == 10
    assert set(p) == set(SkBagging(SVC()).get_params(deep=True))           # the reference's search-grid keys work unchanged
    pipe = make_pipeline(StandardScaler(), BaggingClassifier(SVC(kernel='rbf', class_weight='balanced')))
    assert pipe.steps[-1][0] == 'baggingclassifier'
    pipe.set_params(baggingclassifier__n_estimators=100, baggingclassifier__estimator__C=3.0, baggingclassifier__estimator__gamma=0.1)
    assert pipe[-1].n_estimators == 100 and pipe[-1].estimator.C == 3.0 and pipe[-1].estimator.gamma == 0.1


@pytest.fixture
def no_device(monkeypatch):
    """Any device work fails the test: the refusals below must come first."""
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    from cross_patient_speech_decoding_amd.decoders import bagging

    def boom(*a, **k):
        raise AssertionError('device work before the refusal')
    monkeypatch.setattr(LA, 'device', boom)
    monkeypatch.setattr(LA, 'dgemm', boom)
    monkeypatch.setattr(bagging, 'call', boom)
    monkeypatch.setattr(bagging, 'lib', boom)


X4 = np.array([[0.0, 1.0], [1.0, 0.0], [0.5, 1.5], [1.5, 0.5]])
Y4 = np.array([0, 1, 0, 1])


@pytest.mark.parametrize('estimator', [None, DummyClassifier(), 'svc'], ids=['none', 'dummy', 'sklearn-svc'])
def test_foreign_estimators_are_refused_before_device_work(no_device, estimator):
    if estimator == 'svc':
        from sklearn.svm import SVC as SkSVC
        estimator = SkSVC(kernel='linear')
    with pytest.raises(TypeError, match='decoders.SVC'):
        BaggingClassifier(estimator).fit(X4, Y4)


@pytest.mark.parametrize('kw', [{'max_features': 0.5}, {'max_features': 1}, {'bootstrap_features': True}, {'oob_score': True},
                                {'warm_start': True}], ids=lambda kw: next(iter(kw)) + '=' + str(next(iter(kw.values()))))
def test_unsupported_settings_are_refused_before_device_work(no_device, kw):
    with pytest.raises(NotImplementedError):
        BaggingClassifier(SVC(kernel='linear'), **kw).fit(X4, Y4)


def test_estimator_settings_raise_as_svc_fit_raises_them(no_device):
    with pytest.raises(NotImplementedError, match="kernel='linear' and kernel='rbf'"):
        BaggingClassifier(SVC(kernel='poly')).fit(X4, Y4)
    with pytest.raises(NotImplementedError, match='break_ties'):
        BaggingClassifier(SVC(kernel='linear', break_ties=True)).fit(X4, Y4)
