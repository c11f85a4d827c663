"""decoders.BaggingClassifier on the MI355X: the two new kernels through the C ABI against numpy restatements of their rules
(exact), and the fused ensemble against its two references -- sklearn's BaggingClassifier around decoders.SVC (the same problems,
solved one estimator at a time) and around sklearn's libsvm SVC (what the reference calls)."""
import functools
import os
import sys

import numpy as np
import pytest
from sklearn.ensemble import BaggingClassifier as SkBagging
from sklearn.svm import SVC as SkSVC

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ numpy restatements
def vote_rules(dec_minus_rho, pair_a, pair_b, est_off, k):
    """The voting rules: problem q votes pair_a[q] where its value is > 0 (strictly), else pair_b[q]; an estimator votes for the
    class with the most votes among its problems (first maximum: ties to the lowest index; absent classes have none); votes[r][c]
    counts estimators; pred[r] is the first maximum of votes[r]."""
    m = dec_minus_rho.shape[0]
    rows = np.arange(m)
    win = np.where(dec_minus_rho > 0, pair_a[None, :], pair_b[None, :])
    votes = np.zeros((m, k), dtype=np.int32)
    for e in range(len(est_off) - 1):
        cnt = np.zeros((m, k), dtype=np.int64)
        for q in range(est_off[e], est_off[e + 1]):
            cnt[rows, win[:, q]] += 1
        votes[rows, cnt.argmax(axis=1)] += 1
    return votes, votes.argmax(axis=1).astype(np.int32)


def pairs_of(present):
    return [(a, b) for i, a in enumerate(present) for b in present[i + 1:]]


def dev_tensor(a):
    import torch
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    return torch.from_numpy(np.ascontiguousarray(a)).to(LA.device())


# ------------------------------------------------------------------------------------------------ 1. the vote kernel
def run_vote(dec, ld, rho, pa, pb, est_off, m, E, k):
    import torch
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import call
    dec_d, rho_d = dev_tensor(dec), dev_tensor(rho)
    pa_d, pb_d, eo_d = dev_tensor(pa.astype(np.int32)), dev_tensor(pb.astype(np.int32)), dev_tensor(est_off.astype(np.int32))
    votes = torch.full((m, max(k, 1)), -7, dtype=torch.int32, device=dec_d.device)
    pred = torch.full((m,), -7, dtype=torch.int32, device=dec_d.device)
    call('xps_bag_vote_f64', dec_d.data_ptr(), ld, rho_d.data_ptr(), pa_d.data_ptr(), pb_d.data_ptr(), eo_d.data_ptr(), m, E, k,
         votes.data_ptr(), pred.data_ptr(), _dev.stream())
    torch.cuda.synchronize()
    return votes.cpu().numpy(), pred.cpu().numpy()


@pytest.mark.parametrize('m,E,k,lacking', [(1, 1, 2, False), (7, 10, 3, False), (130, 70, 9, True), (33, 65, 5, True)])
def test_vote_kernel_equals_the_rules_bit_for_bit(m, E, k, lacking):
    rng = np.random.default_rng(1000 * m + E)
    pa, pb, est_off = [], [], [0]
    for e in range(E):
        present = list(range(k))
        if lacking and e % 3 == 1 and e != E - 1:                    # a third of the estimators lack one or two classes (never 0 / 1)
            for c in rng.choice(np.arange(2, k), size=1 + e % 2, replace=False):
                present.remove(int(c))
        for a, b in pairs_of(present):
            pa.append(a)
            pb.append(b)
        est_off.append(len(pa))
    pa, pb, est_off = np.array(pa), np.array(pb), np.array(est_off)
    Q = len(pa)
    ld = Q + 5
    rho = rng.standard_normal(Q)
    dec = rng.standard_normal((m, ld))
    eq = rng.random((m, Q)) < 0.05                                   # about 5 % exactly on the threshold: they vote pair_b
    dec[:, :Q] = np.where(eq, rho[None, :], dec[:, :Q])
    full = np.flatnonzero(np.diff(est_off) == k * (k - 1) // 2)
    if m > 1 and k >= 3:
        # row 0, an intra-estimator tie: in every estimator that has all classes, class a beats class b where b - a <= (k - 1) / 2
        # (a circulant tournament for odd k: every class wins (k - 1) / 2 pairs -> the lowest class takes the estimator's vote)
        for e in full:
            q = np.arange(est_off[e], est_off[e + 1])
            a_wins = (pb[q] - pa[q]) <= (k - 1) // 2
            dec[0, q] = rho[q] + np.where(a_wins, 1.0, -1.0)
        # row 1, an ensemble tie: half of the estimators give every pair of class 0 to class 0, the other half every pair of class
        # 1 to class 1 (an odd one out votes for class 2): votes (E // 2, E // 2, E % 2, 0 ...) -> the prediction is class 0
        for e in range(E):
            q = np.arange(est_off[e], est_off[e + 1])
            fav = 2 if (E % 2 and e == E - 1) else (0 if e < E // 2 else 1)
            if fav == 2 and 2 not in set(pa[q]) | set(pb[q]):
                fav = 0
            a_wins = np.where(pa[q] == fav, True, np.where(pb[q] == fav, False, pa[q] < pb[q]))
            dec[1, q] = rho[q] + np.where(a_wins, 0.5, -0.5)
    want_votes, want_pred = vote_rules(dec[:, :Q] - rho[None, :], pa, pb, est_off, k)
    if m > 1 and k >= 3:                                             # the engineered rows are what they are meant to be
        q = np.arange(est_off[full[0]], est_off[full[0] + 1])
        wins = np.bincount(np.where(dec[0, q] - rho[q] > 0, pa[q], pb[q]), minlength=k)
        assert (wins == wins.max()).sum() >= 2
        assert want_votes[1, 0] == want_votes[1, 1] == want_votes[1].max() and want_pred[1] == 0
    votes, pred = run_vote(dec, ld, rho, pa, pb, est_off, m, E, k)
    np.testing.assert_array_equal(votes, want_votes)
    np.testing.assert_array_equal(pred, want_pred)
    np.testing.assert_array_equal(votes.sum(axis=1), np.full(m, E))


@pytest.mark.parametrize('k', [1, 65, 0, -3])
def test_vote_kernel_refuses_a_class_count_outside_2_to_64(k):
    from cross_patient_speech_decoding_amd._lib import XpsError
    with pytest.raises(XpsError, match='k must be in 2..64'):
        run_vote(np.zeros((2, 4)), 4, np.zeros(1), np.zeros(1, dtype=np.int64), np.ones(1, dtype=np.int64), np.array([0, 1]), 2, 1, k)


def test_vote_kernel_takes_64_classes_and_more_problems_than_one_stage():
    """k = 64 (2016 problems per estimator, every lane a class) and 3 estimators: 6048 problems, more than the kernel stages at once."""
    k, E, m = 64, 3, 5
    rng = np.random.default_rng(64)
    pr = pairs_of(list(range(k)))
    pa = np.tile(np.array([a for a, _ in pr]), E)
    pb = np.tile(np.array([b for _, b in pr]), E)
    est_off = np.arange(E + 1) * len(pr)
    Q = len(pa)
    rho = rng.standard_normal(Q)
    dec = rng.standard_normal((m, Q))
    want_votes, want_pred = vote_rules(dec - rho[None, :], pa, pb, est_off, k)
    votes, pred = run_vote(dec, Q, rho, pa, pb, est_off, m, E, k)
    np.testing.assert_array_equal(votes, want_votes)
    np.testing.assert_array_equal(pred, want_pred)


# ------------------------------------------------------------------------------------------------ 2. the scatter kernel
@pytest.mark.parametrize('Q,n', [(1, 1), (37, 1), (1, 301), (37, 301), (3, 4101)])
def test_coef_scatter_equals_numpy(Q, n):
    """Ragged problems (a problem of 2 points among them where the row allows it), a leading dimension beyond n whose padding
    stays untouched, every element of the Q x n block written (the output starts as NaN); n = 4101 spans three column chunks."""
    import torch
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import call
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    rng = np.random.default_rng(Q * 1000 + n)
    sizes = rng.integers(1, min(n, 200) + 1, Q)
    if n >= 2:
        sizes[Q // 2] = 2
    idx = np.concatenate([rng.permutation(n)[:s] for s in sizes]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    npos = np.array([rng.integers(0, s + 1) for s in sizes], dtype=np.int32)
    if n >= 2:
        npos[Q // 2] = 1
    alpha = rng.random(len(idx)) + 0.25
    ldc = n + 3
    want = np.zeros((Q, n))
    for q in range(Q):
        t = np.arange(sizes[q])
        want[q, idx[off[q] + t]] = np.where(t < npos[q], 1.0, -1.0) * alpha[off[q] + t]
    coef = torch.full((Q, ldc), float('nan'), dtype=torch.float64, device=LA.device())
    a_d, i_d, o_d, p_d = dev_tensor(alpha), dev_tensor(idx), dev_tensor(off), dev_tensor(npos)
    call('xps_bag_coef_scatter_f64', a_d.data_ptr(), i_d.data_ptr(), o_d.data_ptr(), p_d.data_ptr(), Q, n, coef.data_ptr(), ldc,
         _dev.stream())
    torch.cuda.synchronize()
    got = coef.cpu().numpy()
    np.testing.assert_array_equal(got[:, :n], want)
    assert np.isnan(got[:, n:]).all()


# ------------------------------------------------------------------------------------------------ 3. the ensemble
def linear_data(n, d, k):
    """The generator of test_hip_svc_equals_libsvm: overlapping classes, labels that are not 0..k-1."""
    rng = np.random.default_rng(n + d)
    centers = rng.standard_normal((k, d)) * 1.2
    sizes = rng.multinomial(n - 4 * k, np.ones(k) / k) + 4
    X = np.vstack([centers[c] + rng.standard_normal((m, d)) for c, m in enumerate(sizes)])
    y = np.repeat(np.arange(k) * 3 + 1, sizes)
    perm = rng.permutation(len(y))
    X, y = X[perm], y[perm]
    Xte = np.vstack([centers[c] + rng.standard_normal((20, d)) for c in range(k)])
    return X, y, Xte, np.repeat(np.arange(k) * 3 + 1, 20), None


def rbf_data(n, d, k, weighted):
    """The generator of test_hip_svc_rbf_and_class_weights_equal_libsvm: imbalanced classes; integer sample weights with zeros."""
    rng = np.random.default_rng(n * 7 + d)
    centers = rng.standard_normal((k, d)) * 1.1
    sizes = rng.multinomial(n - 5 * k, np.linspace(1, 3, k) / np.linspace(1, 3, k).sum()) + 5
    X = np.vstack([centers[c] + rng.standard_normal((m, d)) for c, m in enumerate(sizes)])
    labels = np.arange(k) * 3 + 1
    y = np.repeat(labels, sizes)
    perm = rng.permutation(len(y))
    X, y = X[perm], y[perm]
    Xte = np.vstack([centers[c] + rng.standard_normal((20, d)) for c in range(k)])
    sw = rng.integers(0, 3, len(y)).astype(np.float64)
    return X, y, Xte, np.repeat(labels, 20), (sw if weighted else None)


SHAPES = {
    'linear-120-10-2': dict(data=lambda: linear_data(120, 10, 2), E=10, svc=dict(kernel='linear'), bag={}),
    'linear-300-40-5': dict(data=lambda: linear_data(300, 40, 5), E=10, svc=dict(kernel='linear'), bag={}),
    'rbf-balanced-260-24-9': dict(data=lambda: rbf_data(260, 24, 9, False), E=12,
                                  svc=dict(kernel='rbf', class_weight='balanced', gamma='scale'), bag={}),
    'rbf-nobootstrap-weights-90-8-4': dict(data=lambda: rbf_data(90, 8, 4, True), E=10,
                                           svc=dict(kernel='rbf', class_weight='balanced', gamma='scale'),
                                           bag=dict(max_samples=0.6, bootstrap=False)),
}


@functools.lru_cache(maxsize=None)
def fitted(name):
    """The fused ensemble and both references on one shape, fitted once and shared by the tests below (read-only)."""
    from cross_patient_speech_decoding_amd.decoders import SVC as DeviceSVC
    from cross_patient_speech_decoding_amd.decoders import BaggingClassifier
    s = SHAPES[name]
    X, y, Xte, yte, sw = s['data']()
    kw = dict(n_estimators=s['E'], random_state=0, **s['bag'])
    fused = BaggingClassifier(DeviceSVC(**s['svc']), **kw).fit(X, y, sample_weight=sw)
    sk_dev = SkBagging(DeviceSVC(**s['svc']), **kw).fit(X, y, sample_weight=sw)
    sk_lib = SkBagging(SkSVC(**s['svc']), **kw).fit(X, y, sample_weight=sw)
    return dict(X=X, y=y, Xte=Xte, yte=yte, sw=sw, fused=fused, sk_dev=sk_dev, sk_lib=sk_lib, dec=fused._pair_decisions(Xte))


@pytest.mark.parametrize('name', list(SHAPES))
def test_ensemble_draws_sklearns_samples(name):
    f = fitted(name)
    got, want = f['fused'].estimators_samples_, f['sk_lib'].estimators_samples_
    assert len(got) == len(want) == SHAPES[name]['E']
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(f['fused'].classes_, f['sk_lib'].classes_)
    assert f['fused'].n_classes_ == len(f['sk_lib'].classes_) and f['fused'].n_features_in_ == f['X'].shape[1]
    assert len(f['fused'].n_iter_) == SHAPES[name]['E'] and all((it > 0).all() for it in f['fused'].n_iter_)


@pytest.mark.parametrize('name', list(SHAPES))
def test_ensemble_pair_decisions_equal_the_separately_fitted_device_svcs(name):
    """Two tol = 1e-3 solutions of the same problems: 2e-2 of the scale, the bar of test_hip_svc_equals_libsvm."""
    f = fitted(name)
    ref = np.concatenate([e._pair_decisions(f['Xte']) for e in f['sk_dev'].estimators_], axis=1)
    dec = f['dec']
    assert dec.shape == ref.shape
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(dec - ref).max())
    print(f'{name}: max |dec - ref| = {err:.3e}, scale {scale:.3f}, bound {2e-2 * scale:.3e}')
    assert err <= 2e-2 * scale


@pytest.mark.parametrize('name', list(SHAPES))
def test_ensemble_predicts_as_sklearn_bagging_of_libsvm(name):
    f = fitted(name)
    p_ref, p = f['sk_lib'].predict(f['Xte']), f['fused'].predict(f['Xte'])
    agree = float(np.mean(p == p_ref))
    s_ref, s = f['sk_lib'].score(f['Xte'], f['yte']), f['fused'].score(f['Xte'], f['yte'])
    print(f'{name}: agreement {agree:.4f}, score {s:.4f} (libsvm-bagged {s_ref:.4f}), '
          f'sklearn-bagged device SVC agreement {float(np.mean(f["sk_dev"].predict(f["Xte"]) == p_ref)):.4f}')
    assert agree >= 0.97
    assert abs(s - s_ref) <= 0.03


@pytest.mark.parametrize('name', list(SHAPES))
def test_ensemble_vote_equals_the_rules_on_its_own_decisions(name):
    f = fitted(name)
    fused, y, n = f['fused'], f['y'], len(f['y'])
    classes, yi = np.unique(y, return_inverse=True)
    base = np.ones(n) if f['sw'] is None else f['sw']
    pa, pb, est_off = [], [], [0]
    for s in fused.estimators_samples_:                                  # the classes each estimator kept, from its samples
        w = base * (np.bincount(s, minlength=n) if fused.bootstrap else np.isin(np.arange(n), s))
        for a, b in pairs_of([c for c in range(len(classes)) if (w[yi == c] > 0).any()]):
            pa.append(a)
            pb.append(b)
        est_off.append(len(pa))
    assert f['dec'].shape == (len(f['Xte']), len(pa))
    votes, pred = vote_rules(f['dec'], np.array(pa), np.array(pb), np.array(est_off), len(classes))
    np.testing.assert_array_equal(fused.predict(f['Xte']), classes.take(pred))
    proba = fused.predict_proba(f['Xte'])
    np.testing.assert_array_equal(proba, votes / float(fused.n_estimators))
    np.testing.assert_array_equal(classes.take(proba.argmax(axis=1)), fused.predict(f['Xte']))


# ------------------------------------------------------------------------------------------------ 4. lost classes
def test_estimators_that_lost_a_class_have_fewer_pairs():
    from cross_patient_speech_decoding_amd.decoders import SVC as DeviceSVC
    from cross_patient_speech_decoding_amd.decoders import BaggingClassifier
    rng = np.random.default_rng(5)
    k, d = 3, 6
    centers = rng.standard_normal((k, d)) * 1.5
    sizes = [30, 28, 2]
    X = np.vstack([centers[c] + rng.standard_normal((m, d)) for c, m in enumerate(sizes)])
    y = np.repeat([1, 4, 7], sizes)
    perm = rng.permutation(len(y))
    X, y = X[perm], y[perm]
    Xte = np.vstack([centers[c] + rng.standard_normal((20, d)) for c in range(k)])
    kw = dict(n_estimators=70, max_samples=0.3, random_state=0)
    fused = BaggingClassifier(DeviceSVC(kernel='linear'), **kw).fit(X, y)
    ref = SkBagging(SkSVC(kernel='linear'), **kw).fit(X, y)
    pairs = np.array([len(it) for it in fused.n_iter_])
    lost = np.array([len(np.unique(y[s])) < 3 for s in fused.estimators_samples_])
    assert 20 <= lost.sum() <= 50                                         # about half of the 70 lose the class of two points
    np.testing.assert_array_equal(pairs, np.where(lost, 1, 3))
    assert fused._pair_decisions(Xte).shape == (60, int(pairs.sum()))
    agree = float(np.mean(fused.predict(Xte) == ref.predict(Xte)))
    print(f'lost classes: {int(lost.sum())} of 70 estimators, agreement {agree:.4f}')
    assert agree >= 0.97
    proba = fused.predict_proba(Xte)
    assert proba.shape == (60, 3)
    np.testing.assert_allclose(proba.sum(axis=1), np.ones(60), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(np.rint(proba * 70).sum(axis=1), np.full(60, 70))
    with pytest.raises(ValueError, match='greater than one'):            # an estimator left with one class: as the single SVC
        BaggingClassifier(DeviceSVC(kernel='linear'), n_estimators=70, max_samples=2, random_state=0).fit(X, y)


def test_estimators_that_see_every_row_pose_the_single_svcs_problems():
    """bootstrap=False, max_samples=1.0: every estimator is handed every row with weight 1, so each poses the problems of the
    single SVC on the same kernel matrix, and the one-workgroup SMO takes the same steps: iterations, rho and the pair decisions
    are the single SVC's bit for bit."""
    from cross_patient_speech_decoding_amd.decoders import SVC as DeviceSVC
    from cross_patient_speech_decoding_amd.decoders import BaggingClassifier
    X, y, Xte, _, _ = linear_data(64, 6, 3)
    svc = DeviceSVC(kernel='linear').fit(X, y)
    bag = BaggingClassifier(DeviceSVC(kernel='linear'), n_estimators=2, bootstrap=False, max_samples=1.0).fit(X, y)
    rho, P = bag._rho.cpu().numpy(), len(svc.n_iter_)
    assert P == 3 and rho.shape == (2 * P,) and (svc.n_iter_ > 0).all()
    dec, dec_svc = bag._pair_decisions(Xte), svc._pair_decisions(Xte)
    for e in range(2):
        np.testing.assert_array_equal(bag.n_iter_[e], svc.n_iter_)
        np.testing.assert_array_equal(rho[e * P:(e + 1) * P].view(np.int64), svc._rho.cpu().numpy().view(np.int64))
        np.testing.assert_array_equal(dec[:, e * P:(e + 1) * P].view(np.int64), dec_svc.view(np.int64))


# ------------------------------------------------------------------------------------------------ 5. one launch per fit
def test_one_smo_launch_one_scatter_launch_per_fit_one_vote_launch_per_predict(monkeypatch):
    from collections import Counter
    from cross_patient_speech_decoding_amd import _lib
    from cross_patient_speech_decoding_amd.decoders import SVC as DeviceSVC
    from cross_patient_speech_decoding_amd.decoders import BaggingClassifier
    counts = Counter()
    real = _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    for mod in list(sys.modules.values()):                               # every module that bound `call` by name
        if getattr(mod, '__name__', '').startswith('cross_patient_speech_decoding_amd') and getattr(mod, 'call', None) is real:
            monkeypatch.setattr(mod, 'call', counting)
    X, y, Xte, _, _ = rbf_data(200, 12, 4, False)
    for svc in (dict(kernel='linear'), dict(kernel='rbf', class_weight='balanced')):
        counts.clear()
        bag = BaggingClassifier(DeviceSVC(**svc), n_estimators=12, random_state=4).fit(X, y)
        assert counts['xps_svm_smo_f64'] == 1 and counts['xps_bag_coef_scatter_f64'] == 1, dict(counts)
        assert counts['xps_rbf_from_gram_f64'] == (1 if svc['kernel'] == 'rbf' else 0)
        assert counts['xps_bag_vote_f64'] == 0
        assert counts['xps_dgemm_small'] + counts['xps_dgemm_splitk'] == (2 if svc['kernel'] == 'linear' else 1)   # Gram (+ W)
        counts.clear()
        bag.predict(Xte)
        assert counts['xps_bag_vote_f64'] == 1 and counts['xps_svm_smo_f64'] == 0, dict(counts)
        counts.clear()
        bag.predict_proba(Xte)
        assert counts['xps_bag_vote_f64'] == 1
        again = BaggingClassifier(DeviceSVC(**svc), n_estimators=12, random_state=4).fit(X, y)
        np.testing.assert_array_equal(again._pair_decisions(Xte), bag._pair_decisions(Xte))          # bit for bit


# ------------------------------------------------------------------------------------------------ 6. drop-in
def test_drop_in_for_the_config1_decoder(golden_dir):
    """The reference's decoder (scripts/aligned_decode_svm.py:262-263) with the fused ensemble in the place of sklearn's bagging:
    the bars test_gpu_decoders.py holds the sklearn-bagged route to."""
    import cross_patient_speech_decoding_amd.alignment as A
    from cross_patient_speech_decoding_amd import decoders
    from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
    pats = [make_patient(p, 72 - 6 * p, T=14, C=12 + 2 * p, n_cond=9, noise=2.0) for p in range(3)]
    pats = [(x.astype(np.float64), y) for x, y in pats]
    Xt, yt = pats[0]
    cross = [(x, y[:, 0], y) for x, y in pats[1:]]
    g = np.load(os.path.join(golden_dir, 'decoders_cfg1.npz'))
    tr, te = g['train_idx'], g['test_idx']
    y1 = yt[:, 0]
    dec = decoders.crossPtDecoder_sepAlign(cross, decoders.BaggingClassifier(decoders.SVC(kernel='linear'), n_estimators=10,
                                                                             random_state=0), A.AlignCCA, n_comp=0.9)
    dec.fit(Xt[tr], y1[tr], y_align=yt[tr])
    pred = dec.predict(Xt[te])
    agree = float(np.mean(pred == g['sepAlign_pred']))
    acc = dec.score(Xt[te], y1[te])
    print(f'drop-in: agreement {agree:.4f}, accuracy {acc:.4f} (golden {float(g["sepAlign_acc"]):.4f})')
    assert agree >= 0.97
    assert abs(acc - float(g['sepAlign_acc'])) <= 0.04
