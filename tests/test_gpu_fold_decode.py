"""decoders.cross_val_decode on the MI355X, end to end.

Data: ``make_patient(p, N + 3 p, T=20, C=c, n_cond=..., k=6, noise=3.0)``; the decode label is ``y[:, 0]``, the alignment label the
full ``y``; splits ``StratifiedKFold(folds, shuffle=True, random_state=0)``; ``tol=1e-6``.

Single SVC (linear and rbf, ``class_weight='balanced'``): expected values are computed on the CPU, per fold
``oracle.align_oracle.process_aligner`` on float64 values, then sklearn's libsvm SVC.  ``y_pred_`` must equal libsvm's prediction on
every held-out row whose libsvm one-vs-one decisions all have magnitude >= 1e-3 (the project's bar), and at most
10 % of the rows may be left out by that rule (a condition on the data, not a tolerance).

Bagged linear SVC (E = 10, ``random_state=0``): expected values come from the per-fold loop over a clone of the model fitted and
asked on the device with the same seed: equal draws, equal predictions on every row whose per-fold vote margin is >= 2 (at most
10 % of the rows left out), balanced accuracy within 0.04."""
import functools
import sys

import numpy as np
import pytest
from sklearn.base import clone
from sklearn.metrics import accuracy_score, balanced_accuracy_score
from sklearn.model_selection import RepeatedStratifiedKFold, StratifiedKFold
from sklearn.svm import SVC as SkSVC

pytestmark = pytest.mark.gpu

from oracle import align_oracle as ao  # noqa: E402
from cross_patient_speech_decoding_amd.utils.synthetic import make_patient  # noqa: E402

T = 20
CASES = {'A': (72, [24, 20, 17], 12, 4), 'B': (90, [33, 20, 40], 18, 5)}           # N, channels (target first), n_cond, folds
TOL = 1e-6
N_COMP = 0.95


def D():
    import cross_patient_speech_decoding_amd.decoders as d
    return d


def A():
    import cross_patient_speech_decoding_amd.alignment as a
    return a


@functools.lru_cache(maxsize=None)
def _inputs(name):
    N, Cs, n_cond, folds = CASES[name]
    pats = [make_patient(p, N + 3 * p, T=T, C=c, n_cond=n_cond, k=6, noise=3.0) for p, c in enumerate(Cs)]
    X, yfull = pats[0]
    pool = [(x, yy[:, 0].copy(), yy) for x, yy in pats[1:]]
    return X, yfull[:, 0].copy(), yfull, pool, folds


def _splits(name, cv=None):
    X, y, _, _, folds = _inputs(name)
    cv = StratifiedKFold(folds, shuffle=True, random_state=0) if cv is None else cv
    return list(cv.split(np.zeros(len(y)), y))


def _model(name, decoder, pool=None, **kw):
    pool = _inputs(name)[3] if pool is None else pool
    return D().crossPtDecoder_sepAlign(pool, decoder, A().AlignCCA, n_comp=N_COMP, **kw)


def _svc(kernel):
    return D().SVC(kernel=kernel, class_weight='balanced', tol=TOL)


@functools.lru_cache(maxsize=None)
def _libsvm(name, kernel, tar_in_train=True, align='full', cv=None):
    """Per split, on the CPU: (held-out trials, libsvm's predictions, whether every one-vs-one decision is >= 1e-3 away from 0)."""
    X, y, yfull, pool, _ = _inputs(name)
    X64 = X.astype(np.float64)
    y_al = yfull if align == 'full' else None                                       # None: the decode label aligns
    pool64 = [(x.astype(np.float64), yy, ya if align == 'full' else yy) for x, yy, ya in pool]
    out = []
    for tr, te in _splits(name, cv):
        X_pool, y_pool, tar = ao.process_aligner(X64[tr], y[tr], None if y_al is None else y_al[tr], pool64, n_components=N_COMP)
        first = 0 if tar_in_train else len(tr)
        clf = SkSVC(kernel=kernel, class_weight='balanced', tol=TOL, decision_function_shape='ovo')
        clf.fit(X_pool[first:].reshape(len(X_pool) - first, -1).astype(np.float64), y_pool[first:])
        Zte = tar.transform(X64[te].reshape(-1, X.shape[-1])).reshape(len(te), -1)
        dec = clf.decision_function(Zte)
        out.append((te, clf.predict(Zte), (np.abs(dec.reshape(len(te), -1)) >= 1e-3).all(axis=1)))
    return out


def _check_against_libsvm(res_pred, ref, y, what):
    """res_pred (N,): equal to libsvm on the rows the bar keeps; at most 10 % left out."""
    N = len(y)
    expected, kept = np.zeros(N, dtype=y.dtype), np.zeros(N, dtype=bool)
    for te, pred, ok in ref:
        expected[te], kept[te] = pred, ok
    left = int(N - kept.sum())
    wrong = int((res_pred[kept] != expected[kept]).sum())
    print(f'{what}: {left}/{N} rows left out, libsvm accuracy {accuracy_score(y, expected):.3f}, device accuracy '
          f'{accuracy_score(y, res_pred):.3f}, {wrong} kept rows differ, {int((res_pred != expected).sum())} rows differ in all')
    assert left <= 0.10 * N, (what, left)
    assert 0.5 < accuracy_score(y, expected) < 1.0                                  # the predictions are not trivially right
    np.testing.assert_array_equal(res_pred[kept], expected[kept])


def _check_fields(res, y, R):
    N, k = len(y), len(np.unique(y))              # (every pooled patient shows the target's classes and no other)
    assert res.y_pred_.shape == (R, N) and res.votes_.shape == (R, N, k) and res.votes_.dtype == np.int32
    assert res.fold_of_trial_.shape == (R, N) and res.confusion_.shape == (R, k, k)
    assert res.accuracy_.shape == (R,) and res.balanced_accuracy_.shape == (R,) and len(res.alignment_) == R
    assert np.array_equal(res.classes_, np.unique(y))
    for r in range(R):
        assert res.confusion_[r].sum() == N
        assert res.accuracy_[r] == accuracy_score(y, res.y_pred_[r])
        assert res.balanced_accuracy_[r] == balanced_accuracy_score(y, res.y_pred_[r])
        assert np.array_equal(res.classes_[res.votes_[r].argmax(axis=1)], res.y_pred_[r])


# ------------------------------------------------------------------------------------------------ single SVC against libsvm
@pytest.mark.parametrize('kernel', ['linear', 'rbf'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_single_svc_predicts_what_libsvm_predicts(name, kernel):
    X, y, yfull, _, folds = _inputs(name)
    res = D().cross_val_decode(_model(name, _svc(kernel)), X, y, y_align=yfull, cv=StratifiedKFold(folds, shuffle=True, random_state=0))
    _check_fields(res, y, 1)
    assert (res.votes_.sum(axis=2) == 1).all() and res.estimators_samples_ == [[[]] * folds]
    for f, (tr, te) in enumerate(_splits(name)):
        assert (res.fold_of_trial_[0, te] == f).all()
    _check_against_libsvm(res.y_pred_[0], _libsvm(name, kernel), y, f'case {name} {kernel}')


@pytest.mark.parametrize('kernel', ['linear', 'rbf'])
def test_tar_in_train_false(kernel):
    X, y, yfull, _, folds = _inputs('A')
    res = D().cross_val_decode(_model('A', _svc(kernel), tar_in_train=False), X, y, y_align=yfull,
                               cv=StratifiedKFold(folds, shuffle=True, random_state=0))
    _check_fields(res, y, 1)
    _check_against_libsvm(res.y_pred_[0], _libsvm('A', kernel, tar_in_train=False), y, f'case A {kernel} tar_in_train=False')


def test_y_align_none_aligns_on_the_decode_label():
    X, y, _, pool, folds = _inputs('A')
    pool1 = [(x, yy, yy) for x, yy, _ in pool]
    res = D().cross_val_decode(_model('A', _svc('linear'), pool=pool1), X, y, cv=StratifiedKFold(folds, shuffle=True, random_state=0))
    _check_fields(res, y, 1)
    _check_against_libsvm(res.y_pred_[0], _libsvm('A', 'linear', align='decode'), y, 'case A linear y_align=None')


def test_repeated_stratified_k_fold_gives_one_row_per_repeat():
    X, y, yfull, _, _ = _inputs('A')
    cv = RepeatedStratifiedKFold(n_splits=4, n_repeats=2, random_state=0)
    res = D().cross_val_decode(_model('A', _svc('linear')), X, y, y_align=yfull, cv=cv)
    _check_fields(res, y, 2)
    ref = _libsvm('A', 'linear', cv=cv)
    assert len(ref) == 8
    for r in range(2):
        _check_against_libsvm(res.y_pred_[r], ref[4 * r:4 * r + 4], y, f'case A linear repeat {r}')
    assert not np.array_equal(res.fold_of_trial_[0], res.fold_of_trial_[1])


# ------------------------------------------------------------------------------------------------ the bagged ensemble
def _bagged(name):
    return _model(name, D().BaggingClassifier(D().SVC(kernel='linear', tol=TOL), n_estimators=10, random_state=0))


@functools.lru_cache(maxsize=None)
def _loop(name):
    """The per-fold loop on the device: per split (held-out trials, predictions, vote margin, draws)."""
    X, y, yfull, _, _ = _inputs(name)
    out = []
    for tr, te in _splits(name):
        m = clone(_bagged(name))
        m.fit(X[tr], y[tr], y_align=yfull[tr])
        counts = np.sort(np.rint(m.decoder.predict_proba(m.preprocess_test(X[te])) * 10), axis=1)
        out.append((te, m.predict(X[te]), counts[:, -1] - counts[:, -2], m.decoder.estimators_samples_))
    return out


@pytest.mark.parametrize('name', sorted(CASES))
def test_bagged_linear_svc_against_the_per_fold_loop(name):
    X, y, yfull, _, folds = _inputs(name)
    N = len(y)
    res = D().cross_val_decode(_bagged(name), X, y, y_align=yfull, cv=StratifiedKFold(folds, shuffle=True, random_state=0))
    _check_fields(res, y, 1)
    assert (res.votes_.sum(axis=2) == 10).all()
    expected, kept = np.zeros(N, dtype=y.dtype), np.zeros(N, dtype=bool)
    for f, (te, pred, margin, draws) in enumerate(_loop(name)):
        expected[te], kept[te] = pred, margin >= 2
        assert len(res.estimators_samples_[0][f]) == 10
        for a, b in zip(res.estimators_samples_[0][f], draws):
            np.testing.assert_array_equal(a, b)
    left = int(N - kept.sum())
    loop_score = balanced_accuracy_score(y, expected)
    print(f'case {name} bagged: {left}/{N} rows left out, balanced accuracy fused {res.balanced_accuracy_[0]:.4f} loop {loop_score:.4f}, '
          f'{int((res.y_pred_[0] != expected).sum())} rows differ in all')
    assert left <= 0.10 * N, left
    np.testing.assert_array_equal(res.y_pred_[0][kept], expected[kept])
    assert abs(res.balanced_accuracy_[0] - loop_score) <= 0.04


# ------------------------------------------------------------------------------------------------ invariance and launches
def _same(a, b):
    return (np.array_equal(a.y_pred_, b.y_pred_) and np.array_equal(a.votes_, b.votes_) and np.array_equal(a.confusion_, b.confusion_)
            and np.array_equal(a.balanced_accuracy_, b.balanced_accuracy_))


@pytest.mark.parametrize('which', ['bagged', 'rbf'])
def test_two_runs_and_every_chunking_give_the_same_bits(which, monkeypatch):
    from cross_patient_speech_decoding_amd.decoders import fold_decode as FD
    from cross_patient_speech_decoding_amd.decoders.search import cut_chunks
    X, y, yfull, _, folds = _inputs('A')
    rbf = which == 'rbf'
    model = _model('A', _svc('rbf')) if rbf else _bagged('A')
    cv = StratifiedKFold(folds, shuffle=True, random_state=0)
    cuts, real = [], FD.cut_plan_chunks                                  # what the engine cut, call by call
    monkeypatch.setattr(FD, 'cut_plan_chunks', lambda *args: cuts.append(real(*args)) or cuts[-1])
    a = D().cross_val_decode(model, X, y, y_align=yfull, cv=cv)
    assert _same(a, D().cross_val_decode(model, X, y, y_align=yfull, cv=cv))
    rows = [a.alignment_[0].pool_with_heldout(f)[0].shape[0] for f in range(folds)]
    per_fold = [8 * n ** 2 for n in rows]
    assert len(cut_chunks(per_fold, 2 ** 30)) == 1 and [len(c) for c in cuts] == [1, 1]
    # the engine's own rule on a one-candidate plan: a chunk holds its kernel matrices and, for rbf, the Gram matrix of each of their
    # views -- with one candidate a second matrix per fold, so the limits that hold 4, 2 and 1 linear folds hold 2, 1 and 1 rbf folds
    plan = FD.build_plan([dict(C=1.0, gamma=1.0 if rbf else None)], [0], [rows], 'rbf' if rbf else 'linear', lambda al, f, spec: spec)
    for max_bytes, chunks in ((4 * max(per_fold), 2 if rbf else 1), (2 * max(per_fold), folds if rbf else 2), (max(per_fold), folds)):
        assert len(cut_chunks(per_fold, max_bytes)) == {4: 1, 2: 2, 1: folds}[max_bytes // max(per_fold)]
        assert len(real(plan, rbf, max_bytes)) == chunks
        assert _same(a, D().cross_val_decode(model, X, y, y_align=yfull, cv=cv, max_bytes=max_bytes))
        assert len(cuts[-1]) == chunks and [m for ch in cuts[-1] for m in ch] == list(range(folds))
        if rbf and max_bytes == max(per_fold):                           # F chunks, each one matrix plus its Gram
            assert all(FD.chunk_bytes(plan, ch, True) == 2 * max(per_fold) for ch in cuts[-1])
    with pytest.raises(ValueError, match='too small'):
        D().cross_val_decode(model, X, y, y_align=yfull, cv=cv, max_bytes=max(per_fold) - 1)


def test_one_launch_of_each_kernel_for_all_folds_and_estimators(monkeypatch):
    from collections import Counter
    from cross_patient_speech_decoding_amd import _lib
    counts, real = Counter(), _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    D()
    for mod in list(sys.modules.values()):                               # every module that bound `call` by name
        if getattr(mod, '__name__', '').startswith('cross_patient_speech_decoding_amd') and getattr(mod, 'call', None) is real:
            monkeypatch.setattr(mod, 'call', counting)
    X, y, yfull, _, folds = _inputs('A')
    cv = StratifiedKFold(folds, shuffle=True, random_state=0)
    # (model, rbf map launches, variance launches): gamma='scale' is the SVC's default; a float gamma needs no variance
    for model, rbf, var in ((_bagged('A'), 0, 0), (_model('A', _svc('linear')), 0, 0), (_model('A', _svc('rbf')), 1, 1),
                            (_model('A', D().SVC(kernel='rbf', gamma=1e-4, class_weight='balanced', tol=TOL)), 1, 0)):
        counts.clear()
        D().cross_val_decode(model, X, y, y_align=yfull, cv=cv)
        print(dict(counts))
        for entry in ('xps_gram_grouped_f64', 'xps_svm_smo_multi_f64', 'xps_svm_cv_score_f64'):
            assert counts[entry] == 1, (entry, dict(counts))
        assert counts['xps_rbf_grouped_from_gram_f64'] == rbf, dict(counts)     # ONE launch for the F folds
        assert counts['xps_var_grouped_f64'] == var, dict(counts)
        assert counts['xps_rbf_from_gram_f64'] == 0, dict(counts)
        for entry in ('xps_svm_smo_f64', 'xps_bag_vote_f64', 'xps_bag_coef_scatter_f64', 'xps_rbf_multi_from_gram_f64'):
            assert counts[entry] == 0, (entry, dict(counts))
