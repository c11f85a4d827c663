"""decoders.AlignedSVCSearchCV and alignment.fit_folds_multi on the MI355X, end to end.

Data (that of tests/test_gpu_fold_decode.py): ``make_patient(p, N + 3 p, T=20, C=c, n_cond=..., k=6, noise=3.0)``; the decode label
is ``y[:, 0]``, the alignment label the full ``y``; splits ``StratifiedKFold(folds, shuffle=True, random_state=0)``; ``tol=1e-6``,
``class_weight='balanced'``.

Single SVC: expected values are computed on the CPU, per (n_comp, fold) ``oracle.align_oracle.process_aligner`` on float64 values,
then per (C, gamma) sklearn's libsvm SVC.  For every candidate ``cv_test_predictions_`` must equal libsvm's prediction on every
held-out row whose libsvm one-vs-one decisions all have magnitude >= 1e-3 (the project's bar), and at most 10 % of a
candidate's rows may be left out by that rule (a condition on the data, not a tolerance: with the reference path alone the worst
candidate of these grids leaves out 3 of 72 rows in case A and 5 of 90 in case B).

Against ``cross_val_decode`` on the same candidate -- the same engine with that candidate alone -- the search is exact on every row:
same Gram bits, same rbf expression, same deterministic SMO."""
import functools
import sys
from collections import Counter

import numpy as np
import pytest
from sklearn.base import clone
from sklearn.metrics import accuracy_score, balanced_accuracy_score
from sklearn.model_selection import ParameterGrid, StratifiedKFold
from sklearn.svm import SVC as SkSVC

pytestmark = pytest.mark.gpu

from oracle import align_oracle as ao  # noqa: E402
from cross_patient_speech_decoding_amd.utils.synthetic import make_patient  # noqa: E402

T = 20
CASES = {'A': (72, [24, 20, 17], 12, 4), 'B': (90, [33, 20, 40], 18, 5)}           # N, channels (target first), n_cond, folds
TOL = 1e-6
N_COMPS = [0.8, 0.95, 6]
GRIDS = {'rbf': {'n_comp': N_COMPS, 'decoder__C': [1, 10, 100], 'decoder__gamma': ['scale', 1e-4]},
         'linear': {'n_comp': N_COMPS, 'decoder__C': [1e-5, 1e-4, 1]}}
BAGGED_GRID = {'n_comp': N_COMPS, 'decoder__estimator__C': [1e-4, 1]}


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


def _cv(name):
    return StratifiedKFold(_inputs(name)[4], shuffle=True, random_state=0)


def _splits(name):
    y = _inputs(name)[1]
    return list(_cv(name).split(np.zeros(len(y)), y))


def _model(name, kernel):
    return D().crossPtDecoder_sepAlign(_inputs(name)[3], D().SVC(kernel=kernel, class_weight='balanced', tol=TOL), A().AlignCCA, n_comp=0.95)


def _bagged(name):
    ens = D().BaggingClassifier(D().SVC(kernel='linear', class_weight='balanced', tol=TOL), n_estimators=10, random_state=0)
    return D().crossPtDecoder_sepAlign(_inputs(name)[3], ens, A().AlignCCA, n_comp=0.95)


@functools.lru_cache(maxsize=None)
def _search(name, kernel, scoring=None, n_cand=None, max_kernel_bytes=2 ** 30):
    """One fitted search (refit off), shared by the tests that only read it."""
    X, y, yfull, _, _ = _inputs(name)
    cands = list(ParameterGrid(GRIDS[kernel]))[:n_cand]
    return D().AlignedSVCSearchCV(_model(name, kernel), candidates=cands, cv=_cv(name), scoring=scoring, refit=False,
                                  max_kernel_bytes=max_kernel_bytes).fit(X, y, y_align=yfull)


def _same(a, b):
    return (np.array_equal(a.cv_confusion_, b.cv_confusion_) and np.array_equal(a.n_components_, b.n_components_)
            and all(np.array_equal(p, q) and np.array_equal(u, v) for (p, u), (q, v) in zip(a.cv_test_predictions_, b.cv_test_predictions_))
            and np.array_equal(a.cv_results_['mean_test_score'], b.cv_results_['mean_test_score']))


# ------------------------------------------------------------------------------------------------ fit_folds_multi
def test_fit_folds_multi_is_bit_identical_to_separate_fits_and_shares_equal_entries():
    import torch
    X, _, yfull, pool, _ = _inputs('A')
    splits = _splits('A')
    values = [0.8, 0.95, 6, 0.8]
    multi = A().fit_folds_multi(X, yfull, pool, splits, values, append_heldout=True)
    assert len(multi) == 4 and multi[0] is multi[3] and multi[0] is not multi[1] and multi[1] is not multi[2] and multi[0] is not multi[2]
    counts = set()
    for v, fa in zip(values[:3], multi[:3]):
        one = A().fit_folds(X, yfull, pool, splits, n_components=v, append_heldout=True)
        assert fa.n_components_ == one.n_components_ and fa.fallbacks_ == one.fallbacks_
        counts.add(tuple(fa.n_components_))
        for f in range(len(splits)):
            for name in ('pca_mean_', 'pca_components_', 'explained_variance_', 'explained_variance_ratio_all_'):
                assert np.array_equal(getattr(fa, name)[f], getattr(one, name)[f]), (v, f, name)
            for name in ('M_a_', 'M_b_', 'canon_corrs_'):
                for p in range(len(pool)):
                    assert np.array_equal(getattr(fa, name)[f][p], getattr(one, name)[f][p]), (v, f, p, name)
            for p in range(len(pool)):
                assert torch.equal(fa.maps_[f][p], one.maps_[f][p])
            assert torch.equal(fa.train_pool(f), one.train_pool(f))
            assert torch.equal(fa.pool_with_heldout(f)[0], one.pool_with_heldout(f)[0])
            assert np.array_equal(fa.pool_with_heldout(f)[1], one.pool_with_heldout(f)[1])
            assert torch.equal(fa.project(f, splits[f][1]), one.project(f, splits[f][1]))
    assert len(counts) == 3                                        # the three values are three different fits on this data
    plain = A().fit_folds_multi(X, yfull, pool, splits, [6])[0]
    with pytest.raises(ValueError, match='append_heldout'):
        plain.pool_with_heldout(0)
    assert torch.equal(plain.train_pool(1), multi[2].train_pool(1))


# ------------------------------------------------------------------------------------------------ single SVC against libsvm
@functools.lru_cache(maxsize=None)
def _libsvm(name, kernel):
    """{(n_comp, C, gamma): per split (libsvm's predictions, whether every one-vs-one decision is >= 1e-3 away from 0)} and
    {n_comp: the oracle's target component count per split}, on the CPU."""
    X, y, yfull, pool, _ = _inputs(name)
    X64 = X.astype(np.float64)
    pool64 = [(x.astype(np.float64), yy, ya) for x, yy, ya in pool]
    grid = GRIDS[kernel]
    out, comps = {}, {}
    for nc in grid['n_comp']:
        comps[nc] = []
        for tr, te in _splits(name):
            X_pool, y_pool, tar = ao.process_aligner(X64[tr], y[tr], yfull[tr], pool64, n_components=nc)
            comps[nc].append(int(tar.n_components_))
            Ztr = X_pool.reshape(len(X_pool), -1).astype(np.float64)
            Zte = tar.transform(X64[te].reshape(-1, X.shape[-1])).reshape(len(te), -1)
            for C in grid['decoder__C']:
                for gamma in grid.get('decoder__gamma', ['scale']):
                    clf = SkSVC(kernel=kernel, C=C, gamma=gamma, class_weight='balanced', tol=TOL, decision_function_shape='ovo')
                    clf.fit(Ztr, y_pool)
                    dec = clf.decision_function(Zte)
                    out.setdefault((nc, C, gamma), []).append((clf.predict(Zte), (np.abs(dec.reshape(len(te), -1)) >= 1e-3).all(axis=1)))
    return out, comps


@pytest.mark.parametrize('kernel', ['linear', 'rbf'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_every_candidate_predicts_what_libsvm_predicts(name, kernel):
    y = _inputs(name)[1]
    N = len(y)
    search = _search(name, kernel)
    ref, comps = _libsvm(name, kernel)
    splits = _splits(name)
    cands = search.cv_results_['params']
    assert len(cands) == (18 if kernel == 'rbf' else 9) and search.n_splits_ == len(splits) and np.array_equal(search.classes_, np.unique(y))
    assert len(search.cv_test_predictions_) == len(splits)
    ref_scores, worst_left = [], 0
    for c, cand in enumerate(cands):
        key = (cand['n_comp'], cand['decoder__C'], cand.get('decoder__gamma', 'scale'))
        assert list(search.n_components_[c]) == comps[cand['n_comp']], (cand, search.n_components_[c])
        left = wrong = 0
        expected = np.zeros(N, dtype=y.dtype)
        for s, ((tr, te), (pred, ok)) in enumerate(zip(splits, ref[key])):
            te_s, lab = search.cv_test_predictions_[s]
            assert np.array_equal(te_s, te) and lab.shape == (len(cands), len(te))
            left += int((~ok).sum())
            wrong += int((lab[c][ok] != pred[ok]).sum())
            expected[te] = pred
        ref_scores.append(accuracy_score(y, expected))
        worst_left = max(worst_left, left)
        assert left <= 0.10 * N, (cand, left)
        assert wrong == 0, (cand, wrong)
    print(f'case {name} {kernel}: at most {worst_left}/{N} rows of a candidate left out; libsvm accuracies {min(ref_scores):.3f} .. '
          f'{max(ref_scores):.3f}; device mean scores {search.cv_results_["mean_test_score"].min():.3f} .. '
          f'{search.cv_results_["mean_test_score"].max():.3f}')
    # the ranking is not vacuous: libsvm's own accuracies spread over 0.39 .. 0.99 (A linear), 0.83 .. 0.99 (A rbf), 0.20 .. 0.97
    # (B linear) and 0.88 .. 1.00 (B rbf) on these grids
    assert max(ref_scores) - min(ref_scores) > 0.1


# ------------------------------------------------------------------------------------------------ candidates side by side and alone
# cross_val_decode is the one-candidate case of the engine the search runs (fold_decode.run_partition), so these two tests check that a
# candidate among others -- sharing an alignment, a Gram matrix or a kernel matrix with them -- gets exactly what it gets alone.  The
# independent references are libsvm on the CPU (above; tests/test_gpu_fold_decode.py for cross_val_decode itself) and, for the bagged
# model, the per-fold device loop of tests/test_gpu_fold_decode.py.
def _check_against_cross_val_decode(search, model, name):
    X, y, yfull, _, _ = _inputs(name)
    for c, cand in enumerate(search.cv_results_['params']):
        res = D().cross_val_decode(clone(model).set_params(**cand), X, y, y_align=yfull, cv=_cv(name))
        for te, lab in search.cv_test_predictions_:
            assert np.array_equal(lab[c], res.y_pred_[0][te]), cand
        assert np.array_equal(search.cv_confusion_[c].sum(axis=0), res.confusion_[0]), cand
        assert list(search.n_components_[c]) == list(res.alignment_[0].n_components_), cand
    return res


def test_every_rbf_candidate_equals_cross_val_decode_on_every_row():
    _check_against_cross_val_decode(_search('A', 'rbf'), _model('A', 'rbf'), 'A')


def test_a_bagged_linear_svc_equals_cross_val_decode_votes_included():
    X, y, yfull, _, _ = _inputs('A')
    model = _bagged('A')
    search = D().AlignedSVCSearchCV(model, BAGGED_GRID, cv=_cv('A'), scoring='balanced_accuracy', refit=False).fit(X, y, y_align=yfull)
    assert len(search.cv_results_['params']) == 6
    _check_against_cross_val_decode(search, model, 'A')
    # the per-split confusion tables are those of the voted predictions
    yi = np.searchsorted(search.classes_, y)
    for c in range(6):
        for s, (te, lab) in enumerate(search.cv_test_predictions_):
            table = np.zeros_like(search.cv_confusion_[c, s])
            np.add.at(table, (yi[te], np.searchsorted(search.classes_, lab[c])), 1)
            assert np.array_equal(table, search.cv_confusion_[c, s])


# ------------------------------------------------------------------------------------------------ bookkeeping
@pytest.mark.parametrize('scoring', [None, 'accuracy', 'balanced_accuracy'])
def test_scores_are_sklearns_metric_on_the_devices_own_predictions(scoring):
    y = _inputs('A')[1]
    search = _search('A', 'rbf', scoring)
    metric = balanced_accuracy_score if scoring == 'balanced_accuracy' else accuracy_score
    res = search.cv_results_
    n_cand = len(res['params'])
    table = np.array([[metric(y[te], lab[c]) for te, lab in search.cv_test_predictions_] for c in range(n_cand)])
    for s in range(search.n_splits_):
        np.testing.assert_array_equal(res[f'split{s}_test_score'], table[:, s])
    np.testing.assert_allclose(res['mean_test_score'], table.mean(axis=1), rtol=1e-15, atol=0)
    np.testing.assert_allclose(res['std_test_score'], table.std(axis=1), rtol=1e-12, atol=1e-15)
    rank = res['rank_test_score']
    assert rank.min() == 1 and search.best_index_ == int(np.flatnonzero(rank == rank.min())[0])
    assert search.best_params_ == res['params'][search.best_index_]
    assert search.best_score_ == res['mean_test_score'][search.best_index_] == res['mean_test_score'].max()
    assert res['params'] == list(ParameterGrid(GRIDS['rbf']))
    for key in GRIDS['rbf']:
        assert list(res[f'param_{key}']) == [p[key] for p in res['params']]
    k = len(np.unique(y))
    assert search.cv_confusion_.shape == (n_cand, 4, k, k) and search.n_components_.shape == (n_cand, 4)
    assert (search.cv_confusion_.sum(axis=(2, 3)) == [len(te) for te, _ in search.cv_test_predictions_]).all()
    assert res['mean_test_score'].max() - res['mean_test_score'].min() > 0.1   # (libsvm's accuracies spread over 0.83 .. 0.99 here)
    with pytest.raises(AttributeError, match='best_estimator_'):
        search.predict(_inputs('A')[0][:2])


def test_refit_fits_the_best_candidate_on_all_trials():
    X, y, yfull, _, _ = _inputs('A')
    model = _model('A', 'linear')
    grid = {'n_comp': [0.8, 6], 'decoder__C': [1e-4, 1]}
    search = D().AlignedSVCSearchCV(model, grid, cv=_cv('A')).fit(X[:60], y[:60], y_align=yfull[:60])
    assert model.n_comp == 0.95 and model.decoder.C == 1.0         # the model handed over is left as it was
    own = clone(model).set_params(**search.best_params_)
    own.fit(X[:60], y[:60], y_align=yfull[:60])
    np.testing.assert_array_equal(search.predict(X[60:]), own.predict(X[60:]))
    assert search.score(X[60:], y[60:]) == own.score(X[60:], y[60:])
    assert search.best_estimator_.n_comp == search.best_params_['n_comp']


# ------------------------------------------------------------------------------------------------ launches and chunks
def _count_calls(monkeypatch):
    from cross_patient_speech_decoding_amd import _lib
    counts, real = Counter(), _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    D()
    for mod in list(sys.modules.values()):                               # every module that bound `call` by name
        if getattr(mod, '__name__', '').startswith('cross_patient_speech_decoding_amd') and getattr(mod, 'call', None) is real:
            monkeypatch.setattr(mod, 'call', counting)
    return counts


def test_the_launch_count_does_not_depend_on_the_number_of_candidates(monkeypatch):
    X, y, yfull, _, _ = _inputs('A')
    counts = _count_calls(monkeypatch)
    seen = []
    cands = list(ParameterGrid(GRIDS['rbf']))
    six = [c for c in cands if c['decoder__C'] == 1]                # all three n_comp values and both gammas
    assert len(six) == 6
    for some in (cands, six):
        counts.clear()
        D().AlignedSVCSearchCV(_model('A', 'rbf'), candidates=some, cv=_cv('A'), refit=False).fit(X, y, y_align=yfull)
        print(len(some), 'candidates:', dict(counts))
        for entry in ('xps_rbf_grouped_from_gram_f64', 'xps_gram_grouped_f64', 'xps_svm_smo_multi_f64', 'xps_svm_cv_score_f64'):
            assert counts[entry] == 1, (entry, dict(counts))                             # one chunk
        assert counts['xps_var_grouped_f64'] == 1                                        # one partition
        for entry in ('xps_rbf_from_gram_f64', 'xps_rbf_multi_from_gram_f64', 'xps_svm_smo_f64', 'xps_bag_vote_f64'):
            assert counts[entry] == 0, (entry, dict(counts))
        seen.append(dict(counts))
    assert seen[0] == seen[1]
    counts.clear()                                                  # a linear kernel: no rbf map and no variance launch
    D().AlignedSVCSearchCV(_model('A', 'linear'), GRIDS['linear'], cv=_cv('A'), refit=False).fit(X, y, y_align=yfull)
    assert counts['xps_gram_grouped_f64'] == counts['xps_svm_smo_multi_f64'] == counts['xps_svm_cv_score_f64'] == 1
    assert counts['xps_rbf_grouped_from_gram_f64'] == counts['xps_var_grouped_f64'] == counts['xps_rbf_from_gram_f64'] == 0


def test_every_chunking_gives_the_same_results_with_one_launch_of_each_kernel_per_chunk(monkeypatch):
    from cross_patient_speech_decoding_amd.decoders import fold_decode as FD
    whole = _search('A', 'rbf')
    X, y, yfull, _, _ = _inputs('A')
    largest = 8 * max(len(tr) + len(te) + sum(len(x) for x, _, _ in _inputs('A')[3]) for tr, te in _splits('A')) ** 2
    counts = _count_calls(monkeypatch)
    chunks = []
    real = FD.cut_plan_chunks
    monkeypatch.setattr(FD, 'cut_plan_chunks', lambda *a: chunks.append(real(*a)) or chunks[-1])
    for limit in (8 * largest, 2 * largest):
        counts.clear()
        cut = D().AlignedSVCSearchCV(_model('A', 'rbf'), GRIDS['rbf'], cv=_cv('A'), refit=False, max_kernel_bytes=limit).fit(X, y, y_align=yfull)
        assert _same(whole, cut)
        n_chunks = len(chunks[-1])
        assert n_chunks > 1 and sorted(m for ch in chunks[-1] for m in ch) == list(range(24))   # 3 alignments x 4 folds x 2 gammas
        for entry in ('xps_rbf_grouped_from_gram_f64', 'xps_gram_grouped_f64', 'xps_svm_smo_multi_f64', 'xps_svm_cv_score_f64'):
            assert counts[entry] == n_chunks, (entry, n_chunks, dict(counts))
        assert counts['xps_var_grouped_f64'] == 1 and counts['xps_rbf_from_gram_f64'] == 0
    assert len(chunks[1]) == 24                                     # one matrix and its Gram per chunk
    with pytest.raises(ValueError, match='max_kernel_bytes'):
        D().AlignedSVCSearchCV(_model('A', 'rbf'), GRIDS['rbf'], cv=_cv('A'), refit=False, max_kernel_bytes=largest - 1).fit(X, y, y_align=yfull)
