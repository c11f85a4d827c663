"""alignment.fold_plan against plain numpy: group ids, per-fold condition lists, per-(fold, patient) shared-condition index
lists, the CSR descriptors, and the splits it must refuse.  No device."""
import numpy as np
import pytest
from sklearn.model_selection import KFold, StratifiedKFold

from cross_patient_speech_decoding_amd.alignment import fold_plan, label2str
from cross_patient_speech_decoding_amd.alignment.AlignCCA import cca_tail
from cross_patient_speech_decoding_amd.utils.synthetic import make_patient


def _inputs(N=60, n_cond=40, k=5, seed=0):
    y = make_patient(0, N, T=2, C=3, n_cond=n_cond, k=2)[1]
    pool = [make_patient(p, N + 3 * p, T=2, C=3, n_cond=n_cond, k=2)[1] for p in (1, 2, 3)]
    splits = list(KFold(k, shuffle=True, random_state=seed).split(np.zeros(N)))
    return y, pool, splits


def test_group_ids_and_group_csr():
    y, pool, splits = _inputs()
    plan = fold_plan(y, pool, splits)
    assert plan.n_folds == 5 and plan.n_groups == 5 and plan.n_trials == 60
    expect = np.empty(60, dtype=np.int64)
    for f, (_, te) in enumerate(splits):
        expect[te] = f
    np.testing.assert_array_equal(plan.group_of_trial, expect)
    seen = np.zeros(60, dtype=int)
    for g in range(plan.n_groups):
        members = plan.group_order[plan.group_start[g]:plan.group_start[g + 1]]
        np.testing.assert_array_equal(members, np.sort(splits[g][1]))       # ascending trial order
        seen[members] += 1
    np.testing.assert_array_equal(seen, 1)                                   # every trial in exactly one group


def test_uncovered_trials_form_one_group_that_is_never_held_out():
    y, pool, splits = _inputs()
    two = [(np.setdiff1d(np.arange(60), te), te) for _, te in splits[:2]]
    plan = fold_plan(y, pool, two)
    assert plan.n_folds == 2 and plan.n_groups == 3
    rest = np.setdiff1d(np.arange(60), np.concatenate([two[0][1], two[1][1]]))
    np.testing.assert_array_equal(np.flatnonzero(plan.group_of_trial == 2), rest)
    np.testing.assert_array_equal(plan.group_order[plan.group_start[2]:plan.group_start[3]], rest)


@pytest.mark.parametrize('labels_2d', [True, False])
def test_condition_lists_and_csr_per_fold(labels_2d):
    y, pool, splits = _inputs()
    if not labels_2d:
        y, pool = y[:, 0] * 10 + y[:, 1], [p[:, 0] * 10 + p[:, 1] for p in pool]      # 1-D labels: '10' < '2' string order
    plan = fold_plan(y, pool, splits)
    keys = label2str(y)
    lost = 0
    for f, (tr, _) in enumerate(splits):
        uniq = np.unique(keys[tr])
        np.testing.assert_array_equal(plan.cond_keys[f], uniq)
        lost += len(np.unique(keys)) - len(uniq)
        seen = np.zeros(60, dtype=int)
        for c, key in enumerate(uniq):
            members = plan.cond_order[f][plan.cond_start[f][c]:plan.cond_start[f][c + 1]]
            np.testing.assert_array_equal(members, tr[keys[tr] == key])     # boolean-mask order inside `train`
            seen[members] += 1
        np.testing.assert_array_equal(seen[tr], 1)                          # each selected trial exactly once
        assert seen.sum() == len(tr)                                        # and no held-out trial
    assert lost > 0                                                          # the input exercises folds that lose conditions


def test_shared_condition_index_lists_per_fold_and_patient():
    y, pool, splits = _inputs()
    plan = fold_plan(y, pool, splits)
    keys = label2str(y)
    differ = set()
    for f, (tr, _) in enumerate(splits):
        u_f = np.unique(keys[tr])
        for p, yp in enumerate(pool):
            u_p = np.unique(label2str(yp))
            np.testing.assert_array_equal(plan.pool_keys[p], u_p)
            _, i_a, i_b = np.intersect1d(u_f, u_p, assume_unique=True, return_indices=True)
            np.testing.assert_array_equal(plan.shared[f][p][0], i_a)
            np.testing.assert_array_equal(plan.shared[f][p][1], i_b)
            assert len(np.unique(i_a)) == len(i_a) and len(np.unique(i_b)) == len(i_b)     # each condition at most once
            differ.add((p, tuple(i_b)))
    assert len(differ) > len(pool)                                           # the lists do differ between folds


def test_train_runs_cover_train_in_order():
    y, pool, splits = _inputs()
    rng = np.random.default_rng(3)
    shuffled = [(rng.permutation(tr), te) for tr, te in splits]              # `train` need not be sorted
    for sp in (splits, shuffled):
        plan = fold_plan(y, pool, sp)
        for f, (tr, _) in enumerate(sp):
            rebuilt = np.full(len(tr), -1)
            for first, count, dst in plan.train_runs[f]:
                assert (rebuilt[dst:dst + count] == -1).all()
                rebuilt[dst:dst + count] = first + np.arange(count)
            np.testing.assert_array_equal(rebuilt, tr)


def test_stratified_splits_are_accepted():
    y, pool, _ = _inputs(N=48, n_cond=4)
    splits = list(StratifiedKFold(4, shuffle=True, random_state=1).split(np.zeros(48), label2str(y)))
    plan = fold_plan(y, pool, splits)
    assert plan.n_groups == 4 and all(len(k) == 4 for k in plan.cond_keys)


def test_overlapping_test_sets_raise():
    y, pool, splits = _inputs()
    bad = list(splits)
    te = np.concatenate([bad[1][1], bad[0][1][:1]])
    bad[1] = (np.setdiff1d(np.arange(60), te), te)
    with pytest.raises(ValueError, match='overlaps another test set'):
        fold_plan(y, pool, bad)


def test_train_that_is_not_the_complement_raises():
    y, pool, splits = _inputs()
    for train in (splits[0][0][:-1], np.concatenate([splits[0][0], splits[0][1][:1]]),
                  np.concatenate([splits[0][0][:-1], splits[0][0][:1]])):
        bad = [(train, splits[0][1])] + splits[1:]
        with pytest.raises(ValueError, match='not the complement'):
            fold_plan(y, pool, bad)
    with pytest.raises(ValueError, match='outside range'):
        fold_plan(y, pool, [(splits[0][0], np.array([60]))])


@pytest.mark.parametrize('shape,top', [((5, 3), 0.9), ((3, 5), 0.9), ((4, 4), 1.0 + 1e-9)])
def test_the_cca_tail_equals_its_line_by_line_restatement(shape, top):
    """M_a, M_b and the clipped S of ``AlignCCA.cca_tail`` (the end of ``_cca_device`` and of the fold-batched ``_solve_cca``) on a
    tall and a wide K, and on a K whose largest computed singular value lies above 1."""
    rng = np.random.default_rng(shape[0] * 10 + shape[1])
    K = rng.standard_normal(shape)
    K *= top / np.linalg.norm(K, 2)
    U, S, Vt = np.linalg.svd(K, full_matrices=False)
    W_a, W_b = rng.standard_normal((7, shape[0])), rng.standard_normal((6, shape[1]))
    M_a, M_b, S_out = cca_tail(W_a, W_b, U, S, Vt)
    d = min(K.shape)
    np.testing.assert_array_equal(M_a, W_a @ U[:, :d])
    np.testing.assert_array_equal(M_b, W_b @ Vt.T[:, :d])
    ref = S[:d].copy()
    ref[ref < 0] = 0
    ref[ref >= 1] = 1
    np.testing.assert_array_equal(S_out, ref)
    assert M_a.shape == (7, d) and M_b.shape == (6, d) and S_out.shape == (d,) and S_out is not S
    if top > 1:
        assert S[0] > 1 and S_out[0] == 1.0 and (S_out[1:] == S[1:d]).all()      # clipped; the input is not touched
    else:
        assert (S_out == S[:d]).all() and 0 < S_out.min() and S_out.max() < 1
