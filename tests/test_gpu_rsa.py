"""alignment/rsa.py on the MI355X: calc_rdm_corr and compare_rdms against the golden fixture (the reference notebook's own functions)
and the long-double restatement of tests/rsa_ref.py within its bars, on float32 and float64 input; the bit-for-bit promises of the
batched forms (the ``_many`` forms equal the single calls, any chunking gives the same bits, null_[q][r] is compare_rdms on the
host-permuted second matrix); the p-values; the launch counts; and rdm_alignment_scores.

The notebook's numbers carry scipy's own rounding (a bar of the same form as the device's), so the device may differ from the
fixture by the sum of both bars."""
import os
import sys

import numpy as np
import pytest

import rsa_ref as RR

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rsa.npz'))
CASES = RR.cases()
NAMES = sorted(CASES)
SEED = 5
_rdms = {}


def RSA():
    from cross_patient_speech_decoding_amd.alignment import rsa
    return rsa


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def rdms():
    """calc_rdm_corr_many of all cases, computed once and left unchanged."""
    if not _rdms:
        out = RSA().calc_rdm_corr_many([CASES[n][0] for n in NAMES], [CASES[n][1] for n in NAMES])
        _rdms.update(dict(zip(NAMES, out)))
    return _rdms


def all_pairs():
    """Every ordered pair of different cases that shares at least 3 conditions, and two cases with themselves, as indices into NAMES."""
    uniq = [RR.cnd_means(*CASES[n])[1] for n in NAMES]
    return [(a, b) for a in range(len(NAMES)) for b in range(len(NAMES))
            if (a != b or a in (0, 3)) and len(np.intersect1d(uniq[a], uniq[b])) >= 3]


def count_calls(monkeypatch):
    from collections import Counter
    from cross_patient_speech_decoding_amd import _lib
    counts, real = Counter(), _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    for mod in list(sys.modules.values()):                               # every module that bound `call` by name
        if getattr(mod, '__name__', '').startswith('cross_patient_speech_decoding_amd') and getattr(mod, 'call', None) is real:
            monkeypatch.setattr(mod, 'call', counting)
    return counts


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('name', NAMES)
def test_calc_rdm_corr_follows_the_notebook_and_the_restatement(name):
    import torch
    rsa = RSA()
    data, labels = CASES[name]
    rdm, uniq = rdms()[name]
    ca, want_uniq = RR.cnd_means(data, labels)
    assert np.array_equal(uniq, want_uniq) and np.array_equal(uniq, GOLD[f'{name}/unique_labels'])
    assert rdm.dtype == np.float64 and rdm.shape == (len(uniq), len(uniq))
    ref, bar = RR.rdm_ref(ca), RR.corr_bar(ca)
    assert bar.max() < 1e-9
    err = np.abs(rdm.astype(RR.LD) - ref)
    assert (err <= bar).all(), f'off by {float(err.max()):.3e}'
    off = ~np.eye(len(uniq), dtype=bool)
    assert (np.abs(rdm - GOLD[f'{name}/rdm'])[off] <= 2 * bar[off]).all()
    assert (np.diag(rdm) == 0.0).all() and np.array_equal(bits(rdm), bits(rdm.T))
    print(f'{name}: largest fraction of the bar {float((err / bar).max()):.2e}')
    # the single call, a flattened (n_trials, D) input and a device tensor give the same bits as the batch
    single, single_uniq = rsa.calc_rdm_corr(data, labels)
    assert np.array_equal(bits(single), bits(rdm)) and np.array_equal(single_uniq, uniq)
    assert np.array_equal(bits(rsa.calc_rdm_corr(data.reshape(len(data), -1), labels)[0]), bits(rdm))
    assert np.array_equal(bits(rsa.calc_rdm_corr(torch.from_numpy(data).cuda(), labels)[0]), bits(rdm))


def test_a_constant_condition_average_gives_nan_in_its_row_and_column():
    rsa = RSA()
    data, labels = CASES['a_n130_T5_d4_k9']
    data = data.copy()
    data[labels == 4] = 0.25                                              # every trial of one condition: a constant average
    rdm, uniq = rsa.calc_rdm_corr(data, labels)
    i = int(np.flatnonzero(uniq == '4')[0])
    nan = np.isnan(rdm)
    assert nan[i].all() and nan[:, i].all() and nan.sum() == 2 * len(uniq) - 1
    assert (np.delete(np.diag(rdm), i) == 0.0).all()
    with pytest.raises(ValueError, match='length at least 2'):
        rsa.compare_rdms_many([rdm[:2, :2]], [uniq[:2]], [(0, 0)])


def test_compare_rdms_follows_the_notebook_the_restatement_and_cos_sim():
    rsa = RSA()
    for (a, b), pearson, cosine in zip(GOLD['pairs'], GOLD['pearson'], GOLD['cosine']):
        (A, ua), (B, ub) = rdms()[a], rdms()[b]
        shared, ia, ib = RR.shared_indices(ua, ub)
        x, y = RR.triangle(A, ia), RR.triangle(B, ib)
        for method, gold in (('pearson', pearson), ('cosine', cosine)):
            got = rsa.compare_rdms(A, ua, B, ub, method=method)
            bar = RR.compare_bar(x, y, method)
            assert isinstance(got, float) and bar < 1e-9
            assert abs(got - RR.compare_ref(A, ia, B, ib, method=method)) <= bar
        assert rsa.compare_rdms(A, ua, B, ub) == rsa.compare_rdms(A, ua, B, ub, method='pearson')
        # against the notebook's numbers: its RDMs differ from the device's within corr_bar, which moves the comparison by at
        # most the largest entry error over the spread of the triangle, on both sides
        slack = sum(2 * RR.corr_bar(RR.cnd_means(*CASES[n])[0]).max() / np.std(t) for n, t in ((a, x), (b, y)))
        assert abs(rsa.compare_rdms(A, ua, B, ub) - pearson) <= RR.compare_bar(x, y) + 2 * slack
        assert abs(rsa.compare_rdms(A, ua, B, ub, method='cosine') - cosine) <= RR.compare_bar(x, y, 'cosine') + 2 * slack
        # the notebook's own matrices through the device comparison: only the comparison's bar is left
        GA, GB = GOLD[f'{a}/rdm'], GOLD[f'{b}/rdm']
        GA, GB = 0.5 * (GA + GA.T), 0.5 * (GB + GB.T)
        gx, gy = RR.triangle(GA, ia), RR.triangle(GB, ib)
        assert abs(rsa.compare_rdms(GA, ua, GB, ub) - RR.compare_ref(GA, ia, GB, ib)) <= RR.compare_bar(gx, gy)


# ------------------------------------------------------------------------------------------------ bit-for-bit promises
@pytest.mark.parametrize('R', (0, 1, 65))
def test_chunks_nulls_p_values_and_launch_counts(R, monkeypatch):
    rsa = RSA()
    from cross_patient_speech_decoding_amd.alignment.metrics import permutation_p_value
    mats, labs = [rdms()[n][0] for n in NAMES], [rdms()[n][1] for n in NAMES]
    pairs = all_pairs()
    assert len(pairs) >= 8 and len({len(np.intersect1d(labs[a], labs[b])) for a, b in pairs}) >= 3         # several m in one call
    counts = count_calls(monkeypatch)
    whole = rsa.compare_rdms_many(mats, labs, pairs, n_permutations=R, random_state=SEED)
    assert dict(counts) == {'xps_rdm_compare_perm_f64': 1}               # one library call (two launches) per chunk, whatever R is
    assert whole.similarity_.shape == (len(pairs),) and whole.null_.shape == (len(pairs), R) and whole.n_permutations == R
    assert whole.similarity_.dtype == np.float64 and whole.null_.dtype == np.float64
    per_pair = 8 * (R + 5)
    for chunks, max_bytes in ((len(pairs), 1), (2, per_pair * -(-len(pairs) // 2)), (1, 2 ** 28)):
        counts.clear()
        cut = rsa.compare_rdms_many(mats, labs, pairs, n_permutations=R, random_state=SEED, max_bytes=max_bytes)
        assert dict(counts) == {'xps_rdm_compare_perm_f64': chunks}
        assert np.array_equal(bits(cut.similarity_), bits(whole.similarity_)) and np.array_equal(bits(cut.null_), bits(whole.null_))
        assert np.array_equal(cut.p_value_, whole.p_value_)
    # the tables: one per distinct m in ascending m, drawn in order; null_[q][r] is compare_rdms on the host-permuted matrix
    ms = [len(np.intersect1d(labs[a], labs[b])) for a, b in pairs]
    tables = RR.permutation_tables(ms, R, np.random.RandomState(SEED))
    assert np.array_equal(whole.n_shared_, ms)
    for q, (a, b) in enumerate(pairs):
        shared, ia, ib = RR.shared_indices(labs[a], labs[b])
        assert np.array_equal(whole.shared_labels_[q], shared)
        assert whole.similarity_[q] == rsa.compare_rdms(mats[a], labs[a], mats[b], labs[b])          # the single call's bits
        x = RR.triangle(mats[a], ia)
        for r in range(1, R + 1):                                        # every permutation of every pair against the restatement
            p = tables[len(shared)][r]
            bar = RR.compare_bar(x, RR.triangle(mats[b], ib[p]))
            assert abs(whole.null_[q, r - 1] - RR.compare_ref(mats[a], ia, mats[b], ib, p)) <= bar < 1e-9, (q, r)
            if r in (1, R // 2, R):
                # compare_rdms on the host-permuted second matrix (which sums its own triangle in another order: equal within
                # both calls' bars, not bit for bit)
                moved = mats[b][np.ix_(ib[p], ib[p])]
                assert abs(whole.null_[q, r - 1] - rsa.compare_rdms(mats[a], labs[a], moved, shared)) <= 2 * bar
        values = np.concatenate([[whole.similarity_[q]], whole.null_[q]])
        assert whole.p_value_[q] == permutation_p_value(values, R)
        assert whole.p_value_[q] == (1 + np.count_nonzero(whole.null_[q] >= whole.similarity_[q])) / (1 + R)
    # random_state=None draws from numpy's global generator, as a host loop would
    np.random.seed(3)
    glob = rsa.compare_rdms_many(mats, labs, pairs, n_permutations=R)
    np.random.seed(3)
    seeded = RR.permutation_tables(ms, R, np.random)
    again = rsa.compare_rdms_many(mats, labs, pairs, n_permutations=R, random_state=np.random.RandomState(3))
    for q, (a, b) in enumerate(pairs[:3]):
        shared, ia, ib = RR.shared_indices(labs[a], labs[b])
        for r in range(1, R + 1, 16):
            p = seeded[len(shared)][r]
            assert abs(glob.null_[q, r - 1] - rsa.compare_rdms(mats[a], labs[a], mats[b][np.ix_(ib[p], ib[p])], shared)) \
                <= 2 * RR.compare_bar(RR.triangle(mats[a], ia), RR.triangle(mats[b], ib[p]))
    assert np.array_equal(bits(glob.null_), bits(again.null_))           # (RandomState(3) is the global generator after seed(3))
    # the cosine method shares everything but the centring; device-resident matrices are taken as they are
    import torch
    cos = rsa.compare_rdms_many(mats, labs, pairs, method='cosine', n_permutations=R, random_state=SEED)
    dev = rsa.compare_rdms_many([torch.from_numpy(m).cuda() for m in mats], labs, pairs, method='cosine', n_permutations=R,
                                random_state=SEED)
    assert np.array_equal(bits(cos.null_), bits(dev.null_)) and np.array_equal(bits(cos.similarity_), bits(dev.similarity_))
    a, b = pairs[0]
    assert cos.similarity_[0] == rsa.compare_rdms(mats[a], labs[a], mats[b], labs[b], method='cosine')
    # a matrix against itself: 1 within the bar (the quotient of a sum of squares by the product of two roots rounds), and a
    # relabelling does as well, with the same bits, only where the draw is the identity (6 conditions have 720 orders, so 65
    # draws hold one now and then)
    own = [q for q, (a, b) in enumerate(pairs) if a == b]
    assert len(own) == 2
    for q in own:
        x = RR.triangle(mats[pairs[q][0]], np.arange(ms[q]))
        assert abs(whole.similarity_[q] - 1.0) <= RR.compare_bar(x, x) < 1e-9
        identity = (tables[ms[q]][1:] == np.arange(ms[q])).all(axis=1)
        assert (whole.null_[q][identity] == whole.similarity_[q]).all() and (whole.null_[q][~identity] < whole.similarity_[q]).all()
        assert whole.p_value_[q] == (1 + np.count_nonzero(identity)) / (1 + R)


@pytest.mark.parametrize('n_sets', (1, 40))
def test_calc_rdm_corr_many_takes_a_fixed_number_of_calls_and_repeats_its_bits(n_sets, monkeypatch):
    rsa = RSA()
    f64 = [n for n in NAMES if CASES[n][0].dtype == np.float64]
    f32 = [n for n in NAMES if CASES[n][0].dtype == np.float32]
    names = [f64[i % len(f64)] for i in range(n_sets)]
    counts = count_calls(monkeypatch)
    out = rsa.calc_rdm_corr_many([CASES[n][0] for n in names], [CASES[n][1] for n in names])
    assert dict(counts) == {'xps_cnd_avg_folds_f64': 1, 'xps_row_standardize_grouped_f64': 1, 'xps_gram_grouped_f64': 1,
                            'xps_rdm_from_corr_grouped_f64': 1}           # whatever the number of data sets
    for n, (rdm, uniq) in zip(names, out):
        assert np.array_equal(bits(rdm), bits(rdms()[n][0])) and np.array_equal(uniq, rdms()[n][1])
    counts.clear()
    mixed = names + f32                                                   # float32 data: np.mean's float32 sums, one call per data set
    again = rsa.calc_rdm_corr_many([CASES[n][0] for n in mixed], [CASES[n][1] for n in mixed])
    assert dict(counts) == {'xps_cnd_avg_folds_f64': 1, 'xps_cnd_avg_f32': len(f32), 'xps_row_standardize_grouped_f64': 1,
                            'xps_gram_grouped_f64': 1, 'xps_rdm_from_corr_grouped_f64': 1}
    for n, (rdm, uniq) in zip(mixed, again):
        assert np.array_equal(bits(rdm), bits(rdms()[n][0]))             # two runs, other neighbours: identical bits


def test_rdm_alignment_scores_is_the_two_calls_on_resident_rdms(monkeypatch):
    rsa = RSA()
    target, others = 'a_n130_T5_d4_k9', ['b_n65_T5_d4_k7_f32', 'c_n97_T3_d7_k9']
    counts = count_calls(monkeypatch)
    res = rsa.rdm_alignment_scores(*CASES[target], [CASES[n][0] for n in others], [CASES[n][1] for n in others], n_permutations=9,
                                   random_state=SEED)
    assert dict(counts) == {'xps_cnd_avg_folds_f64': 1, 'xps_cnd_avg_f32': 1, 'xps_row_standardize_grouped_f64': 1,
                            'xps_gram_grouped_f64': 1, 'xps_rdm_from_corr_grouped_f64': 1, 'xps_rdm_compare_perm_f64': 1}
    assert np.array_equal(bits(res.rdm_target_), bits(rdms()[target][0])) and np.array_equal(res.labels_target_, rdms()[target][1])
    for n, rdm, uniq in zip(others, res.rdms_, res.labels_):
        assert np.array_equal(bits(rdm), bits(rdms()[n][0])) and np.array_equal(uniq, rdms()[n][1])
    mats, labs = [rdms()[n][0] for n in [target] + others], [rdms()[n][1] for n in [target] + others]
    want = rsa.compare_rdms_many(mats, labs, [(0, 1), (0, 2)], n_permutations=9, random_state=SEED)
    assert np.array_equal(bits(res.similarity_), bits(want.similarity_)) and np.array_equal(bits(res.comparison_.null_), bits(want.null_))
    assert np.array_equal(res.p_value_, want.p_value_) and res.mean_similarity_ == float(np.mean(want.similarity_))
