"""alignment/rsa.py and its restatement without a device: tests/rsa_ref.py against the golden fixture (the reference notebook's own
functions) and against scipy.stats.pearsonr / np.triu_indices loops, the permutation tables of compare_rdms_many (ascending m, order
of the draws, np.random.seed reproduction), subset_rdm's rule for a missing label, cos_sim, the new prototypes, and every argument
refusal of the wrappers, raised before the device is looked for and before any permutation is drawn."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy import stats

import rsa_ref as RR
from cross_patient_speech_decoding_amd import _lib, alignment
from cross_patient_speech_decoding_amd.alignment import _linalg as LA
from cross_patient_speech_decoding_amd.alignment import rsa

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rsa.npz'))
CASES = RR.cases()
TOO_SHORT = r'`x` and `y` must have length at least 2\.'


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Any look for the device fails the test: the refusals come first."""
    def boom(*a, **k):
        raise AssertionError('the device was looked for')
    monkeypatch.setattr(LA, 'device', boom)
    monkeypatch.setattr(LA, 'to_device', boom)


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_fixture_holds_the_cases_of_the_restatement():
    assert sorted(CASES) == list(GOLD['names'])
    for name, (data, labels) in CASES.items():
        assert np.array_equal(GOLD[f'{name}/data'], data) and GOLD[f'{name}/data'].dtype == data.dtype
        assert np.array_equal(GOLD[f'{name}/labels'], labels)
    assert os.path.getsize(GOLD.fid.name) < 200 * 1024


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_restated_rdm_is_the_notebooks_and_scipys(name):
    data, labels = CASES[name]
    ca, uniq = RR.cnd_means(data, labels)
    assert np.array_equal(uniq, GOLD[f'{name}/unique_labels'])
    ref, bar = RR.rdm_ref(ca), RR.corr_bar(ca)
    assert bar.max() < 1e-9
    gold = GOLD[f'{name}/rdm']
    off = ~np.eye(len(uniq), dtype=bool)
    assert (np.abs(gold - ref)[off] <= bar[off]).all()
    assert (np.abs(np.diag(gold)) <= 4 * 2.0 ** -53).all() and (np.diag(ref) == 0).all()  # 1 - pearsonr(x, x): 0 or a few ulps of 1
    loop = np.array([[1 - stats.pearsonr(ca[i], ca[j])[0] for j in range(len(ca))] for i in range(len(ca))])
    assert np.array_equal(loop, gold)                                    # the fixture is this loop on numpy's condition means
    print(f'{name}: largest fraction of the bar {float((np.abs(gold - ref)[off] / bar[off]).max()):.2e}')


def test_the_restated_comparison_is_the_notebooks_and_scipys():
    for (a, b), pearson, cosine in zip(GOLD['pairs'], GOLD['pearson'], GOLD['cosine']):
        A, ua, B, ub = GOLD[f'{a}/rdm'], GOLD[f'{a}/unique_labels'], GOLD[f'{b}/rdm'], GOLD[f'{b}/unique_labels']
        shared, ia, ib = RR.shared_indices(ua, ub)
        assert len(shared) >= 3 and np.array_equal(ua[ia], shared) and np.array_equal(ub[ib], shared)
        x, y = RR.triangle(A, ia), RR.triangle(B, ib)
        m = len(shared)
        loop = [(A[ia[u], ia[v]], B[ib[u], ib[v]]) for u in range(m) for v in range(u + 1, m)]         # np.triu_indices order
        assert np.array_equal(np.array(loop), np.stack([x, y], axis=1))
        for method, gold, theirs in (('pearson', pearson, stats.pearsonr(x, y)[0]), ('cosine', cosine, rsa.cos_sim(x, y))):
            bar = RR.compare_bar(x, y, method)
            assert bar < 1e-9 and gold == theirs
            assert abs(gold - RR.compare_ref(A, ia, B, ib, method=method)) <= bar
        p = np.random.default_rng(1).permutation(m)
        assert abs(stats.pearsonr(x, B[np.ix_(ib[p], ib[p])][np.triu_indices(m, k=1)])[0] - RR.compare_ref(A, ia, B, ib, p)) \
            <= RR.compare_bar(x, y)
    assert {tuple(p) for p in GOLD['pairs']} >= {('a_n130_T5_d4_k9', 'b_n65_T5_d4_k7_f32'), ('d_n40_T2_d3_seq', 'e_n48_T2_d3_seq_f32')}


def test_constant_rows_and_clipping_in_the_restatement():
    ca = np.random.default_rng(2).standard_normal((4, 9)) + 3.0
    ca[2] = 0.1
    ref = RR.rdm_ref(ca)
    nan = np.isnan(ref)
    assert nan[2].all() and nan[:, 2].all() and not np.delete(np.delete(nan, 2, 0), 2, 1).any()
    with pytest.warns(stats.ConstantInputWarning):
        assert np.isnan(stats.pearsonr(ca[2], ca[0])[0])
    assert np.isinf(RR.kappa(ca)[2])


# ------------------------------------------------------------------------------------------------ host helpers of the module
def test_subset_rdm_drops_a_shared_label_that_is_missing():
    rdm, uniq = GOLD['a_n130_T5_d4_k9/rdm'], GOLD['a_n130_T5_d4_k9/unique_labels']
    asked = GOLD['subset/asked']
    assert 'no such label' in asked
    got = rsa.subset_rdm(rdm, uniq, asked)
    assert got.shape == (3, 3) and np.array_equal(got, GOLD['subset/result']) and np.array_equal(got, rdm[:3, :3])
    assert np.array_equal(rsa.subset_rdm(rdm, uniq, uniq[[4, 1]]), rdm[np.ix_([4, 1], [4, 1])])
    assert rsa.subset_rdm(rdm, uniq, ['x', 'y']).shape == (0, 0) and rsa.subset_rdm(rdm.tolist(), list(uniq), uniq[:2]).shape == (2, 2)
    assert alignment.subset_rdm is rsa.subset_rdm and alignment.calc_rdm_corr is rsa.calc_rdm_corr
    a, b = np.array([1.0, 2.0, 2.0]), np.array([2.0, 0.0, 1.0])
    assert rsa.cos_sim(a, b) == np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)) == 4.0 / (3.0 * np.sqrt(5.0))


def test_permutation_tables_ascending_m_order_of_draws_and_the_global_generator():
    tables = rsa.permutation_tables([7, 5, 7, 9, 5], 3, random_state=4)
    rng = np.random.RandomState(4)
    assert list(tables) == [5, 7, 9]
    for m in (5, 7, 9):                                                   # ascending m, R draws each, in order
        assert tables[m].shape == (4, m) and tables[m].dtype == np.int32
        assert np.array_equal(tables[m][0], np.arange(m))
        for r in range(1, 4):
            assert np.array_equal(tables[m][r], rng.permutation(m))
    same = RR.permutation_tables([9, 5, 7], 3, np.random.RandomState(4))
    assert all(np.array_equal(tables[m], same[m]) for m in tables)
    np.random.seed(3)                                                     # random_state=None: numpy's global generator
    glob = rsa.permutation_tables([6, 4], 2)
    np.random.seed(3)
    for m in (4, 6):
        for r in (1, 2):
            assert np.array_equal(glob[m][r], np.random.permutation(m))
    assert rsa.permutation_tables([4], 0)[4].shape == (1, 4)
    gen = np.random.default_rng(8)
    assert np.array_equal(rsa.permutation_tables([5], 1, gen)[5][1], np.random.default_rng(8).permutation(5))
    assert rsa.pairs_per_chunk(200, 2 ** 28) == 2 ** 28 // (8 * 205) and rsa.pairs_per_chunk(200, 1) == 1


def test_the_similarity_is_the_elementwise_host_quotient():
    cross, sxx, syy = np.array([[2.0, -9.0, np.nan, 0.0]]), np.array([[4.0]]), np.array([[4.0]])
    assert np.array_equal(rsa._similarity(cross, sxx, syy), [[0.5, -1.0, np.nan, 0.0]], equal_nan=True)
    assert np.isnan(rsa._similarity(np.array([[0.0]]), np.array([[0.0]]), syy)).all()                # a constant triangle


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_every_refusal_comes_before_the_device_and_before_any_draw(monkeypatch):
    class NoDraws:
        def permutation(self, m):
            raise AssertionError('a permutation was drawn')
    data, labels = CASES['a_n130_T5_d4_k9']
    for fn in (rsa.calc_rdm_corr, lambda d, l: rsa.calc_rdm_corr_many([data, d], [labels, l]),
               lambda d, l: rsa.rdm_alignment_scores(data, labels, [d], [l], random_state=NoDraws()),
               lambda d, l: rsa.rdm_alignment_scores(d, l, [data], [labels], random_state=NoDraws())):
        with pytest.raises(ValueError, match=TOO_SHORT):
            fn(data[:, :1, :1], labels)                                  # D = T d = 1
        with pytest.raises(ValueError, match=TOO_SHORT):
            fn(torch.zeros(130, 1), labels)
        with pytest.raises(ValueError, match=r'\(n_trials, T, d\) or \(n_trials, D\)'):
            fn(data[0, 0], labels[:4])
        with pytest.raises(ValueError, match=r'\(n_trials, T, d\) or \(n_trials, D\)'):
            fn(data[:, :, :, None], labels)
        with pytest.raises(ValueError, match='a label vector has 129 entries for 130 samples'):
            fn(data, labels[:129])
    with pytest.raises(ValueError, match='2 data sets and 1 label vectors'):
        rsa.calc_rdm_corr_many([data, data], [labels])
    assert rsa.calc_rdm_corr_many([], []) == []

    eye = 1.0 - np.eye(4)
    names = np.array(['a', 'b', 'c', 'd'])
    ok = ([eye, eye], [names, names], [(0, 1)])
    for args, kw, text in (
            (ok, dict(method='spearman'), "method must be 'pearson' or 'cosine'"),
            (ok, dict(n_permutations=-1), 'n_permutations must be an integer >= 0'),
            (ok, dict(n_permutations=2.5), 'n_permutations must be an integer >= 0'),
            (ok, dict(max_bytes=0), 'max_bytes must be an integer >= 1'),
            (ok, dict(random_state='seed'), 'random_state must be None, an int or a numpy generator'),
            (([eye], [names, names], [(0, 0)]), {}, '1 RDMs and 2 label vectors'),
            (([eye[:3], eye], [names, names], [(0, 1)]), {}, 'an RDM must be a square matrix'),
            (([np.ones(4), eye], [names, names], [(0, 1)]), {}, 'an RDM must be a square matrix'),
            (([eye, eye], [names[:3], names], [(0, 1)]), {}, 'an RDM of 4 conditions needs 4 labels'),
            (([eye, eye], [names, names], [(0, 2)]), {}, 'a pair must be two indices into rdms'),
            (([eye, eye], [names, names], [(0, 1, 1)]), {}, 'a pair must be two indices into rdms'),
            (([eye, eye], [names, names], [(0, -1)]), {}, 'a pair must be two indices into rdms'),
            (([eye, eye], [names, np.array(['a', 'b', 'x', 'y'])], [(0, 0), (0, 1)]), {}, TOO_SHORT),        # 2 shared conditions
            (([eye, eye], [names, np.array(['w', 'z', 'x', 'y'])], [(0, 1)]), {}, TOO_SHORT)):
        with pytest.raises(ValueError, match=text):
            rsa.compare_rdms_many(*args, **{'random_state': NoDraws(), **kw})
    # a permutation null needs a symmetric second matrix: a host matrix that is not is refused (the first one may be anything)
    skew = eye.copy()
    skew[0, 1] = np.nextafter(skew[0, 1], 2.0)
    with pytest.raises(ValueError, match=r'rdms\[1\] is not symmetric bit for bit'):
        rsa.compare_rdms_many([eye, skew], [names, names], [(0, 1), (1, 1)], n_permutations=2, random_state=NoDraws())
    with pytest.raises(ValueError, match=r'rdms\[0\] is not symmetric bit for bit'):
        rsa.compare_rdms_many([torch.from_numpy(skew), eye], [names, names], [(1, 0)], n_permutations=1, random_state=NoDraws())
    with pytest.raises(AssertionError, match='a permutation was drawn'):                   # asked of the second matrix only
        rsa.compare_rdms_many([skew, eye], [names, names], [(0, 1)], n_permutations=1, random_state=NoDraws())
    with pytest.raises(AssertionError, match='the device was looked for'):                 # and only for a null
        rsa.compare_rdms_many([eye, skew], [names, names], [(0, 1)], random_state=NoDraws())
    nan_rdm = eye.copy()
    nan_rdm[2, :] = nan_rdm[:, 2] = np.nan                                                  # a constant condition: NaN is symmetric
    with pytest.raises(AssertionError, match='a permutation was drawn'):
        rsa.compare_rdms_many([eye, nan_rdm], [names, names], [(0, 1)], n_permutations=1, random_state=NoDraws())
    big = np.arange(rsa.MAX_CONDITIONS + 1)
    wide = np.zeros((len(big), len(big)))
    with pytest.raises(ValueError, match=r'1025 shared conditions; at most XPS_RSA_MAX_CONDITIONS = 1024'):
        rsa.compare_rdms_many([wide, wide], [big, big], [(0, 1)], random_state=NoDraws())
    with pytest.raises(ValueError, match=TOO_SHORT):
        rsa.compare_rdms(eye, names, eye, np.array(['a', 'b', 'x', 'y']))
    with pytest.raises(ValueError, match="method must be 'pearson' or 'cosine'"):
        rsa.compare_rdms(eye, names, eye, names, method='kendall')
    # rdm_alignment_scores: too few shared conditions between the label sets are found from the labels alone
    other = np.where(labels <= 2, labels, labels + 100)
    with pytest.raises(ValueError, match=TOO_SHORT):
        rsa.rdm_alignment_scores(data, labels, [data], [other], n_permutations=5, random_state=NoDraws())
    with pytest.raises(ValueError, match="method must be 'pearson' or 'cosine'"):
        rsa.rdm_alignment_scores(data, labels, [data], [labels], method='spearman')
    with pytest.raises(ValueError, match='n_permutations must be an integer >= 0'):
        rsa.rdm_alignment_scores(data, labels, [data], [labels], n_permutations=-3)
    empty = rsa.compare_rdms_many([eye], [names], [], n_permutations=3, random_state=NoDraws())       # no pair: nothing to do
    assert empty.similarity_.shape == (0,) and empty.null_.shape == (0, 3) and empty.p_value_.shape == (0,)


def test_the_device_wrappers_refuse_bad_tensors_without_a_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(LA, 'call', lambda name, *a: calls.append(name))
    X = torch.zeros(3, 4, dtype=torch.float64)                           # a host tensor: refused as it is
    for fn, args in ((LA.row_standardize_grouped, [(X, X)]), (LA.rdm_from_corr_grouped, [(X, X)])):
        with pytest.raises(ValueError, match='device matrix'):
            fn(args)
    with pytest.raises(ValueError, match='device matrix'):
        LA.rdm_compare_perm([(X, 0, X, 3, 3, 0)], np.arange(6), [[0, 3]], np.arange(3), 0)
    with pytest.raises(ValueError, match='R must be non-negative'):
        LA.rdm_compare_perm([], np.arange(6), [[0, 3]], np.arange(3), -1)
    assert LA.row_standardize_grouped([]) is None and LA.rdm_from_corr_grouped([]) is None and calls == []


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_header_declares_the_entries_and_the_constants_match():
    sigs = _lib.SIGNATURES
    v, i, i64, sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
    for name in ('xps_row_standardize_grouped_f64', 'xps_rdm_from_corr_grouped_f64'):
        assert sigs[name] == (i, [v, i, v, sz, v]) and sigs[name + '_workspace'] == (sz, [i])
    assert sigs['xps_rdm_compare_perm_f64'] == (i, [v, i, v, i, v, i64, v, i64, i, i, v, v, i64, v, sz, v])
    assert sigs['xps_rdm_compare_perm_f64_workspace'] == (sz, [i, i, i64, i64])
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    for name, value in (('XPS_RSA_STD_WORDS', LA.RSA_STD_WORDS), ('XPS_RSA_RDM_WORDS', LA.RSA_RDM_WORDS),
                        ('XPS_RSA_PAIR_WORDS', LA.RSA_PAIR_WORDS), ('XPS_RSA_MAX_CONDITIONS', LA.RSA_MAX_CONDITIONS)):
        assert f'#define {name} {value}\n' in header
    assert LA.CP_ROW < LA.RSA_PAIR_WORDS and rsa.MAX_CONDITIONS == 1024
