"""decoders.SVCSearchCV on the MI355X: the three entry points of the search through the C ABI (the multi-gamma kernel matrices and
the multi-matrix SMO bit for bit against the single-matrix entries, the scoring kernel against a numpy restatement of its rules),
and the search against libsvm fold by fold and against GridSearchCV around decoders.SVC."""
import functools
import sys
import warnings

import numpy as np
import pytest
from sklearn.base import clone
from sklearn.metrics import accuracy_score, balanced_accuracy_score
from sklearn.model_selection import GridSearchCV, ParameterGrid, StratifiedKFold
from sklearn.pipeline import make_pipeline
from sklearn.svm import SVC as SkSVC

pytestmark = pytest.mark.gpu

NAN = float('nan')


def dev_tensor(a):
    import torch
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    return torch.from_numpy(np.ascontiguousarray(a)).to(LA.device())


def xps_call(name, *args):
    import torch
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import call
    call(name, *args, _dev.stream())
    torch.cuda.synchronize()


def ptr(t):
    return None if t is None else t.data_ptr()


# ================================================================================================ 1. xps_rbf_multi_from_gram_f64
@pytest.mark.parametrize('m,n,pad,M', [(1, 1, 0, 1), (5, 3, 2, 3), (67, 130, 5, 7)])
def test_rbf_multi_equals_one_single_gamma_call_per_gamma_bit_for_bit(m, n, pad, M):
    import torch
    rng = np.random.default_rng(100 * m + n)
    d = 6
    A, B = rng.standard_normal((m, d)), rng.standard_normal((n, d))
    ldg, ldk = n + pad, n + 2 * pad
    G = np.full((m, ldg), NAN)
    G[:, :n] = A @ B.T
    na, nb = (A * A).sum(axis=1), (B * B).sum(axis=1)
    gammas = np.concatenate([[0.0], 10.0 ** rng.uniform(-4, 3, M - 1)])[:M]
    gammas = gammas[rng.permutation(M)]
    assert (gammas == 0).sum() == 1
    G_d, na_d, nb_d, g_d = dev_tensor(G), dev_tensor(na), dev_tensor(nb), dev_tensor(gammas)
    kstride = m * ldk + 3
    multi = torch.full((M * kstride,), NAN, dtype=torch.float64, device=G_d.device)
    xps_call('xps_rbf_multi_from_gram_f64', ptr(G_d), ldg, ptr(na_d), ptr(nb_d), m, n, ptr(g_d), M, ptr(multi), ldk, kstride)
    multi = multi.cpu().numpy()
    for t, gamma in enumerate(gammas):
        single = torch.full((m, ldk), NAN, dtype=torch.float64, device=G_d.device)
        xps_call('xps_rbf_from_gram_f64', ptr(G_d), ldg, ptr(na_d), ptr(nb_d), m, n, float(gamma), ptr(single), ldk)
        got = multi[t * kstride:t * kstride + m * ldk].reshape(m, ldk)
        want = single.cpu().numpy()
        assert np.isfinite(want[:, :n]).all()
        np.testing.assert_array_equal(got[:, :n].view(np.int64), want[:, :n].view(np.int64))
        assert np.isnan(got[:, n:]).all()                                 # the padding of every matrix is untouched
        if gamma == 0:
            np.testing.assert_array_equal(got[:, :n], np.ones((m, n)))
    assert np.isnan(multi.reshape(M, kstride)[:, m * ldk:]).all()


def test_rbf_multi_refuses_bad_arguments():
    import torch
    from cross_patient_speech_decoding_amd._lib import XpsError
    t = dev_tensor(np.ones(64))
    good = dict(G=ptr(t), ldg=4, na=ptr(t), nb=ptr(t), m=3, n=4, gammas=ptr(t), M=2, K=ptr(t), ldk=4, kstride=16)
    bad = [dict(G=None), dict(na=None), dict(nb=None), dict(gammas=None), dict(K=None), dict(ldg=3), dict(ldk=3), dict(M=-1), dict(m=-1),
           dict(kstride=11)]
    for change in bad:
        with pytest.raises(XpsError, match='xps_rbf_multi_from_gram_f64'):
            xps_call('xps_rbf_multi_from_gram_f64', *{**good, **change}.values())
    xps_call('xps_rbf_multi_from_gram_f64', *{**good, 'kstride': 12}.values())       # 2 * 16 doubles at the tightest stride: in bounds
    torch.cuda.synchronize()


# ================================================================================================ 2. xps_svm_smo_multi_f64
def rbf_matrix(rng, n, ld, gamma):
    X = rng.standard_normal((n, 5))
    sq = (X * X).sum(axis=1)
    K = np.full((n, ld), NAN)
    K[:, :n] = np.exp(-gamma * np.maximum(sq[:, None] + sq[None, :] - 2 * X @ X.T, 0))
    return K


def run_smo(entry, head, idx, sizes, npos, cb):
    import torch
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    i_d, o_d, p_d, c_d = dev_tensor(idx.astype(np.int32)), dev_tensor(off), dev_tensor(np.asarray(npos, dtype=np.int32)), dev_tensor(cb)
    P = len(sizes)
    alpha = torch.full((max(len(idx), 1),), NAN, dtype=torch.float64, device=i_d.device)
    rho = torch.full((max(P, 1),), NAN, dtype=torch.float64, device=i_d.device)
    iters = torch.full((max(P, 1),), -7, dtype=torch.int32, device=i_d.device)
    xps_call(entry, *head, ptr(i_d), ptr(o_d), ptr(p_d), P, int(max(sizes)), ptr(c_d), 1e-3, 100000, ptr(alpha), ptr(rho), ptr(iters))
    return alpha.cpu().numpy(), rho.cpu().numpy(), iters.cpu().numpy()


def test_smo_multi_equals_one_single_matrix_call_per_matrix_bit_for_bit():
    rng = np.random.default_rng(11)
    shapes = [(320, 333, 0.05), (140, 140, 0.3), (70, 77, 1.0)]
    mats = [rbf_matrix(rng, *s) for s in shapes]
    base = np.concatenate([[0], np.cumsum([K.size for K in mats])]).astype(np.int64)
    Kbuf = dev_tensor(np.concatenate([K.ravel() for K in mats]))
    plan = [(0, 300), (2, 2), (1, 63), (0, 64), (2, 65), (1, 2), (0, 65), (1, 64), (2, 63), (0, 2), (1, 65), (0, 63), (2, 64)]
    probs = []
    for m, size in plan:
        points = rng.permutation(shapes[m][0])[:size]
        probs.append(dict(m=m, idx=points, npos=int(rng.integers(1, size)), cb=rng.uniform(0.5, 2.0, size)))
    cat = lambda ps, key: np.concatenate([p[key] for p in ps])
    kbase = dev_tensor(np.array([base[p['m']] for p in probs], dtype=np.int64))
    kld = dev_tensor(np.array([shapes[p['m']][1] for p in probs], dtype=np.int64))
    alpha, rho, iters = run_smo('xps_svm_smo_multi_f64', (ptr(Kbuf), ptr(kbase), ptr(kld)), cat(probs, 'idx'), [len(p['idx']) for p in probs],
                                [p['npos'] for p in probs], cat(probs, 'cb'))
    off = np.concatenate([[0], np.cumsum([len(p['idx']) for p in probs])])
    assert np.isfinite(alpha).all() and np.isfinite(rho).all() and (iters > 0).all()
    for m in range(3):
        own = [q for q, p in enumerate(probs) if p['m'] == m]
        ps = [probs[q] for q in own]
        K_d = dev_tensor(mats[m])
        a1, r1, i1 = run_smo('xps_svm_smo_f64', (ptr(K_d), shapes[m][1]), cat(ps, 'idx'), [len(p['idx']) for p in ps], [p['npos'] for p in ps],
                             cat(ps, 'cb'))
        np.testing.assert_array_equal(np.concatenate([alpha[off[q]:off[q + 1]] for q in own]).view(np.int64), a1.view(np.int64))
        np.testing.assert_array_equal(rho[own].view(np.int64), r1.view(np.int64))
        np.testing.assert_array_equal(iters[own], i1)
        assert (a1 > 0).any()


def test_smo_multi_refuses_bad_arguments():
    from cross_patient_speech_decoding_amd._lib import XpsError, lib
    d, i, l = dev_tensor(np.ones(8)), dev_tensor(np.zeros(8, dtype=np.int32)), dev_tensor(np.zeros(8, dtype=np.int64))
    good = dict(K=ptr(d), kbase=ptr(l), kld=ptr(l), idx=ptr(i), off=ptr(i), npos=ptr(i), nprob=1, max_points=2, cbound=ptr(d), eps=1e-3,
                max_iter=10, alpha=ptr(d), rho=ptr(d), iters=ptr(i))
    bad = [dict(K=None), dict(kbase=None), dict(kld=None), dict(idx=None), dict(off=None), dict(npos=None), dict(cbound=None),
           dict(alpha=None), dict(rho=None), dict(iters=None), dict(nprob=-1), dict(eps=0.0), dict(max_iter=0), dict(max_points=0),
           dict(max_points=int(lib().xps_svm_smo_f64_max_points()) + 1)]
    for change in bad:
        with pytest.raises(XpsError, match='xps_svm_smo_multi_f64'):
            xps_call('xps_svm_smo_multi_f64', *{**good, **change}.values())


# ================================================================================================ 3. xps_svm_cv_score_f64
def score_rules(c, dtype=np.float64):
    """The rules of the scoring kernel, restated: dec = sum_t +-alpha K[r][idx] - rho over the points inside the matrix; the vote goes
    to pair_a where dec > 0 strictly, else to pair_b; the prediction is the first maximum of the k counts; conf[s][true][pred].  A
    held-out row outside the matrix: pred -1, decisions 0, no count.  Also returns the vote counts and sum |alpha K| + |rho|."""
    S, k = len(c['mod_off']) - 1, c['k']
    T = int(c['tst_off'][-1])
    ldd = max(int(np.diff(c['mod_off']).max()), 1)
    pred = np.full(T, -7, dtype=np.int32)
    conf = np.zeros((S, k, k), dtype=np.int32)
    dec = np.full((T, ldd), NAN, dtype=dtype)
    mag = np.zeros((T, ldd), dtype=dtype)
    votes = np.zeros((T, k), dtype=np.int64)
    K = c['K'].astype(dtype)
    alpha, rho = c['alpha'].astype(dtype), c['rho'].astype(dtype)
    for s in range(S):
        n, base, ld = int(c['mn'][s]), int(c['mbase'][s]), int(c['mld'][s])
        for i in range(c['tst_off'][s], c['tst_off'][s + 1]):
            r = int(c['tst'][i])
            if not 0 <= r < n:
                pred[i] = -1
                dec[i, :c['mod_off'][s + 1] - c['mod_off'][s]] = 0
                continue
            for q in range(c['mod_off'][s], c['mod_off'][s + 1]):
                o0, o1 = c['off'][q], c['off'][q + 1]
                j = c['idx'][o0:o1].astype(np.int64)
                ok = (j >= 0) & (j < n)
                sign = np.where(np.arange(o1 - o0) < c['npos'][q], 1, -1)[ok]
                terms = sign * alpha[o0:o1][ok] * K[base + r * ld + j[ok]]
                d = terms.sum(dtype=dtype) - rho[q]
                dec[i, q - c['mod_off'][s]] = d
                mag[i, q - c['mod_off'][s]] = np.abs(terms).sum(dtype=dtype) + abs(rho[q])
                win = c['pair_a'][q] if d > 0 else c['pair_b'][q]
                if 0 <= win < k:
                    votes[i, win] += 1
            pred[i] = votes[i].argmax()
            if 0 <= c['ytrue'][i] < k:
                conf[s, c['ytrue'][i], pred[i]] += 1
    return pred, conf, dec, votes, mag


def run_score(c, want_dec=True, **override):
    import torch
    from cross_patient_speech_decoding_amd._lib import lib
    S, k = len(c['mod_off']) - 1, c['k']
    T = int(c['tst_off'][-1])
    ldd = max(int(np.diff(c['mod_off']).max()), 1) if S else 1
    i32 = lambda key: dev_tensor(np.asarray(c[key], dtype=np.int32))
    t = dict(K=dev_tensor(c['K']), mbase=dev_tensor(np.asarray(c['mbase'], dtype=np.int64)), mld=dev_tensor(np.asarray(c['mld'], dtype=np.int64)),
             mn=i32('mn'), idx=i32('idx'), off=i32('off'), npos=i32('npos'), alpha=dev_tensor(c['alpha']), rho=dev_tensor(c['rho']),
             pair_a=i32('pair_a'), pair_b=i32('pair_b'), tst=i32('tst'), ytrue=i32('ytrue'))
    dev = t['K'].device
    pred = torch.full((max(T, 1),), -7, dtype=torch.int32, device=dev)
    conf = torch.full((max(S, 1), max(k, 1), max(k, 1)), -7, dtype=torch.int32, device=dev)
    dec = torch.full((max(T, 1), ldd), NAN, dtype=torch.float64, device=dev) if want_dec else None
    ws_bytes = int(lib().xps_svm_cv_score_f64_workspace(S))
    ws = torch.zeros(ws_bytes // 4 + 1, dtype=torch.int32, device=dev)
    mod_off, tst_off = np.asarray(c['mod_off'], dtype=np.int32), np.asarray(c['tst_off'], dtype=np.int32)      # host arrays
    args = dict(K=ptr(t['K']), mbase=ptr(t['mbase']), mld=ptr(t['mld']), mn=ptr(t['mn']), idx=ptr(t['idx']), off=ptr(t['off']),
                npos=ptr(t['npos']), alpha=ptr(t['alpha']), rho=ptr(t['rho']), pair_a=ptr(t['pair_a']), pair_b=ptr(t['pair_b']),
                mod_off=mod_off.ctypes.data, tst=ptr(t['tst']), ytrue=ptr(t['ytrue']), tst_off=tst_off.ctypes.data, S=S, k=k, pred=ptr(pred),
                conf=ptr(conf), dec_out=ptr(dec), ldd=ldd, ws=ptr(ws), ws_bytes=ws_bytes)
    args.update(override)
    xps_call('xps_svm_cv_score_f64', *args.values())
    return pred.cpu().numpy()[:T], conf.cpu().numpy()[:S], (dec.cpu().numpy()[:T] if want_dec else None)


MATS = [(320, 327), (311, 333)]                # two square matrices (rows, leading dimension > rows) in one buffer
SIZES = [2, 63, 64, 65, 300]


def pairs_of(present):
    return [(a, b) for i, a in enumerate(present) for b in present[i + 1:]]


def score_case(k, integer, seed, held_out=(1, 3, 4, 5, 9, 0, 4)):
    """Seven models over two matrices: all classes, lacking one, lacking two (where k allows), held-out row counts 1, 3, 4, 5, 9, 0
    and 4; problem sizes cycle through 2, 63, 64, 65, 300 (as the matrix allows).  integer=True: small integer alpha, K and rho, so
    every sum is exact in any order."""
    rng = np.random.default_rng(seed)
    base = np.concatenate([[0], np.cumsum([n * ld for n, ld in MATS])])
    K = rng.integers(-3, 4, base[-1]).astype(np.float64) if integer else rng.standard_normal(base[-1])
    c = dict(k=k, K=K, mbase=[], mld=[], mn=[], idx=[], npos=[], alpha=[], rho=[], pair_a=[], pair_b=[], mod_off=[0], tst=[], ytrue=[],
             tst_off=[0])
    sizes, turn = [], 0
    for s, nt in enumerate(held_out):
        m = s % 2
        n, ld = MATS[m]
        present = list(range(k))
        for _ in range(min(s % 3, k - 2)):                                # models 1, 4: one class less; 2, 5: two less
            present.remove(int(rng.choice(present[1:])))
        for a, b in pairs_of(present):
            size = min(SIZES[turn % len(SIZES)], n - 10)
            turn += 1
            sizes.append(size)
            c['idx'].append(rng.permutation(n)[:size])
            c['npos'].append(int(rng.integers(1, size)))
            c['alpha'].append(rng.integers(0, 5, size).astype(np.float64) if integer else rng.uniform(0.25, 1.25, size))
            c['rho'].append(float(rng.integers(-6, 7)) if integer else float(rng.standard_normal()))
            c['pair_a'].append(a)
            c['pair_b'].append(b)
        c['mod_off'].append(len(sizes))
        c['mbase'].append(base[m]); c['mld'].append(ld); c['mn'].append(n)
        c['tst'] += list(rng.permutation(n)[:nt])
        c['ytrue'] += list(rng.choice(present, nt))
        c['tst_off'].append(len(c['tst']))
    c['off'] = np.concatenate([[0], np.cumsum(sizes)])
    for key in ('idx', 'alpha'):
        c[key] = np.concatenate(c[key])
    for key in ('npos', 'rho', 'pair_a', 'pair_b', 'tst', 'ytrue', 'mod_off', 'tst_off', 'mbase', 'mld', 'mn'):
        c[key] = np.asarray(c[key], dtype=np.float64 if key == 'rho' else np.int64)
    return c


def raw_sum(c, s, i, q):
    """sum_t +-alpha K of held-out row i (global) of model s on problem q (integer cases: exact)."""
    o0, o1 = c['off'][q], c['off'][q + 1]
    row = c['K'][c['mbase'][s] + c['tst'][i] * c['mld'][s] + c['idx'][o0:o1]]
    return float((np.where(np.arange(o1 - o0) < c['npos'][q], 1.0, -1.0) * c['alpha'][o0:o1] * row).sum())


@pytest.mark.parametrize('k', [2, 3, 9, 64])
def test_score_kernel_equals_the_rules_bit_for_bit_on_integer_inputs(k):
    held_out = (1, 3, 4, 5, 9, 0, 4) if k < 64 else (2, 1, 3, 0)          # k = 64: 2016 problems per model, fewer rows
    c = score_case(k, True, 40 + k, held_out)
    rng = np.random.default_rng(k)
    # decisions exactly on the threshold: on the first held-out row of models 1 .. 4 a third of the problems get rho = their sum
    for s in (1, 2, 3, 4)[:len(held_out) - 2]:
        i = c['tst_off'][s]
        for q in range(c['mod_off'][s], c['mod_off'][s + 1]):
            if rng.random() < 0.34 or q == c['mod_off'][s]:
                c['rho'][q] = raw_sum(c, s, i, q)
    # an engineered vote tie on the first held-out row of model 0 (all classes): class a beats class b where b - a <= (k - 1) / 2,
    # a circulant tournament: for odd k every class wins (k - 1) / 2 pairs, for k = 64 the classes 32 .. 63 win 32 each
    if k >= 3:
        i = c['tst_off'][0]
        for q in range(c['mod_off'][0], c['mod_off'][1]):
            a_wins = c['pair_b'][q] - c['pair_a'][q] <= (k - 1) // 2
            c['rho'][q] = raw_sum(c, 0, i, q) - (1.0 if a_wins else -1.0)
    pred, conf, dec, votes, _ = score_rules(c)
    valid = ~np.isnan(dec)
    assert (dec[valid] == 0).sum() >= 4                                   # the engineered cases are what they are meant to be
    if k >= 3:
        first = votes[c['tst_off'][0]]
        assert (first == first.max()).sum() >= 2 and pred[c['tst_off'][0]] == (0 if k % 2 else 32)
    lacking = sorted(k - len(set(c['pair_a'][a:b]) | set(c['pair_b'][a:b])) for a, b in zip(c['mod_off'][:-1], c['mod_off'][1:]))
    assert lacking[-1] == min(2, k - 2) and sorted(np.diff(c['tst_off'])) == sorted(held_out)
    assert k < 9 or set(np.diff(c['off'])) == {2, 63, 64, 65, 300}
    got_pred, got_conf, got_dec = run_score(c)
    np.testing.assert_array_equal(got_pred, pred)
    np.testing.assert_array_equal(got_conf, conf)
    np.testing.assert_array_equal((got_dec[valid] + 0.0).view(np.int64), (dec[valid] + 0.0).view(np.int64))   # (+ 0.0: -0 and +0 are one value)
    assert np.isnan(got_dec[~valid]).all()
    np.testing.assert_array_equal(got_conf.sum(axis=(1, 2)), np.diff(c['tst_off']))
    assert (got_conf[held_out.index(0)] == 0).all()                       # the model without held-out rows: zeros, written
    no_dec_pred, no_dec_conf, _ = run_score(c, want_dec=False)            # dec_out = NULL
    np.testing.assert_array_equal(no_dec_pred, pred)
    np.testing.assert_array_equal(no_dec_conf, conf)


def test_score_kernel_drops_indices_outside_the_matrix():
    c = score_case(5, True, 77)
    rng = np.random.default_rng(78)
    n_of_problem = np.repeat(c['mn'], np.diff(c['mod_off']))
    for q in range(len(c['npos'])):                                       # a fifth of the points: below 0, at n, far beyond
        o0, o1 = c['off'][q], c['off'][q + 1]
        hit = rng.random(o1 - o0) < 0.2
        c['idx'][o0:o1][hit] = rng.choice([-1, -2 ** 31, n_of_problem[q], n_of_problem[q] + 7, 2 ** 31 - 1], hit.sum())
    for s in (0, 1, 3, 4):                                                # held-out rows outside the matrix, classes outside 0 .. k - 1
        c['tst'][c['tst_off'][s]] = [-1, c['mn'][s], 2 ** 31 - 1, -2 ** 31][s % 4]
        c['ytrue'][c['tst_off'][s + 1] - 1] = [-1, 5, 64, 2 ** 31 - 1][s % 4]
    pred, conf, dec, _, _ = score_rules(c)
    assert (pred == -1).sum() == 4 and conf.sum() < c['tst_off'][-1] - 4
    got_pred, got_conf, got_dec = run_score(c)
    np.testing.assert_array_equal(got_pred, pred)
    np.testing.assert_array_equal(got_conf, conf)
    valid = ~np.isnan(dec)
    np.testing.assert_array_equal((got_dec[valid] + 0.0).view(np.int64), (dec[valid] + 0.0).view(np.int64))
    assert np.isnan(got_dec[~valid]).all()


@pytest.mark.parametrize('k', [3, 9])
def test_score_kernel_sums_within_the_bound_of_an_n_term_sum(k):
    """Random real inputs: |dec_out - ref| <= (n_q + 2) 2^-53 (sum_t |alpha_t K_t| + |rho|) with ref in long double (the standard
    bound of an n_q-term sum of rounded products, one more rounding for rho); every |ref| exceeds its bound, so pred and conf are
    compared exactly."""
    c = score_case(k, False, 500 + k)
    pred, conf, ref, _, mag = score_rules(c, dtype=np.longdouble)
    got_pred, got_conf, got_dec = run_score(c)
    valid = ~np.isnan(ref.astype(np.float64))
    n_q = np.zeros(ref.shape)
    for s in range(len(c['mod_off']) - 1):
        cnt = np.diff(c['off'])[c['mod_off'][s]:c['mod_off'][s + 1]]
        n_q[c['tst_off'][s]:c['tst_off'][s + 1], :len(cnt)] = cnt
    bound = (n_q + 2) * 2.0 ** -53 * mag
    err = np.abs(got_dec.astype(np.longdouble) - ref)
    print(f'k={k}: max err / bound = {float((err[valid] / bound[valid]).max()):.3f}, min |ref| / bound = '
          f'{float((np.abs(ref[valid]) / bound[valid]).min()):.3e}')
    assert valid.sum() >= 40 and (err[valid] <= bound[valid]).all()
    assert (np.abs(ref[valid]) > bound[valid]).all()                       # every row qualifies for the exact comparison
    np.testing.assert_array_equal(got_pred, pred)
    np.testing.assert_array_equal(got_conf, conf)


@pytest.mark.parametrize('k', [0, 1, 65])
def test_score_kernel_refuses_a_class_count_outside_2_to_64(k):
    from cross_patient_speech_decoding_amd._lib import XpsError
    c = score_case(3, True, 1)
    with pytest.raises(XpsError, match='k must be in 2..64'):
        run_score(c, k=k)


def test_score_kernel_refuses_descending_offsets_and_null_pointers():
    from cross_patient_speech_decoding_amd._lib import XpsError
    c = score_case(3, True, 2)
    for key in ('mod_off', 'tst_off'):
        for bad in (c[key][::-1].copy(), np.concatenate([c[key][:3], [c[key][2] - 1], c[key][4:]]), np.concatenate([[-1], c[key][1:]])):
            assert len(bad) == len(c[key])
            host = np.asarray(bad, dtype=np.int32)
            with pytest.raises(XpsError, match=key):
                run_score(c, **{key: host.ctypes.data})
    for key in ('K', 'mbase', 'mld', 'mn', 'idx', 'off', 'npos', 'alpha', 'rho', 'pair_a', 'pair_b', 'mod_off', 'tst', 'ytrue', 'tst_off',
                'pred', 'conf', 'ws'):
        with pytest.raises(XpsError, match='null argument'):
            run_score(c, **{key: None})
    with pytest.raises(XpsError, match='bad parameter'):
        run_score(c, ws_bytes=4)
    with pytest.raises(XpsError, match='bad parameter'):
        run_score(c, S=-1)
    with pytest.raises(XpsError, match='ldd'):
        run_score(c, ldd=1)


# ================================================================================================ 4. the search
TOL = 1e-6
GRIDS = {'rbf': {'C': [0.1, 1, 10], 'gamma': [0.01, 0.1, 'scale']}, 'linear': {'C': [0.01, 0.1, 1, 10]}}


def recipe(n=120, d=12, k=4, seed=1):
    rng = np.random.default_rng(seed)
    y = np.arange(n) % k
    rng.shuffle(y)
    centres = 1.2 * rng.standard_normal((k, d))
    return centres[y] + rng.standard_normal((n, d)), y


def libsvm_folds(make_sk, candidates, X, y, splits, transform=None):
    """Per (candidate, fold): sklearn's libsvm SVC on the training rows -> its predictions on the held-out rows and which of them
    are robust (every one-vs-one decision of magnitude >= 1e-3)."""
    pred, robust = {}, {}
    for c, cand in enumerate(candidates):
        for f, (tr, te) in enumerate(splits):
            Ztr, Zte = (X[tr], X[te]) if transform is None else transform(cand, f)
            sk = make_sk(cand).fit(Ztr, y[tr])
            dec = sk.decision_function(Zte)
            pred[c, f] = sk.predict(Zte)
            robust[c, f] = (np.abs(dec.reshape(len(te), -1)) >= 1e-3).all(axis=1)
    return pred, robust


def by_fold_scorer(X, splits, store):
    """A GridSearchCV scorer that keeps the fitted estimator's predictions per (parameters, fold) and returns the accuracy."""
    fold_of_first = {X[te[0]].tobytes(): f for f, (_, te) in enumerate(splits)}

    def scorer(est, Xf, yf):
        p = est.predict(Xf)
        store[repr(sorted(est.get_params().items())), fold_of_first[np.ascontiguousarray(Xf[0]).tobytes()]] = p
        return float(np.mean(p == yf))
    return scorer


@functools.lru_cache(maxsize=None)
def searched(kernel):
    """The fused search, libsvm fold by fold, sklearn's GridSearchCV over libsvm and over decoders.SVC on one grid: computed once,
    shared by the tests below (read-only)."""
    from cross_patient_speech_decoding_amd.decoders import SVC, SVCSearchCV
    X, y = recipe()
    grid = GRIDS[kernel]
    cands = list(ParameterGrid(grid))
    cv = StratifiedKFold(4)
    splits = list(cv.split(X, y))
    settings = dict(kernel=kernel, class_weight='balanced', tol=TOL)
    fused = SVCSearchCV(SVC(**settings), grid, cv=cv).fit(X, y)
    sk_pred, robust = libsvm_folds(lambda cand: SkSVC(decision_function_shape='ovo', **settings, **cand), cands, X, y, splits)
    sk_grid = GridSearchCV(SkSVC(**settings), grid, cv=cv).fit(X, y)
    store = {}
    dev_grid = GridSearchCV(SVC(**settings), grid, cv=cv, scoring=by_fold_scorer(X, splits, store), refit=False).fit(X, y)
    dev_pred = {(c, f): store[repr(sorted(SVC(**settings, **cand).get_params().items())), f] for c, cand in enumerate(cands) for f in range(4)}
    return dict(X=X, y=y, cands=cands, splits=splits, fused=fused, sk_pred=sk_pred, robust=robust, sk_grid=sk_grid, dev_grid=dev_grid,
                dev_pred=dev_pred, settings=settings)


def movable(s, c):
    """How far the non-robust rows of candidate c can move its mean score: each moves its fold's accuracy by 1 / len(fold)."""
    return sum((~s['robust'][c, f]).sum() / len(te) for f, (_, te) in enumerate(s['splits'])) / len(s['splits'])


@pytest.mark.parametrize('kernel', ['rbf', 'linear'])
def test_search_predicts_as_libsvm_on_every_robust_row(kernel):
    s = searched(kernel)
    fused = s['fused']
    assert fused.n_splits_ == 4 and len(fused.cv_test_predictions_) == 4
    assert fused.cv_results_['params'] == s['cands'] == s['sk_grid'].cv_results_['params']
    total = weak = 0
    for f, (te, labels) in enumerate(fused.cv_test_predictions_):
        np.testing.assert_array_equal(te, s['splits'][f][1])
        assert labels.shape == (len(s['cands']), len(te))
        for c in range(len(s['cands'])):
            ok = s['robust'][c, f]
            np.testing.assert_array_equal(labels[c][ok], s['sk_pred'][c, f][ok])
            total += len(ok)
            weak += int((~ok).sum())
    print(f'{kernel}: {weak} of {total} rows are not robust ({weak / total:.4f})')
    assert weak / total <= 0.03                                           # a condition on the input, not a tolerance
    means = s['sk_grid'].cv_results_['mean_test_score']
    order = np.argsort(-means, kind='stable')
    best, second = order[0], order[1]
    print(f'{kernel}: libsvm best {s["cands"][best]} {means[best]:.4f}, runner-up {means[second]:.4f}; fused best {fused.best_params_} '
          f'{fused.best_score_:.4f}')
    if means[best] - means[second] > movable(s, best) + movable(s, second):
        assert fused.best_params_ == s['sk_grid'].best_params_
        assert fused.best_index_ == s['sk_grid'].best_index_


@pytest.mark.parametrize('kernel', ['rbf', 'linear'])
def test_search_scores_are_sklearns_metrics_of_its_own_predictions(kernel):
    from cross_patient_speech_decoding_amd.decoders import search as S
    s = searched(kernel)
    fused, y = s['fused'], s['y']
    res = fused.cv_results_
    bal = S.scores_from_confusion(fused.cv_confusion_, 'balanced_accuracy')
    assert fused.cv_confusion_.shape == (len(s['cands']), 4, 4, 4) and fused.cv_confusion_.dtype == np.int32
    for f, (te, labels) in enumerate(fused.cv_test_predictions_):
        for c in range(len(s['cands'])):
            assert res[f'split{f}_test_score'][c] == accuracy_score(y[te], labels[c])
            assert bal[c, f] == balanced_accuracy_score(y[te], labels[c])
            want = np.zeros((4, 4), dtype=np.int32)
            np.add.at(want, (y[te], labels[c]), 1)
            np.testing.assert_array_equal(fused.cv_confusion_[c, f], want)
    table = np.array([res[f'split{f}_test_score'] for f in range(4)]).T
    again = S.assemble_results(s['cands'], table)
    for key in ('mean_test_score', 'std_test_score', 'rank_test_score'):
        np.testing.assert_array_equal(res[key], again[key])
    assert fused.best_index_ == int(np.flatnonzero(res['rank_test_score'] == 1)[0])
    assert fused.best_params_ == s['cands'][fused.best_index_] and fused.best_score_ == res['mean_test_score'][fused.best_index_]
    np.testing.assert_array_equal(fused.classes_, np.unique(y))


@pytest.mark.parametrize('kernel', ['rbf', 'linear'])
def test_search_agrees_with_gridsearchcv_around_the_device_svc(kernel):
    s = searched(kernel)
    fused = s['fused']
    for f, (te, labels) in enumerate(fused.cv_test_predictions_):
        for c in range(len(s['cands'])):
            ok = s['robust'][c, f]
            np.testing.assert_array_equal(labels[c][ok], s['dev_pred'][c, f][ok])
    diff = np.abs(fused.cv_results_['mean_test_score'] - s['dev_grid'].cv_results_['mean_test_score'])
    room = np.array([movable(s, c) for c in range(len(s['cands']))])
    print(f'{kernel}: max |mean - GridSearchCV(decoders.SVC) mean| = {diff.max():.4f}, room {room.max():.4f}')
    assert (diff <= room + 1e-12).all()


def test_refit_candidates_and_determinism():
    from cross_patient_speech_decoding_amd.decoders import SVC, SVCSearchCV
    s = searched('rbf')
    X, y, fused = s['X'], s['y'], s['fused']
    alone = SVC(**s['settings'], **fused.best_params_).fit(X, y)
    Xnew = recipe(seed=2)[0]
    np.testing.assert_array_equal(fused.predict(Xnew), alone.predict(Xnew))
    np.testing.assert_array_equal(fused.decision_function(Xnew), alone.decision_function(Xnew))
    assert fused.score(X, y) == alone.score(X, y)
    np.testing.assert_array_equal(fused.classes_, alone.classes_)
    cv = StratifiedKFold(4)
    again = SVCSearchCV(SVC(**s['settings']), GRIDS['rbf'], cv=cv, refit=False).fit(X, y)             # two runs: bit-identical
    listed = SVCSearchCV(SVC(**s['settings']), candidates=s['cands'], cv=cv, refit=False).fit(X, y)   # candidates= the same list
    chunked = SVCSearchCV(SVC(**s['settings']), GRIDS['rbf'], cv=cv, refit=False, max_kernel_bytes=8 * 120 * 120).fit(X, y)
    for other in (again, listed, chunked):
        np.testing.assert_array_equal(other.cv_confusion_, fused.cv_confusion_)
        for (_, a), (_, b) in zip(other.cv_test_predictions_, fused.cv_test_predictions_):
            np.testing.assert_array_equal(a, b)
        for key in ('mean_test_score', 'std_test_score', 'rank_test_score'):
            np.testing.assert_array_equal(other.cv_results_[key], fused.cv_results_[key])
        assert other.best_params_ == fused.best_params_ and not hasattr(other, 'best_estimator_')
    with pytest.raises(AttributeError, match='best_estimator_'):
        again.predict(X)


def test_a_small_max_kernel_bytes_cuts_the_search_into_chunks(monkeypatch):
    """One kernel matrix per chunk: the rbf grid has six matrices (gamma 0.01, 0.1 and 'scale' of four folds)."""
    from cross_patient_speech_decoding_amd.decoders import SVC, SVCSearchCV
    from cross_patient_speech_decoding_amd.decoders import search as S
    s = searched('rbf')
    chunks = []
    real = S._run_chunk
    monkeypatch.setattr(S, '_run_chunk', lambda plan, mats, *a: (chunks.append(list(mats)), real(plan, mats, *a))[1])
    got = SVCSearchCV(SVC(**s['settings']), GRIDS['rbf'], cv=StratifiedKFold(4), refit=False, max_kernel_bytes=2 * 8 * 120 * 120).fit(s['X'], s['y'])
    assert chunks == [[0, 1], [2, 3], [4, 5]]
    np.testing.assert_array_equal(got.cv_confusion_, s['fused'].cv_confusion_)
    with pytest.raises(ValueError, match='max_kernel_bytes'):
        SVCSearchCV(SVC(**s['settings']), GRIDS['rbf'], cv=4, max_kernel_bytes=8 * 120 * 120 - 1).fit(s['X'], s['y'])


def test_folds_that_do_not_partition_the_rows_and_a_fold_lacking_a_class():
    from cross_patient_speech_decoding_amd.decoders import SVC, SVCSearchCV
    rng = np.random.default_rng(5)
    sizes = [30, 28, 2]
    centres = rng.standard_normal((3, 6)) * 1.5
    y = np.repeat([1, 4, 7], sizes)
    X = centres[np.repeat(np.arange(3), sizes)] + rng.standard_normal((60, 6))
    perm = rng.permutation(60)
    X, y = X[perm], y[perm]
    rare = np.flatnonzero(y == 7)
    rest = np.flatnonzero(y != 7)
    splits = [(np.concatenate([rest[:35], rare[:1]]), np.concatenate([rest[30:50], rare[1:]])),     # train and test overlap
              (rest[10:45][::-1].copy(), np.concatenate([rare, rest[50:]])),                         # lost class 7; rows 0..9 unused
              (np.concatenate([rare, rest[20:]]), rest[:7])]
    settings = dict(kernel='linear', class_weight='balanced', tol=TOL)
    cands = [{'C': 0.1}, {'C': 1.0}]
    fused = SVCSearchCV(SVC(**settings), candidates=cands, cv=splits, scoring='balanced_accuracy').fit(X, y)
    plain = SVCSearchCV(SVC(**settings), candidates=cands, cv=splits, refit=False).fit(X, y)
    np.testing.assert_array_equal(plain.cv_confusion_, fused.cv_confusion_)
    sk_pred, robust = libsvm_folds(lambda cand: SkSVC(decision_function_shape='ovo', **settings, **cand), cands, X, y, splits)
    assert fused.n_splits_ == 3 and fused.cv_confusion_.shape == (2, 3, 3, 3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for f, (te, labels) in enumerate(fused.cv_test_predictions_):
            np.testing.assert_array_equal(te, splits[f][1])
            for c in range(2):
                ok = robust[c, f]
                np.testing.assert_array_equal(labels[c][ok], sk_pred[c, f][ok])
                own = SVC(**settings, **cands[c]).fit(X[splits[f][0]], y[splits[f][0]]).predict(X[te])
                np.testing.assert_array_equal(labels[c][ok], own[ok])
                assert fused.cv_results_[f'split{f}_test_score'][c] == balanced_accuracy_score(y[te], labels[c])
                assert plain.cv_results_[f'split{f}_test_score'][c] == accuracy_score(y[te], labels[c])
    assert sum((~ok).sum() for ok in robust.values()) <= 2
    assert (fused.cv_confusion_[:, 1, :, 2] == 0).all() and (fused.cv_confusion_[:, 1, 2].sum(axis=1) == 2).all()   # never predicts the lost class
    assert set(np.unique(fused.predict(X))) <= {1, 4, 7}


def test_pipeline_search_fits_the_earlier_steps_once_per_outer_combination_and_fold(monkeypatch):
    import cross_patient_speech_decoding_amd.alignment as A
    from cross_patient_speech_decoding_amd.decoders import SVC, SVCSearchCV
    from cross_patient_speech_decoding_amd.decomposition import DimRedReshape
    X, y = recipe()
    X3 = X.reshape(120, 6, 2)
    pipe = make_pipeline(DimRedReshape(A.PCA), SVC(kernel='rbf', class_weight='balanced', tol=TOL))
    grid = {'dimredreshape__n_components': [0.5, 0.9], 'svc__C': [1, 10], 'svc__gamma': [0.1, 'scale']}
    cands = list(ParameterGrid(grid))
    cv = StratifiedKFold(4)
    splits = list(cv.split(X3, y))
    fits = []
    real = DimRedReshape.fit
    monkeypatch.setattr(DimRedReshape, 'fit', lambda self, X, y=None: (fits.append(self.n_components), real(self, X, y))[1])
    fused = SVCSearchCV(pipe, grid, cv=cv, refit=False).fit(X3, y)
    assert sorted(fits) == [0.5] * 4 + [0.9] * 4                         # sklearn's GridSearchCV fits them 32 times
    assert fused.cv_results_['params'] == cands
    assert list(fused.cv_results_['param_dimredreshape__n_components']) == [c['dimredreshape__n_components'] for c in cands]
    # what GridSearchCV over the same pipeline does per (candidate, fold): clone, set, fit on the training rows, predict
    fitted = {}

    def features(cand, f):
        tr, te = splits[f]
        fitted[0] = clone(pipe).set_params(**cand).fit(X3[tr], y[tr])
        step = fitted[0].steps[0][1]
        return step.transform(X3[tr]), step.transform(X3[te])
    total = weak = 0
    for c, cand in enumerate(cands):
        for f, (tr, te) in enumerate(splits):
            sk_pred, robust = libsvm_folds(lambda cd: SkSVC(kernel='rbf', class_weight='balanced', tol=TOL, decision_function_shape='ovo',
                                                           C=cd['svc__C'], gamma=cd['svc__gamma']), [cand], X3, y, [(tr, te)],
                                           transform=lambda cd, _: features(cd, f))
            ok = robust[0, 0]
            own = fitted[0].predict(X3[te])
            labels = fused.cv_test_predictions_[f][1][c]
            np.testing.assert_array_equal(labels[ok], own[ok])
            np.testing.assert_array_equal(labels[ok], sk_pred[0, 0][ok])
            assert fused.cv_results_[f'split{f}_test_score'][c] == accuracy_score(y[te], labels)
            total += len(ok)
            weak += int((~ok).sum())
    print(f'pipeline: {weak} of {total} rows are not robust')
    assert weak / total <= 0.03
    monkeypatch.setattr(DimRedReshape, 'fit', real)
    best = SVCSearchCV(pipe, grid, cv=cv).fit(X3, y)
    np.testing.assert_array_equal(best.predict(X3), clone(pipe).set_params(**best.best_params_).fit(X3, y).predict(X3))


def test_one_launch_of_each_kernel_whatever_the_number_of_folds_and_candidates(monkeypatch):
    from collections import Counter
    from cross_patient_speech_decoding_amd import _lib
    from cross_patient_speech_decoding_amd.decoders import SVC, SVCSearchCV
    counts = Counter()
    real = _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    for mod in list(sys.modules.values()):                               # every module that bound `call` by name
        if getattr(mod, '__name__', '').startswith('cross_patient_speech_decoding_amd') and getattr(mod, 'call', None) is real:
            monkeypatch.setattr(mod, 'call', counting)
    X, y = recipe()
    svc = SVC(kernel='rbf', class_weight='balanced', tol=TOL)
    seen = []
    for folds, grid in ((4, GRIDS['rbf']), (8, {'C': [0.01, 0.1, 1, 10, 100, 1000], 'gamma': [0.01, 0.1, 'scale']})):
        counts.clear()
        search = SVCSearchCV(svc, grid, cv=folds, refit=False).fit(X, y)
        assert search.cv_confusion_.shape[:2] == (len(ParameterGrid(grid)), folds)
        assert counts['xps_rbf_multi_from_gram_f64'] == 1 and counts['xps_svm_smo_multi_f64'] == 1 and counts['xps_svm_cv_score_f64'] == 1, counts
        assert counts['xps_svm_smo_f64'] == 0 and counts['xps_rbf_from_gram_f64'] == 0 and counts['xps_bag_vote_f64'] == 0
        seen.append(dict(counts))
    assert seen[0] == seen[1]                                             # (with the Gram product and the norms' product)
    counts.clear()
    SVCSearchCV(svc, GRIDS['rbf'], cv=4).fit(X, y)                        # the refit goes through the existing path
    assert counts['xps_svm_smo_multi_f64'] == 1 and counts['xps_svm_smo_f64'] == 1 and counts['xps_rbf_from_gram_f64'] == 1
    counts.clear()
    SVCSearchCV(SVC(kernel='linear'), GRIDS['linear'], cv=4, refit=False).fit(X, y)
    assert counts['xps_rbf_multi_from_gram_f64'] == 0 and counts['xps_svm_smo_multi_f64'] == 1 and counts['xps_svm_cv_score_f64'] == 1
