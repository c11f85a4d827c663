"""The kernels of csrc/xps_rsa.hip on the MI355X: xps_row_standardize_grouped_f64 and xps_rdm_from_corr_grouped_f64 through their
wrappers in alignment/_linalg.py (with the ragged Gram launch between them, as alignment/rsa.py runs them), and
xps_rdm_compare_perm_f64 through the C ABI between guard rows.

References: tests/rsa_ref.py's long-double restatement within the bars it derives -- 4 (D + 6) u kappa_i kappa_j for a correlation
of two rows, 4 (L + 8) u kappa_x kappa_y for a comparison of two triangles of length L -- with scipy.stats.pearsonr beside it within
the sum of both sides' bars; every case asserts that its bar is below 1e-9, so that a wrong index or a dropped term (1e-3 or more)
cannot hide under it.  The bookkeeping of the comparison kernel is held bit for bit on small-integer matrices whose triangle means
are integers: every sum is then exact in any order.  Every matrix lives inside a larger sentinel-filled buffer with a leading
dimension above its width, and the frame is checked after the launches."""
import warnings

import numpy as np
import pytest
from scipy import stats

import rsa_ref as RR
from guarded_buf import SENT64, Buf64

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble


def torch_():
    import torch
    return torch


def LA():
    from cross_patient_speech_decoding_amd.alignment import _linalg
    return _linalg


def RSA():
    from cross_patient_speech_decoding_amd.alignment import rsa
    return rsa


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def same_values(a, b):
    """NaN in the same places (whatever its sign and payload) and the same bits everywhere else."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


class Framed:
    """A (rows, cols) float64 device matrix inside a (rows + 2, cols + pad) buffer of sentinels: view has ld = cols + pad."""

    def __init__(self, rows, cols, pad=3, data=None):
        torch = torch_()
        self.big = torch.full((rows + 2, cols + pad), SENT64, dtype=torch.int64, device=LA().device())
        self.view = self.big.view(torch.float64)[1:rows + 1, :cols]
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float64)))
        self.rows, self.cols = rows, cols

    def frame_intact(self):
        b = self.big.clone()
        b[1:self.rows + 1, :self.cols] = SENT64
        return bool((b == SENT64).all())

    def numpy(self):
        return self.view.cpu().numpy()

    def written(self):
        return bool((self.big[1:self.rows + 1, :self.cols] != SENT64).all())

    def untouched(self):
        return bool((self.big == SENT64).all())


# ------------------------------------------------------------------------------------------------ standardise, Gram, 1 - r
# five problems each; every n_c of {1, 2, 63, 64, 65, 130} and every D of {2, 3, 63, 64, 65, 257, 6000} occurs
BATCHES = {
    'small': [(1, 2), (2, 3), (63, 63), (64, 64), (65, 65)],
    'mixed': [(130, 257), (64, 6000), (2, 2), (65, 3), (63, 64)],
    'long': [(1, 6000), (130, 63), (64, 65), (63, 257), (2, 64)],
}


def batch_inputs(name):
    """Inputs of the form normal + 3.  In every problem with n_c >= 63: row 5 is constant and row 7 is 2^9 times row 6."""
    rng = np.random.default_rng(sorted(BATCHES).index(name))
    out = []
    for n_c, D in BATCHES[name]:
        X = rng.standard_normal((n_c, D)) + 3.0
        if n_c >= 63:
            X[5] = 0.1
            X[7] = X[6] * 2.0 ** 9
        out.append(X)
    return out


def run_rdm_chain(Xs):
    """standardise -> ragged Gram -> 1 - r (in place) on framed matrices; numpy results and the frames."""
    la, torch = LA(), torch_()
    fx = [Framed(*X.shape, data=X) for X in Xs]
    fz = [Framed(*X.shape, pad=5) for X in Xs]
    fg = [Framed(len(X), len(X)) for X in Xs]
    keep = [la.row_standardize_grouped([(x.view, z.view) for x, z in zip(fx, fz)]),
            la.gram_grouped([(z.view, g.view) for z, g in zip(fz, fg)])]
    torch.cuda.synchronize()
    r = [g.numpy() for g in fg]
    keep.append(la.rdm_from_corr_grouped([(g.view, g.view) for g in fg]))
    torch.cuda.synchronize()
    for f in fx + fz + fg:
        assert f.frame_intact(), 'an element outside a matrix was written'
        assert f.written(), 'an element of a matrix was never written'
    assert all(np.array_equal(bits(x.numpy()), bits(X)) for x, X in zip(fx, Xs)), 'an input changed'
    return [z.numpy() for z in fz], r, [g.numpy() for g in fg]


@pytest.mark.parametrize('name', sorted(BATCHES))
def test_correlations_of_a_ragged_batch_stay_within_the_bars_of_the_restatement_and_of_scipy(name):
    Xs = batch_inputs(name)
    Zs, rs, rdms = run_rdm_chain(Xs)
    alone = run_rdm_chain(Xs[1:2])                                       # the same bits alone as in the batch
    assert np.array_equal(bits(alone[0][0]), bits(Zs[1])) and np.array_equal(bits(alone[2][0]), bits(rdms[1]))
    worst = 0.0
    for (n_c, D), X, Z, r, rdm in zip(BATCHES[name], Xs, Zs, rs, rdms):
        const = (X == X[:, :1]).all(axis=1)
        assert const.sum() == (1 if n_c >= 63 else 0)
        live = ~const
        ref, bar = RR.pearson_rows(X), RR.corr_bar(X)
        assert bar[np.ix_(live, live)].max() < 1e-9, f'n_c={n_c} D={D}: a bar of {bar[np.ix_(live, live)].max():.2e} proves nothing'
        nan = np.isnan(r)
        assert np.array_equal(nan, const[:, None] | const[None, :])      # NaN in a constant row and column, nowhere else
        assert np.isnan(Z[const]).all() and not np.isnan(Z[live]).any()
        err = np.abs(r.astype(LD) - ref)[np.ix_(live, live)]
        assert (err <= bar[np.ix_(live, live)]).all(), f'n_c={n_c} D={D}: off by {float(err.max()):.3e}'
        worst = max(worst, float((err / bar[np.ix_(live, live)]).max()))
        assert np.array_equal(bits(r), bits(r.T))                        # the Gram launch's symmetry
        # 1 - clip(r), NaN kept, elementwise; the diagonal exactly 0 where it is not NaN
        want = 1.0 - np.where(nan, np.nan, np.clip(r, -1.0, 1.0))
        want[np.arange(n_c), np.arange(n_c)] = np.where(const, np.nan, 0.0)
        assert same_values(rdm, want)
        assert (np.diag(rdm)[live] == 0.0).all() and (rdm[np.ix_(live, live)] >= 0).all() and (rdm[np.ix_(live, live)] <= 2).all()
        if n_c >= 63:                                                     # a row scaled by 2^k: the same bits
            others = np.delete(np.arange(n_c), [6, 7])                   # (the two rows differ where one of them meets the diagonal)
            assert np.array_equal(bits(Z[7]), bits(Z[6])) and np.array_equal(bits(rdm[7, others]), bits(rdm[6, others]))
            assert rdm[6, 7] <= bar[6, 6]
        with warnings.catch_warnings():                                   # scipy beside it, on the first live rows
            warnings.simplefilter('ignore')
            for i in np.flatnonzero(live)[:4]:
                for j in np.flatnonzero(live):
                    assert abs(r[i, j] - stats.pearsonr(X[i], X[j])[0]) <= 2 * bar[i, j]
    print(f'{name}: largest fraction of the bar {worst:.2e}')


def test_a_row_whose_squared_deviations_underflow_is_nan_not_infinite():
    la, torch = LA(), torch_()
    X = np.array([[0.0, 1e-200, -1e-200, 2e-200], [1.0, 2.0, 4.0, 3.0], [5e-324, 0.0, 0.0, 0.0]])       # rows 0, 2 vary; norm 0
    src, out = Framed(3, 4, data=X), Framed(3, 4, pad=2)
    keep = la.row_standardize_grouped([(src.view, out.view)])
    torch.cuda.synchronize()
    Z = out.numpy()
    assert np.isnan(Z[[0, 2]]).all() and np.isfinite(Z[1]).all() and out.frame_intact()
    d = X[1] - 2.5
    assert np.abs(Z[1] - d / np.sqrt((d * d).sum())).max() <= 4 * U


def test_clipping_lets_nan_through_and_runs_out_of_place():
    la, torch = LA(), torch_()
    r = np.array([[1.0 + 2 * U * 2, -1.0 - 4 * U, np.nan], [0.25, np.nan, -0.5], [np.inf, -np.inf, 1.0]])
    src, out = Framed(3, 3, data=r), Framed(3, 3, pad=1)
    keep = la.rdm_from_corr_grouped([(src.view, out.view)])
    torch.cuda.synchronize()
    want = np.array([[0.0, 2.0, np.nan], [0.75, np.nan, 1.5], [0.0, 2.0, 0.0]])
    assert same_values(out.numpy(), want) and out.frame_intact() and np.array_equal(bits(src.numpy()), bits(r))


# ------------------------------------------------------------------------------------------------ the comparison kernel
def words(A, ia, B, ib, m, table, row):
    """The words of a pair; A, B: Framed matrices."""
    la = LA()
    w = np.zeros(la.RSA_PAIR_WORDS, dtype=np.int64)
    w[:11] = [A.view.data_ptr(), A.view.stride(0), A.rows, ia, B.view.data_ptr(), B.view.stride(0), B.rows, ib, m, table, row]
    return w


def raw_compare(pairs, tables, idx, perms, R, cosine=0, n_rows=None, check=True):
    """xps_rdm_compare_perm_f64 through the C ABI with both outputs between guard rows -> (stats, cross) as numpy."""
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import call, lib
    torch = torch_()
    pairs = np.ascontiguousarray(np.stack(pairs), dtype=np.int64)
    tables = np.ascontiguousarray(tables, dtype=np.int64).reshape(-1, 2)
    idx, perms = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1), np.ascontiguousarray(perms, dtype=np.int32).reshape(-1)
    n = len(pairs)
    n_rows = n if n_rows is None else n_rows
    st, cr = Buf64(4 * n_rows), Buf64((R + 1) * n_rows)
    nb = int(lib().xps_rdm_compare_perm_f64_workspace(n, len(tables), len(idx), len(perms)))
    assert nb >= 8 * pairs.size + 8 * tables.size + 4 * len(idx) + 4 * len(perms)
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=LA().device())
    call('xps_rdm_compare_perm_f64', pairs.ctypes.data, n, tables.ctypes.data, len(tables), idx.ctypes.data, len(idx),
         perms.ctypes.data, len(perms), R, cosine, st.ptr, cr.ptr, n_rows, ws.data_ptr(), nb, _dev.stream())
    torch.cuda.synchronize()
    assert st.guards_intact() and cr.guards_intact(), 'a guard element was written'
    stats_, cross = st.numpy((n_rows, 4)), cr.numpy((n_rows, R + 1))
    if check:
        assert (stats_ != SENT64).all() and (cross != SENT64).all(), 'an element was never written'
    return stats_.view(np.float64), cross.view(np.float64)


def perm_table(rng, m, R):
    return np.stack([np.arange(m)] + [rng.permutation(m) for _ in range(R)]).astype(np.int32)


def integer_matrix(rng, n, symmetric):
    M = rng.integers(-8, 9, size=(n, n))
    if symmetric:
        M = np.triu(M) + np.triu(M, 1).T
    return M.astype(np.int64)


def with_integer_triangle_mean(M, idx, symmetric):
    """M with the entry (idx[0], idx[1]) moved so that the triangle of M over idx adds up to a multiple of its length."""
    m = len(idx)
    L = m * (m - 1) // 2
    s = int(M[np.ix_(idx, idx)][np.triu_indices(m, k=1)].sum())
    M = M.copy()
    M[idx[0], idx[1]] -= s % L
    if symmetric:
        M[idx[1], idx[0]] = M[idx[0], idx[1]]
    return M


@pytest.mark.parametrize('m,R1,lists', [(3, 1, 'descending'), (4, 2, 'scattered'), (63, 64, 'scattered'), (64, 65, 'descending'),
                                        (65, 130, 'scattered'), (129, 2, 'scattered'), (129, 64, 'descending'), (64, 1, 'scattered')])
def test_small_integer_matrices_are_bit_equal_to_exact_integer_arithmetic(m, R1, lists):
    rng = np.random.default_rng(1000 * m + R1)
    R, L = R1 - 1, m * (m - 1) // 2
    na, nb = m + 7, m + 2                                                # the lists pick m conditions of larger matrices
    if lists == 'descending':
        ia, ib = np.arange(na)[::-1][:m].copy(), np.arange(nb)[::-1][2:m + 2].copy()
    else:
        ia, ib = rng.permutation(na)[:m], rng.permutation(nb)[:m]
    symmetric = R > 0                                                    # row 0 alone never reads below B's diagonal ...
    A = with_integer_triangle_mean(integer_matrix(rng, na, False), ia, False)      # ... nor does any row below A's
    B = with_integer_triangle_mean(integer_matrix(rng, nb, symmetric), ib, symmetric)
    P = perm_table(rng, m, R)
    fa, fb = Framed(na, na, data=A), Framed(nb, nb, pad=5, data=B)
    idx = np.concatenate([[99, 98], ia, [97], ib])                       # the lists start past the head of idx
    tri = np.triu_indices(m, k=1)
    x = A[np.ix_(ia, ia)][tri]
    ys = np.stack([B[np.ix_(ib[p], ib[p])][tri] for p in P])
    for cosine in (0, 1):
        stats_, cross = raw_compare([words(fa, 2, fb, 3 + m, m, 0, 0)], [[0, m]], idx, P, R, cosine)
        mx, my = (0, 0) if cosine else (x.sum() // L, ys[0].sum() // L)
        assert cosine or (x.sum() == mx * L and (ys.sum(axis=1) == my * L).all())
        want_stats = np.array([mx, my, ((x - mx) ** 2).sum(), ((ys[0] - my) ** 2).sum()], dtype=np.float64)
        want_cross = ((x - mx)[None, :] * (ys - my)).sum(axis=1).astype(np.float64)
        assert np.array_equal(bits(stats_[0]), bits(want_stats)), f'cosine={cosine}: the statistics'
        assert np.array_equal(bits(cross[0]), bits(want_cross)), f'cosine={cosine}: the cross products'
        alone = raw_compare([words(fa, 2, fb, 3 + m, m, 0, 0)], [[0, m]], idx, P[:1], 0, cosine)[1]
        assert np.array_equal(bits(alone[0]), bits(cross[0, :1]))        # row 0 is the unpermuted comparison
    assert fa.frame_intact() and fb.frame_intact()


def real_rdm(rng, n, D=40):
    M = np.asarray(RR.rdm_ref(rng.standard_normal((n, D)) + 3.0), dtype=np.float64)
    return 0.5 * (M + M.T)


@pytest.mark.parametrize('m,R', [(3, 3), (4, 1), (64, 5), (65, 2), (129, 3)])
def test_real_matrices_stay_within_the_bars_of_the_restatement_of_scipy_and_of_cos_sim(m, R):
    rsa = RSA()
    rng = np.random.default_rng(77 + m)
    na, nb = m + 3, m + 1
    A, B = real_rdm(rng, na), real_rdm(rng, nb)
    ia, ib = rng.permutation(na)[:m], rng.permutation(nb)[:m]
    P = perm_table(rng, m, R)
    fa, fb = Framed(na, na, data=A), Framed(nb, nb, data=B)
    idx = np.concatenate([ia, ib])
    x = RR.triangle(A, ia)
    worst = 0.0
    for method in ('pearson', 'cosine'):
        stats_, cross = raw_compare([words(fa, 0, fb, m, m, 0, 0)], [[0, m]], idx, P, R, int(method == 'cosine'))
        got = rsa._similarity(cross, stats_[:, 2:3], stats_[:, 3:4])[0]
        for r, p in enumerate(P):
            y = RR.triangle(B, ib[p])
            bar = RR.compare_bar(x, y, method)
            assert bar < 1e-9, f'a bar of {bar:.2e} proves nothing'
            err = abs(got[r] - RR.compare_ref(A, ia, B, ib, p, method))
            assert err <= bar, f'{method}, permutation {r}: off by {float(err):.3e}, bar {bar:.3e}'
            worst = max(worst, float(err / bar))
            theirs = stats.pearsonr(x, y)[0] if method == 'pearson' else rsa.cos_sim(x, y)
            assert abs(got[r] - theirs) <= 2 * bar
    print(f'm={m} R={R}: largest fraction of the bar {worst:.2e}')


def test_a_pair_gives_the_same_bits_alone_among_130_pairs_of_mixed_m_and_in_two_launches():
    la, torch = LA(), torch_()
    rng = np.random.default_rng(9)
    R = 5
    sizes = [5, 64, 70, 131]
    mats = [Framed(n, n, data=real_rdm(rng, n, D=12)) for n in sizes]
    ms = [3, 4, 63, 64, 65, 129]
    tabs = {m: perm_table(rng, m, R) for m in ms}
    offs = np.cumsum([0] + [tabs[m].size for m in ms])
    tables = [[offs[t], m] for t, m in enumerate(ms)]
    perms = np.concatenate([tabs[m].reshape(-1) for m in ms])
    pairs, idx, lists = [], [], []
    for q in range(130):
        m = ms[q % len(ms)]
        fit = [i for i, n in enumerate(sizes) if n >= m]
        a, b = fit[rng.integers(len(fit))], fit[rng.integers(len(fit))]
        ia, ib = rng.permutation(sizes[a])[:m], rng.permutation(sizes[b])[:m]
        lists.append((a, ia, b, ib, m))
        pairs.append(words(mats[a], len(idx), mats[b], len(idx) + m, m, ms.index(m), q))
        idx = list(idx) + list(ia) + list(ib)
    batch = raw_compare(pairs, tables, idx, perms, R)
    again = raw_compare(pairs, tables, idx, perms, R)
    assert np.array_equal(bits(batch[0]), bits(again[0])) and np.array_equal(bits(batch[1]), bits(again[1]))
    for q in (0, 5, 64, 129):
        a, ia, b, ib, m = lists[q]
        alone = raw_compare([words(mats[a], 0, mats[b], m, m, 0, 0)], [[0, m]], np.concatenate([ia, ib]), tabs[m], R)
        assert np.array_equal(bits(alone[0][0]), bits(batch[0][q])) and np.array_equal(bits(alone[1][0]), bits(batch[1][q]))
    # output rows in another order, into a larger output: rows nobody names stay untouched
    moved = [w.copy() for w in pairs[:4]]
    for w, row in zip(moved, (6, 0, 3, 1)):
        w[la.CP_ROW] = row
    st, cr = raw_compare(moved, tables, idx, perms, R, n_rows=7, check=False)
    for w, row in zip(pairs[:4], (6, 0, 3, 1)):
        assert np.array_equal(bits(st[row]), bits(batch[0][w[la.CP_ROW]])) and np.array_equal(bits(cr[row]), bits(batch[1][w[la.CP_ROW]]))
    assert (bits(st[[2, 4, 5]]) == SENT64).all() and (bits(cr[[2, 4, 5]]) == SENT64).all()
    # the wrapper builds the same call
    entries = [(mats[a].view, int(pairs[q][la.CP_IA]), mats[b].view, int(pairs[q][la.CP_IB]), m, ms.index(m))
               for q, (a, ia, b, ib, m) in enumerate(lists)]
    stats_d, cross_d, keep = la.rdm_compare_perm(entries, idx, tables, perms, R)
    torch.cuda.synchronize()
    assert np.array_equal(bits(stats_d.cpu().numpy()), bits(batch[0])) and np.array_equal(bits(cross_d.cpu().numpy()), bits(batch[1]))
    assert all(f.frame_intact() for f in mats)


# ------------------------------------------------------------------------------------------------ refusals
def test_the_entries_refuse_bad_tables_before_any_launch():
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import XpsError, call, lib
    la, torch = LA(), torch_()
    X, Z, G = Framed(4, 6), Framed(4, 6), Framed(4, 4)
    ws = torch.empty(64, dtype=torch.int64, device=la.device())
    w, st = ws.data_ptr(), _dev.stream()

    def refused(match, name, *args):
        with pytest.raises(XpsError, match=match):
            call(name, *args, st)

    def table(words_, **edit):
        t = np.zeros((1, 8), dtype=np.int64)
        t[0, :len(words_)] = words_
        for k, v in edit.items():
            t[0, int(k[1:])] = v
        return t
    std = [X.view.data_ptr(), X.view.stride(0), 4, 6, Z.view.data_ptr(), Z.view.stride(0)]
    for edit, match in ((dict(w0=0), 'null matrix'), (dict(w4=0), 'null matrix'), (dict(w1=5), 'ldx < D'), (dict(w5=5), 'ldz < D'),
                        (dict(w2=-1), 'row count'), (dict(w3=0), 'D outside'), (dict(w3=2 ** 31), 'D outside')):
        t = table(std, **edit)
        refused(match, 'xps_row_standardize_grouped_f64', t.ctypes.data, 1, w, 512)
    t = table(std)
    refused('null table', 'xps_row_standardize_grouped_f64', None, 1, w, 512)
    refused('negative count', 'xps_row_standardize_grouped_f64', t.ctypes.data, -1, w, 512)
    refused('65535', 'xps_row_standardize_grouped_f64', t.ctypes.data, 65536, w, 512)
    refused('null workspace', 'xps_row_standardize_grouped_f64', t.ctypes.data, 1, None, 512)
    refused('workspace too small', 'xps_row_standardize_grouped_f64', t.ctypes.data, 1, w, 56)
    rdm = [G.view.data_ptr(), G.view.stride(0), 4, G.view.data_ptr(), G.view.stride(0)]
    for edit, match in ((dict(w0=0), 'null matrix'), (dict(w3=0), 'null matrix'), (dict(w1=3), 'ldg < n'), (dict(w4=3), 'ldo < n'),
                        (dict(w2=-1), 'n outside')):
        t = table(rdm, **edit)
        refused(match, 'xps_rdm_from_corr_grouped_f64', t.ctypes.data, 1, w, 512)
    t = table(rdm)
    refused('null table', 'xps_rdm_from_corr_grouped_f64', None, 1, w, 512)
    refused('null workspace', 'xps_rdm_from_corr_grouped_f64', t.ctypes.data, 1, None, 512)
    refused('workspace too small', 'xps_rdm_from_corr_grouped_f64', t.ctypes.data, 1, w, 56)
    assert lib().xps_row_standardize_grouped_f64_workspace(-1) == 0 and lib().xps_rdm_from_corr_grouped_f64_workspace(3) == 192

    m, R = 4, 2
    A = Framed(6, 6, data=np.ones((6, 6)))
    good = words(A, 0, A, m, m, 0, 0)
    idx = np.array([0, 1, 2, 5, 5, 4, 3, 2], dtype=np.int32)
    perms = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 3, 2]], dtype=np.int32)
    tables = np.array([[0, m]], dtype=np.int64)
    stats_, cross = Buf64(4), Buf64(R + 1)

    def compare(match, pair=good, tables=tables, idx=idx, perms=perms, R=R, cosine=0, n_rows=1, s=stats_.ptr, c=cross.ptr, wsp=w,
                nb=512, n_pairs=1, null=()):
        p = np.ascontiguousarray(pair.reshape(1, -1))
        args = dict(pairs=p.ctypes.data, tables=tables.ctypes.data, idx=idx.ctypes.data, perms=perms.ctypes.data)
        for k in null:
            args[k] = None
        refused(match, 'xps_rdm_compare_perm_f64', args['pairs'], n_pairs, args['tables'], len(tables), args['idx'], len(idx),
                args['perms'], perms.size, R, cosine, s, c, n_rows, wsp, nb)

    def edited(**edit):
        p = good.copy()
        for k, v in edit.items():
            p[getattr(la, k)] = v
        return p
    for k in ('pairs', 'tables', 'idx', 'perms'):
        compare('null table', null=(k,))
    compare('null output', s=None)
    compare('null output', c=None)
    compare('negative count', n_pairs=-1)
    compare('negative count', n_rows=-1)
    compare('R outside', R=-1)
    compare('cosine must be 0 or 1', cosine=2)
    compare('null matrix', pair=edited(CP_A=0))
    compare('null matrix', pair=edited(CP_B=0))
    compare('lda < n', pair=edited(CP_LDA=5))
    compare('ldb < n', pair=edited(CP_LDB=5))
    compare('m outside 2', pair=edited(CP_M=1))
    compare('m outside 2', pair=edited(CP_M=la.RSA_MAX_CONDITIONS + 1))
    compare('m outside 2', tables=np.array([[0, 1]], dtype=np.int64))
    compare("a pair's table has another m", pair=edited(CP_M=3))
    compare('names no permutation table', pair=edited(CP_TABLE=1))
    compare('names no permutation table', pair=edited(CP_TABLE=-1))
    compare('an output row outside', pair=edited(CP_ROW=1))
    compare('an output row outside', pair=edited(CP_ROW=-1))
    compare('an index list reaches outside idx', pair=edited(CP_IB=5))
    compare('an index list reaches outside idx', pair=edited(CP_IA=-1))
    compare('an index at or past the matrix size', pair=edited(CP_NA=5, CP_LDA=9))                # idx holds a 5
    compare('an index at or past the matrix size', idx=np.array([0, 1, 2, 6, 5, 4, 3, 2], dtype=np.int32))
    compare('an index at or past the matrix size', idx=np.array([0, 1, 2, 3, 5, 4, -1, 2], dtype=np.int32))
    compare('not a permutation', perms=np.array([[0, 1, 2, 3], [3, 2, 2, 0], [1, 0, 3, 2]], dtype=np.int32))       # repeats an entry
    compare('not a permutation', perms=np.array([[0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 4, 2]], dtype=np.int32))
    compare('not a permutation', perms=np.array([[0, 1, 2, 3], [3, 2, 1, 0], [1, 0, -1, 2]], dtype=np.int32))
    compare('row 0 of a table is not the identity', perms=np.array([[1, 0, 2, 3], [3, 2, 1, 0], [1, 0, 3, 2]], dtype=np.int32))
    compare('a permutation table reaches outside perms', perms=perms[:2])
    compare('a permutation table reaches outside perms', tables=np.array([[1, m]], dtype=np.int64))
    compare('a permutation table reaches outside perms', tables=np.array([[-4, m]], dtype=np.int64))
    compare('null workspace', wsp=None)
    compare('workspace too small', nb=8 * 12 + 16 + 32 + 48 - 8)
    torch.cuda.synchronize()
    assert stats_.untouched() and cross.untouched()                      # nothing was launched
    assert X.untouched() and Z.untouched() and G.untouched()
    assert lib().xps_rdm_compare_perm_f64_workspace(1, 1, 8, 12) == 8 * 12 + 16 + 32 + 48
    assert lib().xps_rdm_compare_perm_f64_workspace(-1, 1, 8, 12) == 0
