"""The label-grouped sum kernels of csrc/xps_cluster.hip on the MI355X, through their wrappers in alignment/_linalg.py
(label_row_sums, label_col_sums, silhouette_from_sums, centroid_dist_from_sums) and, for the guard rows and the refusals of the
entries, through the C ABI.

References: small-integer operands, for which every sum is exact in any order (bit-equal); real operands against long-double
sums within (n + 2) u sum_j |G_ij| (mode 0: an ascending float64 sum of at most n terms, plus the reference's own rounding) and
(c + 3) u sum_j d_ij over the c terms of a bin (mode 1: the terms are the float64 values of sqrt(max((G_ii + G_jj) - 2 G_ij, 0)),
each operation rounded once as the kernel rounds it; the sqrt and its argument count once per term).  The silhouette rules are
elementwise IEEE operations, so they are held bit for bit against numpy on the kernel's own sums, and the three statistics
against the kernel's summation order restated in numpy (lane-strided ascending sums, then the xor butterfly).
Shapes: the smallest at which the tiling can go wrong -- n around the 64-lane stride of the staging loop and one n (300) beyond
the 256-element LDS segment, R around the 64 label sets of a workgroup, k from 2 to the limit of 64.  G lives in a NaN-padded
buffer with ldg = n + 3."""
import numpy as np
import pytest

from guarded_buf import SENT64, Buf64

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
PAD = 3
# (n, k, R): every n of {3, 63, 64, 65, 130}, every k of {2, 3, 9, 64}, every R of {1, 2, 63, 64, 65, 130}
SHAPES = [(3, 2, 1), (3, 64, 65), (63, 3, 2), (63, 9, 63), (64, 9, 64), (64, 2, 130), (65, 3, 65), (65, 64, 1), (130, 9, 130),
          (130, 64, 63), (130, 3, 64), (64, 64, 2), (300, 9, 3)]


def torch_():
    import torch
    return torch


def LA():
    from cross_patient_speech_decoding_amd.alignment import _linalg
    return _linalg


def dev(a):
    return torch_().from_numpy(np.ascontiguousarray(a)).to(LA().device())


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def padded_gram(G):
    """G in the leading block of an (n + 1, n + PAD) NaN-filled device tensor: a view with ldg = n + PAD."""
    n = len(G)
    big = np.full((n + 1, n + PAD), np.nan)
    big[:n, :n] = G
    return dev(big)[:n, :n]


def label_sets(rng, n, k, R):
    """(n, R) uint8 labels in [0, k).  Set 0: class 0 holds sample 0 alone (a singleton class).  The last set (set 0 when R = 1)
    has no sample of class k - 1 when k >= 3 (an empty class)."""
    y = rng.integers(0, k, size=(n, R))
    y[:, 0] = np.where(y[:, 0] == 0, 1, y[:, 0])
    y[0, 0] = 0
    if k >= 3:
        last = y[:, R - 1]
        y[:, R - 1] = np.where(last == k - 1, 1, last)
    return y.astype(np.uint8)


def counts_of(y, k):
    return np.stack([np.bincount(y[:, r], minlength=k) for r in range(y.shape[1])]).astype(np.int32)


def bin_sums(F, y, k, dtype):
    """S[r][i][q] = sum over j with y[j][r] == q of F[i][j], accumulated in `dtype`."""
    n, R = y.shape
    onehot = (y[:, :, None] == np.arange(k)).astype(dtype)                 # (n, R, k)
    return np.einsum('ij,jrq->riq', F.astype(dtype), onehot)


def mode1_terms(G):
    g = np.diag(G)
    t = np.sqrt(np.maximum((g[:, None] + g[None, :]) - 2.0 * G, 0.0))
    np.fill_diagonal(t, 0.0)
    return t


def wave_stats(s):
    """(mean, positive mean, positive count) of one set in the kernel's order: lane l adds its terms l, l + 64, ... ascending
    from 0.0, then the 64 partial sums meet in the xor butterfly 32, 16, 8, 4, 2, 1."""
    def total(v):
        part = np.zeros(64)
        for i, x in enumerate(v):
            part[i % 64] = part[i % 64] + x
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            part = part + part[lanes ^ o]
        return part[0]
    pos = np.where(s > 0, s, 0.0)
    npos = total((s > 0).astype(np.float64))
    with np.errstate(invalid='ignore'):
        return np.array([total(s) / len(s), total(pos) / npos, npos])


def numpy_silhouettes(S, y, cnt):
    """sklearn's rules, elementwise in float64, on the sums S (R, n, k)."""
    R, n, k = S.shape
    out = np.zeros((R, n))
    for r in range(R):
        own = y[:, r].astype(int)
        c = cnt[r].astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            means = np.where(c > 0, S[r] / np.where(c > 0, c, 1.0), np.inf)
            means[np.arange(n), own] = np.inf
            b = means.min(axis=1)
            a = S[r][np.arange(n), own] / (c[own] - 1.0)
            s = (b - a) / np.maximum(a, b)
        out[r] = np.where((c[own] > 1) & np.isfinite(s), s, 0.0)
    return out


def everything(G, y, k):
    """All four kernels on one Gram matrix and label array; numpy results."""
    la = LA()
    Gd, lt, cnt = padded_gram(G), dev(y), counts_of(y, k)
    S0, S1 = la.label_row_sums(Gd, lt, k, 0), la.label_row_sums(Gd, lt, k, 1)
    sil, stats, keep1 = la.silhouette_from_sums(S1, cnt, lt)
    M = la.label_col_sums(S0, lt, k)
    dg = la.label_col_sums(dev(np.diag(G).copy().reshape(-1, 1)), lt, k)
    dist, keep2 = la.centroid_dist_from_sums(Gd, S0, M, cnt, lt)
    intra = la.label_col_sums(dist.view(y.shape[1], len(G), 1), lt, k)
    torch_().cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in dict(S0=S0, S1=S1, sil=sil, stats=stats, M=M, dg=dg, dist=dist, intra=intra).items()}


@pytest.mark.parametrize('n,k,R', SHAPES)
def test_small_integer_operands_are_bit_equal_to_the_exact_sums(n, k, R):
    rng = np.random.default_rng(100 * n + 10 * k + R)
    G = rng.integers(-8, 9, size=(n, n)).astype(np.float64)
    y = label_sets(rng, n, k, R)
    la, lt = LA(), dev(y)
    S0 = la.label_row_sums(padded_gram(G), lt, k, 0)
    exact = bin_sums(G, y, k, np.int64)
    np.testing.assert_array_equal(S0.cpu().numpy(), exact.astype(np.float64))
    M = la.label_col_sums(S0, lt, k).cpu().numpy()                                     # w = k, one table per set
    np.testing.assert_array_equal(M, np.einsum('riq,irp->rpq', exact, (y[:, :, None] == np.arange(k)).astype(np.int64)))
    v = rng.integers(-8, 9, size=(n, 1)).astype(np.float64)                            # w = 1, one table for every set
    col = la.label_col_sums(dev(v), lt, k).cpu().numpy()
    np.testing.assert_array_equal(col[:, :, 0], bin_sums(v.T, y, k, np.int64)[:, 0, :])
    V3 = rng.integers(-8, 9, size=(R, n, 2)).astype(np.float64)                        # w = 2, one table per set
    got = la.label_col_sums(dev(V3), lt, k).cpu().numpy()
    want = np.einsum('ric,irp->rpc', V3, (y[:, :, None] == np.arange(k)).astype(np.float64))
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize('n,k,R', SHAPES)
def test_real_operands_stay_within_the_derived_bounds_and_the_rules_are_sklearns(n, k, R):
    rng = np.random.default_rng(200 * n + 10 * k + R)
    V = rng.standard_normal((n, 7))
    G = V @ V.T
    G = 0.5 * (G + G.T)
    y = label_sets(rng, n, k, R)
    cnt = counts_of(y, k)
    out = everything(G, y, k)
    # mode 0: (n + 2) u sum_j |G_ij| against the long-double sum, per bin
    err0 = np.abs(out['S0'].astype(LD) - bin_sums(G, y, k, LD))
    bound0 = (n + 2) * U * np.abs(G).sum(axis=1)[None, :, None]
    assert (err0 <= bound0).all()
    # mode 1: (c + 3) u sum of the bin's terms against the long-double sum of the same float64 terms
    t = mode1_terms(G)
    err1 = np.abs(out['S1'].astype(LD) - bin_sums(t, y, k, LD))
    bound1 = (cnt[:, None, :] + 3) * U * bin_sums(t, y, k, LD)
    assert (err1 <= bound1).all()
    print(f'n={n} k={k} R={R}: largest error / bound, mode 0 {float((err0 / bound0).max()):.3f}, '
          f'mode 1 {float(np.where(bound1 > 0, err1 / np.where(bound1 > 0, bound1, 1), 0).max()):.3f}')
    assert (out['S1'] >= 0).all()
    assert out['S1'][0, 0, 0] == 0.0                                  # sample 0 alone in class 0 of set 0: only the diagonal term
    # sklearn's rules, bit for bit on the kernel's own sums; the statistics in the kernel's own order
    np.testing.assert_array_equal(bits(out['sil']), bits(numpy_silhouettes(out['S1'], y, cnt)))
    assert out['sil'][0, 0] == 0.0
    for r in sorted({0, R // 2, R - 1}):
        np.testing.assert_array_equal(out['stats'][r], wave_stats(out['sil'][r]))       # (NaN == NaN here: no positive value)
    # class-block sums and diagonal sums: ascending sums of at most n terms
    sel = (y[:, :, None] == np.arange(k))                                              # (n, R, k)
    Mref = np.einsum('riq,irp->rpq', out['S0'].astype(LD), sel.astype(LD))
    Mabs = np.einsum('riq,irp->rpq', np.abs(out['S0']), sel.astype(np.float64))
    assert (np.abs(out['M'].astype(LD) - Mref) <= (n + 2) * U * Mabs).all()
    assert (np.abs(out['dg'][:, :, 0].astype(LD) - bin_sums(np.diag(G)[None, :], y, k, LD)[:, 0, :]) <= (n + 2) * U * np.trace(G)).all()
    # own-centroid distances: the terms below carry the kernel's own roundings; two additions, the root and the reference's
    # evaluation of it each add at most u of the terms' total size, with a factor 2 for the square taken here
    own = y.T.astype(int)                                                                # (R, n)
    rr = np.arange(R)[:, None]
    npo = cnt[rr, own].astype(np.float64)
    terms = np.stack([np.broadcast_to(np.diag(G), (R, n)), 2.0 * out['S0'][rr, np.arange(n)[None, :], own] / npo,
                      out['M'][rr, own, own] / (npo * npo)])
    d2 = terms[0].astype(LD) - terms[1] + terms[2]
    assert (np.abs(out['dist'].astype(LD) ** 2 - np.maximum(d2, 0)) <= 8 * U * np.abs(terms).sum(axis=0)).all()
    assert out['dist'][0, 0] == 0.0                                                     # the singleton sits on its centroid
    assert (np.abs(out['intra'][:, :, 0].astype(LD) - np.einsum('ri,irp->rp', out['dist'].astype(LD), sel.astype(LD)))
            <= (n + 2) * U * out['dist'].sum(axis=1)[:, None]).all()


def test_a_label_set_gives_the_same_bits_alone_as_in_a_batch_of_130_and_in_two_launches():
    n, k, R = 130, 9, 130
    rng = np.random.default_rng(5)
    V = rng.standard_normal((n, 7))
    G = V @ V.T
    y = label_sets(rng, n, k, R)
    batch, again = everything(G, y, k), everything(G, y, k)
    for name in batch:
        assert np.array_equal(bits(batch[name]), bits(again[name])), f'{name}: two launches differ'
    for r in (0, 63, 64, 129):
        alone = everything(G, y[:, r:r + 1], k)
        for name in batch:
            assert np.array_equal(bits(alone[name][0]), bits(batch[name][r])), f'{name}: set {r} depends on the batch'
    wide = everything(G, y[:, :3], 64)                                  # more (empty) classes beside the same labels
    assert np.array_equal(bits(wide['S1'][:, :, :k]), bits(batch['S1'][:3])) and not wide['S1'][:, :, k:].any()
    assert np.array_equal(bits(wide['sil']), bits(batch['sil'][:3])) and np.array_equal(bits(wide['stats']), bits(batch['stats'][:3]))
    assert np.array_equal(bits(wide['dist']), bits(batch['dist'][:3]))


def test_a_label_at_or_above_k_is_skipped_not_used_as_an_index():
    n, k, R = 65, 3, 2
    rng = np.random.default_rng(6)
    G = rng.integers(-8, 9, size=(n, n)).astype(np.float64)
    y = label_sets(rng, n, k, R)
    bad = y.copy()
    bad[5, 1], bad[9, 0] = 255, 3
    la = LA()
    S0 = la.label_row_sums(padded_gram(G), dev(bad), k, 0).cpu().numpy()
    keep = np.ones((n, R), dtype=bool)
    keep[5, 1] = keep[9, 0] = False
    want = np.einsum('ij,jrq->riq', G, ((bad[:, :, None] == np.arange(k)) & keep[:, :, None]).astype(np.float64))
    np.testing.assert_array_equal(S0, want)
    M = la.label_col_sums(dev(np.ones((n, 1))), dev(bad), k).cpu().numpy()[:, :, 0]
    np.testing.assert_array_equal(M, [[np.sum(bad[:, r] == p) for p in range(k)] for r in range(R)])
    S1 = la.label_row_sums(padded_gram(G @ G.T), dev(bad), k, 1)
    sil, stats, _ = la.silhouette_from_sums(S1, counts_of(np.where(keep, bad, 0), k), dev(bad))
    assert sil[1, 5].item() == 0.0 and sil[0, 9].item() == 0.0 and bool(torch_().isfinite(sil).all())


# ------------------------------------------------------------------------------------------------ guard rows, through the C ABI
def test_nothing_is_written_outside_the_outputs():
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import call, lib
    torch = torch_()
    for n, k, R in ((3, 2, 1), (65, 9, 65), (130, 64, 130)):
        rng = np.random.default_rng(n)
        V = rng.standard_normal((n, 5))
        G = V @ V.T
        y = label_sets(rng, n, k, R)
        want = everything(G, y, k)
        Gd, lt, cnt = padded_gram(G), dev(y), counts_of(y, k)
        S0, S1, sil, stats = Buf64(R * n * k), Buf64(R * n * k), Buf64(R * n), Buf64(R * 3)
        M, dist, intra = Buf64(R * k * k), Buf64(R * n), Buf64(R * k)
        nb = int(lib().xps_silhouette_from_sums_f64_workspace(R, k))
        assert nb >= 4 * R * k and nb == int(lib().xps_centroid_dist_from_sums_f64_workspace(R, k))
        ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=LA().device())
        st = _dev.stream()
        call('xps_label_row_sums_f64', Gd.data_ptr(), n + PAD, lt.data_ptr(), n, R, k, 0, S0.ptr, st)
        call('xps_label_row_sums_f64', Gd.data_ptr(), n + PAD, lt.data_ptr(), n, R, k, 1, S1.ptr, st)
        call('xps_silhouette_from_sums_f64', S1.ptr, cnt.ctypes.data, lt.data_ptr(), n, R, k, sil.ptr, stats.ptr, ws.data_ptr(), nb, st)
        call('xps_label_col_sums_f64', S0.ptr, n * k, lt.data_ptr(), n, R, k, k, M.ptr, st)
        call('xps_centroid_dist_from_sums_f64', Gd.data_ptr(), n + PAD, S0.ptr, M.ptr, cnt.ctypes.data, lt.data_ptr(), n, R, k,
             dist.ptr, ws.data_ptr(), nb, st)
        call('xps_label_col_sums_f64', dist.ptr, n, lt.data_ptr(), n, R, k, 1, intra.ptr, st)
        torch.cuda.synchronize()
        for name, buf in dict(S0=S0, S1=S1, sil=sil, stats=stats, M=M, dist=dist, intra=intra).items():
            assert buf.guards_intact(), f'{name}: a guard element was written'
            got = buf.numpy(want[name].shape)
            assert (got != SENT64).all(), f'{name}: an element was never written'
            assert np.array_equal(got, bits(want[name])), name


# ------------------------------------------------------------------------------------------------ refusals
def test_the_entries_refuse_bad_arguments_before_any_launch():
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import XpsError, call, lib
    torch = torch_()
    n, k, R = 10, 3, 2
    G = dev(np.ones((n, n)))
    lt = dev(np.zeros((n, R), dtype=np.uint8))
    out = Buf64(R * n * k)
    cnt = np.array([[10, 0, 0], [10, 0, 0]], dtype=np.int32)
    ws = torch.empty(16, dtype=torch.int64, device=LA().device())
    g, l, o, w, c = G.data_ptr(), lt.data_ptr(), out.ptr, ws.data_ptr(), cnt.ctypes.data

    def refused(match, name, *args):
        with pytest.raises(XpsError, match=match):
            call(name, *args, _dev.stream())
    for args, match in (((None, n, l, n, R, k, 0, o), 'null argument'), ((g, n, None, n, R, k, 0, o), 'null argument'),
                        ((g, n, l, n, R, k, 0, None), 'null argument'), ((g, n, l, 0, R, k, 0, o), 'n >= 1'),
                        ((g, n, l, n, 0, k, 0, o), 'R >= 1'), ((g, n, l, n, R, 1, 0, o), 'k <= 64'), ((g, n, l, n, R, 65, 0, o), 'k <= 64'),
                        ((g, n - 1, l, n, R, k, 0, o), 'ldg < n'), ((g, n, l, n, R, k, 2, o), 'mode'), ((g, n, l, n, R, k, -1, o), 'mode'),
                        ((g, n, l, n, 64 * 65535 + 1, k, 0, o), 'label sets')):
        refused(match, 'xps_label_row_sums_f64', *args)
    for args, match in (((None, 0, l, n, R, k, 1, o), 'null argument'), ((g, 0, None, n, R, k, 1, o), 'null argument'),
                        ((g, 0, l, n, R, k, 1, None), 'null argument'), ((g, 0, l, 0, R, k, 1, o), 'n >= 1'),
                        ((g, 0, l, n, R, 65, 1, o), 'k <= 64'), ((g, 0, l, n, R, k, 0, o), 'w < 1'),
                        ((g, n - 1, l, n, R, k, 1, o), 'v_set_stride'), ((g, -1, l, n, R, k, 1, o), 'v_set_stride'),
                        ((o, 0, l, n, R, k, 1, o), 'must differ')):
        refused(match, 'xps_label_col_sums_f64', *args)
    bad_sum, negative = cnt.copy(), cnt.copy()
    bad_sum[1, 2] = 1
    negative[0, :2] = (11, -1)
    for args, match in (((None, c, l, n, R, k, o, o, w, 64), 'null argument'), ((g, None, l, n, R, k, o, o, w, 64), 'null argument'),
                        ((g, c, None, n, R, k, o, o, w, 64), 'null argument'), ((g, c, l, n, R, k, None, o, w, 64), 'null argument'),
                        ((g, c, l, n, R, k, o, None, w, 64), 'null argument'), ((g, c, l, n, R, 1, o, o, w, 64), 'k <= 64'),
                        ((g, c, l, 0, R, k, o, o, w, 64), 'n >= 1'), ((g, bad_sum.ctypes.data, l, n, R, k, o, o, w, 64), 'add up to n'),
                        ((g, negative.ctypes.data, l, n, R, k, o, o, w, 64), 'add up to n'),
                        ((g, c, l, n, R, k, o, o, None, 64), 'null workspace'), ((g, c, l, n, R, k, o, o, w, 8), 'workspace too small')):
        refused(match, 'xps_silhouette_from_sums_f64', *args)
    for args, match in (((None, n, g, g, c, l, n, R, k, o, w, 64), 'null argument'), ((g, n, None, g, c, l, n, R, k, o, w, 64), 'null argument'),
                        ((g, n, g, None, c, l, n, R, k, o, w, 64), 'null argument'), ((g, n, g, g, None, l, n, R, k, o, w, 64), 'null argument'),
                        ((g, n, g, g, c, None, n, R, k, o, w, 64), 'null argument'), ((g, n, g, g, c, l, n, R, k, None, w, 64), 'null argument'),
                        ((g, n - 1, g, g, c, l, n, R, k, o, w, 64), 'ldg < n'), ((g, n, g, g, c, l, n, R, 65, o, w, 64), 'k <= 64'),
                        ((g, n, g, g, bad_sum.ctypes.data, l, n, R, k, o, w, 64), 'add up to n'),
                        ((g, n, g, g, c, l, n, R, k, o, None, 64), 'null workspace'), ((g, n, g, g, c, l, n, R, k, o, w, 8), 'workspace too small')):
        refused(match, 'xps_centroid_dist_from_sums_f64', *args)
    torch.cuda.synchronize()
    assert out.untouched()                                                  # nothing was launched
    assert lib().xps_silhouette_from_sums_f64_workspace(0, 3) == 0


def test_the_wrappers_refuse_bad_tensors_before_any_launch(monkeypatch):
    torch, la = torch_(), LA()
    calls = []
    monkeypatch.setattr(la, 'call', lambda name, *a: calls.append(name))
    n, k, R = 10, 3, 2
    G = torch.ones(n, n, dtype=torch.float64, device=la.device())
    lt = torch.zeros(n, R, dtype=torch.uint8, device=la.device())
    S = torch.ones(R, n, k, dtype=torch.float64, device=la.device())
    M = torch.ones(R, k, k, dtype=torch.float64, device=la.device())
    cnt = np.array([[10, 0, 0], [4, 3, 3]])
    for bad in ((G.cpu(), lt, k, 0), (G.float(), lt, k, 0), (G[:9], lt, k, 0), (G.t()[::2].t(), lt, k, 0), (G, lt.cpu(), k, 0),
                (G, lt.int(), k, 0), (G, lt[:, 0], k, 0), (G, lt.t(), k, 0), (G, lt, 1, 0), (G, lt, 65, 0), (G, lt, 2.5, 0),
                (G, lt, k, 2), (G, lt[:0], k, 0)):
        with pytest.raises(ValueError, match='label_row_sums'):
            la.label_row_sums(*bad)
    for bad in ((S.cpu(), lt, k), (S.float(), lt, k), (S[:1], lt, k), (S[:, :9], lt, k), (S.transpose(1, 2), lt, k), (S[0, 0], lt, k),
                (S, lt, 65), (S, lt.cpu(), k), (S[:, :, :0], lt, k)):
        with pytest.raises(ValueError, match='label_col_sums'):
            la.label_col_sums(*bad)
    for bad in ((S.cpu(), cnt, lt), (S[0], cnt, lt), (S[:, :9], cnt, lt), (S, cnt[:1], lt), (S, cnt.astype(float), lt),
                (S, np.array([[10, 0, 0], [4, 3, 2]]), lt), (S, np.array([[11, -1, 0], [4, 3, 3]]), lt), (S, cnt, lt.cpu()),
                (torch.ones(R, n, 1, dtype=torch.float64, device=la.device()), cnt[:, :1], lt)):
        with pytest.raises(ValueError, match='silhouette_from_sums'):
            la.silhouette_from_sums(*bad)
    for bad in ((G[:9], S, M, cnt, lt), (G, S.cpu(), M, cnt, lt), (G, S, M[:, :2], cnt, lt), (G, S, M.float(), cnt, lt),
                (G, S, M, cnt[:1], lt), (G, S, M, cnt, lt.cpu()), (G, S[0], M, cnt, lt)):
        with pytest.raises(ValueError, match='centroid_dist_from_sums'):
            la.centroid_dist_from_sums(*bad)
    assert calls == []
