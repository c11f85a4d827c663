"""rbf_grouped_kernel and var_grouped_kernel (csrc/xps_svm_grouped.hip) on the MI355X through the C ABI
(xps_rbf_grouped_from_gram_f64, xps_var_grouped_f64) and their wrappers alignment/_linalg.py: rbf_grouped, var_grouped.

rbf: every K_p must equal, bit for bit, what xps_rbf_from_gram_f64 writes for the same G with its diagonal as both norm vectors.
All outputs of a launch lie in ONE guarded sentinel buffer (tests/guarded_buf.py) with ldk = n + 3 and a gap between the matrices,
so a padding element, a gap element and a guard element that was written all show.

Variance: the reference is computed with math.fsum from the exact inputs (float32 widens exactly): mean = fsum(x) / count,
var = fsum((x - mean)^2) / count in float64.  The bound is relative 8 * r * D * 2^-53: the worst case of a two-pass float64 sum of
r * D terms in any order (each pass adds at most count - 1 roundings of 2^-53 relative to a sum of non-negative terms for the
deviations, the error of the mean enters squared, and the factor 8 covers both passes, the subtraction, the square and the two
divisions), so it holds for any correct implementation."""
import math

import numpy as np
import pytest

from guarded_buf import SENT64, Buf64

pytestmark = pytest.mark.gpu

PAD, GAP = 3, 37
NS = (1, 63, 64, 65, 130)


def torch_():
    import torch
    return torch


def LA():
    from cross_patient_speech_decoding_amd.alignment import _linalg
    return _linalg


def lib():
    from cross_patient_speech_decoding_amd._lib import lib as _l
    return _l()


def dev(a):
    return torch_().from_numpy(np.ascontiguousarray(a)).to(LA().device())


def gbits(gamma):
    return int(np.float64(gamma).view(np.int64))


# ------------------------------------------------------------------------------------------------ the rbf kernel
def rbf_entry(tab, n_problems, tiles, n_tiles, ws=None, ws_bytes=None):
    """xps_rbf_grouped_from_gram_f64 on host tables (None: a null pointer), then a synchronise."""
    torch = torch_()
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import call
    if ws is None:
        ws_bytes = int(lib().xps_rbf_grouped_from_gram_f64_workspace(max(n_problems, 0), max(n_tiles, 0)))
        ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=LA().device())
    call('xps_rbf_grouped_from_gram_f64', None if tab is None else tab.ctypes.data, n_problems, None if tiles is None else tiles.ctypes.data,
         n_tiles, ws if isinstance(ws, int) else ws.data_ptr(), ws_bytes, _dev.stream())
    torch.cuda.synchronize()


def single(G_d, n, ldg, gamma):
    """xps_rbf_from_gram_f64 on the same G with the diagonal as norms (the one-problem entry: the reference for the grouped entry's bits)."""
    torch = torch_()
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import call
    Gv = torch.as_strided(G_d, (n, n), (ldg, 1))
    sq = torch.diagonal(Gv).contiguous()
    K = torch.empty(n, n, dtype=torch.float64, device=G_d.device)
    call('xps_rbf_from_gram_f64', G_d.data_ptr(), ldg, sq.data_ptr(), sq.data_ptr(), n, n, float(gamma), K.data_ptr(), n, _dev.stream())
    torch.cuda.synchronize()
    return K.cpu().numpy()


def gram(rng, n):
    """A Gram matrix of n points in 5 dimensions in a NaN-padded (n, n + PAD) host array: distances of order 1 to 20."""
    Z = rng.standard_normal((n, 5))
    G = np.full((max(n, 1), n + PAD), np.nan)
    G[:n, :n] = Z @ Z.T
    return G


def test_one_launch_of_ragged_problems_equals_the_single_kernel_bit_for_bit():
    rng = np.random.default_rng(11)
    grams = {n: dev(gram(rng, n)) for n in NS + (0,)}
    # (n, gamma): the five sizes, two problems on one G with different gammas, gamma = 0, and an empty problem
    specs = [(1, 0.7), (63, 0.05), (64, 0.11), (65, 0.02), (130, 0.03), (65, 0.5), (130, 0.0), (0, 1.0)]
    ldk = [n + PAD for n, _ in specs]
    start = np.concatenate([[0], np.cumsum([max(n, 1) * ld + GAP for (n, _), ld in zip(specs, ldk)])])
    out = Buf64(int(start[-1]))
    tab = np.zeros((len(specs), 8), dtype=np.int64)
    for p, (n, gamma) in enumerate(specs):
        tab[p, :6] = [grams[n].data_ptr(), n + PAD, n, gbits(gamma), out.ptr + 8 * int(start[p]), ldk[p]]
    tiles = LA().rbf_tiles([n for n, _ in specs])
    assert len(tiles) == 1 + 1 + 1 + 4 + 9 + 4 + 9
    rbf_entry(tab.reshape(-1), len(specs), tiles, len(tiles))
    assert out.guards_intact(), 'a guard element was written'
    got = out.numpy((int(start[-1]),))
    written = np.zeros(len(got), dtype=bool)
    for p, (n, gamma) in enumerate(specs):
        blk = got[start[p]:start[p] + max(n, 1) * ldk[p]].reshape(max(n, 1), ldk[p])
        mask = written[start[p]:start[p] + max(n, 1) * ldk[p]].reshape(max(n, 1), ldk[p])
        mask[:n, :n] = True
        if n == 0:
            continue
        K = np.ascontiguousarray(blk[:n, :n]).view(np.float64)
        ref = single(grams[n], n, n + PAD, gamma)
        assert np.array_equal(K.view(np.int64), ref.view(np.int64)), (n, gamma)
        assert (np.diag(K) == 1.0).all()
        if gamma == 0:
            assert (K == 1.0).all()
        elif n > 1:
            assert K.min() < 0.9                                   # the map is not trivially ones
    assert (got[~written] == SENT64).all(), 'a padding column or the space between two matrices was written'
    # the result does not depend on the grid: the 130-row problem alone, its tiles in reverse order
    alone = Buf64(130 * 133)
    row = tab[4].copy()
    row[4] = alone.ptr
    rbf_entry(row, 1, np.ascontiguousarray(LA().rbf_tiles([130])[::-1]), 9)
    a = alone.numpy((130, 133))
    assert np.array_equal(a[:, :130], got[start[4]:start[4] + 130 * 133].reshape(130, 133)[:, :130]) and (a[:, 130:] == SENT64).all()


def test_the_rbf_entry_refuses_bad_tables_before_any_launch():
    from cross_patient_speech_decoding_amd._lib import XpsError
    rng = np.random.default_rng(5)
    G = dev(gram(rng, 70))
    out, empty = Buf64(70 * 73), Buf64(8)
    good = np.zeros((2, 8), dtype=np.int64)
    good[0, :6] = [G.data_ptr(), 73, 70, gbits(0.1), out.ptr, 73]
    good[1, :6] = [G.data_ptr(), 73, 0, gbits(0.1), empty.ptr, 3]
    tiles = LA().rbf_tiles([70, 0])
    assert tiles.tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1]]

    def refused(match, tab=good, n_problems=2, tl=tiles, n_tiles=None, **kw):
        with pytest.raises(XpsError, match=match):
            rbf_entry(None if tab is None else np.ascontiguousarray(tab).reshape(-1), n_problems,
                      None if tl is None else np.ascontiguousarray(tl, dtype=np.int32).reshape(-1), len(tiles) if n_tiles is None else n_tiles, **kw)

    def changed(word, value, prob=0):
        tab = good.copy()
        tab[prob, word] = value
        return tab
    refused('null table', tab=None)
    refused('null table', tl=None)
    refused('negative count', n_problems=-1)
    refused('negative count', n_tiles=-1)
    refused('negative count', tab=changed(2, -1))
    refused('ldg < n', tab=changed(1, 69))
    refused('ldk < n', tab=changed(5, 69))
    refused('null matrix', tab=changed(0, 0))
    refused('null matrix', tab=changed(4, 0))
    refused('K aliases G', tab=changed(4, G.data_ptr()))
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        refused('gamma', tab=changed(3, gbits(bad)))
    refused('gamma', tab=changed(3, gbits(-1.0), prob=1))          # (also on a problem without rows)
    refused('names no problem', tl=[[2, 0, 0]], n_tiles=1)
    refused('names no problem', tl=[[-1, 0, 0]], n_tiles=1)
    refused('names no problem', n_problems=0, tl=[[0, 0, 0]], n_tiles=1)
    refused('at or past n', tl=[[0, 2, 0]], n_tiles=1)             # 128 >= 70
    refused('at or past n', tl=[[0, 0, 2]], n_tiles=1)
    refused('at or past n', tl=[[0, -1, 0]], n_tiles=1)
    refused('at or past n', tl=[[1, 0, 0]], n_tiles=1)             # the empty problem has no tile
    refused('null workspace', ws=0, ws_bytes=1 << 20)
    refused('workspace too small', ws=torch_().empty(64, dtype=torch_().int64, device=LA().device()), ws_bytes=8)
    assert out.untouched() and empty.untouched()                   # nothing was launched
    rbf_entry(good.reshape(-1), 2, tiles, len(tiles))              # and the table itself is fine
    K = np.ascontiguousarray(out.numpy((70, 73))[:, :70]).view(np.float64)
    assert np.array_equal(K.view(np.int64), single(G, 70, 73, 0.1).view(np.int64)) and empty.untouched()
    rbf_entry(None, 0, None, 0)                                    # nothing to do: XPS_OK


def test_rbf_grouped_wrapper_shares_a_gram_and_refuses_bad_tensors(monkeypatch):
    torch, la = torch_(), LA()
    rng = np.random.default_rng(9)
    Z = rng.standard_normal((70, 4))
    big = dev(np.pad(Z @ Z.T, ((2, 3), (4, 5))))
    G = big[2:72, 4:74]                                            # a slice of a larger tensor
    K = torch.full((2, 70, 70), -77.125, dtype=torch.float64, device=la.device())
    tables = la.rbf_grouped([(G, 0.1, K[0]), (G, 0.3, K[1])])      # noqa: F841
    Gc = G.contiguous()
    for i, gamma in enumerate((0.1, 0.3)):
        assert np.array_equal(K[i].cpu().numpy().view(np.int64), single(Gc, 70, 70, gamma).view(np.int64))
    calls = []
    monkeypatch.setattr(la, 'call', lambda name, *a: calls.append(name))
    for Gb, g, Kb in ((G.cpu(), 0.1, K[0]), (G, 0.1, K[0].float()), (G, 0.1, K[0][:69]), (G[:, :69], 0.1, K[0]), (G, -1.0, K[0]),
                      (G, float('nan'), K[0]), (G.t()[::2].t(), 0.1, K[0])):
        with pytest.raises(ValueError, match='rbf_grouped'):
            la.rbf_grouped([(G, 0.1, K[1]), (Gb, g, Kb)])
    assert calls == [] and la.rbf_grouped([]) is None


# ------------------------------------------------------------------------------------------------ the variance kernel
def var_entry(tab, n_entries, out, ws=None, ws_bytes=None):
    torch = torch_()
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import call
    if ws is None:
        ws_bytes = int(lib().xps_var_grouped_f64_workspace(max(n_entries, 0)))
        ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=LA().device())
    call('xps_var_grouped_f64', None if tab is None else tab.ctypes.data, n_entries, out, ws if isinstance(ws, int) else ws.data_ptr(), ws_bytes,
         _dev.stream())
    torch.cuda.synchronize()


def fsum_var(block):
    """The float64 population variance of the exact inputs, both sums by math.fsum."""
    x = [float(v) for v in np.asarray(block, dtype=np.float64).ravel()]
    if not x:
        return 0.0
    mean = math.fsum(x) / len(x)
    return math.fsum((v - mean) ** 2 for v in x) / len(x)


def var_cases():
    """(name, host matrix with ldv = D + PAD columns (NaN padding), first row, rows, D)."""
    rng = np.random.default_rng(21)

    def padded(a):
        full = np.full((a.shape[0], a.shape[1] + PAD), np.nan, dtype=a.dtype)
        full[:, :a.shape[1]] = a
        return full
    cases = [('f32 261 x 620', padded(rng.standard_normal((261, 620)).astype(np.float32) * 3), 0, 261, 620),
             ('f64 100 x 37, first row 13', padded(rng.standard_normal((113, 37))), 13, 100, 37),
             ('f32 90 x 1030, first row 5', padded(rng.standard_normal((100, 1030)).astype(np.float32)), 5, 90, 1030),
             ('one element', padded(rng.standard_normal((3, 4))), 2, 1, 1),
             ('empty rows', padded(rng.standard_normal((3, 4))), 1, 0, 4),
             ('empty width', padded(rng.standard_normal((3, 4))), 0, 3, 0),
             ('mean 1e3, deviations 1', padded(1e3 + rng.standard_normal((200, 310))), 0, 200, 310),
             ('f32 mean 1e3, deviations 1', padded((1e3 + rng.standard_normal((64, 129))).astype(np.float32)), 1, 63, 129),
             ('one row of 1025', padded(rng.standard_normal((1, 1025))), 0, 1, 1025)]
    return cases


def test_variances_of_ragged_blocks_stay_within_the_two_pass_bound():
    torch = torch_()
    cases = var_cases()
    mats = [dev(m) for _, m, _, _, _ in cases]
    tab = np.zeros((len(cases), 8), dtype=np.int64)
    for i, ((_, m, first, rows, D), t) in enumerate(zip(cases, mats)):
        tab[i, :6] = [t.data_ptr(), int(m.dtype == np.float32), m.shape[1], first, rows, D]
    out = Buf64(len(cases))
    var_entry(tab.reshape(-1), len(cases), out.ptr)
    assert out.guards_intact()
    got = out.numpy((len(cases),)).view(np.float64)
    again = Buf64(len(cases))
    var_entry(tab.reshape(-1), len(cases), again.ptr)
    assert np.array_equal(again.numpy((len(cases),)), out.numpy((len(cases),))), 'two launches differ'
    worst = 0.0
    for (name, m, first, rows, D), g in zip(cases, got):
        ref = fsum_var(m[first:first + rows, :D])
        if rows * D <= 1:
            assert g == 0.0 and ref == 0.0, name
            continue
        bound = 8 * rows * D * 2.0 ** -53
        ratio = abs(g - ref) / (bound * ref)
        worst = max(worst, ratio)
        print(f'{name}: device {g!r} fsum {ref!r} error / bound {ratio:.4f}')
        assert ratio <= 1.0, (name, g, ref)
    print(f'largest error / bound over the cases: {worst:.4f}')
    # (the one-pass formula E[x^2] - E[x]^2 cancels six decimal digits on this case; check that it is the case it claims to be)
    name, m, first, rows, D = cases[6]
    assert abs(fsum_var(m[first:first + rows, :D]) - 1.0) < 0.05
    # the wrapper: the same numbers from tensors, slices included
    blocks = [(t[:, :D] if D else t[:, :0], first, rows) for (_, _, first, rows, D), t in zip(cases, mats)]
    var_d, tables = LA().var_grouped(blocks)                       # noqa: F841
    assert np.array_equal(var_d.cpu().numpy().view(np.int64), got.view(np.int64))
    assert LA().var_grouped([])[0].numel() == 0
    for i in (0, 1, 6):                                            # and against torch's own reduction, loosely
        _, m, first, rows, D = cases[i]
        t = mats[i][first:first + rows, :D].to(torch.float64).var(unbiased=False).item()
        assert abs(t - got[i]) <= 1e-9 * got[i]


def test_the_variance_entry_refuses_bad_tables_before_any_launch(monkeypatch):
    from cross_patient_speech_decoding_amd._lib import XpsError
    torch, la = torch_(), LA()
    V = dev(np.ones((10, 8)))
    out = Buf64(2)
    good = np.zeros((2, 8), dtype=np.int64)
    good[0, :6] = [V.data_ptr(), 0, 8, 2, 5, 6]
    good[1, :6] = [0, 0, 8, 0, 0, 6]                               # an empty entry needs no matrix

    def refused(match, tab=good, n=2, o=out.ptr, **kw):
        with pytest.raises(XpsError, match=match):
            var_entry(None if tab is None else np.ascontiguousarray(tab).reshape(-1), n, o, **kw)

    def changed(word, value, e=0):
        tab = good.copy()
        tab[e, word] = value
        return tab
    refused('null table', tab=None)
    refused('null table', o=None)
    refused('negative count', n=-1)
    for word in (3, 4, 5):
        refused('negative count', tab=changed(word, -1))
    refused('ldv < D', tab=changed(2, 5))
    refused('null matrix', tab=changed(0, 0))
    refused('v_is_f32', tab=changed(1, 2))
    refused('null workspace', ws=0, ws_bytes=1 << 20)
    refused('workspace too small', ws=torch.empty(64, dtype=torch.int64, device=la.device()), ws_bytes=8)
    assert out.untouched()
    var_entry(good.reshape(-1), 2, out.ptr)
    assert (out.numpy((2,)).view(np.float64) == 0.0).all()         # a constant block and an empty one
    var_entry(None, 0, None)                                       # nothing to do: XPS_OK
    calls = []
    monkeypatch.setattr(la, 'call', lambda name, *a: calls.append(name))
    for blk in ((V.cpu(), 0, 1), (V, 0, 11), (V, -1, 2), (V, 9, 2), (V.t()[::2].t(), 0, 1), (V.half(), 0, 1)):
        with pytest.raises(ValueError, match='var_grouped'):
            la.var_grouped([(V, 0, 10), blk])
    assert calls == []
