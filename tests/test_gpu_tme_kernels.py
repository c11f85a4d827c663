"""The kernels of csrc/xps_tme.hip on the MI355X through the C ABI, every output between sentinel guard rows and every matrix with a
leading dimension above its width; the frames are checked after the launches.

xps_tme_kron_pass_f64 against tests/tme_ref.py's long-double sums.  The bar of a sum of L positive terms is (L + 4) u relative: with
D exact, 1 / D carries u, its square 3 u, the L - 1 additions (L - 1) u in any order, so (L + 2) u covers every output.  The multipliers
of these cases lie on a grid of 2^-20 (small integers in one case), which makes every D = (l_A + l_B) + l_C exact in float64, as
the derivation assumes; sum log D is held to (L + 4) u sum |log D| (a log within 2 u of its value, then the additions).  Every case
asserts that its bar is below 1e-9 relative, so a dropped slab or a wrong index (1e-3 or more) cannot hide under it.  The bookkeeping
is held bit for bit: the three roles of the kernel are one code path, so a problem whose axes are rotated must give the rotated
outputs exactly; a transposition changes the order of the sums and is held to the bar.

xps_tme_core_scale_f64 to 4 u |core| (a division, a root, a product) and xps_tme_mode_product_f64 to the restatement's (K + 4) u
(|A| |B|) elementwise, in the three forms the sampling uses."""
import numpy as np
import pytest

import tme_ref as TR
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


def raw():
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import XpsError, call, lib
    return _dev, XpsError, call, lib


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


class Framed:
    """A (rows, cols) float64 device matrix inside a (rows + 2, cols + pad) buffer of sentinels: view has ld = cols + pad."""

    def __init__(self, rows, cols, pad=3, data=None):
        torch = torch_()
        self.big = torch.full((rows + 2, cols + pad), SENT64, dtype=torch.int64, device=LA().device())
        self.view = self.big.view(torch.float64)[1:rows + 1, :cols]
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float64).reshape(rows, cols)))
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


# ------------------------------------------------------------------------------------------------ the Kronecker-sum pass
class Problem:
    """One problem of the pass: its multipliers on the device and every output between guards."""

    def __init__(self, ls):
        torch, la = torch_(), LA()
        self.ls = [np.ascontiguousarray(v, dtype=np.float64) for v in ls]
        self.k = tuple(len(v) for v in self.ls)
        k0, k1, k2 = self.k
        self.l_d = [torch.from_numpy(v).to(la.device()) for v in self.ls]
        self.w1, self.w2 = [Buf64(n) for n in self.k], [Buf64(n) for n in self.k]
        self.p01, self.p02, self.p12 = Framed(k0, k1, pad=3), Framed(k0, k2, pad=1), Framed(k1, k2, pad=5)
        self.scal = Buf64(2)

    def words(self):
        la = LA()
        w = np.zeros(la.TME_KRON_WORDS, dtype=np.int64)
        w[la.KP_K0:la.KP_K0 + 3] = self.k
        for r in range(3):
            w[la.KP_L0 + r], w[la.KP_W1_0 + r], w[la.KP_W2_0 + r] = self.l_d[r].data_ptr(), self.w1[r].ptr, self.w2[r].ptr
        for word, f in ((la.KP_P01, self.p01), (la.KP_P02, self.p02), (la.KP_P12, self.p12)):
            w[word], w[word + 1] = f.view.data_ptr(), f.view.stride(0)
        w[la.KP_SCAL] = self.scal.ptr
        return w

    def results(self, check=True):
        bufs = self.w1 + self.w2 + [self.scal]
        assert all(b.guards_intact() for b in bufs) and all(f.frame_intact() for f in (self.p01, self.p02, self.p12)), \
            'an element outside an output was written'
        if check:
            assert all(bool((b.view() != SENT64).all()) for b in bufs) and all(f.written() for f in (self.p01, self.p02, self.p12)), \
                'an element of an output was never written'
        vec = lambda b: b.numpy((b.n,)).view(np.float64)                 # noqa: E731
        return dict(w1=[vec(b) for b in self.w1], w2=[vec(b) for b in self.w2], p01=self.p01.numpy(), p02=self.p02.numpy(),
                    p12=self.p12.numpy(), sumlog=vec(self.scal)[0], bad=vec(self.scal)[1])


def run_pass(list_of_ls, check=True):
    """xps_tme_kron_pass_f64 on fresh outputs -> the results of every problem."""
    _dev, _, call, lib = raw()
    torch = torch_()
    probs = [Problem(ls) for ls in list_of_ls]
    tab = np.ascontiguousarray(np.stack([p.words() for p in probs]).reshape(-1))
    nb = int(lib().xps_tme_kron_pass_f64_workspace(len(probs)))
    assert nb >= 8 * tab.size + 16 * LA().TME_MAX_AXIS * len(probs)
    ws = torch.empty(nb // 8 + 1, dtype=torch.int64, device=LA().device())
    call('xps_tme_kron_pass_f64', tab.ctypes.data, len(probs), ws.data_ptr(), nb, _dev.stream())
    torch.cuda.synchronize()
    return [p.results(check) for p in probs]


def grid_multipliers(k, seed, signed=False):
    """Multipliers on a grid of 2^-20 in [0.5, 4.5): every D is exact.  signed: the axis-1 vector is shifted below zero and the
    axis-2 vector up by as much (the same D: a gauge with negative multipliers)."""
    rng = np.random.default_rng(seed)
    ls = [0.5 + rng.integers(0, 2 ** 22, size=n) * 2.0 ** -20 for n in k]
    if signed:
        ls[1], ls[2] = ls[1] - 3.0, ls[2] + 3.0
    return ls


def same_bits(a, b):
    for key in ('p01', 'p02', 'p12'):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    for r in range(3):
        assert np.array_equal(bits(a['w1'][r]), bits(b['w1'][r])) and np.array_equal(bits(a['w2'][r]), bits(b['w2'][r])), f'axis {r}'
    assert np.array_equal(bits(a['sumlog']), bits(b['sumlog'])) and a['bad'] == b['bad']


def within_bars(got, ref, k, name, sumlog_ref=None):
    """Every output within (L + 4) u relative of the reference sums; returns the largest fraction of a bar."""
    L = TR.terms(k)
    worst = 0.0
    pieces = [(got['w1'][r], ref['w1'][r], L['w'][r], f'w1[{r}]') for r in range(3)]
    pieces += [(got['w2'][r], ref['w2'][r], L['w'][r], f'w2[{r}]') for r in range(3)]
    pieces += [(got[key], ref[key], L[key], key) for key in ('p01', 'p02', 'p12')]
    for g, want, terms, what in pieces:
        bar = (terms + 4) * U
        assert bar < 1e-9, f'{name} {what}: a bar of {bar:.2e} proves nothing'
        err = np.abs(np.asarray(g, dtype=LD) - want) / np.abs(want)
        assert (err <= bar).all(), f'{name} {what}: off by {float(err.max()):.3e} relative, bar {bar:.3e}'
        worst = max(worst, float(err.max() / bar))
    if sumlog_ref is not None:
        sumlog, abslog = sumlog_ref
        bar = (L['sumlog'] + 4) * U
        assert bar < 1e-9
        err = abs(LD(got['sumlog']) - sumlog) / abslog
        assert err <= bar, f'{name} sum log D: off by {float(err):.3e} of sum |log D|, bar {bar:.3e}'
        worst = max(worst, float(err / bar))
    return worst


@pytest.mark.parametrize('k', TR.BOXES, ids=str)
def test_the_sums_of_a_box_stay_within_the_bars_alone_signed_and_rotated(k):
    for signed in (False, True):
        ls = grid_multipliers(k, 100 + sum(k), signed)
        ref = TR.marginals(ls)
        assert not ref['bad']
        got = run_pass([ls])[0]
        assert got['bad'] == 0.0
        worst = within_bars(got, ref, k, str(k), (ref['sumlog'], ref['abslog']))
        print(f'{k} signed={signed}: largest fraction of a bar {worst:.2e}')
    # the axes rotated: the rotated outputs bit for bit (the scalar sum log D is taken in another order: its bar)
    rot = run_pass([[ls[1], ls[2], ls[0]]])[0]
    for r in range(3):
        assert np.array_equal(bits(rot['w1'][r]), bits(got['w1'][(r + 1) % 3])) and np.array_equal(bits(rot['w2'][r]), bits(got['w2'][(r + 1) % 3]))
    assert np.array_equal(bits(rot['p01']), bits(got['p12'])) and np.array_equal(bits(rot['p12']), bits(got['p02'].T))
    assert np.array_equal(bits(rot['p02']), bits(got['p01'].T))
    assert abs(LD(rot['sumlog']) - ref['sumlog']) <= (np.prod(k) + 4) * U * ref['abslog']
    # axes 1 and 2 exchanged: the exchanged outputs within the bars
    swp = run_pass([[ls[0], ls[2], ls[1]]])[0]
    ref_swp = dict(w1=[ref['w1'][0], ref['w1'][2], ref['w1'][1]], w2=[ref['w2'][0], ref['w2'][2], ref['w2'][1]], p01=ref['p02'],
                   p02=ref['p01'], p12=ref['p12'].T)
    within_bars(swp, ref_swp, (k[0], k[2], k[1]), f'{k} exchanged')


@pytest.mark.parametrize('k', [(1, 4, 4), (2, 2, 2), (5, 7, 3), (6, 3, 9)], ids=str)
def test_small_integer_multipliers_against_exact_rational_sums(k):
    rng = np.random.default_rng(7 + sum(k))
    ls = [rng.integers(1, 9, size=n).astype(np.float64) for n in k]
    exact = TR.exact_marginals(ls)
    got = run_pass([ls])[0]
    within_bars(got, exact, k, f'{k} integers')
    D = TR.box(ls)
    assert np.array_equal(D, np.round(D)) and got['bad'] == 0.0
    for perm in ((1, 2, 0), (2, 0, 1)):                                  # both rotations, bit for bit
        rot = run_pass([[ls[a] for a in perm]])[0]
        for r in range(3):
            assert np.array_equal(bits(rot['w1'][r]), bits(got['w1'][perm[r]])) and np.array_equal(bits(rot['w2'][r]), bits(got['w2'][perm[r]]))
        pair = {(0, 1): got['p01'], (0, 2): got['p02'], (1, 2): got['p12'], (1, 0): got['p01'].T, (2, 0): got['p02'].T, (2, 1): got['p12'].T}
        for key, (a, b) in (('p01', (0, 1)), ('p02', (0, 2)), ('p12', (1, 2))):
            assert np.array_equal(bits(rot[key]), bits(pair[(perm[a], perm[b])])), f'{perm} {key}'


def test_a_problem_gives_the_same_bits_alone_and_in_ragged_calls_of_two_orders():
    all_ls = [grid_multipliers(k, 200 + i) for i, k in enumerate(TR.BOXES)]
    alone = [run_pass([ls])[0] for ls in all_ls]
    for order in ([0, 1, 2, 3, 4], [3, 0, 4, 2, 1]):
        batch = run_pass([all_ls[i] for i in order])
        for res, i in zip(batch, order):
            same_bits(res, alone[i])
            within_bars(res, TR.marginals(all_ls[i]), TR.BOXES[i], f'ragged {TR.BOXES[i]}')


def test_a_box_with_a_nonpositive_d_is_flagged_and_leaves_its_neighbours_alone():
    good = [grid_multipliers(k, 300 + i) for i, k in enumerate([(5, 7, 3), (2, 2, 2)])]
    bad = grid_multipliers((4, 6, 5), 310)
    bad[1][2] = -bad[0][3] - bad[2][1]                                   # D = 0 at (3, 2, 1)
    bad[1][4] = -20.0                                                    # D < 0 in every slab
    res = run_pass([good[0], bad, good[1]], check=False)
    assert res[1]['bad'] == 4.0 and res[0]['bad'] == 0.0 and res[2]['bad'] == 0.0
    assert TR.marginals(bad)['bad']
    for got, ls in ((res[0], good[0]), (res[2], good[1])):
        same_bits(got, run_pass([ls])[0])
        assert all(np.isfinite(v).all() for v in got['w1'] + got['w2'] + [got['p01'], got['p02'], got['p12'], got['sumlog']])
    one = grid_multipliers((3, 3, 3), 311)
    one[2][0] = -one[0][1] - one[1][1] - 1.0                              # D = -1 at (1, 1, 0)
    flagged = run_pass([one], check=False)[0]['bad']
    assert flagged == float((~(TR.box(one) > 0)).any(axis=(1, 2)).sum()) >= 1.0
    nan = grid_multipliers((3, 3, 3), 312)
    nan[0][2] = np.nan
    assert run_pass([nan], check=False)[0]['bad'] == 1.0


def test_the_wrapper_builds_the_same_call():
    la, torch = LA(), torch_()
    ls = grid_multipliers((5, 7, 3), 400)
    want = run_pass([ls])[0]
    dev = la.device()
    l_d = [torch.from_numpy(v).to(dev) for v in ls]
    new = lambda *s: torch.empty(*s, dtype=torch.float64, device=dev)    # noqa: E731
    pr = dict(l=l_d, w1=[new(5), new(7), new(3)], w2=[new(5), new(7), new(3)], p01=new(5, 7), p02=new(5, 3), p12=new(7, 3), scal=new(2))
    keep = la.tme_kron_pass([pr])
    torch.cuda.synchronize()
    got = dict(w1=[v.cpu().numpy() for v in pr['w1']], w2=[v.cpu().numpy() for v in pr['w2']], p01=pr['p01'].cpu().numpy(),
               p02=pr['p02'].cpu().numpy(), p12=pr['p12'].cpu().numpy(), sumlog=pr['scal'].cpu().numpy()[0], bad=pr['scal'].cpu().numpy()[1])
    same_bits(got, want)
    assert keep is not None


# ------------------------------------------------------------------------------------------------ core scale, mode products
def framed4(S, k0, k1, k2, pad, data=None):
    f = Framed(S * k0 * k1, k2, pad=pad, data=data)
    return f, f.view.unflatten(0, (S, k0, k1))


@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('k', TR.BOXES, ids=str)
def test_core_scale_and_the_middle_mode_product_stay_within_the_elementwise_bars(k, S):
    la, torch = LA(), torch_()
    k0, k1, k2 = k
    n1, n2 = k1 + 1, k2 + 2
    rng = np.random.default_rng(500 + sum(k) + S)
    ls = grid_multipliers(k, 501, signed=True)
    z = rng.standard_normal((S,) + k)
    fz, z4 = framed4(S, k0, k1, k2, 3, z)
    fc, c4 = framed4(S, k0, k1, k2, 2)
    l_d = [torch.from_numpy(np.ascontiguousarray(v)).to(la.device()) for v in ls]
    la.tme_core_scale(z4, l_d, out=c4)
    torch.cuda.synchronize()
    assert fz.frame_intact() and fc.frame_intact() and fc.written() and np.array_equal(bits(fz.numpy()), bits(z.reshape(-1, k2)))
    core = fc.numpy().reshape((S,) + k)
    ref = TR.core_of(z, ls)
    assert (np.abs(core.astype(LD) - ref) <= 4 * U * np.abs(ref)).all(), 'core scale'
    again = la.tme_core_scale(torch.from_numpy(z).to(la.device()), l_d)  # contiguous, a new output: the same bits
    assert np.array_equal(bits(again.cpu().numpy()), bits(core))

    # the middle product: Q_1 (n1 x k1: the leading columns of an n1 x n1 matrix) times each of the S k0 slices (k1 x n2)
    Q = np.linalg.qr(rng.standard_normal((n1, n1)))[0]
    T = rng.standard_normal((S * k0, k1, n2))
    fq = Framed(n1, n1, pad=1, data=Q)
    ft = Framed(S * k0 * k1, n2, pad=3, data=T)
    fo = Framed(S * k0 * n1, n2, pad=4)
    out = fo.view.unflatten(0, (S * k0, n1))
    la.tme_mode_product(fq.view[:, :k1], ft.view.unflatten(0, (S * k0, k1)), out)
    torch.cuda.synchronize()
    assert fq.frame_intact() and ft.frame_intact() and fo.frame_intact() and fo.written()
    got = fo.numpy().reshape(S * k0, n1, n2)
    want = np.einsum('mk,bkn->bmn', Q[:, :k1].astype(LD), T.astype(LD))
    bar = (k1 + 4) * U * np.einsum('mk,bkn->bmn', np.abs(Q[:, :k1]), np.abs(T))
    assert bar.max() < 1e-9 and (np.abs(got.astype(LD) - want) <= bar).all(), 'middle mode product'
    if S == 3:                                                           # a member's bits do not depend on the batch around it
        one = torch.empty(1, n1, n2, dtype=torch.float64, device=la.device())
        la.tme_mode_product(fq.view[:, :k1], ft.view.unflatten(0, (S * k0, k1))[k0:k0 + 1], one)
        assert np.array_equal(bits(one.cpu().numpy()[0]), bits(got[k0]))


def test_the_first_and_last_mode_products_transposed_operand_added_mean_and_float32_store():
    la, torch = LA(), torch_()
    rng = np.random.default_rng(600)
    dev = la.device()
    R, k2, n2 = 131, 33, 35                                              # rows (s, i, j) times Q_2^T, Q_2 stored (n2, k2 of n2)
    A, Q = rng.standard_normal((R, k2)), np.linalg.qr(rng.standard_normal((n2, n2)))[0]
    fa, fq, fo = Framed(R, k2, pad=2, data=A), Framed(n2, n2, pad=1, data=Q), Framed(R, n2, pad=3)
    la.tme_mode_product(fa.view, fq.view[:, :k2], fo.view.unsqueeze(0), b_kcontig=True)
    torch.cuda.synchronize()
    want = A.astype(LD) @ Q[:, :k2].astype(LD).T
    bar = (k2 + 4) * U * (np.abs(A) @ np.abs(Q[:, :k2]).T)
    assert fo.frame_intact() and fo.written() and (np.abs(fo.numpy().astype(LD) - want) <= bar).all()
    S, k0, n0, N = 3, 9, 10, 70                                          # Q_0 times each surrogate's (k0, n1 n2) matrix, plus the mean
    Q0, T, M = np.linalg.qr(rng.standard_normal((n0, n0)))[0], rng.standard_normal((S, k0, N)), rng.standard_normal((n0, N))
    fq0, ft, fm = Framed(n0, n0, pad=1, data=Q0), Framed(S * k0, N, pad=2, data=T), Framed(n0, N, pad=5, data=M)
    want = np.einsum('mk,bkn->bmn', Q0[:, :k0].astype(LD), T.astype(LD)) + M.astype(LD)
    bar = (k0 + 4) * U * np.einsum('mk,bkn->bmn', np.abs(Q0[:, :k0]), np.abs(T)) + U * np.abs(want)
    fo64 = Framed(S * n0, N, pad=3)
    la.tme_mode_product(fq0.view[:, :k0], ft.view.unflatten(0, (S, k0)), fo64.view.unflatten(0, (S, n0)), add=fm.view)
    out32 = torch.full((S, n0 + 1, N + 3), float('nan'), dtype=torch.float32, device=dev)
    la.tme_mode_product(fq0.view[:, :k0], ft.view.unflatten(0, (S, k0)), out32[:, :n0, :N], add=fm.view)
    torch.cuda.synchronize()
    got = fo64.numpy().reshape(S, n0, N)
    assert fo64.frame_intact() and fo64.written() and fm.frame_intact() and (np.abs(got.astype(LD) - want) <= bar).all()
    h32 = out32.cpu().numpy()
    assert np.isnan(h32[:, n0:, :]).all() and np.isnan(h32[:, :, N:]).all()
    assert np.array_equal(h32[:, :n0, :N], got.astype(np.float32))       # the float64 value, rounded once


# ------------------------------------------------------------------------------------------------ refusals
def test_the_entries_refuse_bad_arguments_before_any_launch():
    _dev, XpsError, call, lib = raw()
    la, torch = LA(), torch_()
    p = Problem(grid_multipliers((3, 4, 2), 700))
    good = p.words()
    ws = torch.empty(3000, dtype=torch.int64, device=la.device())
    w, st, nb = ws.data_ptr(), _dev.stream(), 8 * 3000

    def refused(match, name, *args):
        with pytest.raises(XpsError, match=match):
            call(name, *args, st)

    def edited(**edit):
        t = good.copy()
        for key, v in edit.items():
            t[getattr(la, key)] = v
        return np.ascontiguousarray(t)
    for edit, match in ((dict(KP_K0=0), 'a box size outside'), (dict(KP_K2=la.TME_MAX_AXIS + 1), 'a box size outside'),
                        (dict(KP_K1=-4), 'a box size outside'), (dict(KP_L1=0), 'null multipliers'), (dict(KP_W1_2=0), 'null marginal'),
                        (dict(KP_W2_0=0), 'null marginal'), (dict(KP_P01=0), 'null marginal'), (dict(KP_P02=0), 'null marginal'),
                        (dict(KP_P12=0), 'null marginal'), (dict(KP_SCAL=0), 'null scalars'), (dict(KP_LD01=3), 'ld01 < k1'),
                        (dict(KP_LD02=1), 'ld02 < k2'), (dict(KP_LD12=1), 'ld12 < k2')):
        t = edited(**edit)
        refused(match, 'xps_tme_kron_pass_f64', t.ctypes.data, 1, w, nb)
    t = edited()
    refused('null table', 'xps_tme_kron_pass_f64', None, 1, w, nb)
    refused('negative count', 'xps_tme_kron_pass_f64', t.ctypes.data, -1, w, nb)
    refused('65535', 'xps_tme_kron_pass_f64', t.ctypes.data, 65536, w, nb)
    refused('null workspace', 'xps_tme_kron_pass_f64', t.ctypes.data, 1, None, nb)
    need = int(lib().xps_tme_kron_pass_f64_workspace(1))
    assert need == 8 * la.TME_KRON_WORDS + 16 * la.TME_MAX_AXIS and lib().xps_tme_kron_pass_f64_workspace(-1) == 0
    refused('workspace too small', 'xps_tme_kron_pass_f64', t.ctypes.data, 1, w, need - 8)

    z, c = Framed(3 * 4, 2, pad=1), Framed(3 * 4, 2, pad=1)
    l = [v.data_ptr() for v in p.l_d]
    zp, cp = z.view.data_ptr(), c.view.data_ptr()
    for args, match in (((None, 3, *l, 3, 4, 2, 1, cp, 3), 'null tensor'), ((zp, 3, *l, 3, 4, 2, 1, None, 3), 'null tensor'),
                        ((zp, 3, None, l[1], l[2], 3, 4, 2, 1, cp, 3), 'null multipliers'), ((zp, 1, *l, 3, 4, 2, 1, cp, 3), 'ldz < k2'),
                        ((zp, 3, *l, 3, 4, 2, 1, cp, 1), 'ldc < k2'), ((zp, 3, *l, 3, 4, 2, -1, cp, 3), 'negative count'),
                        ((zp, 3, *l, 0, 4, 2, 1, cp, 3), 'a box size outside'), ((zp, 3, *l, 3, 4, 1025, 1, cp, 3), 'a box size outside'),
                        ((zp, 3, *l, 3, 4, 2, 2 ** 20 + 1, cp, 3), 'more than 2\\^20 surrogates')):
        refused(match, 'xps_tme_core_scale_f64', *args)

    A, B, Cm = Framed(4, 3), Framed(3, 5), Framed(8, 5)
    ap, bp, cq = A.view.data_ptr(), B.view.data_ptr(), Cm.view.data_ptr()
    lda, ldb, ldc = A.view.stride(0), B.view.stride(0), Cm.view.stride(0)

    def product(match, A=ap, lda=lda, sa=0, B=bp, ldb=ldb, sb=0, bk=0, add=None, ldadd=0, C=cq, f32=0, ldc=ldc, sc=4 * ldc, M=4, N=5, K=3,
                batch=2):
        refused(match, 'xps_tme_mode_product_f64', A, lda, sa, B, ldb, sb, bk, add, ldadd, C, f32, ldc, sc, M, N, K, batch)
    product('null matrix', A=None)
    product('null matrix', B=None)
    product('null matrix', C=None)
    product('negative size', M=-1)
    product('negative size', batch=-1)
    product('negative size', K=0)
    product('lda < K', lda=2)
    product('ldb below the width of B', ldb=4)
    product('ldb below the width of B', bk=1, ldb=2)
    product('ldc < N', ldc=4)
    product('ldadd < N', add=cq, ldadd=4)
    product('negative batch stride', sa=-1)
    product('negative batch stride', sb=-8)
    product('the outputs of two batch members overlap', sc=3 * ldc + 4)
    product('b_kcontig must be 0 or 1', bk=2)
    product('c_is_f32 must be 0 or 1', f32=2)
    product('more than 2\\^31 - 1 tiles', M=2 ** 30, batch=2 ** 20, sc=2 ** 40)
    torch.cuda.synchronize()
    assert z.untouched() and c.untouched() and A.untouched() and B.untouched() and Cm.untouched()
    assert all(b.untouched() for b in p.w1 + p.w2 + [p.scal]) and p.p01.untouched() and p.p02.untouched() and p.p12.untouched()
