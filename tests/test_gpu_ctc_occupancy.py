"""CTC posterior occupancies on the MI355X (csrc/xps_ctc_occupancy.hip, realtime_sim/ctc_occupancy.py) against the numpy
float64 restatement of the header's contract (tests/ctc_occupancy_ref.py) within TWICE its derived bound: both are float64
evaluations of the same contract, each within one bound of the exact value.  Infinite and NaN entries are matched exactly.
Then the ties to the rest of the CTC family, the C entry point's memory discipline and refusals, and the hooks.

Largest error / (2 x bound) per family, measured (the figures of DESIGN.md 4.9d): printed by every test below."""

import numpy as np
import pytest
import torch

import ctc_ref
from ctc_align_ref import align_ref
from ctc_occupancy_ref import OUTPUTS, occupancy_ref, ratios
from guarded_buf import SENT, Buf

pytestmark = pytest.mark.gpu

SENT_PAIR = np.array([SENT, SENT], np.int32).view(np.int64)[0]


def _rt():
    from cross_patient_speech_decoding_amd import realtime_sim
    return realtime_sim


def _lib():
    from cross_patient_speech_decoding_amd._lib import lib
    return lib()


def _stream():
    from cross_patient_speech_decoding_amd._dev import stream
    return stream()


def _log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _targets(rng, B, L, C, blank):
    labels = [c for c in range(C) if c != blank]
    return rng.choice(labels, size=(B, L)).astype(np.int64)


def _host(occ):
    return {k: (None if getattr(occ, k) is None else getattr(occ, k).cpu().numpy()) for k in OUTPUTS}


def _hold(occ, ref, family):
    """Every output of a CTCOccupancy (or a dict of arrays) within twice the bound of the restatement; prints the ratios."""
    got = occ if isinstance(occ, dict) else _host(occ)
    for k, v in got.items():
        if v is not None:
            assert v.dtype == np.float64 and v.shape == ref[k].shape, (k, v.shape, ref[k].shape)
    r = ratios(got, ref, factor=2.0)
    print(f'{family}: error / (2 x bound): ' + ', '.join(f'{k} {v:.3g}' for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), (family, r)
    if not isinstance(occ, dict):
        assert np.array_equal(occ.feasible.cpu().numpy(), ref['log_z'] > -np.inf)
    return r


def _run(x, tg, Tb, Ls, blank, family, **kw):
    rt = _rt()
    ref = occupancy_ref(x, tg, Tb, Ls, blank, bounds=True)
    occ = rt.posterior_align(torch.from_numpy(np.ascontiguousarray(x)).cuda(), tg, input_lengths=Tb, target_lengths=Ls,
                             blank=blank, **kw)
    _hold(occ, ref, family)
    return occ, ref


# the ragged batch of tests/test_gpu_ctc_align.py: (T_b, L) = (1, 0), (1, 1), (3, 3) distinct, (4, 2) equal labels, (2, 2) equal:
# infeasible, (0, 0), (0, 1): infeasible
RAGGED_T = [1, 1, 3, 4, 2, 0, 0]
RAGGED_L = [0, 1, 3, 2, 2, 0, 1]


def _ragged_targets(C, blank):
    lab = [c for c in range(C) if c != blank]
    a, b, c = lab[0], lab[len(lab) // 2], lab[-1]
    pad = 99                                                # past a target's length: never read
    return np.array([[pad, pad, pad], [b, pad, pad], [c, a, b], [b, b, pad], [a, a, pad], [pad, pad, pad], [c, pad, pad]],
                    np.int64)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('blank', [0, 10])
def test_ragged_batch(blank, dtype):
    Cn = 11
    rng = np.random.default_rng(3)
    x = _log_softmax64(rng.standard_normal((7, 4, Cn)) * 2).astype(dtype)
    tg = _ragged_targets(Cn, blank)
    occ, ref = _run(x, tg, RAGGED_T, RAGGED_L, blank, f'ragged blank {blank} {np.dtype(dtype).name}')
    assert (ref['log_z'] > -np.inf).tolist() == [True, True, True, True, False, True, False]
    assert ref['log_z'][5] == 0.0 and occ.log_z[5].item() == 0.0
    got = _host(occ)
    # the edge rules, exactly: infeasible rows, frames past Tb, tokens past L
    for b in (4, 6):
        assert not got['token_occ'][b].any() and not got['onset'][b].any() and not got['class_occ'][b].any()
        assert not got['expected_frames'][b].any() and np.isnan(got['onset_mean'][b]).all()
    for b in range(7):
        assert not got['class_occ'][b, RAGGED_T[b]:].any() and not got['token_occ'][b, :, RAGGED_L[b]:].any()
        assert np.isnan(got['onset_mean'][b, RAGGED_L[b]:]).all() and not got['expected_frames'][b, RAGGED_L[b]:].any()
    # the readouts
    on_mean, on_sd = occ.onset_times(_rt().window_end_times(4, 6, 4, 0.01))
    ft = _rt().window_end_times(4, 6, 4, 0.01).numpy()
    want = (got['onset'] * ft[None, :, None]).sum(1)
    fin = ~np.isnan(got['onset_mean'])
    assert np.array_equal(np.isnan(on_mean.cpu().numpy()), ~fin) and np.array_equal(np.isnan(on_sd.cpu().numpy()), ~fin)
    assert np.allclose(on_mean.cpu().numpy()[fin], want[fin], rtol=0, atol=1e-12)
    assert on_sd[2, 0].item() <= 1e-7                                     # 3 frames, 3 distinct labels: one path
    assert np.array_equal(occ.peak().cpu().numpy(), got['token_occ'].max(1))
    assert occ.posteriorgram() is occ.class_occ


@pytest.mark.parametrize('L', [31, 32, 33, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 127, 128])
def test_states_across_waves_and_the_workgroup_width(L):
    """S = 2 L + 1.  The workgroup has round(S / 64) waves, 1 .. 4: the width changes between L = 47 | 48 (64 -> 128 lanes),
    79 | 80 (-> 192) and 111 | 112 (-> 256).  S = 63 | 65 | 67, 127 | 129, 191 | 193 and 255 | 257 cross a wave's last
    lane; 65 (64 lanes), 129 (128) and 257 (256) put one state into a second pass of the lanes."""
    rng = np.random.default_rng(100 + L)
    B, T, Cn = 3, L + 8, 7
    x = (rng.standard_normal((B, T, Cn)) * 2).astype(np.float32)
    tg = ctc_ref._targets(rng, B, L, range(1, Cn), (1,))
    _run(x, tg, [T, T, T - 3], [L, L, L - 2], 0, f'states L {L}')


def test_label_cap_at_its_feasibility_edge():
    rng = np.random.default_rng(511)
    T = L = 511
    x = (rng.standard_normal((1, T, 5)) * 2).astype(np.float32)
    tg = ctc_ref._targets(rng, 1, L, range(1, 5))
    occ, ref = _run(x, tg, [T], [L], 0, 'cap L 511 T 511')
    assert np.isfinite(ref['log_z'][0])
    assert np.allclose(occ.token_occ[0].diagonal().cpu().numpy(), 1.0, rtol=0, atol=1e-9)     # one path: token t at frame t
    occ, ref = _run(x, tg, [T - 1], [L], 0, 'cap L 511 T 510')
    assert ref['log_z'][0] == -np.inf and not bool(occ.feasible[0])


@pytest.mark.parametrize('Cn,blank', [(1, 0), (2, 0), (2, 1), (11, 0), (11, 10), (130, 0), (130, 129)])
def test_class_counts_and_blank(Cn, blank):
    rng = np.random.default_rng(300 + Cn + blank)
    B, T, L = 3, 20, (0 if Cn == 1 else 6)
    x = (rng.standard_normal((B, T, Cn)) * 2).astype(np.float32)
    tg = _targets(rng, B, L, Cn, blank) if L else np.zeros((B, 0), np.int64)
    occ, ref = _run(x, tg, [T, T - 1, T - 6], [L, L, max(L - 1, 0)], blank, f'classes C {Cn} blank {blank}')
    rows = occ.class_occ.sum(2).cpu().numpy()
    feasible = ref['log_z'] > -np.inf
    for b, Tb in enumerate([T, T - 1, T - 6]):
        if feasible[b]:
            assert np.allclose(rows[b, :Tb], 1.0, rtol=0, atol=1e-12)


def test_time_major_and_permuted_view_are_read_in_place(monkeypatch):
    rt = _rt()
    from cross_patient_speech_decoding_amd.realtime_sim import ctc_occupancy
    rng = np.random.default_rng(5)
    B, T, Cn, L = 5, 13, 7, 4
    x_tm = torch.from_numpy((rng.standard_normal((T, B, Cn)) * 2).astype(np.float32)).cuda()          # (T, B, C)
    tg = _targets(rng, B, L, Cn, 0)
    Tb, Ls = [13, 12, 7, 13, 1], [4, 3, 4, 0, 1]
    ref = occupancy_ref(x_tm.permute(1, 0, 2).cpu().numpy(), tg, Tb, Ls, 0, bounds=True)
    seen = []
    real = ctc_occupancy.call
    monkeypatch.setattr(ctc_occupancy, 'call', lambda fn, *a: (seen.append((fn, a)), real(fn, *a))[1])
    first = rt.posterior_align(x_tm, tg, input_lengths=Tb, target_lengths=Ls, time_major=True)
    _hold(first, ref, 'time_major')
    view = x_tm.permute(1, 0, 2)                                                                     # (B, T, C), not contiguous
    assert not view.is_contiguous()
    second = rt.posterior_align(view, tg, input_lengths=Tb, target_lengths=Ls)
    wide = torch.zeros(T, B, Cn + 3, device='cuda')
    wide[:, :, :Cn] = x_tm
    third = rt.posterior_align(wide[:, :, :Cn], tg, input_lengths=Tb, target_lengths=Ls, time_major=True)
    for other in (second, third):                                   # the same numbers through other strides: the same bits
        for k in OUTPUTS:
            assert np.array_equal(getattr(other, k).cpu().numpy().view(np.int64), getattr(first, k).cpu().numpy().view(np.int64)), k
    assert [fn for fn, _ in seen] == ['xps_ctc_occupancy'] * 3
    for (_, a), src in zip(seen, (x_tm, x_tm, wide)):
        assert a[0] == src.data_ptr() and a[1] == 1, 'the scores were copied'
        assert (a[2], a[3]) == (src.stride(0), src.stride(1))
    x64 = x_tm.double()
    _hold(rt.posterior_align(x64, tg, input_lengths=Tb, target_lengths=Ls, time_major=True),
          occupancy_ref(x64.permute(1, 0, 2).cpu().numpy(), tg, Tb, Ls, 0, bounds=True), 'float64 time_major')
    _hold(rt.posterior_align(view.cpu(), tg, input_lengths=Tb, target_lengths=Ls), ref, 'host scores')


def test_long_accumulation():
    rng = np.random.default_rng(1500)
    x = (rng.standard_normal((2, 1500, 11)) * 2).astype(np.float32)
    tg = ctc_ref._targets(rng, 2, 5, range(1, 11), (1,))
    _run(x, tg, [1500, 1437], [5, 4], 0, 'long T 1500')


def test_sharp_scores():
    rng = np.random.default_rng(30)
    B, T, Cn, L = 6, 25, 9, 5
    x = (rng.standard_normal((B, T, Cn)) * 30).astype(np.float32)
    tg = ctc_ref._targets(rng, B, L, range(1, Cn), (1,))
    _run(x, tg, [25, 25, 19, 25, 9, 6], [5, 5, 4, 0, 5, 5], 0, 'sharp x 30')


def test_neg_inf_entries():
    rng = np.random.default_rng(7)
    B, T, Cn, L = 12, 17, 6, 3
    p = rng.random((B, T, Cn))
    p[rng.random((B, T, Cn)) < 0.1] = 0.0                               # zero probabilities: -inf log-probabilities
    p[0, 5] = 0.0                                                        # a frame nothing can cross: infeasible
    p[1, :, 0] = 0.0                                                     # the blank is impossible: only blank-free paths
    with np.errstate(divide='ignore', invalid='ignore'):
        lp = np.log(p / np.maximum(p.sum(-1, keepdims=True), 1e-300))
    lp[0, 5] = -np.inf
    assert not np.isnan(lp).any()
    tg = _targets(rng, B, L, Cn, 0)
    tg[1] = [1, 2, 3]
    Tb = np.full(B, T)
    Tb[2] = 9
    occ, ref = _run(lp, tg, Tb, None, 0, '-inf entries float64')
    assert ref['log_z'][0] == -np.inf and 3 <= int((ref['log_z'] > -np.inf).sum()) < B
    _run(lp.astype(np.float32), tg, Tb, None, 0, '-inf entries float32')


def test_exact_case_equals_forced_align():
    """Scores 0 on one labelling and -inf elsewhere: one path holds all the mass, so g and onset are exactly the indicators
    of forced_align's states and token starts, expected_frames its span lengths and onset_mean its start frames."""
    rt = _rt()
    rng = np.random.default_rng(17)
    B, T, Cn = 6, 12, 5
    tg = np.array([[1, 2, 3], [2, 2, 1], [4, 4, 4], [1, 3, 0], [3, 0, 0], [0, 0, 0]], np.int64)
    Ls = [3, 3, 3, 2, 1, 0]
    Tb = [12, 12, 9, 12, 5, 7]
    x = np.full((B, T, Cn), -np.inf, np.float32)
    for b in range(B):
        # a random monotone state path that ends in S - 1 or S - 2 and respects the blank between equal labels
        S = 2 * Ls[b] + 1
        lab = [0] * S
        lab[1::2] = tg[b, :Ls[b]]
        while True:
            s, path = int(rng.integers(0, min(2, S))), []
            for t in range(Tb[b]):
                path.append(s)
                moves = [0] + ([1] if s + 1 < S else []) + ([2] if (s % 2 == 1 and s + 2 < S and lab[s + 2] != lab[s]) else [])
                s += int(rng.choice(moves))
            if path[-1] >= S - 2:
                break
        for t, s in enumerate(path):
            x[b, t, lab[s]] = 0.0
    xd = torch.from_numpy(x).cuda()
    al = rt.forced_align(xd, tg, input_lengths=Tb, target_lengths=Ls)
    occ = rt.posterior_align(xd, tg, input_lengths=Tb, target_lengths=Ls)
    assert bool(al.feasible.all()) and occ.log_z.tolist() == [0.0] * B
    st, t0, t1 = al.states.cpu().numpy(), al.token_start.cpu().numpy(), al.token_end.cpu().numpy()
    ref = align_ref(x, tg, Tb, Ls, 0)
    assert np.array_equal(st, ref[0]) and np.array_equal(t0, ref[1])
    j, t = np.arange(3)[None, None, :], np.arange(T)[None, :, None]
    assert np.array_equal(occ.token_occ.cpu().numpy(), (st[:, :, None] == 2 * j + 1).astype(np.float64))
    assert np.array_equal(occ.onset.cpu().numpy(), ((t0[:, None, :] == t) & (t0[:, None, :] >= 0)).astype(np.float64))
    lab_of = np.where(st % 2 == 1, np.take_along_axis(tg, np.clip(st // 2, 0, 2), 1), 0)
    assert np.array_equal(occ.class_occ.cpu().numpy(), ((lab_of[:, :, None] == np.arange(Cn)) & (st[:, :, None] >= 0)).astype(np.float64))
    assert np.array_equal(occ.expected_frames.cpu().numpy(), np.where(t0 >= 0, t1 - t0, 0).astype(np.float64))
    om = occ.onset_mean.cpu().numpy()
    assert np.array_equal(np.isnan(om), t0 < 0) and np.array_equal(om[t0 >= 0], t0[t0 >= 0].astype(np.float64))


# ---- ties to the family --------------------------------------------------------------------------------------------------------
def test_class_occ_is_the_loss_kernels_gradient_and_log_z_tops_the_best_path():
    """dlogits of xps_ctc_loss_f32 = (softmax - class_occ) / (B max(L, 1)) (tests/ctc_ref.py): the float64 occupancies give that
    gradient within the loss kernel's own grad_bound (plus twice their own bound, scaled).  On log-probabilities
    log_z <= 0, and log_z >= the best path's score: the sum over paths is at least its largest term."""
    rt = _rt()
    from cross_patient_speech_decoding_amd._lib import call
    rng = np.random.default_rng(8)
    T, B, Cn, L = 19, 9, 7, 4
    logits = (rng.standard_normal((T, B, Cn)) * 2).astype(np.float32)                  # time-major, as the loss takes them
    tg = _targets(rng, B, L, Cn, 0)
    tg[1, 1] = tg[1, 0]
    tg[3], tg[4] = [1, 1, 2, 2], [1, 2, 3, 4]                            # 5 frames for 4 + 2: infeasible; 4 frames, 4 labels: one path
    Tb, Ls = np.array([19, 19, 12, 5, 4, 19, 1, 19, 7]), np.array([4, 4, 3, 4, 4, 0, 1, 1, 2])
    nll64, _, dl64, parts = ctc_ref.ctc_ref(logits, tg, Tb, Ls, 0, zero_infinity=True, with_parts=True)
    gb = ctc_ref.grad_bound(parts)
    lg_d = torch.from_numpy(logits).cuda()
    tg_d, il_d, tl_d = (torch.from_numpy(np.asarray(a, np.int64)).cuda() for a in (tg, Tb, Ls))
    nbytes = int(_lib().xps_ctc_loss_f32_workspace(T, B, L))
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    nll, loss, dl = torch.empty(B, device='cuda'), torch.empty(1, device='cuda'), torch.empty(T, B, Cn, device='cuda')
    call('xps_ctc_loss_f32', lg_d.data_ptr(), tg_d.data_ptr(), L, il_d.data_ptr(), tl_d.data_ptr(), T, B, Cn, L, 0, 1,
         nll.data_ptr(), loss.data_ptr(), dl.data_ptr(), ws.data_ptr(), nbytes, _stream())
    occ = rt.posterior_align(lg_d, tg, input_lengths=Tb, target_lengths=Ls, time_major=True)
    ref = occupancy_ref(logits.transpose(1, 0, 2), tg, Tb, Ls, 0, bounds=True)
    cls = occ.class_occ.cpu().numpy().transpose(1, 0, 2)                                # (T, B, C)
    soft = np.exp(_log_softmax64(logits))
    gscale = 1.0 / (B * np.maximum(Ls, 1))[None, :, None]
    live = (np.arange(T)[:, None] < Tb[None, :])[:, :, None] & (ref['log_z'] > -np.inf)[None, :, None]
    mine = np.where(live, (soft - cls) * gscale, 0.0)
    slack = gb + 2 * ref['bound']['class_occ'].transpose(1, 0, 2) * gscale + 4 * 2.0 ** -53
    err = np.abs(mine - dl.cpu().numpy().astype(np.float64))
    print(f'class_occ against dlogits: largest error / slack {float((err / slack).max()):.3g}')
    assert (err <= slack).all()
    assert int((ref['log_z'] > -np.inf).sum()) >= 6 and ref['log_z'][3] == -np.inf
    lp = torch.from_numpy(_log_softmax64(logits)).cuda()
    occ = rt.posterior_align(lp, tg, input_lengths=Tb, target_lengths=Ls, time_major=True)
    al = rt.forced_align(lp, tg, input_lengths=Tb, target_lengths=Ls, time_major=True)
    lz, score = occ.log_z.cpu().numpy(), al.score.cpu().numpy()
    refp = occupancy_ref(_log_softmax64(logits).transpose(1, 0, 2), tg, Tb, Ls, 0, bounds=True)
    for b in range(B):
        print(f'sample {b}: best path {score[b]:.9g} <= log_z {lz[b]:.9g} (-nll64 {-nll64[b]:.9g})')
        if refp['log_z'][b] == -np.inf:
            assert lz[b] == -np.inf and score[b] == -np.inf
        else:
            assert lz[b] <= 0.0 and lz[b] >= score[b] - 2 * refp['bound']['log_z'][b]
            assert abs(lz[b] + nll64[b]) <= 2 * refp['bound']['log_z'][b] + 1e-12 * max(1.0, abs(lz[b]))


# ---- the C entry point: guarded buffers, determinism, NULL outputs, refusals ---------------------------------------------------
NAMES = ('log_z', 'token_occ', 'onset', 'class_occ', 'expected_frames', 'onset_mean', 'ws')


class _Launch:
    """The six outputs and the workspace in ONE guarded buffer of 32-bit words, gaps between, each 8-byte aligned."""
    GAP = 16

    def __init__(self, B, T, Lmax, C):
        self.B, self.T, self.Lmax, self.C = B, T, Lmax, C
        self.ws_bytes = int(_lib().xps_ctc_occupancy_workspace(B, T, Lmax))
        sizes = [2 * B, 2 * B * T * Lmax, 2 * B * T * Lmax, 2 * B * T * C, 2 * B * Lmax, 2 * B * Lmax, (self.ws_bytes + 3) // 4]
        self.off, n = [], 0
        for s in sizes:
            n += n % 2
            self.off.append(n)
            n += s + self.GAP
        self.sizes = sizes
        self.buf = Buf(n)
        self.live = np.zeros(n, bool)
        for o, s in zip(self.off, sizes):
            self.live[o:o + s] = True

    def ptr(self, i):
        return self.buf.ptr + 4 * self.off[i]

    def words(self):
        return self.buf.view().view(torch.int32).cpu().numpy()

    def part(self, name):
        i = NAMES.index(name)
        return self.words()[self.off[i]:self.off[i] + self.sizes[i]]

    def outputs(self):
        B, T, Lmax, C = self.B, self.T, self.Lmax, self.C
        shapes = dict(log_z=(B,), token_occ=(B, T, Lmax), onset=(B, T, Lmax), class_occ=(B, T, C), expected_frames=(B, Lmax),
                      onset_mean=(B, Lmax))
        return {k: self.part(k).view(np.float64).reshape(shapes[k]) for k in OUTPUTS}

    def run(self, x, tg_t, il_t, tl_t, blank_0, /, **kw):
        """One call of xps_ctc_occupancy on tensors; a keyword replaces the argument of that name."""
        from cross_patient_speech_decoding_amd._lib import lib
        a = dict(scores=x.data_ptr(), is_f32=int(x.dtype == torch.float32), st=x.stride(1), sb=x.stride(0), T=self.T, B=self.B,
                 C=x.size(2), Lmax=self.Lmax, tg=tg_t.data_ptr(), tstride=tg_t.stride(0), il=il_t.data_ptr(), tl=tl_t.data_ptr(),
                 blank=blank_0, ws_bytes=self.ws_bytes)
        a.update({k: self.ptr(i) for i, k in enumerate(NAMES)})
        a.update(kw)
        rc = lib().xps_ctc_occupancy(a['scores'], a['is_f32'], a['st'], a['sb'], a['T'], a['B'], a['C'], a['Lmax'], a['tg'],
                                     a['tstride'], a['il'], a['tl'], a['blank'], a['log_z'], a['token_occ'], a['onset'],
                                     a['class_occ'], a['expected_frames'], a['onset_mean'], a['ws'], a['ws_bytes'], _stream())
        torch.cuda.synchronize()
        return rc


def _guarded_case():
    rng = np.random.default_rng(11)
    B, T, Cn, Lmax = 6, 11, 5, 4
    x = torch.from_numpy((rng.standard_normal((B, T, Cn)) * 2).astype(np.float32)).cuda()
    tg = _targets(rng, B, Lmax + 2, Cn, 0)                               # a pitch of Lmax + 2: target_stride > max_target_len
    Tb, Ls = np.array([11, 7, 0, 3, 11, 1]), np.array([4, 2, 0, 3, 0, 4])
    ref = occupancy_ref(x.cpu().numpy(), tg[:, :Lmax], Tb, Ls, 0, bounds=True)
    dev = [torch.from_numpy(np.asarray(a, np.int64)).cuda() for a in (tg, Tb, Ls)]
    return x, dev, ref, (B, T, Cn, Lmax), Tb, Ls


def test_guarded_buffers_and_determinism():
    x, (tg, il, tl), ref, (B, T, Cn, Lmax), Tb, Ls = _guarded_case()
    before = [t.clone() for t in (x.view(torch.int32), tg, il, tl)]
    runs = []
    for _ in range(2):
        la = _Launch(B, T, Lmax, Cn)
        assert la.buf.untouched()
        assert la.run(x, tg, il, tl, 0) == 0
        assert la.buf.guards_intact(), 'a guard row was written'
        w = la.words()
        assert (w[~la.live] == np.int32(SENT)).all(), 'a gap between the buffers was written'
        got = la.outputs()
        for k, v in got.items():
            assert not (v.view(np.int64) == SENT_PAIR).any(), f'an element of {k} was not written'
        _hold(got, ref, 'guarded')
        # the workspace: one double per (b, t, s); cells beyond input_lengths / target_lengths and the tail stay as they were
        Smax = 2 * Lmax + 1
        ws = la.part('ws')
        ws = ws[:len(ws) // 2 * 2].view(np.int64)
        cells = ws[:B * T * Smax].reshape(B, T, Smax)
        written = np.zeros((B, T, Smax), bool)
        for b in range(B):
            written[b, :Tb[b], :2 * Ls[b] + 1] = True
        assert (cells[~written] == SENT_PAIR).all(), 'a workspace cell beyond a sequence\'s lengths was written'
        assert (cells[written] != SENT_PAIR).all(), 'a live workspace cell was not written'
        assert (ws[B * T * Smax:] == SENT_PAIR).all()
        runs.append(w.copy())
    assert np.array_equal(runs[0], runs[1]), 'two launches differ'
    for t, b4 in zip((x.view(torch.int32), tg, il, tl), before):
        assert torch.equal(t, b4), 'an input was written'


@pytest.mark.parametrize('null', ['token_occ', 'onset', 'class_occ', 'expected_frames', 'onset_mean'])
def test_null_output_is_skipped_and_the_others_keep_their_bits(null):
    x, (tg, il, tl), _, (B, T, Cn, Lmax), _, _ = _guarded_case()
    full = _Launch(B, T, Lmax, Cn)
    assert full.run(x, tg, il, tl, 0) == 0
    la = _Launch(B, T, Lmax, Cn)
    assert la.run(x, tg, il, tl, 0, **{null: None}) == 0
    assert la.buf.guards_intact() and (la.words()[~la.live] == np.int32(SENT)).all()
    for k in OUTPUTS:
        if k == null:
            assert (la.part(k) == np.int32(SENT)).all(), 'a NULL output\'s neighbourhood was written'
        else:
            assert np.array_equal(la.part(k), full.part(k)), k


def test_null_lengths_mean_full_lengths_and_out_of_range_values_are_clamped():
    x, (tg, il, tl), _, (B, T, Cn, Lmax), _, _ = _guarded_case()
    la = _Launch(B, T, Lmax, Cn)
    assert la.run(x, tg, il, tl, 0, il=None, tl=None) == 0
    _hold(la.outputs(), occupancy_ref(x.cpu().numpy(), tg.cpu().numpy()[:, :Lmax], None, None, 0, bounds=True), 'null lengths')
    assert la.buf.guards_intact()
    il2 = torch.tensor([T + 50, -3, 2 ** 40, 3, 11, 1], device='cuda')
    tl2 = torch.tensor([Lmax + 9, 2, -(2 ** 35), 3, -1, 4], device='cuda')
    tg2 = tg.clone()
    tg2[0, 1], tg2[3, 0] = 10 ** 12, -7
    la = _Launch(B, T, Lmax, Cn)
    assert la.run(x, tg2, il2, tl2, 0) == 0
    assert la.buf.guards_intact() and (la.words()[~la.live] == np.int32(SENT)).all()
    tgc = np.clip(tg2.cpu().numpy()[:, :Lmax], 0, Cn - 1)
    _hold(la.outputs(), occupancy_ref(x.cpu().numpy(), tgc, il2.cpu().numpy(), tl2.cpu().numpy(), 0, bounds=True), 'clamped')


REFUSALS = [
    (dict(scores=None), 'null argument'),
    (dict(tg=None), 'null argument'),
    (dict(log_z=None), 'null argument'),
    (dict(ws=None), 'workspace too small'),
    (dict(ws_short=1), 'workspace too small'),
    (dict(C=0), 'needs at least one class'),
    (dict(blank=-1), 'blank outside 0..C-1'),
    (dict(blank=5), 'blank outside 0..C-1'),
    (dict(T=-1), 'negative size'),
    (dict(B=-1), 'negative size'),
    (dict(Lmax=-1), 'negative size'),
    (dict(st=-1), 'negative size'),
    (dict(sb=-1), 'negative size'),
    (dict(Lmax=512, tstride=512), 'target longer than 511 labels'),
    (dict(tstride=3), 'target stride smaller than the longest target'),
    (dict(ws_shift=4), 'output or workspace not 8-byte aligned'),
    (dict(onset_shift=4), 'output or workspace not 8-byte aligned'),
    (dict(C=8181, Lmax=0), 'class bins exceed the LDS budget'),
    (dict(C=8141), 'class bins exceed the LDS budget'),
]


@pytest.mark.parametrize('i', range(len(REFUSALS)))
def test_abi_refusals(i):
    kw, text = dict(REFUSALS[i][0]), REFUSALS[i][1]
    x, (tg, il, tl), _, (B, T, Cn, Lmax), _, _ = _guarded_case()
    la = _Launch(B, T, Lmax, Cn)
    if 'ws_short' in kw:
        kw = dict(ws_bytes=la.ws_bytes - kw['ws_short'])
    if 'ws_shift' in kw:
        kw = dict(ws=la.ptr(6) + 4)
    if 'onset_shift' in kw:
        kw = dict(onset=la.ptr(2) + 4)
    assert la.run(x, tg, il, tl, 0, **kw) == -1                          # XPS_E_INVALID
    msg = _lib().xps_last_error().decode()
    assert msg == f'xps_ctc_occupancy: {text}', msg
    assert la.buf.untouched(), 'a refused call wrote to an output'


def test_lds_budget_edge_and_workspace_query():
    """Lmax = 4: 80 * 4 + 96 = 416 bytes without the bins, so C = 8140 fills the 65536-byte budget exactly and 8141 is refused;
    without class_occ no C is too large.  The launches here have no frames, so no score is read."""
    lib = _lib()
    assert lib.xps_ctc_occupancy_workspace(3, 5, 2) >= 3 * 5 * 5 * 8
    assert lib.xps_ctc_occupancy_workspace(0, 5, 2) >= 1 and lib.xps_ctc_occupancy_workspace(3, 0, 2) >= 1
    x, (tg, il, tl), ref, (B, T, Cn, Lmax), _, _ = _guarded_case()
    la = _Launch(B, T, Lmax, Cn)
    assert la.run(x, tg, il, tl, 0, C=8141, class_occ=None, scores=None, T=0) == 0      # no frames: nothing is read
    assert la.run(x, tg, il, tl, 0, C=8140, scores=None, T=0) == 0
    assert la.buf.guards_intact() and la.outputs()['log_z'].tolist() == [-np.inf, -np.inf, 0.0, -np.inf, 0.0, -np.inf]
    assert la.run(x, tg, il, tl, 0, C=8141, scores=None, T=0) == -1
    assert _lib().xps_last_error().decode() == 'xps_ctc_occupancy: class bins exceed the LDS budget'


def test_a_batch_cut_into_runs_equals_the_uncut_batch():
    rt = _rt()
    from cross_patient_speech_decoding_amd.realtime_sim import ctc_occupancy
    rng = np.random.default_rng(21)
    B, T, Cn, L = 11, 9, 6, 3
    x = torch.from_numpy((rng.standard_normal((B, T, Cn)) * 2).astype(np.float32)).cuda()
    tg = _targets(rng, B, L, Cn, 0)
    Tb, Ls = rng.integers(0, T + 1, B), rng.integers(0, L + 1, B)
    whole = rt.posterior_align(x, tg, input_lengths=Tb, target_lengths=Ls)
    per = T * (2 * L + 1) * 8
    assert ctc_occupancy.workspace_runs(B, T, L, 3 * per + 7) == [(0, 3), (3, 6), (6, 9), (9, 11)]
    cut = rt.posterior_align(x, tg, input_lengths=Tb, target_lengths=Ls, max_workspace_bytes=3 * per + 7)
    tm = rt.posterior_align(x.permute(1, 0, 2).contiguous(), tg, input_lengths=Tb, target_lengths=Ls, time_major=True,
                            max_workspace_bytes=4 * per)
    for other in (cut, tm):
        for k in OUTPUTS:
            assert np.array_equal(getattr(other, k).cpu().numpy().view(np.int64), getattr(whole, k).cpu().numpy().view(np.int64)), k
    with pytest.raises(ValueError, match='above max_workspace_bytes'):
        rt.posterior_align(x, tg, max_workspace_bytes=per - 1)
    only = rt.posterior_align(x, tg, input_lengths=Tb, target_lengths=Ls, want=('onset',))
    assert only.token_occ is None and only.class_occ is None and torch.equal(only.onset, whole.onset)
    assert torch.equal(only.log_z, whole.log_z)
    with pytest.raises(ValueError, match='token_occ was not computed'):
        only.peak()


def test_empty_batch_and_no_frames():
    rt = _rt()
    occ = rt.posterior_align(torch.zeros(0, 5, 3, device='cuda'), torch.zeros(0, 2, dtype=torch.int64))
    assert occ.token_occ.shape == (0, 5, 2) and occ.log_z.shape == (0,)
    occ = rt.posterior_align(torch.zeros(2, 0, 3, device='cuda'), [[], [1]])
    assert occ.log_z.tolist() == [0.0, -np.inf] and occ.feasible.tolist() == [True, False]
    assert bool(torch.isnan(occ.onset_mean).all()) and occ.expected_frames.tolist() == [[0.0], [0.0]]
    assert occ.peak().tolist() == [[0.0], [0.0]]
    occ = rt.posterior_align(torch.ones(2, 3, 1, device='cuda'), torch.zeros(2, 0, dtype=torch.int64))    # C = 1: only the blank
    assert occ.log_z.tolist() == [3.0, 3.0] and occ.class_occ.tolist() == [[[1.0]] * 3] * 2


# ---- the model and the session replay ------------------------------------------------------------------------------------------
def test_model_posterior_align_equals_posterior_align_on_its_log_probs():
    rt = _rt()
    torch.manual_seed(0)
    win, stride, Cin, ncls = 6, 4, 4, 5
    m = rt.RealtimeRNNModel(win * Cin, 16, 1, ncls, dropout=0.0, win_size=win, stride=stride).cuda()
    m.train()
    x = torch.randn(3, 30, Cin, device='cuda')
    tg = torch.tensor([[1, 2, 0], [3, 3, 4], [2, 0, 0]])
    tl = [2, 3, 1]
    occ = m.posterior_align(x, tg, target_lengths=tl)
    assert m.training                                                    # the mode is put back
    assert occ.token_occ.shape == (3, m.n_windows(30), 3) and m.n_windows(30) == 7
    m.eval()
    with torch.no_grad():
        lp = torch.log_softmax(m.forward(x), dim=2)
    want = rt.posterior_align(lp, tg, target_lengths=tl, blank=m.blank)
    for k in OUTPUTS:
        assert np.array_equal(getattr(occ, k).cpu().numpy().view(np.int64), getattr(want, k).cpu().numpy().view(np.int64)), k
    _hold(occ, occupancy_ref(lp.cpu().numpy(), tg.numpy(), None, tl, m.blank, bounds=True), 'model hook')
    assert bool(occ.feasible.all()) and bool((occ.log_z <= 0).all())
    mean, sd = occ.onset_times(rt.window_end_times(7, win, stride, 0.01))
    assert bool(torch.isnan(mean[0, 2])) and bool((sd[0, :2] >= 0).all())


def test_session_result_posterior_align_equals_posterior_align():
    rt = _rt()
    rng = np.random.default_rng(13)
    N, n_pred, ncls = 4, 9, 6
    logits = torch.from_numpy(rng.standard_normal((N, n_pred, ncls)).astype(np.float32)).cuda()
    pred_lengths = torch.tensor([9, 4, 9, 2], device='cuda')
    res = rt.SessionResult(logits, None, None, pred_lengths, None, blank=5)
    tg = [[1, 2], [0], [3, 3, 4], [2, 1, 0]]
    occ = res.posterior_align(tg)
    lp = torch.log_softmax(logits, dim=2)
    want = rt.posterior_align(lp, tg, input_lengths=[9, 4, 9, 2], blank=5)
    for k in OUTPUTS:
        assert np.array_equal(getattr(occ, k).cpu().numpy().view(np.int64), getattr(want, k).cpu().numpy().view(np.int64)), k
    pad = np.zeros((N, 3), np.int64)
    for b, t in enumerate(tg):
        pad[b, :len(t)] = t
    _hold(occ, occupancy_ref(lp.cpu().numpy(), pad, [9, 4, 9, 2], [2, 1, 3, 3], 5, bounds=True), 'session hook')
    assert occ.feasible.tolist() == [True, True, True, False]
