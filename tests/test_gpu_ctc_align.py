"""CTC forced alignment on the MI355X (csrc/xps_ctc_align.hip, realtime_sim/ctc_align.py) against the numpy restatement
of the header's contract (tests/ctc_align_ref.py): states, token spans and the path score EXACTLY equal (the recursion is
float64 additions and comparisons only), then the properties that tie it to the rest of the CTC family and the C entry
point's memory discipline and refusals."""

import numpy as np
import pytest
import torch

import ctc_ref
from ctc_align_ref import align_ref, frame_labels
from guarded_buf import SENT, Buf

pytestmark = pytest.mark.gpu


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


def _equal(al, ref, what=''):
    """CTCAlignment == align_ref's tuple, exactly (the score by bits; -inf equals -inf)."""
    states, start, end, score = ref
    assert al.states.dtype == torch.int32 and al.token_start.dtype == torch.int32 and al.score.dtype == torch.float64
    assert np.array_equal(al.states.cpu().numpy(), states), what
    assert np.array_equal(al.token_start.cpu().numpy(), start), what
    assert np.array_equal(al.token_end.cpu().numpy(), end), what
    assert np.array_equal(al.score.cpu().numpy().view(np.int64), score.view(np.int64)), what
    assert np.array_equal(al.feasible.cpu().numpy(), score > -np.inf), what


def _targets(rng, B, L, C, blank):
    labels = [c for c in range(C) if c != blank]
    return rng.choice(labels, size=(B, L)).astype(np.int64)


# the ragged batch of the issue: (T_b, L) = (1, 0), (1, 1), (3, 3) distinct, (4, 2) equal labels, (2, 2) equal: infeasible,
# (0, 0), (0, 1): infeasible
RAGGED_T = [1, 1, 3, 4, 2, 0, 0]
RAGGED_L = [0, 1, 3, 2, 2, 0, 1]


def _ragged_targets(C, blank):
    lab = [c for c in range(C) if c != blank]
    a, b, c = lab[0], lab[len(lab) // 2], lab[-1]
    assert len({a, b, c}) == 3
    pad = 99                                                # past a target's length: never read
    return np.array([[pad, pad, pad], [b, pad, pad], [c, a, b], [b, b, pad], [a, a, pad], [pad, pad, pad], [c, pad, pad]],
                    np.int64)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('blank', [0, 10])
def test_ragged_batch_equals_restatement(blank, dtype):
    rt = _rt()
    Cn = 11
    rng = np.random.default_rng(3)
    x = _log_softmax64(rng.standard_normal((7, 4, Cn)) * 2).astype(dtype)
    tg = _ragged_targets(Cn, blank)
    ref = align_ref(x, tg, RAGGED_T, RAGGED_L, blank)
    assert (ref[3] > -np.inf).tolist() == [True, True, True, True, False, True, False]
    assert 2 in ref[0][3].tolist() and ref[3][5] == 0.0      # the blank between the equal labels is on the path
    al = rt.forced_align(torch.from_numpy(x).cuda(), torch.from_numpy(tg), input_lengths=RAGGED_T, target_lengths=RAGGED_L,
                         blank=blank)
    _equal(al, ref)
    # the readouts: frame labels and spans say the same as the states
    fl = al.frame_labels().cpu().numpy()
    for b in range(7):
        want = frame_labels(ref[0][b], tg[b], blank)
        assert fl[b].tolist() == want
        spans = al.spans(b)
        if ref[3][b] == -np.inf:
            assert spans == []
        else:
            assert spans == [(int(tg[b, j]), int(ref[1][b, j]), int(ref[2][b, j])) for j in range(RAGGED_L[b])]
    # a list of sequences is the padded form
    al2 = rt.forced_align(torch.from_numpy(x).cuda(), [tg[b, :RAGGED_L[b]] for b in range(7)], input_lengths=RAGGED_T,
                          blank=blank)
    _equal(al2, align_ref(x, np.where(tg == 99, 0, tg), RAGGED_T, RAGGED_L, blank))
    # times: onset = time of the first frame, offset = time of the last
    ft = rt.window_end_times(4, 6, 4, 0.01)
    on, off = al.times(ft)
    assert on.shape == (7, 3) and on.dtype == torch.float64
    assert ref[0][2].tolist() == [1, 3, 5, -1]
    assert on[2].tolist() == ft[:3].tolist() and off[2].tolist() == ft[:3].tolist()      # one frame each
    assert bool(torch.isnan(on[4]).all()) and bool(torch.isnan(on[3, 2]))


def test_ragged_batch_two_classes():
    """C = 2: one label besides the blank, so every target repeats it and needs a blank between each pair."""
    rt = _rt()
    rng = np.random.default_rng(4)
    for blank in (0, 1):
        x = (rng.standard_normal((7, 5, 2)) * 2).astype(np.float32)
        tg = np.full((7, 3), 1 - blank, np.int64)
        Tb, L = [1, 1, 5, 4, 2, 0, 0], RAGGED_L                   # row 2: 3 equal labels in exactly the 5 frames they need
        ref = align_ref(x, tg, Tb, L, blank)
        assert ref[0][2].tolist() == [1, 2, 3, 4, 5] and ref[3][4] == -np.inf
        _equal(rt.forced_align(torch.from_numpy(x).cuda(), tg, input_lengths=Tb, target_lengths=L, blank=blank), ref)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('Cn,blank', [(2, 0), (2, 1), (11, 0), (11, 10)])
def test_more_states_than_lanes(Cn, blank, dtype):
    """T = 70, L = 33: S = 67 states, a second pass of the 64 lanes; with C = 2 the 33 equal labels need 65 frames."""
    rt = _rt()
    rng = np.random.default_rng(10 * Cn + blank)
    B, T, L = 3, 70, 33
    x = (rng.standard_normal((B, T, Cn)) * 2).astype(dtype)
    tg = _targets(rng, B, L, Cn, blank)
    Tb, Ls = [70, 70, 64], [33, 20, 33]
    ref = align_ref(x, tg, Tb, Ls, blank)
    assert ref[3][0] > -np.inf and ref[0][0].max() >= 65
    assert (ref[3][2] == -np.inf) == (Cn == 2)                    # 64 frames: one short of what 33 equal labels need
    _equal(rt.forced_align(torch.from_numpy(x).cuda(), tg, input_lengths=Tb, target_lengths=Ls, blank=blank), ref)


def test_time_major_and_permuted_view_are_read_in_place(monkeypatch):
    rt = _rt()
    from cross_patient_speech_decoding_amd.realtime_sim import ctc_align
    rng = np.random.default_rng(5)
    B, T, Cn, L = 5, 13, 7, 4
    x_tm = torch.from_numpy((rng.standard_normal((T, B, Cn)) * 2).astype(np.float32)).cuda()          # (T, B, C)
    tg = _targets(rng, B, L, Cn, 0)
    Tb, Ls = [13, 12, 7, 13, 1], [4, 3, 4, 0, 1]
    ref = align_ref(x_tm.permute(1, 0, 2).cpu().numpy(), tg, Tb, Ls, 0)
    seen = []
    real = ctc_align.call
    monkeypatch.setattr(ctc_align, 'call', lambda fn, *a: (seen.append((fn, a)), real(fn, *a))[1])
    _equal(rt.forced_align(x_tm, tg, input_lengths=Tb, target_lengths=Ls, time_major=True), ref, 'time_major')
    view = x_tm.permute(1, 0, 2)                                                                     # (B, T, C), not contiguous
    assert not view.is_contiguous()
    _equal(rt.forced_align(view, tg, input_lengths=Tb, target_lengths=Ls), ref, 'permuted view')
    wide = torch.zeros(T, B, Cn + 3, device='cuda')
    wide[:, :, :Cn] = x_tm
    _equal(rt.forced_align(wide[:, :, :Cn], tg, input_lengths=Tb, target_lengths=Ls, time_major=True), ref, 'row pitch')
    assert [fn for fn, _ in seen] == ['xps_ctc_align'] * 3
    for (_, a), src in zip(seen, (x_tm, x_tm, wide)):
        assert a[0] == src.data_ptr() and a[1] == 1, 'the scores were copied'
        assert (a[2], a[3]) == (src.stride(0), src.stride(1))
    # a host tensor goes to the device
    _equal(rt.forced_align(view.cpu(), tg, input_lengths=Tb, target_lengths=Ls), ref, 'host scores')


def test_tie_heavy_scores():
    rt = _rt()
    rng = np.random.default_rng(6)
    B, T, Cn, L = 24, 21, 4, 5
    x = np.round(rng.standard_normal((B, T, Cn))) * 0.25                 # a handful of values: most maxima are tied
    x[0] = 0.0                                                           # everything ties: the tie rule alone decides
    tg = _targets(rng, B, L, Cn, 0)
    tg[1] = 2
    Tb, Ls = rng.integers(0, T + 1, B), rng.integers(0, L + 1, B)
    Tb[:2], Ls[:2] = T, L
    for dtype in (np.float32, np.float64):
        ref = align_ref(x.astype(dtype), tg, Tb, Ls, 0)
        _equal(rt.forced_align(torch.from_numpy(x.astype(dtype)).cuda(), tg, input_lengths=Tb, target_lengths=Ls), ref)
    assert (np.diff(ref[0][0]) >= 0).all() and ref[0][0][-1] == 2 * L                                       # equal end values: the path ends in S - 1


def test_rows_with_neg_inf_log_probs():
    rt = _rt()
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
    ref = align_ref(lp, tg, Tb, None, 0)
    assert ref[3][0] == -np.inf and (ref[0][0] == -1).all()
    n_feasible = int((ref[3] > -np.inf).sum())
    assert 3 <= n_feasible < B
    if ref[3][1] > -np.inf:
        assert (ref[0][1] % 2 == 1).all()
    _equal(rt.forced_align(torch.from_numpy(lp).cuda(), tg, input_lengths=Tb), ref)
    _equal(rt.forced_align(torch.from_numpy(lp.astype(np.float32)).cuda(), tg, input_lengths=Tb),
           align_ref(lp.astype(np.float32), tg, Tb, None, 0))


def test_score_is_bounded_by_the_loss():
    """The best path is one term of the sum the loss takes the logarithm of: score <= -nll.  The alignment runs on the
    float64 log-softmax of the logits (its score is the path's log-probability to float64 rounding), the loss kernel on the
    float32 logits; the slack is the loss kernel's own bound on |nll32 - nll64| (tests/ctc_ref.py)."""
    rt = _rt()
    from cross_patient_speech_decoding_amd._lib import call
    rng = np.random.default_rng(8)
    T, B, Cn, L = 19, 9, 7, 4
    logits = (rng.standard_normal((T, B, Cn)) * 2).astype(np.float32)                  # time-major, as the loss takes them
    tg = _targets(rng, B, L, Cn, 0)
    tg[1, 1] = tg[1, 0]
    tg[3], tg[4] = [1, 1, 2, 2], [1, 2, 3, 4]                            # 5 frames for 4 + 2: infeasible; 4 frames, 4 labels: one path
    Tb, Ls = np.array([19, 19, 12, 5, 4, 19, 1, 19, 7]), np.array([4, 4, 3, 4, 4, 0, 1, 1, 2])
    nll64, _, _, parts = ctc_ref.ctc_ref(logits, tg, Tb, Ls, 0, zero_infinity=False, with_parts=True)
    bound = ctc_ref.nll_bound(parts)
    lg_d = torch.from_numpy(logits).cuda()
    tg_d, il_d, tl_d = (torch.from_numpy(np.asarray(a, np.int64)).cuda() for a in (tg, Tb, Ls))
    nbytes = int(_lib().xps_ctc_loss_f32_workspace(T, B, L))
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    nll, loss = torch.empty(B, device='cuda'), torch.empty(1, device='cuda')
    call('xps_ctc_loss_f32', lg_d.data_ptr(), tg_d.data_ptr(), L, il_d.data_ptr(), tl_d.data_ptr(), T, B, Cn, L, 0, 0,
         nll.data_ptr(), loss.data_ptr(), None, ws.data_ptr(), nbytes, _stream())
    lp = torch.from_numpy(_log_softmax64(logits)).cuda()
    al = rt.forced_align(lp, tg, input_lengths=Tb, target_lengths=Ls, time_major=True)
    score, nll = al.score.cpu().numpy(), nll.cpu().numpy().astype(np.float64)
    n_finite = 0
    for b in range(B):
        print(f'sample {b}: score {score[b]:.9g}, -nll32 {-nll[b]:.9g}, -nll64 {-nll64[b]:.9g}, bound {bound[b]:.3g}')
        if np.isinf(nll64[b]):
            assert nll[b] == np.inf and score[b] == -np.inf
        else:
            n_finite += 1
            assert score[b] <= -nll[b] + bound[b]
    assert n_finite >= 6 and n_finite < B
    assert np.isinf(nll64[3])


def test_agrees_with_greedy_where_the_target_is_the_greedy_decode():
    rt = _rt()
    rng = np.random.default_rng(9)
    B, T, Cn = 16, 40, 11
    z = rng.standard_normal((B, T, Cn)).astype(np.float32)
    z[:, :, 0] += 1.5                                                    # blanks between the tokens, as a trained model gives
    z = np.repeat(z[:, ::2], 2, axis=1) + 0.01 * rng.standard_normal((B, T, Cn)).astype(np.float32)   # runs of two frames
    lp = torch.log_softmax(torch.from_numpy(z).cuda(), dim=2)
    tokens, lengths = rt.greedy_decode_device(lp, blank=0)
    assert int(lengths.max()) <= 511 and int(lengths.min()) >= 1
    Lmax = int(lengths.max())
    al = rt.forced_align(lp, tokens[:, :Lmax].clamp(min=0), target_lengths=lengths, blank=0)
    assert bool(al.feasible.all())
    arg = lp.argmax(dim=2)
    fl = al.frame_labels()
    nonblank = fl != 0
    assert int(nonblank.sum()) >= B and bool((fl[nonblank] == arg[nonblank]).all())
    # and the greedy path itself is the best path: its score is the sum of the frame maxima
    best = lp.double().max(dim=2).values.cpu().numpy()
    total = best[:, 0].copy()
    for t in range(1, T):
        total = best[:, t] + total
    assert np.array_equal(al.score.cpu().numpy(), total)


# ---- the C entry point: guarded buffers, determinism, refusals ------------------------------------------------------------------
class _Launch:
    """states, token_start, token_end, path_score and the workspace in ONE guarded buffer of 32-bit words, gaps between."""
    GAP = 16

    def __init__(self, B, T, Lmax):
        self.B, self.T, self.Lmax = B, T, Lmax
        self.ws_bytes = int(_lib().xps_ctc_align_workspace(B, T, Lmax))
        sizes = [B * T, B * Lmax, B * Lmax, 2 * B, (self.ws_bytes + 3) // 4]
        self.off, n = [], 0
        for s in sizes:
            n += n % 2                                                   # 8-byte alignment (the score is float64)
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

    def part(self, i):
        return self.words()[self.off[i]:self.off[i] + self.sizes[i]]

    def run(self, x, tg_t, il_t, tl_t, blank_0, /, **kw):
        """One call of xps_ctc_align on tensors; a keyword replaces the argument of that name."""
        from cross_patient_speech_decoding_amd._lib import lib
        B, T, Lmax = self.B, self.T, self.Lmax
        a = dict(scores=x.data_ptr(), is_f32=int(x.dtype == torch.float32), st=x.stride(1), sb=x.stride(0), T=T, B=B,
                 C=x.size(2), Lmax=Lmax, tg=tg_t.data_ptr(), tstride=tg_t.stride(0), il=il_t.data_ptr(), tl=tl_t.data_ptr(),
                 blank=blank_0, states=self.ptr(0), t0=self.ptr(1), t1=self.ptr(2), score=self.ptr(3), ws=self.ptr(4),
                 ws_bytes=self.ws_bytes)
        a.update(kw)
        rc = lib().xps_ctc_align(a['scores'], a['is_f32'], a['st'], a['sb'], a['T'], a['B'], a['C'], a['Lmax'], a['tg'],
                                 a['tstride'], a['il'], a['tl'], a['blank'], a['states'], a['t0'], a['t1'], a['score'],
                                 a['ws'], a['ws_bytes'], _stream())
        torch.cuda.synchronize()
        return rc


def _guarded_case():
    rng = np.random.default_rng(11)
    B, T, Cn, Lmax = 6, 11, 5, 4
    x = torch.from_numpy((rng.standard_normal((B, T, Cn)) * 2).astype(np.float32)).cuda()
    tg = _targets(rng, B, Lmax + 2, Cn, 0)                               # a pitch of Lmax + 2: target_stride > max_target_len
    Tb, Ls = np.array([11, 7, 0, 3, 11, 1]), np.array([4, 2, 0, 3, 0, 4])
    ref = align_ref(x.cpu().numpy(), tg[:, :Lmax], Tb, Ls, 0)
    dev = [torch.from_numpy(np.asarray(a, np.int64)).cuda() for a in (tg, Tb, Ls)]
    return x, dev, ref, (B, T, Cn, Lmax), Tb, Ls


def test_guarded_buffers_and_determinism():
    x, (tg, il, tl), ref, (B, T, Cn, Lmax), Tb, Ls = _guarded_case()
    before = [t.clone() for t in (x.view(torch.int32), tg, il, tl)]
    runs = []
    for _ in range(2):
        la = _Launch(B, T, Lmax)
        assert la.buf.untouched()
        assert la.run(x, tg, il, tl, 0) == 0
        assert la.buf.guards_intact(), 'a guard row was written'
        w = la.words()
        assert (w[~la.live] == np.int32(SENT)).all(), 'a gap between the buffers was written'
        assert np.array_equal(la.part(0).reshape(B, T), ref[0])         # -1 from input_lengths on is part of the equality
        assert np.array_equal(la.part(1).reshape(B, Lmax), ref[1]) and np.array_equal(la.part(2).reshape(B, Lmax), ref[2])
        assert np.array_equal(la.part(3).view(np.int64), ref[3].view(np.int64))
        # the workspace: one backpointer byte per (b, t, s); cells beyond input_lengths / target_lengths, frame 0 and the
        # tail stay as they were
        Smax = 2 * Lmax + 1
        ws = la.part(4).view(np.uint8)
        sent = np.frombuffer(np.full(len(ws) // 4, SENT, np.int32).tobytes(), np.uint8)
        bp, sentinel = ws[:B * T * Smax].reshape(B, T, Smax), sent[:B * T * Smax].reshape(B, T, Smax)
        written = np.zeros((B, T, Smax), bool)
        for b in range(B):
            written[b, 1:Tb[b], :2 * Ls[b] + 1] = True
        assert np.array_equal(bp[~written], sentinel[~written]), 'a backpointer beyond a sequence\'s lengths was written'
        assert (bp[written] <= 2).all(), 'a live backpointer was not written'
        assert np.array_equal(ws[B * T * Smax:], sent[B * T * Smax:])
        runs.append(w.copy())
    assert np.array_equal(runs[0], runs[1]), 'two launches differ'
    for t, b4 in zip((x.view(torch.int32), tg, il, tl), before):
        assert torch.equal(t, b4), 'an input was written'


def test_null_lengths_mean_full_lengths():
    x, (tg, il, tl), _, (B, T, Cn, Lmax), _, _ = _guarded_case()
    la = _Launch(B, T, Lmax)
    assert la.run(x, tg, il, tl, 0, il=None, tl=None) == 0
    ref = align_ref(x.cpu().numpy(), tg.cpu().numpy()[:, :Lmax], None, None, 0)
    assert np.array_equal(la.part(0).reshape(B, T), ref[0]) and np.array_equal(la.part(3).view(np.int64), ref[3].view(np.int64))
    assert la.buf.guards_intact()


def test_out_of_range_lengths_and_labels_are_clamped():
    """Memory safety only: lengths outside 0..T / 0..Lmax act as clamped, labels outside 0..C-1 as the nearest class."""
    x, (tg, il, tl), _, (B, T, Cn, Lmax), _, _ = _guarded_case()
    il2 = torch.tensor([T + 50, -3, 2 ** 40, 3, 11, 1], device='cuda')
    tl2 = torch.tensor([Lmax + 9, 2, -(2 ** 35), 3, -1, 4], device='cuda')
    tg2 = tg.clone()
    tg2[0, 1], tg2[3, 0] = 10 ** 12, -7
    la = _Launch(B, T, Lmax)
    assert la.run(x, tg2, il2, tl2, 0) == 0
    assert la.buf.guards_intact() and (la.words()[~la.live] == np.int32(SENT)).all()
    tgc = np.clip(tg2.cpu().numpy()[:, :Lmax], 0, Cn - 1)
    ref = align_ref(x.cpu().numpy(), tgc, il2.cpu().numpy(), tl2.cpu().numpy(), 0)
    assert np.array_equal(la.part(0).reshape(B, T), ref[0]) and np.array_equal(la.part(3).view(np.int64), ref[3].view(np.int64))


REFUSALS = [
    (dict(scores=None), 'null argument'),
    (dict(states=None), 'null argument'),
    (dict(tg=None), 'null argument'),
    (dict(t0=None), 'null argument'),
    (dict(t1=None), 'null argument'),
    (dict(score=None), 'null argument'),
    (dict(ws=None), 'workspace too small'),
    (dict(ws_short=1), 'workspace too small'),
    (dict(C=0), 'needs at least one class'),
    (dict(blank=-1), 'blank outside 0..C-1'),
    (dict(blank=5), 'blank outside 0..C-1'),
    (dict(T=-1), 'negative size'),
    (dict(B=-1), 'negative size'),
    (dict(Lmax=-1), 'negative size'),
    (dict(st=-1), 'negative size'),
    (dict(Lmax=512, tstride=512), 'target longer than 511 labels'),
    (dict(tstride=3), 'target stride smaller than the longest target'),
]


@pytest.mark.parametrize('i', range(len(REFUSALS)))
def test_abi_refusals(i):
    kw, text = dict(REFUSALS[i][0]), REFUSALS[i][1]
    x, (tg, il, tl), _, (B, T, Cn, Lmax), _, _ = _guarded_case()
    la = _Launch(B, T, Lmax)
    if 'ws_short' in kw:
        kw = dict(ws_bytes=la.ws_bytes - kw['ws_short'])
    assert la.run(x, tg, il, tl, 0, **kw) == -1                          # XPS_E_INVALID
    msg = _lib().xps_last_error().decode()
    assert msg == f'xps_ctc_align: {text}', msg
    assert la.buf.untouched(), 'a refused call wrote to an output'


def test_workspace_query_and_largest_target():
    lib = _lib()
    assert lib.xps_ctc_align_workspace(3, 5, 2) >= 3 * 5 * 5
    assert lib.xps_ctc_align_workspace(0, 5, 2) >= 1 and lib.xps_ctc_align_workspace(3, 0, 2) >= 1
    # the cap itself runs: 511 labels, S = 1023 (sixteen passes of the lanes), the feasibility edge at T = 511 + repeats
    rt = _rt()
    rng = np.random.default_rng(12)
    T, L, Cn = 520, 511, 5
    x = (rng.standard_normal((2, T, Cn)) * 2).astype(np.float32)
    tg = _targets(rng, 2, L, Cn, 0)
    for i in range(1, L):
        if tg[0, i] == tg[0, i - 1]:
            tg[0, i] = 1 + tg[0, i] % (Cn - 1)
    tg[0, 1], tg[0, 3], tg[0, 5] = tg[0, 0], tg[0, 2], tg[0, 4]                    # a few repeats
    reps = int((tg[0, 1:] == tg[0, :-1]).sum())
    assert 3 <= reps and L + reps <= T
    Tb = [L + reps, L + reps - 1]
    tg[1] = tg[0]
    ref = align_ref(x, tg, Tb, None, 0)
    assert ref[3][0] > -np.inf and ref[3][1] == -np.inf
    _equal(rt.forced_align(torch.from_numpy(x).cuda(), tg, input_lengths=Tb), ref)


def test_empty_batch_and_no_frames():
    rt = _rt()
    al = rt.forced_align(torch.zeros(0, 5, 3, device='cuda'), torch.zeros(0, 2, dtype=torch.int64))
    assert al.states.shape == (0, 5) and al.score.shape == (0,)
    al = rt.forced_align(torch.zeros(2, 0, 3, device='cuda'), [[], [1]])
    assert al.score.tolist() == [0.0, -np.inf] and al.feasible.tolist() == [True, False] and al.token_start.tolist() == [[-1], [-1]]
    al = rt.forced_align(torch.ones(2, 3, 1, device='cuda'), torch.zeros(2, 0, dtype=torch.int64))    # C = 1: only the blank
    assert al.score.tolist() == [3.0, 3.0] and al.states.tolist() == [[0, 0, 0]] * 2 and al.frame_labels().tolist() == [[0] * 3] * 2


# ---- the model and the session replay ------------------------------------------------------------------------------------------
def test_model_forced_align_equals_forced_align_on_its_log_probs():
    rt = _rt()
    torch.manual_seed(0)
    win, stride, Cin, ncls = 6, 4, 4, 5
    m = rt.RealtimeRNNModel(win * Cin, 16, 1, ncls, dropout=0.0, win_size=win, stride=stride).cuda()
    m.train()
    x = torch.randn(3, 30, Cin, device='cuda')
    tg = torch.tensor([[1, 2, 0], [3, 3, 4], [2, 0, 0]])
    tl = [2, 3, 1]
    al = m.forced_align(x, tg, target_lengths=tl)
    assert m.training                                                    # the mode is put back
    assert al.states.shape == (3, m.n_windows(30)) and m.n_windows(30) == 7
    m.eval()
    with torch.no_grad():
        lp = torch.log_softmax(m.forward(x), dim=2)
    want = rt.forced_align(lp, tg, target_lengths=tl, blank=m.blank)
    for a, b in ((al.states, want.states), (al.token_start, want.token_start), (al.token_end, want.token_end),
                 (al.score, want.score)):
        assert torch.equal(a, b)
    _equal(al, align_ref(lp.cpu().numpy(), tg.numpy(), None, tl, m.blank))
    assert bool(al.feasible.all())
    on, off = al.times(rt.window_end_times(7, win, stride, 0.01))
    assert bool((on[0, :2] <= off[0, :2]).all()) and bool(torch.isnan(on[0, 2]))


def test_session_result_align_equals_forced_align():
    rt = _rt()
    rng = np.random.default_rng(13)
    N, n_pred, ncls = 4, 9, 6
    logits = torch.from_numpy(rng.standard_normal((N, n_pred, ncls)).astype(np.float32)).cuda()
    pred_lengths = torch.tensor([9, 4, 9, 2], device='cuda')
    res = rt.SessionResult(logits, None, None, pred_lengths, None, blank=5)
    tg = [[1, 2], [0], [3, 3, 4], [2, 1, 0]]
    al = res.align(tg)
    lp = torch.log_softmax(logits, dim=2)
    want = rt.forced_align(lp, tg, input_lengths=[9, 4, 9, 2], blank=5)
    assert torch.equal(al.states, want.states) and torch.equal(al.score, want.score)
    pad = np.zeros((N, 3), np.int64)
    for b, t in enumerate(tg):
        pad[b, :len(t)] = t
    _equal(al, align_ref(lp.cpu().numpy(), pad, [9, 4, 9, 2], [2, 1, 3, 3], 5))
    assert al.feasible.tolist() == [True, True, True, False]
    assert rt.SessionResult(logits, None, None, pred_lengths, None).blank == 0
