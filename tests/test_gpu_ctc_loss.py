"""xps_ctc_loss_f32 (csrc/xps_ctc.hip) called through the C ABI and held to the float64 reference and the float32 error bounds
of tests/ctc_ref.py over the grid of ctc_ref.grid(): more than one pass of the 64 lanes over the states, the time steps and the
classes, blank != 0, both zero_infinity values, the feasibility edge, empty and clamped lengths, a strided target buffer
with poisoned padding, the logit range, B beyond the 256 threads of the mean kernel, dlogits == NULL, the 511-label limit.
Then the Python layer (XF.ctc_loss, _HipCTCLoss, RealtimeRNNModel._ctc) against the same reference.

Every launch follows one protocol (_launch): nll, loss and dlogits are pre-filled with a sentinel and have a sentinel guard
behind them; the workspace is exactly xps_ctc_loss_f32_workspace bytes of NaN with a guard behind it; afterwards every
element of dlogits has been written, the guards are intact, the read-only inputs keep their bits, and a second launch into the
NaN-refilled workspace gives the same bits.

Out of scope, as in include/xps.h: -inf logits (torch's own gradient is NaN there), labels outside 0..C-1 in live positions
(the caller's contract), and the gradient rows of an infinite-loss sample under zero_infinity = 0 (unspecified, NaN in
torch): those rows must be written, nothing more."""
import functools

import numpy as np
import pytest
import torch

import ctc_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = 0x7FC0DEAD                    # a quiet-NaN bit pattern no kernel produces
QNAN = 0x7FC00000
GUARD = 64                           # elements behind each output, 256 bytes behind the workspace


def _call(name, *args):
    from cross_patient_speech_decoding_amd._lib import call
    call(name, *args)


def _xps_error():
    from cross_patient_speech_decoding_amd._lib import XpsError
    return XpsError


def _stream():
    from cross_patient_speech_decoding_amd._dev import stream
    return stream()


def _workspace_bytes(T, B, Lmax):
    from cross_patient_speech_decoding_amd._lib import lib
    return int(lib().xps_ctc_loss_f32_workspace(T, B, Lmax))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sentinel(n):
    return torch.full((n + GUARD,), SENT, dtype=torch.int32, device='cuda')


@functools.lru_cache(maxsize=None)
def _cases():
    return {c['name']: c for c in R.grid()}


@functools.lru_cache(maxsize=None)
def _ref(name, zi):
    """The float64 reference of a grid case with its bounds, computed once and shared: (nll, loss, dlogits, parts)."""
    c = _cases()[name]
    return R.ctc_ref(c['logits'], c['targets'], c['in_len'], c['tg_len'], c['blank'], zi, with_parts=True)


class Out:
    def __init__(self, nll, loss, dl, shape):
        self.nll_bits, self.loss_bits, self.dl_bits = nll, loss, dl
        self.nll = nll.view(torch.float32).cpu().numpy()
        self.loss = float(loss.view(torch.float32).cpu().numpy()[0])
        self.dl = None if dl is None else dl.view(torch.float32).cpu().numpy().reshape(shape)

    def tuple(self):
        return self.nll, self.loss, self.dl


def _launch(logits, targets, in_len, tg_len, blank, zi, *, stride=None, pad=0, want_grad=True, unspecified=()):
    """One protocol launch pair.  targets (B, Lmax) -> a device buffer of row stride `stride` whose cells past each target
    length (and the stride padding) hold `pad` when pad != 0.  `unspecified`: samples whose gradient rows need not be finite.
    Returns Out (bits and host copies of the live parts)."""
    T, B, C = logits.shape
    Lmax = targets.shape[1]
    stride = max(Lmax, 1) if stride is None else stride
    tg = np.full((B, stride), pad, np.int64)
    tg[:, :targets.shape[1]] = targets
    if pad:
        _, Ls = R.clamp_lengths(T, targets.shape[1], in_len, tg_len)
        for b in range(B):
            tg[b, Ls[b]:] = pad
    lg_d, tg_d, il_d, tl_d = _dev(logits.astype(F32)), _dev(tg), _dev(np.asarray(in_len, np.int64)), _dev(
        np.asarray(tg_len, np.int64))
    before = [t.clone() for t in (lg_d.view(torch.int32), tg_d, il_d, tl_d)]
    nbytes = _workspace_bytes(T, B, Lmax)
    assert nbytes % 4 == 0
    ws = torch.empty(nbytes // 4 + GUARD, dtype=torch.int32, device='cuda')
    runs = []
    for _ in range(2):
        ws[:nbytes // 4] = QNAN
        ws[nbytes // 4:] = SENT
        nll, loss, dl = _sentinel(B), _sentinel(1), (_sentinel(T * B * C) if want_grad else None)
        _call('xps_ctc_loss_f32', lg_d.data_ptr(), tg_d.data_ptr(), stride, il_d.data_ptr(), tl_d.data_ptr(), T, B, C, Lmax,
              blank, int(zi), nll.data_ptr(), loss.data_ptr(), None if dl is None else dl.data_ptr(), ws.data_ptr(),
              nbytes, _stream())
        torch.cuda.synchronize()
        assert bool((nll[B:] == SENT).all()) and bool((loss[1:] == SENT).all()), 'a guard behind nll / loss was written'
        assert bool((ws[nbytes // 4:] == SENT).all()), 'the kernel wrote past the bytes the workspace function returned'
        assert bool((nll[:B] != SENT).all()) and int(loss[0]) != SENT, 'nll / loss was not written'
        if dl is not None:
            assert bool((dl[T * B * C:] == SENT).all()), 'the guard behind dlogits was written'
            assert bool((dl[:T * B * C] != SENT).all()), 'an element of dlogits was not written'
        runs.append((nll[:B].clone(), loss[:1].clone(), None if dl is None else dl[:T * B * C].clone()))
    for a, b in zip(*runs):
        assert a is None or torch.equal(a, b), 'two launches differ'
    for t, b in zip((lg_d.view(torch.int32), tg_d, il_d, tl_d), before):
        assert torch.equal(t, b), 'a read-only input changed'
    out = Out(*runs[0], (T, B, C))
    if out.dl is not None:
        live = [b for b in range(B) if b not in unspecified]
        assert np.isfinite(out.dl[:, live]).all(), 'a gradient element is not finite'
    return out


def _launch_case(c, zi, **kw):
    nll = _ref(c['name'], zi)[0]
    return _launch(c['logits'], c['targets'], c['in_len'], c['tg_len'], c['blank'], zi,
                   unspecified=tuple(np.flatnonzero(~np.isfinite(nll))), **kw)


def _row_sum_ratio(dl, ref):
    """max over the rows of |sum_c dlogits[t, b, :]| / sum_c bound: softmax and occupancy both sum to one."""
    spec = ~np.isnan(ref[2]).any(2)
    s = np.abs(np.where(spec[..., None], dl.astype(np.float64), 0.0).sum(2))
    b = R.grad_bound(ref[3]).sum(2) + 1e-300
    return float((s / b)[spec].max())


# ---- the grid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in R.grid()])
def test_grid_vs_fp64(name):
    c = _cases()[name]
    for zi in c['zi']:
        ref = _ref(name, zi)
        out = _launch_case(c, zi)
        r_nll, r_loss, r_dl = R.error_ratios(out.tuple(), ref)
        r_sum = _row_sum_ratio(out.dl, ref)
        print(f'xps_ctc_loss_f32 {name} zero_infinity={zi}: error / bound nll {r_nll:.4f}, loss {r_loss:.4f}, '
              f'gradient {r_dl:.4f}, row sums {r_sum:.4f}')
        assert r_nll <= 1 and r_loss <= 1 and r_dl <= 1 and r_sum <= 1
        Tb, _ = R.clamp_lengths(c['logits'].shape[0], c['targets'].shape[1], c['in_len'], c['tg_len'])
        for b, tb in enumerate(Tb):
            assert not out.dl[tb:, b].any(), 'a row beyond the input length is not zero'
        dead = ~np.isfinite(ref[0])
        if zi:
            assert not dead.any()
        elif dead.any():
            assert (out.nll[dead] == np.inf).all() and out.loss == np.inf
        # dlogits == NULL: the early return leaves nll and loss as they are
        bare = _launch_case(c, zi, want_grad=False)
        assert torch.equal(bare.nll_bits, out.nll_bits) and torch.equal(bare.loss_bits, out.loss_bits)


# ---- the envelope's refusals: argument checks that return before any launch ----------------------------------------------------
def _refused(code, **kw):
    T, B, C = 6, 2, 5
    rng = np.random.default_rng(1)
    Lmax = kw.pop('Lmax', 3)
    lg_d, tg_d = _dev(rng.standard_normal((T, B, C)).astype(F32)), _dev(np.ones((B, max(Lmax, 1)), np.int64))
    il_d, tl_d = _dev(np.full(B, T, np.int64)), _dev(np.full(B, 2, np.int64))
    nbytes = _workspace_bytes(T, B, Lmax)
    ws = torch.full((nbytes // 4 + GUARD,), SENT, dtype=torch.int32, device='cuda')
    nll, loss, dl = _sentinel(B), _sentinel(1), _sentinel(T * B * C)
    with pytest.raises(_xps_error(), match=rf'code {code}\)'):
        _call('xps_ctc_loss_f32', lg_d.data_ptr(), tg_d.data_ptr(), max(Lmax, 1), il_d.data_ptr(), tl_d.data_ptr(), T, B, C,
              Lmax, 0, 1, nll.data_ptr(), loss.data_ptr(), dl.data_ptr(), ws.data_ptr(), nbytes - kw.get('ws_short', 0),
              _stream())
    torch.cuda.synchronize()
    for t in (nll, loss, dl, ws):
        assert bool((t == SENT).all()), 'a refused call wrote to an output'


def test_512_labels_are_refused_before_any_launch():
    _refused(-1, Lmax=512)                  # XPS_E_INVALID


def test_workspace_one_byte_short_is_refused():
    _refused(-3, ws_short=1)                # XPS_E_WORKSPACE


# ---- empty input with empty target ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('zi', [0, 1])
def test_empty_input_with_empty_target_is_zero(zi):
    """input_length 0 (and below) with target_length 0: the empty alignment, nll = 0 whatever zero_infinity is, as in torch;
    the loss stays finite."""
    rng = np.random.default_rng(2)
    T, B, C = 5, 3, 4
    logits = rng.standard_normal((T, B, C))
    targets = np.asarray([[1, 2], [3, 1], [2, 2]])
    out = _launch(logits, targets, [0, T, -2], [0, 2, 0], 0, zi)
    assert out.nll[0] == 0 and out.nll[2] == 0 and np.isfinite(out.loss)
    assert not out.dl[:, 0].any() and not out.dl[:, 2].any()
    ref = R.ctc_ref(logits.astype(F32), targets, [0, T, -2], [0, 2, 0], 0, zi, with_parts=True)
    assert max(R.error_ratios(out.tuple(), ref)) <= 1


# ---- feasibility edge: the other samples do not see the dead one --------------------------------------------------------------
@pytest.mark.parametrize('i', range(4))
def test_dead_sample_leaves_the_others_alone(i):
    """zero_infinity = 0 and sample 0 one frame short of its only alignment: nll[0] = loss = +inf, and samples 1 and 2 have the
    bits they have when sample 0 is alive (same B) and, up to the factor B in the gradient's scale, when it is not in the
    batch at all.  Sample 0's own gradient rows are unspecified (NaN in torch)."""
    short, exact = _cases()[f'feasible_{i}_short'], _cases()[f'feasible_{i}_exact']
    dead = _launch_case(short, 0)
    alive = _launch_case(exact, 0)
    assert dead.nll[0] == np.inf and dead.loss == np.inf and np.isfinite(alive.nll).all()
    assert torch.equal(dead.nll_bits[1:], alive.nll_bits[1:])
    T, B, C = short['logits'].shape
    assert np.array_equal(dead.dl[:, 1:].view(np.int32), alive.dl[:, 1:].view(np.int32))
    two = _launch(short['logits'][:, 1:], short['targets'][1:], short['in_len'][1:], short['tg_len'][1:], 0, 0)
    assert torch.equal(two.nll_bits, dead.nll_bits[1:])
    a, b = 3.0 * dead.dl[:, 1:].astype(np.float64), 2.0 * two.dl.astype(np.float64)       # 1 / (B L) is rounded: 4 u
    assert (np.abs(a - b) <= 4 * R.U * np.abs(b)).all()


# ---- target stride and padding ------------------------------------------------------------------------------------------------
def test_padding_and_stride_are_never_read():
    c = _cases()['stride']
    clean = _launch_case(c, 1)
    Lmax, C = c['targets'].shape[1], c['logits'].shape[2]
    for pad in (-1, C + 9, 2 ** 40):
        got = _launch_case(c, 1, stride=Lmax + 5, pad=pad)
        assert torch.equal(got.nll_bits, clean.nll_bits) and torch.equal(got.loss_bits, clean.loss_bits)
        assert torch.equal(got.dl_bits, clean.dl_bits)


# ---- shift invariance ---------------------------------------------------------------------------------------------------------
def test_shift_by_1e4_gives_the_base_values():
    """range_shift is range_base + 1e4 exactly (the base sits on a 2^-10 grid), so the float64 values are the same; the
    float32 bound at 1e4 is wider (u |lse| per row) and is the one that applies."""
    base, shift = _cases()['range_base'], _cases()['range_shift']
    assert np.array_equal(shift['logits'].astype(np.float64), base['logits'].astype(np.float64) + 1e4)
    out = _launch_case(shift, 1)
    nll, loss, dl, _ = _ref('range_base', 1)
    ratios = R.error_ratios(out.tuple(), (nll, loss, dl, _ref('range_shift', 1)[3]))
    print(f'shift invariance: error / bound {ratios}')
    assert max(ratios) <= 1


# ---- batch: the mean kernel and independence ------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 256, 257, 300])
def test_loss_is_the_fp64_mean_of_the_device_nll(B):
    """ctc_mean_kernel accumulates nll_b / max(L_b, 1) in float64 (strided beyond 256 samples) and rounds once."""
    c = _cases()[f'batch_B{B}']
    out = _launch_case(c, 1)
    mean = float(np.mean(out.nll.astype(np.float64) / np.maximum(c['tg_len'], 1)))
    assert abs(out.loss - mean) <= R.U * abs(mean) * (1 + 1e-6)
    assert B == 1 or ((c['tg_len'] == 0).any() and (c['tg_len'] == 2).any())


def test_oversized_target_length_is_clamped_in_the_divisor_too():
    """A target length above max_target_len is clamped in the recursion and in the loss's divisor alike."""
    c = _cases()['lengths']
    assert c['tg_len'][6] > c['targets'].shape[1]
    out = _launch_case(c, 1)
    _, Ls = R.clamp_lengths(c['logits'].shape[0], c['targets'].shape[1], c['in_len'], c['tg_len'])
    mean = float(np.mean(out.nll.astype(np.float64) / np.maximum(Ls, 1)))
    assert out.nll[6] > 0 and abs(out.loss - mean) <= R.U * abs(mean) * (1 + 1e-6)


def test_a_sample_does_not_depend_on_its_batch():
    c = _cases()['batch_B256']
    sl = slice(0, 4)
    four = _launch(c['logits'][:, sl], c['targets'][sl], c['in_len'][sl], c['tg_len'][sl], 0, 1)
    for b in range(4):
        one = _launch(c['logits'][:, b:b + 1], c['targets'][b:b + 1], c['in_len'][b:b + 1], c['tg_len'][b:b + 1], 0, 1)
        assert torch.equal(one.nll_bits, four.nll_bits[b:b + 1])
        assert np.array_equal((4 * four.dl[:, b]).view(np.int32), one.dl[:, 0].view(np.int32))      # the factor 4 is exact


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def _XF():
    from cross_patient_speech_decoding_amd.nn_models import functional as XF
    return XF


@pytest.mark.parametrize('name', ['blank_3', 'stride'])
def test_functional_ctc_loss(name, monkeypatch):
    XF = _XF()
    c = _cases()[name]
    nll, loss, dl, parts = _ref(name, 1)
    T, B, C = c['logits'].shape
    tg, il, tl = (torch.from_numpy(c[k]) for k in ('targets', 'in_len', 'tg_len'))
    lbound, gbound = R.loss_bound(parts), R.grad_bound(parts)
    # an upstream gradient of 3, a (B, T, C) tensor seen time-major, int32 targets and lengths
    x = torch.from_numpy(c['logits']).permute(1, 0, 2).contiguous().cuda().requires_grad_(True)
    view = x.permute(1, 0, 2)
    assert not view.is_contiguous()
    out = XF.ctc_loss(view, tg.int().cuda(), il.int(), tl.int(), blank=c['blank'], zero_infinity=True)
    (3 * out).backward()
    assert abs(float(out.detach()) - loss) <= lbound
    got = x.grad.permute(1, 0, 2).cpu().numpy().astype(np.float64)
    assert (np.abs(got - 3 * dl) <= 3 * gbound + 2 * R.U * np.abs(3 * dl)).all()
    # device-resident lengths: a value above T is clamped by the kernel and does not raise
    over = il.clone()
    over[0] = T + 5
    assert int(R.clamp_lengths(T, tg.shape[1], over.numpy(), c['tg_len'])[0][0]) == int(il[0]) == T
    out2 = XF.ctc_loss(torch.from_numpy(c['logits']).cuda(), tg.cuda(), over.cuda(), tl.cuda(), blank=c['blank'])
    assert abs(float(out2) - loss) <= lbound
    # no_grad: the call is made without a gradient buffer
    seen = []
    real = XF.call
    monkeypatch.setattr(XF, 'call', lambda fn, *a: (seen.append((fn, a)), real(fn, *a))[1])
    with torch.no_grad():
        out3 = XF.ctc_loss(x.permute(1, 0, 2), tg.cuda(), il, tl, blank=c['blank'])
    assert [fn for fn, _ in seen] == ['xps_ctc_loss_f32'] and seen[0][1][13] is None and not out3.requires_grad
    assert float(out3) == float(out.detach())


def test_host_target_length_beyond_the_padded_width_raises():
    """torch refuses a target length above targets.shape[1]; so does CTCLossFn.forward for host lengths."""
    XF = _XF()
    c = _cases()['blank_3']
    tg, il, tl = (torch.from_numpy(c[k]) for k in ('targets', 'in_len', 'tg_len'))
    tl = tl.clone()
    tl[1] = tg.shape[1] + 1
    with pytest.raises(RuntimeError):
        torch.nn.functional.ctc_loss(torch.from_numpy(c['logits']).log_softmax(2), tg, il, tl, blank=3)
    with pytest.raises(RuntimeError, match='at least'):
        XF.ctc_loss(torch.from_numpy(c['logits']).cuda(), tg.cuda(), il, tl, blank=3)


def test_module_on_log_probs_and_sum_fallback(monkeypatch):
    """_HipCTCLoss takes log-probabilities as nn.CTCLoss does (the kernel's own log-softmax is then the identity up to
    rounding); reduction='sum' is torch's kernel, not this one: float32, held to 1e-5 of the float64 sum."""
    from cross_patient_speech_decoding_amd.realtime_sim.realtime_nn_model import _HipCTCLoss
    XF = _XF()
    c = _cases()['blank_3']
    tg, il, tl = (torch.from_numpy(c[k]) for k in ('targets', 'in_len', 'tg_len'))
    lp = torch.from_numpy(c['logits']).cuda().log_softmax(2)
    ref = R.ctc_ref(lp.cpu().numpy(), c['targets'], c['in_len'], c['tg_len'], 3, True, with_parts=True)
    seen = []
    real = XF.call
    monkeypatch.setattr(XF, 'call', lambda fn, *a: (seen.append(fn), real(fn, *a))[1])
    mean = _HipCTCLoss(blank=3, zero_infinity=True)(lp, tg.cuda(), il, tl)
    assert seen == ['xps_ctc_loss_f32'] and abs(float(mean) - ref[1]) <= R.loss_bound(ref[3])
    total = _HipCTCLoss(blank=3, reduction='sum', zero_infinity=True)(lp, tg.cuda(), il, tl)
    assert seen == ['xps_ctc_loss_f32'], 'reduction=sum went through the fused kernel'
    assert abs(float(total) - ref[0].sum()) <= 1e-5 * ref[0].sum()


def test_model_ctc_with_a_trial_shorter_than_the_window(golden_dir):
    """RealtimeRNNModel._ctc: trials 2 and 4 are shorter than the 14-sample window, so their adjusted lengths are 0 and -2.
    Trial 2 (two labels) is infeasible and zeroed, trial 4 (no label) has the empty alignment: both contribute 0 to the loss and
    a zero gradient, and the other trials have the reference's values."""
    import os
    from test_gpu_realtime import build
    g = np.load(os.path.join(golden_dir, 'realtime_train_small.npz'))
    m, (C, win, stride, H, L, ncls) = build(g)
    lengths, tl = torch.tensor([62, 62, 10, 62, 5]), torch.tensor([3, 3, 2, 1, 0])
    adjusted = m._adjusted_lengths(lengths)
    assert adjusted.tolist() == [13, 13, 0, 13, -2]
    x, targets = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['targets'])
    loss, logits_tm = m._ctc((x, targets.cuda(), lengths, tl))
    logits_tm.retain_grad()
    loss.backward()
    ref = R.ctc_ref(logits_tm.detach().cpu().numpy(), targets.numpy(), adjusted.numpy(), tl.numpy(), 0, True, with_parts=True)
    grad = logits_tm.grad.cpu().numpy()
    r = R.error_ratios((ref[0], float(loss), grad), ref)
    print(f'_ctc with short trials: error / bound loss {r[1]:.4f}, gradient {r[2]:.4f}')
    assert r[1] <= 1 and r[2] <= 1
    assert ref[0][2] == 0 and ref[0][4] == 0 and (ref[0][[0, 1, 3]] > 0).all()
    assert not grad[:, 2].any() and not grad[:, 4].any() and grad[:, [0, 1, 3]].any()
