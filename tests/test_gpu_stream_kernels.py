"""The four streaming kernels of csrc/xps_stream.hip (xps_gemv_f32, xps_gru_cell_gemv_f32, xps_window_shift_f32,
xps_ctc_collapse_f32) called directly and held to the float64 references and error bounds of tests/stream_ref.py, at the
shapes that reach every branch: the scalar branch of dot_rows (K % 4 != 0, H % 4 != 0), a partial last workgroup, template
widths wider than the live streams (B = 3, 5, 6, 7), win == stride, win == 1, ties, the token-buffer limit.  Then
StreamingDecoder, the batched forward and RealtimePipeline at model shapes that reach the same branches, against float64.

Every launch follows one protocol: buffers have S = B rounded up to a power of two rows plus a guard row; the unused and guard
rows of outputs hold a sentinel that must survive bit for bit; the unused rows of x / h_prev hold NaN and +-inf, which must
not reach a live row; read-only inputs keep their bits; a second launch gives the same bits."""
import functools

import numpy as np
import pytest
import torch

import stream_ref as R

pytestmark = pytest.mark.gpu

from weights import weights_from_seed  # noqa: E402

F32 = np.float32
SENT = 0x7FC0DEAD                    # a quiet-NaN bit pattern no kernel produces
KS = [1, 3, 4, 63, 64, 98, 256, 260, 1792]


def _call(name, *args):
    from cross_patient_speech_decoding_amd._lib import call
    call(name, *args)


def _stream():
    from cross_patient_speech_decoding_amd._dev import stream
    return stream()


def _rows(B):
    return 1 << (B - 1).bit_length()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _padded_in(live, B):
    """(S + 1, width) float32 on the device: the B live rows, then NaN / +inf / -inf in the unused and guard rows."""
    S = _rows(B)
    a = np.empty((S + 1, live.shape[1]), F32)
    a[:B] = live
    for i, r in enumerate(range(B, S + 1)):
        a[r] = (np.nan, np.inf, -np.inf)[i % 3]
    return _dev(a)


def _sentinel_out(B, width):
    S = _rows(B)
    return torch.full((S + 1, width), SENT, dtype=torch.int32, device='cuda').view(torch.float32)


def _check_out(out, again, B):
    """The shared output protocol; returns the live rows as float64."""
    assert torch.equal(_bits(out), _bits(again)), 'two launches differ'
    assert bool((_bits(out[B:]) == SENT).all()), 'an unused or guard row was written'
    live = out[:B].cpu().numpy()
    assert np.isfinite(live).all(), 'a live output is not finite'
    return live.astype(np.float64)


class _Unchanged:
    """Read-only inputs keep their bits."""

    def __init__(self, *tensors):
        self.pairs = [(t, _bits(t).clone()) for t in tensors if t is not None]

    def check(self):
        for t, before in self.pairs:
            assert torch.equal(_bits(t), before), 'a read-only input changed'


# ---- xps_gemv_f32 ---------------------------------------------------------------------------------------------------------
def _gemv(xd, Wd, bd, N, K, B):
    out = _sentinel_out(B, N)
    _call('xps_gemv_f32', xd.data_ptr(), Wd.data_ptr(), None if bd is None else bd.data_ptr(), out.data_ptr(), N, K, B,
          _stream())
    return out


@pytest.mark.parametrize('K', KS)
def test_gemv_vs_fp64(K):
    worst = 0.0
    for N in (1, 4, 5, 11, 130):
        rng = np.random.default_rng(7000 * K + N)
        _, W, bias = R.gemv_inputs(rng, N, K, 1)
        Wd, bd = _dev(W), _dev(bias)
        x0, first = rng.standard_normal(K).astype(F32), {}          # stream 0 has the same row at every B
        for B in range(1, 9):
            for use_bias in (True, False):
                x = rng.standard_normal((B, K)).astype(F32)
                x[0] = x0
                twins = B >= 3 or (B == 2 and not use_bias)
                if twins:
                    x[B - 1] = x[0]
                xd = _padded_in(x, B)
                keep = _Unchanged(xd, Wd, bd)
                b = bias if use_bias else None
                out = _gemv(xd, Wd, bd if use_bias else None, N, K, B)
                live = _check_out(out, _gemv(xd, Wd, bd if use_bias else None, N, K, B), B)
                keep.check()
                err, bound = np.abs(live - R.gemv_ref(x, W, b)), R.gemv_bound(x, W, b)
                assert (err <= bound).all(), (N, K, B, use_bias, float((err / bound).max()))
                worst = max(worst, float((err / bound).max()))
                if twins:
                    assert torch.equal(_bits(out[B - 1]), _bits(out[0]))
                assert torch.equal(_bits(out[0]), _bits(first.setdefault(use_bias, out[0]))), 'the bits depend on B'
    print(f'xps_gemv_f32 K={K}: max error / bound = {worst:.4f}')


def test_gemv_base_pointers_4_bytes_off_take_the_scalar_path():
    """K % 4 != 0 needs no alignment: x and W start 4 bytes past a 16-byte boundary."""
    N, K, B = 5, 98, 3
    rng = np.random.default_rng(98)
    x, W, bias = R.gemv_inputs(rng, N, K, B)
    xa = _padded_in(x, B)
    xd = torch.empty(xa.numel() + 1, dtype=torch.float32, device='cuda')[1:].view_as(xa).copy_(xa)
    Wd = torch.empty(N * K + 1, dtype=torch.float32, device='cuda')[1:].view(N, K).copy_(_dev(W))
    assert xd.data_ptr() % 16 == 4 and Wd.data_ptr() % 16 == 4
    bd = _dev(bias)
    keep = _Unchanged(xd, Wd, bd)
    live = _check_out(_gemv(xd, Wd, bd, N, K, B), _gemv(xd, Wd, bd, N, K, B), B)
    keep.check()
    assert (np.abs(live - R.gemv_ref(x, W, bias)) <= R.gemv_bound(x, W, bias)).all()


# ---- xps_gru_cell_gemv_f32 ------------------------------------------------------------------------------------------------
def _cell(xd, K, wd, hd, H, B):
    out = _sentinel_out(B, H)
    _call('xps_gru_cell_gemv_f32', xd.data_ptr(), K, wd[0].data_ptr(), wd[1].data_ptr(), wd[2].data_ptr(), wd[3].data_ptr(),
          hd.data_ptr(), out.data_ptr(), H, B, _stream())
    return out


@pytest.mark.parametrize('H', [1, 3, 4, 5, 30, 64, 66, 128])
def test_gru_cell_vs_fp64(H):
    worst = 0.0
    for K in (1, 6, 98, 256, 1792):
        for scale in (1.0, 8.0):                    # torch's U(-1, 1) / sqrt(H), and 8 x that: gates reach both rails
            rng = np.random.default_rng(9000 * H + 10 * K + int(scale))
            _, w_ih, w_hh, b_ih, b_hh, _ = R.cell_inputs(rng, H, K, 1, scale)
            wd = [_dev(a) for a in (w_ih, w_hh, b_ih, b_hh)]
            rails = np.zeros(2, bool)
            x0, h0, first = rng.standard_normal(K).astype(F32), rng.uniform(-1, 1, H).astype(F32), None
            for B in (1, 2, 3, 4, 5, 7, 8):
                x = rng.standard_normal((B, K)).astype(F32)
                h = rng.uniform(-1, 1, (B, H)).astype(F32)
                x[0], h[0] = x0, h0                 # stream 0 has the same rows at every B
                twins = B >= 3 or (B == 2 and scale > 1)
                if twins:
                    x[B - 1], h[B - 1] = x[0], h[0]
                xd, hd = _padded_in(x, B), _padded_in(h, B)
                keep = _Unchanged(xd, hd, *wd)
                out = _cell(xd, K, wd, hd, H, B)
                live = _check_out(out, _cell(xd, K, wd, hd, H, B), B)
                keep.check()
                ref, parts = R.gru_cell_ref(x, w_ih, w_hh, b_ih, b_hh, h)
                err, bound = np.abs(live - ref), R.cell_bound(parts)
                assert (err <= bound).all(), (H, K, B, scale, float((err / bound).max()))
                worst = max(worst, float((err / bound).max()))
                if twins:
                    assert torch.equal(_bits(out[B - 1]), _bits(out[0]))
                first = out[0] if first is None else first
                assert torch.equal(_bits(out[0]), _bits(first)), 'the bits depend on B'
                rails |= [parts['z'].min() < 0.02, parts['z'].max() > 0.98]
            if scale > 1 and K >= 98 and H >= 30:
                assert rails.all(), 'the wide weights were meant to saturate the gates both ways'
    print(f'xps_gru_cell_gemv_f32 H={H}: max error / bound = {worst:.4f}')


@pytest.mark.parametrize('H,K,B', [(5, 6, 3), (64, 6, 8), (30, 98, 2)])
def test_gru_cell_takes_each_bias_from_its_own_slot(H, K, B):
    """Zero weights, a different constant per gate and bias vector (and a slope along the units): the output is a function of
    the six bias slots alone, so a bias read from another gate or unit shows at full size."""
    j = np.arange(H) * 0.01
    b_ih = np.concatenate([0.5 + j, -1.0 + j, 2.0 - j]).astype(F32)
    b_hh = np.concatenate([-2.0 - j, 0.5 - j, 1.0 + j]).astype(F32)
    w_ih, w_hh = np.zeros((3 * H, K), F32), np.zeros((3 * H, H), F32)
    rng = np.random.default_rng(H)
    x, h = rng.standard_normal((B, K)).astype(F32), rng.uniform(-1, 1, (B, H)).astype(F32)
    wd = [_dev(a) for a in (w_ih, w_hh, b_ih, b_hh)]
    xd, hd = _padded_in(x, B), _padded_in(h, B)
    live = _check_out(_cell(xd, K, wd, hd, H, B), _cell(xd, K, wd, hd, H, B), B)
    ref, parts = R.gru_cell_ref(x, w_ih, w_hh, b_ih, b_hh, h)
    bound = R.cell_bound(parts)
    assert bound.max() < 2e-6
    assert (np.abs(live - ref) <= bound).all()


# ---- xps_window_shift_f32 -------------------------------------------------------------------------------------------------
def _shift(pd, k, C, Wd, cd, src, win, d, B):
    dst = _sentinel_out(B, win * d)
    _call('xps_window_shift_f32', pd.data_ptr(), k, C, None if Wd is None else Wd.data_ptr(),
          None if cd is None else cd.data_ptr(), src.data_ptr(), dst.data_ptr(), win, d, B, _stream())
    return dst


@pytest.mark.parametrize('win,d,C,k', [(14, 7, 5, 4), (14, 7, 5, 10), (4, 5, 5, 4), (1, 3, 3, 1), (14, 128, 128, 4),
                                       (37, 9, 20, 1)])
def test_window_shift_vs_long_double(win, d, C, k):
    modes = ['map+c', 'map'] + (['identity'] if d == C else [])
    worst = 0.0
    for B in (1, 2, 5, 8):
        for mode in modes:
            rng = np.random.default_rng(100 * win + 10 * B + len(mode))
            power = np.abs(rng.standard_normal((B, k, C))) * 10.0 ** rng.integers(-3, 4, (B, k, 1))
            W = rng.standard_normal((B, C, d)) if mode != 'identity' else None        # a different map per stream
            c = rng.standard_normal((B, d)) if mode == 'map+c' else None
            src = rng.standard_normal((B, win * d)).astype(F32)
            if B >= 5:                                  # twins: the last stream repeats the first
                power[B - 1], src[B - 1] = power[0], src[0]
                if W is not None:
                    W[B - 1] = W[0]
                if c is not None:
                    c[B - 1] = c[0]
            pd, srcd = _dev(power), _padded_in(src, B)
            Wd, cd = (None if a is None else _dev(a) for a in (W, c))
            keep = _Unchanged(pd, srcd, Wd, cd)
            out = _shift(pd, k, C, Wd, cd, srcd, win, d, B)
            assert torch.equal(_bits(out), _bits(_shift(pd, k, C, Wd, cd, srcd, win, d, B)))
            assert bool((_bits(out[B:]) == SENT).all())
            keep.check()
            got = out[:B].cpu().numpy()
            ref, tol = R.window_shift_ref(power, k, W, c, src)
            old = (win - k) * d
            np.testing.assert_array_equal(got[:, :old].view(np.int32), ref[:, :old].view(np.int32))
            if mode == 'identity':
                np.testing.assert_array_equal(got[:, old:].view(np.int32), ref[:, old:].view(np.int32))
            else:
                err = np.abs(got[:, old:].astype(np.float64) - ref[:, old:].astype(np.float64)).reshape(B, k, d)
                assert (err <= tol).all(), (B, mode, float((err / tol).max()))
                worst = max(worst, float((err / tol).max()))
            if B >= 5:
                assert torch.equal(_bits(out[B - 1]), _bits(out[0]))
                assert not torch.equal(_bits(out[1]), _bits(out[0]))
    print(f'xps_window_shift_f32 win={win} d={d} C={C} k={k}: max error / tolerance = {worst:.4f}')


# ---- xps_ctc_collapse_f32 -------------------------------------------------------------------------------------------------
def _collapse_run(logits_d, n_classes, blank, max_tokens, B, every=10):
    """All steps from a fresh state; snapshots (step, argmax, state, tokens) after every `every`-th step and the last."""
    S, T = _rows(B), logits_d.shape[0]
    arg = torch.full((S + 1,), -9, dtype=torch.int64, device='cuda')
    state = torch.full((S + 1, 3), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    state[:B] = torch.tensor([-1, 0, 0], dtype=torch.int32)
    tokens = torch.full((S + 1, max_tokens), -7, dtype=torch.int64, device='cuda')
    snaps = []
    for t in range(T):
        _call('xps_ctc_collapse_f32', logits_d[t].data_ptr(), n_classes, blank, arg.data_ptr(), state.data_ptr(),
              tokens.data_ptr(), max_tokens, B, _stream())
        if (t + 1) % every == 0 or t == T - 1:
            snaps.append((t, arg.cpu().numpy(), state.cpu().numpy(), tokens.cpu().numpy()))
    return snaps


@pytest.mark.parametrize('n_classes', [1, 2, 11, 41])
def test_ctc_collapse_equals_reference_exactly(n_classes):
    T = 60
    for blank in sorted({0, n_classes - 1}):
        for B in (1, 3, 8):
            S = _rows(B)
            rng = np.random.default_rng(1000 * n_classes + 10 * B + blank)
            logits = rng.integers(0, 3, (T, B, n_classes)).astype(F32)         # a grid of three values: ties
            if B >= 3:
                logits[:, B - 1] = logits[:, 0]
            tied = ((logits == logits.max(-1, keepdims=True)).sum(-1) > 1).mean()
            assert tied > (0.5 if n_classes >= 11 else 0.2 if n_classes == 2 else -1), tied
            padded = np.full((T, S + 1, n_classes), np.nan, F32)
            padded[:, :B] = logits
            ld = _dev(padded)
            keep = _Unchanged(ld)
            for max_tokens in (1, 4, 64):
                ref = R.collapse_ref(logits, blank, max_tokens, fill=-7)
                if n_classes >= 2 and max_tokens < 64:
                    first = [min(t for t in range(T) if ref[t][1][s, 2]) for s in range(B) if ref[-1][1][s, 2]]
                    assert first, 'no stream of the reference overflows'
                snaps = _collapse_run(ld, n_classes, blank, max_tokens, B)
                assert [s[0] for s in snaps] == [9, 19, 29, 39, 49, 59]
                for t, arg, state, tokens in snaps:
                    r_arg, r_state, r_tokens = ref[t]
                    np.testing.assert_array_equal(arg[:B], r_arg)
                    np.testing.assert_array_equal(state[:B], r_state)
                    np.testing.assert_array_equal(tokens[:B], r_tokens)     # a full row stays as it was, the flag stays set
                    assert (arg[B:] == -9).all() and (state[B:] == 0x5A5A5A5A).all() and (tokens[B:] == -7).all()
                again = _collapse_run(ld, n_classes, blank, max_tokens, B)
                for a, b in zip(snaps, again):
                    assert all(np.array_equal(u, v) for u, v in zip(a[1:], b[1:]))
            keep.check()


# ---- module level: StreamingDecoder, the batched forward and RealtimePipeline at the shapes that reach the new branches ------
#          (d, win, stride, H, L, n_classes), seed: the seed makes the float64 top-two margin exceed 2e-4 at every step
CONFIGS = {'k98_h30': ((7, 14, 4, 30, 3, 11), 5),           # K = 98 and H = 30: both scalar branches, partial last workgroup
           'win_eq_stride': ((5, 4, 4, 66, 1, 2), 0),       # K = 20 vector, H = 66 scalar
           'win1': ((3, 1, 1, 4, 2, 41), 6)}                # K = 3 scalar, H = 4 vector, one workgroup
N_WINDOWS, MAX_STREAMS = 40, 8


def _stream_model(cfg, seed, fc_gain=1.0):
    from cross_patient_speech_decoding_amd.realtime_sim import RealtimeRNNModel
    d, win, stride, H, L, ncls = cfg
    m = RealtimeRNNModel(win * d, H, L, ncls, dropout=0.0, win_size=win, stride=stride)
    sd = weights_from_seed(m.state_dict(), seed)
    sd['h0'] = torch.from_numpy(np.random.default_rng(seed + 1).uniform(-0.5, 0.5, (L, 1, H)).astype(F32))
    sd['classifier.fc.weight'] = sd['classifier.fc.weight'] * fc_gain
    m.load_state_dict(sd)
    return m.eval()


def _fp64_logits(m, windows):
    """windows (n, T, K) float32 -> (n, T, n_classes) float64 from plain torch modules built from m's state_dict."""
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    K, H, L = sd['rnn.rnn.weight_ih_l0'].shape[1], sd['h0'].shape[2], sd['h0'].shape[0]
    gru = torch.nn.GRU(K, H, L, batch_first=True).double()
    gru.load_state_dict({k[len('rnn.rnn.'):]: v for k, v in sd.items() if k.startswith('rnn.rnn.')})
    fc = torch.nn.Linear(H, sd['classifier.fc.bias'].numel()).double()
    fc.load_state_dict({'weight': sd['classifier.fc.weight'], 'bias': sd['classifier.fc.bias']})
    with torch.no_grad():
        y, _ = gru(windows.double(), sd['h0'].expand(-1, windows.shape[0], -1).contiguous())
        return fc(y)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model on the host, x (8, T, d), windows (8, 40, K), float64 logits (8, 40, n_classes)), computed once."""
    cfg, seed = CONFIGS[name]
    d, win, stride = cfg[:3]
    m = _stream_model(cfg, seed)
    T = win + (N_WINDOWS - 1) * stride
    x = torch.from_numpy(np.random.default_rng(seed + 2).standard_normal((MAX_STREAMS, T, d)).astype(F32))
    idx = (torch.arange(N_WINDOWS) * stride)[:, None] + torch.arange(win)
    windows = x[:, idx, :].reshape(MAX_STREAMS, N_WINDOWS, win * d)
    ref = _fp64_logits(m, windows)
    top = ref.topk(2, dim=-1).values
    assert float((top[..., 0] - top[..., 1]).min()) > 2e-4, 'choose another seed: a float64 top-two margin is below 2e-4'
    return m, x, windows, ref


@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('name', list(CONFIGS))
def test_streaming_decoder_vs_fp64(name, use_graph):
    from cross_patient_speech_decoding_amd.realtime_sim.realtime_nn_model import StreamingDecoder
    m, _, windows, ref = _case(name)
    m = m.cuda()
    for n in (2, 5, 8):
        dec = StreamingDecoder(m, n_streams=n, use_graph=use_graph)
        wd = windows[:n].cuda()
        got, tok = [], []
        for w in range(N_WINDOWS):
            got.append(dec.step(wd[:, w]).clone())
            tok.append(dec.token.clone())
        got, tok = torch.stack(got, 1).cpu().double(), torch.stack(tok, 1).cpu()
        err = float((got - ref[:n]).abs().max())
        print(f'StreamingDecoder {name} n_streams={n} graph={use_graph}: max |logits - fp64| = {err:.3e}')
        assert err <= 1e-4
        assert torch.equal(got.argmax(-1), ref[:n].argmax(-1))
        assert torch.equal(tok, ref[:n].argmax(-1))
        assert bool(torch.isfinite(dec.hbuf).all())


@pytest.mark.parametrize('name', list(CONFIGS))
def test_batched_forward_vs_fp64(name, gemm_precision):
    m, x, _, ref = _case(name)
    with torch.no_grad():
        got = m.cuda()(x.cuda()).cpu().double()
    assert got.shape == ref.shape
    err = float((got - ref).abs().max())
    print(f'forward {name} {gemm_precision}: max |logits - fp64| = {err:.3e}')
    assert err <= 1e-4
    assert torch.equal(got.argmax(-1), ref.argmax(-1))


def _pipe_helpers():
    import test_gpu_realtime_pipeline as P
    from cross_patient_speech_decoding_amd import realtime_sim
    from cross_patient_speech_decoding_amd.realtime_sim import realtime_processing as rp
    return P, realtime_sim, rp


def _ref_tokens(full, s, blank=0, max_tokens=4096):
    """collapse_ref over the offline logits (n, n_pred, n_classes) of stream s -> (tokens, overflow flag)."""
    _, state, tokens = R.collapse_ref(full[s:s + 1].permute(1, 0, 2).cpu().numpy(), blank, max_tokens)[-1]
    return tokens[0, :state[0, 1]], int(state[0, 2])


@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('n_streams', [2, 5])
def test_pipeline_mapped_c5_to_d7_vs_references(n_streams, use_graph):
    """5 channels mapped to 7 features by a different affine map per stream; win 14, stride 4, H 30, L 3 (K = 98)."""
    P, rt, rp = _pipe_helpers()
    C, Tn, n_pred = 5, 40, 25
    cfg = CONFIGS['k98_h30'][0]
    d, win, stride = cfg[:3]
    m = _stream_model(cfg, 77, fc_gain=4.0).cuda()
    rng = np.random.default_rng(50 + n_streams)
    maps = [(rng.standard_normal((C, d)) * 3.0, rng.standard_normal(d) * 0.1) for _ in range(n_streams)]
    Wm, cm = np.stack([w for w, _ in maps]), np.stack([c for _, c in maps])
    bads = [[1], [], [0, 4], [], [2]][:n_streams]
    coefs = P._iir(4, 2)
    bins = rng.standard_normal((n_streams, win + (n_pred - 1) * stride, C, Tn))
    bins *= rng.uniform(0.2, 5.0, (n_streams, bins.shape[1], 1, 1))            # the power moves from bin to bin
    power, _ = P._offline_power(rp, bins, coefs, bads)
    full = P._offline_logits(m, power, maps)
    pipe = rt.RealtimePipeline(m, coefs, C, Tn, n_streams=n_streams, bad_channels=bads, feature_map=maps,
                               use_graph=use_graph)
    p = win - stride
    pipe.prime(bins[:, :p])
    got = []
    for w in range(n_pred):
        before = pipe.features.reshape(n_streams, -1).cpu().numpy()
        got.append(pipe.step(bins[:, p + w * stride:p + (w + 1) * stride]).clone())
        ref, tol = R.window_shift_ref(pipe.power.cpu().numpy(), stride, Wm, cm, before)
        feat = pipe.features.reshape(n_streams, -1).cpu().numpy()
        old = (win - stride) * d
        np.testing.assert_array_equal(feat[:, :old], ref[:, :old])
        err = np.abs(feat[:, old:].astype(np.float64) - ref[:, old:].astype(np.float64)).reshape(tol.shape)
        assert (err <= tol).all()
    got = torch.stack(got, 1)
    assert got.shape == full.shape == (n_streams, n_pred, cfg[5])
    assert float((got - full).abs().max()) <= 1e-4
    assert torch.equal(got.argmax(-1), full.argmax(-1))
    counts = []
    for s in range(n_streams):
        want, over = _ref_tokens(full, s)
        assert not over
        np.testing.assert_array_equal(pipe.decoded(s).cpu().numpy(), want)
        counts.append(len(want))
    print(f'pipeline n_streams={n_streams} graph={use_graph}: tokens per stream {counts}')
    # a token buffer below the token count: decoded raises for the streams that overflow, and only for them
    assert max(counts) >= 2, 'the reference decodes fewer than two tokens in every stream'
    small = rt.RealtimePipeline(m, coefs, C, Tn, n_streams=n_streams, bad_channels=bads, feature_map=maps,
                                use_graph=use_graph, max_tokens=1)
    small.prime(bins[:, :p])
    for w in range(n_pred):
        small.step(bins[:, p + w * stride:p + (w + 1) * stride])
    for s in range(n_streams):
        want, over = _ref_tokens(full, s, max_tokens=1)
        assert over == (counts[s] >= 2)
        if over:
            with pytest.raises(RuntimeError, match='max_tokens'):
                small.decoded(s)
        else:
            np.testing.assert_array_equal(small.decoded(s).cpu().numpy(), want)


@pytest.mark.parametrize('use_graph', [False, True])
def test_pipeline_win_equals_stride_empty_prime(use_graph):
    """win == stride: prime() takes no bins and launches nothing; every step replaces the whole window (k == win)."""
    P, rt, rp = _pipe_helpers()
    cfg = CONFIGS['win_eq_stride'][0]
    d, win, stride = cfg[:3]
    C, Tn, n_pred, n = d, 40, 6, 5
    m = _stream_model(cfg, 78).cuda()
    coefs = P._iir(4, 2)
    rng = np.random.default_rng(60)
    bins = rng.standard_normal((n, n_pred * stride, C, Tn))
    bads = [[], [3], [], [0], []]
    power, _ = P._offline_power(rp, bins, coefs, bads)
    full = P._offline_logits(m, power, [None] * n)
    pipe = rt.RealtimePipeline(m, coefs, C, Tn, n_streams=n, bad_channels=bads, use_graph=use_graph)
    pipe.prime(bins[:, :0])
    assert pipe.frames == 0
    for w in range(n_pred):
        logits = pipe.step(bins[:, w * stride:(w + 1) * stride])
        np.testing.assert_array_equal(pipe.features.cpu().numpy(), power[:, w * stride:(w + 1) * stride].astype(F32))
        assert float((logits - full[:, w]).abs().max()) <= 1e-4
        assert torch.equal(logits.argmax(-1), full[:, w].argmax(-1))
    for s in range(n):
        np.testing.assert_array_equal(pipe.decoded(s).cpu().numpy(), _ref_tokens(full, s, blank=0)[0])
