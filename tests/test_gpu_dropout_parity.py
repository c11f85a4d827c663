"""Training with dropout ON against a float64 reference that consumes the very dropout decisions the kernels made.

Every dropout site draws a 64-bit seed from functional.next_dropout_seed; the tests record those seeds (a wrapper that
returns the real seed), rebuild each site's {0, 1} mask with the kernels' own generator (xps_dropout_f32 in mask mode, in
the HIP layout of the site) and hand the masks to the CPU reference (oracle/seq2seq_oracle.py, ``masks=``).  No test
restates the generator.  To rule out a vacuous pass, every test also asserts the number of sites, each site's dropped
fraction, that the result differs from the undropped one, and that the masks of a shifted seed list fail the comparison.

The TemporalConv tests also hold BatchNorm to float64 under a per-channel offset of 1e2 .. 3e3 times the spread, where a
one-pass E[y^2] - E[y]^2 variance in float32 cancels (BatchNorm statistics)."""
import os

import numpy as np
import pytest
import torch

from weights import weights_from_seed

pytestmark = pytest.mark.gpu

P = 0.3
SEED_STRIDE = 0x9E3779B97F4A7C15             # functional.next_dropout_seed advances by this: +1 stride = the next seed
NOISE_KEY = 'temporal_conv.conv.bias'        # analytically zero gradient (train-mode BatchNorm follows): see test_gpu_seq2seq.py


def XF():
    from cross_patient_speech_decoding_amd.nn_models import functional
    return functional


def lib():
    from cross_patient_speech_decoding_amd._lib import lib as _l
    return _l()


@pytest.fixture(scope='module', autouse=True)
def _built():
    from cross_patient_speech_decoding_amd import _build
    _build.build(verbose=False)
    assert torch.cuda.is_available(), 'gpu tests need the MI355X'


@pytest.fixture
def seeds(monkeypatch):
    """The seeds of every dropout site drawn during the test, in order.  The counter restarts from torch's generator, so
    a test that seeds torch gets the same seeds in every run."""
    xf = XF()
    rec = []
    real = xf.next_dropout_seed

    def recording():
        s = real()
        rec.append(s)
        return s

    monkeypatch.setattr(xf, '_DROP_COUNTER', [0])
    monkeypatch.setattr(xf, 'next_dropout_seed', recording)
    return rec


@pytest.fixture
def cluster_mode():
    """Restores the launch mode of the recurrence after a test changed it (as in test_gpu_gru_cluster.py)."""
    old = lib().xps_get_gru_cluster_mode()
    yield XF().set_gru_cluster_mode
    lib().xps_set_gru_cluster_mode(old)


def site_mask(shape, p, seed):
    """{0, 1} decisions of one dropout site from the kernels' generator, in the site's HIP layout, as float64 on the CPU."""
    xf = XF()
    m = torch.empty(shape, dtype=torch.float32, device='cuda')
    xf.call('xps_dropout_f32', None, None, xf._ptr(m), m.numel(), float(p), int(seed), xf._stream())
    return m.cpu().double()


def shifted(seed_list):
    return [(s + SEED_STRIDE) % 2 ** 64 for s in seed_list]


def check_fraction(mask, p):
    n = mask.numel()
    frac = 1.0 - float(mask.mean())
    assert set(torch.unique(mask).tolist()) <= {0.0, 1.0}
    assert abs(frac - p) <= 5 * (p * (1 - p) / n) ** 0.5 + 1.0 / n, (frac, p, n)


def maxerr(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


# ----------------------------------------------------------------------------- TemporalConv + BatchNorm + ReLU + dropout
def conv_bn_ref(x, w, b, gamma, beta, rm, rv, stride, relu, mask, p, eps, wt, dtype):
    """Conv1d -> BatchNorm1d (train) -> [ReLU] -> x * mask / (1 - p) in `dtype` on the CPU, reference layout (B, F, T').
    Returns out, running mean / var, the four parameter gradients, d(conv output)."""
    prm = [t.detach().to(dtype).clone().requires_grad_(True) for t in (w, b, gamma, beta)]
    rm_, rv_ = rm.to(dtype).clone(), rv.to(dtype).clone()
    y = torch.nn.functional.conv1d(x.to(dtype).permute(0, 2, 1), prm[0], prm[1], stride=stride)
    y.retain_grad()
    o = torch.nn.functional.batch_norm(y, rm_, rv_, prm[2], prm[3], training=True, momentum=0.1, eps=eps)
    if relu:
        o = torch.relu(o)
    if mask is not None:
        o = o * mask.to(dtype) / (1.0 - p)
    if wt is not None:
        (o * wt.to(dtype)).sum().backward()
    return o.detach(), rm_, rv_, [q.grad for q in prm], y.grad


CONV_SHAPES = {           # B, T, Cin, F, k, stride
    'small': (6, 50, 7, 11, 10, 10),                 # ~30 rows: one stage-1 partial, one column block
    'ragged_rows': (37, 71, 7, 11, 5, 3),            # T' = 23: 851 rows, not a multiple of 64
    'F100': (16, 40, 5, 100, 4, 4),                  # two column blocks, the second ragged
    'F257': (40, 60, 3, 257, 6, 6),                  # five column blocks, one column in the last
    'configs3': (2048, 200, 30, 100, 10, 10),        # the bench conv: 40960 rows = 640 stage-1 partials
}


def run_conv_case(shape, relu, prefill, offset, seed):
    """HIP TemporalConvFn (training, fused dropout) vs float64 torch with the same mask; float32 torch on the same data
    sets the scale of the tolerances.  offset: per-channel conv bias of `offset` x the spread of the conv output."""
    B, T, Cin, F, k, s = CONV_SHAPES[shape]
    Tp = (T - k) // s + 1
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, Cin, generator=g)
    w = torch.randn(F, Cin, k, generator=g) / (Cin * k) ** 0.5
    b = torch.randn(F, generator=g) * 0.1
    if offset:
        b = offset * (1.0 + torch.rand(F, generator=g)) * torch.where(torch.rand(F, generator=g) < 0.5, -1.0, 1.0)
    gamma = torch.rand(F, generator=g) + 0.5
    beta = torch.rand(F, generator=g) * 0.6 - 0.3
    rm0 = torch.rand(F, generator=g) * 0.4 - 0.2
    rv0 = torch.rand(F, generator=g) + 0.5
    wt = torch.randn(B, F, Tp, generator=g)
    eps = 1e-5
    if relu:
        # no upstream gradient where the normalised value is within 1e-4 of the ReLU kink: there a rounding difference may
        # flip the gate between float32 and float64 (a few of the 4M elements at the configs[3] shape)
        pre = conv_bn_ref(x, w, b, gamma, beta, rm0, rv0, s, False, None, P, eps, None, torch.float64)[0]
        wt = wt * (pre.abs() > 1e-4).float()
    mask_tm = site_mask((Tp, B, F), P, seed)                 # (T', B, F): the layout the kernels read
    check_fraction(mask_tm, P)
    mask = mask_tm.permute(1, 2, 0)                          # (B, F, T')
    ref = conv_bn_ref(x, w, b, gamma, beta, rm0, rv0, s, relu, mask, P, eps, wt, torch.float64)
    r32 = conv_bn_ref(x, w, b, gamma, beta, rm0, rv0, s, relu, mask, P, eps, wt, torch.float32)

    xf = XF()
    params = [t.cuda().requires_grad_(True) for t in (w, b, gamma, beta)]
    g0 = [torch.randn(q.shape, generator=g) for q in params]
    if prefill:                                              # .grad present: the direct_bn / accumulate branches
        for q, gg in zip(params, g0):
            q.grad = gg.cuda()
    rm, rv = rm0.cuda(), rv0.cuda()
    nbt = torch.zeros((), dtype=torch.long, device='cuda')
    out = xf.TemporalConvFn.apply(x.cuda(), *params, rm, rv, s, True, relu, mask_tm.float().cuda(), 1.0 / (1.0 - P),
                                  0.1, eps, None, None, nbt)
    (out * wt.permute(2, 0, 1).contiguous().cuda()).sum().backward()
    torch.cuda.synchronize()
    assert int(nbt) == 1
    got = out.detach().permute(1, 2, 0).cpu()

    def tol(r32_val, ref_val, floor):
        # a small multiple of float32 torch's own error on the same data, plus a floor relative to the quantity's scale
        return 4 * maxerr(r32_val, ref_val) + floor * max(1.0, float(ref_val.abs().max()))

    errs = {}
    t_out = tol(r32[0], ref[0], 3e-5)
    errs['out'] = (maxerr(got, ref[0]), t_out)
    errs['running_mean'] = (maxerr(rm, ref[1]), 4 * maxerr(r32[1], ref[1]) + 1e-6 * max(1.0, float(ref[1].abs().max())))
    errs['running_var'] = (maxerr(rv, ref[2]), 4 * maxerr(r32[2], ref[2]) + 1e-5 * max(1.0, float(ref[2].abs().max())))
    dy_scale = float(ref[4].abs().sum(dim=(0, 2)).max())     # d(conv bias) = column sums of dy: analytically ~0, noise
    for name, q, gg, r, r3 in zip(('dW', 'dconv_b', 'dgamma', 'dbeta'), params, g0, ref[3], r32[3]):
        want = r + gg.double() if prefill else r
        have = q.grad.detach().cpu()
        if name == 'dconv_b':
            errs[name] = (maxerr(have, want), 4 * maxerr(r3, r) + 1e-5 * dy_scale)
        else:
            errs[name] = (maxerr(have, want), 4 * maxerr(r3, r) + 1e-4 * max(1.0, float(r.abs().max())))
    bad = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not bad, f'error > tolerance: {bad}'
    # not vacuous: the undropped output and the output of the next seed's mask are both far outside the tolerance
    plain = conv_bn_ref(x, w, b, gamma, beta, rm0, rv0, s, relu, None, P, eps, None, torch.float64)[0]
    assert maxerr(got, plain) > 100 * t_out
    wrong = site_mask((Tp, B, F), P, shifted([seed])[0]).permute(1, 2, 0)
    assert maxerr(got, conv_bn_ref(x, w, b, gamma, beta, rm0, rv0, s, relu, wrong, P, eps, None, torch.float64)[0]) > 100 * t_out
    return errs


@pytest.mark.parametrize('shape,relu,prefill', [
    ('small', False, False), ('small', True, True),
    ('ragged_rows', True, False), ('ragged_rows', False, True),
    ('F100', False, False), ('F100', True, True),
    ('F257', True, False), ('F257', False, True),
    ('configs3', False, False), ('configs3', True, True),
])
def test_temporal_conv_bn_dropout_vs_fp64(shape, relu, prefill):
    run_conv_case(shape, relu, prefill, 0.0, 11 + len(shape))


@pytest.mark.parametrize('shape,offset', [('configs3', 1e2), ('configs3', 1e3), ('F100', 3e3)])
def test_batchnorm_statistics_survive_a_large_channel_offset(shape, offset):
    """conv bias = +-(1 .. 2) x offset x the spread of W x: normalised output, running stats and every gradient within a
    small multiple of what float32 torch BatchNorm reaches on the same data.  (A one-pass float32 variance loses about a
    quarter of rstd at offset 1e3 and 40960 rows, and goes negative -- rstd = 1/sqrt(eps) -- at 3e3.)"""
    run_conv_case(shape, False, False, offset, 5)


# ----------------------------------------------------------------------------- encoder with inter-layer dropout
def _encoder_path(T, B, H, precision):
    xf = XF()
    fused = xf.fused_dropout_supported(T, B, H, 2)
    split4 = xf.layer_output_split4_ok(T, B, H, 2, P)
    cluster = lib().xps_gru_seq_status_offset(T, B, H, 2) >= 0
    return fused, split4, cluster


@pytest.mark.parametrize('H,T,B,In,mode', [
    (64, 12, 64, 24, None), (128, 12, 64, 24, None),           # register-resident kernels, dropout fused
    (96, 9, 48, 20, None),                                     # separate dropout pass
    (512, 20, 256, 100, 'persistent'), (512, 20, 256, 100, 'steps'),
    (500, 20, 256, 100, 'persistent'),                         # cluster kernels; split4 output in bf16x3 mode
])
def test_encoder_inter_layer_dropout_vs_masked_fp64_oracle(H, T, B, In, mode, gemm_precision, cluster_mode, seeds):
    from oracle.seq2seq_oracle import gru_masked
    from cross_patient_speech_decoding_amd.nn_models.models import EncoderRNN
    if mode is not None:
        cluster_mode(mode)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    fused, split4, cluster = _encoder_path(T, B, H, gemm_precision)
    if H in (64, 128):
        assert fused and not split4 and not cluster
    elif H == 96:
        assert not fused and not split4 and not cluster
    else:
        assert cluster and not fused and split4 == (gemm_precision == 'bf16x3')
    torch.manual_seed(H + T)
    enc = EncoderRNN(In, H, 2, dropout=P)
    ref_rnn = torch.nn.GRU(In, H, 2, batch_first=True, dropout=P, bidirectional=True).double()
    ref_rnn.load_state_dict({k: v.double() for k, v in enc.rnn.state_dict().items()})
    enc = enc.cuda().train()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(T, B, In, generator=g)
    wy = torch.randn(T, B, 2 * H, generator=g)
    wh = torch.randn(B, H, generator=g)
    xg = x.cuda().requires_grad_(True)
    y, last = enc.forward_tm_last(xg)
    ((y * wy.cuda()).sum() + (last * wh.cuda()).sum()).backward()
    XF().check_gru_status()
    assert len(seeds) == 1                                      # one site: the output of layer 0
    mask = site_mask((T, B, 2 * H), P, seeds[0])
    check_fraction(mask, P)

    def reference(masks, grad=True):
        for q in ref_rnn.parameters():
            q.grad = None
        xr = x.double().permute(1, 0, 2).clone().requires_grad_(True)
        out, hn = gru_masked(ref_rnn, xr, None, [m.permute(1, 0, 2) for m in masks])
        lst = hn[-2] + hn[-1]
        if grad:
            ((out * wy.double().permute(1, 0, 2)).sum() + (lst * wh.double()).sum()).backward()
        return out.detach().permute(1, 0, 2), lst.detach(), xr.grad

    y_ref, last_ref, dx_ref = reference([mask])
    ty, tdx = 5e-5, 1e-4
    assert maxerr(y, y_ref) <= ty, maxerr(y, y_ref)
    assert maxerr(last, last_ref) <= ty, maxerr(last, last_ref)
    e = maxerr(xg.grad, dx_ref.permute(1, 0, 2))
    assert e <= tdx + 1e-4 * float(dx_ref.abs().max()), e
    for name, q in enc.rnn.named_parameters():
        r = dict(ref_rnn.named_parameters())[name].grad
        e = maxerr(q.grad, r)
        assert e <= 2e-4 * max(1.0, float(r.abs().max())), (name, e)
    # not vacuous: undropped (p = 0) and next-seed masks miss by far
    y0, _, _ = reference([torch.ones_like(mask) * (1 - P)], grad=False)    # x * (1 - p) / (1 - p) = x: no dropout
    assert maxerr(y, y0) > 100 * ty
    yw, _, _ = reference([site_mask((T, B, 2 * H), P, shifted(seeds)[0])], grad=False)
    assert maxerr(y, yw) > 100 * ty


# ----------------------------------------------------------------------------- whole training step, dropout 0.3 / 0.3
_step_ref_cache = {}


def oracle_masks(seed_list, Tp, B, F, H, L_enc, L_dec, steps):
    """Rebuild every site's mask from the recorded seeds, in the order the HIP model draws them (conv, encoder layers
    0 .. L-2, then per decode step the inputs of decoder layers 1 .. Ld-1), in the oracle's layouts."""
    it = iter(seed_list)
    conv = site_mask((Tp, B, F), P, next(it))
    enc = [site_mask((Tp, B, 2 * H), P, next(it)) for _ in range(L_enc - 1)]
    dec = [[site_mask((B, H), P, next(it)) for _ in range(L_dec - 1)] for _ in range(steps)]
    for m in [conv] + enc + [d for st in dec for d in st]:
        check_fraction(m, P)
    return {'conv': conv.permute(1, 2, 0), 'enc': [m.permute(1, 0, 2) for m in enc], 'dec': dec}


def run_train_step(cfg, B, T, wseed, xseed, gemm_precision, seeds):
    """ONE full training step (teacher forcing mixed, dropout 0.3 conv / 0.3 rnn) of the HIP Seq2SeqRNN + FlatAdamW against
    the float64 oracle with the same weights, coins and dropout decisions: logits, loss, every gradient, clipped norm,
    updated weights and BatchNorm running statistics, at the tolerances of test_north_star_model_shape_vs_oracle."""
    from oracle.seq2seq_oracle import Seq2SeqOracle
    from cross_patient_speech_decoding_amd.nn_models import Seq2SeqRNN
    from cross_patient_speech_decoding_amd.nn_models.trainer import FlatAdamW
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    C, F, H, Le, Ld, k, s = (cfg[n] for n in ('in_channels', 'n_filters', 'hidden_size', 'n_enc_layers', 'n_dec_layers',
                                               'kernel_size', 'stride'))
    Tp = (T - k) // s + 1
    args = (C, F, H, 9, Le, Ld, k, s, 0, P, P)
    m = Seq2SeqRNN(*args, 'gru', 1e-3, 1e-5, activation=cfg['activation'], decay_iters=5)
    sd = weights_from_seed(m.state_dict(), wseed)
    m.load_state_dict(sd)
    m = m.cuda().train()
    rng = np.random.default_rng(xseed)
    x = torch.from_numpy(rng.standard_normal((B, T, C)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, 9, (B, 3)))
    coins = [True, False, True]
    torch.manual_seed(1234)                                   # fixes the dropout seeds
    opt = FlatAdamW(m, lr=1e-3, weight_decay=1e-5, max_norm=0.5)
    opt.zero_grad()
    out = m(x.cuda(), y.cuda(), coins=coins)
    loss = m.criterion(out.view(-1, 9), y.cuda().view(-1))
    loss.backward()
    XF().check_gru_status()
    grads = {kk: q.grad.detach().cpu().clone() for kk, q in m.named_parameters()}
    opt.step()
    torch.cuda.synchronize()
    assert len(seeds) == 1 + (Le - 1) + 3 * (Ld - 1), len(seeds)
    masks = oracle_masks(seeds, Tp, B, F, H, Le, Ld, 3)

    def oracle():
        o = Seq2SeqOracle(*args, learning_rate=1e-3, l2_reg=1e-5, activation=cfg['activation'])
        o.load_state_dict(sd)
        return o.double()

    key = (tuple(sorted(cfg.items())), B, T, wseed, xseed, tuple(seeds))
    if key not in _step_ref_cache:                            # the float64 step does not depend on the GEMM mode
        orc = oracle().train()
        opt_ref, _ = orc.make_optimizer()
        opt_ref.zero_grad()
        ref = orc(x.double(), y, coins=coins, masks=masks)
        loss_ref = torch.nn.functional.cross_entropy(ref.reshape(-1, 9), y.reshape(-1))
        loss_ref.backward()
        g_ref = {kk: q.grad.detach().clone() for kk, q in orc.named_parameters()}
        gn_ref = float(torch.nn.utils.clip_grad_norm_(orc.parameters(), 0.5))
        opt_ref.step()
        after = {kk: v.detach().clone() for kk, v in orc.state_dict().items()}
        # controls: the same step without dropout, and with the masks of the next seeds
        with torch.no_grad():
            plain = oracle().eval()
            plain.temporal_conv.bn.train()
            ref0 = plain(x.double(), y, coins=coins)
            refw = oracle().train()(x.double(), y, coins=coins, masks=oracle_masks(shifted(seeds), Tp, B, F, H, Le, Ld, 3))
        if len(_step_ref_cache) > 4:
            _step_ref_cache.clear()
        _step_ref_cache[key] = (ref.detach(), float(loss_ref), g_ref, gn_ref, after, ref0, refw)
    ref, loss_ref, g_ref, gn_ref, after, ref0, refw = _step_ref_cache[key]
    out = out.detach().cpu()
    assert maxerr(out, ref) <= 1e-4, maxerr(out, ref)
    assert torch.equal(out.argmax(-1), ref.argmax(-1))
    np.testing.assert_allclose(float(loss.detach()), loss_ref, rtol=1e-5)
    assert maxerr(out, ref0) > 1e-2 and maxerr(out, refw) > 1e-2     # dropout acted; other decisions do not fit
    for kk, gr in g_ref.items():
        if kk == NOISE_KEY:
            continue
        tol = (1e-4 if gemm_precision == 'fp32' else 3e-4) * max(float(gr.abs().max()), 1e-6)
        assert maxerr(grads[kk], gr) <= tol, (kk, maxerr(grads[kk], gr), tol)
    np.testing.assert_allclose(float(opt.grad_norm()), gn_ref, rtol=2e-4)
    sd_after = m.state_dict()
    for kk, q in m.named_parameters():
        if kk == NOISE_KEY:
            continue
        got, want = q.detach().cpu().double().numpy(), after[kk].numpy()
        gr = g_ref[kk].abs().numpy()
        keep = gr > 1e-3 * gr.max()                           # Adam's sign step at the rounding-noise floor: excluded
        np.testing.assert_allclose(got[keep], want[keep], rtol=1e-4, atol=2e-5, err_msg=kk)
    for kk in ('temporal_conv.bn.running_mean', 'temporal_conv.bn.running_var'):
        np.testing.assert_allclose(sd_after[kk].cpu().double().numpy(), after[kk].numpy(), rtol=1e-4, atol=1e-5, err_msg=kk)
    assert int(sd_after['temporal_conv.bn.num_batches_tracked']) == int(after['temporal_conv.bn.num_batches_tracked']) == 1


def test_train_step_with_two_layer_decoder_dropout(gemm_precision, seeds):
    """tiny_relu_dec2 shape with a 2-layer encoder: conv, encoder and per-step decoder sites (1 + 1 + 3) on the composed
    decoder path (XF.dropout on the input of decoder layer 1 every step)."""
    cfg = dict(in_channels=5, n_filters=12, hidden_size=20, n_enc_layers=2, n_dec_layers=2, kernel_size=5, stride=3,
               activation=True)
    run_train_step(cfg, 40, 26, 102, 3, gemm_precision, seeds)


@pytest.mark.parametrize('name', ['configs1', 'configs3'])
def test_train_step_with_dropout_vs_fp64_oracle(name, gemm_precision, seeds):
    """The bench step with dropout on.  configs1: C = 64, H = 128 (fused dropout in the resident GRU kernels), B = 512;
    configs3: d = 30, H = 512 (cluster kernels, separate dropout pass, FMT_Y_SPLIT4 in bf16x3 mode), B = 2048 = the bench
    shard.  Weights and inputs of test_north_star_model_shape_vs_oracle."""
    xf = XF()
    if name == 'configs1':
        cfg = dict(in_channels=64, n_filters=100, hidden_size=128, n_enc_layers=2, n_dec_layers=1, kernel_size=10,
                   stride=10, activation=False)
        B = 512
        assert xf.fused_dropout_supported(20, B, 128, 2)
    else:
        cfg = dict(in_channels=30, n_filters=100, hidden_size=512, n_enc_layers=2, n_dec_layers=1, kernel_size=10,
                   stride=10, activation=False)
        B = 2048
        assert lib().xps_gru_seq_status_offset(20, B, 512, 2) >= 0
        assert xf.layer_output_split4_ok(20, B, 512, 2, P) == (gemm_precision == 'bf16x3')
    H = cfg['hidden_size']
    run_train_step(cfg, B, 200, 40 + H, H, gemm_precision, seeds)
