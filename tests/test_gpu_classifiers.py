"""Single-label classifiers on the device: the max-over-time kernels, the one-launch classification step, SimpleGRU,
TemporalConvRNN and TCN_classifier against torch on the CPU and against the goldens recorded from the reference's own classes
(tests/golden/make_classifier_fixtures.py)."""
import ast
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from weights import weights_from_seed  # noqa: E402

SENTINEL = -12345.5
CASES = ['rnn_none', 'rnn_int', 'rnn_list', 'tcn_relu', 'tcn_noact']
NUM_CLASSES, C_IN = 9, 6


# --------------------------------------------------------------------------- #
# time_max                                                                      #
# --------------------------------------------------------------------------- #
TM_SHAPES = [(1, 1, 1), (2, 3, 7), (10, 5, 100), (199, 4, 64), (3, 130, 260)]


def _tm_input(shape, kind):
    T, B, F = shape
    rng = np.random.default_rng(T * 1000 + B * 10 + F)
    if kind == 'normal':
        z = rng.standard_normal(shape).astype(np.float32)
    elif kind == 'ties':                            # integer-valued: most columns tie; one all-zero column (post-ReLU)
        z = rng.integers(0, 3, shape).astype(np.float32)
        z[:, 0, 0] = 0.0
    else:                                           # NaNs at known places
        z = rng.standard_normal(shape).astype(np.float32)
        z[0, 0, 0] = np.nan                         # a column with two NaNs: the first wins
        z[T - 1, 0, 0] = np.nan
        z[0, B - 1, F - 1] = 50.0                   # a NaN after a larger finite value: the NaN wins
        z[T - 1, B - 1, F - 1] = np.nan
    return torch.from_numpy(z)


def _guarded(t):
    """Device copy of t (leading axis = rows) inside a sentinel-filled buffer with one guard row on each side."""
    buf = torch.full((t.shape[0] + 2,) + tuple(t.shape[1:]), SENTINEL, dtype=t.dtype, device='cuda')
    buf[1:-1].copy_(t)
    return buf, buf[1:-1]


def _guards_intact(buf):
    return bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())


@pytest.mark.parametrize('shape,kind', [(s, 'normal') for s in TM_SHAPES]
                         + [(TM_SHAPES[1], 'ties'), (TM_SHAPES[0], 'ties'), (TM_SHAPES[2], 'ties')]
                         + [(TM_SHAPES[1], 'nan'), (TM_SHAPES[2], 'nan')])
def test_time_max_equals_torch_max_on_cpu(shape, kind):
    from cross_patient_speech_decoding_amd._lib import call
    from cross_patient_speech_decoding_amd.nn_models import functional as XF
    T, B, F = shape
    z = _tm_input(shape, kind)
    zc = z.clone().requires_grad_(True)
    ref_v, ref_i = torch.max(zc, dim=0)
    dout = torch.from_numpy(np.random.default_rng(5).standard_normal((B, F)).astype(np.float32))
    ref_v.backward(dout)
    if kind == 'nan':                               # the reference itself obeys the rule the kernel is written to
        assert ref_i[0, 0] == 0 and ref_i[B - 1, F - 1] == T - 1 and torch.isnan(ref_v[0, 0])
    # autograd path
    zbuf, zg = _guarded(z)
    zg = zg.detach().requires_grad_(True)
    out, arg = XF.time_max(zg, return_indices=True)
    assert out.shape == (B, F) and arg.dtype == torch.int32 and not arg.requires_grad
    assert torch.equal(out.detach().cpu().view(torch.int32), ref_v.detach().view(torch.int32))     # a selection: the same bits
    assert torch.equal(arg.cpu().long(), ref_i)
    out.backward(dout.cuda())
    assert torch.equal(zg.grad.cpu(), zc.grad)
    assert _guards_intact(zbuf)
    # raw entry points on guarded outputs: nothing outside out / arg / dz is written, every element inside is
    out_buf, out_g = _guarded(torch.zeros(1, B * F))
    arg_buf = torch.full((3, B * F), -7, dtype=torch.int32, device='cuda')
    s = torch.cuda.current_stream().cuda_stream
    call('xps_time_max_fwd_f32', zbuf[1:-1].data_ptr(), out_g.data_ptr(), arg_buf[1].data_ptr(), T, B, F, s)
    assert _guards_intact(out_buf) and bool((arg_buf[0] == -7).all()) and bool((arg_buf[2] == -7).all())
    assert torch.equal(out_g.view(B, F).cpu().view(torch.int32), ref_v.detach().view(torch.int32))
    assert torch.equal(arg_buf[1].view(B, F).cpu().long(), ref_i)
    dz_buf, dz_g = _guarded(torch.full((T, B, F), 777.0))            # stale contents: the kernel must overwrite all of it
    call('xps_time_max_bwd_f32', dout.cuda().data_ptr(), arg_buf[1].data_ptr(), dz_g.data_ptr(), T, B, F, s)
    assert _guards_intact(dz_buf)
    assert torch.equal(dz_g.cpu(), zc.grad)


@pytest.mark.parametrize('which', ['z', 'out', 'arg', 'dz'])
def test_time_max_four_byte_path_for_each_misaligned_pointer(which):
    """F % 4 == 0 but one pointer is only 4-byte aligned: the 4-byte path of the forward (z, out or arg misaligned) and of
    the backward (dz misaligned), same results, nothing written outside."""
    from cross_patient_speech_decoding_amd._lib import call
    T, B, F = 5, 67, 8                              # 536 columns: several workgroups, the last one partly idle
    z = _tm_input((T, B, F), 'ties')
    zc = z.clone().requires_grad_(True)
    ref_v, ref_i = torch.max(zc, dim=0)
    dout = torch.from_numpy(np.random.default_rng(6).standard_normal((B, F)).astype(np.float32))
    ref_v.backward(dout)
    st = torch.cuda.current_stream().cuda_stream

    def region(n, dtype, fill, shifted):
        """n elements inside a sentinel-filled buffer, 16-byte aligned or shifted by one 4-byte element."""
        buf = torch.full((n + 8,), fill, dtype=dtype, device='cuda')
        off = 5 if shifted else 4
        assert (buf[off:].data_ptr() % 16 == 0) != shifted
        return buf, buf[off:off + n], off

    zbuf, zv, zo = region(T * B * F, torch.float32, SENTINEL, which == 'z')
    zv.copy_(z.reshape(-1))
    obuf, ov, oo = region(B * F, torch.float32, SENTINEL, which == 'out')
    abuf, av, ao = region(B * F, torch.int32, -7, which == 'arg')
    call('xps_time_max_fwd_f32', zv.data_ptr(), ov.data_ptr(), av.data_ptr(), T, B, F, st)
    assert torch.equal(ov.view(B, F).cpu(), ref_v.detach()) and torch.equal(av.view(B, F).cpu().long(), ref_i)
    for buf, off, n, fill in ((zbuf, zo, T * B * F, SENTINEL), (obuf, oo, B * F, SENTINEL), (abuf, ao, B * F, -7)):
        assert bool((buf[:off] == fill).all()) and bool((buf[off + n:] == fill).all())
    dbuf, dv, do = region(T * B * F, torch.float32, SENTINEL, which == 'dz')
    call('xps_time_max_bwd_f32', dout.cuda().data_ptr(), av.data_ptr(), dv.data_ptr(), T, B, F, st)
    assert torch.equal(dv.view(T, B, F).cpu(), zc.grad)
    assert bool((dbuf[:do] == SENTINEL).all()) and bool((dbuf[do + T * B * F:] == SENTINEL).all())


# --------------------------------------------------------------------------- #
# classify_loss_acc                                                             #
# --------------------------------------------------------------------------- #
def _classify_input(rows, C, kind):
    rng = np.random.default_rng(rows * 100 + C)
    if kind == 'ties':                              # integer logits: tied row maxima, the first index must win
        logits = rng.integers(0, 3, (rows, C)).astype(np.float32)
    else:
        logits = (2.0 * rng.standard_normal((rows, C))).astype(np.float32)
    target = rng.integers(0, C, (rows,))
    if kind == 'one_class':
        target[:] = C - 1
    return torch.from_numpy(logits), torch.from_numpy(target)


def _cmat_cpu(logits, target, C):
    pred = torch.argmax(logits, dim=1)
    return torch.bincount(target * C + pred, minlength=C * C).view(C, C)


@pytest.mark.parametrize('rows,C,kind', [(1, 9, 'normal'), (5, 9, 'normal'), (300, 2, 'normal'), (2049, 9, 'normal'),
                                         (64, 40, 'normal'), (300, 2, 'ties'), (2049, 9, 'ties'), (64, 40, 'one_class')])
def test_classify_loss_acc_equals_cross_entropy_and_cmat(rows, C, kind):
    from cross_patient_speech_decoding_amd.nn_models import cmat_acc
    from cross_patient_speech_decoding_amd.nn_models import functional as XF
    logits, target = _classify_input(rows, C, kind)
    a = logits.cuda().requires_grad_(True)
    b = logits.cuda().requires_grad_(True)
    tg = target.cuda()
    loss_ref = XF.cross_entropy(a, tg)
    loss_ref.backward()
    loss, acc, cmat = XF.classify_loss_acc(b, tg, C)
    assert loss.requires_grad and not acc.requires_grad and not cmat.requires_grad
    assert cmat.dtype == torch.int64 and cmat.shape == (C, C) and acc.dtype == torch.float32
    loss.backward()
    assert torch.equal(loss.detach(), loss_ref.detach())                      # bit-identical loss ...
    assert torch.equal(b.grad, a.grad)                                       # ... and gradient
    ref_cm = _cmat_cpu(logits, target, C)
    assert torch.equal(cmat.cpu(), ref_cm)
    assert int(cmat.sum()) == rows
    assert acc.cpu().item() == cmat_acc(logits, target, C).item()            # exactly trace / rows in fp32
    # a second call on the same stream: the ticket was left at zero, the matrix is overwritten, not accumulated
    loss2, acc2, cmat2 = XF.classify_loss_acc(b.detach(), tg, C)
    assert torch.equal(loss2, loss.detach()) and torch.equal(cmat2, cmat) and torch.equal(acc2, acc)
    # resident unit gradient: returned unscaled, same bits
    c = logits.cuda().requires_grad_(True)
    l3, _, _ = XF.classify_loss_acc(c, tg, C)
    l3.backward(XF.unit_gradient(l3.device))
    assert torch.equal(c.grad, a.grad)


def test_classify_workspace_shared_across_class_counts_and_with_cross_entropy():
    """One stream, one workspace, several blocks: calls with different class counts and row counts, and the fused
    cross-entropy between them, follow one another; every result is that of a fresh computation on the CPU."""
    from cross_patient_speech_decoding_amd.nn_models import cmat_acc
    from cross_patient_speech_decoding_amd.nn_models import functional as XF
    seq = [(2049, 40, 'normal'), (2049, 2, 'ties'), (700, 9, 'normal'), (2049, 2, 'normal'), (1025, 40, 'one_class'), (513, 3, 'ties')]
    for rep in range(2):
        for rows, C, kind in seq:
            logits, target = _classify_input(rows + rep, C, kind)
            lg, tg = logits.cuda(), target.cuda()
            loss, acc, cmat = XF.classify_loss_acc(lg, tg, C)
            ce = XF.cross_entropy(lg, tg)                                    # same workspace, same ticket word
            assert torch.equal(cmat.cpu(), _cmat_cpu(logits, target, C)), (rows, C, kind)
            assert acc.cpu().item() == cmat_acc(logits, target, C).item()
            assert torch.equal(loss, ce)


def test_classify_evaluation_form_writes_no_gradient():
    """dlogits = NULL: loss, accuracy and matrix as in the training form, and nothing outside the outputs is written."""
    from cross_patient_speech_decoding_amd._lib import call, lib
    from cross_patient_speech_decoding_amd.nn_models import functional as XF
    rows, C = 300, 9
    logits, target = _classify_input(rows, C, 'normal')
    lg, tg = logits.cuda(), target.cuda()
    with torch.no_grad():
        loss_e, acc_e, cmat_e = XF.classify_loss_acc(lg, tg, C)
    assert not loss_e.requires_grad
    loss_t, acc_t, cmat_t = XF.classify_loss_acc(lg.clone().requires_grad_(True), tg, C)
    assert torch.equal(loss_e, loss_t.detach()) and torch.equal(acc_e, acc_t) and torch.equal(cmat_e, cmat_t)
    # raw call, every output carved from one sentinel-filled arena (float32 words) with gaps between them
    gap = 64
    n_cm = 2 * C * C                                                   # int64 matrix = 2 words per cell
    arena = torch.full((gap + rows + gap + 2 + gap + 2 + gap + n_cm + gap + rows * C + gap,), SENTINEL, device='cuda')
    o_rl = gap
    o_loss = o_rl + rows + gap
    o_acc = o_loss + 2 + gap
    o_cm = o_acc + 2 + gap
    o_dl = o_cm + n_cm + gap                                           # where a gradient WOULD go: stays sentinel
    assert (arena[o_cm:].data_ptr() % 8) == 0
    nbytes = lib().xps_classify_loss_acc_f32_workspace(rows)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
    base = arena.data_ptr()
    call('xps_classify_loss_acc_f32', lg.data_ptr(), tg.data_ptr(), base + 4 * o_rl, base + 4 * o_loss, None, base + 4 * o_cm,
         base + 4 * o_acc, ws.data_ptr(), ws.numel(), rows, C, torch.cuda.current_stream().cuda_stream)
    written = torch.zeros_like(arena, dtype=torch.bool)
    written[o_rl:o_rl + rows] = True
    written[o_loss] = True
    written[o_acc] = True
    written[o_cm:o_cm + n_cm] = True
    assert bool((arena[~written] == SENTINEL).all())
    assert bool((arena[o_dl:o_dl + rows * C] == SENTINEL).all())
    assert arena[o_loss].item() == loss_e.item() and arena[o_acc].item() == acc_e.item()
    assert torch.equal(arena[o_cm:o_cm + n_cm].view(torch.int64).view(C, C), cmat_e)
    assert int(ws.view(torch.int32)[0]) == 0                           # ticket left at zero


# --------------------------------------------------------------------------- #
# models against the goldens of the reference                                   #
# --------------------------------------------------------------------------- #
@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'classifiers_tiny.npz'))


def build_case(cfg, dropout=0.0):
    from cross_patient_speech_decoding_amd.nn_models import TCN_classifier, TemporalConvRNN
    if cfg['kind'] == 'rnn':
        m = TemporalConvRNN(C_IN, 8, NUM_CLASSES, 16, 2, 3, cfg['dim_fc'], 2, 0, dropout, dropout, 1e-3, 1e-5,
                            activation=cfg['activation'], decay_iters=5)
    else:
        m = TCN_classifier(C_IN, NUM_CLASSES, cfg['dim_fc'], 3, 2, 0, dropout, 1e-3, 1e-5, activation=cfg['activation'])
    m.load_state_dict(weights_from_seed(m.state_dict(), cfg['seed']))
    return m.to('cuda')


def _grad_tolerance(key):
    """The project's tolerances for the same quantities of Seq2SeqRNN (tests/test_gpu_nn_kernels.py): GRU weight gradients
    atol 1e-4 / rtol 1e-3, conv and BN gradients atol 2e-4 / rtol 1e-3; the Linear heads (plain GEMM results of the same
    magnitude as the GRU weight gradients) take the tighter of the two."""
    if key.startswith('temporal_conv.'):
        return dict(atol=2e-4, rtol=1e-3)
    return dict(atol=1e-4, rtol=1e-3)


@pytest.mark.parametrize('case', CASES)
def test_models_match_reference_golden(golden, case, gemm_precision):
    cfg = ast.literal_eval(str(golden[f'{case}/cfg']))
    g = {k[len(case) + 1:]: golden[k] for k in golden.files if k.startswith(case + '/')}
    x, y = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['y']).cuda()
    m = build_case(cfg).eval()
    with torch.no_grad():
        logits = m(x)
    assert logits.shape == (x.shape[0], NUM_CLASSES)
    err = np.abs(logits.cpu().numpy() - g['eval_logits']).max()
    assert err <= 1e-4, err
    np.testing.assert_array_equal(logits.argmax(-1).cpu().numpy(), g['eval_logits'].argmax(-1))
    with torch.no_grad():
        pred = m.predict_step((x, y), 0)
    assert torch.equal(pred, logits)
    # one training_step from the seeded weights
    m = build_case(cfg).train()
    seen = {}
    hook = m.register_forward_hook(lambda mod, i, o: seen.__setitem__('logits', o.detach().clone()))
    m._xps_logged = {}
    loss = m.training_step((x, y), 0)
    hook.remove()
    loss.backward()
    train_logits = seen['logits'].cpu().numpy()
    err = np.abs(train_logits - g['train_logits']).max()
    assert err <= 1e-4, err
    np.testing.assert_array_equal(train_logits.argmax(-1), g['train_logits'].argmax(-1))
    np.testing.assert_allclose(loss.item(), float(g['train_loss']), rtol=2e-5)
    assert set(m._xps_logged) == {'train_loss', 'train_acc'}
    assert float(m._xps_logged['train_acc']) == float(g['train_acc'])
    assert float(m._xps_logged['train_loss']) == loss.item()
    at = 0
    for k, p in m.named_parameters():                 # 'grads': flattened and joined in this order
        assert p.grad is not None, k
        ref = g['grads'][at:at + p.numel()].reshape(tuple(p.shape))
        at += p.numel()
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref, err_msg=k, **_grad_tolerance(k))
    assert at == g['grads'].size
    bn = m.temporal_conv.bn
    np.testing.assert_allclose(bn.running_mean.cpu().numpy(), g['bn_running_mean'], atol=1e-6, rtol=0)
    np.testing.assert_allclose(bn.running_var.cpu().numpy(), g['bn_running_var'], atol=1e-5, rtol=0)
    assert int(bn.num_batches_tracked) == int(g['bn_num_batches_tracked']) == 1


@pytest.mark.parametrize('case', CASES)
def test_five_adamw_steps_follow_reference_losses(golden, case):
    """torch.optim.AdamW on the device parameters (lr 1e-3, weight decay 1e-5, no clipping), the same batch five times:
    the loss of every step against the reference's, at the relative tolerance tests/test_gpu_seq2seq.py applies to a
    step's loss (2e-5)."""
    cfg = ast.literal_eval(str(golden[f'{case}/cfg']))
    x = torch.from_numpy(golden[f'{case}/x']).cuda()
    y = torch.from_numpy(golden[f'{case}/y']).cuda()
    m = build_case(cfg).train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = m.criterion(m(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in losses]
    print(case, losses, list(golden[f'{case}/step_losses']))
    np.testing.assert_allclose(losses, golden[f'{case}/step_losses'], rtol=2e-5)


def test_other_criterion_takes_the_reference_route(golden):
    """A criterion that is not the plain default: criterion(y_hat, y) + cmat_acc, same logged names."""
    from cross_patient_speech_decoding_amd.nn_models import TCN_classifier
    x = torch.from_numpy(golden['tcn_relu/x']).cuda()
    y = torch.from_numpy(golden['tcn_relu/y']).cuda()
    m = TCN_classifier(C_IN, NUM_CLASSES, [8, 7], 3, 2, 0, 0.0, criterion=torch.nn.CrossEntropyLoss(label_smoothing=0.1))
    m.load_state_dict(weights_from_seed(m.state_dict(), int(golden['tcn_relu/seed'])))
    m = m.cuda().train()
    m._xps_logged = {}
    loss = m.training_step((x, y), 0)
    loss.backward()
    ref = torch.nn.functional.cross_entropy(torch.from_numpy(golden['tcn_relu/train_logits']), y.cpu(), label_smoothing=0.1)
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=2e-5)
    assert float(m._xps_logged['train_acc']) == float(golden['tcn_relu/train_acc'])


# --------------------------------------------------------------------------- #
# SimpleGRU alone against torch.nn.GRU + Linear on the CPU                      #
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('T,B,In,H,L', [(1, 3, 4, 16, 1), (7, 5, 8, 128, 2), (3, 130, 12, 320, 1)])
def test_simple_gru_vs_torch_cpu(T, B, In, H, L):
    """Tolerances of the same quantities in tests/test_gpu_nn_kernels.py: outputs 1e-4 (the logits bar), dx atol 5e-5 /
    rtol 1e-4, weight gradients atol 1e-4 / rtol 1e-3."""
    from cross_patient_speech_decoding_amd._lib import lib
    from cross_patient_speech_decoding_amd.nn_models import SimpleGRU
    from cross_patient_speech_decoding_amd.nn_models import functional as XF
    torch.set_num_threads(min(8, len(os.sched_getaffinity(0))))
    if H == 320:
        assert lib().xps_gru_seq_status_offset(T, B, H, 1) >= 0          # this shape runs the cluster recurrence
    out_size = 5
    m = SimpleGRU(In, H, out_size, L, dropout=0.0)
    m.load_state_dict(weights_from_seed(m.state_dict(), 300 + H))
    gru = torch.nn.GRU(In, H, L, batch_first=True)
    fc = torch.nn.Linear(H, out_size)
    gru.load_state_dict({k[4:]: v.clone() for k, v in m.state_dict().items() if k.startswith('gru.')})
    fc.load_state_dict({k[3:]: v.clone() for k, v in m.state_dict().items() if k.startswith('fc.')})
    rng = np.random.default_rng(T + H)
    x = torch.from_numpy(rng.standard_normal((B, T, In)).astype(np.float32))
    w = torch.from_numpy(rng.standard_normal((B, out_size)).astype(np.float32)) / B
    xr = x.clone().requires_grad_(True)
    ref = fc(gru(xr)[0][:, -1, :])
    (ref * w).sum().backward()
    m = m.cuda().train()
    xg = x.cuda().requires_grad_(True)
    out = m(xg)
    (out * w.cuda()).sum().backward()
    XF.check_gru_status()
    assert out.shape == (B, out_size)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=1e-4, rtol=0)
    np.testing.assert_allclose(xg.grad.cpu().numpy(), xr.grad.numpy(), atol=5e-5, rtol=1e-4)
    refs = {**{'gru.' + k: p for k, p in gru.named_parameters()}, **{'fc.' + k: p for k, p in fc.named_parameters()}}
    for k, p in m.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), refs[k].grad.numpy(), atol=1e-4, rtol=1e-3, err_msg=k)
    # the time-major entry gives the same bits
    with torch.no_grad():
        assert torch.equal(m.forward_tm(x.cuda().permute(1, 0, 2).contiguous()), m(x.cuda()))


# --------------------------------------------------------------------------- #
# dropout on, trainer                                                           #
# --------------------------------------------------------------------------- #
def _dropout_model(kind, p):
    from cross_patient_speech_decoding_amd.nn_models import TCN_classifier, TemporalConvRNN
    if kind == 'rnn':
        return TemporalConvRNN(C_IN, 8, NUM_CLASSES, 16, 2, 3, [12], 2, 0, p, p)
    return TCN_classifier(C_IN, NUM_CLASSES, [8, 7], 3, 2, 0, p)


@pytest.mark.parametrize('kind', ['rnn', 'tcn'])
def test_dropout_training_is_finite_and_reproducible(kind):
    from cross_patient_speech_decoding_amd.nn_models import functional as XF
    from cross_patient_speech_decoding_amd.nn_models.trainer import seed_everything
    rng = np.random.default_rng(17)
    x = torch.from_numpy(rng.standard_normal((33, 21, C_IN)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.integers(0, NUM_CLASSES, (33,))).cuda()

    def run():
        seed_everything(11)
        XF._DROP_COUNTER[0] = 0
        m = _dropout_model(kind, 0.3).cuda().train()
        loss = m.training_step((x, y), 0)
        loss.backward()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}, m

    la, ga, m = run()
    lb, gb, _ = run()
    assert torch.isfinite(la)
    for k in ga:
        assert torch.isfinite(ga[k]).all(), k
        assert torch.equal(ga[k], gb[k]), k
    assert torch.equal(la, lb)
    # eval() does not depend on the dropout rates
    m0 = _dropout_model(kind, 0.0)
    m0.load_state_dict(m.state_dict())
    m0 = m0.cuda().eval()
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x), m0(x))


@pytest.mark.parametrize('kind', ['rnn', 'tcn'])
def test_trainer_fit_logs_loss_and_accuracy(kind):
    from cross_patient_speech_decoding_amd.nn_models.trainer import Trainer, seed_everything
    seed_everything(3)
    rng = np.random.default_rng(23)
    X = torch.from_numpy(rng.standard_normal((40, 21, C_IN)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, NUM_CLASSES, (40,)))
    loader = [(X[:20], y[:20]), (X[20:], y[20:])]
    model = _dropout_model(kind, 0.1)
    trainer = Trainer(max_epochs=2)
    trainer.fit(model, loader, loader)
    m = trainer.logged_metrics
    for k in ('train_loss', 'train_acc', 'val_loss', 'val_acc'):
        assert k in m and np.isfinite(m[k]), k
    assert 0.0 <= m['train_acc'] <= 1.0 and 0.0 <= m['val_acc'] <= 1.0
    outs = trainer.predict(model, loader)
    assert len(outs) == 2 and outs[0].shape == (20, NUM_CLASSES)
