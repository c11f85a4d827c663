"""Pin oracle/seq2seq_oracle.py to golden vectors produced by the reference's own
Seq2SeqRNN (tests/golden/make_seq2seq_fixtures.py).  CPU only."""
import ast
import os

import numpy as np
import pytest
import torch

from oracle.seq2seq_oracle import Seq2SeqOracle, cmat_acc, phoneme_error_rate, train_step
from weights import weights_from_seed

LR = 1e-3
# Adam's first step moves a weight by lr * g / (|g| + eps), eps = 1e-8, so where |g| is near zero a last-bit difference of
# the gradient moves the weight by a visible fraction of lr.  The gradients themselves agree across CPU kernels (AVX2 /
# AVX-512 / other vendors' BLAS paths: <= 5e-9 measured), but the updated value of such an element does not: the conv bias
# (it feeds a train-mode BatchNorm, so its gradient is analytically zero and numerically rounding noise) and single
# elements of the weight matrices.  Elements whose reference gradient is >= ADAM_STABLE_GRAD are held to the full
# tolerance; the others to the bound of the step itself (< lr on each side).
ADAM_STABLE_GRAD = 1e-6
NOISE_KEY = 'temporal_conv.conv.bias'


def build(g):
    cfg = ast.literal_eval(str(g['cfg']))
    m = Seq2SeqOracle(cfg['in_channels'], cfg['n_filters'], cfg['hidden_size'], 9, cfg['n_enc_layers'],
                      cfg['n_dec_layers'], cfg['kernel_size'], cfg['stride'], 0, 0.0, 0.0,
                      learning_rate=LR, l2_reg=1e-5, activation=cfg['activation'], decay_iters=5)
    sd = weights_from_seed(m.state_dict(), int(g['seed']))
    m.load_state_dict(sd)
    return m, sd


@pytest.mark.parametrize('name', ['tiny', 'tiny_relu_dec2', 'cfg2'])
def test_eval_forward_matches_reference(golden_dir, name):
    torch.set_num_threads(1)
    g = np.load(os.path.join(golden_dir, f'seq2seq_{name}.npz'))
    m, _ = build(g)
    m.eval()
    x, y = torch.from_numpy(g['x']), torch.from_numpy(g['y'])
    with torch.no_grad():
        logits = m(x, y, teacher_forcing_ratio=0)
    np.testing.assert_allclose(logits.numpy(), g['eval_logits'], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(logits.argmax(-1).numpy(), g['eval_argmax'])
    np.testing.assert_allclose(cmat_acc(logits.view(-1, 9), y.view(-1), 9).numpy(), g['eval_acc'])


@pytest.mark.parametrize('name', ['tiny', 'tiny_relu_dec2', 'cfg2'])
@pytest.mark.parametrize('tag,coin', [('tf1', True), ('tf0', False)])
def test_train_step_matches_reference(golden_dir, name, tag, coin):
    torch.set_num_threads(1)
    g = np.load(os.path.join(golden_dir, f'seq2seq_{name}.npz'))
    m, sd = build(g)
    x, y = torch.from_numpy(g['x']), torch.from_numpy(g['y'])
    opt, _ = m.make_optimizer()
    loss, logits = train_step(m, opt, x, y, coins=[coin] * 3, clip=0.5)
    np.testing.assert_allclose(loss.numpy(), g[f'{tag}_loss'], rtol=1e-6)
    np.testing.assert_allclose(logits.numpy(), g[f'{tag}_logits'], atol=1e-6)
    grads = dict(m.named_parameters())
    if f'{tag}_grad/decoder.fc_out.weight' in g:
        for k, p in grads.items():
            np.testing.assert_allclose(p.grad.numpy(), g[f'{tag}_grad/{k}'], rtol=1e-4, atol=1e-7)
        for k, v in m.state_dict().items():
            got, ref = v.numpy(), g[f'{tag}_after/{k}']
            gr = np.abs(g[f'{tag}_grad/{k}']) if f'{tag}_grad/{k}' in g else np.full(ref.shape, np.inf)
            stable = gr >= ADAM_STABLE_GRAD
            np.testing.assert_allclose(got[stable], ref[stable], rtol=1e-5, atol=1e-7, err_msg=k)
            assert np.all(np.abs(got[~stable] - ref[~stable]) <= 2 * LR), k
    else:
        for k, p in grads.items():
            # (atol: the conv bias's gradient norm is ~3e-9 of rounding noise; every other norm is orders above it)
            np.testing.assert_allclose(p.grad.norm().numpy(), g[f'{tag}_gradnorm/{k}'], rtol=1e-4, atol=1e-7, err_msg=k)
        sd_after = m.state_dict()
        after = np.array([v.double().sum().item() for v in sd_after.values()])
        ref = g[f'{tag}_after_sum']
        # sums over up to 1e5 elements, a few hundred of them with near-zero gradients: lr / 5 is below one element's step
        # gone the other way (up to 2 lr) and above what those elements add across CPU kernels (<= 5e-5 measured); the
        # conv bias, every element of it at the noise floor, is held to the step bound
        atol = np.array([2 * LR * v.numel() if k == NOISE_KEY else LR / 5 for k, v in sd_after.items()])
        bad = np.abs(after - ref) > atol + 1e-6 * np.abs(ref)
        assert not bad.any(), [(k, after[i], ref[i]) for i, k in enumerate(sd_after) if bad[i]]


def test_state_dict_keys_are_the_reference_keys():
    m = Seq2SeqOracle(6, 8, 16, 9, 2, 1, 4, 4)
    keys = set(m.state_dict().keys())
    for k in ['temporal_conv.conv.weight', 'temporal_conv.bn.running_var', 'temporal_conv.bn.num_batches_tracked',
              'encoder.rnn.weight_ih_l0', 'encoder.rnn.weight_hh_l1_reverse', 'encoder.rnn.bias_hh_l0_reverse',
              'decoder.embedding.weight', 'decoder.rnn.bias_ih_l0', 'decoder.fc_out.bias']:
        assert k in keys


def test_per_definition():
    assert phoneme_error_rate([[1, 2, 3]], [[1, 2, 3]]) == 0.0
    assert phoneme_error_rate([[1, 2, 3], [4, 5, 6]], [[1, 9, 3], [5, 6, 7]]) == pytest.approx(100 * 3 / 6)


def _ones_masks(m, B, Tp):
    F, H = m.temporal_conv.conv.out_channels, m.encoder.rnn.hidden_size
    L, Ld = m.encoder.rnn.num_layers, m.decoder.rnn.num_layers
    return {'conv': torch.ones(B, F, Tp, dtype=torch.float64), 'enc': [torch.ones(B, Tp, 2 * H, dtype=torch.float64)] * (L - 1),
            'dec': [[torch.ones(B, H, dtype=torch.float64)] * (Ld - 1)] * m.seq_length}


@pytest.mark.parametrize('name', ['tiny', 'tiny_relu_dec2', 'cfg2'])
def test_all_ones_masks_give_the_unmasked_oracle(golden_dir, name):
    """Explicit masks of ones at p = 0: the layer-by-layer GRUs give what nn.GRU gives, and the reference goldens hold."""
    torch.set_num_threads(1)
    g = np.load(os.path.join(golden_dir, f'seq2seq_{name}.npz'))
    x, y = torch.from_numpy(g['x']), torch.from_numpy(g['y'])
    m, sd = build(g)
    m.eval()
    cfg = ast.literal_eval(str(g['cfg']))
    Tp = (x.shape[1] - cfg['kernel_size']) // cfg['stride'] + 1
    with torch.no_grad():
        plain = m(x, y, teacher_forcing_ratio=0)
        m.double()
        masked = m(x.double(), y, teacher_forcing_ratio=0, masks=_ones_masks(m, x.shape[0], Tp))
    assert masked.dtype == torch.float64
    np.testing.assert_allclose(masked.numpy(), plain.double().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(masked.numpy(), g['eval_logits'], rtol=0, atol=1e-6)
    # a training step in float64 through the masked path against the reference's fp32 goldens
    m2, _ = build(g)
    m2.double()
    opt, _ = m2.make_optimizer()
    loss, logits = train_step(m2, opt, x.double(), y, coins=[True] * 3, clip=0.5, masks=_ones_masks(m2, x.shape[0], Tp))
    np.testing.assert_allclose(loss.numpy(), g['tf1_loss'], rtol=1e-5)
    np.testing.assert_allclose(logits.numpy(), g['tf1_logits'], atol=2e-6)


@pytest.mark.parametrize('ndir,L', [(2, 2), (2, 3), (1, 3)])
def test_masked_gru_is_per_layer_gru_with_the_mask_in_between(ndir, L):
    """gru_masked == hand-composed one-layer nn.GRUs (copied weights) with x * mask / (1 - p) between them, forward and
    backward, in float64; and it is not the undropped GRU."""
    from oracle.seq2seq_oracle import gru_masked
    torch.manual_seed(3)
    B, T, In, H, p = 5, 7, 6, 8, 0.3
    rnn = torch.nn.GRU(In, H, L, batch_first=True, dropout=p, bidirectional=ndir == 2).double()
    x = torch.randn(B, T, In, dtype=torch.float64)
    h0 = torch.randn(L * ndir, B, H, dtype=torch.float64)
    masks = [(torch.rand(B, T, ndir * H) >= p).double() for _ in range(L - 1)]
    assert all(0 < m.mean() < 1 for m in masks)
    wt = torch.randn(B, T, ndir * H, dtype=torch.float64)
    out, hn = gru_masked(rnn, x, h0, masks)
    (out * wt).sum().backward()
    inp, hs, layers = x, [], []
    for l in range(L):
        one = torch.nn.GRU(In if l == 0 else ndir * H, H, 1, batch_first=True, bidirectional=ndir == 2).double()
        with torch.no_grad():
            for sfx in [''] + (['_reverse'] if ndir == 2 else []):
                for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'):
                    getattr(one, f'{n}_l0{sfx}').copy_(getattr(rnn, f'{n}_l{l}{sfx}'))
        o, h = one(inp, h0[l * ndir:(l + 1) * ndir])
        hs.append(h)
        layers.append(one)
        inp = o * masks[l] / (1 - p) if l < L - 1 else o
    (inp * wt).sum().backward()
    torch.testing.assert_close(out, inp, rtol=0, atol=1e-12)
    torch.testing.assert_close(hn, torch.cat(hs, 0), rtol=0, atol=1e-12)
    for l, one in enumerate(layers):
        for sfx in [''] + (['_reverse'] if ndir == 2 else []):
            for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'):
                torch.testing.assert_close(getattr(rnn, f'{n}_l{l}{sfx}').grad, getattr(one, f'{n}_l0{sfx}').grad,
                                           rtol=0, atol=1e-11)
    with torch.no_grad():
        plain, _ = rnn(x, h0)
    assert (plain - out).abs().max() > 1e-3                 # the masks did act
