"""Generate tests/golden/transformer_tiny.npz by running the REFERENCE's own Transformer and CNNTransformer on CPU.

Run where a checkout of the reference is available:
    python tests/golden/make_transformer_fixtures.py <reference checkout>      (or XPS_REFERENCE_ROOT=<reference checkout>)

As in make_classifier_fixtures.py, two in-process module objects stand in for ``lightning`` and ``torchmetrics`` (logging glue
and a bincount confusion matrix only; ``optimizer_step`` of the stand-in base steps the optimiser, as Lightning's does).  Every
arithmetic op the fixtures record (Conv1d, BatchNorm1d, nn.TransformerEncoder, Linear, mean, cross_entropy, AdamW, the
positional table, the scheduler's factor) is the genuine torch / reference code.

Weights are NOT stored: `transformer_weights_from_seed` (also used by the tests).  All cases: dropout 0, B 5, T 21, 9 classes.
Per case ``<case>/...``:
  cfg, seed, x, y, keys (sorted state_dict keys joined by newlines) and shapes (one row per key, padded with -1);
  eval_logits;  train_logits, train_loss, train_acc and grads (every parameter gradient, flattened and joined in
  named_parameters() order) of ONE training_step from the seeded weights;
  bn_running_mean, bn_running_var, bn_num_batches_tracked after that step (the CNN cases only);
  step_losses: the loss of each of 5 AdamW steps (lr 1e-3, weight decay 1e-5, no clipping) from the seeded weights;
  lr_factors: CosineWarmupScheduler(warmup 5, max_iters 50).get_lr_factor(epoch) for epoch 0 .. 59;
  pos_encoding: positional_encoding.pos_encoding[:, :21, :].

A case keeps the first seed (its base seed, then +100, +200, ...) whose eval and train logits have a gap of at least MIN_MARGIN
between the two largest of every row: the tests demand the reference's argmax under a logits tolerance of 1e-4.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_classifier_fixtures import _margin, _register_glue          # noqa: E402
from transformer_weights import transformer_weights_from_seed         # noqa: E402

NUM_CLASSES, C_IN, T, B = 9, 6, 21, 5
MIN_MARGIN = 1e-3
WARMUP, MAX_ITERS = 5, 50

# positional arguments exactly as the tests pass them to the classes under test
CASES = {
    # Transformer(in_channels, num_classes, d_model, kernel_size, stride, padding, n_head, num_layers, dim_fc, dropout,
    #             learning_rate, l2_reg)
    'tr_even': dict(kind='tr', seed=301, d_model=8, n_head=2, num_layers=2, dim_fc=12),
    'tr_odd': dict(kind='tr', seed=302, d_model=9, n_head=3, num_layers=2, dim_fc=12),
    # CNNTransformer(in_channels, num_classes, d_model, kernel_size, stride, padding, n_head, num_layers, dim_fc, cnn_dropout,
    #                transformer_dropout, learning_rate, warmup, max_epochs, l2_reg)
    'cnntr_relu': dict(kind='cnn', seed=303, d_model=8, n_head=4, num_layers=2, dim_fc=12, activation=True),
    'cnntr_noact': dict(kind='cnn', seed=304, d_model=8, n_head=1, num_layers=1, dim_fc=12, activation=False),
}


def build(models, cfg):
    if cfg['kind'] == 'tr':
        return models.Transformer(cfg['d_model'], NUM_CLASSES, cfg['d_model'], 3, 1, 0, cfg['n_head'], cfg['num_layers'],
                                  cfg['dim_fc'], 0.0, 1e-3, 1e-5)
    return models.CNNTransformer(C_IN, NUM_CLASSES, cfg['d_model'], 3, 2, 0, cfg['n_head'], cfg['num_layers'], cfg['dim_fc'],
                                 0.0, 0.0, 1e-3, WARMUP, MAX_ITERS, 1e-5, activation=cfg['activation'])


def run_case(models, name, base_cfg):
    for seed in range(base_cfg['seed'], base_cfg['seed'] + 2000, 100):
        out = {}
        _run_seed(models, name, dict(base_cfg, seed=seed), out)
        margin = min(_margin(out[name + '/eval_logits']), _margin(out[name + '/train_logits']))
        if margin >= MIN_MARGIN:
            print(name, 'seed', seed, 'top-2 margin', margin)
            return out
    raise SystemExit(f'{name}: no seed with a top-2 margin of {MIN_MARGIN}')


def _run_seed(models, name, cfg, out):
    torch.manual_seed(cfg['seed'])
    model = build(models, cfg)
    sd = transformer_weights_from_seed(model.state_dict(), cfg['seed'])
    model.load_state_dict(sd)
    width = cfg['d_model'] if cfg['kind'] == 'tr' else C_IN
    rng = np.random.default_rng(cfg['seed'] + 1)
    x = torch.from_numpy(rng.standard_normal((B, T, width)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, NUM_CLASSES, (B,)))
    pre = name + '/'
    out[pre + 'cfg'] = np.array(repr(cfg))
    out[pre + 'seed'] = np.array(cfg['seed'])
    out[pre + 'x'], out[pre + 'y'] = x.numpy(), y.numpy()
    keys = sorted(model.state_dict().keys())
    out[pre + 'keys'] = np.array('\n'.join(keys))
    shapes = np.full((len(keys), 3), -1, dtype=np.int64)
    for i, k in enumerate(keys):
        shp = tuple(model.state_dict()[k].shape)
        shapes[i, :len(shp)] = shp
    out[pre + 'shapes'] = shapes
    out[pre + 'pos_encoding'] = model.positional_encoding.pos_encoding[:, :T, :].numpy().copy()
    # ---- eval-mode forward -----------------------------------------------------------------------------------------
    model.eval()
    with torch.no_grad():
        out[pre + 'eval_logits'] = model(x).numpy()
    # ---- one training_step of the reference ------------------------------------------------------------------------
    model.load_state_dict(sd)
    model.train()
    seen = {}
    hook = model.register_forward_hook(lambda m, i, o: seen.__setitem__('logits', o.detach().clone()))
    model.zero_grad()
    loss = model.training_step((x, y), 0)
    hook.remove()
    loss.backward()
    assert torch.equal(model._logged['train_loss'], loss.detach())
    out[pre + 'train_logits'] = seen['logits'].numpy()
    out[pre + 'train_loss'] = loss.detach().numpy()
    out[pre + 'train_acc'] = model._logged['train_acc'].numpy()
    out[pre + 'grads'] = np.concatenate([p.grad.numpy().reshape(-1) for _, p in model.named_parameters()])
    if cfg['kind'] == 'cnn':
        bn = model.temporal_conv.bn
        out[pre + 'bn_running_mean'] = bn.running_mean.numpy().copy()
        out[pre + 'bn_running_var'] = bn.running_var.numpy().copy()
        out[pre + 'bn_num_batches_tracked'] = bn.num_batches_tracked.numpy().copy()
    # ---- five AdamW steps on the same batch ------------------------------------------------------------------------
    model.load_state_dict(sd)
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-5)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = model.criterion(model(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    out[pre + 'step_losses'] = np.array(losses, dtype=np.float64)
    # ---- the scheduler's factor ------------------------------------------------------------------------------------
    sch = models.CosineWarmupScheduler(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=1e-3), WARMUP, MAX_ITERS)
    out[pre + 'lr_factors'] = np.array([sch.get_lr_factor(e) for e in range(60)], dtype=np.float64)


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('XPS_REFERENCE_ROOT')
    if not root:
        raise SystemExit(__doc__)
    _register_glue()
    sys.path.insert(0, os.path.join(root, 'aligned_decoding'))
    from nn_models import models                                   # the reference's module
    torch.set_num_threads(1)
    out = dict(torch_version=np.array(torch.__version__), cases=np.array(sorted(CASES)))
    for name, cfg in CASES.items():
        out.update(run_case(models, name, cfg))
    path = os.path.join(HERE, 'transformer_tiny.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
