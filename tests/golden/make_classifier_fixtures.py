"""Generate tests/golden/classifiers_tiny.npz by running the REFERENCE's own TemporalConvRNN and TCN_classifier on CPU.

Run where a checkout of the reference is available:
    python tests/golden/make_classifier_fixtures.py <reference checkout>      (or XPS_REFERENCE_ROOT=<reference checkout>)

As in make_seq2seq_fixtures.py, ``nn_models/models.py`` imports ``lightning`` and ``torchmetrics``; two in-process module
objects stand in for them (logging glue and a bincount confusion matrix only).  Here ``log_dict`` keeps what the step
logged, so the recorded loss and accuracy are the ones the reference's own ``training_step`` computed.  Every arithmetic op
the fixtures record (Conv1d, BatchNorm1d, GRU, Linear, torch.max, cross_entropy, AdamW) is the genuine torch code the
reference calls.

Weights are NOT stored: they are drawn from numpy's PCG64 (`weights_from_seed`, also used by the tests) and loaded with
load_state_dict, so a case holds seed + inputs + outputs.  All cases run with dropout 0.  Per case ``<case>/...``:
  cfg, seed, x, y, keys (the sorted state_dict keys joined by newlines) and shapes (one row per key, padded with -1);
  eval_logits;  train_logits, train_loss, train_acc and grads (every parameter gradient, flattened and joined in
  named_parameters() order) of ONE training_step from the seeded weights;
  bn_running_mean, bn_running_var, bn_num_batches_tracked after that step;
  step_losses: the loss of each of 5 AdamW steps (lr 1e-3, weight decay 1e-5, no clipping) from the seeded weights.

The tests demand the reference's argmax under a logits tolerance of 1e-4, so a case keeps the first seed (its base seed, then
+100, +200, ...) whose eval and train logits have a gap of at least MIN_MARGIN between the two largest of every row.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from weights import weights_from_seed          # noqa: E402


def _register_glue():
    L = types.ModuleType('lightning')

    class LightningModule(torch.nn.Module):
        def log(self, name, value, *a, **k):
            self.__dict__.setdefault('_logged', {})[name] = value.detach().clone()

        def log_dict(self, d, *a, **k):
            for name, value in d.items():
                self.log(name, value)

        def save_hyperparameters(self, *a, **k):
            pass
    L.LightningModule = LightningModule
    sys.modules['lightning'] = L
    tm = types.ModuleType('torchmetrics')
    tmf = types.ModuleType('torchmetrics.functional')
    tmc = types.ModuleType('torchmetrics.functional.classification')

    def multiclass_confusion_matrix(preds, target, num_classes):
        return torch.bincount(target * num_classes + preds,
                              minlength=num_classes ** 2).view(num_classes, num_classes)
    tmc.multiclass_confusion_matrix = multiclass_confusion_matrix
    tm.functional, tmf.classification = tmf, tmc
    sys.modules.update({'torchmetrics': tm, 'torchmetrics.functional': tmf,
                        'torchmetrics.functional.classification': tmc})


NUM_CLASSES, C_IN, T, B = 9, 6, 21, 5
MIN_MARGIN = 1e-3          # ten times the logits tolerance of the tests

# positional arguments exactly as the tests pass them to the classes under test
CASES = {
    # TemporalConvRNN(in_channels, n_filters, num_classes, hidden_size, n_layers, kernel_size, dim_fc, stride, padding,
    #                 cnn_dropout, rnn_dropout, learning_rate, l2_reg)
    'rnn_none': dict(kind='rnn', seed=201, dim_fc=None, activation=True),
    'rnn_int': dict(kind='rnn', seed=202, dim_fc=12, activation=True),
    'rnn_list': dict(kind='rnn', seed=203, dim_fc=[12, 10], activation=True),
    # TCN_classifier(in_channels, num_classes, dim_fc, kernel_size, stride, padding, dropout, learning_rate, l2_reg)
    'tcn_relu': dict(kind='tcn', seed=204, dim_fc=[8, 7], activation=True),
    'tcn_noact': dict(kind='tcn', seed=205, dim_fc=[8, 7], activation=False),
}


def build(models, cfg):
    if cfg['kind'] == 'rnn':
        return models.TemporalConvRNN(C_IN, 8, NUM_CLASSES, 16, 2, 3, cfg['dim_fc'], 2, 0, 0.0, 0.0, 1e-3, 1e-5,
                                      activation=cfg['activation'], decay_iters=5)
    return models.TCN_classifier(C_IN, NUM_CLASSES, cfg['dim_fc'], 3, 2, 0, 0.0, 1e-3, 1e-5,
                                 activation=cfg['activation'])


def _margin(logits):
    top = np.sort(logits, axis=1)
    return float((top[:, -1] - top[:, -2]).min())


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
    sd = weights_from_seed(model.state_dict(), cfg['seed'])
    model.load_state_dict(sd)
    rng = np.random.default_rng(cfg['seed'] + 1)
    x = torch.from_numpy(rng.standard_normal((B, T, C_IN)).astype(np.float32))
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
    # ---- eval-mode forward (running statistics) ------------------------------------------------------------------
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
    # every parameter gradient, flattened and joined in named_parameters() order
    out[pre + 'grads'] = np.concatenate([p.grad.numpy().reshape(-1) for _, p in model.named_parameters()])
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
    path = os.path.join(HERE, 'classifiers_tiny.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == '__main__':
    main()
