"""Single-label classifiers (TemporalConvRNN, SimpleGRU, TCN_classifier): construction, state_dict layout, constructor order,
fixture consistency and ABI declarations.  No GPU: nothing here runs a kernel."""
import ast
import os

import numpy as np
import pytest
import torch

from cross_patient_speech_decoding_amd import _lib
from cross_patient_speech_decoding_amd.nn_models import SimpleGRU, TCN_classifier, TemporalConvRNN
from cross_patient_speech_decoding_amd.nn_models import models as M

CASES = ['rnn_none', 'rnn_int', 'rnn_list', 'tcn_relu', 'tcn_noact']
NUM_CLASSES, C_IN, T, B = 9, 6, 21, 5


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'classifiers_tiny.npz'))


def build_case(cfg):
    """Positional arguments only, in the reference's order (tests/golden/make_classifier_fixtures.py builds the reference's
    classes with the same calls)."""
    if cfg['kind'] == 'rnn':
        return TemporalConvRNN(C_IN, 8, NUM_CLASSES, 16, 2, 3, cfg['dim_fc'], 2, 0, 0.0, 0.0, 1e-3, 1e-5,
                               activation=cfg['activation'], decay_iters=5)
    return TCN_classifier(C_IN, NUM_CLASSES, cfg['dim_fc'], 3, 2, 0, 0.0, 1e-3, 1e-5, activation=cfg['activation'])


@pytest.mark.parametrize('case', CASES)
def test_state_dict_keys_and_shapes_match_reference(golden, case):
    cfg = ast.literal_eval(str(golden[f'{case}/cfg']))
    sd = build_case(cfg).state_dict()
    keys = str(golden[f'{case}/keys']).split('\n')
    assert sorted(sd.keys()) == keys
    shapes = golden[f'{case}/shapes']
    assert shapes.shape == (len(keys), 3)
    for k, row in zip(keys, shapes):
        assert tuple(sd[k].shape) == tuple(int(d) for d in row if d >= 0), k


def test_fixture_is_complete_and_consistent(golden):
    assert sorted(golden['cases']) == sorted(CASES)
    for case in CASES:
        cfg = ast.literal_eval(str(golden[f'{case}/cfg']))
        assert int(golden[f'{case}/seed']) == cfg['seed']
        for k in ('eval_logits', 'train_logits'):            # argmax is demanded under a 1e-4 logits tolerance: a clear winner per row
            top = np.sort(golden[f'{case}/{k}'], axis=1)
            assert (top[:, -1] - top[:, -2]).min() >= 1e-3, (case, k)
        assert golden[f'{case}/x'].shape == (B, T, C_IN) and golden[f'{case}/x'].dtype == np.float32
        assert golden[f'{case}/y'].shape == (B,) and golden[f'{case}/y'].dtype == np.int64
        assert golden[f'{case}/y'].min() >= 0 and golden[f'{case}/y'].max() < NUM_CLASSES
        for k in ('eval_logits', 'train_logits'):
            assert golden[f'{case}/{k}'].shape == (B, NUM_CLASSES)
            assert np.isfinite(golden[f'{case}/{k}']).all()
        assert golden[f'{case}/train_loss'].shape == () and golden[f'{case}/train_acc'].shape == ()
        # accuracy is a count of the 5 trials
        assert abs(float(golden[f'{case}/train_acc']) * B - round(float(golden[f'{case}/train_acc']) * B)) < 1e-6
        logits = golden[f'{case}/train_logits']
        assert float(golden[f'{case}/train_acc']) == pytest.approx((logits.argmax(1) == golden[f'{case}/y']).mean())
        assert golden[f'{case}/step_losses'].shape == (5,)
        np.testing.assert_allclose(golden[f'{case}/step_losses'][0], float(golden[f'{case}/train_loss']), rtol=1e-6)
        assert int(golden[f'{case}/bn_num_batches_tracked']) == 1
        m = build_case(cfg)
        n_filters = m.temporal_conv.conv.out_channels
        assert golden[f'{case}/bn_running_mean'].shape == (n_filters,) == golden[f'{case}/bn_running_var'].shape
        assert golden[f'{case}/grads'].shape == (sum(p.numel() for p in m.parameters()),)
        assert golden[f'{case}/grads'].dtype == np.float32


def test_positional_constructor_order_temporal_conv_rnn():
    m = TemporalConvRNN(6, 8, 9, 16, 2, 3, [12, 10], 2, 1, 0.25, 0.35, 2e-3, 3e-5, None, False, 7)
    conv = m.temporal_conv.conv
    assert (conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding) == (6, 8, (3,), (2,), (1,))
    assert m.num_classes == 9
    assert (m.rnn.gru.input_size, m.rnn.gru.hidden_size, m.rnn.gru.num_layers) == (8, 16, 2)
    assert m.rnn.gru.batch_first and not m.rnn.gru.bidirectional
    assert m.rnn.fc.in_features == 16 and m.rnn.fc.out_features == 12
    assert [(l.in_features, l.out_features) for l in m.fc] == [(12, 10), (10, 9)]
    assert m.temporal_conv.dropout.p == 0.25 and m.rnn.gru.dropout == 0.35
    assert (m.learning_rate, m.l2_reg, m.decay_iters) == (2e-3, 3e-5, 7)
    assert m.temporal_conv.activation is False
    assert isinstance(m.criterion, torch.nn.CrossEntropyLoss)
    cfg = m.configure_optimizers()
    opt, sch = cfg['optimizer'], cfg['lr_scheduler']['scheduler']
    assert isinstance(opt, torch.optim.AdamW)
    assert opt.param_groups[0]['weight_decay'] == 3e-5 and opt.defaults['lr'] == 2e-3
    assert isinstance(sch, torch.optim.lr_scheduler.LinearLR)
    assert (sch.start_factor, sch.end_factor, sch.total_iters) == (1.0, 0.01, 7)
    assert cfg['lr_scheduler']['interval'] == 'epoch'


def test_dim_fc_branches_of_temporal_conv_rnn():
    none = TemporalConvRNN(6, 8, 9, 16, 1, 3)
    assert none.fc is None and none.rnn.fc.out_features == 9
    one = TemporalConvRNN(6, 8, 9, 16, 1, 3, 12)
    assert isinstance(one.fc, torch.nn.Linear) and (one.fc.in_features, one.fc.out_features) == (12, 9)
    assert one.rnn.fc.out_features == 12
    assert 'fc.weight' in one.state_dict() and 'fc.0.weight' not in one.state_dict()


def test_positional_constructor_order_tcn_classifier():
    m = TCN_classifier(6, 9, [8, 7], 3, 2, 1, 0.25, 2e-3, 3e-5, None, False)
    conv = m.temporal_conv.conv
    assert (conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding) == (6, 8, (3,), (2,), (1,))
    assert m.num_classes == 9
    assert [(l.in_features, l.out_features) for l in m.fc] == [(8, 7), (7, 9)]
    assert m.temporal_conv.dropout.p == 0.25 and m.temporal_conv.activation is False
    assert (m.learning_rate, m.l2_reg) == (2e-3, 3e-5)
    assert isinstance(m.configure_optimizers(), torch.optim.AdamW)           # the base class's plain AdamW


def test_tcn_classifier_accepts_int_dim_fc():
    m = TCN_classifier(6, 9, 8, 3)
    assert m.temporal_conv.conv.out_channels == 8
    assert isinstance(m.fc, torch.nn.Linear) and (m.fc.in_features, m.fc.out_features) == (8, 9)


def test_simple_gru_layout_and_bidir():
    g = SimpleGRU(8, 16, 5, 2)
    assert sorted(g.state_dict()) == sorted(
        [f'gru.{w}_{s}_l{l}' for w in ('weight', 'bias') for s in ('ih', 'hh') for l in (0, 1)] + ['fc.weight', 'fc.bias'])
    assert g.gru.dropout == 0.3 and tuple(g.fc.weight.shape) == (5, 16)
    with pytest.raises(NotImplementedError):
        SimpleGRU(8, 16, 5, 2, 0.3, True)


def test_steps_and_data_parallel_hooks():
    for m in (TemporalConvRNN(6, 8, 9, 16, 1, 3), TCN_classifier(6, 9, [8], 3)):
        assert hasattr(m, '_classify_step')
        assert type(m).training_step is M._ClassifyStepMixin.training_step
        assert type(m).predict_step is M.BaseLightningModel.predict_step
        assert m.temporal_conv.process_group is None and m.temporal_conv.global_batch is None
        assert M._plain_hip_criterion(m.criterion)
    assert not M._plain_hip_criterion(torch.nn.CrossEntropyLoss())
    assert not M._plain_hip_criterion(M._HipCrossEntropyLoss(label_smoothing=0.1))


def test_new_entry_points_refuse_cpu_tensors():
    from cross_patient_speech_decoding_amd.nn_models import functional as XF
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        XF.time_max(torch.zeros(3, 2, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        XF.classify_loss_acc(torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64), 3)


def test_abi_symbols_declared_and_bound():
    declared = set(_lib.header_functions())
    for name in ('xps_time_max_fwd_f32', 'xps_time_max_bwd_f32', 'xps_classify_loss_acc_f32',
                 'xps_classify_loss_acc_f32_workspace'):
        assert name in declared and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES['xps_time_max_fwd_f32'][1]) == 7
    assert len(_lib.SIGNATURES['xps_time_max_bwd_f32'][1]) == 7
    assert len(_lib.SIGNATURES['xps_classify_loss_acc_f32'][1]) == 12
    assert len(_lib.SIGNATURES['xps_classify_loss_acc_f32_workspace'][1]) == 1
