"""Host-side checks of the cross-patient CTC data path (no GPU): the C ABI of the new kernels, their argument validation
(which returns before any HIP call), the draw logic of the per-trial augmentations against the draws recorded from the
reference (tests/golden/ctc_data.npz), and select_cv."""
import ctypes
import os

import numpy as np
import pytest
import torch

from cross_patient_speech_decoding_amd import _lib

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'ctc_data.npz')
NEW = ('xps_aug_trial_shift_f32', 'xps_aug_trial_mask_f32', 'xps_aug_trial_scale_f32', 'xps_aug_trial_warp_f32',
       'xps_ctc_greedy_decode', 'xps_edit_distance_supported', 'xps_edit_distance_i64')


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_header_declares_the_new_symbols_and_they_are_bound():
    declared = set(_lib.header_functions())
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    with open(_lib.HEADER_PATH) as f:
        src = f.read()
    assert 'max_pred_len <= 65536, max_tgt_len <= 1024' in src          # the documented limit of the edit-distance kernel


def test_library_exports_the_new_symbols(lib):
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.xps_abi_version() == 4


def test_edit_distance_supported_query(lib):
    assert lib.xps_edit_distance_supported(4096, 256) == 1
    assert lib.xps_edit_distance_supported(0, 0) == 1
    assert lib.xps_edit_distance_supported(65536, 1024) == 1
    assert lib.xps_edit_distance_supported(65537, 3) == 0
    assert lib.xps_edit_distance_supported(10, 1025) == 0
    assert lib.xps_edit_distance_supported(-1, 3) == 0


def test_argument_validation_returns_before_any_hip_call(lib):
    """Every call below must fail with XPS_E_INVALID (-1) on a machine without a GPU: the checks precede the launch."""
    p = ctypes.c_void_p(64)                # a non-null, 16-byte aligned address that is never dereferenced on the host
    q = ctypes.c_void_p(4096)
    # null pointers
    assert lib.xps_aug_trial_shift_f32(None, q, 2, 8, 4, p, None) == -1
    assert lib.xps_aug_trial_shift_f32(p, q, 2, 8, 4, None, None) == -1
    assert lib.xps_aug_trial_mask_f32(p, None, 2, 8, 4, p, 2, None) == -1
    assert lib.xps_aug_trial_scale_f32(p, q, 2, 32, None, None) == -1
    assert lib.xps_aug_trial_warp_f32(p, q, 2, 8, 4, None, None) == -1
    assert lib.xps_ctc_greedy_decode(None, 1, 5, 40, 8, 2, 5, 0, q, q, None) == -1
    assert lib.xps_ctc_greedy_decode(p, 1, 5, 40, 8, 2, 5, 0, q, None, None) == -1
    assert lib.xps_edit_distance_i64(p, 8, None, q, 3, q, 2, 8, 3, q, None) == -1
    assert lib.xps_edit_distance_i64(None, 8, p, q, 3, q, 2, 8, 3, q, None) == -1
    # mask windows outside the sequence
    assert lib.xps_aug_trial_mask_f32(p, q, 2, 8, 4, p, 9, None) == -1
    assert lib.xps_aug_trial_mask_f32(p, q, 2, 8, 4, p, -1, None) == -1
    # in-place roll / warp, bad sizes, unsupported lengths, strides shorter than the padded length
    assert lib.xps_aug_trial_shift_f32(p, p, 2, 8, 4, q, None) == -1
    assert lib.xps_aug_trial_warp_f32(p, p, 2, 8, 4, q, None) == -1
    assert lib.xps_aug_trial_warp_f32(p, q, 2, 0, 4, q, None) == -1
    assert lib.xps_edit_distance_i64(p, 70000, q, q, 3, q, 2, 70000, 3, q, None) == -1
    assert lib.xps_edit_distance_i64(p, 8, q, q, 2000, q, 2, 8, 2000, q, None) == -1
    assert lib.xps_edit_distance_i64(p, 4, q, q, 3, q, 2, 8, 3, q, None) == -1
    assert b'xps_edit_distance_i64' in lib.xps_last_error()


def test_draw_logic_reproduces_the_recorded_draws():
    from cross_patient_speech_decoding_amd.realtime_sim import augmentations as A
    g = np.load(GOLD)
    N, T, _ = g['aug_x'].shape
    seeds = dict(zip(('warp', 'mask', 'shift', 'jitter', 'scale'), (int(s) for s in g['aug_seeds'])))
    torch.manual_seed(seeds['warp'])
    factors, T2 = A.draw_warp_lengths(N, T, 'cpu')
    assert np.array_equal(factors.numpy(), g['aug_warp_factors'])
    assert T2.dtype == torch.int64 and np.array_equal(T2.numpy(), g['aug_warp_T2'])
    torch.manual_seed(seeds['mask'])
    starts, size = A.draw_mask_starts(N, T)
    assert size == int(g['aug_mask_size']) and np.array_equal(starts.numpy(), g['aug_mask_starts'])
    torch.manual_seed(seeds['shift'])
    assert np.array_equal(A.draw_shifts(N, 'cpu').numpy(), g['aug_shifts'])
    torch.manual_seed(seeds['scale'])
    scales = A.draw_scales(N, 'cpu')
    assert scales.shape == (N, 1, 1) and np.array_equal(scales.numpy().reshape(-1), g['aug_scales'])


def test_warp_length_is_a_float32_product_then_truncation():
    """int(T * factor) on a float32 tensor element: a product that is exactly integral in float32 but not in float64."""
    from cross_patient_speech_decoding_amd.realtime_sim import augmentations as A
    torch.manual_seed(3)
    T = 200
    factors, T2 = A.draw_warp_lengths(4096, T, 'cpu')
    ref = np.array([int(T * f) for f in factors[:64]])
    assert np.array_equal(T2[:64].numpy(), ref)
    f32 = (np.float32(T) * factors.numpy()).astype(np.int64)
    assert np.array_equal(T2.numpy(), f32)


def test_select_cv_picks_the_splitter_as_the_reference_does():
    from sklearn.model_selection import KFold, StratifiedKFold
    from cross_patient_speech_decoding_amd.realtime_sim import select_cv
    full = torch.tensor([0, 1, 2] * 5)
    assert isinstance(select_cv(5, full), StratifiedKFold)
    assert isinstance(select_cv(6, full), KFold)                       # a class with fewer trials than folds
    seqs = torch.stack([full, full.flip(0), full], dim=1)              # (N, 3): the first column decides
    assert isinstance(select_cv(5, seqs), StratifiedKFold)
    no_zero = torch.tensor([1, 2] * 6)                                 # bincount gives class 0 a count of 0
    assert isinstance(select_cv(3, no_zero), KFold)
    cv = select_cv(3, no_zero)
    assert cv.shuffle and cv.get_n_splits() == 3


def test_ctc_dataset_items():
    from cross_patient_speech_decoding_amd.realtime_sim import CTCDataset
    X, y = torch.zeros(5, 7, 3), torch.ones(5, 3, dtype=torch.int64)
    ds = CTCDataset(X, y)
    item = ds[2]
    assert len(ds) == 5 and item[0].shape == (7, 3) and item[1].shape == (3,) and item[2:] == (7, 3)
