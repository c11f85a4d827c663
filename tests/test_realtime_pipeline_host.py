"""Host-side parts of the realtime pipeline (no GPU): argument validation of its C entry points (they return -1 with a
message before any HIP call) and the folding of transform stages into one affine feature map."""
import ctypes as C

import numpy as np
import pytest

from cross_patient_speech_decoding_amd import _build, _lib


@pytest.fixture(scope='module')
def lib():
    _build.build(verbose=False)
    return _lib.lib()


def test_pipeline_entry_points_reject_bad_arguments(lib):
    p = C.c_void_p(16)
    assert lib.xps_pipe_frontend_f64(None, 1, 1, 8, 40, None, p, p, 8, 9, p, p, p, 1 << 20, None) == -1
    assert b'xps_pipe_frontend_f64' in lib.xps_last_error()
    assert lib.xps_pipe_frontend_f64(p, 9, 1, 8, 40, None, p, p, 8, 9, p, p, p, 1 << 20, None) == -1
    assert b'streams' in lib.xps_last_error()
    assert lib.xps_pipe_frontend_f64(p, 1, 1, 8, 40, None, p, None, 8, 9, p, p, p, 1 << 20, None) == -1   # state, no a
    assert lib.xps_pipe_frontend_f64(p, 1, 1, 8, 40, None, p, p, 8, 9, p, p, p, 16, None) == -3            # workspace
    assert lib.xps_pipe_frontend_f64_workspace(2, 128, 40, 8) >= 2 * 128 * 40 * 8 * 8
    assert lib.xps_window_shift_f32(p, 5, 8, None, None, p, p, 4, 8, 1, None) == -1                       # k > win
    assert b'xps_window_shift_f32' in lib.xps_last_error()
    assert lib.xps_window_shift_f32(p, 1, 8, None, None, p, p, 4, 6, 1, None) == -1                       # identity, d != C
    assert lib.xps_window_shift_f32(p, 1, 8, None, None, p, p, 4, 8, 1, None) == -1                       # dst aliases src
    assert lib.xps_ctc_collapse_f32(p, 11, 11, p, p, p, 16, 1, None) == -1                                # blank outside
    assert b'xps_ctc_collapse_f32' in lib.xps_last_error()
    assert lib.xps_ctc_collapse_f32(p, 11, 0, p, p, p, 16, 9, None) == -1


def test_feature_map_from_folds_affine_stages():
    from cross_patient_speech_decoding_amd.realtime_sim import feature_map_from
    rng = np.random.default_rng(0)
    W1, m1 = rng.standard_normal((12, 7)), rng.standard_normal(12)
    W2, m2 = rng.standard_normal((7, 5)), rng.standard_normal(7)
    W, c = feature_map_from((W1, m1), (W2, m2), (np.eye(5), None))
    X = rng.standard_normal((9, 12))
    np.testing.assert_allclose(X @ W + c, ((X - m1) @ W1 - m2) @ W2, rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        feature_map_from((W1, m1), (W1, None))
    with pytest.raises(TypeError):
        feature_map_from('pca')
