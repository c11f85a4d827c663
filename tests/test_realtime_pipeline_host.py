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


def test_stream_entry_points_reject_bad_arguments(lib):
    a, b, c, d, e, f, g, h = (C.c_void_p(4096 + 64 * i) for i in range(8))       # eight distinct 16-byte aligned addresses
    off = lambda p: C.c_void_p(p.value + 4)

    def refused(rc, name, word):
        assert rc == -1
        msg = lib.xps_last_error()
        assert name in msg and word in msg, msg

    gemv = lambda x, W, K=8, B=1: lib.xps_gemv_f32(x, W, None, c, 4, K, B, None)
    refused(gemv(off(a), b), b'xps_gemv_f32', b'aligned')
    refused(gemv(a, off(b)), b'xps_gemv_f32', b'aligned')
    refused(gemv(a, b, B=0), b'xps_gemv_f32', b'streams')
    refused(gemv(a, b, B=9), b'xps_gemv_f32', b'streams')
    refused(gemv(None, b), b'xps_gemv_f32', b'bad argument')

    def cell(x=a, w_ih=b, w_hh=c, h_prev=f, h_new=g, K=8, H=8, B=1):
        return lib.xps_gru_cell_gemv_f32(x, K, w_ih, w_hh, d, e, h_prev, h_new, H, B, None)
    name = b'xps_gru_cell_gemv_f32'
    refused(cell(x=off(a)), name, b'x and w_ih')
    refused(cell(w_ih=off(b)), name, b'x and w_ih')
    refused(cell(h_prev=off(f), K=3), name, b'h and w_hh')
    refused(cell(w_hh=off(c), K=3), name, b'h and w_hh')
    refused(cell(B=0), name, b'streams')
    refused(cell(B=9), name, b'streams')
    refused(cell(h_new=f), name, b'alias')
    refused(cell(H=0), name, b'bad argument')


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
