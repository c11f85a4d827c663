"""Host-side parts of the session replay (no GPU): the C entry points are declared, exported and bound, reject every
limit with a message before any HIP call, and the Python surface names the offending shape."""
import ctypes as C

import numpy as np
import pytest

from cross_patient_speech_decoding_amd import _build, _lib

NAMES = ('xps_hg_trials_f64_workspace', 'xps_hg_trials_f64')


@pytest.fixture(scope='module')
def lib():
    _build.build(verbose=False)
    return _lib.lib()


def test_symbols_declared_exported_and_bound(lib):
    declared = _lib.header_functions()
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.xps_abi_version() == 4


def _call(lib, N=4, n_bins=3, Cn=8, Tn=40, bands=8, taps=9, d=8, W=None, features=True, ws=None, raw=True, a=True,
          zi0=False, power=True):
    p = C.c_void_p(16)
    need = lib.xps_hg_trials_f64_workspace(N, n_bins, Cn, Tn, bands)
    return lib.xps_hg_trials_f64(p if raw else None, 0, N, n_bins, Cn, Tn, None, None, 0, p, p if a else None, bands, taps,
                                 p if zi0 else None, 0, None, p if power else None, W, None, None, 1 if W else 0, d,
                                 p if features else None, p, need if ws is None else ws, None)


def test_limits_return_their_error_code_before_any_launch(lib):
    p = C.c_void_p(16)
    for kw, code, word in (({'Tn': 2049}, -1, b'2048'), ({'taps': 33}, -1, b'taps'), ({'bands': 33}, -1, b'bands'),
                           ({'N': 0}, -1, b'bad argument'), ({'W': p, 'd': 0}, -1, b'd >= 1'), ({'raw': False}, -1, b'bad'),
                           ({'d': 6}, -1, b'identity'), ({'a': False, 'zi0': True}, -1, b'IIR'),
                           ({'power': False, 'features': False}, -1, b'nothing')):
        assert _call(lib, **kw) == code, kw
        msg = lib.xps_last_error()
        assert b'xps_hg_trials_f64' in msg and word in msg, (kw, msg)
    need = lib.xps_hg_trials_f64_workspace(4, 3, 8, 40, 8)
    assert need >= 4 * 3 * 8 * 8
    assert _call(lib, ws=need - 1) == -3
    assert b'workspace' in lib.xps_last_error()
    # the general path keeps one squared bin per trial in the workspace
    assert lib.xps_hg_trials_f64_workspace(4, 3, 8, 40, 3) >= need + 4 * 8 * 40 * 3 * 8
    # 2^31 elements and more are sized in 64 bits
    assert lib.xps_hg_trials_f64_workspace(1 << 22, 50, 128, 40, 8) >= (1 << 22) * 50 * 128 * 8


def _cpu_model(d, win=4, stride=2, bidirectional=False):
    from cross_patient_speech_decoding_amd.realtime_sim import RealtimeRNNModel
    return RealtimeRNNModel(win * d, 8, 1, 5, dropout=0.0, win_size=win, stride=stride, bidirectional=bidirectional)


def test_python_shape_errors_name_the_shape():
    from cross_patient_speech_decoding_amd.realtime_sim import SessionReplay, process_HG_trials
    coefs = np.ones((2, 3, 2))
    with pytest.raises(ValueError, match=r'\(3, 8, 40\)'):
        process_HG_trials(np.zeros((3, 8, 40)), coefs)
    with pytest.raises(ValueError, match=r'\(2, 0, 8, 40\)'):
        process_HG_trials(np.zeros((2, 0, 8, 40)), coefs)
    with pytest.raises(ValueError, match='2D or 3D'):
        process_HG_trials(np.zeros((2, 3, 8, 40)), np.ones(4))
    with pytest.raises(ValueError, match=r'\(7, 6\)'):
        SessionReplay(_cpu_model(6), coefs, 8, 40, feature_map=(np.zeros((7, 6)), None))
    with pytest.raises(ValueError, match=r'\(2, 8, 3\)'):
        SessionReplay(_cpu_model(8), coefs, 8, 40, filt_ics=np.zeros((2, 8, 3)))
    with pytest.raises(ValueError, match='input_size'):
        SessionReplay(_cpu_model(5), coefs, 8, 40)
    with pytest.raises(ValueError, match='unidirectional'):
        SessionReplay(_cpu_model(8, bidirectional=True), coefs, 8, 40)
    with pytest.raises(ValueError, match='different numbers of patients'):
        SessionReplay(_cpu_model(8), coefs, 8, 40, bad_channels=[[0], [1]], feature_map=[None, None, None])
    with pytest.raises(RuntimeError, match='GPU'):
        SessionReplay(_cpu_model(8), coefs, 8, 40)             # every shape is right: the model is not on the device
