"""CTC prefix beam search, host side (no GPU): the CPU restatement (tests/ctc_beam_ref.py) against the reference decode's
golden prefixes and nlls, argument checks of the C entry points (-1 and a message before any HIP call) and the size checks
of the Python wrappers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from cross_patient_speech_decoding_amd import _build, _lib
from ctc_beam_ref import beam_search


@pytest.fixture(scope='module')
def lib():
    _build.build(verbose=False)
    return _lib.lib()


def _cases(golden_dir):
    g = np.load(os.path.join(golden_dir, 'ctc_beam.npz'))
    for i in range(int(g['n_cases'])):
        yield g[f'probs_{i}'], int(g[f'blank_{i}']), int(g[f'beam_{i}']), tuple(int(v) for v in g[f'prefix_{i}']), \
            float(g[f'nll_{i}'])


def test_restatement_equals_golden(golden_dir):
    n = 0
    for probs, blank, beam, prefix, nll in _cases(golden_dir):
        with np.errstate(divide='ignore'):
            lp = np.log(probs).reshape(probs.shape)
        got, got_nll = beam_search(lp, beam, blank)
        assert got == prefix
        assert got_nll == nll or (np.isnan(nll) and np.isnan(got_nll))
        n += 1
    assert n >= 30


def test_beam_entry_points_reject_bad_arguments(lib):
    p = C.c_void_p(16)
    f64 = lib.xps_ctc_beam_f64
    ws = lib.xps_ctc_beam_workspace(2, 5, 8, 11)
    assert ws >= 2 * 5 * 8 * 4
    for args in [(p, 0, 2, 5, 65, None, 0, 8, 0),        # classes > 64
                 (p, 0, 2, 5, 11, None, 0, 129, 0),      # beam > 128
                 (p, 0, 2, 5, 11, None, 0, 0, 0),        # beam 0
                 (p, 0, 2, 5, 11, None, 11, 8, 0),       # blank outside
                 (p, 2, 2, 5, 11, None, 0, 8, 0),        # dtype flag
                 (p, 0, 2, 5, 11, None, 0, 8, 2),        # from_logits flag
                 (p, 0, -1, 5, 11, None, 0, 8, 0)]:      # negative batch
        assert f64(*args, p, p, p, p, ws, None) == -1, args
        assert b'xps_ctc_beam_f64' in lib.xps_last_error()
    assert f64(None, 0, 2, 5, 11, None, 0, 8, 0, p, p, p, p, ws, None) == -1
    assert f64(p, 0, 2, 5, 11, None, 0, 8, 0, p, p, p, p, ws - 1, None) == -3             # workspace
    sb = lib.xps_ctc_beam_state_bytes(3, 100, 64)
    assert sb >= 3 * 64 * 100 * 4
    step = lib.xps_ctc_beam_step_f32
    assert step(p, 11, 0, 100, 64, p, sb, 9, None) == -1                                    # streams
    assert b'xps_ctc_beam_step_f32' in lib.xps_last_error()
    assert step(p, 11, 0, 129, 64, p, sb, 3, None) == -1
    assert step(p, 11, 11, 100, 64, p, sb, 3, None) == -1
    assert step(p, 11, 0, 100, 0, p, sb, 3, None) == -1
    assert step(None, 11, 0, 100, 64, p, sb, 3, None) == -1
    assert step(p, 11, 0, 100, 64, p, sb - 1, 3, None) == -3                                # state too small
    ro = lib.xps_ctc_beam_readout
    assert ro(p, sb, 3, 100, 64, 3, p, p, p, None) == -1                                    # stream index
    assert b'xps_ctc_beam_readout' in lib.xps_last_error()
    assert ro(p, sb, 3, 129, 64, 0, p, p, p, None) == -1
    assert ro(p, sb, 3, 100, 64, 0, None, p, p, None) == -1
    assert ro(p, sb - 1, 3, 100, 64, 0, p, p, p, None) == -3


def test_python_wrappers_reject_bad_sizes():
    from cross_patient_speech_decoding_amd.realtime_sim import beam_decode_batch, beam_decode_torch, decode
    lp = torch.zeros(2, 5, 11)
    for kw in [dict(beam_size=0), dict(beam_size=129), dict(blank=11), dict(blank=-1)]:
        with pytest.raises(ValueError):
            beam_decode_batch(lp, **kw)
    with pytest.raises(ValueError):
        beam_decode_batch(torch.zeros(1, 5, 65), beam_size=1)
    with pytest.raises(ValueError):
        beam_decode_batch(torch.zeros(5, 11))
    with pytest.raises(ValueError):
        beam_decode_batch(lp, input_lengths=[5])
    with pytest.raises(ValueError):
        beam_decode_batch(lp, input_lengths=[5, 6])
    with pytest.raises(ValueError):
        decode(np.full((4, 3), 1 / 3), beam_size=200)
    with pytest.raises(ValueError):
        decode(np.full(4, 0.5))
    with pytest.raises(ValueError):
        beam_decode_torch(torch.zeros(4, 3), blank=3)
