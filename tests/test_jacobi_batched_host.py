"""The ragged batched Jacobi entry (xps_jacobi_sweeps_batched_f64) without a GPU: its declaration and binding, the shape query,
every refusal -- each returns before any HIP call, so fake device addresses are never touched -- and the pure-numpy routing of
matrix sizes behind eigh_psd_batched."""
import ctypes as C

import numpy as np
import pytest

from cross_patient_speech_decoding_amd import _build, _lib

ENTRY = 'xps_jacobi_sweeps_batched_f64'
_vp, _i, _i64, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t


@pytest.fixture(scope='module')
def lib():
    _build.build(verbose=False)
    return _lib.lib()


def test_new_symbols_are_declared_bound_and_exported(lib):
    declared = set(_lib.header_functions())
    for name in (ENTRY, ENTRY + '_workspace', 'xps_jacobi_batched_supported'):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES['xps_jacobi_batched_supported'] == (_i, [_i, _i])
    assert _lib.SIGNATURES[ENTRY + '_workspace'] == (_sz, [_i])
    assert _lib.SIGNATURES[ENTRY] == (_i, [_vp, _i64, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp])
    assert lib.xps_abi_version() == 4
    # the single-matrix entry keeps its signature
    assert _lib.SIGNATURES['xps_jacobi_sweeps_f64'] == (_i, [_vp, _i64, _vp, _i64, _i, _i, _i, _vp, _vp, _sz, _vp])


def test_shape_queries(lib):
    for m, n in ((32, 32), (33, 1025), (1025, 1025), (0, 40), (40, 0), (-1, 64)):
        assert not lib.xps_jacobi_batched_supported(m, n), (m, n)
    for m, n in ((33, 33), (1024, 1024), (300, 64), (1, 33), (1024, 33)):
        assert lib.xps_jacobi_batched_supported(m, n), (m, n)
    assert not lib.xps_jacobi_small_supported(130, 130, 0)
    assert lib.xps_jacobi_small_supported(128, 128, 0)
    assert lib.xps_jacobi_sweeps_batched_f64_workspace(0) >= 0
    assert lib.xps_jacobi_sweeps_batched_f64_workspace(7) >= 7 * (8 + 8 + 4 + 4)
    assert lib.xps_jacobi_sweeps_batched_f64_workspace(-1) == 0


W_LEN = 1600 + 63 * 307 + 300      # the last element of the 300 x 64 matrix (ldw 307) that starts at 1600
FAKE = 0x1000                      # a "device address": a refused call never reads it


def base_args(lib):
    """A valid call's arguments for the batch {40 x 40, 300 x 64 with ldw 307}; the buffer ends with the last element."""
    w_off = np.array([0, 1600], dtype=np.int64)
    ldw = np.array([40, 307], dtype=np.int64)
    m = np.array([40, 300], dtype=np.int32)
    n = np.array([40, 64], dtype=np.int32)
    return dict(W=FAKE, w_len=W_LEN, w_off=w_off, ldw=ldw, m=m, n=n, batch=2, sweeps=1, check=1, tol=FAKE, off=FAKE,
                frozen=FAKE, sweeps_done=FAKE, ws=FAKE, ws_bytes=int(lib.xps_jacobi_sweeps_batched_f64_workspace(2)), stream=None)


def refused(lib, match, **change):
    args = base_args(lib)
    args.update(change)
    keep = list(args.values())                                                   # (the host arrays stay alive over the call)
    rc = getattr(lib, ENTRY)(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in keep])
    msg = lib.xps_last_error().decode()
    assert rc == -1, (change, rc)
    assert ENTRY in msg and match in msg, (change, msg)


def test_every_refusal_comes_before_any_hip_call(lib):
    i64 = lambda *v: np.array(v, dtype=np.int64)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    for key in ('W', 'w_off', 'ldw', 'm', 'n', 'tol', 'off', 'frozen', 'sweeps_done', 'ws'):
        refused(lib, 'null argument', **{key: None})
    for change in (dict(batch=-1), dict(batch=65536), dict(sweeps=-1), dict(w_len=-1)):
        refused(lib, 'bad parameter', **change)
    refused(lib, 'workspace too small', ws_bytes=base_args(lib)['ws_bytes'] - 1)
    refused(lib, 'workspace too small', ws_bytes=0)
    for m, n in ((i32(32, 300), i32(32, 64)), (i32(40, 1025), i32(40, 1025)), (i32(40, 33), i32(40, 1025)), (i32(40, 300), i32(40, 32)), (i32(0, 300), i32(40, 64))):
        refused(lib, 'not a shape of the block kernel', m=m, n=n)
    refused(lib, 'leading dimension too small', ldw=i64(39, 307))
    refused(lib, 'leading dimension too small', ldw=i64(40, 299))
    for change in (dict(w_off=i64(-1, 1600)), dict(w_off=i64(0, 1601)), dict(w_len=W_LEN - 1),
                   dict(ldw=i64(40, 308)), dict(w_off=i64(0, 2 ** 62)), dict(ldw=i64(40, 2 ** 61))):
        refused(lib, 'reaches outside the buffer', **change)


def test_an_empty_batch_is_ok_without_a_device(lib):
    args = base_args(lib)
    args.update(batch=0, ws_bytes=int(lib.xps_jacobi_sweeps_batched_f64_workspace(0)))
    keep = list(args.values())
    assert getattr(lib, ENTRY)(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in keep]) == 0


def test_size_routing_matches_a_hand_written_expectation(lib):
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    sizes = [130, 24, 137, 137, 24, 1030, 33, 128]
    small_ok = lambda n: bool(lib.xps_jacobi_small_supported(n, n, 0))
    ragged_ok = lambda n: bool(lib.xps_jacobi_batched_supported(n, n))
    small, ragged, alone = LA.route_sizes(sizes, small_ok, ragged_ok)
    assert small == {24: [1, 4], 33: [6], 128: [7]}                 # 33 fits the one-workgroup kernel: it has the first claim
    assert ragged == [0, 2, 3]
    assert alone == [5]
    # one_at_a_time: nothing goes to the ragged call
    small, ragged, alone = LA.route_sizes(sizes, small_ok, lambda n: False)
    assert small == {24: [1, 4], 33: [6], 128: [7]} and ragged == [] and alone == [0, 2, 3, 5]
    assert LA.route_sizes([], small_ok, ragged_ok) == ({}, [], [])


def test_packed_offsets_are_aligned_and_disjoint():
    from cross_patient_speech_decoding_amd.alignment import _linalg as LA
    offs = LA._packed_offsets([137 * 137, 1, 64, 130 * 130])
    assert offs[0] == 0 and all(o % 64 == 0 for o in offs)
    for o, nxt, ln in zip(offs, offs[1:], [137 * 137, 1, 64, 130 * 130]):
        assert o + ln <= nxt < o + ln + 64
