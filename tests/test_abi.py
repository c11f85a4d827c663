"""The C-ABI library builds, loads and exports every symbol include/xps.h declares.
No compute calls (no GPU needed): argument validation returns before any HIP call."""
import ctypes as C

import pytest

from cross_patient_speech_decoding_amd import _build, _lib


@pytest.fixture(scope='module')
def lib():
    _build.build(verbose=False)
    return _lib.lib()


def test_every_declared_symbol_is_exported_and_bound(lib):
    declared = _lib.header_functions()
    assert len(declared) >= 30
    assert set(declared) == set(_lib.SIGNATURES), set(declared) ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name


def test_abi_version_and_error_channel(lib):
    assert lib.xps_abi_version() == 4
    rm = _lib.rowmap(4)
    rc = lib.xps_gemm_nt_f32(None, C.byref(rm), None, C.byref(rm), None, C.byref(rm), None, 4, 4, 4, 0, None)
    assert rc == -1
    assert b'xps_gemm_nt_f32' in lib.xps_last_error()
    with pytest.raises(_lib.XpsError, match='null argument'):
        _lib.call('xps_gemm_nn_f32', None, C.byref(rm), None, C.byref(rm), None, C.byref(rm), 4, 4, 4, 0, None)
    rc = lib.xps_gru_seq_fwd_f32(None, None, None, None, None, None, 1, 1, 1, 1, None, 0, None)
    assert rc == -1


def test_workspace_queries(lib):
    assert lib.xps_gemm_tn_f32_workspace(384, 100, 40960) >= 384 * 100 * 4
    assert lib.xps_colsum_f32_workspace(1000, 64) >= 4 * 64 * 4
    assert lib.xps_xcov_f64_workspace(409600, 128, 128) >= 128 * 128 * 8
    assert lib.xps_sumsq_f32_workspace(10) >= 8
    assert lib.xps_jacobi_f64_workspace(64) >= 1


def test_product_path_refuses_cpu_tensors():
    import torch
    from cross_patient_speech_decoding_amd.nn_models import functional as XF
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        XF.linear(torch.zeros(2, 3), torch.zeros(4, 3), torch.zeros(4))


_vp, _i, _i64, _f, _d, _sz, _u64 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t, C.c_uint64
_rm = C.POINTER(_lib.RowMap)

# one prototype per C type the header parser knows: the ctypes classes each had in the hand-written table it replaced
PINNED = {
    'xps_last_error': (C.c_char_p, []),
    'xps_gru_seq_status_offset': (C.c_longlong, [_i, _i, _i, _i]),
    'xps_gemm_tn_f32_workspace': (_sz, [_i, _i, _i]),
    'xps_stream_create_low_priority': (_i, [_vp]),
    'xps_gemm_nt_f32': (_i, [_vp, _rm, _vp, _rm, _vp, _rm, _vp, _i, _i, _i, _i, _vp]),
    'xps_gru_seq_fwd_drop_f32': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _f, _u64, _vp, _sz, _vp]),
    'xps_bn_finalize_f32': (_i, [_vp, _d, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _vp]),
    'xps_colsum_f32': (_i, [_vp, _i64, _i, _i, _vp, _vp, _i, _vp, _sz, _vp]),
    'xps_gemm_tn_grouped_f32': (_i, [_vp, _i, _vp, _sz, _vp]),
}


@pytest.mark.parametrize('name', sorted(PINNED))
def test_parsed_signature_matches_the_pinned_ctypes(name):
    assert _lib.SIGNATURES[name] == PINNED[name]


def test_header_parser_fails_loudly_and_reads_awkward_prototypes():
    with pytest.raises(_lib.XpsError, match=r'xps_bad.*short'):
        _lib.parse_signatures('int xps_ok(int a);\nint xps_bad(const float* x, short n);\n')
    for array in ('int xps_arr(const int dims[4], int n);', 'int xps_arr(int x[4]);', 'int xps_arr(float v [], int n);'):
        with pytest.raises(_lib.XpsError, match='xps_arr'):          # an array parameter is a pointer in C: not read as its element
            _lib.parse_signatures(array)
    split = ('/* doc: calls xps_other(x) first */\n'
             'size_t xps_split(const float* const* A,   /* host array */\n'
             '                 int64_t n, /* rows */ double tol,\n'
             '                 void** out);\n')
    assert _lib.parse_signatures(split) == {'xps_split': (_sz, [_vp, _i64, _d, _vp])}
    assert _lib.parse_signatures('#define XPS_OK 0\nlong long xps_nothing(void);\n') == {'xps_nothing': (C.c_longlong, [])}
    with pytest.raises(_lib.XpsError, match='xps_fnptr'):              # a prototype the regex cannot read is not skipped
        _lib.parse_signatures('int xps_fnptr(void (*cb)(int), int n);\n')


def test_dev_ptr_of_none_is_none():
    import torch
    from cross_patient_speech_decoding_amd import _dev
    assert _dev.ptr(None) is None
    t = torch.zeros(3)
    assert _dev.ptr(t) == t.data_ptr()


def test_dev_guards_raise_without_a_gpu():
    import torch
    from cross_patient_speech_decoding_amd import _dev
    with pytest.raises(RuntimeError, match=r'tensors must live on the MI355X \(cuda\) device; the HIP path has no CPU fallback'):
        _dev.need_gpu(None, torch.zeros(1))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='x needs the MI355X: the HIP path has no CPU fallback'):
            _dev.current_device('x')
