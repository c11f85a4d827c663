"""A switch set through the table reaches the code that acts on it -- shown where that is observable without timing: support
queries, workspace sizes, launch forms and the Python predicates.  H = 512 is the smallest shape the cluster path takes with
no pad trials.  No kernel is launched."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from cross_patient_speech_decoding_amd import _build, _switches  # noqa: E402
from cross_patient_speech_decoding_amd._lib import lib  # noqa: E402


@pytest.fixture(scope='module', autouse=True)
def _built():
    _build.build(verbose=False)
    assert torch.cuda.is_available(), 'gpu tests need the MI355X'


@pytest.fixture(autouse=True)
def _bf16x3_and_nothing_left_behind():
    before = _switches.library_switches(), dict(_switches._values)
    with _switches.override(XPS_GEMM_PRECISION='bf16x3'):
        yield
    assert (_switches.library_switches(), dict(_switches._values)) == before


def XF():
    from cross_patient_speech_decoding_amd.nn_models import functional
    return functional


def test_forward_image_exchange_follows_its_switch():
    xf = XF()
    for on in (0, 1, 0):
        with _switches.override(XPS_GRU_XIMG=on):
            assert bool(lib().xps_gru_seq_fwd_image_exchange_supported(8, 512, 512, 2)) == bool(on)
            assert xf.hprev_split_wanted(8, 512, 512, 2)
            assert xf.fwd_ysplit_wanted(8, 512, 512, 2) == bool(on)


def test_bptt_grid_follows_its_switch_down_to_the_memoised_workspace_size():
    xf = XF()
    offset = lib().xps_debug_gru_bwd_status_offset
    offset.restype, offset.argtypes = C.c_longlong, [C.c_int] * 3
    seen = {}
    for on in (0, 1, 0):
        with _switches.override(XPS_GRU_CL2=on):
            assert lib().xps_get_gru_bptt_grid() == on
            now = (lib().xps_gru_seq_bwd_f32_workspace(4, 512, 512, 2), offset(512, 512, 2))
            assert xf._gru_ws_bytes('xps_gru_seq_bwd_f32_workspace', 4, 512, 512, 2) == now[0]      # (no memo reset by hand)
            assert seen.setdefault(on, now) == now
    # the 2-D grid's header holds 160 flag words per round where the 1-D kernel's holds 16, and its query covers both kernels
    assert seen[1][0] >= seen[0][0] > 16 and seen[1][1] > seen[0][1] > 0


def test_cluster_mode_off_changes_the_launch_form_and_the_forward_workspace():
    xf = XF()
    on = xf._launch_form(512, 512), xf._gru_ws_bytes('xps_gru_seq_fwd_f32_workspace', 8, 512, 512, 2)
    with _switches.override(XPS_GRU_CLUSTER='off'):
        assert lib().xps_get_gru_cluster_mode() == 0
        assert xf._launch_form(512, 512) != on[0] and xf._launch_form(512, 512)[0] is False
        assert xf._gru_ws_bytes('xps_gru_seq_fwd_f32_workspace', 8, 512, 512, 2) == 16 < on[1]
        assert lib().xps_gru_seq_fwd_f32_workspace(8, 512, 512, 2) == 16
    assert (xf._launch_form(512, 512), xf._gru_ws_bytes('xps_gru_seq_fwd_f32_workspace', 8, 512, 512, 2)) == on


def test_python_predicates_follow_their_switches():
    xf = XF()
    assert xf.split4_wanted(8, 512, 512, 2)
    with _switches.override(XPS_SPLIT4=0):
        assert not xf.split4_wanted(8, 512, 512, 2) and not xf.split4_mode()
    assert xf.split4_wanted(8, 512, 512, 2)
    assert not xf.fwd_images_wanted(8, 512, 512, 2) and not xf.skinny_dx_wanted(40960, 100, 1536)
    with _switches.override(XPS_FWD_IMAGES=1, XPS_SKINNY_DX=1):
        assert xf.fwd_images_wanted(8, 512, 512, 2)
        assert xf.skinny_dx_wanted(40960, 100, 1536) and not xf.skinny_dx_wanted(40960, 1024, 1536)
        with _switches.override(XPS_GEMM_DMA=0):                      # one parse of XPS_GEMM_DMA: the library's
            assert not xf.skinny_dx_wanted(40960, 100, 1536) and not xf.hprev_split_wanted(8, 512, 512, 2)
    assert not xf.fwd_images_wanted(8, 512, 512, 2) and not xf.skinny_dx_wanted(40960, 100, 1536)
