"""xps_gru_seq_fwd_f32 / xps_gru_seq_bwd_f32 (include/xps.h) called directly on every launch route -- resident (H = 64 / 128),
generic vector / scalar (LDS tile), per-step (H > 128), cluster -- in both product precisions, and held to the float64
restatement and the error bounds of tests/gru_seq_ref.py.

Protocol of every launch.  Each output (y_ext, saved, dgi, dghn, dh0) lies between guard rows and starts filled with a
sentinel (a quiet-NaN bit pattern no kernel produces): afterwards the guards are intact and every element inside is finite,
i.e. written.  Each input lies between NaN guard rows and keeps its bits.  A second launch gives the same bits.  Every case
first asks the library (xps_gru_seq_route) which kernels the call runs and asserts the route the case is named for.

Forward.  For every t and direction the kernel's OWN previous slot of y_ext is h_{t-1}: the float64 step from it must lie
within step_bound of the kernel's slot t + 1, elementwise.  That check does not grow with T and sees every element.  Slots 0
and T + 1 equal h0 bit for bit (or zero); saved = NULL leaves y_ext's bits as they are.

Backward.  dgi, dghn, dh0 against backward_ref through the float64 forward; tolerance = 4 x the error of the float32 numpy
restatement (forward and backward) on the same data, times 40 in bf16x3 mode (the project's factor between the two product
precisions, tests/test_gpu_nn_kernels.py), plus 1e-4 max(1, max |ref|) -- the rule of tests/test_gpu_dropout_parity.py.
dy only, dhn only, both; dh0 NULL and not; dy = NULL gives the bits of an all-zero dy.

Input regimes (gru_seq_ref.seq_inputs): 'normal', and 'saturating' -- gi and w_hh 8 times wider, with planted gi entries of
+-100 that overflow the hardware exponential of the resident and cluster kernels (the gate must come out exactly 0 / +-1,
not NaN) -- each with a random nonzero h0 and with h0 = NULL.  The forward check runs in every regime at every shape.  The
backward runs in the saturating regime where T <= SAT_BWD_MAX_T only: with w_hh 8 times wider the recurrence amplifies a
perturbation at every step, and at T = 64 the float64 backward_ref itself moves by more than the tolerance's floor when gi
moves by 1e-7 of its value, less than float32 resolves (tests/test_gru_seq_ref_host.py shows it on the host), so no float32
computation is determined there.  At T <= 7 the same perturbation moves it by less than a tenth of the floor.

Why the launches that no test made before are in bounds (read before they ran):
* generic kernels, any H <= 624, aligned or not (gru_fwd_kernel / gru_bwd_kernel): W_hh rows go through load_w4, whose vector
  form needs k + 3 < H and whose scalar form guards each of k .. k + 3 against H; it is the only access that depends on the
  weights' alignment.  Hidden-unit tiles run to Hp = H rounded up to 16; row indices beyond H are clamped (jc) for loads and
  masked (j < H, b < B) for stores; LDS rows are ldh = Hp + 4 / ldg = 3 Hp + 4 / ldc = Hp + 4 floats and k + 4 kq + 3 < Hp.
  The dynamic LDS is 2 x 16 x ldh x 4 bytes forward, 16 x (ldg + ldc) x 4 backward: above 64 KiB the launch raises the
  kernel's limit first; H = 624 needs 160 256 bytes of the CU's 163 840.
* per-step kernels (gru_step_fwd_kernel / gru_step_bwd_kernel) with H % 4 != 0, H > 512 or misaligned W_hh: the operands go
  through TileLoader.  Its unguarded 16-byte form is taken only when `fast` (the caller's vec flag: H % 4 == 0 and aligned
  pointers) and `full` hold and the whole 16-deep k-tile lies below kend; otherwise every row is guarded by xoff >= 0 (row <
  B, or a valid gate-strided W_hh row: the forward clears the rows of a ragged last unit tile) and every element by k <
  kend, with 16-byte loads only when vec && k + 3 < kend.  The [k][x] W_hh operand of the backward guards k < kend, x < H the
  same way.  The epilogues read and write under b < B && j < H, and nothing in them depends on H <= 512: the offsets are 64-bit.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gru_seq_ref as R
from guarded_buf import F32, Buf

pytestmark = pytest.mark.gpu

INVALID = -1                         # XPS_E_INVALID
S3 = R.STEP | R.STEP_VECA | R.STEP_VECB
SAT_BWD_MAX_T = 8                    # the saturating regime's backward is checked up to this T (module docstring)


def _lib():
    from cross_patient_speech_decoding_amd._lib import lib
    return lib()


def _stream():
    from cross_patient_speech_decoding_amd._dev import stream
    return stream()


@pytest.fixture(scope='module', autouse=True)
def _built():
    from cross_patient_speech_decoding_amd import _build
    _build.build(verbose=False)
    assert torch.cuda.is_available(), 'gpu tests need the MI355X'


def _ptrs(bufs):
    return (C.c_void_p * len(bufs))(*[b.ptr for b in bufs])


def _ws(nbytes):
    return torch.zeros(int(nbytes), dtype=torch.uint8, device='cuda')


@contextlib.contextmanager
def _settings(cluster_mode=None, step_path=None):
    from cross_patient_speech_decoding_amd import _switches
    lib = _lib()
    old = lib.xps_get_gru_cluster_mode()
    with contextlib.ExitStack() as stack:
        try:
            if cluster_mode is not None:
                assert lib.xps_set_gru_cluster_mode({'off': 0, 'steps': 1, 'persistent': 2}[cluster_mode]) == 0
            if step_path is not None:
                stack.enter_context(_switches.override(XPS_GRU_STEP_PATH=step_path))
            yield
        finally:
            lib.xps_set_gru_cluster_mode(old)


# ---- the references, computed once per (shape, regime, h0) and shared by both precisions and all alignments ------------------
@functools.lru_cache(maxsize=None)
def _problem(T, B, H, ndir, regime, with_h0):
    rng = np.random.default_rng(1000003 * T + 10007 * B + 101 * H + 7 * ndir + len(regime) + int(with_h0))
    gi, w, b, h0 = R.seq_inputs(rng, T, B, H, ndir, regime, with_h0)
    dy = rng.standard_normal((T, B, ndir * H)).astype(F32)
    dhn = rng.standard_normal((ndir, B, H)).astype(F32)
    y64, g64 = R.forward_ref(gi, w, b, h0, T, B, H, ndir)
    y32, g32 = R.forward_ref(gi, w, b, h0, T, B, H, ndir, dtype=F32)
    for a in (gi, dy, dhn, y64, y32, *w, *b) + (() if h0 is None else (h0,)):
        a.setflags(write=False)
    return dict(gi=gi, w=w, b=b, h0=h0, dy=dy, dhn=dhn, y64=y64, g64=g64, y32=y32, g32=g32, bwd={})


def _bwd_ref(P, T, B, H, ndir, use_dy, use_dhn):
    """(float64 dgi, dghn, dh0) and the float32 restatement's max error on each, cached on the problem."""
    key = (use_dy, use_dhn)
    if key not in P['bwd']:
        dy, dhn = (P['dy'] if use_dy else None), (P['dhn'] if use_dhn else None)
        ref = R.backward_ref(dy, dhn, P['y64'], P['g64'], P['w'], T, B, H, ndir)
        r32 = R.backward_ref(dy, dhn, P['y32'], P['g32'], P['w'], T, B, H, ndir, dtype=F32)
        P['bwd'][key] = (ref, [float(np.abs(a.astype(np.float64) - c).max()) for a, c in zip(r32, ref)])
    return P['bwd'][key]


# ---- launches ----------------------------------------------------------------------------------------------------------------
class Device:
    """The inputs of one problem on the device, weights at the alignment the case asks for."""

    def __init__(self, P, T, B, H, ndir, w_off=0, wt_off=0):
        self.shape = (T, B, H, ndir)
        self.gi = Buf(P['gi'].size, data=P['gi'])
        self.w = [Buf(3 * H * H, data=a, off=w_off) for a in P['w']]
        self.wt = [Buf(3 * H * H, data=np.ascontiguousarray(a.T), off=wt_off) for a in P['w']]         # (H, 3H)
        self.b = [Buf(3 * H, data=a) for a in P['b']]
        self.h0 = None if P['h0'] is None else Buf(P['h0'].size, data=P['h0'])
        self.dy = Buf(P['dy'].size, data=P['dy'])
        self.dy0 = Buf(P['dy'].size, data=np.zeros_like(P['dy']))
        self.dhn = Buf(P['dhn'].size, data=P['dhn'])

    def inputs(self):
        return [self.gi, self.dy, self.dy0, self.dhn, *self.w, *self.wt, *self.b] + ([] if self.h0 is None else [self.h0])

    def forward(self, save=True):
        T, B, H, ndir = self.shape
        lib = _lib()
        y = Buf((T + 2) * B * ndir * H)
        saved = Buf(ndir * T * B * 4 * H) if save else None
        nbytes = lib.xps_gru_seq_fwd_f32_workspace(T, B, H, ndir)
        ws = _ws(nbytes)
        rc = lib.xps_gru_seq_fwd_f32(self.gi.ptr, _ptrs(self.w), _ptrs(self.b), None if self.h0 is None else self.h0.ptr, y.ptr,
                                     saved.ptr if save else None, T, B, H, ndir, ws.data_ptr(), nbytes, _stream())
        torch.cuda.synchronize()
        off = lib.xps_gru_seq_status_offset(T, B, H, ndir)
        if rc == 0 and off >= 0:
            assert int(ws[off:off + 4].view(torch.int32).item()) == 0, 'a cluster hand-off timed out'
        return rc, y, saved

    def backward(self, y, saved, dy, dhn, want_dh0):
        T, B, H, ndir = self.shape
        lib = _lib()
        dgi, dghn = Buf(ndir * T * B * 3 * H), Buf(ndir * T * B * H)
        dh0 = Buf(ndir * B * H) if want_dh0 else None
        nbytes = lib.xps_gru_seq_bwd_f32_workspace(T, B, H, ndir)
        ws = _ws(nbytes)
        rc = lib.xps_gru_seq_bwd_f32(None if dy is None else dy.ptr, None if dhn is None else dhn.ptr, y.ptr, saved.ptr,
                                     _ptrs(self.w), _ptrs(self.wt), dgi.ptr, dghn.ptr, dh0.ptr if want_dh0 else None,
                                     T, B, H, ndir, ws.data_ptr(), nbytes, _stream())
        torch.cuda.synchronize()
        off = lib.xps_gru_seq_status_offset(T, B, H, ndir)
        if rc == 0 and off >= 0:
            assert int(ws[off:off + 4].view(torch.int32).item()) == 0, 'a cluster hand-off timed out'
        return rc, dgi, dghn, dh0


def _written(buf, what):
    assert buf.guards_intact(), f'{what}: a guard row was written'
    assert bool(torch.isfinite(buf.view()).all()), f'{what}: an element is not finite (or was never written)'


def _same(a, b, what):
    assert torch.equal(a.bits(), b.bits()), f'{what}: two launches differ'


def check_forward(dev, P, mode, activation):
    """Runs the forward three times (twice with `saved`, once without) and checks the protocol and the per-step bound.
    Returns (y_ext buffer, saved buffer, largest error / bound)."""
    T, B, H, ndir = dev.shape
    rc, y, saved = dev.forward()
    assert rc == 0, _lib().xps_last_error()
    _written(y, 'y_ext')
    _written(saved, 'saved')
    rc2, y2, saved2 = dev.forward()
    assert rc2 == 0
    _same(y, y2, 'y_ext')
    _same(saved, saved2, 'saved')
    rc3, y3, _ = dev.forward(save=False)
    assert rc3 == 0
    _same(y, y3, 'y_ext with saved = NULL')
    got = y.numpy((T + 2, B, ndir * H))
    # slots 0 and T + 1: h0 of the forward / reverse direction bit for bit, zero elsewhere
    want0, wantT = np.zeros((B, ndir * H), F32), np.zeros((B, ndir * H), F32)
    if P['h0'] is not None:
        want0[:, :H] = P['h0'][0]
        if ndir == 2:
            wantT[:, H:] = P['h0'][1]
    np.testing.assert_array_equal(got[0].view(np.int32), want0.view(np.int32))
    np.testing.assert_array_equal(got[T + 1].view(np.int32), wantT.view(np.int32))
    worst = 0.0
    for d in range(ndir):
        cols = slice(d * H, (d + 1) * H)
        for t in range(T):
            src, dst = R._slots(t, d)
            ref, parts = R.step_ref(P['gi'][d, t], P['w'][d], P['b'][d], got[src, :, cols])
            err, bound = np.abs(got[dst, :, cols].astype(np.float64) - ref), R.step_bound(parts, mode, activation)
            ratio = float((err / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (f'direction {d}, t = {t}: error / step_bound = {ratio:.3f} at {np.unravel_index((err / bound).argmax(), err.shape)} '
                                  f'(error {err.max():.3e})')
    return y, saved, worst


VARIANTS = [(True, True, True), (True, False, False), (False, True, True)]          # (dy, dhn, dh0 requested)


def check_backward(dev, P, mode, y, saved, variants):
    """Returns the largest error / tolerance over the outputs and variants."""
    T, B, H, ndir = dev.shape
    mult = 40.0 if mode == 'bf16x3' else 1.0
    shapes = [(ndir, T, B, 3 * H), (ndir, T, B, H), (ndir, B, H)]
    worst = 0.0
    for use_dy, use_dhn, want_dh0 in variants:
        dy, dhn = (dev.dy if use_dy else None), (dev.dhn if use_dhn else None)
        outs = dev.backward(y, saved, dy, dhn, want_dh0)
        assert outs[0] == 0, _lib().xps_last_error()
        again = dev.backward(y, saved, dy, dhn, want_dh0)
        ref, e32 = _bwd_ref(P, T, B, H, ndir, use_dy, use_dhn)
        for name, buf, buf2, r, e, shape in zip(('dgi', 'dghn', 'dh0'), outs[1:], again[1:], ref, e32, shapes):
            if buf is None:
                assert name == 'dh0' and not want_dh0
                continue
            _written(buf, name)
            _same(buf, buf2, name)
            tol = 4 * mult * e + 1e-4 * max(1.0, float(np.abs(r).max()))
            err = float(np.abs(buf.numpy(shape).astype(np.float64) - r).max())
            worst = max(worst, err / tol)
            assert err <= tol, f'{name} (dy {use_dy}, dhn {use_dhn}): error {err:.3e} > tolerance {tol:.3e} (float32 restatement {e:.3e})'
        if not use_dy:                                 # dy = NULL is an all-zero dy, bit for bit
            zero = dev.backward(y, saved, dev.dy0, dhn, want_dh0)
            assert zero[0] == 0
            for name, a, c in zip(('dgi', 'dghn', 'dh0'), outs[1:], zero[1:]):
                if a is not None:
                    _same(a, c, name + ' with dy = NULL against dy = 0')
    return worst


#        id: (T, B, H, ndir, forward route, backward route, options)
#        options: w_off / wt_off = 1 starts W_hh / W_hh^T 4 bytes past a 16-byte boundary; cluster_mode; step_path
def _cases():
    c = {}
    for T, B, H, nd in [(5, 1, 64, 1), (7, 17, 64, 2), (64, 33, 64, 2), (3, 16, 128, 1), (6, 21, 128, 2), (64, 5, 128, 1)]:
        c[f'resident-{T}x{B}x{H}x{nd}'] = (T, B, H, nd, R.RESIDENT, R.RESIDENT, {})
    for H in (4, 20, 68, 124):
        c[f'generic_vec-H{H}'] = (4, 19, H, 2, R.GENERIC_VEC, R.GENERIC_VEC, {})
    for H in (1, 6, 63, 127):
        c[f'generic_scalar-H{H}'] = (4, 19, H, 2, R.GENERIC_SCALAR, R.GENERIC_SCALAR, {})
    for H in (64, 128):
        c[f'generic_scalar_by_alignment-H{H}'] = (4, 19, H, 2, R.GENERIC_SCALAR, R.GENERIC_SCALAR, dict(w_off=1, wt_off=1))
        # one layer on two kernel families: `saved` has one layout on all routes but the cluster's
        c[f'mixed-resident_fwd-scalar_bwd-H{H}'] = (4, 19, H, 2, R.RESIDENT, R.GENERIC_SCALAR, dict(wt_off=1))
        c[f'mixed-scalar_fwd-resident_bwd-H{H}'] = (4, 19, H, 2, R.GENERIC_SCALAR, R.RESIDENT, dict(w_off=1))
    for (T, B, H, nd), code in [((3, 5, 129, 1), R.STEP), ((3, 7, 132, 2), S3), ((4, 130, 256, 2), S3), ((3, 127, 260, 1), S3),
                                ((3, 130, 258, 1), R.STEP), ((2, 5, 516, 1), S3)]:
        c[f'step-{T}x{B}x{H}x{nd}'] = (T, B, H, nd, code, code, {})
    c['step-misaligned_w_hh-3x7x132x2'] = (3, 7, 132, 2, R.STEP | R.STEP_VECA, R.STEP | R.STEP_VECA, dict(w_off=1))
    c[f'step-envelope-H{R.MAX_H_STEP}'] = (2, 3, R.MAX_H_STEP, 1, S3, S3, {})
    for T, B, H, nd in [(3, 5, 132, 2), (3, 5, 256, 1)]:           # H = 256: the backward's tile passes 64 KiB
        c[f'generic_above_128-{T}x{B}x{H}x{nd}'] = (T, B, H, nd, R.GENERIC_VEC, R.GENERIC_VEC, dict(step_path=0))
    c[f'generic-envelope-H{R.MAX_H_TILE}'] = (2, 3, R.MAX_H_TILE, 1, R.GENERIC_VEC, R.GENERIC_VEC, dict(step_path=0))   # both tiles > 64 KiB
    for T, B, H, nd in [(4, 130, 320, 1), (3, 300, 260, 2)]:
        for m in ('persistent', 'steps'):
            c[f'cluster_{m}-{T}x{B}x{H}x{nd}'] = (T, B, H, nd, R.CLUSTER, R.CLUSTER, dict(cluster_mode=m))
        c[f'cluster_off_runs_step-{T}x{B}x{H}x{nd}'] = (T, B, H, nd, S3, S3, dict(cluster_mode='off'))
    return c


CASES = _cases()
WORST = {}


@pytest.mark.parametrize('name', list(CASES))
def test_recurrence_vs_fp64(name, gemm_precision):
    T, B, H, ndir, route_f, route_b, opt = CASES[name]
    mode = gemm_precision
    w_off, wt_off = opt.get('w_off', 0), opt.get('wt_off', 0)
    lib = _lib()
    with _settings(opt.get('cluster_mode'), opt.get('step_path')):
        # which kernels the two calls run: the per-step backward streams W_hh, the other backward routes W_hh^T
        assert lib.xps_gru_seq_route(T, B, H, ndir, int(not w_off), 0) == route_f
        bwd_aligned = (not w_off) if (route_b & R.STEP) else (not wt_off)
        assert lib.xps_gru_seq_route(T, B, H, ndir, int(bwd_aligned), 1) == route_b
        act_f = R.activation_of(route_f)
        fwd_worst = bwd_worst = 0.0
        for regime in ('normal', 'saturating'):
            for with_h0 in (True, False):
                P = _problem(T, B, H, ndir, regime, with_h0)
                dev = Device(P, T, B, H, ndir, w_off, wt_off)
                y, saved, worst = check_forward(dev, P, mode, act_f)
                fwd_worst = max(fwd_worst, worst)
                if regime == 'saturating' and T > SAT_BWD_MAX_T:
                    continue
                variants = VARIANTS if (regime == 'normal') == with_h0 else VARIANTS[:1]
                y_bits, saved_bits = y.bits().clone(), saved.bits().clone()       # inputs of the backward
                bwd_worst = max(bwd_worst, check_backward(dev, P, mode, y, saved, variants))
                assert all(b.unchanged() for b in dev.inputs()), 'a read-only input changed'
                assert torch.equal(y.bits(), y_bits) and torch.equal(saved.bits(), saved_bits), 'the backward wrote y_ext or saved'
    print(f'{name} {mode}: forward max error / step_bound = {fwd_worst:.3f}, backward max error / tolerance = {bwd_worst:.3f}')
    WORST[(name, mode)] = (fwd_worst, bwd_worst)


@pytest.mark.parametrize('step_path,H', [(1, R.MAX_H_STEP + 1), (0, R.MAX_H_TILE + 1)])
def test_one_step_beyond_the_envelope_is_refused_in_both_directions(step_path, H):
    """xps.h: the per-step route stops at XPS_GRU_MAX_H_STEP, the LDS-tile routes at XPS_GRU_MAX_H_TILE, forward and backward
    alike: XPS_E_INVALID, and not one element of an output is written."""
    T, B, ndir = 2, 3, 1
    lib = _lib()
    rng = np.random.default_rng(H)
    P = dict(gi=rng.standard_normal((ndir, T, B, 3 * H)).astype(F32), w=[np.zeros((3 * H, H), F32)], b=[np.zeros(3 * H, F32)],
             h0=None, dy=rng.standard_normal((T, B, ndir * H)).astype(F32), dhn=rng.standard_normal((ndir, B, H)).astype(F32))
    with _settings(None, step_path):
        for aligned in (0, 1):
            for backward in (0, 1):
                assert lib.xps_gru_seq_route(T, B, H, ndir, aligned, backward) == R.REFUSED
                assert lib.xps_gru_seq_route(T, B, H - 1, ndir, aligned, backward) != R.REFUSED
        dev = Device(P, T, B, H, ndir)
        rc, y, saved = dev.forward()
        assert rc == INVALID and y.untouched() and saved.untouched()
        assert b'XPS_GRU_MAX_H' in lib.xps_last_error()
        # a y_ext / saved pair as a forward would have left them (finite values): the backward must refuse all the same
        y_in, saved_in = Buf(y.n, data=np.zeros(y.n, F32)), Buf(saved.n, data=np.full(saved.n, 0.5, F32))
        rc, dgi, dghn, dh0 = dev.backward(y_in, saved_in, dev.dy, dev.dhn, True)
        assert rc == INVALID and dgi.untouched() and dghn.untouched() and dh0.untouched()
        assert all(b.unchanged() for b in dev.inputs() + [y_in, saved_in])
