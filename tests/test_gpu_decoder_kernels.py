"""xps_decoder_fwd_f32 / xps_decoder_bwd_f32 (include/xps.h, csrc/xps_decoder.hip) called directly over their envelope --
H in {64, 128}, C in 1 .. 16, L in 1 .. 8, any B and ntok -- in both product precisions (all four template instances of each
kernel), and the three Python decode paths that share their contract (nn_models/functional.py DecoderFn, DecoderWideFn), all
held to the float64 restatement of tests/decoder_ref.py.

Protocol of every launch (that of tests/test_gpu_gru_recurrence.py).  Each output (logits, tokens, hs, saved, dgi, dghn, dh0)
lies between guard rows and starts filled with a sentinel: afterwards the guards are intact and every element inside is
written -- floats finite, tokens in 0 .. ntok - 1.  Each input lies between NaN guards and keeps its bits.  A second launch
gives the same bits.

Forward.  Nothing is compared across steps, so a token flipped at a near-tied argmax cannot spoil a check and no tolerance
grows with L.  Per step s, from the kernel's OWN hs[s] and OWN tokens[s]: the float64 cell must lie within
gru_seq_ref.step_bound (activation 'hw') of the kernel's hs[s + 1], r, z, n, q of `saved` within the per-gate bounds, the
logits within decoder_ref.logits_bound of the float64 Linear of the kernel's hs[s + 1], and tokens[s + 1] must be EXACTLY
decoder_ref.next_tokens of the kernel's own float32 logits.  hs[0] is h0 bit for bit; saved = NULL changes no bit.

Backward.  The kernel's own hs and saved go back in with dlogits ~ N(0, 1); dgi, dghn, dh0 against decoder_ref.replay with
the kernel's tokens.  Tolerance: 4 x the error of the float32 numpy restatement on the same data, x 40 in bf16x3 mode, plus
1e-4 max(1, max |ref|) (tests/test_gpu_gru_recurrence.py, tests/test_gpu_dropout_parity.py).

Free run.  Without a teacher the kernel's tokens equal the float64 decode's for every trial whose reference top-2 margin is at
least decoder_ref.MARGIN at every step; tests/test_decoder_ref_host.py shows on the host that at most one trial in eight is
left out at the seeds used (in fact none).

Why these launches are in bounds (read in csrc/xps_decoder.hip before they ran): a workgroup is 16 trials and 256 threads;
a dead trial (b >= B) computes on zeros, stores nothing to global memory (every global store is under live / b < B / b0 + r
< B) and reads the teacher row B - 1; the table row is clamped to 0 .. ntok - 1 before the gather; the FC stage indexes
lg[16][16], wfc[16][H + 1] with r < 16, c < C <= 16; all 16-byte accesses are at multiples of 4 floats from pointers the entry
point checked for alignment.  The backward indexes the same way (r = idx / (H / 4) < 16).

What no test of an output can see: the forward zeroes the state of a dead trial in LDS (`live ? .. : 0.f`).  A trial is one
column of the MFMA's B operand, one row of the FC stage and one token, so a dead trial's state reaches no live trial's output,
and its own stores are all guarded; removing that zeroing alone changes no bit of any output (tried on a scratch build).
"""
import functools

import numpy as np
import pytest
import torch

import decoder_ref as D
import gru_seq_ref as R
from guarded_buf import F32, Buf, Buf64

pytestmark = pytest.mark.gpu

INVALID = -1                         # XPS_E_INVALID
HS = (64, 128)


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


def _mult(mode):
    return 40.0 if mode == 'bf16x3' else 1.0


# ---- the cases of the direct kernel test -----------------------------------------------------------------------------------
#   name: (B, C, L, ntok, teacher, flags, regime)
#   teacher: None | 'range' (tokens in 0 .. ntok - 1) | 'wild' (some of them -3 and 40); flags: None | tuple of L ints
def _alt(L):
    return tuple(s % 2 for s in range(L))


CASES = {
    'model-37x9x3': (37, 9, 3, 10, 'range', (1, 0, 1), 'normal'),
    'smallest-1x1x1': (1, 1, 1, 2, None, None, 'normal'),
    'full_tile-16x16x8': (16, 16, 8, 17, None, None, 'normal'),
    'second_workgroup-17x16x8': (17, 16, 8, 17, 'range', _alt(8), 'normal'),
    'all_teacher-15x15x8': (15, 15, 8, 16, 'range', (1,) * 8, 'normal'),
    'argmax_clamps-33x9x8-ntok4': (33, 9, 8, 4, None, None, 'normal'),
    'teacher_clamps-19x5x4': (19, 5, 4, 6, 'wild', (1,) * 4, 'normal'),
    'teacher_without_flags-19x9x4': (19, 9, 4, 10, 'range', None, 'normal'),
    'exact_tie-20x9x4': (20, 9, 4, 10, None, None, 'normal'),
    'saturating-19x9x3': (19, 9, 3, 10, None, None, 'saturating'),
}
TIE_BIAS = 40.0      # |h| <= 1, so |h . w_c| <= sum_k |w_ck| <= sqrt(H) <= 11.4, and |b_c| <= 0.1: rows 2 and 5 at bias 40 beat every other class


@functools.lru_cache(maxsize=None)
def _problem(name, H):
    B, Cn, L, ntok, teacher, flags, regime = CASES[name]
    rng = np.random.default_rng([list(CASES).index(name), H])
    inp = D.decoder_inputs(rng, B, H, Cn, L, ntok, regime)
    if name.startswith('exact_tie'):
        inp.w_fc[5] = inp.w_fc[2]
        inp.b_fc[2] = inp.b_fc[5] = TIE_BIAS
    t = None
    if teacher is not None:
        t = rng.integers(0, ntok, (B, L))
        if teacher == 'wild':
            t[::3, :] = -3
            t[1::3, :] = 40
    dlogits = rng.standard_normal((B, L, Cn)).astype(F32)
    for a in (*inp, dlogits):
        a.setflags(write=False)
    return dict(inp=inp, teacher=t, flags=flags, dlogits=dlogits, start=ntok - 1, dims=(B, H, Cn, L, ntok), replay={})


def _replay(P, tokens):
    """float64 replay for the kernel's tokens and the float32 restatement's max error per output, cached on the problem (the two
    precisions choose the same tokens unless an argmax is nearly tied)."""
    key = tokens.tobytes()
    if key not in P['replay']:
        ref = D.replay(P['inp'], tokens, P['dlogits'])
        r32 = D.replay(P['inp'], tokens, P['dlogits'], dtype=F32)
        P['replay'][key] = (ref, {k: float(np.abs(r32[k].astype(np.float64) - ref[k]).max()) for k in ref})
    return P['replay'][key]


# ---- launches ----------------------------------------------------------------------------------------------------------------
class Device:
    """The inputs of one problem on the device; `off` names buffers to start 4 bytes past a 16-byte boundary."""

    def __init__(self, P, off=()):
        B, H, Cn, L, ntok = self.dims = P['dims']
        inp = P['inp']
        o = lambda k: int(k in off)
        self.off = off
        self.table = Buf(inp.table.size, data=inp.table, off=o('table'))
        self.w_hh = Buf(inp.w_hh.size, data=inp.w_hh, off=o('w_hh'))
        self.w_hh_t = Buf(inp.w_hh.size, data=np.ascontiguousarray(inp.w_hh.T), off=o('w_hh_t'))
        self.b_hh = Buf(inp.b_hh.size, data=inp.b_hh, off=o('b_hh'))
        self.h0 = Buf(inp.h0.size, data=inp.h0)
        self.w_fc = Buf(inp.w_fc.size, data=inp.w_fc)
        self.b_fc = Buf(inp.b_fc.size, data=inp.b_fc)
        self.dlogits = Buf(P['dlogits'].size, data=P['dlogits'])
        self.teacher = None if P['teacher'] is None else Buf64(P['teacher'].size, data=P['teacher'])
        # int32 flags carried in a float32 buffer bit for bit
        self.flags = None if P['flags'] is None else Buf(L, data=np.asarray(P['flags'], np.int32).view(F32))
        assert self.flags is None or self.flags.view().view(torch.int32).tolist() == list(P['flags'])
        self.start = P['start']

    def inputs(self):
        return [b for b in (self.table, self.w_hh, self.w_hh_t, self.b_hh, self.h0, self.w_fc, self.b_fc, self.dlogits,
                            self.teacher, self.flags) if b is not None]

    def forward(self, save=True, dims=None, start=None):
        """dims: the sizes passed to the entry point (the refusal tests pass other ones than the buffers were made for)."""
        B, H, Cn, L, ntok = self.dims
        o = lambda k: int(k in self.off)
        out = dict(logits=Buf(B * L * Cn), tokens=Buf64(L * B), hs=Buf((L + 1) * B * H, off=o('hs')),
                   saved=Buf(L * B * 4 * H, off=o('saved')) if save else None)
        aB, aH, aC, aL, antok = dims or self.dims
        rc = _lib().xps_decoder_fwd_f32(self.table.ptr, self.w_hh.ptr, self.b_hh.ptr, self.h0.ptr, self.w_fc.ptr, self.b_fc.ptr,
                                        None if self.teacher is None else self.teacher.ptr,
                                        None if self.flags is None else self.flags.ptr,
                                        out['logits'].ptr, out['tokens'].ptr, out['hs'].ptr, out['saved'].ptr if save else None,
                                        aB, aH, aC, aL, antok, self.start if start is None else start, _stream())
        torch.cuda.synchronize()
        return rc, out

    def backward(self, hs, saved, dims=None):
        B, H, Cn, L, ntok = self.dims
        o = lambda k: int(k in self.off)
        out = dict(dgi=Buf(L * B * 3 * H, off=o('dgi')), dghn=Buf(L * B * H, off=o('dghn')), dh0=Buf(B * H))
        aB, aH, aC, aL, _ = dims or self.dims
        rc = _lib().xps_decoder_bwd_f32(self.dlogits.ptr, hs.ptr, saved.ptr, self.w_hh_t.ptr, self.w_fc.ptr,
                                        out['dgi'].ptr, out['dghn'].ptr, out['dh0'].ptr, aB, aH, aC, aL, _stream())
        torch.cuda.synchronize()
        return rc, out


def _written(buf, what):
    assert buf.guards_intact(), f'{what}: a guard row was written'
    assert bool(torch.isfinite(buf.view()).all()), f'{what}: an element is not finite (or was never written)'


def _same(a, b, what):
    assert torch.equal(a.bits(), b.bits()), f'{what}: two launches differ'


def _ratio(err, bound, what):
    ratio = err / bound
    worst = float(ratio.max())
    assert worst <= 1.0, f'{what}: error / bound = {worst:.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)} (error {err.max():.3e})'
    return worst


def check_forward(dev, P, mode):
    """Three launches (two with `saved`, one without) and every forward check of the module docstring.  Returns the output
    buffers and the largest error / bound of hs, saved and logits."""
    B, H, Cn, L, ntok = dev.dims
    inp = P['inp']
    rc, out = dev.forward()
    assert rc == 0, _lib().xps_last_error()
    for k in ('logits', 'hs', 'saved'):
        _written(out[k], k)
    assert out['tokens'].guards_intact(), 'tokens: a guard row was written'
    tokens = out['tokens'].numpy((L, B))
    assert tokens.min() >= 0 and tokens.max() <= ntok - 1, 'tokens: out of range (or never written)'
    rc2, out2 = dev.forward()
    assert rc2 == 0
    for k in out:
        _same(out[k], out2[k], k)
    rc3, out3 = dev.forward(save=False)
    assert rc3 == 0
    for k in ('logits', 'tokens', 'hs'):
        _same(out[k], out3[k], k + ' with saved = NULL')
    assert all(b.unchanged() for b in dev.inputs()), 'a read-only input changed'

    hs = out['hs'].numpy((L + 1, B, H))
    saved = out['saved'].numpy((L, B, 4, H))
    logits = out['logits'].numpy((B, L, Cn))
    np.testing.assert_array_equal(hs[0].view(np.int32), inp.h0.view(np.int32))
    assert (tokens[0] == P['start']).all()
    worst = dict(hs=0.0, saved=0.0, logits=0.0)
    for s in range(L):
        ref, parts = D.step(inp.table, tokens[s], inp.w_hh, inp.b_hh, hs[s])
        gb = R.gate_bounds(parts, mode, 'hw')
        worst['hs'] = max(worst['hs'], _ratio(np.abs(hs[s + 1] - ref), gb['h'], f'hs, step {s}'))
        for i, k in enumerate('rznq'):
            worst['saved'] = max(worst['saved'], _ratio(np.abs(saved[s, :, i] - parts[k]), gb[k], f'saved {k}, step {s}'))
        err = np.abs(logits[:, s] - D.logits_ref(hs[s + 1], inp.w_fc, inp.b_fc))
        worst['logits'] = max(worst['logits'], _ratio(err, D.logits_bound(hs[s + 1], inp.w_fc, inp.b_fc), f'logits, step {s}'))
        if s + 1 < L:
            use = P['teacher'] is not None and P['flags'] is not None
            want = D.next_tokens(logits[:, s], P['teacher'][:, s] if use else None, P['flags'][s] if use else 0, ntok)
            np.testing.assert_array_equal(tokens[s + 1], want, err_msg=f'token rule after step {s}')
    return out, tokens, worst


def check_backward(dev, P, mode, out, tokens):
    B, H, Cn, L, ntok = dev.dims
    hs_bits, saved_bits = out['hs'].bits().clone(), out['saved'].bits().clone()
    rc, got = dev.backward(out['hs'], out['saved'])
    assert rc == 0, _lib().xps_last_error()
    rc2, again = dev.backward(out['hs'], out['saved'])
    assert rc2 == 0
    ref, e32 = _replay(P, tokens)
    worst = 0.0
    for k, shape in (('dgi', (L, B, 3 * H)), ('dghn', (L, B, H)), ('dh0', (B, H))):
        _written(got[k], k)
        _same(got[k], again[k], k)
        tol = 4 * _mult(mode) * e32[k] + 1e-4 * max(1.0, float(np.abs(ref[k]).max()))
        err = float(np.abs(got[k].numpy(shape).astype(np.float64) - ref[k]).max())
        worst = max(worst, err / tol)
        assert err <= tol, f'{k}: error {err:.3e} > tolerance {tol:.3e} (float32 restatement {e32[k]:.3e})'
    assert all(b.unchanged() for b in dev.inputs()), 'a read-only input changed'
    assert torch.equal(out['hs'].bits(), hs_bits) and torch.equal(out['saved'].bits(), saved_bits), 'the backward wrote hs or saved'
    return worst


def check_rails(P, out, tokens):
    """The saturating regime: where the float64 pre-activation is beyond the point at which the float32 arithmetic of
    rcp(1 + exp(-x)) has only one answer, the stored gate is exactly that answer.  x >= 18: exp(-x) < 2^-25, 1 + e rounds to
    1.  x <= -89.5: -x log2(e) > 129, the hardware exponential overflows to +inf and rcp(inf) = 0.  tanh(x) = 2 s(2 x) - 1:
    x >= 10 gives s = 1, x <= -10 gives 2 s <= 2^-25 and -1 after the rounding.  Every planted +-100 must land there."""
    B, H, Cn, L, ntok = P['dims']
    inp = P['inp']
    hs = out['hs'].numpy((L + 1, B, H))
    saved = out['saved'].numpy((L, B, 4, H))
    hit = {}
    for s in range(L):
        _, p = D.step(inp.table, tokens[s], inp.w_hh, inp.b_hh, hs[s])
        planted = np.abs(p['gi']) == R.PLANTED
        pre = [p['gi'][0] + p['gh'][0] + p['bh'][0], p['gi'][1] + p['gh'][1] + p['bh'][1], p['gi'][2] + p['r'] * p['q']]
        for g, (name, hi, lo, low_value) in enumerate((('r', 18.0, -89.5, 0.0), ('z', 18.0, -89.5, 0.0), ('n', 10.0, -10.0, -1.0))):
            val = saved[s, :, g]
            up, down = pre[g] >= hi, pre[g] <= lo
            assert (val[up] == 1.0).all(), f'{name}, step {s}: not exactly 1 on the upper rail'
            assert (val[down] == low_value).all(), f'{name}, step {s}: not exactly {low_value} on the lower rail'
            hit[(name, '+')] = hit.get((name, '+'), 0) + int((up & planted[g] & (p['gi'][g] > 0)).sum())
            hit[(name, '-')] = hit.get((name, '-'), 0) + int((down & planted[g] & (p['gi'][g] < 0)).sum())
    assert len(hit) == 6 and min(hit.values()) > 0, f'a planted entry never reached its rail: {hit}'


# Largest error / bound (hs, saved, logits) and backward error / tolerance as this file measured them on an MI355X: an
# observation of how much room the derived bounds leave, not a tolerance.  The tests assert <= 1.  The backward figures are
# small because the floor 1e-4 max(1, max |ref|) of the project's rule dominates the tolerance at these sizes.
#   case                           H   fp32: hs saved logits bwd   bf16x3: hs saved logits bwd
#   model-37x9x3                  64   0.174 0.404 0.033 0.004   0.127 0.183 0.037 0.008
#   model-37x9x3                 128   0.186 0.513 0.017 0.007   0.094 0.150 0.019 0.008
#   smallest-1x1x1                64   0.088 0.174 0.003 0.000   0.089 0.103 0.001 0.002
#   smallest-1x1x1               128   0.192 0.352 0.001 0.000   0.084 0.101 0.001 0.001
#   full_tile-16x16x8             64   0.189 0.491 0.045 0.007   0.146 0.236 0.036 0.010
#   full_tile-16x16x8            128   0.212 0.450 0.024 0.007   0.124 0.165 0.022 0.009
#   second_workgroup-17x16x8      64   0.173 0.405 0.053 0.006   0.148 0.192 0.041 0.009
#   second_workgroup-17x16x8     128   0.199 0.536 0.017 0.009   0.133 0.145 0.026 0.009
#   all_teacher-15x15x8           64   0.195 0.482 0.034 0.006   0.144 0.182 0.035 0.010
#   all_teacher-15x15x8          128   0.195 0.539 0.022 0.005   0.120 0.205 0.019 0.010
#   argmax_clamps-33x9x8-ntok4    64   0.201 0.456 0.037 0.005   0.131 0.190 0.040 0.007
#   argmax_clamps-33x9x8-ntok4   128   0.202 0.395 0.022 0.009   0.120 0.159 0.019 0.008
#   teacher_clamps-19x5x4         64   0.211 0.413 0.031 0.004   0.139 0.195 0.040 0.006
#   teacher_clamps-19x5x4        128   0.190 0.576 0.011 0.003   0.099 0.146 0.020 0.005
#   teacher_without_flags-19x9x4  64   0.197 0.410 0.030 0.004   0.121 0.183 0.039 0.008
#   teacher_without_flags-19x9x4 128   0.196 0.437 0.016 0.004   0.121 0.156 0.021 0.007
#   exact_tie-20x9x4              64   0.196 0.518 0.117 0.003   0.121 0.180 0.142 0.008
#   exact_tie-20x9x4             128   0.202 0.513 0.091 0.006   0.127 0.165 0.090 0.006
#   saturating-19x9x3             64   0.321 0.479 0.033   -     0.269 0.441 0.024   -
#   saturating-19x9x3            128   0.350 0.497 0.013   -     0.343 0.478 0.015   -
# The Python decode paths (test_decode_functions_vs_fp64_replay): error / tolerance at most 0.009 in fp32 and 0.064 in bf16x3.
WORST = {}


@pytest.mark.parametrize('H', HS)
@pytest.mark.parametrize('name', list(CASES))
def test_decoder_kernels_vs_fp64(name, H, gemm_precision):
    mode = gemm_precision
    P = _problem(name, H)
    B, _, Cn, L, ntok = P['dims']
    assert _lib().xps_decoder_supported(H, Cn, L) == 1
    dev = Device(P)
    out, tokens, worst = check_forward(dev, P, mode)
    regime = CASES[name][6]
    if name.startswith('argmax_clamps'):
        logits = out['logits'].numpy((B, L, Cn))
        assert (logits[:, :-1].argmax(-1) > ntok - 1).any(), 'no argmax above ntok - 1: the case does not clamp'
        assert tokens.max() == ntok - 1
    if name.startswith('teacher_clamps'):
        assert (tokens[1:, ::3] == 0).all() and (tokens[1:, 1::3] == ntok - 1).all()
    if name.startswith('teacher_without_flags'):
        logits = out['logits'].numpy((B, L, Cn))
        np.testing.assert_array_equal(tokens[1:], logits[:, :-1].argmax(-1).T)
        assert (tokens[1:] != P['teacher'][:, :-1].T).any()
    if name.startswith('exact_tie'):
        logits = out['logits'].numpy((B, L, Cn))
        np.testing.assert_array_equal(logits[..., 2].view(np.int32), logits[..., 5].view(np.int32))
        assert (logits[..., 2:3] >= logits).all() and (tokens[1:] == 2).all()
    bwd = float('nan')
    if regime == 'saturating':
        check_rails(P, out, tokens)
    else:
        bwd = check_backward(dev, P, mode, out, tokens)
    print(f'{name} H={H} {mode}: max error / bound  hs {worst["hs"]:.3f}  saved {worst["saved"]:.3f}  logits {worst["logits"]:.3f}'
          f'  backward error / tolerance {bwd:.3f}')
    WORST[(name, H, mode)] = (worst, bwd)


@pytest.mark.parametrize('case', list(D.FREE_RUN_SEEDS))
def test_free_run_tokens_equal_the_float64_decode_where_its_margins_hold(case, gemm_precision):
    H, B, Cn, L = case
    inp = D.free_run_inputs(H, B, Cn, L)
    want, _, margins = _free_run_ref(case)
    P = dict(inp=inp, teacher=None, flags=None, dlogits=np.zeros((B, L, Cn), F32), start=Cn, dims=(B, H, Cn, L, Cn + 1))
    rc, out = Device(P).forward(save=False)
    assert rc == 0, _lib().xps_last_error()
    tokens = out['tokens'].numpy((L, B))
    keep = margins.min(0) >= D.MARGIN
    assert keep.mean() >= 1 - D.MAX_EXCLUDED
    np.testing.assert_array_equal(tokens[:, keep], want[:, keep])
    print(f'free run H={H} B={B} C={Cn} L={L} {gemm_precision}: {int(keep.sum())} of {B} trials compared, all tokens equal')


@functools.lru_cache(maxsize=None)
def _free_run_ref(case):
    H, B, Cn, L = case
    return D.free_run(D.free_run_inputs(H, B, Cn, L), None, None, Cn, L=L)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
BASE = (3, 64, 4, 2, 5)              # B, H, C, L, ntok of the valid call every refusal departs from


@functools.lru_cache(maxsize=None)
def _base_problem():
    B, H, Cn, L, ntok = BASE
    rng = np.random.default_rng(77)
    inp = D.decoder_inputs(rng, B, 128, 17, L, ntok, 'normal')         # buffers large enough for every size a refusal names
    return dict(inp=inp, teacher=None, flags=None, dlogits=rng.standard_normal((B, 9, 17)).astype(F32), start=ntok - 1,
                dims=(B, 128, 17, 9, ntok), replay={})


def _dims(**kw):
    d = dict(zip('BHCLn', BASE))
    d.update(kw)
    return tuple(d[k] for k in 'BHCLn')


FWD_REFUSALS = {f'{k}={v}': (dict([(k, v)]), None, ()) for k, v in
                [('H', 32), ('H', 96), ('C', 0), ('C', 17), ('L', 0), ('L', 9), ('B', 0), ('n', 0)]}
FWD_REFUSALS.update({'start_token=ntok': ({}, BASE[4], ()), 'start_token=-1': ({}, -1, ())})
FWD_REFUSALS.update({f'misaligned-{k}': ({}, None, (k,)) for k in ('table', 'w_hh', 'b_hh', 'hs', 'saved')})
BWD_REFUSALS = {f'{k}={v}': (dict([(k, v)]), ()) for k, v in
                [('H', 32), ('H', 96), ('C', 0), ('C', 17), ('L', 0), ('L', 9), ('B', 0)]}
BWD_REFUSALS.update({f'misaligned-{k}': ({}, (k,)) for k in ('hs', 'saved', 'w_hh_t', 'dgi', 'dghn')})


@pytest.mark.parametrize('name', list(FWD_REFUSALS))
def test_forward_refuses_before_any_launch(name):
    """XPS_CHECK_ARG returns before the launch (csrc/xps_decoder.hip): XPS_E_INVALID and not one element of an output written.
    The buffers are sized for the largest shape named, so even a launch that did happen would stay inside them."""
    kw, start, off = FWD_REFUSALS[name]
    P = _base_problem()
    dev = Device(P, off=off)
    rc, out = dev.forward(dims=_dims(**kw), start=P['start'] if start is None else start)
    assert rc == INVALID, name
    assert all(b.untouched() for b in out.values()), 'a refused call wrote an output'
    assert all(b.unchanged() for b in dev.inputs())
    assert _lib().xps_last_error()
    if not off and start is None:                        # the same buffers and the valid sizes: accepted
        rc, out = dev.forward(dims=_dims())
        assert rc == 0, _lib().xps_last_error()


@pytest.mark.parametrize('name', list(BWD_REFUSALS))
def test_backward_refuses_before_any_launch(name):
    kw, off = BWD_REFUSALS[name]
    P = _base_problem()
    B, H, Cn, L, ntok = P['dims']
    dev = Device(P, off=off)
    # an hs / saved pair as a forward would have left them (finite values)
    hs = Buf((L + 1) * B * H, data=np.zeros((L + 1) * B * H, F32), off=int('hs' in off))
    saved = Buf(L * B * 4 * H, data=np.full(L * B * 4 * H, 0.5, F32), off=int('saved' in off))
    rc, out = dev.backward(hs, saved, dims=_dims(**kw))
    assert rc == INVALID, name
    assert all(b.untouched() for b in out.values()), 'a refused call wrote an output'
    assert all(b.unchanged() for b in dev.inputs() + [hs, saved])
    if not off:
        rc, out = dev.backward(hs, saved, dims=_dims())
        assert rc == 0, _lib().xps_last_error()


# ---- the table scatter of the gradient tail, beyond 16 rows ----------------------------------------------------------------------
@pytest.mark.parametrize('n_rows', [16, 17, 21, 64])
def test_scatter_rows_vs_fp64(n_rows):
    """xps_scatter_rows_f32 up to its 64 table rows (a decoder of C classes has C + 1): 150 batch rows (three chunks of 64, the
    last ragged), 70 columns (a ragged second strip), indices that collide, and a row nothing feeds.  Each entry is a float32
    sum of at most 150 terms in some order: |error| <= gamma_150 * sum |terms| (u = 2^-24); accumulate adds one rounding."""
    Bn, cols = 150, 70
    rng = np.random.default_rng(n_rows)
    dout = rng.standard_normal((Bn, cols)).astype(F32)
    idx = rng.integers(0, n_rows - 1, Bn)                                 # row n_rows - 1 is never fed
    idx[:40] = 3
    prior = rng.standard_normal((n_rows, cols)).astype(F32)
    ref, mass = np.zeros((n_rows, cols)), np.zeros((n_rows, cols))
    np.add.at(ref, idx, dout.astype(np.float64))
    np.add.at(mass, idx, np.abs(dout).astype(np.float64))
    bound = (Bn + 1) * R.U / (1 - (Bn + 1) * R.U) * (mass + np.abs(prior))
    lib = _lib()
    d_in, i_in = Buf(dout.size, data=dout), Buf64(Bn, data=idx)
    nbytes = lib.xps_scatter_rows_f32_workspace(Bn, cols, n_rows)
    for accumulate in (0, 1):
        outs = []
        for _ in range(2):
            ws = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
            out = Buf(n_rows * cols, data=prior) if accumulate else Buf(n_rows * cols)
            assert lib.xps_scatter_rows_f32(d_in.ptr, i_in.ptr, out.ptr, Bn, cols, n_rows, accumulate, ws.data_ptr(), nbytes,
                                            _stream()) == 0, lib.xps_last_error()
            torch.cuda.synchronize()
            outs.append(out)
        out = outs[0]
        _same(out, outs[1], 'dtable')
        if accumulate:
            guards = torch.cat([out.buf[:out.lo], out.buf[out.lo + out.n:]])
            assert bool(torch.isnan(guards).all())
        else:
            _written(out, 'dtable')
        got = out.numpy((n_rows, cols)).astype(np.float64)
        want = ref + prior if accumulate else ref
        assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
        if not accumulate:
            assert not got[n_rows - 1].any()
    assert d_in.unchanged() and i_in.unchanged()


def test_scatter_rows_refuses_a_table_beyond_its_rows():
    lib = _lib()
    Bn, cols, n_rows = 8, 8, 65
    d_in, i_in, out = Buf(Bn * cols, data=np.ones(Bn * cols, F32)), Buf64(Bn, data=np.zeros(Bn)), Buf(n_rows * cols)
    nbytes = lib.xps_scatter_rows_f32_workspace(Bn, cols, n_rows)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
    assert lib.xps_scatter_rows_f32(d_in.ptr, i_in.ptr, out.ptr, Bn, cols, n_rows, 0, ws.data_ptr(), nbytes, _stream()) == INVALID
    torch.cuda.synchronize()
    assert out.untouched()


# ---- the Python decode paths on the same reference -------------------------------------------------------------------------------
#   (Function, H, B, C, L): DecoderFn = the one-launch kernels; DecoderWideFn by the route its recurrence takes
FN_SHAPES = {
    'fused-64x19x16x8': ('DecoderFn', 64, 19, 16, 8),
    'fused-128x17x1x1': ('DecoderFn', 128, 17, 1, 1),
    'wide_generic-20x19x9x4': ('DecoderWideFn', 20, 19, 9, 4),               # generic route, fused select
    'wide_generic_C20-68x19x20x3': ('DecoderWideFn', 68, 19, 20, 3),         # C > 16: gemm_nt + xps_next_token
    'wide_step-132x19x9x4': ('DecoderWideFn', 132, 19, 9, 4),                # per-step route
    'wide_resident-64x19x9x4': ('DecoderWideFn', 64, 19, 9, 4),              # resident route
    'fused_as_wide-64x19x9x4': ('DecoderFn', 64, 19, 9, 4),                  # the shape both Functions take
}
REGIMES = ('mixed', 'collide')
PARAMS = ('table', 'h0', 'w_hh', 'b_hh', 'w_fc', 'b_fc')
GRADS = ('dtable', 'dh0', 'dw_hh', 'db_hh', 'dw_fc', 'db_fc')


@functools.lru_cache(maxsize=None)
def _fn_problem(H, B, Cn, L, regime):
    """Keyed by shape, not by Function: the two Functions get the same data at the shape they share."""
    ntok = Cn + 1
    rng = np.random.default_rng([H, B, Cn, L, REGIMES.index(regime)])
    inp = D.decoder_inputs(rng, B, H, Cn, L, ntok, 'normal')
    if regime == 'mixed':                                   # in-range teacher tokens, flags 1, 0, 1, ..
        teacher, flags = rng.integers(0, Cn, (B, L)), tuple(1 - s % 2 for s in range(L))
    else:                                                   # every trial is fed token C // 2 after every step: L x B - B rows collide
        teacher, flags = np.full((B, L), Cn // 2), (1,) * L
    dlogits = rng.standard_normal((B, L, Cn)).astype(F32)
    return dict(inp=inp, teacher=teacher, flags=flags, dlogits=dlogits, start=Cn, dims=(B, H, Cn, L, ntok), replay={})


def _apply(fn_name, P):
    """One forward and backward through the autograd Function: (logits, tokens, six gradients) as numpy."""
    from cross_patient_speech_decoding_amd.nn_models import functional as XF
    B, H, Cn, L, ntok = P['dims']
    params = [torch.from_numpy(np.array(a)).cuda().requires_grad_(True) for a in P['inp']]
    table, w_hh, b_hh, h0, w_fc, b_fc = params
    teacher = torch.from_numpy(P['teacher']).cuda()
    flags = torch.tensor(P['flags'], dtype=torch.int32).cuda()
    logits, tokens = getattr(XF, fn_name).apply(table, h0, w_hh, b_hh, w_fc, b_fc, teacher, flags, P['start'], L)
    assert logits.shape == (B, L, Cn) and tokens.shape == (L, B) and tokens.dtype == torch.int64 and not tokens.requires_grad
    grads = torch.autograd.grad(logits, [table, h0, w_hh, b_hh, w_fc, b_fc], torch.from_numpy(P['dlogits']).cuda())
    torch.cuda.synchronize()
    return logits.detach().cpu().numpy(), tokens.cpu().numpy(), dict(zip(GRADS, (g.cpu().numpy() for g in grads)))


def _fn_tolerances(P, tokens, mode):
    ref, e32 = _replay(P, tokens)
    return ref, {k: 4 * _mult(mode) * e32[k] + 1e-4 * max(1.0, float(np.abs(ref[k]).max())) for k in ('logits',) + GRADS}


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('name', list(FN_SHAPES))
def test_decode_functions_vs_fp64_replay(name, regime, gemm_precision):
    fn_name, H, B, Cn, L = FN_SHAPES[name]
    from cross_patient_speech_decoding_amd.nn_models import functional as XF
    assert XF.decoder_supported(H, Cn, L) == (H in HS and Cn <= 16)
    P = _fn_problem(H, B, Cn, L, regime)
    ntok = P['dims'][4]
    logits, tokens, grads = _apply(fn_name, P)
    # the token rule, exactly, on the returned logits
    assert (tokens[0] == P['start']).all()
    for s in range(L - 1):
        np.testing.assert_array_equal(tokens[s + 1], D.next_tokens(logits[:, s], P['teacher'][:, s], P['flags'][s], ntok))
    if regime == 'collide':
        assert (tokens[1:] == Cn // 2).all()
    ref, tol = _fn_tolerances(P, tokens, gemm_precision)
    got = dict(grads, logits=logits)
    worst = {}
    for k in ('logits',) + GRADS:
        assert got[k].shape == ref[k].shape and np.isfinite(got[k]).all(), k
        err = float(np.abs(got[k].astype(np.float64) - ref[k]).max())
        worst[k] = err / tol[k]
        assert err <= tol[k], f'{k}: error {err:.3e} > tolerance {tol[k]:.3e}'
    # rows of the table no step fed have a gradient of exactly zero
    unfed = sorted(set(range(ntok)) - set(int(t) for t in tokens.ravel()))
    assert not grads['dtable'][unfed].any()
    logits2, tokens2, grads2 = _apply(fn_name, P)
    np.testing.assert_array_equal(logits.view(np.int32), logits2.view(np.int32))
    np.testing.assert_array_equal(tokens, tokens2)
    for k in GRADS:
        np.testing.assert_array_equal(grads[k].view(np.int32), grads2[k].view(np.int32), err_msg=k)
    print(f'{name} {regime} {gemm_precision}: error / tolerance ' + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('regime', REGIMES)
def test_the_two_functions_agree_at_the_shape_both_take(regime, gemm_precision):
    """H = 64 is the one hidden size of the wide cases the one-launch kernels support too: in both token regimes DecoderFn and
    DecoderWideFn choose the same tokens and agree within twice the tolerance each is held to against the float64 replay."""
    _, H, B, Cn, L = FN_SHAPES['wide_resident-64x19x9x4']
    P = _fn_problem(H, B, Cn, L, regime)
    lf, tf, gf = _apply('DecoderFn', P)
    lw, tw, gw = _apply('DecoderWideFn', P)
    np.testing.assert_array_equal(tf, tw)
    _, tol = _fn_tolerances(P, tf, gemm_precision)
    assert float(np.abs(lf - lw).max()) <= 2 * tol['logits']
    for k in GRADS:
        assert float(np.abs(gf[k] - gw[k]).max()) <= 2 * tol[k], k
