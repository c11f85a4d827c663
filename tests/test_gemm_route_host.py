"""xps_gemm_route / xps_gemm_tn_grouped_route (host logic; the library loads without a device and then assumes 256 CUs) swept
against tests/gemm_route_ref.py: anchors on every route, every attribute of an anchor moved alone under every switch setting
and in pairs under the defaults, and a census -- every code of include/xps.h must have been answered at least once."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

import gemm_route_ref as R
from cross_patient_speech_decoding_amd import _lib, _switches

ALIGNED, MISALIGNED = 0x7f0000001000, 0x7f0000001004            # looked at, never through
BIGRPG = 1 << 30
SWITCH_VALUES = dict(XPS_GEMM_PRECISION=(1, 0), XPS_GEMM_SMALL_TILE_BLOCKS=(2048, 0), XPS_GEMM_LONGK_128=(1, 0), XPS_GEMM_BIG=(1, 0),
                     XPS_GEMM_DMA=(1, 0), XPS_PROJ_WS=(1, 0), XPS_GEMM_BIG_DEEP=(0, 1), XPS_GEMM_BIG_MIN_TILES=(192, 1),
                     XPS_GEMM_BIG_TAIL=(1, 0), XPS_TN_BLOCKS=(512, 64), XPS_TN_UNIFORM=(0, 1), XPS_GEMM_BIG_DEEP_TN=(0, 1),
                     XPS_TN_REDUCE=(0, 1, 2))
PLAIN_SWITCHES = ['XPS_GEMM_PRECISION', 'XPS_GEMM_SMALL_TILE_BLOCKS', 'XPS_GEMM_LONGK_128', 'XPS_GEMM_BIG', 'XPS_GEMM_DMA', 'XPS_PROJ_WS',
                  'XPS_GEMM_BIG_DEEP', 'XPS_GEMM_BIG_MIN_TILES', 'XPS_GEMM_BIG_TAIL']
TN_SWITCHES = ['XPS_GEMM_PRECISION', 'XPS_GEMM_BIG', 'XPS_GEMM_DMA', 'XPS_GEMM_BIG_DEEP', 'XPS_TN_BLOCKS', 'XPS_TN_UNIFORM',
               'XPS_GEMM_BIG_DEEP_TN', 'XPS_TN_REDUCE']


def _cus():
    """what the library's cached CU query answers: the current device's count, 256 without a device"""
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count if torch.cuda.is_available() else 256


def _switch_settings(names):
    """the defaults, every switch alone at each other value, every pair of switches at their other values"""
    other = [(n, v) for n in names for v in SWITCH_VALUES[n][1:]]
    yield {}
    for n, v in other:
        yield {n: v}
    for (n1, v1), (n2, v2) in itertools.combinations(other, 2):
        if n1 != n2:
            yield {n1: v1, n2: v2}


def test_defaults_and_codes_are_the_headers_and_the_librarys():
    with open(_lib.HEADER_PATH) as f:
        defs = {k: int(v) for k, v in re.findall(r'#define XPS_GEMM_(\w+) (\d+)', f.read())}
    mine = {'FORM_' + k: getattr(R, 'FORM_' + k) for k in ('NT', 'NN', 'NN2', 'NT_MULTI')}
    mine.update({'ROUTE_' + k: getattr(R, k) for k in ('REFUSED', 'NONE', 'SMALL_M', 'SKINNY', 'BIG', 'BIG_DEEP', 'BIG_DMA', 'TILE', 'TILE_128',
                                                     'TILE_EDGE', 'TILE_BF', 'TILE_PRE', 'PROJ_WS', 'TN_EDGE', 'TN_BF', 'TN_PRE', 'TN_DEEP',
                                                     'TN_UNIFORM', 'TN_FLAT')})
    mine.update({'TN_CLASS_' + k: getattr(R, 'TN_CLASS_' + k) for k in ('128', 'BIG', 'BIG_DMA')})
    assert defs == mine
    lib_rows = _switches.library_switches()
    for name, (default, *_) in SWITCH_VALUES.items():
        assert R.DEFAULTS[name] == default
        if name not in os.environ:
            assert lib_rows[name] == default, name
    assert _lib.SIGNATURES['xps_gemm_route'][1][:2] == [C.c_int, C.c_void_p] and len(_lib.SIGNATURES['xps_gemm_route'][1]) == 15
    assert len(_lib.SIGNATURES['xps_gemm_tn_grouped_route'][1]) == 5


# ---- nt / nn / nn2 / nt_multi -----------------------------------------------------------------------------------------------
# a case: the shape, per operand its alignment / padding of the leading dimension / rows per group / format, and nprob
BASE = dict(K2=0, a=True, b=True, a2=True, b2=True, padA=0, padB=0, rpgA=0, rpgB=0, rpgC=0, gs=0, fmtA=0, fmtB=0, nprob=1)
SPLIT = dict(fmtA=1, fmtB=1)
ANCHORS = [dict(form=R.FORM_NT, M=16, N=128, K=64), dict(form=R.FORM_NT, M=17, N=128, K=64), dict(form=R.FORM_NT, M=128, N=128, K=64),
           dict(form=R.FORM_NT, M=130, N=132, K=64), dict(form=R.FORM_NT, M=4096, N=3072, K=64), dict(form=R.FORM_NT, M=4096, N=3072, K=64, **SPLIT),
           dict(form=R.FORM_NT, M=81920, N=256, K=64), dict(form=R.FORM_NT, M=65536, N=512, K=1024),
           dict(form=R.FORM_NN, M=128, N=128, K=64), dict(form=R.FORM_NN, M=4096, N=3072, K=96), dict(form=R.FORM_NN, M=4096, N=3072, K=96, **SPLIT),
           dict(form=R.FORM_NN, M=24576, N=100, K=512, padB=256, **SPLIT),
           dict(form=R.FORM_NN2, M=24576, N=100, K=1536, K2=1536, padB=256, **SPLIT), dict(form=R.FORM_NN2, M=4096, N=3072, K=96, K2=160),
           dict(form=R.FORM_NN2, M=130, N=132, K=64, K2=20),
           dict(form=R.FORM_NT_MULTI, M=4096, N=128, K=32, nprob=2), dict(form=R.FORM_NT_MULTI, M=4096, N=128, K=256, nprob=2, **SPLIT),
           dict(form=R.FORM_NT_MULTI, M=4096, N=1536, K=112, nprob=2), dict(form=R.FORM_NT_MULTI, M=4096, N=1536, K=320, nprob=2, **SPLIT),
           dict(form=R.FORM_NT_MULTI, M=81920, N=256, K=512, nprob=1), dict(form=R.FORM_NT_MULTI, M=130, N=132, K=64, nprob=3)]
AXES = dict(M=[1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257, 4095, 4096, 4097, 4352, 24320, 24576, 65536, 81920],
            N=[4, 100, 127, 128, 129, 132, 255, 256, 257, 512, 3072, 3073],
            K=[0, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 80, 96, 100, 160, 192, 224, 252, 256, 260, 480, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097],
            K2=[0, 15, 16, 31, 32, 64, 100, 512], a=[True, False], b=[True, False], a2=[True, False], b2=[True, False],
            padA=[0, 1, 4], padB=[0, 1, 4, 256], rpgA=[0, 1], rpgB=[0, 1], rpgC=[0, 1], gs=[0, 1], fmtA=[0, 1, 2], fmtB=[0, 1, 2], nprob=[1, 2, 3, 4])


def _ask(case, sw, seen):
    """the library's and the restatement's answer for one case; both must agree"""
    c = dict(BASE, **case)
    form, M, N, K, K2, nprob = c['form'], c['M'], c['N'], c['K'], c['K2'], c['nprob']
    BK = form in (R.FORM_NT, R.FORM_NT_MULTI)
    brows, bcols = (N, K) if BK else (max(K, K2), N)
    gs = 4096 * 4 + c['gs']                                           # (an odd group stride: no 16-byte loads)
    ra = R.Map(max(K, K2) + c['padA'], M // 2 if c['rpgA'] and M > 1 else BIGRPG, gs, c['fmtA'])
    rb = R.Map(max(bcols, c['padB']) if c['padB'] == 256 else bcols + c['padB'], brows // 2 if c['rpgB'] and brows > 1 else BIGRPG, gs, c['fmtB'])
    rc = R.Map(N, M // 2 if c['rpgC'] and M > 1 else BIGRPG, gs, 0)
    ptr = lambda al: ALIGNED if al else MISALIGNED
    cmaps = [_lib.RowMap(m.gs, m.ld, m.rpg, m.fmt) for m in (ra, rb, rc)]
    lead, tail = C.c_int(-7), C.c_int(-7)
    if form == R.FORM_NT_MULTI:
        bals = [c['b'] if i == nprob - 1 else True for i in range(nprob)]          # (the LAST pointer is the odd one)
        barr = (C.c_void_p * nprob)(*[ptr(al) for al in bals])
        want = R.route_multi(sw, c['a'], ra, bals, rb, rc, nprob, M, N, K)
        b_arg = C.cast(barr, C.c_void_p)
    else:
        want = R.route_plain(sw, form, c['a'], ra, c['b'], rb, rc, M, N, K, c['a2'], c['b2'], K2)
        b_arg = ptr(c['b'])
    got = _lib.lib().xps_gemm_route(form, ptr(c['a']), C.byref(cmaps[0]), b_arg, C.byref(cmaps[1]), ptr(c['a2']), ptr(c['b2']),
                                    C.byref(cmaps[2]), M, N, K, K2, nprob, C.byref(lead), C.byref(tail))
    assert (got, lead.value, tail.value) == want, (c, sw, (got, lead.value, tail.value), want)
    seen[form].add(got)
    seen['tail'].add(tail.value)
    if tail.value != R.NONE:
        assert 0 < lead.value < M and lead.value % 256 == 0 and R.BIG <= got <= R.BIG_DMA


def _moved(anchor, k):
    """the anchor with k of its attributes moved to other values"""
    for keys in itertools.combinations(AXES, k):
        for values in itertools.product(*(AXES[key] for key in keys)):
            yield dict(anchor, **dict(zip(keys, values)))


def test_route_query_equals_the_restated_rule_on_every_route():
    cus = _cus()
    seen = {f: set() for f in R.CODES}
    seen['tail'] = set()
    tail_m = 256 * (cus + cus // 4)                                    # one whole round and a quarter: the 256-tile launch splits
    anchors = [dict(a, M=tail_m) if a['M'] == 81920 else a for a in ANCHORS]
    for setting in _switch_settings(PLAIN_SWITCHES):
        sw = R.switches(cus=cus, **setting)
        with _switches.override(**setting):
            for anchor in anchors:
                for case in _moved(anchor, 1):
                    _ask(case, sw, seen)
                if not setting:
                    for case in _moved(anchor, 2):
                        _ask(case, sw, seen)
    for form, codes in R.CODES.items():
        assert seen[form] == set(codes), (form, sorted(set(codes) - seen[form]), sorted(seen[form] - set(codes)))
    # a tail is a 128- / 64-row tile launch, or (XPS_GEMM_BIG_MIN_TILES=1) another 256-tile launch
    assert R.NONE in seen['tail'] and any(t & R.TILE for t in seen['tail']) and any(R.BIG <= t <= R.BIG_DMA for t in seen['tail'])


def test_route_query_refuses_what_the_entry_points_reject_and_reports_nothing_for_empty_products():
    l = _lib.lib()
    m = _lib.RowMap(0, 64, BIGRPG, 0)
    args = lambda form, M=32, N=32, K=64, nprob=1, A=ALIGNED, A2=ALIGNED: (
        form, A, C.byref(m), ALIGNED, C.byref(m), A2, ALIGNED, C.byref(m), M, N, K, 0, nprob, None, None)
    assert l.xps_gemm_route(*args(R.FORM_NT)) == (R.TILE | R.TILE_128 | R.TILE_EDGE | R.TILE_BF)        # (NULL out-parameters)
    assert l.xps_gemm_route(*args(R.FORM_NT, M=0)) == R.NONE and l.xps_gemm_route(*args(R.FORM_NN, N=0)) == R.NONE
    for bad in (args(-1), args(4), args(R.FORM_NT, M=-1), args(R.FORM_NT, A=None), args(R.FORM_NN2, A2=None)):
        assert l.xps_gemm_route(*bad) == R.REFUSED
    barr = (C.c_void_p * 4)(*[ALIGNED] * 4)
    for nprob in (0, 5):
        assert l.xps_gemm_route(R.FORM_NT_MULTI, ALIGNED, C.byref(m), C.cast(barr, C.c_void_p), C.byref(m), None, None, C.byref(m),
                                32, 32, 64, 0, nprob, None, None) == R.REFUSED


# ---- grouped TN ---------------------------------------------------------------------------------------------------------------
TN_BASE = dict(a=True, b=True, padA=0, padB=0, fmtA=0, fmtB=0)
TN_ANCHORS = [[dict(M=256, N=256, K=4096), dict(M=256, N=256, K=4096, fmtA=1, fmtB=1), dict(M=130, N=100, K=4096)],
              [dict(M=256, N=256, K=4096)], [dict(M=1536, N=1024, K=8192)], [dict(M=128, N=128, K=64)],
              [dict(M=128, N=128, K=512), dict(M=384, N=128, K=512)],
              [dict(M=1024, N=512, K=40960, fmtA=1, fmtB=1), dict(M=1536, N=100, K=40960, fmtA=1)],
              [dict(M=5888, N=2560, K=8192)]]                 # 230 tiles of 256 x 256: the fewest that make one round of splits
TN_AXES = dict(M=[1, 4, 127, 128, 130, 255, 256, 258, 512, 5632], N=[1, 100, 128, 132, 256, 260], K=[0, 16, 63, 64, 65, 512, 4080, 4095, 4096, 4112, 8192, 40960],
               a=[True, False], b=[True, False], padA=[0, 1, 4], padB=[0, 1, 4], fmtA=[0, 1, 2], fmtB=[0, 1, 2])


def _ask_tn(group, sw, seen):
    probs, cprobs = [], (_lib.TnProblem * len(group))()
    for i, p in enumerate(group):
        p = dict(TN_BASE, **p)
        ra, rb = R.Map(p['M'] + p['padA'], BIGRPG, 0, p['fmtA']), R.Map(p['N'] + p['padB'], BIGRPG, 0, p['fmtB'])
        probs.append(R.TnProblem(p['a'], ra, p['b'], rb, p['M'], p['N'], p['K']))
        q = cprobs[i]
        q.A, q.B, q.C = (ALIGNED if p['a'] else MISALIGNED), (ALIGNED if p['b'] else MISALIGNED), ALIGNED
        q.ra, q.rb, q.rc = (_lib.RowMap(m.gs, m.ld, m.rpg, m.fmt) for m in (ra, rb, R.Map(p['N'])))
        q.M, q.N, q.K = p['M'], p['N'], p['K']
    n = len(group)
    cls, sp, kc = ((C.c_int * n)(*[-7] * n) for _ in range(3))
    got = _lib.lib().xps_gemm_tn_grouped_route(C.cast(cprobs, C.c_void_p), n, C.cast(cls, C.c_void_p), C.cast(sp, C.c_void_p),
                                               C.cast(kc, C.c_void_p))
    want = R.tn_plan(sw, probs)
    if want is None:
        assert got == -1, (group, sw, got)
        seen['refused'] += 1
        return
    assert (got, list(cls), list(sp), list(kc)) == want, (group, sw, (got, list(cls), list(sp), list(kc)), want)
    seen['flags'].add(got)
    seen['cls'].update(cls)
    # the instantiation of the 128-tile launch, where one happens
    if R.TN_CLASS_128 in list(cls):
        seen['tile'].add(got & (R.TN_EDGE | R.TN_BF | R.TN_PRE))


def test_grouped_route_query_equals_the_restated_plan():
    seen = dict(flags=set(), cls=set(), tile=set(), refused=0)
    for setting in _switch_settings(TN_SWITCHES):
        sw = R.switches(**setting)
        with _switches.override(**setting):
            for group in TN_ANCHORS:
                _ask_tn(group, sw, seen)
                for i, key in itertools.product(range(len(group)), TN_AXES):
                    for v in TN_AXES[key]:
                        _ask_tn(group[:i] + [dict(group[i], **{key: v})] + group[i + 1:], sw, seen)
    assert seen['cls'] == {R.TN_CLASS_128, R.TN_CLASS_BIG, R.TN_CLASS_BIG_DMA} and seen['refused'] > 0
    for flag in (R.TN_EDGE, R.TN_BF, R.TN_PRE, R.TN_DEEP, R.TN_UNIFORM, R.TN_FLAT):
        assert any(f & flag for f in seen['flags']) and any(not f & flag for f in seen['flags']), flag
    # all six gemm_tn_grouped_kernel<EDGE, BF, PRE> instantiations
    assert seen['tile'] == {e | b for e in (0, R.TN_EDGE) for b in (0, R.TN_BF, R.TN_BF | R.TN_PRE)}
    l = _lib.lib()
    assert l.xps_gemm_tn_grouped_route(None, 1, None, None, None) == -1
    one = (_lib.TnProblem * 13)()
    assert l.xps_gemm_tn_grouped_route(C.cast(one, C.c_void_p), 13, None, None, None) == -1
