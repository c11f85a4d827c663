"""One GPU case per GEMM route (include/xps.h: XPS_GEMM_ROUTE_*, every form that can launch it).  A case first asserts what
xps_gemm_route / xps_gemm_tn_grouped_route answer -- the code it is named for, and the restated rule of tests/gemm_route_ref.py
-- then runs the product and holds it to float64: 1.6e-5 * sum |a||b| in bf16x3 mode, 4e-7 * sum |a||b| in
fp32 mode (tests/test_gpu_nn_kernels.py).  Where a switch sends the same operands down another route, that route is asserted
too and must give the same bits.  Shapes are the smallest that reach a route with more than one block."""
import ctypes as C

import pytest
import torch

import gemm_route_ref as R
from cross_patient_speech_decoding_amd import _build, _switches
from cross_patient_speech_decoding_amd._lib import call, rowmap

pytestmark = pytest.mark.gpu
S0 = dict(XPS_GEMM_SMALL_TILE_BLOCKS=0)                 # 128-row tiles for every tile launch
MIN1 = dict(XPS_GEMM_BIG_MIN_TILES=1)                   # 256 x 256 tiles from the first tile on
NAMES = {R.FORM_NT: 'nt', R.FORM_NN: 'nn', R.FORM_NN2: 'nn2', R.FORM_NT_MULTI: 'multi'}


@pytest.fixture(scope='module', autouse=True)
def _built():
    _build.build(verbose=False)
    assert torch.cuda.is_available(), 'gpu tests need the MI355X'


def XF():
    from cross_patient_speech_decoding_amd.nn_models import functional
    return functional


def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def tile_code(rows, edge, prec, pre):
    return R.TILE | (R.TILE_128 if rows == 128 else 0) | (R.TILE_EDGE if edge else 0) | (R.TILE_BF if prec else 0) | (R.TILE_PRE if pre else 0)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
# a leg: the switches, the operand formats and the route (code, or (code, lead rows, tail code)) they must give
def leg(code, sw=None, fa=0, fb=0):
    return dict(code=code, sw=dict(sw or {}), fa=fa, fb=fb)


def case(form, name, M, N, K, legs, K2=0, nprob=1, ldb=None):
    return dict(id=f'{NAMES[form]}-{name}', form=form, M=M, N=N, K=K, K2=K2 if form == R.FORM_NN2 else 0, nprob=nprob, ldb=ldb, legs=legs)


def direct_cases(form):
    multi = form == R.FORM_NT_MULTI
    np_t, np_b = (3, 2) if multi else (1, 1)
    out = []
    if not multi:
        out.append(case(form, 'small_m', 16, 128, 64, [leg(R.SMALL_M)], K2=32))
    if form == R.FORM_NT:
        out.append(case(form, 'tile128_edge-m17', 17, 128, 64, [leg(tile_code(128, True, 1, False))]))
    for rows, edge, (prec, pre) in [(r, e, p) for r in (64, 128) for e in (False, True) for p in ((0, 0), (1, 0), (1, 1))]:
        M, N = (130, 132) if edge else (128, 128)
        sw = lambda r: dict(S0 if r == 128 else {}, XPS_GEMM_PRECISION=prec)
        legs = [leg(tile_code(rows, edge, prec, pre), sw(rows), fa=pre), leg(tile_code(192 - rows, edge, prec, pre), sw(192 - rows), fa=pre)]
        if pre:
            legs.append(leg(tile_code(rows, edge, prec, False), sw(rows)))
        out.append(case(form, f'tile{rows}{"_edge" if edge else ""}-{"pre" if pre else "bf16x3" if prec else "fp32"}', M, N, 64, legs, K2=32,
                        nprob=np_t))
    # 256 x 256 tiles: two of them; K = 80 (+ 48): whole 16-deep but not 32-deep stages
    for f in ([0] if multi else [0, 1, 2, 3]):
        for fa, fb in ([(0, 0), (1, 1)] if multi else [(f & 1, f >> 1)]):
            out.append(case(form, f'big-fmt{fa + 2 * fb}', 512, 256, 80, K2=48, nprob=np_b,
                            legs=[leg(R.BIG + f, MIN1, fa, fb), leg(tile_code(64, False, 1, fa or fb), dict(MIN1, XPS_GEMM_BIG=0), fa, fb)]))
    deep = dict(MIN1, XPS_GEMM_BIG_DEEP=1)
    out.append(case(form, 'big_deep', 512, 256, 64, K2=32, nprob=np_b,
                    legs=[leg(R.BIG_DEEP, deep), leg(R.BIG, MIN1), leg(tile_code(64, False, 1, False), dict(deep, XPS_GEMM_BIG=0))]))
    out.append(case(form, 'big_dma', 512, 256, 64, K2=32, nprob=np_b,
                    legs=[leg(R.BIG_DMA, MIN1, 1, 1), leg(R.BIG if multi else R.BIG + 3, dict(MIN1, XPS_GEMM_DMA=0), 1, 1), leg(R.BIG, MIN1)]))
    if form in (R.FORM_NT, R.FORM_NT_MULTI):
        out.append(dict(case(form, 'big_tail', 0, 256, 320 if multi else 64, []), tail=True))      # (K > 256: not the projection kernel)
    if form in (R.FORM_NN, R.FORM_NN2):
        K, K2 = (256, 256) if form == R.FORM_NN2 else (512, 0)
        out.append(case(form, 'skinny', 24576, 100, K, K2=K2, ldb=256,
                        legs=[leg(R.SKINNY, None, 1, 1), leg(tile_code(64, True, 1, True), dict(XPS_GEMM_DMA=0), 1, 1)]))
    if multi:
        for K in range(32, 257, 32):
            f = 1 if K == 256 else 0
            out.append(case(form, f'proj_ws-kt{K // 16}', 4096, 128, K, nprob=2,
                            legs=[leg(R.PROJ_WS + K // 16, None, f, f), leg(tile_code(64, False, 1, f), dict(XPS_PROJ_WS=0), f, f)]))
    return out


def with_tail_rows(c, n):
    """the big_tail case on a device of n CUs: one whole round of 256 x 256 tiles and a quarter -- the 256-tile launch takes the
    round and 64-row tiles the rest; XPS_GEMM_BIG_TAIL=0: one launch; same bits from the tile kernels alone"""
    M, lead, tile = 256 * (n + n // 4), 256 * n, tile_code(64, False, 1, False)
    return dict(c, M=M, legs=[leg((R.BIG, lead, tile)), leg((R.BIG, M, R.NONE), dict(XPS_GEMM_BIG_TAIL=0)), leg(tile, dict(XPS_GEMM_BIG=0))])


CASES = [c for form in (R.FORM_NT, R.FORM_NN, R.FORM_NN2, R.FORM_NT_MULTI) for c in direct_cases(form)]


# ---- running a leg ------------------------------------------------------------------------------------------------------------
def operands(c):
    """seeded fp32 operands of a case and their XPS_FMT_SPLIT4 images: made once, never written"""
    g = torch.Generator(device='cuda').manual_seed(1000 * c['form'] + c['M'] + c['N'] + c['K'])
    rnd = lambda *shape, scale=1.0: torch.randn(*shape, generator=g, device='cuda') * scale
    M, N, K, K2, form = c['M'], c['N'], c['K'], c['K2'], c['form']
    ld = max(K, K2)
    o = dict(A=[rnd(M, ld)], bias=[rnd(N) for _ in range(c['nprob'])], C0=rnd(M, N))
    if form == R.FORM_NN2:
        o['A'].append(rnd(M, ld))
    if form in (R.FORM_NT, R.FORM_NT_MULTI):
        o['B'] = [rnd(N, K, scale=0.5) for _ in range(c['nprob'])]
    else:
        o['B'] = [rnd(k, N, scale=0.5) for k in ([K, K2] if form == R.FORM_NN2 else [K])]
    xf = XF()
    o['A4'] = [xf.split4(a) for a in o['A']]
    if c['ldb']:                                         # (skinny: zero-padded split4 images of B, and B itself padded alike)
        o['B4'] = [xf.split4_pad(b, c['ldb']) for b in o['B']]
        o['Bp'] = [torch.nn.functional.pad(b, (0, c['ldb'] - N)).contiguous() for b in o['B']]
    else:
        o['B4'], o['Bp'] = [xf.split4(b) for b in o['B']], o['B']
    return o


def launch_args(c, o, l):
    """(A tensors, B tensors, row maps) of a leg"""
    form, N, K, K2 = c['form'], c['N'], c['K'], c['K2']
    A, B = (o['A4'] if l['fa'] else o['A']), (o['B4'] if l['fb'] else o['Bp'])
    ldb = c['ldb'] or (K if form in (R.FORM_NT, R.FORM_NT_MULTI) else N)
    return A, B, (rowmap(max(K, K2), fmt=l['fa']), rowmap(ldb, fmt=l['fb']), rowmap(N))


def route_of(c, o, l):
    A, B, (ra, rb, rc) = launch_args(c, o, l)
    two = c['form'] == R.FORM_NN2
    return R.ask(c['form'], A[0], ra, B if c['form'] == R.FORM_NT_MULTI else B[0], rb, rc, c['M'], c['N'], c['K'],
                 A2=A[1] if two else None, B2=B[1] if two else None, K2=c['K2'], nprob=c['nprob'])


def restated(c, o, l):
    A, B, (ra, rb, rc) = launch_args(c, o, l)
    al = lambda t: t.data_ptr() % 16 == 0
    m = lambda r: R.Map(r.ld, r.rpg, r.gs, r.fmt)
    sw = R.switches(cus=cus(), **l['sw'])
    if c['form'] == R.FORM_NT_MULTI:
        return R.route_multi(sw, al(A[0]), m(ra), [al(b) for b in B], m(rb), m(rc), c['nprob'], c['M'], c['N'], c['K'])
    two = c['form'] == R.FORM_NN2
    return R.route_plain(sw, c['form'], al(A[0]), m(ra), al(B[0]), m(rb), m(rc), c['M'], c['N'], c['K'],
                         al(A[1]) if two else None, al(B[1]) if two else None, c['K2'])


def run_leg(c, o, l):
    """the leg's product(s): nt accumulates onto C0 with a bias, multi has a bias per problem, nn / nn2 overwrite NaNs"""
    xf = XF()
    A, B, (ra, rb, rc) = launch_args(c, o, l)
    form, M, N, K, K2 = c['form'], c['M'], c['N'], c['K'], c['K2']
    with _switches.override(**l['sw']):
        if form == R.FORM_NT:
            outs = [o['C0'].clone()]
            xf.gemm_nt(A[0], B[0], outs[0], M, N, K, bias=o['bias'][0], ra=ra, rb=rb, rc=rc, accumulate=True)
        elif form == R.FORM_NT_MULTI:
            outs = [torch.full((M, N), float('nan'), device='cuda') for _ in range(c['nprob'])]
            call('xps_gemm_nt_multi_f32', xf._ptr(A[0]), C.byref(ra), xf._ptr_array(B), C.byref(rb), xf._ptr_array(outs), C.byref(rc),
                 xf._ptr_array(o['bias']), c['nprob'], M, N, K, xf._stream())
        else:
            outs = [torch.full((M, N), float('nan'), device='cuda')]
            if form == R.FORM_NN:
                xf.gemm_nn(A[0], B[0], outs[0], M, N, K, ra=ra, rb=rb, rc=rc)
            else:
                call('xps_gemm_nn2_f32', xf._ptr(A[0]), xf._ptr(B[0]), K, xf._ptr(A[1]), xf._ptr(B[1]), K2, C.byref(ra), C.byref(rb),
                     xf._ptr(outs[0]), C.byref(rc), M, N, 0, xf._stream())
        torch.cuda.synchronize()
    return outs


def references(c, o):
    """float64 products and sum |a||b| (+ |bias| + |C0| where the entry adds them), one pair per output"""
    form, K, K2 = c['form'], c['K'], c['K2']
    a = [x.double() for x in o['A']]
    b = [x.double() for x in o['B']]
    if form == R.FORM_NT:
        return [(a[0] @ b[0].T + o['bias'][0].double() + o['C0'].double(), a[0].abs() @ b[0].abs().T + o['bias'][0].abs().double() + o['C0'].abs().double())]
    if form == R.FORM_NT_MULTI:
        return [(a[0] @ w.T + bi.double(), a[0].abs() @ w.abs().T + bi.abs().double()) for w, bi in zip(b, o['bias'])]
    ref, scale = a[0][:, :K] @ b[0], a[0][:, :K].abs() @ b[0].abs()
    if form == R.FORM_NN2:
        ref, scale = ref + a[1][:, :K2] @ b[1], scale + a[1][:, :K2].abs() @ b[1].abs()
    return [(ref, scale)]


@pytest.mark.parametrize('c', CASES, ids=[c['id'] for c in CASES])
def test_route_is_the_one_named_and_its_product_holds_to_fp64(c):
    if c.get('tail'):
        c = with_tail_rows(c, cus())
    o = operands(c)
    first = None
    for l in c['legs']:
        with _switches.override(**l['sw']):
            got = route_of(c, o, l)
            want = l['code'] if isinstance(l['code'], tuple) else (l['code'], c['M'], R.NONE)
            assert got == want, (c['id'], l, got)
            assert got == restated(c, o, l), (c['id'], l)
        outs = run_leg(c, o, l)
        if first is None:
            first = outs
            const = 1.6e-5 if l['sw'].get('XPS_GEMM_PRECISION', 1) else 4e-7
            for out, (ref, scale) in zip(outs, references(c, o)):
                err = (out.double() - ref).abs()
                print(f"{c['id']}: max err / (sum |a||b|) = {float((err / scale).max()):.3e} (bound {const:.1e})")
                assert bool((err <= const * scale).all()), (c['id'], float((err / scale).max()))
        else:
            for a, b in zip(first, outs):
                assert torch.equal(a, b), (c['id'], l)


# ---- grouped TN ---------------------------------------------------------------------------------------------------------------
def tn_case(name, shapes, legs):
    """shapes: (M, N, K, fa, fb, colsum) per problem"""
    return dict(id='tn-' + name, shapes=shapes, legs=legs)


def tn_leg(flags, cls, sw=None):
    return dict(flags=flags, cls=cls, sw=dict(sw or {}))


BIG3 = [(256, 256, 4096, 0, 0, True), (256, 256, 4096, 1, 1, True), (130, 100, 4096, 0, 0, False)]
CLS3 = [R.TN_CLASS_BIG, R.TN_CLASS_BIG_DMA, R.TN_CLASS_128]
DEEP_TN = dict(XPS_GEMM_BIG_DEEP=1, XPS_GEMM_BIG_DEEP_TN=1)
TN_CASES = [
    tn_case('big_dma_128-both_reduces', BIG3, [tn_leg(R.TN_EDGE | R.TN_BF | R.TN_FLAT, CLS3, dict(XPS_TN_REDUCE=1)),
                                             tn_leg(R.TN_EDGE | R.TN_BF, CLS3, dict(XPS_TN_REDUCE=2)),
                                             tn_leg(R.TN_EDGE | R.TN_BF, [R.TN_CLASS_BIG, R.TN_CLASS_BIG, R.TN_CLASS_128], dict(XPS_GEMM_DMA=0)),   # (auto: 64 splits > 32, looped)
                                             tn_leg(R.TN_EDGE | R.TN_BF | R.TN_PRE, [R.TN_CLASS_128] * 3, dict(XPS_GEMM_BIG=0))]),
    tn_case('big_deep', BIG3[:1] * 2, [tn_leg(R.TN_BF | R.TN_DEEP | R.TN_FLAT, [R.TN_CLASS_BIG] * 2, DEEP_TN),
                                       tn_leg(R.TN_BF | R.TN_FLAT, [R.TN_CLASS_BIG] * 2)]),
    tn_case('uniform', [(128, 128, 512, 0, 0, True), (384, 128, 512, 0, 0, False)],
            [tn_leg(R.TN_BF | R.TN_UNIFORM | R.TN_FLAT, [R.TN_CLASS_128] * 2, dict(XPS_TN_UNIFORM=1)), tn_leg(R.TN_BF | R.TN_FLAT, [R.TN_CLASS_128] * 2)]),
] + [tn_case(f'tile{"_edge" if edge else ""}-{"pre" if pre else "bf16x3" if prec else "fp32"}',
             [(132, 100, 256, pre, 0, True) if edge else (128, 128, 256, pre, 0, True)],
             [tn_leg((R.TN_EDGE if edge else 0) | (R.TN_BF if prec else 0) | (R.TN_PRE if pre else 0) | R.TN_FLAT, [R.TN_CLASS_128],
                     dict(XPS_GEMM_PRECISION=prec))])
     for edge in (False, True) for prec, pre in ((0, 0), (1, 0), (1, 1))]


def tn_operands(c):
    g = torch.Generator(device='cuda').manual_seed(7 + len(c['shapes']) + c['shapes'][0][0])
    xf = XF()
    o = []
    for M, N, K, fa, fb, cs in c['shapes']:
        A, B = torch.randn(K, M, generator=g, device='cuda'), torch.randn(K, N, generator=g, device='cuda') * 0.5
        o.append(dict(A=xf.split4(A) if fa else A, B=xf.split4(B) if fb else B, A64=A.double(), B64=B.double()))
    return o


def tn_problems(c, o):
    xf = XF()
    outs = [(torch.full((M, N), float('nan'), device='cuda'), torch.full((M,), float('nan'), device='cuda') if cs else None)
            for M, N, K, fa, fb, cs in c['shapes']]
    probs = [xf.tn_problem(p['A'], p['B'], out, M, N, K, ra=rowmap(M, fmt=fa), rb=rowmap(N, fmt=fb), rc=rowmap(N), colsum_out=col)
             for p, (out, col), (M, N, K, fa, fb, cs) in zip(o, outs, c['shapes'])]
    return probs, outs


def run_tn_leg(c, o, l):
    with _switches.override(**l['sw']):
        probs, outs = tn_problems(c, o)
        keep = XF().gemm_tn_grouped(probs, 'cuda')
        torch.cuda.synchronize()
        del keep
    return outs


@pytest.mark.parametrize('c', TN_CASES, ids=[c['id'] for c in TN_CASES])
def test_grouped_plan_is_the_one_named_and_its_products_hold_to_fp64(c):
    """Legs of one case split k differently or sum the slabs in another order: each is held to float64 on its own (the product
    bound plus the 1e-5 the grouped tests of tests/test_gpu_gemm_big.py allow for the slab sums; column sums of an
    XPS_FMT_SPLIT4 operand within 2^-16 sum |a|), not to the other legs' bits."""
    o = tn_operands(c)
    for l in c['legs']:
        with _switches.override(**l['sw']):
            probs, _ = tn_problems(c, o)
            flags, cls, splits, kchunk = R.ask_tn(probs)
            assert (flags, cls) == (l['flags'], l['cls']), (c['id'], l, flags, cls)
            al = lambda t: t.data_ptr() % 16 == 0
            want = R.tn_plan(R.switches(**l['sw']), [R.TnProblem(al(p['A']), R.Map(M, fmt=fa), al(p['B']), R.Map(N, fmt=fb), M, N, K)
                                                   for p, (M, N, K, fa, fb, cs) in zip(o, c['shapes'])])
            assert (flags, cls, splits, kchunk) == want, (c['id'], l)
        outs = run_tn_leg(c, o, l)
        const = 1.6e-5 if l['sw'].get('XPS_GEMM_PRECISION', 1) else 4e-7
        for p, (out, col) in zip(o, outs):
            err = (out.double() - p['A64'].T @ p['B64']).abs()
            scale = p['A64'].abs().T @ p['B64'].abs()
            print(f"{c['id']} {l['sw']}: max err / (sum |a||b|) = {float((err / scale).max()):.3e} (bound {const:.1e})")
            assert bool((err <= const * scale + 1e-5).all()), (c['id'], l, float((err / scale).max()))
            if col is not None:
                cerr = (col.double() - p['A64'].sum(0)).abs()
                assert bool((cerr <= 2.0 ** -16 * p['A64'].abs().sum(0) + 1e-6).all()), (c['id'], l, float(cerr.max()))
