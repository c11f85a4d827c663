"""The GEMM dispatch rules of csrc/xps_gemm.hip restated in Python (route_gemm, route_gemm_multi, build_group): what
xps_gemm_route and xps_gemm_tn_grouped_route must answer.  tests/test_gemm_route_host.py sweeps the library against these
on the host; the GPU tests assert the route a case is named for before they run it.

An operand is (aligned, Map): whether its pointer is 16-byte aligned, and its row map.  `sw` holds the switches the rules
read, under their XPS_* names, and `cus`, the device's CU count (256 where the library finds no device)."""
import collections

Map = collections.namedtuple('Map', 'ld rpg gs fmt', defaults=(1 << 30, 0, 0))

# include/xps.h
FORM_NT, FORM_NN, FORM_NN2, FORM_NT_MULTI = 0, 1, 2, 3
REFUSED, NONE, SMALL_M, SKINNY, BIG, BIG_DEEP, BIG_DMA, TILE, PROJ_WS = 0, 1, 2, 3, 8, 12, 13, 16, 32
TILE_128, TILE_EDGE, TILE_BF, TILE_PRE = 1, 2, 4, 8
TN_CLASS_128, TN_CLASS_BIG, TN_CLASS_BIG_DMA = 0, 1, 2
TN_EDGE, TN_BF, TN_PRE, TN_DEEP, TN_UNIFORM, TN_FLAT = 1, 2, 4, 8, 16, 32

_TILES = [TILE | m | e | b for m in (0, TILE_128) for e in (0, TILE_EDGE) for b in (0, TILE_BF, TILE_BF | TILE_PRE)]
# every code an entry point can launch (the leading launch; NONE is a tail's)
CODES = {FORM_NT: [REFUSED, SMALL_M, BIG, BIG + 1, BIG + 2, BIG + 3, BIG_DEEP, BIG_DMA] + _TILES,
         FORM_NN: [REFUSED, SMALL_M, SKINNY, BIG, BIG + 1, BIG + 2, BIG + 3, BIG_DEEP, BIG_DMA] + _TILES,
         FORM_NT_MULTI: [REFUSED, BIG, BIG_DEEP, BIG_DMA] + [PROJ_WS + kt for kt in range(2, 17, 2)] + _TILES}
CODES[FORM_NN2] = CODES[FORM_NN]

DEFAULTS = dict(XPS_GEMM_PRECISION=1, XPS_GEMM_SMALL_TILE_BLOCKS=2048, XPS_GEMM_LONGK_128=1, XPS_GEMM_BIG=1, XPS_GEMM_DMA=1,
                XPS_PROJ_WS=1, XPS_GEMM_BIG_DEEP=0, XPS_GEMM_BIG_MIN_TILES=192, XPS_GEMM_BIG_TAIL=1, XPS_TN_BLOCKS=512,
                XPS_TN_UNIFORM=0, XPS_GEMM_BIG_DEEP_TN=0, XPS_TN_REDUCE=0, cus=256)
BM = BN = 128
BKT = 16
TM = TN = 256
SM_MAXM = 16


def switches(**changed):
    assert set(changed) <= set(DEFAULTS), changed
    return dict(DEFAULTS, **changed)


def cdiv(a, b):
    return -(-a // b)


def _vec_ok(al, m):
    return bool(al) and m.ld % 4 == 0 and m.gs % 4 == 0


def _split4(al, m, extent):
    """2: a servable XPS_FMT_SPLIT4 operand, 0: plain fp32, -1: not servable"""
    if m.fmt == 0:
        return 0
    return 2 if m.fmt == 1 and _vec_ok(al, m) and extent % 4 == 0 else -1


def _big_plain(al, m, rows):
    return bool(al) and m.ld % 4 == 0 and max(m.rpg, 1) >= rows


def _rpg(m):
    return max(m.rpg, 1)


def _small_tiles(sw, M, N, K):
    n128 = cdiv(M, 128) * cdiv(N, BN)
    if sw['XPS_GEMM_LONGK_128'] and K >= 1024 and n128 >= 512:
        return False
    return M > 64 and n128 < sw['XPS_GEMM_SMALL_TILE_BLOCKS']


def big_split_rows(sw, M, tiles_per_row_tile):
    cus = sw['cus']
    mt = M // TM
    total = mt * tiles_per_row_tile
    rounds, rem = divmod(total, cus)
    if not sw['XPS_GEMM_BIG_TAIL'] or rounds < 1 or rem == 0 or rem * 4 > cus * 3:
        return M
    mb = rounds * cus // tiles_per_row_tile
    return M if mb < 1 or mb >= mt else mb * TM


def _tile(sw, M, N, ncols, K, fmt):
    mi = 1 if _small_tiles(sw, M, ncols, K) else 2
    bf = sw['XPS_GEMM_PRECISION'] == 1
    edge = M % (64 * mi) != 0 or N % BN != 0
    return TILE | (TILE_128 if mi == 2 else 0) | (TILE_EDGE if edge else 0) | (TILE_BF if bf else 0) | (TILE_PRE if bf and fmt else 0)


def _with_tail(first, M):
    """(code, lead_rows, tail code) of a product whose leading launch is first(rows) -> (code, lead_rows)"""
    code, lead = first(M)
    if code == REFUSED or lead == M:
        return code, lead, NONE
    return code, lead, first(M - lead)[0]


def route_plain(sw, form, a, ra, b, rb, rc, M, N, K, a2=None, b2=None, K2=0):
    """nt (B [n][k]) / nn / nn2 (B [k][n]; a2, b2, K2: the second pair's alignments and contraction).  A is [m][k]."""
    BK = form == FORM_NT
    two = form == FORM_NN2
    if not two:
        a2 = b2 = None
        K2 = 0
    bf = sw['XPS_GEMM_PRECISION'] == 1

    def first(M):
        fA, fB = _split4(a, ra, K), _split4(b, rb, K if BK else N)
        if two and fA > 0:
            fA = _split4(a2, ra, K2)
        if two and fB > 0:
            fB = _split4(b2, rb, K2 if BK else N)
        if fA < 0 or fB < 0 or ((fA or fB) and (not bf or M <= SM_MAXM)):
            return REFUSED, M
        fmt = (1 if fA else 0) | (2 if fB else 0)
        if M <= SM_MAXM:
            return SMALL_M, M
        big_on = sw['XPS_GEMM_BIG'] and bf
        k32 = K % 32 == 0 and K2 % 32 == 0
        plain = (_big_plain(a, ra, M) and _big_plain(b, rb, N if BK else K) and
                 (not two or (_big_plain(a2, ra, M) and _big_plain(b2, rb, N if BK else K2))) and _rpg(rc) >= M)
        if (not BK and big_on and sw['XPS_GEMM_DMA'] and fmt == 3 and N < TN and N % 4 == 0 and rb.ld >= TN and M % TM == 0 and
                M // TM >= 96 and k32 and K + K2 >= 512 and plain):
            return SKINNY, M
        if (big_on and M % TM == 0 and N % TN == 0 and K % BKT == 0 and K2 % BKT == 0 and K >= 64 and
                (M // TM) * (N // TN) >= sw['XPS_GEMM_BIG_MIN_TILES'] and plain):
            lead = big_split_rows(sw, M, N // TN)
            if fmt == 3 and k32 and sw['XPS_GEMM_DMA']:
                return BIG_DMA, lead
            if sw['XPS_GEMM_BIG_DEEP'] and k32 and fmt == 0:
                return BIG_DEEP, lead
            return BIG + fmt, lead
        return _tile(sw, M, N, N, K + K2, fmt), M

    return _with_tail(first, M)


def route_multi(sw, a, ra, bs, rb, rc, nprob, M, N, K):
    """nt_multi: bs = the alignments of the nprob B pointers"""
    bf = sw['XPS_GEMM_PRECISION'] == 1
    bs = list(bs)[:nprob]

    def first(M):
        fA, fB = _split4(a, ra, K), 0
        for b in bs:
            fB = _split4(b, rb, K)
            if fB < 0:
                break
        if fA < 0 or fB < 0 or ((fA or fB) and not bf):
            return REFUSED, M
        fmt = (1 if fA else 0) | (2 if fB else 0)
        vb = all(_vec_ok(b, rb) for b in bs)
        if (bf and sw['XPS_PROJ_WS'] and 32 <= K <= 256 and K % 4 == 0 and N % 32 == 0 and nprob * N >= 256 and M >= 4096 and
                _vec_ok(a, ra) and vb and _rpg(ra) >= M and _rpg(rb) >= N and _rpg(rc) >= M):
            S = cdiv(nprob * N, 256)
            if (min(sw['cus'], cdiv(M, 64) * S) // S) * S >= S:
                return PROJ_WS + 2 * ((K + 31) // 32), M
        if (sw['XPS_GEMM_BIG'] and bf and M % TM == 0 and N % TN == 0 and K % BKT == 0 and K >= 64 and vb and
                (M // TM) * (N // TN) * nprob >= sw['XPS_GEMM_BIG_MIN_TILES'] and _big_plain(a, ra, M) and _rpg(rb) >= N and
                _rpg(rc) >= M):
            lead = big_split_rows(sw, M, (N // TN) * nprob)
            if fmt == 3 and K % 32 == 0 and sw['XPS_GEMM_DMA']:
                return BIG_DMA, lead
            if sw['XPS_GEMM_BIG_DEEP'] and K % 32 == 0 and fmt == 0:
                return BIG_DEEP, lead
            return BIG, lead
        return _tile(sw, M, N, N * nprob, K, fmt), M

    return _with_tail(first, M)


TnProblem = collections.namedtuple('TnProblem', 'a ra b rb M N K')      # A [k][m], B [k][n]


def tn_plan(sw, probs):
    """xps_gemm_tn_grouped_f32's plan: (group flags, [class], [splits], [kchunk]) or None where the list is refused"""
    n = len(probs)
    if n < 1 or n > 12 or any(q.M < 1 or q.N < 1 or q.K < 0 for q in probs):
        return None
    bf = sw['XPS_GEMM_PRECISION'] == 1
    isbig = [bool(sw['XPS_GEMM_BIG'] and bf and q.M % TM == 0 and q.N % TN == 0 and q.K % BKT == 0 and q.K >= 4096 and
                  _big_plain(q.a, q.ra, q.K) and _big_plain(q.b, q.rb, q.K)) for q in probs]
    tiles_big = sum((q.M // TM) * (q.N // TN) for q, big in zip(probs, isbig) if big)
    tiles_small = sum(cdiv(q.M, BM) * cdiv(q.N, BN) for q, big in zip(probs, isbig) if not big)
    sp_big = 1
    if tiles_big > 0:
        r1, r2 = 256 // tiles_big, 512 // tiles_big
        sp_big = r1 if r1 >= 1 and r1 * tiles_big >= 230 else max(r2, 1)
    cls, splits, kchunk, pres = [], [], [], []
    for q, big in zip(probs, isbig):
        tiles = cdiv(q.M, BM) * cdiv(q.N, BN)
        if big:
            sp = min(sp_big, q.K // 512)
        else:
            want = cdiv(sw['XPS_TN_BLOCKS'] * tiles // max(tiles_small, 1), tiles)
            sp = min(want, cdiv(max(q.K, 1), 64))
        sp = min(max(sp, 1), 256)
        kq = 32 if big and q.K % 32 == 0 else BKT
        fA, fB = _split4(q.a, q.ra, q.M), _split4(q.b, q.rb, q.N)
        if fA < 0 or fB < 0 or ((fA or fB) and not bf):
            return None
        cls.append((TN_CLASS_BIG_DMA if fA and fB and sw['XPS_GEMM_DMA'] else TN_CLASS_BIG) if big else TN_CLASS_128)
        splits.append(sp)
        kchunk.append(cdiv(cdiv(max(q.K, 1), sp), kq) * kq)
        pres.append(bool(fA or fB))
    uniform = n > 1 and all(q.K == probs[0].K for q in probs) and sw['XPS_TN_UNIFORM'] and probs[0].K > 0 and tiles_big == 0
    if uniform:
        sp = min(max(min(cdiv(sw['XPS_TN_BLOCKS'], tiles_small), cdiv(probs[0].K, 64)), 1), 256)
        splits = [sp] * n
        kchunk = [cdiv(cdiv(probs[0].K, sp), BKT) * BKT] * n
    small = [i for i in range(n) if not isbig[i]]
    edge = any(probs[i].M % BM or probs[i].N % BN for i in small)
    pre = bf and any(pres[i] for i in small)
    deep = bool(tiles_big > 0 and sw['XPS_GEMM_BIG_DEEP'] and sw['XPS_GEMM_BIG_DEEP_TN'] and
                all(kchunk[i] % 32 == 0 and probs[i].K % 32 == 0 and not pres[i] for i in range(n) if isbig[i]))
    flat = sw['XPS_TN_REDUCE'] == 1 or (sw['XPS_TN_REDUCE'] == 0 and max(splits) <= 32)
    flags = ((TN_EDGE if edge else 0) | (TN_BF if bf else 0) | (TN_PRE if pre else 0) | (TN_DEEP if deep else 0) |
             (TN_UNIFORM if uniform else 0) | (TN_FLAT if flat else 0))
    return flags, cls, splits, kchunk


# ---- asking the library (the GPU tests assert a leg's route before they run it) ---------------------------------------------
def ask(form, A, ra, B, rb, rc, M, N, K, A2=None, B2=None, K2=0, nprob=1):
    """xps_gemm_route for tensors (or raw pointers) and ctypes row maps as the launch takes them: (code, lead_rows, tail code).
    B of FORM_NT_MULTI: the list of the nprob weight tensors."""
    import ctypes as C
    from cross_patient_speech_decoding_amd._lib import lib
    p = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
    if form == FORM_NT_MULTI:
        arr = (C.c_void_p * nprob)(*[p(b) for b in B])
        b_arg = C.cast(arr, C.c_void_p)
    else:
        b_arg = p(B)
    lead, tail = C.c_int(-1), C.c_int(-1)
    code = lib().xps_gemm_route(form, p(A), C.byref(ra), b_arg, C.byref(rb), p(A2), p(B2), C.byref(rc), M, N, K, K2, nprob,
                                C.byref(lead), C.byref(tail))
    return code, lead.value, tail.value


def ask_tn(problems):
    """xps_gemm_tn_grouped_route for a list of _lib.TnProblem: (group flags, [class], [splits], [kchunk])"""
    import ctypes as C
    from cross_patient_speech_decoding_amd._lib import TnProblem, lib
    n = len(problems)
    arr = (TnProblem * n)(*problems)
    cls, sp, kc = ((C.c_int * n)() for _ in range(3))
    flags = lib().xps_gemm_tn_grouped_route(C.cast(arr, C.c_void_p), n, C.cast(cls, C.c_void_p), C.cast(sp, C.c_void_p),
                                            C.cast(kc, C.c_void_p))
    return flags, list(cls), list(sp), list(kc)


def is_tile(code, rows=None, pre=None):
    """code is a 64- / 128-row tile launch (rows: which; pre: whether it reads an XPS_FMT_SPLIT4 operand)"""
    return (TILE <= code < PROJ_WS and (rows is None or rows == (128 if code & TILE_128 else 64)) and
            (pre is None or pre == bool(code & TILE_PRE)))
