"""Plain numpy restatement of the CTC posterior occupancies (xps_ctc_occupancy, include/xps.h), written from the header's
contract in the header's operation order, the error bounds its tests hold the device to, and a brute force over all frame
labellings that shares nothing with the recursion.  Host only: numpy, math and itertools, no torch and no import of the
package under test.

Contract.  l' = (blank, l_1, blank, ..., l_L, blank), S = 2 L + 1, x_t(c) the score widened to float64, [skip s] = s odd,
s >= 3 and l'_s != l'_{s-2}:
    a_0(0) = x_0(blank), a_0(1) = x_0(l_1), else -inf
    a_t(s) = x_t(l'_s) + lse(a_{t-1}(s), a_{t-1}(s-1), [skip s] a_{t-1}(s-2))
    b_{Tb-1}(S-1) = x(l'_{S-1}), b_{Tb-1}(S-2) = x(l'_{S-2}), else -inf
    b_t(s) = x_t(l'_s) + lse(b_{t+1}(s), b_{t+1}(s+1), [skip s+2] b_{t+1}(s+2))
    log_z  = lse(a_{Tb-1}(S-1), a_{Tb-1}(S-2))
    g_t(s) = exp(((a_t(s) + b_t(s)) - x_t(l'_s)) - log_z), 0 where a or b is -inf
    onset_0(j) = g_0(2j+1)
    onset_t(j) = exp((lse(a_{t-1}(2j), [skip 2j+1] a_{t-1}(2j-1)) + b_t(2j+1)) - log_z), 0 where the lse or b is -inf
lse(p1, p2, p3) = log((exp(p1 - m) + exp(p2 - m)) + exp(p3 - m)) + m, m the maximum, an absent term -inf, -inf when m is.
class_occ adds g_t(s) over the states of a class by increasing s; expected_frames = sum_t g_t(2j+1) and
onset_mean = sum_t t onset_t(j) add their frames from Tb - 1 down to 0.  log_z = -inf (or no frames): posteriors 0,
expected_frames 0, onset_mean NaN; tokens past L: 0, 0 and NaN; frames past Tb: 0.  Tb = 0: log_z 0 for L = 0, else -inf.

Error model of the bounds (as DESIGN.md 4.9b derives the loss kernel's; u = 2^-53).  exp and log: at most FN_ULPS = 2 ulps, a
relative error of 2 FN_ULPS u = 4 u.  The scores are exact inputs.
* One step of a (b alike).  lse is a convex combination of its inputs' perturbations, so inherited errors enter as the
  MAXIMUM over the finite inputs.  The three-term lse itself: e_i = exp(p_i - m), one of them exp(0), 1 <= sum <= 3; the
  subtraction roundings u sum |d_i| e^{d_i} <= (2 / e) u, exp 4 u, two additions 2 u, log 4 u log 3 = 4.4 u: less than
  LSE3_C u = 12 u.  `+ m` rounds by u |lse|, `x +` by u |a_t(s)|:
      E_t(s) = max_{finite inputs i} E_{t-1}(i) + 12 u + u |a_t(s) - x| + u |a_t(s)|,   E_0(s) = 0.
  A state that is -inf in exact arithmetic is -inf in any arithmetic (structure, not value) and carries no error.
* log_z: dz = max(E(S-1), E(S-2)) + 12 u + u |log_z|.
* g_t(s) = exp(v), v = ((a + b) - x) - log_z: dv = E_t(s) + E^b_t(s) + u |a + b| + u |(a + b) - x| + u |v| + dz, and since
  g <= 1 the absolute bound dg = expm1(dv) + 4 u.
* onset_t(j) = exp(w), w = (l + b) - log_z, l the lse of a_{t-1}: dl = max over its finite inputs of E_{t-1} + 12 u + u |l|,
  dw = dl + E^b_t(2j+1) + u |l + b| + u |w| + dz, donset = expm1(dw) + 4 u.  onset_0 = g_0.
* class_occ, n states of the class: sum of their dg + (n - 1) u (sum g + sum dg).
* expected_frames: sum_t dg + (Tb - 1) u (sum_t g + sum_t dg).
* onset_mean: the term t onset carries t donset + u t onset; the sum (Tb - 1) u (sum + sum of the terms' errors) more.
No constant here comes from a measurement of the kernel."""
import itertools
import math

import numpy as np

U = 2.0 ** -53
FN_ULPS = 2.0
FN = 2.0 * FN_ULPS
LSE3_C = 12.0
NINF = -np.inf

MUTANTS = ('no_skip', 'skip_across_repeat', 'beta_one_frame_late', 'onset_without_skip')
OUTPUTS = ('log_z', 'token_occ', 'onset', 'class_occ', 'expected_frames', 'onset_mean')


def _lse3(p1, p2, p3):
    """Elementwise, in the header's order; -inf where every term is -inf."""
    m = np.maximum(p1, np.maximum(p2, p3))
    dead = np.isneginf(m)
    ms = np.where(dead, m.dtype.type(0), m)
    with np.errstate(divide='ignore'):
        out = np.log((np.exp(p1 - ms) + np.exp(p2 - ms)) + np.exp(p3 - ms)) + ms
    return np.where(dead, m, out)


def _shift(a, k, fill):
    """a[s - k] at position s (k > 0) or a[s + |k|] (k < 0), `fill` where that runs off the row."""
    out = np.full_like(a, fill)
    if k > 0:
        out[k:] = a[:-k] if k < len(a) else a[:0]
    else:
        out[:k] = a[-k:] if -k < len(a) else a[:0]
    return out


def _fin(v, e):
    return np.where(np.isfinite(v), e, 0.0)


def occupancy_one(x, target, blank, dtype=np.float64, mutant=None, bounds=False):
    """x (Tb, C) scores, target (L,) labels -> dict of log_z (scalar), token_occ (Tb, L), onset (Tb, L), class_occ (Tb, C),
    expected_frames (L,), onset_mean (L,) in `dtype`; with bounds (float64 only) also 'bound', a dict of the same keys."""
    dt = np.dtype(dtype).type
    x = np.asarray(x).astype(dt)
    Tb, C = x.shape
    target = [int(v) for v in target]
    L = len(target)
    S = 2 * L + 1
    ninf = dt(NINF)
    out = dict(log_z=ninf, token_occ=np.zeros((Tb, L), dt), onset=np.zeros((Tb, L), dt), class_occ=np.zeros((Tb, C), dt),
               expected_frames=np.zeros(L, dt), onset_mean=np.full(L, np.nan, dt))
    zero_b = dict(log_z=0.0, token_occ=np.zeros((Tb, L)), onset=np.zeros((Tb, L)), class_occ=np.zeros((Tb, C)),
                  expected_frames=np.zeros(L), onset_mean=np.zeros(L))
    if bounds:
        out['bound'] = zero_b
    if Tb == 0:
        out['log_z'] = dt(0) if L == 0 else ninf
        return out
    lab = np.full(S, blank, np.int64)
    lab[1::2] = target
    odd = np.arange(S) % 2 == 1
    skip_f = np.zeros(S, bool)                              # s - 2 -> s allowed
    skip_f[3:] = odd[3:] & (lab[3:] != lab[1:-2])
    if mutant == 'skip_across_repeat':
        skip_f[3:] = odd[3:]
    if mutant == 'no_skip':
        skip_f[:] = False
    skip_b = np.zeros(S, bool)                              # s -> s + 2 allowed, seen from s
    skip_b[:-2] = skip_f[2:]
    xl = x[:, lab]                                          # (Tb, S)
    with np.errstate(invalid='ignore', over='ignore'):
        a = np.full((Tb, S), ninf, dt)
        a[0, :2] = xl[0, :2]
        for t in range(1, Tb):
            p = a[t - 1]
            a[t] = xl[t] + _lse3(p, _shift(p, 1, ninf), np.where(skip_f, _shift(p, 2, ninf), ninf))
        one = np.full(1, ninf, dt)
        lz = _lse3(a[Tb - 1, S - 1:S], a[Tb - 1, S - 2:S - 1] if S > 1 else one, one)[0]
        out['log_z'] = lz
        if bounds:
            Ea = np.zeros((Tb, S))
            for t in range(1, Tb):
                e = _fin(a[t - 1], Ea[t - 1])
                inh = np.maximum(e, np.maximum(_shift(e, 1, 0.0), np.where(skip_f, _shift(e, 2, 0.0), 0.0)))
                Ea[t] = _fin(a[t], inh + LSE3_C * U + U * np.abs(a[t] - xl[t]) + U * np.abs(a[t]))
            dz = max(Ea[Tb - 1, S - 1], Ea[Tb - 1, S - 2] if S > 1 else 0.0) + LSE3_C * U + U * abs(float(lz))
            zero_b['log_z'] = float(dz) if np.isfinite(lz) else 0.0
        if lz == ninf:
            return out
        b = np.full((Tb, S), ninf, dt)
        t_last = Tb - 2 if (mutant == 'beta_one_frame_late' and Tb >= 2) else Tb - 1
        b[t_last, max(S - 2, 0):] = xl[t_last, max(S - 2, 0):]
        for t in range(t_last - 1, -1, -1):
            n = b[t + 1]
            b[t] = xl[t] + _lse3(n, _shift(n, -1, ninf), np.where(skip_b, _shift(n, -2, ninf), ninf))
        dead = np.isneginf(a) | np.isneginf(b)
        ab = a + b
        abx = ab - xl
        v = abx - lz
        g = np.where(dead, dt(0), np.exp(np.where(dead, dt(0), v)))
        # onset: the mass that enters state 2j+1 at frame t
        prev = np.vstack([np.full((1, S), ninf, dt), a[:-1]])                    # a_{t-1}, frame 0: none
        p1 = np.stack([_shift(r, 1, ninf) for r in prev])
        p2 = np.stack([np.where(skip_f, _shift(r, 2, ninf), ninf) for r in prev])
        if mutant == 'onset_without_skip':
            p2 = np.full_like(p2, ninf)
        l = np.stack([_lse3(p1[t], p2[t], np.full(S, ninf, dt)) for t in range(Tb)])
        odead = np.isneginf(l) | np.isneginf(b)
        lb = l + b
        w = lb - lz
        on = np.where(odead, dt(0), np.exp(np.where(odead, dt(0), w)))
        on[0] = g[0]
    out['token_occ'], out['onset'] = g[:, 1::2].copy(), on[:, 1::2].copy()
    classes = [(c, np.flatnonzero(lab == c)) for c in np.unique(lab)]
    for c, idx in classes:
        acc = g[:, idx[0]].copy()
        for s in idx[1:]:
            acc = acc + g[:, s]
        out['class_occ'][:, c] = acc
    ef, om = np.zeros(L, dt), np.zeros(L, dt)
    for t in range(Tb - 1, -1, -1):
        ef = ef + g[t, 1::2]
        om = om + dt(t) * on[t, 1::2]
    out['expected_frames'], out['onset_mean'] = ef, om
    if not bounds:
        return out
    Eb = np.zeros((Tb, S))
    for t in range(Tb - 2, -1, -1):
        e = _fin(b[t + 1], Eb[t + 1])
        inh = np.maximum(e, np.maximum(_shift(e, -1, 0.0), np.where(skip_b, _shift(e, -2, 0.0), 0.0)))
        with np.errstate(invalid='ignore'):
            Eb[t] = _fin(b[t], inh + LSE3_C * U + U * np.abs(b[t] - xl[t]) + U * np.abs(b[t]))
    fa = lambda q: np.where(np.isfinite(q), np.abs(q), 0.0)                      # noqa: E731
    dv = Ea + Eb + U * fa(ab) + U * fa(abx) + U * fa(v) + dz
    dg = np.where(dead, 0.0, np.expm1(dv) + FN * U)
    ea_prev = np.vstack([np.zeros((1, S)), _fin(a[:-1], Ea[:-1])])
    inh = np.maximum(np.stack([_shift(r, 1, 0.0) for r in ea_prev]),
                     np.stack([np.where(skip_f, _shift(r, 2, 0.0), 0.0) for r in ea_prev]))
    dw = inh + LSE3_C * U + U * fa(l) + Eb + U * fa(lb) + U * fa(w) + dz
    don = np.where(odead, 0.0, np.expm1(dw) + FN * U)
    don[0] = dg[0]
    g64, on64 = g.astype(np.float64), on.astype(np.float64)
    zero_b['token_occ'], zero_b['onset'] = dg[:, 1::2].copy(), don[:, 1::2].copy()
    for c, idx in classes:
        sd = dg[:, idx].sum(1)
        zero_b['class_occ'][:, c] = sd + (len(idx) - 1) * U * (g64[:, idx].sum(1) + sd)
    sd = dg[:, 1::2].sum(0)
    zero_b['expected_frames'] = sd + (Tb - 1) * U * (g64[:, 1::2].sum(0) + sd)
    tt = np.arange(Tb, dtype=np.float64)[:, None]
    terms = tt * on64[:, 1::2]
    te = (tt * don[:, 1::2] + U * terms).sum(0)
    zero_b['onset_mean'] = te + (Tb - 1) * U * (terms.sum(0) + te)
    return out


def occupancy_ref(scores, targets, in_len, tg_len, blank, dtype=np.float64, mutant=None, bounds=False):
    """scores (B, T, C), targets (B, Lmax) ints, in_len / tg_len (B,) ints or None (clamped to 0..T / 0..Lmax) -> dict of
    log_z (B,), token_occ (B, T, Lmax), onset (B, T, Lmax), class_occ (B, T, C), expected_frames (B, Lmax), onset_mean (B, Lmax)
    in `dtype`, padded as the header says; with bounds also 'bound', a dict of float64 arrays of the same shapes (0 on the
    padding, which is exact)."""
    assert mutant is None or mutant in MUTANTS
    dt = np.dtype(dtype).type
    scores = np.asarray(scores)
    B, T, C = scores.shape
    targets = np.asarray(targets, np.int64).reshape(B, -1)
    Lmax = targets.shape[1]
    in_len = np.full(B, T) if in_len is None else np.clip(np.asarray(in_len, np.int64), 0, T)
    tg_len = np.full(B, Lmax) if tg_len is None else np.clip(np.asarray(tg_len, np.int64), 0, Lmax)

    def blank_out(d):
        return dict(log_z=np.zeros(B, d), token_occ=np.zeros((B, T, Lmax), d), onset=np.zeros((B, T, Lmax), d),
                    class_occ=np.zeros((B, T, C), d), expected_frames=np.zeros((B, Lmax), d), onset_mean=np.zeros((B, Lmax), d))
    out, bd = blank_out(dt), blank_out(np.float64)
    out['onset_mean'][:] = np.nan
    for i in range(B):
        Tb, L = int(in_len[i]), int(tg_len[i])
        r = occupancy_one(scores[i, :Tb], targets[i, :L], blank, dtype, mutant, bounds)
        out['log_z'][i] = r['log_z']
        for k in ('token_occ', 'onset'):
            out[k][i, :Tb, :L] = r[k]
        out['class_occ'][i, :Tb] = r['class_occ']
        out['expected_frames'][i, :L], out['onset_mean'][i, :L] = r['expected_frames'], r['onset_mean']
        if bounds:
            q = r['bound']
            bd['log_z'][i] = q['log_z']
            for k in ('token_occ', 'onset'):
                bd[k][i, :Tb, :L] = q[k]
            bd['class_occ'][i, :Tb] = q['class_occ']
            bd['expected_frames'][i, :L], bd['onset_mean'][i, :L] = q['expected_frames'], q['onset_mean']
    if bounds:
        out['bound'] = bd
    return out


def ratio(got, ref, bound, factor=1.0):
    """max |got - ref| / (factor * bound) over the finite entries of ref; the infinite and NaN entries of ref must be matched
    exactly (else inf); 0 / 0 counts as 0, a nonzero or NaN error against a zero bound as inf."""
    got, ref, bound = (np.asarray(v, np.float64).ravel() for v in (got, ref, bound))
    if ref.size == 0:
        return 0.0
    fin = np.isfinite(ref)
    if not (np.array_equal(np.isnan(got[~fin]), np.isnan(ref[~fin]))
            and np.array_equal(got[~fin][~np.isnan(ref[~fin])], ref[~fin][~np.isnan(ref[~fin])])):
        return np.inf
    err, bd = np.abs(got[fin] - ref[fin]), factor * bound[fin]
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bd > 0, err / bd, np.where(err == 0, 0.0, np.inf))
    return float(np.max(np.where(np.isnan(r), np.inf, r)))


def ratios(got, ref, factor=1.0):
    """{output: ratio} of a result dict (any subset of OUTPUTS) against occupancy_ref(..., bounds=True)."""
    return {k: ratio(got[k], ref[k], ref['bound'][k], factor) for k in OUTPUTS if k in got and got[k] is not None}


# ---- a brute force that shares nothing with the recursion ----------------------------------------------------------------------
def collapse(labels, blank):
    merged = [k for i, k in enumerate(labels) if i == 0 or k != labels[i - 1]]
    return [k for k in merged if k != blank]


def brute_force(x, target, blank):
    """Every one of the C^T frame labellings that collapses to `target`, weighted by exp(sum of its frame scores) (math.fsum
    throughout).  Returns (log_z, token_occ (T, L), onset (T, L), class_occ (T, C)); log_z = -inf and zeros when no labelling
    has weight.  For C^T <= 3^6."""
    x = np.asarray(x, np.float64)
    T, C = x.shape
    assert C ** T <= 3 ** 6
    target = [int(v) for v in target]
    L = len(target)
    if T == 0:
        return (0.0 if L == 0 else NINF), np.zeros((0, L)), np.zeros((0, L)), np.zeros((0, C))
    paths = []
    for path in itertools.product(range(C), repeat=T):
        if collapse(path, blank) != target:
            continue
        sc = [float(x[t, k]) for t, k in enumerate(path)]
        if any(v == NINF for v in sc):
            continue
        tok, j = [], -1                                     # the token each frame emits (-1: blank), and which frames start one
        starts = []
        for t, k in enumerate(path):
            new = k != blank and (t == 0 or path[t - 1] != k)
            j += new
            tok.append(j if k != blank else -1)
            starts.append(new)
        paths.append((math.exp(math.fsum(sc)), path, tok, starts))
    z = math.fsum(p[0] for p in paths)
    tok_occ, onset, cls = np.zeros((T, L)), np.zeros((T, L)), np.zeros((T, C))
    if z == 0:
        return NINF, tok_occ, onset, cls
    for t in range(T):
        for j in range(L):
            tok_occ[t, j] = math.fsum(p[0] for p in paths if p[2][t] == j) / z
            onset[t, j] = math.fsum(p[0] for p in paths if p[2][t] == j and p[3][t]) / z
        for c in range(C):
            cls[t, c] = math.fsum(p[0] for p in paths if p[1][t] == c) / z
    return math.log(z), tok_occ, onset, cls
