"""Plain numpy restatement of the fused CTC loss kernel (csrc/xps_ctc.hip, xps_ctc_loss_f32), the float32 error bounds its
tests hold it to, a brute-force likelihood that shares nothing with the recursion, and the inputs of the test grid.  Host
only (numpy, math), no torch and no import of the package under test.

Operation (torch nn.CTCLoss(blank, 'mean', zero_infinity) on log_softmax(logits, 2), logits TIME-major (T, B, C)):
extended label l' = (blank, l_1, blank, ..., l_L, blank), S = 2 L + 1 states, lp_t(c) = logit_t(c) - lse_t,
    alpha_0(s) = lp_0(l'_s) for s < 2, else -inf
    alpha_t(s) = lp_t(l'_s) + logsumexp(alpha_{t-1}(s), alpha_{t-1}(s-1), [l'_s != blank and l'_s != l'_{s-2}] alpha_{t-1}(s-2))
    nll        = -logsumexp(alpha_{Tb-1}(S-1), alpha_{Tb-1}(S-2))
    beta the mirror image from t = Tb - 1 downwards,
    d nll / d logit_t(c) = exp(lp_t(c)) - exp(logsumexp_{s: l'_s = c}(alpha_t(s) + beta_t(s)) + nll - lp_t(c)),
    loss = mean_b(nll_b / max(L_b, 1)), dlogits = d loss / d logits, rows t >= Tb zero.
Contract of the lengths (include/xps.h): Tb = clamp(input_length, 0, T), L = clamp(target_length, 0, max_target_len), the
clamped L also in the loss's divisor.  Tb == 0: nll = 0 for L == 0 (the empty alignment), +inf otherwise, gradient zero.
An infinite nll: with zero_infinity nll = 0 and a zero gradient; without, nll = loss = +inf and the sample's gradient rows
t < Tb are unspecified (NaN here, as in torch).

dtype=np.float32 runs the same recursion in the kernel's operation order with every operation rounded to float32: the row
lse as a sequential sum of exp(logit - max) over the classes, lp = logit - lse, the three-term logsumexp with the maximum
taken first, `+ (p - l)`; the class-wise logsumexp of the gradient as a maximum, then a sequential sum over the states.

Error model of nll_bound / grad_bound.  u = 2^-24.  expf and logf of the device library: at most FN_ULPS = 2 ulps, i.e. a
relative error of at most 2 FN_ULPS u = 4 u.  First order in u, except where an accumulated error passes through exp.

* Row lse, lse_t = log(sum_c exp(d_c)) + mx, d_c = p_c - mx <= 0, the sum >= 1 (the maximum contributes exp(0)):
  d_c is rounded (u |d_c|, which moves exp(d_c) by the relative u |d_c|), expf 4 u, C - 1 additions, so the sum has the
  relative error (4 + C - 1) u + u sum_c |d_c| e^{d_c} / sum; log of it has the same absolute error; logf adds
  4 u |log sum|, the addition of mx u |lse_t|:
      D_t = (C + 3) u + u sum_c |d_c| e^{d_c} / sum + 4 u |log sum| + u |lse_t|.
* lp_t(c) = p_c - lse_t: dlp_t(c) = D_t + u |lp_t(c)|.
* One step of alpha.  logsumexp is a convex combination of its inputs' perturbations, so inherited errors enter as the
  MAXIMUM over the finite inputs.  The three-term logsumexp itself: e_i = exp(a_i - m), one of them exp(0), 1 <= sum <= 3;
  subtraction roundings u sum |d_i| e^{d_i} <= (2 / e) u, expf 4 u, two additions 2 u, logf 4 u log 3 = 4.4 u: less than
  LSE3_C u = 12 u in all.  Then `+ m` rounds by u |lse3| (lse3 = alpha_t(s) - lp), and `+ (p - l)` by u |alpha_t(s)|, with
  p - l carrying dlp:
      E_t(s) = max_{finite inputs i} E_{t-1}(i) + 12 u + u |alpha_t(s) - lp_t(l'_s)| + u |alpha_t(s)| + dlp_t(l'_s),
      E_0(s) = dlp_0(l'_s).
  A state that is -inf in exact arithmetic is -inf in float32 too (structure, not value) and carries no error.  The sum
  over Tb steps of u |alpha| is the T u |nll| drift of float32 log space.
* nll: the two-term logsumexp of the last row: dnll = max(E(S-1), E(S-2)) + 12 u + u |nll|.  beta: E^b like E.
* Gradient g = (y - o) gscale, y = exp(lp), o = exp(x), x = (res + nll) - lp, res = logsumexp over the n states of class c
  of alpha + beta:
      dres = max_{finite s of c}(E_t(s) + E^b_t(s) + u |alpha + beta|) + (4 + (n - 1)(1 + 1/e)) u + 4 u log n + u |res|
      dx   = dres + dnll + dlp + u |res + nll| + u |x|
      dg   = gscale (y (expm1(dlp) + 4 u) + o (expm1(dx) + 4 u) + 4 u (y + o))
  (expf 4 u each; the subtraction, the multiplication and the two roundings of gscale = 1 / (B max(L, 1)): 4 u (y + o).)
  Underflow: a float32 value below 2^-126 has no relative precision left (or is flushed to zero), so y, o and the
  product may each be off by 2^-126 in absolute terms: + 3 * 2^-126.  (In the logsumexps an underflowing term sits next
  to exp(0) = 1 and is below u.)  Rows t >= Tb and the samples zeroed by zero_infinity are exact: bound 0.
* loss: the device sums nll_b / max(L_b, 1) in float64 and rounds once: mean_b(dnll_b / max(L_b, 1)) + u |loss|.
No constant here comes from a measurement of the kernel.
"""
import itertools
import math

import numpy as np

U = 2.0 ** -24
FN_ULPS = 2.0
FN = 2.0 * FN_ULPS          # relative error of expf / logf in units of u
LSE3_C = 12.0
TINY = 2.0 ** -126          # below it float32 loses relative precision, or is flushed to zero
F32 = np.float32

MUTANTS = ('skip_across_repeat', 'no_skip', 'last_state_only', 'no_length_scale', 'length_unclamped_below', 'blank_zero',
           'rows_not_zeroed', 'beta_from_T')


def _lse3(a1, a2, a3):
    m = np.maximum(a1, np.maximum(a2, a3))
    m = np.where(np.isneginf(m), m.dtype.type(0), m)
    return np.log(np.exp(a1 - m) + np.exp(a2 - m) + np.exp(a3 - m)) + m


def _lse2(a1, a2):
    m = max(a1, a2)
    if m == -np.inf:
        m = type(a1)(0)
    return np.log(np.exp(a1 - m) + np.exp(a2 - m)) + m


def _shift(a, k, fill):
    """a[s - k] at position s (k > 0) or a[s + |k|] (k < 0), `fill` where that runs off the row."""
    out = np.full_like(a, fill)
    if k > 0:
        out[k:] = a[:-k] if k < len(a) else a[:0]
    else:
        out[:k] = a[-k:] if -k < len(a) else a[:0]
    return out


def _sample(lg, tgt, Tb, blank, B, dt, mutant, bounds):
    """One sample: lg (T, C) of dtype dt, tgt (L,) ints.  Returns nll (dt scalar, +inf when infeasible), the gradient
    (T, C) of nll / (B max(L, 1)) before any zero_infinity handling (None when nll is infinite), and with `bounds` the
    pair (dnll, dg)."""
    T, C = lg.shape
    L = len(tgt)
    S = 2 * L + 1
    ninf = dt(-np.inf)
    eblank = 0 if mutant == 'blank_zero' else blank
    lab = np.full(S, eblank, np.int64)
    lab[1::2] = tgt
    div = L if mutant == 'length_unclamped_below' else max(L, 1)
    with np.errstate(divide='ignore'):
        gscale = dt(1) / dt(B) if mutant == 'no_length_scale' else dt(1) / (dt(B) * dt(div))
    grad = np.zeros((T, C), dt)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        mx = lg.max(1)
        tot = np.zeros(T, dt)
        for c in range(C):
            tot = tot + np.exp(lg[:, c] - mx)
        lse = np.log(tot) + mx
        lp = lg - lse[:, None]
        if mutant == 'rows_not_zeroed':
            grad[Tb:] = np.exp(lp[Tb:]) * gscale
        if Tb == 0:
            nll = dt(0) if L == 0 else dt(np.inf)
            return nll, (grad if np.isfinite(nll) else None), (0.0, np.zeros((T, C))) if bounds else None
        lpl = lp[:, lab]                                    # (T, S)
        notblank = lab != eblank
        skip_f = np.zeros(S, bool)                          # s - 2 -> s allowed
        skip_f[2:] = notblank[2:] & (lab[2:] != lab[:-2])
        if mutant == 'skip_across_repeat':
            skip_f[2:] = notblank[2:]
        if mutant == 'no_skip':
            skip_f[:] = False
        skip_b = np.zeros(S, bool)                          # s -> s + 2 allowed, seen from s
        skip_b[:-2] = skip_f[2:]
        alpha = np.full((Tb, S), ninf, dt)
        alpha[0, :2] = lpl[0, :2]
        for t in range(1, Tb):
            p = alpha[t - 1]
            alpha[t] = _lse3(p, _shift(p, 1, ninf), np.where(skip_f, _shift(p, 2, ninf), ninf)) + lpl[t]
        last = alpha[Tb - 1]
        l1, l2 = last[S - 1], (last[S - 2] if S > 1 else ninf)
        nll = -l1 if mutant == 'last_state_only' else -_lse2(l1, l2)
        if bounds:
            absd = np.abs(lg - mx[:, None])
            D = ((C - 1 + FN) * U + U * (absd * np.exp(-absd)).sum(1) / tot + FN * U * np.abs(np.log(tot))
                 + U * np.abs(lse))
            dlp = D[:, None] + U * np.abs(lp)               # (T, C)
            dlpl = dlp[:, lab]
            step = np.where(np.isfinite(alpha), LSE3_C * U + U * np.abs(alpha - lpl[:Tb]) + U * np.abs(alpha) + dlpl[:Tb],
                            0.0)
            Ea = np.zeros((Tb, S))
            Ea[0, :2] = dlpl[0, :2]
            for t in range(1, Tb):
                e = np.where(np.isfinite(alpha[t - 1]), Ea[t - 1], 0.0)
                inh = np.maximum(e, np.maximum(_shift(e, 1, 0.0), np.where(skip_f, _shift(e, 2, 0.0), 0.0)))
                Ea[t] = np.where(np.isfinite(alpha[t]), inh + step[t], 0.0)
            dnll = max(Ea[Tb - 1, S - 1], Ea[Tb - 1, S - 2] if S > 1 else 0.0) + LSE3_C * U + U * abs(nll)
        if not np.isfinite(nll):
            return nll, None, (0.0, np.zeros((T, C))) if bounds else None
        Tbeta = T if mutant == 'beta_from_T' else Tb
        beta = np.full((Tbeta, S), ninf, dt)
        beta[Tbeta - 1, max(S - 2, 0):] = lpl[Tbeta - 1, max(S - 2, 0):]
        for t in range(Tbeta - 2, -1, -1):
            n = beta[t + 1]
            beta[t] = _lse3(n, _shift(n, -1, ninf), np.where(skip_b, _shift(n, -2, ninf), ninf)) + lpl[t]
        beta = beta[:Tb]
        ab = alpha + beta
        res = np.full((Tb, C), ninf, dt)
        classes = [(c, np.flatnonzero(lab == c)) for c in np.unique(lab)]
        for c, idx in classes:
            m = ab[:, idx].max(1)
            m = np.where(np.isneginf(m), dt(0), m)
            acc = np.zeros(Tb, dt)
            for s in idx:
                acc = acc + np.exp(ab[:, s] - m)
            res[:, c] = np.log(acc) + m
        y = np.exp(lp[:Tb])
        x = (res + nll) - lp[:Tb]
        o = np.exp(x)
        grad[:Tb] = (y - o) * gscale
        if not bounds:
            return nll, grad, None
        stepb = np.where(np.isfinite(beta), LSE3_C * U + U * np.abs(beta - lpl[:Tb]) + U * np.abs(beta) + dlpl[:Tb], 0.0)
        Eb = np.zeros((Tb, S))
        Eb[Tb - 1, max(S - 2, 0):] = dlpl[Tb - 1, max(S - 2, 0):]
        for t in range(Tb - 2, -1, -1):
            e = np.where(np.isfinite(beta[t + 1]), Eb[t + 1], 0.0)
            inh = np.maximum(e, np.maximum(_shift(e, -1, 0.0), np.where(skip_b, _shift(e, -2, 0.0), 0.0)))
            Eb[t] = np.where(np.isfinite(beta[t]), inh + stepb[t], 0.0)
        Eab = np.where(np.isfinite(ab), Ea + Eb + U * np.abs(ab), 0.0)
        dres = np.zeros((Tb, C))
        for c, idx in classes:
            n = len(idx)
            r = np.where(np.isfinite(res[:, c]), np.abs(res[:, c]), 0.0)
            dres[:, c] = Eab[:, idx].max(1) + (FN + (n - 1) * (1 + math.exp(-1))) * U + FN * U * math.log(n) + U * r
        fin = np.isfinite(x)
        dx = dres + dnll + dlp[:Tb] + U * np.where(fin, np.abs(res + nll), 0.0) + U * np.where(fin, np.abs(x), 0.0)
        dg = np.zeros((T, C))
        dg[:Tb] = (float(gscale) * (y * (np.expm1(dlp[:Tb]) + FN * U) + o * (np.expm1(dx) + FN * U) + 4 * U * (y + o))
                   + 3 * TINY)
        return nll, grad, (dnll, dg)


def clamp_lengths(T, Lmax, in_len, tg_len):
    """The kernel's contract: input lengths clamped to 0..T, target lengths to 0..max_target_len."""
    return (np.clip(np.asarray(in_len, np.int64), 0, T), np.clip(np.asarray(tg_len, np.int64), 0, Lmax))


def ctc_ref(logits, targets, in_len, tg_len, blank, zero_infinity, dtype=np.float64, mutant=None, with_parts=False):
    """logits (T, B, C), targets (B, Lmax) ints (Lmax = max_target_len, may be 0; cells past a length are never read),
    in_len / tg_len (B,) ints.  Returns (nll (B,), loss, dlogits (T, B, C)) in `dtype`; with_parts adds a dict for nll_bound /
    grad_bound / loss_bound (float64 only).  mutant: one of MUTANTS, a deliberately wrong variant for the tests' own proof."""
    assert mutant is None or mutant in MUTANTS
    dt = np.dtype(dtype).type
    logits = np.asarray(logits).astype(dt)
    T, B, C = logits.shape
    targets = np.asarray(targets).reshape(B, -1)
    Tbs, Ls = clamp_lengths(T, targets.shape[1], in_len, tg_len)
    bounds = with_parts and dt is np.float64 and mutant is None
    nll = np.zeros(B, dt)
    dl = np.zeros((T, B, C), dt)
    dnll, dg = np.zeros(B), np.zeros((T, B, C))
    for b in range(B):
        Tb, L = int(Tbs[b]), int(Ls[b])
        tgt = np.asarray([int(v) for v in targets[b, :L]], np.int64)
        v, g, bd = _sample(np.ascontiguousarray(logits[:, b]), tgt, Tb, int(blank), B, dt, mutant, bounds)
        if np.isfinite(v):
            nll[b], dl[:, b] = v, g
            if bounds:
                dnll[b], dg[:, b] = bd
        elif zero_infinity:
            nll[b] = 0                                      # and a zero gradient, exactly
        else:
            nll[b] = np.inf
            dl[:Tb, b] = np.nan                             # unspecified
    div = Ls.astype(np.float64) if mutant == 'length_unclamped_below' else np.maximum(Ls, 1).astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        loss = dt(np.mean(nll.astype(np.float64) / div))    # the device reduces in float64 and rounds once
    if not with_parts:
        return nll, loss, dl
    return nll, loss, dl, dict(nll=nll, loss=loss, dnll=dnll, dg=dg, L=Ls, Tb=Tbs)


def nll_bound(parts):
    """(B,) bound on |float32 nll - float64 nll| of a correct float32 implementation (0 where the nll is exact: zeroed or
    infinite samples, Tb == 0)."""
    return parts['dnll']


def grad_bound(parts):
    """(T, B, C) bound on |float32 dlogits - float64 dlogits|."""
    return parts['dg']


def loss_bound(parts):
    fin = np.isfinite(parts['nll'])
    return float(np.mean(np.where(fin, parts['dnll'], 0.0) / np.maximum(parts['L'], 1))
                 + (U * abs(float(parts['loss'])) if np.isfinite(parts['loss']) else 0.0))


def _ratio(err, bound):
    """max err / bound; 0 / 0 counts as 0, a nonzero (or NaN) error against a zero bound as inf."""
    err, bound = np.asarray(err, np.float64).ravel(), np.asarray(bound, np.float64).ravel()
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.max(np.where(np.isnan(r), np.inf, r)))


def error_ratios(got, ref):
    """(nll, loss, gradient) error / bound ratios of a result (nll, loss, dlogits) against ctc_ref(..., with_parts=True)'s
    tuple.  An infinite nll or loss must match exactly (else inf); the gradient rows the reference leaves unspecified (NaN)
    are left out."""
    nll, loss, dl, parts = ref
    g_nll, g_loss, g_dl = (np.asarray(a, np.float64) for a in got)
    fin = np.isfinite(nll)
    r_nll = _ratio(np.abs(g_nll[fin] - nll[fin]), nll_bound(parts)[fin])
    if not np.array_equal(g_nll[~fin], nll[~fin]):
        r_nll = np.inf
    if np.isfinite(loss):
        r_loss = _ratio(abs(g_loss - loss), loss_bound(parts))
    else:
        r_loss = 0.0 if g_loss == loss else np.inf
    spec = ~np.isnan(dl)
    r_dl = _ratio(np.abs(g_dl[spec] - dl[spec]), grad_bound(parts)[spec])
    return r_nll, r_loss, r_dl


def ctc_brute(logits_one_sample, target, blank):
    """-log of the summed probability of every one of the C^T frame labellings that collapses (merge repeats, then drop
    blanks) to `target`; +inf when none does.  Plain Python, math.fsum; for T <= 5 and C <= 3."""
    rows = [[float(v) for v in r] for r in np.asarray(logits_one_sample, np.float64)]
    T, C = len(rows), len(rows[0])
    assert C ** T <= 3 ** 5
    prob = []
    for r in rows:
        m = max(r)
        e = [math.exp(v - m) for v in r]
        z = math.fsum(e)
        prob.append([v / z for v in e])
    target = [int(v) for v in target]
    terms = []
    for path in itertools.product(range(C), repeat=T):
        merged = [k for i, k in enumerate(path) if i == 0 or k != path[i - 1]]
        if [k for k in merged if k != blank] == target:
            terms.append(math.prod(prob[t][k] for t, k in enumerate(path)))
    total = math.fsum(terms)
    return -math.log(total) if total > 0 else math.inf


# ---- the inputs of the test grid (tests/test_gpu_ctc_loss.py on the device, tests/test_ctc_ref_host.py for the emulation) ----
def _targets(rng, B, L, labels, repeats=()):
    """(B, L) targets without adjacent repeats from `labels` (one label: all repeats); sample b in `repeats` gets up to 3."""
    labels = np.asarray(labels)
    out = np.zeros((B, L), np.int64)
    for b in range(B):
        for i in range(L):
            pool = labels[labels != out[b, i - 1]] if i and len(labels) > 1 else labels
            out[b, i] = rng.choice(pool)
        if b in repeats:
            for i in range(1, min(L, 6), 2):
                out[b, i] = out[b, i - 1]
    return out


def _case(name, family, logits, targets, in_len, tg_len, blank=0, zi=(1,)):
    return dict(name=name, family=family, logits=np.ascontiguousarray(logits, F32),
                targets=np.ascontiguousarray(targets, np.int64), in_len=np.asarray(in_len, np.int64),
                tg_len=np.asarray(tg_len, np.int64), blank=blank, zi=zi)


def n_repeats(t):
    return int(sum(t[i] == t[i - 1] for i in range(1, len(t))))


def grid(family=None):
    """The cases of the test grid as dicts (name, family, logits (T, B, C) float32, targets (B, Lmax) int64, in_len, tg_len,
    blank, zi = the zero_infinity values to run); deterministic."""
    out = []
    for L in (0, 1, 31, 32, 63, 64, 100):                                   # S = 1, 3, 63, 65, 127, 129, 201
        T, B, C = L + 8, 3, 7
        rng = np.random.default_rng(100 + L)
        out.append(_case(f'state_L{L}', 'state', rng.standard_normal((T, B, C)) * 2, _targets(rng, B, L, range(1, C), (1,)),
                         [T, T, T - 3], [L, L, max(L - 2, 0)]))
    rng = np.random.default_rng(511)
    tg = _targets(rng, 2, 511, range(1, 5))
    tg[1] = 3                                                               # needs 1021 frames: infeasible
    out.append(_case('envelope_L511', 'envelope', rng.standard_normal((520, 2, 5)) * 2, tg, [520, 520], [511, 511]))
    for T in (1, 2, 63, 64, 65, 130):
        rng = np.random.default_rng(200 + T)
        out.append(_case(f'time_T{T}', 'time', rng.standard_normal((T, 4, 11)) * 2, _targets(rng, 4, 3, range(1, 11), (1,)),
                         np.minimum([63, 64, 65, T], T), [3, 2, 1, 0] if T < 3 else [3, 3, 2, 3]))
    for scale in (2, 20):
        rng = np.random.default_rng(1500 + scale)
        out.append(_case(f'long_scale{scale}', 'long', rng.standard_normal((1500, 2, 41)) * scale,
                         _targets(rng, 2, 3, range(1, 41), (1,)), [1500, 1437], [3, 3]))
    for C in (1, 2, 63, 64, 65, 130):
        T, B, L = 20, 3, (0 if C == 1 else 6)
        rng = np.random.default_rng(300 + C)
        labels = range(max(C // 2, 1) if C < 65 else 64, C)                 # C >= 65: only labels of the second lane pass
        out.append(_case(f'class_C{C}', 'class', rng.standard_normal((T, B, C)) * 2, _targets(rng, B, L, labels, (1,)),
                         [T, T - 1, T - 6], [L, L, max(L - 1, 0)]))
    for blank in (0, 3, 6):
        T, B, C, L = 12, 3, 7, 4
        rng = np.random.default_rng(400 + blank)
        tg = _targets(rng, B, L, [c for c in range(C) if c != blank], (1,))
        if blank:
            tg[0, 0], tg[0, 1], tg[2, 2], tg[2, 3] = 0, 1, 0, 5             # label 0 is an ordinary label
        out.append(_case(f'blank_{blank}', 'blank', rng.standard_normal((T, B, C)) * 2, tg, [T, T, T - 2], [L, L, L],
                         blank=blank))
    for i, edge in enumerate(([1, 1, 2, 2], [1, 2, 3, 1], [2, 2, 2, 2], [4, 4, 1, 4])):
        r = n_repeats(edge)
        for short in (0, 1):                                                # in_len = L + r: one alignment; one fewer: none
            rng = np.random.default_rng(500 + i)
            tg = _targets(rng, 3, 4, range(1, 5), (2,))
            tg[0] = edge
            out.append(_case(f'feasible_{i}_{"short" if short else "exact"}', 'feasible', rng.standard_normal((10, 3, 5)) * 2,
                             tg, [4 + r - short, 10, 9], [4, 4, 3], zi=(1, 0)))
    rng = np.random.default_rng(600)
    T = 9
    out.append(_case('lengths', 'lengths', rng.standard_normal((T, 7, 5)) * 2, _targets(rng, 7, 3, range(1, 5)),
                     [0, 0, -3, T + 5, 9, 4, 9], [0, 2, 1, 3, -1, 0, 7], zi=(1, 0)))
    rng = np.random.default_rng(700)
    out.append(_case('stride', 'stride', rng.standard_normal((14, 3, 7)) * 2, _targets(rng, 3, 6, range(1, 7), (1,)),
                     [14, 12, 9], [6, 4, 0]))
    rng = np.random.default_rng(800)
    T, B, C = 15, 3, 6
    base = np.round(rng.standard_normal((T, B, C)) * 2 * 1024) / 1024      # multiples of 2^-10: base + 1e4 is exact in float32
    tg_low, tg_top = _targets(rng, B, 3, range(1, 5), (1,)), _targets(rng, B, 3, range(1, 5), (1,))
    tg_top[:, 1] = 5
    low = base.copy()
    low[:, :, 5] = -1e4
    ties = np.round(base)
    ties[:, :, 1] = np.delete(ties, 1, axis=2).max(2)                       # class 1 ties the maximum in every row
    out.append(_case('range_base', 'range', base, tg_low, [T, T - 1, T - 4], [3, 3, 2]))
    assert np.array_equal((base + 1e4).astype(F32).astype(np.float64), base + 1e4)
    out.append(_case('range_shift', 'range', base + 1e4, tg_low, [T, T - 1, T - 4], [3, 3, 2]))
    out.append(_case('range_low_nonlabel', 'range', low, tg_low, [T, T - 1, T - 4], [3, 3, 2]))
    out.append(_case('range_low_label', 'range', low, tg_top, [T, T - 1, T - 4], [3, 3, 2]))
    out.append(_case('range_ties', 'range', ties, tg_low, [T, T - 1, T - 4], [3, 3, 2]))
    for B in (1, 256, 257, 300):
        rng = np.random.default_rng(900 + B)
        out.append(_case(f'batch_B{B}', 'batch', rng.standard_normal((12, B, 5)) * 2, _targets(rng, B, 2, range(1, 5)),
                         rng.integers(6, 13, B), rng.integers(0, 3, B)))
    return [c for c in out if family is None or c['family'] == family]
