"""Plain numpy restatement of CTC forced alignment (xps_ctc_align, include/xps.h), written from the header's contract, and
a brute force over all frame labellings that shares nothing with the recursion.  Host only: numpy and itertools, no torch
and no import of the package under test.

Contract.  Extended label l' = (blank, l_1, blank, ..., l_L, blank), S = 2 L + 1 states, x_t(c) the score widened to
float64; float64 additions and comparisons only, so a correct implementation gives the same bits:
    v_0(0) = x_0(blank), v_0(1) = x_0(l_1), every other state -inf
    v_t(s) = x_t(l'_s) + max(v_{t-1}(s), v_{t-1}(s-1), [s odd, s >= 3 and l'_s != l'_{s-2}] v_{t-1}(s-2))
Tie rule: the first of (stay, s-1, s-2) that attains the maximum wins (a move needs a strictly larger value); the path ends
in S-1 unless v(S-2) is strictly larger.  A score of -inf is infeasible: states and spans -1.  Tb = 0: score 0 for L = 0,
else -inf.  Lengths are clamped to 0..T and 0..Lmax."""
import itertools

import numpy as np

NINF = -np.inf


def align_one(x, target, blank):
    """x (Tb, C) scores, target (L,) labels -> (states (Tb,) int32, start (L,) int32, end (L,) int32, score float64)."""
    x = np.asarray(x).astype(np.float64)
    Tb = x.shape[0]
    target = [int(v) for v in target]
    L = len(target)
    S = 2 * L + 1
    none = (np.full(Tb, -1, np.int32), np.full(L, -1, np.int32), np.full(L, -1, np.int32))
    if Tb == 0:
        return none + (np.float64(0.0) if L == 0 else np.float64(NINF),)
    lab = [blank] * S
    lab[1::2] = target
    rows = x.tolist()                        # Python floats: the same IEEE doubles, without numpy's per-element cost
    v = [NINF] * S
    v[0] = rows[0][lab[0]]
    if S > 1:
        v[1] = rows[0][lab[1]]
    back = [[0] * S]
    for t in range(1, Tb):
        xt, new, bk = rows[t], [0.0] * S, [0] * S
        for s in range(S):
            best, k = v[s], 0
            if s >= 1 and v[s - 1] > best:
                best, k = v[s - 1], 1
            if s % 2 == 1 and s >= 3 and lab[s] != lab[s - 2] and v[s - 2] > best:
                best, k = v[s - 2], 2
            new[s] = xt[lab[s]] + best
            bk[s] = k
        v = new
        back.append(bk)
    s = S - 1
    if S >= 2 and v[S - 2] > v[S - 1]:
        s = S - 2
    score = np.float64(v[s])
    if score == NINF:
        return none + (score,)
    states = np.empty(Tb, np.int32)
    for t in range(Tb - 1, -1, -1):
        states[t] = s
        s -= back[t][s]
    start, end = np.full(L, -1, np.int32), np.full(L, -1, np.int32)
    for j in range(L):
        frames = np.flatnonzero(states == 2 * j + 1)
        start[j], end[j] = frames[0], frames[-1] + 1
    return states, start, end, score


def align_ref(scores, targets, in_len, tg_len, blank):
    """scores (B, T, C), targets (B, Lmax) ints, in_len / tg_len (B,) ints or None ->
    (states (B, T) int32, token_start (B, Lmax) int32, token_end (B, Lmax) int32, score (B,) float64)."""
    scores = np.asarray(scores)
    B, T, _ = scores.shape
    targets = np.asarray(targets, np.int64).reshape(B, -1)
    Lmax = targets.shape[1]
    in_len = np.full(B, T) if in_len is None else np.clip(np.asarray(in_len, np.int64), 0, T)
    tg_len = np.full(B, Lmax) if tg_len is None else np.clip(np.asarray(tg_len, np.int64), 0, Lmax)
    states = np.full((B, T), -1, np.int32)
    start, end = np.full((B, Lmax), -1, np.int32), np.full((B, Lmax), -1, np.int32)
    score = np.zeros(B, np.float64)
    for b in range(B):
        Tb, L = int(in_len[b]), int(tg_len[b])
        st, s0, s1, sc = align_one(scores[b, :Tb], targets[b, :L], blank)
        states[b, :Tb], start[b, :L], end[b, :L], score[b] = st, s0, s1, sc
    return states, start, end, score


def collapse(labels, blank):
    """Merge repeats, then drop blanks."""
    merged = [k for i, k in enumerate(labels) if i == 0 or k != labels[i - 1]]
    return [k for k in merged if k != blank]


def brute_force(x, target, blank):
    """Every one of the C^T frame labellings that collapses to `target`, scored by summing its frame scores in frame order
    (the recursion's own order of additions, so equal paths give equal bits).  Returns (best score or -inf, the list of
    maximising labellings as tuples).  For C^T <= 3^6."""
    x = np.asarray(x, np.float64)
    T, C = x.shape
    assert C ** T <= 3 ** 6
    target = [int(v) for v in target]
    best, arg = NINF, []
    for path in itertools.product(range(C), repeat=T):
        if collapse(path, blank) != target:
            continue
        if T == 0:
            return 0.0, [()]
        total = x[0, path[0]]
        for t in range(1, T):
            total = x[t, path[t]] + total
        if total > best:
            best, arg = total, [path]
        elif total == best and total != NINF:
            arg.append(path)
    return best, arg


def frame_labels(states, target, blank):
    """Labels emitted along a state path (blank on even states); -1 stays -1."""
    return [(-1 if s < 0 else (blank if s % 2 == 0 else int(target[s // 2]))) for s in states]
