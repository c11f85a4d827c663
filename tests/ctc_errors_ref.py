"""Numpy restatement of xps_edit_align's contract (include/xps.h): fill the Levenshtein table D, walk back from (m, n) by the
tie rule that is stated on D alone (diagonal, else insertion, else deletion), and report the distance, the four counts, the
two maps and the confusion matrix.  Nothing here knows how the kernel evaluates the table."""
import numpy as np

HIT, SUB, DEL, INS = 0, 1, 2, 3


def table(a, t):
    """D[i][j] of prediction a against target t, (m + 1, n + 1) int64."""
    m, n = len(a), len(t)
    D = np.zeros((m + 1, n + 1), np.int64)
    D[:, 0] = np.arange(m + 1)
    D[0, :] = np.arange(n + 1)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            D[i, j] = min(D[i - 1, j - 1] + (a[i - 1] != t[j - 1]), D[i - 1, j] + 1, D[i, j - 1] + 1)
    return D


def walk(a, t, D=None):
    """The operations of the contract's walk, in walk order (from the END of the sequences to their start):
    [(op, j, i), ...] with op HIT / SUB (target j, prediction i), DEL (target j, i = -1), INS (j = -1, prediction i)."""
    D = table(a, t) if D is None else D
    i, j = len(a), len(t)
    ops = []
    while i > 0 or j > 0:
        if i > 0 and j > 0:
            ne = int(a[i - 1] != t[j - 1])
            if D[i, j] == D[i - 1, j - 1] + ne:
                ops.append((SUB if ne else HIT, j - 1, i - 1))
                i, j = i - 1, j - 1
            elif D[i, j] == D[i - 1, j] + 1:
                ops.append((INS, -1, i - 1))
                i -= 1
            else:
                assert D[i, j] == D[i, j - 1] + 1
                ops.append((DEL, j - 1, -1))
                j -= 1
        elif i > 0:
            ops.append((INS, -1, i - 1))
            i -= 1
        else:
            ops.append((DEL, j - 1, -1))
            j -= 1
    return ops


def align_pair(a, t):
    """(dist, counts [hits, subs, dels, ins], tgt_to_pred (n,), pred_to_tgt (m,), ops) of one pair."""
    D = table(a, t)
    ops = walk(a, t, D)
    t2p, p2t = np.full(len(t), -9, np.int32), np.full(len(a), -9, np.int32)
    counts = np.zeros(4, np.int64)
    for op, j, i in ops:
        counts[op] += 1
        if j >= 0:
            t2p[j] = i
        if i >= 0:
            p2t[i] = j
    assert (t2p != -9).all() and (p2t != -9).all()
    return int(D[len(a), len(t)]), counts, t2p, p2t, ops


def edit_align_ref(pred, pred_len, tgt, tgt_len, P=None, L=None, n_classes=None):
    """The batch: pred (B, >= P), tgt (B, >= L) int64 with their lengths, clamped to 0..P / 0..L as the kernel clamps them.
    Returns dist (B,), counts (B, 4) int64, tgt_to_pred (B, L), pred_to_tgt (B, P) int32 with -2 past the lengths, and
    confusion (K + 1, K + 1) int64 (None without n_classes; row = target class, row K = insertion, column = predicted class,
    column K = deletion; labels clamped to 0..K-1 for the cell index only)."""
    pred, tgt = np.asarray(pred, np.int64), np.asarray(tgt, np.int64)
    B = pred.shape[0]
    P = pred.shape[1] if P is None else P
    L = tgt.shape[1] if L is None else L
    dist, counts = np.zeros(B, np.int64), np.zeros((B, 4), np.int64)
    t2p, p2t = np.full((B, L), -2, np.int32), np.full((B, P), -2, np.int32)
    K = n_classes
    conf = None if K is None else np.zeros((K + 1, K + 1), np.int64)
    for b in range(B):
        m, n = int(np.clip(pred_len[b], 0, P)), int(np.clip(tgt_len[b], 0, L))
        a, t = pred[b, :m], tgt[b, :n]
        dist[b], counts[b], t2p[b, :n], p2t[b, :m], ops = align_pair(a, t)
        if conf is not None:
            for op, j, i in ops:
                row = K if j < 0 else int(np.clip(t[j], 0, K - 1))
                col = K if i < 0 else int(np.clip(a[i], 0, K - 1))
                conf[row, col] += 1
    return dist, counts, t2p, p2t, conf


def monotone_alignments(m, n):
    """EVERY monotone alignment of m prediction tokens with n target tokens (the Delannoy paths from (0, 0) to (m, n)), for
    the brute force: (gaps (n_paths,) int64, the insertions + deletions of each path; diag (n_paths, m * n) int64, 1 where
    the path aligns prediction i with target j, at i * n + j).  A path's cost is gaps + the unequal pairs on its diagonal."""
    paths = []

    def go(i, j, gaps, cells):
        if i == m and j == n:
            paths.append((gaps, cells))
            return
        if i < m and j < n:
            go(i + 1, j + 1, gaps, cells + [i * n + j])
        if i < m:
            go(i + 1, j, gaps + 1, cells)
        if j < n:
            go(i, j + 1, gaps + 1, cells)
    go(0, 0, 0, [])
    diag = np.zeros((len(paths), m * n), np.int64)
    for p, (_, cells) in enumerate(paths):
        diag[p, cells] = 1
    return np.array([g for g, _ in paths], np.int64), diag
