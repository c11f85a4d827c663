"""Plain float64 restatement of the one-launch autoregressive decoder (include/xps.h: xps_decoder_fwd_f32 /
xps_decoder_bwd_f32) and of the contract the Python decode paths share (nn_models/functional.py DecoderFn, DecoderWideFn).
Host only (numpy), no import of the package under test; built on gru_seq_ref.

Per decode step s = 0 .. L - 1, one GRU layer of H units, C classes, a table of ntok rows (E W_ih^T + b_ih):

    tok_s     = clamp(token chosen after step s - 1, 0, ntok - 1)          tok_0 = clamp(start_token)
    h_{s+1}   = GRU cell(gi = table[tok_s], h_s)                           (gru_seq_ref.step_ref)
    logits_s  = h_{s+1} W_fc^T + b_fc
    next      = teacher[:, s] if a teacher exists and flags[s] else the FIRST maximum of logits_s      (s + 1 < L)

Layouts (xps.h): table (ntok, 3H), teacher (B, L), flags (L,), logits (B, L, C), tokens (L, B) = the clamped input token of
every step, hs (L + 1, B, H), saved (L, B, 4H) = r, z, n, q = W_hn h + b_hn; backward dlogits (B, L, C) -> dgi (L, B, 3H),
dghn (L, B, H), dh0 (B, H).

The cell's error model is gru_seq_ref's (activation 'hw': the decoder kernels use the same rcp(1 + exp) sigmoid and
2 s(2x) - 1 tanh as the resident recurrence kernels).  The decoder's own arithmetic is the output Linear: logits_bound.
"""
from typing import NamedTuple

import numpy as np

import gru_seq_ref as R

U = R.U


class Inputs(NamedTuple):
    table: np.ndarray
    w_hh: np.ndarray
    b_hh: np.ndarray
    h0: np.ndarray
    w_fc: np.ndarray
    b_fc: np.ndarray


def planted_rows(ntok):
    """The table rows decoder_inputs('saturating') plants in: every second one and the last (the models' start token)."""
    return sorted(set(range(0, ntok, 2)) | {ntok - 1})


def decoder_inputs(rng, B, H, C, L, ntok, regime):
    """Float32 Inputs at the scales of gru_seq_ref.seq_inputs: table ~ N(0, 1 / 3), w_hh ~ U(-1, 1) / sqrt(H), b_hh ~
    U(-0.1, 0.1), h0 ~ U(-1, 1), w_fc ~ U(-1, 1) / sqrt(H), b_fc ~ U(-0.1, 0.1).  'saturating': table and w_hh 8 times wider
    and, in each of planted_rows(ntok), +-100 in every gate, both signs twice (where the hardware exponential overflows)."""
    assert regime in ('normal', 'saturating') and L >= 1
    k = 8.0 if regime == 'saturating' else 1.0
    table = (rng.standard_normal((ntok, 3 * H)) * (k / np.sqrt(3.0))).astype(np.float32)
    w_hh = (rng.uniform(-1, 1, (3 * H, H)) * (k / np.sqrt(H))).astype(np.float32)
    b_hh = rng.uniform(-0.1, 0.1, 3 * H).astype(np.float32)
    h0 = rng.uniform(-1, 1, (B, H)).astype(np.float32)
    w_fc = (rng.uniform(-1, 1, (C, H)) / np.sqrt(H)).astype(np.float32)
    b_fc = rng.uniform(-0.1, 0.1, C).astype(np.float32)
    if regime == 'saturating':
        for row in planted_rows(ntok):
            units = rng.permutation(H)[:12]
            for i in range(12):
                table[row, (i % 3) * H + int(units[i])] = R.PLANTED if (i // 3) % 2 == 0 else -R.PLANTED
    return Inputs(table, w_hh, b_hh, h0, w_fc, b_fc)


def step(table, tok, w_hh, b_hh, h_prev):
    """One decode step's cell in float64: (h_new (B, H), parts) = step_ref with gi = table[tok]; tok (B,) in range."""
    return R.step_ref(np.asarray(table)[np.asarray(tok)], w_hh, b_hh, h_prev)


def logits_ref(h, w_fc, b_fc):
    """(B, C) float64."""
    return np.asarray(h, np.float64) @ np.asarray(w_fc, np.float64).T + np.asarray(b_fc, np.float64)


def logits_bound(h, w_fc, b_fc):
    """Elementwise bound (B, C) on |kernel's logits - logits_ref| for the same float32 h.  Derived, not measured: the kernel
    forms a = b_c, then a = fmaf(h_k, w_ck, a) for k = 0 .. H - 1 in float32, H roundings, one per fused multiply-add.  The
    standard running-error result for a recursive sum of n + 1 terms (Higham, Accuracy and Stability of Numerical
    Algorithms, section 3.1, with the products exact inside the fma) is
        |fl(a) - a| <= gamma_n (|b_c| + sum_k |h_k| |w_ck|),   gamma_n = n u / (1 - n u),   u = 2^-24;
    gamma_(H+1) is taken, which also covers a chain that rounds the bias in once more.  A kernel that exceeds it is a finding."""
    h, w_fc, b_fc = (np.abs(np.asarray(a, np.float64)) for a in (h, w_fc, b_fc))
    n = h.shape[1] + 1
    return (n * U / (1 - n * U)) * (h @ w_fc.T + b_fc)


def next_tokens(logits32, teacher_col, flag, ntok):
    """The token rule of xps.h on one step's logits (B, C): the teacher's token if `flag` is set and a teacher exists
    (teacher_col (B,) is not None), else the FIRST maximum (torch.argmax); then clamped to 0 .. ntok - 1, as the kernel clamps
    when it reads the token -- the `tokens` output holds the clamped value."""
    logits32 = np.asarray(logits32)
    if teacher_col is not None and flag:
        t = np.asarray(teacher_col, np.int64)
    else:
        t = np.argmax(logits32, axis=1).astype(np.int64)          # numpy's argmax returns the first maximum
    return np.clip(t, 0, ntok - 1)


def replay(inputs, tokens, dlogits, dtype=np.float64):
    """Forward and BPTT for GIVEN tokens (L, B), all in range: gru_seq_ref.forward_ref / backward_ref with T = L, ndir = 1,
    gi[s] = table[tokens[s]], dy[s] = dlogits[:, s, :] W_fc.  Returns a dict: hs (L + 1, B, H), saved (L, B, 4H) = r, z, n, q,
    logits (B, L, C), dgi (L, B, 3H), dghn (L, B, H), dh0 (B, H) and the parameter gradients dtable (ntok, 3H: row k sums dgi
    over every (step, trial) that fed token k), dw_hh, db_hh, dw_fc, db_fc.  dtype=np.float32 is the plain float32 restatement
    the backward tolerance is measured with."""
    table, w_hh, b_hh, h0, w_fc, b_fc = (np.asarray(a, dtype) for a in inputs)
    tokens = np.asarray(tokens, np.int64)
    L, B = tokens.shape
    H = h0.shape[1]
    ntok = table.shape[0]
    assert tokens.min() >= 0 and tokens.max() < ntok
    dlogits = np.asarray(dlogits, dtype)
    gi = table[tokens]                                                       # (L, B, 3H)
    y, gates = R.forward_ref(gi[None], [w_hh], [b_hh], h0[None], L, B, H, 1, dtype=dtype)
    hs = y[:L + 1]
    saved = np.concatenate([gates[k][0] for k in 'rznq'], axis=-1)
    logits = np.stack([hs[s + 1] @ w_fc.T + b_fc for s in range(L)], axis=1)
    dy = np.stack([dlogits[:, s, :] @ w_fc for s in range(L)])
    dgi, dghn, dh0 = R.backward_ref(dy, None, y, gates, [w_hh], L, B, H, 1, dtype=dtype)
    dgi, dghn, dh0 = dgi[0], dghn[0], dh0[0]
    dtable = np.zeros((ntok, 3 * H), dtype)
    np.add.at(dtable, tokens.reshape(-1), dgi.reshape(L * B, 3 * H))
    dgh = np.concatenate([dgi[..., :2 * H], dghn], axis=-1).reshape(L * B, 3 * H)
    dw_hh = dgh.T @ hs[:L].reshape(L * B, H)
    db_hh = dgh.sum(0)
    dl = dlogits.transpose(1, 0, 2).reshape(L * B, -1)                       # rows (s, b)
    dw_fc = dl.T @ hs[1:].reshape(L * B, H)
    db_fc = dl.sum(0)
    out = dict(hs=hs, saved=saved, logits=logits, dgi=dgi, dghn=dghn, dh0=dh0, dtable=dtable, dw_hh=dw_hh, db_hh=db_hh,
               dw_fc=dw_fc, db_fc=db_fc)
    assert all(v.dtype == dtype for v in out.values())
    return out


def free_run(inputs, teacher, flags, start_token, L=None):
    """The float64 decode that chooses its own tokens.  teacher (B, L) or None, flags (L,) or None; L is read from the teacher
    when there is one.  Returns tokens (L, B), logits (B, L, C) and margins (L - 1, B): the gap between the two largest logits
    of every (step, trial) at which the next token was chosen by argmax, +inf where the teacher chose it (or C = 1)."""
    L = int(np.asarray(teacher).shape[1] if teacher is not None else L)
    table, w_hh, b_hh, h0, w_fc, b_fc = inputs
    B = h0.shape[0]
    ntok = table.shape[0]
    use_teacher = teacher is not None and flags is not None
    tokens = np.zeros((L, B), np.int64)
    logits = np.zeros((B, L, w_fc.shape[0]))
    margins = np.full((max(L - 1, 0), B), np.inf)
    tok = np.clip(np.full(B, start_token, np.int64), 0, ntok - 1)
    h = np.asarray(h0, np.float64)
    for s in range(L):
        tokens[s] = tok
        h, _ = step(table, tok, w_hh, b_hh, h)
        lg = logits_ref(h, w_fc, b_fc)
        logits[:, s] = lg
        if s + 1 < L:
            flag = bool(flags[s]) if use_teacher else False
            tok = next_tokens(lg, np.asarray(teacher)[:, s] if use_teacher else None, flag, ntok)
            if not flag and lg.shape[1] > 1:
                top = np.sort(lg, axis=1)
                margins[s] = top[:, -1] - top[:, -2]
    return tokens, logits, margins


# ---- the free-run cases, shared by the host and the kernel tests ------------------------------------------------------------
MARGIN = 1e-3            # ten times the project's 1e-4 bar on logits
MAX_EXCLUDED = 1 / 8     # share of the trials a free-run case may leave out because a reference margin is below MARGIN
# (H, B, C, L) -> seed; ntok = C + 1, start token C, no teacher.  Seeds chosen on the reference alone: the float64 decode
# keeps every margin at or above MARGIN (tests/test_decoder_ref_host.py asserts the cap and prints the share).
FREE_RUN_SEEDS = {(64, 37, 9, 8): 3, (64, 17, 16, 8): 11, (64, 33, 15, 3): 0,
                  (128, 37, 9, 8): 4, (128, 17, 16, 8): 1, (128, 33, 15, 3): 0}


def free_run_inputs(H, B, C, L):
    rng = np.random.default_rng([FREE_RUN_SEEDS[(H, B, C, L)], H, B, C, L])
    return decoder_inputs(rng, B, H, C, L, C + 1, 'normal')
