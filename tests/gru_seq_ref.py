"""Plain float64 restatement of the fused GRU recurrence (include/xps.h: xps_gru_seq_fwd_f32 / xps_gru_seq_bwd_f32), the
float32 error bound the kernel tests hold one step to, and a restatement of the dispatch rule.  Host only (numpy), no import
of the package under test.

Layouts (xps.h): gi [ndir][T][B][3H] (gate order r, z, n), w_hh [ndir] of (3H, H), b_hh [ndir] of (3H,), h0 [ndir][B][H] or
None, y_ext [T + 2][B][ndir * H]: slot t + 1 = h_t in actual time, slot 0 / slot T + 1 = h0 of the forward / reverse
direction (the other direction's half of those two slots is zero), direction 1 runs t = T - 1 .. 0 and reads slot t + 2.

    r = s(gi_r + W_hr h + b_hr)   z = s(gi_z + W_hz h + b_hz)   q = W_hn h + b_hn   n = tanh(gi_n + r q)   h' = n + z (h - n)

Error model of ONE step given the previous state exactly (step_bound), u = 2^-24:

* Dot products.  The matrix kernels' constant the project holds every GEMM to (tests/test_gpu_nn_kernels.py):
  |fl(dot) - dot| <= DOT[mode] * sum_k |w_k| |h_k|, DOT = 4e-7 for fp32 MFMA chains, 40 times that for bf16x3 split products.
* Activations, by route (ACTIVATION).
  'libm' (generic and per-step kernels: expf, a true division, tanhf): stream_ref.ACT_ULPS float32 ulps of the value.
  'hw' (resident and cluster kernels): sigmoid(x) = v_rcp_f32(1 + v_exp_f32(-x * log2e)), tanh(x) = 2 sigmoid(2 x) - 1.
  AMD's instruction set reference guides (CDNA3 / CDNA4 "Instruction Set Architecture", VOP1 opcode table) give V_EXP_F32
  and V_RCP_F32 as "1 ULP accuracy" (denormals flushed), i.e. a relative error of at most 2^-23 = 2 u.  With e = exp(-x),
  s = 1 / (1 + e):
      t = fl(-x * log2e): one rounding and the rounded constant (|log2e_f32 / log2e - 1| < 0.4 u): t = -x log2e (1 + d),
          |d| <= 1.4 u, so 2^t = e (1 + d'), |d'| <= 1.4 u |x|  (|x| < 90, beyond that s is 0 or 1 to far below u)
      v_exp_f32:  relative 2 u.  Together |de| <= e (1.4 u |x| + 2 u); ds = s^2 de = s (1 - s) (1.4 u |x| + 2 u)
          <= 1.4 u * 0.2239 + 2 u / 4 = 0.82 u        (max |x| s (1 - s) = 0.2239 at |x| = 1.5434, max s (1 - s) = 1/4)
      fl(1 + e):  1 + e in [1, 2]: absolute u, relative u; ds <= u s <= u
      v_rcp_f32:  1 ulp of s; s <= 1 so ulp(s) <= u (s = 1 itself only when 1 + e rounded to 1, which the line above covers)
      sum: SIG_ABS = 0.82 u + u + u < 3 u.  e = +inf (x < -88.7) gives rcp(inf) = 0, e = 0 gives 1: no NaN on either rail.
      tanh: 2 x is exact, 2 s is exact, the error of s doubles: 6 u; fl(2 s - 1) is exact for s >= 1/4 (Sterbenz) and
      rounds once to a value below 1 otherwise (u / 2): TANH_ABS = 6.5 u.
  These are ABSOLUTE allowances (the relative accuracy of the hw tanh near 0 is not claimed: 6.5 u there as everywhere).
  They are derived, not measured: a kernel that exceeds them is a finding.
* Everything else is propagated with the TRUE derivatives s' = s (1 - s), tanh' = 1 - n^2 and a second-order term
  (|s''| <= 0.0963, |tanh''| <= 0.7699), so the bound stays tight when the gates saturate:
      da_g <= D_g + 3 u (|gi_g| + |gh_g| + |b_g|)                                   g = r, z
      dg   <= g (1 - g) da_g + 0.0482 da_g^2 + A_sig                                g = r, z
      dq   <= D_n + u (|gh_n| + |b_n|)
      da_n <= |r| dq + |q| dr + dr dq + 3 u (|gi_n| + |r| |q|)
      dn   <= (1 - n^2) da_n + 0.385 da_n^2 + A_tanh
      dh   <= (1 - z) dn + |h - n| dz + dz dn + 4 u
"""
import numpy as np

import stream_ref as S

U = S.U
DOT = {'fp32': 4e-7, 'bf16x3': 40 * 4e-7}
SIG_ABS = 3.0 * U
TANH_ABS = 6.5 * U
SIG2 = 0.5 / (6.0 * np.sqrt(3.0))            # half of max |sigmoid''|
TANH2 = 0.5 * 4.0 / (3.0 * np.sqrt(3.0))     # half of max |tanh''|

# route codes of xps_gru_seq_route (include/xps.h)
REFUSED, CLUSTER, RESIDENT, GENERIC_VEC, GENERIC_SCALAR, STEP, STEP_VECA, STEP_VECB = 0, 1, 2, 3, 4, 8, 1, 2
MAX_H_TILE, MAX_H_STEP = 624, 1264
ACTIVATION = {CLUSTER: 'hw', RESIDENT: 'hw', GENERIC_VEC: 'libm', GENERIC_SCALAR: 'libm', STEP: 'libm'}


def activation_of(route_code):
    return ACTIVATION[STEP if route_code & STEP else route_code]


def route(T, B, H, ndir, aligned=True, cluster_mode=2, step_path=True, cus=256):
    """The dispatch rule of csrc/xps_gru.hip (gru_route) restated: the code xps_gru_seq_route returns, the same for the
    forward and the backward when all weights share one alignment.  cluster_mode 0 | 1 | 2 = off | steps | persistent,
    step_path = XPS_GRU_STEP_PATH, cus = compute units of the device (the cluster plan needs one per member)."""
    if T < 1 or B < 1 or H < 1 or ndir not in (1, 2):
        return REFUSED
    if cluster_mode != 0 and 256 < H <= 512 and H % 4 == 0 and B >= 128:
        members = -(-H // 32)                        # 32 units per member above H = 256
        if cus // (members * ndir) >= 1 and ndir * (T + 2) * B * 4 * H * 4 < 2 ** 32:
            return CLUSTER
    if H > 128 and step_path:
        if H > MAX_H_STEP:
            return REFUSED
        v4 = H % 4 == 0
        return STEP | (STEP_VECA if v4 else 0) | (STEP_VECB if v4 and aligned else 0)
    if H > MAX_H_TILE:
        return REFUSED
    vec = H % 4 == 0 and aligned
    if vec and H in (64, 128):
        return RESIDENT
    return GENERIC_VEC if vec else GENERIC_SCALAR


def _sigmoid(a):
    e = np.exp(-np.abs(a))
    return np.where(a >= 0, 1.0 / (1.0 + e), e / (1.0 + e)).astype(a.dtype)


def step_ref(gi_t, w_hh, b_hh, h_prev):
    """One step of one direction in float64.  gi_t (B, 3H), w_hh (3H, H), b_hh (3H,), h_prev (B, H).
    Returns (h_new (B, H), parts) with parts as step_bound reads them."""
    gi_t, w_hh, b_hh, h = (np.asarray(a, np.float64) for a in (gi_t, w_hh, b_hh, h_prev))
    B, H = h.shape
    gi = gi_t.reshape(B, 3, H).transpose(1, 0, 2)
    gh = (h @ w_hh.T).reshape(B, 3, H).transpose(1, 0, 2)
    gh_abs = (np.abs(h) @ np.abs(w_hh).T).reshape(B, 3, H).transpose(1, 0, 2)
    bh = np.broadcast_to(b_hh.reshape(3, 1, H), gh.shape)
    r = _sigmoid(gi[0] + gh[0] + bh[0])
    z = _sigmoid(gi[1] + gh[1] + bh[1])
    q = gh[2] + bh[2]
    n = np.tanh(gi[2] + r * q)
    return n + z * (h - n), dict(gi=gi, gh=gh, gh_abs=gh_abs, bh=bh, r=r, z=z, n=n, q=q, h=h)


def step_bound(parts, mode, activation):
    """Elementwise bound (B, H) on |kernel's h_t - step_ref| given the same h_{t-1}; mode 'fp32' | 'bf16x3',
    activation 'libm' | 'hw' (module docstring)."""
    return gate_bounds(parts, mode, activation)['h']


def gate_bounds(parts, mode, activation):
    """The intermediate bounds of the module docstring next to the final one: {'r', 'z', 'q', 'n', 'h'} -> (B, H), for
    kernels that store r, z, n and q = W_hn h + b_hn (the `saved` tensors).  ['h'] is step_bound."""
    gi, gh, bh = np.abs(parts['gi']), np.abs(parts['gh']), np.abs(parts['bh'])
    r, z, n, q, h = parts['r'], parts['z'], parts['n'], parts['q'], parts['h']
    D = DOT[mode] * parts['gh_abs']
    if activation == 'libm':
        A_r, A_z, A_n = S._act_err(r), S._act_err(z), S._act_err(n)
    else:
        assert activation == 'hw'
        A_r = A_z = SIG_ABS
        A_n = TANH_ABS
    da = [D[g] + 3 * U * (gi[g] + gh[g] + bh[g]) for g in (0, 1)]
    dr = r * (1 - r) * da[0] + SIG2 * da[0] ** 2 + A_r
    dz = z * (1 - z) * da[1] + SIG2 * da[1] ** 2 + A_z
    dq = D[2] + U * (gh[2] + bh[2])
    dan = r * dq + np.abs(q) * dr + dr * dq + 3 * U * (gi[2] + r * np.abs(q))
    dn = (1 - n * n) * dan + TANH2 * dan ** 2 + A_n
    return dict(r=dr, z=dz, q=dq, n=dn, h=(1 - z) * dn + np.abs(h - n) * dz + dz * dn + 4 * U)


def _slots(t, d):
    """(slot read as h_{t-1}, slot written) of direction d at actual time t."""
    return (t if d == 0 else t + 2), t + 1


def forward_ref(gi, w_hh, b_hh, h0, T, B, H, ndir, dtype=np.float64):
    """(y_ext (T + 2, B, ndir * H), gates): gates['r' | 'z' | 'n' | 'q'] are (ndir, T, B, H).  dtype=np.float32 makes it the
    plain float32 restatement (numpy's matmul, exp and tanh) the backward tolerance is measured with."""
    gi = np.asarray(gi, dtype).reshape(ndir, T, B, 3 * H)
    y = np.zeros((T + 2, B, ndir * H), dtype)
    gates = {k: np.zeros((ndir, T, B, H), dtype) for k in 'rzqn'}
    for d in range(ndir):
        W, b = np.asarray(w_hh[d], dtype), np.asarray(b_hh[d], dtype)
        cols = slice(d * H, (d + 1) * H)
        if h0 is not None:
            y[0 if d == 0 else T + 1, :, cols] = np.asarray(h0, dtype)[d]
        for s in range(T):
            t = s if d == 0 else T - 1 - s
            src, dst = _slots(t, d)
            h = y[src, :, cols]
            gh = h @ W.T + b
            r = _sigmoid(gi[d, t, :, :H] + gh[:, :H])
            z = _sigmoid(gi[d, t, :, H:2 * H] + gh[:, H:2 * H])
            q = gh[:, 2 * H:]
            n = np.tanh(gi[d, t, :, 2 * H:] + r * q)
            y[dst, :, cols] = n + z * (h - n)
            for k, v in zip('rzqn', (r, z, q, n)):
                gates[k][d, t] = v
    assert y.dtype == dtype
    return y, gates


def backward_ref(dy, dhn, y_ext, gates, w_hh, T, B, H, ndir, dtype=np.float64):
    """BPTT through forward_ref's y_ext and gates: (dgi (ndir, T, B, 3H), dghn (ndir, T, B, H), dh0 (ndir, B, H)).
    dy (T, B, ndir * H) or None, dhn (ndir, B, H) or None (xps.h)."""
    dgi = np.zeros((ndir, T, B, 3 * H), dtype)
    dghn = np.zeros((ndir, T, B, H), dtype)
    dh0 = np.zeros((ndir, B, H), dtype)
    y_ext = np.asarray(y_ext, dtype)
    for d in range(ndir):
        W = np.asarray(w_hh[d], dtype)
        cols = slice(d * H, (d + 1) * H)
        run = np.zeros((B, H), dtype) if dhn is None else np.asarray(dhn, dtype)[d].copy()
        for s in range(T - 1, -1, -1):
            t = s if d == 0 else T - 1 - s
            r, z, q, n = (np.asarray(gates[k][d, t], dtype) for k in 'rzqn')
            hp = y_ext[_slots(t, d)[0], :, cols]
            dh = run if dy is None else run + np.asarray(dy, dtype)[t, :, cols]
            dan = dh * (1 - z) * (1 - n * n)
            daz = dh * (hp - n) * z * (1 - z)
            dar = dan * q * r * (1 - r)
            dgi[d, t] = np.concatenate([dar, daz, dan], axis=1)
            dghn[d, t] = dan * r
            run = dh * z + np.concatenate([dar, daz, dan * r], axis=1) @ W
        dh0[d] = run
    assert dgi.dtype == dtype
    return dgi, dghn, dh0


# ---- the test inputs, shared by the host and the kernel tests ---------------------------------------------------------------
PLANTED = 100.0


def seq_inputs(rng, T, B, H, ndir, regime, with_h0):
    """regime 'normal': w_hh ~ U(-1, 1) / sqrt(H) and b_hh ~ U(-0.1, 0.1) (the scale of golden/weights.py weights_from_seed),
    gi ~ N(0, 1 / 3) (x ~ N(0, 1) through such an input projection).  'saturating': gi x 8, w_hh x 8, and a handful of gi
    entries of +-100 in every gate, where the hardware exponential overflows.  Returns float32 gi, [w_hh], [b_hh], h0 | None."""
    assert regime in ('normal', 'saturating')
    k = 8.0 if regime == 'saturating' else 1.0
    gi = (rng.standard_normal((ndir, T, B, 3 * H)) * (k / np.sqrt(3.0))).astype(np.float32)
    w = [(rng.uniform(-1, 1, (3 * H, H)) * (k / np.sqrt(H))).astype(np.float32) for _ in range(ndir)]
    b = [rng.uniform(-0.1, 0.1, 3 * H).astype(np.float32) for _ in range(ndir)]
    h0 = rng.uniform(-1, 1, (ndir, B, H)).astype(np.float32) if with_h0 else None
    if regime == 'saturating':
        for i in range(12):                     # every gate gets both signs twice
            d, t, s, j = (int(rng.integers(n)) for n in (ndir, T, B, H))
            gi[d, t, s, (i % 3) * H + j] = PLANTED if (i // 3) % 2 == 0 else -PLANTED
    return gi, w, b, h0
