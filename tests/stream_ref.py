"""Plain float64 restatements of the four streaming kernels of csrc/xps_stream.hip (xps_gemv_f32,
xps_gru_cell_gemv_f32, xps_window_shift_f32, xps_ctc_collapse_f32) and the float32 error bounds the kernel tests hold them
to.  Host only (numpy), no import of the package under test.

Error model, u = 2^-24 (float32 unit roundoff), gamma(n) = n u / (1 - n u):

* A dot product of length K summed as dot_rows sums it.  Scalar branch (K % 4 != 0): every product is rounded once, passes
  through at most ceil(K / 64) additions in its lane and 6 additions of the shuffle tree.  Vector branch: one rounding, 3
  additions inside the float4 group, ceil(K / 256) lane additions, 6 shuffle additions.  Either way a product meets at most
  ceil(K / 64) + 10 roundings (FMA contraction only removes some), so
      |fl(dot) - dot| <= D(K) = gamma(ceil(K / 64) + 10) * sum_k |w_k| |x_k|.
* GEMV output: the dot, then `+ bias`: D(K) + 2 u (|dot| + |bias|).
* GRU cell output, first order in the errors of the six dots (see cell_bound).  A = 4 float32 ulps of the activation's value
  (at most 8 u): expf and tanhf of the HIP device library are documented to at most 2 ulp, plus the addition and the
  correctly rounded division of 1 / (1 + e).
"""
import numpy as np

U = 2.0 ** -24
ACT_ULPS = 4.0


def gamma(n):
    return n * U / (1.0 - n * U)


def dot_bound(K, sabs):
    """D(K): bound on the float32 error of a length-K dot product whose sum of |w_k||x_k| is `sabs`."""
    return gamma(-(-int(K) // 64) + 10) * np.asarray(sabs, dtype=np.float64)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def gemv_ref(x, W, bias=None):
    """float64 x @ W.T + bias: x (B, K), W (N, K), bias (N,) or None -> (B, N)."""
    out = _f64(x) @ _f64(W).T
    return out if bias is None else out + _f64(bias)


def gemv_bound(x, W, bias=None):
    """Elementwise bound on |xps_gemv_f32 - gemv_ref|, (B, N)."""
    x, W = _f64(x), _f64(W)
    dot = x @ W.T
    b = 0.0 if bias is None else np.abs(_f64(bias))
    return dot_bound(x.shape[1], np.abs(x) @ np.abs(W).T) + 2 * U * (np.abs(dot) + b)


def _sigmoid(a):
    e = np.exp(-np.abs(a))
    return np.where(a >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def gru_cell_ref(x, w_ih, w_hh, b_ih, b_hh, h_prev):
    """One GRU step in float64, torch gate order (r, z, n): x (B, K), w_ih (3H, K), w_hh (3H, H), b_* (3H,), h_prev (B, H).
    Returns (h_new (B, H), parts): parts['gi'] / parts['gh'] are the pre-activation dot products (3, B, H),
    parts['gi_abs'] / parts['gh_abs'] their sums of |w||x|, parts['r'], ['z'], ['n'] the gate values."""
    x, w_ih, w_hh, b_ih, b_hh, h = (_f64(a) for a in (x, w_ih, w_hh, b_ih, b_hh, h_prev))
    B, H = h.shape
    gi = (x @ w_ih.T).reshape(B, 3, H).transpose(1, 0, 2)
    gh = (h @ w_hh.T).reshape(B, 3, H).transpose(1, 0, 2)
    gi_abs = (np.abs(x) @ np.abs(w_ih).T).reshape(B, 3, H).transpose(1, 0, 2)
    gh_abs = (np.abs(h) @ np.abs(w_hh).T).reshape(B, 3, H).transpose(1, 0, 2)
    bi, bh = b_ih.reshape(3, 1, H), b_hh.reshape(3, 1, H)
    r = _sigmoid(gi[0] + bi[0] + gh[0] + bh[0])
    z = _sigmoid(gi[1] + bi[1] + gh[1] + bh[1])
    n = np.tanh(gi[2] + bi[2] + r * (gh[2] + bh[2]))
    h_new = n + z * (h - n)
    parts = dict(gi=gi, gh=gh, gi_abs=gi_abs, gh_abs=gh_abs, r=r, z=z, n=n, bi=np.broadcast_to(bi, gi.shape),
                 bh=np.broadcast_to(bh, gh.shape), h=h, K=x.shape[1], H=H)
    return h_new, parts


def _act_err(v):
    """A: ACT_ULPS float32 ulps of the activation value v (|v| <= 1, so at most 8 u)."""
    return ACT_ULPS * np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def cell_bound(parts):
    """Elementwise bound on |xps_gru_cell_gemv_f32 - gru_cell_ref|, (B, H), from gru_cell_ref's parts:
        da_g <= D_i,g + D_h,g + 3 u sum|terms|                       (g = r, z: four terms, three additions)
        dr   <= da_r / 4 + A,   dz <= da_z / 4 + A                   (|sigmoid'| <= 1/4)
        dn   <= D_i,n + |r| D_h,n + |gh_n + b_hn| dr + 3 u (|gi_n| + |b_in| + |r| (|gh_n| + |b_hn|)) + A   (|tanh'| <= 1)
        dh   <= (1 - z) dn + |h - n| dz + 4 u                        (h' = n + z (h - n), all magnitudes <= 2)"""
    gi, gh, bi, bh = parts['gi'], parts['gh'], parts['bi'], parts['bh']
    Di, Dh = dot_bound(parts['K'], parts['gi_abs']), dot_bound(parts['H'], parts['gh_abs'])
    r, z, n, h = parts['r'], parts['z'], parts['n'], parts['h']
    da = [Di[g] + Dh[g] + 3 * U * (np.abs(gi[g]) + np.abs(bi[g]) + np.abs(gh[g]) + np.abs(bh[g])) for g in (0, 1)]
    dr = da[0] / 4 + _act_err(r)
    dz = da[1] / 4 + _act_err(z)
    dn = (Di[2] + np.abs(r) * Dh[2] + np.abs(gh[2] + bh[2]) * dr
          + 3 * U * (np.abs(gi[2]) + np.abs(bi[2]) + np.abs(r) * (np.abs(gh[2]) + np.abs(bh[2]))) + _act_err(n))
    return (1 - z) * dn + np.abs(h - n) * dz + 4 * U


def window_shift_ref(power, k, W, c, src):
    """dst[s] = src[s] shifted left by k frames, then the k new frames float32(longdouble(power[s]) @ W[s] + c[s]);
    W None: the identity map, float32(power[s]).  power (B, k, C) float64, W (B, C, d) or None, c (B, d) or None,
    src (B, win * d) float32.  Returns (dst (B, win * d) float32, tol (B, k, d) float64) with
    tol = max(1 float32 ulp of the new frame, C 2^-52 sum|p||w|), zero for the identity map."""
    power, src = _f64(power), np.asarray(src, dtype=np.float32)
    B, kk, C = power.shape
    assert kk == k
    if W is None:
        new = power.astype(np.float32)
        tol = np.zeros(new.shape)
    else:
        W = _f64(W)
        acc = np.einsum('skc,scd->skd', power.astype(np.longdouble), W.astype(np.longdouble))
        if c is not None:
            acc = acc + _f64(c).astype(np.longdouble)[:, None, :]
        new = acc.astype(np.float32)
        sabs = np.einsum('skc,scd->skd', np.abs(power), np.abs(W))
        tol = np.maximum(np.spacing(np.abs(new)).astype(np.float64), C * 2.0 ** -52 * sabs)
    d = new.shape[2]
    dst = np.concatenate([src[:, k * d:], new.reshape(B, k * d)], axis=1)
    assert dst.shape == src.shape
    return dst, tol


def collapse_ref(logits_seq, blank, max_tokens, fill=0):
    """Online greedy CTC collapse of xps_ctc_collapse_f32, step by step in plain Python.  logits_seq (T, B, n_classes);
    token rows start filled with `fill`, state rows as {-1, 0, 0}.  Returns a list of T snapshots
    (argmax (B,) int64, state (B, 3) int32 = {previous argmax, token count, overflow flag}, tokens (B, max_tokens) int64)."""
    logits_seq = np.asarray(logits_seq)
    T, B, n_classes = logits_seq.shape
    state = [[-1, 0, 0] for _ in range(B)]
    tokens = [[fill] * max_tokens for _ in range(B)]
    out = []
    for t in range(T):
        arg = []
        for s in range(B):
            row = logits_seq[t, s]
            best, bi = row[0], 0
            for cls in range(1, n_classes):
                if row[cls] > best:             # strict: the first maximum wins a tie
                    best, bi = row[cls], cls
            arg.append(bi)
            prev, st = state[s][0], state[s]
            st[0] = bi
            if bi != prev and bi != blank:
                if st[1] < max_tokens:
                    tokens[s][st[1]] = bi
                    st[1] += 1
                else:
                    st[2] = 1
        out.append((np.array(arg, dtype=np.int64), np.array(state, dtype=np.int32), np.array(tokens, dtype=np.int64)))
    return out


# ---- the test inputs, shared by the host and the kernel tests ---------------------------------------------------------------
def gemv_inputs(rng, N, K, B):
    """The inputs of the GEMV kernel test: W ~ U(-1, 1) / sqrt(K), x ~ N(0, 1), a bias of the outputs' scale."""
    W = (rng.uniform(-1, 1, (N, K)) / np.sqrt(K)).astype(np.float32)
    x = rng.standard_normal((B, K)).astype(np.float32)
    bias = rng.uniform(-0.5, 0.5, N).astype(np.float32)
    return x, W, bias


def cell_inputs(rng, H, K, B, scale=1.0):
    s = scale / np.sqrt(H)
    w_ih = rng.uniform(-s, s, (3 * H, K)).astype(np.float32)
    w_hh = rng.uniform(-s, s, (3 * H, H)).astype(np.float32)
    b_ih = rng.uniform(-s, s, 3 * H).astype(np.float32)
    b_hh = rng.uniform(-s, s, 3 * H).astype(np.float32)
    x = rng.standard_normal((B, K)).astype(np.float32)
    h = rng.uniform(-1, 1, (B, H)).astype(np.float32)
    return x, w_ih, w_hh, b_ih, b_hh, h
