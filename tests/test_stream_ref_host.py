"""The float64 references and error bounds of tests/stream_ref.py, checked on the host (no GPU): against torch's GRUCell and
itertools.groupby, against a float32 emulation of dot_rows' two reduction orders (csrc/xps_stream.hip), and against emulated
kernels with one defect each, which the bounds must catch.  (The argument checks of the entry points that return before any
launch are in tests/test_realtime_pipeline_host.py.)"""
import itertools

import numpy as np
import pytest
import torch

import stream_ref as R

F32 = np.float32
KS = [1, 3, 4, 63, 64, 98, 256, 260, 1792]


# ---- float32 emulation of the kernels' arithmetic (lanes and shuffle tree written out) ----------------------------------
def emu_dot(w, x, vector, drop_tail=False):
    """One wave's dot product as dot_rows + wave_sum compute it.  vector: lane l takes the float4 groups at 4 l + 256 i,
    each summed ((p0 + p1) + p2) + p3; scalar: lane l takes the elements l + 64 i.  Then the xor-shuffle tree 32 .. 1.
    drop_tail: the defect of a kernel that forgets the last K % 64 elements."""
    w, x = np.asarray(w, F32), np.asarray(x, F32)
    K = w.size
    if drop_tail:
        K -= K % 64
    p = np.zeros(-(-max(K, 1) // 256) * 256, F32)
    p[:K] = w[:K] * x[:K]                                   # products rounded once (no FMA: the larger error)
    acc = np.zeros(64, F32)
    if vector:
        assert K % 4 == 0
        for blk in p.reshape(-1, 64, 4):
            acc = acc + (((blk[:, 0] + blk[:, 1]) + blk[:, 2]) + blk[:, 3])
    else:
        for blk in p.reshape(-1, 64):
            acc = acc + blk
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    assert acc.dtype == F32
    return acc[0]


def emu_gemv(x, W, bias, vector=None, drop_tail=False):
    B, K = x.shape
    vector = K % 4 == 0 if vector is None else vector
    out = np.zeros((B, W.shape[0]), F32)
    for s in range(B):
        for r in range(W.shape[0]):
            v = emu_dot(W[r], x[s], vector, drop_tail)
            out[s, r] = v + (bias[r] if bias is not None else F32(0))
    return out


def emu_cell(x, w_ih, w_hh, b_ih, b_hh, h, swap_bias=False):
    """gru_cell_gemv_kernel in float32.  swap_bias: the defect of reading b_ih[j] where b_ih[H + j] belongs."""
    B, K = x.shape
    H = h.shape[1]
    one = F32(1)
    out = np.zeros((B, H), F32)
    for s in range(B):
        for j in range(H):
            v = [emu_dot(w_ih[g * H + j], x[s], K % 4 == 0) for g in range(3)]
            v += [emu_dot(w_hh[g * H + j], h[s], H % 4 == 0) for g in range(3)]
            r = one / (one + np.exp(-(v[0] + b_ih[j] + v[3] + b_hh[j])))
            z = one / (one + np.exp(-(v[1] + b_ih[j if swap_bias else H + j] + v[4] + b_hh[H + j])))
            n = np.tanh(v[2] + b_ih[2 * H + j] + r * (v[5] + b_hh[2 * H + j]))
            out[s, j] = n + z * (h[s, j] - n)
    assert out.dtype == F32
    return out


# ---- the references against independent statements ---------------------------------------------------------------------
@pytest.mark.parametrize('H,K,B', [(1, 1, 1), (30, 98, 5), (64, 7, 3)])
def test_gru_cell_ref_equals_torch_grucell_double(H, K, B):
    rng = np.random.default_rng(H)
    x, w_ih, w_hh, b_ih, b_hh, h = R.cell_inputs(rng, H, K, B)
    cell = torch.nn.GRUCell(K, H).double()
    with torch.no_grad():
        for p, v in zip((cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh), (w_ih, w_hh, b_ih, b_hh)):
            p.copy_(torch.from_numpy(v.astype(np.float64)))
        want = cell(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(h.astype(np.float64))).numpy()
    got, parts = R.gru_cell_ref(x, w_ih, w_hh, b_ih, b_hh, h)
    assert np.abs(got - want).max() <= 1e-14
    # the parts are the six dots and their absolute sums
    assert parts['gi'].shape == parts['gh_abs'].shape == (3, B, H)
    np.testing.assert_allclose(parts['gi'][1, B - 1, H - 1], w_ih[2 * H - 1].astype(np.float64) @ x[B - 1], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(parts['gh_abs'][2, 0, 0], np.abs(w_hh[2 * H]).astype(np.float64) @ np.abs(h[0]), rtol=1e-13)


def test_gemv_ref_is_x_wt_plus_bias():
    rng = np.random.default_rng(1)
    x, W, bias = R.gemv_inputs(rng, 5, 98, 3)
    want = np.array([[sum(float(W[r, k]) * float(x[s, k]) for k in range(98)) + float(bias[r]) for r in range(5)]
                     for s in range(3)])
    np.testing.assert_allclose(R.gemv_ref(x, W, bias), want, rtol=0, atol=1e-14)
    np.testing.assert_allclose(R.gemv_ref(x, W), want - bias.astype(np.float64), rtol=0, atol=1e-14)


@pytest.mark.parametrize('max_tokens', [3, 64])
def test_collapse_ref_equals_groupby_minus_blank(max_tokens):
    rng = np.random.default_rng(max_tokens)
    T, B, ncls, blank = 50, 4, 5, 2
    ids = rng.integers(0, ncls, (T, B))
    logits = -np.ones((T, B, ncls))
    np.put_along_axis(logits, ids[..., None], 1.0, axis=2)
    snaps = R.collapse_ref(logits, blank, max_tokens, fill=-7)
    assert len(snaps) == T
    overflowed = 0
    for t in (0, 17, T - 1):
        arg, state, tokens = snaps[t]
        np.testing.assert_array_equal(arg, ids[t])
        for s in range(B):
            want = [int(k) for k, _ in itertools.groupby(ids[:t + 1, s]) if k != blank]
            assert state[s, 0] == ids[t, s]
            assert state[s, 1] == min(len(want), max_tokens)
            assert state[s, 2] == int(len(want) > max_tokens)
            overflowed += int(state[s, 2])
            assert list(tokens[s, :state[s, 1]]) == want[:max_tokens]
            assert (tokens[s, state[s, 1]:] == -7).all()
    assert (overflowed > 0) == (max_tokens == 3)


def test_collapse_ref_takes_the_first_maximum():
    logits = np.array([[[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0]]])
    arg, state, tokens = R.collapse_ref(logits, 0, 2)[0]
    assert list(arg) == [1, 0] and list(state[:, 1]) == [1, 0] and tokens[0, 0] == 1


def test_window_shift_ref_identity_is_shift_plus_cast():
    rng = np.random.default_rng(2)
    B, win, d, k = 3, 5, 4, 2
    src = rng.standard_normal((B, win * d)).astype(F32)
    power = rng.standard_normal((B, k, d)) * 1e3 + 1e-9
    dst, tol = R.window_shift_ref(power, k, None, None, src)
    np.testing.assert_array_equal(dst[:, :(win - k) * d], src[:, k * d:])
    np.testing.assert_array_equal(dst[:, (win - k) * d:], power.astype(F32).reshape(B, k * d))
    assert dst.dtype == F32 and not tol.any()
    # mapped by the identity matrix: the same frames; k == win leaves nothing of src
    W = np.broadcast_to(np.eye(d), (B, d, d))
    dst2, tol2 = R.window_shift_ref(power, k, W, None, src)
    np.testing.assert_array_equal(dst2, dst)
    assert (tol2 > 0).all()
    full = rng.standard_normal((B, win, d))
    dst3, _ = R.window_shift_ref(full, win, W, np.ones((B, d)), src)
    np.testing.assert_array_equal(dst3, (full + 1.0).astype(F32).reshape(B, win * d))


# ---- the bounds against the emulated arithmetic -------------------------------------------------------------------------
def test_dot_bound_holds_for_both_reduction_orders():
    """Emulated float32 error / D(K) for the scalar order at every K and the vector order where K % 4 == 0."""
    worst = 0.0
    for K in KS:
        rng = np.random.default_rng(1000 + K)
        x, W, _ = R.gemv_inputs(rng, 12, K, 3)
        ref = R.gemv_ref(x, W)
        bound = R.dot_bound(K, np.abs(x.astype(np.float64)) @ np.abs(W.astype(np.float64)).T)
        for vector in ([False, True] if K % 4 == 0 else [False]):
            got = emu_gemv(x, W, None, vector=vector)
            ratio = float((np.abs(got - ref) / bound).max())
            print(f'dot K={K} {"vector" if vector else "scalar"}: max error / D(K) = {ratio:.4f}')
            assert ratio <= 1.0
            worst = max(worst, ratio)
    assert worst > 1e-3          # the bound is of the error's order, not a formality


def test_gemv_bound_is_tight_enough_to_see_a_dropped_term_at_k_1792():
    rng = np.random.default_rng(1792)
    x, W, bias = R.gemv_inputs(rng, 130, 1792, 8)
    ref, bound = R.gemv_ref(x, W, bias), R.gemv_bound(x, W, bias)
    print(f'K=1792: max bound {bound.max():.3e}, 1e-4 max|out| = {1e-4 * np.abs(ref).max():.3e}')
    assert bound.max() <= 1e-4 * np.abs(ref).max()
    # one dropped product (|w x| ~ 0.5 / sqrt(K) * 0.8 ~ 1e-2) is far outside
    assert np.median(np.abs(W[:, -1:].astype(np.float64) * x[:, -1].astype(np.float64)).T / bound) > 10


@pytest.mark.parametrize('K', [63, 98, 260])
def test_gemv_bound_catches_a_dropped_tail(K):
    rng = np.random.default_rng(K)
    x, W, bias = R.gemv_inputs(rng, 5, K, 2)
    ref, bound = R.gemv_ref(x, W, bias), R.gemv_bound(x, W, bias)
    assert (np.abs(emu_gemv(x, W, bias) - ref) <= bound).all()
    assert (np.abs(emu_gemv(x, W, bias, drop_tail=True) - ref) > bound).any()


@pytest.mark.parametrize('H,K,scale', [(5, 6, 1.0), (30, 98, 1.0), (4, 256, 8.0)])
def test_cell_bound_holds_and_catches_a_bias_from_the_wrong_gate(H, K, scale):
    rng = np.random.default_rng(H * 1000 + K)
    args = R.cell_inputs(rng, H, K, 3, scale)
    ref, parts = R.gru_cell_ref(*args)
    bound = R.cell_bound(parts)
    err = np.abs(emu_cell(*args) - ref)
    print(f'cell H={H} K={K} scale={scale}: max error / bound = {(err / bound).max():.4f}')
    assert (err <= bound).all()
    assert (np.abs(emu_cell(*args, swap_bias=True) - ref) > bound).any()


def test_exact_collapse_comparison_catches_the_last_maximum():
    rng = np.random.default_rng(5)
    logits = rng.integers(0, 3, (20, 2, 11)).astype(F32)
    assert ((logits == logits.max(-1, keepdims=True)).sum(-1) > 1).mean() > 0.5
    last = np.flip(logits, -1)                 # first maximum of the flipped row = last maximum of the row
    wrong = [10 - a for a, _, _ in R.collapse_ref(last, 0, 64)]
    right = [a for a, _, _ in R.collapse_ref(logits, 0, 64)]
    assert any((w != r).any() for w, r in zip(wrong, right))
