"""tests/gru_seq_ref.py checked on the host (no GPU): forward_ref / backward_ref against torch.nn.GRU in float64 with
autograd; step_bound against float32 restatements of one step (three summation orders, both activation forms) at every
(H, regime) tests/test_gpu_gru_recurrence.py launches; step_bound against restatements with one defect each, which it must
catch on most elements; route() at the corners of the dispatch rule."""
import numpy as np
import pytest
import torch

import gru_seq_ref as R

F32 = np.float32
# every hidden size tests/test_gpu_gru_recurrence.py launches
GPU_HS = [1, 4, 6, 20, 63, 64, 68, 124, 127, 128, 129, 132, 256, 258, 260, 320, 516, R.MAX_H_STEP]


# ---- the references against torch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_h0', [False, True])
@pytest.mark.parametrize('T,B,H,ndir', [(1, 1, 1, 1), (5, 3, 6, 1), (4, 2, 5, 2), (3, 4, 8, 2)])
def test_refs_equal_torch_gru_double_with_autograd(T, B, H, ndir, with_h0):
    """gi reaches torch.nn.GRU as its input through W_ih = [0 .. I .. 0] (direction d selects its own 3H columns) and
    b_ih = 0, so x.grad holds dgi of both directions side by side; dghn enters through W_hh.grad and b_hh.grad."""
    rng = np.random.default_rng(100 * T + 10 * H + ndir)
    gi, w, b, h0 = R.seq_inputs(rng, T, B, H, ndir, 'normal', with_h0)
    gru = torch.nn.GRU(ndir * 3 * H, H, 1, bidirectional=(ndir == 2)).double()
    with torch.no_grad():
        for d in range(ndir):
            sfx = '_l0' + ('_reverse' if d else '')
            sel = torch.zeros(3 * H, ndir * 3 * H, dtype=torch.float64)
            sel[:, d * 3 * H:(d + 1) * 3 * H] = torch.eye(3 * H, dtype=torch.float64)
            getattr(gru, 'weight_ih' + sfx).copy_(sel)
            getattr(gru, 'bias_ih' + sfx).zero_()
            getattr(gru, 'weight_hh' + sfx).copy_(torch.from_numpy(w[d].astype(np.float64)))
            getattr(gru, 'bias_hh' + sfx).copy_(torch.from_numpy(b[d].astype(np.float64)))
    x = torch.from_numpy(np.concatenate([gi[d] for d in range(ndir)], axis=-1).astype(np.float64)).requires_grad_(True)
    h0t = None if h0 is None else torch.from_numpy(h0.astype(np.float64)).requires_grad_(True)
    y, hn = gru(x, h0t)
    dy = rng.standard_normal((T, B, ndir * H))
    dhn = rng.standard_normal((ndir, B, H))
    ((y * torch.from_numpy(dy)).sum() + (hn * torch.from_numpy(dhn)).sum()).backward()

    y_ext, gates = R.forward_ref(gi, w, b, h0, T, B, H, ndir)
    assert y_ext.shape == (T + 2, B, ndir * H) and y_ext.dtype == np.float64
    assert np.abs(y_ext[1:T + 1] - y.detach().numpy()).max() <= 1e-14
    # the two h0 slots: slot 0 = h0 of the forward direction, slot T + 1 = h0 of the reverse one, the other halves zero
    want0, wantT = np.zeros((B, ndir * H)), np.zeros((B, ndir * H))
    if h0 is not None:
        want0[:, :H] = h0[0]
        if ndir == 2:
            wantT[:, H:] = h0[1]
    np.testing.assert_array_equal(y_ext[0], want0)
    np.testing.assert_array_equal(y_ext[T + 1], wantT)
    # final states: the forward direction ends at t = T - 1 (slot T), the reverse one at t = 0 (slot 1)
    assert np.abs(y_ext[T, :, :H] - hn[0].detach().numpy()).max() <= 1e-14
    if ndir == 2:
        assert np.abs(y_ext[1, :, H:] - hn[1].detach().numpy()).max() <= 1e-14

    dgi, dghn, dh0 = R.backward_ref(dy, dhn, y_ext, gates, w, T, B, H, ndir)
    xg = x.grad.numpy()
    for d in range(ndir):
        sfx = '_l0' + ('_reverse' if d else '')
        assert np.abs(dgi[d] - xg[..., d * 3 * H:(d + 1) * 3 * H]).max() <= 1e-13
        dgh = np.concatenate([dgi[d][..., :2 * H], dghn[d]], axis=-1)                 # (T, B, 3H)
        assert np.abs(dgh.sum((0, 1)) - getattr(gru, 'bias_hh' + sfx).grad.numpy()).max() <= 1e-12
        hprev = np.stack([y_ext[R._slots(t, d)[0], :, d * H:(d + 1) * H] for t in range(T)])
        dW = np.einsum('tbg,tbh->gh', dgh, hprev)
        assert np.abs(dW - getattr(gru, 'weight_hh' + sfx).grad.numpy()).max() <= 1e-12
    if h0 is not None:
        assert np.abs(dh0 - h0t.grad.numpy()).max() <= 1e-13
    # dy alone and dhn alone add up to both (the backward is linear in its seeds), and None means zero
    a = R.backward_ref(dy, None, y_ext, gates, w, T, B, H, ndir)
    c = R.backward_ref(None, dhn, y_ext, gates, w, T, B, H, ndir)
    for both, p, q in zip((dgi, dghn, dh0), a, c):
        assert np.abs(both - (p + q)).max() <= 1e-13
    z = R.backward_ref(np.zeros_like(dy), dhn, y_ext, gates, w, T, B, H, ndir)
    for p, q in zip(c, z):
        np.testing.assert_array_equal(p, q)


def test_float32_restatement_is_float32_and_close():
    rng = np.random.default_rng(3)
    T, B, H, ndir = 6, 4, 20, 2
    gi, w, b, h0 = R.seq_inputs(rng, T, B, H, ndir, 'normal', True)
    y64, g64 = R.forward_ref(gi, w, b, h0, T, B, H, ndir)
    y32, g32 = R.forward_ref(gi, w, b, h0, T, B, H, ndir, dtype=F32)
    assert y32.dtype == F32 and g32['q'].dtype == F32
    assert 0 < np.abs(y32 - y64).max() < 1e-5
    dy = rng.standard_normal((T, B, ndir * H)).astype(F32)
    out32 = R.backward_ref(dy, None, y32, g32, w, T, B, H, ndir, dtype=F32)
    out64 = R.backward_ref(dy, None, y64, g64, w, T, B, H, ndir)
    assert all(p.dtype == F32 and 0 < np.abs(p - q).max() < 1e-4 for p, q in zip(out32, out64))


def test_saturating_inputs_reach_both_rails_and_plant_every_gate():
    rng = np.random.default_rng(4)
    T, B, H = 4, 19, 64
    gi, w, b, h0 = R.seq_inputs(rng, T, B, H, 2, 'saturating', False)
    planted = np.argwhere(np.abs(gi) == R.PLANTED)
    assert len(planted) >= 10 and {int(c) // H for c in planted[:, 3]} == {0, 1, 2}
    assert {float(v) for v in gi[np.abs(gi) == R.PLANTED]} == {R.PLANTED, -R.PLANTED}
    _, g = R.forward_ref(gi, w, b, h0, T, B, H, 2)
    for k in 'rz':
        assert (g[k] < 1e-3).mean() > 0.05 and (g[k] > 1 - 1e-3).mean() > 0.05
    assert (np.abs(g['n']) > 1 - 1e-3).mean() > 0.3


@pytest.mark.parametrize('T,B,H,ndir,determined', [(64, 5, 128, 1, False), (64, 33, 64, 2, False), (7, 17, 64, 2, True),
                                                   (6, 21, 128, 2, True)])
def test_where_the_saturating_backward_is_determined_by_float32_inputs(T, B, H, ndir, determined):
    """Why tests/test_gpu_gru_recurrence.py checks the saturating regime's backward up to T = 8 only.  With w_hh 8 times
    wider the recurrence amplifies a perturbation at every step: gi * (1 + 1e-7) -- a change below float32's resolution --
    moves the FLOAT64 backward at T = 64 by more than the floor of the kernel test's tolerance, 1e-4 max(1, max |ref|).  The
    reference is then not a function of the float32 inputs to that accuracy; the tolerance's other term, 4 x the float32
    restatement's error, is one draw of the same amplified noise (it varies tenfold from seed to seed) and says nothing about
    another float32 computation.  At T <= 7 the same change stays below a tenth of the floor."""
    rng = np.random.default_rng(T + H)
    gi, w, b, h0 = R.seq_inputs(rng, T, B, H, ndir, 'saturating', True)
    dy = rng.standard_normal((T, B, ndir * H)).astype(F32)
    outs = []
    for g, dt in ((gi, np.float64), (gi.astype(np.float64) * (1 + 1e-7), np.float64), (gi, F32)):
        y, gates = R.forward_ref(g, w, b, h0, T, B, H, ndir, dtype=dt)
        outs.append(R.backward_ref(dy, None, y, gates, w, T, B, H, ndir, dtype=dt)[0].astype(np.float64))
    ref, moved, r32 = outs
    floor = 1e-4 * max(1.0, np.abs(ref).max())
    shift = np.abs(moved - ref).max()
    print(f'T={T} H={H}: max |dgi| {np.abs(ref).max():.2e}, moved by {shift:.2e} under gi (1 + 1e-7), floor {floor:.2e}, '
          f'float32 restatement off by {np.abs(r32 - ref).max():.2e}')
    assert (shift < 0.1 * floor) if determined else (shift > floor)


# ---- the bound against float32 restatements of one step -----------------------------------------------------------------
def emu_dots(h, W, order):
    """h (B, H) @ W (3H, H).T in float32, every product rounded once (no FMA: the larger error), summed in `order`:
    'sequential' k = 0 .. H - 1; 'chains4' four interleaved chains k % 4 added at the end (the k slots of an MFMA);
    'pairwise' numpy's blocked pairwise sum."""
    h, W = np.asarray(h, F32), np.asarray(W, F32)
    H = h.shape[1]
    if order == 'pairwise':
        return np.stack([(row[None, :] * W).sum(-1, dtype=F32) for row in h])
    acc = np.zeros((4 if order == 'chains4' else 1, h.shape[0], W.shape[0]), F32)
    for k in range(H):
        c = k % 4 if order == 'chains4' else 0
        acc[c] = acc[c] + h[:, k:k + 1] * W[None, :, k]
    out = acc[0]
    for c in range(1, acc.shape[0]):
        out = out + acc[c]
    assert out.dtype == F32
    return out


def _sig_libm(x):
    with np.errstate(over='ignore'):             # expf(100) = inf and 1 / inf = 0, as on the device
        return F32(1) / (F32(1) + np.exp(-x))


def _sig_hw(x):
    """rcp(1 + exp2(x * -log2e)) with a correctly rounded exp2 and reciprocal standing in for the 1-ulp instructions."""
    t = x * F32(-1.4426950408889634)
    with np.errstate(over='ignore'):
        e = np.exp2(t.astype(np.float64)).astype(F32)
        s = F32(1) + e
        return (1.0 / s.astype(np.float64)).astype(F32)


def emu_step(gi_t, W, b, h, gh, act, defect=None):
    """One step in float32 as the kernels compute it from the dots gh = emu_dots(h, W, order): (g + acc) + bias,
    q = acc + bias, n + z * (h - n).
    defect: None | 'gate_order' | 'bias_outside' | 'dropped_term' | 'z_exchanged' (in float64 for the non-vacuity check)."""
    dt = F32 if defect is None else np.float64
    gi_t, W, b, h = (np.asarray(a, dt) for a in (gi_t, W, b, h))
    H = h.shape[1]
    if defect is None:
        assert gh.dtype == F32
        sig = _sig_libm if act == 'libm' else _sig_hw
        tanh = np.tanh if act == 'libm' else (lambda x: (2.0 * sig(F32(2) * x).astype(np.float64) - 1.0).astype(F32))
    else:
        gh = (h[:, :H - 1] @ W[:, :H - 1].T) if defect == 'dropped_term' else h @ W.T
        sig, tanh = (lambda x: 1.0 / (1.0 + np.exp(-x))), np.tanh
    g = [gi_t[:, i * H:(i + 1) * H] for i in range(3)]
    a = [gh[:, i * H:(i + 1) * H] for i in range(3)]
    bb = [b[i * H:(i + 1) * H] for i in range(3)]
    i_r, i_z = (1, 0) if defect == 'gate_order' else (0, 1)
    r = sig((g[i_r] + a[i_r]) + bb[i_r])
    z = sig((g[i_z] + a[i_z]) + bb[i_z])
    if defect == 'bias_outside':
        n = tanh(g[2] + r * a[2] + bb[2])
    else:
        n = tanh(g[2] + r * (a[2] + bb[2]))
    out = h + z * (n - h) if defect == 'z_exchanged' else n + z * (h - n)
    assert out.dtype == dt
    return out


def _one_step_case(H, regime, B=6):
    rng = np.random.default_rng(7000 + 10 * H + len(regime))
    gi, w, b, h0 = R.seq_inputs(rng, 1, B, H, 1, regime, True)
    return gi[0, 0], w[0], b[0], h0[0]


# Largest float32 error / step_bound(mode 'fp32') over the three summation orders, per (H, regime) and activation form, as this
# test measured it (numpy 2.x, x86-64): an observation, not a tolerance.  The test asserts <= 1.
#    H:    (normal: libm, hw,  saturating: libm, hw)
MARGIN = {
    1: (0.126, 0.135, 0.037, 0.037), 4: (0.071, 0.104, 0.113, 0.110), 6: (0.152, 0.120, 0.121, 0.140),
    20: (0.162, 0.144, 0.190, 0.226), 63: (0.131, 0.130, 0.312, 0.359), 64: (0.122, 0.142, 0.272, 0.315),
    68: (0.125, 0.142, 0.290, 0.270), 124: (0.167, 0.255, 0.296, 0.347), 127: (0.127, 0.211, 0.326, 0.383),
    128: (0.125, 0.149, 0.292, 0.356), 129: (0.125, 0.152, 0.304, 0.360), 132: (0.142, 0.142, 0.341, 0.391),
    256: (0.134, 0.157, 0.313, 0.372), 258: (0.131, 0.130, 0.314, 0.313), 260: (0.169, 0.173, 0.274, 0.388),
    320: (0.156, 0.136, 0.391, 0.404), 516: (0.159, 0.163, 0.308, 0.359), 1264: (0.223, 0.208, 0.384, 0.414),
}


@pytest.mark.parametrize('H', GPU_HS)
def test_float32_steps_stay_inside_step_bound(H):
    for regime in ('normal', 'saturating'):
        gi_t, W, b, h = _one_step_case(H, regime)
        ref, parts = R.step_ref(gi_t, W, b, h)
        row = []
        dots = {order: emu_dots(h, W, order) for order in ('sequential', 'chains4', 'pairwise')}
        for act in ('libm', 'hw'):
            bound = R.step_bound(parts, 'fp32', act)
            worst = 0.0
            for order, gh in dots.items():
                got = emu_step(gi_t, W, b, h, gh, act)
                assert np.isfinite(got).all()
                ratio = float((np.abs(got.astype(np.float64) - ref) / bound).max())
                assert ratio <= 1.0, (H, regime, act, order, ratio)
                worst = max(worst, ratio)
            row.append(worst)
            assert (R.step_bound(parts, 'bf16x3', act) >= bound).all()
        print(f'H={H} {regime}: max float32 error / step_bound  libm {row[0]:.3f}  hw {row[1]:.3f}')
        if regime == 'saturating':
            assert (parts['z'] < 1e-3).any() and (parts['z'] > 1 - 1e-3).any() or H < 20
    # the bound is of the error's order, not a formality
    assert max(row) > 1e-2
    assert set(MARGIN) == set(GPU_HS)


def test_step_bound_stays_small_where_the_gates_saturate():
    """True derivatives: where r, z and n sit on a rail the bound falls to the activation allowance and the 4 u of the
    update, although sum |w||h| is 8 times the normal one."""
    gi_t, W, b, h = _one_step_case(128, 'saturating', B=32)
    _, parts = R.step_ref(gi_t, W, b, h)
    bound = R.step_bound(parts, 'fp32', 'hw')
    z, n = parts['z'], parts['n']
    rails = (z > 1 - 1e-4) | ((z < 1e-4) & (np.abs(n) > 1 - 1e-4))          # h' = h, or h' = n = +-1
    assert rails.mean() > 0.03
    print(f'on the rails: {rails.mean():.3f} of the elements, bound <= {bound[rails].max():.3e}; elsewhere median '
          f'{np.median(bound[~rails]):.3e}, max {bound.max():.3e}')
    assert bound[rails].max() < 4 * R.U + R.TANH_ABS + 2 * R.SIG_ABS + 2e-7
    assert np.median(bound[~rails]) > bound[rails].max()


# ---- non-vacuity: one defect each, at normal-scale inputs, in both modes' constants -----------------------------------------
DEFECT_HS = [6, 64, 128, 200, 512]
# Share (%) of the elements whose error exceeds step_bound, as this test measured it: defect -> {H: (fp32, bf16x3)}.
# An observation; the test asserts > 50 everywhere.
SHARES = {
    'gate_order': {6: (100.0, 100.0), 64: (100.0, 100.0), 128: (100.0, 100.0), 200: (100.0, 99.9), 512: (100.0, 99.9)},
    'bias_outside': {6: (100.0, 100.0), 64: (100.0, 100.0), 128: (100.0, 100.0), 200: (100.0, 99.9), 512: (100.0, 99.7)},
    'dropped_term': {6: (100.0, 100.0), 64: (100.0, 99.7), 128: (100.0, 99.6), 200: (99.7, 94.2), 512: (100.0, 98.6)},
    'reverse_slot': {6: (100.0, 100.0), 64: (100.0, 100.0), 128: (100.0, 100.0), 200: (100.0, 100.0), 512: (100.0, 100.0)},
    'z_exchanged': {6: (100.0, 100.0), 64: (100.0, 100.0), 128: (100.0, 100.0), 200: (100.0, 100.0), 512: (100.0, 99.9)},
}


def _reverse_slot_defect(H, rng):
    """Direction 1 at time t reads slot t + 2; the defect reads slot t (the state of two steps later in its own order)."""
    T, B = 5, 16
    gi, w, b, h0 = R.seq_inputs(rng, T, B, H, 2, 'normal', True)
    y, _ = R.forward_ref(gi, w, b, h0, T, B, H, 2)
    err, bounds = [], {m: [] for m in R.DOT}
    for t in range(1, T - 1):
        right, parts = R.step_ref(gi[1, t], w[1], b[1], y[t + 2, :, H:])
        assert np.abs(right - y[t + 1, :, H:]).max() <= 1e-14
        wrong, _ = R.step_ref(gi[1, t], w[1], b[1], y[t, :, H:])
        err.append(np.abs(wrong - right))
        for m in R.DOT:
            bounds[m].append(R.step_bound(parts, m, 'libm'))
    return np.stack(err), {m: np.stack(v) for m, v in bounds.items()}


@pytest.mark.parametrize('defect', ['gate_order', 'bias_outside', 'dropped_term', 'reverse_slot', 'z_exchanged'])
def test_step_bound_catches_each_defect_on_most_elements(defect):
    line = []
    for H in DEFECT_HS:
        rng = np.random.default_rng(900 + H)
        if defect == 'reverse_slot':
            err, bounds = _reverse_slot_defect(H, rng)
        else:
            gi, w, b, h0 = R.seq_inputs(rng, 1, 16, H, 1, 'normal', True)
            ref, parts = R.step_ref(gi[0, 0], w[0], b[0], h0[0])
            err = np.abs(emu_step(gi[0, 0], w[0], b[0], h0[0], None, None, defect=defect) - ref)
            # the looser of the two activation allowances at each element
            bounds = {m: np.maximum(R.step_bound(parts, m, 'libm'), R.step_bound(parts, m, 'hw')) for m in R.DOT}
        shares = {m: float((err > bounds[m]).mean()) for m in R.DOT}
        line.append(f'{H}: {100 * shares["fp32"]:.1f} {100 * shares["bf16x3"]:.1f}')
        assert min(shares.values()) > 0.5, (defect, H, shares)
    print(f'{defect}: share of elements beyond step_bound, H: fp32 % bf16x3 %   ' + '   '.join(line))


def test_step_ref_is_one_step_of_forward_ref():
    gi_t, W, b, h = _one_step_case(64, 'normal')
    ref, parts = R.step_ref(gi_t, W, b, h)
    y, gates = R.forward_ref(gi_t[None, None], [W], [b], h[None], 1, h.shape[0], 64, 1)
    assert np.abs(y[1] - ref).max() <= 1e-15
    for k in 'rzqn':
        assert np.abs(gates[k][0, 0] - parts[k]).max() <= 1e-14


# ---- the dispatch rule ------------------------------------------------------------------------------------------------------
def test_route_restates_the_dispatch_rule():
    r = R.route
    assert r(5, 1, 64, 1) == R.RESIDENT and r(3, 16, 128, 2) == R.RESIDENT
    assert r(5, 1, 64, 1, aligned=False) == R.GENERIC_SCALAR and r(5, 1, 128, 1, aligned=False) == R.GENERIC_SCALAR
    assert [r(4, 19, H, 2) for H in (4, 20, 68, 124)] == [R.GENERIC_VEC] * 4
    assert [r(4, 19, H, 2) for H in (1, 6, 63, 127)] == [R.GENERIC_SCALAR] * 4
    assert r(3, 5, 129, 1) == R.STEP and r(3, 130, 258, 1) == R.STEP
    assert r(3, 7, 132, 2) == R.STEP | R.STEP_VECA | R.STEP_VECB
    assert r(3, 7, 132, 2, aligned=False) == R.STEP | R.STEP_VECA
    assert r(3, 5, 132, 2, step_path=False) == R.GENERIC_VEC and r(3, 5, 256, 1, step_path=False) == R.GENERIC_VEC
    assert r(3, 5, 133, 2, step_path=False) == R.GENERIC_SCALAR
    # the envelope: the LDS-tile routes stop at 624, the per-step route at 1264, in both directions
    assert r(2, 3, R.MAX_H_TILE, 1, step_path=False) == R.GENERIC_VEC and r(2, 3, R.MAX_H_TILE + 1, 1, step_path=False) == R.REFUSED
    assert r(2, 3, R.MAX_H_STEP, 1) == R.STEP | 3 and r(2, 3, R.MAX_H_STEP + 1, 1) == R.REFUSED
    # cluster: 256 < H <= 512, H % 4 == 0, B >= 128, not in mode off, saved below 4 GiB
    assert r(4, 130, 320, 1) == R.CLUSTER and r(3, 300, 260, 2, cluster_mode=1) == R.CLUSTER
    assert r(4, 130, 320, 1, cluster_mode=0) == R.STEP | 3 and r(3, 300, 260, 2, cluster_mode=0) == R.STEP | 3
    assert r(4, 127, 320, 1) == R.STEP | 3 and r(4, 130, 256, 2) == R.STEP | 3 and r(4, 130, 258, 1) == R.STEP
    assert r(250, 2048, 512, 1) == R.CLUSTER and r(254, 2048, 512, 1) == R.STEP | 3
    assert r(0, 1, 64, 1) == r(1, 0, 64, 1) == r(1, 1, 0, 1) == r(1, 1, 64, 3) == R.REFUSED
    assert R.activation_of(R.STEP | 3) == 'libm' and R.activation_of(R.CLUSTER) == 'hw'


def test_library_route_query_agrees_where_no_device_is_needed():
    """xps_gru_seq_route is host logic: below H = 257 no cluster plan (and so no device property) enters the decision."""
    from cross_patient_speech_decoding_amd import _build, _lib
    _build.build(verbose=False)
    lib = _lib.lib()
    for (T, B, H, ndir) in [(5, 1, 64, 1), (3, 16, 128, 2), (4, 19, 20, 2), (4, 19, 63, 2), (3, 5, 129, 1), (3, 7, 132, 2),
                            (4, 130, 256, 2), (2, 3, 1, 1), (0, 1, 64, 1), (1, 1, 64, 3),
                            (2, 3, R.MAX_H_STEP, 1), (2, 3, R.MAX_H_STEP + 1, 1)]:
        for aligned in (0, 1):
            for backward in (0, 1):
                assert lib.xps_gru_seq_route(T, B, H, ndir, aligned, backward) == R.route(T, B, H, ndir, bool(aligned)), \
                    (T, B, H, ndir, aligned, backward)
    assert _lib.SIGNATURES['xps_gru_seq_route'][1] == [_lib.C.c_int] * 6
