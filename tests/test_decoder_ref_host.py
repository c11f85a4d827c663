"""tests/decoder_ref.py checked on the host (no GPU): replay against torch.nn.GRUCell + Linear in float64 with autograd; the
table gradient's gather rule; the token rule; logits_bound against float32 fmaf-chain restatements; the per-gate bounds
against float32 restatements of one step and pinned to step_bound's values; and the margin condition on the inputs of the
free-run cases tests/test_gpu_decoder_kernels.py runs."""
import numpy as np
import pytest
import torch

import decoder_ref as D
import gru_seq_ref as R
from test_gru_seq_ref_host import emu_dots, _sig_hw

F32 = np.float32
F64 = torch.float64


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(b).max()), 1e-300))


# ---- replay against torch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,H,C,L,ntok', [(5, 8, 4, 3, 5), (3, 64, 16, 8, 17)])
def test_replay_equals_torch_grucell_and_linear_double_with_autograd(B, H, C, L, ntok):
    rng = np.random.default_rng(1000 * B + H + C + L)
    inp = D.decoder_inputs(rng, B, H, C, L, ntok, 'normal')
    tokens = rng.integers(0, ntok, (L, B))
    dlogits = rng.standard_normal((B, L, C))
    out = D.replay(inp, tokens, dlogits)
    assert out['hs'].shape == (L + 1, B, H) and out['saved'].shape == (L, B, 4 * H) and out['logits'].shape == (B, L, C)

    t = {k: torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(True) for k, v in inp._asdict().items()}
    cell = torch.nn.GRUCell(3 * H, H).double()
    fc = torch.nn.Linear(H, C).double()
    with torch.no_grad():
        cell.weight_ih.copy_(torch.eye(3 * H, dtype=F64))
        cell.bias_ih.zero_()
        cell.weight_hh.copy_(t['w_hh'])
        cell.bias_hh.copy_(t['b_hh'])
        fc.weight.copy_(t['w_fc'])
        fc.bias.copy_(t['b_fc'])
    # path 1: torch's own cell -- states, logits, every parameter gradient, dgi, dh0
    h, hs, gis, lg = t['h0'], [t['h0']], [], []
    for s in range(L):
        gi = t['table'][torch.from_numpy(tokens[s])]
        gi.retain_grad()
        gis.append(gi)
        h = cell(gi, h)
        hs.append(h)
        lg.append(fc(h))
    logits = torch.stack(lg, dim=1)
    (logits * torch.from_numpy(dlogits)).sum().backward()
    assert _rel(out['hs'], torch.stack(hs).detach().numpy()) <= 1e-12
    assert _rel(out['logits'], logits.detach().numpy()) <= 1e-12
    assert _rel(out['dgi'], torch.stack([g.grad for g in gis]).numpy()) <= 1e-12
    assert _rel(out['dh0'], t['h0'].grad.numpy()) <= 1e-12
    assert _rel(out['dtable'], t['table'].grad.numpy()) <= 1e-12
    assert _rel(out['dw_hh'], cell.weight_hh.grad.numpy()) <= 1e-12
    assert _rel(out['db_hh'], cell.bias_hh.grad.numpy()) <= 1e-12
    assert _rel(out['dw_fc'], fc.weight.grad.numpy()) <= 1e-12
    assert _rel(out['db_fc'], fc.bias.grad.numpy()) <= 1e-12
    # path 2: the cell written out in torch, for what GRUCell keeps to itself -- r, z, n, q and dghn = d / dq
    W, b = t['w_hh'].detach(), t['b_hh'].detach()
    h, saved, qs = t['h0'].detach().clone().requires_grad_(True), [], []
    total = 0
    for s in range(L):
        gi = t['table'].detach()[torch.from_numpy(tokens[s])]
        gh = h @ W.T + b
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        q = gh[:, 2 * H:]
        q.retain_grad()
        n = torch.tanh(gi[:, 2 * H:] + r * q)
        h = (1 - z) * n + z * h
        assert float((h - hs[s + 1]).detach().abs().max()) <= 1e-14
        saved.append(torch.cat([r, z, n, q], dim=1))
        qs.append(q)
        total = total + ((h @ t['w_fc'].detach().T) * torch.from_numpy(dlogits[:, s])).sum()
    total.backward()
    assert _rel(out['saved'], torch.stack(saved).detach().numpy()) <= 1e-12
    assert _rel(out['dghn'], torch.stack([q.grad for q in qs]).numpy()) <= 1e-12


def test_float32_replay_is_float32_and_close():
    rng = np.random.default_rng(5)
    B, H, C, L, ntok = 7, 64, 9, 4, 10
    inp = D.decoder_inputs(rng, B, H, C, L, ntok, 'normal')
    tokens = rng.integers(0, ntok, (L, B))
    dlogits = rng.standard_normal((B, L, C)).astype(F32)
    o64, o32 = D.replay(inp, tokens, dlogits), D.replay(inp, tokens, dlogits, dtype=F32)
    for k, v in o32.items():
        assert v.dtype == F32 and 0 < np.abs(v - o64[k]).max() < 1e-4 * max(1.0, np.abs(o64[k]).max()), k


# ---- the table gradient ------------------------------------------------------------------------------------------------------
def test_dtable_sums_colliding_rows_and_leaves_unfed_rows_zero():
    rng = np.random.default_rng(6)
    B, H, C, L, ntok = 6, 8, 4, 3, 5
    inp = D.decoder_inputs(rng, B, H, C, L, ntok, 'normal')
    dlogits = rng.standard_normal((B, L, C))
    out = D.replay(inp, np.full((L, B), 2), dlogits)                      # all trials feed token 2 at every step
    want = np.zeros((ntok, 3 * H))
    want[2] = out['dgi'].sum((0, 1))
    assert np.abs(out['dtable'] - want).max() <= 1e-13 * np.abs(want).max() and np.abs(want[2]).min() > 0
    tokens = rng.integers(0, ntok - 1, (L, B))
    tokens[tokens == 1] = 0                                               # tokens 1 and ntok - 1 are never fed
    out = D.replay(inp, tokens, dlogits)
    assert not out['dtable'][1].any() and not out['dtable'][ntok - 1].any() and out['dtable'][0].any()
    for k in range(ntok):
        sel = out['dgi'][tokens == k]
        assert np.abs(out['dtable'][k] - sel.sum(0)).max() <= 1e-13 * max(1.0, np.abs(sel).max(initial=0.0))


# ---- the token rule ----------------------------------------------------------------------------------------------------------
def test_next_tokens_first_maximum_teacher_and_clamp():
    lg = np.array([[0.5, 2.0, 2.0, -1.0], [3.0, 3.0, 3.0, 3.0], [-1.0, -2.0, -0.5, -0.5], [0.0, -0.0, -1.0, -1.0]], F32)
    np.testing.assert_array_equal(D.next_tokens(lg, None, 0, 5), [1, 0, 2, 0])              # first maximum on exact ties
    teacher = np.array([3, 0, 2, 1])
    np.testing.assert_array_equal(D.next_tokens(lg, teacher, 1, 5), teacher)
    np.testing.assert_array_equal(D.next_tokens(lg, teacher, 0, 5), [1, 0, 2, 0])           # flag clear: argmax
    np.testing.assert_array_equal(D.next_tokens(lg, None, 1, 5), [1, 0, 2, 0])              # flag set, no teacher: argmax
    np.testing.assert_array_equal(D.next_tokens(lg, np.array([-3, 40, 4, 5]), 1, 5), [0, 4, 4, 4])   # clamped both ways
    np.testing.assert_array_equal(D.next_tokens(lg, None, 0, 2), [1, 0, 1, 0])              # an argmax above ntok - 1 clamps
    assert D.next_tokens(lg, None, 0, 5).dtype == np.int64


# ---- the bounds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,C', [(64, 1), (64, 16), (128, 9), (128, 16)])
def test_float32_fmaf_chains_stay_inside_logits_bound(H, C):
    """The kernel's chain restated: a = b, a = fl(a + h_k w_k) with the product exact (float64 holds a float32 product
    exactly, and the sum of it and a float32 to well below float32's rounding).  Also a chain that rounds every product
    first (no fma: twice the roundings) stays inside twice the bound -- the bound is of the error's order."""
    rng = np.random.default_rng(H + C)
    inp = D.decoder_inputs(rng, 32, H, C, 1, C + 1, 'normal')
    h, w, b = inp.h0, inp.w_fc, inp.b_fc
    a = np.broadcast_to(b, (32, C)).astype(F32)
    a2 = a.copy()
    for k in range(H):
        p = h[:, k:k + 1].astype(np.float64) * w[None, :, k].astype(np.float64)
        a = (a.astype(np.float64) + p).astype(F32)
        a2 = a2 + p.astype(F32)
    ref, bound = D.logits_ref(h, w, b), D.logits_bound(h, w, b)
    ratio, ratio2 = float((np.abs(a - ref) / bound).max()), float((np.abs(a2 - ref) / bound).max())
    print(f'H={H} C={C}: fmaf chain error / logits_bound = {ratio:.3f}, unfused chain = {ratio2:.3f}')
    assert ratio <= 1.0 and ratio2 <= 2.0 and ratio > 1e-3
    # a dropped term is beyond the bound on most elements
    dropped = np.abs(D.logits_ref(h[:, :-1], w[:, :-1], b) - ref)
    assert (dropped > bound).mean() > 0.9


def _old_step_bound(parts, mode, activation):
    """step_bound as it stood before gate_bounds was split off, kept here word for word as the pin."""
    import stream_ref as S
    U, SIG2, TANH2 = R.U, R.SIG2, R.TANH2
    gi, gh, bh = np.abs(parts['gi']), np.abs(parts['gh']), np.abs(parts['bh'])
    r, z, n, q, h = parts['r'], parts['z'], parts['n'], parts['q'], parts['h']
    D_ = R.DOT[mode] * parts['gh_abs']
    if activation == 'libm':
        A_r, A_z, A_n = S._act_err(r), S._act_err(z), S._act_err(n)
    else:
        A_r = A_z = R.SIG_ABS
        A_n = R.TANH_ABS
    da = [D_[g] + 3 * U * (gi[g] + gh[g] + bh[g]) for g in (0, 1)]
    dr = r * (1 - r) * da[0] + SIG2 * da[0] ** 2 + A_r
    dz = z * (1 - z) * da[1] + SIG2 * da[1] ** 2 + A_z
    dq = D_[2] + U * (gh[2] + bh[2])
    dan = r * dq + np.abs(q) * dr + dr * dq + 3 * U * (gi[2] + r * np.abs(q))
    dn = (1 - n * n) * dan + TANH2 * dan ** 2 + A_n
    return (1 - z) * dn + np.abs(h - n) * dz + dz * dn + 4 * U


@pytest.mark.parametrize('regime', ['normal', 'saturating'])
@pytest.mark.parametrize('H', [64, 128])
def test_gate_bounds_leave_step_bound_as_it_was_and_hold_float32_gates(H, regime):
    rng = np.random.default_rng(40 + H + len(regime))
    B, C, ntok = 16, 9, 10
    inp = D.decoder_inputs(rng, B, H, C, 1, ntok, regime)
    tok = rng.integers(0, ntok, B)
    ref, parts = D.step(inp.table, tok, inp.w_hh, inp.b_hh, inp.h0)
    for mode in R.DOT:
        for act in ('libm', 'hw'):
            gb = R.gate_bounds(parts, mode, act)
            np.testing.assert_array_equal(R.step_bound(parts, mode, act), _old_step_bound(parts, mode, act))
            np.testing.assert_array_equal(gb['h'], R.step_bound(parts, mode, act))
            assert set(gb) == set('rzqnh') and all(v.shape == (B, H) and (v > 0).all() for v in gb.values())
    # a float32 restatement of the decoder's cell (hw activations) stays inside every per-gate bound
    gi = inp.table[tok]
    gb = R.gate_bounds(parts, 'fp32', 'hw')
    worst = {k: 0.0 for k in 'rzqn'}
    for order in ('sequential', 'chains4', 'pairwise'):
        gh = emu_dots(inp.h0, inp.w_hh, order)
        r = _sig_hw((gi[:, :H] + gh[:, :H]) + inp.b_hh[:H])
        z = _sig_hw((gi[:, H:2 * H] + gh[:, H:2 * H]) + inp.b_hh[H:2 * H])
        q = gh[:, 2 * H:] + inp.b_hh[2 * H:]
        n = (2.0 * _sig_hw(F32(2) * (gi[:, 2 * H:] + r * q)).astype(np.float64) - 1.0).astype(F32)
        for k, v in zip('rzqn', (r, z, q, n)):
            assert v.dtype == F32
            worst[k] = max(worst[k], float((np.abs(v.astype(np.float64) - parts[k]) / gb[k]).max()))
    print(f'H={H} {regime}: float32 error / gate bound ' + ' '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0 and min(worst.values()) > 1e-3
    # exchanging r and z is beyond the bounds on most elements
    if regime == 'normal':
        assert (np.abs(parts['r'] - parts['z']) > gb['r']).mean() > 0.9


def test_saturating_table_plants_every_gate_in_the_rows_it_names():
    rng = np.random.default_rng(8)
    H, ntok = 64, 10
    inp = D.decoder_inputs(rng, 19, H, 9, 3, ntok, 'saturating')
    rows = D.planted_rows(ntok)
    assert ntok - 1 in rows and 0 in rows
    for row in range(ntok):
        cols = np.flatnonzero(np.abs(inp.table[row]) == R.PLANTED)
        if row in rows:
            assert len(cols) == 12 and {int(c) // H for c in cols} == {0, 1, 2}
            assert {float(v) for v in inp.table[row, cols]} == {R.PLANTED, -R.PLANTED}
        else:
            assert len(cols) == 0


# ---- the margin condition of the free-run cases ----------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(D.FREE_RUN_SEEDS))
def test_free_run_cases_keep_their_margins(case):
    """A condition on the INPUTS, met by the float64 reference alone: at most one trial in eight has a top-2 margin below
    MARGIN at any argmax step, so the kernel test may leave those out and still compare at least 7 / 8 of the trials."""
    H, B, C, L = case
    inp = D.free_run_inputs(H, B, C, L)
    tokens, logits, margins = D.free_run(inp, None, None, C, L=L)
    assert tokens.shape == (L, B) and margins.shape == (L - 1, B) and np.isfinite(margins).all()
    assert (tokens[0] == C).all() and tokens.max() <= C and len(np.unique(tokens[1:])) > 1
    excluded = float((margins.min(0) < D.MARGIN).mean())
    print(f'H={H} B={B} C={C} L={L} seed {D.FREE_RUN_SEEDS[case]}: excluded share {excluded:.3f} '
          f'(smallest margin {margins.min():.2e})')
    assert excluded <= D.MAX_EXCLUDED
    # free_run and replay are one computation
    out = D.replay(inp, tokens, np.zeros((B, L, C)))
    assert np.abs(out['logits'] - logits).max() <= 1e-13


def test_free_run_feeds_teacher_tokens_where_the_flag_is_set():
    rng = np.random.default_rng(9)
    B, H, C, L = 6, 64, 9, 4
    inp = D.decoder_inputs(rng, B, H, C, L, C + 1, 'normal')
    teacher = rng.integers(0, C, (B, L))
    tokens, _, margins = D.free_run(inp, teacher, np.array([1, 0, 1, 0]), C)
    np.testing.assert_array_equal(tokens[1], teacher[:, 0])
    np.testing.assert_array_equal(tokens[3], teacher[:, 2])
    assert np.isinf(margins[0]).all() and np.isfinite(margins[1]).all() and np.isinf(margins[2]).all()
    free, _, _ = D.free_run(inp, teacher, None, C)                          # flags = None: every token is the argmax
    alone, _, _ = D.free_run(inp, None, None, C, L=L)
    np.testing.assert_array_equal(free, alone)
