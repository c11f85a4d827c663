"""The numpy restatement of the CTC posterior occupancies (tests/ctc_occupancy_ref.py) held to a brute force over all frame
labellings, to torch's float64 CPU ctc_loss and its gradient, to its own invariants, to the alignment restatement in the exact
case, and its bounds to a long-double run and to four deliberately wrong variants; then the wrapper's host checks and its
cut of a batch into workspace runs.  No device."""
import itertools

import numpy as np
import pytest
import torch

from ctc_align_ref import align_ref
from ctc_occupancy_ref import MUTANTS, OUTPUTS, brute_force, occupancy_one, occupancy_ref, ratio, ratios


def _log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


BRUTE_TARGETS = ([], [1], [2], [1, 2], [1, 1], [2, 1, 2], [1, 1, 2], [1, 1, 1], [2, 2, 1])


def _brute_cases():
    """(x (T, 3), target) over T = 0 .. 6, L <= 3, repeated targets, infeasible ones and -inf entries."""
    rng = np.random.default_rng(0)
    for T, tg in itertools.product(range(7), BRUTE_TARGETS):
        x = rng.standard_normal((T, 3)) * 2
        yield f'T{T} {tg}', x, tg
        if T >= 3:
            y = x.copy()
            y[rng.random((T, 3)) < 0.25] = -np.inf
            yield f'T{T} {tg} -inf', y, tg


def test_restatement_equals_the_brute_force_within_the_bound():
    worst = dict.fromkeys(('log_z', 'token_occ', 'onset', 'class_occ'), 0.0)
    n_infeasible = n_feasible = 0
    for name, x, tg in _brute_cases():
        r = occupancy_one(x, tg, 0, bounds=True)
        z, tok, on, cls = brute_force(x, tg, 0)
        if z == -np.inf:
            n_infeasible += 1
            assert r['log_z'] == -np.inf, name
            assert not r['token_occ'].any() and not r['onset'].any() and not r['class_occ'].any(), name
            assert not r['expected_frames'].any() and np.isnan(r['onset_mean']).all(), name
            continue
        n_feasible += 1
        # the brute force itself: a few hundred products and fsums, each term within 4 u relative (exp) and the quotient 2 u
        own = 8 * 2.0 ** -53
        for k, v in (('log_z', z), ('token_occ', tok), ('onset', on), ('class_occ', cls)):
            err = np.abs(np.asarray(r[k], np.float64) - v)
            bd = np.asarray(r['bound'][k]) + own * np.maximum(np.abs(v), 1.0)
            assert (err <= bd).all(), (name, k, float(err.max()))
            worst[k] = max(worst[k], float(err.max()) if err.size else 0.0)
    print('largest |restatement - brute force|:', worst)
    assert n_feasible >= 60 and n_infeasible >= 20
    assert all(v <= 2e-14 for v in worst.values())


def _torch_case(seed, B, T, C, L, blank):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((T, B, C)) * 2
    labels = [c for c in range(C) if c != blank]
    tg = rng.choice(labels, size=(B, L)).astype(np.int64)
    tg[1, 1] = tg[1, 0]
    Tb = rng.integers(T - 4, T + 1, B)
    Ls = rng.integers(0, L + 1, B)
    Ls[0], Tb[0] = L, T
    return logits, tg, Tb, Ls


@pytest.mark.parametrize('blank', [0, 6])
def test_restatement_equals_torch_float64_ctc_loss(blank):
    """log_z = -nll, and class_occ = softmax - dlogits * B * max(L, 1) for the mean reduction (tests/ctc_ref.py states the
    scaling: dlogits = (softmax - occupancy) / (B max(L, 1))); agreement to 1e-12."""
    T, B, C, L = 23, 6, 7, 4
    logits, tg, Tb, Ls = _torch_case(40 + blank, B, T, C, L, blank)
    lg = torch.from_numpy(logits).requires_grad_(True)
    lp = torch.log_softmax(lg, dim=2)
    nll = torch.nn.functional.ctc_loss(lp, torch.from_numpy(tg), torch.from_numpy(Tb), torch.from_numpy(Ls), blank=blank,
                                       reduction='none', zero_infinity=False)
    loss = torch.nn.functional.ctc_loss(lp, torch.from_numpy(tg), torch.from_numpy(Tb), torch.from_numpy(Ls), blank=blank,
                                        reduction='mean', zero_infinity=False)
    assert bool(torch.isfinite(nll).all())
    loss.backward()
    r = occupancy_ref(lp.detach().numpy().transpose(1, 0, 2), tg, Tb, Ls, blank)
    assert np.abs(r['log_z'] + nll.detach().numpy()).max() <= 1e-12 * np.abs(r['log_z']).max()
    soft = np.exp(lp.detach().numpy())
    want = soft - lg.grad.numpy() * (B * np.maximum(Ls, 1))[None, :, None]
    live = np.arange(T)[:, None] < Tb[None, :]
    got = r['class_occ'].transpose(1, 0, 2)
    assert np.abs(got - want)[live].max() <= 1e-12
    assert not got[~live].any()
    # logits and their log-softmax have the same posteriors; log_z moves by the sum of the frames' constants
    raw = occupancy_ref(logits.transpose(1, 0, 2), tg, Tb, Ls, blank)
    for k in OUTPUTS[1:]:
        assert np.allclose(raw[k], r[k], rtol=0, atol=1e-11, equal_nan=True), k
    lse = (logits - lp.detach().numpy())[:, :, 0]
    shift = np.array([lse[:Tb[b], b].sum() for b in range(B)])
    assert np.allclose(raw['log_z'], r['log_z'] + shift, rtol=1e-13, atol=0)


def test_invariants():
    rng = np.random.default_rng(5)
    B, T, C, L = 8, 15, 6, 4
    x = rng.standard_normal((B, T, C)) * 3
    tg = rng.integers(1, C, (B, L))
    tg[2] = 3
    Tb, Ls = rng.integers(8, T + 1, B), rng.integers(0, L + 1, B)
    Ls[2] = L
    r = occupancy_ref(x, tg, Tb, Ls, 0)
    assert np.isfinite(r['log_z']).all()
    for b in range(B):
        n, l = int(Tb[b]), int(Ls[b])
        assert np.allclose(r['class_occ'][b, :n].sum(1), 1.0, rtol=0, atol=1e-13)
        assert np.allclose(r['onset'][b, :, :l].sum(0), 1.0, rtol=0, atol=1e-13)            # each token starts exactly once
        blank_mass = r['class_occ'][b, :n, 0].sum()
        assert abs(r['expected_frames'][b, :l].sum() + blank_mass - n) <= 1e-12 * n
        assert (np.diff(r['onset_mean'][b, :l]) > 0).all()                                   # tokens start in order
        assert (r['token_occ'][b] >= r['onset'][b] - 1e-15).all()                            # starting at t is being there at t
        assert np.isnan(r['onset_mean'][b, l:]).all() and not r['expected_frames'][b, l:].any()
        assert not r['token_occ'][b, n:].any() and not r['onset'][b, n:].any() and not r['class_occ'][b, n:].any()


def test_exact_case_equals_the_alignment_restatement():
    """Scores 0 on one labelling and -inf elsewhere: g and onset are EXACTLY the indicators of align_ref's states and
    token starts."""
    rng = np.random.default_rng(17)
    for tg, T in (([1, 2, 3], 9), ([2, 2, 1], 8), ([1, 1, 1], 7), ([2], 3), ([], 4)):
        L, S = len(tg), 2 * len(tg) + 1
        lab = [0] * S
        lab[1::2] = tg
        for _ in range(6):
            while True:
                s, path = int(rng.integers(0, min(2, S))), []
                for t in range(T):
                    path.append(s)
                    moves = [0] + ([1] if s + 1 < S else []) + ([2] if (s % 2 == 1 and s + 2 < S and lab[s + 2] != lab[s]) else [])
                    s += int(rng.choice(moves))
                if path[-1] >= S - 2:
                    break
            x = np.full((1, T, 4), -np.inf)
            for t, s in enumerate(path):
                x[0, t, lab[s]] = 0.0
            states, start, _, score = align_ref(x, np.array([tg], np.int64).reshape(1, L), None, None, 0)
            assert states[0].tolist() == path and score[0] == 0.0
            r = occupancy_ref(x, np.array([tg], np.int64).reshape(1, L), None, None, 0)
            assert r['log_z'][0] == 0.0
            j, t = np.arange(L)[None, :], np.arange(T)[:, None]
            assert np.array_equal(r['token_occ'][0], (states[0][:, None] == 2 * j + 1).astype(np.float64))
            assert np.array_equal(r['onset'][0], (start[0][None, :] == t).astype(np.float64))
            assert np.array_equal(r['onset_mean'][0], start[0].astype(np.float64))


def _bound_grid():
    """Small versions of the families the device is held on."""
    rng = np.random.default_rng(77)
    out = []
    for L in (0, 1, 5, 33):
        B, T, C = 3, L + 8, 7
        tg = rng.integers(1, C, (B, L))
        if L >= 2:
            tg[1, 1] = tg[1, 0]
        out.append((f'L{L}', rng.standard_normal((B, T, C)) * 2, tg, [T, T, T - 3], [L, L, max(L - 2, 0)]))
    tg = rng.integers(1, 11, (2, 5))
    out.append(('long', rng.standard_normal((2, 400, 11)) * 2, tg, [400, 371], [5, 4]))
    out.append(('sharp', rng.standard_normal((3, 25, 9)) * 30, rng.integers(1, 9, (3, 5)), [25, 19, 9], [5, 4, 5]))
    x = _log_softmax64(rng.standard_normal((4, 17, 6)) * 2)
    x[rng.random(x.shape) < 0.1] = -np.inf
    out.append(('-inf', x, rng.integers(1, 6, (4, 3)), [17, 17, 9, 17], [3, 2, 3, 0]))
    out.append(('float32 scores', (rng.standard_normal((3, 20, 5)) * 2).astype(np.float32), rng.integers(1, 5, (3, 4)), None, None))
    return out


@pytest.mark.skipif(np.finfo(np.longdouble).nmant <= 52, reason='np.longdouble is the 64-bit double on this machine: '
                    'there is no wider arithmetic to hold the float64 run against')
def test_bounds_hold_against_a_long_double_run():
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for name, x, tg, Tb, Ls in _bound_grid():
        r = occupancy_ref(x, tg, Tb, Ls, 0, bounds=True)
        wide = occupancy_ref(x, tg, Tb, Ls, 0, dtype=np.longdouble)
        for k, v in ratios({k: wide[k].astype(np.float64) for k in OUTPUTS}, r).items():
            worst[k] = max(worst[k], v)
    print('largest |float64 - long double| / bound:', worst)
    assert all(v <= 1.0 for v in worst.values()), worst
    assert max(worst.values()) > 1e-4                       # and the bound is no astronomical overestimate


@pytest.mark.parametrize('mutant', MUTANTS)
def test_wrong_variants_leave_the_bound(mutant):
    assert len(MUTANTS) >= 4
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for name, x, tg, Tb, Ls in _bound_grid():
        r = occupancy_ref(x, tg, Tb, Ls, 0, bounds=True)
        bad = occupancy_ref(x, tg, Tb, Ls, 0, mutant=mutant)
        for k, v in ratios(bad, r, factor=2.0).items():
            worst[k] = max(worst[k], v)
    print(mutant, worst)
    assert max(worst.values()) > 1e3, worst
    hit = {k for k, v in worst.items() if v > 1.0}
    assert {'onset', 'onset_mean'} <= hit
    if mutant != 'onset_without_skip':
        assert {'token_occ', 'class_occ', 'expected_frames'} <= hit


def test_ratio_matches_infinities_and_nans_exactly():
    ref, bd = np.array([0.5, -np.inf, np.nan]), np.array([1e-9, 0.0, 0.0])
    assert ratio(np.array([0.5 + 5e-10, -np.inf, np.nan]), ref, bd) == pytest.approx(0.5)
    assert ratio(np.array([0.5, -1e300, np.nan]), ref, bd) == np.inf
    assert ratio(np.array([0.5, -np.inf, 0.0]), ref, bd) == np.inf
    assert ratio(np.array([np.nan, -np.inf, np.nan]), ref, bd) == np.inf


# ---- the wrapper: every check before any device call, and the cut into workspace runs ----
def _pa(*a, **k):
    from cross_patient_speech_decoding_amd.realtime_sim import posterior_align
    return posterior_align(*a, **k)


def test_wrapper_refusals_need_no_device():
    x = torch.zeros(2, 5, 4)
    tg = torch.tensor([[1, 2], [3, 1]])
    with pytest.raises(ValueError, match='expected three axes'):
        _pa(torch.zeros(5, 4), tg)
    with pytest.raises(ValueError, match=r'expected \(B, Lmax\)'):
        _pa(x, torch.tensor([1, 2]))
    with pytest.raises(ValueError, match='expected integers'):
        _pa(x, tg.float())
    with pytest.raises(ValueError, match='1-D sequences'):
        _pa(x, [torch.tensor([[1]]), torch.tensor([2])])
    for blank in (-1, 4):
        with pytest.raises(ValueError, match=r'blank -?\d outside 0\.\.3'):
            _pa(x, tg, blank=blank)
    with pytest.raises(ValueError, match='3 targets for 2 sequences'):
        _pa(x, torch.zeros(3, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match='3 targets for 2 sequences'):
        _pa(x, [[1], [2], [3]])
    with pytest.raises(ValueError, match='2 targets for 5 sequences'):          # time_major swaps the axes
        _pa(x, tg, time_major=True)
    with pytest.raises(ValueError, match='3 input_lengths for 2 sequences'):
        _pa(x, tg, input_lengths=[5, 5, 5])
    with pytest.raises(ValueError, match='1 target_lengths for 2 sequences'):
        _pa(x, tg, target_lengths=[2])
    for bad in ([6, 5], [-1, 5]):
        with pytest.raises(ValueError, match=r'input_lengths outside 0\.\.5'):
            _pa(x, tg, input_lengths=bad)
    for bad in ([3, 1], [2, -1]):
        with pytest.raises(ValueError, match=r'target_lengths outside 0\.\.2'):
            _pa(x, tg, target_lengths=torch.tensor(bad))
    with pytest.raises(ValueError, match=r'label 4 at position 1: outside 0\.\.3'):
        _pa(x, torch.tensor([[1, 4], [3, 1]]))
    with pytest.raises(ValueError, match=r'label -1 at position 0: outside 0\.\.3'):
        _pa(x, [[1, 2], [-1]])
    with pytest.raises(ValueError, match='must be None'):
        _pa(x, [[1, 2], [1]], target_lengths=[2, 1])
    with pytest.raises(ValueError, match='at most 511'):
        _pa(torch.zeros(1, 3, 4), torch.ones(1, 512, dtype=torch.int64))
    with pytest.raises(ValueError, match='at least one class'):
        _pa(torch.zeros(1, 3, 0), torch.zeros(1, 0, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"want holds 'offset'"):
        _pa(x, tg, want=('onset', 'offset'))
    with pytest.raises(ValueError, match=r'one sequence of 5 frames and 2 labels needs 200 bytes of workspace: above max_workspace_bytes = 199'):
        _pa(x, tg, max_workspace_bytes=199)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='posterior_align needs the MI355X'):
            _pa(x, torch.tensor([[1, 99], [3, 1]]), target_lengths=[1, 2])


def test_the_checks_are_forced_aligns_own():
    from cross_patient_speech_decoding_amd.realtime_sim import ctc_align, ctc_occupancy
    assert ctc_occupancy.check_lattice_inputs is ctc_align.check_lattice_inputs


def test_workspace_runs_is_a_pure_function_of_the_sizes():
    from cross_patient_speech_decoding_amd.realtime_sim.ctc_occupancy import MAX_WORKSPACE_BYTES, workspace_runs
    per = 47 * 11 * 8
    assert workspace_runs(2048, 47, 5, MAX_WORKSPACE_BYTES) == [(0, 2048)]
    assert workspace_runs(10, 47, 5, 3 * per) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert workspace_runs(10, 47, 5, 4 * per - 1) == [(0, 3), (3, 6), (6, 9), (9, 10)]
    assert workspace_runs(10, 47, 5, per) == [(i, i + 1) for i in range(10)]
    assert workspace_runs(10, 47, 5, 10 * per) == [(0, 10)] and workspace_runs(0, 47, 5, 1) == []
    assert workspace_runs(4, 0, 5, 0) == [(0, 4)]                          # no frames: no workspace
    with pytest.raises(ValueError, match='above max_workspace_bytes'):
        workspace_runs(10, 47, 5, per - 1)
    # B = 2048, T = 512, L = 64: 1.08 GB of alpha, just above the default limit: two even runs, not 2032 + 16
    runs = workspace_runs(2048, 512, 64, MAX_WORKSPACE_BYTES)
    assert runs == [(0, 1024), (1024, 2048)]
    assert workspace_runs(10, 47, 5, 4 * per) == [(0, 4), (4, 8), (8, 10)] and workspace_runs(9, 47, 5, 5 * per) == [(0, 5), (5, 9)]
    assert all((b1 - b0) * 512 * 129 * 8 <= MAX_WORKSPACE_BYTES for b0, b1 in runs)
    for B, T, L, lim in ((7, 3, 2, 1000), (100, 9, 0, 80), (33, 5, 511, 10 ** 6)):
        runs = workspace_runs(B, T, L, lim)
        assert [r[0] for r in runs] == [0] + [r[1] for r in runs[:-1]] and runs[-1][1] == B
        assert all(0 < (b1 - b0) * T * (2 * L + 1) * 8 <= lim for b0, b1 in runs)


def test_readouts_on_host_tensors():
    """onset_times, peak and posteriorgram are plain tensor arithmetic on the result's fields."""
    from cross_patient_speech_decoding_amd.realtime_sim import CTCOccupancy
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 6, 4)) * 2
    tg = np.array([[1, 2], [3, 0]])
    r = occupancy_ref(x, tg, [6, 4], [2, 1], 0)
    t = {k: torch.from_numpy(r[k]) for k in OUTPUTS}
    occ = CTCOccupancy(t['log_z'], t['token_occ'], t['onset'], t['class_occ'], t['expected_frames'], t['onset_mean'],
                       torch.from_numpy(tg), torch.tensor([2, 1]), 0)
    assert occ.feasible.tolist() == [True, True] and occ.posteriorgram() is occ.class_occ
    ft = torch.tensor([0.1, 0.2, 0.4, 0.8, 1.6, 3.2], dtype=torch.float64)
    mean, sd = occ.onset_times(ft)
    w = r['onset']
    m = (w * ft.numpy()[None, :, None]).sum(1)
    v = (w * ft.numpy()[None, :, None] ** 2).sum(1) - m ** 2
    assert np.allclose(mean.numpy()[[0, 0, 1], [0, 1, 0]], m[[0, 0, 1], [0, 1, 0]], rtol=0, atol=1e-13)
    assert np.allclose(sd.numpy()[[0, 0, 1], [0, 1, 0]], np.sqrt(v[[0, 0, 1], [0, 1, 0]]), rtol=0, atol=1e-7)
    assert bool(torch.isnan(mean[1, 1])) and bool(torch.isnan(sd[1, 1]))
    # frame index as the time: the mean is onset_mean
    mean, _ = occ.onset_times(torch.arange(6))
    assert np.allclose(mean.numpy()[0], r['onset_mean'][0], rtol=0, atol=1e-13)
    assert np.array_equal(occ.peak().numpy(), r['token_occ'].max(1))
    with pytest.raises(ValueError, match='5 frame times for 6 frames'):
        occ.onset_times(torch.zeros(5))
    none = CTCOccupancy(t['log_z'], None, None, None, t['expected_frames'], t['onset_mean'], torch.from_numpy(tg), torch.tensor([2, 1]), 0)
    for call in (none.peak, none.posteriorgram, lambda: none.onset_times(ft)):
        with pytest.raises(ValueError, match='was not computed'):
            call()
