"""The numpy restatement of CTC forced alignment (tests/ctc_align_ref.py) against a brute force over all frame labellings,
its tie rule on a hand-worked case, every ValueError of realtime_sim.forced_align (raised before any device call), and
window_end_times against the windows RealtimeRNNModel.reformat_time_windows cuts.  No GPU."""
import numpy as np
import pytest
import torch

from ctc_align_ref import align_one, align_ref, brute_force, collapse, frame_labels

BLANKS = (0, 2)
TARGETS = ([], [1], [1, 2], [1, 1], [2, 1], [0, 1], [0, 0], [2, 2])      # with every blank, so some hold "blank" as a label


def _cases():
    for T in range(0, 7):
        for tgt in TARGETS:
            for blank in BLANKS:
                if blank in tgt:
                    continue            # a target never holds the blank
                yield T, tgt, blank


def _check_against_brute(x, tgt, blank):
    states, start, end, score = align_one(x, tgt, blank)
    best, arg = brute_force(x, tgt, blank)
    assert score == best, (score, best)
    T = x.shape[0]
    if best == -np.inf:
        assert (states == -1).all() and (start == -1).all() and (end == -1).all()
        return 0
    path = tuple(frame_labels(states, tgt, blank))
    assert len(path) == T and collapse(path, blank) == list(tgt)
    assert path in arg
    if len(arg) == 1:
        assert path == arg[0]
    # the spans are the path's runs of each odd state
    for j in range(len(tgt)):
        assert (states[start[j]:end[j]] == 2 * j + 1).all() and (states == 2 * j + 1).sum() == end[j] - start[j]
    assert (np.diff(states) >= 0).all()
    return len(arg)


def test_restatement_equals_brute_force_on_all_labellings():
    rng = np.random.default_rng(0)
    n_unique = n_infeasible = 0
    for T, tgt, blank in _cases():
        x = rng.standard_normal((T, 3)) * 2
        n = _check_against_brute(x, tgt, blank)
        n_unique += n == 1
        n_infeasible += n == 0
    assert n_unique >= 40 and n_infeasible >= 10
    # the cases the issue names: a repeated-label target needs the blank between, and one frame fewer is infeasible
    x = rng.standard_normal((3, 3))
    states, start, end, score = align_one(x, [1, 1], 0)
    assert states.tolist() == [1, 2, 3] and start.tolist() == [0, 2] and end.tolist() == [1, 3]
    assert score == (x[1, 0] + x[0, 1]) + x[2, 1] or score == x[2, 1] + (x[1, 0] + x[0, 1])
    assert align_one(x[:2], [1, 1], 0)[3] == -np.inf


def test_restatement_equals_brute_force_with_ties_and_neg_inf():
    rng = np.random.default_rng(1)
    n_tied = 0
    for T, tgt, blank in list(_cases()) * 3:
        x = np.round(rng.standard_normal((T, 3))) * 0.25                   # multiples of 0.25 from a handful of values
        n_tied += _check_against_brute(x, tgt, blank) > 1
        if T:
            x[rng.integers(T), rng.integers(3)] = -np.inf
            _check_against_brute(x, tgt, blank)
    assert n_tied >= 30             # the inputs do tie: this many cases have several maximising labellings


def test_tie_rule_by_hand():
    # all scores equal: every feasible path ties, so the path is decided by the tie rule alone.
    # target (1), blank 0, T = 4, states (b, 1, b).  Forward: v_0 = (0, 0, -inf).  Stay wins every tie, so back(t, 1) = stay
    # for all t, back(t, 2) = stay once v(2) is finite (t >= 2), back(1, 2) = from 1.  End rule: v(2) = v(1), not strictly
    # larger, so the path ends in S - 1 = 2; walking back: t=3: 2 (stay), t=2: 2 (stay), t=1: 2 (came from 1), t=0: 1.
    z = np.zeros((4, 3))
    states, start, end, score = align_one(z, [1], 0)
    assert states.tolist() == [1, 2, 2, 2] and start.tolist() == [0] and end.tolist() == [1] and score == 0.0
    # the end rule: state S-2 only when strictly larger
    z2 = z.copy()
    z2[3, 1] = 0.25                       # ending in the token is now better by 0.25
    states, start, end, score = align_one(z2, [1], 0)
    assert states.tolist() == [1, 1, 1, 1] and (start.tolist(), end.tolist()) == ([0], [4]) and score == 0.25
    # stay before move: at t = 1 state 1 can stay (v = 0) or be entered from state 0 (v = 0): stay, so the token began at 0
    z3 = z.copy()
    z3[2:, 0] = -1.0                     # the trailing blank costs: the path stays in the token to the end
    states, start, end, score = align_one(z3, [1], 0)
    assert states.tolist() == [1, 1, 1, 1] and score == 0.0
    # a move needs a strictly larger value: a better blank at t = 0 makes entering from state 0 win at t = 1
    z4 = z.copy()
    z4[0, 0] = 0.25
    z4[3, 1] = 0.25
    states, start, end, score = align_one(z4, [1], 0)
    assert states.tolist() == [0, 1, 1, 1] and start.tolist() == [1] and score == 0.5
    # the skip s-2 loses ties to s-1: target (1, 2), T = 2 has one path; T = 3 with zeros: end in S-1 = 4
    states, start, end, score = align_one(np.zeros((3, 3)), [1, 2], 0)
    assert states.tolist() == [1, 3, 4] and start.tolist() == [0, 1] and end.tolist() == [1, 2]
    # L = 0: the all-blank path; T = 0: the empty alignment
    states, start, end, score = align_one(np.array([[0.5, 9.0], [0.25, 9.0]]), [], 0)
    assert states.tolist() == [0, 0] and score == 0.75
    assert align_one(np.zeros((0, 3)), [], 0)[3] == 0.0 and align_one(np.zeros((0, 3)), [1], 0)[3] == -np.inf


def test_batch_form_pads_and_clamps():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, 5, 4))
    tg = np.array([[1, 2, 3], [2, 2, 0], [3, 1, 1]])
    states, start, end, score = align_ref(x, tg, [5, 9, -1], [3, 2, 7], 0)
    s1 = align_one(x[1], [2, 2], 0)
    assert np.array_equal(states[1], s1[0]) and start[1].tolist() == s1[1].tolist() + [-1] and score[1] == s1[3]
    assert (states[2] == -1).all() and score[2] == -np.inf and (start[2] == -1).all()
    assert np.array_equal(states[0], align_one(x[0], [1, 2, 3], 0)[0])


# ---- the wrapper's refusals: every one before any device call ----
def _fa(*a, **k):
    from cross_patient_speech_decoding_amd.realtime_sim import forced_align
    return forced_align(*a, **k)


def test_wrapper_refusals_need_no_device():
    x = torch.zeros(2, 5, 4)
    tg = torch.tensor([[1, 2], [3, 1]])
    with pytest.raises(ValueError, match='expected three axes'):
        _fa(torch.zeros(5, 4), tg)
    with pytest.raises(ValueError, match=r'expected \(B, Lmax\)'):
        _fa(x, torch.tensor([1, 2]))
    with pytest.raises(ValueError, match='expected integers'):
        _fa(x, tg.float())
    with pytest.raises(ValueError, match='1-D sequences'):
        _fa(x, [torch.tensor([[1]]), torch.tensor([2])])
    for blank in (-1, 4):
        with pytest.raises(ValueError, match=r'blank -?\d outside 0\.\.3'):
            _fa(x, tg, blank=blank)
    with pytest.raises(ValueError, match='3 targets for 2 sequences'):
        _fa(x, torch.zeros(3, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match='3 targets for 2 sequences'):
        _fa(x, [[1], [2], [3]])
    with pytest.raises(ValueError, match='2 targets for 5 sequences'):          # time_major swaps the axes
        _fa(x, tg, time_major=True)
    with pytest.raises(ValueError, match='3 input_lengths for 2 sequences'):
        _fa(x, tg, input_lengths=[5, 5, 5])
    with pytest.raises(ValueError, match='1 target_lengths for 2 sequences'):
        _fa(x, tg, target_lengths=[2])
    for bad in ([6, 5], [-1, 5]):
        with pytest.raises(ValueError, match=r'input_lengths outside 0\.\.5'):
            _fa(x, tg, input_lengths=bad)
    for bad in ([3, 1], [2, -1]):
        with pytest.raises(ValueError, match=r'target_lengths outside 0\.\.2'):
            _fa(x, tg, target_lengths=torch.tensor(bad))
    with pytest.raises(ValueError, match=r'label 4 at position 1: outside 0\.\.3'):
        _fa(x, torch.tensor([[1, 4], [3, 1]]))
    with pytest.raises(ValueError, match=r'label -1 at position 0: outside 0\.\.3'):
        _fa(x, [[1, 2], [-1]])
    with pytest.raises(ValueError, match='must be None'):
        _fa(x, [[1, 2], [1]], target_lengths=[2, 1])
    with pytest.raises(ValueError, match='at most 511'):
        _fa(torch.zeros(1, 3, 4), torch.ones(1, 512, dtype=torch.int64))
    with pytest.raises(ValueError, match='at least one class'):
        _fa(torch.zeros(1, 3, 0), torch.zeros(1, 0, dtype=torch.int64))
    # a label past a target's length is padding, not an error: the call gets as far as asking for the device
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='forced_align needs the MI355X'):
            _fa(x, torch.tensor([[1, 99], [3, 1]]), target_lengths=[1, 2])


def test_window_end_times_follow_reformat_time_windows():
    from cross_patient_speech_decoding_amd.realtime_sim import RealtimeRNNModel, window_end_times
    win, stride, step = 6, 4, 0.01
    m = RealtimeRNNModel(win * 2, 8, 1, 5, dropout=0.0, win_size=win, stride=stride)
    x = torch.arange(30, dtype=torch.float32)[None, :, None].expand(1, 30, 2).contiguous()     # every row holds its own index
    w = m.reformat_time_windows(x)                                   # (1, n_windows, win * 2)
    nw = m.n_windows(30)
    assert w.shape == (1, nw, win * 2) and nw == 7
    last_row = w[0].max(dim=1).values.double()                        # the latest input row each window holds
    got = window_end_times(nw, win, stride, step)
    assert got.dtype == torch.float64 and torch.equal(got, (last_row + 1) * step)
    assert got[0] == win * step and window_end_times(0, win, stride, step).numel() == 0
    with pytest.raises(ValueError):
        window_end_times(3, 0, 4, step)
