"""The CTC reference of tests/ctc_ref.py checked on the host, before the kernel is held to it (tests/test_gpu_ctc_loss.py):
float64 against torch's float64 CPU ctc_loss and its autograd gradient, float64 against a brute-force enumeration of every
alignment, the float32 emulation of the kernel's operation order inside nll_bound / grad_bound on the inputs of the device
grid, and every deliberately wrong variant (ctc_ref.MUTANTS) outside them on the same inputs."""
import functools
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_ref as R

EPS = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _ref(name, zi):
    """float64 reference with its bounds for one grid case, computed once: (nll, loss, dlogits, parts)."""
    c = _cases()[name]
    return R.ctc_ref(c['logits'], c['targets'], c['in_len'], c['tg_len'], c['blank'], zi, with_parts=True)


@functools.lru_cache(maxsize=None)
def _cases():
    return {c['name']: c for c in R.grid()}


ratios = R.error_ratios


# ---- float64 against torch ------------------------------------------------------------------------------------------------
TORCH_CASES = ['state_L0', 'state_L1', 'state_L31', 'state_L32', 'time_T1', 'time_T2', 'time_T65', 'class_C2', 'class_C65',
               'blank_0', 'blank_3', 'blank_6', 'feasible_0_exact', 'feasible_0_short', 'feasible_2_exact',
               'feasible_2_short', 'lengths', 'range_ties']


@pytest.mark.parametrize('zi', [True, False])
@pytest.mark.parametrize('name', TORCH_CASES)
def test_float64_matches_torch_float64(name, zi):
    """Ragged lengths, repeated labels, L = 0, blank in {0, mid, C - 1}, infeasible samples, in_len = 0 with tg_len 0 and 2.
    torch is given the clamped lengths (it rejects the others).  Tolerance: each of the Tb steps adds a few roundings relative
    to |alpha| <= |nll|: 8 (T + C) 2^-53 max(|value|, 1), and the same relative to the softmax scale 1 / (B max(L, 1)) for
    the gradient.  Under zero_infinity=False torch's gradient rows of an infinite-loss sample are NaN: left out, as the
    reference marks them unspecified."""
    c = _cases()[name]
    lg = c['logits'].astype(np.float64)
    T, B, C = lg.shape
    il, tl = R.clamp_lengths(T, c['targets'].shape[1], c['in_len'], c['tg_len'])
    tg = c['targets'] if c['targets'].shape[1] else np.zeros((B, 1), np.int64)
    x = torch.from_numpy(lg).requires_grad_(True)
    args = (torch.from_numpy(tg), torch.from_numpy(il), torch.from_numpy(tl))
    t_nll = F.ctc_loss(x.log_softmax(2), *args, blank=c['blank'], reduction='none', zero_infinity=zi).detach().numpy()
    t_loss = F.ctc_loss(x.log_softmax(2), *args, blank=c['blank'], reduction='mean', zero_infinity=zi)
    t_grad, = torch.autograd.grad(t_loss, x)
    t_loss, t_grad = float(t_loss.detach()), t_grad.numpy()
    nll, loss, dl = R.ctc_ref(lg, c['targets'], c['in_len'], c['tg_len'], c['blank'], zi)
    tol = 8 * (T + C) * EPS
    fin = np.isfinite(nll)
    assert np.array_equal(np.isfinite(t_nll), fin)
    assert np.array_equal(t_nll[~fin], nll[~fin])                                   # +inf where torch says +inf
    err = np.abs(t_nll[fin] - nll[fin]) / np.maximum(np.abs(nll[fin]), 1)
    assert (err <= tol).all(), err.max()
    if np.isfinite(loss):
        assert abs(t_loss - loss) <= tol * max(abs(loss), 1)
    else:
        assert t_loss == loss
    spec = ~np.isnan(dl)
    assert spec[:, fin].all()
    if not zi:                                                                      # torch: NaN exactly there
        assert np.isnan(t_grad[~spec]).all()
    gerr = np.abs(t_grad[spec] - dl[spec])
    assert (gerr <= tol / B).all(), (gerr.max(), tol / B)
    print(f'{name} zero_infinity={zi}: max nll err {err.max() if err.size else 0:.2e}, grad err {gerr.max():.2e} '
          f'(tolerance {tol:.2e})')


# ---- float64 against brute force ------------------------------------------------------------------------------------------
def test_float64_matches_brute_force():
    """Every target of length 0..3 over the labels {1, 2} (and, with blank = 1, over {0, 2}) at T = 1..5, C = 3.  The minimal
    feasible length T = L + repeats is among them with a finite nll, and one frame fewer must be exactly +inf."""
    checked = infeasible = minimal = 0
    for blank in (0, 1):
        labels = [c for c in range(3) if c != blank]
        for T in range(1, 6):
            lg = np.random.default_rng(10 * T + blank).standard_normal((T, 1, 3)) * 2
            for L in range(4):
                for target in itertools.product(labels, repeat=L):
                    brute = R.ctc_brute(lg[:, 0], target, blank)
                    tg = np.asarray(target, np.int64).reshape(1, L)
                    nll, _, _ = R.ctc_ref(lg, tg, [T], [L], blank, False)
                    need = L + R.n_repeats(target)
                    assert np.isfinite(brute) == (T >= need)
                    if T >= need:
                        assert abs(nll[0] - brute) <= 64 * EPS * max(brute, 1), (T, target, nll[0], brute)
                        minimal += T == need
                    else:
                        assert nll[0] == np.inf
                        infeasible += 1
                    checked += 1
    assert checked == 2 * 5 * 15 and infeasible > 40 and minimal > 20
    print(f'brute force: {checked} targets, {infeasible} infeasible, {minimal} with exactly one alignment class')


# ---- the grid's inputs ------------------------------------------------------------------------------------------------------
def test_grid_reaches_what_it_is_for():
    """The properties of the inputs that the grid's cases are named for."""
    cs = _cases()
    assert [2 * cs[f'state_L{L}']['tg_len'][0] + 1 for L in (0, 1, 31, 32, 63, 64, 100)] == [1, 3, 63, 65, 127, 129, 201]
    assert R.n_repeats(cs['state_L100']['targets'][1]) >= 3 and R.n_repeats(cs['state_L100']['targets'][0]) == 0
    env = _ref('envelope_L511', 1)
    assert env[0][0] > 0 and env[0][1] == 0 and not env[2][:, 1].any() and R.n_repeats(cs['envelope_L511']['targets'][0]) == 0
    for C in (65, 130):
        assert cs[f'class_C{C}']['targets'].min() >= 64
    for blank in (3, 6):
        assert (cs[f'blank_{blank}']['targets'] == 0).any() and not (cs[f'blank_{blank}']['targets'] == blank).any()
    for i in range(4):
        assert np.isfinite(_ref(f'feasible_{i}_exact', 0)[0]).all()
        assert np.array_equal(np.isinf(_ref(f'feasible_{i}_short', 0)[0]), [True, False, False])
    t = cs['range_ties']['logits']
    assert ((t == t.max(2, keepdims=True)).sum(2) >= 2).all()
    assert _ref('range_low_label', 1)[0].min() > 9e3 and np.isfinite(_ref('range_low_label', 1)[0]).all()


# ---- the float32 emulation inside the bounds ------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in R.grid()])
def test_float32_emulation_within_bounds(name):
    """What a correct float32 implementation in the kernel's order loses, against what the bounds allow.  The device's expf /
    logf may differ from numpy's by an ulp or two, so the emulation has to sit well inside: at most 0.9 (the largest
    ratios belong to range_shift, where the error is the half-ulp rounding of `log(sum) + max` at 1e4, 0.82 u |lse|,
    identical on any IEEE machine)."""
    c = _cases()[name]
    worst = [0.0, 0.0, 0.0]
    for zi in c['zi']:
        got = R.ctc_ref(c['logits'], c['targets'], c['in_len'], c['tg_len'], c['blank'], zi, dtype=np.float32)
        assert got[0].dtype == np.float32 and got[2].dtype == np.float32
        worst = [max(a, b) for a, b in zip(worst, ratios(got, _ref(name, zi)))]
    print(f'float32 emulation {name}: error / bound nll {worst[0]:.4f}, loss {worst[1]:.4f}, gradient {worst[2]:.4f}')
    assert max(worst) <= 0.9, worst


# ---- every mutant outside the bounds --------------------------------------------------------------------------------------
# the grid case that must tell each mutant from the operation, and why it can
MUTANT_CASE = {'skip_across_repeat': 'state_L31',              # sample 1 has adjacent repeats
               'no_skip': 'state_L31',
               'last_state_only': 'time_T65',
               'no_length_scale': 'state_L31',
               'length_unclamped_below': 'state_L0',           # L = 0
               'blank_zero': 'blank_3',
               'rows_not_zeroed': 'time_T65',                  # in_len = 63, 64 < T
               'beta_from_T': 'time_T65'}
SMALL = [c['name'] for c in R.grid() if c['family'] not in ('long', 'envelope', 'batch')]


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_mutant_exceeds_bounds(mutant):
    """Each wrong variant, computed in float64 (so with no rounding error of its own to hide behind), leaves the bounds on its
    named case; the number of small grid cases that catch it is printed."""
    assert set(MUTANT_CASE) == set(R.MUTANTS)
    caught = []
    for name in SMALL:
        c = _cases()[name]
        for zi in c['zi']:
            got = R.ctc_ref(c['logits'], c['targets'], c['in_len'], c['tg_len'], c['blank'], zi, mutant=mutant)
            if max(ratios(got, _ref(name, zi))) > 1.0:
                caught.append(name)
                break
    print(f'mutant {mutant}: outside the bounds on {len(caught)} of {len(SMALL)} small grid cases')
    assert MUTANT_CASE[mutant] in caught, caught
