"""CTC prefix beam search, host side (no GPU): the CPU restatement (tests/ctc_beam_ref.py) against the reference decode's
golden prefixes and nlls, argument checks of the C entry points (-1 and a message before any HIP call) and the size checks
of the Python wrappers.

Then what the whole-beam GPU tests (tests/test_gpu_ctc_beam_trace.py) stand on: the decoders of the kernels' state
(tests/ctc_beam_state.py) on hand-built data, every input of the grid (tests/ctc_beam_cases.py) shown to decide nothing by the
last bit of an exp or a log (trace_is_robust), and the discrimination table: for each deliberately wrong rule of
ctc_beam_ref.beam_trace a named case on which the GPU tests' comparison tells it from the right one."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from cross_patient_speech_decoding_amd import _build, _lib
import ctc_beam_cases as G
import ctc_beam_state as S
import f64_ref
from ctc_beam_ref import RULES, beam_search, beam_trace, lse, lse_longdouble, trace_diff, trace_is_robust

needs_long_double = pytest.mark.skipif(not f64_ref.have_long_double(), reason=f64_ref.LONG_DOUBLE_REASON)


@pytest.fixture(scope='module')
def lib():
    _build.build(verbose=False)
    return _lib.lib()


def _cases(golden_dir):
    g = np.load(os.path.join(golden_dir, 'ctc_beam.npz'))
    for i in range(int(g['n_cases'])):
        yield g[f'probs_{i}'], int(g[f'blank_{i}']), int(g[f'beam_{i}']), tuple(int(v) for v in g[f'prefix_{i}']), \
            float(g[f'nll_{i}'])


def test_restatement_equals_golden(golden_dir):
    n = 0
    for probs, blank, beam, prefix, nll in _cases(golden_dir):
        with np.errstate(divide='ignore'):
            lp = np.log(probs).reshape(probs.shape)
        got, got_nll = beam_search(lp, beam, blank)
        assert got == prefix
        assert got_nll == nll or (np.isnan(nll) and np.isnan(got_nll))
        n += 1
    assert n >= 30


def test_beam_entry_points_reject_bad_arguments(lib):
    p = C.c_void_p(16)
    f64 = lib.xps_ctc_beam_f64
    ws = lib.xps_ctc_beam_workspace(2, 5, 8, 11)
    assert ws >= 2 * 5 * 8 * 4
    for args in [(p, 0, 2, 5, 65, None, 0, 8, 0),        # classes > 64
                 (p, 0, 2, 5, 11, None, 0, 129, 0),      # beam > 128
                 (p, 0, 2, 5, 11, None, 0, 0, 0),        # beam 0
                 (p, 0, 2, 5, 11, None, 11, 8, 0),       # blank outside
                 (p, 2, 2, 5, 11, None, 0, 8, 0),        # dtype flag
                 (p, 0, 2, 5, 11, None, 0, 8, 2),        # from_logits flag
                 (p, 0, -1, 5, 11, None, 0, 8, 0)]:      # negative batch
        assert f64(*args, p, p, p, p, ws, None) == -1, args
        assert b'xps_ctc_beam_f64' in lib.xps_last_error()
    assert f64(None, 0, 2, 5, 11, None, 0, 8, 0, p, p, p, p, ws, None) == -1
    assert f64(p, 0, 2, 5, 11, None, 0, 8, 0, p, p, p, p, ws - 1, None) == -3             # workspace
    sb = lib.xps_ctc_beam_state_bytes(3, 100, 64)
    assert sb >= 3 * 64 * 100 * 4
    step = lib.xps_ctc_beam_step_f32
    assert step(p, 11, 0, 100, 64, p, sb, 9, None) == -1                                    # streams
    assert b'xps_ctc_beam_step_f32' in lib.xps_last_error()
    assert step(p, 11, 0, 129, 64, p, sb, 3, None) == -1
    assert step(p, 11, 11, 100, 64, p, sb, 3, None) == -1
    assert step(p, 11, 0, 100, 0, p, sb, 3, None) == -1
    assert step(None, 11, 0, 100, 64, p, sb, 3, None) == -1
    assert step(p, 11, 0, 100, 64, p, sb - 1, 3, None) == -3                                # state too small
    ro = lib.xps_ctc_beam_readout
    assert ro(p, sb, 3, 100, 64, 3, p, p, p, None) == -1                                    # stream index
    assert b'xps_ctc_beam_readout' in lib.xps_last_error()
    assert ro(p, sb, 3, 129, 64, 0, p, p, p, None) == -1
    assert ro(p, sb, 3, 100, 64, 0, None, p, p, None) == -1
    assert ro(p, sb - 1, 3, 100, 64, 0, p, p, p, None) == -3


def test_python_wrappers_reject_bad_sizes():
    from cross_patient_speech_decoding_amd.realtime_sim import beam_decode_batch, beam_decode_torch, decode
    lp = torch.zeros(2, 5, 11)
    for kw in [dict(beam_size=0), dict(beam_size=129), dict(blank=11), dict(blank=-1)]:
        with pytest.raises(ValueError):
            beam_decode_batch(lp, **kw)
    with pytest.raises(ValueError):
        beam_decode_batch(torch.zeros(1, 5, 65), beam_size=1)
    with pytest.raises(ValueError):
        beam_decode_batch(torch.zeros(5, 11))
    with pytest.raises(ValueError):
        beam_decode_batch(lp, input_lengths=[5])
    with pytest.raises(ValueError):
        beam_decode_batch(lp, input_lengths=[5, 6])
    with pytest.raises(ValueError):
        decode(np.full((4, 3), 1 / 3), beam_size=200)
    with pytest.raises(ValueError):
        decode(np.full(4, 0.5))
    with pytest.raises(ValueError):
        beam_decode_torch(torch.zeros(4, 3), blank=3)


# ---- the whole search: beam_trace, lse_longdouble, trace_is_robust ------------------------------------------------------------
def test_trace_first_member_equals_beam_search(golden_dir):
    for probs, blank, beam, prefix, nll in _cases(golden_dir):
        with np.errstate(divide='ignore'):
            lp = np.log(probs).reshape(probs.shape)
        trace = beam_trace(lp, beam, blank)
        assert len(trace) == len(lp)
        got, got_nll = beam_search(lp, beam, blank)
        if not trace:
            assert got == () and str(got_nll) == '-0.0'
            continue
        P, pb, pnb = trace[-1][0]
        assert P == got
        assert -lse(pb, pnb) == got_nll or (np.isnan(got_nll) and np.isnan(-lse(pb, pnb)))
        for frame in trace:
            assert 1 <= len(frame) <= beam and len({m[0] for m in frame}) == len(frame)
    with pytest.raises(ValueError):
        beam_trace([[0.0]], 1, 0, rule='no_such_rule')


@needs_long_double
def test_lse_longdouble_and_robustness():
    ninf = -np.inf
    assert lse_longdouble(ninf, ninf) == ninf and lse_longdouble(ninf, -1.5) == -1.5
    rng = np.random.default_rng(11)
    for _ in range(200):
        a = [float(v) for v in rng.standard_normal(3) * 5]
        assert abs(lse_longdouble(*a) - lse(*a)) <= 2.0 ** -51 * max(1.0, abs(lse(*a)))
    # structural ties survive the wider sum, coincidental ones do not
    assert trace_is_robust(G.log_probs('dupcols'), 12, 0) and trace_is_robust(G.log_probs('uniform'), 20, 0)
    dyadic = np.log(np.tile([0.5, 0.25, 0.125, 0.125], (6, 1)))
    assert not trace_is_robust(dyadic, 8, 0)
    assert trace_is_robust(dyadic[:3], 8, 0)                                  # it fails at frame 3


@needs_long_double
@pytest.mark.parametrize('name', list(G.GRID))
def test_grid_inputs_are_robust(name):
    """Every stream of every case the GPU tests run, as float64 log-probs (the streaming step, from_logits, the float64 offline
    form) and as their float32 roundings (the float32 offline form, but for the exception recorded in the grid)."""
    T, Sn, K, blank = G.dims(name)
    for s in range(G.n_streams_checked(name)):
        assert G.logits(name, s).shape == (T, Sn) and G.logits(name, s).dtype == np.float32
        assert not np.isnan(G.log_probs(name, s)).any() and (G.log_probs(name, s).max(1) > -np.inf).all()
        assert trace_is_robust(G.log_probs(name, s), K, blank), (name, s)
        held = G.frames_held(name, f32=True)
        assert trace_is_robust(G.log_probs(name, s, True)[:held], K, blank), (name, s, 'float32')
        if held < T:
            assert not trace_is_robust(G.log_probs(name, s, True)[:held + 1], K, blank), (name, s, 'the exception is none')
        a, b = G.trace(name, s), G.trace(name, s, True)                       # "the three forms give the same trace"
        assert [[m[0] for m in f] for f in a[:held]] == [[m[0] for m in f] for f in b[:held]]


def test_grid_reaches_its_branches():
    for name, n in G.BOUNDARY.items():
        T, Sn, K, blank = G.dims(name)
        for s in range(3):
            assert n in [len(f) for f in G.trace(name, s)[:-1]], (name, s)   # a frame STARTS with n members: n * S candidates
    assert [G.BOUNDARY[c] * G.dims(c)[1] for c in G.BOUNDARY] == [512, 513, 2048, 2080]
    assert all(len(f) < 128 for f in G.trace('sparse')[:5]) and len(G.trace('sparse')[-1]) == 128
    top = {name: max(max(S.expected_members(f)['cmask']) for f in G.trace(name)) for name in ('full', 'bit63')}
    assert top['full'] >> 32 and G.dims('full')[3] == 63                      # child bits above 31, the blank in the last column
    assert top['bit63'] >> 63                                                 # the top bit of cmask
    tr = G.trace('neginf')
    assert any(lse(pb, pnb) == -np.inf for f in tr for _, pb, pnb in f)     # a member whose score is -inf
    both = set()                                                              # both merge orders: parent before / after the member
    for f in G.trace('random'):
        index = {P: r for r, (P, _, _) in enumerate(f)}
        both |= {index[P[:-1]] < r for P, r in index.items() if P and P[:-1] in index}
    assert both == {True, False}


# Which case shows which wrong rule, under the streaming test's comparison ('all': every member's scores after every frame) and
# under the offline test's ('first': every prefix after every frame, the first member's nll).  Stream 0 of each.
CAUGHT_BY = {
    'tie_high': ('dupcols', 'uniform'),
    'parent_both': ('uniform', 'sparse'),
    'no_self': ('random', 'k1'),
    'repeat_both': ('random', 'neginf'),
    'blank_key': ('sparse',),
    'no_member_check': ('random', 'str_2048'),
}


@pytest.mark.parametrize('rule', RULES)
def test_discrimination_table(rule):
    assert set(CAUGHT_BY) == set(RULES)
    for name in CAUGHT_BY[rule]:
        T, Sn, K, blank = G.dims(name)
        wrong = beam_trace(G.log_probs(name), K, blank, rule=rule)
        for scores in ('all', 'first'):
            assert trace_diff(G.trace(name), wrong, scores) is not None, (rule, name, scores)
    # the comparison itself: a trace equals itself, a last-bit change of a score passes, a change of 1e-11 does not
    ref = G.trace('random')
    assert trace_diff(ref, ref) is None and trace_diff(ref, ref[:-1]) is not None
    P, pb, pnb = ref[-1][3]
    for d, same in ((np.spacing(pnb), True), (1e-11 * abs(pnb), False)):
        got = ref[:-1] + [ref[-1][:3] + [(P, pb, pnb + d)] + ref[-1][4:]]
        assert (trace_diff(ref, got) is None) == same
        assert trace_diff(ref, got, 'first') is None                          # not the first member: the offline form cannot see it


# ---- the decoders of the kernels' state ----------------------------------------------------------------------------------------
def test_state_bytes_formula(lib):
    for B, K, ms in [(1, 1, 1), (1, 3, 5), (3, 100, 64), (8, 128, 4), (2, 57, 6), (8, 16, 13), (1, 128, 4096), (4, 15, 17)]:
        stride = (64 + (K * 68 + 63) // 64 * 64 + ms * K * 4 + 255) // 256 * 256
        assert S.state_stride(K, ms) == stride
        assert lib.xps_ctc_beam_state_bytes(B, K, ms) == B * stride == S.state_bytes(B, K, ms)
    for bad in [(0, 4, 4), (1, 0, 4), (1, 4, 0)]:
        assert lib.xps_ctc_beam_state_bytes(*bad) == 0 == S.state_bytes(*bad)
    assert lib.xps_ctc_beam_workspace(5, 7, 9, 11) == (5 * 7 * 9 * 4 + 255) // 256 * 256


def test_pack_unpack_round_trip():
    rng = np.random.default_rng(5)
    for K, ms in [(1, 1), (3, 4), (16, 13), (57, 6), (128, 5)]:
        header = np.array([ms, K, 0, 0], np.int32)
        members = {}
        for name, dt in S.MEMBER_FIELDS:
            members[name] = rng.standard_normal(K) if np.dtype(dt).kind == 'f' else \
                rng.integers(0, 1 << 62, K).astype(dt) if np.dtype(dt).itemsize == 8 else rng.integers(-1, 1 << 20, K).astype(dt)
        members['p_b'][0] = -np.inf
        hist = rng.integers(0, 65 << 16, (ms, K)).astype(np.int32)
        block = S.pack_state(header, members, hist, K, ms)
        assert block.dtype == np.uint8 and block.size == S.state_stride(K, ms)
        h2, m2, hist2 = S.unpack_state(block, K, ms)
        assert np.array_equal(h2, header) and np.array_equal(hist2, hist)
        for name, dt in S.MEMBER_FIELDS:
            assert m2[name].dtype == np.dtype(dt) and np.array_equal(m2[name], members[name]), name
        assert np.array_equal(S.pack_state(h2, m2, hist2, K, ms), block)
        assert np.array_equal(S.unpack_state(block.tobytes(), K, ms)[2], hist)
        # the fields lie where the layout says: p_b first, parent last, hist behind the rounded set
        assert np.array_equal(block[64:64 + 8 * K].view(np.float64), members['p_b'])
        assert np.array_equal(block[64 + 64 * K:64 + 68 * K].view(np.int32), members['parent'])
        off = 64 + S.set_bytes(K)
        assert np.array_equal(block[off:off + 4 * ms * K].view(np.int32).reshape(ms, K), hist)
        assert not block[off + 4 * ms * K:].any() and not block[16:64].any()
        # canonical: what lies behind n_members does not count
        header[1] = max(1, K // 2)
        a = S.pack_state(header, members, hist, K, ms)
        for name in members:
            members[name][header[1]:] = 7
        b = S.pack_state(header, members, hist, K, ms)
        assert np.array_equal(S.canonical(a, K, ms), S.canonical(b, K, ms)) and (K == 1 or not np.array_equal(a, b))
    with pytest.raises(ValueError):
        S.unpack_state(np.zeros(100, np.uint8), 3, 4)


def _e(prev, tok=-1):
    return prev | (tok + 1) << 16


def test_member_prefix_and_workspace_on_hand_built_backpointers():
    SENT = 0x7FC0DEAD
    # frame 0: (), (2,), (0,)   frame 1: (2,), (2, 0), (), (0, 63)   frame 2: (2, 0), (2, 0, 1)
    hist = np.full((4, 4), SENT, np.int32)
    hist[0, :3] = [_e(0), _e(0, 2), _e(0, 0)]
    hist[1, :4] = [_e(1), _e(1, 0), _e(0), _e(2, 63)]
    hist[2, :2] = [_e(1), _e(1, 1)]
    assert S.split_entry(_e(5, 63)) == (5, 63) and S.split_entry(_e(127)) == (127, -1)
    assert [S.member_prefix(hist, 0, r) for r in range(3)] == [(), (2,), (0,)]
    assert [S.member_prefix(hist, 1, r) for r in range(4)] == [(2,), (2, 0), (), (0, 63)]
    assert [S.member_prefix(hist, 2, r) for r in range(2)] == [(2, 0), (2, 0, 1)]
    (counts, prefixes, stray), (c2, p2, s2) = S.unpack_workspace(np.stack([hist, np.full((4, 4), SENT, np.int32)]), SENT)
    assert counts.tolist() == [3, 4, 2, 0] and stray == 0
    assert prefixes == [[(), (2,), (0,)], [(2,), (2, 0), (), (0, 63)], [(2, 0), (2, 0, 1)], []]
    assert all(prefixes[t][r] == S.member_prefix(hist, t, r) for t in range(3) for r in range(counts[t]))
    assert c2.tolist() == [0, 0, 0, 0] and p2 == [[], [], [], []] and s2 == 0
    bad = hist.copy()
    bad[0, 3] = bad[3, 1] = 0                      # behind the members of frame 0 / in a frame the sequence does not have
    bad[2, 3] = 0
    assert S.unpack_workspace(bad[None], SENT)[0][0].tolist() == [4, 4, 2, 0] and S.unpack_workspace(bad[None], SENT)[0][2] == 2
    bad = hist.copy()
    bad[2, 0] = _e(4)                              # a member frame 1 does not have
    with pytest.raises(ValueError):
        S.unpack_workspace(bad[None], SENT)
    assert SENT >= 65 << 16                        # no backpointer (member < 128, token + 1 <= 64) equals the sentinel


def test_expected_members():
    frame = [((2,), -1.0, -2.0), ((2, 0), -np.inf, -3.0), ((), -4.0, -np.inf), ((0, 63), -np.inf, -5.0), ((2, 63), -np.inf, -6.0)]
    m = S.expected_members(frame)
    assert m['len'] == [1, 2, 0, 2, 2] and m['last'] == [2, 0, -1, 63, 63] and m['parent'] == [2, 0, -1, -1, 0]
    assert m['cmask'] == [1 | 1 << 63, 0, 1 << 2, 0, 0]
    assert m['p_b'][0] == -1.0 and m['p_nb'][4] == -6.0
    assert m['h1'][2] == 0 == m['hp1'][2] == m['hp1'][0] and m['h1'][0] == 3 and m['hp1'][1] == m['h1'][0]
    assert m['h2'][1] == (3 * S.HBASE2 + 1) % S.HMOD and m['h1'][3] == (S.HBASE1 + 64) % S.HMOD


# ---- the GPU tests' checks on states written by a stand-in for the kernel: the restatement itself, right or wrong ------------
def _hist_rows(tr):
    prev, rows = {(): 0}, []
    for f in tr:
        rows.append([prev[P] if P in prev else prev[P[:-1]] | (P[-1] + 1) << 16 for P, _, _ in f])
        prev = {P: r for r, (P, _, _) in enumerate(f)}
    return rows


def _state_from_trace(tr, t, K, ms, garbage=0):
    """The block a correct step leaves after frame t of the search `tr`; `garbage` fills the member slots behind the beam."""
    hist = np.zeros((ms, K), np.int32)
    for u, row in enumerate(_hist_rows(tr[:t + 1])):
        hist[u, :len(row)] = row
    exp, members = S.expected_members(tr[t]), {}
    for name, dt in S.MEMBER_FIELDS:
        members[name] = np.full(K, garbage, dt)
        members[name][:len(tr[t])] = np.array(exp[name], dtype=dt)
    return S.pack_state([t + 1, len(tr[t]), 0, 0], members, hist, K, ms)


def _offline_from_traces(trs, T, K):
    SENT = 0x7FC0DEAD
    B = len(trs)
    ws, prefix = np.full((B, T, K), SENT, np.int32), np.full((B, T), -1, np.int64)
    plen, nll = np.zeros(B, np.int64), np.zeros(B)
    for b, tr in enumerate(trs):
        for t, row in enumerate(_hist_rows(tr)):
            ws[b, t, :len(row)] = row
        P, pb, pnb = tr[-1][0] if tr else ((), 0.0, -np.inf)
        prefix[b, :len(P)], plen[b], nll[b] = P, len(P), -lse(pb, pnb)
    return prefix, plen, nll, ws


def _refused(check, *args):
    try:
        check(*args)
    except (AssertionError, ValueError):
        return True
    return False


@pytest.mark.parametrize('name', list(G.GRID))
def test_checks_accept_the_restatement_and_refuse_a_changed_state(name):
    SENT = 0x7FC0DEAD
    T, Sn, K, blank = G.dims(name)
    tr = G.trace(name)
    for t in range(T):
        block = _state_from_trace(tr, t, K, T + 1, garbage=3)
        S.check_block(block, tr, t, K, T + 1, name)
        assert np.array_equal(S.canonical(block, K, T + 1), S.canonical(_state_from_trace(tr, t, K, T + 1), K, T + 1))
    block, r = _state_from_trace(tr, T - 1, K, T + 1), len(tr[-1]) - 1
    for field, _ in S.MEMBER_FIELDS:                                           # one field of the last member, one step off
        h, m, hist = S.unpack_state(block, K, T + 1)
        if m[field].dtype.kind == 'f':
            m[field][r] = -1.0 if m[field][r] == -np.inf else m[field][r] - 1e-11 * max(1.0, abs(m[field][r]))
        else:
            m[field][r] += 1
        assert _refused(S.check_block, S.pack_state(h, m, hist, K, T + 1), tr, T - 1, K, T + 1, name), field
    for where in ((0, K - 1), (T, 0)):                                         # a backpointer behind the beam / in a frame not run
        h, m, hist = S.unpack_state(block, K, T + 1)
        if hist[where] == 0:
            hist[where] = 1
            assert _refused(S.check_block, S.pack_state(h, m, hist, K, T + 1), tr, T - 1, K, T + 1, name), where
    refs = [tr, [], tr[:1], tr[:T - 1]]
    out = _offline_from_traces(refs, T, K)
    S.check_offline(*out, refs, T, SENT, name)
    for b, t, r in ((0, T - 1, K - 1), (1, 0, 0), (3, T - 1, 0)):              # the last slot, an empty sequence, a frame past the end
        ws = out[3].copy()
        ws[b, t, r] = 0 if ws[b, t, r] == SENT else SENT
        assert _refused(S.check_offline, *out[:3], ws, refs, T, SENT, name), (b, t, r)
    nll = out[2].copy()
    nll[0] *= 1 + 1e-11
    assert nll[0] == out[2][0] or _refused(S.check_offline, out[0], out[1], nll, out[3], refs, T, SENT, name)


@pytest.mark.parametrize('rule', RULES)
def test_checks_refuse_each_wrong_rule(rule):
    """The discrimination table once more, through the GPU tests' own checks: a kernel that computed the wrong rule would leave
    these states and this workspace."""
    SENT = 0x7FC0DEAD
    for name in CAUGHT_BY[rule]:
        T, Sn, K, blank = G.dims(name)
        ref, wrong = G.trace(name), beam_trace(G.log_probs(name), K, blank, rule=rule)
        seen = [_refused(S.check_block, _state_from_trace(wrong, t, K, T + 1), ref, t, K, T + 1, name) for t in range(T)]
        assert any(seen), (rule, name, 'streaming')
        assert _refused(S.check_offline, *_offline_from_traces([wrong], T, K), [ref], T, SENT, name), (rule, name, 'offline')
