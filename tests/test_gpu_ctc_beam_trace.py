"""The CTC prefix beam search on the MI355X held to its restatement member by member (csrc/xps_ctc_beam.hip against
tests/ctc_beam_ref.py::beam_trace): xps_ctc_beam_f64, xps_ctc_beam_step_f32 and xps_ctc_beam_readout called at the C ABI, every
buffer between guard words, over the grid of tests/ctc_beam_cases.py.

(a) streaming: after every step the state of every stream is decoded (tests/ctc_beam_state.py) and every member of rank below
    n_members is compared: the prefix walked back through hist, len, last, parent, cmask, both prefix hashes, p_b and p_nb.
(b) offline: the backpointer workspace starts as a sentinel; it must decode to the restatement's member count and prefixes in
    every frame, at every rank, and hold the sentinel everywhere else; three input forms (float64 log-probs, float32 log-probs,
    float32 logits), ragged lengths, lengths outside 0 .. T.
(c) streaming and offline agree bit for bit: backpointers as int32, the readout of every stream after every frame.
(d) a step at step == max_steps changes nothing but the overflow flag.

Comparison: integers and prefixes equal (so the order of members with equal scores is the restatement's: the tie rule);
scores |got - ref| <= 1e-12 max(1, |ref|), -inf where the restatement has -inf (ctc_beam_ref.close, the bound of
tests/test_gpu_ctc_beam.py between this kernel and this reference).  tests/test_ctc_beam_host.py shows on the host that every
input decides nothing by the last bit of an exp or a log, so the host's libm and the device's must give the same beam, and that
each deliberately wrong merge or tie rule changes at least one of these cases under this comparison.

Why these launches are in bounds (read in csrc/xps_ctc_beam.hip before they ran): both entry points check the sizes and the
workspace / state bytes they are given against their own formulas; the offline kernel writes hist[b][t][r] for t < len <= T,
r < n_new <= K and prefix[b][0 .. T), the step writes inside its stream's block of state_stride bytes for step < max_steps,
and the readout writes prefix[0 .. len), len <= step <= max_steps."""
import functools

import numpy as np
import pytest
import torch

import ctc_beam_cases as G
import ctc_beam_state as S
from ctc_beam_ref import close, lse
from guarded_buf import G as GUARD, SENT, SENT64

pytestmark = pytest.mark.gpu

FORMS = ('f64', 'f32', 'logits')     # offline input: float64 log-probs, float32 log-probs, float32 logits (from_logits = 1)


def _lib():
    from cross_patient_speech_decoding_amd._lib import lib
    return lib()


def _stream():
    from cross_patient_speech_decoding_amd._dev import stream
    return stream()


@pytest.fixture(scope='module', autouse=True)
def _built():
    from cross_patient_speech_decoding_amd import _build
    _build.build(verbose=False)
    assert torch.cuda.is_available(), 'gpu tests need the MI355X'


def _once(fn):
    """functools.lru_cache that also remembers a failure: a launch that went wrong is not sent again by the next test."""
    memo = {}

    @functools.wraps(fn)
    def wrapper(*key):
        if key not in memo:
            try:
                memo[key] = (fn(*key), None)
            except BaseException as e:           # noqa: B902 -- remembered and raised again, below
                memo[key] = (None, e)
        val, err = memo[key]
        if err is not None:
            raise err
        return val
    return wrapper


class Words:
    """Device bytes as int32 words between two guard rows of SENT.  data: an input (any numpy array of 4- or 8-byte elements),
    its bits are remembered; else nbytes of output filled with `fill` words."""

    def __init__(self, nbytes=None, data=None, fill=SENT):
        if data is not None:
            raw = np.frombuffer(np.ascontiguousarray(data).tobytes(), np.int32)
            nbytes = raw.nbytes
        assert nbytes % 4 == 0
        self.n = nbytes // 4
        self.buf = torch.full((GUARD + self.n + GUARD,), SENT, dtype=torch.int32, device='cuda')
        if data is not None:
            self.buf[GUARD:GUARD + self.n] = torch.from_numpy(raw.copy()).cuda()
            self.before = self.buf.clone()
        elif fill != SENT:
            self.buf[GUARD:GUARD + self.n] = fill
        self.ptr = self.buf.data_ptr() + 4 * GUARD
        assert self.ptr % 16 == 0

    def host(self, dtype=np.uint8):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().view(dtype)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.n:] == SENT).all())

    def unchanged(self):
        return torch.equal(self.buf, self.before)


def _bits(a):
    return np.asarray(a, np.float64).view(np.int64)


# ---- the launches, each sent once and shared by the tests that look at it ----------------------------------------------------
@_once
def _stream_run(name, B, max_steps, n_steps):
    """n_steps steps of B streams from a zeroed state.  Returns the state after every step ([B][stride] bytes) and the readout
    of every stream after every step: (prefix [B][max_steps] int64 as left by the kernel in a SENT64 row, len [B], nll [B])."""
    lib = _lib()
    T, Sn, K, blank = G.dims(name)
    frames = [min(t, T - 1) for t in range(n_steps)]                         # past the input's end: its last frame again
    z = np.stack([[G.logits(name, s)[t] for s in range(B)] for t in frames])     # [n_steps][B][S]
    zin = Words(data=z)
    nbytes = int(lib.xps_ctc_beam_state_bytes(B, K, max_steps))
    stride = S.state_stride(K, max_steps)
    assert nbytes == B * stride
    st = Words(nbytes, fill=0)
    blocks, reads = [], []
    for t in range(n_steps):
        rc = lib.xps_ctc_beam_step_f32(zin.ptr + 4 * t * B * Sn, Sn, blank, K, max_steps, st.ptr, nbytes, B, _stream())
        assert rc == 0, lib.xps_last_error()
        prefix, plen, nll = Words(8 * B * max_steps), Words(8 * B), Words(8 * B)
        for s in range(B):
            rc = lib.xps_ctc_beam_readout(st.ptr, nbytes, B, K, max_steps, s, prefix.ptr + 8 * s * max_steps, plen.ptr + 8 * s,
                                          nll.ptr + 8 * s, _stream())
            assert rc == 0, lib.xps_last_error()
        torch.cuda.synchronize()
        blocks.append(st.host().reshape(B, stride).copy())
        reads.append((prefix.host(np.int64).reshape(B, max_steps).copy(), plen.host(np.int64).copy(), nll.host(np.float64).copy()))
        assert prefix.guards_intact() and plen.guards_intact() and nll.guards_intact()
        assert st.guards_intact() and zin.guards_intact() and zin.unchanged()
    return blocks, reads


@_once
def _offline_run(name, form, seqs):
    """One launch of xps_ctc_beam_f64 over seqs = ((stream, length), ..): sequence b holds all T frames of its stream, the
    length says how many of them count.  Returns prefix [B][T], len [B], nll [B] and the workspace as int32 [B][T][K] (all of
    them started as sentinels)."""
    lib = _lib()
    T, Sn, K, blank = G.dims(name)
    B = len(seqs)
    if form == 'logits':
        x = np.stack([G.logits(name, s) for s, _ in seqs])
    else:
        x = np.stack([G.log_probs(name, s) for s, _ in seqs])
        x = x.astype(np.float32) if form == 'f32' else x
    assert x.dtype == (np.float64 if form == 'f64' else np.float32) and x.shape == (B, T, Sn)
    xin, lens = Words(data=x), Words(data=np.array([n for _, n in seqs], np.int64))
    ws_bytes = int(lib.xps_ctc_beam_workspace(B, T, K, Sn))
    assert ws_bytes >= 4 * B * T * K
    ws, prefix, plen, nll = Words(ws_bytes), Words(8 * B * T), Words(8 * B), Words(8 * B)
    rc = lib.xps_ctc_beam_f64(xin.ptr, int(form != 'f64'), B, T, Sn, lens.ptr, blank, K, int(form == 'logits'), prefix.ptr,
                              plen.ptr, nll.ptr, ws.ptr, ws_bytes, _stream())
    assert rc == 0, lib.xps_last_error()
    torch.cuda.synchronize()
    for w in (xin, lens, ws, prefix, plen, nll):
        assert w.guards_intact()
    assert xin.unchanged() and lens.unchanged()
    w = ws.host(np.int32)
    assert (w[B * T * K:] == SENT).all()                                     # the rounding of the workspace's size
    return (prefix.host(np.int64).reshape(B, T).copy(), plen.host(np.int64).copy(), nll.host(np.float64).copy(),
            w[:B * T * K].reshape(B, T, K).copy())


def _ragged(name):
    """(stream, length) of the offline test's five sequences: lengths T, 0, 1, T - 1, T."""
    T = G.dims(name)[0]
    return ((0, T), (1, 0), (2, 1), (0, T - 1), (1, T))


# ---- (a) streaming, every frame, every member ---------------------------------------------------------------------------------
def _stream_params():
    return [pytest.param(name, B, id=f'{name}-B{B}') for name in G.GRID for B in (1, 3, 8) if B < 8 or name in G.B8]


@pytest.mark.parametrize('name, B', _stream_params())
def test_streaming_holds_the_whole_beam(name, B):
    T, Sn, K, blank = G.dims(name)
    blocks, _ = _stream_run(name, B, T + 1, T)
    alone, _ = _stream_run(name, 1, T + 1, T)
    for t in range(T):
        for s in range(B):
            S.check_block(blocks[t][s], G.trace(name, s), t, K, T + 1, (name, B, 'frame', t, 'stream', s))
        # a stream's block changes through its own steps only: stream 0 run alone leaves the same block
        assert np.array_equal(S.canonical(blocks[t][0], K, T + 1), S.canonical(alone[t][0], K, T + 1)), (name, B, t)


# ---- (b) offline, every frame, every rank -----------------------------------------------------------------------------------------
def _check_offline(name, form, seqs, out):
    T = G.dims(name)[0]
    refs = [G.trace(name, s, form == 'f32')[:min(max(n, 0), T)] for s, n in seqs]      # the kernel's clamp
    S.check_offline(*out, refs, G.frames_held(name, form == 'f32'), SENT, (name, form))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('name', list(G.GRID))
def test_offline_holds_every_rank(name, form):
    T, Sn, K, blank = G.dims(name)
    seqs = _ragged(name)
    out = _offline_run(name, form, seqs)
    _check_offline(name, form, seqs, out)
    if form == 'logits':
        # the three forms give the same search: backpointers equal as int32 where the float32 rounding is held to it
        for other in ('f64', 'f32'):
            ws = _offline_run(name, other, seqs)[3]
            held = G.frames_held(name, other == 'f32')
            assert np.array_equal(ws[:, :held], out[3][:, :held]), (name, other)
        # lengths outside 0 .. T are clamped
        wild = ((0, T + 5), (1, -3), (2, 1), (0, T - 1), (1, T))
        clamped = _offline_run(name, form, wild)
        _check_offline(name, form, wild, clamped)
        for a, b in zip(clamped, out):
            assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)


# ---- (c) streaming equals offline, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(G.GRID))
def test_streaming_equals_offline_bit_for_bit(name):
    T, Sn, K, blank = G.dims(name)
    B = G.n_streams_checked(name)
    blocks, reads = _stream_run(name, B, T + 1, T)
    seqs = tuple((s, t + 1) for s in range(B) for t in range(T))              # every stream cut after every frame
    prefix, plen, nll, ws = _offline_run(name, 'logits', seqs)
    for s in range(B):
        hist = S.unpack_state(blocks[T - 1][s], K, T + 1)[2]
        for t in range(T):
            b = s * T + t
            n = len(G.trace(name, s)[t])
            assert np.array_equal(hist[t, :n], ws[b, t, :n]) and np.array_equal(ws[s * T + T - 1, t], ws[b, t]), (name, s, t)
            r_prefix, r_len, r_nll = reads[t]
            L = int(plen[b])
            assert r_len[s] == L, (name, s, t)
            assert r_prefix[s, :L].tolist() == prefix[b, :L].tolist(), (name, s, t)
            assert (r_prefix[s, L:] == SENT64).all(), (name, s, t, 'readout wrote behind the prefix')
            assert _bits(r_nll[s]) == _bits(nll[b]), (name, s, t, float(r_nll[s]), float(nll[b]))


# ---- (d) overflow leaves the beam alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, B', [('random', 3), ('sparse', 1)])
def test_overflowing_step_leaves_the_beam_alone(name, B):
    K = G.dims(name)[2]
    blocks, reads = _stream_run(name, B, 3, 5)
    for s in range(B):
        S.check_block(blocks[2][s], G.trace(name, s), 2, K, 3, (name, 'before the overflow', s))
        third = blocks[2][s].copy()
        assert third.view(np.int32)[2] == 0
        third.view(np.int32)[2] = 1
        assert np.array_equal(blocks[3][s], third), (name, s, 'the fourth step changed more than the flag')
        assert np.array_equal(blocks[4][s], third), (name, s, 'the fifth step changed something')
        for a, b in zip(reads[2], reads[4]):                                  # the readout is still the three-frame result
            assert np.array_equal(a[s].view(np.int64), b[s].view(np.int64)), (name, s)
        P, pb, pnb = G.trace(name, s)[2][0]
        assert reads[4][1][s] == len(P) and reads[4][0][s, :len(P)].tolist() == list(P)
        assert close(float(reads[4][2][s]), -lse(pb, pnb))
