"""Decoders for what the CTC beam kernels leave behind (csrc/xps_ctc_beam.hip; the layout is written down in include/xps.h at
xps_ctc_beam_step_f32): the streaming state of one stream and the offline kernel's backpointer workspace, back into prefixes
and member arrays that can be compared with ctc_beam_ref.beam_trace.  numpy only; pack_state is the inverse of unpack_state
so that the decoder itself is tested on the host (tests/test_ctc_beam_host.py).

One stream block:
    header, 64 bytes      int32 {step, n_members, overflow, 0}
    member set            K * 68 bytes rounded up to a multiple of 64:
                          double p_b[K], p_nb[K]; uint64 h1[K], h2[K], hp1[K], hp2[K], cmask[K]; int32 len[K], last[K], parent[K]
    backpointers          int32 hist[max_steps][K] = member of the previous frame | (appended token + 1) << 16
    stride                rounded up to a multiple of 256
Slots of the member set at rank >= n_members, and the padding behind it, hold nothing: the step copies the whole set from
LDS, whatever those slots held there.  hist slots at rank >= the frame's member count and frames >= step are never written."""
import numpy as np

HEADER_BYTES = 64
MEMBER_FIELDS = (('p_b', np.float64), ('p_nb', np.float64), ('h1', np.uint64), ('h2', np.uint64), ('hp1', np.uint64),
                 ('hp2', np.uint64), ('cmask', np.uint64), ('len', np.int32), ('last', np.int32), ('parent', np.int32))
HMOD = (1 << 61) - 1
HBASE1 = 0x1f3d5b79a2c4e68d % HMOD
HBASE2 = 0x0b9e2a6c7f15d34b % HMOD


def set_bytes(K):
    return (K * 68 + 63) // 64 * 64


def state_stride(K, max_steps):
    return (HEADER_BYTES + set_bytes(K) + max_steps * K * 4 + 255) // 256 * 256


def state_bytes(B, K, max_steps):
    """xps_ctc_beam_state_bytes, restated."""
    return 0 if B < 1 or K < 1 or max_steps < 1 else B * state_stride(K, max_steps)


def _field_offsets(K):
    off, out = HEADER_BYTES, {}
    for name, dt in MEMBER_FIELDS:
        out[name] = (off, np.dtype(dt))
        off += K * np.dtype(dt).itemsize
    return out


def unpack_state(block, K, max_steps):
    """One stream block (state_stride bytes, uint8 array or bytes) -> (header int32[4], {field: array[K]}, hist int32[max_steps][K]).
    The arrays are copies."""
    block = np.frombuffer(bytes(block), np.uint8) if not isinstance(block, np.ndarray) else np.ascontiguousarray(block, np.uint8)
    if block.size != state_stride(K, max_steps):
        raise ValueError(f'a stream block of K = {K}, max_steps = {max_steps} has {state_stride(K, max_steps)} bytes, not {block.size}')
    raw = block.tobytes()
    header = np.frombuffer(raw, np.int32, 4, 0).copy()
    members = {name: np.frombuffer(raw, dt, K, off).copy() for name, (off, dt) in _field_offsets(K).items()}
    hist = np.frombuffer(raw, np.int32, max_steps * K, HEADER_BYTES + set_bytes(K)).reshape(max_steps, K).copy()
    return header, members, hist


def pack_state(header, members, hist, K, max_steps):
    """The inverse of unpack_state: a block of state_stride bytes (uint8 array), zero wherever the layout holds nothing."""
    block = np.zeros(state_stride(K, max_steps), np.uint8)
    block[:16] = np.asarray(header, np.int32).reshape(4).view(np.uint8)
    for name, (off, dt) in _field_offsets(K).items():
        a = np.ascontiguousarray(members[name], dt).reshape(K)
        block[off:off + a.nbytes] = a.view(np.uint8)
    h = np.ascontiguousarray(hist, np.int32).reshape(max_steps, K)
    off = HEADER_BYTES + set_bytes(K)
    block[off:off + h.nbytes] = h.reshape(-1).view(np.uint8)
    return block


def canonical(block, K, max_steps):
    """The block with everything the layout leaves unspecified set to zero (member slots at rank >= n_members, the padding of
    the member set): two blocks hold the same state when their canonical forms are equal bytes."""
    header, members, hist = unpack_state(block, K, max_steps)
    n = int(header[1]) if header[0] > 0 else 0
    for a in members.values():
        a[n:] = 0
    return pack_state(header, members, hist, K, max_steps)


def split_entry(e):
    """A backpointer -> (member of the previous frame, appended token or -1)."""
    e = int(e)
    return e & 0xffff, (e >> 16) - 1


def member_prefix(hist, t, r):
    """The prefix of rank r after frame t (0-based), walked back through hist[t], hist[t - 1], .. as the readout walks."""
    out = []
    for u in range(t, -1, -1):
        r, tok = split_entry(hist[u][r])
        if tok >= 0:
            out.append(tok)
    return tuple(reversed(out))


def frame_prefixes(hist, counts):
    """Prefixes of every written rank of every frame, built forwards: prefixes[t][r] for r < counts[t].  Raises when a
    backpointer names a member the previous frame does not have."""
    prev, out = [()], []
    for t, n in enumerate(counts):
        cur = []
        for r in range(int(n)):
            k, tok = split_entry(hist[t][r])
            if not 0 <= k < len(prev):
                raise ValueError(f'frame {t} rank {r}: backpointer to member {k} of {len(prev)}')
            cur.append(prev[k] + ((tok,) if tok >= 0 else ()))
        out.append(cur)
        prev = cur
    return out


def unpack_workspace(ws, sentinel):
    """The offline kernel's workspace int32[B][T][K], pre-filled with `sentinel` (a value no backpointer can equal: a
    backpointer is below 65 << 16) -> per sequence (counts[T], prefixes, stray): counts[t] = the leading slots of frame t that
    were written, prefixes[t][r] the prefix of every one of them (frames after the first unwritten one: none), stray = slots
    written behind an unwritten one, in a frame or after an unwritten frame.  A sound workspace has stray == 0."""
    ws = np.asarray(ws)
    out = []
    for seq in ws:
        written = seq != np.int32(sentinel)
        counts = np.where(written.all(1), seq.shape[1], written.argmin(1))
        live = np.cumprod(counts > 0) if len(counts) else counts           # frames before the first unwritten one
        stray = int(written.sum() - (counts * live).sum())
        counts = counts * live
        out.append((counts, frame_prefixes(seq, counts), stray))
    return out


def prefix_hash(prefix, base):
    h = 0
    for tok in prefix:
        h = (h * base + tok + 1) % HMOD
    return h


def expected_members(frame):
    """The member arrays the kernel must hold for one frame of a beam_trace: {field: list} over the ranks; parent = the rank of
    prefix[:-1] or -1, cmask bit s set exactly when prefix + (s,) is a member, the two prefix hashes of DESIGN.md 4.8."""
    index = {P: r for r, (P, _, _) in enumerate(frame)}
    out = {name: [] for name, _ in MEMBER_FIELDS}
    for P, pb, pnb in frame:
        out['p_b'].append(pb)
        out['p_nb'].append(pnb)
        out['h1'].append(prefix_hash(P, HBASE1))
        out['h2'].append(prefix_hash(P, HBASE2))
        out['hp1'].append(prefix_hash(P[:-1], HBASE1))
        out['hp2'].append(prefix_hash(P[:-1], HBASE2))
        out['cmask'].append(sum(1 << Q[-1] for Q in index if len(Q) == len(P) + 1 and Q[:-1] == P))
        out['len'].append(len(P))
        out['last'].append(P[-1] if P else -1)
        out['parent'].append(index.get(P[:-1], -1) if P else -1)
    return out


# ---- the checks of tests/test_gpu_ctc_beam_trace.py; here so that tests/test_ctc_beam_host.py can show on states built from
# ---- the restatement that they accept the right state and refuse a wrong one
def check_block(block, ref, t, K, max_steps, what):
    """The state of one stream after frame t, which started as zeros, against the restatement's frames ref[0 .. t]."""
    from ctc_beam_ref import frame_diff
    block = np.asarray(block, np.uint8)
    header, members, hist = unpack_state(block, K, max_steps)
    frame, n = ref[t], len(ref[t])
    assert header.tolist() == [t + 1, n, 0, 0], (what, header)
    got = [(member_prefix(hist, t, r), float(members['p_b'][r]), float(members['p_nb'][r])) for r in range(n)]
    assert frame_diff(frame, got) is None, (what, frame_diff(frame, got))
    exp = expected_members(frame)
    for name, dt in MEMBER_FIELDS[2:]:                                        # everything but the scores: equal
        assert np.array_equal(members[name][:n], np.array(exp[name], dtype=dt)), (what, name)
    for u in range(t + 1):                                                    # backpointers: the members' slots and nothing else
        assert not hist[u, len(ref[u]):].any(), (what, 'hist behind the members of frame', u)
        prev = 1 if u == 0 else len(ref[u - 1])
        assert ((hist[u, :len(ref[u])] & 0xffff) < prev).all() and ((hist[u, :len(ref[u])] >> 16) <= 64).all(), (what, u)
    assert not hist[t + 1:].any(), (what, 'hist of frames not run')
    assert not block[16:HEADER_BYTES].any() and not block[HEADER_BYTES + set_bytes(K) + 4 * max_steps * K:].any(), (what, 'padding')


def check_offline(prefix, plen, nll, ws, refs, held, sentinel, what):
    """The outputs of one xps_ctc_beam_f64 launch (prefix [B][T], len [B], nll [B], the workspace int32 [B][T][K] that started
    as `sentinel`) against refs[b] = the restatement's frames of sequence b, as many as its clamped length.  held: the leading
    frames in which the prefixes are compared (ctc_beam_cases.frames_held); the member counts are compared in all of them."""
    from ctc_beam_ref import NEG_INF, close, lse
    T = ws.shape[1]
    for b, (ref, (counts, prefixes, stray)) in enumerate(zip(refs, unpack_workspace(ws, sentinel))):
        n = len(ref)
        assert stray == 0, (what, b, 'workspace written behind the members or after the last frame')
        assert counts.tolist() == [len(f) for f in ref] + [0] * (T - n), (what, b)
        for t in range(min(n, held)):
            assert prefixes[t] == [m[0] for m in ref[t]], (what, b, 'frame', t)
        if n <= held:
            P, pb, pnb = ref[-1][0] if n else ((), 0.0, NEG_INF)
            assert prefix[b].tolist() == list(P) + [-1] * (T - len(P)), (what, b)
            assert plen[b] == len(P), (what, b)
            assert close(float(nll[b]), -lse(pb, pnb)), (what, b, float(nll[b]), -lse(pb, pnb))
        if n == 0:
            assert plen[b] == 0 and str(float(nll[b])) == '-0.0' and (prefix[b] == -1).all(), (what, b)
