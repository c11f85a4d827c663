"""CPU restatement of the CTC prefix beam search (realtime_sim/ctc_decoder.py: decode) as candidates per time step, the
form the HIP kernel (csrc/xps_ctc_beam.hip) computes.  Plain Python floats; `lse` may be swapped for a wider type.

For beam member k (prefix P_k, scores p_b, p_nb) and a frame of log-probs lp:
  unchanged P_k:   p_b' = lse(-inf, p_b + lp[blank], p_nb + lp[blank])
                   p_nb' = -inf, folded with lse(acc, *args) over (key order):
                       self-merge (p_nb + lp[last],)                     key (last, k, 1)   if P_k is not empty
                       extension of member j with P_j == P_k[:-1]        key (last, j, 0)
                           args (p_b_j + p,) if last(P_j) == last(P_k) else (p_b_j + p, p_nb_j + p)
  extension P_k + (s,), s != blank, unless that prefix is a member:
                   p_b' = -inf, p_nb' = lse(-inf, p_b + lp[s]) if s == last(P_k) else lse(-inf, p_b + lp[s], p_nb + lp[s])
                   key (s, k, 0)
A candidate's insertion order is the smallest key of its contributions (the unchanged one also has (blank, k, 0)); the
next beam is the first beam_size candidates by lse(p_b', p_nb') descending, ties by insertion order.

beam_trace returns the whole search, every member after every frame; beam_search is its first member after the last frame."""
import math

NEG_INF = -math.inf


def lse(*a):
    if all(v == NEG_INF for v in a):
        return NEG_INF
    m = max(a)
    s = 0.0
    for v in a:
        s += math.exp(v - m)
    return m + math.log(s)


RULES = ('tie_high', 'parent_both', 'no_self', 'repeat_both', 'blank_key', 'no_member_check')


def beam_trace(lp, beam_size=100, blank=0, lse=lse, rule=None):
    """lp: (T, S) log-probs -> for every frame the beam in rank order, a list of (prefix tuple, p_b, p_nb).

    rule = None is the search.  A name from RULES breaks one rule of it on purpose; these variants exist only to show that a
    test input tells the right rule from the wrong one (tests/test_ctc_beam_host.py: the discrimination table):
      'tie_high'         equal scores go to the LATER insertion key
      'parent_both'      the parent member always contributes p_b and p_nb, also when it ends in the same token
      'no_self'          the self-merge (last, k, 1) is dropped
      'repeat_both'      an extension by the member's own last token also takes p_nb
      'blank_key'        the unchanged candidate's key is always (blank, k, 0), not the smallest of its contributions
      'no_member_check'  extensions that are already members are not skipped"""
    if rule is not None and rule not in RULES:
        raise ValueError(f'rule {rule!r} is not one of {RULES}')
    beam = [((), 0.0, NEG_INF)]
    trace = []
    for row in lp:
        row = [float(v) for v in row]
        index = {p: k for k, (p, _, _) in enumerate(beam)}
        cands = []                                     # (insertion key, prefix, p_b, p_nb)
        for k, (P, pb, pnb) in enumerate(beam):
            last = P[-1] if P else None
            b = lse(NEG_INF, pb + row[blank], pnb + row[blank])
            contrib = [((blank, k, 0), None)]
            if P:
                if rule != 'no_self':
                    contrib.append(((last, k, 1), (pnb + row[last],)))
                j = index.get(P[:-1])
                if j is not None:
                    _, pbj, pnbj = beam[j]
                    q = row[last]
                    only_pb = beam[j][0][-1:] == (last,) and rule != 'parent_both'
                    contrib.append(((last, j, 0), (pbj + q,) if only_pb else (pbj + q, pnbj + q)))
            contrib.sort(key=lambda c: c[0])
            nb = NEG_INF
            for _, args in contrib:
                if args is not None:
                    nb = lse(nb, *args)
            cands.append(((blank, k, 0) if rule == 'blank_key' else contrib[0][0], P, b, nb))
            for s in range(len(row)):
                if s == blank or (P + (s,) in index and rule != 'no_member_check'):
                    continue
                q = row[s]
                own = s == last and rule != 'repeat_both'
                nb = lse(NEG_INF, pb + q) if own else lse(NEG_INF, pb + q, pnb + q)
                cands.append(((s, k, 0), P + (s,), NEG_INF, nb))
        cands.sort(key=lambda c: c[0], reverse=rule == 'tie_high')   # insertion order, then a stable sort by score
        cands = sorted(cands, key=lambda c: lse(c[2], c[3]), reverse=True)[:beam_size]
        beam = [(P, b, nb) for _, P, b, nb in cands]
        trace.append(beam)
    return trace


def beam_search(lp, beam_size=100, blank=0, lse=lse):
    """lp: (T, S) log-probs (rows of floats) -> (prefix tuple, nll): the first member after the last frame."""
    trace = beam_trace(lp, beam_size, blank, lse=lse)
    P, pb, pnb = trace[-1][0] if trace else ((), 0.0, NEG_INF)
    return P, -lse(pb, pnb)


def lse_longdouble(*a):
    """lse with the same left-to-right sum carried in numpy.longdouble and rounded to double once, at the end."""
    import numpy as np
    if all(v == NEG_INF for v in a):
        return NEG_INF
    m = np.longdouble(max(a))
    s = np.longdouble(0.0)
    for v in a:
        s += np.exp(np.longdouble(v) - m)
    return float(m + np.log(s))


def trace_is_robust(lp, beam_size, blank):
    """True when the search carried in double and the one carried in long double (lse_longdouble) hold the same prefixes in
    the same order after every frame.  Then no decision of the search hangs on the last bit of an exp or a log, and a device
    libm that differs from the host's there must still produce this beam.  Ties between equal operands through equal
    operations survive the change of precision; coincidental ties and near-ties do not.  Needs a long double wider than
    double (f64_ref.have_long_double)."""
    from f64_ref import LONG_DOUBLE_REASON, have_long_double
    if not have_long_double():
        raise RuntimeError(LONG_DOUBLE_REASON)
    a = beam_trace(lp, beam_size, blank)
    b = beam_trace(lp, beam_size, blank, lse=lse_longdouble)
    return all([m[0] for m in fa] == [m[0] for m in fb] for fa, fb in zip(a, b))


# ---- the comparison of the GPU tests (tests/test_gpu_ctc_beam_trace.py), also used on the host to show what it can tell apart
def close(got, ref, tol=1e-12):
    """A score against the restatement's: -inf where that has -inf, else |got - ref| <= tol * max(1, |ref|)."""
    if ref == NEG_INF:
        return got == NEG_INF
    return bool(abs(got - ref) <= tol * max(1.0, abs(ref)))      # False for a NaN


def frame_diff(ref, got, scores=True):
    """None when the beam `got` of one frame equals the restatement's `ref`: as many members, the same prefixes in the same
    order and, with scores, every p_b and p_nb close().  Else a line that says where they differ."""
    if len(got) != len(ref):
        return f'{len(got)} members, reference {len(ref)}'
    for r, ((P, pb, pnb), (Q, qb, qnb)) in enumerate(zip(ref, got)):
        if P != Q:
            return f'rank {r}: prefix {Q}, reference {P}'
        if scores and not (close(qb, pb) and close(qnb, pnb)):
            return f'rank {r} {P}: (p_b, p_nb) = ({qb!r}, {qnb!r}), reference ({pb!r}, {pnb!r})'
    return None


def trace_diff(ref, got, scores='all'):
    """None or the first difference of two traces.  scores = 'all': what the streaming test sees (every member's scores after
    every frame); 'first': what the offline test sees (every prefix after every frame, the nll of the first member after the
    last one)."""
    if len(ref) != len(got):
        return f'{len(got)} frames, reference {len(ref)}'
    for t, (fr, fg) in enumerate(zip(ref, got)):
        d = frame_diff(fr, fg, scores == 'all')
        if d:
            return f'frame {t}: {d}'
    if scores == 'first' and ref:
        (_, pb, pnb), (_, qb, qnb) = ref[-1][0], got[-1][0]
        if not close(-lse(qb, qnb), -lse(pb, pnb)):
            return f'nll {-lse(qb, qnb)!r}, reference {-lse(pb, pnb)!r}'
    return None
