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
next beam is the first beam_size candidates by lse(p_b', p_nb') descending, ties by insertion order."""
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


def beam_search(lp, beam_size=100, blank=0, lse=lse):
    """lp: (T, S) log-probs (rows of floats) -> (prefix tuple, nll)."""
    beam = [((), 0.0, NEG_INF)]
    for row in lp:
        row = [float(v) for v in row]
        index = {p: k for k, (p, _, _) in enumerate(beam)}
        cands = []                                     # (insertion key, prefix, p_b, p_nb)
        for k, (P, pb, pnb) in enumerate(beam):
            last = P[-1] if P else None
            b = lse(NEG_INF, pb + row[blank], pnb + row[blank])
            contrib = [((blank, k, 0), None)]
            if P:
                contrib.append(((last, k, 1), (pnb + row[last],)))
                j = index.get(P[:-1])
                if j is not None:
                    _, pbj, pnbj = beam[j]
                    q = row[last]
                    args = (pbj + q,) if (beam[j][0][-1:] == (last,)) else (pbj + q, pnbj + q)
                    contrib.append(((last, j, 0), args))
            contrib.sort(key=lambda c: c[0])
            nb = NEG_INF
            for _, args in contrib:
                if args is not None:
                    nb = lse(nb, *args)
            cands.append((contrib[0][0], P, b, nb))
            for s in range(len(row)):
                if s == blank or P + (s,) in index:
                    continue
                q = row[s]
                nb = lse(NEG_INF, pb + q) if s == last else lse(NEG_INF, pb + q, pnb + q)
                cands.append(((s, k, 0), P + (s,), NEG_INF, nb))
        cands.sort(key=lambda c: c[0])                 # insertion order, then a stable sort by score
        cands = sorted(cands, key=lambda c: lse(c[2], c[3]), reverse=True)[:beam_size]
        beam = [(P, b, nb) for _, P, b, nb in cands]
    P, pb, pnb = beam[0]
    return P, -lse(pb, pnb)
