"""Generate tests/golden/ctc_beam.npz from the REFERENCE's realtime_sim/ctc_decoder.py decode (prefix beam search).
Build container only (numpy + torch).  About 40 cases: random and peaked posteriors, rows with exact zeros, uniform rows,
blank != 0, beam 1 / 2 / 16 / 100, T 0..47, S 2..11.  A case is kept only if decode gives the same prefix with its
logsumexp evaluated in float64 and in np.longdouble: ties that rest on one last-bit rounding (which another exp / log
could flip) are dropped.  Case i: probs_i (T, S) float64, blank_i, beam_i, prefix_i (int64), nll_i."""
import os
import sys

import numpy as np

sys.path.insert(0, '/root/reference/aligned_decoding')
import realtime_sim.ctc_decoder as ref      # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def _lse_long(*args):
    if all(a == ref.NEG_INF for a in args):
        return ref.NEG_INF
    a = [np.longdouble(v) for v in args]
    m = max(a)
    return m + np.log(sum(np.exp(v - m) for v in a))


def _decode_long(probs, beam, blank):
    f64 = ref.logsumexp
    ref.logsumexp = _lse_long
    try:
        return ref.decode(probs, beam, blank)[0]
    finally:
        ref.logsumexp = f64


def _probs(rng, kind, T, S):
    if kind == 'uniform':
        return np.full((T, S), 1.0 / S)
    if kind == 'peaked':                                  # softmax of scaled Gaussian logits: a trained model's look
        z = rng.standard_normal((T, S)) * 3.0
        e = np.exp(z - z.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)
    p = rng.random((T, S))
    if kind == 'zeros':
        p[rng.random((T, S)) < 0.35] = 0.0
        p[:, 0] = np.where(p.sum(1) == 0, 1.0, p[:, 0])
    if kind == 'mixed' and T:                             # some uniform rows between random ones
        p[rng.random(T) < 0.3] = 1.0
    return p / p.sum(1, keepdims=True)


def main():
    rng = np.random.default_rng(2024)
    specs = []
    for T in (0, 1, 2, 5):
        specs.append(('random', T, 4, 2, 0))
    for beam in (1, 2, 16, 100):
        for kind in ('random', 'peaked', 'zeros'):
            specs.append((kind, 47, 11, beam, 0))
    for beam in (1, 2, 16, 100):
        specs.append(('uniform', int(rng.integers(3, 20)), int(rng.integers(2, 6)), beam, 0))
        specs.append(('mixed', 30, 8, beam, 3))
        specs.append(('random', 23, 5, beam, 4))
    for S in (2, 3, 5, 8, 11):
        specs.append(('peaked', 40, S, 100, S - 1))
        specs.append(('zeros', 12, S, 16, S // 2))
    out, kept, dropped = {}, 0, 0
    with np.errstate(divide='ignore'):
        for kind, T, S, beam, blank in specs:
            probs = _probs(rng, kind, T, S)
            prefix, nll = ref.decode(probs, beam, blank)
            if _decode_long(probs, beam, blank) != prefix:
                dropped += 1
                continue
            out[f'probs_{kept}'] = probs
            out[f'blank_{kept}'] = np.int64(blank)
            out[f'beam_{kept}'] = np.int64(beam)
            out[f'prefix_{kept}'] = np.asarray(prefix, dtype=np.int64)
            out[f'nll_{kept}'] = np.float64(nll)
            out[f'kind_{kept}'] = np.array(kind)
            kept += 1
    out['n_cases'] = np.int64(kept)
    path = os.path.join(HERE, 'ctc_beam.npz')
    np.savez_compressed(path, **out)
    print(f'{path}: {kept} cases ({dropped} dropped as rounding-dependent), {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
