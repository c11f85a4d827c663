"""Tensor maximum entropy surrogate benchmark: surrogates.TME on one (trials, T, channels) = (150, 200, 128)
float64 tensor -- the fit (centring, one ragged Gram launch for the three Sigma_r, the batched eigendecomposition, the Newton
iteration with one ragged pass per evaluation) and the sampling of S = 64 surrogates (one draw and one scaling launch, three
batched mode products per chunk, the mean tensor added in the last one's epilogue).

Data: utils.synthetic.make_patient(0, trials, T, C): smooth latent trajectories mixed into the channels plus noise, so the three
spectra decay as a patient's do.  A run is timed by the host clock with a device synchronise on both sides; `--warmup` untimed
runs, then the median and minimum of `--runs`.  The sampling is timed with a fixed seed and checked to give the same bits in
every run.  Progress goes to stderr.

    python tools/bench_tme.py [--runs 10] [--warmup 2] [--surrogates 64]     prints one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cross_patient_speech_decoding_amd.surrogates import TME                             # noqa: E402
from cross_patient_speech_decoding_amd.utils.synthetic import make_patient              # noqa: E402


def timed(fn, what):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    print(f'{what}: {ms:.1f} ms', file=sys.stderr, flush=True)
    return ms, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--surrogates', type=int, default=64)
    ap.add_argument('--trials', type=int, default=150)
    ap.add_argument('--T', type=int, default=200)
    ap.add_argument('--channels', type=int, default=128)
    ap.add_argument('--max-bytes', type=int, default=2 ** 30)
    args = ap.parse_args()
    if args.runs < 3 or args.warmup < 1:
        ap.error('--runs must be at least 3 and --warmup at least 1')
    x, _ = make_patient(0, args.trials, T=args.T, C=args.channels)
    X = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    for i in range(args.warmup):
        timed(lambda: TME().fit(X), 'fit, warm-up')
    fits = [timed(lambda: TME().fit(X), f'fit, run {i}') for i in range(args.runs)]
    model = fits[-1][1]
    S = args.surrogates

    def sample():
        return model.sample(S, random_state=0, max_bytes=args.max_bytes)
    for i in range(args.warmup):
        timed(sample, 'sample, warm-up')
    t_s, first, same = [], None, True
    for i in range(args.runs):                                           # (one result is kept: a draw is 2 GB)
        ms, res = timed(sample, f'sample, run {i}')
        t_s.append(ms)
        if first is None:
            first = res
        else:
            same = same and torch.equal(res, first)
        del res
    t_f = [f[0] for f in fits]
    n0, n1, n2 = model.shape_
    k0, k1, k2 = model.kept_
    flops = 2.0 * S * (k0 * k1 * k2 * n2 + k0 * k1 * n1 * n2 + k0 * n0 * n1 * n2)
    out = {'bench': 'tme', 'device': torch.cuda.get_device_name(0), 'shape': list(model.shape_), 'kept': list(model.kept_),
           'dtype': 'float64', 'runs': args.runs, 'warmup': args.warmup,
           'timed': 'host clock with a device synchronise on both sides, median (min)',
           'fit_ms': round(statistics.median(t_f), 3), 'fit_min_ms': round(min(t_f), 3), 'newton_launches': int(model.n_iter_),
           'residual': float(model.residual_), 'surrogates': S, 'sample_ms': round(statistics.median(t_s), 3),
           'sample_min_ms': round(min(t_s), 3), 'sample_ms_per_surrogate': round(statistics.median(t_s) / S, 4),
           'mode_product_tflops': round(flops / (statistics.median(t_s) * 1e-3) / 1e12, 3),
           'same_bits_every_run': bool(same)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
