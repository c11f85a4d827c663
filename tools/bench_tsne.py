"""Exact t-SNE benchmark: manifold.TSNE with default arguments -- one fit at n = 150, 600 and 1200 trials and one
batch of 16 data sets of n = 150 as ONE device problem -- beside sklearn.manifold.TSNE with method='exact' and with its default
method='barnes_hut' on the host's threads, in the same process on the same data.

Data: 9 Gaussian class blobs in D = 50 features (the shape of the notebooks' flattened PCA latents), float64, fixed seeds; both
sides start from the same PCA init.  A run is timed by the host clock with a device synchronise on both sides; `--warmup`
untimed runs, then the median and minimum of `--runs`.  sklearn's exact fit takes ~1 s at n = 150 and tens of seconds at
n = 1200: each comparator gets `--comparator-runs` timed runs, and the JSON line says how many.  Also reported: the fit's time per
descent launch (the whole fit over max_iter + 2 launches; rocprofv3 --kernel-trace gives the kernel's own time), and the batch's
time over 16 single fits -- below 1 / 16-th of them per data set means the single fit leaves the device idle between launches.
Progress goes to stderr.

    python tools/bench_tsne.py [--runs 10] [--warmup 2] [--comparator-runs 1] [--sizes 150 600 1200] [--batch 16]    one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from sklearn.manifold import TSNE as SkTSNE

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cross_patient_speech_decoding_amd.manifold import TSNE                              # noqa: E402


def blobs(n, seed, D=50, k=9):
    rng = np.random.default_rng(seed)
    codes = rng.permutation(np.arange(n) % k)
    return rng.standard_normal((k, D))[codes] + rng.standard_normal((n, D))


def pca_init(X):
    Xc = X - X.mean(axis=0)
    _, _, Vt = np.linalg.svd(Xc, full_matrices=False)
    Y = (Xc @ Vt[:2].T).astype(np.float32)
    return (Y / np.std(Y[:, 0]) * 1e-4).astype(np.float64)


def timed(fn, what):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    print(f'{what}: {ms:.1f} ms', file=sys.stderr, flush=True)
    return ms, res


def stats(ms):
    return {'ms': round(statistics.median(ms), 3), 'min_ms': round(min(ms), 3), 'runs': len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--comparator-runs', type=int, default=1, help='timed runs of each sklearn fit (no warm-up: nothing is compiled)')
    ap.add_argument('--sizes', type=int, nargs='+', default=[150, 600, 1200])
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--no-comparators', action='store_true')
    args = ap.parse_args()
    if args.runs < 3 or args.warmup < 1 or args.comparator_runs < 1:
        ap.error('--runs must be at least 3, --warmup and --comparator-runs at least 1')
    out = {'bench': 'tsne', 'device': torch.cuda.get_device_name(0), 'features': 50, 'max_iter': 1000, 'perplexity': 30.0,
           'host_threads': os.cpu_count() if 'OMP_NUM_THREADS' not in os.environ else int(os.environ['OMP_NUM_THREADS']),
           'timed': 'one fit, host clock with a device synchronise on both sides, median (min)'}

    def device_fit(Xs, inits):
        ts = TSNE()
        ts.fit_transform_many(Xs, inits=inits)
        return ts

    def host_fit(Xs, inits, method):
        return [SkTSNE(method=method, init=y).fit(X) for X, y in zip(Xs, inits)]

    def compare(key, Xs):
        inits = [pca_init(X) for X in Xs]
        for i in range(args.warmup):
            timed(lambda: device_fit(Xs, inits), f'{key} device, warm-up')
        runs = [timed(lambda: device_fit(Xs, inits), f'{key} device, run {i}') for i in range(args.runs)]
        ts = runs[-1][1]
        res = {'n': len(Xs[0]), 'data_sets': len(Xs), 'device': stats([r[0] for r in runs]),
               'device_kl': [round(v, 5) for v in ts.kl_divergences_[:4]], 'device_n_iter': ts.n_iters_[:4]}
        res['device_us_per_launch'] = round(res['device']['ms'] * 1e3 / (max(ts.n_iters_) + 3), 2)
        if not args.no_comparators:
            for method in ('exact', 'barnes_hut'):
                host = [timed(lambda: host_fit(Xs, inits, method), f'{key} sklearn {method}, run {i}') for i in range(args.comparator_runs)]
                res[f'sklearn_{method}'] = stats([h[0] for h in host])
                res[f'sklearn_{method}_kl'] = [round(float(f.kl_divergence_), 5) for f in host[-1][1][:4]]
                res[f'sklearn_{method}_over_device'] = round(res[f'sklearn_{method}']['ms'] / res['device']['ms'], 2)
        out[key] = res
        return res

    single = {}
    for n in args.sizes:
        single[n] = compare(f'n{n}', [blobs(n, 1000 + n)])
    if args.batch > 1:
        n = args.sizes[0]
        res = compare(f'batch{args.batch}_n{n}', [blobs(n, 2000 + i) for i in range(args.batch)])
        res['over_one_fit'] = round(res['device']['ms'] / single[n]['device']['ms'], 3)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
