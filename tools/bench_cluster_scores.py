"""Cluster separability benchmark: alignment.metrics.cluster_scores -- one Gram matrix, every score of every
label set a label-grouped sum over it -- beside the loop of sklearn calls the reference's figure analyses make
(silhouette_samples and its positive mean, calinski_harabasz_score, davies_bouldin_score, once per label vector, each call
recomputing what it needs from the data), in the same process on the same data.

Data: utils.synthetic.make_patient, a target of 150 trials plus 3 pooled patients of 150 trials, T = 20 samples, the channels
reduced by the device PCA of the target at n_components = 0.95 (every patient through the target's components: the notebooks'
unaligned pooled space; the scores' cost does not depend on what the latent space means), flattened to T * d features, float32;
labels: the first phoneme (9 classes).  R = 0 (the labels alone) and R = 200 shuffles drawn from RandomState(0) -- the sklearn
loop scores the very same label vectors.  A run is timed by the host clock with a device synchronise on both sides; `--warmup`
untimed runs, then the median and minimum of `--runs`.  The sklearn loop at R = 200 takes ~10 s per run: it gets
`--comparator-runs` timed runs after one warm-up, and the JSON line says how many.  Progress goes to stderr.

    python tools/bench_cluster_scores.py [--runs 10] [--warmup 2] [--comparator-runs 3] [--shuffles 200]     prints one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from sklearn import metrics as SK

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cross_patient_speech_decoding_amd.alignment import PCA, cluster_scores             # noqa: E402
from cross_patient_speech_decoding_amd.utils.synthetic import make_patient              # noqa: E402


def pooled_latents(trials, pooled, T, C):
    pats = [make_patient(p, trials, T=T, C=C) for p in range(1 + pooled)]
    pca = PCA(n_components=0.95).fit(pats[0][0].reshape(-1, C))
    X = np.concatenate([pca.transform(x) for x, _ in pats]).astype(np.float32)
    y = np.concatenate([yy[:, 0] for _, yy in pats])
    return X.reshape(len(X), -1), y, int(pca.n_components_)


def sklearn_loop(X, label_sets):
    out = np.empty((len(label_sets), 4))
    for r, y in enumerate(label_sets):
        s = SK.silhouette_samples(X, y)
        out[r] = [s.mean(), np.mean(s[np.where(s > 0)]), SK.calinski_harabasz_score(X, y), SK.davies_bouldin_score(X, y)]
    return out


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
    ap.add_argument('--comparator-runs', type=int, default=3, help='timed runs of the sklearn loop at R = --shuffles (one warm-up)')
    ap.add_argument('--shuffles', type=int, default=200)
    ap.add_argument('--trials', type=int, default=150)
    ap.add_argument('--pooled', type=int, default=3)
    ap.add_argument('--channels', type=int, default=256)
    args = ap.parse_args()
    if args.runs < 10 or args.warmup < 2 or args.comparator_runs < 1:
        ap.error('--runs must be at least 10, --warmup at least 2 and --comparator-runs at least 1')
    X, y, d = pooled_latents(args.trials, args.pooled, 20, args.channels)
    X64 = X.astype(np.float64)
    out = {'bench': 'cluster_scores', 'device': torch.cuda.get_device_name(0), 'shape': list(X.shape), 'dtype': str(X.dtype),
           'T': 20, 'd': d, 'n_classes': int(len(np.unique(y))), 'runs': args.runs, 'warmup': args.warmup,
           'timed': 'one call for all label sets, host clock with a device synchronise on both sides, median (min)'}
    for R in (0, args.shuffles):
        def device():
            return cluster_scores(X, y, n_shuffles=R, random_state=0)
        for i in range(args.warmup):
            _, cs = timed(device, f'R={R} device, warm-up')
        t_d = [timed(device, f'R={R} device, run {i}')[0] for i in range(args.runs)]
        c_runs = args.runs if R == 0 else args.comparator_runs
        timed(lambda: sklearn_loop(X64, cs.labels_), f'R={R} sklearn loop, warm-up')
        host = [timed(lambda: sklearn_loop(X64, cs.labels_), f'R={R} sklearn loop, run {i}') for i in range(c_runs)]
        t_h, ref = [h[0] for h in host], host[-1][1]
        got = np.stack([cs.silhouette_, cs.silhouette_pos_, cs.calinski_harabasz_, cs.davies_bouldin_], axis=1)
        med_d, med_h = statistics.median(t_d), statistics.median(t_h)
        out[f'R{R}'] = {'label_sets': R + 1, 'device_ms': round(med_d, 3), 'device_min_ms': round(min(t_d), 3),
                        'sklearn_loop_ms': round(med_h, 3), 'sklearn_loop_min_ms': round(min(t_h), 3), 'sklearn_loop_runs': c_runs,
                        'ratio': round(med_h / med_d, 2), 'device_not_slower': bool(med_d <= med_h),
                        'max_rel_diff_to_sklearn': float(np.nanmax(np.abs(got - ref) / np.abs(ref))),
                        'p_values': {k: round(v, 5) for k, v in cs.p_value_.items()}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
