"""Fold-batched alignment benchmark: ``process_aligner_folds`` (one alignment.fit_folds for every fold) beside a
loop of ``process_aligner`` over the same splits -- what the data modules did before -- in the same process on the same data, in
interleaved runs.

Shape: the reference's training notebook.  Target (144, 200, 111); pooled patients of 111, 63, 149, 74, 144, 171, 201 channels
(144 + 3 p trials each); 20 KFold splits; PCA keeps 0.95 of the variance; inputs are host float32 arrays for both routes, as the
data modules hold them.  A run is the whole setup of all folds, timed by the host clock with a device synchronise on both
sides; `warmup` untimed runs of each route, then the median of `runs` runs.  Calls into libxps.so are counted for one run of
each route (every enqueueing entry point goes through alignment._linalg.call).

    python tools/bench_fold_align.py [--runs 10] [--warmup 2] [--folds 20]        prints one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from sklearn.model_selection import KFold

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cross_patient_speech_decoding_amd.alignment import AlignCCA, _linalg                                   # noqa: E402
from cross_patient_speech_decoding_amd.nn_models.data_utils.datamodules import process_aligner, process_aligner_folds  # noqa: E402
from cross_patient_speech_decoding_amd.utils.synthetic import make_patient                                  # noqa: E402

POOL_CHANNELS = (111, 63, 149, 74, 144, 171, 201)


def batched(X, y, pool, splits):
    return process_aligner_folds(X, y, y, pool, splits)


def per_fold(X, y, pool, splits):
    return [process_aligner(X[tr], y[tr], y[tr], pool, AlignCCA) for tr, _ in splits]


def run(route, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = route(*args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def count_calls(route, *args):
    counts, real = {}, _linalg.call

    def counting(name, *a):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *a)
    _linalg.call = counting
    try:
        route(*args)
    finally:
        _linalg.call = real
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--folds', type=int, default=20)
    ap.add_argument('--trials', type=int, default=144)
    ap.add_argument('--T', type=int, default=200)
    args = ap.parse_args()
    X, y = make_patient(0, args.trials, T=args.T, C=111)
    pool = []
    for p, c in enumerate(POOL_CHANNELS, start=1):
        x, yy = make_patient(p, args.trials + 3 * p, T=args.T, C=c)
        pool.append((x, yy, yy))
    splits = list(KFold(args.folds, shuffle=True, random_state=0).split(X))
    a = (X, y, pool, splits)
    for _ in range(args.warmup):
        run(batched, *a)
        run(per_fold, *a)
    t_b, t_p = [], []
    for _ in range(args.runs):                               # interleaved: both routes see the same state of the machine
        tb, out_b = run(batched, *a)
        tp, out_p = run(per_fold, *a)
        t_b.append(tb)
        t_p.append(tp)
    same_k = all(b[0].shape == q[0].shape for b, q in zip(out_b, out_p))
    diff = max(float((b[0].cpu() - q[0]).abs().max() / q[0].abs().max()) for b, q in zip(out_b, out_p)) if same_k else None
    cb, cp = count_calls(batched, *a), count_calls(per_fold, *a)
    med_b, med_p = statistics.median(t_b), statistics.median(t_p)
    print(json.dumps({'bench': 'fold_align', 'device': torch.cuda.get_device_name(0), 'target': list(X.shape),
                      'pool_channels': list(POOL_CHANNELS), 'folds': args.folds, 'runs': args.runs, 'warmup': args.warmup,
                      'timed': 'setup of all folds, host clock, median',
                      'batched_ms': round(med_b, 2), 'batched_min_ms': round(min(t_b), 2),
                      'per_fold_ms': round(med_p, 2), 'per_fold_min_ms': round(min(t_p), 2), 'ratio': round(med_p / med_b, 2),
                      'same_component_counts': bool(same_k), 'max_rel_diff_pooled': diff,
                      'libxps_calls_batched': sum(cb.values()), 'libxps_calls_per_fold': sum(cp.values()),
                      'libxps_calls_batched_by_name': cb}))


if __name__ == '__main__':
    main()
