"""SVC grid-search benchmark: the fused search (decoders.SVCSearchCV) beside sklearn's
GridSearchCV(decoders.SVC(...), n_jobs=None) -- the route a user had before the fused search existed -- in the same process on the
same data, in interleaved runs.

Data: flattened trials of utils.synthetic.make_patient (T 14 x 10 channels = 140 features, first phoneme of 9 as the label), 500
rows.  Estimator: SVC(kernel='rbf', class_weight='balanced').  Sizes: 5 folds x 5 candidates and 20 folds x 25 candidates (the grid
C in 1e-1..1e3 x gamma in 1e-4..1, or its diagonal).  Neither route refits.  A run is
fit(X, y), timed by the host clock with a device synchronise on both sides; `warmup` untimed runs of each route, then the median
of `runs` runs.

    python tools/bench_svc_search.py [--runs 10] [--warmup 2] [--sizes 5x5 20x25]        prints one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from sklearn.model_selection import GridSearchCV, StratifiedKFold

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cross_patient_speech_decoding_amd.decoders import SVC, SVCSearchCV               # noqa: E402
from cross_patient_speech_decoding_amd.utils.synthetic import make_patient             # noqa: E402


def features(n=500):
    X, y = make_patient(0, n, T=14, C=10, n_cond=64, noise=2.0)
    return X.reshape(len(X), -1).astype(np.float64), y[:, 0]


def candidates(n):
    """n (C, gamma) pairs of the 5 x 5 grid C in 1e-1..1e3, gamma in 1e-4..1 (for n < 25: along its diagonal, wrapping); the same
    pairs for both routes."""
    grid = [{'C': C, 'gamma': gamma} for C in (0.1, 1.0, 10.0, 100.0, 1000.0) for gamma in (1e-4, 1e-3, 1e-2, 1e-1, 1.0)]
    return grid if n == len(grid) else [grid[(6 * i) % len(grid)] for i in range(n)]


def run(search, X, y):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    search.fit(X, y)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--sizes', nargs='+', default=['5x5', '20x25'], help='folds x candidates')
    args = ap.parse_args()
    if args.runs < 10:
        ap.error('--runs must be at least 10')
    X, y = features()
    svc = dict(kernel='rbf', class_weight='balanced')
    cases = []
    for size in args.sizes:
        folds, n_cand = (int(v) for v in size.split('x'))
        cands = candidates(n_cand)
        cv = StratifiedKFold(folds)
        fused = SVCSearchCV(SVC(**svc), candidates=cands, cv=cv, refit=False)
        grid = GridSearchCV(SVC(**svc), [{key: [val] for key, val in c.items()} for c in cands], cv=cv, n_jobs=None, refit=False)
        for _ in range(args.warmup):
            run(fused, X, y)
            run(grid, X, y)
        t_f, t_g = [], []
        for _ in range(args.runs):                           # interleaved: both routes see the same state of the machine
            t_f.append(run(fused, X, y))
            t_g.append(run(grid, X, y))
        med_f, med_g = statistics.median(t_f), statistics.median(t_g)
        diff = np.abs(fused.cv_results_['mean_test_score'] - grid.cv_results_['mean_test_score'])
        cases.append({'folds': folds, 'candidates': n_cand, 'fused_ms': round(med_f, 3), 'gridsearchcv_ms': round(med_g, 3),
                      'fused_min_ms': round(min(t_f), 3), 'gridsearchcv_min_ms': round(min(t_g), 3), 'ratio': round(med_g / med_f, 2),
                      'max_mean_score_diff': round(float(diff.max()), 4), 'same_best': bool(fused.best_index_ == grid.best_index_),
                      'fused_best_score': round(float(fused.best_score_), 4), 'gridsearchcv_best_score': round(float(grid.best_score_), 4)})
    print(json.dumps({'bench': 'svc_search', 'device': torch.cuda.get_device_name(0), 'n': len(y), 'n_features': X.shape[1],
                      'n_classes': int(len(np.unique(y))), 'svc': svc, 'runs': args.runs, 'warmup': args.warmup,
                      'timed': 'fit without refit, host clock, median', 'cases': cases}))


if __name__ == '__main__':
    main()
