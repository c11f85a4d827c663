"""SVC search through DimRedReshape(PCA) benchmark: SVCSearchCV(batch_pca=True) -- one Gram matrix for all
folds, one eigendecomposition per fold for all component counts -- beside the same search with batch_pca=False over
DimRedReshape(sklearn.decomposition.PCA), the route a user had at this width before (one host PCA fit per (n_components, fold)),
in the same process on the same data, in interleaved runs.  The batch_pca=False route over DimRedReshape(GramPCA) is reported too,
for information, from fewer runs.

Data: utils.synthetic.make_patient at the reference notebook's shape (144 trials, 200 samples, 111 channels: 22 200 features per
flattened trial, float32), first phoneme of 9 as the label.  20 seeded KFold splits passed as a list; 25 seeded candidates:
n_components from np.arange(0.1, 1, 0.1), C in 1e-1..1e3, gamma in 1e-4..1 (the ranges of 4.15).  Estimator:
make_pipeline(DimRedReshape(...), SVC(kernel='rbf', class_weight='balanced')).  No route refits.  A run is fit(X, y), timed by the
host clock with a device synchronise on both sides; `warmup` untimed runs of each route, then the median and minimum of `runs`.
The comparator fits one host PCA of 137 x 22 200 per (distinct n_components, fold), 160 per run (about half a minute): `--comparator-runs` / `--comparator-warmup` give it
fewer runs than the fused route (interleaved with the fused route's first runs), and the JSON line says how many it got.
Progress goes to stderr, one line per run.

    python tools/bench_pca_search.py [--runs 10] [--warmup 2] [--comparator-runs 10] [--comparator-warmup 2] [--info-runs 3]
                                                                                                     prints one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time
from collections import Counter

import numpy as np
import torch
from sklearn.decomposition import PCA as SkPCA
from sklearn.model_selection import KFold
from sklearn.pipeline import make_pipeline

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cross_patient_speech_decoding_amd import _lib                                      # noqa: E402
from cross_patient_speech_decoding_amd.alignment import GramPCA                         # noqa: E402
from cross_patient_speech_decoding_amd.decoders import SVC, SVCSearchCV                 # noqa: E402
from cross_patient_speech_decoding_amd.decomposition import DimRedReshape               # noqa: E402
from cross_patient_speech_decoding_amd.utils.synthetic import make_patient              # noqa: E402


def candidates(n=25, seed=0):
    rng = np.random.default_rng(seed)
    fractions = np.arange(0.1, 1, 0.1)
    return [{'dimredreshape__n_components': float(rng.choice(fractions)), 'svc__C': float(10.0 ** rng.uniform(-1, 3)),
             'svc__gamma': float(10.0 ** rng.uniform(-4, 0))} for _ in range(n)]


def run(search, X, y, what=''):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    search.fit(X, y)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    print(f'{what}: {ms:.1f} ms', file=sys.stderr, flush=True)
    return ms


def library_calls(search, X, y, what):
    """Calls into libxps.so of one (untimed, warm-up) fit, by entry point (every module binds `call` by name: all of them are patched
    and restored)."""
    counts = Counter()
    real = _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    bound = [mod for mod in list(sys.modules.values())
             if getattr(mod, '__name__', '').startswith('cross_patient_speech_decoding_amd') and getattr(mod, 'call', None) is real]
    for mod in bound:
        mod.call = counting
    try:
        run(search, X, y, what)
    finally:
        for mod in bound:
            mod.call = real
    return dict(sorted(counts.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--comparator-runs', type=int, default=None, help='timed runs of the sklearn-PCA route (default: --runs)')
    ap.add_argument('--comparator-warmup', type=int, default=None, help='warm-up runs of the sklearn-PCA route (default: --warmup)')
    ap.add_argument('--info-runs', type=int, default=3, help='runs of the batch_pca=False / GramPCA route (reported for information)')
    ap.add_argument('--trials', type=int, default=144)
    args = ap.parse_args()
    if args.runs < 10 or args.warmup < 1:
        ap.error('--runs must be at least 10 and --warmup at least 1')
    c_runs = args.runs if args.comparator_runs is None else args.comparator_runs
    c_warm = args.warmup if args.comparator_warmup is None else args.comparator_warmup
    if not (1 <= c_runs <= args.runs and c_warm >= 1):
        ap.error('--comparator-runs must be in 1..--runs and --comparator-warmup at least 1')
    X, y_full = make_patient(0, args.trials, T=200, C=111)
    y = y_full[:, 0]
    splits = list(KFold(20, shuffle=True, random_state=0).split(X))
    cands = candidates()
    svc = dict(kernel='rbf', class_weight='balanced')
    fused = SVCSearchCV(make_pipeline(DimRedReshape(GramPCA), SVC(**svc)), candidates=cands, cv=splits, refit=False, batch_pca=True)
    host = SVCSearchCV(make_pipeline(DimRedReshape(SkPCA), SVC(**svc)), candidates=cands, cv=splits, refit=False)
    gram = SVCSearchCV(make_pipeline(DimRedReshape(GramPCA), SVC(**svc)), candidates=cands, cv=splits, refit=False)
    calls_f = library_calls(fused, X, y, 'fused, warm-up')    # the first warm-up run of each route also counts its library calls
    calls_h = library_calls(host, X, y, 'sklearn-PCA route, warm-up')
    for i in range(1, max(args.warmup, c_warm)):
        if i < args.warmup:
            run(fused, X, y, 'fused, warm-up')
        if i < c_warm:
            run(host, X, y, 'sklearn-PCA route, warm-up')
    t_f, t_h = [], []
    for i in range(args.runs):                               # interleaved: both routes see the same state of the machine
        t_f.append(run(fused, X, y, f'fused, run {i}'))
        if i < c_runs:
            t_h.append(run(host, X, y, f'sklearn-PCA route, run {i}'))
    t_g = [run(gram, X, y, 'GramPCA route, ' + ('warm-up' if i == 0 else f'run {i - 1}')) for i in range(args.info_runs + 1)][1:] if args.info_runs else []
    med_f, med_h = statistics.median(t_f), statistics.median(t_h)
    diff = np.abs(fused.cv_results_['mean_test_score'] - host.cv_results_['mean_test_score'])
    out = {'bench': 'pca_search', 'device': torch.cuda.get_device_name(0), 'shape': list(X.shape), 'dtype': str(X.dtype),
           'n_classes': int(len(np.unique(y))), 'folds': len(splits), 'candidates': len(cands), 'svc': svc, 'runs': args.runs,
           'warmup': args.warmup, 'comparator_runs': c_runs, 'comparator_warmup': c_warm, 'timed': 'fit without refit, host clock, median',
           'fused_ms': round(med_f, 3), 'fused_min_ms': round(min(t_f), 3),
           'sklearn_pca_route_ms': round(med_h, 3), 'sklearn_pca_route_min_ms': round(min(t_h), 3), 'ratio': round(med_h / med_f, 2),
           'fused_not_slower': bool(med_f <= med_h),
           'max_mean_score_diff': round(float(diff.max()), 4), 'same_best': bool(fused.best_index_ == host.best_index_),
           'fused_best_score': round(float(fused.best_score_), 4), 'sklearn_pca_route_best_score': round(float(host.best_score_), 4),
           'fallbacks': len(fused.pca_fallbacks_),
           'grampca_route_ms': round(statistics.median(t_g), 3) if t_g else None, 'grampca_route_runs': len(t_g),
           'same_best_as_grampca_route': bool(fused.best_index_ == gram.best_index_) if t_g else None,
           'library_calls_fused': calls_f, 'library_calls_sklearn_pca_route': calls_h,
           'n_library_calls_fused': sum(calls_f.values()), 'n_library_calls_sklearn_pca_route': sum(calls_h.values())}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
