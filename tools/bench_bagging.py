"""Bagged-SVC benchmark: fit + predict of the fused ensemble (decoders.BaggingClassifier) beside sklearn's
BaggingClassifier around decoders.SVC -- the route a user had before the fused ensemble existed -- in the same process on the same
data, in interleaved rounds.

Data: flattened trials of utils.synthetic.make_patient (T 14 x 10 channels = 140 features, first phoneme of 9 as the label),
500 training and 120 test rows.  Cases: E = 10 and E = 100, SVC(kernel='linear') and SVC(kernel='rbf', class_weight='balanced').
A run is fit(X, y) then predict(X_test), timed by the host clock (predict ends in the download of the predictions, so the device
is idle when the clock stops); `warmup` untimed runs of each route, then the median of `runs` runs.

    python tools/bench_bagging.py [--runs 10] [--warmup 2] [--estimators 10 100]        prints one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from sklearn.ensemble import BaggingClassifier as SkBagging

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cross_patient_speech_decoding_amd.decoders import SVC, BaggingClassifier          # noqa: E402
from cross_patient_speech_decoding_amd.utils.synthetic import make_patient             # noqa: E402


def features(n_train=500, n_test=120):
    X, y = make_patient(0, n_train + n_test, T=14, C=10, n_cond=64, noise=2.0)
    X = X.reshape(len(X), -1).astype(np.float64)
    y = y[:, 0]
    return X[:n_train], y[:n_train], X[n_train:], y[n_train:]


def run(model, X, y, Xte):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pred = model.fit(X, y).predict(Xte)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--estimators', type=int, nargs='+', default=[10, 100])
    args = ap.parse_args()
    if args.runs < 10:
        ap.error('--runs must be at least 10')
    X, y, Xte, yte = features()
    cases = []
    for name, svc in (('linear', dict(kernel='linear')), ('rbf-balanced', dict(kernel='rbf', class_weight='balanced'))):
        for E in args.estimators:
            fused = BaggingClassifier(SVC(**svc), n_estimators=E, random_state=0)
            bagged = SkBagging(SVC(**svc), n_estimators=E, random_state=0)
            for _ in range(args.warmup):
                run(fused, X, y, Xte)
                run(bagged, X, y, Xte)
            t_f, t_b = [], []
            for _ in range(args.runs):                       # interleaved: both routes see the same state of the machine
                ms, p_f = run(fused, X, y, Xte)
                t_f.append(ms)
                ms, p_b = run(bagged, X, y, Xte)
                t_b.append(ms)
            med_f, med_b = statistics.median(t_f), statistics.median(t_b)
            cases.append({'svc': name, 'n_estimators': E, 'fused_ms': round(med_f, 3), 'sklearn_bagged_ms': round(med_b, 3),
                          'fused_min_ms': round(min(t_f), 3), 'sklearn_bagged_min_ms': round(min(t_b), 3),
                          'ratio': round(med_b / med_f, 2), 'agreement': round(float(np.mean(p_f == p_b)), 4),
                          'fused_accuracy': round(float(np.mean(p_f == yte)), 4),
                          'sklearn_bagged_accuracy': round(float(np.mean(p_b == yte)), 4)})
    print(json.dumps({'bench': 'bagging', 'device': torch.cuda.get_device_name(0), 'n_train': len(y), 'n_test': len(yte),
                      'n_features': X.shape[1], 'n_classes': int(len(np.unique(y))), 'runs': args.runs, 'warmup': args.warmup,
                      'timed': 'fit + predict, host clock, median', 'cases': cases}))


if __name__ == '__main__':
    main()
