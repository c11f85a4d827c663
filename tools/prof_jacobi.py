"""Jacobi profiling targets.

    python tools/prof_jacobi.py                       target for rocprofv3: one eigh_sym_top(1024, 30) (per-round Jacobi launches)
    python tools/prof_jacobi.py --ragged [--batch 20] [--n 137] [--groups 1,2,4,8] [--runs 10] [--warmup 2]
        DESIGN.md 4.18: `batch` PSD matrices of `n` rows decomposed by eigh_psd_batched (ONE ragged call) beside the loop of
        eigh_psd over them, in the same process in interleaved runs, host clock with a device synchronise on both sides; the
        ragged route once per blind-group size of --groups.  Prints one JSON line: both medians, the sweeps per matrix, the
        calls into libxps.so of each route, and whether the two routes gave the same bits.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from cross_patient_speech_decoding_amd.alignment import _linalg as LA


def eigh_top_target():
    rng = np.random.default_rng(0)
    B = rng.standard_normal((1024, 300)); C = torch.from_numpy(B @ B.T / 300 + 0.5 * np.eye(1024)).cuda()
    for _ in range(2):
        w, V = LA.eigh_sym_top(C, 30)
    torch.cuda.synchronize()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def counted(fn):
    counts, real = {}, LA.call

    def counting(name, *a):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *a)
    LA.call = counting
    try:
        fn()
    finally:
        LA.call = real
    return counts


def ragged(args):
    rng = np.random.default_rng(0)
    Cs = []
    for i in range(args.batch):                               # Gram matrices of `n` centred rows of 4 n features: full rank - 1 + shift
        F = rng.standard_normal((args.n, 4 * args.n))
        F -= F.mean(axis=0)
        Cs.append(F @ F.T + 1e-3 * np.eye(args.n))
    Cs = np.stack(Cs)
    groups = [int(g) for g in args.groups.split(',')]
    routes = {'loop of eigh_psd': lambda: [LA.eigh_psd(LA.to_device(C)) for C in Cs]}
    for g in groups:
        def route(g=g):
            LA.RAGGED_GROUP = g
            return LA.eigh_psd_batched(Cs)
        routes[f'ragged, group {g}'] = route
    default_group = LA.RAGGED_GROUP
    times = {name: [] for name in routes}
    outs = {}
    for i in range(args.warmup + args.runs):                  # interleaved: every route sees the same state of the machine
        for name, fn in routes.items():
            ms, outs[name] = timed(fn)
            if i >= args.warmup:
                times[name].append(ms)
    calls = {name: counted(fn) for name, fn in routes.items()}
    LA.RAGGED_GROUP = default_group
    ref = outs['loop of eigh_psd']
    same = {name: all(np.array_equal(w, wr) and np.array_equal(V, Vr) for (w, V), (wr, Vr) in zip(out, ref))
            for name, out in outs.items()}
    Ws = [LA.to_device(C + LA._shift_of(LA.to_device(C)) * np.eye(args.n)) for C in Cs]
    _, sweeps = LA.jacobi_ragged(Ws)
    print(json.dumps({'bench': 'jacobi_ragged', 'device': torch.cuda.get_device_name(0), 'batch': args.batch, 'n': args.n,
                      'runs': args.runs, 'warmup': args.warmup, 'timed': 'host clock, median (min)', 'default_group': default_group,
                      'ms': {name: [round(statistics.median(t), 3), round(min(t), 3)] for name, t in times.items()},
                      'same_bits_as_loop': same, 'sweeps_per_matrix': [int(s) for s in sweeps],
                      'libxps_calls': {name: sum(c.values()) for name, c in calls.items()},
                      'libxps_calls_by_name': calls}))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--ragged', action='store_true')
    ap.add_argument('--batch', type=int, default=20)
    ap.add_argument('--n', type=int, default=137)
    ap.add_argument('--groups', default='1,2,4,8')
    ap.add_argument('--runs', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    ragged(a) if a.ragged else eigh_top_target()
