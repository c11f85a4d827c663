"""RDM similarity benchmark: alignment.rsa.rdm_alignment_scores -- condition averages, one standardise launch, one
ragged Gram launch, one comparison call for every pair and every label permutation -- beside the host loop the reference's figure
notebooks make (a double loop of scipy.stats.pearsonr calls per RDM, then pearsonr of the two upper triangles; the Mantel null by
fancy indexing of the second matrix, once per permutation), in the same process on the same arrays.

Data: utils.synthetic.make_patient as in tools/bench_cluster_scores.py: a target of 150 trials plus 3 other patients of 150 trials,
T = 20 samples, 256 channels, each patient reduced by its own device PCA at n_components = 0.9 (the notebooks' to_align_sub) to
(n_trials, T, d) float64; labels: the full three-phoneme sequences (64 conditions).  R = 0 and R = 200 permutations from
RandomState(0) -- the host loop uses the very same permutation tables.  A run is timed by the host clock with a device synchronise
on both sides; `--warmup` untimed runs, then the median and minimum of `--runs` on both sides.  Progress goes to stderr.

    python tools/bench_rsa.py [--runs 10] [--warmup 2] [--permutations 200]     prints one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy import stats

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cross_patient_speech_decoding_amd.alignment import PCA, rsa                         # noqa: E402
from cross_patient_speech_decoding_amd.alignment.alignment_utils import label2str       # noqa: E402
from cross_patient_speech_decoding_amd.utils.synthetic import make_patient              # noqa: E402


def latents(trials, others, T, C):
    out = []
    for p in range(1 + others):
        x, y = make_patient(p, trials, T=T, C=C)
        z = PCA(n_components=0.9).fit_transform(x.reshape(-1, C))
        out.append((np.asarray(z, dtype=np.float64).reshape(trials, T, -1), y))
    return out


def host_rdm(data, labels):
    """The notebooks' calc_rdm_corr: condition averages, then the double loop of pearsonr calls."""
    keys = label2str(labels)
    uniq = np.unique(keys)
    flat = data.reshape(len(data), -1)
    ca = np.stack([np.mean(flat[keys == c], axis=0) for c in uniq])
    rdm = np.zeros((len(uniq), len(uniq)))
    for i in range(len(uniq)):
        for j in range(len(uniq)):
            rdm[i, j] = 1 - stats.pearsonr(ca[i], ca[j])[0]
    return rdm, uniq


def host_loop(pats, R, seed):
    """RDMs of every patient, the comparison of each other patient with the target, and R relabelled comparisons each."""
    rdms = [host_rdm(x, y) for x, y in pats]
    lists = [rsa._shared_indices(rdms[0][1], u) for _, u in rdms[1:]]
    tables = rsa.permutation_tables([len(s) for s, _, _ in lists], R, seed)
    out = np.empty((len(lists), R + 1))
    for q, (shared, ia, ib) in enumerate(lists):
        tri = np.triu_indices(len(shared), k=1)
        x = rdms[0][0][np.ix_(ia, ia)][tri]
        B = rdms[q + 1][0]
        for r, p in enumerate(tables[len(shared)]):
            out[q, r] = stats.pearsonr(x, B[np.ix_(ib[p], ib[p])][tri])[0]
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
    ap.add_argument('--permutations', type=int, default=200)
    ap.add_argument('--trials', type=int, default=150)
    ap.add_argument('--others', type=int, default=3)
    ap.add_argument('--channels', type=int, default=256)
    args = ap.parse_args()
    if args.runs < 10 or args.warmup < 2:
        ap.error('--runs must be at least 10 and --warmup at least 2')
    pats = latents(args.trials, args.others, 20, args.channels)
    (tx, ty), rest = pats[0], pats[1:]
    out = {'bench': 'rsa', 'device': torch.cuda.get_device_name(0), 'shapes': [list(x.shape) for x, _ in pats], 'dtype': 'float64',
           'n_conditions': [int(len(np.unique(label2str(y)))) for _, y in pats], 'runs': args.runs, 'warmup': args.warmup,
           'timed': 'RDMs of all patients and every comparison with its null, host clock with a device synchronise on both sides, '
                    'median (min)'}
    for R in (0, args.permutations):
        def device():
            return rsa.rdm_alignment_scores(tx, ty, [x for x, _ in rest], [y for _, y in rest], n_permutations=R, random_state=0)
        for i in range(args.warmup):
            timed(device, f'R={R} device, warm-up')
        runs = [timed(device, f'R={R} device, run {i}') for i in range(args.runs)]
        t_d, res = [r[0] for r in runs], runs[-1][1]
        for i in range(args.warmup):
            timed(lambda: host_loop(pats, R, 0), f'R={R} host loop, warm-up')
        host = [timed(lambda: host_loop(pats, R, 0), f'R={R} host loop, run {i}') for i in range(args.runs)]
        t_h, ref = [h[0] for h in host], host[-1][1]
        got = np.concatenate([res.similarity_[:, None], res.comparison_.null_], axis=1)
        med_d, med_h = statistics.median(t_d), statistics.median(t_h)
        out[f'R{R}'] = {'comparisons': int(got.size), 'n_shared': [int(m) for m in res.comparison_.n_shared_],
                        'device_ms': round(med_d, 3), 'device_min_ms': round(min(t_d), 3),
                        'host_loop_ms': round(med_h, 3), 'host_loop_min_ms': round(min(t_h), 3),
                        'ratio': round(med_h / med_d, 2), 'device_not_slower': bool(med_d <= med_h),
                        'max_abs_diff_to_host_loop': float(np.max(np.abs(got - ref))),
                        'similarity': [round(float(v), 6) for v in res.similarity_],
                        'p_values': [round(float(v), 5) for v in res.p_value_]}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
