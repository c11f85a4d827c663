"""CTC forced alignment, one launch (realtime_sim.forced_align; csrc/xps_ctc_align.hip), at the CTC training shape
(B = 2048 trials x 47 windows x 11 classes, targets of up to 5 phonemes) and at T = 512, L = 64, beside the numpy
restatement tests/ctc_align_ref.py on one host core (timed on a few sequences, scaled to the batch).  The device time is a
host clock around the launch with a device synchronise on both sides, after warm-ups; the median of --reps runs.  The kernel
is a chain of T dependent steps per sequence and is latency-bound by construction: no share of a peak rate is quoted.
Prints one JSON line.

    python tools/bench_ctc_align.py [--reps 15] [--warmup 3] [--host-seqs 8]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = (dict(name='training', B=2048, T=47, C=11, L=5, ragged=True), dict(name='long', B=2048, T=512, C=11, L=64, ragged=False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-seqs', type=int, default=8)
    a = ap.parse_args()
    if a.reps < 9:
        raise SystemExit('--reps: the median is taken over at least 9 runs')
    from ctc_align_ref import align_ref
    from cross_patient_speech_decoding_amd._dev import stream, workspace
    from cross_patient_speech_decoding_amd._lib import call, lib
    from cross_patient_speech_decoding_amd.realtime_sim import forced_align
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    rows = []
    for sh in SHAPES:
        B, T, Cn, L = sh['B'], sh['T'], sh['C'], sh['L']
        rng = np.random.default_rng(0)
        z = (rng.standard_normal((B, T, Cn)) * 3.0).astype(np.float32)
        tg = rng.integers(1, Cn, (B, L)).astype(np.int64)
        tl = rng.integers(1, L + 1, B).astype(np.int64) if sh['ragged'] else np.full(B, L, np.int64)
        lp = torch.log_softmax(torch.from_numpy(z).to(dev), dim=2)
        al = forced_align(lp, tg, target_lengths=tl)                   # the wrapper once: checks, copies, module load
        n = a.host_seqs
        t0 = time.perf_counter()
        ref = align_ref(lp[:n].cpu().numpy(), tg[:n], None, tl[:n], 0)
        host_s = (time.perf_counter() - t0) / n
        assert np.array_equal(al.states[:n].cpu().numpy(), ref[0]) and np.array_equal(al.score[:n].cpu().numpy(), ref[3])
        # the launch alone: outputs and workspace allocated once, as a caller that aligns every batch of an epoch would
        tg_d, tl_d = torch.from_numpy(tg).to(dev), torch.from_numpy(tl).to(dev)
        states = torch.empty(B, T, dtype=torch.int32, device=dev)
        t_start, t_end = (torch.empty(B, L, dtype=torch.int32, device=dev) for _ in range(2))
        score = torch.empty(B, dtype=torch.float64, device=dev)
        ws_bytes = int(lib().xps_ctc_align_workspace(B, T, L))
        ws = workspace(ws_bytes, dev)

        def launch():
            call('xps_ctc_align', lp.data_ptr(), 1, lp.stride(1), lp.stride(0), T, B, Cn, L, tg_d.data_ptr(), L, None,
                 tl_d.data_ptr(), 0, states.data_ptr(), t_start.data_ptr(), t_end.data_ptr(), score.data_ptr(),
                 ws.data_ptr(), ws_bytes, stream(dev))

        for _ in range(a.warmup):
            launch()
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            launch()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        assert torch.equal(states, al.states) and torch.equal(score, al.score)
        ms = float(np.median(times)) * 1e3
        rows.append({'shape': sh['name'], 'B': B, 'T': T, 'C': Cn, 'L_max': L, 'device_ms_median': round(ms, 4),
                     'device_ms_min': round(min(times) * 1e3, 4), 'device_ms_max': round(max(times) * 1e3, 4),
                     'reps': a.reps, 'warmup': a.warmup, 'sequences_per_s': round(B / (ms * 1e-3)),
                     'host_ms_per_sequence': round(host_s * 1e3, 4), 'host_ms_batch_one_core': round(host_s * B * 1e3, 1),
                     'host_sequences_timed': n, 'workspace_bytes': ws_bytes})
    print(json.dumps({'tool': 'bench_ctc_align', 'host': 'numpy restatement (tests/ctc_align_ref.py), one core',
                      'timing': 'host clock, device synchronise on both sides', 'rows': rows}))


if __name__ == '__main__':
    main()
