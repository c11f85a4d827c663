"""Offline CTC prefix beam search throughput at config 5's validation shape: B trials x 47 windows x 11 classes, beam 8
and 100, one launch (realtime_sim.beam_decode_batch; csrc/xps_ctc_beam.hip).  Against a host search timed on a few
trials on one core: the reference decode when --reference names its aligned_decoding directory, else the CPU restatement
tests/ctc_beam_ref.py (the same search, pure Python).  Prints one JSON line.

    python tools/bench_ctc_beam.py [--B 1024] [--reps 20] [--host-trials 3] [--reference DIR]"""
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


def host_search(reference):
    if reference:
        sys.path.insert(0, reference)
        from realtime_sim.ctc_decoder import decode
        return 'reference decode', lambda p, beam: decode(p, beam, 0)
    from ctc_beam_ref import beam_search
    return 'CPU restatement (tests/ctc_beam_ref.py)', lambda p, beam: beam_search(np.log(p), beam, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--B', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-trials', type=int, default=3)
    ap.add_argument('--reference', default=None)
    a = ap.parse_args()
    from cross_patient_speech_decoding_amd.realtime_sim.ctc_decoder import _beam_device, beam_decode_batch
    torch.cuda.set_device(0)
    T, S = 47, 11
    rng = np.random.default_rng(0)
    z = (rng.standard_normal((a.B, T, S)) * 3.0).astype(np.float32)
    x = torch.from_numpy(z).cuda()
    probs = np.exp(z.astype(np.float64))
    probs /= probs.sum(-1, keepdims=True)
    host_name, host = host_search(a.reference)
    rows = []
    for beam in (8, 100):
        beam_decode_batch(x, beam_size=beam, from_logits=True)           # module load, LDS attribute
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        dev = []
        for _ in range(a.reps):
            ev[0].record()
            _beam_device(x, None, beam, 0, True)
            ev[1].record()
            ev[1].synchronize()
            dev.append(ev[0].elapsed_time(ev[1]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            beam_decode_batch(x, beam_size=beam, from_logits=True)
        wall = (time.perf_counter() - t0) / a.reps
        t0 = time.perf_counter()
        for i in range(a.host_trials):
            host(probs[i], beam)
        host_s = (time.perf_counter() - t0) / a.host_trials
        ms = float(np.median(dev))
        rows.append({'beam': beam, 'device_ms_median': round(ms, 3), 'wall_ms_with_lists': round(wall * 1e3, 3),
                     'trials_per_s': round(a.B / (ms * 1e-3)), 'host_s_per_trial': round(host_s, 4),
                     'host_trials_per_s': round(1.0 / host_s, 1), 'speedup_vs_host_core': round(host_s * a.B / (ms * 1e-3))})
    print(json.dumps({'tool': 'bench_ctc_beam', 'shape': f'B{a.B} T{T} S{S} from_logits', 'host': host_name,
                      'host_cores': 1, 'host_cpus_visible': len(os.sched_getaffinity(0)), 'rows': rows}))


if __name__ == '__main__':
    main()
