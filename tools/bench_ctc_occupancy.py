"""CTC posterior occupancies, one launch (xps_ctc_occupancy; csrc/xps_ctc_occupancy.hip), at the two shapes of
tools/bench_ctc_align.py: the CTC training shape (B = 2048 trials x 47 windows x 11 classes, targets of up to 5 phonemes)
and T = 512, L = 64.  The device time is a host clock around the launch with a device synchronise on both sides, after
warm-ups; the median of --reps runs; outputs and workspace are allocated once.  Each shape is timed with every output, with
log_z and the two moments only (no posterior tensor leaves, so the difference is their store traffic and the class sums),
and at B = 256 (one workgroup per CU: the latency of one sequence's dependent chain).  Beside each time: the bytes the
launch moves (alpha written and read back, the outputs) and the double-precision exp / log evaluations it makes, so that
the rate can be set against the memory and the vector units.  Prints one JSON line.

    python tools/bench_ctc_occupancy.py [--reps 15] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (dict(name='training', B=2048, T=47, C=11, L=5, ragged=True), dict(name='long', B=2048, T=512, C=11, L=64, ragged=False))
SMALL_B = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    if a.reps < 9:
        raise SystemExit('--reps: the median is taken over at least 9 runs')
    from cross_patient_speech_decoding_amd._dev import stream, workspace
    from cross_patient_speech_decoding_amd._lib import call, lib
    from cross_patient_speech_decoding_amd.realtime_sim import posterior_align
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
        occ = posterior_align(lp[:64], tg[:64], target_lengths=tl[:64])         # the wrapper once: checks, copies, module load
        tg_d, tl_d = torch.from_numpy(tg).to(dev), torch.from_numpy(tl).to(dev)

        def out(*shape):
            return torch.empty(*shape, dtype=torch.float64, device=dev)
        log_z, ef, om = out(B), out(B, L), out(B, L)
        tok, ons, cls = out(B, T, L), out(B, T, L), out(B, T, Cn)
        ws_bytes = int(lib().xps_ctc_occupancy_workspace(B, T, L))
        ws = workspace(ws_bytes, dev)
        states = int((2 * tl + 1).sum()) * T                                     # (sequence, frame, state) cells of the batch

        for n, full in ((B, True), (B, False), (SMALL_B, True)):
            def launch():
                call('xps_ctc_occupancy', lp.data_ptr(), 1, lp.stride(1), lp.stride(0), T, n, Cn, L, tg_d.data_ptr(), L, None,
                     tl_d.data_ptr(), 0, log_z.data_ptr(), tok.data_ptr() if full else None, ons.data_ptr() if full else None,
                     cls.data_ptr() if full else None, ef.data_ptr(), om.data_ptr(), ws.data_ptr(), ws_bytes, stream(dev))

            for _ in range(a.warmup):
                launch()
            times = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                launch()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            if full:
                assert torch.equal(tok[:64], occ.token_occ) and torch.equal(log_z[:64], occ.log_z)
            ms = float(np.median(times)) * 1e3
            cells = states * n // B
            alpha_bytes = 2 * 8 * cells + 2 * 8 * (cells // 2)                   # written, read back; the two onset predecessors of the odd states
            out_bytes = (2 * n * T * L + n * T * Cn) * 8 if full else 0
            fn_calls = cells * 4 + cells * 5 + (cells // 2) * 5                  # pass 1: 3 exp + log; pass 2: 3 exp + log + exp; onset: 3 exp + log + exp
            rows.append({'shape': sh['name'], 'B': n, 'T': T, 'C': Cn, 'L_max': L, 'outputs': 'all' if full else 'log_z and moments',
                         'device_ms_median': round(ms, 4), 'device_ms_min': round(min(times) * 1e3, 4),
                         'device_ms_max': round(max(times) * 1e3, 4), 'reps': a.reps, 'warmup': a.warmup,
                         'sequences_per_s': round(n / (ms * 1e-3)), 'workspace_bytes': ws_bytes,
                         'alpha_traffic_bytes': alpha_bytes, 'output_bytes': out_bytes,
                         'traffic_GB_per_s': round((alpha_bytes + out_bytes) / (ms * 1e-3) / 1e9, 1),
                         'exp_log_calls': fn_calls, 'exp_log_G_per_s': round(fn_calls / (ms * 1e-3) / 1e9, 2)})
    print(json.dumps({'tool': 'bench_ctc_occupancy', 'timing': 'host clock, device synchronise on both sides', 'rows': rows}))


if __name__ == '__main__':
    main()
