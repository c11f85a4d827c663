"""Edit-operation alignment, one launch (realtime_sim.edit_align; csrc/xps_edit_align.hip), at the CTC training shape
(B = 2048 pairs, decoded lengths up to 47, targets of up to 5 phonemes, 11 classes) and at P = 512, L = 64: with every
output and with dist + counts only, beside xps_edit_distance_i64 at the same shape in the same session and the numpy
restatement tests/ctc_errors_ref.py on one host core (timed on a few pairs, scaled to the batch); every output but the
confusion matrix is timed as well, which prices the matrix.  The device time is
a host clock around the launch with a device synchronise on both sides, after warm-ups; the median of --reps runs, buffers
allocated once.  The kernel is a chain of dependent rows and then of dependent byte loads per pair: latency-bound by
construction, no share of a peak rate is quoted.  Prints one JSON line.

    python tools/bench_edit_align.py [--reps 15] [--warmup 3] [--host-pairs 8]"""
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

SHAPES = (dict(name='training', B=2048, P=47, L=5, K=11, ragged=True), dict(name='long', B=2048, P=512, L=64, K=11, ragged=False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-pairs', type=int, default=8)
    a = ap.parse_args()
    if a.reps < 9:
        raise SystemExit('--reps: the median is taken over at least 9 runs')
    from ctc_errors_ref import edit_align_ref
    from cross_patient_speech_decoding_amd._dev import stream, workspace
    from cross_patient_speech_decoding_amd._lib import call, lib
    from cross_patient_speech_decoding_amd.realtime_sim import edit_align
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)

    def timed(launch):
        for _ in range(a.warmup):
            launch()
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            launch()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return {'ms_median': round(float(np.median(times)) * 1e3, 4), 'ms_min': round(min(times) * 1e3, 4),
                'ms_max': round(max(times) * 1e3, 4)}

    rows = []
    for sh in SHAPES:
        B, P, L, K = sh['B'], sh['P'], sh['L'], sh['K']
        rng = np.random.default_rng(0)
        pred = rng.integers(1, K, (B, P)).astype(np.int64)
        tgt = rng.integers(1, K, (B, L)).astype(np.int64)
        pl = rng.integers(0, P + 1, B).astype(np.int64) if sh['ragged'] else np.full(B, P, np.int64)
        tl = rng.integers(1, L + 1, B).astype(np.int64) if sh['ragged'] else np.full(B, L, np.int64)
        p_d, t_d, pl_d, tl_d = (torch.from_numpy(v).to(dev) for v in (pred, tgt, pl, tl))
        ea = edit_align(p_d, pl, t_d, tl, n_classes=K)                  # the wrapper once: checks, copies, module load
        n = a.host_pairs
        t0 = time.perf_counter()
        ref = edit_align_ref(pred[:n], pl[:n], tgt[:n], tl[:n], n_classes=K)
        host_s = (time.perf_counter() - t0) / n
        assert np.array_equal(ea.counts[:n].cpu().numpy(), ref[1]) and np.array_equal(ea.target_to_pred[:n].cpu().numpy(), ref[2])

        def buffers(width):
            """Outputs and workspace for rows declared `width` tokens wide, allocated once."""
            nbytes = int(lib().xps_edit_align_workspace(B, width, L))
            return dict(dist=torch.empty(B, dtype=torch.int64, device=dev), counts=torch.empty(B, 4, dtype=torch.int64, device=dev),
                        t2p=torch.empty(B, L, dtype=torch.int32, device=dev), p2t=torch.empty(B, width, dtype=torch.int32, device=dev),
                        conf=torch.zeros(K + 1, K + 1, dtype=torch.int64, device=dev), ws=workspace(nbytes, dev), ws_bytes=nbytes)

        def launcher(src, width, o, maps, conf=None):
            conf = maps if conf is None else conf

            def launch():
                call('xps_edit_align', src.data_ptr(), src.stride(0), pl_d.data_ptr(), t_d.data_ptr(), L, tl_d.data_ptr(), B,
                     width, L, K, o['dist'].data_ptr(), o['counts'].data_ptr(), o['t2p'].data_ptr() if maps else None,
                     o['p2t'].data_ptr() if maps else None, o['conf'].data_ptr() if conf else None, o['ws'].data_ptr(),
                     o['ws_bytes'], stream(dev))
            return launch

        o = buffers(P)
        row = {'shape': sh['name'], 'B': B, 'P': P, 'L_max': L, 'K': K, 'reps': a.reps, 'warmup': a.warmup,
               'workspace_bytes': o['ws_bytes'],
               'every_output': timed(launcher(p_d, P, o, True)), 'all_but_confusion': timed(launcher(p_d, P, o, True, False)),
               'dist_and_counts': timed(launcher(p_d, P, o, False))}
        assert torch.equal(o['dist'], ea.distance) and torch.equal(o['counts'], ea.counts)
        assert torch.equal(o['t2p'], ea.target_to_pred) and torch.equal(o['p2t'], ea.pred_to_target)
        assert torch.equal(o['conf'], ea.confusion * (a.warmup + a.reps))        # the matrix accumulates over the launches
        dist = torch.empty(B, dtype=torch.int64, device=dev)
        row['edit_distance_i64'] = timed(lambda: call('xps_edit_distance_i64', p_d.data_ptr(), P, pl_d.data_ptr(), t_d.data_ptr(),
                                                      L, tl_d.data_ptr(), B, P, L, dist.data_ptr(), stream(dev)))
        assert torch.equal(dist, ea.distance)
        ms = row['every_output']['ms_median']
        row.update({'pairs_per_s': round(B / (ms * 1e-3)), 'host_ms_per_pair': round(host_s * 1e3, 4),
                    'host_ms_batch_one_core': round(host_s * B * 1e3, 1), 'host_pairs_timed': n})
        rows.append(row)
    print(json.dumps({'tool': 'bench_edit_align', 'host': 'numpy restatement (tests/ctc_errors_ref.py), one core',
                      'timing': 'host clock, device synchronise on both sides', 'rows': rows}))


if __name__ == '__main__':
    main()
