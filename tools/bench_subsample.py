"""Electrode subsampling kernels (csrc/xps_subsample.hip): device time against a device-to-device copy and
against what a user would write with framework ops on the device.

At N trials of an X x Y grid with T samples, float32 and float64 (events around the enqueued work, median / min / max of
--reps after --warmup; index arrays are uploaded before the clock starts for every path):
  single   one grouping (contact sizes 1 and 2) through xps_group_mean_*: ms and GB/s of the input alone and of input +
           output, beside copy_d2d = y.copy_(x) of the same input tensor (GB/s counts its read and its write)
  sweep    contact sizes 1..8 in one xps_group_mean_many_* launch, beside the same groupings as a loop of single launches
           and beside the framework composition data[:, ix, iy].mean(1).permute(0, 2, 1).contiguous() per group
  select   every (X/2, Y/2) window (91 on 12 x 24) of channel-last features in one xps_select_channels_* launch, beside a
           loop of single launches and beside X[:, :, idx] per window
and, in the same run, whether the outputs of the paths are the same bits.  Prints one JSON line.

    python tools/bench_subsample.py [--N 2048] [--X 12] [--Y 24] [--T 200] [--reps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_stats(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def row(stats, nbytes=None, **extra):
    r = {'ms_median_min_max': [round(v, 4) for v in stats]}
    if nbytes is not None:
        r['GBps'] = round(nbytes / stats[0] * 1e-6, 1)
    r.update(extra)
    return r


def main():
    ap = argparse.ArgumentParser()
    for name, default in (('N', 2048), ('X', 12), ('Y', 24), ('T', 200), ('reps', 20), ('warmup', 3)):
        ap.add_argument('--' + name, type=int, default=default)
    a = ap.parse_args()
    from cross_patient_speech_decoding_amd import processing_utils as PU
    from cross_patient_speech_decoding_amd._lib import call
    from cross_patient_speech_decoding_amd.processing_utils.spatial_avg_subsampling import _csr
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    N, X, Y, T, C = a.N, a.X, a.Y, a.T, a.X * a.Y
    i32 = lambda v: torch.from_numpy(np.asarray(v).astype(np.int32)).cuda()           # noqa: E731
    out = {'tool': 'bench_subsample', 'shape': f'N{N} grid{X}x{Y} T{T}'}

    groupings = [PU.spatial_avg_idxs((X, Y), k) for k in range(1, 9)]
    csr = [_csr((N, X, Y, T), g, 'bench') for g in groupings]
    gstart = np.concatenate([[0], np.cumsum([len(o) - 1 for o, _ in csr])])
    mstart = np.concatenate([[0], np.cumsum([len(m) for _, m in csr])])
    Gtot, S = int(gstart[-1]), len(csr)
    d_gstart, d_members = i32(gstart), i32(np.concatenate([m for _, m in csr]))
    d_offsets = i32(np.concatenate([o[:-1] + ms for (o, _), ms in zip(csr, mstart[:-1])] + [mstart[-1:]]))
    d_single = [(i32(o), i32(m)) for o, m in csr]
    d_idx = [(torch.from_numpy(np.concatenate([g[:, 0] for g in grp])).cuda(), torch.from_numpy(np.concatenate([g[:, 1] for g in grp])).cuda(),
              len(grp), len(grp[0])) for grp in groupings]

    for dtype, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
        es = 4 if dtype == torch.float32 else 8
        data = torch.randn(N, X, Y, T, device='cuda', dtype=dtype)
        in_bytes = data.numel() * es
        y = torch.empty_like(data)
        res = {'copy_d2d': row(device_stats(lambda: y.copy_(data), a.reps, a.warmup), 2 * in_bytes)}
        del y
        slab = torch.empty(N * T * Gtot, dtype=torch.float64, device='cuda')
        loop = torch.empty_like(slab)

        def single(s, dst):
            o, m = d_single[s]
            call(f'xps_group_mean_{tag}', data.data_ptr(), N, C, T, o.data_ptr(), m.data_ptr(), len(o) - 1,
                 dst.data_ptr() + 8 * N * T * int(gstart[s]), st)

        def sweep():
            call(f'xps_group_mean_many_{tag}', data.data_ptr(), N, C, T, d_gstart.data_ptr(), d_offsets.data_ptr(), d_members.data_ptr(),
                 S, Gtot, slab.data_ptr(), st)

        def loop_of_single():
            for s in range(S):
                single(s, loop)

        def framework(keep=None):
            for s, (ix, iy, G, k) in enumerate(d_idx):          # equal-sized groups: one gather of all groups, mean over the members
                r = data[:, ix, iy].view(N, G, k, T).mean(dim=2).permute(0, 2, 1).contiguous()
                if keep is not None:
                    keep.append(r)

        for s in (0, 1):
            G = int(gstart[s + 1] - gstart[s])
            stats = device_stats(lambda: single(s, loop), a.reps, a.warmup)
            res[f'single_contact{s + 1}'] = row(stats, in_bytes + N * T * G * 8, input_GBps=round(in_bytes / stats[0] * 1e-6, 1))
        res['sweep_1_launch'] = row(device_stats(sweep, a.reps, a.warmup), in_bytes + slab.numel() * 8)
        res['sweep_loop_of_single'] = row(device_stats(loop_of_single, a.reps, a.warmup), S * in_bytes + slab.numel() * 8)
        res['sweep_framework'] = row(device_stats(framework, a.reps, a.warmup))
        fw = []
        framework(fw)
        torch.cuda.synchronize()
        views = [slab[N * T * int(p):N * T * int(q)].view(N, T, int(q - p)) for p, q in zip(gstart[:-1], gstart[1:])]
        res['bits'] = {'sweep_equals_loop': bool(torch.equal(slab.view(torch.int64), loop.view(torch.int64))),
                       'framework_equals_sweep_per_contact': [bool(torch.equal(f.to(torch.float64), v)) for f, v in zip(fw, views)],
                       'framework_max_abs_diff': max(float((f.to(torch.float64) - v).abs().max()) for f, v in zip(fw, views))}
        del fw, views, slab, loop, data
        torch.cuda.empty_cache()

        # ---- channel selection: every half-grid window of channel-last features
        feats = torch.randn(N, T, C, device='cuda', dtype=dtype)
        wins = [g[:, 0] * Y + g[:, 1] for g in PU.grid_susbsample_idxs((X, Y), (X // 2, Y // 2))]
        lstart = np.concatenate([[0], np.cumsum([len(w) for w in wins])])
        d_lstart, d_widx = i32(lstart), i32(np.concatenate(wins))
        d_two = [i32([0, len(w)]) for w in wins]
        d_win64 = [torch.from_numpy(w).cuda() for w in wins]
        Ltot, W = int(lstart[-1]), len(wins)
        sel, sel_loop = (torch.empty(N * T * Ltot, dtype=dtype, device='cuda') for _ in range(2))

        def select_sweep():
            call(f'xps_select_channels_{tag}', feats.data_ptr(), N, T, C, d_lstart.data_ptr(), d_widx.data_ptr(), W, Ltot, sel.data_ptr(), st)

        def select_loop():
            for w in range(W):
                call(f'xps_select_channels_{tag}', feats.data_ptr(), N, T, C, d_two[w].data_ptr(), d_widx.data_ptr() + 4 * int(lstart[w]),
                     1, len(wins[w]), sel_loop.data_ptr() + es * N * T * int(lstart[w]), st)

        def select_framework():
            for w in range(W):
                feats[:, :, d_win64[w]]

        f_bytes = feats.numel() * es
        res['select_windows'] = W
        res['select_1_launch'] = row(device_stats(select_sweep, a.reps, a.warmup), f_bytes + sel.numel() * es)
        res['select_loop_of_single'] = row(device_stats(select_loop, a.reps, a.warmup), W * f_bytes + sel.numel() * es)
        res['select_framework'] = row(device_stats(select_framework, a.reps, a.warmup), W * f_bytes + sel.numel() * es)
        as_int = torch.int32 if es == 4 else torch.int64
        sv = [sel[N * T * int(p):N * T * int(q)].view(N, T, int(q - p)) for p, q in zip(lstart[:-1], lstart[1:])]
        res['bits'].update(select_equals_loop=bool(torch.equal(sel.view(as_int), sel_loop.view(as_int))),
                           select_equals_framework=all(bool(torch.equal(v.view(as_int), feats[:, :, i].view(as_int))) for v, i in zip(sv, d_win64)))
        assert res['bits']['sweep_equals_loop'] and res['bits']['select_equals_loop'] and res['bits']['select_equals_framework'], res['bits']
        out[tag] = res
        del feats, sel, sel_loop, sv
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
