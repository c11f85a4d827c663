"""Single-label classifier kernels and models (csrc/xps_classify.hip): device time on one GPU.

  time_max   xps_time_max_fwd_f32 / _bwd_f32 on (T', B, F) tensors beside torch.max(z, dim=0) and its autograd, and beside the
             time HBM needs for the 4 T' B F bytes a pass has to move (at the 6.29 TB/s a float4 copy reaches on this part; the
             8 TB/s specification is printed too).  "_hbm" figures rotate over a ring of tensors of twice the 256 MiB Infinity
             Cache, so each call streams from / to HBM; "_cache_resident" figures repeat on one tensor that fits in that cache and
             measure the cache; the autograd backward figures write a dz that the allocator hands out (it may stay resident).
             The 4-byte path is timed on a base pointer that is only 4-byte aligned.
  classify   XF.classify_loss_acc beside XF.cross_entropy + cmat_acc on the same logits: device kernels per call (counted by
             torch.profiler) and time
  step       one training step (forward, loss, backward, fused AdamW) of TemporalConvRNN and TCN_classifier

Call times: events around --inner back-to-back calls, median / min / max per call over --reps samples after --warmup untimed
samples; they include the host's enqueue time, which is longer than a microsecond kernel.  Kernel counts and device time per
call ("kernels", "device_us_per_call") come from torch.profiler's device records.  Prints one JSON line.

    python tools/bench_classifier.py [--T 20] [--B 2048] [--F 100] [--F2 512] [--H 128] [--classes 9] [--reps 100] [--inner 20]"""
import argparse
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12
RING_BYTES = 512 << 20              # twice the 256 MiB Infinity Cache


def device_stats(fn, reps, warmup, inner):
    for _ in range(warmup * inner):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps):
        ev[0].record()
        for _ in range(inner):
            fn()
        ev[1].record()
        ev[1].synchronize()
        times.append(ev[0].elapsed_time(ev[1]) * 1e3 / inner)
    return [round(float(v), 3) for v in (np.median(times), np.min(times), np.max(times))]       # us per call


def count_kernels(fn, calls=20):
    """Device kernels launched by one call of fn and their summed device time per call in us, from torch.profiler's device
    records of `calls` calls (None where the profiler is not available).  The event timings above include the host's enqueue
    time, which exceeds the device time of a microsecond kernel; this figure does not."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')
               and not e.name.lower().startswith(('memcpy', 'memset'))]
        total = sum(float(e.time_range.elapsed_us()) for e in evs)
        return {'kernels': len(evs) / calls, 'device_us_per_call': round(total / calls, 3), 'names': sorted({e.name[:60] for e in evs})}
    except Exception as exc:                                       # noqa: BLE001 - a figure that is missing, not a wrong one
        return {'kernels': None, 'error': repr(exc)[:200]}


def main():
    ap = argparse.ArgumentParser()
    for name, default in (('T', 20), ('B', 2048), ('F', 100), ('F2', 512), ('H', 128), ('classes', 9), ('C', 64), ('reps', 100),
                          ('warmup', 5), ('inner', 20)):
        ap.add_argument('--' + name, type=int, default=default)
    a = ap.parse_args()
    from cross_patient_speech_decoding_amd.nn_models import TCN_classifier, TemporalConvRNN, cmat_acc
    from cross_patient_speech_decoding_amd.nn_models import functional as XF
    from cross_patient_speech_decoding_amd.nn_models.trainer import FlatAdamW
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    out = {'tool': 'bench_classifier', 'device': torch.cuda.get_device_name(0), 'us_median_min_max': True}
    st = (a.reps, a.warmup, a.inner)

    # ---- max over time ---------------------------------------------------------------------------------------------
    from cross_patient_speech_decoding_amd._lib import call
    stream = torch.cuda.current_stream().cuda_stream
    for F in (a.F, a.F2):
        nbytes = 4 * a.T * a.B * F
        ring_n = -(-RING_BYTES // nbytes) + 1                      # consecutive calls touch different buffers: 2 x the Infinity Cache in all
        ring = [torch.randn(a.T, a.B, F, device='cuda') for _ in range(ring_n)]
        z = ring[0]
        dout = torch.randn(a.B, F, device='cuda')
        zr = z.clone().requires_grad_(True)
        ours, arg = XF.time_max(zr, return_indices=True)
        ref_v, ref_i = torch.max(z, dim=0)
        same = bool(torch.equal(ours.detach(), ref_v)) and bool(torch.equal(arg.long(), ref_i))
        tv = torch.max(zr, dim=0)[0]
        out_raw = torch.empty(a.B, F, device='cuda')
        arg_raw = torch.empty(a.B, F, dtype=torch.int32, device='cuda')
        nxt = itertools.cycle(range(ring_n))
        res = {'bytes_per_pass': nbytes, 'ring_buffers': ring_n, 'hbm_us_at_6.29TBps': round(nbytes / HBM_MEASURED * 1e6, 3),
               'hbm_us_at_8TBps': round(nbytes / HBM_SPEC * 1e6, 3), 'equals_torch_max_on_device': same}
        # forward, input from HBM (ring) and input resident in the Infinity Cache (one tensor)
        res['fwd_hip_hbm'] = device_stats(lambda: XF.time_max(ring[next(nxt)]), *st)
        res['fwd_torch_max_hbm'] = device_stats(lambda: torch.max(ring[next(nxt)], dim=0), *st)
        res['fwd_hip_cache_resident'] = device_stats(lambda: XF.time_max(z), *st)
        res['fwd_torch_max_cache_resident'] = device_stats(lambda: torch.max(z, dim=0), *st)
        res['fwd_kernels_hbm'] = {'hip': count_kernels(lambda: XF.time_max(ring[next(nxt)]), 2 * ring_n),
                                  'torch': count_kernels(lambda: torch.max(ring[next(nxt)], dim=0), 2 * ring_n)}
        res['bwd_kernels_raw_hbm'] = count_kernels(lambda: call('xps_time_max_bwd_f32', dout.data_ptr(), arg.data_ptr(), ring[next(nxt)].data_ptr(),
                                                                a.T, a.B, F, stream), 2 * ring_n)
        # backward: the raw entry point writing the ring (HBM), and both autograd routes (dz from the allocator: may stay cache resident)
        res['bwd_hip_raw_hbm'] = device_stats(lambda: call('xps_time_max_bwd_f32', dout.data_ptr(), arg.data_ptr(), ring[next(nxt)].data_ptr(),
                                                           a.T, a.B, F, stream), *st)
        res['bwd_hip_autograd'] = device_stats(lambda: torch.autograd.grad(ours, zr, dout, retain_graph=True), *st)
        res['bwd_torch_max_autograd'] = device_stats(lambda: torch.autograd.grad(tv, zr, dout, retain_graph=True), *st)
        res['bwd_kernels'] = {'hip': count_kernels(lambda: torch.autograd.grad(ours, zr, dout, retain_graph=True)),
                              'torch': count_kernels(lambda: torch.autograd.grad(tv, zr, dout, retain_graph=True))}
        # the 4-byte path: the same tensors read from a base that is only 4-byte aligned
        flat = [torch.randn(a.T * a.B * F + 4, device='cuda') for _ in range(ring_n)]
        res['fwd_hip_4byte_path_hbm'] = device_stats(lambda: call('xps_time_max_fwd_f32', flat[next(nxt)][1:].data_ptr(), out_raw.data_ptr(),
                                                                  arg_raw.data_ptr(), a.T, a.B, F, stream), *st)
        out[f'time_max_T{a.T}_B{a.B}_F{F}'] = res
        del ring, flat, z, zr, ours, tv
        torch.cuda.empty_cache()

    # ---- classification step ---------------------------------------------------------------------------------------
    logits = torch.randn(a.B, a.classes, device='cuda')
    target = torch.randint(0, a.classes, (a.B,), device='cuda')
    lg = logits.clone().requires_grad_(True)

    def fused():
        return XF.classify_loss_acc(lg, target, a.classes)

    def composed():
        return XF.cross_entropy(lg, target), cmat_acc(logits, target, a.classes)

    f, c = fused(), composed()
    out[f'classify_rows{a.B}_C{a.classes}'] = {
        'fused': device_stats(fused, *st), 'cross_entropy_plus_cmat_acc': device_stats(composed, *st),
        'fused_kernels': count_kernels(fused), 'composed_kernels': count_kernels(composed),
        'same_loss_bits': bool(torch.equal(f[0].detach(), c[0].detach())), 'same_acc': bool(f[1] == c[1])}

    # ---- one training step of each model ---------------------------------------------------------------------------
    x = torch.randn(a.B, a.T * 10, a.C, device='cuda')
    y = torch.randint(0, a.classes, (a.B,), device='cuda')
    models = {'TemporalConvRNN': TemporalConvRNN(a.C, a.F, a.classes, a.H, 2, 10, None, 10, 0, 0.3, 0.3),
              'TCN_classifier': TCN_classifier(a.C, a.classes, [a.F, 64], 10, 10, 0, 0.3)}
    for name, m in models.items():
        m = m.cuda().train()
        opt = FlatAdamW(m, lr=1e-3, weight_decay=1e-5)
        one = XF.unit_gradient(x.device)

        def step():
            opt.zero_grad()
            loss = m.training_step((x, y), 0)
            loss.backward(one)
            opt.step()

        out[f'step_{name}'] = {'us': device_stats(step, a.reps, a.warmup, max(1, a.inner // 4)), 'kernels': count_kernels(step, 5)}
        XF.check_gru_status()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
