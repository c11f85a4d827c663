"""Cross-patient CTC data path: validation_step wall time and the per-trial augmentation kernels' bandwidth.

validation_step at B trials x T samples x d features, L-label targets: the model's own step (one decode launch, one
edit-distance launch, PER read once) against the host path it replaced, restated here on the SAME batch and model -- B
boolean-mask gathers for the decode, then every decoded sequence copied to the host and a pure-Python Levenshtein per trial.
Median of --reps after --warmup, wall clock around a synchronised step including the float() of the PER.

Augmentations at N x T x C: device time per kernel (events), GB/s counting one read and one write of the tensor, against a
device-to-device copy of the same tensor.  Prints one JSON line.

    python tools/bench_ctc_data.py [--B 2048] [--T 200] [--d 30] [--N 4096] [--C 128] [--reps 20] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def host_validation_step(model, batch):
    """The step before the decode / edit-distance kernels: same loss, host decode bookkeeping and host PER."""
    loss, logits_tm = model._ctc(batch)
    with torch.no_grad():
        best = logits_tm.permute(1, 0, 2).argmax(dim=2)
        keep = torch.ones_like(best, dtype=torch.bool)
        keep[:, 1:] = best[:, 1:] != best[:, :-1]
        keep &= best != model.blank
        decoded = [best[b][keep[b]] for b in range(best.size(0))]
        targets, lengths = batch[1].cpu(), batch[3].cpu()
        dist = sum(host_edit_distance(p.cpu().tolist(), t[:int(l)].tolist()) for p, t, l in zip(decoded, targets, lengths))
        per = dist / float(lengths.sum()) * 100
    return float(loss), per


def device_validation_step(model, batch):
    model._xps_logged = {}
    loss = model.validation_step(batch, 0)
    return float(loss), float(model._xps_logged['val_PER'])


def wall_median(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def device_median(fn, reps, warmup):
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
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    for name, default in (('B', 2048), ('T', 200), ('d', 30), ('L', 3), ('N', 4096), ('C', 128), ('reps', 20), ('warmup', 3)):
        ap.add_argument('--' + name, type=int, default=default)
    a = ap.parse_args()
    from cross_patient_speech_decoding_amd._lib import call
    from cross_patient_speech_decoding_amd.realtime_sim import RealtimeRNNModel
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    ncls = 10
    model = RealtimeRNNModel(14 * a.d, 128, 2, ncls, dropout=0.0).cuda().eval()
    with torch.no_grad():                              # an untrained model emits blanks only: level the classifier bias so the decode has work
        model.classifier.fc.bias.zero_()
    batch = (torch.from_numpy(rng.standard_normal((a.B, a.T, a.d)).astype(np.float32)).cuda(),
             torch.from_numpy(rng.integers(1, ncls, (a.B, a.L))).cuda(), torch.full((a.B,), a.T).cuda(),
             torch.full((a.B,), a.L).cuda())
    with torch.no_grad():
        new = device_validation_step(model, batch)
        old = host_validation_step(model, batch)
        assert abs(new[1] - old[1]) <= 1e-9 * max(1.0, abs(old[1])), (new, old)
        dev_ms = wall_median(lambda: device_validation_step(model, batch), a.reps, a.warmup)
        host_ms = wall_median(lambda: host_validation_step(model, batch), a.reps, a.warmup)
        fwd_ms = wall_median(lambda: float(model._ctc(batch)[0]), a.reps, a.warmup)
    out = {'tool': 'bench_ctc_data', 'validation_shape': f'B{a.B} T{a.T} d{a.d} L{a.L}', 'val_PER': new[1],
           'validation_step_ms': {'kernels_median_min_max': [round(v, 3) for v in dev_ms],
                                  'host_path_median_min_max': [round(v, 3) for v in host_ms],
                                  'loss_only_median_min_max': [round(v, 3) for v in fwd_ms]}}

    x = torch.randn(a.N, a.T, a.C, device='cuda')
    y = torch.empty_like(x)
    st = torch.cuda.current_stream().cuda_stream
    shifts = torch.randint(-20, 21, (a.N,), device='cuda')
    starts = torch.randint(0, a.T - a.T // 10 + 1, (a.N,), device='cuda')
    scales = torch.empty(a.N, device='cuda').uniform_(0.9, 1.1)
    T2 = (a.T * torch.empty(a.N, device='cuda').uniform_(0.8, 1.2)).long()
    nbytes = 2 * x.numel() * 4
    kernels = {
        'copy_d2d': lambda: y.copy_(x),
        'shift': lambda: call('xps_aug_trial_shift_f32', x.data_ptr(), y.data_ptr(), a.N, a.T, a.C, shifts.data_ptr(), st),
        'mask': lambda: call('xps_aug_trial_mask_f32', x.data_ptr(), y.data_ptr(), a.N, a.T, a.C, starts.data_ptr(), a.T // 10, st),
        'scale': lambda: call('xps_aug_trial_scale_f32', x.data_ptr(), y.data_ptr(), a.N, a.T * a.C, scales.data_ptr(), st),
        'warp': lambda: call('xps_aug_trial_warp_f32', x.data_ptr(), y.data_ptr(), a.N, a.T, a.C, T2.data_ptr(), st),
    }
    rows = {}
    for name, fn in kernels.items():
        ms = device_median(fn, a.reps, a.warmup)
        rows[name] = {'ms': round(ms, 4), 'GBps': round(nbytes / ms * 1e-6, 1)}
    out['augmentation_shape'] = f'N{a.N} T{a.T} C{a.C}'
    out['augmentation'] = rows
    print(json.dumps(out))


if __name__ == '__main__':
    main()
