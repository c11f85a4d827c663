"""Device time of the session-replay frontend (xps_hg_trials_f64) against the streaming frontend looped over the same
resident trials (xps_pipe_frontend_f64, ceil(N / 8) calls with k = n_bins), and a device-to-device copy of the input as
the memory ceiling.  Events around each repetition: median of --reps after --warmup, min / max given.  One JSON line.

    python tools/bench_hg_trials.py [--N 2048 --bins 50 --C 128 --Tn 40 --bands 8 --order 4] [--general] [--end-to-end]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from cross_patient_speech_decoding_amd._lib import call, lib  # noqa: E402
from cross_patient_speech_decoding_amd.realtime_sim import realtime_processing as rp  # noqa: E402


def iir(nb, order):
    import scipy.signal as signal
    out = []
    for k in range(nb):
        b, a = signal.butter(order, [60 + 12 * k, 72 + 12 * k], btype='band', fs=2000)
        out.append(np.stack([a, b], axis=1))
    return np.stack(out)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms))}


def frontends(N, n_bins, C, Tn, bands, order, reps, warmup):
    dev = torch.device('cuda')
    coefs = iir(bands, order)
    b, a, zi = rp._split_coefs(coefs, C, None)
    taps = b.shape[1]
    bd, ad, zd = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (b, a, zi))
    gen = torch.Generator(device=dev).manual_seed(1)
    raw = torch.randn(N, n_bins, C, Tn, dtype=torch.float64, device=dev, generator=gen) * 30.0
    good = torch.ones(N, C, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    power = torch.empty(N, n_bins, C, dtype=torch.float64, device=dev)
    state = torch.empty(N, bands, C, taps - 1, dtype=torch.float64, device=dev)
    nbytes = int(lib().xps_hg_trials_f64_workspace(N, n_bins, C, Tn, bands))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def new():
        call('xps_hg_trials_f64', raw.data_ptr(), 0, N, n_bins, C, Tn, None, good.data_ptr(), 1, bd.data_ptr(), ad.data_ptr(),
             bands, taps, zd.data_ptr(), 0, state.data_ptr(), power.data_ptr(), None, None, None, 0, 0, None, ws.data_ptr(),
             nbytes, st)

    power_p = torch.empty_like(power)
    state_p = torch.empty_like(state)
    pbytes = int(lib().xps_pipe_frontend_f64_workspace(8, C, Tn, bands))
    pws = torch.empty(pbytes, dtype=torch.uint8, device=dev)
    zi_all = zd.expand(N, -1, -1, -1)

    def parent():
        state_p.copy_(zi_all)
        for s0 in range(0, N, 8):
            n = min(8, N - s0)
            call('xps_pipe_frontend_f64', raw[s0:s0 + n].data_ptr(), n, n_bins, C, Tn, good[s0:s0 + n].data_ptr(),
                 bd.data_ptr(), ad.data_ptr(), bands, taps, state_p[s0:s0 + n].data_ptr(), power_p[s0:s0 + n].data_ptr(),
                 pws.data_ptr(), pbytes, st)

    dst = torch.empty_like(raw)
    t_new = timed(new, reps, warmup)
    t_parent = timed(parent, reps, warmup)
    t_copy = timed(lambda: dst.copy_(raw), reps, warmup)
    same = bool(torch.equal(power, power_p) and torch.equal(state, state_p))
    in_bytes = raw.numel() * 8
    return {'shape': {'N': N, 'n_bins': n_bins, 'C': C, 'Tn': Tn, 'bands': bands, 'taps': taps},
            'input_GB': in_bytes / 1e9, 'new': t_new, 'parent_loop': t_parent, 'copy_d2d': t_copy,
            'speedup_median': t_parent['median_ms'] / t_new['median_ms'],
            'new_GBps_of_input': in_bytes / 1e6 / t_new['median_ms'],
            'copy_GBps_of_input': in_bytes / 1e6 / t_copy['median_ms'],
            'new_faster_beyond_spread': t_new['max_ms'] < t_parent['min_ms'], 'bitwise_equal': same}


def end_to_end(N, n_bins, C, Tn, reps, warmup, subset=16):
    """2048 trials through SessionReplay.run against RealtimePipeline.run 8 at a time (timed on `subset`, scaled)."""
    from cross_patient_speech_decoding_amd.realtime_sim import RealtimePipeline, RealtimeRNNModel, SessionReplay
    dev = torch.device('cuda')
    torch.manual_seed(0)
    m = RealtimeRNNModel(14 * C, 128, 2, 11, dropout=0.0, win_size=14, stride=4).to(dev).eval()
    coefs = iir(8, 4)
    gen = torch.Generator(device=dev).manual_seed(2)
    raw = torch.randn(N, n_bins, C, Tn, dtype=torch.float64, device=dev, generator=gen) * 30.0
    sr = SessionReplay(m, coefs, C, Tn)
    t_new = timed(lambda: sr.run(raw), reps, warmup)
    pipe = RealtimePipeline(m, coefs, C, Tn, n_streams=8)

    def parent():
        for s0 in range(0, subset, 8):
            pipe.run(raw[s0:s0 + 8])
    t_sub = timed(parent, max(3, reps // 4), 1)
    scale = N / subset
    return {'session_replay_run': t_new, 'pipeline_run_subset': dict(t_sub, trials=subset),
            'pipeline_run_scaled_ms': t_sub['median_ms'] * scale, 'speedup': t_sub['median_ms'] * scale / t_new['median_ms']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--N', type=int, default=2048)
    ap.add_argument('--bins', type=int, default=50)
    ap.add_argument('--C', type=int, default=128)
    ap.add_argument('--Tn', type=int, default=40)
    ap.add_argument('--bands', type=int, default=8)
    ap.add_argument('--order', type=int, default=4)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--general', action='store_true', help='also time a general-path band count (bands - 1)')
    ap.add_argument('--end-to-end', action='store_true', help='also SessionReplay.run against RealtimePipeline.run')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_hg_trials needs the MI355X')
    out = {'tool': 'bench_hg_trials', 'frontend': frontends(a.N, a.bins, a.C, a.Tn, a.bands, a.order, a.reps, a.warmup)}
    if a.general:
        out['frontend_general'] = frontends(a.N, a.bins, a.C, a.Tn, a.bands - 1, a.order, a.reps, a.warmup)
    if a.end_to_end:
        out['end_to_end'] = end_to_end(a.N, a.bins, a.C, a.Tn, a.reps, a.warmup)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
