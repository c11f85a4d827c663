"""Per-prediction latency of the realtime pipeline (realtime_sim/realtime_pipeline.py) at the config-5 shape: 128 channels x
40 samples per bin, 8 IIR bands of order 4, win 14, stride 4, H 128, L 2, 11 classes; feature maps identity (d = 128) and
PCA -> CCA (d = 30); 1 and 4 streams.  Prints one JSON line.

  latency: the stride bins are written into pinned host memory, then H2D copy, graph replay, D2H of logits and token and a
           synchronise, per prediction (wall clock; median / p90 / p99 over --n predictions after --warmup).
  device:  time of the graph replay alone between two events (median), replayed back to back.

The reference's 2.06 ms per prediction (figure_analyses/supp/supp_fig_24.ipynb) was measured on other hardware and includes
its host-side transform: context only.

  --decoder beam --beam-size N: the pipeline also advances an N-wide CTC prefix beam search per prediction (one more
           launch); --streams 1,4,8 picks the stream counts.

    python tools/realtime_latency.py [--n 2000] [--warmup 200] [--decoder greedy|beam] [--beam-size 100] [--streams 1,4]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _coefs():
    import scipy.signal as signal
    out = []
    for k in range(8):
        b, a = signal.butter(4, [70 + 10 * k, 80 + 10 * k], btype='band', fs=2000)
        out.append(np.stack([a, b], axis=1))
    return np.stack(out)


def _pca_cca(C, d):
    from cross_patient_speech_decoding_amd.alignment import AlignCCA, PCA
    from cross_patient_speech_decoding_amd.realtime_sim import feature_map_from
    from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
    Xb_raw, yb = make_patient(1, 256, T=20, C=C)
    pca = PCA(n_components=d).fit(Xb_raw.reshape(-1, C))
    Xa, ya = make_patient(0, 256, T=20, C=d)
    cca = AlignCCA(return_space='b_to_a')
    cca.fit(Xa, pca.transform(Xb_raw), ya, yb)
    return feature_map_from(pca, cca)


def measure(d, n_streams, n, warmup, fmap, decoder='greedy', beam_size=100):
    from cross_patient_speech_decoding_amd.realtime_sim import RealtimePipeline, RealtimeRNNModel
    C, Tn, win, stride, H, L, ncls = 128, 40, 14, 4, 128, 2, 11
    torch.manual_seed(0)
    m = RealtimeRNNModel(win * d, H, L, ncls, dropout=0.0, win_size=win, stride=stride).cuda().eval()
    pipe = RealtimePipeline(m, _coefs(), C, Tn, n_streams=n_streams, feature_map=fmap, use_graph=True,
                            max_tokens=1 << 16, decoder=decoder, beam_size=beam_size, max_steps=warmup + n + 256)
    rng = np.random.default_rng(1)
    src = rng.standard_normal((64, n_streams, stride, C, Tn))
    bins = torch.empty(n_streams, stride, C, Tn, dtype=torch.float64).pin_memory()
    out_l = torch.empty(n_streams, ncls).pin_memory()
    out_t = torch.empty(n_streams, dtype=torch.int64).pin_memory()
    pipe.prime(rng.standard_normal((n_streams, win - stride, C, Tn)))
    lat = []
    for i in range(warmup + n):
        bins.numpy()[...] = src[i % 64]            # the new bins arrive in pinned host memory
        t0 = time.perf_counter()
        pipe.step(bins)
        out_l.copy_(pipe.logits, non_blocking=True)
        out_t.copy_(pipe.token, non_blocking=True)
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t0)
    lat = np.array(lat[warmup:]) * 1e6
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dev = []
    for i in range(200):
        ev[0].record()
        pipe.graphs[pipe.parity].replay()
        pipe.parity ^= 1
        ev[1].record()
        ev[1].synchronize()
        dev.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return {'d': d, 'streams': n_streams, 'n': int(len(lat)), 'latency_us_median': round(float(np.median(lat)), 1),
            'latency_us_p90': round(float(np.percentile(lat, 90)), 1),
            'latency_us_p99': round(float(np.percentile(lat, 99)), 1),
            'device_us_per_replay_median': round(float(np.median(dev[20:])), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=200)
    ap.add_argument('--decoder', choices=('greedy', 'beam'), default='greedy')
    ap.add_argument('--beam-size', type=int, default=100)
    ap.add_argument('--streams', default='1,4')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    maps = {128: None, 30: _pca_cca(128, 30)}
    streams = [int(v) for v in a.streams.split(',')]
    rows = [measure(d, s, a.n, a.warmup, maps[d], a.decoder, a.beam_size) for d in (128, 30) for s in streams]
    launches = 1 + 1 + 2 + 1 + 1               # frontend, map / shift, L = 2 GRU cells, classifier, collapse
    launches += a.decoder == 'beam'            # beam step
    print(json.dumps({'tool': 'realtime_latency', 'shape': 'config5 C128 Tn40 bands8 order4 win14 stride4 H128 L2 cls11',
                      'decoder': a.decoder, 'beam_size': a.beam_size if a.decoder == 'beam' else None,
                      'launches_per_prediction': launches, 'reference_ms_per_prediction': 2.06,
                      'reference_note': 'other hardware, includes the host transform: context only', 'rows': rows}))


if __name__ == '__main__':
    main()
