"""Encoder-stack benchmark of the Transformer classifiers; sibling of tools/bench_classifier.py.

  stack      forward + backward of the encoder stack (3 layers, d_model 64, 8 heads, dim_fc 128, dropout 0.3, training) through
             the HIP kernels beside torch.nn.TransformerEncoder with the same weights, same device, same process, in
             interleaved rounds: B 2048 with S 200 (Transformer) and S 20 (CNNTransformer behind a kernel-10 stride-10 conv).
  kernels    each new kernel alone at those shapes (device events), with the FLOPs and bytes the algorithm needs and the
             share of the bound they give (fp32 vector peak 157.3 TFLOP/s, measured HBM copy rate 6.29 TB/s).

    python tools/bench_transformer.py [--rounds 7] [--B 2048]          prints one JSON line per result
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cross_patient_speech_decoding_amd.nn_models import functional as XF          # noqa: E402
from cross_patient_speech_decoding_amd.nn_models.models import _encoder_stack_tm, _make_encoder   # noqa: E402

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 6.29e12


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters          # ms


def bench_stack(B, S, rounds, iters, D=64, nh=8, dfc=128, L=3, p=0.3):
    torch.manual_seed(0)
    enc = _make_encoder(D, nh, dfc, p, L).cuda().train()
    x_bm = torch.randn(B, S, D, device='cuda')
    x_tm = x_bm.permute(1, 0, 2).contiguous()
    g_bm = torch.randn(B, S, D, device='cuda')
    g_tm = g_bm.permute(1, 0, 2).contiguous()

    def hip():
        enc.zero_grad(set_to_none=True)
        z = x_tm.detach().requires_grad_(True)
        _encoder_stack_tm(enc, z, True).backward(g_tm)

    def ref():
        enc.zero_grad(set_to_none=True)
        z = x_bm.detach().requires_grad_(True)
        enc(z).backward(g_bm)

    for fn in (hip, ref, hip, ref):                  # warm-up: code objects, allocator, library heuristics
        fn()
    torch.cuda.synchronize()
    t_hip, t_ref = [], []
    for _ in range(rounds):
        t_hip.append(timed(hip, iters))
        t_ref.append(timed(ref, iters))
    # same weights, dropout off: the two stacks compute the same function
    enc.eval()
    with torch.no_grad():
        a = _encoder_stack_tm(enc, x_tm[:, :64].contiguous(), False).permute(1, 0, 2)
        b = enc(x_bm[:64])
    return dict(what='stack_fwd_bwd', B=B, S=S, d_model=D, heads=nh, dim_fc=dfc, layers=L, dropout=p, iters=iters,
                hip_ms=t_hip, torch_ms=t_ref, hip_median_ms=statistics.median(t_hip), torch_median_ms=statistics.median(t_ref),
                torch_spread_ms=max(t_ref) - min(t_ref), hip_spread_ms=max(t_hip) - min(t_hip),
                eval_max_abs_diff=float((a - b).abs().max()))


def bench_kernels(B, S, rounds, iters, D=64, nh=8, dfc=128, p=0.3):
    dh, R = D // nh, S * B
    qkv = torch.randn(R, 3 * D, device='cuda', requires_grad=True)
    x = torch.randn(R, D, device='cuda', requires_grad=True)
    r = torch.randn(R, D, device='cuda', requires_grad=True)
    w, bias = torch.ones(D, device='cuda', requires_grad=True), torch.zeros(D, device='cuda', requires_grad=True)
    h = torch.randn(R, dfc, device='cuda', requires_grad=True)
    g = torch.randn(R, D, device='cuda')
    gh = torch.randn(R, dfc, device='cuda')
    out = []

    def report(name, fwd, cot, flops_f, bytes_f, flops_b, bytes_b):
        y = fwd()
        y.backward(cot)                              # warm-up of both directions
        tf = [timed(fwd, iters) for _ in range(rounds)]
        holder = {}

        def both():
            holder['y'] = fwd()
            holder['y'].backward(cot)
        tb = [timed(both, iters) for _ in range(rounds)]
        f_ms = statistics.median(tf)
        b_ms = max(statistics.median(tb) - f_ms, 1e-6)
        for tag, ms, fl, by in (('fwd', f_ms, flops_f, bytes_f), ('bwd', b_ms, flops_b, bytes_b)):
            bound_ms = 1e3 * max(fl / PEAK_FLOPS, by / PEAK_BYTES)
            out.append(dict(what='kernel', name=f'{name}_{tag}', B=B, S=S, ms=ms, flops=fl, bytes=by,
                            bound='flops' if fl / PEAK_FLOPS > by / PEAK_BYTES else 'bytes', bound_ms=bound_ms,
                            share_of_bound=bound_ms / ms, tflops=fl / ms / 1e9, gbytes_per_s=by / ms / 1e6))

    att = 4.0 * B * nh * S * S * dh                      # QK^T and PV, 2 FLOPs per multiply-add
    report('attention_p0.3', lambda: XF.self_attention(qkv, B, S, nh, p, True), g, att, 4.0 * R * 4 * D,
           2.5 * att, 4.0 * R * (3 * D + 2 * D + 3 * D))
    report('attention_p0', lambda: XF.self_attention(qkv, B, S, nh, 0.0, True), g, att, 4.0 * R * 4 * D,
           2.5 * att, 4.0 * R * (3 * D + 2 * D + 3 * D))
    report('add_layer_norm_p0.3', lambda: XF.add_layer_norm(x, r, w, bias, 1e-5, p, True), g, 8.0 * R * D, 4.0 * R * 3 * D,
           12.0 * R * D, 4.0 * R * 5 * D)
    report('relu_dropout_p0.3', lambda: XF.relu_dropout(h, p, True), gh, 2.0 * R * dfc, 4.0 * R * 2 * dfc, 1.0 * R * dfc,
           4.0 * R * 3 * dfc)
    z = torch.randn(S, B, D, device='cuda', requires_grad=True)
    report('time_mean', lambda: XF.time_mean(z), torch.randn(B, D, device='cuda'), 1.0 * R * D, 4.0 * (R * D + B * D),
           1.0 * R * D, 4.0 * (R * D + B * D))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--B', type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_transformer needs the GPU: there is no CPU fallback')
    for S, iters in ((200, 5), (20, 20)):
        print(json.dumps(bench_stack(args.B, S, args.rounds, iters)), flush=True)
        for row in bench_kernels(args.B, S, max(3, args.rounds // 2), iters):
            print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
