// Cross-patient CTC training data on the device (reference realtime_sim/augmentations.py, realtime_sim/realtime_nn_model.py
// validation_step / calc_PER, realtime_sim/ctc_decoder.py greedy_decode_batch):
//   per-trial augmentations  one random draw PER TRIAL (device arrays made by the caller with the reference's generator calls),
//                            (N, T, C) fp32, single pass, coalesced along the channel index (16-byte vectors when C % 4 == 0);
//                            `out` is a plain pointer: a slab of the concatenated training tensor works
//     shift   out[n, t] = x[n, (t - shift[n]) mod T]                                   (bit-exact)
//     mask    [start[n], start[n] + size) along time zeroed                            (bit-exact)
//     scale   x[n] * scale[n], one fp32 multiply                                       (bit-exact)
//     warp    ATen upsample_linear1d (align_corners = False) T -> T2[n] -> T, fp32, fused: the intermediate row is never stored
//   greedy CTC decode        argmax per frame (first maximum, NaN = maximum like torch.argmax) -> collapse repeats -> drop
//                            blanks; one wave per sequence, frames across the lanes, compaction by ballot; one launch per batch
// The edit distance of the decoded batch (xps_edit_distance_i64) is the row pass of the edit-operation alignment and lives
// with it in xps_edit_align.hip.
#include "xps_common.h"

namespace {

inline int blocks_for(long long n) {
    long long b = (n + 255) / 256;
    return (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
}
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------------------
// per-trial shift / mask
template <bool V4>
__global__ __launch_bounds__(256) void trial_shift_mask_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int T, int C,
                                                               const long long* __restrict__ shift,
                                                               const long long* __restrict__ mstart, int msize) {
    // out[n, t, :] = (mstart[n] <= t < mstart[n] + msize) ? 0 : x[n, (t - shift[n]) mod T, :]   (NULL array: no shift / no mask)
    const int cw = V4 ? C / 4 : C;
    const long long total = (long long)N * T * cw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cw);
        const long long r = i / cw;
        const int t = (int)(r % T);
        const long long n = r / T;
        int ts = t;
        if (shift) {
            long long s = ((long long)t - shift[n]) % T;
            if (s < 0) s += T;
            ts = (int)s;
        }
        bool masked = false;
        if (mstart) {
            const long long m0 = mstart[n];
            masked = t >= m0 && t < m0 + msize;
        }
        if (V4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!masked) v = reinterpret_cast<const float4*>(x)[(n * T + ts) * cw + c];
            reinterpret_cast<float4*>(out)[i] = v;
        } else {
            out[i] = masked ? 0.f : x[(n * T + ts) * cw + c];
        }
    }
}

template <bool V4>
__global__ __launch_bounds__(256) void trial_scale_kernel(const float* __restrict__ x, float* __restrict__ out, long long N, long long row,
                                                          const float* __restrict__ scale) {
#pragma clang fp contract(off)
    const long long rw = V4 ? row / 4 : row;
    const long long total = N * rw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const float s = scale[i / rw];
        if (V4) {
            float4 v = reinterpret_cast<const float4*>(x)[i];
            v.x = __fmul_rn(v.x, s); v.y = __fmul_rn(v.y, s); v.z = __fmul_rn(v.z, s); v.w = __fmul_rn(v.w, s);
            reinterpret_cast<float4*>(out)[i] = v;
        } else {
            out[i] = __fmul_rn(x[i], s);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// per-trial warp.  ATen's upsample_linear1d, align_corners = False (area_pixel_compute_source_index + guard_index_and_lambda):
//   scale = float(in) / float(out); src = scale * (dst + 0.5f) - 0.5f, clamped at 0; i0 = min(int(src), in - 1);
//   i1 = i0 + (i0 < in - 1); w1 = clamp(src - i0, 0, 1); w0 = 1 - w1; value = v[i0] * w0 + v[i1] * w1
struct Tap { int i0, i1; float w0, w1; };
__device__ inline Tap linear_tap(float scale, int dst, int in) {
#pragma clang fp contract(off)
    // one rounding for scale * (dst + 0.5) - 0.5, as ATen's CPU kernels compute it (built with fused multiply-add): with two
    // roundings the coordinate is off by an ulp at T ~ 200, 3e-5 in the result
    float src = __fmaf_rn(scale, (float)dst + 0.5f, -0.5f);
    if (src < 0.f) src = 0.f;
    int i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    Tap p;
    p.i0 = i0;
    p.i1 = i0 + (i0 < in - 1 ? 1 : 0);
    float l = src - (float)i0;
    l = l < 0.f ? 0.f : (l > 1.f ? 1.f : l);
    p.w1 = l;
    p.w0 = 1.f - l;
    return p;
}

template <bool V4>
__global__ __launch_bounds__(256) void trial_warp_kernel(const float* __restrict__ x, float* __restrict__ out, int N, int T, int C,
                                                         const long long* __restrict__ T2s) {
#pragma clang fp contract(off)
    const int cw = V4 ? C / 4 : C;
    const long long total = (long long)N * T * cw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cw);
        const long long r = i / cw;
        const int t = (int)(r % T);
        const long long n = r / T;
        long long t2l = T2s[n];
        const int T2 = t2l < 1 ? 1 : (t2l > (1 << 24) ? (1 << 24) : (int)t2l);
        const Tap o = linear_tap((float)T2 / (float)T, t, T2);           // stage 2: T2 -> T, output sample t
        const float s1 = (float)T / (float)T2;                          // stage 1: T -> T2, intermediate samples o.i0, o.i1
        const Tap a = linear_tap(s1, o.i0, T), b = linear_tap(s1, o.i1, T);
        const long long base = n * T * cw + c;
        if (V4) {
            const float4* xv = reinterpret_cast<const float4*>(x);
            const float4 a0 = xv[base + (long long)a.i0 * cw], a1 = xv[base + (long long)a.i1 * cw];
            const float4 b0 = xv[base + (long long)b.i0 * cw], b1 = xv[base + (long long)b.i1 * cw];
            float4 v;
            v.x = (a0.x * a.w0 + a1.x * a.w1) * o.w0 + (b0.x * b.w0 + b1.x * b.w1) * o.w1;
            v.y = (a0.y * a.w0 + a1.y * a.w1) * o.w0 + (b0.y * b.w0 + b1.y * b.w1) * o.w1;
            v.z = (a0.z * a.w0 + a1.z * a.w1) * o.w0 + (b0.z * b.w0 + b1.z * b.w1) * o.w1;
            v.w = (a0.w * a.w0 + a1.w * a.w1) * o.w0 + (b0.w * b.w0 + b1.w * b.w1) * o.w1;
            reinterpret_cast<float4*>(out)[i] = v;
        } else {
            const float ma = x[base + (long long)a.i0 * cw] * a.w0 + x[base + (long long)a.i1 * cw] * a.w1;
            const float mb = x[base + (long long)b.i0 * cw] * b.w0 + x[base + (long long)b.i1 * cw] * b.w1;
            out[i] = ma * o.w0 + mb * o.w1;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// batched greedy CTC decode: one wave per sequence, 4 sequences per workgroup
template <typename TI>
__global__ __launch_bounds__(256) void greedy_decode_kernel(const TI* __restrict__ logits, long long stride_t, long long stride_b,
                                                            int T, int B, int C, int blank, long long* __restrict__ tokens,
                                                            long long* __restrict__ lengths) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;                                                  // whole wave leaves together
    const TI* seq = logits + (long long)b * stride_b;
    long long* row = tokens + (long long)b * T;
    int count = 0;
    int carry = -1;                                                      // argmax of the frame before this chunk
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        int best = -1;
        if (t < T) {
            const TI* f = seq + (long long)t * stride_t;
            TI bv = f[0];
            best = 0;
            for (int c = 1; c < C; ++c) {
                const TI v = f[c];
                if (v > bv || (v != v && bv == bv)) { bv = v; best = c; }   // first maximum; the first NaN wins (torch.argmax)
            }
        }
        int prev = __shfl_up(best, 1, 64);
        if (lane == 0) prev = carry;
        const bool keep = t < T && best != prev && best != blank;
        const unsigned long long m = __ballot(keep);
        if (keep) row[count + __popcll(m & ((1ull << lane) - 1ull))] = (long long)best;
        count += __popcll(m);
        carry = __shfl(best, 63, 64);
    }
    for (int t = count + lane; t < T; t += 64) row[t] = -1;
    if (lane == 0) lengths[b] = count;
}

}  // namespace

extern "C" int xps_aug_trial_shift_f32(const float* x, float* out, int N, int T, int C, const int64_t* shift, void* stream) {
    XPS_CHECK_ARG(N >= 0 && T >= 1 && C >= 1, "bad argument");
    XPS_CHECK_ARG(x && out && shift, "null argument");
    XPS_CHECK_ARG(x != out, "in-place roll is not supported");
    if (N == 0) return XPS_OK;
    const bool v4 = C % 4 == 0 && al16(x) && al16(out);
    const long long total = (long long)N * T * (v4 ? C / 4 : C);
    const long long* sh = reinterpret_cast<const long long*>(shift);
    if (v4) hipLaunchKernelGGL(trial_shift_mask_kernel<true>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, out, N, T, C, sh, (const long long*)nullptr, 0);
    else hipLaunchKernelGGL(trial_shift_mask_kernel<false>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, out, N, T, C, sh, (const long long*)nullptr, 0);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_aug_trial_mask_f32(const float* x, float* out, int N, int T, int C, const int64_t* start, int size, void* stream) {
    XPS_CHECK_ARG(N >= 0 && T >= 1 && C >= 1, "bad argument");
    XPS_CHECK_ARG(size >= 0 && size <= T, "mask window outside the sequence");
    XPS_CHECK_ARG(x && out && start, "null argument");
    if (N == 0) return XPS_OK;
    const bool v4 = C % 4 == 0 && al16(x) && al16(out);
    const long long total = (long long)N * T * (v4 ? C / 4 : C);
    const long long* st = reinterpret_cast<const long long*>(start);
    if (v4) hipLaunchKernelGGL(trial_shift_mask_kernel<true>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, out, N, T, C, (const long long*)nullptr, st, size);
    else hipLaunchKernelGGL(trial_shift_mask_kernel<false>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, out, N, T, C, (const long long*)nullptr, st, size);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_aug_trial_scale_f32(const float* x, float* out, int N, int64_t row_len, const float* scale, void* stream) {
    XPS_CHECK_ARG(N >= 0 && row_len >= 1, "bad argument");
    XPS_CHECK_ARG(x && out && scale, "null argument");
    if (N == 0) return XPS_OK;
    const bool v4 = row_len % 4 == 0 && al16(x) && al16(out);
    const long long total = (long long)N * (v4 ? row_len / 4 : row_len);
    if (v4) hipLaunchKernelGGL(trial_scale_kernel<true>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, out, (long long)N, (long long)row_len, scale);
    else hipLaunchKernelGGL(trial_scale_kernel<false>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, out, (long long)N, (long long)row_len, scale);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_aug_trial_warp_f32(const float* x, float* out, int N, int T, int C, const int64_t* T2, void* stream) {
    XPS_CHECK_ARG(N >= 0 && T >= 1 && C >= 1, "bad argument");
    XPS_CHECK_ARG(x && out && T2, "null argument");
    XPS_CHECK_ARG(x != out, "in-place warp is not supported");
    if (N == 0) return XPS_OK;
    const bool v4 = C % 4 == 0 && al16(x) && al16(out);
    const long long total = (long long)N * T * (v4 ? C / 4 : C);
    const long long* t2 = reinterpret_cast<const long long*>(T2);
    if (v4) hipLaunchKernelGGL(trial_warp_kernel<true>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, out, N, T, C, t2);
    else hipLaunchKernelGGL(trial_warp_kernel<false>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, x, out, N, T, C, t2);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_ctc_greedy_decode(const void* logits, int is_f32, int64_t stride_t, int64_t stride_b, int T, int B, int C,
                                     int blank, int64_t* tokens, int64_t* lengths, void* stream) {
    XPS_CHECK_ARG(T >= 0 && B >= 0 && C >= 1 && stride_t >= 0 && stride_b >= 0, "bad argument");
    XPS_CHECK_ARG(lengths || B == 0, "null argument");
    XPS_CHECK_ARG((logits && tokens) || B == 0 || T == 0, "null argument");
    if (B == 0) return XPS_OK;
    long long* tk = reinterpret_cast<long long*>(tokens);
    long long* ln = reinterpret_cast<long long*>(lengths);
    if (is_f32)
        hipLaunchKernelGGL(greedy_decode_kernel<float>, dim3(cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, (const float*)logits,
                           (long long)stride_t, (long long)stride_b, T, B, C, blank, tk, ln);
    else
        hipLaunchKernelGGL(greedy_decode_kernel<double>, dim3(cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, (const double*)logits,
                           (long long)stride_t, (long long)stride_b, T, B, C, blank, tk, ln);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
