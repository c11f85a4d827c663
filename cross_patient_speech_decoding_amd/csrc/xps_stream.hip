// Batch-1 (few-stream) streaming inference kernels for the realtime decoder (BASELINE config 5).
// A 20 ms step touches every weight once and each weight is used by 1..8 streams only, so the step is
// bound by how fast the weights stream through (2.9 MB for the config-5 layer 0), not by FLOPs: one
// WAVE per output row, 16-byte loads along k, shuffle reduction — no LDS, no MFMA.  The GRU cell kernel
// needs no inter-workgroup exchange: hidden unit j depends only on its own rows of W_ih / W_hh and on
// the (shared, read-only) previous state, so one launch per layer suffices and the launches of a step
// are replayed from a hipGraph.
#include "xps_common.h"

namespace {

constexpr int MAXS = 8;   // streams per launch

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int SB>
__device__ inline void dot_rows(const float* __restrict__ wrow, const float* __restrict__ x, int K, int ldx, int lane,
                                float (&acc)[SB]) {
    // wrow: one weight row (K floats, 16-byte aligned when K % 4 == 0); x: SB input rows.
    // The FMAs are written out: left to the compiler, the contraction of w.x * v.x + w.y * v.y + ... came out differently for
    // the streams of one launch (the streams are packed in pairs and either product may be the rounded one) and for the
    // template widths, so a stream's bits depended on its row and on B.
    if ((K & 3) == 0) {
        for (int k = lane * 4; k < K; k += 256) {
            const float4 w = *reinterpret_cast<const float4*>(wrow + k);
#pragma unroll
            for (int s = 0; s < SB; ++s) {
                const float4 v = *reinterpret_cast<const float4*>(x + (long long)s * ldx + k);
                acc[s] += fmaf(w.w, v.w, fmaf(w.z, v.z, fmaf(w.y, v.y, w.x * v.x)));
            }
        }
    } else {
        for (int k = lane; k < K; k += 64) {
            const float w = wrow[k];
#pragma unroll
            for (int s = 0; s < SB; ++s) acc[s] = fmaf(w, x[(long long)s * ldx + k], acc[s]);
        }
    }
}

template <int SB>
__global__ __launch_bounds__(256) void gemv_kernel(const float* __restrict__ x, const float* __restrict__ W,
                                                   const float* __restrict__ bias, float* __restrict__ out,
                                                   int N, int K, int B) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    float acc[SB];
#pragma unroll
    for (int s = 0; s < SB; ++s) acc[s] = 0.f;
    dot_rows<SB>(W + (long long)row * K, x, K, K, lane, acc);
#pragma unroll
    for (int s = 0; s < SB; ++s) {
        const float v = wave_sum(acc[s]);
        if (lane == 0 && s < B) out[(long long)s * N + row] = v + (bias ? bias[row] : 0.f);
    }
}

template <int SB>
__global__ __launch_bounds__(256) void gru_cell_gemv_kernel(const float* __restrict__ x, int K,
                                                            const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                                                            const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                            const float* __restrict__ h_prev, float* __restrict__ h_new,
                                                            int H, int B) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= H) return;
    float gi[3][SB], gh[3][SB];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
#pragma unroll
        for (int s = 0; s < SB; ++s) { gi[g][s] = 0.f; gh[g][s] = 0.f; }
        dot_rows<SB>(w_ih + (long long)(g * H + j) * K, x, K, K, lane, gi[g]);
        dot_rows<SB>(w_hh + (long long)(g * H + j) * H, h_prev, H, H, lane, gh[g]);
    }
#pragma unroll
    for (int s = 0; s < SB; ++s) {
        float v[6];
#pragma unroll
        for (int g = 0; g < 3; ++g) { v[g] = wave_sum(gi[g][s]); v[3 + g] = wave_sum(gh[g][s]); }
        if (lane == 0 && s < B) {
            const float r = sigmoidf_acc(v[0] + b_ih[j] + v[3] + b_hh[j]);
            const float z = sigmoidf_acc(v[1] + b_ih[H + j] + v[4] + b_hh[H + j]);
            const float n = tanhf(fmaf(r, v[5] + b_hh[2 * H + j], v[2] + b_ih[2 * H + j]));
            const float hp = h_prev[(long long)s * H + j];
            h_new[(long long)s * H + j] = fmaf(z, hp - n, n);
        }
    }
}

}  // namespace

#define DISPATCH_SB(B, CALL)          \
    if ((B) <= 1) { CALL(1) }         \
    else if ((B) <= 2) { CALL(2) }    \
    else if ((B) <= 4) { CALL(4) }    \
    else { CALL(8) }

extern "C" int xps_gemv_f32(const float* x, const float* W, const float* bias, float* out, int N, int K, int B,
                            void* stream) {
    XPS_CHECK_ARG(x && W && out && N >= 1 && K >= 1, "bad argument");
    XPS_CHECK_ARG(B >= 1 && B <= MAXS, "1..8 streams per call");
    XPS_CHECK_ARG((K & 3) != 0 || (((uintptr_t)x | (uintptr_t)W) & 15) == 0, "x and W must be 16-byte aligned");
    // rows beyond B of x must be readable: callers pass buffers padded to the template width
#define CALL(S) hipLaunchKernelGGL(gemv_kernel<S>, dim3(cdiv(N, 4)), dim3(256), 0, (hipStream_t)stream, x, W, bias, out, N, K, B);
    DISPATCH_SB(B, CALL)
#undef CALL
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_gru_cell_gemv_f32(const float* x, int K, const float* w_ih, const float* w_hh, const float* b_ih,
                                     const float* b_hh, const float* h_prev, float* h_new, int H, int B, void* stream) {
    XPS_CHECK_ARG(x && w_ih && w_hh && b_ih && b_hh && h_prev && h_new && K >= 1 && H >= 1, "bad argument");
    XPS_CHECK_ARG(B >= 1 && B <= MAXS, "1..8 streams per call");
    XPS_CHECK_ARG(h_prev != h_new, "h_new must not alias h_prev (other workgroups still read it)");
    XPS_CHECK_ARG((K & 3) != 0 || (((uintptr_t)x | (uintptr_t)w_ih) & 15) == 0, "x and w_ih must be 16-byte aligned");
    XPS_CHECK_ARG((H & 3) != 0 || (((uintptr_t)h_prev | (uintptr_t)w_hh) & 15) == 0, "h and w_hh must be 16-byte aligned");
#define CALL(S) hipLaunchKernelGGL(gru_cell_gemv_kernel<S>, dim3(cdiv(H, 4)), dim3(256), 0, (hipStream_t)stream, x, K, w_ih, w_hh, b_ih, b_hh, h_prev, h_new, H, B);
    DISPATCH_SB(B, CALL)
#undef CALL
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

// ---- realtime pipeline glue (realtime_sim/realtime_pipeline.py) --------------------------------------------------------
namespace {

// dst[s] = src[s] shifted left by k frames, the k new frames float32(power[s][j] @ W[s] + c[s]) appended at the end.
// One thread per window element; src and dst are different buffers (ping-pong), so no workgroup reads what another
// writes.  W == NULL: identity (d == C), the frames are the cast powers.
__global__ __launch_bounds__(256) void window_shift_kernel(const double* __restrict__ power, int k, int C,
                                                           const double* __restrict__ W, const double* __restrict__ cvec,
                                                           const float* __restrict__ src, float* __restrict__ dst,
                                                           int win, int d) {
    const int s = blockIdx.y;
    const int K = win * d;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= K) return;
    const int f = q / d, e = q % d;
    float v;
    if (f < win - k) {
        v = src[(long long)s * K + q + k * d];
    } else {
        const double* p = power + ((long long)s * k + (f - (win - k))) * C;
        if (W) {
            const double* w = W + (long long)s * C * d + e;
            double acc = 0.0;
            for (int i = 0; i < C; ++i) acc += p[i] * w[(long long)i * d];
            if (cvec) acc += cvec[(long long)s * d + e];
            v = (float)acc;
        } else {
            v = (float)p[e];
        }
    }
    dst[(long long)s * K + q] = v;
}

// Online greedy CTC collapse, one thread per stream: a = first maximum of the logits (torch.argmax); a token is appended when
// a differs from the previous step's argmax and is not blank.  state[s] = {previous argmax (-1 before the first step),
// token count, overflow flag}; plain per-lane stores.
__global__ void ctc_collapse_kernel(const float* __restrict__ logits, int n_classes, int blank, long long* __restrict__ argmax,
                                    int* __restrict__ state, long long* __restrict__ tokens, int max_tokens, int B) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B) return;
    const float* p = logits + (long long)s * n_classes;
    float best = p[0];
    int bi = 0;
    for (int c = 1; c < n_classes; ++c)
        if (p[c] > best) { best = p[c]; bi = c; }
    argmax[s] = bi;
    int* st = state + 3 * s;
    const int prev = st[0];
    st[0] = bi;
    if (bi != prev && bi != blank) {
        const int n = st[1];
        if (n < max_tokens) {
            tokens[(long long)s * max_tokens + n] = bi;
            st[1] = n + 1;
        } else {
            st[2] = 1;
        }
    }
}

}  // namespace

extern "C" int xps_window_shift_f32(const double* power, int k, int C, const double* W, const double* c, const float* src,
                                    float* dst, int win, int d, int B, void* stream) {
    XPS_CHECK_ARG(power && src && dst && k >= 1 && C >= 1 && d >= 1 && win >= 1, "bad argument");
    XPS_CHECK_ARG(B >= 1 && B <= MAXS, "1..8 streams per call");
    XPS_CHECK_ARG(k <= win, "more new frames than the window holds");
    XPS_CHECK_ARG(W || d == C, "the identity map needs d == C");
    XPS_CHECK_ARG(src != dst, "dst must not alias src (other workgroups still read it)");
    hipLaunchKernelGGL(window_shift_kernel, dim3(cdiv((long long)win * d, 256), B), dim3(256), 0, (hipStream_t)stream,
                       power, k, C, W, c, src, dst, win, d);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_ctc_collapse_f32(const float* logits, int n_classes, int blank, int64_t* argmax, int32_t* state,
                                    int64_t* tokens, int max_tokens, int B, void* stream) {
    XPS_CHECK_ARG(logits && argmax && state && tokens && n_classes >= 1 && max_tokens >= 1, "bad argument");
    XPS_CHECK_ARG(B >= 1 && B <= MAXS, "1..8 streams per call");
    XPS_CHECK_ARG(blank >= 0 && blank < n_classes, "blank outside the classes");
    hipLaunchKernelGGL(ctc_collapse_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, logits, n_classes, blank,
                       (long long*)argmax, (int*)state, (long long*)tokens, max_tokens, B);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
