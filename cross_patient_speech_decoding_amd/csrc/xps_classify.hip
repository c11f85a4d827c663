// Single-label classifiers (TemporalConvRNN / TCN_classifier, reference nn_models/models.py:111-205, :393-448):
//   * max over time of a time-major (T, B, F) tensor with the index of the maximum, and its backward;
//   * the classification step in ONE launch: mean cross-entropy + gradient (the bits of xps_cross_entropy_loss_grad_f32),
//     confusion matrix of argmax against the target, accuracy = trace / rows.
#include "xps_ce.h"

namespace {

// ---- max over time ------------------------------------------------------------------------------------------------
// torch.max(x, dim)'s rule on the CPU: a NaN counts as the maximum; among equal maxima (and among NaNs) the FIRST index wins.
// `a` replaces `b` as the running maximum of a scan in increasing t:
__device__ inline bool tm_takes_over(float a, float b) { return a > b || (a != a && b == b); }
// the same order between two candidates with their indices, in any order (an index < 0: no candidate)
__device__ inline bool tm_better(float a, int ia, float b, int ib) {
    if (ib < 0) return ia >= 0;
    if (ia < 0) return false;
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ia < ib);
    return a > b || (a == b && ia < ib);
}

constexpr int TM_SLICES = 4;          // waves of a block: wave w scans t = w, w + 4, ... of the block's columns

// V adjacent floats in one access: 16 bytes where V = 4 (p 16-byte aligned), 4 bytes where V = 1
template <int V> __device__ inline void tm_load(const float* __restrict__ p, float (&x)[V]) {
    if constexpr (V == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
    } else {
        x[0] = *p;
    }
}
template <int V> __device__ inline void tm_store(float* __restrict__ p, const float (&x)[V]) {
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(p) = (f32x4){x[0], x[1], x[2], x[3]};
    else *p = x[0];
}

// One pass over z.  A block of 4 waves owns 64 * V adjacent columns n of the N = B * F (lanes along the contiguous axis: a
// wave reads 64 * V * 4 contiguous bytes per step, 16 bytes per lane where V = 4); wave w scans the steps t = w (mod 4), so a
// small B * F still puts 4 waves per 64 * V columns on the machine and keeps T / 4 independent loads per lane in flight.  The
// four slice results meet in LDS under the (value, index) order above.
template <int V>
__global__ __launch_bounds__(64 * TM_SLICES) void time_max_fwd_kernel(const float* __restrict__ z, float* __restrict__ out,
                                                                       int* __restrict__ arg, int T, long long N) {
    __shared__ float s_v[TM_SLICES - 1][V][64];        // [slice][j][lane]: a wave-instruction touches 64 adjacent words
    __shared__ int s_i[TM_SLICES - 1][V][64];          // (slice 0 keeps its candidates in registers)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long n0 = ((long long)blockIdx.x * 64 + lane) * V;
    const bool live = n0 < N;                       // V = 4: N % 4 == 0, so a live lane owns 4 valid columns
    float best[V];
    int bi[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { best[j] = 0.f; bi[j] = -1; }
    if (live && w < T) {
        const float* p = z + (long long)w * N + n0;
        tm_load<V>(p, best);
#pragma unroll
        for (int j = 0; j < V; ++j) bi[j] = w;
#pragma unroll 4
        for (int t = w + TM_SLICES; t < T; t += TM_SLICES) {
            p += (long long)TM_SLICES * N;
            float x[V];
            tm_load<V>(p, x);
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (tm_takes_over(x[j], best[j])) { best[j] = x[j]; bi[j] = t; }
        }
    }
    if (w > 0) {
#pragma unroll
        for (int j = 0; j < V; ++j) { s_v[w - 1][j][lane] = best[j]; s_i[w - 1][j][lane] = bi[j]; }
    }
    __syncthreads();
    if (w == 0 && live) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float b = best[j];
            int i = bi[j];
#pragma unroll
            for (int s = 1; s < TM_SLICES; ++s) {
                const float c = s_v[s - 1][j][lane];
                const int ci = s_i[s - 1][j][lane];
                if (tm_better(c, ci, b, i)) { b = c; i = ci; }
            }
            best[j] = b;
            bi[j] = i;
        }
        tm_store<V>(out + n0, best);
        if constexpr (V == 4) {
            typedef int i32x4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<i32x4*>(arg + n0) = (i32x4){bi[0], bi[1], bi[2], bi[3]};
        } else {
            arg[n0] = bi[0];
        }
    }
}

// dz[t][n] = dout[n] where t == arg[n], else 0: every element of dz is written exactly once (no memset, no atomics).
// Same decomposition as the forward: wave w writes the steps t = w (mod 4) of its block's columns.
template <int V>
__global__ __launch_bounds__(64 * TM_SLICES) void time_max_bwd_kernel(const float* __restrict__ dout, const int* __restrict__ arg,
                                                                       float* __restrict__ dz, int T, long long N) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long n0 = ((long long)blockIdx.x * 64 + lane) * V;
    if (n0 >= N) return;
    float g[V];
    int a[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { g[j] = dout[n0 + j]; a[j] = arg[n0 + j]; }
    float* p = dz + (long long)w * N + n0;
    for (int t = w; t < T; t += TM_SLICES) {
        float v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = (a[j] == t) ? g[j] : 0.f;
        tm_store<V>(p, v);
        p += (long long)TM_SLICES * N;
    }
}

// ---- classification step ------------------------------------------------------------------------------------------
// argmax of one row: the first maximum wins and a NaN counts as the maximum (torch.argmax)
__device__ inline int row_argmax(const float* __restrict__ p, int C) {
    float b = p[0];
    int bi = 0;
    for (int c = 1; c < C; ++c)
        if (tm_takes_over(p[c], b)) { b = p[c]; bi = c; }
    return bi;
}

// Every block: CE_BLOCK rows through ce_row (loss, gradient) and its loss partial to `part` (ce_block_sum_ticket): exactly the
// work of ce_loss_grad_kernel.  The block with the last ticket adds the partials in index order (the bits of that kernel),
// zeroes cmat, and makes the confusion pass itself: row_argmax of every row straight from `logits` -- an input, which no block
// writes, so nothing but the loss partials is handed from block to block -- counted into cmat with 64-bit vector atomics
// (integer adds: any order gives the same matrix; the prediction is in [0, C) by construction, the target is checked), the
// correct rows counted in LDS, acc = trace / rows.  That pass runs in one block: rows / 256 rows per thread, a batch's worth.
__global__ __launch_bounds__(CE_BLOCK) void classify_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                            float* __restrict__ row_loss, float* __restrict__ loss,
                                                            float* __restrict__ dlogits, long long* __restrict__ cmat,
                                                            float* __restrict__ acc, double* part, unsigned* ticket,
                                                            long long rows, int C) {
    __shared__ double sh[CE_BLOCK];
    __shared__ unsigned last;
    __shared__ unsigned long long trace;
    const long long r = (long long)blockIdx.x * CE_BLOCK + threadIdx.x;
    double l = 0.0;
    if (r < rows) {
        const float rl = ce_row(logits + r * C, target[r], C, rows, dlogits ? dlogits + r * C : nullptr);
        row_loss[r] = rl;
        l = (double)rl;
    }
    if (!ce_block_sum_ticket(l, sh, &last, part, ticket)) return;
    const long long cells = (long long)C * C;
    for (long long i = threadIdx.x; i < cells; i += CE_BLOCK) cmat[i] = 0;
    if (threadIdx.x == 0) trace = 0ull;
    __threadfence();                                            // the zeros reach L2 before any thread's atomics on them
    __syncthreads();
    unsigned long long mine = 0ull;
    for (long long i = threadIdx.x; i < rows; i += CE_BLOCK) {
        const long long tg = target[i];
        const int pr = row_argmax(logits + i * C, C);
        if (tg >= 0 && tg < C) {
            atomicAdd(reinterpret_cast<unsigned long long*>(cmat + tg * C + pr), 1ull);
            mine += (tg == pr) ? 1ull : 0ull;
        }
    }
    if (mine) atomicAdd(&trace, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        loss[0] = ce_mean_of_partials(part, rows);
        acc[0] = (float)trace / (float)rows;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call on this stream
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ticket (16-byte header) | part: blocks doubles -- the layout of xps_cross_entropy_loss_grad_f32's workspace
inline size_t classify_ws_bytes(long long rows) { return 16 + (size_t)cdiv(rows > 0 ? rows : 1, CE_BLOCK) * sizeof(double); }

}  // namespace

extern "C" int xps_time_max_fwd_f32(const float* z, float* out, int* arg, int T, int B, int F, void* stream) {
    XPS_CHECK_ARG(z && out && arg, "null argument");
    XPS_CHECK_ARG(T >= 1 && B >= 1 && F >= 1, "T, B and F must be positive");
    const long long N = (long long)B * F;
    if (F % 4 == 0 && aligned16(z) && aligned16(out) && aligned16(arg))
        hipLaunchKernelGGL(time_max_fwd_kernel<4>, dim3(cdiv(N / 4, 64)), dim3(64 * TM_SLICES), 0, (hipStream_t)stream, z, out, arg, T, N);
    else
        hipLaunchKernelGGL(time_max_fwd_kernel<1>, dim3(cdiv(N, 64)), dim3(64 * TM_SLICES), 0, (hipStream_t)stream, z, out, arg, T, N);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_time_max_bwd_f32(const float* dout, const int* arg, float* dz, int T, int B, int F, void* stream) {
    XPS_CHECK_ARG(dout && arg && dz, "null argument");
    XPS_CHECK_ARG(T >= 1 && B >= 1 && F >= 1, "T, B and F must be positive");
    const long long N = (long long)B * F;
    if (F % 4 == 0 && aligned16(dz))
        hipLaunchKernelGGL(time_max_bwd_kernel<4>, dim3(cdiv(N / 4, 64)), dim3(64 * TM_SLICES), 0, (hipStream_t)stream, dout, arg, dz, T, N);
    else
        hipLaunchKernelGGL(time_max_bwd_kernel<1>, dim3(cdiv(N, 64)), dim3(64 * TM_SLICES), 0, (hipStream_t)stream, dout, arg, dz, T, N);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" size_t xps_classify_loss_acc_f32_workspace(int64_t rows) { return classify_ws_bytes(rows); }

extern "C" int xps_classify_loss_acc_f32(const float* logits, const int64_t* target, float* row_loss, float* loss, float* dlogits,
                                         int64_t* cmat, float* acc, void* workspace, size_t workspace_bytes, int64_t rows,
                                         int n_classes, void* stream) {
    XPS_CHECK_ARG(logits && target && row_loss && loss && cmat && acc, "null argument");
    XPS_CHECK_ARG(rows >= 1 && n_classes >= 1, "rows and n_classes must be positive");
    if (!workspace || workspace_bytes < classify_ws_bytes(rows) || (reinterpret_cast<uintptr_t>(workspace) & 7)) {
        xps_set_error("xps_classify_loss_acc_f32: workspace too small or misaligned");
        return XPS_E_WORKSPACE;
    }
    unsigned* ticket = (unsigned*)workspace;              // FIRST word, as in xps_cross_entropy_loss_grad_f32: one zeroed buffer serves both
    double* part = (double*)workspace + 2;
    hipLaunchKernelGGL(classify_kernel, dim3(cdiv(rows, CE_BLOCK)), dim3(CE_BLOCK), 0, (hipStream_t)stream, logits, (const long long*)target,
                       row_loss, loss, dlogits, (long long*)cmat, acc, part, ticket, (long long)rows, n_classes);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
