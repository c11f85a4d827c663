// Transformer encoder layer kernels (nn_models/models.py:451-597 of the reference: nn.TransformerEncoderLayer, post-norm, ReLU):
// fused multi-head self-attention forward / backward, residual add + LayerNorm forward / backward, ReLU + dropout, the
// positional-encoding add and the mean over time.  All fp32; activations are TIME-major rows (s, b).  DESIGN.md 4.13.
#include "xps_common.h"
#include <math.h>

namespace {

// keep decision of ONE element of a dropout site: element i is uniform (i & 1) of pair i >> 1 -- what dropout_keep4 /
// xps_dropout_f32 give the same flat index
__device__ inline float keep1(unsigned long long seed, long long i, float p) {
    float u0, u1;
    rng_pair(seed, i >> 1, u0, u1);
    return ((i & 1) ? u1 : u0) >= p ? 1.f : 0.f;
}

// keep factors (0 or dscale) of the N (even) consecutive elements i0 .. i0 + N - 1 of a site, one hash per two elements (+ one):
// an odd i0 shifts the pairs by one element, so the second uniform of a hash is carried to the next step
template <int N>
__device__ inline void keep_run(unsigned long long seed, long long i0, float p, float dscale, float (&kf)[N]) {
    const int e = (int)(i0 & 1);
    float u0, carry;
    rng_pair(seed, i0 >> 1, u0, carry);
#pragma unroll
    for (int jj = 0; jj < N; jj += 2) {
        float n0, n1;
        rng_pair(seed, (i0 + jj + e) >> 1, n0, n1);
        const float d0 = e ? carry : n0, d1 = e ? n0 : n1;
        carry = n1;
        kf[jj] = d0 >= p ? dscale : 0.f;
        kf[jj + 1] = d1 >= p ? dscale : 0.f;
    }
}

// keys per inner step: their K / V rows are in flight in registers together, 64 floats per lane
constexpr int attn_chunk(int dpl) { return dpl <= 4 ? 16 : 64 / dpl; }

template <int LPQ>
__device__ inline float group_sum(float v) {
#pragma unroll
    for (int o = 1; o < LPQ; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

template <int DPL>
__device__ inline float dot_lds(const float (&a)[DPL], const float* __restrict__ row) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < DPL; d += 4) {
        const f32x4 k = *reinterpret_cast<const f32x4*>(row + d);
        s = fmaf(a[d], k[0], s);
        s = fmaf(a[d + 1], k[1], s);
        s = fmaf(a[d + 2], k[2], s);
        s = fmaf(a[d + 3], k[3], s);
    }
    return s;
}

template <int DPL>
__device__ inline void axpy_lds(float (&acc)[DPL], float a, const float* __restrict__ row) {
#pragma unroll
    for (int d = 0; d < DPL; d += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + d);
        acc[d] = fmaf(a, v[0], acc[d]);
        acc[d + 1] = fmaf(a, v[1], acc[d + 1]);
        acc[d + 2] = fmaf(a, v[2], acc[d + 2]);
        acc[d + 3] = fmaf(a, v[3], acc[d + 3]);
    }
}

// Rows of qkv: row (s, b) at (s * B + b) * 3 D; q | k | v at column 0 | D | 2 D, head h at + h * dh.
// A [TILE][DHP] LDS image of column block `col` (head h of q, k or v, or of a D-wide tensor) of rows first .. first + TILE - 1 of
// one trial; zero beyond dh and beyond row S - 1; `mul` scales it.
template <int DHP, int TILE>
__device__ inline void stage_rows(float* __restrict__ dst, const float* __restrict__ src, long long ld, int col, int first, int S, int B,
                                  int b, int dh, float mul) {
    for (int i = threadIdx.x; i < TILE * DHP; i += blockDim.x) {
        const int j = i / DHP, d = i % DHP, row = first + j;
        float v = 0.f;
        if (row < S && d < dh) v = src[((long long)row * B + b) * ld + col + d] * mul;
        dst[i] = v;
    }
}

// ---- forward --------------------------------------------------------------------------------------------------------------
// One workgroup: one (trial, head) and blockDim / LPQ queries; LPQ adjacent lanes share a query, each holds DPL of the head's
// dimensions (q, accumulator) in registers.  Keys and values stream through LDS in tiles of TILE keys, CH scores at a time:
// online softmax (running maximum m, running sum l, accumulator rescaled once per CH keys).  lse = m + log l.
template <int DPL, int LPQ, int TILE>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ ctx, float* __restrict__ lse,
                                                       int B, int S, int nh, int dh, float scale, float p, float dscale,
                                                       unsigned long long seed) {
    constexpr int DHP = DPL * LPQ, CH = attn_chunk(DPL);
    __shared__ __attribute__((aligned(16))) float Ks[TILE * DHP];
    __shared__ __attribute__((aligned(16))) float Vs[TILE * DHP];
    const int bh = blockIdx.x, b = bh / nh, h = bh % nh, D = nh * dh;
    const long long ld = 3LL * D;
    const int qpb = blockDim.x / LPQ, lp = threadIdx.x % LPQ;
    int qi = blockIdx.y * qpb + threadIdx.x / LPQ;
    const bool valid = qi < S;
    if (!valid) qi = S - 1;                                   // idle lanes redo the last query (they take part in shuffles and barriers)
    const float* qrow = qkv + ((long long)qi * B + b) * ld + h * dh;
    float q[DPL], acc[DPL];
#pragma unroll
    for (int d = 0; d < DPL; ++d) {
        const int dd = lp * DPL + d;
        q[d] = dd < dh ? qrow[dd] * scale : 0.f;
        acc[d] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    const long long rowbase = ((long long)bh * S + qi) * S;   // dropout index ((b nh + h) S + q) S + k
    for (int k0 = 0; k0 < S; k0 += TILE) {
        __syncthreads();
        stage_rows<DHP, TILE>(Ks, qkv, ld, D + h * dh, k0, S, B, b, dh, 1.f);
        stage_rows<DHP, TILE>(Vs, qkv, ld, 2 * D + h * dh, k0, S, B, b, dh, 1.f);
        __syncthreads();
        const int nk = min(TILE, S - k0);
        for (int c = 0; c < nk; c += CH) {
            float s[CH];
#pragma unroll
            for (int jj = 0; jj < CH; ++jj) s[jj] = group_sum<LPQ>(dot_lds<DPL>(q, Ks + (c + jj) * DHP + lp * DPL));
            float cm = -INFINITY;
#pragma unroll
            for (int jj = 0; jj < CH; ++jj) {
                if (c + jj >= nk) s[jj] = -INFINITY;
                cm = fmaxf(cm, s[jj]);
            }
            const float mnew = fmaxf(m, cm);                  // finite: key c < nk exists
            const float alpha = __expf(m - mnew);             // m = -inf at the first chunk: 0
            l *= alpha;
#pragma unroll
            for (int d = 0; d < DPL; ++d) acc[d] *= alpha;
            float kf[CH];
            if (p > 0.f) keep_run<CH>(seed, rowbase + k0 + c, p, dscale, kf);
#pragma unroll
            for (int jj = 0; jj < CH; ++jj) {
                const float pr = __expf(s[jj] - mnew);        // masked keys: exp(-inf) = 0
                l += pr;
                axpy_lds<DPL>(acc, p > 0.f ? pr * kf[jj] : pr, Vs + (c + jj) * DHP + lp * DPL);
            }
            m = mnew;
        }
    }
    if (valid) {
        const float inv = 1.0f / l;
        float* orow = ctx + ((long long)qi * B + b) * D + h * dh;
#pragma unroll
        for (int d = 0; d < DPL; ++d) {
            const int dd = lp * DPL + d;
            if (dd < dh) orow[dd] = acc[d] * inv;
        }
        if (lp == 0) lse[(long long)bh * S + qi] = m + logf(l);
    }
}

// ---- backward, query side: dq and delta = dO . O --------------------------------------------------------------------------
// Same mapping as the forward.  p = exp(s - lse), ds = p (keep / (1 - p_drop) dO.v - delta), dq = scale sum_k ds k.
template <int DPL, int LPQ, int TILE>
__global__ __launch_bounds__(256) void attn_bwd_q_kernel(const float* __restrict__ dctx, const float* __restrict__ qkv,
                                                         const float* __restrict__ ctx, const float* __restrict__ lse,
                                                         float* __restrict__ dqkv, float* __restrict__ delta_out, int B, int S, int nh,
                                                         int dh, float scale, float p, float dscale, unsigned long long seed) {
    constexpr int DHP = DPL * LPQ, CH = attn_chunk(DPL);
    __shared__ __attribute__((aligned(16))) float Ks[TILE * DHP];
    __shared__ __attribute__((aligned(16))) float Vs[TILE * DHP];
    const int bh = blockIdx.x, b = bh / nh, h = bh % nh, D = nh * dh;
    const long long ld = 3LL * D;
    const int qpb = blockDim.x / LPQ, lp = threadIdx.x % LPQ;
    int qi = blockIdx.y * qpb + threadIdx.x / LPQ;
    const bool valid = qi < S;
    if (!valid) qi = S - 1;
    const long long r = (long long)qi * B + b;
    float q[DPL], dO[DPL], dq[DPL];
    float dl = 0.f;
#pragma unroll
    for (int d = 0; d < DPL; ++d) {
        const int dd = lp * DPL + d;
        const bool in = dd < dh;
        q[d] = in ? qkv[r * ld + h * dh + dd] * scale : 0.f;
        dO[d] = in ? dctx[r * D + h * dh + dd] : 0.f;
        dl = fmaf(dO[d], in ? ctx[r * D + h * dh + dd] : 0.f, dl);
        dq[d] = 0.f;
    }
    const float delta = group_sum<LPQ>(dl);
    const float ls = lse[(long long)bh * S + qi];
    const long long rowbase = ((long long)bh * S + qi) * S;
    for (int k0 = 0; k0 < S; k0 += TILE) {
        __syncthreads();
        stage_rows<DHP, TILE>(Ks, qkv, ld, D + h * dh, k0, S, B, b, dh, 1.f);
        stage_rows<DHP, TILE>(Vs, qkv, ld, 2 * D + h * dh, k0, S, B, b, dh, 1.f);
        __syncthreads();
        const int nk = min(TILE, S - k0);
        for (int c = 0; c < nk; c += CH) {
            float kf[CH];
            if (p > 0.f) keep_run<CH>(seed, rowbase + k0 + c, p, dscale, kf);
#pragma unroll
            for (int jj = 0; jj < CH; ++jj) {
                const float* kr = Ks + (c + jj) * DHP + lp * DPL;
                const float s = group_sum<LPQ>(dot_lds<DPL>(q, kr));
                const float dpv = group_sum<LPQ>(dot_lds<DPL>(dO, Vs + (c + jj) * DHP + lp * DPL));
                float ds = 0.f;
                if (c + jj < nk) ds = __expf(s - ls) * ((p > 0.f ? kf[jj] * dpv : dpv) - delta);
                axpy_lds<DPL>(dq, ds, kr);
            }
        }
    }
    if (valid) {
#pragma unroll
        for (int d = 0; d < DPL; ++d) {
            const int dd = lp * DPL + d;
            if (dd < dh) dqkv[r * ld + h * dh + dd] = dq[d] * scale;
        }
        if (lp == 0) delta_out[(long long)bh * S + qi] = delta;
    }
}

// ---- backward, key side: dk and dv ----------------------------------------------------------------------------------------
// One thread group per KEY; queries (scaled q, dO, lse, delta) stream through LDS in tiles.  Every sum runs over the queries in
// index order inside one thread: no atomics, the same bits every run.
template <int DPL, int LPQ, int TILE>
__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(const float* __restrict__ dctx, const float* __restrict__ qkv,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          float* __restrict__ dqkv, int B, int S, int nh, int dh, float scale, float p,
                                                          float dscale, unsigned long long seed) {
    constexpr int DHP = DPL * LPQ;
    __shared__ __attribute__((aligned(16))) float Qs[TILE * DHP];
    __shared__ __attribute__((aligned(16))) float Os[TILE * DHP];
    __shared__ float Ls[TILE], Ds[TILE];
    const int bh = blockIdx.x, b = bh / nh, h = bh % nh, D = nh * dh;
    const long long ld = 3LL * D;
    const int kpb = blockDim.x / LPQ, lp = threadIdx.x % LPQ;
    int ki = blockIdx.y * kpb + threadIdx.x / LPQ;
    const bool valid = ki < S;
    if (!valid) ki = S - 1;
    const long long r = (long long)ki * B + b;
    float k[DPL], v[DPL], dk[DPL], dv[DPL];
#pragma unroll
    for (int d = 0; d < DPL; ++d) {
        const int dd = lp * DPL + d;
        const bool in = dd < dh;
        k[d] = in ? qkv[r * ld + D + h * dh + dd] : 0.f;
        v[d] = in ? qkv[r * ld + 2 * D + h * dh + dd] : 0.f;
        dk[d] = dv[d] = 0.f;
    }
    for (int q0 = 0; q0 < S; q0 += TILE) {
        __syncthreads();
        stage_rows<DHP, TILE>(Qs, qkv, ld, h * dh, q0, S, B, b, dh, scale);
        stage_rows<DHP, TILE>(Os, dctx, D, h * dh, q0, S, B, b, dh, 1.f);
        for (int i = threadIdx.x; i < TILE; i += blockDim.x) {
            const bool in = q0 + i < S;
            Ls[i] = in ? lse[(long long)bh * S + q0 + i] : 0.f;
            Ds[i] = in ? delta[(long long)bh * S + q0 + i] : 0.f;
        }
        __syncthreads();
        const int nq = min(TILE, S - q0);
        for (int j = 0; j < nq; ++j) {
            const float* qr = Qs + j * DHP + lp * DPL;
            const float* orow = Os + j * DHP + lp * DPL;
            const float s = group_sum<LPQ>(dot_lds<DPL>(k, qr));
            const float dpv = group_sum<LPQ>(dot_lds<DPL>(v, orow));
            const float pr = __expf(s - Ls[j]);
            float kf = 1.f;
            if (p > 0.f) kf = keep1(seed, ((long long)bh * S + q0 + j) * S + ki, p) * dscale;
            axpy_lds<DPL>(dv, pr * kf, orow);
            axpy_lds<DPL>(dk, pr * (kf * dpv - Ds[j]), qr);
        }
    }
    if (valid) {
#pragma unroll
        for (int d = 0; d < DPL; ++d) {
            const int dd = lp * DPL + d;
            if (dd < dh) {
                dqkv[r * ld + D + h * dh + dd] = dk[d];
                dqkv[r * ld + 2 * D + h * dh + dd] = dv[d];
            }
        }
    }
}

// head dimension -> (dimensions per lane, lanes per query, key tile)
#define ATTN_DISPATCH(dh, CALL)                  \
    do {                                         \
        if ((dh) <= 4) { CALL(4, 1, 64); }       \
        else if ((dh) <= 8) { CALL(8, 1, 64); }  \
        else if ((dh) <= 16) { CALL(16, 1, 64); } \
        else if ((dh) <= 32) { CALL(32, 1, 64); } \
        else if ((dh) <= 64) { CALL(32, 2, 64); } \
        else { CALL(32, 4, 32); }                \
    } while (0)

inline int attn_lpq(int dh) { return dh <= 32 ? 1 : (dh <= 64 ? 2 : 4); }
inline int attn_threads(int S, int dh) {
    const long long want = ((long long)S * attn_lpq(dh) + 63) / 64 * 64;
    return (int)(want < 256 ? want : 256);
}
inline bool attn_shape_ok(int B, int S, int nh, int dh) {
    if (B < 1 || S < 1 || nh < 1 || dh < 1 || dh > 128) return false;
    if ((long long)B * nh > 0x7fffffffLL || (long long)nh * dh > (1 << 20)) return false;
    const int qpb = attn_threads(S, dh) / attn_lpq(dh);
    return cdiv(S, qpb) <= 65535;
}

// ---- residual add + LayerNorm ---------------------------------------------------------------------------------------------
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

constexpr int LN_WAVES = 4;
constexpr int LN_MAX_D = 1024;
constexpr int LN_MAX_BLOCKS = 512;

// One wave per row.  The row is d = (x - x[0]) + (r' - r'[0]), r' = dropout(r): LayerNorm does not see a shift of its row, and
// the differences are exact where the row's offset is large against its spread.  Two passes over d held in LDS: mean, then the
// sum of (d - mean)^2.  mean_out is the mean of d.
__global__ __launch_bounds__(64 * LN_WAVES) void add_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ rr,
                                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   float* __restrict__ y, float* __restrict__ mean_out,
                                                                   float* __restrict__ rstd_out, long long rows, int D, float eps, float p,
                                                                   float dscale, unsigned long long seed) {
    extern __shared__ __attribute__((aligned(16))) float ln_smem[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* st = ln_smem + (size_t)w * D;
    for (long long row = (long long)blockIdx.x * LN_WAVES + w; row < rows; row += (long long)gridDim.x * LN_WAVES) {
        const float* xr = x + row * D;
        const float* rp = rr + row * D;
        const float x0 = xr[0];
        const float r0 = p > 0.f ? rp[0] * keep1(seed, row * D, p) * dscale : rp[0];
        float sum = 0.f;
        for (int c = lane; c < D; c += 64) {
            const float rv = p > 0.f ? rp[c] * keep1(seed, row * D + c, p) * dscale : rp[c];
            const float d = (xr[c] - x0) + (rv - r0);
            st[c] = d;
            sum += d;
        }
        const float mean = wave_sum(sum) / (float)D;
        float ss = 0.f;
        for (int c = lane; c < D; c += 64) {
            const float t = st[c] - mean;
            ss = fmaf(t, t, ss);
        }
        const float rstd = 1.0f / sqrtf(wave_sum(ss) / (float)D + eps);
        for (int c = lane; c < D; c += 64) y[row * D + c] = (st[c] - mean) * rstd * gamma[c] + beta[c];
        if (lane == 0) {
            mean_out[row] = mean;
            rstd_out[row] = rstd;
        }
    }
}

// dv = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma; dx = dv, dr = dv keep / (1 - p).  dgamma / dbeta: each wave adds
// its rows (in row order) into its own LDS row, the block's four waves are added in wave order into part[block], and
// add_ln_bwd_finish adds the blocks in block order.
__global__ __launch_bounds__(64 * LN_WAVES) void add_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                   const float* __restrict__ rr, const float* __restrict__ gamma,
                                                                   const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
                                                                   float* __restrict__ dx, float* __restrict__ dr, float* __restrict__ part,
                                                                   long long rows, int D, float p, float dscale, unsigned long long seed) {
    extern __shared__ __attribute__((aligned(16))) float ln_smem[];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* xh = ln_smem + (size_t)w * D;
    float* gs = ln_smem + (size_t)(LN_WAVES + w) * D;
    float* pg = ln_smem + (size_t)(2 * LN_WAVES + w) * D;
    float* pb = ln_smem + (size_t)(3 * LN_WAVES + w) * D;
    for (int c = lane; c < D; c += 64) pg[c] = pb[c] = 0.f;
    for (long long row = (long long)blockIdx.x * LN_WAVES + w; row < rows; row += (long long)gridDim.x * LN_WAVES) {
        const float* xr = x + row * D;
        const float* rp = rr + row * D;
        const float x0 = xr[0];
        const float r0 = p > 0.f ? rp[0] * keep1(seed, row * D, p) * dscale : rp[0];
        const float mean = mean_in[row], rstd = rstd_in[row];
        float s1 = 0.f, s2 = 0.f;
        for (int c = lane; c < D; c += 64) {
            const float rv = p > 0.f ? rp[c] * keep1(seed, row * D + c, p) * dscale : rp[c];
            const float xhat = (((xr[c] - x0) + (rv - r0)) - mean) * rstd;
            const float dyv = dy[row * D + c];
            const float g = dyv * gamma[c];
            xh[c] = xhat;
            gs[c] = g;
            s1 += g;
            s2 = fmaf(g, xhat, s2);
            pb[c] += dyv;
            pg[c] = fmaf(dyv, xhat, pg[c]);
        }
        s1 = wave_sum(s1) / (float)D;
        s2 = wave_sum(s2) / (float)D;
        for (int c = lane; c < D; c += 64) {
            const float dv = rstd * (gs[c] - s1 - xh[c] * s2);
            dx[row * D + c] = dv;
            if (p > 0.f) dr[row * D + c] = dv * keep1(seed, row * D + c, p) * dscale;
            else if (dr != dx) dr[row * D + c] = dv;
        }
    }
    __syncthreads();
    float* out = part + (size_t)blockIdx.x * 2 * D;
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        float a = 0.f, bsum = 0.f;
        for (int ww = 0; ww < LN_WAVES; ++ww) {
            a += ln_smem[(size_t)(2 * LN_WAVES + ww) * D + c];
            bsum += ln_smem[(size_t)(3 * LN_WAVES + ww) * D + c];
        }
        out[c] = a;
        out[D + c] = bsum;
    }
}

__global__ void add_ln_bwd_finish(const float* __restrict__ part, int blocks, int D, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= D) return;
    float a = 0.f, b = 0.f;
    for (int i = 0; i < blocks; ++i) {
        a += part[(size_t)i * 2 * D + c];
        b += part[(size_t)i * 2 * D + D + c];
    }
    dgamma[c] = a;
    dbeta[c] = b;
}

inline int ln_blocks(long long rows) {
    const long long g = (rows + LN_WAVES - 1) / LN_WAVES;
    return (int)(g < 1 ? 1 : (g > LN_MAX_BLOCKS ? LN_MAX_BLOCKS : g));
}

// ---- element kernels --------------------------------------------------------------------------------------------------------
__global__ void relu_dropout_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, long long n, float p, float dscale,
                                        unsigned long long seed) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float v = fmaxf(x[i], 0.f);
        if (p > 0.f) v = v * keep1(seed, i, p) * dscale;
        out[i] = v;
    }
}

// out > 0 exactly where the input was positive AND kept: the saved output is the gate
__global__ void relu_dropout_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out, float* __restrict__ dx, long long n,
                                        float dscale) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dx[i] = out[i] > 0.f ? dout[i] * dscale : 0.f;
}

// out [S][B][D] = z + table[s]; z is [S][B][D] (batch_major = 0) or [B][S][D] (1)
__global__ void add_positional_kernel(const float* __restrict__ z, const float* __restrict__ table, float* __restrict__ out, int S, int B,
                                      int D, int batch_major) {
    const long long n = (long long)S * B * D;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int d = (int)(i % D);
        const long long sb = i / D;
        const int b = (int)(sb % B), s = (int)(sb / B);
        const long long src = batch_major ? ((long long)b * S + s) * D + d : i;
        out[i] = z[src] + table[(long long)s * D + d];
    }
}

// out [N] = (sum over t in order of z[t][n]) / T
__global__ void time_mean_fwd_kernel(const float* __restrict__ z, float* __restrict__ out, int T, long long N) {
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += z[(long long)t * N + n];
    out[n] = s / (float)T;
}

__global__ void time_mean_bwd_kernel(const float* __restrict__ dout, float* __restrict__ dz, int T, long long N) {
    const long long total = (long long)T * N;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        dz[i] = dout[i % N] / (float)T;
}

inline int ew_blocks(long long n) {
    const long long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

extern "C" int xps_attention_supported(int B, int S, int n_head, int dh) { return attn_shape_ok(B, S, n_head, dh) ? 1 : 0; }

extern "C" int xps_attention_fwd_f32(const float* qkv, float* ctx, float* lse, int B, int S, int n_head, int dh, float p, uint64_t seed,
                                     void* stream) {
    XPS_CHECK_ARG(qkv && ctx && lse, "null argument");
    XPS_CHECK_ARG(attn_shape_ok(B, S, n_head, dh), "unsupported shape (B, S, n_head >= 1, 1 <= dh <= 128)");
    XPS_CHECK_ARG(p >= 0.f && p < 1.f, "p must be in [0, 1)");
    const int threads = attn_threads(S, dh), qpb = threads / attn_lpq(dh);
    const dim3 grid(B * n_head, cdiv(S, qpb));
    const float scale = 1.0f / sqrtf((float)dh), dscale = 1.0f / (1.0f - p);
#define XPS_ATTN_FWD(DPL, LPQ, TILE)                                                                                                \
    hipLaunchKernelGGL((attn_fwd_kernel<DPL, LPQ, TILE>), grid, dim3(threads), 0, (hipStream_t)stream, qkv, ctx, lse, B, S, n_head, dh, \
                       scale, p, dscale, (unsigned long long)seed)
    ATTN_DISPATCH(dh, XPS_ATTN_FWD);
#undef XPS_ATTN_FWD
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" size_t xps_attention_bwd_f32_workspace(int B, int S, int n_head, int dh) {
    if (!attn_shape_ok(B, S, n_head, dh)) return 16;
    return (size_t)B * n_head * S * sizeof(float) + 16;
}

extern "C" int xps_attention_bwd_f32(const float* dctx, const float* qkv, const float* ctx, const float* lse, float* dqkv, int B, int S,
                                     int n_head, int dh, float p, uint64_t seed, void* workspace, size_t workspace_bytes, void* stream) {
    XPS_CHECK_ARG(dctx && qkv && ctx && lse && dqkv, "null argument");
    XPS_CHECK_ARG(attn_shape_ok(B, S, n_head, dh), "unsupported shape (B, S, n_head >= 1, 1 <= dh <= 128)");
    XPS_CHECK_ARG(p >= 0.f && p < 1.f, "p must be in [0, 1)");
    if (!workspace || workspace_bytes < xps_attention_bwd_f32_workspace(B, S, n_head, dh) || (reinterpret_cast<uintptr_t>(workspace) & 3)) {
        xps_set_error("xps_attention_bwd_f32: workspace too small or misaligned");
        return XPS_E_WORKSPACE;
    }
    float* delta = (float*)workspace;
    const int threads = attn_threads(S, dh), qpb = threads / attn_lpq(dh);
    const dim3 grid(B * n_head, cdiv(S, qpb));
    const float scale = 1.0f / sqrtf((float)dh), dscale = 1.0f / (1.0f - p);
#define XPS_ATTN_BWD_Q(DPL, LPQ, TILE)                                                                                                   \
    hipLaunchKernelGGL((attn_bwd_q_kernel<DPL, LPQ, TILE>), grid, dim3(threads), 0, (hipStream_t)stream, dctx, qkv, ctx, lse, dqkv, delta, \
                       B, S, n_head, dh, scale, p, dscale, (unsigned long long)seed)
    ATTN_DISPATCH(dh, XPS_ATTN_BWD_Q);
#undef XPS_ATTN_BWD_Q
    XPS_CHECK_LAUNCH();
#define XPS_ATTN_BWD_KV(DPL, LPQ, TILE)                                                                                                \
    hipLaunchKernelGGL((attn_bwd_kv_kernel<DPL, LPQ, TILE>), grid, dim3(threads), 0, (hipStream_t)stream, dctx, qkv, lse, delta, dqkv, B, \
                       S, n_head, dh, scale, p, dscale, (unsigned long long)seed)
    ATTN_DISPATCH(dh, XPS_ATTN_BWD_KV);
#undef XPS_ATTN_BWD_KV
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_add_layer_norm_fwd_f32(const float* x, const float* r, const float* gamma, const float* beta, float* y, float* mean,
                                          float* rstd, int64_t rows, int D, float eps, float p, uint64_t seed, void* stream) {
    XPS_CHECK_ARG(x && r && gamma && beta && y && mean && rstd, "null argument");
    XPS_CHECK_ARG(rows >= 1 && D >= 1 && D <= LN_MAX_D, "rows >= 1 and 1 <= D <= 1024");
    XPS_CHECK_ARG(p >= 0.f && p < 1.f && eps > 0.f, "p must be in [0, 1), eps positive");
    hipLaunchKernelGGL(add_ln_fwd_kernel, dim3(ln_blocks(rows)), dim3(64 * LN_WAVES), (size_t)LN_WAVES * D * sizeof(float),
                       (hipStream_t)stream, x, r, gamma, beta, y, mean, rstd, (long long)rows, D, eps, p, 1.0f / (1.0f - p),
                       (unsigned long long)seed);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" size_t xps_add_layer_norm_bwd_f32_workspace(int64_t rows, int D) {
    if (rows < 1 || D < 1) return 16;
    return (size_t)ln_blocks(rows) * 2 * D * sizeof(float) + 16;
}

extern "C" int xps_add_layer_norm_bwd_f32(const float* dy, const float* x, const float* r, const float* gamma, const float* mean,
                                          const float* rstd, float* dx, float* dr, float* dgamma, float* dbeta, int64_t rows, int D,
                                          float p, uint64_t seed, void* workspace, size_t workspace_bytes, void* stream) {
    XPS_CHECK_ARG(dy && x && r && gamma && mean && rstd && dx && dr && dgamma && dbeta, "null argument");
    XPS_CHECK_ARG(rows >= 1 && D >= 1 && D <= LN_MAX_D, "rows >= 1 and 1 <= D <= 1024");
    XPS_CHECK_ARG(p >= 0.f && p < 1.f, "p must be in [0, 1)");
    XPS_CHECK_ARG(p == 0.f || dr != dx, "with dropout dx and dr differ: two buffers");
    if (!workspace || workspace_bytes < xps_add_layer_norm_bwd_f32_workspace(rows, D) || (reinterpret_cast<uintptr_t>(workspace) & 3)) {
        xps_set_error("xps_add_layer_norm_bwd_f32: workspace too small or misaligned");
        return XPS_E_WORKSPACE;
    }
    const int blocks = ln_blocks(rows);
    hipLaunchKernelGGL(add_ln_bwd_kernel, dim3(blocks), dim3(64 * LN_WAVES), (size_t)4 * LN_WAVES * D * sizeof(float), (hipStream_t)stream,
                       dy, x, r, gamma, mean, rstd, dx, dr, (float*)workspace, (long long)rows, D, p, 1.0f / (1.0f - p),
                       (unsigned long long)seed);
    XPS_CHECK_LAUNCH();
    hipLaunchKernelGGL(add_ln_bwd_finish, dim3(cdiv(D, 64)), dim3(64), 0, (hipStream_t)stream, (const float*)workspace, blocks, D, dgamma,
                       dbeta);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_relu_dropout_fwd_f32(const float* x, float* out, int64_t n, float p, uint64_t seed, void* stream) {
    XPS_CHECK_ARG(x && out && n >= 0 && p >= 0.f && p < 1.f, "bad argument");
    if (n == 0) return XPS_OK;
    hipLaunchKernelGGL(relu_dropout_fwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, x, out, (long long)n, p,
                       1.0f / (1.0f - p), (unsigned long long)seed);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_relu_dropout_bwd_f32(const float* dout, const float* out, float* dx, int64_t n, float p, void* stream) {
    XPS_CHECK_ARG(dout && out && dx && n >= 0 && p >= 0.f && p < 1.f, "bad argument");
    if (n == 0) return XPS_OK;
    hipLaunchKernelGGL(relu_dropout_bwd_kernel, dim3(ew_blocks(n)), dim3(256), 0, (hipStream_t)stream, dout, out, dx, (long long)n,
                       1.0f / (1.0f - p));
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_add_positional_f32(const float* z, const float* table, float* out, int S, int B, int D, int batch_major, void* stream) {
    XPS_CHECK_ARG(z && table && out, "null argument");
    XPS_CHECK_ARG(S >= 1 && B >= 1 && D >= 1, "S, B and D must be positive");
    hipLaunchKernelGGL(add_positional_kernel, dim3(ew_blocks((long long)S * B * D)), dim3(256), 0, (hipStream_t)stream, z, table, out, S, B, D,
                       batch_major ? 1 : 0);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_time_mean_fwd_f32(const float* z, float* out, int T, int B, int F, void* stream) {
    XPS_CHECK_ARG(z && out, "null argument");
    XPS_CHECK_ARG(T >= 1 && B >= 1 && F >= 1, "T, B and F must be positive");
    const long long N = (long long)B * F;
    hipLaunchKernelGGL(time_mean_fwd_kernel, dim3(cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, z, out, T, N);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_time_mean_bwd_f32(const float* dout, float* dz, int T, int B, int F, void* stream) {
    XPS_CHECK_ARG(dout && dz, "null argument");
    XPS_CHECK_ARG(T >= 1 && B >= 1 && F >= 1, "T, B and F must be positive");
    const long long N = (long long)B * F;
    hipLaunchKernelGGL(time_mean_bwd_kernel, dim3(ew_blocks((long long)T * N)), dim3(256), 0, (hipStream_t)stream, dout, dz, T, N);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
