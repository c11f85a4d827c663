// Fold-batched PCA -> CCA alignment for gfx950: every fold of a k-fold split as one device problem.
//
//  xps_xcov_grouped_f64    a TABLE of centred cross-moment problems in one launch (+ one reduce launch): per problem
//                          sum (a - c_a)(b - c_b)^T, sum (a - c_a), sum (b - c_b) and the row count over two lists of
//                          row blocks.  The tile is xps_f64_tile.h's, as in gemm_f64_kernel (xps_align.hip): 64 x 64 outputs
//                          per workgroup, 16 staged rows per step, fp32 / fp64 inputs converted and centred while staged
//                          to LDS.  Split-K writes slabs that the reduce adds in slab order: two runs give
//                          the same bits.
//  xps_loo_sum_f64         out[f] = sum over g != f of in[g], ascending g, plain adds.
//  xps_apply_grouped_f64   a table of (X - mean) W products with ragged widths in one launch (xps_apply_f64's arithmetic).
//  xps_cnd_avg_folds_f64   a table of segment means: fp64 sums over listed trials in list order.
//  xps_gram_grouped_f64    a table of Gram matrices G_p = V_p V_p^T with ragged row counts and contraction lengths in one launch:
//                          one workgroup per 64 x 64 tile of the lower triangle, the contraction walked whole in ascending k,
//                          off-diagonal tiles mirrored, so every G_p is symmetric bit for bit and the same for any grid.
//
// The tables are DEVICE arrays of int64 words built by the caller (alignment/_linalg.py checks every extent against the
// tensors it was given before it uploads one); the kernels trust them.  xps_gram_grouped_f64 alone takes HOST tables: its entry
// checks them and copies them to the device on the stream.
#include "xps_common.h"
#include "xps_f64_tile.h"

namespace {

// words of one xps_xcov_grouped_f64 problem
enum { XP_A, XP_B, XP_LDA, XP_LDB, XP_A32, XP_B32, XP_CA, XP_CB, XP_BLKA, XP_BLKB, XP_NBLK, XP_BLKLEN, XP_DA, XP_DB,
       XP_OUT, XP_SLAB, XP_SPLITS, XP_KCHUNK, XP_WORDS_USED };
static_assert(XP_WORDS_USED <= XPS_XCOV_GROUPED_WORDS, "problem words");
// words of one xps_apply_grouped_f64 entry
enum { AP_X, AP_X32, AP_LDX, AP_ROWS, AP_MEAN, AP_W, AP_LDW, AP_DIN, AP_DOUT, AP_OUT, AP_LDO, AP_O32, AP_WORDS_USED };
static_assert(AP_WORDS_USED <= XPS_APPLY_GROUPED_WORDS, "entry words");
// words of one xps_cnd_avg_folds_f64 segment
enum { CS_SRC, CS_ROWLEN, CS_OUT, CS_BEGIN, CS_END, CS_WORDS_USED };
static_assert(CS_WORDS_USED <= XPS_CND_AVG_FOLDS_WORDS, "segment words");
// words of one xps_gram_grouped_f64 problem
enum { GG_V, GG_V32, GG_LDV, GG_N, GG_D, GG_G, GG_LDG, GG_WORDS_USED };
static_assert(GG_WORDS_USED <= XPS_GRAM_GROUPED_WORDS, "problem words");

// Storage row of contraction index k of a problem: row k % blk_len of block k / blk_len of its list of K / blk_len blocks.
struct BlockRows {
    const long long* blk;
    int blk_len, K;
    __device__ long long operator()(int k) const { return k < K ? blk[k / blk_len] + (k % blk_len) : 0; }
};

// One workgroup per (problem, 64-row tile of C, 64-column tile of C, K split); tiles[4 t ..] = {problem, mt, nt, split}.
// Slab of a split: [C (da x db) | s_a (da) | s_b (db)].
__global__ __launch_bounds__(256) void xcov_grouped_kernel(const long long* __restrict__ probs, const int* __restrict__ tiles) {
    __shared__ __attribute__((aligned(16))) double As[DK][DLD];
    __shared__ __attribute__((aligned(16))) double Bs[DK][DLD];
    const int* tl = tiles + 4 * (long long)blockIdx.x;
    const long long* P = probs + (long long)tl[0] * XPS_XCOV_GROUPED_WORDS;
    const int mt = tl[1], nt = tl[2], split = tl[3];
    const Mat64 A{reinterpret_cast<const void*>(P[XP_A]), P[XP_LDA], reinterpret_cast<const double*>(P[XP_CA]), (int)P[XP_A32]};
    const Mat64 B{reinterpret_cast<const void*>(P[XP_B]), P[XP_LDB], reinterpret_cast<const double*>(P[XP_CB]), (int)P[XP_B32]};
    const int blk_len = (int)P[XP_BLKLEN], da = (int)P[XP_DA], db = (int)P[XP_DB];
    const int K = (int)P[XP_NBLK] * blk_len, kchunk = (int)P[XP_KCHUNK];
    const BlockRows rows_a{reinterpret_cast<const long long*>(P[XP_BLKA]), blk_len, K};
    const BlockRows rows_b{reinterpret_cast<const long long*>(P[XP_BLKB]), blk_len, K};
    double* slab = reinterpret_cast<double*>(P[XP_SLAB]) + (long long)split * ((long long)da * db + da + db);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = mt * DM, n0 = nt * DN;
    const int kbeg = split * kchunk;
    const int kend = min(K, kbeg + kchunk);

    f64x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f64x4){0.0, 0.0, 0.0, 0.0};
    double colsum = 0.0;                       // wave 0: s_a of column m0 + lane (nt == 0); wave 1: s_b of n0 + lane (mt == 0)

    for (int k0 = kbeg; k0 < kend; k0 += DK) {
        stage_xc(A, As, m0, da, k0, kend, tid, rows_a);
        stage_xc(B, Bs, n0, db, k0, kend, tid, rows_b);
        __syncthreads();
        mfma_f64_tile(As, Bs, acc, tid);
        if (wave == 0 && nt == 0) {
#pragma unroll
            for (int k = 0; k < DK; ++k) colsum += As[k][lane];
        } else if (wave == 1 && mt == 0) {
#pragma unroll
            for (int k = 0; k < DK; ++k) colsum += Bs[k][lane];
        }
        __syncthreads();
    }
    store_f64_tile(acc, m0, n0, da, db, tid, [&](int row, int col, double v) { slab[(long long)row * db + col] = v; });
    if (wave == 0 && nt == 0 && m0 + lane < da) slab[(long long)da * db + m0 + lane] = colsum;
    if (wave == 1 && mt == 0 && n0 + lane < db) slab[(long long)da * db + da + n0 + lane] = colsum;
}

// out of a problem: [C | s_a | s_b | count], each element the sum of its slabs in slab order.
__global__ void xcov_grouped_reduce(const long long* __restrict__ probs) {
    const long long* P = probs + (long long)blockIdx.y * XPS_XCOV_GROUPED_WORDS;
    const int da = (int)P[XP_DA], db = (int)P[XP_DB], splits = (int)P[XP_SPLITS];
    const long long len = (long long)da * db + da + db;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx > len) return;
    double* out = reinterpret_cast<double*>(P[XP_OUT]);
    if (idx == len) { out[len] = (double)(P[XP_NBLK] * P[XP_BLKLEN]); return; }
    const double* slabs = reinterpret_cast<const double*>(P[XP_SLAB]);
    double s = 0.0;
    for (int z = 0; z < splits; ++z) s += slabs[(long long)z * len + idx];
    out[idx] = s;
}

__global__ void loo_sum_kernel(const double* __restrict__ in, double* __restrict__ out, int G, long long len) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= len) return;
    const int f = blockIdx.y;
    double s = 0.0;
    for (int g = 0; g < G; ++g)
        if (g != f) s += in[(long long)g * len + e];
    out[(long long)f * len + e] = s;
}

// One workgroup per (entry, 64-row tile, 64-column tile); tiles[3 t ..] = {entry, mt, nt}.
__global__ __launch_bounds__(256) void apply_grouped_kernel(const long long* __restrict__ ents, const int* __restrict__ tiles) {
    __shared__ __attribute__((aligned(16))) double As[DK][DLD];
    __shared__ __attribute__((aligned(16))) double Bs[DK][DLD];
    const int* tl = tiles + 3 * (long long)blockIdx.x;
    const long long* E = ents + (long long)tl[0] * XPS_APPLY_GROUPED_WORDS;
    const Mat64 X{reinterpret_cast<const void*>(E[AP_X]), E[AP_LDX], reinterpret_cast<const double*>(E[AP_MEAN]), (int)E[AP_X32]};
    const Mat64 W{reinterpret_cast<const void*>(E[AP_W]), E[AP_LDW], nullptr, 0};
    const int rows = (int)E[AP_ROWS], d_in = (int)E[AP_DIN], d_out = (int)E[AP_DOUT];
    const long long ldo = E[AP_LDO];
    void* out = reinterpret_cast<void*>(E[AP_OUT]);
    const int o32 = (int)E[AP_O32];

    const int tid = threadIdx.x;
    const int m0 = tl[1] * DM, n0 = tl[2] * DN;

    f64x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < d_in; k0 += DK) {
        stage_kc(X, As, m0, rows, k0, d_in, tid);
        stage_xc(W, Bs, n0, d_out, k0, d_in, tid);
        __syncthreads();
        mfma_f64_tile(As, Bs, acc, tid);
        __syncthreads();
    }
    store_f64_tile(acc, m0, n0, rows, d_out, tid, [&](int row, int col, double v) {
        const long long o = (long long)row * ldo + col;
        if (o32) reinterpret_cast<float*>(out)[o] = (float)v;
        else reinterpret_cast<double*>(out)[o] = v;
    });
}

__global__ void cnd_avg_folds_kernel(const long long* __restrict__ segs, const int* __restrict__ trials) {
    const long long* S = segs + (long long)blockIdx.y * XPS_CND_AVG_FOLDS_WORDS;
    const long long row_len = S[CS_ROWLEN];
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= row_len) return;
    const double* src = reinterpret_cast<const double*>(S[CS_SRC]);
    double* out = reinterpret_cast<double*>(S[CS_OUT]);
    const long long b = S[CS_BEGIN], en = S[CS_END];
    if (en <= b) { out[e] = 0.0; return; }
    double acc = src[(long long)trials[b] * row_len + e];
    for (long long i = b + 1; i < en; ++i) acc += src[(long long)trials[i] * row_len + e];
    out[e] = acc / (double)(en - b);
}

// One workgroup per (problem, 64-row tile ti, 64-column tile tj <= ti); tiles[3 t ..] = {problem, ti, tj}.  Both operands are row
// blocks of V, staged contraction-contiguous.  An off-diagonal tile is stored to (ti, tj) and, transposed, to (tj, ti); a diagonal
// tile is stored as computed: its elements (i, j) and (j, i) are sums of the same products in the same order (k ascending).
__global__ __launch_bounds__(256) void gram_grouped_kernel(const long long* __restrict__ probs, const int* __restrict__ tiles) {
    __shared__ __attribute__((aligned(16))) double As[DK][DLD];
    __shared__ __attribute__((aligned(16))) double Bs[DK][DLD];
    const int* tl = tiles + 3 * (long long)blockIdx.x;
    const long long* P = probs + (long long)tl[0] * XPS_GRAM_GROUPED_WORDS;
    const Mat64 V{reinterpret_cast<const void*>(P[GG_V]), P[GG_LDV], nullptr, (int)P[GG_V32]};
    const int n = (int)P[GG_N], D = (int)P[GG_D];
    double* G = reinterpret_cast<double*>(P[GG_G]);
    const long long ldg = P[GG_LDG];

    const int tid = threadIdx.x;
    const int m0 = tl[1] * DM, n0 = tl[2] * DN;
    const bool mirror = m0 != n0;

    f64x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < D; k0 += DK) {
        stage_kc(V, As, m0, n, k0, D, tid);
        stage_kc(V, Bs, n0, n, k0, D, tid);
        __syncthreads();
        mfma_f64_tile(As, Bs, acc, tid);
        __syncthreads();
    }
    store_f64_tile(acc, m0, n0, n, n, tid, [&](int row, int col, double v) {
        G[(long long)row * ldg + col] = v;
        if (mirror) G[(long long)col * ldg + row] = v;
    });
}

inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace

extern "C" int xps_xcov_grouped_f64(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, int max_out_len,
                                    void* stream) {
    XPS_CHECK_ARG(n_problems >= 0 && n_tiles >= 0 && max_out_len >= 0, "bad argument");
    if (n_problems == 0) return XPS_OK;
    XPS_CHECK_ARG(problems && (tiles || n_tiles == 0) && max_out_len >= 4, "null table");
    XPS_CHECK_ARG(n_problems <= 65535, "more than 65535 problems in one call");
    if (n_tiles > 0) {
        hipLaunchKernelGGL(xcov_grouped_kernel, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream,
                           (const long long*)problems, (const int*)tiles);
        XPS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(xcov_grouped_reduce, dim3(cdiv(max_out_len, 256), n_problems), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)problems);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_loo_sum_f64(const double* in, double* out, int n_groups, int n_out, int64_t len, void* stream) {
    XPS_CHECK_ARG(in && out && n_groups >= 1 && n_out >= 0 && n_out <= n_groups && len >= 0 && in != out, "bad argument");
    if (n_out == 0 || len == 0) return XPS_OK;
    hipLaunchKernelGGL(loo_sum_kernel, dim3(cdiv(len, 256), n_out), dim3(256), 0, (hipStream_t)stream, in, out, n_groups,
                       (long long)len);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_apply_grouped_f64(const int64_t* entries, int n_entries, const int32_t* tiles, int n_tiles, void* stream) {
    XPS_CHECK_ARG(n_entries >= 0 && n_tiles >= 0, "bad argument");
    if (n_entries == 0 || n_tiles == 0) return XPS_OK;
    XPS_CHECK_ARG(entries && tiles, "null table");
    hipLaunchKernelGGL(apply_grouped_kernel, dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, (const long long*)entries,
                       (const int*)tiles);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_cnd_avg_folds_f64(const int64_t* segments, int n_segments, const int32_t* trials, int64_t max_row_len,
                                     void* stream) {
    XPS_CHECK_ARG(n_segments >= 0 && max_row_len >= 0, "bad argument");
    if (n_segments == 0 || max_row_len == 0) return XPS_OK;
    XPS_CHECK_ARG(segments && trials, "null table");
    XPS_CHECK_ARG(n_segments <= 65535, "more than 65535 segments in one call");
    hipLaunchKernelGGL(cnd_avg_folds_kernel, dim3(cdiv(max_row_len, 256), n_segments), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)segments, (const int*)trials);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" size_t xps_gram_grouped_f64_workspace(int n_problems, int n_tiles) {
    if (n_problems < 0 || n_tiles < 0) return 0;
    return align8(sizeof(long long) * XPS_GRAM_GROUPED_WORDS * (size_t)n_problems) + align8(3 * sizeof(int) * (size_t)n_tiles);
}

extern "C" int xps_gram_grouped_f64(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, void* ws,
                                    size_t ws_bytes, void* stream) {
    XPS_CHECK_ARG(n_problems >= 0 && n_tiles >= 0, "negative count");
    if (n_problems == 0 && n_tiles == 0) return XPS_OK;
    XPS_CHECK_ARG((problems || n_problems == 0) && (tiles || n_tiles == 0), "null table");
    for (int p = 0; p < n_problems; ++p) {                         // both tables are HOST arrays: checked here, then copied
        const int64_t* P = problems + (size_t)XPS_GRAM_GROUPED_WORDS * p;
        XPS_CHECK_ARG(P[GG_N] >= 0 && P[GG_D] >= 0, "negative count");
        XPS_CHECK_ARG(P[GG_N] <= INT32_MAX - DM && P[GG_D] <= INT32_MAX - DK, "n or D beyond int32");
        XPS_CHECK_ARG(P[GG_V32] == 0 || P[GG_V32] == 1, "v_is_f32 must be 0 or 1");
        XPS_CHECK_ARG(P[GG_LDV] >= P[GG_D], "ldv < D");
        XPS_CHECK_ARG(P[GG_LDG] >= P[GG_N], "ldg < n");
        XPS_CHECK_ARG(P[GG_N] == 0 || (P[GG_G] != 0 && (P[GG_V] != 0 || P[GG_D] == 0)), "null matrix");
    }
    for (int t = 0; t < n_tiles; ++t) {
        const int32_t* tl = tiles + 3 * (size_t)t;
        XPS_CHECK_ARG(tl[0] >= 0 && tl[0] < n_problems, "a tile names no problem");
        const int64_t n = problems[(size_t)XPS_GRAM_GROUPED_WORDS * tl[0] + GG_N];
        XPS_CHECK_ARG(tl[2] >= 0 && tl[2] <= tl[1], "a tile above the diagonal (tj <= ti is needed)");
        XPS_CHECK_ARG((int64_t)tl[1] * DM < n, "a tile origin at or past n");
    }
    if (n_tiles == 0) return XPS_OK;
    XPS_CHECK_ARG(ws, "null workspace");
    XPS_CHECK_ARG(ws_bytes >= xps_gram_grouped_f64_workspace(n_problems, n_tiles), "workspace too small");
    static_assert(sizeof(long long) == sizeof(int64_t), "the table is read as long long");
    hipStream_t st = (hipStream_t)stream;
    long long* probs_d = static_cast<long long*>(ws);
    int* tiles_d = reinterpret_cast<int*>(static_cast<char*>(ws) + align8(sizeof(long long) * XPS_GRAM_GROUPED_WORDS * (size_t)n_problems));
    hipError_t e = hipMemcpyAsync(probs_d, problems, sizeof(long long) * XPS_GRAM_GROUPED_WORDS * (size_t)n_problems, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(tiles_d, tiles, 3 * sizeof(int) * (size_t)n_tiles, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { xps_set_error("%s: copying the tables failed: %s", __func__, hipGetErrorString(e)); return XPS_E_HIP; }
    hipLaunchKernelGGL(gram_grouped_kernel, dim3(n_tiles), dim3(256), 0, st, (const long long*)probs_d, (const int*)tiles_d);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
