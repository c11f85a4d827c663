// The two ragged kernels of the aligned search (decoders/aligned_search.py): what keeps the launch count of a
// search over n_comp, C and gamma independent of the number of candidates.
//
//  xps_rbf_grouped_from_gram_f64   the rbf map of a table of square Gram matrices in one launch: problem p reads G_p (n_p x n_p) and
//                                  writes K_p[i][j] = xps_rbf_from_gram(gamma_p, G_p[i][i], G_p[j][j], G_p[i][j]) -- the expression of
//                                  xps_svm_rbf.h, so the bits are xps_rbf_from_gram_f64's with the Gram diagonal as norms.  One
//                                  workgroup per 64 x 64 tile; a wave reads and writes 64 consecutive doubles of a row (one 512-byte
//                                  run) per step.  Several problems may read one G with different gammas.
//  xps_var_grouped_f64             the population variance of the elements of a table of row blocks in one launch: one workgroup per
//                                  entry, two passes (mean, then squared deviations) in float64; a thread adds its elements in
//                                  ascending order, the 1024 partial sums meet in a fixed tree.  No atomics: two runs, the same bits.
//
// Both entries take HOST tables (the convention of xps_gram_grouped_f64): they are checked here, then copied into the caller's
// device workspace on the stream; the kernels trust them.
#include <math.h>
#include <string.h>

#include "xps_common.h"
#include "xps_svm_rbf.h"

namespace {

// words of one xps_rbf_grouped_from_gram_f64 problem
enum { RG_G, RG_LDG, RG_N, RG_GAMMA, RG_K, RG_LDK, RG_WORDS_USED };
static_assert(RG_WORDS_USED <= XPS_RBF_GROUPED_WORDS, "problem words");
// words of one xps_var_grouped_f64 entry
enum { VG_V, VG_V32, VG_LDV, VG_FIRST, VG_ROWS, VG_D, VG_WORDS_USED };
static_assert(VG_WORDS_USED <= XPS_VAR_GROUPED_WORDS, "entry words");

constexpr int RT = 64;             // the rbf tile: 64 rows of 64 consecutive doubles
constexpr int VT = 1024;           // threads of a variance workgroup

// One workgroup per (problem, 64-row tile ti, 64-column tile tj); tiles[3 t ..] = {problem, ti, tj}.  Wave w owns the rows
// w, w + 4, ... of the tile, lane l its column l: every load and store of a wave is one run of 64 doubles.
__global__ __launch_bounds__(256) void rbf_grouped_kernel(const long long* __restrict__ probs, const int* __restrict__ tiles) {
    __shared__ double nrow[RT], ncol[RT];
    const int* tl = tiles + 3 * (long long)blockIdx.x;
    const long long* P = probs + (long long)tl[0] * XPS_RBF_GROUPED_WORDS;
    const double* G = reinterpret_cast<const double*>(P[RG_G]);
    double* K = reinterpret_cast<double*>(P[RG_K]);
    const long long ldg = P[RG_LDG], ldk = P[RG_LDK];
    const int n = (int)P[RG_N];
    const double gamma = __longlong_as_double(P[RG_GAMMA]);
    const int m0 = tl[1] * RT, n0 = tl[2] * RT;
    const int tid = threadIdx.x;
    if (tid < 2 * RT) {                                            // the norms of the tile's rows and columns: the Gram diagonal
        const int i = (tid < RT ? m0 : n0 - RT) + tid;
        const double v = i < n ? G[(long long)i * ldg + i] : 0.0;
        (tid < RT ? nrow : ncol)[tid & (RT - 1)] = v;
    }
    __syncthreads();
    const int c = tid & (RT - 1), j = n0 + c;
    if (j >= n) return;
    const double nb = ncol[c];
#pragma unroll 4
    for (int r = tid / RT; r < RT; r += 256 / RT) {
        const int i = m0 + r;
        if (i >= n) break;
        K[(long long)i * ldk + j] = xps_rbf_from_gram(gamma, nrow[r], nb, G[(long long)i * ldg + j]);
    }
}

__device__ inline double load_elem(const void* V, int is32, long long at) {
    return is32 ? (double)static_cast<const float*>(V)[at] : static_cast<const double*>(V)[at];
}

// The sum of the workgroup's VT values in a fixed tree; every thread receives it.
__device__ inline double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();                                               // (red may still be read from the previous sum)
    red[tid] = v;
    __syncthreads();
    for (int s = VT / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// One workgroup per entry.  Element e of the block (row e / D, column e % D) belongs to thread e % VT; a thread walks its
// elements in ascending e, keeping (row, column) without a division per element.
__global__ __launch_bounds__(VT) void var_grouped_kernel(const long long* __restrict__ entries, double* __restrict__ out) {
    __shared__ double red[VT];
    const long long* E = entries + (long long)blockIdx.x * XPS_VAR_GROUPED_WORDS;
    const void* V = reinterpret_cast<const void*>(E[VG_V]);
    const int is32 = (int)E[VG_V32];
    const long long ldv = E[VG_LDV], first = E[VG_FIRST], rows = E[VG_ROWS], D = E[VG_D];
    const long long count = rows * D;
    const int tid = threadIdx.x;
    if (count == 0) {
        if (tid == 0) out[blockIdx.x] = 0.0;
        return;
    }
    const long long step_r = VT / D, step_c = VT % D, r0 = first + tid / D, c0 = tid % D;
    double acc = 0.0;
    long long r = r0, c = c0;
    for (long long e = tid; e < count; e += VT) {
        acc += load_elem(V, is32, r * ldv + c);
        r += step_r;
        c += step_c;
        if (c >= D) { c -= D; ++r; }
    }
    const double mean = block_sum(acc, red) / (double)count;
    acc = 0.0;
    r = r0;
    c = c0;
    for (long long e = tid; e < count; e += VT) {
        const double d = load_elem(V, is32, r * ldv + c) - mean;
        acc += d * d;
        r += step_r;
        c += step_c;
        if (c >= D) { c -= D; ++r; }
    }
    const double total = block_sum(acc, red);
    if (tid == 0) out[blockIdx.x] = total / (double)count;
}

inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace

extern "C" size_t xps_rbf_grouped_from_gram_f64_workspace(int n_problems, int n_tiles) {
    if (n_problems < 0 || n_tiles < 0) return 0;
    return align8(sizeof(long long) * XPS_RBF_GROUPED_WORDS * (size_t)n_problems) + align8(3 * sizeof(int) * (size_t)n_tiles);
}

extern "C" int xps_rbf_grouped_from_gram_f64(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, void* ws,
                                             size_t ws_bytes, void* stream) {
    XPS_CHECK_ARG(n_problems >= 0 && n_tiles >= 0, "negative count");
    if (n_problems == 0 && n_tiles == 0) return XPS_OK;
    XPS_CHECK_ARG((problems || n_problems == 0) && (tiles || n_tiles == 0), "null table");
    for (int p = 0; p < n_problems; ++p) {                         // both tables are HOST arrays: checked here, then copied
        const int64_t* P = problems + (size_t)XPS_RBF_GROUPED_WORDS * p;
        XPS_CHECK_ARG(P[RG_N] >= 0, "negative count");
        XPS_CHECK_ARG(P[RG_N] <= INT32_MAX - RT, "n beyond int32");
        XPS_CHECK_ARG(P[RG_LDG] >= P[RG_N], "ldg < n");
        XPS_CHECK_ARG(P[RG_LDK] >= P[RG_N], "ldk < n");
        double gamma;
        memcpy(&gamma, &P[RG_GAMMA], sizeof gamma);
        XPS_CHECK_ARG(isfinite(gamma) && gamma >= 0.0, "a gamma that is negative or not finite");
        XPS_CHECK_ARG(P[RG_N] == 0 || (P[RG_G] != 0 && P[RG_K] != 0), "null matrix");
        XPS_CHECK_ARG(P[RG_N] == 0 || P[RG_G] != P[RG_K], "K aliases G");
    }
    for (int t = 0; t < n_tiles; ++t) {
        const int32_t* tl = tiles + 3 * (size_t)t;
        XPS_CHECK_ARG(tl[0] >= 0 && tl[0] < n_problems, "a tile names no problem");
        const int64_t n = problems[(size_t)XPS_RBF_GROUPED_WORDS * tl[0] + RG_N];
        XPS_CHECK_ARG(tl[1] >= 0 && tl[2] >= 0 && (int64_t)tl[1] * RT < n && (int64_t)tl[2] * RT < n, "a tile origin at or past n");
    }
    if (n_tiles == 0) return XPS_OK;
    XPS_CHECK_ARG(ws, "null workspace");
    XPS_CHECK_ARG(ws_bytes >= xps_rbf_grouped_from_gram_f64_workspace(n_problems, n_tiles), "workspace too small");
    static_assert(sizeof(long long) == sizeof(int64_t), "the table is read as long long");
    hipStream_t st = (hipStream_t)stream;
    const size_t prob_bytes = sizeof(long long) * XPS_RBF_GROUPED_WORDS * (size_t)n_problems;
    long long* probs_d = static_cast<long long*>(ws);
    int* tiles_d = reinterpret_cast<int*>(static_cast<char*>(ws) + align8(prob_bytes));
    hipError_t e = hipMemcpyAsync(probs_d, problems, prob_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(tiles_d, tiles, 3 * sizeof(int) * (size_t)n_tiles, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { xps_set_error("%s: copying the tables failed: %s", __func__, hipGetErrorString(e)); return XPS_E_HIP; }
    hipLaunchKernelGGL(rbf_grouped_kernel, dim3(n_tiles), dim3(256), 0, st, (const long long*)probs_d, (const int*)tiles_d);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" size_t xps_var_grouped_f64_workspace(int n_entries) {
    if (n_entries < 0) return 0;
    return align8(sizeof(long long) * XPS_VAR_GROUPED_WORDS * (size_t)n_entries);
}

extern "C" int xps_var_grouped_f64(const int64_t* entries, int n_entries, double* out, void* ws, size_t ws_bytes, void* stream) {
    XPS_CHECK_ARG(n_entries >= 0, "negative count");
    if (n_entries == 0) return XPS_OK;
    XPS_CHECK_ARG(entries && out, "null table");
    for (int i = 0; i < n_entries; ++i) {                          // the table is a HOST array: checked here, then copied
        const int64_t* E = entries + (size_t)XPS_VAR_GROUPED_WORDS * i;
        XPS_CHECK_ARG(E[VG_FIRST] >= 0 && E[VG_ROWS] >= 0 && E[VG_D] >= 0, "negative count");
        XPS_CHECK_ARG(E[VG_FIRST] <= INT32_MAX && E[VG_ROWS] <= INT32_MAX && E[VG_D] <= INT32_MAX, "a count beyond int32");
        XPS_CHECK_ARG(E[VG_V32] == 0 || E[VG_V32] == 1, "v_is_f32 must be 0 or 1");
        XPS_CHECK_ARG(E[VG_LDV] >= E[VG_D], "ldv < D");
        XPS_CHECK_ARG(E[VG_ROWS] * E[VG_D] == 0 || E[VG_V] != 0, "null matrix");
    }
    XPS_CHECK_ARG(ws, "null workspace");
    XPS_CHECK_ARG(ws_bytes >= xps_var_grouped_f64_workspace(n_entries), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(ws, entries, sizeof(long long) * XPS_VAR_GROUPED_WORDS * (size_t)n_entries, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { xps_set_error("%s: copying the table failed: %s", __func__, hipGetErrorString(e)); return XPS_E_HIP; }
    hipLaunchKernelGGL(var_grouped_kernel, dim3(n_entries), dim3(VT), 0, st, (const long long*)ws, out);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
