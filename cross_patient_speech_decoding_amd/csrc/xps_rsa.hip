// Representational dissimilarity analysis (alignment/rsa.py): what turns the figure notebooks' double loop
// of scipy.stats.pearsonr calls and their RDM comparison into a fixed number of launches, however many data sets, pairs and
// label permutations there are.
//
//  xps_row_standardize_grouped_f64  every row of a table of matrices becomes (x - mean) / |x - mean| (pearsonr's arithmetic), so
//                                   that ONE xps_gram_grouped_f64 launch yields every r_ij of every data set.  One workgroup per
//                                   row; a thread adds its elements in ascending order, the 256 partial sums meet in a fixed tree.
//  xps_rdm_from_corr_grouped_f64    rdm = 1 - clip(r, -1, 1) with NaN kept and the diagonal 0; in place on the Gram output.
//  xps_rdm_compare_perm_f64         the hot path: the centred cross products of the upper triangles of two RDMs over their shared
//                                   conditions, for the identity and R relabellings of the second matrix.  One wave per (pair,
//                                   permutation); the four statistics of a pair are taken once, by one wave, in the same order.
//
// All three take HOST tables (the convention of xps_gram_grouped_f64): they are checked here, then copied into the caller's device
// workspace on the stream; the kernels trust them.  No atomics; the summation order is a function of the problem alone.
#include <math.h>
#include <string.h>

#include "xps_common.h"

namespace {

// words of one xps_row_standardize_grouped_f64 problem
enum { RS_X, RS_LDX, RS_ROWS, RS_D, RS_Z, RS_LDZ, RS_WORDS_USED };
static_assert(RS_WORDS_USED <= XPS_RSA_STD_WORDS, "problem words");
// words of one xps_rdm_from_corr_grouped_f64 problem
enum { RC_G, RC_LDG, RC_N, RC_OUT, RC_LDO, RC_WORDS_USED };
static_assert(RC_WORDS_USED <= XPS_RSA_RDM_WORDS, "problem words");
// words of one xps_rdm_compare_perm_f64 pair
enum { CP_A, CP_LDA, CP_NA, CP_IA, CP_B, CP_LDB, CP_NB, CP_IB, CP_M, CP_TABLE, CP_ROW, CP_WORDS_USED };
static_assert(CP_WORDS_USED <= XPS_RSA_PAIR_WORDS, "pair words");

constexpr int ST = 256;            // threads of a row workgroup
constexpr int CW = 4;              // waves of a compare workgroup: four permutations of one pair
constexpr int MAXC = XPS_RSA_MAX_CONDITIONS;

// The sum of the workgroup's ST values in a fixed tree; every thread receives it.
__device__ inline double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();                                               // (red may still be read from the previous sum)
    red[tid] = v;
    __syncthreads();
    for (int s = ST / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// One workgroup per (row, problem).  Thread t owns the elements t, t + 256, ... of the row.  The mean takes two passes (the sum
// over D, then the sum of the deviations from it over D: the second corrects the rounding of the first), the norm a third; a
// row whose elements are all equal is NaN, as scipy's constant-input rule makes it, and so is any row of norm 0.
__global__ __launch_bounds__(ST) void row_standardize_kernel(const long long* __restrict__ probs) {
    __shared__ double red[ST];
    const long long* P = probs + (long long)blockIdx.y * XPS_RSA_STD_WORDS;
    const int row = blockIdx.x;
    if (row >= P[RS_ROWS]) return;
    const long long D = P[RS_D];
    const double* x = reinterpret_cast<const double*>(P[RS_X]) + row * P[RS_LDX];
    double* z = reinterpret_cast<double*>(P[RS_Z]) + row * P[RS_LDZ];
    const int tid = threadIdx.x;
    const double first = x[0];
    double acc = 0.0;
    int differs = 0;
    for (long long e = tid; e < D; e += ST) {
        const double v = x[e];
        acc += v;
        differs |= (v != first);
    }
    const int varies = __syncthreads_or(differs);
    const double m0 = block_sum(acc, red) / (double)D;
    acc = 0.0;
    for (long long e = tid; e < D; e += ST) acc += x[e] - m0;
    const double mean = m0 + block_sum(acc, red) / (double)D;
    acc = 0.0;
    for (long long e = tid; e < D; e += ST) {
        const double d = x[e] - mean;
        acc += d * d;
    }
    const double norm = varies ? sqrt(block_sum(acc, red)) : 0.0;
    // a norm of 0 (a constant row, or deviations whose squares underflow) or NaN: a NaN row (x may be z: own element)
    for (long long e = tid; e < D; e += ST) z[e] = norm > 0.0 ? (x[e] - mean) / norm : __longlong_as_double(0x7FF8000000000000LL);
}

// One workgroup per (row, problem): out[i][j] = 1 - clip(r[i][j]); a NaN passes (both comparisons are false); the diagonal is 0
// unless it is NaN (a constant condition: NaN in its whole row and column).
__global__ __launch_bounds__(ST) void rdm_from_corr_kernel(const long long* __restrict__ probs) {
    const long long* P = probs + (long long)blockIdx.y * XPS_RSA_RDM_WORDS;
    const int i = blockIdx.x;
    const int n = (int)P[RC_N];
    if (i >= n) return;
    const double* g = reinterpret_cast<const double*>(P[RC_G]) + i * P[RC_LDG];
    double* o = reinterpret_cast<double*>(P[RC_OUT]) + i * P[RC_LDO];
    for (int j = threadIdx.x; j < n; j += ST) {
        double r = g[j];
        r = r > 1.0 ? 1.0 : r;
        r = r < -1.0 ? -1.0 : r;
        const double d = 1.0 - r;
        o[j] = (j == i && d == d) ? 0.0 : d;
    }
}

// The upper triangle k = 1 of the two gathered matrices in np.triu_indices order, as one wave walks it: u ascending, lane l
// takes v = u + 1 + l, u + 1 + l + 64, ...  ja[v] = ia[v], jb[v] = ib[p[v]] are staged in LDS.  f(x, y) is called once per
// element in the lane's fixed order.
template <class F>
__device__ inline void walk_triangle(const double* __restrict__ A, long long lda, const double* __restrict__ B, long long ldb,
                                     const int* ja, const int* jb, int m, int lane, F f) {
    for (int u = 0; u + 1 < m; ++u) {
        const double* a = A + ja[u] * lda;
        const double* b = B + jb[u] * ldb;
        for (int v = u + 1 + lane; v < m; v += 64) f(a[ja[v]], b[jb[v]]);
    }
}

// One wave per pair: stats[row] = {mean_x, mean_y, sxx, syy} of the unpermuted triangles (cosine: both means 0).
__global__ __launch_bounds__(64) void rdm_stats_kernel(const long long* __restrict__ pairs, const int* __restrict__ idx, int cosine,
                                                       double* __restrict__ stats) {
    __shared__ int ja[MAXC], jb[MAXC];
    const long long* P = pairs + (long long)blockIdx.x * XPS_RSA_PAIR_WORDS;
    const int m = (int)P[CP_M], lane = threadIdx.x;
    const double* A = reinterpret_cast<const double*>(P[CP_A]);
    const double* B = reinterpret_cast<const double*>(P[CP_B]);
    const long long lda = P[CP_LDA], ldb = P[CP_LDB];
    for (int v = lane; v < m; v += 64) {
        ja[v] = idx[P[CP_IA] + v];
        jb[v] = idx[P[CP_IB] + v];
    }
    __syncthreads();
    double mx = 0.0, my = 0.0;
    if (!cosine) {
        double sx = 0.0, sy = 0.0;
        walk_triangle(A, lda, B, ldb, ja, jb, m, lane, [&](double x, double y) { sx += x; sy += y; });
        const double L = 0.5 * (double)m * (double)(m - 1);
        mx = wave_sum_f64(sx) / L;
        my = wave_sum_f64(sy) / L;
    }
    double sxx = 0.0, syy = 0.0;
    walk_triangle(A, lda, B, ldb, ja, jb, m, lane, [&](double x, double y) {
        const double dx = x - mx, dy = y - my;
        sxx += dx * dx;
        syy += dy * dy;
    });
    sxx = wave_sum_f64(sxx);
    syy = wave_sum_f64(syy);
    if (lane == 0) {
        double* s = stats + 4 * P[CP_ROW];
        s[0] = mx; s[1] = my; s[2] = sxx; s[3] = syy;
    }
}

// Workgroup (pair = blockIdx.x, four permutations from 4 blockIdx.y): wave w takes row r = 4 blockIdx.y + w of the pair's table.
// cross[row][r] = sum_{u<v} (A[ia[u]][ia[v]] - mean_x) (B[ib[p[u]]][ib[p[v]]] - mean_y).
__global__ __launch_bounds__(64 * CW) void rdm_cross_kernel(const long long* __restrict__ pairs, const long long* __restrict__ tables,
                                                            const int* __restrict__ idx, const int* __restrict__ perms, int R1,
                                                            const double* __restrict__ stats, double* __restrict__ cross) {
    __shared__ int ja[MAXC], jb[CW][MAXC];
    const long long* P = pairs + (long long)blockIdx.x * XPS_RSA_PAIR_WORDS;
    const int m = (int)P[CP_M], lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = blockIdx.y * CW + w;
    const int rr = r < R1 ? r : R1 - 1;                            // a wave past the table repeats the last row and stores nothing
    const int* p = perms + tables[2 * P[CP_TABLE]] + (long long)rr * m;
    for (int v = threadIdx.x; v < m; v += 64 * CW) ja[v] = idx[P[CP_IA] + v];
    for (int v = lane; v < m; v += 64) jb[w][v] = idx[P[CP_IB] + p[v]];
    __syncthreads();
    const double* s = stats + 4 * P[CP_ROW];
    const double mx = s[0], my = s[1];
    double acc = 0.0;
    walk_triangle(reinterpret_cast<const double*>(P[CP_A]), P[CP_LDA], reinterpret_cast<const double*>(P[CP_B]), P[CP_LDB], ja, jb[w],
                  m, lane, [&](double x, double y) { acc += (x - mx) * (y - my); });
    acc = wave_sum_f64(acc);
    if (lane == 0 && r < R1) cross[P[CP_ROW] * R1 + r] = acc;
}

inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

// The row-per-workgroup launch of the first two entries: grid (largest row count, problems).
template <class K>
int launch_rows(K kernel, const int64_t* problems, int n_problems, int words, int rows_word, void* ws, hipStream_t st, const char* who) {
    int64_t most = 0;
    for (int p = 0; p < n_problems; ++p) most = problems[(size_t)words * p + rows_word] > most ? problems[(size_t)words * p + rows_word] : most;
    if (most == 0) return XPS_OK;
    hipError_t e = hipMemcpyAsync(ws, problems, sizeof(long long) * words * (size_t)n_problems, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { xps_set_error("%s: copying the table failed: %s", who, hipGetErrorString(e)); return XPS_E_HIP; }
    hipLaunchKernelGGL(kernel, dim3((unsigned)most, (unsigned)n_problems), dim3(ST), 0, st, (const long long*)ws);
    e = hipGetLastError();
    if (e != hipSuccess) { xps_set_error("%s: launch failed: %s", who, hipGetErrorString(e)); return XPS_E_HIP; }
    return XPS_OK;
}

}  // namespace

extern "C" size_t xps_row_standardize_grouped_f64_workspace(int n_problems) {
    if (n_problems < 0) return 0;
    return align8(sizeof(long long) * XPS_RSA_STD_WORDS * (size_t)n_problems);
}

extern "C" int xps_row_standardize_grouped_f64(const int64_t* problems, int n_problems, void* ws, size_t ws_bytes, void* stream) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the table is read as long long");
    XPS_CHECK_ARG(n_problems >= 0, "negative count");
    if (n_problems == 0) return XPS_OK;
    XPS_CHECK_ARG(problems, "null table");
    XPS_CHECK_ARG(n_problems <= 65535, "more than 65535 problems");
    for (int p = 0; p < n_problems; ++p) {                         // the table is a HOST array: checked here, then copied
        const int64_t* P = problems + (size_t)XPS_RSA_STD_WORDS * p;
        XPS_CHECK_ARG(P[RS_ROWS] >= 0 && P[RS_ROWS] <= INT32_MAX, "a row count outside int32");
        XPS_CHECK_ARG(P[RS_D] >= 1 && P[RS_D] <= INT32_MAX, "D outside 1 .. int32");
        XPS_CHECK_ARG(P[RS_LDX] >= P[RS_D], "ldx < D");
        XPS_CHECK_ARG(P[RS_LDZ] >= P[RS_D], "ldz < D");
        XPS_CHECK_ARG(P[RS_ROWS] == 0 || (P[RS_X] != 0 && P[RS_Z] != 0), "null matrix");
    }
    XPS_CHECK_ARG(ws, "null workspace");
    XPS_CHECK_ARG(ws_bytes >= xps_row_standardize_grouped_f64_workspace(n_problems), "workspace too small");
    return launch_rows(row_standardize_kernel, problems, n_problems, XPS_RSA_STD_WORDS, RS_ROWS, ws, (hipStream_t)stream, __func__);
}

extern "C" size_t xps_rdm_from_corr_grouped_f64_workspace(int n_problems) {
    if (n_problems < 0) return 0;
    return align8(sizeof(long long) * XPS_RSA_RDM_WORDS * (size_t)n_problems);
}

extern "C" int xps_rdm_from_corr_grouped_f64(const int64_t* problems, int n_problems, void* ws, size_t ws_bytes, void* stream) {
    XPS_CHECK_ARG(n_problems >= 0, "negative count");
    if (n_problems == 0) return XPS_OK;
    XPS_CHECK_ARG(problems, "null table");
    XPS_CHECK_ARG(n_problems <= 65535, "more than 65535 problems");
    for (int p = 0; p < n_problems; ++p) {
        const int64_t* P = problems + (size_t)XPS_RSA_RDM_WORDS * p;
        XPS_CHECK_ARG(P[RC_N] >= 0 && P[RC_N] <= INT32_MAX, "n outside int32");
        XPS_CHECK_ARG(P[RC_LDG] >= P[RC_N], "ldg < n");
        XPS_CHECK_ARG(P[RC_LDO] >= P[RC_N], "ldo < n");
        XPS_CHECK_ARG(P[RC_N] == 0 || (P[RC_G] != 0 && P[RC_OUT] != 0), "null matrix");
    }
    XPS_CHECK_ARG(ws, "null workspace");
    XPS_CHECK_ARG(ws_bytes >= xps_rdm_from_corr_grouped_f64_workspace(n_problems), "workspace too small");
    return launch_rows(rdm_from_corr_kernel, problems, n_problems, XPS_RSA_RDM_WORDS, RC_N, ws, (hipStream_t)stream, __func__);
}

extern "C" size_t xps_rdm_compare_perm_f64_workspace(int n_pairs, int n_tables, int64_t n_idx, int64_t n_perm) {
    if (n_pairs < 0 || n_tables < 0 || n_idx < 0 || n_perm < 0) return 0;
    return align8(sizeof(long long) * XPS_RSA_PAIR_WORDS * (size_t)n_pairs) + align8(2 * sizeof(long long) * (size_t)n_tables) +
           align8(sizeof(int) * (size_t)n_idx) + align8(sizeof(int) * (size_t)n_perm);
}

extern "C" int xps_rdm_compare_perm_f64(const int64_t* pairs, int n_pairs, const int64_t* tables, int n_tables, const int32_t* idx,
                                        int64_t n_idx, const int32_t* perms, int64_t n_perm, int R, int cosine, double* stats,
                                        double* cross, int64_t n_rows, void* ws, size_t ws_bytes, void* stream) {
    XPS_CHECK_ARG(n_pairs >= 0 && n_tables >= 0 && n_idx >= 0 && n_perm >= 0 && n_rows >= 0, "negative count");
    XPS_CHECK_ARG(R >= 0 && R < CW * 65535, "R outside 0 .. 262139");
    XPS_CHECK_ARG(cosine == 0 || cosine == 1, "cosine must be 0 or 1");
    if (n_pairs == 0) return XPS_OK;
    XPS_CHECK_ARG(pairs && tables && idx && perms, "null table");
    XPS_CHECK_ARG(stats && cross, "null output");
    const int64_t R1 = (int64_t)R + 1;
    for (int t = 0; t < n_tables; ++t) {                           // every table: (R + 1, m) inside perms, row 0 the identity,
        const int64_t off = tables[2 * (size_t)t], m = tables[2 * (size_t)t + 1];          // every row a permutation of [0, m)
        XPS_CHECK_ARG(m >= 2 && m <= MAXC, "m outside 2 .. XPS_RSA_MAX_CONDITIONS");
        XPS_CHECK_ARG(off >= 0 && off <= n_perm && R1 * m <= n_perm - off, "a permutation table reaches outside perms");
        unsigned char seen[MAXC];
        for (int64_t r = 0; r < R1; ++r) {
            const int32_t* p = perms + off + r * m;
            memset(seen, 0, (size_t)m);
            for (int64_t v = 0; v < m; ++v) {
                XPS_CHECK_ARG(p[v] >= 0 && p[v] < m && !seen[p[v]], "a table row is not a permutation of [0, m)");
                XPS_CHECK_ARG(r > 0 || p[v] == v, "row 0 of a table is not the identity");
                seen[p[v]] = 1;
            }
        }
    }
    for (int q = 0; q < n_pairs; ++q) {
        const int64_t* P = pairs + (size_t)XPS_RSA_PAIR_WORDS * q;
        XPS_CHECK_ARG(P[CP_A] != 0 && P[CP_B] != 0, "null matrix");
        XPS_CHECK_ARG(P[CP_M] >= 2 && P[CP_M] <= MAXC, "m outside 2 .. XPS_RSA_MAX_CONDITIONS");
        XPS_CHECK_ARG(P[CP_NA] >= 1 && P[CP_NA] <= INT32_MAX && P[CP_NB] >= 1 && P[CP_NB] <= INT32_MAX, "a matrix size outside int32");
        XPS_CHECK_ARG(P[CP_LDA] >= P[CP_NA], "lda < n");
        XPS_CHECK_ARG(P[CP_LDB] >= P[CP_NB], "ldb < n");
        XPS_CHECK_ARG(P[CP_TABLE] >= 0 && P[CP_TABLE] < n_tables, "a pair names no permutation table");
        XPS_CHECK_ARG(tables[2 * (size_t)P[CP_TABLE] + 1] == P[CP_M], "a pair's table has another m");
        XPS_CHECK_ARG(P[CP_ROW] >= 0 && P[CP_ROW] < n_rows, "an output row outside the outputs");
        XPS_CHECK_ARG(P[CP_IA] >= 0 && P[CP_IA] <= n_idx - P[CP_M] && P[CP_IB] >= 0 && P[CP_IB] <= n_idx - P[CP_M],
                      "an index list reaches outside idx");
        for (int64_t v = 0; v < P[CP_M]; ++v) {
            const int32_t a = idx[P[CP_IA] + v], b = idx[P[CP_IB] + v];
            XPS_CHECK_ARG(a >= 0 && a < P[CP_NA] && b >= 0 && b < P[CP_NB], "an index at or past the matrix size");
        }
    }
    XPS_CHECK_ARG(ws, "null workspace");
    XPS_CHECK_ARG(ws_bytes >= xps_rdm_compare_perm_f64_workspace(n_pairs, n_tables, n_idx, n_perm), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const size_t pair_bytes = sizeof(long long) * XPS_RSA_PAIR_WORDS * (size_t)n_pairs, table_bytes = 2 * sizeof(long long) * (size_t)n_tables;
    const size_t idx_bytes = sizeof(int) * (size_t)n_idx, perm_bytes = sizeof(int) * (size_t)n_perm;
    char* base = static_cast<char*>(ws);
    long long* pairs_d = reinterpret_cast<long long*>(base);
    long long* tables_d = reinterpret_cast<long long*>(base + align8(pair_bytes));
    int* idx_d = reinterpret_cast<int*>(base + align8(pair_bytes) + align8(table_bytes));
    int* perms_d = reinterpret_cast<int*>(base + align8(pair_bytes) + align8(table_bytes) + align8(idx_bytes));
    hipError_t e = hipMemcpyAsync(pairs_d, pairs, pair_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(tables_d, tables, table_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(idx_d, idx, idx_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(perms_d, perms, perm_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { xps_set_error("%s: copying the tables failed: %s", __func__, hipGetErrorString(e)); return XPS_E_HIP; }
    hipLaunchKernelGGL(rdm_stats_kernel, dim3(n_pairs), dim3(64), 0, st, (const long long*)pairs_d, (const int*)idx_d, cosine, stats);
    XPS_CHECK_LAUNCH();
    hipLaunchKernelGGL(rdm_cross_kernel, dim3(n_pairs, (unsigned)((R1 + CW - 1) / CW)), dim3(64 * CW), 0, st, (const long long*)pairs_d,
                       (const long long*)tables_d, (const int*)idx_d, (const int*)perms_d, (int)R1, (const double*)stats, cross);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
