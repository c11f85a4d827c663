// Fold-batched PCA in front of the SVC search for gfx950: one Gram matrix of all trials serves every fold, one score matrix per
// fold serves every component count.
//
//  xps_gram_center_folds_f64   Kc_f[a][b] = G[r_a][r_b] - m[a] - m[b] + mm for every fold f of a split, from the N x N Gram matrix G
//                              of all trials about ONE centre: the Gram matrix of a fold's rows about the mean of ITS training rows.
//                              m[a] = (1 / n_tr) sum_{t < n_tr} G[r_a][r_t], mm = (1 / n_tr) sum_{b < n_tr} m[b].  A row mean is summed
//                              by one wave: lane l adds its terms t = l, l + 64, ... in ascending order from 0, then the 64 partial
//                              sums meet in a fixed xor butterfly (32, 16, 8, 4, 2, 1).  No atomics: the bits do not depend on the
//                              grid or on the run.  A workgroup owns a block of rows of one fold and walks the columns with
//                              consecutive threads, so a row of G is gathered by neighbouring lanes.
//  xps_prefix_kernels_f64      the linear / rbf kernel matrices of the column prefixes Z[:, :r] of a table of score matrices: one
//                              thread owns element (i, j), accumulates acc = fma(z_ik, z_jk, acc) for k ascending and writes every
//                              output of a cut r when k reaches it, then goes on.  The squared norms run through the same chain on
//                              the staged rows, so na_i is element (i, i) bit for bit and the rbf diagonal is exactly 1.  Plain
//                              v_fma_f64: the products are tiny (n^2 R <= 144^2 * 143), the cuts arbitrary, and the matrices of a
//                              cut are those of Z[:, :r] alone bit for bit.  Z is read once for all cuts and all gammas.
//
// Both entries take their small tables as HOST arrays, check them, and copy them into a DEVICE workspace on the stream
// (xps_svm_cv_score_f64 does the same with its offsets): what a kernel indexes with has been checked by the call that launches it.
#include <math.h>
#include <vector>
#include "xps_common.h"
#include "xps_svm_rbf.h"

namespace {

constexpr int GC_ROWS = 16;          // rows of a fold per workgroup of xps_gram_center_folds_f64
constexpr int GC_WORDS = 4;          // per fold in the workspace: list offset, n_all, n_tr, first element of Kc_f
constexpr int PK_T = 16, PK_K = 32;  // xps_prefix_kernels_f64: 16 x 16 outputs per workgroup, 32 columns of Z per stage
enum { PK_Z, PK_LDZ, PK_N, PK_R, PK_CUT0, PK_CUT1, PK_WORDS_USED };
static_assert(PK_WORDS_USED <= XPS_PREFIX_KERNELS_WORDS, "problem words");

// flag[0] = 1 if an index of the list lies outside [0, N)
__global__ void gc_check_rows_kernel(const int* __restrict__ rows, long long total, int N, long long* flag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total && (rows[i] < 0 || rows[i] >= N)) flag[0] = 1;
}

// One wave per row a of fold blockIdx.y: m[off + a] = (1 / n_tr) sum_t G[r_a][r_t].
__global__ __launch_bounds__(256) void gc_row_mean_kernel(const double* __restrict__ G, long long ldg, const int* __restrict__ rows,
                                                          const long long* __restrict__ folds, double* __restrict__ m) {
    const long long* F = folds + (long long)blockIdx.y * GC_WORDS;
    const long long off = F[0];
    const int n_all = (int)F[1], n_tr = (int)F[2];
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= n_all) return;                                   // (a whole wave leaves: the butterfly below stays complete)
    const double* g = G + (long long)rows[off + a] * ldg;
    double s = 0.0;
    for (int t = lane; t < n_tr; t += 64) s += g[rows[off + t]];
    s = wave_sum_f64(s);
    if (lane == 0) m[off + a] = s / (double)n_tr;
}

// One workgroup per block of GC_ROWS rows of fold blockIdx.y: wave 0 forms mm, then every thread walks the columns.
__global__ __launch_bounds__(256) void gc_center_kernel(const double* __restrict__ G, long long ldg, const int* __restrict__ rows,
                                                        const long long* __restrict__ folds, const double* __restrict__ m,
                                                        double* __restrict__ Kc) {
    __shared__ double mm_s;
    const long long* F = folds + (long long)blockIdx.y * GC_WORDS;
    const long long off = F[0];
    const int n_all = (int)F[1], n_tr = (int)F[2];
    const int a0 = blockIdx.x * GC_ROWS;
    if (a0 >= n_all) return;
    if (threadIdx.x < 64) {
        double s = 0.0;
        for (int b = threadIdx.x; b < n_tr; b += 64) s += m[off + b];
        s = wave_sum_f64(s);
        if (threadIdx.x == 0) mm_s = s / (double)n_tr;
    }
    __syncthreads();
    const double mm = mm_s;
    double* out = Kc + F[3];
    const int a1 = min(n_all, a0 + GC_ROWS);
    for (int a = a0; a < a1; ++a) {
        const double* g = G + (long long)rows[off + a] * ldg;
        const double ma = m[off + a];
        for (int b = threadIdx.x; b < n_tr; b += 256)
            out[(long long)a * n_tr + b] = ((g[rows[off + b]] - ma) - m[off + b]) + mm;
    }
}

// One workgroup per {problem, row tile, column tile}: thread (ti, tj) owns element (i0 + ti, j0 + tj).
__global__ __launch_bounds__(256) void prefix_kernels_kernel(const long long* __restrict__ probs, const int* __restrict__ cuts,
                                                             const int* __restrict__ cut_out, const double* __restrict__ gammas,
                                                             const long long* __restrict__ dest, const int* __restrict__ tiles,
                                                             int rbf, double* __restrict__ K) {
    __shared__ double Zi[PK_T][PK_K + 1];
    __shared__ double Zj[PK_T][PK_K + 1];
    const int* tl = tiles + 3 * (long long)blockIdx.x;
    const long long* P = probs + (long long)tl[0] * XPS_PREFIX_KERNELS_WORDS;
    const double* Z = reinterpret_cast<const double*>(P[PK_Z]);
    const long long ldz = P[PK_LDZ];
    const int n = (int)P[PK_N], R = (int)P[PK_R], cut1 = (int)P[PK_CUT1];
    int c = (int)P[PK_CUT0];
    const int i0 = tl[1] * PK_T, j0 = tl[2] * PK_T;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int i = i0 + ti, j = j0 + tj;
    const int last = min(R, cuts[cut1 - 1]);                  // nothing is read past the last cut
    int next = cuts[c];
    double acc = 0.0, ni = 0.0, nj = 0.0;
    for (int k0 = 0; k0 < last; k0 += PK_K) {
        // stage rows i0.. and j0.., columns k0 .. k0 + 31: thread t takes row t >> 4, columns 2 (t & 15) and + 1
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int kk = 2 * tj + e, k = k0 + kk;
            Zi[ti][kk] = (i < n && k < last) ? Z[(long long)i * ldz + k] : 0.0;
            Zj[ti][kk] = (j0 + ti < n && k < last) ? Z[(long long)(j0 + ti) * ldz + k] : 0.0;
        }
        __syncthreads();
        const int kend = min(PK_K, last - k0);
        for (int kk = 0; kk < kend; ++kk) {
            const double a = Zi[ti][kk], b = Zj[tj][kk];
            acc = fma(a, b, acc);
            ni = fma(a, a, ni);
            nj = fma(b, b, nj);
            if (k0 + kk + 1 == next) {                        // (uniform over the workgroup)
                if (i < n && j < n) {
                    const long long e = (long long)i * n + j;
                    for (int o = cut_out[c]; o < cut_out[c + 1]; ++o)
                        K[dest[o] + e] = rbf ? xps_rbf_from_gram(gammas[o], ni, nj, acc) : acc;
                }
                ++c;
                next = c < cut1 ? cuts[c] : -1;
            }
        }
        __syncthreads();
    }
}

inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace

extern "C" size_t xps_gram_center_folds_f64_workspace(int n_folds, int64_t total_rows) {
    if (n_folds < 0 || total_rows < 0) return 0;
    return sizeof(long long) * (1 + (size_t)GC_WORDS * n_folds) + sizeof(double) * (size_t)total_rows;
}

extern "C" int xps_gram_center_folds_f64(const double* G, int64_t ldg, int N, const int32_t* rows, const int32_t* fold_off,
                                         const int32_t* n_train, int n_folds, double* Kc, void* ws, size_t ws_bytes, void* stream) {
    XPS_CHECK_ARG(G && rows && fold_off && n_train && Kc && ws, "null argument");
    XPS_CHECK_ARG(N >= 1 && ldg >= N && n_folds >= 0 && n_folds <= 65535, "bad parameter");
    XPS_CHECK_ARG(fold_off[0] == 0, "fold_off must start at 0");
    std::vector<long long> meta(1 + (size_t)GC_WORDS * n_folds, 0);
    long long kc = 0;
    int max_all = 0;
    for (int f = 0; f < n_folds; ++f) {                            // fold_off / n_train are HOST arrays: checked here, then copied
        XPS_CHECK_ARG(fold_off[f + 1] >= fold_off[f], "fold_off must ascend");
        const int n_all = fold_off[f + 1] - fold_off[f];
        XPS_CHECK_ARG(n_train[f] >= 1 && n_train[f] <= n_all, "n_train must be in 1..the fold's row count");
        long long* F = meta.data() + 1 + (size_t)GC_WORDS * f;
        F[0] = fold_off[f]; F[1] = n_all; F[2] = n_train[f]; F[3] = kc;
        kc += (long long)n_all * n_train[f];
        max_all = n_all > max_all ? n_all : max_all;
    }
    if (n_folds == 0) return XPS_OK;
    const long long total = fold_off[n_folds];
    XPS_CHECK_ARG(ws_bytes >= xps_gram_center_folds_f64_workspace(n_folds, total), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    long long* meta_d = static_cast<long long*>(ws);
    double* m_d = reinterpret_cast<double*>(meta_d + meta.size());
    long long bad = 0;
    hipError_t e = hipMemcpyAsync(meta_d, meta.data(), meta.size() * sizeof(long long), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(gc_check_rows_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, rows, total, N, meta_d);
        e = hipGetLastError();
    }
    // the row list is a DEVICE array: its check runs there, and the call waits for the verdict before anything indexes G with it
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, meta_d, sizeof(long long), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { xps_set_error("%s: checking the row list failed: %s", __func__, hipGetErrorString(e)); return XPS_E_HIP; }
    XPS_CHECK_ARG(bad == 0, "a row index lies outside [0, N)");
    hipLaunchKernelGGL(gc_row_mean_kernel, dim3(cdiv(max_all, 4), n_folds), dim3(256), 0, st, G, (long long)ldg, rows, meta_d + 1, m_d);
    XPS_CHECK_LAUNCH();
    hipLaunchKernelGGL(gc_center_kernel, dim3(cdiv(max_all, GC_ROWS), n_folds), dim3(256), 0, st, G, (long long)ldg, rows, meta_d + 1,
                       m_d, Kc);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" size_t xps_prefix_kernels_f64_workspace(int n_problems, int n_cuts, int n_out, int n_tiles) {
    if (n_problems < 0 || n_cuts < 0 || n_out < 0 || n_tiles < 0) return 0;
    return align8(sizeof(long long) * XPS_PREFIX_KERNELS_WORDS * (size_t)n_problems) + align8(sizeof(int) * (size_t)n_cuts) +
           align8(sizeof(int) * ((size_t)n_cuts + 1)) + 2 * sizeof(double) * (size_t)n_out + align8(3 * sizeof(int) * (size_t)n_tiles);
}

extern "C" int xps_prefix_kernels_f64(const int64_t* problems, int n_problems, const int32_t* cuts, const int32_t* cut_out, int n_cuts,
                                      const double* gammas, const int64_t* dest, int n_out, const int32_t* tiles, int n_tiles, int rbf,
                                      double* K, int64_t k_len, void* ws, size_t ws_bytes, void* stream) {
    XPS_CHECK_ARG(n_problems >= 0 && n_cuts >= 0 && n_out >= 0 && n_tiles >= 0 && k_len >= 0 && (rbf == 0 || rbf == 1), "bad parameter");
    if (n_problems == 0) return XPS_OK;
    XPS_CHECK_ARG(problems && cuts && cut_out && gammas && dest && tiles && K && ws, "null argument");
    XPS_CHECK_ARG(ws_bytes >= xps_prefix_kernels_f64_workspace(n_problems, n_cuts, n_out, n_tiles), "workspace too small");
    XPS_CHECK_ARG(cut_out[0] == 0 && cut_out[n_cuts] == n_out, "cut_out must run from 0 to n_out");
    for (int c = 0; c < n_cuts; ++c) XPS_CHECK_ARG(cut_out[c + 1] >= cut_out[c], "cut_out must ascend");
    for (int o = 0; o < n_out; ++o) XPS_CHECK_ARG(gammas[o] >= 0.0 && gammas[o] < INFINITY, "a gamma is negative or not finite");
    int at = 0;
    for (int p = 0; p < n_problems; ++p) {                         // every table is a HOST array: checked here, then copied
        const int64_t* P = problems + (size_t)XPS_PREFIX_KERNELS_WORDS * p;
        XPS_CHECK_ARG(P[PK_Z] != 0, "null score matrix");
        XPS_CHECK_ARG(P[PK_N] >= 1 && P[PK_N] <= 46340, "n must be in 1..46340");
        XPS_CHECK_ARG(P[PK_R] >= 1 && P[PK_R] < (1LL << 31) && P[PK_LDZ] >= P[PK_R], "R < 1 or ldz < R");
        XPS_CHECK_ARG(P[PK_CUT0] == at && P[PK_CUT1] > P[PK_CUT0] && P[PK_CUT1] <= n_cuts, "the cut lists must follow each other, none empty");
        at = (int)P[PK_CUT1];
        for (int c = (int)P[PK_CUT0]; c < at; ++c) {
            XPS_CHECK_ARG(cuts[c] >= 1 && cuts[c] <= P[PK_R], "a cut of 0 or beyond R");
            XPS_CHECK_ARG(c == P[PK_CUT0] || cuts[c] > cuts[c - 1], "cuts must ascend");
            for (int o = cut_out[c]; o < cut_out[c + 1]; ++o)
                XPS_CHECK_ARG(dest[o] >= 0 && dest[o] + P[PK_N] * P[PK_N] <= k_len, "an output reaches outside K");
        }
    }
    XPS_CHECK_ARG(at == n_cuts, "cuts that belong to no problem");
    for (int t = 0; t < n_tiles; ++t) {
        const int32_t* tl = tiles + 3 * (size_t)t;
        XPS_CHECK_ARG(tl[0] >= 0 && tl[0] < n_problems, "a tile names no problem");
        const int64_t nt = (problems[(size_t)XPS_PREFIX_KERNELS_WORDS * tl[0] + PK_N] + PK_T - 1) / PK_T;
        XPS_CHECK_ARG(tl[1] >= 0 && tl[1] < nt && tl[2] >= 0 && tl[2] < nt, "a tile lies outside its problem");
    }
    if (n_tiles == 0) return XPS_OK;
    static_assert(sizeof(long long) == sizeof(int64_t), "the tables are read as long long");
    hipStream_t st = (hipStream_t)stream;
    char* w = static_cast<char*>(ws);
    long long* probs_d = reinterpret_cast<long long*>(w);  w += align8(sizeof(long long) * XPS_PREFIX_KERNELS_WORDS * (size_t)n_problems);
    int* cuts_d = reinterpret_cast<int*>(w);               w += align8(sizeof(int) * (size_t)n_cuts);
    int* cut_out_d = reinterpret_cast<int*>(w);            w += align8(sizeof(int) * ((size_t)n_cuts + 1));
    double* gammas_d = reinterpret_cast<double*>(w);       w += sizeof(double) * (size_t)n_out;
    long long* dest_d = reinterpret_cast<long long*>(w);   w += sizeof(long long) * (size_t)n_out;
    int* tiles_d = reinterpret_cast<int*>(w);
    hipError_t e = hipMemcpyAsync(probs_d, problems, sizeof(long long) * XPS_PREFIX_KERNELS_WORDS * (size_t)n_problems, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cuts_d, cuts, sizeof(int) * (size_t)n_cuts, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(cut_out_d, cut_out, sizeof(int) * ((size_t)n_cuts + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n_out) e = hipMemcpyAsync(gammas_d, gammas, sizeof(double) * (size_t)n_out, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n_out) e = hipMemcpyAsync(dest_d, dest, sizeof(long long) * (size_t)n_out, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(tiles_d, tiles, 3 * sizeof(int) * (size_t)n_tiles, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { xps_set_error("%s: copying the tables failed: %s", __func__, hipGetErrorString(e)); return XPS_E_HIP; }
    hipLaunchKernelGGL(prefix_kernels_kernel, dim3(n_tiles), dim3(256), 0, st, probs_d, cuts_d, cut_out_d, gammas_d, dest_d, tiles_d, rbf, K);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
