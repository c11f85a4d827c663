// Bagged one-vs-one SVC ensemble for gfx950: what stands between ONE batched SMO launch (xps_svm.hip) over the E x P binary
// problems of a BaggingClassifier(SVC) (reference: scripts/aligned_decode_svm.py:262-263, n_estimators searched over 10..100 in
// scripts/aligned_decode_svm_ncv.py:151-159) and its prediction.  Two kernels:
//   bag_coef_scatter_kernel  packed alpha of the Q problems -> the dense signed coefficient matrix (Q x n), zeros included;
//   bag_vote_kernel          decision values (m x Q) -> per-estimator libsvm vote -> ensemble vote counts and prediction.
// Both are integer / copy work: no floating-point sums, no atomics, results independent of the launch geometry.
#include "xps_common.h"
#include "xps_wave_first_max.h"

namespace {

constexpr int BAG_THREADS = 256;
constexpr int BAG_WAVES = BAG_THREADS / 64;

// ---- coefficient scatter ------------------------------------------------------------------------------------------------
// Block (q, chunk): the columns [chunk * TILE, chunk * TILE + TILE) of row q are assembled in LDS -- zero fill, then the points of
// problem q that fall into the chunk, +alpha for the first npos[q] of them and -alpha for the others -- and written out as whole
// lines.  The row is never written twice, so there is no global write-after-write to order; a point index outside [0, n) is
// dropped.  Points of one problem are distinct rows of the kernel matrix (a repeated index would keep one of its values).
constexpr int SCATTER_TILE = 2048;      // doubles per chunk: 16 KiB of LDS

__global__ __launch_bounds__(BAG_THREADS) void bag_coef_scatter_kernel(const double* __restrict__ alpha, const int* __restrict__ idx,
                                                                       const int* __restrict__ off, const int* __restrict__ npos, int n,
                                                                       double* __restrict__ coef, long long ldc) {
    __shared__ double row[SCATTER_TILE];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int c0 = blockIdx.y * SCATTER_TILE;
    const int len = min(SCATTER_TILE, n - c0);
    const int o0 = off[q], cnt = off[q + 1] - o0, np = npos[q];
    for (int t = tid; t < len; t += BAG_THREADS) row[t] = 0.0;
    __syncthreads();
    for (int t = tid; t < cnt; t += BAG_THREADS) {
        const long long j = (long long)idx[o0 + t] - c0;
        if (j >= 0 && j < len) row[j] = t < np ? alpha[o0 + t] : -alpha[o0 + t];
    }
    __syncthreads();
    double* out = coef + (long long)q * ldc + c0;
    for (int t = tid; t < len; t += BAG_THREADS) out[t] = row[t];
}

// ---- vote ---------------------------------------------------------------------------------------------------------------
// One workgroup per test row.  The estimators are taken in groups whose problems fit the LDS stage (VOTE_STAGE winners, one byte
// each; an estimator has at most 64 * 63 / 2 = 2016 problems, so a group is never empty):
//   1. all 256 threads read the group's decision values -- consecutive problems of one row, i.e. whole lines -- with rho and the
//      pair, and store the problem's winning class: pair_a where dec - rho > 0 (strictly), else pair_b;
//   2. wave w takes the group's estimators w, w + 4, ...: lane c counts the winners equal to class c (every lane reads the same
//      byte: an LDS broadcast), the wave's first maximum is the estimator's class, and that lane adds one to its ensemble count.
// At the end the four waves' counts are added in wave order (integers) and wave 0 writes votes[r][:] and their first maximum.
// A malformed est_off cannot write out of bounds: problems outside [0, ld) are not read, a group is cut at VOTE_STAGE problems,
// and a class index outside [0, k) matches no lane.  An estimator without problems casts no vote.
constexpr int VOTE_STAGE = 4096;

__global__ __launch_bounds__(BAG_THREADS) void bag_vote_kernel(const double* __restrict__ dec, long long ld, const double* __restrict__ rho,
                                                               const int* __restrict__ pair_a, const int* __restrict__ pair_b,
                                                               const int* __restrict__ est_off, int E, int k, int* __restrict__ votes,
                                                               int* __restrict__ pred) {
    __shared__ unsigned char win[VOTE_STAGE];
    __shared__ int s_votes[BAG_WAVES][64];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* drow = dec + (long long)r * ld;
    int mine = 0;                                       // ensemble votes of class `lane` from this wave's estimators
    int e0 = 0;
    while (e0 < E) {                                    // (block-uniform: est_off is the same for every thread)
        const int q0 = est_off[e0];
        int e1 = e0 + 1;
        while (e1 < E && est_off[e1 + 1] - q0 <= VOTE_STAGE) ++e1;
        const int nq = min(est_off[e1] - q0, VOTE_STAGE);
        for (int t = tid; t < nq; t += BAG_THREADS) {
            const int q = q0 + t;
            int w = 255;
            if (q >= 0 && q < ld) w = (drow[q] - rho[q] > 0.0) ? pair_a[q] : pair_b[q];
            win[t] = (unsigned char)(w >= 0 && w < 64 ? w : 255);
        }
        __syncthreads();
        for (int e = e0 + wave; e < e1; e += BAG_WAVES) {
            const int b = max(est_off[e] - q0, 0), end = min(est_off[e + 1] - q0, nq);
            int cnt = 0;
            for (int t = b; t < end; ++t) cnt += (win[t] == lane);
            int v = lane < k ? cnt : -1, c = lane;
            wave_first_max(v, c);
            if (end > b && lane == c) ++mine;
        }
        __syncthreads();
        e0 = e1;
    }
    s_votes[wave][lane] = mine;
    __syncthreads();
    if (wave == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < BAG_WAVES; ++w) total += s_votes[w][lane];
        if (lane < k) votes[(long long)r * k + lane] = total;
        int v = lane < k ? total : -1, c = lane;
        wave_first_max(v, c);
        if (lane == 0) pred[r] = c;
    }
}

}  // namespace

extern "C" int xps_bag_coef_scatter_f64(const double* alpha, const int* idx, const int* off, const int* npos, int nprob, int n,
                                        double* coef, int64_t ldc, void* stream) {
    XPS_CHECK_ARG(alpha && idx && off && npos && coef, "null argument");
    XPS_CHECK_ARG(nprob >= 0 && n >= 1 && ldc >= n, "bad parameter");
    if (nprob == 0) return XPS_OK;
    const int chunks = cdiv(n, SCATTER_TILE);
    XPS_CHECK_ARG(chunks <= 65535, "row too long");
    hipLaunchKernelGGL(bag_coef_scatter_kernel, dim3(nprob, chunks), dim3(BAG_THREADS), 0, (hipStream_t)stream, alpha, idx, off, npos, n,
                       coef, (long long)ldc);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_bag_vote_f64(const double* dec, int64_t ld, const double* rho, const int* pair_a, const int* pair_b, const int* est_off,
                                int m, int E, int k, int* votes, int* pred, void* stream) {
    XPS_CHECK_ARG(dec && rho && pair_a && pair_b && est_off && votes && pred, "null argument");
    XPS_CHECK_ARG(m >= 0 && E >= 1 && ld >= 1, "bad parameter");
    XPS_CHECK_ARG(k >= 2 && k <= 64, "k must be in 2..64 (one lane of a wave per class)");
    if (m == 0) return XPS_OK;
    hipLaunchKernelGGL(bag_vote_kernel, dim3(m), dim3(BAG_THREADS), 0, (hipStream_t)stream, dec, (long long)ld, rho, pair_a, pair_b, est_off,
                       E, k, votes, pred);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
