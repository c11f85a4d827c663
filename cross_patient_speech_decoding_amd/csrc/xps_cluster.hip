// Cluster separability scores for gfx950 (alignment/metrics.py): label-grouped sums over ONE n x n Gram matrix
// for many label vectors at once -- the true labels, the shuffles of a permutation null, other labellings of the same trials.
//
//  xps_label_row_sums_f64         S[r][i][q] = sum over j with y_r[j] = q of f(i, j), j ascending; f = G[i][j] (mode 0) or the
//                                 euclidean distance sqrt(max(G[i][i] + G[j][j] - 2 G[i][j], 0)) (mode 1; no n x n distance matrix
//                                 is stored).  One 64-lane workgroup per (row i, block of 64 label sets): a lane owns one label set
//                                 and keeps its k bins in LDS as [class][lane]; the row of G is turned into f in LDS segments that
//                                 every lane reads as a broadcast, so the row crosses HBM once per 64 label sets.
//  xps_label_col_sums_f64         M[r][p][c] = sum over i with y_r[i] = p of V[r][i][c], i ascending; one thread per output.
//  xps_silhouette_from_sums_f64   sklearn's silhouette rules on the mode-1 sums; one wave per label set, which also takes the set's
//                                 mean, mean of the positive values and their count (lane-strided adds, then wave_sum_f64).
//  xps_centroid_dist_from_sums_f64  distance of every sample to the centroid of its own class, from the mode-0 sums.
//
// Float64 throughout, no atomics; every sum is taken by one lane in ascending index order (the three statistics by the fixed
// butterfly), so a label set's results do not depend on the grid, the stream or the other label sets of the launch.  A label
// >= k is skipped, never used as an index.  The per-set class counts are HOST tables: the entries check them and copy them into
// the caller's workspace on the stream.
#include "xps_common.h"

namespace {

constexpr int LANES = 64;      // label sets per workgroup of label_row_sums_kernel: one per lane
constexpr int SEG = 256;       // elements of a row of G turned into f per LDS segment

__global__ __launch_bounds__(LANES) void label_row_sums_kernel(const double* __restrict__ G, long long ldg,
                                                               const uint8_t* __restrict__ labels_t, int n, int R, int k, int mode,
                                                               double* __restrict__ S) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* bins = lds;                       // [k][LANES]: lane l's bin q at q * LANES + l (consecutive lanes, consecutive banks)
    double* seg = lds + (size_t)k * LANES;    // [SEG]
    const int lane = threadIdx.x, i = blockIdx.x, r0 = blockIdx.y * LANES, r = r0 + lane;
    for (int q = 0; q < k; ++q) bins[q * LANES + lane] = 0.0;
    const double* row = G + (long long)i * ldg;
    const double gii = row[i];
    for (int j0 = 0; j0 < n; j0 += SEG) {
        const int m = min(SEG, n - j0);
        __syncthreads();                      // the previous segment has been consumed
        for (int t = lane; t < m; t += LANES) {
            const int j = j0 + t;
            double v = row[j];
            if (mode) {
                // sklearn's euclidean_distances expression; each operation rounds once (no contraction into an fma)
                const double d2 = __dsub_rn(__dadd_rn(gii, G[(long long)j * ldg + j]), __dmul_rn(2.0, v));
                v = (j != i && d2 > 0.0) ? __dsqrt_rn(d2) : 0.0;
            }
            seg[t] = v;
        }
        __syncthreads();
        if (r < R) {
            const uint8_t* lab = labels_t + (long long)j0 * R + r;
#pragma unroll 4
            for (int t = 0; t < m; ++t) {
                const int y = lab[(long long)t * R];
                if (y < k) bins[y * LANES + lane] += seg[t];
            }
        }
    }
    __syncthreads();
    // S[r][i][0 .. k): the k bins of a label set are contiguous in the output
    const int sets = min(LANES, R - r0);
    for (int e = lane; e < sets * k; e += LANES) {
        const int rr = e / k, q = e - rr * k;
        S[((long long)(r0 + rr) * n + i) * k + q] = bins[q * LANES + rr];
    }
}

__global__ __launch_bounds__(256) void label_col_sums_kernel(const double* __restrict__ V, long long v_set_stride,
                                                             const uint8_t* __restrict__ labels_t, int n, int R, int k, int w,
                                                             double* __restrict__ M) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)R * k * w) return;
    const int c = (int)(e % w), p = (int)((e / w) % k);
    const long long r = e / ((long long)w * k);
    const double* v = V + r * v_set_stride + c;
    const uint8_t* lab = labels_t + r;
    double acc = 0.0;
#pragma unroll 4
    for (int i = 0; i < n; ++i)
        if (lab[(long long)i * R] == p) acc += v[(long long)i * w];
    M[e] = acc;
}

// One wave per label set.  s follows sklearn.metrics.silhouette_samples: a = own-class sum / (count - 1), b = the smallest
// sum / count over the other non-empty classes, s = (b - a) / max(a, b); 0 for a sample alone in its class and for 0 / 0.
__global__ __launch_bounds__(64) void silhouette_kernel(const double* __restrict__ S, const int* __restrict__ counts,
                                                        const uint8_t* __restrict__ labels_t, int n, int R, int k,
                                                        double* __restrict__ sil, double* __restrict__ stats) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int* cnt = counts + (long long)r * k;
    double sum = 0.0, pos = 0.0, npos = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double* Si = S + ((long long)r * n + i) * k;
        const int y = labels_t[(long long)i * R + r];
        double s = 0.0;
        if (y < k && cnt[y] > 1) {
            double a = 0.0, b = 0.0;
            bool other = false;
            for (int q = 0; q < k; ++q) {
                const int c = cnt[q];
                if (q == y) a = Si[q] / (double)(c - 1);
                else if (c > 0) {
                    const double m = Si[q] / (double)c;
                    b = (!other || m < b) ? m : b;
                    other = true;
                }
            }
            const double big = a > b ? a : b;
            if (other && big > 0.0) s = (b - a) / big;
        }
        sil[(long long)r * n + i] = s;
        sum += s;
        if (s > 0.0) { pos += s; npos += 1.0; }
    }
    sum = wave_sum_f64(sum);
    pos = wave_sum_f64(pos);
    npos = wave_sum_f64(npos);
    if (lane == 0) {
        stats[3 * (long long)r] = sum / (double)n;
        stats[3 * (long long)r + 1] = pos / npos;          // 0 / 0 = NaN: np.mean of an empty selection
        stats[3 * (long long)r + 2] = npos;
    }
}

// dist[r][i] = sqrt(max(G[i][i] - 2 S0[r][i][p] / n_p + M[r][p][p] / n_p^2, 0)), p = y_r[i]: |x_i - centroid of its class|
__global__ __launch_bounds__(256) void centroid_dist_kernel(const double* __restrict__ G, long long ldg, const double* __restrict__ S0,
                                                            const double* __restrict__ M, const int* __restrict__ counts,
                                                            const uint8_t* __restrict__ labels_t, int n, int R, int k,
                                                            double* __restrict__ dist) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)R * n) return;
    const long long r = e / n;
    const int i = (int)(e - r * n);
    const int p = labels_t[(long long)i * R + r];
    double d = 0.0;
    if (p < k && counts[r * k + p] > 0) {
        const double np = (double)counts[r * k + p];
        const double d2 = G[(long long)i * ldg + i] - 2.0 * S0[e * k + p] / np + M[(r * k + p) * k + p] / (np * np);
        d = d2 > 0.0 ? __dsqrt_rn(d2) : 0.0;
    }
    dist[e] = d;
}

inline size_t counts_bytes(int R, int k) { return (sizeof(int) * (size_t)R * (size_t)k + 7) & ~(size_t)7; }

// The (R, k) class counts of a call: every count in [0, n], every set's counts add up to n.  HOST table.
bool counts_ok(const int32_t* counts, int n, int R, int k) {
    for (int r = 0; r < R; ++r) {
        long long tot = 0;
        for (int q = 0; q < k; ++q) {
            const int32_t c = counts[(size_t)r * k + q];
            if (c < 0 || c > n) return false;
            tot += c;
        }
        if (tot != n) return false;
    }
    return true;
}

}  // namespace

#define XPS_CLUSTER_SHAPE_OK(n, R, k) ((n) >= 1 && (R) >= 1 && (k) >= 2 && (k) <= XPS_CLUSTER_MAX_CLASSES)

extern "C" int xps_label_row_sums_f64(const double* G, int64_t ldg, const uint8_t* labels_t, int n, int R, int k, int mode,
                                      double* S, void* stream) {
    XPS_CHECK_ARG(G && labels_t && S, "null argument");
    XPS_CHECK_ARG(XPS_CLUSTER_SHAPE_OK(n, R, k), "n >= 1, R >= 1 and 2 <= k <= 64 are needed");
    XPS_CHECK_ARG(ldg >= n, "ldg < n");
    XPS_CHECK_ARG(mode == 0 || mode == 1, "mode must be 0 or 1");
    XPS_CHECK_ARG(cdiv(R, LANES) <= 65535, "more than 65535 * 64 label sets in one call");
    const size_t lds = sizeof(double) * ((size_t)k * LANES + SEG);
    hipLaunchKernelGGL(label_row_sums_kernel, dim3(n, cdiv(R, LANES)), dim3(LANES), lds, (hipStream_t)stream, G, (long long)ldg,
                       labels_t, n, R, k, mode, S);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_label_col_sums_f64(const double* V, int64_t v_set_stride, const uint8_t* labels_t, int n, int R, int k, int w,
                                      double* M, void* stream) {
    XPS_CHECK_ARG(V && labels_t && M, "null argument");
    XPS_CHECK_ARG(XPS_CLUSTER_SHAPE_OK(n, R, k), "n >= 1, R >= 1 and 2 <= k <= 64 are needed");
    XPS_CHECK_ARG(w >= 1, "w < 1");
    XPS_CHECK_ARG(v_set_stride == 0 || v_set_stride >= (int64_t)n * w, "v_set_stride must be 0 (one V for all sets) or >= n * w");
    XPS_CHECK_ARG(V != M, "V and M must differ");
    const long long total = (long long)R * k * w;
    XPS_CHECK_ARG(total <= 256LL * INT32_MAX, "R * k * w beyond the grid");
    hipLaunchKernelGGL(label_col_sums_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, V, (long long)v_set_stride,
                       labels_t, n, R, k, w, M);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" size_t xps_silhouette_from_sums_f64_workspace(int R, int k) {
    if (R < 1 || k < 1) return 0;
    return counts_bytes(R, k);
}

extern "C" int xps_silhouette_from_sums_f64(const double* S, const int32_t* counts, const uint8_t* labels_t, int n, int R, int k,
                                            double* sil, double* stats, void* ws, size_t ws_bytes, void* stream) {
    XPS_CHECK_ARG(S && counts && labels_t && sil && stats, "null argument");
    XPS_CHECK_ARG(XPS_CLUSTER_SHAPE_OK(n, R, k), "n >= 1, R >= 1 and 2 <= k <= 64 are needed");
    XPS_CHECK_ARG(counts_ok(counts, n, R, k), "the class counts of a label set are negative or do not add up to n");
    XPS_CHECK_ARG(ws, "null workspace");
    XPS_CHECK_ARG(ws_bytes >= xps_silhouette_from_sums_f64_workspace(R, k), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(ws, counts, sizeof(int) * (size_t)R * k, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { xps_set_error("%s: copying the counts failed: %s", __func__, hipGetErrorString(e)); return XPS_E_HIP; }
    hipLaunchKernelGGL(silhouette_kernel, dim3(R), dim3(64), 0, st, S, (const int*)ws, labels_t, n, R, k, sil, stats);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" size_t xps_centroid_dist_from_sums_f64_workspace(int R, int k) {
    if (R < 1 || k < 1) return 0;
    return counts_bytes(R, k);
}

extern "C" int xps_centroid_dist_from_sums_f64(const double* G, int64_t ldg, const double* S0, const double* M,
                                               const int32_t* counts, const uint8_t* labels_t, int n, int R, int k, double* dist,
                                               void* ws, size_t ws_bytes, void* stream) {
    XPS_CHECK_ARG(G && S0 && M && counts && labels_t && dist, "null argument");
    XPS_CHECK_ARG(XPS_CLUSTER_SHAPE_OK(n, R, k), "n >= 1, R >= 1 and 2 <= k <= 64 are needed");
    XPS_CHECK_ARG(ldg >= n, "ldg < n");
    XPS_CHECK_ARG(counts_ok(counts, n, R, k), "the class counts of a label set are negative or do not add up to n");
    XPS_CHECK_ARG(ws, "null workspace");
    XPS_CHECK_ARG(ws_bytes >= xps_centroid_dist_from_sums_f64_workspace(R, k), "workspace too small");
    const long long total = (long long)R * n;
    XPS_CHECK_ARG(total <= 256LL * INT32_MAX, "R * n beyond the grid");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(ws, counts, sizeof(int) * (size_t)R * k, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { xps_set_error("%s: copying the counts failed: %s", __func__, hipGetErrorString(e)); return XPS_E_HIP; }
    hipLaunchKernelGGL(centroid_dist_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, G, (long long)ldg, S0, M, (const int*)ws,
                       labels_t, n, R, k, dist);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
