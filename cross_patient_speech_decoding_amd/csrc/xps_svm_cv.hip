// Cross-validated SVC grid search for gfx950 (decoders/search.py; reference: GridSearchCV / BayesSearchCV over
// make_pipeline(DimRedReshape(PCA), SVC(kernel='rbf', class_weight='balanced')), scripts/aligned_decode_svm_ncv.py:398-402,422-425):
// what stands around ONE batched SMO launch (xps_svm.hip: xps_svm_smo_multi_f64) over the problems of all (candidate, fold) models.
//   rbf_multi_from_gram_kernel  one Gram matrix -> the kernel matrices of M gamma values, every Gram element read once;
//   svm_cv_score_kernel         a model's held-out rows (rows of its own kernel matrix) -> one-vs-one decisions -> libsvm's vote ->
//                               predictions and the k x k confusion counts of the model.
// The score kernel sums each decision in a fixed order and counts in integers: no atomics, results independent of the launch geometry.
#include "xps_common.h"
#include "xps_svm_rbf.h"
#include "xps_wave_first_max.h"

namespace {

// ---- kernel matrices of M gamma values ------------------------------------------------------------------------------------
// One thread per element of G: the element and the two norms are read once, the M results go to K + g * kstride.
__global__ __launch_bounds__(256) void rbf_multi_from_gram_kernel(const double* __restrict__ G, long long ldg, const double* __restrict__ na,
                                                                  const double* __restrict__ nb, int m, int n,
                                                                  const double* __restrict__ gammas, int M, double* __restrict__ K,
                                                                  long long ldk, long long kstride) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)m * n) return;
    const int i = (int)(e / n), j = (int)(e % n);
    const double a = na[i], b = nb[j], g = G[(long long)i * ldg + j];
    double* out = K + (long long)i * ldk + j;
    for (int t = 0; t < M; ++t) out[(long long)t * kstride] = xps_rbf_from_gram(gammas[t], a, b, g);
}

// ---- scoring --------------------------------------------------------------------------------------------------------------
constexpr int CV_THREADS = 256;
constexpr int CV_WAVES = CV_THREADS / 64;

// One workgroup of four waves per model s.  Held-out rows are taken four at a time, wave w the row i0 + w.  For each problem q of
// the model the lanes stride over its points (alpha and idx coalesced, K gathered inside the one row), every lane adds its terms
// in ascending t, and a butterfly of six exchanges -- the same order for every row and grid -- gives all lanes the sum; problem q
// votes pair_a[q] where sum - rho[q] > 0 STRICTLY, else pair_b[q]; lane c counts the votes of class c in a register and the wave's
// first maximum is the prediction.  After each round of four rows, thread 0 adds the (true, predicted) cells of the four waves, in
// wave order, to the k x k table in LDS; at the end the table is written out whole (zeros included).
// Nothing outside a model's matrix is dereferenced: a point index outside [0, mn[s]) adds no term; a held-out row outside it gets
// pred = -1, decisions of 0 and no count; a true class outside [0, k) is not counted; a pair class outside [0, k) matches no lane.
__global__ __launch_bounds__(CV_THREADS) void svm_cv_score_kernel(const double* __restrict__ K, const long long* __restrict__ mbase,
                                                                  const long long* __restrict__ mld, const int* __restrict__ mn,
                                                                  const int* __restrict__ idx, const int* __restrict__ off,
                                                                  const int* __restrict__ npos, const double* __restrict__ alpha,
                                                                  const double* __restrict__ rho, const int* __restrict__ pair_a,
                                                                  const int* __restrict__ pair_b, const int* __restrict__ mod_off,
                                                                  const int* __restrict__ tst, const int* __restrict__ ytrue,
                                                                  const int* __restrict__ tst_off, int k, int* __restrict__ pred,
                                                                  int* __restrict__ conf, double* __restrict__ dec_out, long long ldd) {
    __shared__ int s_conf[64 * 64];
    __shared__ int s_cell[CV_WAVES];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kk = k * k;
    for (int t = tid; t < kk; t += CV_THREADS) s_conf[t] = 0;
    const int q0 = mod_off[s], q1 = mod_off[s + 1];
    const int t0 = tst_off[s], nt = tst_off[s + 1] - t0;
    const int n = mn[s];
    const long long ld = mld[s];
    const double* Km = K + mbase[s];
    __syncthreads();
    for (int i0 = 0; i0 < nt; i0 += CV_WAVES) {                 // (block-uniform trip count: the barriers below are reached by all)
        const int i = i0 + wave;
        int cell = -1;
        if (i < nt) {
            const int r = tst[t0 + i];
            const bool row_ok = r >= 0 && r < n;
            const double* Kr = Km + (long long)(row_ok ? r : 0) * ld;
            int mine = 0;                                       // votes of class `lane` on this row
            for (int q = q0; q < q1; ++q) {
                const int o0 = off[q], cnt = off[q + 1] - o0, np = npos[q];
                double acc = 0.0;
                if (row_ok) {
                    for (int t = lane; t < cnt; t += 64) {
                        const int j = idx[o0 + t];
                        if (j >= 0 && j < n) {
                            const double a = alpha[o0 + t];
                            acc += (t < np ? a : -a) * Kr[j];
                        }
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
                const double dec = row_ok ? acc - rho[q] : 0.0;
                if (dec_out && lane == 0) dec_out[(long long)(t0 + i) * ldd + (q - q0)] = dec;
                const int win = dec > 0.0 ? pair_a[q] : pair_b[q];
                mine += (win == lane);
            }
            int v = lane < k ? mine : -1, c = lane;
            wave_first_max(v, c);
            const int p = row_ok ? c : -1;
            const int y = ytrue[t0 + i];
            if (lane == 0) pred[t0 + i] = p;
            if (p >= 0 && y >= 0 && y < k) cell = y * k + p;
        }
        if (lane == 0) s_cell[wave] = cell;
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 0; w < CV_WAVES; ++w) {
                const int c = s_cell[w];
                if (c >= 0) ++s_conf[c];
            }
        }
        __syncthreads();
    }
    int* out = conf + (long long)s * kk;
    for (int t = tid; t < kk; t += CV_THREADS) out[t] = s_conf[t];
}

}  // namespace

extern "C" int xps_rbf_multi_from_gram_f64(const double* G, int64_t ldg, const double* na, const double* nb, int m, int n,
                                           const double* gammas, int M, double* K, int64_t ldk, int64_t kstride, void* stream) {
    XPS_CHECK_ARG(G && na && nb && gammas && K, "null argument");
    XPS_CHECK_ARG(m >= 0 && n >= 0 && M >= 0 && ldg >= n && ldk >= n, "bad argument");
    XPS_CHECK_ARG(M <= 1 || m == 0 || kstride >= (int64_t)(m - 1) * ldk + n, "kstride: the matrices overlap");
    if (m == 0 || n == 0 || M == 0) return XPS_OK;
    hipLaunchKernelGGL(rbf_multi_from_gram_kernel, dim3(cdiv((long long)m * n, 256)), dim3(256), 0, (hipStream_t)stream, G, (long long)ldg, na,
                       nb, m, n, gammas, M, K, (long long)ldk, (long long)kstride);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" size_t xps_svm_cv_score_f64_workspace(int S) { return S < 0 ? 0 : 2 * ((size_t)S + 1) * sizeof(int); }

extern "C" int xps_svm_cv_score_f64(const double* K, const int64_t* mbase, const int64_t* mld, const int* mn, const int* idx, const int* off,
                                    const int* npos, const double* alpha, const double* rho, const int* pair_a, const int* pair_b,
                                    const int* mod_off, const int* tst, const int* ytrue, const int* tst_off, int S, int k, int* pred,
                                    int* conf, double* dec_out, int64_t ldd, void* ws, size_t ws_bytes, void* stream) {
    XPS_CHECK_ARG(K && mbase && mld && mn && idx && off && npos && alpha && rho && pair_a && pair_b && mod_off && tst && ytrue && tst_off &&
                  pred && conf && ws, "null argument");
    XPS_CHECK_ARG(k >= 2 && k <= 64, "k must be in 2..64 (one lane of a wave per class)");
    XPS_CHECK_ARG(S >= 0 && ws_bytes >= xps_svm_cv_score_f64_workspace(S), "bad parameter");
    XPS_CHECK_ARG(mod_off[0] >= 0 && tst_off[0] >= 0, "mod_off / tst_off must start at or above 0");
    int most = 0;
    for (int s = 0; s < S; ++s) {                                   // mod_off / tst_off are HOST arrays: checked here, then copied
        XPS_CHECK_ARG(mod_off[s + 1] >= mod_off[s], "mod_off must ascend");
        XPS_CHECK_ARG(tst_off[s + 1] >= tst_off[s], "tst_off must ascend");
        most = mod_off[s + 1] - mod_off[s] > most ? mod_off[s + 1] - mod_off[s] : most;
    }
    XPS_CHECK_ARG(!dec_out || ldd >= most, "ldd is smaller than a model's problem count");
    if (S == 0) return XPS_OK;
    int* offs = static_cast<int*>(ws);
    const size_t bytes = ((size_t)S + 1) * sizeof(int);
    hipError_t e = hipMemcpyAsync(offs, mod_off, bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpyAsync(offs + S + 1, tst_off, bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) { xps_set_error("%s: copying the offsets failed: %s", __func__, hipGetErrorString(e)); return XPS_E_HIP; }
    static_assert(sizeof(long long) == sizeof(int64_t), "mbase / mld are read as long long");
    hipLaunchKernelGGL(svm_cv_score_kernel, dim3(S), dim3(CV_THREADS), 0, (hipStream_t)stream, K, reinterpret_cast<const long long*>(mbase),
                       reinterpret_cast<const long long*>(mld), mn, idx, off, npos, alpha, rho, pair_a, pair_b, offs, tst, ytrue, offs + S + 1, k,
                       pred, conf, dec_out, (long long)ldd);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
