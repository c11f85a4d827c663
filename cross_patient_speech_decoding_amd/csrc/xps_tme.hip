// Tensor maximum entropy surrogates (surrogates/tme.py): random (n0, n1, n2) tensors that keep a data
// tensor's mean and its three marginal covariances (Elsayed & Cunningham 2017) and nothing else.
//
//  xps_tme_kron_pass_f64     the Newton iteration's device half, ragged over problems.  W_ijk = 1 / D_ijk, D_ijk = l0_i + l1_j +
//                            l2_k over the k0 x k1 x k2 box of a problem; the box is never stored.  Workgroup (a, problem) owns
//                            index a of ONE axis A and walks the plane of the other two, B then C in cyclic order: it writes the
//                            single marginals of W and W^2 at a and row a of the pairwise marginal of W^2 over (A, B).  The three
//                            roles A = 0, 1, 2 are the same code, so the outputs of a problem whose axes are rotated are the
//                            rotated outputs bit for bit.  Role 0 also leaves sum log D and the D <= 0 flag of its slab in the
//                            workspace; a second launch adds them per problem.
//  xps_tme_core_scale_f64    core = z * sqrt(W) for S surrogates of a problem, elementwise.
//  xps_tme_mode_product_f64  C[b] = A[b] op(B[b]) (+ add) for a batch of equally shaped products on the f64 MFMA tile, operands
//                            with a batch stride (0: shared).  The three mode products of a surrogate are three calls: the middle
//                            one is S k0 products Q_1 (n1 x k1) T[s][i] (k1 x n2) on the slices where they lie -- no transposed
//                            copy --, the last one adds the mean tensor and stores float32 when asked.
//
// No atomics; every sum is taken in an order that is a function of the problem alone.
#include <math.h>

#include "xps_f64_tile.h"

namespace {

// words of one xps_tme_kron_pass_f64 problem
enum { KP_K0, KP_K1, KP_K2, KP_L0, KP_L1, KP_L2, KP_W1_0, KP_W1_1, KP_W1_2, KP_W2_0, KP_W2_1, KP_W2_2, KP_P01, KP_LD01, KP_P02,
       KP_LD02, KP_P12, KP_LD12, KP_SCAL, KP_WORDS_USED };
static_assert(KP_WORDS_USED <= XPS_TME_KRON_WORDS, "problem words");

constexpr int MAXA = XPS_TME_MAX_AXIS;
constexpr int KT = 256;                // threads of a pass workgroup: 4 waves

// Workgroup (a of the concatenated axes, problem).  Wave w takes b = w, w + 4, ... of axis B; lane l takes c = l, l + 64, ... of
// axis C and adds its terms in that order; the 64 partial sums of a row meet in wave_sum_f64's butterfly, a wave adds its rows
// in ascending b, and the four waves meet as (w0 + w1) + (w2 + w3).
__global__ __launch_bounds__(KT) void kron_pass_kernel(const long long* __restrict__ probs, double* __restrict__ part) {
    __shared__ double sh[3][4];
    __shared__ int shbad[4];
    const long long* P = probs + (long long)blockIdx.y * XPS_TME_KRON_WORDS;
    const int k[3] = {(int)P[KP_K0], (int)P[KP_K1], (int)P[KP_K2]};
    int a = blockIdx.x, r;
    if (a < k[0]) r = 0;
    else if (a < k[0] + k[1]) { r = 1; a -= k[0]; }
    else if (a < k[0] + k[1] + k[2]) { r = 2; a -= k[0] + k[1]; }
    else return;
    const int rb = (r + 1) % 3, rc = (r + 2) % 3;
    const double* lA = reinterpret_cast<const double*>(P[KP_L0 + r]);
    const double* lB = reinterpret_cast<const double*>(P[KP_L0 + rb]);
    const double* lC = reinterpret_cast<const double*>(P[KP_L0 + rc]);
    const int kB = k[rb], kC = k[rc];
    // the pairwise marginal over (A, B) is element (a, b) of P01 (role 0), of P12 (role 1), and element (b, a) of P02 (role 2)
    double* pw;
    long long sa, sb;
    if (r == 0) { pw = reinterpret_cast<double*>(P[KP_P01]); sa = P[KP_LD01]; sb = 1; }
    else if (r == 1) { pw = reinterpret_cast<double*>(P[KP_P12]); sa = P[KP_LD12]; sb = 1; }
    else { pw = reinterpret_cast<double*>(P[KP_P02]); sa = 1; sb = P[KP_LD02]; }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double la = lA[a];
    double t1 = 0.0, t2 = 0.0, tl = 0.0;
    int bad = 0;
    for (int b = wave; b < kB; b += 4) {
        const double lab = la + lB[b];
        double s1 = 0.0, s2 = 0.0, sl = 0.0;
        for (int c = lane; c < kC; c += 64) {
            const double D = lab + lC[c];
            bad |= !(D > 0.0);
            const double w = 1.0 / D;
            s1 += w;
            s2 += w * w;
            if (r == 0) sl += log(D);
        }
        s1 = wave_sum_f64(s1);
        s2 = wave_sum_f64(s2);
        if (r == 0) sl = wave_sum_f64(sl);
        if (lane == 0) pw[a * sa + b * sb] = s2;
        t1 += s1;
        t2 += s2;
        tl += sl;
    }
    const int wave_bad = __any(bad);
    if (lane == 0) {
        sh[0][wave] = t1;
        sh[1][wave] = t2;
        sh[2][wave] = tl;
        shbad[wave] = wave_bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        reinterpret_cast<double*>(P[KP_W1_0 + r])[a] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
        reinterpret_cast<double*>(P[KP_W2_0 + r])[a] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
        if (r == 0) {
            double* mine = part + (long long)blockIdx.y * 2 * MAXA;
            mine[a] = (sh[2][0] + sh[2][1]) + (sh[2][2] + sh[2][3]);
            mine[MAXA + a] = (shbad[0] | shbad[1] | shbad[2] | shbad[3]) ? 1.0 : 0.0;
        }
    }
}

// One workgroup per problem: scal = {sum log D, number of axis-0 slabs that hold a D <= 0} from the slab values of role 0.
// Thread t adds the slabs t, t + 256, ... in ascending order; the 256 partial sums meet in a fixed tree.
__global__ __launch_bounds__(KT) void kron_finish_kernel(const long long* __restrict__ probs, const double* __restrict__ part) {
    __shared__ double red[2][KT];
    const long long* P = probs + (long long)blockIdx.x * XPS_TME_KRON_WORDS;
    const double* mine = part + (long long)blockIdx.x * 2 * MAXA;
    const int k0 = (int)P[KP_K0], tid = threadIdx.x;
    double sl = 0.0, sb = 0.0;
    for (int a = tid; a < k0; a += KT) {
        sl += mine[a];
        sb += mine[MAXA + a];
    }
    red[0][tid] = sl;
    red[1][tid] = sb;
    __syncthreads();
    for (int s = KT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* scal = reinterpret_cast<double*>(P[KP_SCAL]);
        scal[0] = red[0][0];
        scal[1] = red[1][0];
    }
}

// core[row][k] = z[row][k] * sqrt(1 / ((l0[i] + l1[j]) + l2[k])), row = (s k0 + i) k1 + j: D as the pass adds it.
__global__ __launch_bounds__(256) void core_scale_kernel(const double* __restrict__ z, long long ldz, const double* __restrict__ l0,
                                                         const double* __restrict__ l1, const double* __restrict__ l2, int k0, int k1,
                                                         int k2, long long total, double* __restrict__ core, long long ldc) {
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += step) {
        const int kk = (int)(e % k2);
        const long long row = e / k2;
        const int j = (int)(row % k1), i = (int)((row / k1) % k0);
        const double D = (l0[i] + l1[j]) + l2[kk];
        core[row * ldc + kk] = z[row * ldz + kk] * sqrt(1.0 / D);
    }
}

// Workgroup = (batch member, row tile, column tile), the column tile fastest.  C[b] = A[b] op(B[b]) + add on the 64 x 64 tile of
// xps_f64_tile.h, the contraction ascending.  A is stored [m][k]; B [k][n], or [n][k] with BK.
template <bool BK>
__global__ __launch_bounds__(256) void mode_product_kernel(const double* __restrict__ A, long long lda, long long sa,
                                                           const double* __restrict__ B, long long ldb, long long sb,
                                                           const double* __restrict__ add, long long ldadd, void* __restrict__ Cp,
                                                           int c_is_f32, long long ldc, long long sc, int M, int N, int K, int tm,
                                                           int tn) {
    __shared__ __attribute__((aligned(16))) double As[DK][DLD];
    __shared__ __attribute__((aligned(16))) double Bs[DK][DLD];
    const int tid = threadIdx.x;
    long long wg = blockIdx.x;
    const int n0 = (int)(wg % tn) * DN;
    wg /= tn;
    const int m0 = (int)(wg % tm) * DM;
    const long long b = wg / tm;
    const Mat64 a{A + b * sa, lda, nullptr, 0}, bm{B + b * sb, ldb, nullptr, 0};

    f64x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += DK) {
        stage_kc(a, As, m0, M, k0, K, tid);
        if (BK) stage_kc(bm, Bs, n0, N, k0, K, tid);
        else stage_xc(bm, Bs, n0, N, k0, K, tid);
        __syncthreads();
        mfma_f64_tile(As, Bs, acc, tid);
        __syncthreads();
    }
    store_f64_tile(acc, m0, n0, M, N, tid, [&](int row, int col, double v) {
        if (add) v += add[(long long)row * ldadd + col];
        const long long o = b * sc + (long long)row * ldc + col;
        if (c_is_f32) reinterpret_cast<float*>(Cp)[o] = (float)v;
        else reinterpret_cast<double*>(Cp)[o] = v;
    });
}

inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

}  // namespace

extern "C" size_t xps_tme_kron_pass_f64_workspace(int n_problems) {
    if (n_problems < 0) return 0;
    return align8(sizeof(long long) * XPS_TME_KRON_WORDS * (size_t)n_problems) + sizeof(double) * 2 * MAXA * (size_t)n_problems;
}

extern "C" int xps_tme_kron_pass_f64(const int64_t* problems, int n_problems, void* ws, size_t ws_bytes, void* stream) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the table is read as long long");
    XPS_CHECK_ARG(n_problems >= 0, "negative count");
    if (n_problems == 0) return XPS_OK;
    XPS_CHECK_ARG(problems, "null table");
    XPS_CHECK_ARG(n_problems <= 65535, "more than 65535 problems");
    int64_t most = 0;
    for (int p = 0; p < n_problems; ++p) {                         // the table is a HOST array: checked here, then copied
        const int64_t* P = problems + (size_t)XPS_TME_KRON_WORDS * p;
        for (int r = 0; r < 3; ++r) {
            XPS_CHECK_ARG(P[KP_K0 + r] >= 1 && P[KP_K0 + r] <= MAXA, "a box size outside 1 .. XPS_TME_MAX_AXIS");
            XPS_CHECK_ARG(P[KP_L0 + r] != 0, "null multipliers");
            XPS_CHECK_ARG(P[KP_W1_0 + r] != 0 && P[KP_W2_0 + r] != 0, "null marginal");
        }
        XPS_CHECK_ARG(P[KP_P01] != 0 && P[KP_P02] != 0 && P[KP_P12] != 0, "null marginal");
        XPS_CHECK_ARG(P[KP_SCAL] != 0, "null scalars");
        XPS_CHECK_ARG(P[KP_LD01] >= P[KP_K1], "ld01 < k1");
        XPS_CHECK_ARG(P[KP_LD02] >= P[KP_K2], "ld02 < k2");
        XPS_CHECK_ARG(P[KP_LD12] >= P[KP_K2], "ld12 < k2");
        const int64_t all = P[KP_K0] + P[KP_K1] + P[KP_K2];
        most = all > most ? all : most;
    }
    XPS_CHECK_ARG(ws, "null workspace");
    XPS_CHECK_ARG(ws_bytes >= xps_tme_kron_pass_f64_workspace(n_problems), "workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const size_t table_bytes = sizeof(long long) * XPS_TME_KRON_WORDS * (size_t)n_problems;
    double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + align8(table_bytes));
    hipError_t e = hipMemcpyAsync(ws, problems, table_bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { xps_set_error("%s: copying the table failed: %s", __func__, hipGetErrorString(e)); return XPS_E_HIP; }
    hipLaunchKernelGGL(kron_pass_kernel, dim3((unsigned)most, (unsigned)n_problems), dim3(KT), 0, st, (const long long*)ws, part);
    XPS_CHECK_LAUNCH();
    hipLaunchKernelGGL(kron_finish_kernel, dim3((unsigned)n_problems), dim3(KT), 0, st, (const long long*)ws, (const double*)part);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_tme_core_scale_f64(const double* z, int64_t ldz, const double* l0, const double* l1, const double* l2, int k0,
                                      int k1, int k2, int64_t n_sur, double* core, int64_t ldc, void* stream) {
    XPS_CHECK_ARG(n_sur >= 0, "negative count");
    XPS_CHECK_ARG(k0 >= 1 && k0 <= MAXA && k1 >= 1 && k1 <= MAXA && k2 >= 1 && k2 <= MAXA, "a box size outside 1 .. XPS_TME_MAX_AXIS");
    XPS_CHECK_ARG(n_sur <= (int64_t)1 << 20, "more than 2^20 surrogates");
    if (n_sur == 0) return XPS_OK;
    XPS_CHECK_ARG(z && core, "null tensor");
    XPS_CHECK_ARG(l0 && l1 && l2, "null multipliers");
    XPS_CHECK_ARG(ldz >= k2, "ldz < k2");
    XPS_CHECK_ARG(ldc >= k2, "ldc < k2");
    const long long total = (long long)n_sur * k0 * k1 * k2;
    long long blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(core_scale_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, z, (long long)ldz, l0, l1, l2, k0,
                       k1, k2, total, core, (long long)ldc);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_tme_mode_product_f64(const double* A, int64_t lda, int64_t sa, const double* B, int64_t ldb, int64_t sb,
                                        int b_kcontig, const double* add, int64_t ldadd, void* C, int c_is_f32, int64_t ldc,
                                        int64_t sc, int64_t M, int N, int K, int64_t batch, void* stream) {
    XPS_CHECK_ARG(M >= 0 && N >= 0 && K >= 1 && batch >= 0, "negative size");
    XPS_CHECK_ARG(M <= INT32_MAX - DM && N <= INT32_MAX - DN && K <= INT32_MAX - DK, "a size outside int32");
    XPS_CHECK_ARG(b_kcontig == 0 || b_kcontig == 1, "b_kcontig must be 0 or 1");
    XPS_CHECK_ARG(c_is_f32 == 0 || c_is_f32 == 1, "c_is_f32 must be 0 or 1");
    if (M == 0 || N == 0 || batch == 0) return XPS_OK;
    XPS_CHECK_ARG(A && B && C, "null matrix");
    XPS_CHECK_ARG(lda >= K, "lda < K");
    XPS_CHECK_ARG(ldb >= (b_kcontig ? K : N), "ldb below the width of B");
    XPS_CHECK_ARG(ldc >= N, "ldc < N");
    XPS_CHECK_ARG(!add || ldadd >= N, "ldadd < N");
    XPS_CHECK_ARG(sa >= 0 && sb >= 0, "negative batch stride");
    XPS_CHECK_ARG(batch == 1 || sc >= (M - 1) * ldc + N, "the outputs of two batch members overlap");
    const long long tm = cdiv(M, DM), tn = cdiv(N, DN);
    XPS_CHECK_ARG(tm * tn <= INT32_MAX / batch, "more than 2^31 - 1 tiles");
    const dim3 grid((unsigned)(tm * tn * batch));
    hipStream_t st = (hipStream_t)stream;
    if (b_kcontig)
        hipLaunchKernelGGL((mode_product_kernel<true>), grid, dim3(256), 0, st, A, (long long)lda, (long long)sa, B, (long long)ldb,
                           (long long)sb, add, (long long)ldadd, C, c_is_f32, (long long)ldc, (long long)sc, (int)M, N, K, (int)tm, (int)tn);
    else
        hipLaunchKernelGGL((mode_product_kernel<false>), grid, dim3(256), 0, st, A, (long long)lda, (long long)sa, B, (long long)ldb,
                           (long long)sb, add, (long long)ldadd, C, c_is_f32, (long long)ldc, (long long)sc, (int)M, N, K, (int)tm, (int)tn);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
