// Exact t-SNE for gfx950 (manifold/tsne.py): sklearn's _t_sne.py / _utils.pyx recipe, batched over data sets
// of different n.  The arithmetic is written down in include/xps.h; this file follows it operation by operation.
//
//  xps_tsne_sqdist_f32      d2 = max((G_ii + G_jj) - 2 G_ij, 0) rounded to float32, exactly 0 on the diagonal.
//  xps_tsne_affinities_f64  two launches: the perplexity search (one wave per row, the row of d2 in LDS) writes the conditional
//                           probabilities C, beta, the step count and the row sum of C; the second takes S = 2 sum_i rowsum_i
//                           and writes P_ij = max((C_ij + C_ji) / S, eps).
//  xps_tsne_descent_f64     one priming launch, then ONE launch per iteration for all problems.  Every workgroup of a problem
//                           rebuilds the problem's update step from the previous launch's per-row partial sums (O(n), the same
//                           bits in every workgroup), keeps the new embedding in LDS and takes the partial sums of ITS rows at
//                           it; the problem's first workgroup alone writes the state back.  State and partial sums are
//                           double-buffered by the launch's parity: no launch reads what a workgroup of the same launch writes.
//
// Float64, no atomics, no grid barrier.  Every sum over j of a row and every sum over rows is taken by one wave: lane l adds
// its terms l, l + 64, ... in ascending order, then wave_sum_f64's butterfly.  No operation is contracted into an fma, so the
// numpy restatement (tests/tsne_ref.py) rounds where the kernels round.
#include "xps_common.h"
#include <float.h>
#include <math.h>
#include <string.h>

#pragma clang fp contract(off)

namespace {

enum { TS_N, TS_NC, TS_G, TS_LDG, TS_D2, TS_C, TS_P, TS_BETA, TS_STEPS, TS_ROWSUM, TS_YIN, TS_YOUT, TS_STATE, TS_ITBEGIN, TS_LR,
       TS_WORDS_USED };
static_assert(TS_WORDS_USED <= XPS_TSNE_WORDS, "problem words");

constexpr int TILE = XPS_TSNE_TILE_ROWS;     // rows of a problem per workgroup: one per wave
constexpr int WAVES = 4;
constexpr int THREADS = 64 * WAVES;
constexpr int HEAD = XPS_TSNE_STATE_HEAD;
constexpr double EPS_F64 = 2.220446049250313e-16;
// the arrays of a state half, n doubles each, after the HEAD convergence words
enum { A_Y0, A_Y1, A_U0, A_U1, A_GA0, A_GA1, A_GR0, A_GR1, A_S, A_A0, A_A1, A_B0, A_B1, A_E1, A_E2, A_COUNT };
static_assert(A_COUNT == XPS_TSNE_STATE_ARRAYS, "state arrays");
enum { CV_IT, CV_ERROR, CV_BEST_ERROR, CV_BEST_IT, CV_DONE, CV_Z, CV_NORM };

inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

__global__ __launch_bounds__(THREADS) void tsne_sqdist_kernel(const long long* __restrict__ probs, const int* __restrict__ tiles) {
    const int* tl = tiles + 2 * (long long)blockIdx.x;
    const long long* P = probs + (long long)tl[0] * XPS_TSNE_WORDS;
    const int n = (int)P[TS_N], row0 = tl[1] * TILE;
    const double* G = reinterpret_cast<const double*>(P[TS_G]);
    const long long ldg = P[TS_LDG];
    float* D2 = reinterpret_cast<float*>(P[TS_D2]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < TILE; r += WAVES) {
        const int i = row0 + r;
        if (i >= n) break;
        const double gii = G[(long long)i * ldg + i];
        for (int j = lane; j < n; j += 64) {
            const double d = (gii + G[(long long)j * ldg + j]) - 2.0 * G[(long long)i * ldg + j];
            D2[(long long)i * n + j] = (j != i && d > 0.0) ? (float)d : 0.0f;
        }
    }
}

// sklearn.manifold._utils._binary_search_perplexity for one row per wave; the row of d2 lies in the wave's LDS segment.
__global__ __launch_bounds__(THREADS) void tsne_search_kernel(const long long* __restrict__ probs, const int* __restrict__ tiles,
                                                              int n_max, double desired_entropy) {
    extern __shared__ __attribute__((aligned(16))) float rows[];
    const int* tl = tiles + 2 * (long long)blockIdx.x;
    const long long* P = probs + (long long)tl[0] * XPS_TSNE_WORDS;
    const int n = (int)P[TS_N], row0 = tl[1] * TILE;
    const float* D2 = reinterpret_cast<const float*>(P[TS_D2]);
    double* C = reinterpret_cast<double*>(P[TS_C]);
    double* beta_out = reinterpret_cast<double*>(P[TS_BETA]);
    int* steps_out = reinterpret_cast<int*>(P[TS_STEPS]);
    double* rowsum = reinterpret_cast<double*>(P[TS_ROWSUM]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* d = rows + (size_t)wave * n_max;
    const double tol = (double)1e-5f, eps_sum = (double)1e-8f;          // the .pyx keeps both constants in a C float
    for (int r = wave; r < TILE; r += WAVES) {
        const int i = row0 + r;
        if (i >= n) break;                                               // wave-uniform
        for (int j = lane; j < n; j += 64) d[j] = D2[(long long)i * n + j];   // a lane reads back only what it wrote
        double beta = 1.0, bmin = -INFINITY, bmax = INFINITY, beta_used = 1.0, sum = 0.0;
        int steps = 0;
        for (int l = 0; l < 100; ++l) {
            double acc = 0.0;
            for (int j = lane; j < n; j += 64)
                if (j != i) acc += exp(-(double)d[j] * beta);
            sum = wave_sum_f64(acc);
            if (sum == 0.0) sum = eps_sum;
            acc = 0.0;
            for (int j = lane; j < n; j += 64)
                if (j != i) acc += (double)d[j] * (exp(-(double)d[j] * beta) / sum);
            const double sd = wave_sum_f64(acc);
            const double diff = (log(sum) + beta * sd) - desired_entropy;
            beta_used = beta;
            steps = l + 1;
            if (fabs(diff) <= tol) break;
            if (diff > 0.0) {
                bmin = beta;
                beta = (bmax == INFINITY) ? beta * 2.0 : (beta + bmax) / 2.0;
            } else {
                bmax = beta;
                beta = (bmin == -INFINITY) ? beta / 2.0 : (beta + bmin) / 2.0;
            }
        }
        double acc = 0.0;
        for (int j = lane; j < n; j += 64) {
            const double c = (j != i) ? exp(-(double)d[j] * beta_used) / sum : 0.0;
            C[(long long)i * n + j] = c;
            acc += c;
        }
        acc = wave_sum_f64(acc);
        if (lane == 0) {
            beta_out[i] = beta;
            steps_out[i] = steps;
            rowsum[i] = acc;
        }
    }
}

__global__ __launch_bounds__(THREADS) void tsne_joint_kernel(const long long* __restrict__ probs, const int* __restrict__ tiles) {
    __shared__ double total;
    const int* tl = tiles + 2 * (long long)blockIdx.x;
    const long long* P = probs + (long long)tl[0] * XPS_TSNE_WORDS;
    const int n = (int)P[TS_N], row0 = tl[1] * TILE;
    const double* C = reinterpret_cast<const double*>(P[TS_C]);
    const double* rowsum = reinterpret_cast<const double*>(P[TS_ROWSUM]);
    double* Pm = reinterpret_cast<double*>(P[TS_P]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0) {
        double acc = 0.0;
        for (int i = lane; i < n; i += 64) acc += rowsum[i];
        acc = 2.0 * wave_sum_f64(acc);                                   // sum of all C_ij + C_ji
        if (lane == 0) total = acc > EPS_F64 ? acc : EPS_F64;
    }
    __syncthreads();
    const double S = total;
    for (int r = wave; r < TILE; r += WAVES) {
        const int i = row0 + r;
        if (i >= n) break;
        for (int j = lane; j < n; j += 64) {
            const double p = (C[(long long)i * n + j] + C[(long long)j * n + i]) / S;
            Pm[(long long)i * n + j] = (j == i) ? 0.0 : (p > EPS_F64 ? p : EPS_F64);
        }
    }
}

// The partial sums of row i at the embedding (y0, y1) in LDS: s = sum_j w, a_c = sum_j P w d_c, b_c = sum_j w^2 d_c and, with
// ERR, e1 = sum_j P log(P (1 + |d|^2)), e2 = sum_j P; j != i, w = 1 / (1 + |d|^2), d = y_i - y_j.
template <bool ERR>
__device__ inline void row_pass(const double* __restrict__ Pi, const double* y0, const double* y1, int n, int i, int lane, double* wr) {
    const double yi0 = y0[i], yi1 = y1[i];
    double s = 0.0, a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0, e1 = 0.0, e2 = 0.0;
#pragma unroll 4
    for (int j = lane; j < n; j += 64) {
        const double p = Pi[j];
        const double d0 = yi0 - y0[j], d1 = yi1 - y1[j];
        const double q = 1.0 + (d0 * d0 + d1 * d1);
        const double w = (j == i) ? 0.0 : 1.0 / q;
        s += w;
        const double pw = p * w, w2 = w * w;
        a0 += pw * d0;
        a1 += pw * d1;
        b0 += w2 * d0;
        b1 += w2 * d1;
        if (ERR && j != i) {
            e1 += p * log(p * q);
            e2 += p;
        }
    }
    s = wave_sum_f64(s);
    a0 = wave_sum_f64(a0);
    a1 = wave_sum_f64(a1);
    b0 = wave_sum_f64(b0);
    b1 = wave_sum_f64(b1);
    if (ERR) {
        e1 = wave_sum_f64(e1);
        e2 = wave_sum_f64(e2);
    }
    if (lane == 0) {
        wr[HEAD + (size_t)A_S * n + i] = s;
        wr[HEAD + (size_t)A_A0 * n + i] = a0;
        wr[HEAD + (size_t)A_A1 * n + i] = a1;
        wr[HEAD + (size_t)A_B0 * n + i] = b0;
        wr[HEAD + (size_t)A_B1 * n + i] = b1;
        if (ERR) {
            wr[HEAD + (size_t)A_E1 * n + i] = e1;
            wr[HEAD + (size_t)A_E2 * n + i] = e2;
        }
    }
}

// One iteration of sklearn's _gradient_descent for every problem (prime = 0), or the start of a phase (prime = 1: update = 0,
// gains = 1, best error = DBL_MAX, the embedding taken from Y_in).  Reads state half wr_half ^ 1, writes half wr_half.
__global__ __launch_bounds__(THREADS) void tsne_descent_kernel(const long long* __restrict__ probs, const int* __restrict__ tiles,
                                                               int prime, int wr_half, int max_iter, double momentum, double exag,
                                                               int n_iter_without_progress, double min_grad_norm) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int* tl = tiles + 2 * (long long)blockIdx.x;
    const long long* P = probs + (long long)tl[0] * XPS_TSNE_WORDS;
    const int n = (int)P[TS_N], nc = (int)P[TS_NC], row0 = tl[1] * TILE;
    const bool first = tl[1] == 0;                                       // the problem's first workgroup writes the state
    double* st = reinterpret_cast<double*>(P[TS_STATE]);
    const size_t half = HEAD + (size_t)A_COUNT * n;
    const double* rd = st + (size_t)(wr_half ^ 1) * half;
    double* wr = st + (size_t)wr_half * half;
    double* y0 = lds;
    double* y1 = lds + n;
    double* bc = lds + 2 * (size_t)n;                                    // [0] Z, [1] done
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int next_it;                                                         // the iteration that will read this launch's partial sums

    if (prime) {
        next_it = (int)P[TS_ITBEGIN];
        const double* Yin = reinterpret_cast<const double*>(P[TS_YIN]);
        for (int i = tid; i < n; i += THREADS) {
            const double v0 = Yin[(long long)i * nc], v1 = nc == 2 ? Yin[(long long)i * nc + 1] : 0.0;
            y0[i] = v0;
            y1[i] = v1;
            if (first) {
                wr[HEAD + (size_t)A_Y0 * n + i] = v0;
                wr[HEAD + (size_t)A_Y1 * n + i] = v1;
                wr[HEAD + (size_t)A_U0 * n + i] = 0.0;
                wr[HEAD + (size_t)A_U1 * n + i] = 0.0;
                wr[HEAD + (size_t)A_GA0 * n + i] = 1.0;
                wr[HEAD + (size_t)A_GA1 * n + i] = 1.0;
                wr[HEAD + (size_t)A_GR0 * n + i] = 0.0;
                wr[HEAD + (size_t)A_GR1 * n + i] = 0.0;
            }
        }
        if (first && tid == 0) {
            wr[CV_IT] = (double)next_it;
            wr[CV_ERROR] = DBL_MAX;
            wr[CV_BEST_ERROR] = DBL_MAX;
            wr[CV_BEST_IT] = (double)next_it;
            wr[CV_DONE] = 0.0;
            wr[CV_Z] = 0.0;
            wr[CV_NORM] = 0.0;
            wr[7] = 0.0;
        }
    } else {
        if (rd[CV_DONE] != 0.0) {                                        // uniform over the problem: its state stays as it stopped
            if (first && tid < HEAD) wr[tid] = rd[tid];
            return;
        }
        const int it = (int)rd[CV_IT];
        const double lr = __longlong_as_double(P[TS_LR]);
        if (wave == 0) {
            double z = 0.0;
#pragma unroll 4
            for (int i = lane; i < n; i += 64) z += rd[HEAD + (size_t)A_S * n + i];
            z = wave_sum_f64(z);
            if (lane == 0) bc[0] = z;
        }
        __syncthreads();
        const double Z = bc[0], rz = 1.0 / Z;
#pragma unroll 2
        for (int i = tid; i < n; i += THREADS) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                double y = rd[HEAD + (size_t)(A_Y0 + c) * n + i], u = 0.0, ga = 1.0, g = 0.0;
                if (c < nc) {
                    g = 4.0 * (exag * rd[HEAD + (size_t)(A_A0 + c) * n + i] - rz * rd[HEAD + (size_t)(A_B0 + c) * n + i]);
                    u = rd[HEAD + (size_t)(A_U0 + c) * n + i];
                    ga = rd[HEAD + (size_t)(A_GA0 + c) * n + i];
                    ga = (u * g < 0.0) ? ga + 0.2 : ga * 0.8;
                    ga = ga < 0.01 ? 0.01 : ga;
                    u = momentum * u - lr * (g * ga);
                    y = y + u;
                }
                (c == 0 ? y0 : y1)[i] = y;
                if (first) {
                    wr[HEAD + (size_t)(A_Y0 + c) * n + i] = y;
                    wr[HEAD + (size_t)(A_U0 + c) * n + i] = u;
                    wr[HEAD + (size_t)(A_GA0 + c) * n + i] = ga;
                    wr[HEAD + (size_t)(A_GR0 + c) * n + i] = g;
                }
            }
        }
        const bool check = (it + 1) % 50 == 0, last = it == max_iter - 1;
        if (first) {
            __syncthreads();                                             // this workgroup's own gradient and gains are visible to it
            if (wave == 0) {
                double error = NAN, best = rd[CV_BEST_ERROR], best_it = rd[CV_BEST_IT], norm = rd[CV_NORM];
                bool done = false;
                if (check || last) {
                    double e1 = 0.0, e2 = 0.0;
                    for (int i = lane; i < n; i += 64) {
                        e1 += rd[HEAD + (size_t)A_E1 * n + i];
                        e2 += rd[HEAD + (size_t)A_E2 * n + i];
                    }
                    e1 = wave_sum_f64(e1);
                    e2 = wave_sum_f64(e2);
                    error = exag * (e1 + log(exag * Z) * e2);
                }
                if (check) {
                    double q = 0.0;
                    for (int i = lane; i < n; i += 64) {
                        const double s0 = wr[HEAD + (size_t)A_GR0 * n + i] * wr[HEAD + (size_t)A_GA0 * n + i];
                        const double s1 = wr[HEAD + (size_t)A_GR1 * n + i] * wr[HEAD + (size_t)A_GA1 * n + i];
                        q += s0 * s0 + s1 * s1;
                    }
                    norm = sqrt(wave_sum_f64(q));
                    if (error < best) {
                        best = error;
                        best_it = (double)it;
                    } else if ((double)it - best_it > (double)n_iter_without_progress) {
                        done = true;
                    }
                    if (norm <= min_grad_norm) done = true;
                }
                if (last) done = true;
                if (lane == 0) {
                    wr[CV_IT] = (double)(done ? it : it + 1);
                    wr[CV_ERROR] = error;
                    wr[CV_BEST_ERROR] = best;
                    wr[CV_BEST_IT] = best_it;
                    wr[CV_DONE] = done ? 1.0 : 0.0;
                    wr[CV_Z] = Z;
                    wr[CV_NORM] = norm;
                    wr[7] = 0.0;
                    bc[1] = done ? 1.0 : 0.0;
                }
            }
            __syncthreads();
            if (bc[1] != 0.0) {                                          // the embedding sklearn returns: after this iteration's step
                double* Yout = reinterpret_cast<double*>(P[TS_YOUT]);
                for (int i = tid; i < n; i += THREADS) {
                    Yout[(long long)i * nc] = y0[i];
                    if (nc == 2) Yout[(long long)i * nc + 1] = y1[i];
                }
            }
        }
        if (last) return;                                                // no iteration follows: no partial sums
        next_it = it + 1;
    }
    __syncthreads();                                                     // the embedding is complete in LDS
    const bool want_err = (next_it + 1) % 50 == 0 || next_it == max_iter - 1;
    const double* Pm = reinterpret_cast<const double*>(P[TS_P]);
    for (int r = wave; r < TILE; r += WAVES) {
        const int i = row0 + r;
        if (i >= n) break;
        if (want_err) row_pass<true>(Pm + (long long)i * n, y0, y1, n, i, lane, wr);
        else row_pass<false>(Pm + (long long)i * n, y0, y1, n, i, lane, wr);
    }
}

// Both HOST tables of a call: every problem's n and nc, and the tile table, which must be the canonical one -- the problems in
// order, each with its row tiles 0 .. ceil(n / TILE) - 1 ascending (so every row has one workgroup and tile 0 exists).
const char* tables_bad(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles) {
    if (!problems || !tiles) return "null table";
    if (n_problems < 1 || n_tiles < 1) return "no problem or no tile";
    long long t = 0;
    for (int p = 0; p < n_problems; ++p) {
        const int64_t* P = problems + (size_t)XPS_TSNE_WORDS * p;
        if (P[TS_N] < 2 || P[TS_N] > XPS_TSNE_MAX_SAMPLES) return "n outside 2 .. XPS_TSNE_MAX_SAMPLES";
        if (P[TS_NC] != 1 && P[TS_NC] != 2) return "n_components must be 1 or 2";
        const int nt = (int)((P[TS_N] + TILE - 1) / TILE);
        for (int r = 0; r < nt; ++r, ++t) {
            if (t >= n_tiles || tiles[2 * t] != p || tiles[2 * t + 1] != r)
                return "the tile table is not {problem, row tile} for every tile of XPS_TSNE_TILE_ROWS rows of every problem in order";
        }
    }
    if (t != n_tiles) return "the tile table has more tiles than the problems have";
    return nullptr;
}

int max_n(const int64_t* problems, int n_problems) {
    int64_t m = 0;
    for (int p = 0; p < n_problems; ++p) m = problems[(size_t)XPS_TSNE_WORDS * p + TS_N] > m ? problems[(size_t)XPS_TSNE_WORDS * p + TS_N] : m;
    return (int)m;
}

size_t tables_bytes(int n_problems, int n_tiles) {
    return align8(sizeof(long long) * XPS_TSNE_WORDS * (size_t)n_problems) + align8(2 * sizeof(int) * (size_t)n_tiles);
}

int copy_tables(const char* fn, const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, void* ws, hipStream_t st,
                const long long** probs_d, const int** tiles_d) {
    static_assert(sizeof(long long) == sizeof(int64_t), "the table is read as long long");
    long long* pd = static_cast<long long*>(ws);
    int* td = reinterpret_cast<int*>(static_cast<char*>(ws) + align8(sizeof(long long) * XPS_TSNE_WORDS * (size_t)n_problems));
    hipError_t e = hipMemcpyAsync(pd, problems, sizeof(long long) * XPS_TSNE_WORDS * (size_t)n_problems, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(td, tiles, 2 * sizeof(int) * (size_t)n_tiles, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) { xps_set_error("%s: copying the tables failed: %s", fn, hipGetErrorString(e)); return XPS_E_HIP; }
    *probs_d = pd;
    *tiles_d = td;
    return XPS_OK;
}

// dynamic LDS above 64 KiB needs the attribute; both kernels stay below XPS_TSNE_MAX_SAMPLES' need
bool allow_lds(const void* kern, size_t bytes) {
    return bytes <= 65536 || hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

}  // namespace

#define XPS_TSNE_CHECK_TABLES()                                                             \
    do {                                                                                    \
        const char* bad_ = tables_bad(problems, n_problems, tiles, n_tiles);                \
        XPS_CHECK_ARG(!bad_, bad_);                                                         \
        XPS_CHECK_ARG(ws, "null workspace");                                                \
        XPS_CHECK_ARG(ws_bytes >= tables_bytes(n_problems, n_tiles), "workspace too small"); \
    } while (0)

extern "C" size_t xps_tsne_state_bytes(int n) {
    if (n < 1) return 0;
    return 2 * sizeof(double) * (HEAD + (size_t)A_COUNT * (size_t)n);
}

extern "C" size_t xps_tsne_sqdist_f32_workspace(int n_problems, int n_tiles) {
    return (n_problems < 1 || n_tiles < 1) ? 0 : tables_bytes(n_problems, n_tiles);
}

extern "C" int xps_tsne_sqdist_f32(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, void* ws,
                                   size_t ws_bytes, void* stream) {
    XPS_TSNE_CHECK_TABLES();
    for (int p = 0; p < n_problems; ++p) {
        const int64_t* P = problems + (size_t)XPS_TSNE_WORDS * p;
        XPS_CHECK_ARG(P[TS_G] && P[TS_D2], "null matrix");
        XPS_CHECK_ARG(P[TS_LDG] >= P[TS_N], "ldg < n");
    }
    const long long* pd;
    const int* td;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = copy_tables(__func__, problems, n_problems, tiles, n_tiles, ws, st, &pd, &td)) return rc;
    hipLaunchKernelGGL(tsne_sqdist_kernel, dim3(n_tiles), dim3(THREADS), 0, st, pd, td);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" size_t xps_tsne_affinities_f64_workspace(int n_problems, int n_tiles) {
    return (n_problems < 1 || n_tiles < 1) ? 0 : tables_bytes(n_problems, n_tiles);
}

extern "C" int xps_tsne_affinities_f64(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, double perplexity,
                                       void* ws, size_t ws_bytes, void* stream) {
    XPS_TSNE_CHECK_TABLES();
    XPS_CHECK_ARG(perplexity > 0.0 && perplexity < INFINITY, "perplexity must be positive and finite");
    for (int p = 0; p < n_problems; ++p) {
        const int64_t* P = problems + (size_t)XPS_TSNE_WORDS * p;
        XPS_CHECK_ARG(P[TS_D2] && P[TS_C] && P[TS_P] && P[TS_BETA] && P[TS_STEPS] && P[TS_ROWSUM], "null matrix or vector");
        XPS_CHECK_ARG(P[TS_C] != P[TS_P], "C and P must differ");
        XPS_CHECK_ARG(perplexity < (double)P[TS_N], "perplexity must be less than n");
    }
    const int n_max = max_n(problems, n_problems);
    const size_t lds = sizeof(float) * WAVES * (size_t)n_max;
    XPS_CHECK_ARG(allow_lds(reinterpret_cast<const void*>(tsne_search_kernel), lds), "the rows of d2 do not fit the LDS");
    const long long* pd;
    const int* td;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = copy_tables(__func__, problems, n_problems, tiles, n_tiles, ws, st, &pd, &td)) return rc;
    const double desired = log((double)(float)perplexity);              // the .pyx takes the perplexity as a C float
    hipLaunchKernelGGL(tsne_search_kernel, dim3(n_tiles), dim3(THREADS), lds, st, pd, td, n_max, desired);
    XPS_CHECK_LAUNCH();
    hipLaunchKernelGGL(tsne_joint_kernel, dim3(n_tiles), dim3(THREADS), 0, st, pd, td);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" size_t xps_tsne_descent_f64_workspace(int n_problems, int n_tiles) {
    return (n_problems < 1 || n_tiles < 1) ? 0 : tables_bytes(n_problems, n_tiles);
}

extern "C" int xps_tsne_descent_f64(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, int n_launches,
                                    int max_iter, double momentum, double exaggeration, int n_iter_without_progress,
                                    double min_grad_norm, void* ws, size_t ws_bytes, void* stream) {
    XPS_TSNE_CHECK_TABLES();
    XPS_CHECK_ARG(n_launches >= 0 && max_iter >= 1, "n_launches >= 0 and max_iter >= 1 are needed");
    XPS_CHECK_ARG(momentum >= 0.0 && momentum < INFINITY && exaggeration > 0.0 && exaggeration < INFINITY,
                  "momentum must be finite and non-negative, the exaggeration finite and positive");
    XPS_CHECK_ARG(n_iter_without_progress >= 0 && min_grad_norm == min_grad_norm, "n_iter_without_progress < 0 or min_grad_norm NaN");
    for (int p = 0; p < n_problems; ++p) {
        const int64_t* P = problems + (size_t)XPS_TSNE_WORDS * p;
        XPS_CHECK_ARG(P[TS_P] && P[TS_YIN] && P[TS_YOUT] && P[TS_STATE], "null matrix or state");
        XPS_CHECK_ARG(P[TS_ITBEGIN] >= 0 && P[TS_ITBEGIN] < max_iter, "it_begin outside 0 .. max_iter - 1");
        double lr;
        memcpy(&lr, &P[TS_LR], sizeof lr);
        XPS_CHECK_ARG(lr > 0.0 && lr < INFINITY, "the learning rate must be positive and finite");
    }
    const size_t lds = sizeof(double) * (2 * (size_t)max_n(problems, n_problems) + 2);
    XPS_CHECK_ARG(allow_lds(reinterpret_cast<const void*>(tsne_descent_kernel), lds), "the embedding does not fit the LDS");
    const long long* pd;
    const int* td;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = copy_tables(__func__, problems, n_problems, tiles, n_tiles, ws, st, &pd, &td)) return rc;
    for (int t = 0; t <= n_launches; ++t) {                              // launch 0 primes half 0; launch t reads half (t - 1) & 1
        hipLaunchKernelGGL(tsne_descent_kernel, dim3(n_tiles), dim3(THREADS), lds, st, pd, td, t == 0 ? 1 : 0, t & 1, max_iter,
                           momentum, exaggeration, n_iter_without_progress, min_grad_norm);
        XPS_CHECK_LAUNCH();
    }
    return XPS_OK;
}
