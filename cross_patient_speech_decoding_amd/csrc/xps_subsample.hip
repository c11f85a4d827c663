// Electrode subsampling on the device (reference processing_utils/spatial_avg_subsampling.py:74-90 spatial_avg_data, and the
// X[:, :, idx] slices of the grid / cross-patient subsample scripts).  DESIGN.md 4.11.
//
//   group mean : data [N][C][T] (the reference's (trials, X, Y, T), grid flattened row-major) -> out [N][T][G] float64, one
//                output channel per group of input channels (CSR: offsets[G + 1], members[offsets[G]]).  The mean of a group
//                is np.mean(data[:, ix, iy], axis=1): the members summed ONE BY ONE IN MEMBER ORDER in the input's dtype
//                (the reduced axis is not the contiguous one, so numpy's pairwise summation does not apply), one division
//                by the member count in that dtype, then widened to float64 by the assignment into the float64 result.
//   select     : x [N][T][C] -> out [N][T][L] = x[:, :, idx], the input's bits.
//
// Both come for S groupings / index lists at once: a workgroup owns one trial and a tile of TT time samples, stages the
// C x TT input tile in LDS (loads coalesced along the input's contiguous index) and then serves EVERY grouping from that
// tile before it goes on, so a launch reads the input from HBM once however many groupings it has.  Outputs of a tile and
// grouping are TT x G_s consecutive elements of the slab: written coalesced; the LDS tile is what turns the layout.
// No atomics, every output element is computed by one thread from the tile alone: bits do not depend on launch geometry.
#include "xps_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int LOADS = 8;                   // loads in flight per lane while a tile is staged
constexpr int LDS_BUDGET = 48 * 1024;      // per workgroup: 3 resident workgroups per CU (160 KiB), no attribute needed

// largest power of two <= 32 whose tile (row pitch tt + pad) fits the budget; 0 if even one sample does not
inline int tile_samples(int C, int elem, int pad) {
    for (int tt = 32; tt >= 1; tt >>= 1)
        if ((long long)C * (tt + pad) * elem <= LDS_BUDGET) return tt;
    return 0;
}

__device__ inline float div_rn(float a, float b) { return __fdiv_rn(a, b); }
__device__ inline double div_rn(double a, double b) { return a / b; }

// MEAN: tile[c][TT + 1] (odd pitch: the lanes of a wave read different channels of one sample without bank conflicts).
// group_start == nullptr: one grouping of Gtot groups.
template <typename T>
__global__ __launch_bounds__(THREADS) void group_mean_kernel(const T* __restrict__ data, int C, int Tn, int tt_shift, int tiles,
                                                             const int* __restrict__ group_start, const int* __restrict__ offsets,
                                                             const int* __restrict__ members, int S, int Gtot, long long NT,
                                                             double* __restrict__ out) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    T* tile = reinterpret_cast<T*>(lds_raw);
    const int TT = 1 << tt_shift, pitch = TT + 1;
    const long long n = blockIdx.x / tiles;
    const int t0 = (int)(blockIdx.x % tiles) << tt_shift;
    const int tv = min(TT, Tn - t0);                     // valid samples of this tile
    const T* src = data + n * C * (long long)Tn + t0;
    const int total = C << tt_shift;
    // LOADS independent loads per lane are issued before the first LDS store waits for one: a lane's round trip to HBM is
    // what bounds a streaming kernel with this little arithmetic
    for (int i0 = threadIdx.x; i0 < total; i0 += THREADS * LOADS) {
        T v[LOADS];
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const int i = i0 + u * THREADS, c = i >> tt_shift, t = i & (TT - 1);
            v[u] = (i < total && t < tv) ? src[(long long)c * Tn + t] : (T)0;
        }
#pragma unroll
        for (int u = 0; u < LOADS; ++u) {
            const int i = i0 + u * THREADS, c = i >> tt_shift, t = i & (TT - 1);
            if (i < total) tile[c * pitch + t] = v[u];
        }
    }
    __syncthreads();
    for (int s = 0; s < S; ++s) {
        const int g0 = group_start ? group_start[s] : 0;
        const int G = (group_start ? group_start[s + 1] : Gtot) - g0;
        double* dst = out + NT * g0 + (n * Tn + t0) * G;  // slab s is [N][T][G]: this tile's outputs are tv * G consecutive elements
        const int cnt = tv * G;
        for (int o = threadIdx.x; o < cnt; o += THREADS) {
            const int t = o / G, g = o - t * G;
            const int m0 = offsets[g0 + g], m1 = offsets[g0 + g + 1];
            T acc = tile[members[m0] * pitch + t];
            for (int m = m0 + 1; m < m1; ++m) acc = acc + tile[members[m] * pitch + t];
            const T mean = div_rn(acc, (T)(m1 - m0));
            dst[o] = (double)mean;
        }
    }
}

// SELECT: channel-last input, a tile is TT x C consecutive elements; no arithmetic.
template <typename T>
__global__ __launch_bounds__(THREADS) void select_kernel(const T* __restrict__ x, int C, int Tn, int tt_shift, int tiles,
                                                         const int* __restrict__ list_start, const int* __restrict__ idx, int S,
                                                         long long NT, T* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    T* tile = reinterpret_cast<T*>(lds_raw);
    const int TT = 1 << tt_shift;
    const long long n = blockIdx.x / tiles;
    const int t0 = (int)(blockIdx.x % tiles) << tt_shift;
    const int tv = min(TT, Tn - t0);
    const T* src = x + (n * Tn + t0) * C;
    const int total = tv * C;
    for (int i0 = threadIdx.x; i0 < total; i0 += THREADS * LOADS) {
        T v[LOADS];
#pragma unroll
        for (int u = 0; u < LOADS; ++u) v[u] = i0 + u * THREADS < total ? src[i0 + u * THREADS] : (T)0;
#pragma unroll
        for (int u = 0; u < LOADS; ++u)
            if (i0 + u * THREADS < total) tile[i0 + u * THREADS] = v[u];
    }
    __syncthreads();
    for (int s = 0; s < S; ++s) {
        const int l0 = list_start[s];
        const int L = list_start[s + 1] - l0;
        T* dst = out + NT * l0 + (n * Tn + t0) * L;
        const int cnt = tv * L;
        for (int o = threadIdx.x; o < cnt; o += THREADS) {
            const int t = o / L, j = o - t * L;
            dst[o] = tile[t * C + idx[l0 + j]];
        }
    }
}

template <typename T>
int group_mean_launch(const char* who, const T* data, int N, int C, int Tn, const int32_t* group_start, const int32_t* offsets,
                      const int32_t* members, int S, int Gtot, double* out, void* stream) {
    if (!(N >= 0 && C >= 1 && Tn >= 1 && S >= 1 && Gtot >= 1)) {
        xps_set_error("%s: bad argument", who);
        return XPS_E_INVALID;
    }
    if (N == 0) return XPS_OK;
    if (!(data && offsets && members && out)) {
        xps_set_error("%s: null argument", who);
        return XPS_E_INVALID;
    }
    const int tt = tile_samples(C, (int)sizeof(T), 1);
    if (tt == 0) {
        xps_set_error("%s: %d channels do not fit one LDS tile", who, C);
        return XPS_E_INVALID;
    }
    const int tiles = cdiv(Tn, tt);
    if ((long long)N * tiles > 0x7fffffffLL) {
        xps_set_error("%s: too many tiles for one launch", who);
        return XPS_E_INVALID;
    }
    const size_t lds = (size_t)C * (tt + 1) * sizeof(T);
    hipLaunchKernelGGL(group_mean_kernel<T>, dim3((unsigned)((long long)N * tiles)), dim3(THREADS), lds, (hipStream_t)stream, data, C, Tn,
                       __builtin_ctz(tt), tiles, group_start, offsets, members, S, Gtot, (long long)N * Tn, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        xps_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
        return XPS_E_HIP;
    }
    return XPS_OK;
}

}  // namespace

extern "C" int xps_group_mean_f32(const float* data, int N, int C, int T, const int32_t* offsets, const int32_t* members, int G,
                                  double* out, void* stream) {
    return group_mean_launch<float>(__func__, data, N, C, T, nullptr, offsets, members, 1, G, out, stream);
}

extern "C" int xps_group_mean_f64(const double* data, int N, int C, int T, const int32_t* offsets, const int32_t* members, int G,
                                  double* out, void* stream) {
    return group_mean_launch<double>(__func__, data, N, C, T, nullptr, offsets, members, 1, G, out, stream);
}

extern "C" int xps_group_mean_many_f32(const float* data, int N, int C, int T, const int32_t* group_start, const int32_t* offsets,
                                       const int32_t* members, int S, int Gtot, double* out, void* stream) {
    XPS_CHECK_ARG(group_start, "null argument");
    return group_mean_launch<float>(__func__, data, N, C, T, group_start, offsets, members, S, Gtot, out, stream);
}

extern "C" int xps_group_mean_many_f64(const double* data, int N, int C, int T, const int32_t* group_start, const int32_t* offsets,
                                       const int32_t* members, int S, int Gtot, double* out, void* stream) {
    XPS_CHECK_ARG(group_start, "null argument");
    return group_mean_launch<double>(__func__, data, N, C, T, group_start, offsets, members, S, Gtot, out, stream);
}

namespace {
template <typename T>
int select_launch(const char* who, const T* x, int N, int Tn, int C, const int32_t* list_start, const int32_t* idx, int S, int Ltot,
                  T* out, void* stream) {
    const char* bad = nullptr;
    const int tt = tile_samples(C, (int)sizeof(T), 0);
    const int tiles = cdiv(Tn, tt ? tt : 1);
    if (!(N >= 0 && C >= 1 && Tn >= 1 && S >= 1 && Ltot >= 1)) bad = "bad argument";
    else if (N == 0) return XPS_OK;
    else if (!(x && list_start && idx && out)) bad = "null argument";
    else if (tt == 0) bad = "the channels of one sample do not fit one LDS tile";
    else if ((long long)N * tiles > 0x7fffffffLL) bad = "too many tiles for one launch";
    if (bad) {
        xps_set_error("%s: %s", who, bad);
        return XPS_E_INVALID;
    }
    const size_t lds = (size_t)C * tt * sizeof(T);
    hipLaunchKernelGGL(select_kernel<T>, dim3((unsigned)((long long)N * tiles)), dim3(THREADS), lds, (hipStream_t)stream, x, C, Tn,
                       __builtin_ctz(tt), tiles, list_start, idx, S, (long long)N * Tn, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        xps_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
        return XPS_E_HIP;
    }
    return XPS_OK;
}
}  // namespace

extern "C" int xps_select_channels_f32(const float* x, int N, int T, int C, const int32_t* list_start, const int32_t* idx, int S,
                                       int Ltot, float* out, void* stream) {
    return select_launch<float>(__func__, x, N, T, C, list_start, idx, S, Ltot, out, stream);
}

extern "C" int xps_select_channels_f64(const double* x, int N, int T, int C, const int32_t* list_start, const int32_t* idx, int S,
                                       int Ltot, double* out, void* stream) {
    return select_launch<double>(__func__, x, N, T, C, list_start, idx, S, Ltot, out, stream);
}
