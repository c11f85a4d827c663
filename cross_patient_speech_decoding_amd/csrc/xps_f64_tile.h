// The float64 MFMA tile of the alignment kernels, once: gemm_f64_kernel (xps_align.hip), xcov_grouped_kernel,
// apply_grouped_kernel and gram_grouped_kernel (xps_fold_align.hip) are built from these pieces and keep only their table
// decoding, side sums and stores.
//
// A workgroup of 256 threads (4 waves) owns 64 x 64 outputs and walks the contraction in steps of 16: both operands are staged
// to LDS as S[k][x] (16 x 64, rows padded to 66 doubles: 2 x 16 x 66 x 8 = 16896 bytes), fp32 / fp64 elements converted and
// centred on the way, then wave w multiplies rows 16 w .. 16 w + 15 of the tile with v_mfma_f64_16x16x4_f64.
//
// f64 MFMA operand mapping (16x16x4, lane l: n = l & 15, kq = l >> 4):
//   A[row n][k kq], B[k kq][col n], D[row = kq + 4*i][col = n] in register i.
#pragma once
#include "xps_common.h"

constexpr int DM = 64, DN = 64, DK = 16, DLD = 66;

struct Mat64 {
    const void* p;
    long long ld;
    const double* mean;   // indexed by the CONTIGUOUS (storage column) index, or null
    int is_f32;
};

__device__ inline double ld_elem(const Mat64& m, long long off) {
    return m.is_f32 ? (double)reinterpret_cast<const float*>(m.p)[off] : reinterpret_cast<const double*>(m.p)[off];
}

// Stage S[k][x] = M[x0 + x][k0 + k] - mean[k0 + k] of a matrix stored [x][k] (k contiguous); zero at or past X / kend.
// Thread t: x = x0 + (t >> 2), k = k0 + 4 (t & 3) .. + 3.
__device__ inline void stage_kc(const Mat64& m, double (*S)[DLD], int x0, int X, int k0, int kend, int tid) {
    const int x = x0 + (tid >> 2), kb = k0 + (tid & 3) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = kb + i;
        double v = 0.0;
        if (x < X && k < kend) {
            v = ld_elem(m, (long long)x * m.ld + k);
            if (m.mean) v -= m.mean[k];
        }
        S[(tid & 3) * 4 + i][tid >> 2] = v;
    }
}

// Stage S[k][x] = M[row_of(k0 + k)][x0 + x] - mean[x0 + x] of a matrix stored [k][x] (x contiguous); zero at or past X / kend.
// row_of(k) is the storage row of contraction index k: the identity for a plain matrix, a walk over a list of row blocks for
// the grouped cross moments.  It is asked for every k of the step, also at or past kend (the row is then not read), so a map
// that reads a table guards its own extent.  Thread t: k = k0 + (t >> 4), x = x0 + 4 (t & 15) .. + 3.
struct PlainRows {
    __device__ long long operator()(int k) const { return k; }
};
template <class RowOf = PlainRows>
__device__ inline void stage_xc(const Mat64& m, double (*S)[DLD], int x0, int X, int k0, int kend, int tid, RowOf row_of = RowOf()) {
    const int k = k0 + (tid >> 4), xb = x0 + (tid & 15) * 4;
    const long long row = row_of(k);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = xb + i;
        double v = 0.0;
        if (x < X && k < kend) {
            v = ld_elem(m, row * m.ld + x);
            if (m.mean) v -= m.mean[x];
        }
        S[tid >> 4][(tid & 15) * 4 + i] = v;
    }
}

// The 16 staged contraction steps into this wave's 16 x 64 outputs: acc[j] = columns 16 j .. 16 j + 15, k ascending.
__device__ inline void mfma_f64_tile(const double (*As)[DLD], const double (*Bs)[DLD], f64x4 (&acc)[4], int tid) {
    const int wave = tid >> 6, n = tid & 15, kq = (tid >> 4) & 3;
#pragma unroll
    for (int ks = 0; ks < DK; ks += 4) {
        const double a = As[ks + kq][wave * 16 + n];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double b = Bs[ks + kq][j * 16 + n];
            acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
        }
    }
}

// Walk this lane's 16 accumulators in the D layout: store(row, col, value) for every output inside M x N.
template <class Store>
__device__ inline void store_f64_tile(const f64x4 (&acc)[4], int m0, int n0, int M, int N, int tid, Store store) {
    const int wave = tid >> 6, n = tid & 15, kq = (tid >> 4) & 3;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = m0 + wave * 16 + kq + 4 * i, col = n0 + j * 16 + n;
            if (row < M && col < N) store(row, col, acc[j][i]);
        }
}
