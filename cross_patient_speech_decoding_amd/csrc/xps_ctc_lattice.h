// The CTC lattice of a known target, as every kernel over it sets it up: the state cap, a sequence's clamped extents, the
// extended label l' = (blank, l_1, blank, ..., l_L, blank), the skip rule, and the argument checks and the float / double
// launch pair of the entry points.  Shared by xps_ctc_align.hip (max-plus) and xps_ctc_occupancy.hip (sum-product);
// xps_ctc.hip (the loss) takes the cap from here and nothing else: its skip rule is written on labels, not on parity, and
// its arithmetic is its own.
#pragma once
#include "xps_common.h"

constexpr int CTC_MAXS = 1024;       // 2 * max target length + 1 states: 511 labels

// One sequence's extents: Tb frames and Lb labels, clamped to the batch's (a NULL length array: full length), S = 2 Lb + 1
// states of the batch's Smax = 2 Lmax + 1.
struct CtcExtent { int Tb, Lb, S, Smax; };

__device__ __forceinline__ CtcExtent ctc_extent(const long long* in_len, const long long* tg_len,
                                                int b, int Tn, int Lmax) {
    CtcExtent e;
    const long long tb = in_len ? in_len[b] : (long long)Tn;
    e.Tb = tb < 0 ? 0 : (tb > Tn ? Tn : (int)tb);
    const long long lb = tg_len ? tg_len[b] : (long long)Lmax;
    e.Lb = lb < 0 ? 0 : (lb > Lmax ? Lmax : (int)lb);
    e.S = 2 * e.Lb + 1;
    e.Smax = 2 * Lmax + 1;
    return e;
}

// lab[s] = l'_s for s < S, by `width` lanes
__device__ __forceinline__ void ctc_fill_labels(int* lab, const long long* tgt, int S, int blank, int C, int lane,
                                                int width) {
    for (int s = lane; s < S; s += width) {
        long long l = (s & 1) ? tgt[s >> 1] : (long long)blank;
        lab[s] = l < 0 ? 0 : (l >= C ? C - 1 : (int)l);         // memory safety only: labels are the caller's contract
    }
}

// may a path enter state s from s - 2: s is a token, not the first, and differs from the token before it
__device__ __forceinline__ bool ctc_skip(const int* lab, int s) { return (s & 1) && s >= 3 && lab[s] != lab[s - 2]; }

// The argument checks common to the entries over the lattice.  A macro, so that __func__ is the entry's own name.
#define XPS_CTC_CHECK_LATTICE_ARGS()                                                                                      \
    do {                                                                                                                  \
        XPS_CHECK_ARG(T >= 0 && B >= 0 && max_target_len >= 0 && stride_t >= 0 && stride_b >= 0, "negative size");        \
        XPS_CHECK_ARG(C >= 1, "needs at least one class");                                                                \
        XPS_CHECK_ARG(blank >= 0 && blank < C, "blank outside 0..C-1");                                                   \
        XPS_CHECK_ARG(2 * (long long)max_target_len + 1 <= CTC_MAXS, "target longer than 511 labels");                    \
        XPS_CHECK_ARG(target_stride >= max_target_len, "target stride smaller than the longest target");                  \
    } while (0)

// Launch KERNEL<float> or KERNEL<double> over the entry's own arguments (scores, is_f32, the strides, T, C,
// max_target_len, targets, the lengths, blank), then the kernel's outputs.
#define XPS_CTC_LAUNCH(KERNEL, grid, block, lds, ...)                                                                     \
    do {                                                                                                                  \
        const long long* tg_ = reinterpret_cast<const long long*>(targets);                                               \
        const long long* il_ = reinterpret_cast<const long long*>(input_lengths);                                         \
        const long long* tl_ = reinterpret_cast<const long long*>(target_lengths);                                        \
        if (is_f32)                                                                                                       \
            hipLaunchKernelGGL(KERNEL<float>, grid, block, lds, (hipStream_t)stream, (const float*)scores,                \
                               (long long)stride_t, (long long)stride_b, T, C, max_target_len, tg_,                       \
                               (long long)target_stride, il_, tl_, blank, __VA_ARGS__);                                   \
        else                                                                                                              \
            hipLaunchKernelGGL(KERNEL<double>, grid, block, lds, (hipStream_t)stream, (const double*)scores,              \
                               (long long)stride_t, (long long)stride_b, T, C, max_target_len, tg_,                       \
                               (long long)target_stride, il_, tl_, blank, __VA_ARGS__);                                   \
    } while (0)
