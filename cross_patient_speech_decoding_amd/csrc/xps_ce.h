// The cross-entropy row routine and the fixed-order block / grid reduction, shared by the fused loss-and-gradient launch
// (xps_nn.hip: ce_loss_grad_kernel) and the one-launch classification step (xps_classify.hip): both produce the same bits.
#pragma once
#include "xps_common.h"

constexpr int CE_BLOCK = 256;         // rows per block = threads per block: the partial sums depend on it

// loss of one row of C logits; drow (optional) = d(mean loss over `rows` rows) / d(logits of this row)
__device__ inline float ce_row(const float* __restrict__ p, long long tg, int C, long long rows, float* __restrict__ drow) {
    float mx = p[0];
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, p[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(p[c] - mx);
    const float rl = (logf(s) + mx) - p[tg];
    if (drow) {
        const float g = 1.f / (float)rows, inv = 1.f / s;
        for (int c = 0; c < C; ++c) drow[c] = g * (expf(p[c] - mx) * inv - (c == tg ? 1.f : 0.f));
    }
    return rl;
}

// Tree sum of one value per thread (sh: CE_BLOCK doubles of LDS); thread 0 leaves the block's partial in part[blockIdx.x] and
// takes a ticket.  Returns true, in every thread of the block, in the block that took the LAST ticket: that block sees every
// block's partial after the acquire fence here (ONLY the partials: stores that other threads made before calling this are not
// released by thread 0's fence -- a kernel that hands more from block to block must fence in every storing thread).  Partials are published
// with agent-scope fences around the ticket (cdna_hip_programming.md, Guideline 16): release before the atomic, acquire after.
__device__ inline bool ce_block_sum_ticket(double l, double* sh, unsigned* last, double* part, unsigned* ticket) {
    sh[threadIdx.x] = l;
    __syncthreads();
    for (int st = CE_BLOCK / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[blockIdx.x] = sh[0];
        __threadfence();                                          // release: the partial before the ticket
        *last = (atomicAdd(ticket, 1u) == gridDim.x - 1) ? 1u : 0u;
    }
    __syncthreads();
    const bool is_last = *last != 0u;
    if (is_last) __threadfence();                                 // acquire: every block's partial
    return is_last;
}

// one thread of the last block: the partials IN INDEX ORDER (the result does not depend on which block is last)
__device__ inline float ce_mean_of_partials(const double* part, long long rows) {
    double a = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) a += __hip_atomic_load(part + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (float)(a / (double)rows);
}
