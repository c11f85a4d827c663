// CTC forced alignment: the Viterbi best path of a KNOWN target sequence through per-frame scores (the max-plus twin of
// the alpha recursion in xps_ctc.hip), its per-frame states, per-token frame spans and score.  One 64-lane workgroup per
// sequence, one launch for the batch, no host synchronisation, no allocation.  The lattice set-up (state cap, clamped
// extents, extended labels, skip rule, the entry's common checks and launch pair) is xps_ctc_lattice.h's, shared with
// xps_ctc_occupancy.hip.
//
// Contract (include/xps.h has the same text).  Extended label l' = (blank, l_1, blank, ..., l_L, blank), S = 2 L + 1 states,
// x_t(c) the score of class c at frame t widened to float64; everything below is float64 additions and comparisons:
//     v_0(0) = x_0(blank), v_0(1) = x_0(l_1), every other state -inf
//     v_t(s) = x_t(l'_s) + max(v_{t-1}(s), v_{t-1}(s-1), [s odd, s >= 3, l'_s != l'_{s-2}] v_{t-1}(s-2))
// Tie rule: among the predecessors the FIRST of (stay, s-1, s-2) that attains the maximum wins -- a move needs a strictly
// larger value -- and the path ends in S-1 unless v_{Tb-1}(S-2) is strictly larger.  path_score = v_{Tb-1}(end).
// A score of -inf (too few frames for the target, or every path crosses a -inf score) is infeasible: states and spans -1.
// Tb == 0: score 0 for L == 0, else -inf.
//
// The kernel is latency-bound by construction: Tb dependent steps of S <= 1023 states, then a backtrace of Tb dependent
// one-byte loads by one lane.  The two rows of v and the labels live in LDS sized by the batch's longest target (lanes
// stride over s); the backpointers, one byte per (t, s), go to the caller's workspace at ((b * T + t) * Smax + s),
// Smax = 2 * max_target_len + 1: only t in 1..Tb-1 and s < S of a sequence are written.
#include "xps_ctc_lattice.h"

namespace {
// two rows of Smax + 2 doubles and Smax labels, Smax = 2 * Lmax + 1: 20.5 KB at the cap, 232 bytes at Lmax = 5
inline size_t align_lds_bytes(int Lmax) {
    const size_t Smax = 2 * (size_t)Lmax + 1;
    return 2 * (Smax + 2) * sizeof(double) + Smax * sizeof(int);
}

template <typename T>
__global__ __launch_bounds__(64) void ctc_align_kernel(const T* __restrict__ scores, long long stride_t, long long stride_b,
                                                       int Tn, int C, int Lmax, const long long* __restrict__ targets,
                                                       long long tstride, const long long* __restrict__ in_len,
                                                       const long long* __restrict__ tg_len, int blank,
                                                       int* __restrict__ states, int* __restrict__ tok_start,
                                                       int* __restrict__ tok_end, double* __restrict__ path_score,
                                                       unsigned char* __restrict__ bp_all) {
    extern __shared__ double lds[];             // align_lds_bytes(Lmax): sized by the batch's longest target, not by the cap
    const int b = blockIdx.x, lane = threadIdx.x;
    const double NINF = -INFINITY;
    const CtcExtent e = ctc_extent(in_len, tg_len, b, Tn, Lmax);
    const int Tb = e.Tb, Lb = e.Lb, S = e.S, Smax = e.Smax;
    double* const row0 = lds;                   // the two rows of v, index s + 2: two -inf guards in front
    double* const row1 = lds + Smax + 2;
    int* const lab = reinterpret_cast<int*>(lds + 2 * (Smax + 2));
    const long long* tgt = targets + (long long)b * tstride;
    const T* x = scores + (long long)b * stride_b;
    unsigned char* bp = bp_all + (long long)b * Tn * Smax;
    int* st = states + (long long)b * Tn;
    int* ts = tok_start + (long long)b * Lmax;
    int* te = tok_end + (long long)b * Lmax;

    ctc_fill_labels(lab, tgt, S, blank, C, lane, 64);
    for (int s = lane; s < S + 2; s += 64) { row0[s] = NINF; row1[s] = NINF; }
    for (int t = Tb + lane; t < Tn; t += 64) st[t] = -1;
    for (int j = lane; j < Lmax; j += 64) { ts[j] = -1; te[j] = -1; }
    __syncthreads();

    if (Tb == 0) {
        if (lane == 0) path_score[b] = Lb == 0 ? 0.0 : NINF;
        return;
    }
    for (int s = lane; s < S && s < 2; s += 64) row0[s + 2] = (double)x[lab[s]];
    __syncthreads();
    for (int t = 1; t < Tb; ++t) {
        const double* prev = (t & 1) ? row0 : row1;
        double* cur = (t & 1) ? row1 : row0;
        const T* p = x + t * stride_t;
        unsigned char* bt = bp + (long long)t * Smax;
        for (int s = lane; s < S; s += 64) {
            const double xs = (double)p[lab[s]];
            double m = prev[s + 2];
            int k = 0;
            const double a1 = prev[s + 1];                      // s == 0: the -inf guard, never strictly larger
            if (a1 > m) { m = a1; k = 1; }
            if (ctc_skip(lab, s)) {
                const double a2 = prev[s];
                if (a2 > m) { m = a2; k = 2; }
            }
            cur[s + 2] = xs + m;
            bt[s] = (unsigned char)k;
        }
        __syncthreads();
    }
    if (lane != 0) return;
    // ---- end rule and backtrace (one lane; the block's own backpointer stores are visible after the barrier) ----
    const double* last = ((Tb - 1) & 1) ? row1 : row0;
    int s = S - 1;
    double best = last[s + 2];
    if (S >= 2 && last[S - 2 + 2] > best) { s = S - 2; best = last[s + 2]; }
    path_score[b] = best;
    if (best == NINF) {
        for (int t = 0; t < Tb; ++t) st[t] = -1;
        return;
    }
    int nxt = -1;                                               // the state at frame t + 1
    for (int t = Tb - 1; t >= 0; --t) {
        st[t] = s;
        if ((s & 1) && s != nxt) te[s >> 1] = t + 1;
        const int k = t > 0 ? (int)bp[(long long)t * Smax + s] : 0;
        if ((s & 1) && (k != 0 || t == 0)) ts[s >> 1] = t;
        nxt = s;
        s -= k;                                                 // k <= s by construction (k = 1 needs a finite v(s-1), k = 2 s >= 3)
        if (s < 0) s = 0;                                       // NaN scores: unspecified path, no out-of-range index
    }
}
}  // namespace

extern "C" size_t xps_ctc_align_workspace(int B, int T, int max_target_len) {
    if (B < 1 || T < 1 || max_target_len < 0) return 16;
    return (size_t)B * (size_t)T * (2 * (size_t)max_target_len + 1) + 16;
}

extern "C" int xps_ctc_align(const void* scores, int is_f32, int64_t stride_t, int64_t stride_b, int T, int B, int C,
                             int max_target_len, const int64_t* targets, int64_t target_stride,
                             const int64_t* input_lengths, const int64_t* target_lengths, int blank, int32_t* states,
                             int32_t* token_start, int32_t* token_end, double* path_score, void* workspace,
                             size_t workspace_bytes, void* stream) {
    XPS_CTC_CHECK_LATTICE_ARGS();
    if (B == 0) return XPS_OK;
    XPS_CHECK_ARG(path_score, "null argument");
    XPS_CHECK_ARG((scores && states) || T == 0, "null argument");
    XPS_CHECK_ARG((targets && token_start && token_end) || max_target_len == 0, "null argument");
    XPS_CHECK_ARG(workspace && workspace_bytes >= xps_ctc_align_workspace(B, T, max_target_len), "workspace too small");
    unsigned char* bp = reinterpret_cast<unsigned char*>(workspace);
    XPS_CTC_LAUNCH(ctc_align_kernel, dim3(B), dim3(64), align_lds_bytes(max_target_len), states, token_start, token_end,
                   path_score, bp);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
