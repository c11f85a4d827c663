// CTC posterior occupancies: the forward-backward posteriors of a KNOWN target sequence through per-frame scores -- how much
// of the probability mass has token j emitted at frame t (token_occ), started at frame t (onset), and class c emitted at
// frame t (class_occ) -- with log Z and the two first moments (expected_frames, onset_mean).  The sum-product twin of the
// best path in xps_ctc_align.hip.  One workgroup per sequence, one launch for the batch, no host synchronisation, no
// allocation, no floating-point atomics.  The lattice set-up (state cap, clamped extents, extended labels, skip rule, the
// entry's common checks and launch pair) is xps_ctc_lattice.h's, shared with xps_ctc_align.hip; the double lse3 stays here:
// its term order is contract.
//
// Contract: include/xps.h (the recursion, the order of the terms of every lse and of every sum, the edge rules).
//
// Layout.  Pass 1 walks the frames forwards: a_t(s) from the rolling row in LDS, written to the next row and to the caller's
// workspace at ((b * T + t) * Smax + s), Smax = 2 * max_target_len + 1 (only t < Tb, s < S).  Pass 2 walks them backwards:
// b_t(s) from the rolling row, a_t(s), a_{t-1}(s-1) and a_{t-1}(s-2) back from the workspace, and the posteriors of frame t
// leave at once.  The workgroup has Smax / 64 waves, rounded to the nearest, at least one and at most four (four passes of
// the lanes at the cap of 1023 states): a state costs three exp and a log in double in pass 1 and up to seven exp and two
// log in pass 2, some hundreds of cycles each, so the states of one frame are worth spreading over the CU's four SIMDs;
// but a wave that holds one state (S = 129 on 192 lanes) costs a wave slot for nothing and was measured slower than
// letting that state take a second pass.  No result depends on the width.
// Class sums: the states of one class form a chain by increasing s (built once per sequence); the lane of the chain's first
// state adds g along it into the class's LDS bin, then the lanes copy the C bins out.  One barrier per frame, two with
// class_occ.
#include "xps_ctc_lattice.h"

#include <cstdint>

namespace {
constexpr int OCC_MAX_WIDTH = 256;
constexpr size_t OCC_LDS_BUDGET = 65536;
constexpr int OCC_HEAD = 0x10000, OCC_END = 0xFFFF;

// two rows of Smax + 4 doubles (two -inf guard cells on each side), g (Smax doubles), the two moment rows (Lmax doubles
// each), the labels and the chains (Smax ints each): 80 Lmax + 96 bytes; the class bins (C doubles) where class_occ is asked for
inline size_t occ_lds_bytes(int Lmax, int C, bool bins) {
    const size_t Smax = 2 * (size_t)Lmax + 1;
    return (2 * (Smax + 4) + Smax + 2 * (size_t)Lmax) * sizeof(double) + 2 * Smax * sizeof(int)
           + (bins ? (size_t)C * sizeof(double) : 0);
}

// Smax / 64 waves rounded to the nearest, 1 .. 4: a wave is added once half of it has states
inline int occ_width(int Lmax) {
    const int Smax = 2 * Lmax + 1;
    const int w = (Smax + 32) / 64 * 64;
    return w < 64 ? 64 : (w > OCC_MAX_WIDTH ? OCC_MAX_WIDTH : w);
}

// log((exp(p1 - m) + exp(p2 - m)) + exp(p3 - m)) + m, m the maximum; -inf when every term is -inf
__device__ __forceinline__ double lse3(double p1, double p2, double p3) {
    const double m = fmax(p1, fmax(p2, p3));
    if (m == -INFINITY) return -INFINITY;
    return log((exp(p1 - m) + exp(p2 - m)) + exp(p3 - m)) + m;
}

template <typename T>
__global__ __launch_bounds__(OCC_MAX_WIDTH) void ctc_occupancy_kernel(
    const T* __restrict__ scores, long long stride_t, long long stride_b, int Tn, int C, int Lmax,
    const long long* __restrict__ targets, long long tstride, const long long* __restrict__ in_len,
    const long long* __restrict__ tg_len, int blank, double* __restrict__ log_z, double* __restrict__ token_occ,
    double* __restrict__ onset, double* __restrict__ class_occ, double* __restrict__ expected_frames,
    double* __restrict__ onset_mean, double* __restrict__ alpha_all) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds[];    // occ_lds_bytes(Lmax, C, class_occ != NULL)
    const int b = blockIdx.x, tid = threadIdx.x, W = blockDim.x;
    const double NINF = -INFINITY;
    const CtcExtent e = ctc_extent(in_len, tg_len, b, Tn, Lmax);
    const int Tb = e.Tb, Lb = e.Lb, S = e.S, Smax = e.Smax;
    double* const row0 = lds;                       // index s + 2: two -inf guards in front, two behind state S - 1
    double* const row1 = row0 + Smax + 4;
    double* const g = row1 + Smax + 4;
    double* const ef = g + Smax;                    // sum_t g_t(2j+1)
    double* const om = ef + Lmax;                   // sum_t t * onset_t(j)
    double* const bins = om + Lmax;
    int* const lab = reinterpret_cast<int*>(bins + (class_occ ? C : 0));
    int* const chain = lab + Smax;                  // next state of the same class (OCC_END: none) | OCC_HEAD on the first
    const long long* tgt = targets + (long long)b * tstride;
    const T* x = scores + (long long)b * stride_b;
    double* const aw = alpha_all + (long long)b * Tn * Smax;
    double* const tok = token_occ ? token_occ + (long long)b * Tn * Lmax : nullptr;
    double* const ons = onset ? onset + (long long)b * Tn * Lmax : nullptr;
    double* const cls = class_occ ? class_occ + (long long)b * Tn * C : nullptr;

    ctc_fill_labels(lab, tgt, S, blank, C, tid, W);
    for (int s = tid; s < Smax + 4; s += W) { row0[s] = NINF; row1[s] = NINF; }
    for (int j = tid; j < Lmax; j += W) { ef[j] = 0.0; om[j] = 0.0; }
    if (cls)
        for (int c = tid; c < C; c += W) bins[c] = 0.0;              // a class without a state stays 0
    // frames from Tb on: zero
    if (tok)
        for (long long i = (long long)Tb * Lmax + tid; i < (long long)Tn * Lmax; i += W) tok[i] = 0.0;
    if (ons)
        for (long long i = (long long)Tb * Lmax + tid; i < (long long)Tn * Lmax; i += W) ons[i] = 0.0;
    if (cls)
        for (long long i = (long long)Tb * C + tid; i < (long long)Tn * C; i += W) cls[i] = 0.0;
    __syncthreads();
    if (cls)
        for (int s = tid; s < S; s += W) {
            const int l = lab[s];
            int nx = OCC_END, head = OCC_HEAD;
            for (int q = s + 1; q < S; ++q)
                if (lab[q] == l) { nx = q; break; }
            for (int q = s - 1; q >= 0; --q)
                if (lab[q] == l) { head = 0; break; }
            chain[s] = nx | head;
        }

    // ---- pass 1: a_t(s), forwards ----
    double lz = Lb == 0 ? 0.0 : NINF;               // Tb == 0
    if (Tb > 0) {
        for (int s = tid; s < S; s += W) {
            const double a = s < 2 ? (double)x[lab[s]] : NINF;
            row0[s + 2] = a;
            aw[s] = a;
        }
        __syncthreads();
        for (int t = 1; t < Tb; ++t) {
            const double* prev = (t & 1) ? row0 : row1;
            double* cur = (t & 1) ? row1 : row0;
            const T* p = x + t * stride_t;
            double* at = aw + (long long)t * Smax;
            for (int s = tid; s < S; s += W) {
                const double xs = (double)p[lab[s]];
                const bool skip = ctc_skip(lab, s);
                const double a = xs + lse3(prev[s + 2], prev[s + 1], skip ? prev[s] : NINF);
                cur[s + 2] = a;
                at[s] = a;
            }
            __syncthreads();
        }
        const double* last = ((Tb - 1) & 1) ? row1 : row0;
        lz = lse3(last[S - 1 + 2], last[S - 2 + 2], NINF);           // S == 1: the front guard
    }
    if (tid == 0) log_z[b] = lz;
    const double qnan = __builtin_nan("");
    if (lz == NINF || Tb == 0) {                    // infeasible, or no frames: nothing to occupy
        if (tok)
            for (long long i = tid; i < (long long)Tb * Lmax; i += W) tok[i] = 0.0;
        if (ons)
            for (long long i = tid; i < (long long)Tb * Lmax; i += W) ons[i] = 0.0;
        if (cls)
            for (long long i = tid; i < (long long)Tb * C; i += W) cls[i] = 0.0;
        for (int j = tid; j < Lmax; j += W) {
            if (expected_frames) expected_frames[(long long)b * Lmax + j] = 0.0;
            if (onset_mean) onset_mean[(long long)b * Lmax + j] = qnan;
        }
        return;
    }

    // ---- pass 2: b_t(s) backwards; the posteriors of frame t leave as soon as b_t is known ----
    __syncthreads();                                // the last row of a has been read by every lane: the rows are free
    for (int s = tid; s < Smax + 4; s += W) { row0[s] = NINF; row1[s] = NINF; }
    __syncthreads();
    for (int t = Tb - 1; t >= 0; --t) {
        const double* nxt = (t & 1) ? row0 : row1;
        double* cur = (t & 1) ? row1 : row0;
        const T* p = x + t * stride_t;
        const double* at = aw + (long long)t * Smax;
        for (int s = tid; s < Smax; s += W) {
            if (s >= S) {                           // tokens past the target's length: zero
                if (s & 1) {
                    if (tok) tok[(long long)t * Lmax + (s >> 1)] = 0.0;
                    if (ons) ons[(long long)t * Lmax + (s >> 1)] = 0.0;
                }
                continue;
            }
            const double a = at[s];
            const bool odd = s & 1;
            const bool skip_in = ctc_skip(lab, s);
            double p1 = NINF, p2 = NINF;
            if (odd && t > 0) {
                p1 = at[s - 1 - Smax];                               // a_{t-1}(2j)
                if (skip_in) p2 = at[s - 2 - Smax];                  // a_{t-1}(2j-1)
            }
            const double xs = (double)p[lab[s]];
            double bt;
            if (t == Tb - 1)
                bt = s >= S - 2 ? xs : NINF;
            else {
                const bool skip_out = s + 2 < S && ctc_skip(lab, s + 2);
                bt = xs + lse3(nxt[s + 2], nxt[s + 3], skip_out ? nxt[s + 4] : NINF);
            }
            cur[s + 2] = bt;
            const double gs = (a == NINF || bt == NINF) ? 0.0 : exp(((a + bt) - xs) - lz);
            g[s] = gs;
            if (odd) {
                const int j = s >> 1;
                double on = gs;
                if (t > 0) {
                    const double l = lse3(p1, p2, NINF);
                    on = (l == NINF || bt == NINF) ? 0.0 : exp((l + bt) - lz);
                }
                if (tok) tok[(long long)t * Lmax + j] = gs;
                if (ons) ons[(long long)t * Lmax + j] = on;
                ef[j] += gs;
                om[j] += (double)t * on;
            }
        }
        __syncthreads();
        if (cls) {
            for (int s = tid; s < S; s += W) {
                int ch = chain[s];
                if (!(ch & OCC_HEAD)) continue;
                double acc = g[s];
                for (int q = ch & OCC_END; q != OCC_END; q = chain[q] & OCC_END) acc += g[q];
                bins[lab[s]] = acc;
            }
            __syncthreads();
            double* ct = cls + (long long)t * C;
            for (int c = tid; c < C; c += W) ct[c] = bins[c];
        }
    }
    // ef / om cells were only ever touched by the lane of their own state
    for (int s = tid; s < Smax; s += W) {
        if (!(s & 1)) continue;
        const int j = s >> 1;
        if (expected_frames) expected_frames[(long long)b * Lmax + j] = s < S ? ef[j] : 0.0;
        if (onset_mean) onset_mean[(long long)b * Lmax + j] = s < S ? om[j] : qnan;
    }
}
}  // namespace

extern "C" size_t xps_ctc_occupancy_workspace(int B, int T, int max_target_len) {
    if (B < 1 || T < 1 || max_target_len < 0) return 16;
    return (size_t)B * (size_t)T * (2 * (size_t)max_target_len + 1) * sizeof(double) + 16;
}

extern "C" int xps_ctc_occupancy(const void* scores, int is_f32, int64_t stride_t, int64_t stride_b, int T, int B, int C,
                                 int max_target_len, const int64_t* targets, int64_t target_stride,
                                 const int64_t* input_lengths, const int64_t* target_lengths, int blank, double* log_z,
                                 double* token_occ, double* onset, double* class_occ, double* expected_frames,
                                 double* onset_mean, void* workspace, size_t workspace_bytes, void* stream) {
    XPS_CTC_CHECK_LATTICE_ARGS();
    if (B == 0) return XPS_OK;
    XPS_CHECK_ARG(log_z, "null argument");
    XPS_CHECK_ARG(scores || T == 0, "null argument");
    XPS_CHECK_ARG(targets || max_target_len == 0, "null argument");
    XPS_CHECK_ARG(workspace && workspace_bytes >= xps_ctc_occupancy_workspace(B, T, max_target_len), "workspace too small");
    XPS_CHECK_ARG((((uintptr_t)log_z | (uintptr_t)token_occ | (uintptr_t)onset | (uintptr_t)class_occ |
                    (uintptr_t)expected_frames | (uintptr_t)onset_mean | (uintptr_t)workspace) & 7) == 0,
                  "output or workspace not 8-byte aligned");
    const size_t lds = occ_lds_bytes(max_target_len, C, class_occ != nullptr);
    XPS_CHECK_ARG(lds <= OCC_LDS_BUDGET, "class bins exceed the LDS budget");
    double* aw = reinterpret_cast<double*>(workspace);
    XPS_CTC_LAUNCH(ctc_occupancy_kernel, dim3(B), dim3(occ_width(max_target_len)), lds, log_z, token_occ, onset, class_occ,
                   expected_frames, onset_mean, aw);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
