// CTC prefix beam search on the device (realtime_sim/ctc_decoder.py decode / beam_decode_batch, RealtimePipeline's beam
// decoder).  fp64 throughout, the same operations in the same order as the reference's dict-based search:
// one workgroup per sequence, one call of beam_step per frame.  The offline batch keeps the beam in LDS for all frames;
// the streaming step keeps it in a caller-owned device state between graph replays and runs the same beam_step, so a
// stream after n frames is bit-identical to the offline search over those n frames.
#include "xps_common.h"

#pragma clang fp contract(off)   // every + and - rounds on its own, as the reference's Python floats do

namespace {

constexpr int BEAM_MAX = 128, CLS_MAX = 64, CAND_MAX = 8192, MAXS = 8, MAX_STEPS = 1 << 20;
constexpr int OFF_THREADS = 256, STEP_THREADS = 1024;
constexpr int INVALID_KEY = 1 << 20, PAD_KEY = 0x7fffffff, CAND_PAD = 8;
constexpr double NEG_INF = -__builtin_inf();

// Prefix identity: two polynomial hashes modulo the Mersenne prime 2^61 - 1 with independent bases, plus the length.
constexpr unsigned long long HMOD = (1ull << 61) - 1, HBASE1 = 0x1f3d5b79a2c4e68dull % HMOD,
                             HBASE2 = 0x0b9e2a6c7f15d34bull % HMOD;

__device__ inline unsigned long long mulmod61(unsigned long long a, unsigned long long b) {
    const unsigned long long lo = a * b, hi = __umul64hi(a, b);              // a, b < 2^61: hi < 2^58
    unsigned long long r = (lo & HMOD) + (lo >> 61) + (hi << 3);             // 2^64 = 8 * 2^61 = 8 (mod HMOD)
    r = (r & HMOD) + (r >> 61);
    return r >= HMOD ? r - HMOD : r;
}
__device__ inline unsigned long long hash_push(unsigned long long h, unsigned long long base, int tok) {
    const unsigned long long r = mulmod61(h, base) + (unsigned long long)(tok + 1);
    return r >= HMOD ? r - HMOD : r;
}

// The reference's logsumexp(*args): -inf if every argument is -inf, else m + log(sum exp(a - m)) summed left to right,
// m the first maximum.
__device__ inline double lse2(double a, double b) {
    if (a == NEG_INF && b == NEG_INF) return NEG_INF;
    const double m = b > a ? b : a;
    double s = 0.0;
    s += exp(a - m);
    s += exp(b - m);
    return m + log(s);
}
__device__ inline double lse3(double a, double b, double c) {
    if (a == NEG_INF && b == NEG_INF && c == NEG_INF) return NEG_INF;
    double m = b > a ? b : a;
    m = c > m ? c : m;
    double s = 0.0;
    s += exp(a - m);
    s += exp(b - m);
    s += exp(c - m);
    return m + log(s);
}
// lse(-inf, a, b) and lse(-inf, a): the leading -inf adds exp(-inf) = 0.0 to an exact 0.0, so the sum starts at the
// first real term; with m = a, lse(-inf, a) = a + log(exp(0.0)) = a + 0.0.  Same bits as the general forms.
__device__ inline double lse_ninf(double a, double b) {
    if (a == NEG_INF && b == NEG_INF) return NEG_INF;
    const double m = b > a ? b : a;
    double s = exp(a - m);
    s += exp(b - m);
    return m + log(s);
}
__device__ inline double lse_ninf(double a) { return a == NEG_INF ? NEG_INF : a + 0.0; }

// Insertion key (s, member, sub) of the reference's dict, lexicographic as one int.
__device__ inline int ikey(int s, int k, int sub) { return (s * BEAM_MAX + k) * 2 + sub; }

// One set of beam members, K = beam_size slots; the arrays may live in LDS or in global memory (flat pointers).
struct Beam {
    double *pb, *pnb;
    unsigned long long *h1, *h2, *hp1, *hp2;   // hashes of the prefix and of the prefix without its last token
    unsigned long long* cmask;                 // bit s: prefix + (s,) is a member
    int *len, *last, *parent;                  // last = -1 for (); parent = member equal to prefix[:-1], or -1
};
__host__ __device__ inline size_t beam_set_bytes(int K) { return ((size_t)K * 68 + 63) / 64 * 64; }
__device__ inline Beam beam_at(unsigned char* p, int K) {
    Beam b;
    b.pb = (double*)p;
    b.pnb = b.pb + K;
    b.h1 = (unsigned long long*)(b.pnb + K);
    b.h2 = b.h1 + K;
    b.hp1 = b.h2 + K;
    b.hp2 = b.hp1 + K;
    b.cmask = b.hp2 + K;
    b.len = (int*)(b.cmask + K);
    b.last = b.len + K;
    b.parent = b.last + K;
    return b;
}
__device__ inline void beam_init(const Beam& b) {   // the empty prefix, p_b = log 1, p_nb = -inf
    b.pb[0] = 0.0;
    b.pnb[0] = NEG_INF;
    b.h1[0] = b.h2[0] = b.hp1[0] = b.hp2[0] = b.cmask[0] = 0;
    b.len[0] = 0;
    b.last[0] = -1;
    b.parent[0] = -1;
}

// Streaming state of one stream: header {step, n_members, overflow, 0} int32, the member set after `step` frames,
// backpointers hist[max_steps][K] int32 = member of the previous step | (appended token + 1) << 16.
__host__ __device__ inline size_t state_stride(int K, int max_steps) {
    return (64 + beam_set_bytes(K) + (size_t)max_steps * K * 4 + 255) / 256 * 256;
}

// lp[s] (LDS) = row as fp64, or its fp64 log-softmax (x - m) - log(sum exp(x - m)).
__device__ inline void load_row(const void* row, int is_f32, int S, int from_logits, double* lp) {
    const int s = threadIdx.x;
    if (s >= S) return;
    auto at = [&](int i) { return is_f32 ? (double)((const float*)row)[i] : ((const double*)row)[i]; };
    double x = at(s);
    if (from_logits) {
        double m = at(0);
        for (int i = 1; i < S; ++i) m = at(i) > m ? at(i) : m;
        double sum = 0.0;
        for (int i = 0; i < S; ++i) sum += exp(at(i) - m);
        x = (x - m) - log(sum);
    }
    lp[s] = x;
}

// The unchanged candidate of member k: scores and insertion key.
__device__ inline void unchanged_cand(const Beam& b, int k, const double* lp, int blank, double& npb, double& npnb, int& key) {
    const double pb = b.pb[k], pnb = b.pnb[k];
    npb = lse_ninf(pb + lp[blank], pnb + lp[blank]);
    npnb = NEG_INF;
    key = ikey(blank, k, 0);
    if (b.len[k] == 0) return;
    const int last = b.last[k], j = b.parent[k];
    const double q = lp[last];
    key = min(key, ikey(last, k, 1));
    if (j < 0) {
        npnb = lse_ninf(pnb + q);
        return;
    }
    key = min(key, ikey(last, j, 0));
    if (k < j) npnb = lse2(npnb, pnb + q);                           // self-merge (last, k, 1) first
    if (b.last[j] == last) npnb = lse2(npnb, b.pb[j] + q);           // extension of j (last, j, 0)
    else npnb = lse3(npnb, b.pb[j] + q, b.pnb[j] + q);
    if (j < k) npnb = lse2(npnb, pnb + q);
}

__device__ inline double ext_pnb(const Beam& b, int k, int s, const double* lp) {
    const double q = lp[s];
    return s == b.last[k] ? lse_ninf(b.pb[k] + q) : lse_ninf(b.pb[k] + q, b.pnb[k] + q);
}

// win[rank] = c for the valid candidates of rank < n_new: every thread compares U candidates with all N8 slots.
template <int U>
__device__ __forceinline__ void rank_candidates(const double* csc, const int* cik, int N, int N8, int n_new, int* win) {
    const int nt = blockDim.x;
    for (int c0 = threadIdx.x; c0 < N; c0 += U * nt) {
        double sc[U];
        int key[U], r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * nt;
            sc[u] = c < N ? csc[c] : NEG_INF;
            key[u] = c < N ? cik[c] : INVALID_KEY - 1;
            r[u] = 0;
        }
        for (int c2 = 0; c2 < N8; c2 += CAND_PAD) {   // eight LDS broadcasts in flight per round
            double s2[CAND_PAD];
            int k2[CAND_PAD];
#pragma unroll
            for (int v = 0; v < CAND_PAD; ++v) {
                s2[v] = csc[c2 + v];
                k2[v] = cik[c2 + v];
            }
#pragma unroll
            for (int v = 0; v < CAND_PAD; ++v)
#pragma unroll
                for (int u = 0; u < U; ++u) r[u] += (s2[v] > sc[u]) | ((s2[v] == sc[u]) & (k2[v] < key[u]));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u * nt;
            if (c < N && key[u] < INVALID_KEY && r[u] < n_new) win[r[u]] = c;
        }
    }
}

// One frame for the calling workgroup: cur (n members) -> nxt, backpointers into hist[0 .. n_new).  Candidate c = k * S + s
// is the unchanged prefix of member k for s == blank, else its extension by s.  cur, nxt, lp, csc / cik [K * S + CAND_PAD]
// and win [K] are LDS.
// Returns the new member count (the same in every thread).  Starts and ends with the workgroup in step.
__device__ __forceinline__ int beam_step(const double* lp, int S, int blank, int K, const Beam cur, int n, const Beam nxt, double* csc,
                         int* cik, int* win, int* hist) {
    const int tid = threadIdx.x, nt = blockDim.x, N = n * S, N8 = (N + CAND_PAD - 1) / CAND_PAD * CAND_PAD;
    // candidates: score = lse(p_b', p_nb') (NaN ranks as -inf), insertion key; merged extensions are invalid; the padding
    // to a multiple of 8 ranks after everything
    for (int c = tid; c < N8; c += nt) {
        if (c >= N) {
            csc[c] = NEG_INF;
            cik[c] = PAD_KEY;
            continue;
        }
        const int k = c / S, s = c - k * S;
        double sc;
        int key;
        if (s == blank) {
            double npb, npnb;
            unchanged_cand(cur, k, lp, blank, npb, npnb, key);
            sc = lse2(npb, npnb);
        } else if ((cur.cmask[k] >> s) & 1ull) {
            sc = NEG_INF;
            key = INVALID_KEY + c;
        } else {
            sc = lse_ninf(ext_pnb(cur, k, s, lp));
            key = ikey(s, k, 0);
        }
        csc[c] = sc != sc ? NEG_INF : sc;
        cik[c] = key;
    }
    int n_valid = N;
    for (int k = 0; k < n; ++k) n_valid -= __popcll(cur.cmask[k]);
    const int n_new = min(K, n_valid);
    __syncthreads();
    // rank = number of candidates before c in (score descending, key ascending); invalid ones come after every valid one.
    // U candidates per thread and pass: 1 while two passes cover them (the streaming step's 1024 threads), else 4.
    if (N <= 2 * nt) rank_candidates<1>(csc, cik, N, N8, n_new, win);
    else rank_candidates<4>(csc, cik, N, N8, n_new, win);
    __syncthreads();
    // the new members, in rank order
    for (int r = tid; r < n_new; r += nt) {
        const int c = win[r], k = c / S, s = c - k * S;
        if (s == blank) {
            int key;
            unchanged_cand(cur, k, lp, blank, nxt.pb[r], nxt.pnb[r], key);
            nxt.h1[r] = cur.h1[k];
            nxt.h2[r] = cur.h2[k];
            nxt.hp1[r] = cur.hp1[k];
            nxt.hp2[r] = cur.hp2[k];
            nxt.len[r] = cur.len[k];
            nxt.last[r] = cur.last[k];
            hist[r] = k;
        } else {
            nxt.pb[r] = NEG_INF;
            nxt.pnb[r] = ext_pnb(cur, k, s, lp);
            nxt.hp1[r] = cur.h1[k];
            nxt.hp2[r] = cur.h2[k];
            nxt.h1[r] = hash_push(cur.h1[k], HBASE1, s);
            nxt.h2[r] = hash_push(cur.h2[k], HBASE2, s);
            nxt.len[r] = cur.len[k] + 1;
            nxt.last[r] = s;
            hist[r] = k | ((s + 1) << 16);
        }
    }
    __syncthreads();
    // links among the new members: parent (prefix[:-1]) and the tokens whose extension is already a member
    for (int m = tid; m < n_new; m += nt) {
        const int lm = nxt.len[m];
        const unsigned long long h1 = nxt.h1[m], h2 = nxt.h2[m], hp1 = nxt.hp1[m], hp2 = nxt.hp2[m];
        int parent = -1;
        unsigned long long mask = 0;
#pragma unroll 4
        for (int j = 0; j < n_new; ++j) {
            const int lj = nxt.len[j];
            if (lj + 1 == lm && nxt.h1[j] == hp1 && nxt.h2[j] == hp2) parent = j;
            if (lm + 1 == lj && nxt.hp1[j] == h1 && nxt.hp2[j] == h2) mask |= 1ull << nxt.last[j];
        }
        nxt.parent[m] = parent;
        nxt.cmask[m] = mask;
    }
    __syncthreads();
    return n_new;
}

// Prefix of member 0 after `steps` frames from the backpointers (one thread), its length and nll.
__device__ void walk_back(const int* hist, int K, int steps, int len, long long* prefix) {
    int i = 0, pos = len - 1;
    for (int t = steps - 1; t >= 0; --t) {
        const int e = hist[(long long)t * K + i];
        const int tok = (e >> 16) - 1;
        if (tok >= 0) prefix[pos--] = tok;
        i = e & 0xffff;
    }
}

__device__ inline unsigned char* lds_carve(unsigned char*& p, size_t bytes) {   // 16-byte aligned pieces
    unsigned char* r = p;
    p += (bytes + 15) / 16 * 16;
    return r;
}

__global__ __launch_bounds__(OFF_THREADS) void ctc_beam_kernel(const void* __restrict__ lp_in, int is_f32, int T, int S,
                                                               const long long* __restrict__ lens, int blank, int K,
                                                               int from_logits, long long* __restrict__ prefix,
                                                               long long* __restrict__ plen, double* __restrict__ nll,
                                                               int* __restrict__ hist_all) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    unsigned char* p = lds_raw;
    double* lp = (double*)lds_carve(p, CLS_MAX * sizeof(double));
    double* csc = (double*)lds_carve(p, ((size_t)K * S + CAND_PAD) * sizeof(double));
    const size_t sb = beam_set_bytes(K);
    unsigned char* sets = lds_carve(p, 2 * sb);
    int* cik = (int*)lds_carve(p, ((size_t)K * S + CAND_PAD) * sizeof(int));
    int* win = (int*)lds_carve(p, (size_t)K * sizeof(int));

    const int b = blockIdx.x;
    long long tb = lens ? lens[b] : T;
    const int Tb = (int)(tb < 0 ? 0 : tb > T ? T : tb);
    int* hist = hist_all + (long long)b * T * K;
    const size_t esz = is_f32 ? 4 : 8;
    const unsigned char* rows = (const unsigned char*)lp_in + (size_t)b * T * S * esz;
    if (threadIdx.x == 0) beam_init(beam_at(sets, K));
    __syncthreads();
    int n = 1;
    for (int t = 0; t < Tb; ++t) {
        load_row(rows + (size_t)t * S * esz, is_f32, S, from_logits, lp);
        __syncthreads();
        n = beam_step(lp, S, blank, K, beam_at(sets + (t & 1) * sb, K), n, beam_at(sets + ((t & 1) ^ 1) * sb, K), csc, cik,
                      win, hist + (long long)t * K);
    }
    const Beam fin = beam_at(sets + (Tb & 1) * sb, K);
    const int len = fin.len[0];
    long long* out = prefix + (long long)b * T;
    if (threadIdx.x == 0) {
        walk_back(hist, K, Tb, len, out);
        plen[b] = len;
        nll[b] = -lse2(fin.pb[0], fin.pnb[0]);
    }
    for (int i = len + threadIdx.x; i < T; i += blockDim.x) out[i] = -1;
}

// The beam is copied into LDS, advanced by the offline kernel's beam_step, and copied back.
__global__ __launch_bounds__(STEP_THREADS) void ctc_beam_step_kernel(const float* __restrict__ logits, int S, int blank, int K,
                                                                     int max_steps, unsigned char* __restrict__ state,
                                                                     size_t stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    unsigned char* p = lds_raw;
    double* lp = (double*)lds_carve(p, CLS_MAX * sizeof(double));
    double* csc = (double*)lds_carve(p, ((size_t)K * S + CAND_PAD) * sizeof(double));
    const size_t sb = beam_set_bytes(K);
    unsigned char* sets = lds_carve(p, 2 * sb);
    int* cik = (int*)lds_carve(p, ((size_t)K * S + CAND_PAD) * sizeof(int));
    int* win = (int*)lds_carve(p, (size_t)K * sizeof(int));

    const int b = blockIdx.x;
    unsigned char* st = state + (size_t)b * stride;
    int* hdr = (int*)st;
    const int step = hdr[0];
    const int n = step == 0 ? 1 : min(max(hdr[1], 1), K);
    __syncthreads();                                  // every thread has read the header before thread 0 rewrites it
    if (step >= max_steps) {                          // sticky overflow: the beam stays as it is
        if (threadIdx.x == 0) hdr[2] = 1;
        return;
    }
    unsigned long long* gset = (unsigned long long*)(st + 64);
    int* hist = (int*)(st + 64 + sb) + (long long)step * K;
    if (step == 0) {
        if (threadIdx.x == 0) beam_init(beam_at(sets, K));
    } else {
        for (size_t i = threadIdx.x; i < sb / 8; i += blockDim.x) ((unsigned long long*)sets)[i] = gset[i];
    }
    load_row(logits + (long long)b * S, 1, S, 1, lp);
    __syncthreads();
    const int n_new = beam_step(lp, S, blank, K, beam_at(sets, K), n, beam_at(sets + sb, K), csc, cik, win, hist);
    for (size_t i = threadIdx.x; i < sb / 8; i += blockDim.x) gset[i] = ((const unsigned long long*)(sets + sb))[i];
    if (threadIdx.x == 0) {
        hdr[0] = step + 1;
        hdr[1] = n_new;
    }
}

__global__ void ctc_beam_readout_kernel(const unsigned char* __restrict__ st, int K, int max_steps,
                                        long long* __restrict__ prefix, long long* __restrict__ plen, double* __restrict__ nll) {
    if (threadIdx.x != 0) return;
    const int step = min(((const int*)st)[0], max_steps);
    if (step == 0) {
        plen[0] = 0;
        nll[0] = -lse2(0.0, NEG_INF);
        return;
    }
    const Beam fin = beam_at((unsigned char*)st + 64, K);
    const int len = fin.len[0];
    walk_back((const int*)(st + 64 + beam_set_bytes(K)), K, step, len, prefix);
    plen[0] = len;
    nll[0] = -lse2(fin.pb[0], fin.pnb[0]);
}

inline size_t r16(size_t b) { return (b + 15) / 16 * 16; }
size_t beam_lds(int K, int S) {   // the carving order of both kernels: lp, csc, two member sets, cik, win
    return r16(CLS_MAX * 8) + r16(((size_t)K * S + CAND_PAD) * 8) + r16(2 * beam_set_bytes(K)) +
           r16(((size_t)K * S + CAND_PAD) * 4) + r16((size_t)K * 4);
}

int raise_lds_limit(const void* fn, size_t bytes, bool& done) {
    if (!done) {
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return XPS_E_HIP;
        done = true;
    }
    return XPS_OK;
}

}  // namespace

#define XPS_BEAM_CHECK_SIZES(S, K, blank)                                                                           \
    XPS_CHECK_ARG((S) >= 1 && (S) <= CLS_MAX, "n_classes outside 1..64");                                           \
    XPS_CHECK_ARG((K) >= 1 && (K) <= BEAM_MAX, "beam_size outside 1..128");                                         \
    XPS_CHECK_ARG((long long)(K) * (S) <= CAND_MAX, "beam_size * n_classes > 8192");                                \
    XPS_CHECK_ARG((blank) >= 0 && (blank) < (S), "blank outside the classes")

extern "C" size_t xps_ctc_beam_workspace(int B, int T, int beam_size, int n_classes) {
    (void)n_classes;
    if (B < 0 || T < 0 || beam_size < 1) return 0;
    return ((size_t)B * T * beam_size * 4 + 255) / 256 * 256;
}

extern "C" int xps_ctc_beam_f64(const void* log_probs, int is_f32, int B, int T, int n_classes,
                                const int64_t* input_lengths, int blank, int beam_size, int from_logits, int64_t* prefix,
                                int64_t* prefix_len, double* nll, void* workspace, size_t workspace_bytes, void* stream) {
    XPS_CHECK_ARG(B >= 0 && T >= 0, "bad argument");
    XPS_CHECK_ARG((is_f32 == 0 || is_f32 == 1) && (from_logits == 0 || from_logits == 1), "flags must be 0 or 1");
    XPS_BEAM_CHECK_SIZES(n_classes, beam_size, blank);
    if (B == 0) return XPS_OK;
    XPS_CHECK_ARG(prefix_len && nll && (T == 0 || (log_probs && prefix && workspace)), "bad argument");
    if (workspace_bytes < xps_ctc_beam_workspace(B, T, beam_size, n_classes)) {
        xps_set_error("xps_ctc_beam_f64: workspace of %zu bytes, %zu needed", workspace_bytes,
                      xps_ctc_beam_workspace(B, T, beam_size, n_classes));
        return XPS_E_WORKSPACE;
    }
    static bool attr = false;
    if (raise_lds_limit(reinterpret_cast<const void*>(ctc_beam_kernel), beam_lds(BEAM_MAX, CAND_MAX / BEAM_MAX) + 4096,
                        attr) != XPS_OK) {
        xps_set_error("xps_ctc_beam_f64: cannot raise the dynamic LDS limit");
        return XPS_E_HIP;
    }
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(B), dim3(OFF_THREADS), beam_lds(beam_size, n_classes), (hipStream_t)stream,
                       log_probs, is_f32, T, n_classes, (const long long*)input_lengths, blank, beam_size, from_logits,
                       (long long*)prefix, (long long*)prefix_len, nll, (int*)workspace);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" size_t xps_ctc_beam_state_bytes(int n_streams, int beam_size, int max_steps) {
    if (n_streams < 1 || beam_size < 1 || max_steps < 1) return 0;
    return (size_t)n_streams * state_stride(beam_size, max_steps);
}

extern "C" int xps_ctc_beam_step_f32(const float* logits, int n_classes, int blank, int beam_size, int max_steps,
                                     void* state, size_t state_bytes, int B, void* stream) {
    XPS_CHECK_ARG(logits && state, "bad argument");
    XPS_CHECK_ARG(B >= 1 && B <= MAXS, "1..8 streams per call");
    XPS_CHECK_ARG(max_steps >= 1 && max_steps <= MAX_STEPS, "max_steps outside 1..2^20");
    XPS_BEAM_CHECK_SIZES(n_classes, beam_size, blank);
    if (state_bytes < xps_ctc_beam_state_bytes(B, beam_size, max_steps)) {
        xps_set_error("xps_ctc_beam_step_f32: state of %zu bytes, %zu needed", state_bytes,
                      xps_ctc_beam_state_bytes(B, beam_size, max_steps));
        return XPS_E_WORKSPACE;
    }
    static bool attr = false;
    if (raise_lds_limit(reinterpret_cast<const void*>(ctc_beam_step_kernel), beam_lds(BEAM_MAX, CAND_MAX / BEAM_MAX) + 4096,
                        attr) != XPS_OK) {
        xps_set_error("xps_ctc_beam_step_f32: cannot raise the dynamic LDS limit");
        return XPS_E_HIP;
    }
    hipLaunchKernelGGL(ctc_beam_step_kernel, dim3(B), dim3(STEP_THREADS), beam_lds(beam_size, n_classes),
                       (hipStream_t)stream, logits, n_classes, blank, beam_size, max_steps, (unsigned char*)state,
                       state_stride(beam_size, max_steps));
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_ctc_beam_readout(const void* state, size_t state_bytes, int B, int beam_size, int max_steps, int s,
                                    int64_t* prefix, int64_t* prefix_len, double* nll, void* stream) {
    XPS_CHECK_ARG(state && prefix && prefix_len && nll, "bad argument");
    XPS_CHECK_ARG(B >= 1 && B <= MAXS, "1..8 streams per call");
    XPS_CHECK_ARG(s >= 0 && s < B, "stream index outside 0..B-1");
    XPS_CHECK_ARG(beam_size >= 1 && beam_size <= BEAM_MAX, "beam_size outside 1..128");
    XPS_CHECK_ARG(max_steps >= 1 && max_steps <= MAX_STEPS, "max_steps outside 1..2^20");
    if (state_bytes < xps_ctc_beam_state_bytes(B, beam_size, max_steps)) {
        xps_set_error("xps_ctc_beam_readout: state of %zu bytes, %zu needed", state_bytes,
                      xps_ctc_beam_state_bytes(B, beam_size, max_steps));
        return XPS_E_WORKSPACE;
    }
    hipLaunchKernelGGL(ctc_beam_readout_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       (const unsigned char*)state + (size_t)s * state_stride(beam_size, max_steps), beam_size, max_steps,
                       (long long*)prefix, (long long*)prefix_len, nll);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
