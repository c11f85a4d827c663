// Edit-operation alignment: the Levenshtein alignment of B padded pairs, i.e. which prediction tokens hit, substitute or
// are inserted and which target tokens are deleted -- the breakdown of a PER and the confusion matrix of a CTC decoder.
// One wave per pair, one launch for the batch, no host synchronisation, no allocation.
//
// Contract (include/xps.h has the same text).  a = pred of length m, t = tgt of length n:
//     D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + [a_i != t_j], D[i-1][j] + 1, D[i][j-1] + 1)
// Tie rule, on D alone: walking back from (m, n), at i > 0 and j > 0 take the diagonal if D[i][j] == D[i-1][j-1] + [a_i != t_j],
// else the insertion (i-1, j) if D[i][j] == D[i-1][j] + 1, else the deletion (i, j-1); i = 0: deletions, j = 0: insertions.
//
// The forward pass, edit_align_pair<NCH, WALK>, is written once for both entries: the target across the lanes in NCH register
// chunks of 64 columns, 64 prediction tokens per load, the in-row dependency cur[j] = min(tmp[j], cur[j-1] + 1) removed by
// the prefix minimum cur[j] = j + min_{k <= j}(tmp[k] - k), a 6-step wave scan.  xps_edit_distance_i64 launches it with
// WALK = false (edit_distance_kernel: the row pass and dist[b], no other store), and so does xps_edit_align when dist is
// the only output asked for.  With WALK = true, where it has D[i-1][j-1], D[i-1][j] and D[i][j] of a cell
// at hand it evaluates the tie rule and stores the cell's backpointer byte (0 hit, 1 substitution, 2 insertion, 3 deletion):
// 64 consecutive bytes per row and chunk.  Lane 0 then walks at most m + n dependent byte loads back from (m, n) and writes
// the maps, the counts and the confusion adds; the -2 padding of the maps is stored by all lanes before the forward pass, so
// those stores drain behind it.
// The bytes go to the caller's workspace at (b * P + i - 1) * L + j - 1 (P, L the padded extents).  At the training shape a
// pair's table is 4 cache lines that its own CU has just written, and keeping them in LDS instead measured within 3 % of
// this, so there is one route.
// Confusion adds: (K + 1)^2 <= EA_BIN_CELLS cells are summed per workgroup in LDS by the walking lanes and flushed as one
// 64-bit atomic add per non-zero cell, 64 consecutive cells per wave-instruction; adds to the same few cells from every
// walking lane of the chip serialise at the memory side (8.2 ms against 0.54 ms at 2048 x 512 x 64, 11 classes).
#include "xps_common.h"

namespace {
constexpr int EA_BIG = 1 << 29;
constexpr int EA_MAX_PRED = 65536, EA_MAX_TGT = 1024;      // xps_edit_distance_supported: the caps of both entries
constexpr int EA_BIN_CELLS = 8192;                         // confusion cells a workgroup sums in LDS: 32 KB, K <= 89

__device__ inline int ea_prefix_min(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (lane >= d) v = o < v ? o : v;
    }
    return v;
}

__device__ inline int ea_class(long long v, int K) { return v < 0 ? 0 : (v >= K ? K - 1 : (int)v); }

__device__ inline void ea_count(unsigned long long* conf, unsigned int* hist, int cell) {
    if (hist) atomicAdd(hist + cell, 1u);
    else atomicAdd(conf + cell, 1ull);
}

// One pair, by one wave.  WALK: keep the backpointers and walk them back; without it the row pass alone runs, dist[b] is
// the only store and nothing from K on is looked at.  bp: the pair's P * L backpointer bytes in the workspace; hist: the
// workgroup's confusion bins in LDS, or NULL when the adds go straight to `conf`.
template <int NCH, bool WALK>
__device__ inline void edit_align_pair(const long long* __restrict__ pred, long long pred_stride,
                                       const long long* __restrict__ pred_len, const long long* __restrict__ tgt,
                                       long long tgt_stride, const long long* __restrict__ tgt_len, int b, int lane, int P, int L,
                                       long long* __restrict__ dist, int K, long long* __restrict__ counts,
                                       int* __restrict__ tgt_to_pred, int* __restrict__ pred_to_tgt,
                                       unsigned long long* __restrict__ conf, unsigned int* hist, unsigned char* bp) {
    long long ml = pred_len[b], nl = tgt_len[b];
    const int m = ml < 0 ? 0 : (ml > P ? P : (int)ml);                  // lengths clamped to the padded extents: no access outside
    const int n = nl < 0 ? 0 : (nl > L ? L : (int)nl);
    const long long* a = pred + (long long)b * pred_stride;
    const long long* t = tgt + (long long)b * tgt_stride;
    int* t2p = WALK && tgt_to_pred ? tgt_to_pred + (long long)b * L : nullptr;
    int* p2t = WALK && pred_to_tgt ? pred_to_tgt + (long long)b * P : nullptr;
    if (t2p)
        for (int j = n + lane; j < L; j += 64) t2p[j] = -2;
    if (p2t)
        for (int i = m + lane; i < P; i += 64) p2t[i] = -2;

    int prev[NCH];                 // prev[c] = D[i-1][j], j = 64 c + lane + 1
    long long tg[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int j = 64 * c + lane + 1;
        prev[c] = j;
        tg[c] = j <= n ? t[j - 1] : 0;
    }
    const int nch = (n + 63) >> 6;                                       // chunks in use (wave-uniform)
    for (int i0 = 0; i0 < m; i0 += 64) {
        const long long mine = i0 + lane < m ? a[i0 + lane] : 0;         // 64 prediction tokens per load, broadcast per row
        const int rows = m - i0 < 64 ? m - i0 : 64;
        for (int r = 0; r < rows; ++r) {
            const long long tok = __shfl(mine, r, 64);
            const int i = i0 + r + 1;
            unsigned char* row = WALK ? bp + (i - 1) * L : nullptr;      // (i - 1) * L < 2^26
            int diag = i - 1;                                            // D[i-1][64 c]   (column before the chunk)
            int left = i;                                                // D[i][64 c]
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                if (c < nch) {
                    const int j = 64 * c + lane + 1;
                    const int up = prev[c];
                    int ul = __shfl_up(up, 1, 64);
                    if (lane == 0) ul = diag;
                    const int neq = tok != tg[c] ? 1 : 0;
                    const int sub = ul + neq;
                    const int tmp = up + 1 < sub ? up + 1 : sub;
                    const int v = ea_prefix_min(j <= n ? tmp - j : EA_BIG, lane);
                    const int lft = left - 64 * c;                       // (D[i][64 c] + 1) - (64 c + 1): the carried-in run
                    const int cur = j + (v < lft ? v : lft);
                    diag = __shfl(up, 63, 64);
                    left = __shfl(cur, 63, 64);
                    prev[c] = j <= n ? cur : j;
                    if (WALK && j <= n)                                  // the tie rule, on D[i][j], D[i-1][j-1], D[i-1][j]
                        row[j - 1] = (unsigned char)(cur == sub ? neq : (cur == up + 1 ? 2 : 3));
                }
            }
        }
    }
    int res = m;                                                         // n == 0: D[m][0]
    if (n > 0) {
        const int c_last = (n - 1) >> 6, l_last = (n - 1) & 63;
        int val = 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            if (c == c_last) val = prev[c];
        res = __shfl(val, l_last, 64);
    }
    if (lane == 0) dist[b] = res;
    if (!WALK) return;
    __threadfence_block();                                               // the wave's own backpointer stores, before lane 0 reads them
    if (lane != 0) return;
    // ---- the walk back from (m, n): one lane, at most m + n dependent byte loads ----
    int i = m, j = n;
    int hits = 0, subs = 0, dels = 0, ins = 0;
    const int K1 = K + 1;
    while (i > 0 || j > 0) {
        const int k = i == 0 ? 3 : (j == 0 ? 2 : (int)bp[(i - 1) * L + (j - 1)]);
        if (k <= 1) {
            if (t2p) t2p[j - 1] = i - 1;
            if (p2t) p2t[i - 1] = j - 1;
            if (conf) ea_count(conf, hist, ea_class(t[j - 1], K) * K1 + ea_class(a[i - 1], K));
            hits += 1 - k;
            subs += k;
            --i;
            --j;
        } else if (k == 2) {
            if (p2t) p2t[i - 1] = -1;
            if (conf) ea_count(conf, hist, K * K1 + ea_class(a[i - 1], K));
            ++ins;
            --i;
        } else {
            if (t2p) t2p[j - 1] = -1;
            if (conf) ea_count(conf, hist, ea_class(t[j - 1], K) * K1 + K);
            ++dels;
            --j;
        }
    }
    if (counts) {
        long long* cnt = counts + 4ll * b;
        cnt[0] = hits;
        cnt[1] = subs;
        cnt[2] = dels;
        cnt[3] = ins;
    }
}

// 4 waves, 4 pairs: the row pass alone.
template <int NCH>
__global__ __launch_bounds__(256) void edit_distance_kernel(const long long* __restrict__ pred, long long pred_stride,
                                                            const long long* __restrict__ pred_len, const long long* __restrict__ tgt,
                                                            long long tgt_stride, const long long* __restrict__ tgt_len, int B,
                                                            int P, int L, long long* __restrict__ dist) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b < B)
        edit_align_pair<NCH, false>(pred, pred_stride, pred_len, tgt, tgt_stride, tgt_len, b, threadIdx.x & 63, P, L, dist, 0,
                                    nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// 4 waves, 4 pairs.  Dynamic LDS: `bins` confusion counters of the workgroup (0: none).
template <int NCH>
__global__ __launch_bounds__(256) void edit_align_kernel(const long long* __restrict__ pred, long long pred_stride,
                                                         const long long* __restrict__ pred_len, const long long* __restrict__ tgt,
                                                         long long tgt_stride, const long long* __restrict__ tgt_len, int B,
                                                         int P, int L, long long* __restrict__ dist, int K,
                                                         long long* __restrict__ counts, int* __restrict__ tgt_to_pred,
                                                         int* __restrict__ pred_to_tgt, unsigned long long* __restrict__ conf,
                                                         unsigned char* __restrict__ ws, int bins) {
    extern __shared__ unsigned int ea_lds[];
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    unsigned int* hist = bins ? ea_lds : nullptr;
    if (bins) {
        for (int c = threadIdx.x; c < bins; c += 256) ea_lds[c] = 0;
        __syncthreads();
    }
    if (b < B) {                                                         // a whole wave at a time: no divergence at the barriers
        edit_align_pair<NCH, true>(pred, pred_stride, pred_len, tgt, tgt_stride, tgt_len, b, lane, P, L, dist, K, counts,
                                   tgt_to_pred, pred_to_tgt, conf, hist, ws + (size_t)b * (size_t)P * (size_t)L);
    }
    if (bins) {                                                          // one add per non-zero cell and workgroup, 64 cells per
        __syncthreads();                                                 // wave-instruction: 4 pairs' steps cost a few instructions
        for (int c = threadIdx.x; c < bins; c += 256) {
            const unsigned int v = ea_lds[c];
            if (v) atomicAdd(conf + c, (unsigned long long)v);
        }
    }
}

// KERNEL<NCH> for the padded target extent, 4 pairs per workgroup, over the entry's own arguments up to dist, then the
// kernel's further arguments
#define XPS_EDIT_LAUNCH_NCH(KERNEL, NCH, lds, ...)                                                                            \
    hipLaunchKernelGGL(KERNEL<NCH>, dim3(cdiv(B, 4)), dim3(256), lds, (hipStream_t)stream,                                    \
                       reinterpret_cast<const long long*>(pred), (long long)pred_stride,                                      \
                       reinterpret_cast<const long long*>(pred_len), reinterpret_cast<const long long*>(tgt),                 \
                       (long long)tgt_stride, reinterpret_cast<const long long*>(tgt_len), B, max_pred_len, max_tgt_len,      \
                       reinterpret_cast<long long*>(dist), ##__VA_ARGS__)
#define XPS_EDIT_LAUNCH(KERNEL, lds, ...)                                                                                     \
    do {                                                                                                                      \
        if (max_tgt_len <= 64) XPS_EDIT_LAUNCH_NCH(KERNEL, 1, lds, ##__VA_ARGS__);                                            \
        else if (max_tgt_len <= 256) XPS_EDIT_LAUNCH_NCH(KERNEL, 4, lds, ##__VA_ARGS__);                                      \
        else XPS_EDIT_LAUNCH_NCH(KERNEL, 16, lds, ##__VA_ARGS__);                                                             \
    } while (0)
}  // namespace

extern "C" size_t xps_edit_align_workspace(int B, int max_pred_len, int max_tgt_len) {
    if (B < 1 || max_pred_len < 1 || max_tgt_len < 1) return 16;
    return (size_t)B * (size_t)max_pred_len * (size_t)max_tgt_len + 16;
}

extern "C" int xps_edit_distance_supported(int max_pred_len, int max_tgt_len) {
    return max_pred_len >= 0 && max_pred_len <= EA_MAX_PRED && max_tgt_len >= 0 && max_tgt_len <= EA_MAX_TGT;
}

extern "C" int xps_edit_distance_i64(const int64_t* pred, int64_t pred_stride, const int64_t* pred_len, const int64_t* tgt,
                                     int64_t tgt_stride, const int64_t* tgt_len, int B, int max_pred_len, int max_tgt_len,
                                     int64_t* dist, void* stream) {
    XPS_CHECK_ARG(B >= 0, "bad argument");
    XPS_CHECK_ARG(xps_edit_distance_supported(max_pred_len, max_tgt_len), "sequence lengths outside the supported range");
    XPS_CHECK_ARG(pred_stride >= max_pred_len && tgt_stride >= max_tgt_len, "row stride shorter than the padded length");
    if (B == 0) return XPS_OK;
    XPS_CHECK_ARG(pred_len && tgt_len && dist, "null argument");
    XPS_CHECK_ARG((pred || max_pred_len == 0) && (tgt || max_tgt_len == 0), "null argument");
    XPS_EDIT_LAUNCH(edit_distance_kernel, 0);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}

extern "C" int xps_edit_align(const int64_t* pred, int64_t pred_stride, const int64_t* pred_len, const int64_t* tgt,
                              int64_t tgt_stride, const int64_t* tgt_len, int B, int max_pred_len, int max_tgt_len,
                              int n_classes, int64_t* dist, int64_t* counts, int32_t* tgt_to_pred, int32_t* pred_to_tgt,
                              int64_t* confusion, void* workspace, size_t workspace_bytes, void* stream) {
    XPS_CHECK_ARG(B >= 0, "bad argument");
    XPS_CHECK_ARG(xps_edit_distance_supported(max_pred_len, max_tgt_len), "sequence lengths outside the supported range");
    XPS_CHECK_ARG(pred_stride >= max_pred_len && tgt_stride >= max_tgt_len, "row stride shorter than the padded length");
    XPS_CHECK_ARG(!confusion || n_classes >= 1, "a confusion matrix needs at least one class");
    if (B == 0) return XPS_OK;
    XPS_CHECK_ARG(pred_len && tgt_len && dist, "null argument");
    XPS_CHECK_ARG((pred || max_pred_len == 0) && (tgt || max_tgt_len == 0), "null argument");
    XPS_CHECK_ARG(workspace && workspace_bytes >= xps_edit_align_workspace(B, max_pred_len, max_tgt_len), "workspace too small");
    if (!counts && !tgt_to_pred && !pred_to_tgt && !confusion) {        // dist alone: no backpointers, no walk
        XPS_EDIT_LAUNCH(edit_distance_kernel, 0);
        XPS_CHECK_LAUNCH();
        return XPS_OK;
    }
    long long* cn = reinterpret_cast<long long*>(counts);
    unsigned long long* cf = reinterpret_cast<unsigned long long*>(confusion);
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    const long long conf_cells = ((long long)n_classes + 1) * ((long long)n_classes + 1);
    const int bins = confusion && conf_cells <= EA_BIN_CELLS ? (int)conf_cells : 0;
    XPS_EDIT_LAUNCH(edit_align_kernel, sizeof(unsigned int) * (size_t)bins, n_classes, cn, tgt_to_pred, pred_to_tgt, cf, ws, bins);
    XPS_CHECK_LAUNCH();
    return XPS_OK;
}
