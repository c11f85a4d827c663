/* xps.h -- C ABI of libxps.so, the MI355X (gfx950) hot path of the cross-patient
 * speech-decoding trainer.
 *
 * The reference (coganlab/cross_patient_speech_decoding) is pure Python and has no
 * FFI of its own; every entry point below replaces a library call the reference
 * makes on its aligned-training path.  The "replaces" notes cite
 * /root/reference/aligned_decoding/<file>:<line>.
 *
 * Contract (boundary B2)
 *   - plain pointers and sizes only; all data pointers are DEVICE pointers unless a
 *     parameter is documented as host;
 *   - the caller owns every buffer, including workspaces whose size is returned by
 *     the matching xps_*_workspace() query; the library never allocates, frees or
 *     keeps a pointer after the call returns;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); it
 *     never synchronises, so calls compose with autograd ordering and can be
 *     captured into a hipGraph;
 *   - return value: 0 = ok, negative = error (XPS_E_*); xps_last_error() returns a
 *     thread-local message.  No C++ exception crosses the boundary;
 *   - re-entrant.  Global state: ONE table of process-wide switches (xps_set_switch below; among them the product precision
 *     of the matrix kernels and the launch form of the H > 256 recurrence), each a plain integer read at call time,
 *     plus a per-device cache of immutable device facts (CU count, resident workgroups of the cluster kernels) and the
 *     caller's per-device status word (xps_gru_set_status_word); nothing else outlives a call.
 *
 * Matrices are row-major float32 unless stated.  A "row map" (rpg, gs, ld) addresses
 * row i of a matrix at element offset  (i / rpg) * gs + (i % rpg) * ld ; an ordinary
 * matrix has rpg >= rows and ld = leading dimension.  It lets one GEMM read the
 * strided-convolution windows of a (trial x time x channel) tensor and write
 * time-major results without a copy.
 */
#ifndef XPS_H
#define XPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XPS_OK 0
#define XPS_E_INVALID (-1)     /* bad argument / unsupported shape */
#define XPS_E_HIP (-2)         /* a HIP runtime call failed */
#define XPS_E_WORKSPACE (-3)   /* workspace too small */

typedef struct xps_rowmap {
    int64_t gs;    /* stride between groups of rows            */
    int64_t ld;    /* stride between rows inside a group       */
    int32_t rpg;   /* rows per group (>= 1)                    */
    int32_t fmt;   /* XPS_FMT_F32 (0) or XPS_FMT_SPLIT4 (1): element format of a GEMM INPUT operand (ignored for outputs) */
} xps_rowmap;
/* XPS_FMT_SPLIT4: every aligned group of four consecutive fp32 elements (16 bytes, along the contiguous index) holds the
 * bf16 split of its values instead: bytes 0-7 = hi[0..3] = bf16(x[0..3]), bytes 8-15 = lo[0..3] = bf16(x[j] - hi[j]) -- exactly
 * what the bf16x3 tile kernels compute while they stage an fp32 operand.  A producer that owns the split anyway (the BPTT
 * kernels through xps_gru_seq_bwd_split4_f32, a dropout pass or a weight matrix through xps_split4_f32) writes it once; the GEMM entry points (nt / nn / nn2 / nt_multi /
 * tn_grouped, bf16x3 mode only) then stage the operand without any conversion arithmetic and return the SAME BITS as for
 * the fp32 operand (a bias gradient folded from a split4 A operand sums hi + lo: within 2^-17 relative of the fp32 sum).
 * Needs 16-byte aligned operands, leading dimensions and the contiguous extent multiples of 4; else XPS_E_INVALID. */
#define XPS_FMT_F32 0
#define XPS_FMT_SPLIT4 1

const char* xps_last_error(void);
int xps_abi_version(void);
/* a HIP stream at the lowest priority of the device (for work that must yield to the caller's main stream) */
int xps_stream_create_low_priority(void** stream);
int xps_stream_destroy(void* stream);
/* The library's switches (README.md, "Switches", lists the rows: name, default, values).  Every row starts at its default or at
 * what the environment variable of the same name says WHEN THE LIBRARY IS FIRST USED; the environment is not looked at
 * again, so a change inside a process goes through xps_set_switch (process-wide, not while launches of another thread are
 * in flight; a workspace is sized and used under the same values).  xps_set_switch: XPS_E_INVALID, with a message, for an
 * unknown name or a value outside the row's range.  xps_list_switches writes one "NAME=value" line per row into buf (n bytes;
 * XPS_E_INVALID if they do not fit; 1024 bytes do). */
int xps_set_switch(const char* name, long long value);
int xps_get_switch(const char* name, long long* value);
int xps_list_switches(char* buf, size_t n);
/* Product precision of the tiled GEMM entry points below (xps_gemm_*) and of the fused GRU recurrence (xps_gru_seq_*,
 * every H): 0 = fp32 MFMA, exact fp32 fma chains; 1 = bf16 split products (the default): every fp32 operand is split hi + lo in bf16 while it is staged and a product is
 * accumulated in fp32 as lo*hi + hi*lo + hi*hi on the bf16 matrix pipe (relative product error ~2^-16; results
 * stay inside the 1e-4 parity bar; BASELINE.json names bf16 for this path).  A view of the row XPS_GEMM_PRECISION
 * (environment: fp32 | bf16x3); returns XPS_E_INVALID for other modes. */
int xps_set_gemm_precision(int mode);
int xps_get_gemm_precision(void);
/* Tile shape of the matrix kernels in bf16x3 mode (a view of the row XPS_GEMM_BIG): 1 (default) lets large
 * interior shapes (M, N multiples of 256, k ranges multiples of 16, plain 16-byte aligned operands, >= 192 tiles) run on
 * 256 x 256 tiles / 8 waves; 0 keeps every product on the 128 x 128 (64 x 128) tiles.  Same arithmetic per k-tile in both:
 * products whose k range is not split (nt / nn / nn2 / nt_multi) have the same bits either way. */
int xps_set_gemm_big_tiles(int on);
int xps_get_gemm_big_tiles(void);

/* ------------------------------------------------------------------------- */
/* Dense fp32 contractions: bf16 split products (default) or the f32-input     */
/* MFMA with exact fp32 fma chains (xps_set_gemm_precision above).              */
/* Replaces the GEMMs inside torch.nn.Conv1d / nn.GRU / nn.Linear and their     */
/* autograd (nn_models/models.py:616,661,739,746).                               */
/* ------------------------------------------------------------------------- */

/* C[m][n] (+)= sum_k A[m][k] * B[n][k] + bias[n]      (A: M x K, B: N x K)   */
int xps_gemm_nt_f32(const float* A, const xps_rowmap* ra, const float* B, const xps_rowmap* rb,
                    float* C, const xps_rowmap* rc, const float* bias,
                    int M, int N, int K, int accumulate, void* stream);
/* C[m][n] (+)= sum_k A[m][k] * B[k][n]                (A: M x K, B: K x N)   */
int xps_gemm_nn_f32(const float* A, const xps_rowmap* ra, const float* B, const xps_rowmap* rb,
                    float* C, const xps_rowmap* rc,
                    int M, int N, int K, int accumulate, void* stream);
/* nprob (1..4) problems C_i = A B_i^T + bias_i sharing A and all sizes / row maps, in ONE launch (the input
 * projections of every direction of a GRU layer).  B, C, bias are HOST arrays of device pointers.       */
int xps_gemm_nt_multi_f32(const float* A, const xps_rowmap* ra, const float* const* B, const xps_rowmap* rb,
                          float* const* C, const xps_rowmap* rc, const float* const* bias, int nprob,
                          int M, int N, int K, void* stream);
/* C (+)= A1 B1 + A2 B2  (A_i: M x K_i, B_i: K_i x N, both pairs share the row maps): the input gradient of
 * a bidirectional layer, both directions summed in registers in one launch.    */
int xps_gemm_nn2_f32(const float* A1, const float* B1, int K1, const float* A2, const float* B2, int K2,
                     const xps_rowmap* ra, const xps_rowmap* rb, float* C, const xps_rowmap* rc,
                     int M, int N, int accumulate, void* stream);
/* C[m][n] (+)= sum_k A[k][m] * B[k][n]                (A: K x M, B: K x N)
 * split-K over deterministic partial slabs in `workspace`.                    */
size_t xps_gemm_tn_f32_workspace(int M, int N, int K);
int xps_gemm_tn_f32(const float* A, const xps_rowmap* ra, const float* B, const xps_rowmap* rb,
                    float* C, const xps_rowmap* rc,
                    int M, int N, int K, int accumulate,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Grouped form: up to 12 weight-gradient problems  C_p (+)= A_p^T B_p  in ONE launch (+ one
 * reduce launch).  colsum_a, when not NULL, receives  colsum_a[m] (+)= sum_k A_p[k][m]  (the bias
 * gradient) folded from the staged A tiles inside the same launch — no separate reduction pass.
 * `probs` is a HOST array; it is copied into the kernel arguments.                        */
typedef struct xps_tn_problem {
    const float* A; const float* B; float* C; float* colsum_a;
    xps_rowmap ra, rb, rc;
    int32_t M, N, K, accumulate;      /* bit 0: C and colsum_a accumulate; bit 1: colsum_a alone accumulates */
} xps_tn_problem;
size_t xps_gemm_tn_grouped_f32_workspace(const xps_tn_problem* probs, int n);
int xps_gemm_tn_grouped_f32(const xps_tn_problem* probs, int n, void* workspace, size_t workspace_bytes,
                            void* stream);

/* Which kernel a product runs: the one dispatch decision of nt / nn / nn2 / nt_multi as a query (host logic only: it follows
 * the switches and the device's CU count like the launches do, and calls the function the launches call).  `form` names the
 * entry point; the other arguments are the entry point's own.  Pointers are looked at for their alignment, never through --
 * except B of XPS_GEMM_FORM_NT_MULTI, the HOST array of nprob device pointers.  A2 / B2 / K2: nn2's second pair (its K1 is K),
 * ignored by the other forms; nprob: nt_multi only.
 * Returns the XPS_GEMM_ROUTE_* code of the leading launch.  *lead_rows: the rows it covers; where that is less than M (a
 * 256-tile launch keeps the whole rounds of tiles) *tail_route is the code of the launch that takes the rows behind them,
 * else XPS_GEMM_ROUTE_NONE.  Both out-parameters may be NULL.  REFUSED: the entry point returns XPS_E_INVALID (also returned
 * for arguments the entry point rejects); NONE: M or N is 0, nothing is launched.
 *   SMALL_M         gemm_small_kernel (M <= 16)
 *   SKINNY          nn / nn2: one 256-wide LDS-DMA tile per 256 rows, N < 256 (gemm_big_kernel<.., 5>)
 *   BIG + f         256 x 256 tiles, 16-deep register-staged loop; nt / nn / nn2: f = 0..3 (bit 0: A is XPS_FMT_SPLIT4, bit 1: B
 *                   is), one instantiation each; nt_multi: f = 0, one instantiation for all formats
 *   BIG_DEEP        256 x 256 tiles, 32-deep stages (XPS_GEMM_BIG_DEEP=1)
 *   BIG_DMA         256 x 256 tiles, LDS-DMA loop (both operands XPS_FMT_SPLIT4)
 *   TILE | flags    gemm_f32_kernel / gemm_nt_multi_kernel: _128 = 128-row tiles (else 64), _EDGE = masked edges, _BF = bf16x3
 *                   products (else fp32 MFMA), _PRE = an XPS_FMT_SPLIT4 operand (implies _BF)
 *   PROJ_WS + KT    nt_multi: weight-stationary projection kernel, KT = 2 ceil(K / 32) = 2, 4 .. 16 */
#define XPS_GEMM_FORM_NT 0
#define XPS_GEMM_FORM_NN 1
#define XPS_GEMM_FORM_NN2 2
#define XPS_GEMM_FORM_NT_MULTI 3
#define XPS_GEMM_ROUTE_REFUSED 0
#define XPS_GEMM_ROUTE_NONE 1
#define XPS_GEMM_ROUTE_SMALL_M 2
#define XPS_GEMM_ROUTE_SKINNY 3
#define XPS_GEMM_ROUTE_BIG 8
#define XPS_GEMM_ROUTE_BIG_DEEP 12
#define XPS_GEMM_ROUTE_BIG_DMA 13
#define XPS_GEMM_ROUTE_TILE 16
#define XPS_GEMM_ROUTE_TILE_128 1
#define XPS_GEMM_ROUTE_TILE_EDGE 2
#define XPS_GEMM_ROUTE_TILE_BF 4
#define XPS_GEMM_ROUTE_TILE_PRE 8
#define XPS_GEMM_ROUTE_PROJ_WS 32
int xps_gemm_route(int form, const float* A, const xps_rowmap* ra, const void* B, const xps_rowmap* rb, const float* A2,
                   const float* B2, const xps_rowmap* rc, int M, int N, int K, int K2, int nprob, int* lead_rows,
                   int* tail_route);
/* The plan xps_gemm_tn_grouped_f32 launches for a problem list (the function it calls; host logic only).  Per problem, into
 * arrays of n ints (each may be NULL): cls = XPS_GEMM_TN_CLASS_*, splits = its k-split count, kchunk = the k rows of a split.
 * Returns the group's XPS_GEMM_ROUTE_TN_* flags or-ed together, or XPS_E_INVALID where the launch refuses the list.
 *   _EDGE, _BF, _PRE  the gemm_tn_grouped_kernel<EDGE, BF, PRE> instantiation that serves the 128-tile problems (launched when
 *                     there is one): an edge tile / bf16x3 products / an XPS_FMT_SPLIT4 operand among them
 *   _DEEP             the 256-tile problems run gemm_big_tn_kernel<true> (32-deep stages), else <false> (launched when there is one)
 *   _UNIFORM          one common split count, blocks ordered by k-chunk first (XPS_TN_UNIFORM=1)
 *   _FLAT             gemm_tn_grouped_reduce_flat, else gemm_tn_grouped_reduce (XPS_TN_REDUCE) */
#define XPS_GEMM_TN_CLASS_128 0       /* 128 x 128 tiles */
#define XPS_GEMM_TN_CLASS_BIG 1       /* 256 x 256 tiles, register-staged loop */
#define XPS_GEMM_TN_CLASS_BIG_DMA 2   /* 256 x 256 tiles, LDS-DMA loop */
#define XPS_GEMM_ROUTE_TN_EDGE 1
#define XPS_GEMM_ROUTE_TN_BF 2
#define XPS_GEMM_ROUTE_TN_PRE 4
#define XPS_GEMM_ROUTE_TN_DEEP 8
#define XPS_GEMM_ROUTE_TN_UNIFORM 16
#define XPS_GEMM_ROUTE_TN_FLAT 32
int xps_gemm_tn_grouped_route(const xps_tn_problem* probs, int n, int* cls, int* splits, int* kchunk);

/* out[c] (+)= sum_r X[r][c] (and optionally sum_r X[r][c]^2 into out_sq), two-stage,
 * deterministic.  Bias gradients and BatchNorm batch statistics.               */
size_t xps_colsum_f32_workspace(int rows, int cols);
int xps_colsum_f32(const float* X, int64_t ldx, int rows, int cols, float* out, float* out_sq,
                   int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Fused GRU recurrence.  Replaces torch.nn.GRU's per-step cell                 */
/* (nn_models/models.py:661-663,687 encoder; :739-740,759 decoder).             */
/*                                                                             */
/* Layout (time-major, all directions in one call):                            */
/*   gi    [ndir][T][B][3H]  x_t W_ih^T + b_ih, gate order r,z,n (PyTorch)      */
/*   w_hh  [ndir] pointers to (3H x H) ; b_hh [ndir] pointers to (3H)           */
/*   h0    [ndir][B][H] or NULL (zeros)                                         */
/*   y_ext [T+2][B][ndir*H]  slot t+1 holds h_t of every direction in ACTUAL     */
/*          time; slot 0 / slot T+1 hold h0 of the forward / reverse direction;  */
/*          direction 1 runs t = T-1 .. 0                                       */
/*   saved ndir*T*B*4H floats: r, z, n, (W_hn h + b_hn) for the backward (or NULL).  OPAQUE: written by the forward entry point and
 *          read by the backward entry point of the same shape and mode only; [ndir][T][B][4H] on most paths, member-major
 *          ([ndir][T][H/32][B][4][32]) on the cluster path when H % 32 == 0 (sequential HBM streams per workgroup)            */
/* ------------------------------------------------------------------------- */
/* 256 < H <= 512 (H % 4 == 0, B >= 128): cluster-persistent recurrence (csrc/xps_gru_cluster.hip): W_hh stays in the registers
 * of a cluster of workgroups for the whole sequence, the members exchange h_t through `workspace` inside ONE launch.
 * xps_set_gru_cluster_mode / XPS_GRU_CLUSTER = off | steps | persistent (0 | 1 | 2, default 2): 1 runs the same kernels one
 * step per launch, 0 the per-step GEMM kernels.  A hand-off that timed out (3 s; e.g. two such launches of different processes
 * sharing one GPU) sets the 32-bit word at byte xps_gru_seq_status_offset() of the workspace to 1 (-1: the shape has no
 * status word); the caller checks it whenever it synchronises anyway.                                                    */
size_t xps_gru_seq_fwd_f32_workspace(int T, int B, int H, int ndir);
long long xps_gru_seq_status_offset(int T, int B, int H, int ndir);
/* A caller-owned, zero-initialised 32-bit DEVICE word for the current device (NULL: none) that outlives the workspaces: a
 * hand-off that timed out stores 1 there as well, so a trainer checks ONE word per device where it reads the loss instead of
 * keeping every launch's workspace alive.  The persistent form is only launched when the occupancy query says the device
 * holds the whole grid at once; otherwise (and always with mode 1) the same kernels run one step per launch.               */
int xps_gru_set_status_word(unsigned* device_word);
/* BPTT kernel of the cluster path in bf16x3 mode, 384 < H <= 512: 0 (default) = every member of a 16-workgroup cluster contracts
 * all 3H gate-gradient columns of its trials; 1 (XPS_GRU_CL2=1) = the members form a 4 x 4 grid, contract one K slice each and
 * exchange partial sums (a third of the LDS-DMA ingest, a second hand-off per step; same results up to summation order;
 * measured on a par: DESIGN.md 4.5).  A view of the row XPS_GRU_CL2; the workspace query follows the row.                   */
int xps_set_gru_bptt_grid(int two_dimensional);
int xps_get_gru_bptt_grid(void);
int xps_set_gru_cluster_mode(int mode);
int xps_get_gru_cluster_mode(void);
int xps_gru_seq_fwd_f32(const float* gi, const float* const* w_hh, const float* const* b_hh,
                        const float* h0, float* y_ext, float* saved,
                        int T, int B, int H, int ndir, void* workspace, size_t workspace_bytes, void* stream);

/* Backward through the recurrence (BPTT).
 *   dy     [T][B][ndir*H]   gradient w.r.t. the layer output (actual time), or NULL (all zero)
 *   dhn    [ndir][B][H]     gradient w.r.t. the FINAL hidden state of each direction (h at t = T-1 forward,
 *                           t = 0 reverse), or NULL; it seeds the running dh, so a layer whose per-step
 *                           output is unused downstream needs no dy buffer at all
 *   w_hh   [ndir] pointers to W_hh (3H x H) and  w_hh_t [ndir] pointers to W_hh^T (H x 3H, see
 *          xps_transpose_f32): H <= 128 keeps W_hh^T resident in registers for all steps; larger H runs one
 *          fused GEMM + gate-gradient launch per step on W_hh (workspace: xps_gru_seq_bwd_f32_workspace)
 *   dgi    [ndir][T][B][3H] gradient w.r.t. gi   (= w.r.t. input pre-activations r, z, n)
 *   dghn   [ndir][T][B][H]  n-gate part of the gradient w.r.t. (h_{t-1} W_hh^T + b_hh); its r and z
 *                           parts equal those of dgi, so they are not stored twice
 *   dh0    [ndir][B][H]     gradient w.r.t. h0 (or NULL)                       */
size_t xps_gru_seq_bwd_f32_workspace(int T, int B, int H, int ndir);
int xps_gru_seq_bwd_f32(const float* dy, const float* dhn, const float* y_ext, const float* saved,
                        const float* const* w_hh, const float* const* w_hh_t, float* dgi, float* dghn, float* dh0,
                        int T, int B, int H, int ndir, void* workspace, size_t workspace_bytes, void* stream);
/* Which kernels the two entry points above launch for a shape: the one dispatch decision both make, as a query (host logic
 * only; it follows xps_set_gru_cluster_mode, XPS_GRU_STEP_PATH and the device's CU count like the launches do).
 *   weights_aligned16  every W_hh pointer (forward) / every W_hh and W_hh^T pointer (backward) is 16-byte aligned.  A call
 *                      decides from the pointers it streams: W_hh in the forward and in the per-step backward, W_hh^T in the
 *                      backward of the other routes; `saved` has one layout on all routes but the cluster's, so a forward and
 *                      a backward that land on different kernels of those routes still belong together.
 *   backward           0: xps_gru_seq_fwd_f32, 1: xps_gru_seq_bwd_f32
 * The answer assumes 16-byte aligned activation buffers (y_ext, dgi, dghn; the resident, generic-vector and cluster kernels
 * require them; the per-step kernels drop VECA for a buffer that is not).
 * Envelope.  XPS_GRU_ROUTE_REFUSED: both entry points return XPS_E_INVALID and write nothing.  The routes that keep a state /
 * gradient tile in LDS (RESIDENT, GENERIC_*) stop at H = XPS_GRU_MAX_H_TILE in BOTH directions: the backward's tile, 16 trials
 * x (4 Hp + 8) floats with Hp = H rounded up to 16, must fit 160 KiB.  They serve H <= 128, and larger H only with
 * XPS_GRU_STEP_PATH=0.  The per-step kernels hold no tile; they stop at H = XPS_GRU_MAX_H_STEP in both directions, the largest
 * H the forward has ever accepted and the largest the tests launch.  The cluster kernels serve 256 < H <= 512. */
#define XPS_GRU_MAX_H_TILE 624
#define XPS_GRU_MAX_H_STEP 1264
#define XPS_GRU_ROUTE_REFUSED 0
#define XPS_GRU_ROUTE_CLUSTER 1          /* csrc/xps_gru_cluster.hip, persistent or one step per launch */
#define XPS_GRU_ROUTE_RESIDENT 2         /* H = 64 / 128, W_hh in registers */
#define XPS_GRU_ROUTE_GENERIC_VEC 3      /* LDS-tile kernel, 16-byte weight loads */
#define XPS_GRU_ROUTE_GENERIC_SCALAR 4   /* LDS-tile kernel, scalar weight loads (H % 4 != 0 or misaligned weights) */
#define XPS_GRU_ROUTE_STEP 8             /* one launch per step; or-ed with the two flags below: 8 .. 11 */
#define XPS_GRU_ROUTE_STEP_VECA 1        /* 16-byte loads of the activation operand (H % 4 == 0) */
#define XPS_GRU_ROUTE_STEP_VECB 2        /* 16-byte loads of W_hh (H % 4 == 0 and aligned weights) */
int xps_gru_seq_route(int T, int B, int H, int ndir, int weights_aligned16, int backward);
/* Inter-layer dropout of a multi-layer GRU (torch.nn.GRU(dropout=p): nn_models/models.py:661-663, applied to the outputs of
 * every layer but the last) fused into the recurrence kernels of the register-resident shapes (H = 64 / 128;
 * xps_gru_seq_fused_dropout_supported says which): the forward kernel also writes y_drop (T x B x ndir*H) = y * keep / (1 - p)
 * with keep = the decisions xps_dropout_f32(seed) makes for the same flat index, the backward kernel takes dy as the gradient
 * w.r.t. y_drop and applies the same decisions while it loads it.  Same bits as the separate xps_dropout_f32 passes. */
int xps_gru_seq_fused_dropout_supported(int T, int B, int H, int ndir);
int xps_gru_seq_fwd_drop_f32(const float* gi, const float* const* w_hh, const float* const* b_hh,
                             const float* h0, float* y_ext, float* saved,
                             int T, int B, int H, int ndir, float* y_drop, float drop_p, uint64_t drop_seed,
                             void* workspace, size_t workspace_bytes, void* stream);
int xps_gru_seq_bwd_drop_f32(const float* dy, const float* dhn, const float* y_ext, const float* saved,
                             const float* const* w_hh, const float* const* w_hh_t, float* dgi, float* dghn, float* dh0,
                             int T, int B, int H, int ndir, float drop_p, uint64_t drop_seed,
                             void* workspace, size_t workspace_bytes, void* stream);
/* xps_gru_seq_fwd_f32 that ALSO writes XPS_FMT_SPLIT4 images (see xps_rowmap) of its outputs, from the epilogue that holds the
 * values (cluster-persistent shapes, 256 < H <= 512, bf16x3 mode: xps_gru_seq_fwd_images_supported): y_split (T + 2, B, ndir*H):
 * the image of y_ext, slot for slot -- h_prev of the dW_hh products; y_drop_split (T, B, ndir*H): the image of
 * dropout(y, drop_p, drop_seed) (drop_p = 0: of y) -- the input of the next layer's projection and dW_ih.  Either may be NULL.
 * Same bits as xps_split4_f32 over the finished tensors (one pass each over 168 MB at configs[3]'s shape, which this replaces).
 * Reference: the layer stack of nn_models/models.py:661-699 (torch.nn.GRU(dropout=p)). */
int xps_gru_seq_fwd_images_supported(int T, int B, int H, int ndir);
/* 1: for this shape the launch uses y_split as its in-kernel exchange buffer (H = 512, batch without pad trials): the image then
 * REPLACES the ring buffer's stores (one store per lane and round fewer) instead of adding one; callers ask for y_split by default
 * only where this holds. */
int xps_gru_seq_fwd_image_exchange_supported(int T, int B, int H, int ndir);
int xps_gru_seq_fwd_images_f32(const float* gi, const float* const* w_hh, const float* const* b_hh,
                               const float* h0, float* y_ext, float* saved, int T, int B, int H, int ndir,
                               float* y_split, float* y_drop_split, float drop_p, uint64_t drop_seed,
                               void* workspace, size_t workspace_bytes, void* stream);
/* The same backward with dgi / dghn written as XPS_FMT_SPLIT4 groups (see xps_rowmap): their only readers are GEMMs (weight
 * gradients, the layer's input gradient), and the BPTT kernels hold the bf16 hi / lo split of every gate gradient anyway.
 * bf16x3 mode; cluster-persistent shapes (256 < H <= 512) and the register-resident ones (H = 64 / 128):
 * xps_gru_seq_bwd_split4_supported.  drop_p > 0: the fused inter-layer dropout of xps_gru_seq_bwd_drop_f32 (resident shapes). */
int xps_gru_seq_bwd_split4_supported(int T, int B, int H, int ndir);
int xps_gru_seq_bwd_split4_f32(const float* dy, const float* dhn, const float* y_ext, const float* saved,
                               const float* const* w_hh, const float* const* w_hh_t, float* dgi, float* dghn, float* dh0,
                               int T, int B, int H, int ndir, float drop_p, uint64_t drop_seed,
                               void* workspace, size_t workspace_bytes, void* stream);

int xps_transpose_f32(const float* src, float* dst, int rows, int cols, void* stream);
/* 1..4 equally shaped matrices in one launch (host arrays of device pointers): both directions' W_hh^T */
int xps_transpose_batched_f32(const float* const* src, float* const* dst, int n, int rows, int cols, void* stream);

/* ------------------------------------------------------------------------- */
/* TemporalConv = Conv1d -> BatchNorm1d -> [ReLU] -> Dropout                    */
/* (nn_models/models.py:599-636).  The convolution itself is xps_gemm_nt_f32     */
/* over window rows; these are the fused normalisation passes.                   */
/*   y, out : [rows][F]  rows = T' * B                                           */
/*   stats  : [2F] stats[0:F] = sum of y over rows (xps_colsum_f32), then      */
/*            stats[F:2F] = sum of (y - mf)^2, mf = float(stats[c] / count)       */
/*            (xps_bn_centered_sumsq_f32); under data parallelism (SyncBN) the    */
/*            caller all-reduces each half by sum before the next step;          */
/*            count = global number of rows                                      */
/* ------------------------------------------------------------------------- */
/* second statistics pass: out_sq[c] = sum_r (y[r][c] - mf[c])^2, workspace of xps_colsum_f32_workspace(rows, F) */
int xps_bn_centered_sumsq_f32(const float* y, int rows, int F, const float* stats, double count, float* out_sq,
                              void* workspace, size_t workspace_bytes, void* stream);
/* num_batches_tracked: device int64 counter (BatchNorm1d buffer) incremented by one, or NULL */
int xps_bn_finalize_f32(const float* stats, double count, float* mean, float* rstd,
                        float* running_mean, float* running_var, int64_t* num_batches_tracked,
                        float momentum, float eps, int F, void* stream);
int xps_bn_apply_f32(const float* y, const float* mean, const float* rstd,
                     const float* gamma, const float* beta, const float* drop_mask, float drop_scale,
                     float* out, int64_t rows, int F, int relu, void* stream);
/* eval mode: running statistics */
/* xps_bn_finalize_f32 + xps_bn_apply_f32 in one launch (same values bit for bit; F <= 8192) */
int xps_bn_finalize_apply_f32(const float* y, const float* stats, double count, const float* gamma, const float* beta,
                              float* mean, float* rstd, float* running_mean, float* running_var,
                              int64_t* num_batches_tracked, float momentum, float eps, const float* drop_mask,
                              float drop_scale, float* out, int64_t rows, int F, int relu, void* stream);
int xps_bn_apply_eval_f32(const float* y, const float* running_mean, const float* running_var, float eps,
                          const float* gamma, const float* beta, float* out,
                          int64_t rows, int F, int relu, void* stream);
/* backward: pass 1 = g = dout * mask * relu'(out); sums[0:F] = sum g, sums[F:2F] = sum g*xhat
 *           (caller all-reduces sums under DP); dbeta_acc / dgamma_acc (optional, [F]): the LOCAL sums are
 *           also added into them (parameter gradients straight into their buffers); pass 2 = dy */
size_t xps_bn_bwd_workspace(int64_t rows, int F);
int xps_bn_bwd_reduce_f32(const float* dout, const float* out, const float* y, const float* mean,
                          const float* rstd, const float* drop_mask, float drop_scale, int relu,
                          float* sums, float* dbeta_acc, float* dgamma_acc, int64_t rows, int F,
                          void* workspace, size_t workspace_bytes, void* stream);
int xps_bn_bwd_apply_f32(const float* dout, const float* out, const float* y, const float* mean,
                         const float* rstd, const float* gamma, const float* drop_mask,
                         float drop_scale, int relu, const float* sums, double count,
                         float* dy, int64_t rows, int F, void* stream);

/* ------------------------------------------------------------------------- */
/* Decoder glue (nn_models/models.py:285-299,758-761)                           */
/* ------------------------------------------------------------------------- */
/* Fused autoregressive decoder: all L decode steps of a ONE-layer GRU decoder in one launch
 * (input-projection gather by token -> GRU cell, W_hh resident in registers -> Linear -> next token =
 * teacher token if flags[s] else first-max argmax).  Supported: H in {64, 128}, C <= 16, L <= 8
 * (xps_decoder_supported); other shapes use the composed entry points.
 *   table  [ntok][3H]  E W_ih^T + b_ih        teacher [B][L] (or NULL)   flags [L] DEVICE int32 (or NULL)
 *   logits [B][L][C]   tokens [L][B] input token of every step
 *   hs     [L+1][B][H] hidden state before step s (slot s) / after it (slot s+1)
 *   saved  [L][B][4H]  r, z, n, (W_hn h + b_hn)  (NULL in eval)
 * backward: dlogits [B][L][C] -> dgi [L][B][3H], dghn [L][B][H], dh0 [B][H]; weight gradients follow
 * from xps_gemm_tn_grouped_f32 / xps_scatter_rows_f32 over those buffers.                          */
int xps_decoder_supported(int H, int C, int L);
int xps_decoder_fwd_f32(const float* table, const float* w_hh, const float* b_hh, const float* h0,
                        const float* w_fc, const float* b_fc, const int64_t* teacher, const int32_t* flags,
                        float* logits, int64_t* tokens, float* hs, float* saved,
                        int B, int H, int C, int L, int ntok, int start_token, void* stream);
int xps_decoder_bwd_f32(const float* dlogits, const float* hs, const float* saved, const float* w_hh_t,
                        const float* w_fc, float* dgi, float* dghn, float* dh0,
                        int B, int H, int C, int L, void* stream);

/* Streaming (batch-1 .. 8 streams) inference for the realtime decoder (realtime_sim/realtime_nn_model.py
 * :153-170, one window per call): weight-streaming GEMV kernels, one wave per output row.
 *   x, h_prev, h_new, out are [S][.] with S = 1, 2, 4 or 8 rows ALLOCATED (S = B rounded up to a power
 *   of two); only the first B rows are written.  h_new must not alias h_prev.  The rows B .. S-1 of
 *   x and h_prev are read (any values, NaN included) and reach no live row.  A stream's output bits
 *   depend on its own input row alone: not on the row it occupies, not on B.  x and W (x and w_ih,
 *   h_prev and w_hh) must be 16-byte aligned when K (H) is a multiple of 4; otherwise any float
 *   alignment is taken.                                                                            */
int xps_gemv_f32(const float* x, const float* W, const float* bias, float* out, int N, int K, int B,
                 void* stream);
int xps_gru_cell_gemv_f32(const float* x, int K, const float* w_ih, const float* w_hh, const float* b_ih,
                          const float* b_hh, const float* h_prev, float* h_new, int H, int B, void* stream);

/* Realtime pipeline glue (realtime_sim/realtime_pipeline.py): the window of a stream is win frames of d floats, one
 * contiguous row of win*d; rows [S][win*d] as above.
 * xps_window_shift_f32: dst[s] = src[s] shifted left by k frames (1 <= k <= win), followed by the k new frames
 *   float32(power[s][j] @ W[s] + c[s]) (power [B][k][C] float64, W [B][C][d] float64, c [B][d] float64 or NULL;
 *   W == NULL: identity, d == C).  dst must not alias src (ping-pong pair).
 * xps_ctc_collapse_f32: online greedy CTC collapse of one step.  argmax[b] = first maximum of logits[b] (torch.argmax);
 *   state [B][3] int32 = {previous argmax (-1 before the first step), token count, overflow flag}; the argmax is
 *   appended to tokens[b][0 .. max_tokens) when it differs from the previous one and is not `blank`, and the overflow flag
 *   is set (sticky) instead when the row is full.  Counts and flags are the caller's to reset.                     */
int xps_window_shift_f32(const double* power, int k, int C, const double* W, const double* c, const float* src,
                         float* dst, int win, int d, int B, void* stream);
int xps_ctc_collapse_f32(const float* logits, int n_classes, int blank, int64_t* argmax, int32_t* state,
                         int64_t* tokens, int max_tokens, int B, void* stream);

/* CTC prefix beam search (realtime_sim/ctc_decoder.py), fp64, the reference decode's result and tie order.
 * Sizes: 1 <= beam_size <= 128, 1 <= n_classes <= 64, beam_size * n_classes <= 8192, 0 <= blank < n_classes; else
 * XPS_E_INVALID before any launch.
 * ..._f64: the offline batch, one launch, one workgroup per sequence.  log_probs [B][T][n_classes] float32
 *   (is_f32 = 1) or float64, input_lengths [B] int64 (NULL: all T; clamped to 0..T); from_logits = 1 applies a row-wise fp64 log-softmax first.
 *   prefix [B][T] int64 gets the best prefix of each sequence (-1 after its end), prefix_len [B] int64 its length,
 *   nll [B] float64 its -logsumexp(p_b, p_nb).  Workspace: ..._workspace bytes (backpointers).
 * ..._step_f32: the streaming form.  Advances the beam of each of B (1..8) streams by one frame of float32
 *   logits [B][n_classes] (always from_logits).  state: ..._state_bytes(B, beam_size, max_steps) bytes, one
 *   block per stream starting with int32 {step, n_members, overflow, 0}; all zero = the empty beam (the caller's reset).
 *   A step with step == max_steps sets the sticky overflow flag and leaves the beam as it is.  Graph-capturable.
 *   Layout of one stream block (tests/ctc_beam_state.py decodes it):
 *     header, 64 bytes: int32 {step, n_members, overflow, 0};
 *     member set, beam_size * 68 bytes rounded up to a multiple of 64, K = beam_size: double p_b[K], p_nb[K];
 *       uint64 h1[K], h2[K] (hashes of the prefix), hp1[K], hp2[K] (of the prefix without its last token), cmask[K]
 *       (bit t: prefix + (t,) is a member); int32 len[K], last[K] (-1 for the empty prefix), parent[K] (the rank of the
 *       prefix without its last token, or -1).  Ranks >= n_members and the padding are unspecified;
 *     backpointers: int32 hist[max_steps][K], hist[t][r] = rank in the previous frame | (appended token + 1) << 16 for
 *       the member of rank r after frame t; ranks >= that frame's member count and frames >= step are not written;
 *     the block's stride is rounded up to a multiple of 256 bytes.
 * ..._readout: stream s's best prefix so far into prefix [max_steps] int64, its length and nll (one each). */
size_t xps_ctc_beam_workspace(int B, int T, int beam_size, int n_classes);
int xps_ctc_beam_f64(const void* log_probs, int is_f32, int B, int T, int n_classes, const int64_t* input_lengths,
                     int blank, int beam_size, int from_logits, int64_t* prefix, int64_t* prefix_len, double* nll,
                     void* workspace, size_t workspace_bytes, void* stream);
size_t xps_ctc_beam_state_bytes(int n_streams, int beam_size, int max_steps);
int xps_ctc_beam_step_f32(const float* logits, int n_classes, int blank, int beam_size, int max_steps, void* state,
                          size_t state_bytes, int B, void* stream);
int xps_ctc_beam_readout(const void* state, size_t state_bytes, int B, int beam_size, int max_steps, int s,
                         int64_t* prefix, int64_t* prefix_len, double* nll, void* stream);

/* CTC forced alignment (realtime_sim/ctc_align.py): the Viterbi best path of a KNOWN target through the
 * frame scores, one launch for the batch, one 64-lane workgroup per sequence, no host synchronisation.
 * scores: float32 (is_f32 = 1) or float64, any per-frame scores (no softmax is applied: with log-probabilities the path
 *   score is the path's log-probability); frame t of sequence b starts at element t * stride_t + b * stride_b, its C
 *   classes are contiguous -- (T, B, C) and (B, T, C) tensors and permuted views of them are read in place.
 * targets [B][target_stride] int64, max_target_len = Lmax <= target_stride; input_lengths / target_lengths [B] int64, NULL:
 *   all T / all Lmax.  Lengths are clamped to 0..T / 0..Lmax and labels to 0..C-1 for memory safety only.
 * Recursion, float64 additions and comparisons only.  Tb and L the lengths of a sequence, extended label
 *   l' = (blank, l_1, blank, ..., l_L, blank), S = 2 L + 1 states, x_t(c) the score widened to float64:
 *     v_0(0) = x_0(blank), v_0(1) = x_0(l_1), every other state -inf;
 *     v_t(s) = x_t(l'_s) + max(v_{t-1}(s), v_{t-1}(s-1), [s odd, s >= 3 and l'_s != l'_{s-2}] v_{t-1}(s-2)).
 * TIE RULE (part of the contract): among the predecessors the first of (stay, s-1, s-2) that attains the maximum wins, so
 *   a move needs a strictly larger value; the path ends in state S-1 unless v_{Tb-1}(S-2) is strictly larger.
 * Outputs: states [B][T] int32, the extended-state index of each frame, -1 from frame Tb on; token_start / token_end
 *   [B][Lmax] int32, the first frame and one past the last frame spent in state 2 j + 1, -1 for j >= L; path_score [B]
 *   float64 = v_{Tb-1}(end state).  A path score of -inf is INFEASIBLE (fewer frames than L + the number of adjacent equal
 *   labels, or every path crosses a -inf score): all states and spans -1.  Tb = 0: score 0 for L = 0, else infeasible.
 *   L = 0: the all-blank path.  NaN or +inf scores: an unspecified path, no out-of-range access.
 * Workspace: ..._workspace bytes, one backpointer byte per (b, t, s) at (b * T + t) * (2 Lmax + 1) + s; only 1 <= t < Tb,
 *   s < S are written.
 * XPS_E_INVALID before any launch: a negative size or stride, C < 1, blank outside 0..C-1, 2 Lmax + 1 > 1023 (the CTC
 *   loss's state cap), target_stride < Lmax, a NULL pointer that the sizes need, a workspace smaller than ..._workspace. */
size_t xps_ctc_align_workspace(int B, int T, int max_target_len);
int xps_ctc_align(const void* scores, int is_f32, int64_t stride_t, int64_t stride_b, int T, int B, int C,
                  int max_target_len, const int64_t* targets, int64_t target_stride, const int64_t* input_lengths,
                  const int64_t* target_lengths, int blank, int32_t* states, int32_t* token_start, int32_t* token_end,
                  double* path_score, void* workspace, size_t workspace_bytes, void* stream);

/* CTC posterior occupancies (realtime_sim/ctc_occupancy.py): the forward-backward posteriors of a KNOWN
 * target, i.e. how much of the probability mass has token j emitted at, or started at, frame t.  One launch for the batch,
 * one workgroup per sequence (64 .. 256 lanes, by the states of the longest target), no host synchronisation.
 * Inputs: exactly xps_ctc_align's, with the same meaning (scores float32 widened exactly, or float64, read in place through
 *   (stride_t, stride_b) with contiguous classes; lengths clamped to 0..T / 0..Lmax and labels to 0..C-1 for memory safety
 *   only; padding is never read).  No softmax is applied: a per-frame constant shifts every path alike, so the posteriors
 *   are the same for logits and their log-softmax and log_z moves by the sum of the constants; with log-probabilities
 *   log_z = -nll.
 * Recursion, float64, log domain.  l' = (blank, l_1, blank, ..., l_L, blank), S = 2 L + 1, x_t(c) the widened score,
 *   [skip s] = s odd, s >= 3 and l'_s != l'_{s-2}; a state index outside 0..S-1 reads as -inf:
 *     a_0(0) = x_0(blank), a_0(1) = x_0(l_1), else -inf
 *     a_t(s) = x_t(l'_s) + lse(a_{t-1}(s), a_{t-1}(s-1), [skip s] a_{t-1}(s-2))
 *     b_{Tb-1}(S-1) = x(l'_{S-1}), b_{Tb-1}(S-2) = x(l'_{S-2}), else -inf
 *     b_t(s) = x_t(l'_s) + lse(b_{t+1}(s), b_{t+1}(s+1), [skip s+2] b_{t+1}(s+2))
 *     log_z  = lse(a_{Tb-1}(S-1), a_{Tb-1}(S-2))
 *     g_t(s) = exp(((a_t(s) + b_t(s)) - x_t(l'_s)) - log_z), 0 where a_t(s) or b_t(s) is -inf
 *     onset_0(j) = g_0(2j+1)
 *     onset_t(j) = exp((lse(a_{t-1}(2j), [skip 2j+1] a_{t-1}(2j-1)) + b_t(2j+1)) - log_z), 0 where the lse or b is -inf
 *   ORDER.  lse(p1, p2, p3) = log((exp(p1 - m) + exp(p2 - m)) + exp(p3 - m)) + m with m = max(p1, max(p2, p3)), the terms in
 *   the order written above, an absent term -inf (it adds an exact 0), and -inf when m is -inf.  class_occ sums g_t(s) over
 *   the states of a class by increasing s (the blank column: the even states).  expected_frames and onset_mean add their
 *   frames from t = Tb - 1 down to 0, onset_mean's term the rounded product (double)t * onset_t(j).  No floating-point
 *   atomics: two launches give the same bytes, and a sequence's results do not depend on the rest of the batch.
 * Outputs, float64; log_z is always written, each of the others may be NULL and is then skipped; every element of a
 *   non-NULL output is written.  log_z [B].  token_occ [B][T][Lmax] = g_t(2j+1).  onset [B][T][Lmax].  class_occ [B][T][C]:
 *   rows t < Tb sum to 1.  expected_frames [B][Lmax] = sum_t g_t(2j+1).  onset_mean [B][Lmax] = sum_t t onset_t(j).
 *   Frames t >= Tb and tokens j >= L are 0 in the three tensors; expected_frames is 0 and onset_mean NaN for j >= L.
 *   log_z = -inf is INFEASIBLE: every posterior 0, expected_frames 0, onset_mean NaN.  Tb = 0: log_z 0 for L = 0, else
 *   infeasible.  NaN or +inf scores: unspecified values, no out-of-range access.
 * Workspace: ..._workspace bytes, 8-byte aligned: a_t(s) as one double per (b, t, s) at (b * T + t) * (2 Lmax + 1) + s; only
 *   t < Tb, s < S are written.
 * LDS: 80 Lmax + 96 bytes (two rows of a / b with -inf guard cells, g, the two moment rows, the labels and the per-class
 *   chains), plus 8 C for the class bins when class_occ is given; the kernel's budget is 65536 bytes, so class_occ takes
 *   C <= 3070 at Lmax = 511 and C <= 8180 at Lmax = 0.
 * XPS_E_INVALID before any launch: everything xps_ctc_align refuses (a negative size or stride, C < 1, blank outside
 *   0..C-1, Lmax > 511, target_stride < Lmax, a NULL pointer that the sizes need, a workspace smaller than ..._workspace), an
 *   output or workspace that is not 8-byte aligned, and class bins that do not fit the LDS budget. */
size_t xps_ctc_occupancy_workspace(int B, int T, int max_target_len);
int xps_ctc_occupancy(const void* scores, int is_f32, int64_t stride_t, int64_t stride_b, int T, int B, int C,
                      int max_target_len, const int64_t* targets, int64_t target_stride, const int64_t* input_lengths,
                      const int64_t* target_lengths, int blank, double* log_z, double* token_occ, double* onset,
                      double* class_occ, double* expected_frames, double* onset_mean, void* workspace,
                      size_t workspace_bytes, void* stream);

/* out[b][:] = table[idx[b]][:]  (embedding / precomputed input projection rows) */
int xps_gather_rows_f32(const float* table, const int64_t* idx, float* out,
                        int B, int cols, int n_rows, void* stream);
/* dtable[r][:] (+)= sum_{b: idx[b]==r} dout[b][:]  (deterministic two-stage; n_rows <= 64) */
size_t xps_scatter_rows_f32_workspace(int B, int cols, int n_rows);
int xps_scatter_rows_f32(const float* dout, const int64_t* idx, float* dtable,
                         int B, int cols, int n_rows, int accumulate,
                         void* workspace, size_t workspace_bytes, void* stream);
/* next[b] = use_teacher[0] ? teacher[b*teacher_stride] : argmax_c logits[b][c]
 * (first maximal index, as torch.argmax); use_teacher is a DEVICE flag so the
 * decode loop has no host synchronisation.                                     */
int xps_next_token(const float* logits, int n_classes, const int64_t* teacher, int64_t teacher_stride,
                   const int32_t* use_teacher, int64_t* next, int B, void* stream);
/* Decode-step glue of a one-layer GRU decoder whose recurrence runs on the general GRU entry points (nn_models/models.py:
 * 285-301, 749-757): logits (B x C, C <= 16) = h W_fc^T + b_fc, next[b] = teacher token (device flag set) or the first
 * maximum of the logits, gi_next[b] = table[next[b]] (the token's row of the input-projection table, 3H floats) in one
 * launch.  next / gi_next may be NULL (last step: logits only). */
int xps_decoder_select_f32(const float* h, const float* w_fc, const float* b_fc, float* logits,
                           const int64_t* teacher, int64_t teacher_stride, const int32_t* use_teacher,
                           const float* table, int64_t* next, float* gi_next, int B, int H, int C, int ntok, void* stream);
/* Inverted dropout with a counter-based generator (no mask round trip through torch's RNG kernels):
 * mask[i] = (u_i >= p) in {0,1}, u_i a function of (seed, i) only;  if x != NULL also
 * out[i] = x[i] * mask[i] / (1 - p) in the same pass.  mask may be NULL when x is given: the backward pass then
 * regenerates the decisions by the same call on the incoming gradient (same seed), no mask tensor exists;
 * with a stored mask the backward is xps_mask_scale_f32.                                                 */
int xps_dropout_f32(const float* x, float* out, float* mask, int64_t n, float p, uint64_t seed, void* stream);
/* out = the XPS_FMT_SPLIT4 image (see xps_rowmap) of dropout(x) -- drop_p = 0: of x itself; else the values xps_dropout_f32(x,
 * seed) would write, decisions regenerated in the backward by xps_dropout_f32 on the gradient as before.  For tensors that only
 * GEMMs read (a layer input that exists only as the dropped output of the previous layer, weights once per forward pass):
 * the tile kernels then stage them without conversion arithmetic.  n % 4 == 0, 16-byte aligned buffers. */
int xps_split4_f32(const float* x, float* out, int64_t n, float drop_p, uint64_t seed, void* stream);
/* XPS_FMT_SPLIT4 image of a rows x cols fp32 matrix (leading dimension ldx) written with leading dimension ldo >= cols and ZERO
 * beyond column cols: a [k][n] GEMM operand whose rows are readable to a full 256-column tile (the skinny input-gradient product
 * of a layer with few input channels -- configs[3] layer 0: dx = dgi W_ih with In = 100 -- takes the LDS-DMA loop that way) */
int xps_split4_pad_f32(const float* x, int64_t ldx, int rows, int cols, float* out, int64_t ldo, void* stream);
/* out = x * mask * scale */
int xps_mask_scale_f32(const float* x, const float* mask, float scale, float* out, int64_t n, void* stream);
/* out = a + b (elementwise) */
int xps_add_f32(const float* a, const float* b, float* out, int64_t n, void* stream);

/* ------------------------------------------------------------------------- */
/* Loss and optimiser (nn_models/models.py:318-320 CrossEntropyLoss;            */
/* :373-389 AdamW; scripts/train_seq2seq.py:178 gradient_clip_val=0.5)           */
/* ------------------------------------------------------------------------- */
/* mean cross-entropy over `rows` rows of `n_classes` logits; row_loss [rows] scratch */
int xps_cross_entropy_fwd_f32(const float* logits, const int64_t* target, float* row_loss,
                              float* loss, int64_t rows, int n_classes, void* stream);
int xps_cross_entropy_bwd_f32(const float* logits, const int64_t* target, const float* gout,
                              float* dlogits, int64_t rows, int n_classes, void* stream);
/* Loss and UNIT gradient d(mean loss)/d(logits) in one launch (dlogits may be NULL: loss only).  `workspace`
 * (xps_cross_entropy_loss_grad_f32_workspace bytes, 8-byte aligned) holds a ticket word (its first word) and per-block partial sums; the ticket must
 * be ZERO at the first call and is left zero by every call: one zero-initialised buffer per stream serves all calls.            */
size_t xps_cross_entropy_loss_grad_f32_workspace(int64_t rows);
int xps_cross_entropy_loss_grad_f32(const float* logits, const int64_t* target, float* row_loss, float* loss,
                                    float* dlogits, void* workspace, size_t workspace_bytes, int64_t rows,
                                    int n_classes, void* stream);
/* The classification step of the single-label classifiers (nn_models/models.py:34-86 of the reference: criterion + cmat_acc)
 * in ONE launch: loss / row_loss / dlogits exactly as xps_cross_entropy_loss_grad_f32 (same row routine, same fixed-order
 * reduction: bit-identical; dlogits may be NULL: evaluation, no gradient is written); cmat [n_classes][n_classes] int64 =
 * confusion matrix, rows the true class, columns argmax(logits) (first maximum wins, a NaN counts as the maximum), zeroed and
 * filled by the launch itself; acc[0] = trace(cmat) / rows as fp32.  Targets outside [0, n_classes) are not counted in cmat.
 * `workspace` as for xps_cross_entropy_loss_grad_f32, same size and layout (ticket in its first word, zero at the first call,
 * left zero; one zero-initialised buffer may serve both entry points).                                                    */
size_t xps_classify_loss_acc_f32_workspace(int64_t rows);
int xps_classify_loss_acc_f32(const float* logits, const int64_t* target, float* row_loss, float* loss, float* dlogits,
                              int64_t* cmat, float* acc, void* workspace, size_t workspace_bytes, int64_t rows,
                              int n_classes, void* stream);
/* Max over time of a TIME-major tensor z [T][B][F] (TCN_classifier, nn_models/models.py:444 of the reference: torch.max over
 * the time axis): out [B][F] = the maximum, arg [B][F] int32 = its time index.  Among equal maxima the first index wins; a
 * NaN counts as the maximum and the first NaN wins (torch.max on the CPU).  out is a selection: bit-exact.
 * 16-byte accesses where F % 4 == 0 and the pointers are 16-byte aligned, 4-byte accesses otherwise.                        */
int xps_time_max_fwd_f32(const float* z, float* out, int* arg, int T, int B, int F, void* stream);
/* dz [T][B][F]: dz[t][b][f] = dout[b][f] where t == arg[b][f], else 0.  EVERY element of dz is written (no memset needed). */
int xps_time_max_bwd_f32(const float* dout, const int* arg, float* dz, int T, int B, int F, void* stream);

/* ------------------------------------------------------------------------- */
/* Transformer encoder layer (nn_models/models.py:451-597 of the reference:     */
/* nn.TransformerEncoderLayer, post-norm, ReLU, batch_first) -- DESIGN.md 4.13   */
/* ------------------------------------------------------------------------- */
/* Fused multi-head self-attention on TIME-major rows.  qkv [S*B][3 D], D = n_head * dh: row (s, b) = s * B + b holds q | k | v
 * (the packed in-projection output), head h at columns h * dh of each.  Per (trial b, head h):
 *   scores = (q / sqrt(dh)) k^T, P = softmax over keys (row maximum subtracted), Pd = P * keep / (1 - p), ctx = Pd v.
 * ctx [S*B][D] head-concatenated; lse [B][n_head][S] = row maximum + log of the row's sum of exponentials (what the backward
 * needs to rebuild P).  fp32 throughout; the S x S probabilities exist in registers only; keys stream through LDS in tiles (64
 * keys, 32 where dh > 64), so S is not bounded by LDS.  keep = the decision xps_dropout_f32(seed) makes for flat index
 * ((b * n_head + h) * S + query) * S + key  (p = 0: no dropout, seed ignored).  Envelope (xps_attention_supported): B, S,
 * n_head >= 1, 1 <= dh <= 128. */
int xps_attention_supported(int B, int S, int n_head, int dh);
int xps_attention_fwd_f32(const float* qkv, float* ctx, float* lse, int B, int S, int n_head, int dh, float p, uint64_t seed,
                          void* stream);
/* dqkv [S*B][3 D] (EVERY element written) from dctx: P is recomputed from q, k and lse, the dropout decisions from the seed.
 * Two launches: per query (dq, and delta = dctx . ctx into the workspace), then per key (dk, dv: each a sum over the queries in
 * index order inside one thread).  No atomics: the same bits every run. */
size_t xps_attention_bwd_f32_workspace(int B, int S, int n_head, int dh);
int xps_attention_bwd_f32(const float* dctx, const float* qkv, const float* ctx, const float* lse, float* dqkv, int B, int S,
                          int n_head, int dh, float p, uint64_t seed, void* workspace, size_t workspace_bytes, void* stream);
/* y = LayerNorm(x + dropout(r)) * gamma + beta over rows of D <= 1024 elements (biased variance, nn.LayerNorm); dropout(r) =
 * r * keep / (1 - p) with xps_dropout_f32(seed)'s decisions at flat index row * D + column (p = 0: none).  One wave per row; the
 * row is held in LDS as differences from its first element and the statistics are two passes over it (mean, then the sum of
 * squared deviations).  mean [rows] (of those differences) and rstd [rows] are what the backward reads. */
int xps_add_layer_norm_fwd_f32(const float* x, const float* r, const float* gamma, const float* beta, float* y, float* mean,
                               float* rstd, int64_t rows, int D, float eps, float p, uint64_t seed, void* stream);
/* dx = d(x + dropout(r)), dr = dx * keep / (1 - p) (p = 0: dr may be the SAME buffer as dx), dgamma / dbeta [D] reduced over the
 * rows in a fixed order (per wave, per workgroup, then over workgroups in the workspace). */
size_t xps_add_layer_norm_bwd_f32_workspace(int64_t rows, int D);
int xps_add_layer_norm_bwd_f32(const float* dy, const float* x, const float* r, const float* gamma, const float* mean,
                               const float* rstd, float* dx, float* dr, float* dgamma, float* dbeta, int64_t rows, int D, float p,
                               uint64_t seed, void* workspace, size_t workspace_bytes, void* stream);
/* out = max(x, 0) * keep / (1 - p), decisions of xps_dropout_f32(seed) at the flat index (the feed-forward block) */
int xps_relu_dropout_fwd_f32(const float* x, float* out, int64_t n, float p, uint64_t seed, void* stream);
/* dx = dout / (1 - p) where out > 0 (input positive and kept), else 0: the forward's output is the gate, no seed needed */
int xps_relu_dropout_bwd_f32(const float* dout, const float* out, float* dx, int64_t n, float p, void* stream);
/* out [S][B][D] (TIME-major) = z + table[s]; z is [S][B][D], or [B][S][D] where batch_major != 0; table [>= S][D] */
int xps_add_positional_f32(const float* z, const float* table, float* out, int S, int B, int D, int batch_major, void* stream);
/* Mean over time of a TIME-major z [T][B][F]: out [B][F] = (z[0] + z[1] + ... in this order) / T; dz[t][b][f] = dout[b][f] / T */
int xps_time_mean_fwd_f32(const float* z, float* out, int T, int B, int F, void* stream);
int xps_time_mean_bwd_f32(const float* dout, float* dz, int T, int B, int F, void* stream);
/* CTC loss of the realtime CTC-RNN family (realtime_sim/realtime_nn_model.py:150, :213-224:
 * nn.CTCLoss(blank, reduction='mean', zero_infinity) on log_softmax(logits)).  logits [T][B][C] TIME-major raw
 * scores (the log-softmax is fused); targets [B][target_stride] int64 (padded); lengths int64 [B].
 * nll [B] per-sample negative log-likelihood; loss[0] = mean_b(nll_b / max(L_b, 1)); dlogits (optional, [T][B][C])
 * = d loss[0] / d logits.  One launch for the batch; workspace holds the alpha lattice.
 * Contract (tests/test_gpu_ctc_loss.py pins every line of it):
 *   - Sizes: T, B, C >= 1, 0 <= blank < C, 0 <= max_target_len <= 511 (2 L + 1 states are held in LDS),
 *     target_stride >= max_target_len; else XPS_E_INVALID before any launch, nothing written.  A workspace below
 *     xps_ctc_loss_f32_workspace(T, B, max_target_len) bytes: XPS_E_WORKSPACE, nothing written.  The kernel stays inside
 *     those bytes and needs no initial contents.
 *   - Lengths are clamped on the device: Tb = clamp(input_lengths[b], 0, T), L = clamp(target_lengths[b], 0,
 *     max_target_len), and the clamped L is also the loss's divisor.  Only targets[b][0 .. L) is read: the cells past a
 *     sample's length and the stride padding may hold anything.  Labels in live cells must lie in 0 .. C-1 (the caller's
 *     contract; the kernel only keeps them from addressing outside the row).
 *   - Tb == 0: nll = 0 when L == 0 (the empty alignment, as torch), +inf otherwise; the sample's gradient is zero.
 *   - An infinite nll (no alignment fits): with zero_infinity nll[b] = 0 and the sample's gradient is zero; without,
 *     nll[b] = loss[0] = +inf and the sample's gradient rows t < Tb are unspecified (NaN in torch).  The other samples'
 *     nll and gradient rows do not change either way.
 *   - Every element of dlogits is written; the rows t >= Tb of a sample are zero.  dlogits == NULL: nll and loss only,
 *     the same bits.
 *   - nll[b] depends on sample b alone, dlogits[.][b][.] on sample b and on B through the factor 1 / (B max(L, 1)).
 *   - Logits are finite; -inf logits are unspecified (torch's own gradient is NaN there).                          */
size_t xps_ctc_loss_f32_workspace(int T, int B, int max_target_len);
int xps_ctc_loss_f32(const float* logits, const int64_t* targets, int64_t target_stride,
                     const int64_t* input_lengths, const int64_t* target_lengths, int T, int B, int C,
                     int max_target_len, int blank, int zero_infinity, float* nll, float* loss,
                     float* dlogits, void* workspace, size_t workspace_bytes, void* stream);
/* sumsq[0] = sum g^2 over the flat gradient (deterministic two-stage) */
size_t xps_sumsq_f32_workspace(int64_t n);
int xps_sumsq_f32(const float* g, int64_t n, float* sumsq, void* workspace, size_t workspace_bytes,
                  void* stream);
/* AdamW over flat buffers with clip-by-global-norm folded in:
 *   coef = min(1, max_norm / (sqrt(sumsq[0]) + 1e-6))  (max_norm <= 0: no clip)
 *   g *= coef (written back);  torch.optim.AdamW update with step count `step` (>= 1) */
int xps_adamw_f32(float* p, float* g, float* m, float* v, int64_t n, const float* sumsq, float max_norm,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                  void* stream);
/* the two above in TWO launches instead of three: gradient-norm partials, then clip + AdamW with the final fold of
 * the partials inside (sumsq[0], optional, receives the total = squared pre-clip norm); workspace as xps_sumsq_f32 */
int xps_clip_adamw_f32(float* p, float* g, float* m, float* v, int64_t n, float* sumsq, float max_norm, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int step, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Alignment (alignment/alignment_utils.py:42-61 cnd_avg; AlignCCA.py:235-285;   */
/* AlignMCCA.py:140-154 -> mvlearn MCCA; JointPCA.py:165-211; sklearn PCA at     */
/* nn_models/data_utils/datamodules.py:542-548)                                  */
/* ------------------------------------------------------------------------- */
/* Segmented condition mean.  data [N][row_len] (row_len = T*d), trials of
 * condition c are order[start[c] .. start[c+1]) (original trial order inside a
 * condition).  The sum runs trial after trial in the INPUT dtype, is divided by
 * the count in that dtype and stored as float64 -- np.mean semantics, bit for bit. */
int xps_cnd_avg_f32(const float* data, const int32_t* order, const int32_t* start, double* out,
                    int n_cond, int64_t row_len, void* stream);
int xps_cnd_avg_f64(const double* data, const int32_t* order, const int32_t* start, double* out,
                    int n_cond, int64_t row_len, void* stream);
/* column sums in float64 of an n x d matrix (float32 or float64 input) */
size_t xps_colsum_f64_workspace(int64_t n, int d);
int xps_colsum_f64(const void* X, int is_f32, int64_t ldx, int64_t n, int d, double* out,
                   void* workspace, size_t workspace_bytes, void* stream);
/* Centred cross-covariance on the f64 MFMA:
 *   C[i][j] = sum_r (A[r][i] - mean_a[i]) * (B[r][j] - mean_b[j])        (da x db, float64)
 * A, B float32 or float64 (n x da, n x db); A == B gives the Gram / covariance.  */
size_t xps_xcov_f64_workspace(int64_t n, int da, int db);
int xps_xcov_f64(const void* A, int a_is_f32, int64_t lda, const double* mean_a,
                 const void* B, int b_is_f32, int64_t ldb, const double* mean_b,
                 double* C, int64_t ldc, int64_t n, int da, int db,
                 void* workspace, size_t workspace_bytes, void* stream);
/* Fold-batched alignment (alignment/fold_align.py): every fold of a k-fold split as one device problem.  The tables below
 * are DEVICE arrays of int64 words that the caller builds and bounds-checks (alignment/_linalg.py); pointers are stored as
 * integers, 0 = NULL where a word is optional.
 *
 * xps_xcov_grouped_f64: n_problems centred cross-moment problems in one launch plus one reduce launch, on the tile of
 * xps_xcov_f64 (f64 MFMA, float32 / float64 inputs converted and centred while staged).  A problem reads `nblk` row blocks of
 * `blk_len` consecutive rows from A (n x da) and from B (n x db) -- block j starts at row blk_a[j] of A and blk_b[j] of B --
 * and writes  out = [ C (da x db, ld db) | s_a (da) | s_b (db) | count ]  with
 *   C = sum (a - c_a)(b - c_b)^T,  s_a = sum (a - c_a),  s_b = sum (b - c_b),  count = nblk * blk_len   (zeros for nblk = 0).
 * Words of a problem (XPS_XCOV_GROUPED_WORDS each):
 *   0 A, 1 B, 2 lda, 3 ldb, 4 a_is_f32, 5 b_is_f32, 6 c_a (or 0), 7 c_b (or 0), 8 blk_a (int64[nblk]), 9 blk_b, 10 nblk,
 *   11 blk_len (>= 1), 12 da, 13 db, 14 out (da*db + da + db + 1 doubles), 15 slabs (splits * (da*db + da + db) doubles of
 *   workspace owned by this problem), 16 splits (>= 1), 17 kchunk (rows per split, a multiple of 16, splits * kchunk >= rows).
 * tiles: int32[4 * n_tiles] = {problem, row tile, column tile, split} for EVERY 64 x 64 tile of every split of every problem.
 * Slabs are added in split order: the result does not depend on scheduling.  max_out_len = the largest da*db + da + db + 1. */
#define XPS_XCOV_GROUPED_WORDS 20
int xps_xcov_grouped_f64(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, int max_out_len,
                         void* stream);
/* out[f][e] = sum over g != f, in ascending g, of in[g][e]  (f < n_out <= n_groups, e < len): plain float64 adds from 0. */
int xps_loo_sum_f64(const double* in, double* out, int n_groups, int n_out, int64_t len, void* stream);
/* n_entries products  out = (X - mean) W  in one launch, xps_apply_f64's arithmetic.  Words of an entry
 * (XPS_APPLY_GROUPED_WORDS each): 0 X, 1 x_is_f32, 2 ldx, 3 rows, 4 mean (float64[d_in], or 0), 5 W (float64 d_in x d_out),
 * 6 ldw, 7 d_in, 8 d_out, 9 out, 10 ldo, 11 out_is_f32.  tiles: int32[3 * n_tiles] = {entry, 64-row tile, 64-column tile}. */
#define XPS_APPLY_GROUPED_WORDS 12
int xps_apply_grouped_f64(const int64_t* entries, int n_entries, const int32_t* tiles, int n_tiles, void* stream);
/* n_segments means of float64 rows: out[e] = (sum over i in [begin, end) of src[trials[i] * row_len + e]) / (end - begin),
 * added in list order in float64 (zeros for an empty list).  Words of a segment (XPS_CND_AVG_FOLDS_WORDS each): 0 src,
 * 1 row_len, 2 out (row_len doubles), 3 begin, 4 end (into the device int32 array `trials`).  At most 65535 segments. */
#define XPS_CND_AVG_FOLDS_WORDS 8
int xps_cnd_avg_folds_f64(const int64_t* segments, int n_segments, const int32_t* trials, int64_t max_row_len,
                          void* stream);
/* n_problems Gram matrices  G_p = V_p V_p^T  in one launch (decoders/fold_decode.py: the kernel matrix of every fold of a
 * cross-validated aligned decode).  V_p is row-major float32 or float64, n rows of D contraction elements, leading dimension
 * ldv >= D; G_p float64 n x n, leading dimension ldg >= n; n and D differ per problem.  Words of a problem
 * (XPS_GRAM_GROUPED_WORDS each): 0 V, 1 v_is_f32, 2 ldv, 3 n, 4 D, 5 G, 6 ldg.  tiles: int32[3 * n_tiles] = {problem, 64-row tile
 * ti, 64-column tile tj} for every tile with tj <= ti of every problem; one workgroup per tile walks the whole contraction in
 * ascending k on the f64 MFMA and stores an off-diagonal tile to (ti, tj) and, transposed, to (tj, ti): G_p is symmetric bit for
 * bit and does not depend on the grid.  No atomics.  Elements of G_p beyond column n of a row are not written; D = 0 gives zeros.
 * Both tables are HOST arrays: the call checks them (null tables, negative counts, ldv < D, ldg < n, null matrices, a tile that
 * names no problem, lies above the diagonal or starts at or past n: XPS_E_INVALID before any launch; so a problem with n = 0 has
 * no tiles and writes nothing) and copies them into ws (DEVICE, xps_gram_grouped_f64_workspace(...) bytes) on the stream; they
 * must stay valid until the stream has passed the call.  Nothing synchronises. */
#define XPS_GRAM_GROUPED_WORDS 8
size_t xps_gram_grouped_f64_workspace(int n_problems, int n_tiles);
int xps_gram_grouped_f64(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, void* ws, size_t ws_bytes,
                         void* stream);
/* Fold-batched PCA in front of the SVC search (decoders/search.py, batch_pca=True: the DimRedReshape(PCA) step of
 * scripts/aligned_decode_svm_ncv.py:171-177 for all folds and all n_components at once).
 *
 * xps_gram_center_folds_f64: G is the N x N Gram matrix (leading dimension ldg >= N) of all rows about ONE centre.  Fold f owns the
 * entries rows[fold_off[f] .. fold_off[f + 1]) of the DEVICE int32 list `rows`: its n_train[f] training rows, then its held-out
 * rows (n_all_f in all; a fold may have no held-out rows; the order inside a fold is the caller's).  It receives the dense
 * n_all_f x n_train[f] matrix
 *   Kc_f[a][b] = ((G[r_a][r_b] - m[a]) - m[b]) + mm,   m[a] = (1 / n_tr) sum_{t < n_tr} G[r_a][r_t],   mm = (1 / n_tr) sum_{b < n_tr} m[b]
 * at Kc + sum_{g < f} n_all_g * n_train[g]: the Gram matrix of the fold's rows about the mean of its training rows.  A sum is
 * taken by one wave: lane l adds its terms l, l + 64, ... in ascending order, then the 64 partial sums meet in a fixed butterfly;
 * no atomics, so two runs give the same bits.  fold_off (n_folds + 1) and n_train (n_folds) are HOST arrays: the call checks
 * that fold_off ascends from 0 and 1 <= n_train[f] <= n_all_f, and copies them into ws (DEVICE,
 * xps_gram_center_folds_f64_workspace(n_folds, fold_off[n_folds]) bytes).  The row list is checked on the device and the call
 * WAITS for the stream to learn the verdict: a null pointer, an index outside [0, N) or a bad offset is refused with
 * XPS_E_INVALID before anything is read through the list, so nothing outside G is read.  At most 65535 folds.
 *
 * xps_prefix_kernels_f64: the kernel matrices of column prefixes of score matrices.  Problem p (XPS_PREFIX_KERNELS_WORDS int64
 * words: 0 Z (device pointer, n x R float64), 1 ldz (>= R), 2 n (>= 1), 3 R (>= 1), 4 cut_begin, 5 cut_end) owns the cuts
 * cuts[cut_begin .. cut_end): 1 <= r_1 < r_2 < ... <= R, the lists of the problems following each other, none empty.  Cut c
 * owns the outputs cut_out[c] .. cut_out[c + 1]) (cut_out[0] = 0, cut_out[n_cuts] = n_out); output o is the dense n x n matrix at
 * element dest[o] of K (k_len elements; dest[o] + n * n <= k_len; the caller keeps the outputs apart):
 *   rbf = 0:  K_o[i][j] = acc_r(i, j),   acc_r(i, j) = fma(z_i,r-1, z_j,r-1, ... fma(z_i0, z_j0, 0))      (k ascending)
 *   rbf = 1:  K_o[i][j] = exp(-gammas[o] (acc_r(i, i) + acc_r(j, j) - 2 acc_r(i, j)))    (xps_rbf_from_gram_f64's expression)
 * One thread owns (i, j) and carries its accumulator across the cuts, so Z is read once for all cuts and gammas, and the
 * matrices of cut r are those of a call that has the single cut r, bit for bit; the rbf diagonal is exactly 1 and gamma = 0 gives
 * ones.  tiles: int32[3 * n_tiles] = {problem, 16-row tile, 16-column tile} for every tile of every problem.  ALL tables
 * (problems, cuts, cut_out, gammas, dest, tiles) are HOST arrays: the call checks them (cuts that do not ascend, a cut of 0 or
 * beyond R, n < 1, R < 1, ldz < R, an output outside K, a negative or non-finite gamma, a tile outside its problem, null
 * pointers: XPS_E_INVALID before any launch) and copies them into ws (DEVICE, xps_prefix_kernels_f64_workspace(...) bytes) on
 * the stream; they must stay valid until the stream has passed the call.  Nothing synchronises. */
size_t xps_gram_center_folds_f64_workspace(int n_folds, int64_t total_rows);
int xps_gram_center_folds_f64(const double* G, int64_t ldg, int N, const int32_t* rows, const int32_t* fold_off,
                              const int32_t* n_train, int n_folds, double* Kc, void* ws, size_t ws_bytes, void* stream);
#define XPS_PREFIX_KERNELS_WORDS 8
size_t xps_prefix_kernels_f64_workspace(int n_problems, int n_cuts, int n_out, int n_tiles);
int xps_prefix_kernels_f64(const int64_t* problems, int n_problems, const int32_t* cuts, const int32_t* cut_out, int n_cuts,
                           const double* gammas, const int64_t* dest, int n_out, const int32_t* tiles, int n_tiles, int rbf,
                           double* K, int64_t k_len, void* ws, size_t ws_bytes, void* stream);
/* One-sided Jacobi (Hestenes) on a column-major m x n float64 matrix W (n <= m is not
 * required): rotates column pairs of W and of V (n x n, column-major, identity on
 * entry) until all pairs are orthogonal.  On exit W = U * diag(sigma), V = right
 * singular vectors.  For a symmetric PSD matrix this is its eigendecomposition.
 * `sweeps` full sweeps are enqueued (no host sync); off[0] receives the largest
 * |cos angle| seen in the last sweep.                                          */
/* V may be NULL (rotations not accumulated: for a positive-definite matrix the eigenvectors are the normalised
 * columns of W).                                                                */
size_t xps_jacobi_f64_workspace(int n);
int xps_jacobi_sweeps_f64(double* W, int64_t ldw, double* V, int64_t ldv, int m, int n, int sweeps,
                          double* off, void* workspace, size_t workspace_bytes, void* stream);
/* A ragged batch through the block kernel of xps_jacobi_sweeps_f64: `batch` column-major matrices of different (m, n, ldw)
 * in ONE device buffer W of w_len doubles, matrix b at W + w_off[b] (the matrices must not overlap: not checked).
 * xps_jacobi_batched_supported(m, n): the shapes the block kernel takes (no V, m <= 1024, n > 32) up to 1024 columns;
 * anything else is refused.  `sweeps` sweeps run on every matrix with frozen[b] == 0: one launch per block round covers
 * the batch (1 + max_nb - 1 launches a sweep, max_nb over the batch), and a matrix's iterates are those of
 * xps_jacobi_sweeps_f64 on it alone, bit for bit.  off[b] (DEVICE) receives the largest |cos angle| of the call's last
 * sweep; frozen matrices keep theirs.  check != 0: after the last sweep, on the device, the matrices that ran add `sweeps`
 * to sweeps_done[b] and set frozen[b] = 1 where off[b] <= tol[b].  tol, off, frozen and sweeps_done are DEVICE arrays of
 * `batch` elements that the caller owns and initialises.  w_off, ldw, m and n are HOST arrays: the call checks them (every
 * matrix inside W, ldw >= m, a supported shape: XPS_E_INVALID before any HIP call) and copies them into ws (DEVICE,
 * xps_jacobi_sweeps_batched_f64_workspace(batch) bytes) on the stream; they must stay valid until the stream has passed
 * the call.  batch > 65535 (the grid's second dimension) is refused too.  Nothing synchronises.  batch == 0: XPS_OK,
 * nothing is launched. */
int xps_jacobi_batched_supported(int m, int n);
size_t xps_jacobi_sweeps_batched_f64_workspace(int batch);
int xps_jacobi_sweeps_batched_f64(double* W, int64_t w_len, const int64_t* w_off, const int64_t* ldw, const int* m,
                                  const int* n, int batch, int sweeps, int check, const double* tol, double* off,
                                  int32_t* frozen, int32_t* sweeps_done, void* ws, size_t ws_bytes, void* stream);
/* Small problems (n <= 128 columns, n*m doubles within one workgroup's LDS): the WHOLE decomposition of each of
 * `batch` matrices (stride_w / stride_v doubles apart) in one launch, one workgroup per matrix; sweeps run
 * until the largest |cos angle| of a sweep is <= tol or max_sweeps.  V (optional) is SET to the accumulated
 * rotations (identity on entry is implied).  sweeps_done[batch], off[batch]: optional device outputs.       */
/* Whitening factors of a batch of small symmetric positive definite blocks: A_b = scale * R_b + shift * I = L L^T,
 * S_b = L^-T (upper triangular; S_b^T A_b S_b = I).  Replaces the per-view R_b^-1/2 the reference obtains inside
 * scipy.linalg.eigh(LHS, RHS) (mvlearn MCCA behind alignment/AlignMCCA.py:140-154; a generalised symmetric eigenproblem is
 * reduced with the Cholesky factor of RHS there too).  R_b at R + b * stride_r (row-major, ldr; the lower triangle is read),
 * A_b (optional, may be NULL) and S_b written at A + b * stride_a / S + b * stride_s.  n <= 136 (one workgroup, LDS resident).
 * info[b] = 0, or j + 1 when pivot j is not positive (S_b is then not written). */
int xps_chol_whiten_supported(int n);
int xps_chol_whiten_f64(const double* R, int64_t ldr, int64_t stride_r, double scale, double shift, double* A, int64_t lda,
                        int64_t stride_a, double* S, int64_t lds, int64_t stride_s, int n, int batch, int32_t* info,
                        void* stream);
int xps_jacobi_small_supported(int m, int n, int want_v);
int xps_jacobi_small_f64(double* W, int64_t ldw, int64_t stride_w, double* V, int64_t ldv, int64_t stride_v,
                         int m, int n, int batch, int max_sweeps, double tol, int32_t* sweeps_done, double* off,
                         void* stream);
/* Per-bin high-gamma features of the realtime pipeline (realtime_sim/realtime_processing.py:10-164 process_HG):
 * common average reference over the `good` channels (do_car) -> `bands` filters in scipy.signal.lfilter's direct-form-II-
 * transposed arithmetic (b, a: [bands][taps], normalised by a[0] inside; a == NULL: FIR) with the carried state
 * zi [bands][C][taps-1] updated in place (NULL: zero state) -> RMS over (time, bands) per channel in numpy's summation order.
 * data [C][Tn] float64.  Optional outputs: car_out [C][Tn], filtered [C][Tn][bands], power [C] (filtered and power are
 * exclusive: the power pass squares its copy in place; without `filtered` the copy lives in the workspace).            */
size_t xps_process_hg_f64_workspace(int C, int Tn, int bands);
int xps_process_hg_f64(const double* data, int C, int Tn, const uint8_t* good, const double* b, const double* a,
                       int bands, int taps, double* zi, int do_car, double* car_out, double* filtered,
                       double* power, void* workspace, size_t workspace_bytes, void* stream);
/* The realtime pipeline's frontend: xps_process_hg_f64 (CAR over the good channels -> band-pass with carried state -> RMS)
 * over k consecutive bins of n_streams (1..8) streams in one launch.  bins [n_streams][k][C][Tn], good [n_streams][C]
 * (NULL: all good), b, a [bands][taps] as above (a == NULL: FIR, every bin from a zero state), zi [n_streams][bands][C][taps-1]
 * carried from bin to bin and updated in place (IIR; NULL: zero state per bin), power [n_streams][k][C].  Bin j of stream s
 * gives the bits of xps_process_hg_f64 on that bin alone with the state left by bin j-1. */
size_t xps_pipe_frontend_f64_workspace(int n_streams, int C, int Tn, int bands);
int xps_pipe_frontend_f64(const double* bins, int n_streams, int k, int C, int Tn, const uint8_t* good, const double* b,
                          const double* a, int bands, int taps, double* zi, double* power, void* workspace,
                          size_t workspace_bytes, void* stream);
/* Session replay (realtime_sim/session_replay.py): the frontend over N recorded trials in one launch.
 *   raw [N][n_bins][C][Tn] float64, or float32 (raw_is_f32 = 1) widened on load; bins_per_trial [N] int64 (NULL: n_bins;
 *   clamped to 0..n_bins): trial n has that many bins, the rows after them are written as zeros.
 *   good [C] or (good_per_trial = 1) [N][C], NULL: all good.  b, a [bands][taps] as above (a == NULL: FIR, no carried state).
 *   zi0 [bands][C][taps-1] or (zi_per_trial = 1) [N][bands][C][taps-1], NULL: zero; zi_out [N][bands][C][taps-1] or NULL.
 *   power [N][n_bins][C] or NULL: row j of trial n has the bits xps_pipe_frontend_f64 gives bin j of a stream that started
 *   from zi0 and was fed bins 0..j of the trial; zi_out[n] that stream's state after the trial's last bin.
 *   features [N][n_bins][d] float32 or NULL: float32(power[n][j] @ W[m] + c[m]) with m = map_of_trial[n] (NULL: 0), summed
 *   as xps_window_shift_f32 sums it; W [n_maps][C][d], c [n_maps][d] or NULL; W == NULL: identity, d == C.  A map index
 *   outside 0..n_maps-1 gives NaN rows (map_of_trial may be given with W == NULL, only to be checked against n_maps).
 *   ..._workspace cannot know which outputs are asked for, so it always holds N*n_bins*C doubles (the power, used when
 *   power == NULL) plus, for bands != 8, N*C*Tn*bands doubles (the squared bin of every trial).
 * Tn <= 2048, 1 <= bands, taps <= 32, 1 <= N < 2^31; offsets are 64-bit.  bands == 8 sums in registers; other band counts
 * go through the workspace.  Nothing synchronises. */
size_t xps_hg_trials_f64_workspace(int64_t N, int n_bins, int C, int Tn, int bands);
int xps_hg_trials_f64(const void* raw, int raw_is_f32, int64_t N, int n_bins, int C, int Tn,
                      const int64_t* bins_per_trial, const uint8_t* good, int good_per_trial, const double* b,
                      const double* a, int bands, int taps, const double* zi0, int zi_per_trial, double* zi_out,
                      double* power, const double* W, const double* c, const int32_t* map_of_trial, int n_maps, int d,
                      float* features, void* workspace, size_t workspace_bytes, void* stream);
/* Y[r][:] = (X[r][:] - mean) @ Wt   X: n x d_in (float32 or float64), W: d_in x d_out float64,
 * Y float64 or float32.  Batched transform apply of every aligner.              */
int xps_apply_f64(const void* X, int x_is_f32, int64_t ldx, const double* mean, const double* W,
                  int64_t ldw, void* Y, int y_is_f32, int64_t ldy, int64_t n, int d_in, int d_out,
                  void* stream);
/* Batched C-SVC training on a precomputed kernel matrix (config-1 decode path: the one-vs-one linear SVMs sklearn's
 * SVC(kernel='linear') trains through libsvm; reference call sites decoders/cross_pt_decoders.py:29-38, scripts/aligned_decode_svm.py:262-263).
 * K: n_all x n_all kernel (Gram) matrix, float64, leading dimension ldk.  Problem p: the points idx[off[p] .. off[p+1]) of K, the
 * first npos[p] with label +1, the rest -1 (libsvm's binary sub-problem of a class pair).  One workgroup per problem runs libsvm's
 * SMO (WSS 2, eps stopping rule, calculate_rho) with alpha / gradient in LDS (max_points = the largest problem, at most
 * xps_svm_smo_f64_max_points()); cbound[off[p] + t] = the point's upper bound C * sample_weight (> 0: libsvm drops zero-weight
 * points before training, so does the caller).  Outputs: alpha[off[p] + t], rho[p], iterations[p].                          */
/* RBF kernel matrix from a Gram matrix (SVC(kernel='rbf'): scripts/aligned_decode_svm_ncv.py:313-317):
 * K[i][j] = exp(-gamma (na[i] + nb[j] - 2 G[i][j])), G = A B^T (m x n), na / nb the squared row norms of A / B -- libsvm's formula */
int xps_rbf_from_gram_f64(const double* G, int64_t ldg, const double* na, const double* nb, int m, int n, double gamma,
                          double* K, int64_t ldk, void* stream);
size_t xps_svm_smo_f64_max_points(void);
int xps_svm_smo_f64(const double* K, int64_t ldk, const int* idx, const int* off, const int* npos, int nprob, int max_points,
                    const double* cbound, double eps, int max_iter, double* alpha, double* rho, int* iterations, void* stream);
/* Bagged SVC ensemble (sklearn's BaggingClassifier(SVC), scripts/aligned_decode_svm.py:262-263): all E x P binary problems of the
 * ensemble are posed to ONE xps_svm_smo_f64 launch as index lists into one kernel matrix; these two kernels are the rest.
 * xps_bag_coef_scatter_f64: coef (nprob x n, leading dimension ldc >= n, every element written) = the dense signed dual
 * coefficients: coef[q][idx[off[q] + t]] = +alpha[off[q] + t] for t < npos[q], -alpha[off[q] + t] for the other points of problem
 * q, zero elsewhere (idx, off, npos, alpha as in xps_svm_smo_f64; an index outside [0, n) is dropped).
 * xps_bag_vote_f64: dec is m x Q row-major (ld >= Q), Q = est_off[E]; problem q votes for class pair_a[q] where dec[r][q] - rho[q]
 * > 0 (strictly) and for pair_b[q] otherwise (pair_a[q] < pair_b[q], indices into the ensemble's classes); estimator e owns the
 * problems est_off[e] .. est_off[e + 1]) and votes for the class with the most of their votes (ties: the lowest index, libsvm's
 * rule; an estimator without problems casts no vote); votes[r][c] (m x k, int32) counts the estimators, pred[r] (int32) is the
 * first maximum of votes[r].  Integer arithmetic, no atomics.  k must be in 2..64: anything else is refused.                    */
int xps_bag_coef_scatter_f64(const double* alpha, const int* idx, const int* off, const int* npos, int nprob, int n,
                             double* coef, int64_t ldc, void* stream);
int xps_bag_vote_f64(const double* dec, int64_t ld, const double* rho, const int* pair_a, const int* pair_b, const int* est_off,
                     int m, int E, int k, int* votes, int* pred, void* stream);
/* Cross-validated SVC grid search (GridSearchCV / BayesSearchCV over SVC(kernel='rbf', class_weight='balanced') behind DimRedReshape,
 * scripts/aligned_decode_svm_ncv.py:398-402,422-425): every fold's training set is a sub-block of one kernel matrix, every gamma an
 * element-wise map of one Gram matrix, every C a bound vector, and a fold's held-out rows are rows of the same matrix.
 * xps_rbf_multi_from_gram_f64: K + g * kstride (m x n, leading dimension ldk) = exp(-gammas[g] (na[i] + nb[j] - 2 G[i][j])) for g < M;
 * gammas is a DEVICE array, each element of G is read once, and every matrix equals xps_rbf_from_gram_f64's for that gamma bit for bit.
 * xps_svm_smo_multi_f64: xps_svm_smo_f64 with a matrix per problem: problem p works on the matrix that starts at element kbase[p] of
 * K with leading dimension kld[p] (device arrays); the same kernel, the same iterates.
 * xps_svm_cv_score_f64: model s < S (a candidate on a fold) owns the problems mod_off[s] .. mod_off[s + 1]) in the idx / off / npos /
 * alpha / rho layout of the SMO entry with the class indices pair_a[q] < pair_b[q], the square matrix of mn[s] rows that starts at
 * element mbase[s] of K with leading dimension mld[s], the held-out rows tst[tst_off[s] .. tst_off[s + 1]) (row indices into its
 * matrix) and their true class indices ytrue[...].  dec(r, q) = sum_t +-alpha[off[q] + t] K_s[r][idx[off[q] + t]] - rho[q] (+ for
 * t < npos[q], the convention of xps_bag_coef_scatter_f64); q votes pair_a[q] where dec > 0 STRICTLY, else pair_b[q]; the prediction
 * is the first maximum of the k vote counts (libsvm).  Outputs: pred[tst_off[s] + i] (int32), conf[s][true][pred] (S x k x k int32,
 * every element written, zeros for a model without held-out rows), and, unless dec_out is NULL, dec_out[(tst_off[s] + i) * ldd +
 * (q - mod_off[s])] (ldd >= the largest problem count of a model).  mod_off and tst_off (S + 1 ints each) are HOST arrays: the call
 * checks that they ascend from a value >= 0 and copies them into ws (DEVICE, xps_svm_cv_score_f64_workspace(S) bytes) on the stream.
 * Nothing outside a model's matrix is dereferenced: a point index outside [0, mn[s]) adds no term; a held-out row outside it gets
 * pred = -1, decisions of 0 and no count; a true class outside [0, k) is not counted.  k must be in 2..64.  Fixed summation order,
 * integer votes and counts, no atomics: the result does not depend on the grid.                                                  */
int xps_rbf_multi_from_gram_f64(const double* G, int64_t ldg, const double* na, const double* nb, int m, int n, const double* gammas,
                                int M, double* K, int64_t ldk, int64_t kstride, void* stream);
int xps_svm_smo_multi_f64(const double* K, const int64_t* kbase, const int64_t* kld, const int* idx, const int* off, const int* npos,
                          int nprob, int max_points, const double* cbound, double eps, int max_iter, double* alpha, double* rho,
                          int* iterations, void* stream);
size_t xps_svm_cv_score_f64_workspace(int S);
int xps_svm_cv_score_f64(const double* K, const int64_t* mbase, const int64_t* mld, const int* mn, const int* idx, const int* off,
                         const int* npos, const double* alpha, const double* rho, const int* pair_a, const int* pair_b,
                         const int* mod_off, const int* tst, const int* ytrue, const int* tst_off, int S, int k, int* pred, int* conf,
                         double* dec_out, int64_t ldd, void* ws, size_t ws_bytes, void* stream);
/* The ragged kernels of the search through the aligned decoder (decoders/aligned_search.py; BayesSearchCV over a
 * crossPtDecoder_sepAlign, scripts/aligned_decode_svm_ncv.py:388-413): the kernel matrices of all (alignment, fold, gamma) and the
 * 'scale' variances of all (alignment, fold) in one launch each, however many candidates are searched.  Both follow
 * xps_gram_grouped_f64's convention: HOST tables, checked by the call and copied into ws (DEVICE, ..._workspace(...) bytes) on the
 * stream; they must stay valid until the stream has passed the call.  Nothing synchronises.
 *
 * xps_rbf_grouped_from_gram_f64: n_problems rbf maps of square Gram matrices.  Words of a problem (XPS_RBF_GROUPED_WORDS each):
 * 0 G (float64 n x n), 1 ldg (>= n), 2 n, 3 gamma (the bits of a double, finite and >= 0), 4 K (float64 n x n), 5 ldk (>= n).
 *   K_p[i][j] = exp(-gamma_p (G_p[i][i] + G_p[j][j] - 2 G_p[i][j])):
 * xps_rbf_from_gram_f64's bits for na = nb = the diagonal of G_p.  Several problems may read one G with different gammas; a K may
 * not be a G of the call (K == G of its own problem is refused, the rest is the caller's).  tiles: int32[3 * n_tiles] =
 * {problem, 64-row tile ti, 64-column tile tj} for every tile of every problem; one workgroup per tile, no atomics, the result does
 * not depend on the grid.  Elements of K_p beyond column n of a row are not written; a problem with n = 0 has no tiles and writes
 * nothing.  Refused with XPS_E_INVALID before any launch: null tables or matrices, negative counts, ldg < n, ldk < n, a negative or
 * non-finite gamma, a tile that names no problem or starts at or past n, a null or too small workspace.
 *
 * xps_var_grouped_f64: out[e] (float64, DEVICE, n_entries elements) = the population variance of all elements of entry e's row
 * block: the mean of the squared deviations from the mean of its rows * D elements (numpy's X.var(); 0 for an empty block).  Words
 * of an entry (XPS_VAR_GROUPED_WORDS each): 0 V (row-major float32 or float64), 1 v_is_f32, 2 ldv (>= D), 3 first row, 4 rows, 5 D.
 * One workgroup per entry; two passes in float64 (the mean, then the deviations); a thread adds its elements in ascending order
 * and the partial sums meet in a fixed tree: no atomics, two runs give the same bits.  Refused with XPS_E_INVALID before any
 * launch: a null table, output or matrix, negative counts, ldv < D, v_is_f32 outside 0 / 1, a null or too small workspace. */
#define XPS_RBF_GROUPED_WORDS 8
size_t xps_rbf_grouped_from_gram_f64_workspace(int n_problems, int n_tiles);
int xps_rbf_grouped_from_gram_f64(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, void* ws,
                                  size_t ws_bytes, void* stream);
#define XPS_VAR_GROUPED_WORDS 8
size_t xps_var_grouped_f64_workspace(int n_entries);
int xps_var_grouped_f64(const int64_t* entries, int n_entries, double* out, void* ws, size_t ws_bytes, void* stream);
/* small dense float64 GEMM C = op(A) op(B)  (row-major, op = transpose flag) */
int xps_dgemm_small(const double* A, int64_t lda, int ta, const double* B, int64_t ldb, int tb,
                    double* C, int64_t ldc, int M, int N, int K, void* stream);
/* the same product with the contraction split over workgroups (few output tiles, long K: the skinny products of the MCCA
 * eigensolve); deterministic partial slabs in `workspace` (xps_dgemm_splitk_workspace bytes), one reduce launch */
size_t xps_dgemm_splitk_workspace(int M, int N, int K);
int xps_dgemm_splitk(const double* A, int64_t lda, int ta, const double* B, int64_t ldb, int tb, double* C, int64_t ldc,
                     int M, int N, int K, void* workspace, size_t workspace_bytes, void* stream);
/* Chebyshev filter of an n x m block A (row-major, leading dimension m) by the symmetric n x n matrix C: the scaled three-term
 * recurrence of the top-k eigensolve behind AlignMCCA.fit (alignment/AlignMCCA.py:152-153 hands the generalised eigenproblem
 * to mvlearn / scipy.linalg.eigh): Y_1 = (C A - c A) sigma1 / e, Y_{j+1} = (C Y_j - c Y_j) 2 sigma_{j+1} / e - sigma_j sigma_{j+1} Y_{j-1},
 * sigma_{j+1} = 1 / (2 / sigma1 - sigma_j); `deg` >= 1 products, all enqueued by this one call; out (n x m, leading dimension m)
 * receives Y_deg and may not be A (refused: XPS_E_INVALID); C has leading dimension ldc >= n, e > 0.  Each product is summed as
 * xps_dgemm_splitk sums it; the reduce of its slabs applies the three-term update.                                          */
/* `steps` Lanczos steps (no reorthogonalisation) on the symmetric n x n matrix C (leading dimension ldc) from v0 / ||v0||: v0 (n,
 * device) may have any non-zero length, it is normalised on the device inside the call (no host synchronisation; a zero v0 gives
 * NaN).  alpha[steps], beta[steps] (device arrays) = diagonal / off-diagonal of the tridiagonal matrix whose extreme Ritz values
 * bound the spectrum for the filter */
size_t xps_lanczos_f64_workspace(int n);
int xps_lanczos_f64(const double* C, int64_t ldc, int n, int steps, const double* v0, double* alpha, double* beta,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t xps_cheb_filter_f64_workspace(int n, int m);
int xps_cheb_filter_f64(const double* C, int64_t ldc, int n, const double* A, int m, int deg, double c, double e, double sigma1,
                        double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Training-set augmentations on (trial x time x channel) fp32 tensors           */
/* (nn_models/data_utils/augmentations.py:13-90).  The caller makes the random    */
/* draw exactly as the reference does (numpy / torch global generators) and       */
/* passes it in; x and out are [N][T][C], out != x for shift / warp.               */
/*   time_shift : out = torch.roll(x, shift, dims=1)                 (:51-62)      */
/*   time_mask  : out = x with [start, start + size) along time zeroed (:32-48)     */
/*   scale      : out = x * scale                                      (:79-89)    */
/*   jitter     : out = x + noise * level  (noise: the N(0,1) draw)    (:65-76)    */
/*   time_warp  : scipy.ndimage.zoom(order=1) to T2 samples, then torchvision       */
/*                Resize back to T (bilinear, antialias), fused          (:13-29)   */
/* ------------------------------------------------------------------------- */
int xps_aug_time_shift_f32(const float* x, float* out, int N, int T, int C, int shift, void* stream);
int xps_aug_time_mask_f32(const float* x, float* out, int N, int T, int C, int start, int size, void* stream);
int xps_aug_scale_f32(const float* x, float* out, int64_t n, float scale, void* stream);
int xps_aug_jitter_f32(const float* x, const float* noise, float* out, int64_t n, float level, void* stream);
int xps_aug_time_warp_f32(const float* x, float* out, int N, int T, int C, int T2, void* stream);

/* ------------------------------------------------------------------------- */
/* Cross-patient CTC training data (csrc/xps_ctc_data.hip)         */
/* ------------------------------------------------------------------------- */
/* Per-trial augmentations (realtime_sim/augmentations.py:14-90): ONE draw per trial, handed in as a DEVICE array of N
 * entries made by the caller with the reference's generator calls.  x, out [N][T][C] fp32, single pass; `out` may point into
 * a larger buffer (a slab of the concatenated training tensor); out != x for shift / warp.
 *   trial_shift : out[n, t] = x[n, (t - shift[n]) mod T]      (:52-61; shift int64, any value)
 *   trial_mask  : [start[n], start[n] + size) along time zeroed (:37-49; start int64; 0 <= size <= T, else XPS_E_INVALID;
 *                 the part of a window that lies outside 0..T is ignored)
 *   trial_scale : out[n] = x[n] * scale[n], one fp32 multiply   (:78-90; rows of row_len = T * C floats)
 *   trial_warp  : two linear resamplings T -> T2[n] -> T, each ATen's upsample_linear1d with align_corners = False (source
 *                 coordinate scale * (dst + 0.5) - 0.5 clamped at 0, neighbour index clamped at the end, fp32), fused: the
 *                 intermediate row is never stored (:14-34; T2 int64 = int(T * factor[n]) computed by the caller, >= 1)
 *   jitter      : element-wise already: xps_aug_jitter_f32 above                                     (:64-75)            */
int xps_aug_trial_shift_f32(const float* x, float* out, int N, int T, int C, const int64_t* shift, void* stream);
int xps_aug_trial_mask_f32(const float* x, float* out, int N, int T, int C, const int64_t* start, int size, void* stream);
int xps_aug_trial_scale_f32(const float* x, float* out, int N, int64_t row_len, const float* scale, void* stream);
int xps_aug_trial_warp_f32(const float* x, float* out, int N, int T, int C, const int64_t* T2, void* stream);
/* Greedy CTC decode of a batch in one launch (realtime_sim/ctc_decoder.py:172-189): per frame the first maximum over the C
 * classes (torch.argmax: lowest index on ties, the first NaN counts as the maximum), repeats collapsed, blanks dropped.
 * logits: float32 (is_f32 = 1) or float64 scores or log-probabilities; frame t of sequence b starts at element
 * t * stride_t + b * stride_b, its classes are contiguous -- (T, B, C) and (B, T, C) tensors both work.  Every one of the T
 * frames is decoded.  tokens [B][T] int64: the decoded labels of sequence b, then -1; lengths [B] int64: their number. */
int xps_ctc_greedy_decode(const void* logits, int is_f32, int64_t stride_t, int64_t stride_b, int T, int B, int C,
                          int blank, int64_t* tokens, int64_t* lengths, void* stream);
/* Unit-cost Levenshtein distance of B padded pairs in one launch (torchaudio.functional.edit_distance as used by calc_PER,
 * realtime_sim/realtime_nn_model.py:307-324): pred [B][pred_stride] int64 with pred_len [B] int64, tgt [B][tgt_stride] int64 with
 * tgt_len [B] int64 -> dist [B] int64.  max_pred_len / max_tgt_len: upper bounds of the lengths (<= the strides; a larger
 * length entry is clamped to its bound).  Supported: max_pred_len <= 65536, max_tgt_len <= 1024
 * (xps_edit_distance_supported); else XPS_E_INVALID before any launch. */
int xps_edit_distance_supported(int max_pred_len, int max_tgt_len);
int xps_edit_distance_i64(const int64_t* pred, int64_t pred_stride, const int64_t* pred_len, const int64_t* tgt,
                          int64_t tgt_stride, const int64_t* tgt_len, int B, int max_pred_len, int max_tgt_len,
                          int64_t* dist, void* stream);
/* Edit-operation alignment (csrc/xps_edit_align.hip, realtime_sim/ctc_errors.py): the Levenshtein
 * alignment behind the distance, i.e. WHICH tokens were hit, substituted, deleted and inserted.  One launch for the batch, one
 * wave per pair, no host synchronisation, no allocation; a pair's per-pair outputs do not depend on the rest of its batch.
 * Inputs: exactly xps_edit_distance_i64's, with the same meaning (pred [B][pred_stride] int64 with pred_len [B], tgt
 *   [B][tgt_stride] int64 with tgt_len [B]; max_pred_len <= 65536, max_tgt_len <= 1024; a length entry is clamped to
 *   0..max_pred_len / 0..max_tgt_len; padding is never read), and n_classes = K, read only when `confusion` is given.
 * Names.  A HIT is a prediction token aligned to an equal target token, a SUBSTITUTION one aligned to an unequal target
 *   token, an INSERTION a prediction token aligned to nothing, a DELETION a target token aligned to nothing.
 * Table, a = pred of length m, t = tgt of length n, tokens 1-based:
 *     D[i][0] = i,  D[0][j] = j,
 *     D[i][j] = min(D[i-1][j-1] + [a_i != t_j], D[i-1][j] + 1, D[i][j-1] + 1).
 * TIE RULE (part of the contract, stated on D alone so that no evaluation order can change it).  Walk back from (m, n).  At
 *   a cell with i > 0 and j > 0: take the diagonal (i-1, j-1) if D[i][j] == D[i-1][j-1] + [a_i != t_j]; else the insertion
 *   (i-1, j) if D[i][j] == D[i-1][j] + 1; else the deletion (i, j-1).  On the border i = 0 there are only deletions, on the
 *   border j = 0 only insertions.  A diagonal step aligns a_i with t_j (a hit when they are equal, else a substitution).
 * Outputs; `dist` is always written, each of the others may be NULL and is then skipped; every element of a non-NULL
 *   per-pair output is written.
 *   dist [B] int64 = D[m][n] (= xps_edit_distance_i64's).
 *   counts [B][4] int64 = hits, substitutions, deletions, insertions: hits + substitutions + deletions = n,
 *     hits + substitutions + insertions = m, substitutions + deletions + insertions = dist.
 *   tgt_to_pred [B][max_tgt_len] int32: the 0-based index of the prediction token aligned to target token j, -1 for a
 *     deleted one, -2 for j >= n.
 *   pred_to_tgt [B][max_pred_len] int32: the 0-based index of the target token aligned to prediction token i, -1 for an
 *     inserted one, -2 for i >= m.
 *   confusion [K+1][K+1] int64, ADDED INTO (the caller zeroes it; launches and batches accumulate into one matrix): row =
 *     target class, row K = no target (an insertion); column = predicted class, column K = nothing (a deletion); one count
 *     per step of the walk, so cell (K, K) is never touched.  64-bit integer atomic adds, no floating point: the sum does
 *     not depend on the order and two runs give the same bytes.  (K + 1)^2 <= 8192 cells are first summed per workgroup
 *     (4 pairs) in LDS and reach the matrix as one add per non-zero cell; a larger matrix takes one add per step of the
 *     walk; no result depends on that route.  Labels outside 0..K-1 are the caller's to refuse; the
 *     kernel clamps them to 0..K-1 for the cell index only (memory safety), never for the comparison a_i != t_j.
 * Workspace: ..._workspace bytes, one backpointer byte per cell at (b * max_pred_len + i - 1) * max_tgt_len + j - 1
 *   (0 hit, 1 substitution, 2 insertion, 3 deletion: the tie rule evaluated in the forward pass); only cells with
 *   1 <= i <= m and 1 <= j <= n may be written.
 * XPS_E_INVALID before any launch: everything xps_edit_distance_i64 refuses (B < 0, lengths outside
 *   xps_edit_distance_supported, a stride shorter than its padded length), K < 1 when `confusion` is given, a NULL pointer
 *   that the sizes need, a workspace that is NULL or smaller than ..._workspace. */
size_t xps_edit_align_workspace(int B, int max_pred_len, int max_tgt_len);
int xps_edit_align(const int64_t* pred, int64_t pred_stride, const int64_t* pred_len, const int64_t* tgt,
                   int64_t tgt_stride, const int64_t* tgt_len, int B, int max_pred_len, int max_tgt_len, int n_classes,
                   int64_t* dist, int64_t* counts, int32_t* tgt_to_pred, int32_t* pred_to_tgt, int64_t* confusion,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Electrode subsampling (csrc/xps_subsample.hip): spatial        */
/* averaging over groups of grid channels and channel selection, for one          */
/* grouping or a whole sweep of them in one launch.                                */
/* ------------------------------------------------------------------------- */
/* processing_utils/spatial_avg_subsampling.py:74-90 (spatial_avg_data).  data [N][C][T]: the reference's (trials, X, Y, T)
 * with the grid flattened row-major, C = X * Y.  Groups in CSR form: offsets[G + 1] (offsets[0] = 0) and members[offsets[G]],
 * int32 channel numbers in [0, C), every group non-empty, groups may be ragged and may share channels (DEVICE arrays; the
 * caller validates them: the library cannot read them without synchronising).  out [N][T][G] float64, channel-last.
 * Arithmetic = np.mean(data[:, ix, iy], axis=1): the members of a group added one by one in member order in the INPUT's
 * dtype, one division by the member count in that dtype, then widened to float64; no fused multiply-add, no atomics, the
 * bits do not depend on the launch geometry.  XPS_E_INVALID when the C channels of one time sample exceed the LDS tile
 * (C > 6144 for f32, C > 3072 for f64). */
int xps_group_mean_f32(const float* data, int N, int C, int T, const int32_t* offsets, const int32_t* members, int G,
                       double* out, void* stream);
int xps_group_mean_f64(const double* data, int N, int C, int T, const int32_t* offsets, const int32_t* members, int G,
                       double* out, void* stream);
/* S groupings in ONE launch (CSR of CSR): grouping s owns the groups group_start[s] .. group_start[s + 1] - 1 (int32
 * [S + 1], group_start[0] = 0, group_start[S] = Gtot) of the shared offsets[Gtot + 1] / members arrays.  out: one buffer of
 * N * T * Gtot float64; the slab of grouping s starts at element N * T * group_start[s] and is [N][T][G_s].  Every staged
 * input tile serves all S groupings before the next is loaded: the input is read from HBM once per launch.  Each slab
 * holds the bits xps_group_mean_* gives for that grouping alone. */
int xps_group_mean_many_f32(const float* data, int N, int C, int T, const int32_t* group_start, const int32_t* offsets,
                            const int32_t* members, int S, int Gtot, double* out, void* stream);
int xps_group_mean_many_f64(const double* data, int N, int C, int T, const int32_t* group_start, const int32_t* offsets,
                            const int32_t* members, int S, int Gtot, double* out, void* stream);
/* X[:, :, idx_s] for S index lists in one launch (scripts/aligned_decode_grid_subsample.py slices the channel-last features
 * of every sliding window this way).  x [N][T][C] fp32; list s is idx[list_start[s] .. list_start[s + 1] - 1] (int32 device
 * arrays, list_start[0] = 0, list_start[S] = Ltot, entries in [0, C)); out: N * T * Ltot fp32, slab s at element
 * N * T * list_start[s], [N][T][L_s], the input's bits.  XPS_E_INVALID for C > 12288 (the channels of one sample exceed the
 * LDS tile). */
int xps_select_channels_f32(const float* x, int N, int T, int C, const int32_t* list_start, const int32_t* idx, int S,
                            int Ltot, float* out, void* stream);
/* the same for float64 features (C <= 6144) */
int xps_select_channels_f64(const double* x, int N, int T, int C, const int32_t* list_start, const int32_t* idx, int S,
                            int Ltot, double* out, void* stream);

/* ------------------------------------------------------------------------- */
/* Cluster separability scores (csrc/xps_cluster.hip):            */
/* label-grouped sums over ONE Gram matrix for R label vectors at once.            */
/* ------------------------------------------------------------------------- */
/* The R label vectors of a call are ONE transposed DEVICE array labels_t[j][r] (uint8, n rows of R bytes) with values in
 * [0, k), 2 <= k <= XPS_CLUSTER_MAX_CLASSES; a label >= k is skipped by every kernel, never used as an index.  All arithmetic
 * is float64 without atomics, every sum is taken by one lane in ascending index order: the results of a label set do not depend
 * on the grid, the stream or the other label sets of the call.  Nothing allocates or synchronises; every refusal (null pointers,
 * n < 1, R < 1, k outside 2..64, ldg < n, ...) is XPS_E_INVALID before any launch.
 *
 * xps_label_row_sums_f64: S[r][i][q] = sum over j with y_r[j] = q, j ascending, of f(i, j); S is (R, n, k) contiguous.
 *   mode 0:  f = G[i][j]
 *   mode 1:  f = sqrt(max((G[i][i] + G[j][j]) - 2 G[i][j], 0)), each operation rounded once, and exactly 0 for j = i
 *            (sklearn's euclidean_distances through the Gram matrix; the n x n distance matrix is never stored)
 * G is n x n with leading dimension ldg >= n.  R <= 64 * 65535.
 *
 * xps_label_col_sums_f64: M[r][p][c] = sum over i with y_r[i] = p, i ascending, of V[r][i][c]; V is (R, n, w) with v_set_stride
 * elements between two sets (>= n * w, or 0: one (n, w) table shared by every set), M is (R, k, w) contiguous, w >= 1.
 *
 * xps_silhouette_from_sums_f64: from the mode-1 sums S and the class counts of every set (counts, (R, k) int32, HOST: checked --
 * each in [0, n], each set adding up to n -- and copied into ws, DEVICE, ..._workspace(R, k) bytes, on the stream; valid until
 * the stream has passed the call), sklearn.metrics.silhouette_samples: a = own-class sum / (count - 1), b = the smallest
 * sum / count over the other NON-EMPTY classes, s = (b - a) / max(a, b), 0 for a sample alone in its class and for 0 / 0.
 * sil is (R, n); stats is (R, 3) = {mean of s, mean of the positive s (NaN when none is), number of positive s}, taken by one
 * wave per set: lane l adds its terms l, l + 64, ... in ascending order, then the 64 partial sums meet in a fixed butterfly.
 *
 * xps_centroid_dist_from_sums_f64: dist[r][i] = sqrt(max(G[i][i] - 2 S0[r][i][p] / n_p + M[r][p][p] / n_p^2, 0)) with p = y_r[i]
 * and n_p its count: the distance of sample i to the centroid of its own class (Davies-Bouldin), from the mode-0 sums S0
 * (R, n, k) and their class-block sums M (R, k, k) = xps_label_col_sums_f64 of S0 with w = k.  counts and ws as above. */
#define XPS_CLUSTER_MAX_CLASSES 64
int xps_label_row_sums_f64(const double* G, int64_t ldg, const uint8_t* labels_t, int n, int R, int k, int mode, double* S,
                           void* stream);
int xps_label_col_sums_f64(const double* V, int64_t v_set_stride, const uint8_t* labels_t, int n, int R, int k, int w, double* M,
                           void* stream);
size_t xps_silhouette_from_sums_f64_workspace(int R, int k);
int xps_silhouette_from_sums_f64(const double* S, const int32_t* counts, const uint8_t* labels_t, int n, int R, int k, double* sil,
                                 double* stats, void* ws, size_t ws_bytes, void* stream);
size_t xps_centroid_dist_from_sums_f64_workspace(int R, int k);
int xps_centroid_dist_from_sums_f64(const double* G, int64_t ldg, const double* S0, const double* M, const int32_t* counts,
                                    const uint8_t* labels_t, int n, int R, int k, double* dist, void* ws, size_t ws_bytes,
                                    void* stream);

/* ------------------------------------------------------------------------- */
/* Exact t-SNE (csrc/xps_tsne.hip; manifold/tsne.py):              */
/* sklearn's _t_sne.py / _utils.pyx, batched over data sets of different n.        */
/* ------------------------------------------------------------------------- */
/* Every entry takes xps_gram_grouped_f64's convention: a HOST table of XPS_TSNE_WORDS int64 words per problem and a HOST tile
 * table int32[2 * n_tiles] = {problem, row tile}, which must list, for the problems in order, every tile of XPS_TSNE_TILE_ROWS
 * rows in ascending order (cdiv(n, 4) tiles per problem; one workgroup of four waves each, a wave per row).  The call checks both and copies them into ws
 * (DEVICE, ..._workspace(n_problems, n_tiles) bytes) on the stream; they stay valid until the stream has passed the call.
 * Nothing allocates or synchronises.  Refused with XPS_E_INVALID before any launch: null tables, no problem, n outside
 * 2 .. XPS_TSNE_MAX_SAMPLES, n_components outside {1, 2}, another tile table, a null workspace or one too small, and what each
 * entry lists.  Words of a problem (an entry reads only those it names):
 *   0 n   1 n_components   2 G (double, n x n)   3 ldg   4 d2 (float, n x n contiguous)   5 C (double, n x n contiguous)
 *   6 P (double, n x n contiguous)   7 beta (double, n)   8 steps (int32, n)   9 rowsum (double, n)   10 Y_in (double, n x nc)
 *   11 Y_out (double, n x nc)   12 state (double, xps_tsne_state_bytes(n) bytes)   13 it_begin   14 learning rate (the bits of a double)
 *
 * Float64, no atomics; no operation is contracted into an fma.  SUMMATION ORDER of every sum over j of a row and of every sum
 * over rows: lane l of one wave adds its terms l, l + 64, ... in ascending order, then the 64 partial sums meet in the fixed
 * butterfly of xps_silhouette_from_sums_f64.  So a problem's results do not depend on the grid, the batch or the stream.
 *
 * xps_tsne_sqdist_f32 (words 0, 2, 3, 4): d2[i][j] = (float)max((G_ii + G_jj) - 2 G_ij, 0), exactly 0 for j = i
 * (sklearn's euclidean_distances(squared=True) through the Gram matrix, then distances.astype(float32)).  Refused: ldg < n.
 *
 * xps_tsne_affinities_f64 (words 0, 4 .. 9), two launches.  The first is _binary_search_perplexity for every row i, one wave
 * each: beta = 1, beta_min = -inf, beta_max = inf; at most 100 steps of
 *     sum = sum_{j != i} exp(-d2_ij * beta)   (0 -> (double)1e-8f);      sd = sum_{j != i} d2_ij * (exp(-d2_ij * beta) / sum)
 *     diff = (log(sum) + beta * sd) - log((double)(float)perplexity);      stop if |diff| <= (double)1e-5f
 *     diff > 0: beta_min = beta; beta = beta_max == inf ? beta * 2 : (beta + beta_max) / 2
 *     else:     beta_max = beta; beta = beta_min == -inf ? beta / 2 : (beta + beta_min) / 2
 * (the .pyx holds the perplexity and both constants in C floats).  C[i][j] = exp(-d2_ij * beta) / sum of the LAST step taken,
 * C[i][i] = 0; steps[i] = the number of steps taken (100: exhausted); beta[i] = beta as the loop leaves it (after the update of
 * an exhausted search); rowsum[i] = sum_j C[i][j].  The second launch: S = max(2 sum_i rowsum[i], eps), the sum of all
 * C_ij + C_ji;  P[i][j] = max((C_ij + C_ji) / S, eps), P[i][i] = 0;  eps = 2.220446049250313e-16.  Refused: a perplexity that
 * is not positive and finite or not below every n; C == P.
 *
 * xps_tsne_descent_f64 (words 0, 1, 6, 10 .. 14): 1 + n_launches launches.  With d = y_i - y_j, q_ij = 1 + |d|^2 (the squares
 * added component 0 first), w_ij = 1 / q_ij, the PARTIAL SUMS of row i at an embedding are, over j != i,
 *     s_i = sum w_ij      a_i[c] = sum (P_ij w_ij) d[c]      b_i[c] = sum (w_ij w_ij) d[c]
 *     e1_i = sum P_ij log(P_ij q_ij)      e2_i = sum P_ij          (e1, e2 only where the next iteration evaluates the error)
 * Launch 0 PRIMES a phase of _gradient_descent: Y = Y_in, update = 0, gains = 1, error = best error = DBL_MAX, iteration =
 * best iteration = it_begin, and the partial sums at Y.  Launch t >= 1 runs iteration i of every problem that is not done:
 *     Z = sum_i s_i;   grad = 4 (e a_i[c] - (1 / Z) b_i[c]),   e = exaggeration
 *     gains = update * grad < 0 ? gains + 0.2 : gains * 0.8, at least 0.01;   update = momentum * update - lr * (grad * gains)
 *     Y += update;   at i == max_iter - 1 or (i + 1) % 50 == 0:  error = e ((sum_i e1_i) + log(e Z) (sum_i e2_i)), else NaN
 *     at (i + 1) % 50 == 0:  error < best error ? best = error, best iteration = i : done if i - best iteration >
 *         n_iter_without_progress;   done if sqrt(sum_i ((grad gains)[0]^2 + (grad gains)[1]^2)) <= min_grad_norm
 *     done at i == max_iter - 1;   then the partial sums at the new Y, unless i == max_iter - 1.
 * This is sklearn's exact _kl_divergence without its clamp Q = max(w / Z, eps): the clamp is inactive while w_ij / Z > eps,
 * which tests/tsne_ref.py asserts for every case it is held to.  When a problem becomes done its Y (after the step: what
 * _gradient_descent returns) is written to Y_out; later launches skip it by a uniform branch, so its state stays as it stopped.
 * STATE: two halves of XPS_TSNE_STATE_HEAD + XPS_TSNE_STATE_ARRAYS * n doubles; launch t reads half (t - 1) & 1 and writes
 * half t & 1, so the result of the call is in half n_launches & 1.  A half: {iteration (the next to run; sklearn's `it` once
 * done), error, best error, best iteration, done, Z, gradient norm of the last check, 0}, then the arrays of n doubles
 * Y[0] Y[1] update[0] update[1] gains[0] gains[1] grad[0] grad[1] s a[0] a[1] b[0] b[1] e1 e2 (component 1 of a
 * one-component problem: Y = update = grad = 0, gains = 1).  The problem's first workgroup alone writes the first eight
 * arrays and the head; every workgroup rebuilds the step in LDS from the read half and writes the partial sums of its rows.
 * Y_in may be Y_out.  Refused: n_launches < 0, max_iter < 1, it_begin outside 0 .. max_iter - 1, a momentum that is negative or
 * not finite, an exaggeration or a learning rate that is not positive and finite, n_iter_without_progress < 0, a NaN
 * min_grad_norm, null P / Y_in / Y_out / state. */
#define XPS_TSNE_WORDS 16
#define XPS_TSNE_TILE_ROWS 4
#define XPS_TSNE_MAX_SAMPLES 4096
#define XPS_TSNE_STATE_HEAD 8
#define XPS_TSNE_STATE_ARRAYS 15
size_t xps_tsne_state_bytes(int n);
size_t xps_tsne_sqdist_f32_workspace(int n_problems, int n_tiles);
int xps_tsne_sqdist_f32(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, void* ws, size_t ws_bytes,
                        void* stream);
size_t xps_tsne_affinities_f64_workspace(int n_problems, int n_tiles);
int xps_tsne_affinities_f64(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, double perplexity, void* ws,
                            size_t ws_bytes, void* stream);
size_t xps_tsne_descent_f64_workspace(int n_problems, int n_tiles);
int xps_tsne_descent_f64(const int64_t* problems, int n_problems, const int32_t* tiles, int n_tiles, int n_launches, int max_iter,
                         double momentum, double exaggeration, int n_iter_without_progress, double min_grad_norm, void* ws,
                         size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Representational dissimilarity analysis (csrc/xps_rsa.hip; alignment/rsa.py;   */
/* DESIGN.md 4.23): the figure notebooks' calc_rdm_corr / compare_rdms, batched.   */
/* ------------------------------------------------------------------------- */
/* Every entry takes xps_gram_grouped_f64's convention: HOST tables of int64 words, checked by the call and copied into ws (DEVICE,
 * ..._workspace(...) bytes) on the stream; they stay valid until the stream has passed the call.  Nothing allocates or
 * synchronises; every refusal is XPS_E_INVALID before any launch.  Float64, no atomics; every sum is taken in an order that is a
 * function of the problem alone (a thread or lane adds its elements in ascending order, the partial sums meet in a fixed tree),
 * so a problem's bits do not depend on the grid, the stream or the other problems of the call.
 *
 * xps_row_standardize_grouped_f64: every row x of every problem's matrix X (rows x D, leading dimension ldx >= D) becomes
 * z = (x - mean) / |x - mean| in Z (leading dimension ldz >= D; Z may be X), scipy.stats.pearsonr's arithmetic: the Gram matrix
 * of Z holds every r_ij.  mean = m0 + sum(x - m0) / D with m0 = sum(x) / D; |.| = sqrt(sum d^2).  A row whose elements are all
 * equal (scipy's constant input) and any row of norm 0 become NaN.  Words of a problem (XPS_RSA_STD_WORDS each): 0 X, 1 ldx,
 * 2 rows, 3 D (>= 1), 4 Z, 5 ldz.  At most 65535 problems.  Refused: a null table or matrix, negative counts, D < 1, ldx < D,
 * ldz < D, a null or too small workspace.
 *
 * xps_rdm_from_corr_grouped_f64: out[i][j] = 1 - clip(r[i][j], -1, 1) for every problem; a NaN stays a NaN; the diagonal is
 * exactly 0 unless it is NaN.  Words of a problem (XPS_RSA_RDM_WORDS each): 0 r (n x n), 1 ldr (>= n), 2 n, 3 out (n x n; may be
 * r), 4 ldo (>= n).  At most 65535 problems.  Refused: a null table or matrix, a negative n, ldr < n, ldo < n, a null or too
 * small workspace.
 *
 * xps_rdm_compare_perm_f64: for every pair q of matrices (A, B) with index lists ia, ib of m shared conditions and for every row
 * p of the pair's permutation table, over the upper triangle u < v in np.triu_indices order, x = A[ia[u]][ia[v]] and
 * y_p = B[ib[p[u]]][ib[p[v]]]:
 *     stats[row] = {mean_x, mean_y, sxx, syy} of x and y_identity (sums of squared deviations; cosine = 1: both means 0),
 *     cross[row][r] = sum (x - mean_x) (y_p - mean_y) for row r of the table, r = 0 .. R.
 * B must be symmetric: a relabelling then leaves the multiset of its triangle, and so mean_y and syy, unchanged.  The Pearson
 * (cosine) similarity under permutation r is cross[row][r] / (sqrt(sxx) sqrt(syy)), taken by the caller.  One wave per (pair,
 * permutation) and one per pair for the statistics: u ascending, lane l takes v = u + 1 + l, + 64, ... and adds its terms in
 * that order; the 64 partial sums meet in the butterfly of xps_silhouette_from_sums_f64.
 * Words of a pair (XPS_RSA_PAIR_WORDS each): 0 A (DEVICE, float64), 1 lda, 2 na (A is na x na), 3 the offset of ia in idx, 4 B,
 * 5 ldb, 6 nb, 7 the offset of ib in idx, 8 m, 9 its permutation table, 10 its output row.  tables: int64[2 n_tables] = {offset
 * in perms, m}; table t is perms[offset .. offset + (R + 1) m) as (R + 1, m) int32 and may be shared by every pair of that m.
 * idx (int32[n_idx]) and perms (int32[n_perm]) are HOST arrays like the tables.  stats is (n_rows, 4), cross (n_rows, R + 1),
 * DEVICE; output rows of two pairs must differ.  Refused: null tables, matrices or outputs, negative counts, lda < na, ldb < nb,
 * m < 2 or m > XPS_RSA_MAX_CONDITIONS, an index list outside idx, an index at or past the matrix size, a table outside perms or
 * of another m than its pair, a table row that is not a permutation of [0, m) (a repeated or out-of-range entry), a row 0 that
 * is not the identity, an output row outside [0, n_rows), R < 0, cosine outside 0 / 1, a null or too small workspace. */
#define XPS_RSA_STD_WORDS 8
#define XPS_RSA_RDM_WORDS 8
#define XPS_RSA_PAIR_WORDS 12
#define XPS_RSA_MAX_CONDITIONS 1024
size_t xps_row_standardize_grouped_f64_workspace(int n_problems);
int xps_row_standardize_grouped_f64(const int64_t* problems, int n_problems, void* ws, size_t ws_bytes, void* stream);
size_t xps_rdm_from_corr_grouped_f64_workspace(int n_problems);
int xps_rdm_from_corr_grouped_f64(const int64_t* problems, int n_problems, void* ws, size_t ws_bytes, void* stream);
size_t xps_rdm_compare_perm_f64_workspace(int n_pairs, int n_tables, int64_t n_idx, int64_t n_perm);
int xps_rdm_compare_perm_f64(const int64_t* pairs, int n_pairs, const int64_t* tables, int n_tables, const int32_t* idx,
                             int64_t n_idx, const int32_t* perms, int64_t n_perm, int R, int cosine, double* stats, double* cross,
                             int64_t n_rows, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Tensor maximum entropy surrogates (csrc/xps_tme.hip; surrogates/tme.py;        */
/* DESIGN.md 4.24): random tensors with a data tensor's marginal covariances.     */
/* ------------------------------------------------------------------------- */
/* Float64, no atomics; every sum is taken in an order that is a function of the problem alone, so a problem's bits do not depend
 * on the grid, the stream, the other problems of a call or the chunking of a batch.  Nothing allocates or synchronises; every
 * refusal is XPS_E_INVALID before any launch.
 *
 * xps_tme_kron_pass_f64 takes xps_gram_grouped_f64's convention: a HOST table of int64 words, checked by the call and copied into
 * ws (DEVICE, ..._workspace(n_problems) bytes) on the stream.  For every problem, with W_ijk = 1 / D_ijk and
 * D_ijk = (l0[i] + l1[j]) + l2[k] over the k0 x k1 x k2 box (never stored):
 *     w1_r[a] = sum of W over the two other axes,   w2_r[a] = the same sum of W^2            (r = 0, 1, 2)
 *     p01[i][j] = sum_k W^2,   p02[i][k] = sum_j W^2,   p12[j][k] = sum_i W^2
 *     scal[0] = sum log D,   scal[1] = the number of axis-0 slabs i that hold a D <= 0 (or NaN): 0 when every D is positive.
 * Workgroup (a, problem) owns index a of ONE axis A and walks the plane of the other two, B = A + 1 and C = A + 2 (mod 3): wave w
 * takes b = w, w + 4, ..., lane l adds its terms c = l, l + 64, ... in that order (D = (l_A[a] + l_B[b]) + l_C[c]), the 64 partial
 * sums of a row (a, b) meet in the butterfly of xps_silhouette_from_sums_f64 -- that is the pairwise marginal over (A, B): p01 for
 * A = 0, p12 for A = 1, the TRANSPOSE of p02 for A = 2 --, a wave adds its rows in ascending b and the four waves meet as
 * (w0 + w1) + (w2 + w3).  The three roles are one code path: a problem whose axes are rotated gives the rotated outputs bit for bit.
 * sum log D is taken by the role-0 workgroups in the same order and added over i by a second launch (thread t takes i = t, t + 256,
 * ... ascending; a fixed tree).  Each role evaluates 1 / D itself: three divisions per box element instead of a k0 x k1 x k2 array
 * and a cross-workgroup reduction.  Outputs of a problem with a D <= 0 hold infinities or NaN; other problems are not touched.
 * Words of a problem (XPS_TME_KRON_WORDS each): 0-2 k0 k1 k2 (1 .. XPS_TME_MAX_AXIS), 3-5 l0 l1 l2 (DEVICE), 6-8 w1_0 w1_1 w1_2,
 * 9-11 w2_0 w2_1 w2_2, 12 p01, 13 ld01 (>= k1), 14 p02, 15 ld02 (>= k2), 16 p12, 17 ld12 (>= k2), 18 scal (2 doubles).  At most
 * 65535 problems.  Refused: a null table, vector, marginal or scalar pair, a negative count, a box size outside
 * 1 .. XPS_TME_MAX_AXIS, a leading dimension below its width, a null or too small workspace.
 *
 * xps_tme_core_scale_f64: core[row][k] = z[row][k] * sqrt(1 / D_ijk) for the n_sur k0 k1 rows row = (s k0 + i) k1 + j of n_sur
 * surrogates, z with row stride ldz >= k2 and core with ldc >= k2; core may be z when ldc == ldz.  Refused: null pointers,
 * negative counts, a box size outside 1 .. XPS_TME_MAX_AXIS, ldz < k2, ldc < k2, more than 2^20 surrogates.
 *
 * xps_tme_mode_product_f64: C[b] = A[b] op(B[b]) + add for b = 0 .. batch - 1 on the f64 MFMA tile of xps_f64_tile.h, the
 * contraction ascending.  A[b] = A + b sa is M x K (element (m, k) at m lda + k); B[b] = B + b sb is K x N (element (k, n) at
 * k ldb + n), or with b_kcontig = 1 stored as N x K (element at n ldb + k); a stride of 0 shares the operand.  add (or null) is
 * M x N with ldadd, shared by the batch; C[b] = C + b sc elements with ldc, float32 when c_is_f32.  The mode products of S
 * surrogates are three calls: the middle one is batch = S k0 products on the slices where they lie.  Refused: null
 * matrices, negative sizes or strides, K < 1, lda < K, ldb below B's width, ldc < N, ldadd < N, batch outputs that overlap
 * (sc < (M - 1) ldc + N), more than 2^31 - 1 tiles. */
#define XPS_TME_KRON_WORDS 20
#define XPS_TME_MAX_AXIS 1024
size_t xps_tme_kron_pass_f64_workspace(int n_problems);
int xps_tme_kron_pass_f64(const int64_t* problems, int n_problems, void* ws, size_t ws_bytes, void* stream);
int xps_tme_core_scale_f64(const double* z, int64_t ldz, const double* l0, const double* l1, const double* l2, int k0, int k1, int k2,
                           int64_t n_sur, double* core, int64_t ldc, void* stream);
int xps_tme_mode_product_f64(const double* A, int64_t lda, int64_t sa, const double* B, int64_t ldb, int64_t sb, int b_kcontig,
                             const double* add, int64_t ldadd, void* C, int c_is_f32, int64_t ldc, int64_t sc, int64_t M, int N, int K,
                             int64_t batch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XPS_H */
