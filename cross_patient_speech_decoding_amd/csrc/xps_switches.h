// The library's run-time switches: ONE table (rows in xps_api.hip: environment name, default, range, parse rule), filled from
// the environment once, on first access; afterwards a switch is one relaxed atomic load and changes only through
// xps_set_switch (include/xps.h) or one of the four older setter pairs, which are views of their rows.
#pragma once

namespace xps_sw {

enum Id {
    GEMM_PRECISION,           // 0 = fp32 MFMA, 1 = bf16 split products
    GEMM_SMALL_TILE_BLOCKS,   // 64-row tiles below this many 128-row tiles
    GEMM_LONGK_128,           // long contractions keep the 128-row tile
    GEMM_BIG,                 // 256 x 256 tiles
    GEMM_DMA,                 // LDS-DMA k loops on split4 operands
    PROJ_WS,                  // weight-stationary projection kernel
    GEMM_BIG_DEEP,            // 32-deep stages of the 256-tile kernels
    GEMM_BIG_MIN_TILES,       // fewest 256-tiles that take the 256-tile kernels
    GEMM_BIG_TAIL,            // trailing rows of a ragged last round go to the 128-tile kernels
    TN_BLOCKS,                // block target of the grouped weight-gradient launch
    TN_UNIFORM,               // one split count for a group of equal k
    GEMM_BIG_DEEP_TN,         // 32-deep stages in the weight-gradient form as well
    TN_REDUCE,                // 0 = by split count, 1 = flat, 2 = looped
    GRU_STEP_PATH,            // per-step GEMM kernels for H > 128 outside the cluster path
    GRU_CLUSTER,              // 0 = off, 1 = one step per launch, 2 = persistent
    GRU_CL_CUS,               // plan the cluster kernels for at most this many CUs (0: all)
    GRU_CL2,                  // 4 x 4 BPTT grid
    GRU_XIMG,                 // forward kernel exchanges through the split4 image of y_ext
    GRU_XOUT,                 // 1-D BPTT kernel exchanges through its own outputs
    COUNT
};

long long get(Id id);
void store(Id id, long long value);      // (no range check: for setters that have validated the value themselves)
inline bool on(Id id) { return get(id) != 0; }

}  // namespace xps_sw
