// The row-group layout of the gather kernels (gat_attn.hip, ra_attn.hip, gin.hip): a GROUP of G lanes (4 <= G <= 64, a power of two) owns
// one row, lane l of the group holds the VEC-wide column chunks c = VEC * (l + G * k), k < NK, and BLOCK / G rows share a workgroup, so a
// narrow row (32 floats: G = 8) leaves no lane idle.  A chunk past the row's width is skipped by its lane (loads and stores), while the
// group's reductions still run on all G lanes: whether a group has a row at all is group-uniform.
#pragma once
#include "common.h"

namespace wsi {

struct RowCfg { int G, VEC, NK; };

// The layout of a row of `width` floats made of units of `unit` floats that no chunk may straddle (a head; the whole row without heads).
// VEC = 4 when every pointer and stride allows 16-byte accesses (vec4_ok) and unit % 4 == 0; G = the smallest power of two (>= 4,
// >= min_lanes, <= 64) that covers the row's chunks; NK = the power of two of chunks per lane that covers the rest.
// (tests/row_group_cases.py restates this rule; tests/test_row_group.py holds the two against each other)
inline RowCfg row_cfg(int width, int unit, int min_lanes, bool vec4_ok) {
    RowCfg c;
    c.VEC = (vec4_ok && unit % 4 == 0) ? 4 : 1;
    const int chunks = width / c.VEC;
    c.G = 4;
    while (c.G < 64 && (c.G < chunks || c.G < min_lanes)) c.G <<= 1;
    const int need = (chunks + c.G - 1) / c.G;
    c.NK = 1;
    while (c.NK < need) c.NK <<= 1;
    return c;
}

// Every (G, VEC, NK) row_cfg can give: NARROW for a width up to 1024, WIDE the four further ones up to 4096.  X is handed to each entry.
#define ROW_GROUP_CASES(NARROW, WIDE, X)                                                                \
    NARROW(X, 4, 4, 1)   NARROW(X, 8, 4, 1)   NARROW(X, 16, 4, 1)  NARROW(X, 32, 4, 1)  NARROW(X, 64, 4, 1)  \
    NARROW(X, 64, 4, 2)  NARROW(X, 64, 4, 4)  WIDE(X, 64, 4, 8)    WIDE(X, 64, 4, 16)                        \
    NARROW(X, 4, 1, 1)   NARROW(X, 8, 1, 1)   NARROW(X, 16, 1, 1)  NARROW(X, 32, 1, 1)  NARROW(X, 64, 1, 1)  \
    NARROW(X, 64, 1, 2)  NARROW(X, 64, 1, 4)  NARROW(X, 64, 1, 8)  NARROW(X, 64, 1, 16)                      \
    WIDE(X, 64, 1, 32)   WIDE(X, 64, 1, 64)

#define ROW_GROUP_CASE_(CALL, G_, V_, K_) case V_ * 100000 + G_ * 100 + K_: CALL(G_, V_, K_); break;
#define ROW_GROUP_NONE_(CALL, G_, V_, K_)
#define ROW_GROUP_SWITCH_(who, cfg, CALL, WIDE)                                                                       \
    do {                                                                                                              \
        switch ((cfg).VEC * 100000 + (cfg).G * 100 + (cfg).NK) {                                                      \
            ROW_GROUP_CASES(ROW_GROUP_CASE_, WIDE, CALL)                                                              \
            default: set_error(who ": no kernel for G=%d VEC=%d NK=%d", (cfg).G, (cfg).VEC, (cfg).NK); return WSI_ENOSYS; \
        }                                                                                                             \
    } while (0)
// CALL(G, VEC, NK) of the instantiation cfg names, inside a function that returns a WSI_* code; `who` starts the error text.
// NARROW instantiates the 16 narrow cases only, ALL the 20.
#define ROW_GROUP_DISPATCH_NARROW(who, cfg, CALL) ROW_GROUP_SWITCH_(who, cfg, CALL, ROW_GROUP_NONE_)
#define ROW_GROUP_DISPATCH_ALL(who, cfg, CALL) ROW_GROUP_SWITCH_(who, cfg, CALL, ROW_GROUP_CASE_)

// ---------------------------------------------------------------- device side
// first column of chunk k of lane gl of a group
template <int G, int VEC>
__device__ __forceinline__ int chunk_col(int gl, int k) { return VEC * (gl + G * k); }

// this lane within its group, the group's first lane within the wave (for __shfl), and the group's row in a grid of BLOCK-thread workgroups
template <int G>
__device__ __forceinline__ int group_lane() { return threadIdx.x & (G - 1); }
template <int G>
__device__ __forceinline__ int group_base() { return threadIdx.x & 63 & ~(G - 1); }
template <int G, int BLOCK>
__device__ __forceinline__ int group_row() { return (int)blockIdx.x * (BLOCK / G) + (int)threadIdx.x / G; }

template <int NK, int VEC>
__device__ __forceinline__ void zero_chunks(float (&a)[NK][VEC]) {
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int j = 0; j < VEC; ++j) a[k][j] = 0.f;
}

}  // namespace wsi
