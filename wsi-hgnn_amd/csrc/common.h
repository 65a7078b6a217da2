// Shared device/host helpers for libwsi_hgnn.so (gfx950 only; wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>

#include "../../include/wsi_hgnn.h"

namespace wsi {

void set_error(const char* fmt, ...);

// Measurement switches (kernel variants, ablations, A/B knobs of tools/) exist ONLY in a library built with -DWSI_ABLATE
// (wsi_hgnn_amd.build.build_native(ablate=True) -> libwsi_hgnn_ablate.so, loaded by tools/ through _native.set_library_path).
// The product library reads no environment variable: knob() is a constant there, the variants are not instantiated, and
// tests/test_boundary.py checks that the shared object does not even import getenv.
#ifdef WSI_ABLATE
inline const char* knob(const char* name) { return getenv(name); }
#else
constexpr const char* knob(const char*) { return nullptr; }
#endif

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return WSI_EFAULT;
    }
    return WSI_OK;
}

// CALL(NV) for a row of D floats held by one wave, NV (a power of two, <= 16) per lane: column c = lane + 64 * i
#define WSI_NV_DISPATCH(D, CALL)                 \
    {                                            \
        const int nv_ = ((D) + 63) / 64;         \
        if (nv_ <= 1) { CALL(1); }               \
        else if (nv_ <= 2) { CALL(2); }          \
        else if (nv_ <= 4) { CALL(4); }          \
        else if (nv_ <= 8) { CALL(8); }          \
        else if (nv_ <= 16) { CALL(16); }        \
        else { set_error("feature width %d > 1024 unsupported", (D)); return WSI_ENOSYS; } \
    }

// ---------------------------------------------------------------- cross-lane (DPP within a 16-lane row)
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}

// Sum over aligned groups of LPH consecutive lanes; every lane of the group gets the total.
// Steps 1,2 = quad_perm, 4 = row_half_mirror, 8 = row_mirror (DPP, no LDS traffic); 16/32 cross
// the 16-lane DPP row and go through ds_bpermute (__shfl_xor).
template <int LPH>
__device__ __forceinline__ float group_sum(float x) {
    if (LPH >= 2) x += dpp_mov<0xB1>(x);   // quad_perm [1,0,3,2]
    if (LPH >= 4) x += dpp_mov<0x4E>(x);   // quad_perm [2,3,0,1]
    if (LPH >= 8) x += dpp_mov<0x141>(x);  // row_half_mirror
    if (LPH >= 16) x += dpp_mov<0x140>(x); // row_mirror
    if (LPH >= 32) x += __shfl_xor(x, 16);
    if (LPH >= 64) x += __shfl_xor(x, 32);
    return x;
}

__device__ __forceinline__ float wave_sum(float x) { return group_sum<64>(x); }

// x of the lane CTRL selects; a lane whose source lane is not active keeps its OWN x (`old` = x, no bound_ctrl).  That is the neutral element of a
// maximum, where the 0 of dpp_mov is not: group_max is the maximum over the ACTIVE lanes of the group, as group_sum is their sum.
template <int CTRL>
__device__ __forceinline__ int dpp_self(int x) { return __builtin_amdgcn_update_dpp(x, x, CTRL, 0xf, 0xf, false); }
template <int CTRL>
__device__ __forceinline__ float dpp_self(float x) { return __int_as_float(dpp_self<CTRL>(__float_as_int(x))); }

__device__ __forceinline__ float lane_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ int lane_max(int a, int b) { return max(a, b); }

// Maximum (float or int) over aligned groups of G consecutive lanes, the steps of group_sum; every lane of the group gets it.
// A maximum is exact in any order.
template <int G, typename T>
__device__ __forceinline__ T group_max(T x) {
    if (G >= 2) x = lane_max(x, dpp_self<0xB1>(x));
    if (G >= 4) x = lane_max(x, dpp_self<0x4E>(x));
    if (G >= 8) x = lane_max(x, dpp_self<0x141>(x));
    if (G >= 16) x = lane_max(x, dpp_self<0x140>(x));
    if (G >= 32) x = lane_max(x, __shfl_xor(x, 16));
    if (G >= 64) x = lane_max(x, __shfl_xor(x, 32));
    return x;
}

template <typename T>
__device__ __forceinline__ T wave_max(T x) { return group_max<64>(x); }

__device__ __forceinline__ float leaky_relu(float v, float slope) { return v > 0.f ? v : v * slope; }

// The row of this wave in a grid of WAVES-wave workgroups that gives every row a wave (wave-uniform, in a scalar register); -1 beyond n.
template <int WAVES>
__device__ __forceinline__ int row_of_wave(int n) {
    int w = (int)blockIdx.x * WAVES + (int)(threadIdx.x >> 6);
    w = __builtin_amdgcn_readfirstlane(w);
    return w < n ? w : -1;
}

// Bijective workgroup remap: workgroup b of n runs on XCD b % 8; remapped, each XCD takes one contiguous eighth of the work.
__device__ __forceinline__ int xcd_remap(int b, int n) {
    const int q = n >> 3, r = n & 7;
    const int xcd = b & 7, idx = b >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// ---------------------------------------------------------------- workgroup scans (256 threads) and the descriptor-row search
// Compaction everywhere in the library is a two-level scan and never an atomic, so the compacted order is the input order, run after run:
// tiles of 1024 elements write their sums, ONE workgroup scans the tile sums (launch_tile_scan), the tiles scan again and scatter.

// Exclusive prefix of a 0/1 flag over the 256 lanes of the workgroup (ballot + popcount per wave, the 4 wave totals through LDS); `total` = their sum.
// 256 threads, two barriers; `lds` holds 4 ints and may be reused by the next call (the second barrier guards it).
__device__ __forceinline__ int block_flag_scan(bool flag, int* lds, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    const int excl = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) lds[w] = __popcll(b);
    __syncthreads();
    const int t0 = lds[0], t1 = lds[1], t2 = lds[2], t3 = lds[3];
    __syncthreads();
    total = t0 + t1 + t2 + t3;
    return excl + (w > 0 ? t0 : 0) + (w > 1 ? t1 : 0) + (w > 2 ? t2 : 0);
}

// Inclusive prefix of x over the 256 lanes of the workgroup (__shfl_up ladder per wave, the 4 wave totals through LDS); `total` = the workgroup's sum.
// The same preconditions: 256 threads, two barriers, 4 ints of `lds` that the next call may reuse.
__device__ __forceinline__ int block_scan_inclusive(int x, int* lds, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    const int t0 = lds[0], t1 = lds[1], t2 = lds[2], t3 = lds[3];
    __syncthreads();
    total = t0 + t1 + t2 + t3;
    return x + (w > 0 ? t0 : 0) + (w > 1 ? t1 : 0) + (w > 2 ? t2 : 0);
}

// Last of n descriptor rows (`stride` int64 words each) whose word `col` - the row's first tile - is <= b.  Rows without elements own no tile and
// are never found.
__device__ __forceinline__ int find_row(const int64_t* __restrict__ rows, int stride, int col, int n, int b) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rows[(int64_t)mid * stride + col] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The middle level (segment_table.hip), one workgroup for any number of tiles: tile_sum[0 .. ntiles) -> its exclusive prefix in place,
// tile_sum[ntiles] = the total (the array holds ntiles + 1 words); with nseg > 0 also counts[s] = elements kept in segment s, whose first tile is
// word `col` of row s of `rows` (`stride` int64 words per row).
void launch_tile_scan(int32_t* tile_sum, int ntiles, const int64_t* rows, int stride, int col, int nseg, int32_t* counts, hipStream_t st);

// ---------------------------------------------------------------- counter-based draws: a 32-bit hash of (index, sub-seed)
__host__ __device__ __forceinline__ uint32_t drop_fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__host__ __device__ __forceinline__ uint32_t index_hash(uint32_t i, uint32_t sub) { return drop_fmix32(i * 0x9E3779B1u + sub); }
// element i is drawn with probability thr / 65536 (the transforms' draw rule: include/wsi_hgnn.h, wsi_augment_*)
__host__ __device__ __forceinline__ bool drawn(uint32_t i, uint32_t sub, uint32_t thr) { return (index_hash(i, sub) & 0xffffu) < thr; }

// dropout (WSI_EPI_DROPOUT; the contract is in include/wsi_hgnn.h): one hash decides a pair of columns
__host__ __device__ __forceinline__ uint32_t drop_pair_hash(uint32_t row, uint32_t pair, uint32_t pairs_per_row, uint32_t seed) {
    return index_hash(row * pairs_per_row + pair, seed);
}
// factor (scale or 0) of element (row, col) of the masked tensor
__device__ __forceinline__ float drop_factor1(uint32_t row, uint32_t col, uint32_t pairs, uint32_t seed, uint32_t thr, float scale) {
    const uint32_t h = drop_pair_hash(row, col >> 1, pairs, seed);
    return (((col & 1u) ? (h >> 16) : (h & 0xffffu)) >= thr) ? scale : 0.f;
}
// the four factors of columns col .. col + 3 of one row (col % 4 == 0): two hashes
__device__ __forceinline__ float4 drop_factor4(uint32_t row, uint32_t col, uint32_t pairs, uint32_t seed, uint32_t thr, float scale) {
    const uint32_t h0 = drop_pair_hash(row, col >> 1, pairs, seed), h1 = drop_pair_hash(row, (col >> 1) + 1, pairs, seed);
    return make_float4((h0 & 0xffffu) >= thr ? scale : 0.f, (h0 >> 16) >= thr ? scale : 0.f, (h1 & 0xffffu) >= thr ? scale : 0.f, (h1 >> 16) >= thr ? scale : 0.f);
}
// the draw of this launch: the group's seed + the device word, read ONCE per epilogue into `wsi_drop_seed` (WSI_DROP_SEED), which the two macros use
#define WSI_DROP_SEED(G, epi) const uint32_t wsi_drop_seed = (((epi) & WSI_EPI_DROPOUT) && (G).drop_seed_base) ? (G).drop_seed + *(G).drop_seed_base : (G).drop_seed
#define WSI_DROP4(G, row_in_group, col_in_group) drop_factor4((uint32_t)((G).drop_row0 + (row_in_group)), (uint32_t)((G).drop_col0 + (col_in_group)), (G).drop_pairs, wsi_drop_seed, (G).drop_thr, (G).drop_scale)
#define WSI_DROP1(G, row_in_group, col_in_group) drop_factor1((uint32_t)((G).drop_row0 + (row_in_group)), (uint32_t)((G).drop_col0 + (col_in_group)), (G).drop_pairs, wsi_drop_seed, (G).drop_thr, (G).drop_scale)

// ---------------------------------------------------------------- host: may a pointer (and its row stride, in floats) take 16-byte accesses
// (a null pointer counts as aligned: optional operands pass)
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool vec_ok(const void* p, int64_t ld) { return aligned16(p) && ld % 4 == 0; }

// ---------------------------------------------------------------- four consecutive floats
// columns col .. col + 3 of a D-wide row, at p; beyond D: 0 / not written.  vec: p may take a 16-byte access.
__device__ __forceinline__ void load4_tail(float (&v)[4], const float* __restrict__ p, int col, int D, bool vec) {
    if (vec && col + 3 < D) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (col + i < D) ? p[i] : 0.f;
    }
}

__device__ __forceinline__ void store4_tail(float* __restrict__ p, const float (&v)[4], int col, int D, bool vec) {
    if (vec && col + 3 < D) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (col + i < D) p[i] = v[i];
    }
}

// 4 consecutive floats starting at p (logical index i0 of a dimension of extent n); zero beyond n. Scalar, any alignment.
__device__ __forceinline__ float4 load4_guarded(const float* __restrict__ p, int i0, int n) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i0 + 0 < n) r.x = p[0];
    if (i0 + 1 < n) r.y = p[1];
    if (i0 + 2 < n) r.z = p[2];
    if (i0 + 3 < n) r.w = p[3];
    return r;
}

// ---------------------------------------------------------------- one attention head's rows in LDS (D floats each, 16-byte aligned)
// <a, b>: a in registers, b a staged row
template <int D>
__device__ __forceinline__ float dot4(const float (&a)[D], const float* __restrict__ b) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < D; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(b + c);
        acc = fmaf(a[c], v.x, acc); acc = fmaf(a[c + 1], v.y, acc); acc = fmaf(a[c + 2], v.z, acc); acc = fmaf(a[c + 3], v.w, acc);
    }
    return acc;
}

// rows [n, D] of one head's column block (src points at its first column of the first row, row stride ld) -> LDS, by a workgroup of THREADS
template <int D, int THREADS>
__device__ __forceinline__ void stage_rows(float* __restrict__ dst, const float* __restrict__ src, int64_t ld, int n) {
    for (int i = threadIdx.x; i < n * (D / 4); i += THREADS) {
        const int row = i / (D / 4), c = (i - row * (D / 4)) * 4;
        *reinterpret_cast<float4*>(dst + row * D + c) = *reinterpret_cast<const float4*>(src + (int64_t)row * ld + c);
    }
}

// ---------------------------------------------------------------- V contiguous floats per lane
template <int V>
__device__ __forceinline__ void load_vec(float (&r)[V], const float* __restrict__ p) {
    if constexpr (V % 4 == 0) {
#pragma unroll
        for (int i = 0; i < V / 4; ++i) {
            const float4 t = reinterpret_cast<const float4*>(p)[i];
            r[4 * i + 0] = t.x; r[4 * i + 1] = t.y; r[4 * i + 2] = t.z; r[4 * i + 3] = t.w;
        }
    } else if constexpr (V == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        r[0] = t.x; r[1] = t.y;
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) r[i] = p[i];
    }
}

template <int V>
__device__ __forceinline__ void store_vec(float* __restrict__ p, const float (&r)[V]) {
    if constexpr (V % 4 == 0) {
#pragma unroll
        for (int i = 0; i < V / 4; ++i)
            reinterpret_cast<float4*>(p)[i] = make_float4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
    } else if constexpr (V == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(r[0], r[1]);
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) p[i] = r[i];
    }
}

}  // namespace wsi
