// Train-time graph augmentation on the device (wsi_hgnn_amd/transforms.py; the reference: data.py:16-23 - DropNode, DropEdge, NodeShuffle, FeatMask
// through dgl.transforms).  Contract and draw rule: include/wsi_hgnn.h (wsi_augment_*).  Every decision is a hash of (sub-seed, element index), so
// flags are RECOMPUTED wherever they are needed instead of stored; output positions come from the two-level scans of common.h (never atomics).
#include "common.h"

namespace wsi {

constexpr int AUG_TILE = 1024;            // elements per workgroup: 4 rounds of 256 lanes
constexpr int AUG_NROW = 6;               // int64 words per node-segment descriptor: n, off, first_tile, seed, thr, quota + 1 (0: none)
constexpr int AUG_EROW = 14;              // ... per edge segment: n, off, first_tile, u, v, sim, src_off, dst_off, seed, thr, mode, n_src, n_dst, quota + 1

// the survivor quota of a row from its last word (quota + 1; 0 = no quota): ranks at or beyond it are truncated
__device__ __forceinline__ int aug_quota(int64_t w) { return w > 0 && w - 1 < INT32_MAX ? (int)(w - 1) : INT32_MAX; }

// ---------------------------------------------------------------- nodes
// pass 0: tile_sum[tile] = kept nodes of the tile;  pass 1 (after the scan): new_id / kept.  A row with a quota keeps the first `quota` of
// its survivors (node-id order): the others get new_id -1 as if drawn, and the segment's first tile clamps counts[s] - the tile sums stay
// those of the draw, so every rank is the untruncated one.
template <int PASS>
__global__ __launch_bounds__(256) void aug_nodes_kernel(const int64_t* __restrict__ desc, int nseg, int32_t* __restrict__ tile_sum,
                                                        int32_t* __restrict__ new_id, int64_t* __restrict__ kept, int32_t* __restrict__ counts) {
    __shared__ int lds[4];
    const int b = blockIdx.x;
    const int seg = find_row(desc, AUG_NROW, 2, nseg, b);
    const int64_t* d = desc + (int64_t)seg * AUG_NROW;
    const int64_t n = d[0], off = d[1];
    const int ft = (int)d[2];
    const uint32_t seed = (uint32_t)d[3], thr = (uint32_t)d[4];
    const int quota = aug_quota(d[5]);
    const int64_t i0 = (int64_t)(b - ft) * AUG_TILE;
    int run = PASS == 1 ? tile_sum[b] - tile_sum[ft] : 0;      // position inside the type's compacted range
    for (int r = 0; r < AUG_TILE / 256; ++r) {
        const int64_t i = i0 + r * 256 + threadIdx.x;
        const bool keep = i < n && !drawn((uint32_t)i, seed, thr);
        int total;
        const int excl = block_flag_scan(keep, lds, total);
        if (PASS == 1 && i < n) {
            const bool stay = keep && run + excl < quota;
            new_id[off + i] = stay ? run + excl : -1;
            if (stay) kept[off + run + excl] = i;
        }
        run += total;
    }
    if (PASS == 0 && threadIdx.x == 0) tile_sum[b] = run;
    if (PASS == 1 && b == ft && threadIdx.x == 0 && counts[seg] > quota) counts[seg] = quota;
}

// ---------------------------------------------------------------- edges
// stage 1 flag of edge i of a relation: both endpoints kept (new_id, NULL = all kept) and, with mode 0, not drawn by its own index
__device__ __forceinline__ bool aug_edge_flag1(const int64_t* d, const int32_t* __restrict__ new_id, int64_t i, int64_t& u, int64_t& v) {
    u = reinterpret_cast<const int64_t*>(d[3])[i];
    v = reinterpret_cast<const int64_t*>(d[4])[i];
    bool f = u >= 0 && u < d[11] && v >= 0 && v < d[12];          // an endpoint outside its node type indexes nothing: the edge goes
    if (f && new_id) {
        f = new_id[d[6] + u] >= 0 && new_id[d[7] + v] >= 0;
        if (f) { u = new_id[d[6] + u]; v = new_id[d[7] + v]; }
    }
    if (d[10] == 0) f = f && !drawn((uint32_t)i, (uint32_t)d[8], (uint32_t)d[9]);
    return f;
}

// pass 0: tile sums of stage 1;  pass 1: rank1[e] = rank of e among the stage-1 survivors of its relation (-1: gone), tile sums of stage 2
// (mode 1: the survivor is drawn BY THAT RANK - its index in the graph DropEdge receives behind DropNode);  pass 2: stable scatter.
// A row with a quota keeps the first `quota` of its final survivors; pass 2 then leaves the FINAL decision in rank1 (-1: gone, by either draw
// or by the quota) for csrc/slot_aug.hip, and the segment's first tile clamps counts[s].
template <int PASS>
__global__ __launch_bounds__(256) void aug_edges_kernel(const int64_t* __restrict__ desc, int nseg, int ntiles, const int32_t* __restrict__ new_id,
                                                        int32_t* __restrict__ tile_sum, int32_t* __restrict__ rank1,
                                                        int64_t* __restrict__ out_u, int64_t* __restrict__ out_v, float* __restrict__ out_sim,
                                                        int64_t* __restrict__ out_eid, int32_t* __restrict__ counts) {
    __shared__ int lds[4];
    const int b = blockIdx.x;
    const int seg = find_row(desc, AUG_EROW, 2, nseg, b);
    const int64_t* d = desc + (int64_t)seg * AUG_EROW;
    const int quota = aug_quota(d[13]);
    const int64_t n = d[0], off = d[1];
    const int ft = (int)d[2];
    const uint32_t seed = (uint32_t)d[8], thr = (uint32_t)d[9];
    const bool by_rank = d[10] != 0;
    const float* sim = reinterpret_cast<const float*>(d[5]);
    int32_t* sum1 = tile_sum;                     // [ntiles + 1]
    int32_t* sum2 = tile_sum + ntiles + 1;        // [ntiles + 1]
    const int64_t i0 = (int64_t)(b - ft) * AUG_TILE;
    int run = PASS == 1 ? sum1[b] - sum1[ft] : (PASS == 2 ? sum2[b] - sum2[ft] : 0);
    int cnt2 = 0;
    for (int r = 0; r < AUG_TILE / 256; ++r) {
        const int64_t i = i0 + r * 256 + threadIdx.x;
        int64_t u = 0, v = 0;
        bool f;
        if (PASS == 2) {
            const int rk = i < n ? rank1[off + i] : -1;
            f = rk >= 0 && !(by_rank && drawn((uint32_t)rk, seed, thr));
        } else {
            f = i < n && aug_edge_flag1(d, new_id, i, u, v);
        }
        int total;
        const int excl = block_flag_scan(f, lds, total);
        if (PASS == 1) {
            const int rk = f ? run + excl : -1;
            if (i < n) rank1[off + i] = rk;
            const bool f2 = f && !(by_rank && drawn((uint32_t)rk, seed, thr));
            cnt2 += __popcll(__ballot(f2));       // per wave; summed over the 4 waves below
        }
        if (PASS == 2 && d[13] > 0 && i < n && !(f && run + excl < quota)) rank1[off + i] = -1;
        if (PASS == 2 && f && run + excl < quota) {
            aug_edge_flag1(d, new_id, i, u, v);   // the renumbered endpoints (its flag is known to hold)
            const int64_t p = off + run + excl;
            out_u[p] = u;
            out_v[p] = v;
            out_eid[p] = i;
            if (sim) out_sim[p] = sim[i];
        }
        run += total;
    }
    if (PASS == 0 && threadIdx.x == 0) sum1[b] = run;
    if (PASS == 1) {
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = cnt2;
        __syncthreads();
        if (threadIdx.x == 0) sum2[b] = lds[0] + lds[1] + lds[2] + lds[3];
    }
    if (PASS == 2 && b == ft && threadIdx.x == 0 && counts[seg] > quota) counts[seg] = quota;
}

// ---------------------------------------------------------------- NodeShuffle keys: (segment << 32) | hash, one stable sort orders every type at once
__global__ __launch_bounds__(256) void aug_keys_kernel(const int64_t* __restrict__ desc, int nseg, int64_t* __restrict__ keys) {
    const int b = blockIdx.x;
    const int s = find_row(desc, AUG_NROW, 2, nseg, b);
    const int64_t* d = desc + (int64_t)s * AUG_NROW;
    const int64_t n = d[0], off = d[1];
    const int64_t i0 = (int64_t)(b - (int)d[2]) * AUG_TILE;
#pragma unroll
    for (int r = 0; r < AUG_TILE / 256; ++r) {
        const int64_t i = i0 + r * 256 + threadIdx.x;
        if (i < n) keys[off + i] = ((int64_t)s << 32) | (int64_t)index_hash((uint32_t)i, (uint32_t)d[3]);
    }
}

// ---------------------------------------------------------------- fused feature gather: out[i, c] = colkeep(c) ? x[row_of[i], c] : 0
// One wave per output row, 16 bytes per lane and access: a 1024-wide row is four independent 1 KiB loads in flight per wave, then four stores.
// The column mask is a function of (seed, column): each lane hashes ITS columns once, before the row loop (bit 4k + j of `bits`: column
// 4 (lane + 64 k) + j is zeroed), for the first 8 column groups (2048 columns); wider rows hash again per row.
__device__ __forceinline__ uint32_t aug_col_bits(int c, int F, uint32_t seed, uint32_t thr) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (c + j < F && drawn((uint32_t)(c + j), seed, thr)) m |= 1u << j;
    return m;
}

template <bool VEC>
__global__ __launch_bounds__(256) void aug_gather_kernel(const float* __restrict__ x, int64_t ldx, int64_t src_rows, const int64_t* __restrict__ row_of,
                                                         float* __restrict__ out, int64_t ldo, int64_t rows, int F, uint32_t seed, uint32_t thr) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    if (VEC) {
        uint32_t bits = 0;
        if (thr)
            for (int k = 0; k < 8 && 4 * (lane + 64 * k) < F; ++k) bits |= aug_col_bits(4 * (lane + 64 * k), F, seed, thr) << (4 * k);
        for (int64_t i = wave; i < rows; i += nwaves) {
            const int64_t r = row_of ? row_of[i] : i;
            const bool ok = r >= 0 && r < src_rows;                  // an index outside the table reads nothing: the row is zeros
            const float4* __restrict__ xr = reinterpret_cast<const float4*>(x + (ok ? r : 0) * ldx);
            float4* __restrict__ orow = reinterpret_cast<float4*>(out + i * ldo);
            for (int k0 = 0; 4 * (lane + 64 * k0) < F; k0 += 4) {
                float4 t[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c4 = lane + 64 * (k0 + k);
                    t[k] = (ok && 4 * c4 < F) ? xr[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c4 = lane + 64 * (k0 + k);
                    if (4 * c4 >= F) break;
                    const uint32_t m = !thr ? 0u : (k0 + k < 8 ? (bits >> (4 * (k0 + k))) & 15u : aug_col_bits(4 * c4, F, seed, thr));
                    if (m & 1u) t[k].x = 0.f;
                    if (m & 2u) t[k].y = 0.f;
                    if (m & 4u) t[k].z = 0.f;
                    if (m & 8u) t[k].w = 0.f;
                    orow[c4] = t[k];
                }
            }
        }
    } else {
        // tail path: widths that are no multiple of 4 (or rows that are not 16-byte aligned): one element per lane and access
        for (int64_t i = wave; i < rows; i += nwaves) {
            const int64_t r = row_of ? row_of[i] : i;
            const bool ok = r >= 0 && r < src_rows;
            const float* __restrict__ xr = x + (ok ? r : 0) * ldx;
            float* __restrict__ orow = out + i * ldo;
            for (int c = lane; c < F; c += 64)
                orow[c] = (ok && !(thr && drawn((uint32_t)c, seed, thr))) ? xr[c] : 0.f;
        }
    }
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_augment_nodes(const int64_t* desc, int32_t nseg, int32_t ntiles, int32_t* tile_sum, int32_t* new_id, int64_t* kept,
                                 int32_t* counts, void* stream) {
    if (nseg < 0 || ntiles < 0) { set_error("augment_nodes: bad argument"); return WSI_EINVAL; }
    if (nseg == 0) return WSI_OK;
    if (!desc || !tile_sum || !counts || (ntiles > 0 && (!new_id || !kept))) { set_error("augment_nodes: null pointer"); return WSI_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    if (ntiles > 0) hipLaunchKernelGGL(aug_nodes_kernel<0>, dim3(ntiles), dim3(256), 0, s, desc, (int)nseg, tile_sum, new_id, kept, counts);
    launch_tile_scan(tile_sum, (int)ntiles, desc, AUG_NROW, 2, (int)nseg, counts, s);
    if (ntiles > 0) hipLaunchKernelGGL(aug_nodes_kernel<1>, dim3(ntiles), dim3(256), 0, s, desc, (int)nseg, tile_sum, new_id, kept, counts);
    return check_launch("augment_nodes");
}

extern "C" int wsi_augment_edges(const int64_t* desc, int32_t nseg, int32_t ntiles, const int32_t* new_id, int32_t* tile_sum, int32_t* rank1,
                                 int64_t* out_u, int64_t* out_v, float* out_sim, int64_t* out_eid, int32_t* counts, void* stream) {
    if (nseg < 0 || ntiles < 0) { set_error("augment_edges: bad argument"); return WSI_EINVAL; }
    if (nseg == 0) return WSI_OK;
    if (!desc || !tile_sum || !counts || (ntiles > 0 && (!rank1 || !out_u || !out_v || !out_sim || !out_eid))) {
        set_error("augment_edges: null pointer");
        return WSI_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    int32_t* sum2 = tile_sum + ntiles + 1;
    if (ntiles > 0) hipLaunchKernelGGL(aug_edges_kernel<0>, dim3(ntiles), dim3(256), 0, s, desc, (int)nseg, (int)ntiles, new_id, tile_sum, rank1, out_u, out_v, out_sim, out_eid, counts);
    launch_tile_scan(tile_sum, (int)ntiles, desc, AUG_EROW, 2, (int)nseg, counts, s);
    if (ntiles > 0) hipLaunchKernelGGL(aug_edges_kernel<1>, dim3(ntiles), dim3(256), 0, s, desc, (int)nseg, (int)ntiles, new_id, tile_sum, rank1, out_u, out_v, out_sim, out_eid, counts);
    launch_tile_scan(sum2, (int)ntiles, desc, AUG_EROW, 2, (int)nseg, counts, s);
    if (ntiles > 0) hipLaunchKernelGGL(aug_edges_kernel<2>, dim3(ntiles), dim3(256), 0, s, desc, (int)nseg, (int)ntiles, new_id, tile_sum, rank1, out_u, out_v, out_sim, out_eid, counts);
    return check_launch("augment_edges");
}

extern "C" int wsi_augment_keys(const int64_t* desc, int32_t nseg, int32_t ntiles, int64_t* keys, void* stream) {
    if (nseg < 0 || ntiles < 0) { set_error("augment_keys: bad argument"); return WSI_EINVAL; }
    if (nseg == 0 || ntiles == 0) return WSI_OK;
    if (!desc || !keys) { set_error("augment_keys: null pointer"); return WSI_EINVAL; }
    hipLaunchKernelGGL(aug_keys_kernel, dim3(ntiles), dim3(256), 0, (hipStream_t)stream, desc, (int)nseg, keys);
    return check_launch("augment_keys");
}

extern "C" int wsi_gather_rows_masked(const float* x, int64_t ldx, int64_t src_rows, const int64_t* row_of, float* out, int64_t ldo, int64_t rows,
                                      int32_t F, uint32_t mask_seed, uint32_t mask_threshold, void* stream) {
    if (rows < 0 || src_rows < 0 || F < 0 || mask_threshold > 65536u) { set_error("gather_rows_masked: bad argument"); return WSI_EINVAL; }
    if (rows == 0 || F == 0) return WSI_OK;
    if (!x && src_rows > 0) { set_error("gather_rows_masked: null pointer"); return WSI_EINVAL; }
    if (!out || (!row_of && rows > src_rows)) { set_error("gather_rows_masked: null pointer"); return WSI_EINVAL; }
    if (ldx < F || ldo < F) { set_error("gather_rows_masked: row stride below the width"); return WSI_EINVAL; }
    const bool vec = F % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const int64_t blocks = (rows + 3) / 4;
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048));
    if (vec) hipLaunchKernelGGL(aug_gather_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, src_rows, row_of, out, ldo, rows, (int)F, mask_seed, mask_threshold);
    else hipLaunchKernelGGL(aug_gather_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, src_rows, row_of, out, ldo, rows, (int)F, mask_seed, mask_threshold);
    return check_launch("gather_rows_masked");
}
