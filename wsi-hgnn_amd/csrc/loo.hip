// Leave-one-node-out batches on the device (graph.leave_one_out_batch; the GEM explainers of explainers/gem.py run the model on the graph without
// node r, once per node).  Contract: include/wsi_hgnn.h (wsi_loo_*).  Copy b of the batch is the graph without node r_b of ONE node type t; a
// descriptor row is one (relation, copy) pair, the flag of an edge is two compares, and output positions come from a two-level exclusive scan
// (tile sums -> one block scans them -> tiles scatter), never from atomics: survivors keep the input order, run after run.  The host knows every
// copy's surviving count in advance (graph.leave_one_out_tables), so a row's output offset `off` is exact and the rows of a relation tile its output
// range without gaps: the relation-major, copy-major layout of graph.batch.  `cap` (the predicted count) bounds every write of a row.
#include "gemm_common.h"

namespace wsi {

constexpr int LOO_TILE = 1024;            // elements per workgroup: 4 rounds of 256 lanes
constexpr int LOO_EROW = 12;              // int64 words per edge row: n, off, first_tile, u, v, sim, r_src, r_dst, add_src, add_dst, cap, -
constexpr int LOO_NROW = 6;               // ... per node-type row: n (= B * per), off, first_tile, per, is_t, -

// last row whose first tile is <= b (rows without elements own no tile and are never found)
__device__ __forceinline__ int loo_find_row(const int64_t* __restrict__ desc, int row, int nrow, int b) {
    int lo = 0, hi = nrow - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(int64_t)mid * row + 2] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// exclusive prefix of a 0/1 flag over the 256 lanes of the workgroup (ballot + popcount per wave, the 4 wave totals through LDS); `total` = their sum.
// Two barriers; `lds` holds 4 ints and may be reused by the next call (the second barrier guards it).
__device__ __forceinline__ int loo_flag_scan(bool flag, int* lds, int& total) {
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

// ---------------------------------------------------------------- scan of the tile sums (one workgroup, any number of tiles)
// tile_sum[0 .. ntiles) -> exclusive prefix in place, tile_sum[ntiles] = total; counts[s] = survivors of row s.
__global__ __launch_bounds__(256) void loo_scan_tiles_kernel(int32_t* __restrict__ tile_sum, int ntiles, const int64_t* __restrict__ desc, int nrow,
                                                             int32_t* __restrict__ counts) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < ntiles; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < ntiles ? tile_sum[i] : 0;
        int x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        const int t0 = wsum[0], t1 = wsum[1], t2 = wsum[2], t3 = wsum[3];
        __syncthreads();
        const int before = (w > 0 ? t0 : 0) + (w > 1 ? t1 : 0) + (w > 2 ? t2 : 0);
        if (i < ntiles) tile_sum[i] = carry + before + x - v;
        carry += t0 + t1 + t2 + t3;
    }
    if (threadIdx.x == 0) tile_sum[ntiles] = carry;
    __syncthreads();                      // the prefix is read back below by other lanes of this workgroup
    for (int s = threadIdx.x; s < nrow; s += 256) {
        const int a = (int)desc[(int64_t)s * LOO_EROW + 2];
        const int b = s + 1 < nrow ? (int)desc[(int64_t)(s + 1) * LOO_EROW + 2] : ntiles;
        counts[s] = tile_sum[b] - tile_sum[a];
    }
}

// ---------------------------------------------------------------- edges
// pass 0: tile_sum[tile] = survivors of the tile;  pass 1 (after the scan): stable scatter of the renumbered survivors
template <int PASS>
__global__ __launch_bounds__(256) void loo_edges_kernel(const int64_t* __restrict__ desc, int nrow, int32_t* __restrict__ tile_sum,
                                                        int64_t* __restrict__ out_u, int64_t* __restrict__ out_v, float* __restrict__ out_sim,
                                                        int64_t* __restrict__ out_eid) {
    __shared__ int lds[4];
    const int b = blockIdx.x;
    const int64_t* d = desc + (int64_t)loo_find_row(desc, LOO_EROW, nrow, b) * LOO_EROW;
    const int64_t n = d[0], off = d[1];
    const int ft = (int)d[2];
    const int64_t* __restrict__ eu = reinterpret_cast<const int64_t*>(d[3]);
    const int64_t* __restrict__ ev = reinterpret_cast<const int64_t*>(d[4]);
    const float* __restrict__ sim = reinterpret_cast<const float*>(d[5]);
    const int64_t ru = d[6], rv = d[7];           // the removed id on that side, or INT64_MAX when the side has another node type
    const int64_t au = d[8], av = d[9], cap = d[10];
    const int64_t i0 = (int64_t)(b - ft) * LOO_TILE;
    int run = PASS == 1 ? tile_sum[b] - tile_sum[ft] : 0;       // position inside the row's output range
    for (int r = 0; r < LOO_TILE / 256; ++r) {
        const int64_t i = i0 + r * 256 + threadIdx.x;
        int64_t u = 0, v = 0;
        bool f = false;
        if (i < n) {
            u = eu[i];
            v = ev[i];
            f = u != ru && v != rv;
        }
        int total;
        const int excl = loo_flag_scan(f, lds, total);
        if (PASS == 1 && f) {
            const int64_t p = run + excl;
            if (p < cap) {                        // a row never writes past the count the host sized it for (check mode reports the difference)
                out_u[off + p] = u - (u > ru ? 1 : 0) + au;
                out_v[off + p] = v - (v > rv ? 1 : 0) + av;
                out_eid[off + p] = i;
                if (sim) out_sim[off + p] = sim[i];
            }
        }
        run += total;
    }
    if (PASS == 0 && threadIdx.x == 0) tile_sum[b] = run;
}

// ---------------------------------------------------------------- row index of every node type: row_of[off + b * per + i] = i + (is_t && i >= r_b)
__global__ __launch_bounds__(256) void loo_rows_kernel(const int64_t* __restrict__ desc, int nrow, const int64_t* __restrict__ removed, int ncopies,
                                                       int64_t* __restrict__ row_of) {
    const int b = blockIdx.x;
    const int64_t* d = desc + (int64_t)loo_find_row(desc, LOO_NROW, nrow, b) * LOO_NROW;
    const int64_t n = d[0], off = d[1], per = d[3];
    const bool is_t = d[4] != 0;
    const int64_t i0 = (int64_t)(b - (int)d[2]) * LOO_TILE;
#pragma unroll
    for (int r = 0; r < LOO_TILE / 256; ++r) {
        const int64_t k = i0 + r * 256 + threadIdx.x;
        if (k < n) {                              // n > 0 implies per > 0
            const int64_t c = k / per, i = k - c * per;
            row_of[off + k] = i + ((is_t && c < ncopies && i >= removed[c]) ? 1 : 0);
        }
    }
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_loo_edges(const int64_t* desc, int32_t nrow, int32_t ntiles, int32_t* tile_sum, int64_t* out_u, int64_t* out_v, float* out_sim,
                             int64_t* out_eid, int32_t* counts, void* stream) {
    if (nrow < 0 || ntiles < 0) { set_error("loo_edges: bad argument"); return WSI_EINVAL; }
    if (nrow == 0) return WSI_OK;
    if (!desc || !tile_sum || !counts || (ntiles > 0 && (!out_u || !out_v || !out_sim || !out_eid))) {
        set_error("loo_edges: null pointer");
        return WSI_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    if (ntiles > 0) hipLaunchKernelGGL(loo_edges_kernel<0>, dim3(ntiles), dim3(256), 0, s, desc, (int)nrow, tile_sum, out_u, out_v, out_sim, out_eid);
    hipLaunchKernelGGL(loo_scan_tiles_kernel, dim3(1), dim3(256), 0, s, tile_sum, (int)ntiles, desc, (int)nrow, counts);
    if (ntiles > 0) hipLaunchKernelGGL(loo_edges_kernel<1>, dim3(ntiles), dim3(256), 0, s, desc, (int)nrow, tile_sum, out_u, out_v, out_sim, out_eid);
    return check_launch("loo_edges");
}

extern "C" int wsi_loo_rows(const int64_t* desc, int32_t nrow, int32_t ntiles, const int64_t* removed, int32_t ncopies, int64_t* row_of, void* stream) {
    if (nrow < 0 || ntiles < 0 || ncopies < 0) { set_error("loo_rows: bad argument"); return WSI_EINVAL; }
    if (nrow == 0 || ntiles == 0) return WSI_OK;
    if (!desc || !removed || !row_of) { set_error("loo_rows: null pointer"); return WSI_EINVAL; }
    hipLaunchKernelGGL(loo_rows_kernel, dim3(ntiles), dim3(256), 0, (hipStream_t)stream, desc, (int)nrow, removed, (int)ncopies, row_of);
    return check_launch("loo_rows");
}
