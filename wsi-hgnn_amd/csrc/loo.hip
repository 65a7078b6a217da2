// Leave-one-node-out batches on the device (graph.leave_one_out_batch; the GEM explainers of explainers/gem.py run the model on the graph without
// node r, once per node).  Contract: include/wsi_hgnn.h (wsi_loo_*).  Copy b of the batch is the graph without node r_b of ONE node type t; a
// descriptor row is one (relation, copy) pair, the flag of an edge is two compares, and output positions come from the two-level scan of common.h
// (never atomics: survivors keep the input order).  The host knows every
// copy's surviving count in advance (graph.leave_one_out_tables), so a row's output offset `off` is exact and the rows of a relation tile its output
// range without gaps: the relation-major, copy-major layout of graph.batch.  `cap` (the predicted count) bounds every write of a row.
#include "common.h"

namespace wsi {

constexpr int LOO_TILE = 1024;            // elements per workgroup: 4 rounds of 256 lanes
constexpr int LOO_EROW = 12;              // int64 words per edge row: n, off, first_tile, u, v, sim, r_src, r_dst, add_src, add_dst, cap, -
constexpr int LOO_NROW = 6;               // ... per node-type row: n (= B * per), off, first_tile, per, is_t, -

// ---------------------------------------------------------------- edges
// pass 0: tile_sum[tile] = survivors of the tile;  pass 1 (after the scan): stable scatter of the renumbered survivors
template <int PASS>
__global__ __launch_bounds__(256) void loo_edges_kernel(const int64_t* __restrict__ desc, int nrow, int32_t* __restrict__ tile_sum,
                                                        int64_t* __restrict__ out_u, int64_t* __restrict__ out_v, float* __restrict__ out_sim,
                                                        int64_t* __restrict__ out_eid) {
    __shared__ int lds[4];
    const int b = blockIdx.x;
    const int64_t* d = desc + (int64_t)find_row(desc, LOO_EROW, 2, nrow, b) * LOO_EROW;
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
        const int excl = block_flag_scan(f, lds, total);
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
    const int64_t* d = desc + (int64_t)find_row(desc, LOO_NROW, 2, nrow, b) * LOO_NROW;
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
    launch_tile_scan(tile_sum, (int)ntiles, desc, LOO_EROW, 2, (int)nrow, counts, s);
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
