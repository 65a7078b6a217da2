// The fill of a padded GTNMIL graph slot (gtn.GraphSlot).  Contract: include/wsi_hgnn.h.
//
// A slot is `cells` cells of `cell_rows` rows each; slide i of a batch lies at the head of cell i, the rest of the cell is dead, the cells
// behind the last slide are all dead.  The block-diagonal adjacency of the batch is the slides' LOCAL CSR / CSC tables (gtn.SlideSet keeps them
// on the device) one after the other: pointers shifted by the slide's first entry, indices by the cell's first row.  A dead row gets an empty
// range - the running entry offset on both sides - so the kernels that walk rowptr / colptr (wsi_spmm_sum, wsi_mincut_fwd / _bwd) read nothing
// for it, and nothing behind the batch's last entry is ever referenced.
//   rows    : a wave per slot row: the feature row copied (16-byte lane accesses when both sides allow, scalar otherwise) or zeroed, live[r],
//             rowptr[r], colptr[r]; trailing workgroups write cell_live, labels and the two scalar words.
//   entries : a thread per entry of the batch: the owning slide by binary search over the descriptors' first entries, then src / csc_dst
//             rebased and the weights copied (1.0 where the slide has none).
// Two launches whatever the batch; no atomics, no read-back, no allocation: the same bits run after run.
#include "common.h"

namespace wsi {

constexpr int GS_DESC = 16;             // int64 words per slide: [x, x_stride, rowptr, src, edge_w, colptr, csc_dst, edge_w_csc, rows, entries, dst_entry, label, 0...]
enum { GS_X = 0, GS_XLD = 1, GS_ROWPTR = 2, GS_SRC = 3, GS_W = 4, GS_COLPTR = 5, GS_CSCDST = 6, GS_WCSC = 7, GS_N = 8, GS_E = 9, GS_E0 = 10, GS_LABEL = 11 };
constexpr int GS_THREADS = 256;
constexpr int GS_ROWS = 16;             // slot rows per workgroup of the row kernel (4 per wave)

__global__ __launch_bounds__(GS_THREADS) void graph_slot_rows_kernel(const int64_t* __restrict__ desc, int num_slides, int cells, int cell_rows,
                                                                     int feats, bool dst_vec, int row_blocks, int64_t total_entries,
                                                                     float inv_cells, float live_rows, float* __restrict__ x,
                                                                     float* __restrict__ live, float* __restrict__ cell_live,
                                                                     float* __restrict__ scalars, int64_t* __restrict__ labels,
                                                                     int32_t* __restrict__ rowptr, int32_t* __restrict__ colptr) {
    if ((int)blockIdx.x >= row_blocks) {                 // the per-cell tables and the scalar words
        const int g = ((int)blockIdx.x - row_blocks) * GS_THREADS + threadIdx.x;
        if (g < cells) {
            cell_live[g] = g < num_slides ? 1.f : 0.f;
            labels[g] = g < num_slides ? desc[(int64_t)g * GS_DESC + GS_LABEL] : (int64_t)-100;
        }
        if (g == 0) { scalars[0] = inv_cells; scalars[1] = live_rows; }
        return;
    }
    const int64_t num_rows = (int64_t)cells * cell_rows;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int q = 0; q < GS_ROWS / 4; ++q) {
        const int64_t r = (int64_t)blockIdx.x * GS_ROWS + q * 4 + wave;
        if (r >= num_rows) return;
        const int g = (int)(r / cell_rows);
        const int64_t j = r - (int64_t)g * cell_rows;
        const int64_t* d = desc + (int64_t)g * GS_DESC;
        const bool in_slide = g < num_slides;
        const bool alive = in_slide && j < d[GS_N];
        const float* src = nullptr;
        int64_t stride = 0;
        if (alive) {
            stride = d[GS_XLD];
            src = reinterpret_cast<const float*>(d[GS_X]) + j * stride;
        }
        if (lane == 0) {
            // a dead row's range is empty: the first entry behind its cell's slide (behind the whole batch for an unused cell)
            int64_t rp = in_slide ? d[GS_E0] + d[GS_E] : total_entries, cp = rp;
            if (alive) {
                rp = d[GS_E0] + reinterpret_cast<const int32_t*>(d[GS_ROWPTR])[j];
                cp = d[GS_E0] + reinterpret_cast<const int32_t*>(d[GS_COLPTR])[j];
            }
            live[r] = alive ? 1.f : 0.f;
            rowptr[r] = (int32_t)rp;
            colptr[r] = (int32_t)cp;
            if (r == num_rows - 1) { rowptr[num_rows] = (int32_t)total_entries; colptr[num_rows] = (int32_t)total_entries; }
        }
        float* dstp = x + r * feats;
        const bool vec = dst_vec && (src == nullptr || (((reinterpret_cast<uintptr_t>(src) & 15) == 0) && (stride % 4 == 0)));
        if (vec) {
            for (int col = lane * 4; col < feats; col += 256)
                *reinterpret_cast<float4*>(dstp + col) = src ? *reinterpret_cast<const float4*>(src + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int col = lane; col < feats; col += 64) dstp[col] = src ? src[col] : 0.f;
        }
    }
}

__global__ __launch_bounds__(GS_THREADS) void graph_slot_entries_kernel(const int64_t* __restrict__ desc, int num_slides, int cell_rows,
                                                                        int64_t total_entries, int32_t* __restrict__ src, float* __restrict__ edge_w,
                                                                        int32_t* __restrict__ csc_dst, float* __restrict__ edge_w_csc) {
    for (int64_t e = (int64_t)blockIdx.x * GS_THREADS + threadIdx.x; e < total_entries; e += (int64_t)gridDim.x * GS_THREADS) {
        // the last slide whose first entry is <= e (a slide without entries shares its first entry with its successor)
        int lo = 0, hi = num_slides - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (desc[(int64_t)mid * GS_DESC + GS_E0] <= e) lo = mid; else hi = mid - 1;
        }
        const int64_t* d = desc + (int64_t)lo * GS_DESC;
        const int64_t k = e - d[GS_E0];
        if (k < 0 || k >= d[GS_E]) continue;
        const int32_t base = (int32_t)((int64_t)lo * cell_rows);
        const float* w = reinterpret_cast<const float*>(d[GS_W]);
        const float* wc = reinterpret_cast<const float*>(d[GS_WCSC]);
        src[e] = reinterpret_cast<const int32_t*>(d[GS_SRC])[k] + base;
        csc_dst[e] = reinterpret_cast<const int32_t*>(d[GS_CSCDST])[k] + base;
        edge_w[e] = w ? w[k] : 1.f;
        edge_w_csc[e] = wc ? wc[k] : 1.f;
    }
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_graph_slot_fill(const int64_t* slide_desc, int32_t num_slides, int32_t cells, int32_t cell_rows, int32_t feats,
                                   int64_t entry_cap, int64_t total_entries, float inv_cells, float live_rows,
                                   float* x, float* live, float* cell_live, float* scalars, int64_t* labels,
                                   int32_t* rowptr, int32_t* src, float* edge_w, int32_t* colptr, int32_t* csc_dst, float* edge_w_csc,
                                   void* stream) {
    if (num_slides < 0 || cells < 1 || cell_rows < 1 || feats < 1 || num_slides > cells || entry_cap < 0 || total_entries < 0 ||
        total_entries > entry_cap || entry_cap > 0x7fffffff || (int64_t)cells * cell_rows >= 0x7fffffff) {
        set_error("graph_slot_fill: bad argument"); return WSI_EINVAL;
    }
    if ((num_slides > 0 && !slide_desc) || !x || !live || !cell_live || !scalars || !labels || !rowptr || !colptr ||
        (total_entries > 0 && (!src || !edge_w || !csc_dst || !edge_w_csc))) {
        set_error("graph_slot_fill: null pointer"); return WSI_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const int64_t num_rows = (int64_t)cells * cell_rows;
    const int row_blocks = (int)((num_rows + GS_ROWS - 1) / GS_ROWS), cell_blocks = (cells + GS_THREADS - 1) / GS_THREADS;
    const bool dst_vec = ((reinterpret_cast<uintptr_t>(x) & 15) == 0) && (feats % 4 == 0);
    hipLaunchKernelGGL(graph_slot_rows_kernel, dim3(row_blocks + cell_blocks), dim3(GS_THREADS), 0, st, slide_desc, (int)num_slides, (int)cells,
                       (int)cell_rows, (int)feats, dst_vec, row_blocks, total_entries, inv_cells, live_rows, x, live, cell_live, scalars, labels,
                       rowptr, colptr);
    if (total_entries > 0) {
        int64_t blocks = (total_entries + GS_THREADS - 1) / GS_THREADS;
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(graph_slot_entries_kernel, dim3((unsigned)blocks), dim3(GS_THREADS), 0, st, slide_desc, (int)num_slides, (int)cell_rows,
                           total_entries, src, edge_w, csc_dst, edge_w_csc);
    }
    return check_launch("graph_slot_fill");
}
