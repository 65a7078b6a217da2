// Tables written from pieces: ONE launch over a table of segment descriptors, every segment a run of elements that are an offset copy of a stored
// piece, a lookup, a fill or index arithmetic.  Two users, one kernel: the kernel plan of a block-diagonal batch (graph.assemble_plan,
// wsi_plan_assemble: ~90 framework launches per new batch as tensor operations) and the fill of a padded batch slot (data.BatchSlot,
// graph.slot_fill, wsi_slot_fill), whose filler parts are index arithmetic (csrc/slot_math.h) and whose features are a 16-byte
// streaming copy.  Contract: include/wsi_hgnn.h (segment descriptor tables).
#include "common.h"
#include "slot_math.h"

namespace wsi {

constexpr int SEG_ROW = 10;               // int64 words per segment descriptor
constexpr int SEG_BLOCK = 1024;           // elements per workgroup (modes 5: 16-byte elements)

// desc (device, int64): per segment  [out, in1, in2, tab_off, key, add, stride, n, mode, block_start], then the tables the tab_off's point into.
//  mode 0  int32 out[i] = add + i * stride + in1[i] + tab[in2[i]]        (in1, in2: int64 arrays or null; tab = desc + tab_off + key)
//  mode 1  4-byte copy out[i] = in1[i]                                   mode 2  4-byte fill out[i] = (uint32) add
//  mode 3  int32 out[i] = tab[i]                                         mode 4  int64 out[i] = tab[i]
//  mode 5  16-byte copy out[i] = in1[i], or zero fill when in1 is null (n counts 16-byte elements; both pointers 16-byte aligned)
//  filler modes, tab = the filler block of slot_math.h, key = node type:
//  mode 10 rowptr of the filler's segments      mode 11 src of the filler's edges      mode 13 colptr of the filler's sources
//  mode 14 out[i] = add + stride * (destination of the filler's i-th edge): the softmax segment of every filler edge
//  mode 12 CSC entries of the filler's edges: out = csc_eid and in1 = csc_dst, the WHOLE tables (the entry's position is computed)
__global__ __launch_bounds__(256) void segment_table_kernel(const int64_t* __restrict__ desc, int nsegs) {
    const int b = blockIdx.x;
    int lo = 0, hi = nsegs - 1;           // last segment whose block_start <= b
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (desc[(int64_t)mid * SEG_ROW + 9] <= b) lo = mid; else hi = mid - 1;
    }
    const int64_t* d = desc + (int64_t)lo * SEG_ROW;
    const int64_t n = d[7];
    const int mode = (int)d[8];
    const int64_t i0 = ((int64_t)b - d[9]) * SEG_BLOCK;
    const int64_t* tab = d[3] >= 0 ? desc + d[3] : nullptr;
    const int64_t key = d[4], add = d[5], stride = d[6];
#pragma unroll
    for (int r = 0; r < SEG_BLOCK / 256; ++r) {
        const int64_t i = i0 + r * 256 + threadIdx.x;          // a wave's 64 lanes: 64 consecutive elements (modes 5: one contiguous KB)
        if (i >= n) break;
        switch (mode) {
        case 0: {
            const int64_t* in1 = reinterpret_cast<const int64_t*>(d[1]);
            const int64_t* in2 = reinterpret_cast<const int64_t*>(d[2]);
            int64_t v = add + i * stride;
            if (in1) v += in1[i];
            if (tab) v += tab[key + (in2 ? in2[i] : 0)];
            reinterpret_cast<int32_t*>(d[0])[i] = (int32_t)v;
            break;
        }
        case 1: reinterpret_cast<uint32_t*>(d[0])[i] = reinterpret_cast<const uint32_t*>(d[1])[i]; break;
        case 2: reinterpret_cast<uint32_t*>(d[0])[i] = (uint32_t)add; break;
        case 3: reinterpret_cast<int32_t*>(d[0])[i] = (int32_t)tab[key + i]; break;
        case 4: reinterpret_cast<int64_t*>(d[0])[i] = tab[key + i]; break;
        case 5: {
            const uint4* in = reinterpret_cast<const uint4*>(d[1]);
            reinterpret_cast<uint4*>(d[0])[i] = in ? in[i] : make_uint4(0u, 0u, 0u, 0u);
            break;
        }
        case 10: reinterpret_cast<int32_t*>(d[0])[i] = (int32_t)filler_rowptr(tab, key, i); break;
        case 11: reinterpret_cast<int32_t*>(d[0])[i] = (int32_t)filler_src(tab, key, i); break;
        case 12: {
            int64_t slot, eid, dst;
            filler_csc(tab, key, i, &slot, &eid, &dst);
            reinterpret_cast<int32_t*>(d[0])[slot] = (int32_t)eid;
            reinterpret_cast<int32_t*>(d[1])[slot] = (int32_t)dst;
            break;
        }
        case 13: reinterpret_cast<int32_t*>(d[0])[i] = (int32_t)filler_colptr(tab, key, i); break;
        case 14: {
            const int64_t* f = filler_type(tab, key);
            int64_t node, k;
            filler_owner(i, f[FP_EF], f[FP_NF], &node, &k);
            reinterpret_cast<int32_t*>(d[0])[i] = (int32_t)(add + node * stride);
            break;
        }
        default: break;
        }
    }
}

// The middle level of every two-level compaction scan (common.h: launch_tile_scan), for the node/edge draws of augment.hip, the leave-one-out
// rows of loo.hip, the flag segments of slot_aug.hip and, with nseg == 0 (no counts), the per-relation counts of plan_rel.hip.  One workgroup
// walks any number of tiles in rounds of 256 and carries the running total from round to round.
__global__ __launch_bounds__(256) void tile_scan_kernel(int32_t* __restrict__ tile_sum, int ntiles, const int64_t* __restrict__ rows, int stride,
                                                        int col, int nseg, int32_t* __restrict__ counts) {
    __shared__ int lds[4];
    int carry = 0;
    for (int base = 0; base < ntiles; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < ntiles ? tile_sum[i] : 0;
        int total;
        const int incl = block_scan_inclusive(v, lds, total);
        if (i < ntiles) tile_sum[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0) tile_sum[ntiles] = carry;
    __syncthreads();                      // the prefix is read back below by other lanes of this workgroup
    for (int s = threadIdx.x; s < nseg; s += 256) {
        const int a = (int)rows[(int64_t)s * stride + col];
        const int b = s + 1 < nseg ? (int)rows[(int64_t)(s + 1) * stride + col] : ntiles;
        counts[s] = tile_sum[b] - tile_sum[a];
    }
}

void launch_tile_scan(int32_t* tile_sum, int ntiles, const int64_t* rows, int stride, int col, int nseg, int32_t* counts, hipStream_t st) {
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(256), 0, st, tile_sum, ntiles, rows, stride, col, nseg, counts);
}

// Which node types the real slides of a filled slot hold (wsi_type_present): one wave, lane t reads the b_cap readout words of node type t.
__global__ __launch_bounds__(64) void type_present_kernel(const float* __restrict__ seg_nonempty, int T, int graphs, int b_cap,
                                                          float* __restrict__ out) {
    for (int t = threadIdx.x; t < T; t += 64) {
        bool any = false;
        for (int b = 0; b < b_cap; ++b) any = any || seg_nonempty[(int64_t)t * graphs + b] != 0.f;
        out[t] = any ? 1.f : 0.f;
    }
}

// GraphConv's degree norms of a filled homogeneous slot (wsi_degree_norms): thread i reads two words of each pointer table.  The reciprocal
// square root is taken in double and rounded once: torch's float32 rsqrt on this device returns that value for every degree, the one-ulp
// v_rsq_f32 behind rsqrtf does not (418 of the degrees 1 .. 4096 differ), and an eager step on the slot's graph must see torch's bits.
__device__ __forceinline__ float degree_norm(int deg) { return (float)(1.0 / sqrt((double)(deg > 1 ? deg : 1))); }

__global__ __launch_bounds__(256) void degree_norms_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colptr, int n,
                                                           float* __restrict__ in_norm, float* __restrict__ out_norm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    in_norm[i] = degree_norm(rowptr[i + 1] - rowptr[i]);
    out_norm[i] = degree_norm(colptr[i + 1] - colptr[i]);
}

// Which rows of a filled homogeneous slot belong to its real slides, and how many they are (wsi_slot_live_rows): thread i reads one word of
// row_seg; thread 0 of the grid adds the b_cap counts in index order (integers below 2^24 as fp32: the sum is exact).
__global__ __launch_bounds__(256) void slot_live_rows_kernel(const int32_t* __restrict__ row_seg, const float* __restrict__ seg_counts, int n,
                                                             int b_cap, float* __restrict__ live, float* __restrict__ live_rows) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) live[i] = row_seg[i] < b_cap ? 1.f : 0.f;
    if (i == 0) {
        float s = 0.f;
        for (int b = 0; b < b_cap; ++b) s += seg_counts[b];
        live_rows[0] = s;
    }
}

static int launch_segment_table(const char* who, const int64_t* desc, int32_t nsegs, int32_t total_blocks, void* stream) {
    if (nsegs < 0 || total_blocks < 0) { set_error("%s: bad argument", who); return WSI_EINVAL; }
    if (nsegs == 0 || total_blocks == 0) return WSI_OK;
    if (!desc) { set_error("%s: null pointer", who); return WSI_EINVAL; }
    hipLaunchKernelGGL(segment_table_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, desc, (int)nsegs);
    return check_launch(who);
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_plan_assemble(const int64_t* desc, int32_t nsegs, int32_t total_blocks, void* stream) {
    return launch_segment_table("plan_assemble", desc, nsegs, total_blocks, stream);
}

extern "C" int wsi_slot_fill(const int64_t* desc, int32_t nsegs, int32_t total_blocks, void* stream) {
    return launch_segment_table("slot_fill", desc, nsegs, total_blocks, stream);
}

extern "C" int wsi_type_present(const float* seg_nonempty, int32_t T, int32_t graphs, int32_t b_cap, float* out, void* stream) {
    if (T < 1 || graphs < 0 || b_cap < 0 || b_cap > graphs) { set_error("type_present: bad argument"); return WSI_EINVAL; }
    if (!out || (!seg_nonempty && b_cap > 0)) { set_error("type_present: null pointer"); return WSI_EINVAL; }
    hipLaunchKernelGGL(type_present_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, seg_nonempty, (int)T, (int)graphs, (int)b_cap, out);
    return check_launch("type_present");
}

extern "C" int wsi_degree_norms(const int32_t* rowptr, const int32_t* colptr, int32_t n, float* in_norm, float* out_norm, void* stream) {
    if (n < 0) { set_error("degree_norms: bad argument"); return WSI_EINVAL; }
    if (n == 0) return WSI_OK;
    if (!rowptr || !colptr || !in_norm || !out_norm) { set_error("degree_norms: null pointer"); return WSI_EINVAL; }
    hipLaunchKernelGGL(degree_norms_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, rowptr, colptr, (int)n, in_norm, out_norm);
    return check_launch("degree_norms");
}

extern "C" int wsi_slot_live_rows(const int32_t* row_seg, const float* seg_counts, int32_t n, int32_t graphs, int32_t b_cap, float* live,
                                  float* live_rows, void* stream) {
    if (n < 0 || graphs < 0 || b_cap < 0 || b_cap > graphs) { set_error("slot_live_rows: bad argument"); return WSI_EINVAL; }
    if (!live_rows || (!seg_counts && b_cap > 0) || (n > 0 && (!row_seg || !live))) { set_error("slot_live_rows: null pointer"); return WSI_EINVAL; }
    hipLaunchKernelGGL(slot_live_rows_kernel, dim3(n > 0 ? (n + 255) / 256 : 1), dim3(256), 0, (hipStream_t)stream, row_seg, seg_counts, (int)n,
                       (int)b_cap, live, live_rows);
    return check_launch("slot_live_rows");
}
