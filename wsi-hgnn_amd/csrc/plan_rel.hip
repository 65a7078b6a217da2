// The per-relation-source plan derived from the base plan (graph.plan_by_relation).  Contract: include/wsi_hgnn.h.
//
// HGT's K/V tables hold one row per (relation, source node): row(r, u) = rel_rows[r].lo + (u - type_off[source type of r]).  The relation of an
// edge is a function of its softmax segment (segment = seg_off[t] + node * R[t] + slot; relation = the slot's), so the per-relation plan is a
// pure function of the base plan: `src` is a renumbering, and the CSC by (relation, source) is a STABLE PARTITION of every source's base CSC
// entries by relation - a source's base entries are in CSR order already, a subsequence of them still is.
//   source<0> : a wave per source node, lanes striding its CSC entries: the entry's relation, src_rel[edge] = its row, and per relation of the
//               node's source type the number of entries (ballot + popcount, running counts in registers) -> counts[row].  Every row (r, u)
//               belongs to exactly one (wave, relation): counts is written whole, no atomics.
//   scan      : exclusive prefix sum of counts -> colptr_rel: the two-level scan of common.h (tile sums, launch_tile_scan, tiles rank).
//   source<1> : the same walk; an entry's rank inside its row is the running count + the popcount under the lane mask, so entries keep their
//               relative order: csc_eid_rel / csc_dst_rel [colptr_rel[row] + rank].
// Five launches on the caller's stream; integers only, no atomics, no allocation, no read-back: identical calls give identical bits.
#include "common.h"

namespace wsi {

constexpr int PR_TILE = WSI_PLAN_REL_TILE;       // counts per workgroup of the scan: 4 rounds of 256 lanes
constexpr int PR_MAX_K = WSI_PLAN_REL_MAX_RELS;  // relations per source type: one running count each, in registers

struct PlanRel {
    const int32_t* src; const int32_t* colptr; const int32_t* csc_eid; const int32_t* csc_dst; const int32_t* edge_seg; const int32_t* hdr;
    int32_t* src_rel; int32_t* colptr_rel; int32_t* csc_eid_rel; int32_t* csc_dst_rel; int32_t* counts; int32_t* partials;
    int N, E, S, T, NR, NS, ntiles;
};

// the header table (graph.PlanHeader.relation_table): 4 words [T, NR, NS, N], then
//   type_off[T+1] seg_off[T+1] R[T] slot_ptr[T+1] slot_rel[NR] rel_lo[NR] rel_src[NR] rel_k[NR] srel_ptr[T+1] srel[NR]
struct PlanRelHeader {
    const int32_t *type_off, *seg_off, *R, *slot_ptr, *slot_rel, *rel_lo, *rel_src, *rel_k, *srel_ptr, *srel;
    __device__ __forceinline__ PlanRelHeader(const int32_t* h, int T, int NR) {
        type_off = h + 4; seg_off = type_off + T + 1; R = seg_off + T + 1; slot_ptr = R + T; slot_rel = slot_ptr + T + 1;
        rel_lo = slot_rel + NR; rel_src = rel_lo + NR; rel_k = rel_src + NR; srel_ptr = rel_k + NR; srel = srel_ptr + T + 1;
    }
};

// relation of softmax segment `seg`, -1 when the segment lies in no node type's range
__device__ __forceinline__ int pr_relation(const PlanRelHeader& h, int T, int NR, int S, int seg) {
    if (seg < 0 || seg >= S) return -1;
    int t = 0;
    while (t + 1 < T && seg >= h.seg_off[t + 1]) ++t;
    const int R = h.R[t];
    if (R < 1) return -1;
    const int r = h.slot_rel[h.slot_ptr[t] + (seg - h.seg_off[t]) % R];
    return (r >= 0 && r < NR) ? r : -1;
}

template <int PASS>
__global__ __launch_bounds__(256) void pr_source_kernel(PlanRel a) {
    const int lane = threadIdx.x & 63;
    const int u = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (u >= a.N) return;                                   // (wave-uniform; the kernel has no workgroup barrier)
    const PlanRelHeader h(a.hdr, a.T, a.NR);
    int s = 0;
    while (s + 1 < a.T && u >= h.type_off[s + 1]) ++s;
    const int ul = u - h.type_off[s];
    const int k0 = h.srel_ptr[s];
    int nk = h.srel_ptr[s + 1] - k0;
    nk = nk < 0 ? 0 : (nk > PR_MAX_K ? PR_MAX_K : nk);
    // lane k < nk holds what belongs to the k-th relation of this source type: the row (r_k, u) and, in the scatter, where the row starts
    int row_lane = -1, base_lane = 0;
    if (lane < nk) {
        const int r = h.srel[k0 + lane];
        if (r >= 0 && r < a.NR) row_lane = h.rel_lo[r] + ul;
        if (row_lane < 0 || row_lane >= a.NS) row_lane = -1;
        if (PASS == 1 && row_lane >= 0) base_lane = a.colptr_rel[row_lane];
    }
    int cnt[PR_MAX_K];
#pragma unroll
    for (int k = 0; k < PR_MAX_K; ++k) cnt[k] = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int lo = a.colptr[u], hi = a.colptr[u + 1];
    for (int j0 = lo; j0 < hi; j0 += 64) {
        const int j = j0 + lane;
        int k = -1, eid = 0;
        if (j < hi && j >= 0 && j < a.E) {
            eid = a.csc_eid[j];
            if (eid >= 0 && eid < a.E) {
                const int r = pr_relation(h, a.T, a.NR, a.S, a.edge_seg[eid]);
                if (r >= 0 && h.rel_src[r] == s) k = h.rel_k[r];
                if (k >= nk) k = -1;
            }
        }
        int rank = 0;
#pragma unroll
        for (int kk = 0; kk < PR_MAX_K; ++kk) {
            if (kk < nk) {                                  // (uniform)
                const unsigned long long m = __ballot(k == kk);
                if (k == kk) rank = cnt[kk] + __popcll(m & below);
                cnt[kk] += __popcll(m);
            }
        }
        const int sel = k < 0 ? 0 : k;
        const int row = __shfl(row_lane, sel);
        const int base = __shfl(base_lane, sel);
        if (k >= 0 && row >= 0) {
            if (PASS == 0) {
                a.src_rel[eid] = row;
            } else {
                const int pos = base + rank;
                if (pos >= 0 && pos < a.E) {
                    a.csc_eid_rel[pos] = eid;
                    a.csc_dst_rel[pos] = a.csc_dst[j];
                }
            }
        }
    }
    if (PASS == 0) {
        int mine = 0;
#pragma unroll
        for (int kk = 0; kk < PR_MAX_K; ++kk)
            if (lane == kk) mine = cnt[kk];
        if (row_lane >= 0) a.counts[row_lane] = mine;
    }
}

__global__ __launch_bounds__(256) void pr_zero_kernel(int32_t* __restrict__ out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = 0;
}

__global__ __launch_bounds__(256) void pr_tile_sum_kernel(PlanRel a) {
    __shared__ int lds[4];
    int sum = 0;
    for (int r = 0; r < PR_TILE / 256; ++r) {
        const int i = blockIdx.x * PR_TILE + r * 256 + threadIdx.x;
        sum += i < a.NS ? a.counts[i] : 0;
    }
    int total;
    block_scan_inclusive(sum, lds, total);
    if (threadIdx.x == 0) a.partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void pr_tile_scan_kernel(PlanRel a) {
    __shared__ int lds[4];
    int run = a.partials[blockIdx.x];
    for (int r = 0; r < PR_TILE / 256; ++r) {
        const int i = blockIdx.x * PR_TILE + r * 256 + threadIdx.x;
        const int v = i < a.NS ? a.counts[i] : 0;
        int total;
        const int incl = block_scan_inclusive(v, lds, total);
        if (i < a.NS) a.colptr_rel[i] = run + incl - v;
        if (i == a.NS - 1) a.colptr_rel[a.NS] = run + incl;
        run += total;
    }
}

}  // namespace wsi

using namespace wsi;

extern "C" int64_t wsi_plan_by_relation_scratch_words(int32_t num_src_rows) {
    if (num_src_rows < 0) return -1;
    return (int64_t)num_src_rows + ((int64_t)num_src_rows + PR_TILE - 1) / PR_TILE + 1;
}

extern "C" int wsi_plan_by_relation(const int32_t* src, const int32_t* colptr, const int32_t* csc_eid, const int32_t* csc_dst,
                                    const int32_t* edge_seg, int32_t num_nodes, int32_t num_edges, int32_t num_segs,
                                    const int32_t* header, int32_t header_words, int32_t num_types, int32_t num_rels, int32_t num_src_rows,
                                    int32_t max_src_rels, int32_t* src_rel, int32_t* colptr_rel, int32_t* csc_eid_rel, int32_t* csc_dst_rel,
                                    int32_t* scratch, int64_t scratch_words, void* stream) {
    if (num_nodes < 0 || num_edges < 0 || num_segs < 0 || num_types < 1 || num_rels < 0 || num_src_rows < 0 || max_src_rels < 0) {
        set_error("plan_by_relation: bad argument");
        return WSI_EINVAL;
    }
    if (max_src_rels > PR_MAX_K) {
        set_error("plan_by_relation: %d relations leave one source node type, at most %d are supported", (int)max_src_rels, PR_MAX_K);
        return WSI_EINVAL;
    }
    if (header_words != 5 * num_types + 5 * num_rels + 8) {
        set_error("plan_by_relation: the header table has %d words, %d node types and %d relations need %d", (int)header_words, (int)num_types,
                  (int)num_rels, 5 * (int)num_types + 5 * (int)num_rels + 8);
        return WSI_EINVAL;
    }
    if (!colptr_rel) { set_error("plan_by_relation: null pointer (colptr_rel)"); return WSI_EINVAL; }
    hipStream_t s = (hipStream_t)stream;
    const bool empty = num_edges == 0 || num_src_rows == 0 || num_nodes == 0 || !src || !colptr || !csc_eid || !csc_dst || !edge_seg;
    if (empty) {
        if (num_edges > 0 && num_src_rows > 0 && num_nodes > 0) { set_error("plan_by_relation: null pointer"); return WSI_EINVAL; }
        hipLaunchKernelGGL(pr_zero_kernel, dim3((unsigned)(((int64_t)num_src_rows + 1 + 255) / 256)), dim3(256), 0, s, colptr_rel, (int)num_src_rows + 1);
        return check_launch("plan_by_relation");
    }
    if (!header || !src_rel || !csc_eid_rel || !csc_dst_rel || !scratch) { set_error("plan_by_relation: null pointer"); return WSI_EINVAL; }
    if (scratch_words < wsi_plan_by_relation_scratch_words(num_src_rows)) {
        set_error("plan_by_relation: scratch of %lld words, %lld needed", (long long)scratch_words,
                  (long long)wsi_plan_by_relation_scratch_words(num_src_rows));
        return WSI_ENOMEM;
    }
    PlanRel a;
    a.src = src; a.colptr = colptr; a.csc_eid = csc_eid; a.csc_dst = csc_dst; a.edge_seg = edge_seg; a.hdr = header;
    a.src_rel = src_rel; a.colptr_rel = colptr_rel; a.csc_eid_rel = csc_eid_rel; a.csc_dst_rel = csc_dst_rel;
    a.counts = scratch; a.partials = scratch + num_src_rows;
    a.N = num_nodes; a.E = num_edges; a.S = num_segs; a.T = num_types; a.NR = num_rels; a.NS = num_src_rows;
    a.ntiles = (num_src_rows + PR_TILE - 1) / PR_TILE;
    const dim3 waves((unsigned)((num_nodes + 3) / 4));
    hipLaunchKernelGGL(pr_source_kernel<0>, waves, dim3(256), 0, s, a);
    hipLaunchKernelGGL(pr_tile_sum_kernel, dim3((unsigned)a.ntiles), dim3(256), 0, s, a);
    launch_tile_scan(a.partials, a.ntiles, nullptr, 0, 0, 0, nullptr, s);
    hipLaunchKernelGGL(pr_tile_scan_kernel, dim3((unsigned)a.ntiles), dim3(256), 0, s, a);
    hipLaunchKernelGGL(pr_source_kernel<1>, waves, dim3(256), 0, s, a);
    return check_launch("plan_by_relation");
}
