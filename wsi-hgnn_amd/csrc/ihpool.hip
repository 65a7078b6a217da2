// IHPool's cluster assignment (H2MIL, baselines/H2MIL/code/IHPool.py:138-142 and :185-189 at dis = 'ou') for gfx950.
// Contract: include/wsi_hgnn.h.  Every member of a segment goes to the seed of that segment nearest in
//   |xy_s - xy_n|_2 + |f_s - f_n|
// - one launch for all segments of all slides instead of one distance matrix, one sort and several read-backs per substructure.
// Rules where the reference leaves the outcome open: equal distances go to the LOWEST seed (the seeds are visited in order and only a
// strictly smaller distance replaces the best one); a member that IS a seed belongs to its own cluster whatever the distances say.
// The members arrive grouped by segment (member_seg non-decreasing), so a block of 256 consecutive members spans a run of segments; it
// walks that run and stages each segment's seeds through LDS in tiles of IH_TILE, every thread whose member belongs to the segment
// scanning the tile.  Integer output, no atomics: identical calls give identical results.
#include "common.h"
#include <math.h>

namespace wsi {

constexpr int IH_BLOCK = 256;
constexpr int IH_TILE = 64;

__global__ __launch_bounds__(IH_BLOCK) void ihpool_assign_kernel(const float* __restrict__ xyf, int num_nodes, const int32_t* __restrict__ member_node,
                                                                 const int32_t* __restrict__ member_seg, int m, const int32_t* __restrict__ seed_ptr,
                                                                 const int32_t* __restrict__ seed_node, int num_segs, int num_seeds,
                                                                 int32_t* __restrict__ assign) {
    __shared__ float sx[IH_TILE], sy[IH_TILE], sf[IH_TILE];
    __shared__ int sn[IH_TILE];
    const int first = (int)blockIdx.x * IH_BLOCK, i = first + (int)threadIdx.x;
    const int last = min(first + IH_BLOCK, m) - 1;               // first <= last: the grid covers m members
    const bool mine = i < m;
    int node = mine ? member_node[i] : -1;
    const int seg = mine ? member_seg[i] : -1;
    if (node < 0 || node >= num_nodes) node = -1;
    float x = 0.f, y = 0.f, f = 0.f;
    if (node >= 0) { x = xyf[(int64_t)node * 3]; y = xyf[(int64_t)node * 3 + 1]; f = xyf[(int64_t)node * 3 + 2]; }
    float best = INFINITY;
    int arg = -1;
    const int s0 = max(member_seg[first], 0), s1 = min(member_seg[last], num_segs - 1);      // block-uniform
    for (int s = s0; s <= s1; ++s) {
        const int k0 = max(seed_ptr[s], 0), k1 = min(seed_ptr[s + 1], num_seeds);
        for (int base = k0; base < k1; base += IH_TILE) {
            const int cnt = min(IH_TILE, k1 - base);
            __syncthreads();
            if ((int)threadIdx.x < cnt) {
                int sd = seed_node[base + (int)threadIdx.x];
                const bool ok = sd >= 0 && sd < num_nodes;
                sn[threadIdx.x] = ok ? sd : -2;                  // a seed outside the table matches no member and is infinitely far
                sx[threadIdx.x] = ok ? xyf[(int64_t)sd * 3] : INFINITY;
                sy[threadIdx.x] = ok ? xyf[(int64_t)sd * 3 + 1] : 0.f;
                sf[threadIdx.x] = ok ? xyf[(int64_t)sd * 3 + 2] : 0.f;
            }
            __syncthreads();
            if (seg == s && node >= 0) {
                for (int j = 0; j < cnt; ++j) {
                    const float dx = sx[j] - x, dy = sy[j] - y;
                    const float d = sn[j] == node ? -1.f : sqrtf(dx * dx + dy * dy) + fabsf(sf[j] - f);
                    if (d < best) { best = d; arg = base - k0 + j; }
                }
            }
        }
    }
    if (mine) assign[i] = arg;
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_ihpool_assign(const float* xyf, int32_t num_nodes, const int32_t* member_node, const int32_t* member_seg, int32_t num_members,
                                 const int32_t* seed_ptr, const int32_t* seed_node, int32_t num_segs, int32_t num_seeds, int32_t* assign, void* stream) {
    if (num_nodes < 0 || num_members < 0 || num_segs < 0 || num_seeds < 0) {
        set_error("ihpool_assign: bad shape nodes=%d members=%d segments=%d seeds=%d", num_nodes, num_members, num_segs, num_seeds);
        return WSI_EINVAL;
    }
    if (num_members == 0) return WSI_OK;
    if (!xyf || !member_node || !member_seg || !seed_ptr || !assign || (num_seeds > 0 && !seed_node)) { set_error("ihpool_assign: null pointer"); return WSI_EINVAL; }
    hipLaunchKernelGGL(ihpool_assign_kernel, dim3((num_members + IH_BLOCK - 1) / IH_BLOCK), dim3(IH_BLOCK), 0, (hipStream_t)stream, xyf, num_nodes,
                       member_node, member_seg, num_members, seed_ptr, seed_node, num_segs, num_seeds, assign);
    return check_launch("ihpool_assign");
}
