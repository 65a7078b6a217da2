// Slide graphs from patch grids for gfx950: the 8-neighbour adjacency of GTNMIL (baselines/GTNMIL/feature_extractor/build_graphs.py:78-96) and
// the three-level tree of H2MIL (baselines/H2MIL/code/github_pretreat.py:94-329).  Contract and semantics: include/wsi_hgnn.h.
// Both are exact look-ups in many small integer point sets, so there is one open-addressing table for all sets of a call, keyed by
//   (set << 50) | ((x + 1) << 25) | (y + 1)        0 <= x, y < 2^24, set < 2^13
// (the bias makes the probes at -1 and 2^24 representable; they match nothing).  Three passes: index (64-bit compare-and-swap on the key, the
// winner writes the row; integer atomic max for the per-set maxima), count (items per node; for the tree also the parent of every level-2
// node, an integer atomic max over the covering rows = "the last in order wins"), write (probes again, writes at the prefix-sum offsets,
// no atomics; its one flag is a plain store of a constant).  Which SLOT a key lands in depends on the order the threads arrive; what a
// look-up RETURNS does not (keys are unique or the call is refused), and every output position is a
// function of the look-ups' results alone - so the output is the same on every run.
// Every probe loop runs at most `capacity` steps.  Look-ups that miss and indices outside their tables are ignored, never followed.
#include "common.h"

namespace wsi {

constexpr int GG_BLOCK = 256;
constexpr unsigned long long GG_EMPTY = ~0ull;
constexpr int GG_COORD_LIMIT = 1 << 24;
constexpr int GG_MAX_SETS = 1 << 13;

struct GridTable {
    const unsigned long long* keys;
    const int32_t* rows;
    uint32_t mask;             // capacity - 1
    int32_t num_points;
};

__device__ __forceinline__ bool gg_valid(int c) { return c >= 0 && c < GG_COORD_LIMIT; }

// x, y in [-1, 2^24]
__device__ __forceinline__ unsigned long long gg_key(int set, int x, int y) {
    return ((unsigned long long)set << 50) | ((unsigned long long)(x + 1) << 25) | (unsigned long long)(y + 1);
}

__device__ __forceinline__ uint32_t gg_hash(unsigned long long k) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (uint32_t)k;
}

// The row stored under (set, x, y), or -1.  x, y in [-1, 2^24]; at most capacity steps.
__device__ __forceinline__ int gg_find(const GridTable& t, int set, int x, int y) {
    const unsigned long long key = gg_key(set, x, y);
    uint32_t slot = gg_hash(key) & t.mask;
    for (uint32_t step = 0; step <= t.mask; ++step) {
        const unsigned long long k = t.keys[slot];
        if (k == key) {
            const int r = t.rows[slot];
            return (r >= 0 && r < t.num_points) ? r : -1;
        }
        if (k == GG_EMPTY) return -1;
        slot = (slot + 1) & t.mask;
    }
    return -1;
}

// The set of point p: the last s with set_ptr[s] <= p.  set_ptr is expected non-decreasing from 0 to P; a search never leaves [0, S).
__device__ __forceinline__ int gg_set_of(const int32_t* __restrict__ set_ptr, int S, int p) {
    int lo = 0, hi = S - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (set_ptr[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The maxima go through one atomic per wave and coordinate where the whole wave lies in one set (all but the waves on a set boundary): ten
// thousand atomics on one address serialise in L2 and took 1.8 ms at 80 000 points; 64 times fewer take microseconds.
__global__ __launch_bounds__(GG_BLOCK) void grid_index_kernel(const int32_t* __restrict__ coords, int P, const int32_t* __restrict__ set_ptr, int S,
                                                              unsigned long long* __restrict__ keys, int32_t* __restrict__ rows, uint32_t mask,
                                                              int32_t* __restrict__ set_max, int32_t* __restrict__ flags) {
    const int p = (int)blockIdx.x * GG_BLOCK + (int)threadIdx.x;
    const bool in = p < P;                                        // (no lane leaves before the wave reductions)
    const int x = in ? coords[2 * (int64_t)p] : -1, y = in ? coords[2 * (int64_t)p + 1] : -1;
    const bool ok = in && gg_valid(x) && gg_valid(y);
    if (in && !ok) atomicOr(flags, WSI_GRID_BAD_COORD);
    const int s = in ? gg_set_of(set_ptr, S, p) : -1;
    const int s_hi = wave_max(s), s_lo = -wave_max(in ? -s : -0x7fffffff);
    if (s_lo == s_hi) {
        const int mx = wave_max(ok ? x : -1), my = wave_max(ok ? y : -1);
        if ((threadIdx.x & 63) == 0 && mx >= 0) {                 // lane 0 holds the wave's lowest point: it is `in` whenever any lane is
            atomicMax(set_max + 2 * s_hi, mx);
            atomicMax(set_max + 2 * s_hi + 1, my);
        }
    } else if (ok) {
        atomicMax(set_max + 2 * s, x);
        atomicMax(set_max + 2 * s + 1, y);
    }
    if (!ok) return;
    const unsigned long long key = gg_key(s, x, y);
    uint32_t slot = gg_hash(key) & mask;
    for (uint32_t step = 0; step <= mask; ++step) {
        const unsigned long long prev = atomicCAS(keys + slot, GG_EMPTY, key);
        if (prev == GG_EMPTY) { rows[slot] = p; return; }
        if (prev == key) { atomicOr(flags, WSI_GRID_REPEATED); return; }
        slot = (slot + 1) & mask;
    }
    atomicOr(flags, WSI_GRID_TABLE_FULL);
}

// The 8 neighbours in the order of github_pretreat.py:147-170.
__constant__ int GG_DX[8] = {0, 0, 1, -1, 1, -1, 1, -1};
__constant__ int GG_DY[8] = {1, -1, 0, 0, 1, 1, -1, -1};

__device__ __forceinline__ void gg_sort2(int& a, int& b) { const int lo = min(a, b), hi = max(a, b); a = lo; b = hi; }

// ---------------------------------------------------------------- GTNMIL: the entries of row p, columns ascending
template <bool WRITE>
__global__ __launch_bounds__(GG_BLOCK) void grid_adj_kernel(const int32_t* __restrict__ coords, int P, const int32_t* __restrict__ set_ptr, int S,
                                                            GridTable t, int32_t* __restrict__ counts, const int64_t* __restrict__ incl,
                                                            int64_t* __restrict__ out_row, int64_t* __restrict__ out_col) {
    const int p = (int)blockIdx.x * GG_BLOCK + (int)threadIdx.x;
    if (p >= P) return;
    const int x = coords[2 * (int64_t)p], y = coords[2 * (int64_t)p + 1];
    int h[8], n = 0;
    if (gg_valid(x) && gg_valid(y)) {
        const int s = gg_set_of(set_ptr, S, p);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            h[k] = gg_find(t, s, x + GG_DX[k], y + GG_DY[k]);
            n += h[k] >= 0;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = -1;
    }
    if (!WRITE) { counts[p] = n; return; }
    if (n != counts[p]) return;                                   // (the two passes read one table: they agree)
#pragma unroll
    for (int k = 0; k < 8; ++k) if (h[k] < 0) h[k] = 0x7fffffff;  // misses sort behind the hits
    // Batcher's 19-comparator network for 8 keys: fixed indices, the keys stay in registers
    gg_sort2(h[0], h[1]); gg_sort2(h[2], h[3]); gg_sort2(h[4], h[5]); gg_sort2(h[6], h[7]);
    gg_sort2(h[0], h[2]); gg_sort2(h[1], h[3]); gg_sort2(h[4], h[6]); gg_sort2(h[5], h[7]);
    gg_sort2(h[1], h[2]); gg_sort2(h[5], h[6]);
    gg_sort2(h[0], h[4]); gg_sort2(h[1], h[5]); gg_sort2(h[2], h[6]); gg_sort2(h[3], h[7]);
    gg_sort2(h[2], h[4]); gg_sort2(h[3], h[5]);
    gg_sort2(h[1], h[2]); gg_sort2(h[3], h[4]); gg_sort2(h[5], h[6]);
    const int64_t off = incl[p] - n;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < n) { out_row[off + k] = p; out_col[off + k] = h[k]; }
}

// ---------------------------------------------------------------- H2MIL
// Points: the level-1 nodes of all slides, then the level-2 nodes of all slides; set b < B = level 1 of slide b, set B + b = level 2 of slide b.
// Work item w < n1 = section A of level-1 point w; n1 <= w < 2 n1 = section B of level-1 point w - n1; otherwise section C of level-2 point
// w - n1.  Its place in the count array [slide][section][node] and the global row of its node follow from the slide's offsets.
struct TreeItem {
    int section, point, slide, count_index, row, root, first1;   // first1: the slide's first level-1 POINT; row / root: global node rows
};

__device__ __forceinline__ TreeItem gg_tree_item(int w, int n1, const int32_t* __restrict__ set_ptr, int B) {
    TreeItem it;
    it.section = w < n1 ? 0 : (w < 2 * n1 ? 1 : 2);
    it.point = it.section == 0 ? w : w - n1;
    const int s = gg_set_of(set_ptr, 2 * B, it.point);
    it.slide = it.section == 2 ? s - B : s;
    if (it.slide < 0 || it.slide >= B) { it.slide = -1; return it; }          // a set table that does not describe [level 1 | level 2]
    const int p1 = set_ptr[it.slide], p1e = set_ptr[it.slide + 1];           // level-1 points of the slide
    const int p2 = set_ptr[B + it.slide] - n1;                               // level-2 nodes before the slide
    const int cnt1 = p1e - p1;
    const int base = 2 * p1 + p2;                                            // count-array items before the slide
    it.first1 = p1;
    it.root = p1 + p2 + it.slide;
    if (it.section == 2) {
        const int j = it.point - set_ptr[B + it.slide];
        it.count_index = base + 2 * cnt1 + j;
        it.row = it.root + 1 + cnt1 + j;
    } else {
        const int i = it.point - p1;
        it.count_index = base + it.section * cnt1 + i;
        it.row = it.root + 1 + i;
    }
    return it;
}

template <bool WRITE>
__global__ __launch_bounds__(GG_BLOCK) void grid_tree_kernel(const int32_t* __restrict__ coords, int P, const int32_t* __restrict__ set_ptr, int B, int n1,
                                                             const int32_t* __restrict__ cover, GridTable t, int32_t* __restrict__ counts,
                                                             int32_t* __restrict__ parent, const int64_t* __restrict__ incl,
                                                             const int32_t* __restrict__ set_max, int64_t* __restrict__ out_src,
                                                             int64_t* __restrict__ out_dst, int64_t* __restrict__ node_type,
                                                             int64_t* __restrict__ node_tree, double* __restrict__ xy, int32_t* __restrict__ flags) {
    const int n2 = P - n1, items = 2 * n1 + n2;
    const int w = (int)blockIdx.x * GG_BLOCK + (int)threadIdx.x;
    if (w >= items) return;
    const TreeItem it = gg_tree_item(w, n1, set_ptr, B);
    if (it.slide < 0 || it.count_index < 0 || it.count_index >= items) return;
    const int x = coords[2 * (int64_t)it.point], y = coords[2 * (int64_t)it.point + 1];
    const bool ok = gg_valid(x) && gg_valid(y);
    // global node row of a level-2 point q of this slide (q - n1 level-2 nodes precede it; every earlier slide and this one add a root)
    const int row2_shift = set_ptr[it.slide + 1] - n1 + it.slide + 1;
    int h[8], n = 0;
    if (it.section == 0) {
        // github_pretreat.py:106-133: r -> root, root -> r, then the children (a,c), (b,c), (a,d), (b,d) that exist, each both ways
        const int a = cover[4 * (int64_t)it.point], b = cover[4 * (int64_t)it.point + 1];
        const int c = cover[4 * (int64_t)it.point + 2], d = cover[4 * (int64_t)it.point + 3];
        const int cx[4] = {a, b, a, b}, cy[4] = {c, c, d, d};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            h[k] = (gg_valid(cx[k]) && gg_valid(cy[k])) ? gg_find(t, B + it.slide, cx[k], cy[k]) : -1;
            if (h[k] >= 0 && h[k] < n1) h[k] = -1;
            n += h[k] >= 0;
        }
        if (!WRITE) {
            counts[it.count_index] = 2 + 2 * n;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (h[k] >= 0) atomicMax(parent + (h[k] - n1), it.row);           // the last covering level-1 node in order: the largest row
            return;
        }
        if (2 + 2 * n != counts[it.count_index]) return;
        int64_t e = incl[it.count_index] - (2 + 2 * n);
        out_src[e] = it.row; out_dst[e] = it.root; ++e;
        out_src[e] = it.root; out_dst[e] = it.row; ++e;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (h[k] >= 0) {
                const int child = h[k] + row2_shift;
                out_src[e] = it.row; out_dst[e] = child; ++e;
                out_src[e] = child; out_dst[e] = it.row; ++e;
            }
        // the node's own tables, and the root's by the slide's first level-1 node
        node_type[it.row] = 1;
        node_tree[it.row] = it.root;
        xy[2 * (int64_t)it.row] = (double)x / (double)set_max[2 * it.slide];
        xy[2 * (int64_t)it.row + 1] = (double)y / (double)set_max[2 * it.slide + 1];
        if (it.point == it.first1) {
            node_type[it.root] = 0;
            node_tree[it.root] = -1;
            xy[2 * (int64_t)it.root] = 0.0;
            xy[2 * (int64_t)it.root + 1] = 0.0;
        }
        return;
    }
    // sections B and C (:142-170, :173-202): self -> neighbour for the neighbours that exist, in the order of GG_DX / GG_DY
    const int set = it.section == 1 ? it.slide : B + it.slide;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        h[k] = ok ? gg_find(t, set, x + GG_DX[k], y + GG_DY[k]) : -1;
        if (h[k] >= 0 && ((h[k] < n1) != (it.section == 1))) h[k] = -1;
        n += h[k] >= 0;
    }
    if (!WRITE) { counts[it.count_index] = n; return; }
    if (n != counts[it.count_index]) return;
    int64_t e = incl[it.count_index] - n;
    const int shift = it.section == 1 ? it.row - it.point : row2_shift;       // points of one level of one slide are consecutive rows
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (h[k] >= 0) { out_src[e] = it.row; out_dst[e] = h[k] + shift; ++e; }
    if (it.section == 2) {
        const int par = parent[it.point - n1];
        if (par < 0) flags[1] = WSI_GRID_UNCOVERED;                           // a plain store: every writer stores the same word
        node_type[it.row] = 2;
        node_tree[it.row] = par < 0 ? -2 : par;
        xy[2 * (int64_t)it.row] = (double)x / (double)set_max[2 * (B + it.slide)];
        xy[2 * (int64_t)it.row + 1] = (double)y / (double)set_max[2 * (B + it.slide) + 1];
    }
}

static bool power_of_two(int64_t c) { return c > 0 && (c & (c - 1)) == 0; }

static int grid_args(const char* what, int32_t mode, int32_t P, int32_t S, int32_t n1, int32_t capacity) {
    if (mode != WSI_GRID_ADJACENCY && mode != WSI_GRID_TREE) { set_error("%s: unknown mode %d", what, mode); return WSI_EINVAL; }
    if (P < 0 || S < 1 || S > GG_MAX_SETS || !power_of_two(capacity) || (int64_t)capacity < 2 * (int64_t)P || P > (1 << 28)) {
        set_error("%s: bad shape points=%d sets=%d capacity=%d (1 <= sets <= %d, capacity a power of two >= 2 points)", what, P, S, capacity, GG_MAX_SETS);
        return WSI_EINVAL;
    }
    if (mode == WSI_GRID_TREE && (S % 2 != 0 || n1 < 0 || n1 > P)) {
        set_error("%s: a tree call has the sets [level 1 of every slide | level 2 of every slide] and 0 <= n1 <= points; sets=%d n1=%d points=%d", what, S, n1, P);
        return WSI_EINVAL;
    }
    return WSI_OK;
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_grid_index(const int32_t* coords, int32_t num_points, const int32_t* set_ptr, int32_t num_sets, int64_t* keys, int32_t* rows,
                              int32_t capacity, int32_t* set_max, int32_t* flags, void* stream) {
    if (int rc = grid_args("grid_index", WSI_GRID_ADJACENCY, num_points, num_sets, 0, capacity)) return rc;
    if (!keys || !rows || !set_max || !flags || !set_ptr || (num_points > 0 && !coords)) { set_error("grid_index: null pointer"); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(keys, 0xff, (size_t)capacity * sizeof(int64_t), st) != hipSuccess ||                // every slot empty
        hipMemsetAsync(set_max, 0xff, (size_t)num_sets * 2 * sizeof(int32_t), st) != hipSuccess ||         // -1: below every valid coordinate
        hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), st) != hipSuccess)
        return check_launch("grid_index(memset)");
    if (num_points > 0)
        hipLaunchKernelGGL(grid_index_kernel, dim3((num_points + GG_BLOCK - 1) / GG_BLOCK), dim3(GG_BLOCK), 0, st, coords, num_points, set_ptr, num_sets,
                           reinterpret_cast<unsigned long long*>(keys), rows, (uint32_t)capacity - 1u, set_max, flags);
    return check_launch("grid_index");
}

extern "C" int wsi_grid_count(int32_t mode, const int32_t* coords, int32_t num_points, const int32_t* set_ptr, int32_t num_sets, int32_t n1,
                              const int32_t* cover, const int64_t* keys, const int32_t* rows, int32_t capacity, int32_t* counts, int32_t* parent,
                              void* stream) {
    if (int rc = grid_args("grid_count", mode, num_points, num_sets, n1, capacity)) return rc;
    if (num_points == 0) return WSI_OK;
    const bool tree = mode == WSI_GRID_TREE;
    if (!coords || !set_ptr || !keys || !rows || !counts || (tree && ((n1 > 0 && !cover) || (num_points > n1 && !parent)))) {
        set_error("grid_count: null pointer");
        return WSI_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const GridTable t{reinterpret_cast<const unsigned long long*>(keys), rows, (uint32_t)capacity - 1u, num_points};
    if (!tree) {
        hipLaunchKernelGGL(grid_adj_kernel<false>, dim3((num_points + GG_BLOCK - 1) / GG_BLOCK), dim3(GG_BLOCK), 0, st, coords, num_points, set_ptr, num_sets,
                           t, counts, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr);
    } else {
        const int items = num_points + n1;
        if (num_points > n1 && hipMemsetAsync(parent, 0xff, (size_t)(num_points - n1) * sizeof(int32_t), st) != hipSuccess)    // -1: covered by nothing
            return check_launch("grid_count(memset)");
        hipLaunchKernelGGL(grid_tree_kernel<false>, dim3((items + GG_BLOCK - 1) / GG_BLOCK), dim3(GG_BLOCK), 0, st, coords, num_points, set_ptr, num_sets / 2,
                           n1, cover, t, counts, parent, (const int64_t*)nullptr, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t*)nullptr,
                           (int64_t*)nullptr, (int64_t*)nullptr, (double*)nullptr, (int32_t*)nullptr);
    }
    return check_launch("grid_count");
}

extern "C" int wsi_grid_write(int32_t mode, const int32_t* coords, int32_t num_points, const int32_t* set_ptr, int32_t num_sets, int32_t n1,
                              const int32_t* cover, const int64_t* keys, const int32_t* rows, int32_t capacity, const int32_t* counts,
                              const int64_t* offsets_incl, const int32_t* parent, const int32_t* set_max, int64_t* out_a, int64_t* out_b,
                              int64_t* node_type, int64_t* node_tree, double* x_y_index, int32_t* flags, void* stream) {
    if (int rc = grid_args("grid_write", mode, num_points, num_sets, n1, capacity)) return rc;
    if (num_points == 0) return WSI_OK;
    const bool tree = mode == WSI_GRID_TREE;
    if (!coords || !set_ptr || !keys || !rows || !counts || !offsets_incl || !out_a || !out_b ||
        (tree && (!set_max || !node_type || !node_tree || !x_y_index || !flags || (n1 > 0 && !cover) || (num_points > n1 && !parent)))) {
        set_error("grid_write: null pointer");
        return WSI_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const GridTable t{reinterpret_cast<const unsigned long long*>(keys), rows, (uint32_t)capacity - 1u, num_points};
    if (!tree) {
        hipLaunchKernelGGL(grid_adj_kernel<true>, dim3((num_points + GG_BLOCK - 1) / GG_BLOCK), dim3(GG_BLOCK), 0, st, coords, num_points, set_ptr, num_sets,
                           t, const_cast<int32_t*>(counts), offsets_incl, out_a, out_b);
    } else {
        const int items = num_points + n1;
        hipLaunchKernelGGL(grid_tree_kernel<true>, dim3((items + GG_BLOCK - 1) / GG_BLOCK), dim3(GG_BLOCK), 0, st, coords, num_points, set_ptr, num_sets / 2,
                           n1, cover, t, const_cast<int32_t*>(counts), const_cast<int32_t*>(parent), offsets_incl, set_max, out_a, out_b, node_type,
                           node_tree, x_y_index, flags);
    }
    return check_launch("grid_write");
}
