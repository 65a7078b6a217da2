// Explanations scored against annotations (wsi_hgnn_amd/localization.py).  Contract: include/wsi_hgnn.h.
//
// wsi_loc_labels: which patch centres lie strictly inside a ring of their own slide's annotation (even-odd rule, boundary excluded), in two
// launches: (tile of 256 centres) x (chunk of <= chunk_edges ring edges) -> one word per (chunk, centre), then per centre the words of its
// slide's chunks folded ring by ring.  wsi_loc_score: per slide and score column the exact Mann-Whitney pair counts and the AUC, in three
// launches.  wsi_loc_owner: which patch owns every pixel of a heat map.  Every quantity is an integer or ONE fp64 operation sequence in a fixed
// order; the only atomic is the integer maximum of the owner image.  Nothing is allocated, nothing read back; identical calls give identical bits.
#include "common.h"
#include <math.h>

namespace wsi {

constexpr int LOC_TILE = WSI_LOC_TILE;

// A tile row: (slide, first row, rows, first row's position within its slide).  A slide row: (first scratch word, rows, first tile).
struct LocTile { int slide, first, count, local; };

__device__ __forceinline__ LocTile loc_tile(const int32_t* __restrict__ tiles, int t) {
    const int4 v = reinterpret_cast<const int4*>(tiles)[t];
    return {v.x, v.y, v.z, v.w};
}

// ---------------------------------------------------------------- labels, pass 1
// word = parity of the crossings of the chunk's edges | 2 * (the centre lies on one of them).  An edge (x0, y0) -> (x1, y1) is crossed iff
// (y0 > y) != (y1 > y) and (o > 0) == (y1 > y0), o = (x1 - x0)(y - y0) - (x - x0)(y1 - y0); the centre is on it iff o == 0 inside the edge's
// closed box.  No division.  A centre outside the ring's closed box gets 0 without looking at an edge; a tile with no centre inside it stages nothing.
__global__ __launch_bounds__(LOC_TILE) void loc_chunk_words_kernel(const double* __restrict__ centres, int num_centres, const int32_t* __restrict__ tiles,
                                                                   const int64_t* __restrict__ slides, const double* __restrict__ vertices,
                                                                   int64_t num_vertices, const int64_t* __restrict__ ring_ptr,
                                                                   const double* __restrict__ ring_box, int num_rings,
                                                                   const int32_t* __restrict__ chunks, int num_chunks,
                                                                   const int32_t* __restrict__ slide_chunk_ptr, int chunk_edges,
                                                                   int32_t* __restrict__ scratch, int64_t scratch_words) {
    __shared__ double2 vert[WSI_LOC_CHUNK_MAX + 1];
    const int tid = threadIdx.x;
    const LocTile T = loc_tile(tiles, blockIdx.x);
    const int k0 = slide_chunk_ptr[T.slide], nk = slide_chunk_ptr[T.slide + 1] - k0;
    if ((int)blockIdx.y >= nk) return;                               // (uniform) this slide has fewer chunks than the widest of the batch
    const int k = k0 + (int)blockIdx.y;
    if (k < 0 || k >= num_chunks) return;
    const int4 ch = reinterpret_cast<const int4*>(chunks)[k];        // (ring, first edge, edges, slide)
    const int ring = ch.x, e0 = ch.y, ne = min(ch.z, chunk_edges);
    const int64_t rows = slides[(int64_t)T.slide * 3 + 1];
    const int64_t at = slides[(int64_t)T.slide * 3] + (int64_t)blockIdx.y * rows + T.local + tid;
    const bool active = tid < T.count && T.first + tid < num_centres && at >= 0 && at < scratch_words;
    double x = 0.0, y = 0.0;
    bool inbox = false;
    const bool ring_ok = ring >= 0 && ring < num_rings && e0 >= 0 && ne >= 0;
    if (active && ring_ok) {
        x = centres[2 * (int64_t)(T.first + tid)];
        y = centres[2 * (int64_t)(T.first + tid) + 1];
        const double* box = ring_box + 4 * (int64_t)ring;
        inbox = x >= box[0] && y >= box[1] && x <= box[2] && y <= box[3];
    }
    if (!__syncthreads_or(inbox ? 1 : 0)) {                          // the reject path: no edge is read
        if (active) scratch[at] = 0;
        return;
    }
    const int64_t v0 = ring_ptr[ring], nv = ring_ptr[ring + 1] - v0;
    for (int j = tid; j <= ne; j += LOC_TILE) {                      // edges e0 .. e0 + ne - 1 need vertices e0 .. e0 + ne; the ring closes on its first
        int64_t idx = (int64_t)e0 + j;
        if (idx >= nv) idx -= nv;
        const int64_t g = v0 + idx;
        const bool ok = idx >= 0 && idx < nv && g >= 0 && g < num_vertices;
        vert[j] = ok ? make_double2(vertices[2 * g], vertices[2 * g + 1]) : make_double2(0.0, 0.0);
    }
    __syncthreads();
    if (!active) return;
    int parity = 0, on_edge = 0;
    if (inbox) {
        double2 a = vert[0];
        for (int e = 0; e < ne; ++e) {                               // every lane reads the same vertex: an LDS broadcast
            const double2 b = vert[e + 1];
            const double o = (b.x - a.x) * (y - a.y) - (x - a.x) * (b.y - a.y);
            const bool up = b.y > a.y;
            parity ^= (((a.y > y) != (b.y > y)) && ((o > 0.0) == up)) ? 1 : 0;
            on_edge |= (o == 0.0 && x >= fmin(a.x, b.x) && x <= fmax(a.x, b.x) && y >= fmin(a.y, b.y) && y <= fmax(a.y, b.y)) ? 1 : 0;
            a = b;
        }
    }
    scratch[at] = parity | (on_edge << 1);
}

// ---------------------------------------------------------------- labels, pass 2
// Per centre: the chunks of its slide in order; parities XORed within a ring, a ring with a flagged chunk contains nothing, rings ORed.
__global__ __launch_bounds__(LOC_TILE) void loc_fold_kernel(int num_centres, const int32_t* __restrict__ tiles, const int64_t* __restrict__ slides,
                                                            const int32_t* __restrict__ chunks, int num_chunks,
                                                            const int32_t* __restrict__ slide_chunk_ptr, const int32_t* __restrict__ scratch,
                                                            int64_t scratch_words, int32_t* __restrict__ labels) {
    const int tid = threadIdx.x;
    const LocTile T = loc_tile(tiles, blockIdx.x);
    if (tid >= T.count || T.first + tid >= num_centres) return;
    const int k0 = slide_chunk_ptr[T.slide];
    const int nk = min(slide_chunk_ptr[T.slide + 1], num_chunks) - k0;
    const int64_t rows = slides[(int64_t)T.slide * 3 + 1];
    const int64_t base = slides[(int64_t)T.slide * 3] + T.local + tid;
    int inside = 0, parity = 0, on_edge = 0, ring = -1;
    for (int j = 0; j < nk; ++j) {
        const int r = chunks[4 * (int64_t)(k0 + j)];                 // (uniform)
        if (r != ring) {
            inside |= parity & (on_edge ^ 1);
            parity = on_edge = 0;
            ring = r;
        }
        const int64_t at = base + (int64_t)j * rows;
        const int w = (at >= 0 && at < scratch_words) ? scratch[at] : 0;
        parity ^= w & 1;
        on_edge |= (w >> 1) & 1;
    }
    inside |= parity & (on_edge ^ 1);
    labels[T.first + tid] = inside;
}

// ---------------------------------------------------------------- pair counting
// Block (tile, column): lane i holds one row of the tile (it takes part iff its label is not 0) and walks every row j of the SAME slide through LDS
// tiles of 256: the score where row j is labelled 0, NaN elsewhere (NaN is neither greater than nor equal to anything: it counts nothing).
// partial[(c * T + tile) * 5 + ..] = #(s_i > s_j), #(s_i == s_j), positives, negatives and non-finite scores among the tile's own rows.
__global__ __launch_bounds__(LOC_TILE) void loc_pairs_kernel(const float* __restrict__ scores, int num_rows, int C, const int32_t* __restrict__ labels,
                                                             const int32_t* __restrict__ tiles, const int64_t* __restrict__ slides,
                                                             int64_t* __restrict__ partial) {
    __shared__ float sc[LOC_TILE];
    __shared__ unsigned long long red[5][LOC_TILE];
    const int tid = threadIdx.x, c = blockIdx.y;
    const LocTile T = loc_tile(tiles, blockIdx.x);
    const int r0 = T.first - T.local;
    const int r1 = (int)min((int64_t)num_rows, r0 + slides[(int64_t)T.slide * 3 + 1]);
    const int i = T.first + tid;
    const bool own = tid < T.count && i < r1 && r0 >= 0;
    const int lab = own ? labels[i] : 0;
    const float si = own ? scores[(int64_t)i * C + c] : 0.f;
    const bool mine = own && lab != 0;
    unsigned long long gt = 0, eq = 0;
    if (__syncthreads_or(mine ? 1 : 0)) {                            // (uniform) a tile without a positive counts no pair
        for (int j0 = max(r0, 0); j0 < r1; j0 += LOC_TILE) {
            const int j = j0 + tid;
            sc[tid] = (j < r1 && labels[j] == 0) ? scores[(int64_t)j * C + c] : NAN;
            __syncthreads();
            if (mine) {
                unsigned g = 0, e = 0;                               // (at most 256 each per tile)
#pragma unroll 8
                for (int k = 0; k < LOC_TILE; ++k) {
                    const float sj = sc[k];
                    g += si > sj ? 1u : 0u;
                    e += si == sj ? 1u : 0u;
                }
                gt += g;
                eq += e;
            }
            __syncthreads();
        }
    }
    red[0][tid] = gt;
    red[1][tid] = eq;
    red[2][tid] = mine ? 1 : 0;
    red[3][tid] = (own && lab == 0) ? 1 : 0;
    red[4][tid] = (own && !isfinite(si)) ? 1 : 0;
    __syncthreads();
    for (int o = LOC_TILE / 2; o > 0; o >>= 1) {
        if (tid < o)
            for (int q = 0; q < 5; ++q) red[q][tid] += red[q][tid + o];
        __syncthreads();
    }
    if (tid < 5) partial[((int64_t)c * gridDim.x + blockIdx.x) * 5 + tid] = (int64_t)red[tid][0];
}

// One thread per (slide, column): the slide's tile partials added in order, then auc = (2 gt + eq) / (2 P N) as one fp64 division.
// counts [B, C, 4] = (P, N, gt, eq); flags [B, C] = WSI_LOC_NONFINITE where a score of the slide is not finite, whose AUC is NaN, as is a one-class slide's.
__global__ __launch_bounds__(64) void loc_auc_kernel(const int64_t* __restrict__ slides, int B, int C, int num_tiles, const int64_t* __restrict__ partial,
                                                     int64_t* __restrict__ counts, int32_t* __restrict__ flags, double* __restrict__ auc) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= B * C) return;
    const int s = idx / C, c = idx - s * C;
    const int64_t rows = slides[(int64_t)s * 3 + 1], t0 = slides[(int64_t)s * 3 + 2];
    const int64_t nt = (rows + LOC_TILE - 1) / LOC_TILE;
    int64_t v[5] = {0, 0, 0, 0, 0};
    for (int64_t t = t0; t < t0 + nt && t < num_tiles; ++t)
        for (int q = 0; q < 5; ++q) v[q] += partial[((int64_t)c * num_tiles + t) * 5 + q];
    const int64_t gt = v[0], eq = v[1], P = v[2], Nn = v[3];
    counts[4 * (int64_t)idx] = P;
    counts[4 * (int64_t)idx + 1] = Nn;
    counts[4 * (int64_t)idx + 2] = gt;
    counts[4 * (int64_t)idx + 3] = eq;
    flags[idx] = v[4] ? WSI_LOC_NONFINITE : 0;
    auc[idx] = (P > 0 && Nn > 0 && !v[4]) ? (double)(2 * gt + eq) / (double)(2 * P * Nn) : (double)NAN;
}

// The sum of n <= 128 values `stride` apart, a NaN counting 0, in the order of numpy's pairwise summation (eight running sums, then the rest).
__device__ double loc_block_sum(const double* __restrict__ a, int64_t stride, int n) {
    auto at = [&](int i) { const double v = a[(int64_t)i * stride]; return v == v ? v : 0.0; };
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += at(i);
        return res;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = at(j);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += at(i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += at(i);
    return res;
}

// mean[c] = the NaN-skipping mean over slides of column c: numpy.nanmean of that vector to the last bit (NaN -> 0, numpy's pairwise order - halves
// cut at a multiple of 8 above 128 values - then one division by the number of values that are not NaN); NaN if there is none.
__global__ __launch_bounds__(64) void loc_mean_kernel(const double* __restrict__ auc, int B, int C, double* __restrict__ mean) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    int off[32], len[32], stage[32];
    double left[32];
    int sp = 0;
    off[0] = 0; len[0] = B; stage[0] = 0;
    double res = 0.0;
    bool have = false;
    while (sp >= 0) {
        const int n2 = (len[sp] / 2) - ((len[sp] / 2) % 8);
        if (!have) {
            if (len[sp] <= 128 || sp >= 30) {
                res = loc_block_sum(auc + (int64_t)off[sp] * C + c, C, len[sp]);
                have = true;
                --sp;
            } else {
                stage[sp] = 1;
                off[sp + 1] = off[sp]; len[sp + 1] = n2; stage[sp + 1] = 0;
                ++sp;
            }
        } else if (stage[sp] == 1) {
            left[sp] = res;
            stage[sp] = 2;
            off[sp + 1] = off[sp] + n2; len[sp + 1] = len[sp] - n2; stage[sp + 1] = 0;
            ++sp;
            have = false;
        } else {
            res = left[sp] + res;
            --sp;
        }
    }
    int64_t cnt = 0;
    for (int s = 0; s < B; ++s) { const double v = auc[(int64_t)s * C + c]; cnt += v == v ? 1 : 0; }
    mean[c] = cnt > 0 ? res / (double)cnt : (double)NAN;
}

// ---------------------------------------------------------------- heat map
// Patch i paints the pixels x .. x + patch, y .. y + patch (inclusive, clipped); where patches overlap the highest index owns the pixel.
__global__ __launch_bounds__(LOC_TILE) void loc_owner_kernel(const int32_t* __restrict__ grid_xy, int num_patches, int patch, int height, int width,
                                                             int32_t* __restrict__ owner) {
    const int i = blockIdx.x;
    const int64_t x0 = grid_xy[2 * (int64_t)i], y0 = grid_xy[2 * (int64_t)i + 1];
    const int side = patch + 1;
    for (int p = threadIdx.x; p < side * side; p += LOC_TILE) {
        const int64_t x = x0 + p % side, y = y0 + p / side;
        if (x >= 0 && x < width && y >= 0 && y < height) atomicMax(&owner[y * width + x], i);
    }
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_loc_labels(const double* centres, int32_t num_centres, const int32_t* tiles, int32_t num_tiles, const int64_t* slides,
                              int32_t num_slides, const double* vertices, int64_t num_vertices, const int64_t* ring_ptr, const double* ring_box,
                              int32_t num_rings, const int32_t* chunks, int32_t num_chunks, const int32_t* slide_chunk_ptr,
                              int32_t max_slide_chunks, int32_t chunk_edges, int32_t* scratch, int64_t scratch_words, int32_t* labels, void* stream) {
    if (num_centres < 0 || num_tiles < 0 || num_slides < 0 || num_vertices < 0 || num_rings < 0 || num_chunks < 0 || max_slide_chunks < 0 ||
        scratch_words < 0) {
        set_error("loc_labels: negative count");
        return WSI_EINVAL;
    }
    if (chunk_edges < 1 || chunk_edges > WSI_LOC_CHUNK_MAX) { set_error("loc_labels: chunk_edges %d outside 1 .. %d", chunk_edges, WSI_LOC_CHUNK_MAX); return WSI_EINVAL; }
    if (max_slide_chunks > WSI_LOC_MAX_SLIDE_CHUNKS) { set_error("loc_labels: %d chunks in one slide (at most %d)", max_slide_chunks, WSI_LOC_MAX_SLIDE_CHUNKS); return WSI_EINVAL; }
    if (num_tiles == 0) return WSI_OK;
    if (!centres || !tiles || !slides || !labels || !slide_chunk_ptr || num_slides == 0 ||
        (num_chunks > 0 && (!vertices || !ring_ptr || !ring_box || !chunks || !scratch))) {
        set_error("loc_labels: null pointer");
        return WSI_EINVAL;
    }
    if (((uintptr_t)tiles & 15) || ((uintptr_t)chunks & 15)) { set_error("loc_labels: the tile and chunk tables are 16-byte aligned"); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    if (num_chunks > 0 && max_slide_chunks > 0) {
        hipLaunchKernelGGL(loc_chunk_words_kernel, dim3(num_tiles, max_slide_chunks), dim3(LOC_TILE), 0, st, centres, (int)num_centres, tiles, slides,
                           vertices, num_vertices, ring_ptr, ring_box, (int)num_rings, chunks, (int)num_chunks, slide_chunk_ptr, (int)chunk_edges,
                           scratch, scratch_words);
        const int rc = check_launch("loc_labels (chunks)");
        if (rc != WSI_OK) return rc;
    }
    hipLaunchKernelGGL(loc_fold_kernel, dim3(num_tiles), dim3(LOC_TILE), 0, st, (int)num_centres, tiles, slides, chunks, (int)num_chunks,
                       slide_chunk_ptr, scratch, scratch_words, labels);
    return check_launch("loc_labels");
}

extern "C" int wsi_loc_score(const float* scores, int32_t num_rows, int32_t C, const int32_t* labels, const int32_t* tiles, int32_t num_tiles,
                             const int64_t* slides, int32_t num_slides, int64_t* partial, int64_t* counts, int32_t* flags, double* auc,
                             double* mean, void* stream) {
    if (num_rows < 0 || num_tiles < 0 || num_slides < 0) { set_error("loc_score: negative count"); return WSI_EINVAL; }
    if (C < 1 || C > WSI_LOC_MAX_COLUMNS) { set_error("loc_score: %d score columns outside 1 .. %d", C, WSI_LOC_MAX_COLUMNS); return WSI_EINVAL; }
    if ((int64_t)num_slides * C > (int64_t)1 << 30) { set_error("loc_score: too many (slide, column) pairs"); return WSI_EINVAL; }
    if (!mean || (num_slides > 0 && (!slides || !counts || !flags || !auc)) || (num_tiles > 0 && (!scores || !labels || !tiles || !partial))) {
        set_error("loc_score: null pointer");
        return WSI_EINVAL;
    }
    if ((uintptr_t)tiles & 15) { set_error("loc_score: the tile table is 16-byte aligned"); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    if (num_tiles > 0) {
        hipLaunchKernelGGL(loc_pairs_kernel, dim3(num_tiles, C), dim3(LOC_TILE), 0, st, scores, (int)num_rows, (int)C, labels, tiles, slides, partial);
        const int rc = check_launch("loc_score (pairs)");
        if (rc != WSI_OK) return rc;
    }
    if (num_slides > 0) {
        hipLaunchKernelGGL(loc_auc_kernel, dim3((num_slides * C + 63) / 64), dim3(64), 0, st, slides, (int)num_slides, (int)C, (int)num_tiles, partial,
                           counts, flags, auc);
        const int rc = check_launch("loc_score (auc)");
        if (rc != WSI_OK) return rc;
    }
    hipLaunchKernelGGL(loc_mean_kernel, dim3((C + 63) / 64), dim3(64), 0, st, auc, (int)num_slides, (int)C, mean);
    return check_launch("loc_score");
}

extern "C" int wsi_loc_owner(const int32_t* grid_xy, int32_t num_patches, int32_t patch, int32_t height, int32_t width, int32_t* owner,
                             void* stream) {
    if (num_patches < 0 || height < 0 || width < 0) { set_error("loc_owner: negative count"); return WSI_EINVAL; }
    if (patch < 0 || patch > WSI_LOC_MAX_PATCH) { set_error("loc_owner: patch %d outside 0 .. %d", patch, WSI_LOC_MAX_PATCH); return WSI_EINVAL; }
    if ((int64_t)height * width >= (int64_t)1 << 31) { set_error("loc_owner: the image has 2^31 pixels or more"); return WSI_EINVAL; }
    if (num_patches == 0 || height == 0 || width == 0) return WSI_OK;
    if (!grid_xy || !owner) { set_error("loc_owner: null pointer"); return WSI_EINVAL; }
    hipLaunchKernelGGL(loc_owner_kernel, dim3(num_patches), dim3(LOC_TILE), 0, (hipStream_t)stream, grid_xy, (int)num_patches, (int)patch, (int)height,
                       (int)width, owner);
    return check_launch("loc_owner");
}
