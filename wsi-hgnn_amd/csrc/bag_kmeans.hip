// ReMix on the device for gfx950 (baselines/ReMix_DSMIL_ABMIL: reduce.py, tools/clustering.py, train_remix_k-fold.py:71-107):
//   wsi_bag_kmeans_step : one Lloyd iteration of a k-means over the rows of many bags at once (the reduction's hot path)
//   wsi_remix_nearest   : the closest partner prototype of every prototype of a mixed bag
//   wsi_remix_rows      : every output row of every mixed bag of a step from a row descriptor table
// Contract: include/wsi_hgnn.h.
//
// The k-means step streams the rows once over the chunk tables of wsi_segment_reduce_fwd (chunks never straddle bags), like bag_attn.hip:
//   stage 1: workgroup = chunk.  The bag's K centroids sit in LDS.  Rows go through in tiles of KM_TILE: a wave loads KM_ROWS rows into
//            registers (16 bytes per lane and access), normalises them, forms the K squared distances as sums of (x - c)^2 (no
//            |x|^2 - 2 x.c + |c|^2 cancellation), takes the first minimum and parks the normalised row in an LDS tile.  Then every thread
//            owns four columns and adds the tile's rows, in row order, into the register accumulator of the row's label (the label is
//            uniform over the workgroup: a scalar branch selects the accumulator).  A row is read from memory once; the sums have one
//            fixed order; no atomics.  -> partial[chunk, k, :], the chunk's label counts and its share of the objective
//   stage 2: workgroup = (bag, 64 columns): the bag's chunks are combined in chunk order (four interleaved chains added in a fixed
//            order, as bag_pool_stage2), the means are formed and the empty clusters are split, all on the device.
// Rows wider than 1024 columns take kmeans_stage1_wide: same results to rounding, rows re-read from cache, accumulators in `partial`.
#include "common.h"
#include <math.h>

namespace wsi {

constexpr int KM_THREADS = 256;
constexpr int KM_ROWS = 2;                  // rows a wave carries through the centroids together: one LDS read of a centroid serves both
constexpr int KM_TILE = 4 * KM_ROWS;        // rows of a tile (four waves)
constexpr int KM_WIDE_TILE = 32;            // rows of a tile of the wide path
constexpr int KM_MAX_K = 16;
constexpr int KM_S2_COLS = 64;
constexpr float KM_NORM_EPS = 1e-10f;       // tools/clustering.py:44
constexpr float KM_SPLIT_EPS = 1.f / 1024.f;

// rows of the bag of chunk `ch`
__device__ __forceinline__ int km_bag_rows(const int32_t* __restrict__ chunk_row, const int32_t* __restrict__ seg_chunk, int s) {
    return chunk_row[seg_chunk[s + 1]] - chunk_row[seg_chunk[s]];
}

// ------------------------------------------------------------------------------------------------ stage 1, D <= 256 * NJ <= 1024
// KP: K rounded up to a power of two (the register accumulators are indexed statically); NJ: 256-column groups a lane holds of a row.
template <int KP, int NJ>
__global__ __launch_bounds__(KM_THREADS) void kmeans_stage1(const float* __restrict__ x, int64_t ldx, int32_t D, bool vec_x,
                                                            const float* __restrict__ centroids, int32_t K, bool normalize, bool update,
                                                            const int32_t* __restrict__ chunk_row, const int32_t* __restrict__ chunk_seg,
                                                            const int32_t* __restrict__ seg_chunk, int32_t* __restrict__ labels,
                                                            float* __restrict__ partial, bool vec_p, int32_t* __restrict__ pcount,
                                                            float* __restrict__ pobj) {
    constexpr int W = NJ * 256;
    const int ch = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = chunk_row[ch], r1 = chunk_row[ch + 1];
    const int s = chunk_seg[ch];
    if (km_bag_rows(chunk_row, seg_chunk, s) < K) {          // a bag with fewer rows than clusters: labels 0, nothing else (stage 2 writes its zeros)
        for (int r = r0 + tid; r < r1; r += KM_THREADS) labels[r] = 0;
        return;
    }
    __shared__ __attribute__((aligned(16))) float sc[KP][W];                 // the bag's centroids; 0 beyond K and beyond D
    __shared__ __attribute__((aligned(16))) float st[KM_TILE][W];            // the tile's normalised rows
    __shared__ int slab[KM_TILE];
    __shared__ float sobj[4];
    for (int idx = tid; idx < KP * W; idx += KM_THREADS) {
        const int k = idx / W, col = idx - k * W;
        sc[k][col] = (k < K && col < D) ? centroids[((int64_t)s * K + k) * D + col] : 0.f;
    }
    __syncthreads();
    float acc[KP][4];
    int cnt[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        cnt[k] = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[k][i] = 0.f;
    }
    float obj = 0.f;
    const int pcol = tid * 4;                   // the four columns this thread accumulates
    const bool own = pcol < W;
    for (int t0 = r0; t0 < r1; t0 += KM_TILE) {
        // ---- the tile's rows: distances and labels, a wave takes KM_ROWS rows
        float v[KM_ROWS][NJ][4];
#pragma unroll
        for (int j = 0; j < KM_ROWS; ++j) {
            const int row = t0 + wave * KM_ROWS + j;
#pragma unroll
            for (int g = 0; g < NJ; ++g) {
                const int col = g * 256 + lane * 4;
                if (row < r1 && col < D) load4_tail(v[j][g], x + (int64_t)row * ldx + col, col, D, vec_x);
                else { v[j][g][0] = v[j][g][1] = v[j][g][2] = v[j][g][3] = 0.f; }
            }
        }
        if (normalize) {
#pragma unroll
            for (int j = 0; j < KM_ROWS; ++j) {
                float ss = 0.f;
#pragma unroll
                for (int g = 0; g < NJ; ++g) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) ss = fmaf(v[j][g][i], v[j][g][i], ss);
                }
                const float inv = 1.f / (sqrtf(wave_sum(ss)) + KM_NORM_EPS);        // a zero row stays zero
#pragma unroll
                for (int g = 0; g < NJ; ++g) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[j][g][i] *= inv;
                }
            }
        }
        float best[KM_ROWS];
        int lab[KM_ROWS];
#pragma unroll
        for (int j = 0; j < KM_ROWS; ++j) { best[j] = INFINITY; lab[j] = 0; }
        // all K partial distances first, then their K * KM_ROWS reductions side by side (independent chains hide one another's latency)
        float d[KP][KM_ROWS];
#pragma unroll
        for (int k = 0; k < KP; ++k) {
#pragma unroll
            for (int j = 0; j < KM_ROWS; ++j) d[k][j] = 0.f;
            if (k < K) {
#pragma unroll
                for (int g = 0; g < NJ; ++g) {
                    const float4 c = *reinterpret_cast<const float4*>(&sc[k][g * 256 + lane * 4]);
                    const float cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                    for (int j = 0; j < KM_ROWS; ++j) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float e = v[j][g][i] - cc[i];
                            d[k][j] = fmaf(e, e, d[k][j]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            if (k < K) {
#pragma unroll
                for (int j = 0; j < KM_ROWS; ++j) d[k][j] = wave_sum(d[k][j]);          // the same bits in every lane
            }
        }
#pragma unroll
        for (int k = 0; k < KP; ++k) {
#pragma unroll
            for (int j = 0; j < KM_ROWS; ++j)
                if (k < K && d[k][j] < best[j]) { best[j] = d[k][j]; lab[j] = k; }       // strict: the smallest k wins a tie
        }
#pragma unroll
        for (int j = 0; j < KM_ROWS; ++j) {
            const int t = wave * KM_ROWS + j, row = t0 + t;
            if (row < r1) {
                obj += best[j];
                if (lane == 0) { labels[row] = lab[j]; slab[t] = lab[j]; }
                if (update) {
#pragma unroll
                    for (int g = 0; g < NJ; ++g)
                        *reinterpret_cast<float4*>(&st[t][g * 256 + lane * 4]) = make_float4(v[j][g][0], v[j][g][1], v[j][g][2], v[j][g][3]);
                }
            }
        }
        __syncthreads();
        // ---- the tile's rows in row order into the accumulator of their label: a thread owns four columns
        if (own) {
            const int nt = min(KM_TILE, r1 - t0);
            for (int t = 0; t < nt; ++t) {
                const int l = __builtin_amdgcn_readfirstlane(slab[t]);
                float4 tv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (update) tv = *reinterpret_cast<const float4*>(&st[t][pcol]);
#pragma unroll
                for (int k = 0; k < KP; ++k) {
                    if (l == k) {                                  // (scalar branch)
                        acc[k][0] += tv.x; acc[k][1] += tv.y; acc[k][2] += tv.z; acc[k][3] += tv.w;
                        cnt[k] += 1;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (update && own && pcol < D) {
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < K) store4_tail(partial + ((int64_t)ch * K + k) * D + pcol, acc[k], pcol, D, vec_p);
    }
    if (lane == 0) sobj[wave] = obj;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < K) pcount[(int64_t)ch * K + k] = cnt[k];
        pobj[ch] = (sobj[0] + sobj[1]) + (sobj[2] + sobj[3]);
    }
}

// ------------------------------------------------------------------------------------------------ stage 1, any D (used beyond 1024 columns)
// The same two phases per tile of KM_WIDE_TILE rows, with nothing held across the row: a wave makes one pass over its row for the norm and one
// per centroid for the distance (the re-reads come from cache), and the accumulators are the chunk's own rows of `partial` (a thread owns
// its columns of them, rows are added in row order).  Slower; same contract.
__global__ __launch_bounds__(KM_THREADS) void kmeans_stage1_wide(const float* __restrict__ x, int64_t ldx, int32_t D, bool vec_x,
                                                                 const float* __restrict__ centroids, bool vec_c, int32_t K, bool normalize,
                                                                 bool update, const int32_t* __restrict__ chunk_row,
                                                                 const int32_t* __restrict__ chunk_seg, const int32_t* __restrict__ seg_chunk,
                                                                 int32_t* __restrict__ labels, float* __restrict__ partial,
                                                                 int32_t* __restrict__ pcount, float* __restrict__ pobj) {
    const int ch = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r0 = chunk_row[ch], r1 = chunk_row[ch + 1];
    const int s = chunk_seg[ch];
    if (km_bag_rows(chunk_row, seg_chunk, s) < K) {
        for (int r = r0 + tid; r < r1; r += KM_THREADS) labels[r] = 0;
        return;
    }
    __shared__ int slab[KM_WIDE_TILE];
    __shared__ float sinv[KM_WIDE_TILE];
    __shared__ int scnt[KM_MAX_K];
    __shared__ float sobj[4];
    const float* __restrict__ cen = centroids + (int64_t)s * K * D;
    float* __restrict__ mine = partial + (int64_t)ch * K * D;
    if (update)
        for (int64_t i = tid; i < (int64_t)K * D; i += KM_THREADS) mine[i] = 0.f;
    if (tid < KM_MAX_K) scnt[tid] = 0;
    float obj = 0.f;
    __syncthreads();
    for (int t0 = r0; t0 < r1; t0 += KM_WIDE_TILE) {
        const int nt = min(KM_WIDE_TILE, r1 - t0);
        for (int t = wave; t < nt; t += 4) {
            const float* __restrict__ xr = x + (int64_t)(t0 + t) * ldx;
            float inv = 1.f;
            if (normalize) {
                float ss = 0.f;
                for (int col = lane * 4; col < D; col += 256) {
                    float v[4];
                    load4_tail(v, xr + col, col, D, vec_x);
#pragma unroll
                    for (int i = 0; i < 4; ++i) ss = fmaf(v[i], v[i], ss);
                }
                inv = 1.f / (sqrtf(wave_sum(ss)) + KM_NORM_EPS);
            }
            float best = INFINITY;
            int lab = 0;
            for (int k = 0; k < K; ++k) {
                float d = 0.f;
                for (int col = lane * 4; col < D; col += 256) {
                    float v[4], c[4];
                    load4_tail(v, xr + col, col, D, vec_x);
                    load4_tail(c, cen + (int64_t)k * D + col, col, D, vec_c);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float e = v[i] * inv - c[i];
                        d = fmaf(e, e, d);
                    }
                }
                d = wave_sum(d);
                if (d < best) { best = d; lab = k; }
            }
            obj += best;
            if (lane == 0) { labels[t0 + t] = lab; slab[t] = lab; sinv[t] = inv; }
        }
        __syncthreads();
        if (update) {
            for (int col = tid; col < D; col += KM_THREADS) {
                for (int t = 0; t < nt; ++t) {
                    float* __restrict__ p = mine + (int64_t)slab[t] * D + col;
                    *p += x[(int64_t)(t0 + t) * ldx + col] * sinv[t];
                }
            }
        }
        if (tid == 0)
            for (int t = 0; t < nt; ++t) scnt[slab[t]] += 1;
        __syncthreads();
    }
    if (lane == 0) sobj[wave] = obj;
    __syncthreads();
    if (tid < K) pcount[(int64_t)ch * K + tid] = scnt[tid];
    if (tid == 0) pobj[ch] = (sobj[0] + sobj[1]) + (sobj[2] + sobj[3]);
}

// ------------------------------------------------------------------------------------------------ stage 2
// workgroup = (bag, KM_S2_COLS columns); wave w takes the bag's chunks c0 + w, c0 + w + 4, ... in chunk order, the four chains are added in
// wave order.  Wave 0 then forms the means and walks the empty clusters (every lane makes the same decisions from the same counts).
__global__ __launch_bounds__(KM_THREADS) void kmeans_stage2(const float* __restrict__ partial, const int32_t* __restrict__ pcount,
                                                            const float* __restrict__ pobj, int32_t K, int32_t D,
                                                            const int32_t* __restrict__ chunk_row, const int32_t* __restrict__ seg_chunk,
                                                            int32_t* __restrict__ counts, float* __restrict__ objective,
                                                            float* __restrict__ new_centroids) {
    const int s = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = blockIdx.y * KM_S2_COLS + lane;
    const bool valid = col < D;
    const bool first = blockIdx.y == 0;
    const bool update = new_centroids != nullptr;
    const int c0 = seg_chunk[s], c1 = seg_chunk[s + 1];
    __shared__ float sa[4][KM_MAX_K][KM_S2_COLS];
    __shared__ float sm[KM_MAX_K][KM_S2_COLS];
    __shared__ int scn[4][KM_MAX_K];
    __shared__ int stot[KM_MAX_K];
    if (chunk_row[c1] - chunk_row[c0] < K) {                   // fewer rows than clusters: every output of the bag is 0
        if (wave == 0) {
            if (update && valid)
                for (int k = 0; k < K; ++k) new_centroids[((int64_t)s * K + k) * D + col] = 0.f;
            if (first && lane < K) counts[(int64_t)s * K + lane] = 0;
            if (first && lane == 0) objective[s] = 0.f;
        }
        return;
    }
    if (lane < K) {
        int c = 0;
        for (int ch = c0 + wave; ch < c1; ch += 4) c += pcount[(int64_t)ch * K + lane];
        scn[wave][lane] = c;
    }
    if (update) {
        for (int k = 0; k < K; ++k) {
            float a = 0.f;
            if (valid)
                for (int ch = c0 + wave; ch < c1; ch += 4) a += partial[((int64_t)ch * K + k) * D + col];
            sa[wave][k][lane] = a;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    for (int k = 0; k < K; ++k) {
        const int c = (scn[0][k] + scn[1][k]) + (scn[2][k] + scn[3][k]);
        stot[k] = c;                                           // (every lane stores the same value)
        if (update) sm[k][lane] = c > 0 ? ((sa[0][k][lane] + sa[1][k][lane]) + (sa[2][k][lane] + sa[3][k][lane])) / (float)c : 0.f;
    }
    if (update) {
        // faiss's split of an empty cluster with a deterministic donor: the largest current count, the lowest index on a tie
        const float e = (col & 1) ? -KM_SPLIT_EPS : KM_SPLIT_EPS;
        for (int k = 0; k < K; ++k) {
            if (stot[k] != 0) continue;
            int donor = 0, most = 0;
            for (int j = 0; j < K; ++j)
                if (stot[j] > most) { most = stot[j]; donor = j; }
            const float cd = sm[donor][lane];
            sm[k][lane] = cd * (1.f + e);
            sm[donor][lane] = cd * (1.f - e);
            const int half = most / 2;
            stot[k] = half;
            stot[donor] = most - half;
        }
        if (valid)
            for (int k = 0; k < K; ++k) new_centroids[((int64_t)s * K + k) * D + col] = sm[k][lane];
    }
    if (first && lane < K) counts[(int64_t)s * K + lane] = stot[lane];
    if (first && lane == 0) {
        float o = 0.f;
        for (int ch = c0; ch < c1; ++ch) o += pobj[ch];
        objective[s] = o;
    }
}

// ------------------------------------------------------------------------------------------------ mixing
// nearest[b, i] = first minimum over j of |P[src[b], i] - P[tgt[b], j]|^2: workgroup = mixed bag, a wave takes a pair (i, j) at a time
__global__ __launch_bounds__(KM_THREADS) void remix_nearest_kernel(const float* __restrict__ protos, int32_t S, int32_t K, int32_t D, bool vec,
                                                                   const int32_t* __restrict__ src, const int32_t* __restrict__ tgt,
                                                                   int32_t* __restrict__ nearest) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sb = src[b], tb = tgt[b];
    if ((unsigned)sb >= (unsigned)S || (unsigned)tb >= (unsigned)S) {          // an index outside the bank: no read, the row of zeros
        if ((int)threadIdx.x < K) nearest[(int64_t)b * K + threadIdx.x] = 0;
        return;
    }
    const float* __restrict__ sp = protos + (int64_t)sb * K * D;
    const float* __restrict__ tp = protos + (int64_t)tb * K * D;
    __shared__ float sd[KM_MAX_K * KM_MAX_K];
    for (int p = wave; p < K * K; p += 4) {
        const int i = p / K, j = p - i * K;
        float d = 0.f;
        for (int col = lane * 4; col < D; col += 256) {
            float a[4], c[4];
            load4_tail(a, sp + (int64_t)i * D + col, col, D, vec);
            load4_tail(c, tp + (int64_t)j * D + col, col, D, vec);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float e = a[q] - c[q];
                d = fmaf(e, e, d);
            }
        }
        d = wave_sum(d);
        if (lane == 0) sd[p] = d;
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        const int i = threadIdx.x;
        float best = sd[i * K];
        int at = 0;
        for (int j = 1; j < K; ++j)
            if (sd[i * K + j] < best) { best = sd[i * K + j]; at = j; }
        nearest[(int64_t)b * K + i] = at;
    }
}

// one output row per workgroup, from its descriptor of 8 words [op, slot, src_row, partner, replaced, v, bits(lambda), bits(1 - lambda)]
__global__ __launch_bounds__(KM_THREADS) void remix_rows_kernel(const float* __restrict__ protos, const float* __restrict__ shifts, int32_t S,
                                                                int32_t K, int32_t V, int32_t D, const int32_t* __restrict__ nearest,
                                                                int32_t num_slots, const int32_t* __restrict__ desc, float* __restrict__ out) {
    const int o = blockIdx.x;
    const int32_t* __restrict__ d = desc + (int64_t)o * 8;
    const int op = d[0], slot = d[1], src_row = d[2], partner = d[3], replaced = d[4], v = d[5];
    const float lam = __int_as_float(d[6]), oml = __int_as_float(d[7]);
    float* __restrict__ orow = out + (int64_t)o * D;
    const bool needs_partner = op != WSI_REMIX_KEEP || replaced;
    bool ok = (unsigned)src_row < (unsigned)(S * K) && op >= WSI_REMIX_KEEP && op <= WSI_REMIX_COV;
    int c = 0;
    if (needs_partner) {
        ok = ok && (unsigned)slot < (unsigned)num_slots && (unsigned)partner < (unsigned)S;
        if (ok) c = nearest[slot];
        ok = ok && (unsigned)c < (unsigned)K;
    }
    if (op == WSI_REMIX_COV) ok = ok && shifts != nullptr && (unsigned)v < (unsigned)V;
    if (!ok) {                                                   // a descriptor that points outside the bank: no read, a row of zeros
        for (int col = threadIdx.x; col < D; col += KM_THREADS) orow[col] = 0.f;
        return;
    }
    const float* __restrict__ tgt = protos + ((int64_t)partner * K + c) * D;
    const float* __restrict__ cur = replaced ? tgt : protos + (int64_t)src_row * D;
    const float* __restrict__ sh = op == WSI_REMIX_COV ? shifts + (((int64_t)partner * K + c) * V + v) * D : nullptr;
    for (int col = threadIdx.x; col < D; col += KM_THREADS) {
        float r;
        if (op == WSI_REMIX_KEEP) r = cur[col];
        else if (op == WSI_REMIX_APPEND) r = tgt[col];
        else if (op == WSI_REMIX_INTERPOLATE) r = __fadd_rn(__fmul_rn(oml, cur[col]), __fmul_rn(lam, tgt[col]));   // two products, one sum: numpy's order
        else r = __fadd_rn(cur[col], __fmul_rn(lam, sh[col]));
        orow[col] = r;
    }
}

}  // namespace wsi

using namespace wsi;

#define KM_LAUNCH(KP, NJ) hipLaunchKernelGGL((kmeans_stage1<KP, NJ>), dim3(num_chunks), dim3(KM_THREADS), 0, st, x, ldx, D, vec_ok(x, ldx),  \
                                             centroids, K, normalize != 0, update, chunk_row, chunk_seg, seg_chunk, labels, partial,              \
                                             vec_ok(partial, D), pcount, pobj)
#define KM_DISPATCH_NJ(KP)                                                                                \
    if (D <= 256) KM_LAUNCH(KP, 1); else if (D <= 512) KM_LAUNCH(KP, 2); else KM_LAUNCH(KP, 4)

extern "C" int wsi_bag_kmeans_step(const float* x, int64_t ldx, int32_t D, const float* centroids, int32_t K, int32_t normalize,
                                   const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks,
                                   const int32_t* seg_chunk, int32_t num_segs, float* partial,
                                   int32_t* labels, int32_t* counts, float* objective, float* new_centroids, void* stream) {
    if (D <= 0 || K <= 0 || num_chunks < 0 || num_segs < 0 || ldx < D) { set_error("bag_kmeans_step: bad argument"); return WSI_EINVAL; }
    if (K > KM_MAX_K) { set_error("bag_kmeans_step: %d clusters (at most %d are compiled)", (int)K, KM_MAX_K); return WSI_ENOSYS; }
    if (num_segs == 0) return WSI_OK;
    if (!centroids || !chunk_row || !seg_chunk || !counts || !objective || !partial || (num_chunks > 0 && (!x || !chunk_seg || !labels))) {
        set_error("bag_kmeans_step: null pointer"); return WSI_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool update = new_centroids != nullptr;
    int32_t* pcount = reinterpret_cast<int32_t*>(partial + (int64_t)num_chunks * K * D);
    float* pobj = partial + (int64_t)num_chunks * K * (D + 1);
    if (num_chunks) {
        if (D > 1024) {
            hipLaunchKernelGGL(kmeans_stage1_wide, dim3(num_chunks), dim3(KM_THREADS), 0, st, x, ldx, D, vec_ok(x, ldx), centroids,
                               vec_ok(centroids, D), K, normalize != 0, update, chunk_row, chunk_seg, seg_chunk, labels, partial, pcount, pobj);
        } else if (K <= 2) { KM_DISPATCH_NJ(2); }
        else if (K <= 4) { KM_DISPATCH_NJ(4); }
        else if (K <= 8) { KM_DISPATCH_NJ(8); }
        else { KM_DISPATCH_NJ(16); }
    }
    hipLaunchKernelGGL(kmeans_stage2, dim3(num_segs, (D + KM_S2_COLS - 1) / KM_S2_COLS), dim3(KM_THREADS), 0, st, (const float*)partial,
                       (const int32_t*)pcount, (const float*)pobj, K, D, chunk_row, seg_chunk, counts, objective, new_centroids);
    return check_launch("bag_kmeans_step");
}

extern "C" int wsi_remix_nearest(const float* protos, int32_t S, int32_t K, int32_t D, const int32_t* src, const int32_t* tgt, int32_t B,
                                 int32_t* nearest, void* stream) {
    if (S < 0 || K <= 0 || D <= 0 || B < 0) { set_error("remix_nearest: bad argument"); return WSI_EINVAL; }
    if (K > KM_MAX_K) { set_error("remix_nearest: %d prototypes per bag (at most %d are compiled)", (int)K, KM_MAX_K); return WSI_ENOSYS; }
    if (B == 0) return WSI_OK;
    if (!protos || !src || !tgt || !nearest) { set_error("remix_nearest: null pointer"); return WSI_EINVAL; }
    hipLaunchKernelGGL(remix_nearest_kernel, dim3(B), dim3(KM_THREADS), 0, (hipStream_t)stream, protos, S, K, D, vec_ok(protos, D), src, tgt,
                       nearest);
    return check_launch("remix_nearest");
}

extern "C" int wsi_remix_rows(const float* protos, const float* shifts, int32_t S, int32_t K, int32_t V, int32_t D,
                              const int32_t* nearest, int32_t num_slots, const int32_t* desc, int32_t rows, float* out, void* stream) {
    if (S < 0 || K <= 0 || D <= 0 || V < 0 || rows < 0 || num_slots < 0) { set_error("remix_rows: bad argument"); return WSI_EINVAL; }
    if (rows == 0) return WSI_OK;
    if (!protos || !desc || !out || (num_slots > 0 && !nearest)) { set_error("remix_rows: null pointer"); return WSI_EINVAL; }
    hipLaunchKernelGGL(remix_rows_kernel, dim3(rows), dim3(KM_THREADS), 0, (hipStream_t)stream, protos, shifts, S, K, V, D, nearest, num_slots,
                       desc, out);
    return check_launch("remix_rows");
}
