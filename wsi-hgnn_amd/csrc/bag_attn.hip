// Bag softmax pooling for gfx950: per segment (bag) and per score column a softmax over the segment's rows followed by the weighted sum
// of a value row - ABMIL's softmax(A) @ H (baselines/ReMix_DSMIL_ABMIL/model/abmil.py:25-28), DSMIL's softmax(Q q_max^T / sqrt(128))^T V
// (model/dsmil.py:50-52) and a global attention readout are this one operation.  Contract: include/wsi_hgnn.h.
//
// HBM-bound streaming over the chunk tables of wsi_segment_reduce_fwd (chunks never straddle segments): every value row is read once with
// 16-byte lane accesses, the weights of a tile of rows are formed once per workgroup in LDS (precise expf: the kernel waits on memory, not
// on the exponentials), and the result is two-stage with a fixed summation order - no atomics, the same bits run after run.
//   forward  stage 1: workgroup = (chunk, 256-column tile): online softmax over the chunk's rows in tiles of BAG_TILE rows - running
//                     maximum m, rescaled sum l and rescaled accumulator per column -> partial[chunk, c, :], m[chunk, c], l[chunk, c]
//            stage 2: per (segment, c, column): M = max m;  L = sum l e^(m - M);  out = sum partial e^(m - M) / L;  lse = M + log L
//                     (M and log L are also written apart - stats - which is what the backward forms its weights from)
//   backward        : delta[s, c] = <g_out[s, c], out[s, c]> in a small leading launch; then every row is independent: a wave takes four
//                     rows at a time across all of D (g_out[s] is re-read from cache, values from memory once, g_values written once).
// The DSMIL score step (scores[r, c] = <Q[r], q_max[seg(r), c]>) and its row gradient are the two small row-wise kernels at the end.
#include "common.h"
#include <math.h>

namespace wsi {

constexpr int BAG_THREADS = 256;
constexpr int BAG_TILE = 128;     // rows whose weights a workgroup holds in LDS at a time (two per lane of the wave that forms them)
constexpr int BAG_ROWS = 4;       // rows a wave of the backward carries through D together: one read of g_out[s] serves four rows

// ------------------------------------------------------------------------------------------------ forward
template <int C>
__global__ __launch_bounds__(BAG_THREADS) void bag_pool_stage1(const float* __restrict__ scores, int64_t lds, float scale,
                                                               const float* __restrict__ values, int64_t ldv, int32_t D, bool vec,
                                                               const int32_t* __restrict__ chunk_row, float* __restrict__ partial,
                                                               float* __restrict__ pm, float* __restrict__ pl) {
    const int ch = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = blockIdx.y * 256 + lane * 4;
    const int r0 = chunk_row[ch], r1 = chunk_row[ch + 1];
    __shared__ float sp[BAG_TILE][C];          // e^(scale * score - running maximum) of the tile's rows
    __shared__ float sm[C], sl[C], sf[C];      // running maximum, rescaled sum, this tile's rescale factor of what came before
    __shared__ float sh[4][256];
    if ((int)threadIdx.x < C) { sm[threadIdx.x] = -INFINITY; sl[threadIdx.x] = 0.f; }
    __syncthreads();
    float acc[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[c][i] = 0.f;
    }
    for (int t0 = r0; t0 < r1; t0 += BAG_TILE) {
        const int nr = min(BAG_TILE, r1 - t0);
        // the tile's weights: wave w forms columns w, w + 4; a lane holds rows lane and lane + 64
        for (int c = wave; c < C; c += 4) {
            float sv[BAG_TILE / 64];
#pragma unroll
            for (int k = 0; k < BAG_TILE / 64; ++k) {
                const int row = lane + 64 * k;
                sv[k] = (row < nr) ? scale * scores[(int64_t)(t0 + row) * lds + c] : -INFINITY;
            }
            float tm = sv[0];
#pragma unroll
            for (int k = 1; k < BAG_TILE / 64; ++k) tm = fmaxf(tm, sv[k]);
            tm = wave_max(tm);
            const float mo = sm[c];
            const float mn = fmaxf(mo, tm);
            const float ms = (mn == -INFINITY) ? 0.f : mn;      // a column of -inf alone: weights 0, never inf - inf
            float ps = 0.f;
#pragma unroll
            for (int k = 0; k < BAG_TILE / 64; ++k) {
                const int row = lane + 64 * k;
                if (row < nr) {
                    const float p = expf(sv[k] - ms);
                    sp[row][c] = p;
                    ps += p;
                }
            }
            ps = wave_sum(ps);
            if (lane == 0) {
                const float f = expf(mo - ms);
                sl[c] = fmaf(sl[c], f, ps);
                sm[c] = mn;
                sf[c] = f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float f = sf[c];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[c][i] *= f;
        }
        if (col < D) {
#pragma unroll 4
            for (int row = wave; row < nr; row += 4) {
                float v[4];
                load4_tail(v, values + (int64_t)(t0 + row) * ldv + col, col, D, vec);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float w = sp[row][c];
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[c][i] = fmaf(w, v[i], acc[c][i]);
                }
            }
        }
        __syncthreads();
    }
    const int t = threadIdx.x;
    const int oc = blockIdx.y * 256 + t;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (c) __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) sh[wave][lane * 4 + i] = acc[c][i];
        __syncthreads();
        if (oc < D) partial[((int64_t)ch * C + c) * D + oc] = (sh[0][t] + sh[1][t]) + (sh[2][t] + sh[3][t]);
    }
    if (blockIdx.y == 0 && t < C) {
        pm[(int64_t)ch * C + t] = sm[t];
        pl[(int64_t)ch * C + t] = sl[t];
    }
}

// stage 2: workgroup = (segment, 64 entries of the flattened [C, D] row); wave w takes the segment's chunks c0 + w, c0 + w + 4, ... in chunk
// order and the four waves' sums are added in wave order: a fixed order whatever the launch, and four chunk reads in flight per column
// (a bag of 10 000 rows has 79 chunks and, at D = 1024, only 1024 columns to spread them over).
constexpr int BAG_S2_COLS = 64;
__global__ __launch_bounds__(BAG_THREADS) void bag_pool_stage2(const float* __restrict__ partial, const float* __restrict__ pm,
                                                               const float* __restrict__ pl, int32_t C, int32_t D,
                                                               const int32_t* __restrict__ seg_chunk, float* __restrict__ out,
                                                               float* __restrict__ lse, float* __restrict__ stats) {
    const int s = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int idx = blockIdx.y * BAG_S2_COLS + lane;
    const bool valid = idx < C * D;
    const int c = valid ? idx / D : 0, col = valid ? idx - c * D : 0;
    const int c0 = seg_chunk[s], c1 = seg_chunk[s + 1];
    __shared__ float shm[4][BAG_S2_COLS], shl[4][BAG_S2_COLS], sha[4][BAG_S2_COLS];
    float m = -INFINITY;
    for (int ch = c0 + wave; ch < c1; ch += 4) m = fmaxf(m, pm[(int64_t)ch * C + c]);
    shm[wave][lane] = m;
    __syncthreads();
    const float M = fmaxf(fmaxf(shm[0][lane], shm[1][lane]), fmaxf(shm[2][lane], shm[3][lane]));
    const float Ms = (M == -INFINITY) ? 0.f : M;
    float L = 0.f, a = 0.f;
#pragma unroll 4
    for (int ch = c0 + wave; ch < c1; ch += 4) {
        const float w = expf(pm[(int64_t)ch * C + c] - Ms);
        L = fmaf(pl[(int64_t)ch * C + c], w, L);
        a = fmaf(partial[((int64_t)ch * C + c) * D + col], w, a);
    }
    shl[wave][lane] = L;
    sha[wave][lane] = a;
    __syncthreads();
    if (wave != 0 || !valid) return;
    L = (shl[0][lane] + shl[1][lane]) + (shl[2][lane] + shl[3][lane]);
    a = (sha[0][lane] + sha[1][lane]) + (sha[2][lane] + sha[3][lane]);
    const bool live = (L != 0.f);            // an empty segment (and a column of -inf alone): out = 0, lse = 0
    out[((int64_t)s * C + c) * D + col] = live ? a / L : 0.f;
    if (col == 0) {
        // the maximum and the log of the rescaled sum are also kept apart: at scores near -1e4 their float32 sum has lost what the backward needs
        const float logl = live ? logf(L) : 0.f, mx = live ? Ms : 0.f;
        lse[(int64_t)s * C + c] = mx + logl;
        if (stats) { stats[((int64_t)s * C + c) * 2] = mx; stats[((int64_t)s * C + c) * 2 + 1] = logl; }
    }
}

// ------------------------------------------------------------------------------------------------ backward
// delta[s, c] = <g_out[s, c, :], out[s, c, :]>: workgroup = (s, c)
__global__ __launch_bounds__(BAG_THREADS) void bag_pool_delta(const float* __restrict__ g_out, const float* __restrict__ out, int32_t D,
                                                              float* __restrict__ delta) {
    const int64_t base = (int64_t)blockIdx.x * D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float a = 0.f;
    for (int col = threadIdx.x; col < D; col += BAG_THREADS) a = fmaf(g_out[base + col], out[base + col], a);
    a = wave_sum(a);
    __shared__ float sh[4];
    if (lane == 0) sh[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) delta[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// workgroup = (chunk, share y of gridDim.y): the chunk's groups of BAG_ROWS rows are dealt round-robin to the 4 * gridDim.y waves (rows are
// independent, so the host picks gridDim.y for the fill alone); a wave takes its group through all of D (lanes: 4 columns each, 256 a step).
template <int C>
__global__ __launch_bounds__(BAG_THREADS) void bag_pool_bwd_rows(const float* __restrict__ g_out, bool vec_g,
                                                                 const float* __restrict__ scores, int64_t lds, float scale,
                                                                 const float* __restrict__ stats, const float* __restrict__ delta,
                                                                 const float* __restrict__ values, int64_t ldv, int32_t D, bool vec_v,
                                                                 const int32_t* __restrict__ chunk_row, const int32_t* __restrict__ chunk_seg,
                                                                 float* __restrict__ g_scores, int64_t ldgs,
                                                                 float* __restrict__ g_values, int64_t ldgv, bool vec_gv) {
    const int ch = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r0 = chunk_row[ch], r1 = chunk_row[ch + 1];
    const int s = chunk_seg[ch];
    const float* __restrict__ gs = g_out + (int64_t)s * C * D;
    const bool want_gs = g_scores != nullptr, want_gv = g_values != nullptr;
    const int mj = lane / C, mc = lane - mj * C;            // the (row of the group, column) whose weight this lane forms
    for (int rb = r0 + ((int)blockIdx.y * 4 + wave) * BAG_ROWS; rb < r1; rb += 4 * BAG_ROWS * (int)gridDim.y) {
        float mine_p = 0.f;
        if (lane < BAG_ROWS * C && rb + mj < r1)
            mine_p = expf((scale * scores[(int64_t)(rb + mj) * lds + mc] - stats[((int64_t)s * C + mc) * 2]) - stats[((int64_t)s * C + mc) * 2 + 1]);
        float p[BAG_ROWS][C], dot[BAG_ROWS][C];
#pragma unroll
        for (int j = 0; j < BAG_ROWS; ++j) {
#pragma unroll
            for (int c = 0; c < C; ++c) { p[j][c] = __shfl(mine_p, j * C + c); dot[j][c] = 0.f; }
        }
        for (int col = lane * 4; col < D; col += 256) {
            float v[BAG_ROWS][4], gv[BAG_ROWS][4];
#pragma unroll
            for (int j = 0; j < BAG_ROWS; ++j) {
                if (rb + j < r1) load4_tail(v[j], values + (int64_t)(rb + j) * ldv + col, col, D, vec_v);
                else { v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0.f; }
#pragma unroll
                for (int i = 0; i < 4; ++i) gv[j][i] = 0.f;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float g[4];
                load4_tail(g, gs + (int64_t)c * D + col, col, D, vec_g);
#pragma unroll
                for (int j = 0; j < BAG_ROWS; ++j) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        dot[j][c] = fmaf(g[i], v[j][i], dot[j][c]);
                        gv[j][i] = fmaf(p[j][c], g[i], gv[j][i]);
                    }
                }
            }
            if (want_gv) {
#pragma unroll
                for (int j = 0; j < BAG_ROWS; ++j)
                    if (rb + j < r1) store4_tail(g_values + (int64_t)(rb + j) * ldgv + col, gv[j], col, D, vec_gv);
            }
        }
        if (want_gs) {                          // (uniform)
            float mine = 0.f;
#pragma unroll
            for (int j = 0; j < BAG_ROWS; ++j) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float tot = wave_sum(dot[j][c]);
                    if (lane == j * C + c) mine = tot;
                }
            }
            if (lane < BAG_ROWS * C && rb + mj < r1)
                g_scores[(int64_t)(rb + mj) * ldgs + mc] = scale * mine_p * (mine - delta[(int64_t)s * C + mc]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ DSMIL score step
// scores[r, c] = <x[r, :], t[seg(r), c, :]>: workgroup = chunk, a wave takes a row at a time.
template <int C>
__global__ __launch_bounds__(BAG_THREADS) void bag_scores_fwd_rows(const float* __restrict__ x, int64_t ldx, int32_t D, bool vec_x,
                                                                   const float* __restrict__ t, bool vec_t,
                                                                   const int32_t* __restrict__ chunk_row, const int32_t* __restrict__ chunk_seg,
                                                                   float* __restrict__ scores, int64_t lds) {
    const int ch = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r0 = chunk_row[ch], r1 = chunk_row[ch + 1];
    const float* __restrict__ ts = t + (int64_t)chunk_seg[ch] * C * D;
    for (int r = r0 + wave; r < r1; r += 4) {
        float dot[C];
#pragma unroll
        for (int c = 0; c < C; ++c) dot[c] = 0.f;
        for (int col = lane * 4; col < D; col += 256) {
            float v[4];
            load4_tail(v, x + (int64_t)r * ldx + col, col, D, vec_x);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float g[4];
                load4_tail(g, ts + (int64_t)c * D + col, col, D, vec_t);
#pragma unroll
                for (int i = 0; i < 4; ++i) dot[c] = fmaf(g[i], v[i], dot[c]);
            }
        }
        float mine = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float tot = wave_sum(dot[c]);
            if (lane == c) mine = tot;
        }
        if (lane < C) scores[(int64_t)r * lds + lane] = mine;
    }
}

// gx[r, :] = sum_c w[r, c] * t[seg(r), c, :]  (+ sum_c w2[r, c] * t2[seg(r), c, :])
template <int C>
__global__ __launch_bounds__(BAG_THREADS) void bag_scores_bwd_rows(const float* __restrict__ w, int64_t ldw, const float* __restrict__ t,
                                                                   const float* __restrict__ w2, int64_t ldw2, const float* __restrict__ t2,
                                                                   int32_t D, bool vec_t,
                                                                   const int32_t* __restrict__ chunk_row, const int32_t* __restrict__ chunk_seg,
                                                                   float* __restrict__ gx, int64_t ldgx, bool vec_gx) {
    const int ch = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r0 = chunk_row[ch], r1 = chunk_row[ch + 1];
    const int64_t tb = (int64_t)chunk_seg[ch] * C * D;
    const bool two = w2 != nullptr;
    for (int r = r0 + wave; r < r1; r += 4) {
        float wr[C], wr2[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            wr[c] = w[(int64_t)r * ldw + c];
            wr2[c] = two ? w2[(int64_t)r * ldw2 + c] : 0.f;
        }
        for (int col = lane * 4; col < D; col += 256) {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float g[4];
                load4_tail(g, t + tb + (int64_t)c * D + col, col, D, vec_t);
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = fmaf(wr[c], g[i], a[i]);
            }
            if (two) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    float g[4];
                    load4_tail(g, t2 + tb + (int64_t)c * D + col, col, D, vec_t);
#pragma unroll
                    for (int i = 0; i < 4; ++i) a[i] = fmaf(wr2[c], g[i], a[i]);
                }
            }
            store4_tail(gx + (int64_t)r * ldgx + col, a, col, D, vec_gx);
        }
    }
}

static inline int bag_check_c(const char* what, int32_t C) {
    if (C > 8) { set_error("%s: %d score columns (at most 8 are compiled)", what, (int)C); return WSI_ENOSYS; }
    return WSI_OK;
}

}  // namespace wsi

using namespace wsi;

#define BAG_DISPATCH_C(C, KERNEL, ...)                                                                   \
    switch (C) {                                                                                         \
        case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;                                       \
        case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;                                       \
        case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break;                                       \
        case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;                                       \
        case 5: hipLaunchKernelGGL(KERNEL<5>, __VA_ARGS__); break;                                       \
        case 6: hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__); break;                                       \
        case 7: hipLaunchKernelGGL(KERNEL<7>, __VA_ARGS__); break;                                       \
        default: hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__); break;                                      \
    }

extern "C" int wsi_bag_softmax_pool_fwd(const float* scores, int64_t lds, int32_t C, float scale,
                                        const float* values, int64_t ldv, int32_t D,
                                        const int32_t* chunk_row, int32_t num_chunks, const int32_t* seg_chunk, int32_t num_segs,
                                        float* partial, float* out, float* lse, float* stats, void* stream) {
    if (D <= 0 || C <= 0 || num_chunks < 0 || num_segs < 0 || lds < C || ldv < D) { set_error("bag_softmax_pool_fwd: bad argument"); return WSI_EINVAL; }
    if (int rc = bag_check_c("bag_softmax_pool_fwd", C)) return rc;
    if (num_segs == 0) return WSI_OK;
    if (!chunk_row || !seg_chunk || !out || !lse || (num_chunks > 0 && (!scores || !values || !partial))) {
        set_error("bag_softmax_pool_fwd: null pointer"); return WSI_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    float* pm = partial + (int64_t)num_chunks * C * D;
    float* pl = pm + (int64_t)num_chunks * C;
    const dim3 g1(num_chunks, (D + 255) / 256), g2(num_segs, (C * D + BAG_S2_COLS - 1) / BAG_S2_COLS);
    if (num_chunks) {
        BAG_DISPATCH_C(C, bag_pool_stage1, g1, dim3(BAG_THREADS), 0, st, scores, lds, scale, values, ldv, D, vec_ok(values, ldv),
                       chunk_row, partial, pm, pl);
    }
    hipLaunchKernelGGL(bag_pool_stage2, g2, dim3(BAG_THREADS), 0, st, (const float*)partial, (const float*)pm, (const float*)pl, C, D,
                       seg_chunk, out, lse, stats);
    return check_launch("bag_softmax_pool_fwd");
}

extern "C" int wsi_bag_softmax_pool_bwd(const float* g_out, const float* out, const float* scores, int64_t lds, int32_t C, float scale,
                                        const float* stats, const float* values, int64_t ldv, int32_t D,
                                        const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks, int32_t num_segs,
                                        float* delta, float* g_scores, int64_t ldgs, float* g_values, int64_t ldgv, void* stream) {
    if (D <= 0 || C <= 0 || num_chunks < 0 || num_segs < 0 || lds < C || ldv < D || (g_scores && ldgs < C) || (g_values && ldgv < D)) {
        set_error("bag_softmax_pool_bwd: bad argument"); return WSI_EINVAL;
    }
    if (int rc = bag_check_c("bag_softmax_pool_bwd", C)) return rc;
    if (num_segs == 0 || num_chunks == 0 || (!g_scores && !g_values)) return WSI_OK;
    if (!g_out || !scores || !stats || !values || !chunk_row || !chunk_seg || (g_scores && (!out || !delta))) {
        set_error("bag_softmax_pool_bwd: null pointer"); return WSI_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    if (g_scores) hipLaunchKernelGGL(bag_pool_delta, dim3(num_segs * C), dim3(BAG_THREADS), 0, st, g_out, out, D, delta);
    // few chunks (one bag of 10 000 rows: 79) would leave most of the chip idle: up to 8 workgroups share a chunk's rows, towards ~2048 in all
    const int share = num_chunks >= 2048 ? 1 : (2048 / num_chunks > 8 ? 8 : 2048 / num_chunks);
    BAG_DISPATCH_C(C, bag_pool_bwd_rows, dim3(num_chunks, share), dim3(BAG_THREADS), 0, st, g_out, vec_ok(g_out, D), scores, lds, scale, stats,
                   (const float*)delta, values, ldv, D, vec_ok(values, ldv), chunk_row, chunk_seg, g_scores, ldgs, g_values, ldgv,
                   vec_ok(g_values, ldgv));
    return check_launch("bag_softmax_pool_bwd");
}

extern "C" int wsi_bag_scores_fwd(const float* x, int64_t ldx, int32_t D, const float* t, int32_t C,
                                  const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks,
                                  float* scores, int64_t lds, void* stream) {
    if (D <= 0 || C <= 0 || num_chunks < 0 || ldx < D || lds < C) { set_error("bag_scores_fwd: bad argument"); return WSI_EINVAL; }
    if (int rc = bag_check_c("bag_scores_fwd", C)) return rc;
    if (num_chunks == 0) return WSI_OK;
    if (!x || !t || !chunk_row || !chunk_seg || !scores) { set_error("bag_scores_fwd: null pointer"); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    BAG_DISPATCH_C(C, bag_scores_fwd_rows, dim3(num_chunks), dim3(BAG_THREADS), 0, st, x, ldx, D, vec_ok(x, ldx), t, vec_ok(t, D),
                   chunk_row, chunk_seg, scores, lds);
    return check_launch("bag_scores_fwd");
}

extern "C" int wsi_bag_scores_bwd(const float* w, int64_t ldw, const float* t, const float* w2, int64_t ldw2, const float* t2,
                                  int32_t C, int32_t D, const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks,
                                  float* gx, int64_t ldgx, void* stream) {
    if (D <= 0 || C <= 0 || num_chunks < 0 || ldw < C || ldgx < D || (w2 && ldw2 < C)) { set_error("bag_scores_bwd: bad argument"); return WSI_EINVAL; }
    if (int rc = bag_check_c("bag_scores_bwd", C)) return rc;
    if (num_chunks == 0) return WSI_OK;
    if (!w || !t || !chunk_row || !chunk_seg || !gx || ((w2 != nullptr) != (t2 != nullptr))) { set_error("bag_scores_bwd: null pointer"); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    BAG_DISPATCH_C(C, bag_scores_bwd_rows, dim3(num_chunks), dim3(BAG_THREADS), 0, st, w, ldw, t, w2, ldw2, t2, D,
                   vec_ok(t, D) && (!t2 || vec_ok(t2, D)), chunk_row, chunk_seg, gx, ldgx, vec_ok(gx, ldgx));
    return check_launch("bag_scores_bwd");
}
