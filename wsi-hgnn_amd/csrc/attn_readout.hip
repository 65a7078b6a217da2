// Global attention readout for gfx950 (dgl's GlobalAttentionPooling behind graph_pooling_type 'att', models/HEATNet4.py:182-187 and :219,
// models/GCN.py): per segment - the rows of one (node type, graph) - a softmax over the rows of a one-column gate, gate[r] = <x[r], w> + b,
// then the weighted sum of the same rows.  Contract: include/wsi_hgnn.h.
//
// HBM-bound streaming over the chunk tables of wsi_segment_reduce_fwd (chunks never straddle segments), structured like csrc/bag_attn.hip -
// but the gate is a function of the row itself, so the row's dot product is taken in the pass that accumulates the row: x is read ONCE,
// where the composite form (a one-column GEMM, three segmented reductions, an exp and a materialised x * p) reads or writes [rows, D] five times.
//   forward  stage 1: workgroup = chunk.  A wave takes two rows at a time across all of D (16-byte lane loads; w stays in registers), reduces
//                     their dot products across the wave and carries an online softmax of its own - running maximum m, rescaled sum l, rescaled
//                     accumulator.  The four waves' states are merged through LDS in wave order -> partial[chunk, :], m[chunk], l[chunk].
//            stage 2: per (segment, column): M = max m;  L = sum l e^(m - M);  out = sum partial e^(m - M) / L;  stats = (M, log L) kept apart.
//   backward        : delta[s] = <g_out[s], out[s]> in a small leading launch; then workgroup = chunk, and as all of a chunk's rows belong to
//                     one segment, g_out[s] stays in registers beside w: per row one read of x, one dot product, one write of g_x (skipped
//                     when g_x is NULL), and g_gate * x accumulated per wave -> the chunk's partial of g_w | g_b; a last launch adds the
//                     chunks' partials in chunk order.
// No atomics anywhere: the same bits run after run.
#include "common.h"
#include <math.h>

namespace wsi {

constexpr int AR_THREADS = 256;
constexpr int AR_ROWS = 2;            // rows a wave has in flight
constexpr int AR_MAX_D = 2048;        // w, (g_out[s],) the accumulator and the rows in flight are registers: 8 steps of 256 columns at most
constexpr int AR_S2_COLS = 64;

// columns j * 256 + lane * 4 .. + 3 of a D-wide row, for the NV steps j a lane holds
template <int NV>
__device__ __forceinline__ void ar_load_row(float (&v)[NV][4], const float* __restrict__ p, int lane, int D, bool vec) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int col = j * 256 + lane * 4;
        if (j * 256 < D) load4_tail(v[j], p + col, col, D, vec);
        else { v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0.f; }
    }
}

template <int NV>
__device__ __forceinline__ float ar_dot(const float (&a)[NV][4], const float (&b)[NV][4]) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = fmaf(a[j][i], b[j][i], acc);
    }
    return wave_sum(acc);
}

// The four waves' [NV][4] registers summed in wave order into dst[0 .. D): 256 columns a step through sh[4][256].
template <int NV>
__device__ __forceinline__ void ar_merge_waves(const float (&acc)[NV][4], float (*sh)[256], int wave, int lane, int D, float* __restrict__ dst) {
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        if (j * 256 < D) {                       // (uniform)
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 4; ++i) sh[wave][lane * 4 + i] = acc[j][i];
            __syncthreads();
            if (j * 256 + t < D) dst[j * 256 + t] = (sh[0][t] + sh[1][t]) + (sh[2][t] + sh[3][t]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward
template <int NV>
__global__ __launch_bounds__(AR_THREADS) void attn_readout_stage1(const float* __restrict__ x, int64_t ldx, int32_t D, bool vec_x,
                                                                  const float* __restrict__ w, bool vec_w, const float* __restrict__ bias,
                                                                  const int32_t* __restrict__ chunk_row, float* __restrict__ partial,
                                                                  float* __restrict__ pm, float* __restrict__ pl, float* __restrict__ gate) {
    const int ch = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r0 = chunk_row[ch], r1 = chunk_row[ch + 1];
    __shared__ float sh[4][256];
    __shared__ float swm[4], swl[4];
    float wr[NV][4], acc[NV][4];
    ar_load_row<NV>(wr, w, lane, D, vec_w);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = 0.f;
    }
    const float b = bias ? bias[0] : 0.f;
    float m = -INFINITY, l = 0.f;
    for (int rb = r0 + wave * AR_ROWS; rb < r1; rb += 4 * AR_ROWS) {
        float v[AR_ROWS][NV][4], g[AR_ROWS];
#pragma unroll
        for (int k = 0; k < AR_ROWS; ++k) {
            if (rb + k < r1) ar_load_row<NV>(v[k], x + (int64_t)(rb + k) * ldx, lane, D, vec_x);     // (uniform)
        }
#pragma unroll
        for (int k = 0; k < AR_ROWS; ++k) {
            if (rb + k < r1) {
                g[k] = ar_dot<NV>(v[k], wr) + b;
                if (lane == 0) gate[rb + k] = g[k];
                const float mn = fmaxf(m, g[k]);
                const float ms = (mn == -INFINITY) ? 0.f : mn;       // a gate of -inf alone: weight 0, never inf - inf
                const float f = expf(m - ms), p = expf(g[k] - ms);
                l = fmaf(l, f, p);
#pragma unroll
                for (int j = 0; j < NV; ++j) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[j][i] = fmaf(acc[j][i], f, p * v[k][j][i]);
                }
                m = mn;
            }
        }
    }
    // the waves' states under one maximum, then added in wave order
    if (lane == 0) { swm[wave] = m; swl[wave] = l; }
    __syncthreads();
    const float M = fmaxf(fmaxf(swm[0], swm[1]), fmaxf(swm[2], swm[3]));
    const float Ms = (M == -INFINITY) ? 0.f : M;
    const float f = expf(m - Ms);                 // a wave without rows: e^(-inf) = 0
#pragma unroll
    for (int j = 0; j < NV; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] *= f;
    }
    ar_merge_waves<NV>(acc, sh, wave, lane, D, partial + (int64_t)ch * D);
    if (threadIdx.x == 0) {
        pm[ch] = M;
        pl[ch] = (swl[0] * expf(swm[0] - Ms) + swl[1] * expf(swm[1] - Ms)) + (swl[2] * expf(swm[2] - Ms) + swl[3] * expf(swm[3] - Ms));
    }
}

// stage 2: workgroup = (segment, 64 columns); wave w takes the segment's chunks c0 + w, c0 + w + 4, ... in chunk order and the four waves' sums
// are added in wave order (the order of bag_pool_stage2: fixed whatever the launch, four chunk reads in flight per column).
__global__ __launch_bounds__(AR_THREADS) void attn_readout_stage2(const float* __restrict__ partial, const float* __restrict__ pm,
                                                                  const float* __restrict__ pl, int32_t D,
                                                                  const int32_t* __restrict__ seg_chunk, float* __restrict__ out,
                                                                  float* __restrict__ stats) {
    const int s = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int col = blockIdx.y * AR_S2_COLS + lane;
    const bool valid = col < D;
    const int c0 = seg_chunk[s], c1 = seg_chunk[s + 1];
    __shared__ float shm[4], shl[4][AR_S2_COLS], sha[4][AR_S2_COLS];
    float m = -INFINITY;
    for (int ch = c0 + wave; ch < c1; ch += 4) m = fmaxf(m, pm[ch]);
    if (lane == 0) shm[wave] = m;
    __syncthreads();
    const float M = fmaxf(fmaxf(shm[0], shm[1]), fmaxf(shm[2], shm[3]));
    const float Ms = (M == -INFINITY) ? 0.f : M;
    float L = 0.f, a = 0.f;
#pragma unroll 4
    for (int ch = c0 + wave; ch < c1; ch += 4) {
        const float e = expf(pm[ch] - Ms);
        L = fmaf(pl[ch], e, L);
        if (valid) a = fmaf(partial[(int64_t)ch * D + col], e, a);
    }
    shl[wave][lane] = L;
    sha[wave][lane] = a;
    __syncthreads();
    if (wave != 0 || !valid) return;
    L = (shl[0][lane] + shl[1][lane]) + (shl[2][lane] + shl[3][lane]);
    a = (sha[0][lane] + sha[1][lane]) + (sha[2][lane] + sha[3][lane]);
    const bool live = (L != 0.f);                // an empty segment: out = 0, stats = (0, 0)
    out[(int64_t)s * D + col] = live ? a / L : 0.f;
    // the maximum and the log of the rescaled sum stay apart: at gates near -1e4 their float32 sum has lost what the backward needs
    if (col == 0) { stats[(int64_t)s * 2] = live ? Ms : 0.f; stats[(int64_t)s * 2 + 1] = live ? logf(L) : 0.f; }
}

// ------------------------------------------------------------------------------------------------ backward
// delta[s] = <g_out[s, :], out[s, :]>: workgroup = segment
__global__ __launch_bounds__(AR_THREADS) void attn_readout_delta(const float* __restrict__ g_out, const float* __restrict__ out, int32_t D,
                                                                 float* __restrict__ delta) {
    const int64_t base = (int64_t)blockIdx.x * D;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float a = 0.f;
    for (int col = threadIdx.x; col < D; col += AR_THREADS) a = fmaf(g_out[base + col], out[base + col], a);
    a = wave_sum(a);
    __shared__ float sh[4];
    if (lane == 0) sh[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) delta[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// workgroup = chunk -> g_x rows (when asked for) and pwb[chunk, 0 .. D] = the chunk's sum of g_gate[r] * x[r] | g_gate[r]
template <int NV>
__global__ __launch_bounds__(AR_THREADS) void attn_readout_bwd_rows(const float* __restrict__ g_out, bool vec_g, const float* __restrict__ gate,
                                                                    const float* __restrict__ stats, const float* __restrict__ delta,
                                                                    const float* __restrict__ x, int64_t ldx, int32_t D, bool vec_x,
                                                                    const float* __restrict__ w, bool vec_w,
                                                                    const int32_t* __restrict__ chunk_row, const int32_t* __restrict__ chunk_seg,
                                                                    float* __restrict__ g_x, int64_t ldgx, bool vec_gx, float* __restrict__ pwb) {
    const int ch = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r0 = chunk_row[ch], r1 = chunk_row[ch + 1];
    __shared__ float sh[4][256];
    __shared__ float sgb[4];
    float wr[NV][4], gs[NV][4], aw[NV][4];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { aw[j][i] = 0.f; gs[j][i] = 0.f; wr[j][i] = 0.f; }
    }
    float ab = 0.f;
    if (r0 < r1) {                                // (uniform; an empty chunk - the padding of a slot's tables - owns no segment: its partial is 0)
        const int s = chunk_seg[ch];
        ar_load_row<NV>(wr, w, lane, D, vec_w);
        ar_load_row<NV>(gs, g_out + (int64_t)s * D, lane, D, vec_g);
        const float mx = stats[(int64_t)s * 2], logl = stats[(int64_t)s * 2 + 1], dl = delta[s];
        for (int rb = r0 + wave * AR_ROWS; rb < r1; rb += 4 * AR_ROWS) {
            float v[AR_ROWS][NV][4];
#pragma unroll
            for (int k = 0; k < AR_ROWS; ++k) {
                if (rb + k < r1) ar_load_row<NV>(v[k], x + (int64_t)(rb + k) * ldx, lane, D, vec_x);
            }
#pragma unroll
            for (int k = 0; k < AR_ROWS; ++k) {
                if (rb + k < r1) {
                    const float p = expf((gate[rb + k] - mx) - logl);
                    const float gg = p * (ar_dot<NV>(v[k], gs) - dl);
                    ab += gg;
#pragma unroll
                    for (int j = 0; j < NV; ++j) {
                        float o[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            aw[j][i] = fmaf(gg, v[k][j][i], aw[j][i]);
                            o[i] = fmaf(gg, wr[j][i], p * gs[j][i]);
                        }
                        const int col = j * 256 + lane * 4;
                        if (g_x && j * 256 < D) store4_tail(g_x + (int64_t)(rb + k) * ldgx + col, o, col, D, vec_gx);
                    }
                }
            }
        }
    }
    float* __restrict__ dst = pwb + (int64_t)ch * (D + 1);
    ar_merge_waves<NV>(aw, sh, wave, lane, D, dst);
    if (lane == 0) sgb[wave] = ab;
    __syncthreads();
    if (threadIdx.x == 0) dst[D] = (sgb[0] + sgb[1]) + (sgb[2] + sgb[3]);
}

// g_wb[c] = sum over the chunks, in chunk order per wave and the waves in wave order, of pwb[chunk, c]: workgroup = 64 of the D + 1 columns
__global__ __launch_bounds__(AR_THREADS) void attn_readout_bwd_reduce(const float* __restrict__ pwb, int32_t num_chunks, int32_t D1,
                                                                      float* __restrict__ g_wb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * AR_S2_COLS + lane;
    __shared__ float sh[4][AR_S2_COLS];
    float a = 0.f;
    if (col < D1) {
#pragma unroll 4
        for (int ch = wave; ch < num_chunks; ch += 4) a += pwb[(int64_t)ch * D1 + col];
    }
    sh[wave][lane] = a;
    __syncthreads();
    if (wave == 0 && col < D1) g_wb[col] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

static inline int ar_check_d(const char* what, int32_t D) {
    if (D > AR_MAX_D) { set_error("%s: feature width %d (at most %d is compiled)", what, (int)D, AR_MAX_D); return WSI_ENOSYS; }
    return WSI_OK;
}

}  // namespace wsi

using namespace wsi;

// the instantiation with the fewest 256-column steps that covers D
#define AR_DISPATCH_NV(D, KERNEL, ...)                                                                   \
    do {                                                                                                 \
        if ((D) <= 256) hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__);                                      \
        else if ((D) <= 512) hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__);                                 \
        else if ((D) <= 1024) hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__);                                \
        else hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__);                                                 \
    } while (0)

extern "C" int wsi_attn_readout_fwd(const float* x, int64_t ldx, int32_t D, const float* w, const float* bias,
                                    const int32_t* chunk_row, int32_t num_chunks, const int32_t* seg_chunk, int32_t num_segs,
                                    float* partial, float* out, float* gate, float* stats, void* stream) {
    if (D <= 0 || num_chunks < 0 || num_segs < 0 || ldx < D) { set_error("attn_readout_fwd: bad argument"); return WSI_EINVAL; }
    if (int rc = ar_check_d("attn_readout_fwd", D)) return rc;
    if (num_segs == 0) return WSI_OK;
    if (!chunk_row || !seg_chunk || !out || !stats || (num_chunks > 0 && (!x || !w || !partial || !gate))) {
        set_error("attn_readout_fwd: null pointer"); return WSI_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    float* pm = partial + (int64_t)num_chunks * D;
    float* pl = pm + num_chunks;
    if (num_chunks) {
        AR_DISPATCH_NV(D, attn_readout_stage1, dim3(num_chunks), dim3(AR_THREADS), 0, st, x, ldx, D, vec_ok(x, ldx), w, vec_ok(w, 4), bias,
                       chunk_row, partial, pm, pl, gate);
    }
    hipLaunchKernelGGL(attn_readout_stage2, dim3(num_segs, (D + AR_S2_COLS - 1) / AR_S2_COLS), dim3(AR_THREADS), 0, st, (const float*)partial,
                       (const float*)pm, (const float*)pl, D, seg_chunk, out, stats);
    return check_launch("attn_readout_fwd");
}

extern "C" int wsi_attn_readout_bwd(const float* g_out, const float* out, const float* gate, const float* stats,
                                    const float* x, int64_t ldx, int32_t D, const float* w,
                                    const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks, int32_t num_segs,
                                    float* scratch, float* g_x, int64_t ldgx, float* g_wb, void* stream) {
    if (D <= 0 || num_chunks < 0 || num_segs < 0 || ldx < D || (g_x && ldgx < D)) { set_error("attn_readout_bwd: bad argument"); return WSI_EINVAL; }
    if (int rc = ar_check_d("attn_readout_bwd", D)) return rc;
    if (!g_wb || !scratch || (num_chunks > 0 && num_segs > 0 && (!g_out || !out || !gate || !stats || !x || !w || !chunk_row || !chunk_seg))) {
        set_error("attn_readout_bwd: null pointer"); return WSI_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    float* delta = scratch;
    float* pwb = scratch + num_segs;
    if (num_chunks > 0 && num_segs > 0) {
        hipLaunchKernelGGL(attn_readout_delta, dim3(num_segs), dim3(AR_THREADS), 0, st, g_out, out, D, delta);
        AR_DISPATCH_NV(D, attn_readout_bwd_rows, dim3(num_chunks), dim3(AR_THREADS), 0, st, g_out, vec_ok(g_out, D), gate, stats,
                       (const float*)delta, x, ldx, D, vec_ok(x, ldx), w, vec_ok(w, 4), chunk_row, chunk_seg, g_x, ldgx, vec_ok(g_x, ldgx), pwb);
    }
    // (no chunk: the sums are empty and g_w | g_b = 0)
    hipLaunchKernelGGL(attn_readout_bwd_reduce, dim3((D + 1 + AR_S2_COLS - 1) / AR_S2_COLS), dim3(AR_THREADS), 0, st, (const float*)pwb,
                       (num_segs > 0 ? num_chunks : 0), D + 1, g_wb);
    return check_launch("attn_readout_bwd");
}
