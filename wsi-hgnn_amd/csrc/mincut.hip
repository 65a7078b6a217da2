// Mincut assignment over a sparse adjacency for gfx950 (torch_geometric's dense_mincut_pool, baselines/GTNMIL/models/GraphTransformer.py:67, without
// the dense [B, Nmax, Nmax] adjacency).  Contract: include/wsi_hgnn.h.
//
// Packed layout: the rows of all graphs one after the other, one plan segment per graph; the adjacency is a CSR by row (ptr / idx / optional
// constant weight per entry; repeated entries add up, rows may be empty, nothing is assumed symmetric).  K <= 128 assignment columns: a wave
// owns a row and a lane its columns `lane` and `lane + 64`, so a neighbour's row of s is gathered as one 4 K byte run.
//   forward   pass 1 (rows)  : s = softmax(z), d = sum of the row's weights, chunk partials of d |s|^2
//             pass 2 (edges) : t = A s (entries in CSR order), chunk partials of <s, t>
//             pass 3         : the partials of a graph's chunks summed in chunk order -> num[g], den[g]
//   backward  one pass (rows): t' = A^T s along the CSC side, u = g_s + g_num (t + t') + 2 g_den d s, g_z = s (u - <s, u>)
// Every sum has one order (lanes strided over a row's entries and a fixed butterfly, waves in wave order, chunks in chunk order): no atomics,
// the same bits run after run.  All three row passes wait on dependent 4 K byte gathers (one per adjacency entry), not on arithmetic or on
// the streaming rate: up to MC_SHARE workgroups share a chunk's rows so that a batch of few chunks still fills the chip.
#include "common.h"
#include <math.h>

namespace wsi {

constexpr int MC_THREADS = 256;      // four waves: four rows in flight per workgroup
constexpr int MC_MAX_K = 128;
constexpr int MC_MAX_SHARE = 8;

// the four waves' lane-uniform partial sums, added in wave order by thread 0
__device__ __forceinline__ void mc_block_store(float a, int lane, int wave, float* __restrict__ dst) {
    __shared__ float sh[4];
    if (lane == 0) sh[wave] = a;
    __syncthreads();
    if (threadIdx.x == 0) *dst = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// pass 1: workgroup = (chunk, share y)
__global__ __launch_bounds__(MC_THREADS) void mincut_rows_fwd(const float* __restrict__ z, int64_t ldz, int32_t K,
                                                              const int32_t* __restrict__ ptr, const float* __restrict__ edge_w,
                                                              const int32_t* __restrict__ chunk_row, float* __restrict__ s,
                                                              float* __restrict__ deg, float* __restrict__ pden) {
    const int ch = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r0 = chunk_row[ch], r1 = chunk_row[ch + 1];
    const bool has0 = lane < K, has1 = lane + 64 < K;
    float den = 0.f;
    for (int r = r0 + (int)blockIdx.y * 4 + wave; r < r1; r += 4 * (int)gridDim.y) {
        const float* __restrict__ zr = z + (int64_t)r * ldz;
        const float z0 = has0 ? zr[lane] : -INFINITY, z1 = has1 ? zr[lane + 64] : -INFINITY;
        const float m = wave_max(fmaxf(z0, z1));
        const float e0 = has0 ? expf(z0 - m) : 0.f, e1 = has1 ? expf(z1 - m) : 0.f;
        const float inv = 1.f / wave_sum(e0 + e1);
        const float s0 = e0 * inv, s1 = e1 * inv;
        if (has0) s[(int64_t)r * K + lane] = s0;
        if (has1) s[(int64_t)r * K + lane + 64] = s1;
        const int e_lo = ptr[r], e_hi = ptr[r + 1];
        float d = 0.f;
        if (edge_w) { for (int e = e_lo + lane; e < e_hi; e += 64) d += edge_w[e]; d = wave_sum(d); }
        else d = (float)(e_hi - e_lo);
        if (lane == 0) deg[r] = d;
        den = fmaf(d, wave_sum(fmaf(s0, s0, s1 * s1)), den);
    }
    mc_block_store(den, lane, wave, pden + (int64_t)ch * gridDim.y + blockIdx.y);
}

// out[r] = sum over the entries e of row r of w[e] * s[idx[e]]  (a wave's two columns per lane; entries in order, four gathers in flight)
__device__ __forceinline__ void mc_gather_row(const float* __restrict__ s, int32_t K, const int32_t* __restrict__ idx, const float* __restrict__ w,
                                              int e_lo, int e_hi, int lane, bool has0, bool has1, float& t0, float& t1) {
    t0 = 0.f; t1 = 0.f;
    int e = e_lo;
    for (; e + 4 <= e_hi; e += 4) {
        float a0[4], a1[4], we[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float* __restrict__ sj = s + (int64_t)idx[e + k] * K;
            we[k] = w ? w[e + k] : 1.f;
            a0[k] = has0 ? sj[lane] : 0.f;
            a1[k] = has1 ? sj[lane + 64] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { t0 = fmaf(we[k], a0[k], t0); t1 = fmaf(we[k], a1[k], t1); }
    }
    for (; e < e_hi; ++e) {
        const float* __restrict__ sj = s + (int64_t)idx[e] * K;
        const float we = w ? w[e] : 1.f;
        t0 = fmaf(we, has0 ? sj[lane] : 0.f, t0);
        t1 = fmaf(we, has1 ? sj[lane + 64] : 0.f, t1);
    }
}

// pass 2: workgroup = (chunk, share y)
__global__ __launch_bounds__(MC_THREADS) void mincut_edges_fwd(const float* __restrict__ s, int32_t K, const int32_t* __restrict__ ptr,
                                                               const int32_t* __restrict__ idx, const float* __restrict__ edge_w,
                                                               const int32_t* __restrict__ chunk_row, float* __restrict__ t,
                                                               float* __restrict__ pnum) {
    const int ch = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r0 = chunk_row[ch], r1 = chunk_row[ch + 1];
    const bool has0 = lane < K, has1 = lane + 64 < K;
    float num = 0.f;
    for (int r = r0 + (int)blockIdx.y * 4 + wave; r < r1; r += 4 * (int)gridDim.y) {
        float t0, t1;
        mc_gather_row(s, K, idx, edge_w, ptr[r], ptr[r + 1], lane, has0, has1, t0, t1);
        const float s0 = has0 ? s[(int64_t)r * K + lane] : 0.f, s1 = has1 ? s[(int64_t)r * K + lane + 64] : 0.f;
        if (has0) t[(int64_t)r * K + lane] = t0;
        if (has1) t[(int64_t)r * K + lane + 64] = t1;
        num += wave_sum(fmaf(s0, t0, s1 * t1));
    }
    mc_block_store(num, lane, wave, pnum + (int64_t)ch * gridDim.y + blockIdx.y);
}

// pass 3: one wave per graph; lanes strided over the graph's partials, then the butterfly
__global__ __launch_bounds__(64) void mincut_graph_sums(const float* __restrict__ pnum, const float* __restrict__ pden, int32_t share,
                                                        const int32_t* __restrict__ seg_chunk, float* __restrict__ num, float* __restrict__ den) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int p0 = seg_chunk[g] * share, p1 = seg_chunk[g + 1] * share;
    float a = 0.f, b = 0.f;
    for (int p = p0 + lane; p < p1; p += 64) { a += pnum[p]; b += pden[p]; }
    a = wave_sum(a); b = wave_sum(b);
    if (lane == 0) { num[g] = a; den[g] = b; }
}

// backward: workgroup = (chunk, share y); a wave takes a row
__global__ __launch_bounds__(MC_THREADS) void mincut_rows_bwd(const float* __restrict__ g_s, int64_t ldgs, const float* __restrict__ g_num,
                                                              const float* __restrict__ g_den, const float* __restrict__ s,
                                                              const float* __restrict__ t, const float* __restrict__ deg, int32_t K,
                                                              const int32_t* __restrict__ colptr, const int32_t* __restrict__ csc_dst,
                                                              const float* __restrict__ edge_w_csc, const int32_t* __restrict__ chunk_row,
                                                              const int32_t* __restrict__ chunk_seg, float* __restrict__ g_z) {
    const int ch = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r0 = chunk_row[ch], r1 = chunk_row[ch + 1];
    const int g = chunk_seg[ch];
    const bool has0 = lane < K, has1 = lane + 64 < K;
    const float gn = g_num ? g_num[g] : 0.f, gd2 = g_den ? 2.f * g_den[g] : 0.f;
    for (int r = r0 + (int)blockIdx.y * 4 + wave; r < r1; r += 4 * (int)gridDim.y) {
        float tt0 = 0.f, tt1 = 0.f;
        if (g_num) mc_gather_row(s, K, csc_dst, edge_w_csc, colptr[r], colptr[r + 1], lane, has0, has1, tt0, tt1);
        const int64_t b = (int64_t)r * K;
        const float s0 = has0 ? s[b + lane] : 0.f, s1 = has1 ? s[b + lane + 64] : 0.f;
        const float dd = gd2 * deg[r];
        float u0 = 0.f, u1 = 0.f;
        if (has0) u0 = (g_s ? g_s[(int64_t)r * ldgs + lane] : 0.f) + gn * (t[b + lane] + tt0) + dd * s0;
        if (has1) u1 = (g_s ? g_s[(int64_t)r * ldgs + lane + 64] : 0.f) + gn * (t[b + lane + 64] + tt1) + dd * s1;
        const float dot = wave_sum(fmaf(s0, u0, s1 * u1));
        if (has0) g_z[b + lane] = s0 * (u0 - dot);
        if (has1) g_z[b + lane + 64] = s1 * (u1 - dot);
    }
}

static inline int mc_share(int32_t num_chunks) {
    if (num_chunks <= 0 || num_chunks >= 2048) return 1;
    const int s = 2048 / num_chunks;
    return s > MC_MAX_SHARE ? MC_MAX_SHARE : s;
}

}  // namespace wsi

using namespace wsi;

extern "C" int32_t wsi_mincut_partials(int32_t num_chunks) { return 2 * (num_chunks > 0 ? num_chunks : 0) * mc_share(num_chunks); }

extern "C" int wsi_mincut_fwd(const float* z, int64_t ldz, int32_t n, int32_t K, const int32_t* ptr, const int32_t* idx, const float* edge_w,
                              const int32_t* chunk_row, int32_t num_chunks, const int32_t* seg_chunk, int32_t num_segs,
                              float* s, float* t, float* deg, float* partial, float* num, float* den, void* stream) {
    if (n < 0 || K <= 0 || num_chunks < 0 || num_segs < 0 || ldz < K) { set_error("mincut_fwd: bad argument"); return WSI_EINVAL; }
    if (K > MC_MAX_K) { set_error("mincut_fwd: %d assignment columns (at most %d are compiled)", (int)K, MC_MAX_K); return WSI_ENOSYS; }
    if (num_segs == 0) return WSI_OK;
    if (!seg_chunk || !num || !den || (num_chunks > 0 && (!z || !ptr || !chunk_row || !s || !t || !deg || !partial))) {
        set_error("mincut_fwd: null pointer"); return WSI_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const int share = mc_share(num_chunks);
    float* pnum = partial;
    float* pden = partial + (int64_t)num_chunks * share;
    if (num_chunks) {
        hipLaunchKernelGGL(mincut_rows_fwd, dim3(num_chunks, share), dim3(MC_THREADS), 0, st, z, ldz, K, ptr, edge_w, chunk_row, s, deg, pden);
        hipLaunchKernelGGL(mincut_edges_fwd, dim3(num_chunks, share), dim3(MC_THREADS), 0, st, (const float*)s, K, ptr, idx, edge_w, chunk_row, t, pnum);
    }
    hipLaunchKernelGGL(mincut_graph_sums, dim3(num_segs), dim3(64), 0, st, (const float*)pnum, (const float*)pden, share, seg_chunk, num, den);
    return check_launch("mincut_fwd");
}

extern "C" int wsi_mincut_bwd(const float* g_s, int64_t ldgs, const float* g_num, const float* g_den, const float* s, const float* t,
                              const float* deg, int32_t n, int32_t K, const int32_t* colptr, const int32_t* csc_dst, const float* edge_w_csc,
                              const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks, float* g_z, void* stream) {
    if (n < 0 || K <= 0 || num_chunks < 0 || (g_s && ldgs < K)) { set_error("mincut_bwd: bad argument"); return WSI_EINVAL; }
    if (K > MC_MAX_K) { set_error("mincut_bwd: %d assignment columns (at most %d are compiled)", (int)K, MC_MAX_K); return WSI_ENOSYS; }
    if (num_chunks == 0) return WSI_OK;
    if (!s || !t || !deg || !colptr || !chunk_row || !chunk_seg || !g_z) { set_error("mincut_bwd: null pointer"); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mincut_rows_bwd, dim3(num_chunks, mc_share(num_chunks)), dim3(MC_THREADS), 0, st, g_s, ldgs, g_num, g_den, s, t, deg, K,
                       colptr, csc_dst, edge_w_csc, chunk_row, chunk_seg, g_z);
    return check_launch("mincut_bwd");
}
