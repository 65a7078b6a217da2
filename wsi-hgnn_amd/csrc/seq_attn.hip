// Multi-head attention over a short sequence for gfx950: the attention of baselines/GTNMIL/models/ViT.py:183-215 (101 tokens, 8 heads of 8) in one
// launch per direction.  Contract: include/wsi_hgnn.h.
//
// Workgroup = one (sequence b, head h): q, k, v of the head (n <= 128 rows of d in {8, 16} floats: at most 24 KB, 40 KB in the backward with
// g_out) are staged in LDS with 16-byte accesses and every score is recomputed from there - the [n, n] probabilities never exist in memory.
// Four consecutive lanes share a query row (the backward's second phase: a key row) and split the other index four ways (j = part, part + 4,
// ...); their partial results meet through two DPP quad steps, so every sum has one order: no atomics, the same bits run after run.
//   forward   : m_i = max_j s_ij, l_i = sum_j e^(s_ij - m_i), out_i = sum_j e^(s_ij - m_i) v_j / l_i, lse_i = m_i + log l_i  (s = scale q k^T)
//   backward  : P_ij = e^(s_ij - lse_i), dP_ij = <g_out_i, v_j>, delta_i = sum_j P_ij dP_ij, dS_ij = P_ij (dP_ij - delta_i)
//               phase 1 (query rows): delta_i, then g_q_i = scale sum_j dS_ij k_j
//               phase 2 (key rows)  : g_v_j = sum_i P_ij g_out_i, g_k_j = scale sum_i dS_ij q_i
// The grid is B * H workgroups (64 at the reference's B = 8): the launch is bound by its own latency - the dependent LDS reads and
// exponentials of one workgroup - not by memory or arithmetic; it replaces a chain of launches, which is where its time is won.
#include "common.h"
#include <math.h>

namespace wsi {

constexpr int SA_MAX_N = 128;
constexpr int SA_THREADS = 4 * SA_MAX_N;

template <int D>
__global__ __launch_bounds__(SA_THREADS) void seq_attn_fwd(const float* __restrict__ qkv, int32_t n, int32_t H, float scale,
                                                           float* __restrict__ out, float* __restrict__ lse) {
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int64_t ld = 3 * (int64_t)H * D;
    const float* __restrict__ base = qkv + (int64_t)b * n * ld + h * D;
    __shared__ __attribute__((aligned(16))) float sq[SA_MAX_N * D], sk[SA_MAX_N * D], sv[SA_MAX_N * D];
    stage_rows<D, SA_THREADS>(sq, base, ld, n);
    stage_rows<D, SA_THREADS>(sk, base + (int64_t)H * D, ld, n);
    stage_rows<D, SA_THREADS>(sv, base + 2 * (int64_t)H * D, ld, n);
    __syncthreads();
    const int i = threadIdx.x >> 2, part = threadIdx.x & 3;
    if (i >= n) return;                                   // (whole quads leave together; no barrier follows)
    float q[D];
#pragma unroll
    for (int c = 0; c < D; ++c) q[c] = sq[i * D + c] * scale;
    float m = -INFINITY;
    for (int j = part; j < n; j += 4) m = fmaxf(m, dot4<D>(q, sk + j * D));
    m = group_max<4>(m);                                   // (n >= 1: key 0 belongs to part 0, so the quad's maximum is finite)
    float l = 0.f, acc[D];
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = 0.f;
    for (int j = part; j < n; j += 4) {
        const float p = expf(dot4<D>(q, sk + j * D) - m);
        l += p;
#pragma unroll
        for (int c = 0; c < D; ++c) acc[c] = fmaf(p, sv[j * D + c], acc[c]);
    }
    l = group_sum<4>(l);
    const float inv = 1.f / l;
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = group_sum<4>(acc[c]) * inv;
    // the quad's four lanes write a quarter of the row each
    float* __restrict__ o = out + ((int64_t)b * n + i) * H * D + h * D;
#pragma unroll
    for (int c = 0; c < D; ++c)
        if (c / (D / 4) == part) o[c] = acc[c];
    if (part == 0) lse[((int64_t)b * H + h) * n + i] = m + logf(l);
}

template <int D>
__global__ __launch_bounds__(SA_THREADS) void seq_attn_bwd(const float* __restrict__ g_out, const float* __restrict__ qkv,
                                                           const float* __restrict__ lse, int32_t n, int32_t H, float scale,
                                                           float* __restrict__ g_qkv) {
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int64_t ld = 3 * (int64_t)H * D;
    const float* __restrict__ base = qkv + (int64_t)b * n * ld + h * D;
    float* __restrict__ gbase = g_qkv + (int64_t)b * n * ld + h * D;
    __shared__ __attribute__((aligned(16))) float sq[SA_MAX_N * D], sk[SA_MAX_N * D], sv[SA_MAX_N * D], sg[SA_MAX_N * D];
    __shared__ float sl[SA_MAX_N], sd[SA_MAX_N];
    stage_rows<D, SA_THREADS>(sq, base, ld, n);
    stage_rows<D, SA_THREADS>(sk, base + (int64_t)H * D, ld, n);
    stage_rows<D, SA_THREADS>(sv, base + 2 * (int64_t)H * D, ld, n);
    stage_rows<D, SA_THREADS>(sg, g_out + (int64_t)b * n * H * D + h * D, (int64_t)H * D, n);
    if ((int)threadIdx.x < n) sl[threadIdx.x] = lse[((int64_t)b * H + h) * n + threadIdx.x];
    __syncthreads();
    const int i = threadIdx.x >> 2, part = threadIdx.x & 3;
    const bool live = i < n;
    // ---- phase 1: this quad's query row i
    if (live) {
        float q[D], g[D];
#pragma unroll
        for (int c = 0; c < D; ++c) { q[c] = sq[i * D + c] * scale; g[c] = sg[i * D + c]; }
        const float li = sl[i];
        float delta = 0.f;
        for (int j = part; j < n; j += 4) delta = fmaf(expf(dot4<D>(q, sk + j * D) - li), dot4<D>(g, sv + j * D), delta);
        delta = group_sum<4>(delta);
        if (part == 0) sd[i] = delta;
        float gq[D];
#pragma unroll
        for (int c = 0; c < D; ++c) gq[c] = 0.f;
        for (int j = part; j < n; j += 4) {
            const float ds = expf(dot4<D>(q, sk + j * D) - li) * (dot4<D>(g, sv + j * D) - delta);
#pragma unroll
            for (int c = 0; c < D; ++c) gq[c] = fmaf(ds, sk[j * D + c], gq[c]);
        }
        float* __restrict__ o = gbase + (int64_t)i * ld;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const float tot = group_sum<4>(gq[c]) * scale;
            if (c / (D / 4) == part) o[c] = tot;
        }
    }
    __syncthreads();
    // ---- phase 2: this quad's key row j = i
    if (!live) return;
    float kj[D], vj[D], gk[D], gv[D];
#pragma unroll
    for (int c = 0; c < D; ++c) { kj[c] = sk[i * D + c] * scale; vj[c] = sv[i * D + c]; gk[c] = 0.f; gv[c] = 0.f; }
    for (int r = part; r < n; r += 4) {
        const float p = expf(dot4<D>(kj, sq + r * D) - sl[r]);
        const float ds = p * (dot4<D>(vj, sg + r * D) - sd[r]);
#pragma unroll
        for (int c = 0; c < D; ++c) { gv[c] = fmaf(p, sg[r * D + c], gv[c]); gk[c] = fmaf(ds, sq[r * D + c], gk[c]); }
    }
    float* __restrict__ ok = gbase + (int64_t)i * ld + (int64_t)H * D;
    float* __restrict__ ov = gbase + (int64_t)i * ld + 2 * (int64_t)H * D;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const float tk = group_sum<4>(gk[c]) * scale, tv = group_sum<4>(gv[c]);
        if (c / (D / 4) == part) { ok[c] = tk; ov[c] = tv; }
    }
}

static inline int sa_check(const char* what, int32_t B, int32_t n, int32_t H, int32_t d) {
    if (B < 0 || n < 0 || H <= 0 || d <= 0) { set_error("%s: bad argument", what); return WSI_EINVAL; }
    if (n > SA_MAX_N || (d != 8 && d != 16)) {
        set_error("%s: n = %d, head width %d (compiled: n <= %d, head width 8 or 16)", what, (int)n, (int)d, SA_MAX_N);
        return WSI_ENOSYS;
    }
    return WSI_OK;
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_seq_attn_fwd(const float* qkv, int32_t B, int32_t n, int32_t H, int32_t d, float scale, float* out, float* lse, void* stream) {
    if (int rc = sa_check("seq_attn_fwd", B, n, H, d)) return rc;
    if (B == 0 || n == 0) return WSI_OK;
    if (!qkv || !out || !lse) { set_error("seq_attn_fwd: null pointer"); return WSI_EINVAL; }
    if (!aligned16(qkv)) { set_error("seq_attn_fwd: qkv must be 16-byte aligned"); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    if (d == 8) hipLaunchKernelGGL(seq_attn_fwd<8>, dim3(B * H), dim3(SA_THREADS), 0, st, qkv, n, H, scale, out, lse);
    else hipLaunchKernelGGL(seq_attn_fwd<16>, dim3(B * H), dim3(SA_THREADS), 0, st, qkv, n, H, scale, out, lse);
    return check_launch("seq_attn_fwd");
}

extern "C" int wsi_seq_attn_bwd(const float* g_out, const float* qkv, const float* lse, int32_t B, int32_t n, int32_t H, int32_t d, float scale,
                                float* g_qkv, void* stream) {
    if (int rc = sa_check("seq_attn_bwd", B, n, H, d)) return rc;
    if (B == 0 || n == 0) return WSI_OK;
    if (!g_out || !qkv || !lse || !g_qkv) { set_error("seq_attn_bwd: null pointer"); return WSI_EINVAL; }
    if (!aligned16(qkv) || !aligned16(g_out)) { set_error("seq_attn_bwd: qkv and g_out must be 16-byte aligned"); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    if (d == 8) hipLaunchKernelGGL(seq_attn_bwd<8>, dim3(B * H), dim3(SA_THREADS), 0, st, g_out, qkv, lse, n, H, scale, g_qkv);
    else hipLaunchKernelGGL(seq_attn_bwd<16>, dim3(B * H), dim3(SA_THREADS), 0, st, g_out, qkv, lse, n, H, scale, g_qkv);
    return check_launch("seq_attn_bwd");
}
