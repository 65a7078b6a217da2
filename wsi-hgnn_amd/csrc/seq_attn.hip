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
__device__ __forceinline__ float sa_dot(const float (&a)[D], const float* __restrict__ b) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < D; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(b + c);
        acc = fmaf(a[c], v.x, acc); acc = fmaf(a[c + 1], v.y, acc); acc = fmaf(a[c + 2], v.z, acc); acc = fmaf(a[c + 3], v.w, acc);
    }
    return acc;
}

__device__ __forceinline__ float sa_quad_sum(float x) { return group_sum<4>(x); }

__device__ __forceinline__ float sa_quad_max(float x) {
    x = fmaxf(x, dpp_mov<0xB1>(x));
    return fmaxf(x, dpp_mov<0x4E>(x));
}

// rows [n, D] of one head's column block (src points at its first column of the sequence's first row) -> LDS
template <int D>
__device__ __forceinline__ void sa_stage(float* __restrict__ dst, const float* __restrict__ src, int64_t ld, int n) {
    for (int i = threadIdx.x; i < n * (D / 4); i += SA_THREADS) {
        const int row = i / (D / 4), c = (i - row * (D / 4)) * 4;
        *reinterpret_cast<float4*>(dst + row * D + c) = *reinterpret_cast<const float4*>(src + (int64_t)row * ld + c);
    }
}

template <int D>
__global__ __launch_bounds__(SA_THREADS) void seq_attn_fwd(const float* __restrict__ qkv, int32_t n, int32_t H, float scale,
                                                           float* __restrict__ out, float* __restrict__ lse) {
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int64_t ld = 3 * (int64_t)H * D;
    const float* __restrict__ base = qkv + (int64_t)b * n * ld + h * D;
    __shared__ __attribute__((aligned(16))) float sq[SA_MAX_N * D], sk[SA_MAX_N * D], sv[SA_MAX_N * D];
    sa_stage<D>(sq, base, ld, n);
    sa_stage<D>(sk, base + (int64_t)H * D, ld, n);
    sa_stage<D>(sv, base + 2 * (int64_t)H * D, ld, n);
    __syncthreads();
    const int i = threadIdx.x >> 2, part = threadIdx.x & 3;
    if (i >= n) return;                                   // (whole quads leave together; no barrier follows)
    float q[D];
#pragma unroll
    for (int c = 0; c < D; ++c) q[c] = sq[i * D + c] * scale;
    float m = -INFINITY;
    for (int j = part; j < n; j += 4) m = fmaxf(m, sa_dot<D>(q, sk + j * D));
    m = sa_quad_max(m);                                   // (n >= 1: key 0 belongs to part 0, so the quad's maximum is finite)
    float l = 0.f, acc[D];
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = 0.f;
    for (int j = part; j < n; j += 4) {
        const float p = expf(sa_dot<D>(q, sk + j * D) - m);
        l += p;
#pragma unroll
        for (int c = 0; c < D; ++c) acc[c] = fmaf(p, sv[j * D + c], acc[c]);
    }
    l = sa_quad_sum(l);
    const float inv = 1.f / l;
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = sa_quad_sum(acc[c]) * inv;
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
    sa_stage<D>(sq, base, ld, n);
    sa_stage<D>(sk, base + (int64_t)H * D, ld, n);
    sa_stage<D>(sv, base + 2 * (int64_t)H * D, ld, n);
    sa_stage<D>(sg, g_out + (int64_t)b * n * H * D + h * D, (int64_t)H * D, n);
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
        for (int j = part; j < n; j += 4) delta = fmaf(expf(sa_dot<D>(q, sk + j * D) - li), sa_dot<D>(g, sv + j * D), delta);
        delta = sa_quad_sum(delta);
        if (part == 0) sd[i] = delta;
        float gq[D];
#pragma unroll
        for (int c = 0; c < D; ++c) gq[c] = 0.f;
        for (int j = part; j < n; j += 4) {
            const float ds = expf(sa_dot<D>(q, sk + j * D) - li) * (sa_dot<D>(g, sv + j * D) - delta);
#pragma unroll
            for (int c = 0; c < D; ++c) gq[c] = fmaf(ds, sk[j * D + c], gq[c]);
        }
        float* __restrict__ o = gbase + (int64_t)i * ld;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const float tot = sa_quad_sum(gq[c]) * scale;
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
        const float p = expf(sa_dot<D>(kj, sq + r * D) - sl[r]);
        const float ds = p * (sa_dot<D>(vj, sg + r * D) - sd[r]);
#pragma unroll
        for (int c = 0; c < D; ++c) { gv[c] = fmaf(p, sg[r * D + c], gv[c]); gk[c] = fmaf(ds, sq[r * D + c], gk[c]); }
    }
    float* __restrict__ ok = gbase + (int64_t)i * ld + (int64_t)H * D;
    float* __restrict__ ov = gbase + (int64_t)i * ld + 2 * (int64_t)H * D;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const float tk = sa_quad_sum(gk[c]) * scale, tv = sa_quad_sum(gv[c]);
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

static inline bool sa_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_seq_attn_fwd(const float* qkv, int32_t B, int32_t n, int32_t H, int32_t d, float scale, float* out, float* lse, void* stream) {
    if (int rc = sa_check("seq_attn_fwd", B, n, H, d)) return rc;
    if (B == 0 || n == 0) return WSI_OK;
    if (!qkv || !out || !lse) { set_error("seq_attn_fwd: null pointer"); return WSI_EINVAL; }
    if (!sa_aligned(qkv)) { set_error("seq_attn_fwd: qkv must be 16-byte aligned"); return WSI_EINVAL; }
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
    if (!sa_aligned(qkv) || !sa_aligned(g_out)) { set_error("seq_attn_bwd: qkv and g_out must be 16-byte aligned"); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    if (d == 8) hipLaunchKernelGGL(seq_attn_bwd<8>, dim3(B * H), dim3(SA_THREADS), 0, st, g_out, qkv, lse, n, H, scale, g_qkv);
    else hipLaunchKernelGGL(seq_attn_bwd<16>, dim3(B * H), dim3(SA_THREADS), 0, st, g_out, qkv, lse, n, H, scale, g_qkv);
    return check_launch("seq_attn_bwd");
}
