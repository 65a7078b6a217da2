// Multi-head GAT attention (DGL GATConv, models/GAT.py:17-92) for gfx950.  Contracts: include/wsi_hgnn.h.
//   el | er   = per-head sums of ft * attn_l / attn_r                                   -> wsi_gat_scores
//   s_e       = leaky_relu(el[u] + er[v]);  a = edge_softmax over v's in-edges (no epsilon);  a = attn_drop(a)
//   rst[v]    = act(sum_e a_e * ft[u] + bias)                                            -> wsi_gat_attn_fwd
// Layout: the row groups of row_group.h, a row being the H heads side by side (G >= H).  A chunk never straddles two heads (VEC = 4
// only when D % 4 == 0), so the head of every chunk is a per-lane constant; the per-(edge, head) softmax weight is computed by lane h
// of the group and fetched by the others with one ds_bpermute per chunk.  The forward keeps only out and the per-(node, head)
// log-sum-exp (as max | log of the shifted sum): the backward recomputes every a_e from el, er and lse.  Every reduction runs in a fixed
// order (no atomics): results are bit-reproducible.
// Backward (source-major, the shape of the HEAT backward):
//   prep  g_rst = g_out * act'(out), column partials of g_rst (bias gradient)
//   A     CSC by source u: g_ft[u] = sum a_e g_rst[w];  g_a[e,h] = g_rst[w]_h . ft[u]_h   (one g_rst row gather per edge)
//   B     CSR by destination v (scalar): delta = sum a g_a;  g_pre = a (g_a - delta) lrelu';  g_er[v] = sum g_pre
//   C     by source u: g_el[u] = sum g_pre;  g_ft[u,h,:] += g_el attn_l[h] + g_er attn_r[h];  column partials of g_attn_l/r
//   sum   the fixed-shape column partials, in order
// Message scale (the *_scaled entry points; GNNExplainer's sigmoid(edge_mask), explainers/gnn_explainer.py:21-33): one fp32 factor s_e per
// edge multiplies the MESSAGE a~_e ft[u] after the softmax.  SCALED is a compile-time switch of the forward, pass A and pass B:
//   fwd   out[v] = act(sum_e a~_e s_e ft[u] + bias)
//   A     g_ft[u] = sum a~_e s_e g_rst[w];  g_a keeps the RAW dot r[e,h] = g_rst[w]_h . ft[u]_h
//   B     d loss / d a~ = s_e r[e,h];  g_scale[e] = sum_h a~_{e,h} r[e,h]  (the lane that owns edge e adds its heads in order)
// The unscaled instantiations contain none of it.
#include "row_group.h"
#include <math.h>

namespace wsi {

constexpr int GA_BLOCK = 256;
constexpr int GA_MAX_HEADS = 16;
constexpr int GA_MAX_WIDTH = 4096;
constexpr int GA_PART_BLOCKS = 128;        // fixed grid of the kernels that write column partials (the partial count is a function of G only)
constexpr int GA_B_LANES = 16;             // group size of the scalar pass B

enum { GA_ACT_NONE = 0, GA_ACT_RELU = 1, GA_ACT_LEAKY = 2 };

// head of every chunk of this lane (0 for chunks past the row: their loads and stores are skipped, their group reductions still run)
template <int G, int VEC, int NK>
__device__ __forceinline__ void chunk_heads(int gl, int F, int D, int (&hk)[NK], bool (&ok)[NK]) {
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = chunk_col<G, VEC>(gl, k);
        ok[k] = c < F;
        hk[k] = ok[k] ? c / D : 0;
    }
}

// sum over the group of the products of head h, delivered to lane h of the group (H rounds of a group reduction)
template <int G, int NK>
__device__ __forceinline__ float per_head_sums(const float (&p)[NK], const int (&hk)[NK], int H, int gl) {
    float mine = 0.f;
    for (int h = 0; h < H; ++h) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) t += hk[k] == h ? p[k] : 0.f;
        t = group_sum<G>(t);
        if (gl == h) mine = t;
    }
    return mine;
}

// eler[n, 0:H] = el, eler[n, H:2H] = er
template <int G, int VEC, int NK>
__global__ __launch_bounds__(GA_BLOCK) void gat_scores_kernel(const float* __restrict__ ft, int64_t ldf, int n, int H, int D,
                                                              const float* __restrict__ attn_l, const float* __restrict__ attn_r,
                                                              float* __restrict__ eler) {
    const int gl = group_lane<G>(), row = group_row<G, GA_BLOCK>();
    if (row >= n) return;                                        // group-uniform
    const int F = H * D;
    int hk[NK];
    bool ok[NK];
    chunk_heads<G, VEC, NK>(gl, F, D, hk, ok);
    float pl[NK], pr[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        pl[k] = pr[k] = 0.f;
        if (ok[k]) {
            const int c = chunk_col<G, VEC>(gl, k);
            float x[VEC], al[VEC], ar[VEC];
            load_vec<VEC>(x, ft + (int64_t)row * ldf + c);
            load_vec<VEC>(al, attn_l + c);
            load_vec<VEC>(ar, attn_r + c);
#pragma unroll
            for (int j = 0; j < VEC; ++j) { pl[k] = fmaf(x[j], al[j], pl[k]); pr[k] = fmaf(x[j], ar[j], pr[k]); }
        }
    }
    const float sl = per_head_sums<G, NK>(pl, hk, H, gl);
    const float sr = per_head_sums<G, NK>(pr, hk, H, gl);
    if (gl < H) {
        eler[(int64_t)row * 2 * H + gl] = sl;
        eler[(int64_t)row * 2 * H + H + gl] = sr;
    }
}

// per-(destination, head) log-sum-exp of the scores, held by lane h of the group as its two parts: the max (+inf for a node without
// in-edges: no a_e) and the log of the max-subtracted sum.  a_e = exp((s_e - max) - log_sum): s_e - max is exact near the max, so a
// score of size 60 costs no bits (exp(s_e - lse) with lse rounded to fp32 scales a whole node's a_e by up to 1 + 2e-6 there, and
// the softmax gradient no longer sums to zero over the node's edges).
template <int G>
__device__ __forceinline__ float softmax_lse(const float* __restrict__ eler, const int32_t* __restrict__ src, int v, int e0, int e1,
                                             int H, int gl, float slope, float& log_sum) {
    float mine = INFINITY;
    log_sum = 0.f;
    for (int h = 0; h < H; ++h) {
        const float erv = eler[(int64_t)v * 2 * H + H + h];
        float m = -INFINITY, l = 0.f;
        for (int e = e0 + gl; e < e1; e += G) {
            const float s = leaky_relu(eler[(int64_t)src[e] * 2 * H + h] + erv, slope);
            if (s > m) { l = l * expf(m - s) + 1.f; m = s; }
            else l += expf(s - m);
        }
        const float M = group_max<G>(m);
        l = m == -INFINITY ? 0.f : l * expf(m - M);
        const float L = group_sum<G>(l);
        if (gl == h && e1 > e0) { mine = M; log_sum = logf(L); }
    }
    return mine;
}

struct GatDrop {
    uint32_t seed, thr;
    const uint32_t* seed_base;
    float scale;
};

__device__ __forceinline__ float edge_factor(const GatDrop& dr, uint32_t seed, int e, int h, int H) {
    return dr.thr ? drop_factor1((uint32_t)e, (uint32_t)h, (uint32_t)((H + 1) / 2), seed, dr.thr, dr.scale) : 1.f;
}

__device__ __forceinline__ float act_fwd(float z, int act, float act_slope) {
    return act == GA_ACT_RELU ? fmaxf(z, 0.f) : act == GA_ACT_LEAKY ? leaky_relu(z, act_slope) : z;
}

template <int G, int VEC, int NK, bool SCALED>
__global__ __launch_bounds__(GA_BLOCK) void gat_fwd_kernel(const float* __restrict__ ft, int64_t ldf, const float* __restrict__ eler, int n, int H, int D,
                                                           const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                                                           const int32_t* __restrict__ order, float slope, GatDrop dr,
                                                           const float* __restrict__ bias, int act, float act_slope,
                                                           float* __restrict__ out, int64_t ldo, float* __restrict__ lse,
                                                           const float* __restrict__ escale) {
    const int gl = group_lane<G>(), gbase = group_base<G>(), gi = group_row<G, GA_BLOCK>();
    if (gi >= n) return;                                         // group-uniform
    const int v = order ? order[gi] : gi;
    const int F = H * D;
    const uint32_t seed = dr.seed + (dr.seed_base ? *dr.seed_base : 0u);
    int hk[NK];
    bool ok[NK];
    chunk_heads<G, VEC, NK>(gl, F, D, hk, ok);
    const int e0 = rowptr[v], e1 = rowptr[v + 1];
    float my_ls;
    const float my_m = softmax_lse<G>(eler, src, v, e0, e1, H, gl, slope, my_ls);
    const float my_er = gl < H ? eler[(int64_t)v * 2 * H + H + gl] : 0.f;
    float acc[NK][VEC];
    zero_chunks(acc);
    for (int e = e0; e < e1; ++e) {
        const int u = src[e];
        float a = 0.f;
        if (gl < H) {
            a = expf((leaky_relu(eler[(int64_t)u * 2 * H + gl] + my_er, slope) - my_m) - my_ls) * edge_factor(dr, seed, e, gl, H);
            if constexpr (SCALED) a *= escale[e];
        }
        const float* __restrict__ row = ft + (int64_t)u * ldf;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const float ak = __shfl(a, gbase + hk[k]);
            if (ok[k]) {
                float x[VEC];
                load_vec<VEC>(x, row + chunk_col<G, VEC>(gl, k));
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[k][j] = fmaf(ak, x[j], acc[k][j]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (ok[k]) {
            const int c = chunk_col<G, VEC>(gl, k);
            float b[VEC];
            if (bias) load_vec<VEC>(b, bias + c);
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[k][j] = act_fwd(acc[k][j] + (bias ? b[j] : 0.f), act, act_slope);
            store_vec<VEC>(out + (int64_t)v * ldo + c, acc[k]);
        }
    }
    if (gl < H) {
        lse[(int64_t)v * 2 * H + gl] = my_m;
        lse[(int64_t)v * 2 * H + H + gl] = my_ls;
    }
}

// g_rst = g_out * act'(out) (written only when act != none) and the column partials of g_rst: part[r, 2F + c]
template <int G, int VEC, int NK>
__global__ __launch_bounds__(GA_BLOCK) void gat_act_bwd_kernel(const float* __restrict__ g_out, int64_t ldg, const float* __restrict__ out, int64_t ldo,
                                                               int n, int F, int act, float act_slope, float* __restrict__ g_rst,
                                                               float* __restrict__ part) {
    const int gl = group_lane<G>(), gid = group_row<G, GA_BLOCK>();
    const int groups = GA_PART_BLOCKS * (GA_BLOCK / G);
    float s[NK][VEC];                                            // (zero_chunks and chunk_col change this kernel's code: spelled out)
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int j = 0; j < VEC; ++j) s[k][j] = 0.f;
    for (int r = gid; r < n; r += groups) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int c = VEC * (gl + G * k);
            if (c < F) {
                float g[VEC];
                load_vec<VEC>(g, g_out + (int64_t)r * ldg + c);
                if (act != GA_ACT_NONE) {
                    float o[VEC];
                    load_vec<VEC>(o, out + (int64_t)r * ldo + c);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) g[j] = o[j] > 0.f ? g[j] : (act == GA_ACT_RELU ? 0.f : g[j] * act_slope);
                    store_vec<VEC>(g_rst + (int64_t)r * F + c, g);
                }
#pragma unroll
                for (int j = 0; j < VEC; ++j) s[k][j] += g[j];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = VEC * (gl + G * k);
        if (c < F) store_vec<VEC>(part + (int64_t)gid * 3 * F + 2 * F + c, s[k]);
    }
}

// pass A: one group per source u (in order_src); g_ft[u] = sum over out-edges of a~_e (s_e) g_rst[w], g_a[e,h] = g_rst[w]_h . ft[u]_h
template <int G, int VEC, int NK, bool SCALED>
__global__ __launch_bounds__(GA_BLOCK) void gat_bwd_src_kernel(const float* __restrict__ ft, int64_t ldf, const float* __restrict__ eler,
                                                               const float* __restrict__ lse, const float* __restrict__ g_rst, int64_t ldr,
                                                               int n, int H, int D, const int32_t* __restrict__ colptr,
                                                               const int32_t* __restrict__ csc_eid, const int32_t* __restrict__ csc_dst,
                                                               const int32_t* __restrict__ order, float slope, GatDrop dr,
                                                               float* __restrict__ g_ft, int64_t ldgf, float* __restrict__ g_a,
                                                               const float* __restrict__ escale) {
    const int gl = group_lane<G>(), gbase = group_base<G>(), gi = group_row<G, GA_BLOCK>();
    if (gi >= n) return;
    const int u = order ? order[gi] : gi;
    const int F = H * D;
    const uint32_t seed = dr.seed + (dr.seed_base ? *dr.seed_base : 0u);
    int hk[NK];
    bool ok[NK];
    chunk_heads<G, VEC, NK>(gl, F, D, hk, ok);
    float fu[NK][VEC], acc[NK][VEC];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) { fu[k][j] = 0.f; acc[k][j] = 0.f; }
        if (ok[k]) load_vec<VEC>(fu[k], ft + (int64_t)u * ldf + chunk_col<G, VEC>(gl, k));
    }
    const float my_el = gl < H ? eler[(int64_t)u * 2 * H + gl] : 0.f;
    const int j0 = colptr[u], j1 = colptr[u + 1];
    for (int jj = j0; jj < j1; ++jj) {
        const int e = csc_eid[jj], w = csc_dst[jj];
        float a = 0.f;
        if (gl < H) {
            a = expf((leaky_relu(my_el + eler[(int64_t)w * 2 * H + H + gl], slope) - lse[(int64_t)w * 2 * H + gl]) - lse[(int64_t)w * 2 * H + H + gl]) *
                edge_factor(dr, seed, e, gl, H);
            if constexpr (SCALED) a *= escale[e];
        }
        const float* __restrict__ row = g_rst + (int64_t)w * ldr;
        float p[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const float ak = __shfl(a, gbase + hk[k]);
            p[k] = 0.f;
            if (ok[k]) {
                float g[VEC];
                load_vec<VEC>(g, row + chunk_col<G, VEC>(gl, k));
#pragma unroll
                for (int j = 0; j < VEC; ++j) { acc[k][j] = fmaf(ak, g[j], acc[k][j]); p[k] = fmaf(g[j], fu[k][j], p[k]); }
            }
        }
        const float ga = per_head_sums<G, NK>(p, hk, H, gl);
        if (gl < H) g_a[(int64_t)e * H + gl] = ga;
    }
#pragma unroll
    for (int k = 0; k < NK; ++k)
        if (ok[k]) store_vec<VEC>(g_ft + (int64_t)u * ldgf + chunk_col<G, VEC>(gl, k), acc[k]);
}

// pass B: one 16-lane group per destination v; in place g_a (d loss / d a~, SCALED: the raw dot r) -> d loss / d a -> g_pre (d loss / d pre-activation score);
// g_er[v, h].  SCALED: d loss / d a~ = s_e r, and g_scale[e] = sum_h a~ r is built head by head by the one lane that visits edge e.
template <bool SCALED>
__global__ __launch_bounds__(GA_BLOCK) void gat_bwd_dst_kernel(const float* __restrict__ eler, const float* __restrict__ lse, int n, int H,
                                                               const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                                                               float slope, GatDrop dr, float* __restrict__ g_a, float* __restrict__ g_er,
                                                               const float* __restrict__ escale, float* __restrict__ g_scale) {
    constexpr int G = GA_B_LANES;
    const int gl = group_lane<G>(), v = group_row<G, GA_BLOCK>();
    if (v >= n) return;
    const uint32_t seed = dr.seed + (dr.seed_base ? *dr.seed_base : 0u);
    const int e0 = rowptr[v], e1 = rowptr[v + 1];
    for (int h = 0; h < H; ++h) {
        const float erv = eler[(int64_t)v * 2 * H + H + h], M = lse[(int64_t)v * 2 * H + h], LS = lse[(int64_t)v * 2 * H + H + h];
        float d = 0.f;
        for (int e = e0 + gl; e < e1; e += G) {
            const float a = expf((leaky_relu(eler[(int64_t)src[e] * 2 * H + h] + erv, slope) - M) - LS);
            // t = d loss / d a: g_a times the factors of a~, rounded ONCE and kept in g_a for the second sweep.  delta and g_pre then see the
            // same number: a destination with one in-edge (a = 1, delta = t) gets a score gradient of exactly zero, as a softmax of one term
            // has (g_a * f - delta contracted into one fma would leave the rounding of the product there)
            float t;
            if constexpr (SCALED) {
                const float r = g_a[(int64_t)e * H + h], f = edge_factor(dr, seed, e, h, H), gs = a * f * r;
                g_scale[e] = h ? g_scale[e] + gs : gs;
                t = r * (f * escale[e]);
            } else {
                t = g_a[(int64_t)e * H + h] * edge_factor(dr, seed, e, h, H);
            }
            g_a[(int64_t)e * H + h] = t;
            d = fmaf(a, t, d);
        }
        const float delta = group_sum<G>(d);
        float gr = 0.f;
        for (int e = e0 + gl; e < e1; e += G) {
            const float pre = eler[(int64_t)src[e] * 2 * H + h] + erv;
            const float a = expf((leaky_relu(pre, slope) - M) - LS);
            const float gp = a * (g_a[(int64_t)e * H + h] - delta) * (pre > 0.f ? 1.f : slope);
            g_a[(int64_t)e * H + h] = gp;
            gr += gp;
        }
        gr = group_sum<G>(gr);
        if (gl == 0) g_er[(int64_t)v * H + h] = gr;
    }
}

// pass C: fixed grid, groups stride over the sources u; g_el[u] = sum g_pre over u's out-edges; rank-1 row update of g_ft; column
// partials part[r, 0:F] = sum g_el ft, part[r, F:2F] = sum g_er ft
template <int G, int VEC, int NK>
__global__ __launch_bounds__(GA_BLOCK) void gat_bwd_attn_kernel(const float* __restrict__ ft, int64_t ldf, const float* __restrict__ g_pre,
                                                                const float* __restrict__ g_er, int n, int H, int D,
                                                                const int32_t* __restrict__ colptr, const int32_t* __restrict__ csc_eid,
                                                                const float* __restrict__ attn_l, const float* __restrict__ attn_r,
                                                                float* __restrict__ g_ft, int64_t ldgf, float* __restrict__ part) {
    const int gl = group_lane<G>(), gbase = group_base<G>(), gid = group_row<G, GA_BLOCK>();
    const int groups = GA_PART_BLOCKS * (GA_BLOCK / G);
    const int F = H * D;
    int hk[NK];
    bool ok[NK];
    chunk_heads<G, VEC, NK>(gl, F, D, hk, ok);
    float al[NK][VEC], ar[NK][VEC], pl[NK][VEC], pr[NK][VEC];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) { al[k][j] = ar[k][j] = pl[k][j] = pr[k][j] = 0.f; }
        if (ok[k]) {
            load_vec<VEC>(al[k], attn_l + chunk_col<G, VEC>(gl, k));
            load_vec<VEC>(ar[k], attn_r + chunk_col<G, VEC>(gl, k));
        }
    }
    for (int u = gid; u < n; u += groups) {
        const int j0 = colptr[u], j1 = colptr[u + 1];
        float gel = 0.f;
        for (int h = 0; h < H; ++h) {
            float t = 0.f;
            for (int jj = j0 + gl; jj < j1; jj += G) t += g_pre[(int64_t)csc_eid[jj] * H + h];
            t = group_sum<G>(t);
            if (gl == h) gel = t;
        }
        const float ger = gl < H ? g_er[(int64_t)u * H + gl] : 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const float lk = __shfl(gel, gbase + hk[k]), rk = __shfl(ger, gbase + hk[k]);
            if (ok[k]) {
                const int c = chunk_col<G, VEC>(gl, k);
                float x[VEC], g[VEC];
                load_vec<VEC>(x, ft + (int64_t)u * ldf + c);
                load_vec<VEC>(g, g_ft + (int64_t)u * ldgf + c);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    g[j] = fmaf(lk, al[k][j], fmaf(rk, ar[k][j], g[j]));
                    pl[k][j] = fmaf(lk, x[j], pl[k][j]);
                    pr[k][j] = fmaf(rk, x[j], pr[k][j]);
                }
                store_vec<VEC>(g_ft + (int64_t)u * ldgf + c, g);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (ok[k]) {
            const int c = chunk_col<G, VEC>(gl, k);
            store_vec<VEC>(part + (int64_t)gid * 3 * F + c, pl[k]);
            store_vec<VEC>(part + (int64_t)gid * 3 * F + F + c, pr[k]);
        }
    }
}

// out[c] = sum over the `rows` partial rows, in row order; columns [0,F) -> g_attn_l, [F,2F) -> g_attn_r, [2F,3F) -> g_bias (optional)
__global__ __launch_bounds__(256) void gat_colsum_kernel(const float* __restrict__ part, int rows, int F, float* __restrict__ g_l,
                                                         float* __restrict__ g_r, float* __restrict__ g_b) {
    const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (c >= 3 * F) return;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += part[(int64_t)r * 3 * F + c];
    if (c < F) g_l[c] = s;
    else if (c < 2 * F) g_r[c - F] = s;
    else if (g_b) g_b[c - 2 * F] = s;
}

// GraphConv edge-weight gradient (wsi_sddmm_dot): g_w[e] = oscale[w] iscale[u] <g[w], x[u]> for every CSR entry e = (u -> w).  The layout of
// the forward above with one head: a group per destination w keeps g[w] (masked by relu_ref[w] > 0) in registers and gathers x[u] once per edge.
template <int G, int VEC, int NK>
__global__ __launch_bounds__(GA_BLOCK) void sddmm_dot_kernel(const float* __restrict__ g, int64_t ldg, const float* __restrict__ x, int64_t ldx, int n, int D,
                                                             const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                                                             const float* __restrict__ iscale, const float* __restrict__ oscale,
                                                             const float* __restrict__ relu_ref, int64_t ldref, float* __restrict__ g_w) {
    const int gl = group_lane<G>(), w = group_row<G, GA_BLOCK>();
    if (w >= n) return;                                          // group-uniform
    float gw[NK][VEC];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = chunk_col<G, VEC>(gl, k);
#pragma unroll
        for (int j = 0; j < VEC; ++j) gw[k][j] = 0.f;
        if (c < D) {
            load_vec<VEC>(gw[k], g + (int64_t)w * ldg + c);
            if (relu_ref) {
                float y[VEC];
                load_vec<VEC>(y, relu_ref + (int64_t)w * ldref + c);
#pragma unroll
                for (int j = 0; j < VEC; ++j) gw[k][j] = y[j] > 0.f ? gw[k][j] : 0.f;
            }
        }
    }
    const float os = oscale ? oscale[w] : 1.f;
    const int e0 = rowptr[w], e1 = rowptr[w + 1];
    for (int e = e0; e < e1; ++e) {
        const int u = src[e];
        const float* __restrict__ row = x + (int64_t)u * ldx;
        float p = 0.f;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int c = chunk_col<G, VEC>(gl, k);
            if (c < D) {
                float v[VEC];
                load_vec<VEC>(v, row + c);
#pragma unroll
                for (int j = 0; j < VEC; ++j) p = fmaf(gw[k][j], v[j], p);
            }
        }
        p = group_sum<G>(p);
        if (gl == 0) g_w[e] = os * (iscale ? iscale[u] : 1.f) * p;
    }
}

// ---------------------------------------------------------------------------------------------------- host side
static int ga_check_shape(const char* what, int32_t n, int32_t H, int32_t D) {
    if (n < 0 || H < 1 || H > GA_MAX_HEADS || D < 1 || (int64_t)H * D > GA_MAX_WIDTH) {
        set_error("%s: bad shape n=%d heads=%d D=%d (1 <= heads <= %d, 1 <= heads*D <= %d)", what, n, H, D, GA_MAX_HEADS, GA_MAX_WIDTH);
        return WSI_EINVAL;
    }
    return WSI_OK;
}

static int ga_part_rows(int G) { return GA_PART_BLOCKS * (GA_BLOCK / G); }

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_gat_scores(const float* ft, int64_t ldf, int32_t n, int32_t H, int32_t D, const float* attn_l, const float* attn_r,
                              float* eler, void* stream) {
    if (int rc = ga_check_shape("gat_scores", n, H, D)) return rc;
    if (ldf < (int64_t)H * D) { set_error("gat_scores: ldf=%lld < heads*D", (long long)ldf); return WSI_EINVAL; }
    if (!ft || !attn_l || !attn_r || !eler) { set_error("gat_scores: null pointer"); return WSI_EINVAL; }
    if (n == 0) return WSI_OK;
    const RowCfg cfg = row_cfg(H * D, D, H, ldf % 4 == 0 && aligned16(ft) && aligned16(attn_l) && aligned16(attn_r));
    hipStream_t st = (hipStream_t)stream;
    const int per = GA_BLOCK / cfg.G;
#define CALL(G_, V_, K_) hipLaunchKernelGGL((gat_scores_kernel<G_, V_, K_>), dim3((n + per - 1) / per), dim3(GA_BLOCK), 0, st, ft, ldf, n, H, D, attn_l, attn_r, eler)
    ROW_GROUP_DISPATCH_ALL("gat", cfg, CALL);
#undef CALL
    return check_launch("gat_scores");
}

// both forward entry points; SCALED picks the instantiation that reads edge_scale (checked non-null by the caller)
template <bool SCALED>
static int ga_fwd(const char* what, const float* ft, int64_t ldf, const float* eler, int32_t n, int32_t H, int32_t D,
                  const int32_t* rowptr, const int32_t* src, const int32_t* order_dst, float negative_slope,
                  uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_threshold, float drop_scale,
                  const float* bias, int32_t activation, float act_slope, const float* edge_scale, float* out, int64_t ldo, float* lse, void* stream) {
    if (int rc = ga_check_shape(what, n, H, D)) return rc;
    const int64_t F = (int64_t)H * D;
    if (ldf < F || ldo < F) { set_error("%s: row stride below heads*D", what); return WSI_EINVAL; }
    if (activation < 0 || activation > 2) { set_error("%s: activation %d (0 none, 1 relu, 2 leaky_relu)", what, activation); return WSI_EINVAL; }
    if (drop_threshold > 65535u) { set_error("%s: drop_threshold %u > 65535", what, drop_threshold); return WSI_EINVAL; }
    if (!ft || !eler || !rowptr || !src || !out || !lse || (SCALED && !edge_scale)) { set_error("%s: null pointer", what); return WSI_EINVAL; }
    if (n == 0) return WSI_OK;
    const RowCfg cfg = row_cfg(H * D, D, H, ldf % 4 == 0 && ldo % 4 == 0 && aligned16(ft) && aligned16(out) && aligned16(bias));
    const GatDrop dr{drop_seed, drop_threshold, drop_seed_base, drop_scale};
    hipStream_t st = (hipStream_t)stream;
    const int per = GA_BLOCK / cfg.G;
#define CALL(G_, V_, K_) hipLaunchKernelGGL((gat_fwd_kernel<G_, V_, K_, SCALED>), dim3((n + per - 1) / per), dim3(GA_BLOCK), 0, st, ft, ldf, eler, n, H, D, \
                                            rowptr, src, order_dst, negative_slope, dr, bias, (int)activation, act_slope, out, ldo, lse, edge_scale)
    ROW_GROUP_DISPATCH_ALL("gat", cfg, CALL);
#undef CALL
    return check_launch(what);
}

extern "C" int wsi_gat_attn_fwd(const float* ft, int64_t ldf, const float* eler, int32_t n, int32_t H, int32_t D,
                                const int32_t* rowptr, const int32_t* src, const int32_t* order_dst, float negative_slope,
                                uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_threshold, float drop_scale,
                                const float* bias, int32_t activation, float act_slope, float* out, int64_t ldo, float* lse, void* stream) {
    return ga_fwd<false>("gat_attn_fwd", ft, ldf, eler, n, H, D, rowptr, src, order_dst, negative_slope, drop_seed, drop_seed_base, drop_threshold,
                         drop_scale, bias, activation, act_slope, nullptr, out, ldo, lse, stream);
}

extern "C" int wsi_gat_attn_fwd_scaled(const float* ft, int64_t ldf, const float* eler, int32_t n, int32_t H, int32_t D,
                                       const int32_t* rowptr, const int32_t* src, const int32_t* order_dst, float negative_slope,
                                       uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_threshold, float drop_scale,
                                       const float* bias, int32_t activation, float act_slope, const float* edge_scale,
                                       float* out, int64_t ldo, float* lse, void* stream) {
    return ga_fwd<true>("gat_attn_fwd_scaled", ft, ldf, eler, n, H, D, rowptr, src, order_dst, negative_slope, drop_seed, drop_seed_base,
                        drop_threshold, drop_scale, bias, activation, act_slope, edge_scale, out, ldo, lse, stream);
}

// workspace: g_rst [n, F] (only when activation != none), g_a / g_pre [E, H], g_er [n, H], column partials [rows(G), 3F]
static int64_t ga_ws_layout(int32_t n, int32_t E, int32_t H, int32_t D, int32_t activation, int64_t* off) {
    const int64_t F = (int64_t)H * D;
    const RowCfg cfg = row_cfg(H * D, D, H, true);
    const RowCfg cfg1 = row_cfg(H * D, D, H, false);
    const int rows = ga_part_rows(cfg.G < cfg1.G ? cfg.G : cfg1.G);       // enough for either vector width
    auto up = [](int64_t b) { return (b + 255) & ~(int64_t)255; };
    off[0] = 0;
    off[1] = off[0] + up(activation ? (int64_t)n * F * 4 : 0);
    off[2] = off[1] + up((int64_t)E * H * 4);
    off[3] = off[2] + up((int64_t)n * H * 4);
    return off[3] + up((int64_t)rows * 3 * F * 4);
}

extern "C" int64_t wsi_gat_attn_bwd_workspace_bytes(int32_t n, int32_t E, int32_t H, int32_t D, int32_t activation) {
    if (ga_check_shape("gat_attn_bwd_workspace_bytes", n, H, D) || E < 0 || activation < 0 || activation > 2) return -1;
    int64_t off[4];
    return ga_ws_layout(n, E, H, D, activation, off);
}

// both backward entry points; SCALED: edge_scale in, g_edge_scale [E] out (same workspace)
template <bool SCALED>
static int ga_bwd(const char* what, const float* ft, int64_t ldf, const float* eler, const float* lse, const float* out, int64_t ldo,
                  const float* g_out, int64_t ldg, int32_t n, int32_t E, int32_t H, int32_t D,
                  const int32_t* rowptr, const int32_t* src, const int32_t* colptr, const int32_t* csc_eid,
                  const int32_t* csc_dst, const int32_t* order_src, const float* attn_l, const float* attn_r,
                  float negative_slope, uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_threshold,
                  float drop_scale, int32_t activation, float act_slope, const float* edge_scale, void* workspace, int64_t workspace_bytes,
                  float* g_ft, int64_t ldgf, float* g_attn_l, float* g_attn_r, float* g_bias, float* g_edge_scale, void* stream) {
    if (int rc = ga_check_shape(what, n, H, D)) return rc;
    const int64_t F = (int64_t)H * D;
    if (E < 0) { set_error("%s: E=%d", what, E); return WSI_EINVAL; }
    if (ldf < F || ldo < F || ldg < F || ldgf < F) { set_error("%s: row stride below heads*D", what); return WSI_EINVAL; }
    if (activation < 0 || activation > 2) { set_error("%s: activation %d (0 none, 1 relu, 2 leaky_relu)", what, activation); return WSI_EINVAL; }
    if (drop_threshold > 65535u) { set_error("%s: drop_threshold %u > 65535", what, drop_threshold); return WSI_EINVAL; }
    if (!ft || !eler || !lse || !g_out || !rowptr || !src || !colptr || !csc_eid || !csc_dst || !attn_l || !attn_r || !workspace ||
        !g_ft || !g_attn_l || !g_attn_r || (activation && !out) || (SCALED && (!edge_scale || !g_edge_scale))) {
        set_error("%s: null pointer", what);
        return WSI_EINVAL;
    }
    // g_rst and the column partials live in the workspace at 256-byte offsets and take the 16-byte accesses of the vector-4 kernels
    if (!aligned16(workspace)) { set_error("%s: workspace %p is not 16-byte aligned", what, workspace); return WSI_EINVAL; }
    int64_t off[4];
    const int64_t need = ga_ws_layout(n, E, H, D, activation, off);
    if (workspace_bytes < need) { set_error("%s: workspace %lld < %lld bytes", what, (long long)workspace_bytes, (long long)need); return WSI_ENOMEM; }
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* g_rst = activation ? (float*)(ws + off[0]) : nullptr;
    float* g_a = (float*)(ws + off[1]);
    float* g_er = (float*)(ws + off[2]);
    float* part = (float*)(ws + off[3]);
    const float* rst = activation ? g_rst : g_out;
    const int64_t ldr = activation ? F : ldg;
    const bool v4 = ldf % 4 == 0 && ldo % 4 == 0 && ldg % 4 == 0 && ldgf % 4 == 0 && aligned16(ft) && aligned16(out) && aligned16(g_out) &&
                    aligned16(g_ft) && aligned16(attn_l) && aligned16(attn_r);
    const RowCfg cfg = row_cfg(H * D, D, H, v4);
    const GatDrop dr{drop_seed, drop_threshold, drop_seed_base, drop_scale};
    const int per = GA_BLOCK / cfg.G;
    if (n > 0) {
#define CALL(G_, V_, K_) hipLaunchKernelGGL((gat_act_bwd_kernel<G_, V_, K_>), dim3(GA_PART_BLOCKS), dim3(GA_BLOCK), 0, st, g_out, ldg, out, ldo, n, (int)F, \
                                            (int)activation, act_slope, g_rst, part)
        ROW_GROUP_DISPATCH_ALL("gat", cfg, CALL);
#undef CALL
#define CALL(G_, V_, K_) hipLaunchKernelGGL((gat_bwd_src_kernel<G_, V_, K_, SCALED>), dim3((n + per - 1) / per), dim3(GA_BLOCK), 0, st, ft, ldf, eler, lse, rst, ldr, \
                                            n, H, D, colptr, csc_eid, csc_dst, order_src, negative_slope, dr, g_ft, ldgf, g_a, edge_scale)
        ROW_GROUP_DISPATCH_ALL("gat", cfg, CALL);
#undef CALL
        constexpr int per_b = GA_BLOCK / GA_B_LANES;
        hipLaunchKernelGGL((gat_bwd_dst_kernel<SCALED>), dim3((n + per_b - 1) / per_b), dim3(GA_BLOCK), 0, st, eler, lse, n, H, rowptr, src, negative_slope, dr, g_a, g_er,
                           edge_scale, g_edge_scale);
#define CALL(G_, V_, K_) hipLaunchKernelGGL((gat_bwd_attn_kernel<G_, V_, K_>), dim3(GA_PART_BLOCKS), dim3(GA_BLOCK), 0, st, ft, ldf, (const float*)g_a, \
                                            (const float*)g_er, n, H, D, colptr, csc_eid, attn_l, attn_r, g_ft, ldgf, part)
        ROW_GROUP_DISPATCH_ALL("gat", cfg, CALL);
#undef CALL
        hipLaunchKernelGGL(gat_colsum_kernel, dim3((unsigned)((3 * F + 255) / 256)), dim3(256), 0, st, (const float*)part, ga_part_rows(cfg.G), (int)F,
                           g_attn_l, g_attn_r, g_bias);
    } else {
        if (hipMemsetAsync(g_attn_l, 0, F * 4, st) != hipSuccess || hipMemsetAsync(g_attn_r, 0, F * 4, st) != hipSuccess ||
            (g_bias && hipMemsetAsync(g_bias, 0, F * 4, st) != hipSuccess))
            return check_launch(SCALED ? "gat_attn_bwd_scaled(memset)" : "gat_attn_bwd(memset)");
    }
    return check_launch(what);
}

extern "C" int wsi_gat_attn_bwd(const float* ft, int64_t ldf, const float* eler, const float* lse, const float* out, int64_t ldo,
                                const float* g_out, int64_t ldg, int32_t n, int32_t E, int32_t H, int32_t D,
                                const int32_t* rowptr, const int32_t* src, const int32_t* colptr, const int32_t* csc_eid,
                                const int32_t* csc_dst, const int32_t* order_src, const float* attn_l, const float* attn_r,
                                float negative_slope, uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_threshold,
                                float drop_scale, int32_t activation, float act_slope, void* workspace, int64_t workspace_bytes,
                                float* g_ft, int64_t ldgf, float* g_attn_l, float* g_attn_r, float* g_bias, void* stream) {
    return ga_bwd<false>("gat_attn_bwd", ft, ldf, eler, lse, out, ldo, g_out, ldg, n, E, H, D, rowptr, src, colptr, csc_eid, csc_dst, order_src,
                         attn_l, attn_r, negative_slope, drop_seed, drop_seed_base, drop_threshold, drop_scale, activation, act_slope, nullptr,
                         workspace, workspace_bytes, g_ft, ldgf, g_attn_l, g_attn_r, g_bias, nullptr, stream);
}

extern "C" int wsi_gat_attn_bwd_scaled(const float* ft, int64_t ldf, const float* eler, const float* lse, const float* out, int64_t ldo,
                                       const float* g_out, int64_t ldg, int32_t n, int32_t E, int32_t H, int32_t D,
                                       const int32_t* rowptr, const int32_t* src, const int32_t* colptr, const int32_t* csc_eid,
                                       const int32_t* csc_dst, const int32_t* order_src, const float* attn_l, const float* attn_r,
                                       float negative_slope, uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_threshold,
                                       float drop_scale, int32_t activation, float act_slope, const float* edge_scale,
                                       void* workspace, int64_t workspace_bytes, float* g_ft, int64_t ldgf, float* g_attn_l, float* g_attn_r,
                                       float* g_bias, float* g_edge_scale, void* stream) {
    return ga_bwd<true>("gat_attn_bwd_scaled", ft, ldf, eler, lse, out, ldo, g_out, ldg, n, E, H, D, rowptr, src, colptr, csc_eid, csc_dst, order_src,
                        attn_l, attn_r, negative_slope, drop_seed, drop_seed_base, drop_threshold, drop_scale, activation, act_slope, edge_scale,
                        workspace, workspace_bytes, g_ft, ldgf, g_attn_l, g_attn_r, g_bias, g_edge_scale, stream);
}

extern "C" int wsi_sddmm_dot(const float* g, int64_t ldg, const float* x, int64_t ldx, int32_t n, int32_t D,
                             const int32_t* rowptr, const int32_t* src, const float* iscale, const float* oscale,
                             const float* relu_ref, int64_t ldref, float* g_w, void* stream) {
    if (n < 0 || D <= 0 || D > 1024) { set_error("sddmm_dot: bad shape n=%d D=%d (1 <= D <= 1024)", n, D); return WSI_EINVAL; }
    if (ldg < D || ldx < D || (relu_ref && ldref < D)) { set_error("sddmm_dot: row stride below D"); return WSI_EINVAL; }
    if (n == 0) return WSI_OK;
    if (!g || !x || !rowptr || !src || !g_w) { set_error("sddmm_dot: null pointer"); return WSI_EINVAL; }
    const RowCfg cfg = row_cfg(D, D, 1, ldg % 4 == 0 && ldx % 4 == 0 && (!relu_ref || ldref % 4 == 0) && aligned16(g) && aligned16(x) && aligned16(relu_ref));
    hipStream_t st = (hipStream_t)stream;
    const int per = GA_BLOCK / cfg.G;
#define CALL(G_, V_, K_) hipLaunchKernelGGL((sddmm_dot_kernel<G_, V_, K_>), dim3((n + per - 1) / per), dim3(GA_BLOCK), 0, st, g, ldg, x, ldx, n, D, \
                                            rowptr, src, iscale, oscale, relu_ref, ldref, g_w)
    ROW_GROUP_DISPATCH_ALL("gat", cfg, CALL);
#undef CALL
    return check_launch("sddmm_dot");
}
