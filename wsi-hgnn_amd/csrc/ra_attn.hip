// RAConv's two-level attention (H2MIL, baselines/H2MIL/code/RAConv.py at heads = 1, add_self_loops = False, dropout = 0) for gfx950.
// Contracts: include/wsi_hgnn.h.  With t(e) = node_type[u_e] in {0, 1, 2} and the GROUP of e = (v_e, t(e)):
//   a_e     = softmax over the edges of group (v, t) of leaky_relu(el[u_e] + er[v])
//   q_vt    = leaky_relu(mean_{e in (v,t)} pl[u_e] + pr[v])            beta_vt = softmax over the groups PRESENT at v of q_vt
//   out[v]  = sum_e beta_{v,t(e)} a_e ft[u_e] + bias                    (a node without in-edges: out = bias)
// Both softmaxes subtract the maximum.  torch_geometric's softmax adds 1e-16 to a denominator that is >= 1 after that subtraction,
// below float64 resolution relative to 1: the kernels omit it.
// Layout: the row groups of row_group.h.  The per-edge weight is a scalar: the lanes of a group compute the weights of G consecutive
// edges at once (one edge each) and hand them round with ds_bpermute while the row gathers run, so an edge costs one expf per group,
// not one per lane.  The forward keeps out and, per (node, type), max | log of the shifted sum | group count | beta
// (stat [n, 3, 4]); the backward recomputes every edge weight from sc and stat.  Nothing is stored per edge by the forward.
// Backward (no atomics, every sum in one fixed order):
//   A  CSC by source u (t(e) is a constant of u): g_ft[u] = sum_e beta a_e g_out[v_e];  r_e = <g_out[v_e], ft[u]>
//   B  CSR by destination v, 16 lanes: A_vt = sum a_e r_e;  g_pre_e = beta_vt a_e (r_e - A_vt) lrelu'  (in place of r_e);  g_er[v] = sum g_pre;
//      g_q_vt = beta_vt (A_vt - sum_t' beta_vt' A_vt') lrelu';  gq[v, t] = g_q_vt / count;  g_pr[v] = sum_t g_q_vt
//   C  by source u, 16 lanes: g_el[u] = sum g_pre_e;  g_pl[u] = sum gq[v_e, t(u)]
//   bias: column partials of g_out over a fixed grid, added in order.
#include "row_group.h"
#include <math.h>

namespace wsi {

constexpr int RA_BLOCK = 256;
constexpr int RA_MAX_WIDTH = 4096;
constexpr int RA_S_LANES = 16;             // group size of the scalar passes B and C

__device__ __forceinline__ int ra_type(const int32_t* __restrict__ node_type, int u) { return min(max(node_type[u], 0), 2); }
__device__ __forceinline__ float ra_pick(int t, float a, float b, float c) { return t == 0 ? a : t == 1 ? b : c; }

template <int G, int VEC, int NK>
__global__ __launch_bounds__(RA_BLOCK) void ra_fwd_kernel(const float* __restrict__ ft, int64_t ldf, const float* __restrict__ sc,
                                                          const int32_t* __restrict__ node_type, int n, int C,
                                                          const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src, float slope,
                                                          const float* __restrict__ bias, float* __restrict__ out, int64_t ldo,
                                                          float* __restrict__ stat) {
    const int gl = group_lane<G>(), gbase = group_base<G>(), v = group_row<G, RA_BLOCK>();
    if (v >= n) return;                                          // group-uniform
    const int e0 = rowptr[v], e1 = rowptr[v + 1];
    const float erv = sc[(int64_t)v * 4 + 1], prv = sc[(int64_t)v * 4 + 3];
    // per type: running max / shifted sum of the scores, edge count, sum of pl over this lane's edges
    float m[3], l[3], cn[3], ps[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { m[k] = -INFINITY; l[k] = 0.f; cn[k] = 0.f; ps[k] = 0.f; }
    for (int e = e0 + gl; e < e1; e += G) {
        const int u = src[e], t = ra_type(node_type, u);
        const float s = leaky_relu(sc[(int64_t)u * 4] + erv, slope), p = sc[(int64_t)u * 4 + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (t == k) {
                if (s > m[k]) { l[k] = l[k] * expf(m[k] - s) + 1.f; m[k] = s; }
                else l[k] += expf(s - m[k]);
                cn[k] += 1.f;
                ps[k] += p;
            }
        }
    }
    float M[3], LS[3], q[3], beta[3];
    float qmax = -INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float Mk = group_max<G>(m[k]);
        const float L = group_sum<G>(m[k] == -INFINITY ? 0.f : l[k] * expf(m[k] - Mk));
        cn[k] = group_sum<G>(cn[k]);
        ps[k] = group_sum<G>(ps[k]);
        const bool present = cn[k] > 0.f;
        M[k] = present ? Mk : INFINITY;
        LS[k] = present ? logf(L) : 0.f;
        q[k] = present ? leaky_relu(ps[k] / cn[k] + prv, slope) : -INFINITY;
        qmax = fmaxf(qmax, q[k]);
    }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) { beta[k] = cn[k] > 0.f ? expf(q[k] - qmax) : 0.f; den += beta[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) beta[k] = den > 0.f ? beta[k] / den : 0.f;

    float acc[NK][VEC];                                          // (zero_chunks changes this kernel's code: spelled out)
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[k][j] = 0.f;
    for (int base = e0; base < e1; base += G) {
        const int me = base + gl;
        int u_m = 0;
        float a_m = 0.f;
        if (me < e1) {
            u_m = src[me];
            const int t = ra_type(node_type, u_m);
            const float s = leaky_relu(sc[(int64_t)u_m * 4] + erv, slope);
            a_m = expf((s - ra_pick(t, M[0], M[1], M[2])) - ra_pick(t, LS[0], LS[1], LS[2])) * ra_pick(t, beta[0], beta[1], beta[2]);
        }
        const int cnt = min(G, e1 - base);
        for (int j = 0; j < cnt; ++j) {
            const int u = __shfl(u_m, gbase + j);
            const float a = __shfl(a_m, gbase + j);
            const float* __restrict__ row = ft + (int64_t)u * ldf;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int c = chunk_col<G, VEC>(gl, k);
                if (c < C) {
                    float x[VEC];
                    load_vec<VEC>(x, row + c);
#pragma unroll
                    for (int jj = 0; jj < VEC; ++jj) acc[k][jj] = fmaf(a, x[jj], acc[k][jj]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = chunk_col<G, VEC>(gl, k);
        if (c < C) {
            if (bias) {
                float b[VEC];
                load_vec<VEC>(b, bias + c);
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[k][j] += b[j];
            }
            store_vec<VEC>(out + (int64_t)v * ldo + c, acc[k]);
        }
    }
    if (gl == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float* __restrict__ st = stat + (int64_t)v * 12 + k * 4;
            st[0] = M[k]; st[1] = LS[k]; st[2] = cn[k]; st[3] = beta[k];
        }
    }
}

// pass A: one group per source u; g_ft[u] = sum over u's out-edges of beta a_e g_out[w], r[e] = <g_out[w], ft[u]>
template <int G, int VEC, int NK>
__global__ __launch_bounds__(RA_BLOCK) void ra_bwd_src_kernel(const float* __restrict__ ft, int64_t ldf, const float* __restrict__ sc,
                                                              const int32_t* __restrict__ node_type, const float* __restrict__ stat,
                                                              const float* __restrict__ g_out, int64_t ldg, int n, int C,
                                                              const int32_t* __restrict__ colptr, const int32_t* __restrict__ csc_eid,
                                                              const int32_t* __restrict__ csc_dst, float slope,
                                                              float* __restrict__ g_ft, int64_t ldgf, float* __restrict__ r) {
    const int gl = group_lane<G>(), gbase = group_base<G>(), u = group_row<G, RA_BLOCK>();
    if (u >= n) return;                                          // group-uniform
    const int t = ra_type(node_type, u);
    const float el = sc[(int64_t)u * 4];
    float fu[NK][VEC], acc[NK][VEC];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) { fu[k][j] = 0.f; acc[k][j] = 0.f; }
        const int c = chunk_col<G, VEC>(gl, k);
        if (c < C) load_vec<VEC>(fu[k], ft + (int64_t)u * ldf + c);
    }
    const int j0 = colptr[u], j1 = colptr[u + 1];
    for (int base = j0; base < j1; base += G) {
        const int me = base + gl;
        int e_m = 0, w_m = 0;
        float a_m = 0.f;
        if (me < j1) {
            e_m = csc_eid[me];
            w_m = csc_dst[me];
            const float* __restrict__ st = stat + (int64_t)w_m * 12 + t * 4;
            a_m = expf((leaky_relu(el + sc[(int64_t)w_m * 4 + 1], slope) - st[0]) - st[1]) * st[3];
        }
        const int cnt = min(G, j1 - base);
        for (int j = 0; j < cnt; ++j) {
            const int w = __shfl(w_m, gbase + j), e = __shfl(e_m, gbase + j);
            const float a = __shfl(a_m, gbase + j);
            const float* __restrict__ row = g_out + (int64_t)w * ldg;
            float p = 0.f;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int c = chunk_col<G, VEC>(gl, k);
                if (c < C) {
                    float g[VEC];
                    load_vec<VEC>(g, row + c);
#pragma unroll
                    for (int jj = 0; jj < VEC; ++jj) { acc[k][jj] = fmaf(a, g[jj], acc[k][jj]); p = fmaf(g[jj], fu[k][jj], p); }
                }
            }
            p = group_sum<G>(p);
            if (gl == 0) r[e] = p;
        }
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = chunk_col<G, VEC>(gl, k);
        if (c < C) store_vec<VEC>(g_ft + (int64_t)u * ldgf + c, acc[k]);
    }
}

// pass B: 16 lanes per destination v; r (in: r_e, out: g_pre_e), gq [n, 3], g_sc[v, 1] = g_er, g_sc[v, 3] = g_pr
__global__ __launch_bounds__(RA_BLOCK) void ra_bwd_dst_kernel(const float* __restrict__ sc, const int32_t* __restrict__ node_type,
                                                              const float* __restrict__ stat, int n, const int32_t* __restrict__ rowptr,
                                                              const int32_t* __restrict__ src, float slope, float* __restrict__ r,
                                                              float* __restrict__ gq, float* __restrict__ g_sc) {
    constexpr int G = RA_S_LANES;
    const int gl = group_lane<G>(), v = group_row<G, RA_BLOCK>();
    if (v >= n) return;
    const int e0 = rowptr[v], e1 = rowptr[v + 1];
    const float erv = sc[(int64_t)v * 4 + 1], prv = sc[(int64_t)v * 4 + 3];
    float M[3], LS[3], cn[3], beta[3], A[3], ps[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* __restrict__ st = stat + (int64_t)v * 12 + k * 4;
        M[k] = st[0]; LS[k] = st[1]; cn[k] = st[2]; beta[k] = st[3];
        A[k] = 0.f; ps[k] = 0.f;
    }
    for (int e = e0 + gl; e < e1; e += G) {
        const int u = src[e], t = ra_type(node_type, u);
        const float s = leaky_relu(sc[(int64_t)u * 4] + erv, slope);
        const float a = expf((s - ra_pick(t, M[0], M[1], M[2])) - ra_pick(t, LS[0], LS[1], LS[2]));
        const float ar = a * r[e], p = sc[(int64_t)u * 4 + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (t == k) { A[k] += ar; ps[k] += p; }
    }
    float abar = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        A[k] = group_sum<G>(A[k]);
        ps[k] = group_sum<G>(ps[k]);
        abar = fmaf(beta[k], A[k], abar);
    }
    float ger = 0.f;
    for (int e = e0 + gl; e < e1; e += G) {
        const int u = src[e], t = ra_type(node_type, u);
        const float pre = sc[(int64_t)u * 4] + erv;
        const float a = expf((leaky_relu(pre, slope) - ra_pick(t, M[0], M[1], M[2])) - ra_pick(t, LS[0], LS[1], LS[2]));
        const float gp = ra_pick(t, beta[0], beta[1], beta[2]) * a * (r[e] - ra_pick(t, A[0], A[1], A[2])) * (pre > 0.f ? 1.f : slope);
        r[e] = gp;
        ger += gp;
    }
    ger = group_sum<G>(ger);
    if (gl == 0) {
        float gpr = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float g = 0.f;
            if (cn[k] > 0.f) {
                const float qpre = ps[k] / cn[k] + prv;
                const float gqv = beta[k] * (A[k] - abar) * (qpre > 0.f ? 1.f : slope);
                gpr += gqv;
                g = gqv / cn[k];
            }
            gq[(int64_t)v * 3 + k] = g;
        }
        g_sc[(int64_t)v * 4 + 1] = ger;
        g_sc[(int64_t)v * 4 + 3] = gpr;
    }
}

// pass C: 16 lanes per source u; g_sc[u, 0] = g_el = sum of g_pre over u's out-edges, g_sc[u, 2] = g_pl = sum of gq[w, t(u)]
__global__ __launch_bounds__(RA_BLOCK) void ra_bwd_score_kernel(const int32_t* __restrict__ node_type, int n, const int32_t* __restrict__ colptr,
                                                                const int32_t* __restrict__ csc_eid, const int32_t* __restrict__ csc_dst,
                                                                const float* __restrict__ g_pre, const float* __restrict__ gq,
                                                                float* __restrict__ g_sc) {
    constexpr int G = RA_S_LANES;
    const int gl = group_lane<G>(), u = group_row<G, RA_BLOCK>();
    if (u >= n) return;
    const int t = ra_type(node_type, u);
    float gel = 0.f, gpl = 0.f;
    for (int jj = colptr[u] + gl; jj < colptr[u + 1]; jj += G) {
        gel += g_pre[csc_eid[jj]];
        gpl += gq[(int64_t)csc_dst[jj] * 3 + t];
    }
    gel = group_sum<G>(gel);
    gpl = group_sum<G>(gpl);
    if (gl == 0) {
        g_sc[(int64_t)u * 4] = gel;
        g_sc[(int64_t)u * 4 + 2] = gpl;
    }
}

// part[b, c] = sum of g_out[r, c] over the rows r = b, b + WSI_RA_BIAS_PARTS, ...
__global__ __launch_bounds__(256) void ra_bias_part_kernel(const float* __restrict__ g_out, int64_t ldg, int n, int C, float* __restrict__ part) {
    const int c = (int)blockIdx.x * 256 + (int)threadIdx.x, b = (int)blockIdx.y;
    if (c >= C) return;
    float s = 0.f;
    for (int r = b; r < n; r += WSI_RA_BIAS_PARTS) s += g_out[(int64_t)r * ldg + c];
    part[(int64_t)b * C + c] = s;
}

__global__ __launch_bounds__(256) void ra_bias_sum_kernel(const float* __restrict__ part, int C, float* __restrict__ g_bias) {
    const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int b = 0; b < WSI_RA_BIAS_PARTS; ++b) s += part[(int64_t)b * C + c];
    g_bias[c] = s;
}

// ---------------------------------------------------------------------------------------------------- host side
static int ra_check_shape(const char* what, int32_t n, int32_t C) {
    if (n < 0 || C < 1 || C > RA_MAX_WIDTH) {
        set_error("%s: bad shape n=%d C=%d (n >= 0, 1 <= C <= %d)", what, n, C, RA_MAX_WIDTH);
        return WSI_EINVAL;
    }
    return WSI_OK;
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_ra_attn_fwd(const float* ft, int64_t ldf, const float* sc, const int32_t* node_type, int32_t n, int32_t C,
                               const int32_t* rowptr, const int32_t* src, float negative_slope, const float* bias,
                               float* out, int64_t ldo, float* stat, void* stream) {
    if (int rc = ra_check_shape("ra_attn_fwd", n, C)) return rc;
    if (ldf < C || ldo < C) { set_error("ra_attn_fwd: row stride below C"); return WSI_EINVAL; }
    if (n == 0) return WSI_OK;
    if (!ft || !sc || !node_type || !rowptr || !src || !out || !stat) { set_error("ra_attn_fwd: null pointer"); return WSI_EINVAL; }
    const RowCfg cfg = row_cfg(C, C, 1, ldf % 4 == 0 && ldo % 4 == 0 && aligned16(ft) && aligned16(out) && aligned16(bias));
    hipStream_t st = (hipStream_t)stream;
    const int per = RA_BLOCK / cfg.G;
#define CALL(G_, V_, K_) hipLaunchKernelGGL((ra_fwd_kernel<G_, V_, K_>), dim3((n + per - 1) / per), dim3(RA_BLOCK), 0, st, ft, ldf, sc, node_type, n, C, \
                                            rowptr, src, negative_slope, bias, out, ldo, stat)
    ROW_GROUP_DISPATCH_ALL("ra_attn", cfg, CALL);
#undef CALL
    return check_launch("ra_attn_fwd");
}

extern "C" int wsi_ra_attn_bwd(const float* ft, int64_t ldf, const float* sc, const int32_t* node_type, const float* stat,
                               const float* g_out, int64_t ldg, int32_t n, int32_t E, int32_t C,
                               const int32_t* rowptr, const int32_t* src, const int32_t* colptr, const int32_t* csc_eid,
                               const int32_t* csc_dst, float negative_slope, float* edge_ws, float* group_ws, float* bias_ws,
                               float* g_ft, int64_t ldgf, float* g_sc, float* g_bias, void* stream) {
    if (int rc = ra_check_shape("ra_attn_bwd", n, C)) return rc;
    if (E < 0) { set_error("ra_attn_bwd: E=%d", E); return WSI_EINVAL; }
    if (ldf < C || ldg < C || ldgf < C) { set_error("ra_attn_bwd: row stride below C"); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (g_bias && hipMemsetAsync(g_bias, 0, (size_t)C * 4, st) != hipSuccess) return check_launch("ra_attn_bwd(memset)");
        return WSI_OK;
    }
    if (!ft || !sc || !node_type || !stat || !g_out || !rowptr || !src || !colptr || !csc_eid || !csc_dst || !group_ws || !g_ft || !g_sc ||
        (E > 0 && !edge_ws) || (g_bias && !bias_ws)) {
        set_error("ra_attn_bwd: null pointer");
        return WSI_EINVAL;
    }
    const RowCfg cfg = row_cfg(C, C, 1, ldf % 4 == 0 && ldg % 4 == 0 && ldgf % 4 == 0 && aligned16(ft) && aligned16(g_out) && aligned16(g_ft));
    const int per = RA_BLOCK / cfg.G;
#define CALL(G_, V_, K_) hipLaunchKernelGGL((ra_bwd_src_kernel<G_, V_, K_>), dim3((n + per - 1) / per), dim3(RA_BLOCK), 0, st, ft, ldf, sc, node_type, stat, \
                                            g_out, ldg, n, C, colptr, csc_eid, csc_dst, negative_slope, g_ft, ldgf, edge_ws)
    ROW_GROUP_DISPATCH_ALL("ra_attn", cfg, CALL);
#undef CALL
    constexpr int per_s = RA_BLOCK / RA_S_LANES;
    hipLaunchKernelGGL(ra_bwd_dst_kernel, dim3((n + per_s - 1) / per_s), dim3(RA_BLOCK), 0, st, sc, node_type, stat, n, rowptr, src, negative_slope,
                       edge_ws, group_ws, g_sc);
    hipLaunchKernelGGL(ra_bwd_score_kernel, dim3((n + per_s - 1) / per_s), dim3(RA_BLOCK), 0, st, node_type, n, colptr, csc_eid, csc_dst,
                       (const float*)edge_ws, (const float*)group_ws, g_sc);
    if (g_bias) {
        hipLaunchKernelGGL(ra_bias_part_kernel, dim3((C + 255) / 256, WSI_RA_BIAS_PARTS), dim3(256), 0, st, g_out, ldg, n, C, bias_ws);
        hipLaunchKernelGGL(ra_bias_sum_kernel, dim3((C + 255) / 256), dim3(256), 0, st, (const float*)bias_ws, C, g_bias);
    }
    return check_launch("ra_attn_bwd");
}
