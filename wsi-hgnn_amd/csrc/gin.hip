// GINConv aggregation (DGL GINConv(apply_func, aggregator_type, init_eps, learn_eps), models/GIN.py:120-121) for gfx950.  Contracts:
// include/wsi_hgnn.h.
//   neigh[w] = reduce_{e: u -> w} (s_e x[u]),  reduce = sum | mean | max;   out[w] = (1 + eps) x[w] + neigh[w] (+ bias)
// Layout: the row groups of row_group.h.  The edge loop is unrolled over U edges (4 when a lane holds at most 8 floats of a row, else 2):
// the U gathers are issued before the first is used, and every edge position i mod U has an accumulator of its own.  The accumulators
// are combined in the order 0 .. U-1, so every sum has one order and the first-position rule of the maximum survives: each accumulator
// sees its positions in rising order and keeps the first of equal values, and of equal values in two accumulators the lower position wins.
//   forward   CSR by destination w:  the messages of w's in-edges; max also writes arg[w, c] = the CSR position of the first maximum
//   backward  CSC by source u:       gx[u] = (1 + eps) g[u] + sum_{e: u -> w} s_e c_w [arg[w, c] == e] g[w]   (c_w = 1 / indeg(w) under mean)
//   edge grad CSR by destination w:  g_s[e] = c_w sum_c [arg[w, c] == e] g[w, c] x[u, c]; g[w] (and arg[w]) stay in the group's registers
//   eps grad  sum of g * x over the whole table: a fixed grid of partials, then ONE workgroup adds them in order (two launches)
// MODE and SCALED (edge_s != NULL) are compile-time switches: the unscaled sum contains neither a multiply nor a compare.  eps is read
// through a device pointer.  No atomics anywhere: identical calls give identical bits.
#include "row_group.h"
#include <math.h>

namespace wsi {

constexpr int GI_BLOCK = 256;
constexpr int GI_MAX_WIDTH = 1024;
constexpr int GI_EPS_BLOCKS = 256;         // fixed grid of the eps-gradient partials (= the threads of the launch that adds them)
constexpr int GI_EPS_UNROLL = 4;

template <int VEC, int NK>
struct gi_unroll { static constexpr int U = (VEC * NK <= 8) ? 4 : 2; };

// VEC int32 words at p, through the float accessors of common.h (a move of bits)
template <int VEC>
__device__ __forceinline__ void load_ivec(int (&r)[VEC], const int32_t* __restrict__ p) {
    float t[VEC];
    load_vec<VEC>(t, reinterpret_cast<const float*>(p));
#pragma unroll
    for (int j = 0; j < VEC; ++j) r[j] = __float_as_int(t[j]);
}

template <int VEC>
__device__ __forceinline__ void store_ivec(int32_t* __restrict__ p, const int (&r)[VEC]) {
    float t[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) t[j] = __int_as_float(r[j]);
    store_vec<VEC>(reinterpret_cast<float*>(p), t);
}

template <int G, int VEC, int NK, int MODE, bool SCALED>
__global__ __launch_bounds__(GI_BLOCK) void gin_fwd_kernel(const float* __restrict__ x, int64_t ldx, int n, int D,
                                                           const int32_t* __restrict__ rowptr, const int32_t* __restrict__ src,
                                                           const float* __restrict__ edge_s, const float* __restrict__ eps,
                                                           const float* __restrict__ bias, float* __restrict__ out, int64_t ldo,
                                                           int32_t* __restrict__ arg) {
    constexpr int U = gi_unroll<VEC, NK>::U;
    constexpr bool ISMAX = MODE == WSI_GIN_MAX;
    const int gl = group_lane<G>(), w = group_row<G, GI_BLOCK>();
    if (w >= n) return;                                          // group-uniform
    bool ok[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) ok[k] = chunk_col<G, VEC>(gl, k) < D;
    const int e0 = rowptr[w], e1 = rowptr[w + 1];
    float acc[U][NK][VEC];
    int best[ISMAX ? U : 1][NK][VEC];
#pragma unroll
    for (int i = 0; i < U; ++i)
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                acc[i][k][j] = ISMAX ? -INFINITY : 0.f;
                if constexpr (ISMAX) best[i][k][j] = -1;
            }
    for (int e = e0; e < e1; e += U) {                           // (group-uniform trip count; the last round may be partial)
        float v[U][NK][VEC], s[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const bool live = e + i < e1;
            const int u = live ? src[e + i] : 0;
            s[i] = (SCALED && live) ? edge_s[e + i] : 1.f;
            const float* __restrict__ row = x + (int64_t)u * ldx;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[i][k][j] = 0.f;
                if (live && ok[k]) load_vec<VEC>(v[i][k], row + chunk_col<G, VEC>(gl, k));
            }
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            if (e + i < e1) {
#pragma unroll
                for (int k = 0; k < NK; ++k)
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        if constexpr (ISMAX) {
                            const float m = SCALED ? s[i] * v[i][k][j] : v[i][k][j];
                            if (m > acc[i][k][j]) { acc[i][k][j] = m; best[i][k][j] = e + i; }
                        } else if constexpr (SCALED) {
                            acc[i][k][j] = fmaf(s[i], v[i][k][j], acc[i][k][j]);
                        } else {
                            acc[i][k][j] += v[i][k][j];
                        }
                    }
            }
        }
    }
    const float ope = 1.f + eps[0];
    const float deg = (float)(e1 - e0 > 1 ? e1 - e0 : 1);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (ok[k]) {
            const int c = chunk_col<G, VEC>(gl, k);
            float xw[VEC], b[VEC], o[VEC];
            int a[VEC];
            load_vec<VEC>(xw, x + (int64_t)w * ldx + c);
            if (bias) load_vec<VEC>(b, bias + c);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float r = acc[0][k][j];
                if constexpr (ISMAX) {
                    int p = best[0][k][j];
#pragma unroll
                    for (int i = 1; i < U; ++i) {
                        const float ri = acc[i][k][j];
                        const int pi = best[i][k][j];
                        if (pi >= 0 && (ri > r || (ri == r && pi < p))) { r = ri; p = pi; }
                    }
                    a[j] = p;
                    r = p >= 0 ? r : 0.f;
                } else {
#pragma unroll
                    for (int i = 1; i < U; ++i) r += acc[i][k][j];
                    if constexpr (MODE == WSI_GIN_MEAN) r = r / deg;
                }
                o[j] = fmaf(ope, xw[j], r) + (bias ? b[j] : 0.f);
            }
            store_vec<VEC>(out + (int64_t)w * ldo + c, o);
            if constexpr (ISMAX) {
                if (arg) store_ivec<VEC>(arg + (int64_t)w * D + c, a);
            }
        }
    }
}

template <int G, int VEC, int NK, int MODE, bool SCALED>
__global__ __launch_bounds__(GI_BLOCK) void gin_bwd_kernel(const float* __restrict__ g, int64_t ldg, int n, int D,
                                                           const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colptr,
                                                           const int32_t* __restrict__ csc_eid, const int32_t* __restrict__ csc_dst,
                                                           const float* __restrict__ edge_s, const float* __restrict__ eps,
                                                           const int32_t* __restrict__ arg, float* __restrict__ gx, int64_t ldgx) {
    constexpr int U = gi_unroll<VEC, NK>::U;
    constexpr bool ISMAX = MODE == WSI_GIN_MAX;
    constexpr bool COEF = SCALED || MODE == WSI_GIN_MEAN;
    const int gl = group_lane<G>(), u = group_row<G, GI_BLOCK>();
    if (u >= n) return;                                          // group-uniform
    bool ok[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) ok[k] = chunk_col<G, VEC>(gl, k) < D;
    float acc[U][NK][VEC];
#pragma unroll
    for (int i = 0; i < U; ++i) zero_chunks(acc[i]);
    const int j0 = colptr[u], j1 = colptr[u + 1];
    for (int jj = j0; jj < j1; jj += U) {
        float v[U][NK][VEC], cf[U];
        int a[ISMAX ? U : 1][NK][VEC], eid[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const bool live = jj + i < j1;
            const int w = live ? csc_dst[jj + i] : 0;
            eid[i] = live ? csc_eid[jj + i] : -2;
            cf[i] = (SCALED && live) ? edge_s[eid[i]] : 1.f;
            if constexpr (MODE == WSI_GIN_MEAN) {
                const int d = live ? rowptr[w + 1] - rowptr[w] : 1;
                cf[i] = cf[i] / (float)(d > 1 ? d : 1);
            }
            const float* __restrict__ row = g + (int64_t)w * ldg;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[i][k][j] = 0.f;
                if (live && ok[k]) {
                    load_vec<VEC>(v[i][k], row + chunk_col<G, VEC>(gl, k));
                    if constexpr (ISMAX) load_ivec<VEC>(a[i][k], arg + (int64_t)w * D + chunk_col<G, VEC>(gl, k));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            if (jj + i < j1) {
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    if (ok[k]) {
#pragma unroll
                        for (int j = 0; j < VEC; ++j) {
                            float t = v[i][k][j];
                            if constexpr (ISMAX) t = a[i][k][j] == eid[i] ? t : 0.f;
                            if constexpr (COEF) acc[i][k][j] = fmaf(cf[i], t, acc[i][k][j]);
                            else acc[i][k][j] += t;
                        }
                    }
                }
            }
        }
    }
    const float ope = 1.f + eps[0];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (ok[k]) {
            const int c = chunk_col<G, VEC>(gl, k);
            float gu[VEC], o[VEC];
            load_vec<VEC>(gu, g + (int64_t)u * ldg + c);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float r = acc[0][k][j];
#pragma unroll
                for (int i = 1; i < U; ++i) r += acc[i][k][j];
                o[j] = fmaf(ope, gu[j], r);
            }
            store_vec<VEC>(gx + (int64_t)u * ldgx + c, o);
        }
    }
}

// one group per destination w: g[w] (and arg[w] under max) in registers, one gather of x[u] per edge, U edges in flight
template <int G, int VEC, int NK, bool ISMAX>
__global__ __launch_bounds__(GI_BLOCK) void gin_edge_grad_kernel(const float* __restrict__ g, int64_t ldg, const float* __restrict__ x, int64_t ldx,
                                                                 int n, int D, const int32_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ src, bool mean, const int32_t* __restrict__ arg,
                                                                 float* __restrict__ g_s) {
    constexpr int U = gi_unroll<VEC, NK>::U;
    const int gl = group_lane<G>(), w = group_row<G, GI_BLOCK>();
    if (w >= n) return;                                          // group-uniform
    bool ok[NK];
    float gw[NK][VEC];
    int aw[ISMAX ? NK : 1][VEC];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int c = chunk_col<G, VEC>(gl, k);
        ok[k] = c < D;
#pragma unroll
        for (int j = 0; j < VEC; ++j) gw[k][j] = 0.f;
        if (ok[k]) {
            load_vec<VEC>(gw[k], g + (int64_t)w * ldg + c);
            if constexpr (ISMAX) load_ivec<VEC>(aw[k], arg + (int64_t)w * D + c);
        }
    }
    const int e0 = rowptr[w], e1 = rowptr[w + 1];
    const float deg = (mean && e1 - e0 > 1) ? (float)(e1 - e0) : 1.f;
    for (int e = e0; e < e1; e += U) {
        float v[U][NK][VEC];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const bool live = e + i < e1;
            const int u = live ? src[e + i] : 0;
            const float* __restrict__ row = x + (int64_t)u * ldx;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) v[i][k][j] = 0.f;
                if (live && ok[k]) load_vec<VEC>(v[i][k], row + chunk_col<G, VEC>(gl, k));
            }
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            float p = 0.f;
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                if (ok[k]) {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) {
                        if constexpr (ISMAX) p = fmaf(aw[k][j] == e + i ? gw[k][j] : 0.f, v[i][k][j], p);
                        else p = fmaf(gw[k][j], v[i][k][j], p);
                    }
                }
            }
            p = group_sum<G>(p);                                 // (every lane of the group is here: the trip count is group-uniform)
            if (gl == 0 && e + i < e1) g_s[e + i] = p / deg;
        }
    }
}

// partial[b] = the sum of g * x over the elements workgroup b strides over, added lane-first, then wave by wave
__global__ __launch_bounds__(GI_BLOCK) void gin_eps_partial_kernel(const float* __restrict__ g, int64_t ldg, const float* __restrict__ x, int64_t ldx,
                                                                   int n, int D, float* __restrict__ partial) {
    const int64_t total = (int64_t)n * D, step = (int64_t)GI_EPS_BLOCKS * GI_BLOCK;
    float acc[GI_EPS_UNROLL];
#pragma unroll
    for (int i = 0; i < GI_EPS_UNROLL; ++i) acc[i] = 0.f;
    for (int64_t t0 = (int64_t)blockIdx.x * GI_BLOCK + threadIdx.x; t0 < total; t0 += step * GI_EPS_UNROLL) {
        float a[GI_EPS_UNROLL], b[GI_EPS_UNROLL];
#pragma unroll
        for (int i = 0; i < GI_EPS_UNROLL; ++i) {
            const int64_t t = t0 + step * i;
            const bool live = t < total;
            const int64_t r = live ? t / D : 0;
            const int c = live ? (int)(t - r * D) : 0;
            a[i] = live ? g[r * ldg + c] : 0.f;
            b[i] = live ? x[r * ldx + c] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < GI_EPS_UNROLL; ++i) acc[i] = fmaf(a[i], b[i], acc[i]);
    }
    float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    s = wave_sum(s);
    __shared__ float sh[GI_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(GI_EPS_BLOCKS) void gin_eps_finish_kernel(const float* __restrict__ partial, float* __restrict__ g_eps) {
    static_assert(GI_EPS_BLOCKS == 256, "one partial per thread, four waves");
    float s = wave_sum(partial[threadIdx.x]);
    __shared__ float sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) g_eps[0] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// ---------------------------------------------------------------------------------------------------- host side
static int gi_check_shape(const char* what, int32_t n, int32_t D) {
    if (n < 0 || D <= 0) { set_error("%s: bad shape n=%d D=%d", what, n, D); return WSI_EINVAL; }
    if (D > GI_MAX_WIDTH) { set_error("%s: D=%d > %d", what, D, GI_MAX_WIDTH); return WSI_ENOSYS; }
    return WSI_OK;
}

static int gi_check_mode(const char* what, int32_t mode) {
    if (mode != WSI_GIN_SUM && mode != WSI_GIN_MEAN && mode != WSI_GIN_MAX) {
        set_error("%s: mode %d (0 sum, 1 mean, 2 max)", what, mode);
        return WSI_EINVAL;
    }
    return WSI_OK;
}

template <int MODE, bool SCALED>
static int gi_fwd(const float* x, int64_t ldx, int32_t n, int32_t D, const int32_t* rowptr, const int32_t* src, const float* edge_s,
                  const float* eps, const float* bias, float* out, int64_t ldo, int32_t* arg, RowCfg cfg, hipStream_t st) {
    const int per = GI_BLOCK / cfg.G;
#define CALL(G_, V_, K_) hipLaunchKernelGGL((gin_fwd_kernel<G_, V_, K_, MODE, SCALED>), dim3((n + per - 1) / per), dim3(GI_BLOCK), 0, st, x, ldx, \
                                            (int)n, (int)D, rowptr, src, edge_s, eps, bias, out, ldo, arg)
    ROW_GROUP_DISPATCH_NARROW("gin", cfg, CALL);
#undef CALL
    return WSI_OK;
}

template <int MODE, bool SCALED>
static int gi_bwd(const float* g, int64_t ldg, int32_t n, int32_t D, const int32_t* rowptr, const int32_t* colptr, const int32_t* csc_eid,
                  const int32_t* csc_dst, const float* edge_s, const float* eps, const int32_t* arg, float* gx, int64_t ldgx, RowCfg cfg,
                  hipStream_t st) {
    const int per = GI_BLOCK / cfg.G;
#define CALL(G_, V_, K_) hipLaunchKernelGGL((gin_bwd_kernel<G_, V_, K_, MODE, SCALED>), dim3((n + per - 1) / per), dim3(GI_BLOCK), 0, st, g, ldg, \
                                            (int)n, (int)D, rowptr, colptr, csc_eid, csc_dst, edge_s, eps, arg, gx, ldgx)
    ROW_GROUP_DISPATCH_NARROW("gin", cfg, CALL);
#undef CALL
    return WSI_OK;
}

template <bool ISMAX>
static int gi_edge(const float* g, int64_t ldg, const float* x, int64_t ldx, int32_t n, int32_t D, const int32_t* rowptr, const int32_t* src,
                   bool mean, const int32_t* arg, float* g_s, RowCfg cfg, hipStream_t st) {
    const int per = GI_BLOCK / cfg.G;
#define CALL(G_, V_, K_) hipLaunchKernelGGL((gin_edge_grad_kernel<G_, V_, K_, ISMAX>), dim3((n + per - 1) / per), dim3(GI_BLOCK), 0, st, g, ldg, \
                                            x, ldx, (int)n, (int)D, rowptr, src, mean, arg, g_s)
    ROW_GROUP_DISPATCH_NARROW("gin", cfg, CALL);
#undef CALL
    return WSI_OK;
}

// FN<MODE, SCALED>(args) for the run-time (mode, scaled)
#define GI_BY_MODE(rc, FN, mode, scaled, ...)                                                                       \
    do {                                                                                                            \
        if ((mode) == WSI_GIN_SUM) rc = (scaled) ? FN<WSI_GIN_SUM, true>(__VA_ARGS__) : FN<WSI_GIN_SUM, false>(__VA_ARGS__);      \
        else if ((mode) == WSI_GIN_MEAN) rc = (scaled) ? FN<WSI_GIN_MEAN, true>(__VA_ARGS__) : FN<WSI_GIN_MEAN, false>(__VA_ARGS__); \
        else rc = (scaled) ? FN<WSI_GIN_MAX, true>(__VA_ARGS__) : FN<WSI_GIN_MAX, false>(__VA_ARGS__);                \
    } while (0)

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_gin_aggregate_fwd(const float* x, int64_t ldx, int32_t n, int32_t D, const int32_t* rowptr, const int32_t* src,
                                     const float* edge_s, const float* eps, int32_t mode, const float* bias, float* out, int64_t ldo,
                                     int32_t* arg, void* stream) {
    if (int rc = gi_check_shape("gin_aggregate_fwd", n, D)) return rc;
    if (int rc = gi_check_mode("gin_aggregate_fwd", mode)) return rc;
    if (ldx < D || ldo < D) { set_error("gin_aggregate_fwd: row stride below D"); return WSI_EINVAL; }
    if (n == 0) return WSI_OK;
    if (!x || !rowptr || !eps || !out) { set_error("gin_aggregate_fwd: null pointer"); return WSI_EINVAL; }     // (src: NULL for a graph without edges, never read then)
    const bool has_arg = mode == WSI_GIN_MAX && arg;
    const RowCfg cfg = row_cfg(D, D, 1, vec_ok(x, ldx) && vec_ok(out, ldo) && aligned16(bias) && (!has_arg || aligned16(arg)));
    int rc;
    GI_BY_MODE(rc, gi_fwd, mode, edge_s != nullptr, x, ldx, n, D, rowptr, src, edge_s, eps, bias, out, ldo, arg, cfg, (hipStream_t)stream);
    if (rc) return rc;
    return check_launch("gin_aggregate_fwd");
}

extern "C" int wsi_gin_aggregate_bwd(const float* g, int64_t ldg, int32_t n, int32_t D, const int32_t* rowptr, const int32_t* colptr,
                                     const int32_t* csc_eid, const int32_t* csc_dst, const float* edge_s, const float* eps, int32_t mode,
                                     const int32_t* arg, float* gx, int64_t ldgx, void* stream) {
    if (int rc = gi_check_shape("gin_aggregate_bwd", n, D)) return rc;
    if (int rc = gi_check_mode("gin_aggregate_bwd", mode)) return rc;
    if (ldg < D || ldgx < D) { set_error("gin_aggregate_bwd: row stride below D"); return WSI_EINVAL; }
    if (n == 0) return WSI_OK;
    if (!g || !rowptr || !colptr || !eps || !gx || (mode == WSI_GIN_MAX && !arg)) {                     // (csc_eid, csc_dst: NULL without edges)
        set_error("gin_aggregate_bwd: null pointer");
        return WSI_EINVAL;
    }
    const RowCfg cfg = row_cfg(D, D, 1, vec_ok(g, ldg) && vec_ok(gx, ldgx) && (mode != WSI_GIN_MAX || aligned16(arg)));
    int rc;
    GI_BY_MODE(rc, gi_bwd, mode, edge_s != nullptr, g, ldg, n, D, rowptr, colptr, csc_eid, csc_dst, edge_s, eps, arg, gx, ldgx, cfg,
               (hipStream_t)stream);
    if (rc) return rc;
    return check_launch("gin_aggregate_bwd");
}

extern "C" int wsi_gin_edge_grad(const float* g, int64_t ldg, const float* x, int64_t ldx, int32_t n, int32_t D, const int32_t* rowptr,
                                 const int32_t* src, int32_t mode, const int32_t* arg, float* g_s, void* stream) {
    if (int rc = gi_check_shape("gin_edge_grad", n, D)) return rc;
    if (int rc = gi_check_mode("gin_edge_grad", mode)) return rc;
    if (ldg < D || ldx < D) { set_error("gin_edge_grad: row stride below D"); return WSI_EINVAL; }
    if (n == 0) return WSI_OK;
    if (!g || !x || !rowptr || (mode == WSI_GIN_MAX && !arg)) { set_error("gin_edge_grad: null pointer"); return WSI_EINVAL; }   // (src, g_s: NULL without edges)
    const RowCfg cfg = row_cfg(D, D, 1, vec_ok(g, ldg) && vec_ok(x, ldx) && (mode != WSI_GIN_MAX || aligned16(arg)));
    const int rc = mode == WSI_GIN_MAX ? gi_edge<true>(g, ldg, x, ldx, n, D, rowptr, src, false, arg, g_s, cfg, (hipStream_t)stream)
                                       : gi_edge<false>(g, ldg, x, ldx, n, D, rowptr, src, mode == WSI_GIN_MEAN, arg, g_s, cfg, (hipStream_t)stream);
    if (rc) return rc;
    return check_launch("gin_edge_grad");
}

extern "C" int32_t wsi_gin_eps_partials(void) { return GI_EPS_BLOCKS; }

extern "C" int wsi_gin_eps_grad(const float* g, int64_t ldg, const float* x, int64_t ldx, int32_t n, int32_t D, float* partial, float* g_eps,
                                void* stream) {
    if (int rc = gi_check_shape("gin_eps_grad", n, D)) return rc;
    if (ldg < D || ldx < D) { set_error("gin_eps_grad: row stride below D"); return WSI_EINVAL; }
    if (n == 0) return WSI_OK;
    if (!g || !x || !partial || !g_eps) { set_error("gin_eps_grad: null pointer"); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gin_eps_partial_kernel, dim3(GI_EPS_BLOCKS), dim3(GI_BLOCK), 0, st, g, ldg, x, ldx, (int)n, (int)D, partial);
    hipLaunchKernelGGL(gin_eps_finish_kernel, dim3(1), dim3(GI_EPS_BLOCKS), 0, st, (const float*)partial, g_eps);
    return check_launch("gin_eps_grad");
}
