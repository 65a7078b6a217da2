// BatchNorm1d over the LIVE rows of a padded table (ops.masked_batch_norm; gtn.GCNBlock on a gtn.GraphSlot).  Contract:
// include/wsi_hgnn.h.
//
// x [rows, C] is a narrow table (C = 64 in the reference) of tens of thousands of rows, live [rows] is 0 / 1, and the number of live rows is a
// word on the DEVICE (a captured step replays over batches of other sizes).  Everything here streams the table once per pass:
//   statistics : workgroup = (chunk of MB_CHUNK rows, 64 columns); a lane owns a column, a wave every fourth row, eight rows in flight.  Each
//                lane keeps a running (count, mean, M2) of its live rows (Welford), the four waves are merged in wave order (Chan), and the
//                chunk's triple is stored.  A second small launch merges a column's chunk triples - lanes strided over the chunks in chunk
//                order, then a fixed butterfly - and writes mean, 1 / sqrt(var + eps) and the running statistics.  The variance is CENTRED at
//                every level: no E[x^2] - mean^2 anywhere.
//   normalise  : elementwise, 16-byte lane accesses when C and the strides allow; dead rows are written as 0.
//   backward   : the same two-level shape for dbeta = sum g and dgamma = sum g xhat (plain sums in one fixed order), then an elementwise pass
//                dx = gamma rstd (g - dbeta / n - xhat dgamma / n), 0 in dead rows.
// No atomics; every sum has one order, so identical calls give identical bits.
//
// BatchNorm + ReLU in the same passes (wsi_masked_bn_relu_fwd / _bwd; models/GIN.py): a `bool RELU` parameter on the normalise,
// gradient-sum and dx kernels.  With y = mb_affine(x, mean, rstd, gamma, beta), forward writes y > 0 ? y : 0 and both backward kernels
// read g as g [y > 0], recomputing y from x and the saved stats through the SAME function: the sign backward sees is the sign forward used,
// bit for bit, and neither y nor a mask is stored.  y == 0 is on the zero side.  The statistics kernels do not know about the ReLU.
#include "common.h"
#include <math.h>
#include <initializer_list>

namespace wsi {

constexpr int MB_THREADS = 256;
constexpr int MB_CHUNK = 128;           // rows per workgroup of the two partial kernels (32 per wave)
constexpr int MB_UNROLL = 8;            // rows a wave has in flight

struct mb_moments { float n, mean, m2; };

// Chan's merge of two (count, mean, M2) triples; either side may be empty.
__device__ __forceinline__ mb_moments mb_merge(const mb_moments a, const mb_moments b) {
    if (b.n == 0.f) return a;
    if (a.n == 0.f) return b;
    const float n = a.n + b.n, delta = b.mean - a.mean;
    mb_moments o;
    o.n = n;
    o.mean = a.mean + delta * (b.n / n);
    o.m2 = a.m2 + b.m2 + delta * delta * (a.n * b.n / n);
    return o;
}

__global__ __launch_bounds__(MB_THREADS) void masked_bn_moments_kernel(const float* __restrict__ x, int64_t ldx, int rows, int C,
                                                                       const float* __restrict__ live, float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c = (int)blockIdx.y * 64 + lane;
    const bool has = c < C;
    const int r0 = (int)blockIdx.x * MB_CHUNK;
    const int r1 = r0 + MB_CHUNK < rows ? r0 + MB_CHUNK : rows;
    mb_moments a = {0.f, 0.f, 0.f};
    for (int rb = r0 + wave; rb < r1; rb += 4 * MB_UNROLL) {
        float xv[MB_UNROLL], lv[MB_UNROLL];
#pragma unroll
        for (int k = 0; k < MB_UNROLL; ++k) {
            const int r = rb + 4 * k;
            const bool ok = r < r1;
            lv[k] = ok ? live[r] : 0.f;
            xv[k] = (ok && has) ? x[(int64_t)r * ldx + c] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < MB_UNROLL; ++k) {
            if (lv[k] != 0.f) {                                  // (wave-uniform: live is a property of the row)
                a.n += 1.f;
                const float d = xv[k] - a.mean;
                a.mean += d / a.n;
                a.m2 = fmaf(d, xv[k] - a.mean, a.m2);
            }
        }
    }
    __shared__ float sh[3][4][64];
    sh[0][wave][lane] = a.n; sh[1][wave][lane] = a.mean; sh[2][wave][lane] = a.m2;
    __syncthreads();
    if (wave == 0 && has) {
        mb_moments t = {sh[0][0][lane], sh[1][0][lane], sh[2][0][lane]};
#pragma unroll
        for (int w = 1; w < 4; ++w) t = mb_merge(t, mb_moments{sh[0][w][lane], sh[1][w][lane], sh[2][w][lane]});
        float* p = partial + (int64_t)blockIdx.x * 3 * C;
        p[c] = t.n; p[C + c] = t.mean; p[2 * C + c] = t.m2;
    }
}

// one wave per column: the chunk triples merged in one fixed order; n = the live-row count word
__global__ __launch_bounds__(64) void masked_bn_finish_kernel(const float* __restrict__ partial, int chunks, int C, const float* __restrict__ live_rows,
                                                              float momentum, float eps, float* __restrict__ running_mean,
                                                              float* __restrict__ running_var, float* __restrict__ stats) {
    const int c = blockIdx.x, lane = threadIdx.x;
    mb_moments a = {0.f, 0.f, 0.f};
    for (int p = lane; p < chunks; p += 64) {
        const float* q = partial + (int64_t)p * 3 * C;
        a = mb_merge(a, mb_moments{q[c], q[C + c], q[2 * C + c]});
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        mb_moments b = {__shfl_xor(a.n, o), __shfl_xor(a.mean, o), __shfl_xor(a.m2, o)};
        a = (lane & o) ? mb_merge(b, a) : mb_merge(a, b);        // (both lanes of a pair merge lower-lane-first: the same bits in both)
    }
    if (lane == 0) {
        const float n = live_rows[0];
        const float var = a.m2 / n;
        stats[c] = a.mean;
        stats[C + c] = 1.f / sqrtf(var + eps);
        if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * a.mean;
        if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (a.m2 / (n - 1.f));
    }
}

__global__ __launch_bounds__(64) void masked_bn_eval_stats_kernel(const float* __restrict__ running_mean, const float* __restrict__ running_var,
                                                                  int C, float eps, float* __restrict__ stats) {
    const int c = (int)blockIdx.x * 64 + threadIdx.x;
    if (c < C) { stats[c] = running_mean[c]; stats[C + c] = 1.f / sqrtf(running_var[c] + eps); }
}

// the affine output of one entry: the one expression forward and (RELU) both backward kernels evaluate
__device__ __forceinline__ float mb_affine(float x, float mean, float rstd, float gamma, float beta) {
    return fmaf((x - mean) * rstd, gamma, beta);
}

// y = live ? (x - mean) rstd gamma + beta : 0;  RELU: max(y, 0), y == 0 and dead rows giving 0
template <int V, bool RELU>
__global__ __launch_bounds__(MB_THREADS) void masked_bn_apply_kernel(const float* __restrict__ x, int64_t ldx, int rows, int C,
                                                                     const float* __restrict__ live, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, const float* __restrict__ stats,
                                                                     float* __restrict__ y, int64_t ldy) {
    const int cv = (C + V - 1) / V;
    const int64_t total = (int64_t)rows * cv;
    for (int64_t i = (int64_t)blockIdx.x * MB_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * MB_THREADS) {
        const int r = (int)(i / cv), c = (int)(i - (int64_t)r * cv) * V;
        float v[V] = {}, o[V];
        const bool alive = live[r] != 0.f;
        if (alive) load_vec<V>(v, x + (int64_t)r * ldx + c);
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float yk = mb_affine(v[k], stats[c + k], stats[C + c + k], gamma ? gamma[c + k] : 1.f, beta ? beta[c + k] : 0.f);
            o[k] = alive && (!RELU || yk > 0.f) ? yk : 0.f;
        }
        store_vec<V>(y + (int64_t)r * ldy + c, o);
    }
}

// chunk partials of dbeta = sum g and dgamma = sum g xhat over the live rows;  RELU: g counts where the forward's y was > 0
template <bool RELU>
__global__ __launch_bounds__(MB_THREADS) void masked_bn_grad_sums_kernel(const float* __restrict__ gy, int64_t ldg, const float* __restrict__ x,
                                                                         int64_t ldx, int rows, int C, const float* __restrict__ live,
                                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                         const float* __restrict__ stats, float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int c = (int)blockIdx.y * 64 + lane;
    const bool has = c < C;
    const int r0 = (int)blockIdx.x * MB_CHUNK;
    const int r1 = r0 + MB_CHUNK < rows ? r0 + MB_CHUNK : rows;
    const float mean = has ? stats[c] : 0.f, rstd = has ? stats[C + c] : 0.f;
    const float gam = (RELU && has && gamma) ? gamma[c] : 1.f, bet = (RELU && has && beta) ? beta[c] : 0.f;
    float sg = 0.f, sgx = 0.f;
    for (int rb = r0 + wave; rb < r1; rb += 4 * MB_UNROLL) {
        float xv[MB_UNROLL], gv[MB_UNROLL];
#pragma unroll
        for (int k = 0; k < MB_UNROLL; ++k) {
            const int r = rb + 4 * k;
            const bool ok = r < r1 && has && live[r] != 0.f;
            xv[k] = ok ? x[(int64_t)r * ldx + c] : mean;
            gv[k] = ok ? gy[(int64_t)r * ldg + c] : 0.f;
            if (RELU) gv[k] = mb_affine(xv[k], mean, rstd, gam, bet) > 0.f ? gv[k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < MB_UNROLL; ++k) {
            sg += gv[k];
            sgx = fmaf(gv[k], (xv[k] - mean) * rstd, sgx);
        }
    }
    __shared__ float sh[2][4][64];
    sh[0][wave][lane] = sg; sh[1][wave][lane] = sgx;
    __syncthreads();
    if (wave == 0 && has) {
        float* p = partial + (int64_t)blockIdx.x * 2 * C;
        p[c] = (sh[0][0][lane] + sh[0][1][lane]) + (sh[0][2][lane] + sh[0][3][lane]);
        p[C + c] = (sh[1][0][lane] + sh[1][1][lane]) + (sh[1][2][lane] + sh[1][3][lane]);
    }
}

__global__ __launch_bounds__(64) void masked_bn_grad_finish_kernel(const float* __restrict__ partial, int chunks, int C, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta) {
    const int c = blockIdx.x, lane = threadIdx.x;
    float sg = 0.f, sgx = 0.f;
    for (int p = lane; p < chunks; p += 64) {
        const float* q = partial + (int64_t)p * 2 * C;
        sg += q[c]; sgx += q[C + c];
    }
    sg = wave_sum(sg); sgx = wave_sum(sgx);
    if (lane == 0) { dbeta[c] = sg; dgamma[c] = sgx; }
}

// training: dx = gamma rstd (g - dbeta / n - xhat dgamma / n);  eval (the statistics are constants): dx = gamma rstd g;  0 in dead rows.
// RELU: g is taken as 0 where the forward's y was <= 0 (beta is read for that alone)
template <int V, bool RELU>
__global__ __launch_bounds__(MB_THREADS) void masked_bn_dx_kernel(const float* __restrict__ gy, int64_t ldg, const float* __restrict__ x, int64_t ldx,
                                                                  int rows, int C, const float* __restrict__ live, const float* __restrict__ live_rows,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ stats, const float* __restrict__ dgamma,
                                                                  const float* __restrict__ dbeta, bool training, float* __restrict__ dx,
                                                                  int64_t lddx) {
    const int cv = (C + V - 1) / V;
    const int64_t total = (int64_t)rows * cv;
    const float inv_n = training ? 1.f / live_rows[0] : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * MB_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * MB_THREADS) {
        const int r = (int)(i / cv), c = (int)(i - (int64_t)r * cv) * V;
        float v[V] = {}, g[V] = {}, o[V];
        const bool alive = live[r] != 0.f;
        if (alive) { load_vec<V>(v, x + (int64_t)r * ldx + c); load_vec<V>(g, gy + (int64_t)r * ldg + c); }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            if (alive) {
                const float rstd = stats[C + c + k], xhat = (v[k] - stats[c + k]) * rstd;
                float gk = g[k];
                if (RELU) gk = mb_affine(v[k], stats[c + k], rstd, gamma ? gamma[c + k] : 1.f, beta ? beta[c + k] : 0.f) > 0.f ? gk : 0.f;
                const float t = training ? gk - dbeta[c + k] * inv_n - xhat * (dgamma[c + k] * inv_n) : gk;
                o[k] = (gamma ? gamma[c + k] : 1.f) * rstd * t;
            } else o[k] = 0.f;
        }
        store_vec<V>(dx + (int64_t)r * lddx + c, o);
    }
}

static inline int mb_chunks(int32_t rows) { return rows > 0 ? (rows + MB_CHUNK - 1) / MB_CHUNK : 0; }

static inline int mb_stream_blocks(int64_t total) {
    const int64_t b = (total + MB_THREADS - 1) / MB_THREADS;
    return (int)(b < 2048 ? (b > 0 ? b : 1) : 2048);
}

static inline bool mb_vec4(int32_t C, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> lds) {
    if (C % 4) return false;
    for (const void* p : ptrs) if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    for (int64_t ld : lds) if (ld % 4) return false;
    return true;
}

}  // namespace wsi

using namespace wsi;

extern "C" int32_t wsi_masked_bn_chunks(int32_t rows) { return mb_chunks(rows); }

template <bool RELU>
static int masked_bn_fwd(const char* who, const float* x, int64_t ldx, int32_t rows, int32_t C, const float* live, const float* live_rows,
                         const float* gamma, const float* beta, float* running_mean, float* running_var, int32_t training, float momentum,
                         float eps, float* partial, float* stats, float* y, int64_t ldy, void* stream) {
    if (rows < 0 || C <= 0 || ldx < C || ldy < C || !(eps >= 0.f)) { set_error("%s: bad argument", who); return WSI_EINVAL; }
    if (rows == 0) return WSI_OK;
    if (!x || !live || !stats || !y || (training && (!live_rows || !partial)) || (!training && (!running_mean || !running_var))) {
        set_error("%s: null pointer", who); return WSI_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    if (training) {
        const int chunks = mb_chunks(rows);
        hipLaunchKernelGGL(masked_bn_moments_kernel, dim3(chunks, (C + 63) / 64), dim3(MB_THREADS), 0, st, x, ldx, (int)rows, (int)C, live, partial);
        hipLaunchKernelGGL(masked_bn_finish_kernel, dim3(C), dim3(64), 0, st, (const float*)partial, chunks, (int)C, live_rows, momentum, eps,
                           running_mean, running_var, stats);
    } else {
        hipLaunchKernelGGL(masked_bn_eval_stats_kernel, dim3((C + 63) / 64), dim3(64), 0, st, (const float*)running_mean, (const float*)running_var,
                           (int)C, eps, stats);
    }
    if (mb_vec4(C, {x, y}, {ldx, ldy}))
        hipLaunchKernelGGL((masked_bn_apply_kernel<4, RELU>), dim3(mb_stream_blocks((int64_t)rows * (C / 4))), dim3(MB_THREADS), 0, st, x, ldx,
                           (int)rows, (int)C, live, gamma, beta, (const float*)stats, y, ldy);
    else
        hipLaunchKernelGGL((masked_bn_apply_kernel<1, RELU>), dim3(mb_stream_blocks((int64_t)rows * C)), dim3(MB_THREADS), 0, st, x, ldx,
                           (int)rows, (int)C, live, gamma, beta, (const float*)stats, y, ldy);
    return check_launch(who);
}

template <bool RELU>
static int masked_bn_bwd(const char* who, const float* gy, int64_t ldg, const float* x, int64_t ldx, int32_t rows, int32_t C, const float* live,
                         const float* live_rows, const float* gamma, const float* beta, const float* stats, int32_t training, float* partial,
                         float* dgamma, float* dbeta, float* dx, int64_t lddx, void* stream) {
    if (rows < 0 || C <= 0 || ldg < C || ldx < C || lddx < C) { set_error("%s: bad argument", who); return WSI_EINVAL; }
    if (!dgamma || !dbeta) { set_error("%s: null pointer", who); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    const int chunks = mb_chunks(rows);
    if (rows > 0 && (!gy || !x || !live || !stats || !partial || !dx || (training && !live_rows))) {
        set_error("%s: null pointer", who); return WSI_EINVAL;
    }
    if (rows > 0)
        hipLaunchKernelGGL(masked_bn_grad_sums_kernel<RELU>, dim3(chunks, (C + 63) / 64), dim3(MB_THREADS), 0, st, gy, ldg, x, ldx, (int)rows, (int)C,
                           live, gamma, beta, stats, partial);
    hipLaunchKernelGGL(masked_bn_grad_finish_kernel, dim3(C), dim3(64), 0, st, (const float*)partial, chunks, (int)C, dgamma, dbeta);
    if (rows > 0) {
        if (mb_vec4(C, {gy, x, dx}, {ldg, ldx, lddx}))
            hipLaunchKernelGGL((masked_bn_dx_kernel<4, RELU>), dim3(mb_stream_blocks((int64_t)rows * (C / 4))), dim3(MB_THREADS), 0, st, gy, ldg, x,
                               ldx, (int)rows, (int)C, live, live_rows, gamma, beta, stats, (const float*)dgamma, (const float*)dbeta, training != 0,
                               dx, lddx);
        else
            hipLaunchKernelGGL((masked_bn_dx_kernel<1, RELU>), dim3(mb_stream_blocks((int64_t)rows * C)), dim3(MB_THREADS), 0, st, gy, ldg, x, ldx,
                               (int)rows, (int)C, live, live_rows, gamma, beta, stats, (const float*)dgamma, (const float*)dbeta, training != 0,
                               dx, lddx);
    }
    return check_launch(who);
}

extern "C" int wsi_masked_bn_fwd(const float* x, int64_t ldx, int32_t rows, int32_t C, const float* live, const float* live_rows,
                                 const float* gamma, const float* beta, float* running_mean, float* running_var, int32_t training,
                                 float momentum, float eps, float* partial, float* stats, float* y, int64_t ldy, void* stream) {
    return masked_bn_fwd<false>("masked_bn_fwd", x, ldx, rows, C, live, live_rows, gamma, beta, running_mean, running_var, training, momentum, eps,
                                partial, stats, y, ldy, stream);
}

extern "C" int wsi_masked_bn_bwd(const float* gy, int64_t ldg, const float* x, int64_t ldx, int32_t rows, int32_t C, const float* live,
                                 const float* live_rows, const float* gamma, const float* stats, int32_t training, float* partial,
                                 float* dgamma, float* dbeta, float* dx, int64_t lddx, void* stream) {
    return masked_bn_bwd<false>("masked_bn_bwd", gy, ldg, x, ldx, rows, C, live, live_rows, gamma, nullptr, stats, training, partial, dgamma, dbeta,
                                dx, lddx, stream);
}

extern "C" int wsi_masked_bn_relu_fwd(const float* x, int64_t ldx, int32_t rows, int32_t C, const float* live, const float* live_rows,
                                      const float* gamma, const float* beta, float* running_mean, float* running_var, int32_t training,
                                      float momentum, float eps, float* partial, float* stats, float* y, int64_t ldy, void* stream) {
    return masked_bn_fwd<true>("masked_bn_relu_fwd", x, ldx, rows, C, live, live_rows, gamma, beta, running_mean, running_var, training, momentum,
                               eps, partial, stats, y, ldy, stream);
}

extern "C" int wsi_masked_bn_relu_bwd(const float* gy, int64_t ldg, const float* x, int64_t ldx, int32_t rows, int32_t C, const float* live,
                                      const float* live_rows, const float* gamma, const float* beta, const float* stats, int32_t training,
                                      float* partial, float* dgamma, float* dbeta, float* dx, int64_t lddx, void* stream) {
    return masked_bn_bwd<true>("masked_bn_relu_bwd", gy, ldg, x, ldx, rows, C, live, live_rows, gamma, beta, stats, training, partial, dgamma,
                               dbeta, dx, lddx, stream);
}
