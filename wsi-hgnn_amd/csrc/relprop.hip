// Relevance propagation for GraphCAM of GTNMIL on gfx950: the rules of baselines/GTNMIL/models/layers.py at alpha = 1 (Linear, Clone + Add, and
// the attention rule of models/ViT.py:217-240 with the block's layer map), for G slides and C classes per launch.  Contract: include/wsi_hgnn.h.
//
// The reference applies each rule to one slide and one class by re-running the layer under torch.autograd.grad; here a rule is one launch over
// [G, C, n, width].  Everything is fp32 and every sum has one order (no atomics): the same bits run after run.
//   lrp_linear    : workgroup = LL_TM token rows.  W is staged once in LDS (rows padded by one float: the lanes walk it by row in the first phase,
//                   by column in the second, both without bank conflicts) and read as W+ or W- by the sign of the x it meets.  Phase A forms
//                   Z = X+ W+^T + X- W-^T per token - shared by all classes -, phase B S = sd(R, Z) and x * (S W+-) per (token, class).  A W that does
//                   not fit is walked in row tiles (re-staged per pass of phase B: the shapes of the model all fit in one tile).
//   lrp_residual  : workgroup = one (slide, class); pass 1 forms the three whole-tensor sums (lane-strided partial sums, a wave butterfly, the
//                   waves in order), pass 2 recomputes the elements and scales them.
//   lrp_attention : workgroup = one (slide, class, head), the layout of seq_attn.hip: q, k, v, the head's relevance, g_out and S2 in LDS, four
//                   lanes per query row (second phase: per key row) meeting through two DPP steps.  The heads' terms of the layer map go to a
//                   scratch table and lrp_head_mean adds them in order - G * C * H workgroups instead of G * C walking the heads, on launches
//                   that are bound by the latency of one workgroup's dependent LDS reads, not by memory or arithmetic.
#include "common.h"
#include <math.h>

namespace wsi {

__device__ __forceinline__ float lrp_sd(float a, float b) {
    float den = b + 1e-9f;
    if (den == 0.f) den = 1e-9f;
    return b != 0.f ? a / den : 0.f;
}

// ------------------------------------------------------------------------------------------------ linear
constexpr int LL_THREADS = 256;
constexpr int LL_TM = 4;               // token rows per workgroup
constexpr int LL_PP = 3;               // (token, class) pairs per thread and pass of phase B
constexpr int LL_MAX_WIDTH = 256;
constexpr int LL_LDS_FLOATS = 16384;   // 64 KB

// tile rows [o0, o0 + to) of W [fout, fin] -> Ws with row stride fin + 1
__device__ __forceinline__ void ll_stage_w(float* __restrict__ Ws, const float* __restrict__ W, int o0, int to, int fin) {
    for (int idx = threadIdx.x; idx < to * fin; idx += LL_THREADS) {
        const int o = idx / fin, k = idx - o * fin;
        Ws[o * (fin + 1) + k] = W[(int64_t)(o0 + o) * fin + k];
    }
}

__global__ __launch_bounds__(LL_THREADS) void lrp_linear_kernel(const float* __restrict__ X, const float* __restrict__ W, const float* __restrict__ R,
                                                                int64_t rows, int32_t n, int32_t C, int32_t fin, int32_t fout, int32_t TO,
                                                                int32_t KS, int32_t NG, float* __restrict__ out) {
    extern __shared__ float smem[];
    float* __restrict__ Ws = smem;                            // [TO, fin + 1]
    float* __restrict__ Xs = Ws + TO * (fin + 1);             // [LL_TM, fin]
    float* __restrict__ Zs = Xs + LL_TM * fin;                // [LL_TM, fout]
    float* __restrict__ Ss = Zs + LL_TM * fout;               // [NG * LL_PP, fout]
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * LL_TM;
    for (int idx = tid; idx < LL_TM * fin; idx += LL_THREADS) {
        const int64_t r = row0 + idx / fin;
        Xs[idx] = r < rows ? X[r * fin + idx % fin] : 0.f;
    }
    const int ntiles = (fout + TO - 1) / TO;
    // ---- phase A: Z[t, o] = sum_k x (x >= 0 ? w+ : w-), lane = output column
    for (int o0 = 0; o0 < fout; o0 += TO) {
        const int to = min(TO, fout - o0);
        if (o0) __syncthreads();
        ll_stage_w(Ws, W, o0, to, fin);
        __syncthreads();
        for (int o = tid; o < to; o += LL_THREADS) {
            float z[LL_TM];
#pragma unroll
            for (int t = 0; t < LL_TM; ++t) z[t] = 0.f;
            const float* __restrict__ w = Ws + o * (fin + 1);
            for (int k = 0; k < fin; ++k) {
                const float wp = fmaxf(w[k], 0.f), wn = fminf(w[k], 0.f);
#pragma unroll
                for (int t = 0; t < LL_TM; ++t) {
                    const float x = Xs[t * fin + k];
                    z[t] = fmaf(x, x >= 0.f ? wp : wn, z[t]);
                }
            }
#pragma unroll
            for (int t = 0; t < LL_TM; ++t) Zs[t * fout + o0 + o] = z[t];
        }
    }
    __syncthreads();
    // ---- phase B: lane = input column k, thread group gidx takes the pairs (token, class) pj = j * NG + gidx of every pass
    const int k = tid % KS, gidx = tid / KS;
    const bool worker = gidx < NG && k < fin;
    const int npairs = LL_TM * C, CH = NG * LL_PP;
    for (int p0 = 0; p0 < npairs; p0 += CH) {
        for (int idx = tid; idx < CH * fout; idx += LL_THREADS) {
            const int pj = idx / fout, o = idx - pj * fout, p = p0 + pj;
            float s = 0.f;
            if (p < npairs) {
                const int t = p / C, c = p - t * C;
                const int64_t r = row0 + t;
                if (r < rows) {
                    const int64_t g = r / n, i = r - g * n;
                    s = lrp_sd(R[(((g * C + c) * n) + i) * fout + o], Zs[t * fout + o]);
                }
            }
            Ss[idx] = s;
        }
        __syncthreads();
        float acc[LL_PP], xj[LL_PP];
#pragma unroll
        for (int j = 0; j < LL_PP; ++j) {
            const int p = p0 + j * NG + gidx;
            acc[j] = 0.f;
            xj[j] = (worker && p < npairs) ? Xs[(p / C) * fin + k] : 0.f;
        }
        for (int o0 = 0; o0 < fout; o0 += TO) {
            const int to = min(TO, fout - o0);
            if (ntiles > 1) {                                  // (one tile: W is still staged from phase A)
                __syncthreads();
                ll_stage_w(Ws, W, o0, to, fin);
                __syncthreads();
            }
            if (worker) {
                for (int o = 0; o < to; ++o) {
                    const float w = Ws[o * (fin + 1) + k];
                    const float wp = fmaxf(w, 0.f), wn = fminf(w, 0.f);
#pragma unroll
                    for (int j = 0; j < LL_PP; ++j) acc[j] = fmaf(Ss[(j * NG + gidx) * fout + o0 + o], xj[j] >= 0.f ? wp : wn, acc[j]);
                }
            }
        }
        if (worker) {
#pragma unroll
            for (int j = 0; j < LL_PP; ++j) {
                const int p = p0 + j * NG + gidx;
                if (p >= npairs) continue;
                const int t = p / C, c = p - t * C;
                const int64_t r = row0 + t;
                if (r >= rows) continue;
                const int64_t g = r / n, i = r - g * n;
                out[(((g * C + c) * n) + i) * fin + k] = xj[j] * acc[j];
            }
        }
        __syncthreads();                                       // Ss is rewritten by the next pass
    }
}

// ------------------------------------------------------------------------------------------------ clone + add
constexpr int LR_THREADS = 512;
constexpr int LR_WAVES = LR_THREADS / 64;

__device__ __forceinline__ float lr_rel(float x, float r1, float r2, bool two) { return two ? x * (lrp_sd(r1, x) + lrp_sd(r2, x)) : r1; }

__device__ __forceinline__ float4 lr_rel4(const float4* __restrict__ X4, const float4* __restrict__ r14, const float4* __restrict__ r24, int e) {
    const float4 r1 = r14[e];
    if (!r24) return r1;
    const float4 x = X4[e], r2 = r24[e];
    return make_float4(lr_rel(x.x, r1.x, r2.x, true), lr_rel(x.y, r1.y, r2.y, true), lr_rel(x.z, r1.z, r2.z, true), lr_rel(x.w, r1.w, r2.w, true));
}

__global__ __launch_bounds__(LR_THREADS) void lrp_residual_kernel(const float* __restrict__ X, const float* __restrict__ r1, const float* __restrict__ r2,
                                                                  const float* __restrict__ A, const float* __restrict__ B, int32_t C, int32_t ne4,
                                                                  float* __restrict__ out_a, float* __restrict__ out_b) {
    const int64_t gc = blockIdx.x, g = gc / C;
    const float4* __restrict__ A4 = reinterpret_cast<const float4*>(A) + g * ne4;
    const float4* __restrict__ B4 = reinterpret_cast<const float4*>(B) + g * ne4;
    const float4* __restrict__ X4 = r2 ? reinterpret_cast<const float4*>(X) + g * ne4 : nullptr;
    const float4* __restrict__ r14 = reinterpret_cast<const float4*>(r1) + gc * ne4;
    const float4* __restrict__ r24 = r2 ? reinterpret_cast<const float4*>(r2) + gc * ne4 : nullptr;
    float4* __restrict__ oa = reinterpret_cast<float4*>(out_a) + gc * ne4;
    float4* __restrict__ ob = reinterpret_cast<float4*>(out_b) + gc * ne4;
    __shared__ float part[3][LR_WAVES];
    float sa = 0.f, sb = 0.f, sr = 0.f;
    for (int e = threadIdx.x; e < ne4; e += LR_THREADS) {
        const float4 a = A4[e], b = B4[e], r = lr_rel4(X4, r14, r24, e);
        const float s0 = lrp_sd(r.x, a.x + b.x), s1 = lrp_sd(r.y, a.y + b.y), s2 = lrp_sd(r.z, a.z + b.z), s3 = lrp_sd(r.w, a.w + b.w);
        sa += (a.x * s0 + a.y * s1) + (a.z * s2 + a.w * s3);
        sb += (b.x * s0 + b.y * s1) + (b.z * s2 + b.w * s3);
        sr += (r.x + r.y) + (r.z + r.w);
    }
    sa = wave_sum(sa); sb = wave_sum(sb); sr = wave_sum(sr);
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = sa; part[1][threadIdx.x >> 6] = sb; part[2][threadIdx.x >> 6] = sr;
    }
    __syncthreads();
    sa = sb = sr = 0.f;
#pragma unroll
    for (int w = 0; w < LR_WAVES; ++w) { sa += part[0][w]; sb += part[1][w]; sr += part[2][w]; }
    const float both = fabsf(sa) + fabsf(sb);
    const float fa = lrp_sd(lrp_sd(fabsf(sa), both) * sr, sa), fb = lrp_sd(lrp_sd(fabsf(sb), both) * sr, sb);
    for (int e = threadIdx.x; e < ne4; e += LR_THREADS) {
        const float4 a = A4[e], b = B4[e], r = lr_rel4(X4, r14, r24, e);
        const float s0 = lrp_sd(r.x, a.x + b.x), s1 = lrp_sd(r.y, a.y + b.y), s2 = lrp_sd(r.z, a.z + b.z), s3 = lrp_sd(r.w, a.w + b.w);
        oa[e] = make_float4(a.x * s0 * fa, a.y * s1 * fa, a.z * s2 * fa, a.w * s3 * fa);
        ob[e] = make_float4(b.x * s0 * fb, b.y * s1 * fb, b.z * s2 * fb, b.w * s3 * fb);
    }
}

// ------------------------------------------------------------------------------------------------ attention
constexpr int LA_MAX_N = 128;
constexpr int LA_THREADS = 4 * LA_MAX_N;

// dst: the heads' terms [G * C * H, n, n] (H > 1) or M itself (H = 1)
template <int D>
__global__ __launch_bounds__(LA_THREADS) void lrp_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ lse, const float* __restrict__ R,
                                                                   const float* __restrict__ g_out, int32_t C, int32_t n, int32_t H, float scale,
                                                                   float* __restrict__ dst, float* __restrict__ cam) {
    const int64_t blk = blockIdx.x, gc = blk / H, g = gc / C;
    const int h = (int)(blk - gc * H);
    const int64_t ld = 3 * (int64_t)H * D, lr = (int64_t)H * D;
    const float* __restrict__ base = qkv + g * n * ld + h * D;
    float* __restrict__ cbase = cam + gc * n * ld + h * D;
    __shared__ __attribute__((aligned(16))) float sq[LA_MAX_N * D], sk[LA_MAX_N * D], sv[LA_MAX_N * D], sr[LA_MAX_N * D], sg[LA_MAX_N * D],
        ss2[LA_MAX_N * D];
    __shared__ float sl[LA_MAX_N];
    stage_rows<D, LA_THREADS>(sq, base, ld, n);
    stage_rows<D, LA_THREADS>(sk, base + lr, ld, n);
    stage_rows<D, LA_THREADS>(sv, base + 2 * lr, ld, n);
    stage_rows<D, LA_THREADS>(sr, R + gc * n * lr + h * D, lr, n);
    if (g_out) stage_rows<D, LA_THREADS>(sg, g_out + gc * n * lr + h * D, lr, n);
    if ((int)threadIdx.x < n) sl[threadIdx.x] = lse[(g * H + h) * n + threadIdx.x];
    __syncthreads();
    const int i = threadIdx.x >> 2, part = threadIdx.x & 3;
    const bool live = i < n;
    // ---- this quad's query row i: S2_i, then the row of cam_attn, the layer map's term and cam_q
    if (live) {
        float q[D], s2[D], gi[D], acc[D];
#pragma unroll
        for (int c = 0; c < D; ++c) { q[c] = sq[i * D + c]; acc[c] = 0.f; gi[c] = g_out ? sg[i * D + c] : 0.f; }
        const float li = sl[i];
        for (int j = part; j < n; j += 4) {
            const float p = expf(dot4<D>(q, sk + j * D) * scale - li);
#pragma unroll
            for (int c = 0; c < D; ++c) acc[c] = fmaf(p, sv[j * D + c], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < D; ++c) {
            s2[c] = lrp_sd(sr[i * D + c], group_sum<4>(acc[c]));            // Z2 = P v: every lane of the quad has the whole row
            if (c / (D / 4) == part) ss2[i * D + c] = s2[c];
            acc[c] = 0.f;
        }
        float* __restrict__ m = dst + (blk * n + i) * n;
        for (int j = part; j < n; j += 4) {
            const float z1 = dot4<D>(q, sk + j * D);
            const float ca = expf(z1 * scale - li) * dot4<D>(s2, sv + j * D) * 0.5f;
            const float s1 = lrp_sd(ca, z1);
#pragma unroll
            for (int c = 0; c < D; ++c) acc[c] = fmaf(s1, sk[j * D + c], acc[c]);
            m[j] = fmaxf(g_out ? dot4<D>(gi, sv + j * D) * ca : ca, 0.f);
        }
        float* __restrict__ o = cbase + (int64_t)i * ld;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const float tot = group_sum<4>(acc[c]);
            if (c / (D / 4) == part) o[c] = q[c] * tot * 0.5f;
        }
    }
    __syncthreads();
    // ---- this quad's key row j = i: cam_k and cam_v
    if (!live) return;
    float kj[D], vj[D], ak[D], av[D];
#pragma unroll
    for (int c = 0; c < D; ++c) { kj[c] = sk[i * D + c]; vj[c] = sv[i * D + c]; ak[c] = 0.f; av[c] = 0.f; }
    for (int r = part; r < n; r += 4) {
        const float z1 = dot4<D>(kj, sq + r * D);
        const float p = expf(z1 * scale - sl[r]);
        const float s1 = lrp_sd(p * dot4<D>(vj, ss2 + r * D) * 0.5f, z1);
#pragma unroll
        for (int c = 0; c < D; ++c) { ak[c] = fmaf(s1, sq[r * D + c], ak[c]); av[c] = fmaf(p, ss2[r * D + c], av[c]); }
    }
    float* __restrict__ ok = cbase + (int64_t)i * ld + lr;
    float* __restrict__ ov = cbase + (int64_t)i * ld + 2 * lr;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const float tk = group_sum<4>(ak[c]), tv = group_sum<4>(av[c]);
        if (c / (D / 4) == part) { ok[c] = kj[c] * tk * 0.5f; ov[c] = vj[c] * tv * 0.5f; }
    }
}

// M[gc, e] = (sum_h partial[gc, h, e]) / H, the heads in order
__global__ __launch_bounds__(256) void lrp_head_mean(const float* __restrict__ partial, int64_t total, int64_t nn, int32_t H, float* __restrict__ M) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t gc = e / nn, r = e - gc * nn;
    const float* __restrict__ p = partial + gc * H * nn + r;
    float acc = 0.f;
    for (int h = 0; h < H; ++h) acc += p[(int64_t)h * nn];
    M[e] = acc / (float)H;
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_lrp_linear(const float* X, const float* W, const float* R, int32_t G, int32_t C, int32_t n, int32_t fan_in, int32_t fan_out,
                              float* out_rel, void* stream) {
    if (G < 0 || C < 0 || n < 0 || fan_in <= 0 || fan_out <= 0) { set_error("lrp_linear: bad argument"); return WSI_EINVAL; }
    if (fan_in % 4 || fan_in > LL_MAX_WIDTH || fan_out > LL_MAX_WIDTH) {
        set_error("lrp_linear: widths %d -> %d (compiled: an input width that is a multiple of 4, both widths <= %d)", (int)fan_in, (int)fan_out,
                  LL_MAX_WIDTH);
        return WSI_ENOSYS;
    }
    if (G == 0 || C == 0 || n == 0) return WSI_OK;
    if (!X || !W || !R || !out_rel) { set_error("lrp_linear: null pointer"); return WSI_EINVAL; }
    int KS = 4;
    while (KS < fan_in) KS *= 2;
    const int NG = LL_THREADS / KS < 4 ? LL_THREADS / KS : 4;
    const int fixed = LL_TM * fan_in + LL_TM * fan_out + NG * LL_PP * fan_out;
    int TO = (LL_LDS_FLOATS - fixed) / (fan_in + 1);
    if (TO > fan_out) TO = fan_out;
    const size_t lds = sizeof(float) * ((size_t)TO * (fan_in + 1) + fixed);
    const int64_t rows = (int64_t)G * n;
    hipLaunchKernelGGL(lrp_linear_kernel, dim3((unsigned)((rows + LL_TM - 1) / LL_TM)), dim3(LL_THREADS), lds, (hipStream_t)stream, X, W, R, rows, n, C,
                       fan_in, fan_out, TO, KS, NG, out_rel);
    return check_launch("lrp_linear");
}

extern "C" int wsi_lrp_residual(const float* X, const float* r1, const float* r2, const float* A, const float* B, int32_t G, int32_t C, int32_t n,
                                int32_t E, float* out_a, float* out_b, void* stream) {
    if (G < 0 || C < 0 || n < 0 || E <= 0 || (int64_t)n * E >= INT32_MAX) { set_error("lrp_residual: bad argument"); return WSI_EINVAL; }
    if (E % 4) { set_error("lrp_residual: width %d (compiled: a multiple of 4)", (int)E); return WSI_ENOSYS; }
    if (G == 0 || C == 0 || n == 0) return WSI_OK;
    if (!r1 || !A || !B || !out_a || !out_b || (r2 && !X)) { set_error("lrp_residual: null pointer"); return WSI_EINVAL; }
    if (!aligned16(r1) || !aligned16(A) || !aligned16(B) || !aligned16(out_a) || !aligned16(out_b) || (r2 && (!aligned16(r2) || !aligned16(X)))) {
        set_error("lrp_residual: every tensor must be 16-byte aligned");
        return WSI_EINVAL;
    }
    hipLaunchKernelGGL(lrp_residual_kernel, dim3((unsigned)(G * C)), dim3(LR_THREADS), 0, (hipStream_t)stream, X, r1, r2, A, B, C, n * E / 4, out_a, out_b);
    return check_launch("lrp_residual");
}

extern "C" int wsi_lrp_attention(const float* qkv, const float* lse, const float* R, const float* g_out, int32_t G, int32_t C, int32_t n, int32_t H,
                                 int32_t d, float scale, float* partial, float* cam_qkv, float* M, void* stream) {
    if (G < 0 || C < 0 || n < 0 || H <= 0 || d <= 0) { set_error("lrp_attention: bad argument"); return WSI_EINVAL; }
    if (n > LA_MAX_N || (d != 8 && d != 16)) {
        set_error("lrp_attention: n = %d, head width %d (compiled: n <= %d, head width 8 or 16)", (int)n, (int)d, LA_MAX_N);
        return WSI_ENOSYS;
    }
    if (G == 0 || C == 0 || n == 0) return WSI_OK;
    if (!qkv || !lse || !R || !cam_qkv || !M || (H > 1 && !partial)) { set_error("lrp_attention: null pointer"); return WSI_EINVAL; }
    if (!aligned16(qkv) || !aligned16(R) || (g_out && !aligned16(g_out))) {
        set_error("lrp_attention: qkv, R and g_out must be 16-byte aligned");
        return WSI_EINVAL;
    }
    if ((int64_t)G * C * H > INT32_MAX) { set_error("lrp_attention: too many (slide, class, head) triples"); return WSI_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    float* dst = H > 1 ? partial : M;
    const dim3 grid((unsigned)(G * C * H));
    if (d == 8) hipLaunchKernelGGL(lrp_attention_kernel<8>, grid, dim3(LA_THREADS), 0, st, qkv, lse, R, g_out, C, n, H, scale, dst, cam_qkv);
    else hipLaunchKernelGGL(lrp_attention_kernel<16>, grid, dim3(LA_THREADS), 0, st, qkv, lse, R, g_out, C, n, H, scale, dst, cam_qkv);
    if (int rc = check_launch("lrp_attention")) return rc;
    if (H > 1) {
        const int64_t nn = (int64_t)n * n, total = (int64_t)G * C * nn;
        hipLaunchKernelGGL(lrp_head_mean, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, partial, total, nn, H, M);
        return check_launch("lrp_head_mean");
    }
    return WSI_OK;
}
