// Epoch metrics of the multi-label MIL baselines kept on the device (wsi_hgnn_amd/mil/metrics.py::BagEpochMetrics).  Contract: include/wsi_hgnn.h.
//
// wsi_bag_metrics_update appends one batch's counted bags to the accumulator in ONE launch that a hipGraph can record: nothing is allocated,
// nothing read back.  wsi_bag_metrics_finalize turns the accumulated rows into the integers behind the reference's test() (train_tcga_k-fold.py:
// 136-154, train_remix_k-fold.py:189-207): per class the ROC-optimal threshold of multi_label_roc / optimal_thresh with the counts at it and the
// pair counts of the AUC, then the hard predictions' exact-match count and the confusion matrix of the decoded labels - two launches.  Every
// count is an integer, every float sum has one order and no float is added atomically: the buffers hold the same bits run after run.
#include "common.h"
#include <math.h>

namespace wsi {

constexpr int BM_TILE = 256;                                   // segments per step of the update, threads of the row pass
constexpr int BM_ROWS = WSI_BAG_METRICS_MAX_ROWS;              // rows one workgroup sorts in LDS
constexpr int BM_THREADS = 1024;                               // threads of the per-class workgroup
constexpr int BM_PER = BM_ROWS / BM_THREADS;                   // contiguous rows per thread in its scans
static_assert(BM_PER == 4 && BM_ROWS <= 65536, "the scans read an int4 per thread; a point packs (row << 16) | tps");

// BCEWithLogits of one row, the mean over its C classes (the stable form, in fp64: a step holds a handful of bags, and the epoch's sum then
// carries no rounding of its terms worth the name)
__device__ __forceinline__ double bce_row(const float* __restrict__ x, const float* __restrict__ t, int C) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) {
        const double v = (double)x[c];
        s += fmax(v, 0.0) - v * (double)t[c] + log1p(exp(-fabs(v)));
    }
    return s / (double)C;
}

// One workgroup walks the segments 256 at a time; a segment's place behind the cursor is its rank among the counted ones in front of it (one LDS
// scan per step), so the stored order is the segment order.  The losses of a step are summed by a fixed tree in fp64, the steps in order.
__global__ __launch_bounds__(BM_TILE) void bag_metrics_update_kernel(const float* __restrict__ bag_pred, const float* __restrict__ max_pred,
                                                                     const float* __restrict__ targets, const float* __restrict__ weights, int S,
                                                                     int C, int32_t* __restrict__ state, float* __restrict__ scores,
                                                                     float* __restrict__ row_targets, int capacity) {
    __shared__ int scan[BM_TILE];
    __shared__ double ls[BM_TILE];
    __shared__ int flag_bits;
    const int tid = threadIdx.x;
    int cursor = state[0];
    cursor = cursor < 0 ? 0 : (cursor > capacity ? capacity : cursor);
    if (tid == 0) flag_bits = 0;
    double loss = 0.0;                               // thread 0's running sum
    int seen = 0;                                    // counted segments so far, dropped ones included (uniform)
    __syncthreads();
    for (int base = 0; base < S; base += BM_TILE) {
        const int s = base + tid;
        bool counted = false;
        const float* x = bag_pred + (int64_t)s * C;
        const float* m = max_pred ? max_pred + (int64_t)s * C : nullptr;
        const float* t = targets + (int64_t)s * C;
        if (s < S && weights[s] > 0.f) {             // (a padding segment's rows are never looked at)
            bool finite = true, good = true;
            for (int c = 0; c < C; ++c) {
                finite = finite && isfinite(x[c]) && (!m || isfinite(m[c]));
                good = good && (t[c] == 0.f || t[c] == 1.f);
            }
            if (!finite) atomicOr(&flag_bits, WSI_BAG_METRICS_NONFINITE);
            if (!good) atomicOr(&flag_bits, WSI_BAG_METRICS_BAD_TARGET);
            counted = finite && good;
        }
        scan[tid] = counted ? 1 : 0;
        __syncthreads();
        for (int o = 1; o < BM_TILE; o <<= 1) {                      // inclusive scan
            const int v = tid >= o ? scan[tid - o] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int total = scan[BM_TILE - 1];
        double mine = 0.0;
        if (counted) {
            const int64_t pos = (int64_t)cursor + seen + scan[tid] - 1;
            if (pos >= capacity) {
                atomicOr(&flag_bits, WSI_BAG_METRICS_OVERFLOW);      // dropped: nothing is written at or past the capacity
            } else {
                for (int c = 0; c < C; ++c) {
                    scores[pos * C + c] = 1.f / (1.f + expf(-x[c]));
                    row_targets[pos * C + c] = t[c];
                }
                const double lb = bce_row(x, t, C);
                mine = m ? 0.5 * lb + 0.5 * bce_row(m, t, C) : lb;
            }
        }
        ls[tid] = mine;
        __syncthreads();
        for (int o = BM_TILE / 2; o > 0; o >>= 1) {
            if (tid < o) ls[tid] += ls[tid + o];
            __syncthreads();
        }
        if (tid == 0) loss += ls[0];
        seen += total;
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t end = (int64_t)cursor + seen;
        state[0] = (int32_t)(end > capacity ? capacity : end);
        if (flag_bits) state[1] |= flag_bits;
        if (seen) *reinterpret_cast<double*>(state + 2) += loss;
    }
}

// In-place inclusive scan of arr[0 .. BM_ROWS): every thread its BM_PER contiguous entries, then the threads' totals (Hillis-Steele over `part`).
__device__ __forceinline__ void block_scan(int* arr, int* part, int tid) {
    int4 v = reinterpret_cast<int4*>(arr)[tid];
    v.y += v.x; v.z += v.y; v.w += v.z;
    part[tid] = v.w;
    __syncthreads();
    for (int o = 1; o < BM_THREADS; o <<= 1) {
        const int a = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += a;
        __syncthreads();
    }
    const int off = tid ? part[tid - 1] : 0;
    v.x += off; v.y += off; v.z += off; v.w += off;
    reinterpret_cast<int4*>(arr)[tid] = v;
    __syncthreads();
}

__device__ __forceinline__ int64_t double_bits(double x) { return __double_as_longlong(x); }

// Workgroup c: the ROC optimum and the pair counts of class c (the rule is in include/wsi_hgnn.h).  key = (score bits << 1) | label bit, sorted
// descending by a bitonic network over the next power of two (the padding keys are 0 and sort behind every real key or equal one: the first n
// entries are the rows).  LDS: 3 x 16 KiB of rows + 4 KiB of scan partials.
__global__ __launch_bounds__(BM_THREADS) void bag_metrics_roc_kernel(const int32_t* __restrict__ state, const float* __restrict__ scores,
                                                                     const float* __restrict__ row_targets, int C, int capacity,
                                                                     int64_t* __restrict__ result) {
    __shared__ __attribute__((aligned(16))) uint32_t key[BM_ROWS];
    __shared__ __attribute__((aligned(16))) int tpi[BM_ROWS];            // positives among the sorted rows [0 .. i]
    __shared__ __attribute__((aligned(16))) int pts[BM_ROWS];            // point flags, their scan, then the points (row << 16) | tps
    __shared__ int part[BM_THREADS];
    __shared__ double w_loss[BM_THREADS / 64];
    __shared__ int w_at[BM_THREADS / 64];
    __shared__ long long w_gt[BM_THREADS / 64], w_eq[BM_THREADS / 64];
    const int tid = threadIdx.x, c = blockIdx.x;
    int64_t* out = result + WSI_BAG_METRICS_RESULT_HEAD + 8 * c;
    int n = state[0];
    n = n < 0 ? 0 : (n > capacity ? capacity : n);
    n = n > BM_ROWS ? BM_ROWS : n;
    int npad = 2;
    while (npad < n) npad <<= 1;
    for (int i = tid; i < BM_ROWS; i += BM_THREADS)
        key[i] = i < n ? ((__float_as_uint(scores[(int64_t)i * C + c]) << 1) | (row_targets[(int64_t)i * C + c] != 0.f ? 1u : 0u)) : 0u;
    __syncthreads();
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = tid; idx < (npad >> 1); idx += BM_THREADS) {
                const int i = ((idx & ~(j - 1)) << 1) | (idx & (j - 1)), l = i | j;
                const uint32_t a = key[i], b = key[l];
                if (((i & k) == 0) ? a < b : a > b) { key[i] = b; key[l] = a; }
            }
            __syncthreads();
        }
    for (int i = tid; i < BM_ROWS; i += BM_THREADS) tpi[i] = (int)(key[i] & 1u);
    __syncthreads();
    block_scan(tpi, part, tid);
    const int P = n > 0 ? tpi[n - 1] : 0, Nn = n - P;
    if (P == 0 || Nn == 0) {                                         // (uniform) roc_auc_score raises here: NaN, and the row pass sets the flag
        if (tid == 0) {
            out[0] = double_bits((double)NAN); out[1] = 0; out[2] = 0; out[3] = P; out[4] = Nn; out[5] = 0; out[6] = 0;
            out[7] = double_bits((double)NAN);
        }
        return;
    }
    for (int i = tid; i < BM_ROWS; i += BM_THREADS)                  // the last row of every tie group
        pts[i] = (i < n && (i == n - 1 || (key[i] >> 1) != (key[i + 1] >> 1))) ? 1 : 0;
    __syncthreads();
    block_scan(pts, part, tid);
    const int4 inc = reinterpret_cast<const int4*>(pts)[tid];
    const int before = tid ? pts[tid * BM_PER - 1] : 0;
    const int m = pts[BM_ROWS - 1];                                  // number of points (>= 2: both labels occur)
    __syncthreads();
    {
        const int i = tid * BM_PER;
        if (inc.x != before) pts[inc.x - 1] = (i << 16) | tpi[i];
        if (inc.y != inc.x) pts[inc.y - 1] = ((i + 1) << 16) | tpi[i + 1];
        if (inc.z != inc.y) pts[inc.z - 1] = ((i + 2) << 16) | tpi[i + 2];
        if (inc.w != inc.z) pts[inc.w - 1] = ((i + 3) << 16) | tpi[i + 3];
    }
    __syncthreads();
    double bl = INFINITY;
    int ba = 0x7fffffff;                                             // place in the candidate order: 0 = the prepended (0, 0), k + 1 = point k
    long long gt = 0, eq = 0;
    if (tid == 0) { bl = 0.0; ba = 0; }                              // 0 / N - 0 / P
    for (int k = tid; k < m; k += BM_THREADS) {
        const uint32_t w = (uint32_t)pts[k];
        const int tps = (int)(w & 0xffffu), fps = (int)(w >> 16) + 1 - tps;
        int tp0 = 0, fp0 = 0;
        if (k > 0) {
            const uint32_t w0 = (uint32_t)pts[k - 1];
            tp0 = (int)(w0 & 0xffffu);
            fp0 = (int)(w0 >> 16) + 1 - tp0;
        }
        gt += (long long)(tps - tp0) * (long long)(Nn - fps);        // the group's positives over every negative behind the group
        eq += (long long)(tps - tp0) * (long long)(fps - fp0);
        bool keep = m <= 2 || k == 0 || k == m - 1;
        if (!keep) {
            const uint32_t w1 = (uint32_t)pts[k + 1];
            const int tp1 = (int)(w1 & 0xffffu), fp1 = (int)(w1 >> 16) + 1 - tp1;
            keep = (fp0 - 2 * fps + fp1) != 0 || (tp0 - 2 * tps + tp1) != 0;
        }
        if (keep) {
            const double loss = (double)fps / (double)Nn - (double)tps / (double)P;
            if (loss < bl) { bl = loss; ba = k + 1; }                // (k ascends: a strict '<' keeps the first)
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ol = __shfl_xor(bl, o);
        const int oa = __shfl_xor(ba, o);
        if (ol < bl || (ol == bl && oa < ba)) { bl = ol; ba = oa; }
        gt += __shfl_xor(gt, o);
        eq += __shfl_xor(eq, o);
    }
    if ((tid & 63) == 0) { w_loss[tid >> 6] = bl; w_at[tid >> 6] = ba; w_gt[tid >> 6] = gt; w_eq[tid >> 6] = eq; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < BM_THREADS / 64; ++w) {
            if (w_loss[w] < bl || (w_loss[w] == bl && w_at[w] < ba)) { bl = w_loss[w]; ba = w_at[w]; }
            gt += w_gt[w];
            eq += w_eq[w];
        }
        double thr = (double)INFINITY;
        int tp = 0, fp = 0;
        if (ba > 0) {
            const uint32_t w = (uint32_t)pts[ba - 1];
            tp = (int)(w & 0xffffu);
            fp = (int)(w >> 16) + 1 - tp;
            thr = (double)__uint_as_float(key[w >> 16] >> 1);
        }
        out[0] = double_bits(thr); out[1] = tp; out[2] = fp; out[3] = P; out[4] = Nn; out[5] = gt; out[6] = eq;
        out[7] = double_bits((double)(2 * gt + eq) / (double)(2 * (long long)P * (long long)Nn));
    }
}

// One workgroup: the hard predictions of every row under the thresholds the launch before wrote, the rows equal to their targets, the confusion
// matrix of the decoded labels (integer LDS atomics: a count does not depend on the order of arrival), and the head of the result block.
__global__ __launch_bounds__(BM_TILE) void bag_metrics_rows_kernel(const int32_t* __restrict__ state, const float* __restrict__ scores,
                                                                   const float* __restrict__ row_targets, int C, int capacity, int64_t* result) {
    __shared__ double thr[WSI_BAG_METRICS_MAX_CLASSES];
    __shared__ int conf[WSI_BAG_METRICS_MAX_CLASSES * WSI_BAG_METRICS_MAX_CLASSES];
    __shared__ int exact, one_label;
    const int tid = threadIdx.x, K = C > 1 ? C : 2;
    int n = state[0];
    n = n < 0 ? 0 : (n > capacity ? capacity : n);
    for (int j = tid; j < K * K; j += BM_TILE) conf[j] = 0;
    if (tid == 0) { exact = 0; one_label = 0; }
    __syncthreads();
    if (tid < C) {
        const int64_t* cls = result + WSI_BAG_METRICS_RESULT_HEAD + 8 * tid;
        thr[tid] = __longlong_as_double(cls[0]);
        if (cls[3] == 0 || cls[4] == 0) atomicOr(&one_label, 1);
    }
    __syncthreads();
    for (int i = tid; i < n; i += BM_TILE) {
        bool same = true;
        int yp = -1, yt = -1;
        for (int c = 0; c < C; ++c) {
            const bool p = (double)scores[(int64_t)i * C + c] >= thr[c], t = row_targets[(int64_t)i * C + c] != 0.f;
            same = same && p == t;
            if (p && yp < 0) yp = c;
            if (t && yt < 0) yt = c;
        }
        if (C == 1) { yp = yp < 0 ? 0 : 1; yt = yt < 0 ? 0 : 1; }    // the value itself
        else { yp = yp < 0 ? 0 : yp; yt = yt < 0 ? 0 : yt; }         // argmax: the first 1, an all-zero row decodes to 0
        atomicAdd(&conf[yt * K + yp], 1);
        if (same) atomicAdd(&exact, 1);
    }
    __syncthreads();
    for (int j = tid; j < K * K; j += BM_TILE) result[WSI_BAG_METRICS_RESULT_HEAD + 8 * C + j] = conf[j];
    if (tid == 0) {
        result[0] = n;
        result[1] = state[1] | (one_label ? WSI_BAG_METRICS_ONE_LABEL : 0);
        result[2] = reinterpret_cast<const int64_t*>(state)[1];      // the fp64 loss sum, as its bits
        result[3] = exact;
    }
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_bag_metrics_update(const float* bag_pred, const float* max_pred, const float* targets, const float* weights, int32_t S, int32_t C,
                                      int32_t* state, float* scores, float* row_targets, int32_t capacity, void* stream) {
    if (S <= 0 || C <= 0 || C > WSI_BAG_METRICS_MAX_CLASSES || (int64_t)S * C > 65536 || capacity < 0 || capacity > WSI_BAG_METRICS_MAX_ROWS) {
        set_error("bag_metrics_update: unsupported shape (%d segments, %d classes, capacity %d)", S, C, capacity);
        return WSI_ENOSYS;
    }
    if (!bag_pred || !targets || !weights || !state || ((uintptr_t)state & 7) || (capacity > 0 && (!scores || !row_targets))) {
        set_error("bag_metrics_update: null or misaligned pointer");
        return WSI_EINVAL;
    }
    hipLaunchKernelGGL(bag_metrics_update_kernel, dim3(1), dim3(BM_TILE), 0, (hipStream_t)stream, bag_pred, max_pred, targets, weights, (int)S, (int)C,
                       state, scores, row_targets, (int)capacity);
    return check_launch("bag_metrics_update");
}

extern "C" int wsi_bag_metrics_finalize(const int32_t* state, const float* scores, const float* row_targets, int32_t C, int32_t capacity,
                                        int64_t* result, void* stream) {
    if (C <= 0 || C > WSI_BAG_METRICS_MAX_CLASSES || capacity < 0 || capacity > WSI_BAG_METRICS_MAX_ROWS) {
        set_error("bag_metrics_finalize: unsupported shape (%d classes, capacity %d)", C, capacity);
        return WSI_ENOSYS;
    }
    if (!state || ((uintptr_t)state & 7) || !result || ((uintptr_t)result & 7) || (capacity > 0 && (!scores || !row_targets))) {
        set_error("bag_metrics_finalize: null or misaligned pointer");
        return WSI_EINVAL;
    }
    hipLaunchKernelGGL(bag_metrics_roc_kernel, dim3(C), dim3(BM_THREADS), 0, (hipStream_t)stream, state, scores, row_targets, (int)C, (int)capacity,
                       result);
    const int rc = check_launch("bag_metrics_finalize (roc)");
    if (rc != WSI_OK) return rc;
    hipLaunchKernelGGL(bag_metrics_rows_kernel, dim3(1), dim3(BM_TILE), 0, (hipStream_t)stream, state, scores, row_targets, (int)C, (int)capacity,
                       result);
    return check_launch("bag_metrics_finalize");
}
