// Epoch metrics kept on the device (wsi_hgnn_amd/metrics.py::EpochMetrics).  Contract: include/wsi_hgnn.h.
//
// wsi_metrics_update appends one batch's counted rows to the accumulator in ONE launch that a hipGraph can record: nothing is allocated, nothing
// read back.  wsi_metrics_finalize turns the accumulated rows into the reference's numbers (utils.py:37-47: precision / recall / F1 / AUC, plus
// accuracy and mean cross entropy) in two launches.  Every count is an integer and every float sum has one order: the buffers hold the same bits
// run after run.
#include "common.h"
#include <math.h>

namespace wsi {

constexpr int64_t METRICS_IGNORE_INDEX = -100;     // torch's default ignore_index, as csrc/loss.hip
constexpr int METRICS_TILE = 256;                  // rows per step of the update, rows per tile / block of the pair counting

__device__ __forceinline__ double* state_loss(int32_t* state) { return reinterpret_cast<double*>(state + 2); }
__device__ __forceinline__ const double* state_loss(const int32_t* state) { return reinterpret_cast<const double*>(state + 2); }

// One workgroup walks the rows 256 at a time; a row's place behind the cursor is its rank among the counted rows in front of it (one LDS scan per
// step), so the stored order is the row order.  The cross entropies of a step are summed by a fixed tree in fp64, the steps in order.
__global__ __launch_bounds__(METRICS_TILE) void metrics_update_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int B, int C,
                                                                      int32_t* __restrict__ state, float* __restrict__ probs,
                                                                      int64_t* __restrict__ row_labels, int64_t* __restrict__ row_preds, int capacity) {
    __shared__ int scan[METRICS_TILE];
    __shared__ double ce[METRICS_TILE];
    __shared__ int flag_bits;
    const int tid = threadIdx.x;
    int cursor = state[0];
    cursor = cursor < 0 ? 0 : (cursor > capacity ? capacity : cursor);
    int32_t* conf = state + WSI_METRICS_STATE_HEAD;
    if (tid == 0) flag_bits = 0;
    double loss = 0.0;                               // thread 0's running sum
    int seen = 0;                                    // counted rows so far, dropped ones included (uniform)
    __syncthreads();
    for (int base = 0; base < B; base += METRICS_TILE) {
        const int b = base + tid;
        bool counted = false;
        int64_t y = METRICS_IGNORE_INDEX;
        const float* row = logits + (int64_t)b * C;
        if (b < B) {
            y = labels[b];
            if (y != METRICS_IGNORE_INDEX) {         // an ignored row's logits are never looked at
                if (y < 0 || y >= C) {
                    atomicOr(&flag_bits, WSI_METRICS_BAD_LABEL);
                } else {
                    bool finite = true;
                    for (int c = 0; c < C; ++c) finite = finite && isfinite(row[c]);
                    if (finite) counted = true;
                    else atomicOr(&flag_bits, WSI_METRICS_NONFINITE);
                }
            }
        }
        scan[tid] = counted ? 1 : 0;
        __syncthreads();
        for (int o = 1; o < METRICS_TILE; o <<= 1) {                 // inclusive scan
            const int v = tid >= o ? scan[tid - o] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int total = scan[METRICS_TILE - 1];
        double mine = 0.0;
        if (counted) {
            const int64_t pos = (int64_t)cursor + seen + scan[tid] - 1;
            if (pos >= capacity) {
                atomicOr(&flag_bits, WSI_METRICS_OVERFLOW);          // dropped: nothing is written at or past the capacity
            } else {
                float mx = row[0];
                int arg = 0;
                for (int c = 1; c < C; ++c)
                    if (row[c] > mx) { mx = row[c]; arg = c; }       // the FIRST maximum, as numpy.argmax
                float den = 0.f;
                for (int c = 0; c < C; ++c) den += expf(row[c] - mx);
                for (int c = 0; c < C; ++c) probs[pos * C + c] = expf(row[c] - mx) / den;
                row_labels[pos] = y;
                row_preds[pos] = arg;
                atomicAdd(&conf[(int)y * C + arg], 1);               // integer: the sum does not depend on the order of arrival
                mine = (double)((logf(den) + mx) - row[y]);
            }
        }
        ce[tid] = mine;
        __syncthreads();
        for (int o = METRICS_TILE / 2; o > 0; o >>= 1) {
            if (tid < o) ce[tid] += ce[tid + o];
            __syncthreads();
        }
        if (tid == 0) loss += ce[0];
        seen += total;
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t end = (int64_t)cursor + seen;
        state[0] = (int32_t)(end > capacity ? capacity : end);
        if (flag_bits) state[1] |= flag_bits;
        if (seen) *state_loss(state) += loss;
    }
}

// Pair counting of the one-vs-rest Mann-Whitney statistic: block (x, c) holds 256 rows i (one per lane; those labelled c take part) and walks every
// row j through LDS tiles of 256: the score of column c where row j is labelled otherwise, NaN where it is labelled c or lies past the rows (a stored
// probability is never NaN, and NaN is neither greater than nor equal to anything: such an entry counts nothing).
// partial[(c * gridDim.x + x) * 2 + {0, 1}] = #(s_i > s_j), #(s_i == s_j).
__global__ __launch_bounds__(METRICS_TILE) void metrics_pairs_kernel(const int32_t* __restrict__ state, const float* __restrict__ probs,
                                                                     const int64_t* __restrict__ row_labels, int C, int capacity,
                                                                     int64_t* __restrict__ partial) {
    __shared__ float sc[METRICS_TILE];
    __shared__ unsigned long long red[2][METRICS_TILE];
    const int tid = threadIdx.x, c = blockIdx.y;
    int n = state[0];
    n = n < 0 ? 0 : (n > capacity ? capacity : n);
    const int i = blockIdx.x * METRICS_TILE + tid;
    unsigned long long gt = 0, eq = 0;
    if (blockIdx.x * METRICS_TILE < n) {                             // (uniform: a block past the rows writes zeros)
        const bool mine = i < n && row_labels[i] == c;
        const float si = i < n ? probs[(int64_t)i * C + c] : 0.f;
        for (int j0 = 0; j0 < n; j0 += METRICS_TILE) {
            const int j = j0 + tid;
            sc[tid] = (j < n && row_labels[j] != c) ? probs[(int64_t)j * C + c] : NAN;
            __syncthreads();
            if (mine) {
                unsigned g = 0, e = 0;                               // (at most 256 each per tile)
#pragma unroll 8
                for (int k = 0; k < METRICS_TILE; ++k) {
                    const float sj = sc[k];
                    g += si > sj ? 1u : 0u;
                    e += si == sj ? 1u : 0u;
                }
                gt += g;
                eq += e;
            }
            __syncthreads();
        }
    }
    red[0][tid] = gt;
    red[1][tid] = eq;
    __syncthreads();
    for (int o = METRICS_TILE / 2; o > 0; o >>= 1) {
        if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        int64_t* out = partial + ((int64_t)c * gridDim.x + blockIdx.x) * 2;
        out[0] = (int64_t)red[0][0];
        out[1] = (int64_t)red[1][0];
    }
}

__device__ __forceinline__ double ratio(double a, double b) { return b > 0.0 ? a / b : 0.0; }

// One workgroup: lane c the numbers of class c, lane 0 the aggregates.  The conventions are io.classification_metrics': an empty denominator gives
// 0 for precision / recall / F1 and NaN for an AUC; the operations and their order are those of that function, so the results agree to the last bit.
__global__ __launch_bounds__(64) void metrics_result_kernel(const int32_t* __restrict__ state, int C, int capacity, const int64_t* __restrict__ partial,
                                                            int nblocks, double* __restrict__ result) {
    __shared__ double cls[32][4];
    const int c = threadIdx.x;
    const int32_t* conf = state + WSI_METRICS_STATE_HEAD;
    int n = state[0];
    n = n < 0 ? 0 : (n > capacity ? capacity : n);
    if (c < C) {
        int64_t tp = conf[c * C + c], row = 0, col = 0;
        for (int k = 0; k < C; ++k) { row += conf[c * C + k]; col += conf[k * C + c]; }
        const double p = ratio((double)tp, (double)col), r = ratio((double)tp, (double)row);
        const double f = p + r > 0.0 ? 2.0 * p * r / (p + r) : 0.0;
        int64_t gt = 0, eq = 0;
        for (int x = 0; x < nblocks; ++x) { gt += partial[((int64_t)c * nblocks + x) * 2]; eq += partial[((int64_t)c * nblocks + x) * 2 + 1]; }
        const int64_t P = row, Nn = (int64_t)n - row;
        const double auc = (P > 0 && Nn > 0) ? (double)(2 * gt + eq) / (double)(2 * P * Nn) : (double)NAN;
        cls[c][0] = p; cls[c][1] = r; cls[c][2] = f; cls[c][3] = auc;
        for (int k = 0; k < 4; ++k) result[WSI_METRICS_RESULT_HEAD + 4 * c + k] = cls[c][k];
    }
    __syncthreads();
    if (c == 0) {
        int64_t hits = 0;
        for (int k = 0; k < C; ++k) hits += conf[k * C + k];
        result[0] = (double)n;
        result[1] = (double)state[1];
        result[2] = n > 0 ? (double)hits / (double)n : (double)NAN;
        result[3] = n > 0 ? *state_loss(state) / (double)n : (double)NAN;
        // 'binary': class 1 against the rest; the single-threshold ROC of hard predictions, (TPR + TNR) / 2, as ONE fraction of integers
        double bp = 0.0, br = 0.0, bf = 0.0, ba = (double)NAN;
        if (C > 1) {
            bp = cls[1][0]; br = cls[1][1]; bf = cls[1][2];
            int64_t tp = conf[C + 1], P = 0, col = 0;
            for (int k = 0; k < C; ++k) { P += conf[C + k]; col += conf[k * C + 1]; }
            const int64_t Nn = (int64_t)n - P, fp = col - tp, fn = P - tp, tn = Nn - fp;
            if (P > 0 && Nn > 0) ba = (double)(2 * tp * tn + tp * fp + tn * fn) / (double)(2 * P * Nn);
        }
        result[4] = bp; result[5] = br; result[6] = bf; result[7] = ba;
        for (int k = 0; k < 4; ++k) {                                // 'macro': sum(xs) / C
            double s = 0.0;
            for (int j = 0; j < C; ++j) s += cls[j][k];
            result[8 + k] = s / (double)C;
        }
    }
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_metrics_update(const float* logits, const int64_t* labels, int32_t B, int32_t C, int32_t* state, float* probs,
                                  int64_t* row_labels, int64_t* row_preds, int32_t capacity, void* stream) {
    if (B <= 0 || C <= 0 || C > 32 || (int64_t)B * C > 65536 || capacity < 0) { set_error("metrics_update: unsupported shape %d x %d", B, C); return WSI_ENOSYS; }
    if (!logits || !labels || !state || ((uintptr_t)state & 7) || (capacity > 0 && (!probs || !row_labels || !row_preds))) {
        set_error("metrics_update: null or misaligned pointer");
        return WSI_EINVAL;
    }
    hipLaunchKernelGGL(metrics_update_kernel, dim3(1), dim3(METRICS_TILE), 0, (hipStream_t)stream, logits, labels, (int)B, (int)C, state, probs,
                       row_labels, row_preds, (int)capacity);
    return check_launch("metrics_update");
}

extern "C" int wsi_metrics_finalize(const int32_t* state, const float* probs, const int64_t* row_labels, int32_t C, int32_t capacity,
                                    int64_t* pair_partials, double* result, void* stream) {
    if (C <= 0 || C > 32 || capacity < 0) { set_error("metrics_finalize: unsupported shape (%d classes, capacity %d)", C, capacity); return WSI_ENOSYS; }
    if (!state || ((uintptr_t)state & 7) || !result || (capacity > 0 && (!probs || !row_labels || !pair_partials))) {
        set_error("metrics_finalize: null or misaligned pointer");
        return WSI_EINVAL;
    }
    const int nblocks = (capacity + METRICS_TILE - 1) / METRICS_TILE;
    if (nblocks > 0) {
        hipLaunchKernelGGL(metrics_pairs_kernel, dim3(nblocks, C), dim3(METRICS_TILE), 0, (hipStream_t)stream, state, probs, row_labels, (int)C,
                           (int)capacity, pair_partials);
        const int rc = check_launch("metrics_finalize (pairs)");
        if (rc != WSI_OK) return rc;
    }
    hipLaunchKernelGGL(metrics_result_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, (int)C, (int)capacity, pair_partials, nblocks, result);
    return check_launch("metrics_finalize");
}
