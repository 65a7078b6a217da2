// Patch dropout of many bags and the fill of a padded bag slot (mil.dropout_patches, mil.BagSlot).  Contract: include/wsi_hgnn.h.
//
// The reference drops patches per bag on the host (train_tcga_k-fold.py:90-96): keep k rows without replacement, append m of the kept rows again.
// Here the draw is a hash of (row, bag draw word) and the choice is "the k smallest (key1, row)" / "the m kept rows with the smallest (key2, row)":
//   selection : one workgroup per bag.  The k-th smallest key is found by a radix select over RECOMPUTED keys - four passes of one 256-bin LDS
//               histogram, most significant byte first, integer atomics only (same bits run after run) - then one pass in row order writes the
//               kept rows: a row is kept when its key is below the threshold, or equals it and fewer than `need` equal keys came before it (the
//               lower row wins a tie); its place is a block scan.  The pad rows repeat this over the kept rows just written (read back from L2).
//               No key is ever stored; a bag knows nothing of the others.
//   rows      : a wave per destination row: which bag owns it (binary search over the descriptors), which source row (the table above, or the
//               row itself), then a streaming copy - 16-byte lane accesses when both sides allow, a scalar path otherwise.  Rows no bag owns
//               (the filler of a slot) are zeroed.  The same launch writes the row -> segment table and copies the host-built small tables.
#include "common.h"

namespace wsi {

constexpr int BS_DESC = 8;              // int64 words per bag: [src, stride, n, k, m, dst_row, draw, 0]
constexpr int BS_SEL_THREADS = 1024;    // selection: 16 waves walk a bag's rows 1024 at a time
constexpr int BS_SEL_WAVES = BS_SEL_THREADS / 64;
constexpr int BS_ROW_THREADS = 256;
constexpr int BS_ROWS = 16;             // destination rows per workgroup of the row kernel (4 per wave)

__device__ __forceinline__ uint32_t bs_key(uint32_t i, uint32_t s, uint32_t mask) { return index_hash(i, s) & mask; }

// inclusive scan of v over the workgroup's threads in thread order; total = the sum over all of them.  (Two barriers: wsum is reused.)
// Not common.h's block_scan_inclusive: this one serves 1024 threads (16 wave totals) and has its first barrier BEFORE the totals are written.
__device__ __forceinline__ uint32_t bs_block_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < BS_SEL_WAVES; ++w) {
        const uint32_t x = wsum[w];
        if (w < wave) base += x;
        tot += x;
    }
    total = tot;
    return v + base;
}

// The `want` smallest (key, position) of a list of `count` rows, written in list order to out[0 .. want).  list == nullptr: the rows 0 .. count - 1
// themselves; otherwise row j of the list is list[j] (ascending, so the order of positions is the order of rows).  1 <= want <= count.
__device__ void bs_select(const int32_t* list, int count, int want, uint32_t seed, uint32_t mask, int32_t* out, int64_t out_room,
                          uint32_t* hist, uint32_t* wsum, uint32_t* pick) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0, pmask = 0, remaining = (uint32_t)want;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int j = tid; j < count; j += BS_SEL_THREADS) {
            const uint32_t row = list ? (uint32_t)__hip_atomic_load(list + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (uint32_t)j;
            const uint32_t key = bs_key(row, seed, mask);
            if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        const uint32_t h = tid < 256 ? hist[tid] : 0u;
        uint32_t total;
        const uint32_t incl = bs_block_scan(h, wsum, total);
        if (tid < 256 && incl - h < remaining && remaining <= incl) { pick[0] = (uint32_t)tid; pick[1] = incl - h; }
        __syncthreads();
        prefix |= pick[0] << shift;
        pmask |= 255u << shift;
        remaining -= pick[1];
        __syncthreads();
    }
    const uint32_t T = prefix, need = remaining;        // keys below T are all taken; of the keys equal to T the first `need` in list order
    uint32_t lt_base = 0, eq_base = 0;
    for (int j0 = 0; j0 < count; j0 += BS_SEL_THREADS) {
        const int j = j0 + tid;
        const bool valid = j < count;
        uint32_t row = 0, key = 0xffffffffu;
        if (valid) {
            row = list ? (uint32_t)__hip_atomic_load(list + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (uint32_t)j;
            key = bs_key(row, seed, mask);
        }
        const uint32_t lt = (valid && key < T) ? 1u : 0u, eq = (valid && key == T) ? 1u : 0u;
        const uint32_t packed = lt | (eq << 16);           // (at most 1024 of either per tile: 16 bits each)
        uint32_t total;
        const uint32_t excl = bs_block_scan(packed, wsum, total) - packed;
        const uint32_t lt_before = lt_base + (excl & 0xffffu), eq_before = eq_base + (excl >> 16);
        if (lt || (eq && eq_before < need)) {
            const int64_t pos = (int64_t)lt_before + (eq_before < need ? eq_before : need);
            if (pos < out_room) out[pos] = (int32_t)row;
        }
        lt_base += total & 0xffffu;
        eq_base += total >> 16;
    }
}

__global__ __launch_bounds__(BS_SEL_THREADS) void bag_dropout_select_kernel(const int64_t* __restrict__ desc, uint32_t mask,
                                                                            int32_t* sel, int64_t sel_rows) {
    const int64_t* d = desc + (int64_t)blockIdx.x * BS_DESC;
    const int64_t n64 = d[2];
    const int64_t dst = d[5];
    if (n64 <= 0 || n64 > 0x7fffffff || dst < 0 || dst >= sel_rows) return;
    const int n = (int)n64;
    const int k = (int)(d[3] < 0 ? 0 : (d[3] > n ? n : d[3]));
    const int m = (int)(d[4] < 0 ? 0 : (d[4] > k ? k : d[4]));
    const uint32_t draw = (uint32_t)d[6];
    const int64_t room = sel_rows - dst;                 // rows of sel this bag may write
    int32_t* out = sel + dst;
    __shared__ uint32_t hist[256], wsum[BS_SEL_WAVES], pick[2];
    if (k == n) {                                        // nothing dropped: the rows themselves
        for (int j = threadIdx.x; j < k; j += BS_SEL_THREADS) if (j < room) out[j] = j;
    } else if (k > 0) {
        bs_select(nullptr, n, k, drop_fmix32(draw), mask, out, room, hist, wsum, pick);
    }
    if (m == 0 || k >= room) return;
    __threadfence();
    __syncthreads();                                     // the kept rows are in memory: the pad rows are chosen among them
    bs_select(out, k, m, drop_fmix32(draw ^ 0x85EBCA6Bu), mask, out + k, room - k, hist, wsum, pick);
}

__global__ __launch_bounds__(BS_ROW_THREADS) void bag_slot_rows_kernel(const int64_t* __restrict__ desc, int num_bags,
                                                                       const int32_t* __restrict__ sel, float* __restrict__ rows, int64_t ld,
                                                                       int feats, int64_t num_rows, bool dst_vec, int row_blocks,
                                                                       int32_t* __restrict__ row_seg, int32_t filler_seg,
                                                                       const int32_t* __restrict__ small_src, int32_t* __restrict__ small_dst,
                                                                       int small_words) {
    if ((int)blockIdx.x >= row_blocks) {                 // the host-built small tables: a plain word copy
        const int64_t i = ((int64_t)blockIdx.x - row_blocks) * BS_ROW_THREADS + threadIdx.x;
        if (i < small_words) small_dst[i] = small_src[i];
        return;
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int q = 0; q < BS_ROWS / 4; ++q) {
        const int64_t r = (int64_t)blockIdx.x * BS_ROWS + q * 4 + wave;
        if (r >= num_rows) return;
        // the last bag whose first destination row is <= r (empty bags share a first row with their successor)
        int lo = -1;
        if (num_bags > 0 && desc[5] <= r) {
            lo = 0;
            int hi = num_bags - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (desc[(int64_t)mid * BS_DESC + 5] <= r) lo = mid; else hi = mid - 1;
            }
        }
        const float* src = nullptr;
        int64_t stride = 0;
        if (lo >= 0) {
            const int64_t* d = desc + (int64_t)lo * BS_DESC;
            const int64_t j = r - d[5];
            if (j < d[3] + d[4]) {
                const int64_t i = sel ? (int64_t)sel[r] : j;
                if (i >= 0 && i < d[2]) {
                    stride = d[1];
                    src = reinterpret_cast<const float*>(d[0]) + i * stride;
                }
            } else lo = -1;
        }
        if (row_seg && lane == 0) row_seg[r] = lo >= 0 ? lo : filler_seg;
        float* dstp = rows + r * ld;
        const bool vec = dst_vec && (src == nullptr || (((reinterpret_cast<uintptr_t>(src) & 15) == 0) && (stride % 4 == 0)));
        if (vec) {
            for (int col = lane * 4; col < feats; col += 256)
                *reinterpret_cast<float4*>(dstp + col) = src ? *reinterpret_cast<const float4*>(src + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            for (int col = lane; col < feats; col += 64) dstp[col] = src ? src[col] : 0.f;
        }
    }
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_bag_dropout_select(const int64_t* bag_desc, int32_t num_bags, int32_t key_bits, int32_t* sel, int64_t sel_rows,
                                      void* stream) {
    if (num_bags < 0 || sel_rows < 0 || key_bits < 1 || key_bits > 32) { set_error("bag_dropout_select: bad argument"); return WSI_EINVAL; }
    if (num_bags == 0 || sel_rows == 0) return WSI_OK;
    if (!bag_desc || !sel) { set_error("bag_dropout_select: null pointer"); return WSI_EINVAL; }
    const uint32_t mask = key_bits == 32 ? 0xffffffffu : ((1u << key_bits) - 1u);
    hipLaunchKernelGGL(bag_dropout_select_kernel, dim3(num_bags), dim3(BS_SEL_THREADS), 0, (hipStream_t)stream, bag_desc, mask, sel, sel_rows);
    return check_launch("bag_dropout_select");
}

extern "C" int wsi_bag_slot_fill(const int64_t* bag_desc, int32_t num_bags, const int32_t* sel, float* rows, int64_t ld, int32_t feats,
                                 int64_t num_rows, int32_t* row_seg, int32_t filler_seg,
                                 const int32_t* small_src, int32_t* small_dst, int32_t small_words, void* stream) {
    if (num_bags < 0 || feats <= 0 || ld < feats || num_rows < 0 || small_words < 0 || num_rows > 0x7fffffff) {
        set_error("bag_slot_fill: bad argument"); return WSI_EINVAL;
    }
    if ((num_bags > 0 && !bag_desc) || (num_rows > 0 && !rows) || (small_words > 0 && (!small_src || !small_dst))) {
        set_error("bag_slot_fill: null pointer"); return WSI_EINVAL;
    }
    const int row_blocks = (int)((num_rows + BS_ROWS - 1) / BS_ROWS), small_blocks = (small_words + BS_ROW_THREADS - 1) / BS_ROW_THREADS;
    if (row_blocks + small_blocks == 0) return WSI_OK;
    const bool dst_vec = ((reinterpret_cast<uintptr_t>(rows) & 15) == 0) && (ld % 4 == 0) && (feats % 4 == 0);
    hipLaunchKernelGGL(bag_slot_rows_kernel, dim3(row_blocks + small_blocks), dim3(BS_ROW_THREADS), 0, (hipStream_t)stream, bag_desc,
                       (int)num_bags, sel, rows, ld, (int)feats, num_rows, dst_vec, row_blocks, row_seg, filler_seg, small_src, small_dst,
                       (int)small_words);
    return check_launch("bag_slot_fill");
}
