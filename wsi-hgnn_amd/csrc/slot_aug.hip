// Fill of a padded batch slot with AUGMENTED slides (graph.slot_fill_augmented): the draw is taken on the device (wsi_augment_nodes /
// wsi_augment_edges over one descriptor row per (slide, node type) / (slide, relation)), and the slot's tables are written from the survivors'
// counts WITHOUT reading them back.  A stored slide's plan pieces are in CSR order already and DropNode renumbers monotonically, so the pieces of
// the augmented slide are stable compactions of the stored ones: keep flags -> the two-level scans of common.h -> one single-thread layout kernel
// (csrc/slot_layout.h) turns the counts into every offset -> the real slides PUSH their surviving entries to (device offset + rank), grids sized by the stored counts; the filler and the tails are PULLED by position, grids sized by the
// capacities, from the closed forms of csrc/slot_math.h.  No atomics: every position is a scan result.  Contract: include/wsi_hgnn.h.
#include <string.h>

#include "common.h"
#include "slot_layout.h"
#include "slot_math.h"

namespace wsi {

constexpr int SA_TILE = 1024;             // elements per workgroup: 4 rounds of 256 lanes
constexpr int SA_FROW = 8;                // int64 words per flag segment: n, off, first_tile, kind, p0, p1, b, -
constexpr int SA_PROW = 10;               // ... per push segment: n, first_block, kind, b, t, p0, p1, p2, p3, flag segment
constexpr int SA_XROW = 3;                // ... per (slide, type) feature table: pointer, rows, mask sub-seed
constexpr int SA_EROW = 14;               // wsi_augment_edges' row
constexpr int SA_NROW = 6;                // wsi_augment_nodes' row
constexpr int64_t SA_COO_MASK = (1ll << 40) - 1;

// the 55 argument words of include/wsi_hgnn.h (wsi_slot_aug_*), by name: every field is 8 bytes, the order is the words'
struct Args {
    const int64_t* desc;
    int64_t off_node, off_edge, off_flag, off_push, off_feat, off_shape, off_misc;
    int64_t B, T, R, N, S, E, G;
    int64_t nflag, flag_tiles, npush, push_blocks, nodes_stored, ns_mode, F, mask_thr, feat_aligned;
    int32_t* new_id; int64_t* kept; int32_t* ncnt; int32_t* rank1; int32_t* ftile; int32_t* frank; int32_t* fcnt; int64_t* keys; const int64_t* perm; int64_t* L;
    int32_t* rowptr; int32_t* colptr; int32_t* node_seg; int32_t* src; int32_t* csc_eid; int32_t* csc_dst; int32_t* order_dst; int32_t* order_src;
    float* sim; float* inv_rd; int32_t* readout_ptr; int64_t* labels; float* feat; int32_t* edge_seg; int32_t* row_seg;
    int32_t* chunk_row; int32_t* chunk_seg; int32_t* seg_chunk; float* seg_counts; float* seg_inv_counts; float* seg_nonempty;
};
constexpr int SA_WORDS = 55;
static_assert(sizeof(Args) == SA_WORDS * 8, "the argument words and the struct must agree");

// misc block: noff[B T] (first element of (b, t) in new_id / kept / keys), nstored[B T], coo_base[B], labels[G], shuffle sub-seeds [B T]
__device__ __forceinline__ const int64_t* sa_noff(const Args& a) { return a.desc + a.off_misc; }
__device__ __forceinline__ const int64_t* sa_nstored(const Args& a) { return a.desc + a.off_misc + a.B * a.T; }
__device__ __forceinline__ const int64_t* sa_coo_base(const Args& a) { return a.desc + a.off_misc + 2 * a.B * a.T; }
__device__ __forceinline__ const int64_t* sa_labels(const Args& a) { return a.desc + a.off_misc + 2 * a.B * a.T + a.B; }
__device__ __forceinline__ const int64_t* sa_key_seed(const Args& a) { return a.desc + a.off_misc + 2 * a.B * a.T + a.B + a.G; }

// does element i of flag segment d survive the draw
__device__ __forceinline__ bool sa_keep(const Args& a, const int64_t* __restrict__ d, int64_t i) {
    const int64_t b = d[6];
    if (d[3] == 0) {              // an entry of the slide's CSR or CSC pieces: its COO edge (relation << 40 | index in the slide's concatenated COO)
        const int64_t m = reinterpret_cast<const int64_t*>(d[4])[i];
        const int64_t* e = a.desc + a.off_edge + (b * a.R + (m >> 40)) * SA_EROW;
        const int rk = a.rank1[sa_coo_base(a)[b] + (m & SA_COO_MASK)];
        if (e[13] != 0) return rk >= 0;            // a relation with a quota: wsi_augment_edges left the FINAL decision in rank1
        return rk >= 0 && !(e[10] != 0 && drawn((uint32_t)rk, (uint32_t)e[8], (uint32_t)e[9]));
    }
    const int64_t l = reinterpret_cast<const int64_t*>(d[4])[i], t = reinterpret_cast<const int64_t*>(d[5])[i];
    return a.new_id[sa_noff(a)[b * a.T + t] + l] >= 0;
}

// PASS 0: tile sums.  PASS 1 (after the scan): rank[off + i] = kept entries of the segment in front of i, as r when i is kept and ~r when not
template <int PASS>
__global__ __launch_bounds__(256) void sa_flags_kernel(Args a) {
    __shared__ int lds[4];
    const int blk = blockIdx.x;
    const int64_t* rows = a.desc + a.off_flag;
    const int64_t* d = rows + (int64_t)find_row(rows, SA_FROW, 2, (int)a.nflag, blk) * SA_FROW;
    const int64_t n = d[0], off = d[1];
    const int ft = (int)d[2];
    const int64_t i0 = (int64_t)(blk - ft) * SA_TILE;
    int run = PASS == 1 ? a.ftile[blk] - a.ftile[ft] : 0;
    for (int r = 0; r < SA_TILE / 256; ++r) {
        const int64_t i = i0 + r * 256 + threadIdx.x;
        const bool keep = i < n && sa_keep(a, d, i);
        int total;
        const int excl = block_flag_scan(keep, lds, total);
        if (PASS == 1 && i < n) a.frank[off + i] = keep ? run + excl : ~(run + excl);
        run += total;
    }
    if (PASS == 0 && threadIdx.x == 0) a.ftile[blk] = run;
}

// counts -> every offset of the fill and the readout's small tables; labels ride along
__global__ void sa_layout_kernel(Args a) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        slot_layout(a.desc + a.off_shape, a.ncnt, a.fcnt, a.L, a.readout_ptr, a.chunk_row, a.chunk_seg, a.seg_chunk, a.seg_counts, a.seg_inv_counts,
                    a.seg_nonempty);
        const int64_t* lab = sa_labels(a);
        for (int64_t g = 0; g < a.G; ++g) a.labels[g] = lab[g];
    }
}

// NodeShuffle's sort keys of every stored node position: (segment << 33) | key; positions at or beyond the segment's limit (the survivors'
// count when the shuffle follows DropNode) carry 1 << 32, above every real key.  ns_mode 0: no shuffle, key = position.
__global__ __launch_bounds__(256) void sa_keys_kernel(Args a) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= a.nodes_stored) return;
    const int64_t* noff = sa_noff(a);
    int s = (int)(a.B * a.T) - 1;
    while (s > 0 && noff[s] > x) --s;
    const int64_t i = x - noff[s];
    const int64_t limit = a.ns_mode == 2 ? (int64_t)a.ncnt[s] : sa_nstored(a)[s];
    const int64_t key = i < limit ? (a.ns_mode == 0 ? i : (int64_t)index_hash((uint32_t)i, (uint32_t)sa_key_seed(a)[s])) : (1ll << 32);
    a.keys[x] = ((int64_t)s << 33) | key;
}

// kept entries of flag segment s in front of position v (v may be the segment's end)
__device__ __forceinline__ int64_t sa_prefix(const Args& a, int64_t s, int64_t v) {
    const int64_t* d = a.desc + a.off_flag + s * SA_FROW;
    if (v >= d[0]) return a.fcnt[s];
    const int r = a.frank[d[1] + v];
    return r >= 0 ? r : ~r;
}

// the real slides: every surviving node, CSR edge, CSC entry and order entry writes itself at (device offset + rank).  Every position is
// checked against the table it goes to: with capacities below the stored counts (survivor quotas) a wrong count may misplace an
// entry, it cannot write outside a table.
__device__ __forceinline__ bool sa_in(int64_t p, int64_t n) { return p >= 0 && p < n; }

__global__ __launch_bounds__(256) void sa_push_kernel(Args a) {
    const int blk = blockIdx.x;
    const int64_t* rows = a.desc + a.off_push;
    const int64_t* d = rows + (int64_t)find_row(rows, SA_PROW, 1, (int)a.npush, blk) * SA_PROW;
    const int64_t n = d[0], kind = d[2], b = d[3], t = d[4], B = a.B, T = a.T;
    const int64_t* L = a.L;
    const int64_t* node = L + SLOT_L_NODE(B, T);
    const int64_t* edge = L + SLOT_L_EDGE(B, T);
    const int64_t* csc = L + SLOT_L_CSC(B, T);
    const int64_t* seg = L + SLOT_L_SEG(B, T);
    const int64_t* ord = L + SLOT_L_ORD(B, T);
    const int64_t* noff = sa_noff(a);
    const int64_t bt = b * T + t;
    const int64_t i0 = (int64_t)(blk - d[1]) * SA_TILE;
#pragma unroll 1
    for (int r = 0; r < SA_TILE / 256; ++r) {
        const int64_t i = i0 + r * 256 + threadIdx.x;
        if (i >= n) break;
        if (kind == 0) {                                  // node i of (b, t): p0 = stored rowptr piece [n R], p1 = stored colptr piece [n]
            const int m = a.new_id[noff[bt] + i];
            if (m < 0) continue;
            const int64_t R = slot_shape_type(a.desc + a.off_shape, t)[SS_R];
            const int64_t* rp = reinterpret_cast<const int64_t*>(d[5]);
            for (int64_t q = 0; q < R; ++q)
                if (sa_in(seg[bt] + m * R + q, a.S)) a.rowptr[seg[bt] + m * R + q] = (int32_t)(edge[bt] + sa_prefix(a, bt, rp[i * R + q]));
            if (!sa_in(node[bt] + m, a.N)) continue;
            a.colptr[node[bt] + m] = (int32_t)(csc[bt] + sa_prefix(a, B * T + bt, reinterpret_cast<const int64_t*>(d[6])[i]));
            a.row_seg[node[bt] + m] = (int32_t)(t * a.G + b);
        } else if (kind == 1) {                           // CSR edge i into (b, t): p0 = src_l, p1 = src_t, p2 = sim, p3 = local segment (node R + slot)
            const int rk = a.frank[(a.desc + a.off_flag + d[9] * SA_FROW)[1] + i];
            if (rk < 0) continue;
            const int64_t R = slot_shape_type(a.desc + a.off_shape, t)[SS_R];
            const int64_t pos = edge[bt] + rk;
            if (!sa_in(pos, a.E)) continue;
            const int64_t st = b * T + reinterpret_cast<const int64_t*>(d[6])[i];
            a.src[pos] = (int32_t)(node[st] + a.new_id[noff[st] + reinterpret_cast<const int64_t*>(d[5])[i]]);
            a.sim[pos] = reinterpret_cast<const float*>(d[7])[i];
            const int64_t ls = reinterpret_cast<const int64_t*>(d[8])[i];
            a.edge_seg[pos] = (int32_t)(seg[bt] + (int64_t)a.new_id[noff[bt] + ls / R] * R + ls % R);
        } else if (kind == 2) {                           // CSC entry i out of (b, t): p0 = eid_l, p1 = ent_t, p2 = dst_l
            const int rk = a.frank[(a.desc + a.off_flag + d[9] * SA_FROW)[1] + i];
            if (rk < 0) continue;
            const int64_t pos = csc[bt] + rk;
            if (!sa_in(pos, a.E)) continue;
            const int64_t dt = b * T + reinterpret_cast<const int64_t*>(d[6])[i];
            a.csc_eid[pos] = (int32_t)(edge[dt] + sa_prefix(a, dt, reinterpret_cast<const int64_t*>(d[5])[i]));
            a.csc_dst[pos] = (int32_t)(node[dt] + a.new_id[noff[dt] + reinterpret_cast<const int64_t*>(d[7])[i]]);
        } else {                                          // order entry i of slide b: p0 = local id, p1 = node type; kind 3 heavy, 4 light, 5 source
            const int rk = a.frank[(a.desc + a.off_flag + d[9] * SA_FROW)[1] + i];
            if (rk < 0) continue;
            const int64_t nt = b * T + reinterpret_cast<const int64_t*>(d[6])[i];
            const int32_t id = (int32_t)(node[nt] + a.new_id[noff[nt] + reinterpret_cast<const int64_t*>(d[5])[i]]);
            const int64_t pos = ord[(kind == 5 ? 2 : kind - 3) * B + b] + rk;
            if (!sa_in(pos, a.N)) continue;
            if (kind == 5) a.order_src[pos] = id;
            else a.order_dst[pos] = id;
        }
    }
}

// the filler and the tails, by position: [0, S] rowptr, then [0, N] colptr / node_seg / inv_rd / row_seg / orders, then [0, E) the edge tables
__global__ __launch_bounds__(256) void sa_pull_kernel(Args a) {
    int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t B = a.B, T = a.T;
    const int64_t* shape = a.desc + a.off_shape;
    const int64_t* L = a.L;
    const int64_t* nn = L + SLOT_L_N(B, T);
    const int64_t* ee = L + SLOT_L_E(B, T);
    const int64_t* fp = L + SLOT_L_FILL(B, T);
    if (x <= a.S) {
        if (x == a.S) { a.rowptr[x] = (int32_t)a.E; return; }
        int64_t t = T - 1;
        while (t > 0 && slot_shape_type(shape, t)[SS_SOFF] > x) --t;
        const int64_t* s = slot_shape_type(shape, t);
        const int64_t y = x - s[SS_SOFF] - nn[t] * s[SS_R];
        if (y >= 0 && s[SS_R] > 0) a.rowptr[x] = (int32_t)filler_rowptr(fp, t, y);
        return;
    }
    x -= a.S + 1;
    if (x <= a.N) {
        if (x == a.N) { a.colptr[x] = (int32_t)a.E; a.node_seg[x] = (int32_t)a.S; return; }
        int64_t t = T - 1;
        while (t > 0 && slot_shape_type(shape, t)[SS_TOFF] > x) --t;
        const int64_t* s = slot_shape_type(shape, t);
        const int64_t l = x - s[SS_TOFF];
        a.node_seg[x] = (int32_t)(s[SS_SOFF] + l * s[SS_R]);
        a.inv_rd[x] = s[SS_R] > 0 ? (float)(1.0 / (double)s[SS_R]) : 0.0f;
        const int64_t u = l - nn[t];
        if (u >= 0) {
            a.colptr[x] = (int32_t)filler_colptr(fp, t, u);
            a.row_seg[x] = (int32_t)(t * a.G + a.G - 1);
            int64_t pos = (L + SLOT_L_ORD(B, T))[3 * B] + u;              // behind the real nodes: the filler's, ascending
            for (int64_t k = 0; k < t; ++k) pos += filler_type(fp, k)[FP_NF];
            if (pos >= 0 && pos < a.N) { a.order_dst[pos] = (int32_t)x; a.order_src[pos] = (int32_t)x; }
        }
        return;
    }
    x -= a.N + 1;
    if (x < a.E) {
        int64_t t = T - 1;
        while (t > 0 && slot_shape_type(shape, t)[SS_EBASE] > x) --t;
        const int64_t* s = slot_shape_type(shape, t);
        const int64_t k = x - s[SS_EBASE] - ee[t];
        if (k < 0) return;
        const int64_t* f = filler_type(fp, t);
        a.src[x] = (int32_t)filler_src(fp, t, k);
        a.sim[x] = 0.0f;
        int64_t nd, kk;
        filler_owner(k, f[FP_EF], f[FP_NF], &nd, &kk);
        a.edge_seg[x] = (int32_t)(s[SS_SOFF] + (nn[t] + nd) * s[SS_R]);
        int64_t slot, eid, dst;
        filler_csc(fp, t, k, &slot, &eid, &dst);
        if (slot >= 0 && slot < a.E) { a.csc_eid[slot] = (int32_t)eid; a.csc_dst[slot] = (int32_t)dst; }
    }
}

// features: one wave per row of the slot's table.  A real row m of (b, t) gathers the slide's stored row through the composed row index
// (kept = DropNode's survivors, perm = the sorted shuffle keys) with FeatMask's column draw applied on the way; filler rows are zero.
template <bool VEC>
__global__ __launch_bounds__(256) void sa_feat_kernel(Args a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= a.N) return;
    const int64_t B = a.B, T = a.T;
    const int F = (int)a.F;
    const int64_t* shape = a.desc + a.off_shape;
    const int64_t* node = a.L + SLOT_L_NODE(B, T);
    int64_t t = T - 1;
    while (t > 0 && slot_shape_type(shape, t)[SS_TOFF] > g) --t;
    const float* xr = nullptr;
    uint32_t seed = 0;
    if (g - slot_shape_type(shape, t)[SS_TOFF] < (a.L + SLOT_L_N(B, T))[t]) {
        int64_t b = B - 1;
        while (b > 0 && node[b * T + t] > g) --b;
        const int64_t bt = b * T + t, m = g - node[bt], off = sa_noff(a)[bt];
        int64_t r;
        if (a.ns_mode == 2) r = a.kept[off + (a.perm[off + m] - off)];
        else r = a.perm[off + a.kept[off + m]] - off;
        const int64_t* xd = a.desc + a.off_feat + bt * SA_XROW;
        if (r >= 0 && r < xd[1]) xr = reinterpret_cast<const float*>(xd[0]) + r * F;
        seed = (uint32_t)xd[2];
    }
    const uint32_t thr = (uint32_t)a.mask_thr;
    float* orow = a.feat + g * F;
    if (VEC) {
        for (int c = 4 * lane; c < F; c += 256) {
            float4 v = xr ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (xr && thr) {
                if (drawn((uint32_t)c, seed, thr)) v.x = 0.f;
                if (drawn((uint32_t)c + 1, seed, thr)) v.y = 0.f;
                if (drawn((uint32_t)c + 2, seed, thr)) v.z = 0.f;
                if (drawn((uint32_t)c + 3, seed, thr)) v.w = 0.f;
            }
            *reinterpret_cast<float4*>(orow + c) = v;
        }
    } else {
        for (int c = lane; c < F; c += 64) orow[c] = (xr && !(thr && drawn((uint32_t)c, seed, thr))) ? xr[c] : 0.f;
    }
}

// survivor quotas: what the draw exceeded them by, from the tile sums the two augmentation calls leave behind (the counts
// themselves are clamped by then).  ONE thread, plain loads and stores, stream-ordered behind the fill's scans and in front of the next fill's:
// ovf[0] += 1 when some quota bound in this fill, ovf[1] / ovf[2] = the largest excess any fill has seen of a node / an edge row.
__device__ __forceinline__ int64_t sa_excess(const int64_t* rows, int stride, int nrow, const int32_t* tsum) {
    int64_t worst = 0;
    for (int s = 0; s < nrow; ++s) {
        const int64_t* d = rows + (int64_t)s * stride;
        if (d[0] <= 0 || d[stride - 1] <= 0) continue;
        const int64_t ft = d[2], nt = (d[0] + SA_TILE - 1) / SA_TILE;
        const int64_t over = (int64_t)tsum[ft + nt] - tsum[ft] - (d[stride - 1] - 1);
        worst = over > worst ? over : worst;
    }
    return worst;
}

__global__ void sa_quota_kernel(const int64_t* nrows, int nnode, const int32_t* tsum_n, const int64_t* erows, int nedge, const int32_t* tsum_e2,
                                int64_t* ovf) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t xn = sa_excess(nrows, SA_NROW, nnode, tsum_n);
    const int64_t xe = nedge > 0 ? sa_excess(erows, SA_EROW, nedge, tsum_e2) : 0;
    if (xn > 0 || xe > 0) ovf[0] += 1;
    if (xn > ovf[1]) ovf[1] = xn;
    if (xe > ovf[2]) ovf[2] = xe;
}

static bool sa_bad(const int64_t* words, Args* a, const char* what) {
    if (!words) { set_error("%s: null pointer", what); return true; }
    memcpy(a, words, sizeof(Args));
    if (!a->desc || a->B < 1 || a->T < 1 || a->R < 0 || a->N < 1 || a->S < 0 || a->E < 0 || a->G < a->B + 1 || a->nflag < 0 || a->flag_tiles < 0 ||
        a->npush < 0 || a->push_blocks < 0 || a->nodes_stored < 0 || a->F < 0 || a->ns_mode < 0 || a->ns_mode > 2 || a->mask_thr < 0 || a->mask_thr > 65536) {
        set_error("%s: bad argument", what);
        return true;
    }
    return false;
}

}  // namespace wsi

using namespace wsi;

extern "C" int wsi_slot_aug_keys(const int64_t* args, void* stream) {
    Args args_, *a = &args_;
    if (sa_bad(args, a, "slot_aug_keys")) return WSI_EINVAL;
    if (a->nodes_stored == 0) return WSI_OK;
    if (!a->keys || !a->ncnt) { set_error("slot_aug_keys: null pointer"); return WSI_EINVAL; }
    hipLaunchKernelGGL(sa_keys_kernel, dim3((unsigned)((a->nodes_stored + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
    return check_launch("slot_aug_keys");
}

extern "C" int wsi_slot_aug_scan(const int64_t* args, void* stream) {
    Args args_, *a = &args_;
    if (sa_bad(args, a, "slot_aug_scan")) return WSI_EINVAL;
    if (!a->new_id || !a->ncnt || !a->rank1 || !a->ftile || !a->frank || !a->fcnt || !a->L || !a->readout_ptr || !a->chunk_row || !a->chunk_seg ||
        !a->seg_chunk || !a->seg_counts || !a->seg_inv_counts || !a->seg_nonempty || !a->labels) {
        set_error("slot_aug_scan: null pointer");
        return WSI_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    if (a->flag_tiles > 0) hipLaunchKernelGGL(sa_flags_kernel<0>, dim3((unsigned)a->flag_tiles), dim3(256), 0, s, *a);
    launch_tile_scan(a->ftile, (int)a->flag_tiles, a->desc + a->off_flag, SA_FROW, 2, (int)a->nflag, a->fcnt, s);
    if (a->flag_tiles > 0) hipLaunchKernelGGL(sa_flags_kernel<1>, dim3((unsigned)a->flag_tiles), dim3(256), 0, s, *a);
    hipLaunchKernelGGL(sa_layout_kernel, dim3(1), dim3(64), 0, s, *a);
    return check_launch("slot_aug_scan");
}

extern "C" int wsi_slot_aug_write(const int64_t* args, void* stream) {
    Args args_, *a = &args_;
    if (sa_bad(args, a, "slot_aug_write")) return WSI_EINVAL;
    if (!a->new_id || !a->kept || !a->perm || !a->frank || !a->fcnt || !a->L || !a->rowptr || !a->colptr || !a->node_seg || !a->order_dst ||
        !a->order_src || !a->inv_rd || !a->row_seg || !a->feat || (a->E > 0 && (!a->src || !a->csc_eid || !a->csc_dst || !a->sim || !a->edge_seg))) {
        set_error("slot_aug_write: null pointer");
        return WSI_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    if (a->push_blocks > 0) hipLaunchKernelGGL(sa_push_kernel, dim3((unsigned)a->push_blocks), dim3(256), 0, s, *a);
    const int64_t pulls = a->S + 1 + a->N + 1 + a->E;
    hipLaunchKernelGGL(sa_pull_kernel, dim3((unsigned)((pulls + 255) / 256)), dim3(256), 0, s, *a);
    if (a->F > 0) {
        const bool vec = a->F % 4 == 0 && (reinterpret_cast<uintptr_t>(a->feat) & 15) == 0 && a->feat_aligned != 0;
        const dim3 grid((unsigned)((a->N + 3) / 4));
        if (vec) hipLaunchKernelGGL(sa_feat_kernel<true>, grid, dim3(256), 0, s, *a);
        else hipLaunchKernelGGL(sa_feat_kernel<false>, grid, dim3(256), 0, s, *a);
    }
    return check_launch("slot_aug_write");
}

extern "C" int wsi_slot_aug_quota(const int64_t* node_rows, int32_t nnode, const int32_t* tsum_n, const int64_t* edge_rows, int32_t nedge,
                                  int32_t etiles, const int32_t* tsum_e, int64_t* overflow, void* stream) {
    if (nnode < 0 || nedge < 0 || etiles < 0) { set_error("slot_aug_quota: bad argument"); return WSI_EINVAL; }
    if (!node_rows || !tsum_n || !overflow || (nedge > 0 && (!edge_rows || !tsum_e))) { set_error("slot_aug_quota: null pointer"); return WSI_EINVAL; }
    hipLaunchKernelGGL(sa_quota_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, node_rows, (int)nnode, tsum_n, edge_rows, (int)nedge,
                       nedge > 0 ? tsum_e + etiles + 1 : tsum_e, overflow);
    return check_launch("slot_aug_quota");
}
