/*
 * wsi_hgnn.h — C-ABI of libwsi_hgnn.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * message-passing hot path of HKU-MedAI/WSI-HGNN.
 *
 * The reference has NO native layer: its hot path is Python calling DGL's message-passing API and
 * torch.nn.Linear.  Each entry point below therefore cites the reference *call site*
 * (file:line under /root/reference) whose DGL / BLAS kernels it replaces; INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch tensors in the shipped host code);
 *     the library never allocates, frees or retains user-visible memory; scratch is passed in;
 *   - row-major contiguous fp32 data, int32 indices; `ld*` are row strides in ELEMENTS;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it, no internal sync;
 *   - returns 0 on success, a negative errno-style code otherwise (WSI_E*); wsi_last_error() gives
 *     a thread-local message.  No C++ exception crosses the boundary;
 *   - re-entrant, NO global mutable state: the caller selects the device (hipSetDevice / torch.cuda.device) before the
 *     call; the only library-held datum is the thread-local error string.  What used to be process-wide is now passed per
 *     call: the GEMM arithmetic mode is an argument of wsi_gemm_grouped, and the side stream the attention entry points
 *     use for hub nodes lives in a caller-owned wsi_context_t (one per device, or per thread; NULL = no side stream).
 */
#ifndef WSI_HGNN_H
#define WSI_HGNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WSI_OK        0
#define WSI_EINVAL  (-22)   /* bad argument (shape / alignment / null pointer) */
#define WSI_ENOSYS  (-38)   /* shape not supported by the compiled kernel set   */
#define WSI_EFAULT  (-14)   /* HIP runtime reported a launch error              */
#define WSI_ENOMEM  (-12)   /* caller-provided workspace too small              */

#define WSI_ABI_VERSION 26

int         wsi_abi_version(void);
const char* wsi_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Caller-owned execution context ("one context per device for multi-GPU processes").
 * Holds one non-blocking side stream + a fork/join event pair on the device that is current at creation.  The attention
 * entry points launch the few long-running hub-node workgroups on it, forked from and joined to the caller's stream with
 * events (every effect stays ordered on `stream` from the caller's point of view), so they run UNDER the main launch.
 * A context may be shared by threads (fork..join is serialised by a mutex inside it); pass NULL to run everything in
 * order on `stream`.  Destroy only after the work that used it has completed.
 */
typedef struct wsi_context wsi_context_t;
int  wsi_context_create(wsi_context_t** out);
void wsi_context_destroy(wsi_context_t* ctx);

/* ------------------------------------------------------------------------------------------------
 * HEAT relation attention (per-relation edge softmax + weighted neighbour sum + cross-relation mean)
 *
 * Replaces, for ALL relations of a layer in one launch:
 *   models/HEATNet4.py:103      ea = e_linear(sim)                               (a4)
 *   models/HEATNet4.py:109,111  apply_edges(fn.v_dot_u('q','k','t')) * ea / sqrt_dk   (DGL SDDMM, a5)
 *   models/HEATNet4.py:113      edge_softmax(sub_graph, score)                   (5 DGL kernels, a6)
 *   models/HEATNet4.py:118-119  multi_update_all(u_mul_e -> sum, cross_reducer='mean')  (DGL SpMM, a7)
 * (identically models/HEATNet2.py:78-94).
 *
 * Graph layout (two-level CSR by destination, see wsi-hgnn_amd/graph.py):
 *   node_seg[N+1] : relation-slot segments of dst node w are [node_seg[w], node_seg[w+1])
 *   rowptr[S+1]   : in-edges of segment s are [rowptr[s], rowptr[s+1])  (edge ids in "CSR order")
 *   src[E]        : global source node id of each edge, CSR order;  sim[E]: edge scalar, CSR order
 *   order[N]      : optional (may be NULL) processing order of dst nodes
 *   num_heavy     : 0, or the number of leading entries of `order` that hold the highest in-degree nodes (kNN hubs).
 *                   Those of them with more than 32 in-edges are processed by a cooperative instantiation of the kernel
 *                   (one workgroup per node: 8 waves x 4 gathered rows in flight instead of 1 x 2, partial softmax
 *                   states merged through LDS in a fixed order), launched ahead of the main one: a launch ends when its
 *                   longest serial gather chain ends, and a hub with hundreds of in-edges IS that chain.
 *                   Deterministic; differs from the single-wave order only in fp32 rounding.  Ignored by the generic kernels.
 * Tables: q/k/v rows of node i start at q + i*ldq (etc.); D = H*d_k floats per row.
 *   t[w, :]   = (1/#segments(w)) * sum_s sum_{e in s} softmax_s(score)[e,h] * v[src[e], h, :]
 *   score[e,h]= (q[w,h,:] . k[src[e],h,:]) * (e_weight*sim[e] + e_bias) / sqrt(d_k)
 * Saved for backward: score[E,H] (raw logits) and lse[S,H] (log-sum-exp per segment and head).
 * Specialised (coalesced 16-byte lane loads, DPP head reductions): D in {128,256,512} x H in {1,2,4,8,16} with
 * 16-byte aligned tables; any other D <= 1024, H <= 16, D % H == 0 runs a generic (slower) kernel; else WSI_ENOSYS.
 */
#define WSI_ATTN_XCD_CONTIGUOUS 1   /* flags: every XCD walks one contiguous eighth of `order` (workgroup b runs on XCD b % 8): for
                                      orders with locality (wsi-hgnn_amd/graph.py::apply_locality_order, kNN graphs) the rows gathered
                                      by the waves in flight on an XCD then share its 4 MiB L2; pointless (slightly negative) for
                                      random graphs, whose default order is heaviest-first */
#define WSI_ATTN_HUB_DEGREE(d) (((d) & 0xffff) << 8)   /* flags bits 8..23: in-degree above which a leading entry of `order` goes to the
                                      cooperative hub kernel (0 = 32); must be the threshold the caller used to choose num_heavy */
int wsi_heat_attn_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                      int32_t num_nodes, int32_t D, int32_t H,
                      const int32_t* node_seg, const int32_t* rowptr, const int32_t* src, const float* sim,
                      const int32_t* order, int32_t num_heavy, int32_t flags,
                      const float* e_weight, const float* e_bias,
                      float* t, int64_t ldt, float* score, float* lse,
                      uint32_t* t_absmax,   /* optional [N] (one part per row): receives the absmax bits (see wsi_gemm_group_t.a_absmax)
                                               of every row of t - the WSI_GEMM_FP16X3 scale of the projection that consumes t, for
                                               free while the row is in registers; NULL = not wanted */
                      wsi_context_t* ctx, void* stream);

/* Forward of a layer whose aggregate t is only read through per-segment sums (wsi_attn_pool_t): scores and softmax statistics only -
 * `score` [E, H] and `lse` [num_segs, H] exactly as wsi_heat_attn_fwd writes them; no v, no t.  Fast kernels only (D in {128, 256, 512}). */
int wsi_heat_attn_scores_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, int32_t num_nodes, int32_t D, int32_t H,
                             const int32_t* node_seg, const int32_t* rowptr, const int32_t* src, const float* sim,
                             const int32_t* order, int32_t num_heavy, int32_t flags, const float* e_weight, const float* e_bias,
                             float* score, float* lse, wsi_context_t* ctx, void* stream);

/* ctab[u, b, h] = sum over the out-edges e of source node u into destination node type b of exp(score[e,h] - lse[edge_seg[e],h]) / R_dst:
 * the coefficient with which v[u]_h enters the SUM of t over the (type b, graph of u) segment.  edge_seg[E]: softmax segment (row of lse) of
 * every CSR edge; CSC arrays and inv_rd as in wsi_heat_attn_bwd; row_seg / segs_per_type / n_types as in wsi_attn_pool_t. */
int wsi_heat_pool_coeff(const float* score, const float* lse, const int32_t* edge_seg,
                        const int32_t* colptr, const int32_t* csc_eid, const int32_t* csc_dst, const float* inv_rd,
                        const int32_t* row_seg, int32_t segs_per_type, int32_t n_types, int32_t H, int32_t num_src,
                        float* ctab, void* stream);

/* gtab[u, b, h] = h[u, :] . y[type(u), b * segs_per_type + graph(u), h, :] + beta[type(u), (same segment), h]  for every node row u: what an edge
 * from u into a destination of type b adds to pass 1's ga, per head (wsi_attn_pool_t.gtab).  chunk_row / chunk_seg: the readout plan's chunk tables
 * (a chunk = at most 128 rows of ONE (type, graph) segment, wsi_segment_reduce_bwd's arguments).  D in {128, 256, 512}; n_types * H * (D + 4) * 4 <= 64 KB. */
int wsi_heat_pool_gtab(const float* h, int64_t ldh, int32_t D, int32_t H, const float* y, const float* beta,
                       const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks,
                       int32_t segs_per_type, int32_t n_types, float* gtab, void* stream);

/*
 * Backward of the above (the autograd of DGL's SDDMM/SpMM/edge_softmax that loss.backward() reaches
 * from trainer/train_gnn.py:70).  Three deterministic, atomic-free passes; without a pool descriptor:
 *   pass A (src-major over CSC, gathers g_t; v[u] is the wave's own row):
 *                                  a[e,h] = exp(score - lse)  (written over `score`),
 *                                  ga[e,h] = (g_t[w]/R_w)[h,:] . v[u,h,:],  g_v[u] = sum a*g_t[w]/R_w
 *   pass 2 (dst-major, gathers k): delta, g_s = a*(ga-delta); g_q[w]; gsc[e,h] = g_s*ea/sqrt_dk;
 *                                  gea[e,h] = g_s * (q.k)/sqrt_dk
 *   pass C (src-major over CSC, gathers q): g_k[u] = sum gsc*q[w]
 * so that g_t, k and q each cross the fabric once per edge; with a pool descriptor (and in the generic kernels) pass 1 (dst-major,
 * gathers v or reads a table: a, ga) and pass 3 (src-major: g_k and, generic, g_v) take the place of A and C;
 * and a fixed-shape two-stage reduction  g_e_weight = sum gea*sim,  g_e_bias = sum gea.
 * Every row of gq/gk/gv is written (zeros for nodes without edges): no memset needed.
 *   colptr[num_src+1], csc_eid[E] (CSR edge id), csc_dst[E] (global dst): CSC by source ROW of the k/v tables
 *   (num_src = N for HEAT, where src[] holds global node ids; for HGT the k/v tables hold one row per
 *   (relation, source node) — models/HGT.py:92-97 — and src[] / the CSC index those stacked rows).
 *   inv_rd[N]: 1/#segments of each node.  order_dst/order_src: optional processing orders; num_heavy as in the forward
 *   (applies to passes 1 and 2, which walk order_dst).
 *   ga, gsc, gea: caller scratch, E*H floats each.  red_ws: >= 1024 floats, 8-byte aligned (the e_linear gradients are summed in float64: 512 partial sums).  g_e[2] = {g_weight, g_bias}.
 */
/* Optional descriptor for the backward of a layer whose output is read ONLY through a sum / mean readout over S = n_types * segs_per_type
 * segments of node rows (segment = node type * segs_per_type + graph; models/HEATNet4.py:219 after :128-135).  The gradient of t then
 * has S distinct rows (g_t / g_t_row), and g_v - a [N, D] matrix of rank <= S*H - is never formed: pass 3 writes, per source node u,
 *   ctab[u, b, h] = sum over u's out-edges e into destination type b of a[e, h] / R_dst      (the coefficients of g_v[u]_h = sum_b ctab * g_t[seg]_h)
 *   r_out[u, :]   = omg[type(u)] * g_row[seg(u), :] + sum_{b, h} ctab[u, b, h] * y[type(u), b * segs_per_type + graph(u), h, :]
 * i.e. the residual term of the K|Q|V dX epilogue with g_v W_v already added (y[tau, s, h, :] = (W_v^tau rows of head h)^T g_t[s]_h, a
 * [D] vector per source type, segment and head, prepared by the caller with one small grouped GEMM).  The caller gets dW_v from
 * wsi_segment_weighted_sums(h, ctab) and runs the dX / dW projections on the K and Q chunks only.  gv may be NULL.  Fast kernels only. */
typedef struct wsi_attn_pool {
    const int32_t* row_seg;      /* [N] */
    int32_t segs_per_type, n_types;       /* n_types <= 8 */
    const float* y;              /* [n_types][S][H][D] */
    const float* g_row;          /* [S][D]: gradient of every output row of the segment */
    const float* omg;            /* [n_types]: 1 - sigmoid(skip) of the type (1 where the layer passes h through) */
    float* r_out; int64_t ldr;   /* [N][D] */
    float* ctab;                 /* [N][n_types][H] */
    int32_t ctab_ready;          /* 1: ctab was filled by the forward (wsi_heat_pool_coeff); pass 3 reads it instead of binning again */
    const float* h; int64_t ldh; /* optional: the layer input [N][D].  With it the layer never computed V at all (forward: wsi_heat_attn_scores_fwd +
                                    wsi_heat_pool_coeff + weighted sums): pass 1 gathers h[src] and takes
                                    ga[e,h] = (h[src] . y[type(src), seg(dst), h, :] + beta[type(src), seg(dst), h]) / R_dst;  v may then be NULL */
    const float* beta;           /* [n_types][S][H]: g_t[seg]_h . b_v^tau (rows of head h); required with h */
    const float* gtab;           /* optional [N][n_types][H] from wsi_heat_pool_gtab: those dot products taken once per SOURCE node; pass 1 is then one
                                    flat per-(edge, head) lookup, ga[e,h] = gtab[src, type(dst), h] / R_dst, and gathers no row at all (h / beta unused) */
    const int32_t* edge_seg;     /* with gtab: [E] softmax segment (row of lse) of every CSR edge */
    const int32_t* seg_dst;      /* with gtab: [num softmax segments] destination node of the segment */
} wsi_attn_pool_t;

int wsi_heat_attn_bwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                      int32_t num_nodes, int32_t num_src, int32_t num_edges, int32_t D, int32_t H,
                      const int32_t* node_seg, const int32_t* rowptr, const int32_t* src, const float* sim,
                      const int32_t* colptr, const int32_t* csc_eid, const int32_t* csc_dst,
                      const float* inv_rd, const int32_t* order_dst, int32_t num_heavy, const int32_t* order_src, int32_t flags,
                      const float* e_weight, const float* e_bias,
                      const float* g_t, int64_t ldgt,
                      const int32_t* g_t_row, /* optional [N]: node w's gradient row is g_t[g_t_row[w]] - for a gradient with few DISTINCT
                                                 rows (the layer under a sum / mean readout gets one per (graph, node type)): the caller
                                                 passes that small table instead of N broadcast rows and pass 3's per-edge gathers of it
                                                 stay in the L2; NULL = row w of an [N, D] g_t */
                      const float* score,   /* the logits [E, H] the forward wrote (read only); NULL = they are in score_a (in place) */
                      float* score_a,       /* receives the attention probabilities exp(score - lse): E*H floats, may be the score buffer itself */
                      const float* lse,
                      float* ga, float* gsc, float* gea, float* red_ws,
                      float* gq, int64_t ldgq, float* gk, int64_t ldgk, float* gv, int64_t ldgv,
                      float* g_e,
                      uint32_t* g_absmax,   /* optional [max(N, num_src)][2] (two parts per row; zero it first): slot 0 of row r receives
                                               the absmax bits of gq[r], slot 1 those of gk[r] and gv[r] together - the row scale of a
                                               [N, 3D] g_k|g_q|g_v table that feeds one WSI_GEMM_FP16X3 dX projection; NULL = not wanted */
                      const wsi_attn_pool_t* pool,   /* optional, see above; NULL = the plain backward */
                      wsi_context_t* ctx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Grouped fp32 GEMM on the matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, k-ordered fma chain).
 *
 * Replaces the torch.nn.Linear calls of the path, grouped over node types in ONE launch:
 *   models/HEATNet4.py:202      adapt_ws[t](feat)                      (a2)
 *   models/HEATNet4.py:100-102  k/v/q_linears[t](h)  (deduplicated per node type)   (a3)
 *   models/HEATNet4.py:134-135  a_linears[t](t) + sigmoid-gated skip   (a8, fused epilogue)
 *   models/HEATNet4.py:219,243-245  linears_prediction / head_*        (a10)
 * and their autograd (dX = dY W, dW = dY^T X).
 *
 * op:  WSI_GEMM_NT  C[M,N] = A[M,K] * B[N,K]^T          (forward:  Y = X W^T)
 *      WSI_GEMM_NN  C[M,N] = A[M,K] * B[K,N]            (dX = dY W, W stored [out,in] = [K,N]); the
 *                   reduction may be split over up to 3 B matrices of `b_chunk` rows each (B, B1, B2):
 *                   dX = [dK|dQ|dV] * [W_k; W_q; W_v] in one launch without concatenating the weights
 *      WSI_GEMM_TN  C[M,N] = A[K,M]^T * B[K,N]          (dW = dY^T X; reduction over rows, split-K
 *                                                        through `workspace`, deterministic)
 * epilogue flags, applied in this order to x = sum_k a*b (s = sigmoid(*gate)):
 *      WSI_EPI_BIAS        x += bias[n]                                   (NT/NN)
 *      WSI_EPI_GELU        x  = gelu(x)   (exact erf form; models/HGT.py:180)   (NT/NN)
 *      WSI_EPI_MUL_M       x *= Mm[m,n]   (the nn.Dropout of models/HEATNet4.py:135 `self.drop(self.a_linears[..](t))`:
 *                                          Mm = keep mask / (1-p), drawn by the caller)           (NT/NN)
 *      WSI_EPI_SCALE_GATE  x *= s                                         (all ops)
 *      WSI_EPI_ADD_R       x += R[m,n] * (WSI_EPI_R_1MG ? (1-s) : 1)      (NT/NN)
 *      WSI_EPI_ACCUMULATE  x += C_old[m,n]                                (all ops)
 *   WSI_EPI_GATED_SKIP = BIAS|SCALE_GATE|ADD_R|R_1MG :  C = s*(x+bias) + (1-s)*R   (HEATNet4.py:128,135)
 *   A NULL `gate` in a group means s = 1 for that group.
 * Alignment: fastest path needs lda/ldb multiples of 4 elements and 16-byte aligned A/B; anything else
 * (odd strides, K tails, edge tiles) takes a guarded scalar-load path inside the same kernel.
 */
typedef struct wsi_gemm_group {
    const float* A;
    const float* B;
    float*       C;
    const float* bias;   /* [N] or NULL */
    const float* R;      /* residual [M,N] for ADD_R or NULL */
    const float* gate;   /* device scalar for SCALE_GATE / R_1MG, or NULL (s = 1) */
    const float* B1;     /* NN only: 2nd / 3rd chunk of the reduction dimension, or NULL */
    const float* B2;
    int64_t lda, ldb, ldc, ldr;
    int32_t M, N, K;
    int32_t b_chunk;     /* NN with B1/B2: rows of the reduction per B matrix (multiple of 32); else 0 */
    const float* Mm;     /* MUL_M: [M,N] multiplier with leading dimension ldm, else NULL */
    int64_t  ldm;
    float*   colsum_out; /* TN only, may be NULL: receives sum_k A[k][m] for m in [0,M) (x sigmoid(*gate) under SCALE_GATE,
                            added to its previous contents under ACCUMULATE, exactly like C): the bias gradient
                            colsum(dY) computed from the tiles the dW GEMM stages anyway */
    /* WSI_GEMM_FP16X3 scale exchange between producers and consumers on the path (pointers may be NULL; ignored by the
       other precisions).  "absmax bits" = the IEEE bit pattern of a max of |x| (unsigned compare = magnitude compare).  A
       row's scale is given as `parts` PARTIAL maxima, row-major [rows][parts]; the consumer takes their maximum - so every
       producer writes its own slot with a plain store (device-scope atomics cost more than the pass they would save). */
    const uint32_t* a_absmax; /* NT / NN: partial absmax bits of the M rows of A over its K columns, already known to the
                                 caller (written by the kernels that produced A): the call skips its own pass over A */
    uint32_t*       c_absmax; /* NT / NN: receives partial absmax bits of the rows of C this group writes (final values,
                                 after the epilogue): slot c_absmax_first + j of row m (at c_absmax[m * c_absmax_parts + ..])
                                 for j < wsi_gemm_absmax_parts(N); groups writing other column blocks of the same rows use
                                 other slots; slots nobody writes must hold 0 */
    int32_t a_absmax_parts;   /* slots per row of a_absmax (>= 1 when a_absmax is given) */
    int32_t c_absmax_parts;   /* slots per row of c_absmax (its row pitch) */
    int32_t c_absmax_first;   /* first slot this group writes */
    int32_t reserved;
    /* WSI_EPI_DROPOUT (NT / NN): the keep mask of nn.Dropout(p) as a FUNCTION of (seed, element) instead of a tensor - see wsi_dropout_keep below */
    uint32_t drop_seed;       /* the draw: one value per (layer, forward call) */
    uint32_t drop_threshold;  /* element kept iff its 16 hash bits >= drop_threshold = round(p * 65536); 0 keeps everything */
    float    drop_scale;      /* 1 / (1 - p) */
    int32_t  drop_row0;       /* row of the masked tensor that row 0 of this group's C is (the mask belongs to the tensor, not to the grouping) */
    int32_t  drop_cols;       /* columns of the masked tensor (its row pitch in the index space of the hash) */
    int32_t  drop_col0;       /* column of the masked tensor that column 0 of this group's C is */
    const uint32_t* drop_seed_base; /* optional DEVICE word added to drop_seed (mod 2^32) when the kernel runs: a step replayed as one hipGraph
                                       advances that word between replays and so draws new masks with the launch arguments frozen */
    /* COLUMN statistics exchange for the scaled-fp16 weight gradients (WSI_GEMM_TN under FP16X3 / AUTO).  Such a launch scales every COLUMN of
       A and of B by a power of two taken from the column's absmax over the group's K rows, and - with colsum_out - sums the columns of A.  Without
       the fields below it makes its own pass over both operands; a producer on the path that writes the tensor anyway can leave the statistics
       instead.  Layout: PARTIAL tables, row-major [parts][ld]: row p holds the statistic over SOME of the rows (a producer: one part per 128-row
       tile of its group, in row order); the consumer combines the parts in order (maxima: any order; sums: part 0 first - deterministic). */
    uint32_t*       c_colmax;    /* NT / NN: receives partial absmax bits of the COLUMNS of C (final values): part m / 128, columns 0 .. N of the
                                    group at c_colmax[part * c_col_ld + n]; NULL = not wanted.  Honoured only when wsi_gemm_writes_colstats says so */
    float*          c_colsum;    /* ... and the partial column sums, same layout, or NULL */
    int64_t         c_col_ld;
    const uint32_t* a_colmax;    /* TN: partial absmax bits of A's M columns over the K rows, [a_col_parts][a_col_ld], or NULL (own pass) */
    const float*    a_colsum;    /* TN with colsum_out: partial sums of A's columns, same layout, or NULL (own pass, over A again) */
    const uint32_t* b_colmax;    /* TN: the same for B's N columns, [b_col_parts][b_col_ld] */
    int64_t         a_col_ld, b_col_ld;
    int32_t         a_col_parts, b_col_parts;
    /* WSI_GEMM_FP16X3, NT / NN: B (the weights) already in the kernel's packed form - wsi_gemm_packed_b_bytes(N, K) bytes, 16-byte aligned, filled by
       wsi_gemm_pack_b from the SAME B / B1 / B2 / ldb / N / K / b_chunk - or NULL: the call packs B itself (one more launch per call).  Weights
       change only in the optimizer step: a trainer packs them all once behind it.  Ignored by the other precisions and by TN. */
    void*           b_packed;
} wsi_gemm_group_t;

#define WSI_GEMM_NT 0
#define WSI_GEMM_NN 1
#define WSI_GEMM_TN 2

#define WSI_EPI_BIAS        1
#define WSI_EPI_ACCUMULATE  2
#define WSI_EPI_SCALE_GATE  4
#define WSI_EPI_GELU        8
#define WSI_EPI_ADD_R       16
#define WSI_EPI_R_1MG       32
#define WSI_EPI_MUL_M       64
#define WSI_EPI_DROPOUT     256  /* x *= keep(seed, row, col) ? drop_scale : 0 at the position of MUL_M (NT/NN; not together with MUL_M): the nn.Dropout of
                                    models/HEATNet4.py:135 drawn INSIDE the epilogue from a counter-based generator - no mask tensor is written, read or kept
                                    for the backward, which regenerates it (wsi_dropout_apply) */
#define WSI_EPI_BACKGROUND  128  /* TN only; a launch hint, not arithmetic: at most ONE workgroup of this launch per CU, so that a memory-bound kernel
                                    the caller runs on another stream at the same time (the attention backward) keeps half of every CU's
                                    registers and LDS.  Results are bit-identical with or without it. */
#define WSI_EPI_GATED_SKIP  (WSI_EPI_BIAS | WSI_EPI_SCALE_GATE | WSI_EPI_ADD_R | WSI_EPI_R_1MG)

#define WSI_GEMM_MAX_GROUPS 24
#define WSI_GEMM_ABSMAX_PARTS(N) (2 * (((N) + 127) / 128))   /* slots a group of N output columns writes per row of c_absmax */

/* Arithmetic of one wsi_gemm_grouped call (`precision`; the reference has one knob of this kind too: torch's
 * `torch.backends.cuda.matmul.allow_tf32`, which trainer/train_gnn.py leaves at its fp32 default):
 *   WSI_GEMM_FP32   v_mfma_f32_32x32x2_f32: products and sums in IEEE fp32.
 *   WSI_GEMM_BF16X6 every fp32 operand is split exactly into 3 bf16 terms and x*y is summed in fp32 from the 6 largest
 *                   cross products on the bf16 matrix cores; per-product relative error <= ~2^-22, i.e. results agree
 *                   with the fp32 path to fp32 rounding noise (NOT a reduced-precision mode), at up to 16/6 the rate.
 *   WSI_GEMM_FP16X3 the same idea with half the matrix work.  NT / NN: every row of A and every output column of B - TN (weight gradients,
 *                   C = A^T B: the contraction runs over the rows): every COLUMN of A and of B, the absmax taken over the group's K rows
 *                   (a_colmax / b_colmax, or a pass of the call's own) - is
 *                   scaled by a power of two so that its largest element lies in [2^14, 2^15), split into 2 fp16 terms with
 *                   round-to-nearest at both levels (|x - x0 - x1| <= 2^-23 |x|: one bit short of fp32), the second one stored
 *                   times 2^11 so that both are normal fp16 numbers for every element within 2^-28 of its row's largest (smaller
 *                   ones are flushed: absolute error <= 2^-28 of the row's largest; an element 2^-d below the row's largest keeps
 *                   22 bits for d <= 17, 39 - d beyond); x*y is summed in fp32 from 3 products on the fp16 matrix cores (the
 *                   dropped x1*y1 is <= 2^-22 |x y|), the two cross products in an accumulator of their own that is folded in
 *                   with weight 2^-11; the scales are undone exactly (v_ldexp_f32) before the epilogue.  Per product the error is
 *                   <= 2^-21 |x y| (exact fp32: none, its error is 2^-24 per accumulation step): for K >~ 100 a dot product is as
 *                   accurate as fp32's (accumulation dominates: ::test_gemm_emulated_error_vs_fp32_mfma), for short ones the bound
 *                   allows 4x fp32's element-wise error (measured at K = 16 / 64 / 128: 0.97x / 0.37x / 0.52x of fp32's maximum, mean
 *                   1.3x at K = 16: ::test_gemm_fp16x3_short_dot_products); a large element that meets an exact zero exposes the
 *                   narrower window of the small ones (bound 2^-19 per product at d = 20; measured 2^-23.1 of the remaining sum at
 *                   K = 256, fp32 2^-21.6: ::test_gemm_fp16x3_outlier_times_zero).  NT / NN need workspace for the
 *                   absmax pre-pass and the packed planes of B (wsi_gemm_workspace_bytes says how much; 16-byte aligned).
 * A per-call argument, not library state: two callers in one process may use different modes concurrently. */
#define WSI_GEMM_FP32   0
#define WSI_GEMM_BF16X6 1
#define WSI_GEMM_FP16X3 2
#define WSI_GEMM_AUTO   3   /* the faster of the two fp32-class emulations for the launch's shape: FP16X3 when the launch is large
                               enough to amortise its pre-pass - NT / NN: >= 12 GFLOP in total and every K >= 384; TN: >= 30 GFLOP, every group >= 2048 rows;
                               on a large batch (a group of >= 24576 rows) NT / NN from 5 GFLOP and K >= 256, TN from 4 GFLOP with >= 8192 rows
                               per group; TN outputs at least 192 x 192 always -,
                               else BF16X6; c_absmax is honoured either way, so scales keep flowing between
                               mixed launches */

/* The counter-based dropout mask (WSI_EPI_DROPOUT).  Element (row, col) of a [rows, cols] tensor is KEPT iff
 *     bits16(fmix32((row * ceil(cols / 2) + col / 2) * 0x9E3779B1 + seed), col & 1) >= threshold        (fmix32 = MurmurHash3's 32-bit finaliser;
 * bits16(h, 0) = h & 0xffff, bits16(h, 1) = h >> 16; all arithmetic modulo 2^32): a pure function of (seed, row, col), so the forward's epilogue and the
 * backward regenerate the same mask, and a test can replay it on the host (wsi_hgnn_amd.ops.dropout_keep_mask).  Keep probability 1 - threshold / 65536.
 * seed = the call's seed argument + *seed_base (a device word, optional; see wsi_gemm_group_t.drop_seed_base).
 * wsi_dropout_apply: out[r, c] = keep ? x[r, c] * scale : 0 for the rows [row0, row0 + rows) of the masked tensor - the backward of the dropout
 * (g_y = g_out * mask) without a stored mask; in place when out == x. */
int wsi_dropout_apply(const float* x, int64_t ldx, float* out, int64_t ldo, int32_t rows, int32_t cols, int32_t row0, int32_t tensor_cols, int32_t col0,
                      uint32_t seed, const uint32_t* seed_base, uint32_t threshold, float scale, void* stream);

/* bytes of workspace wsi_gemm_grouped needs for this call (0 for NT/NN unless the launch runs scaled-fp16); same `precision` as the
 * call (the split-K plan depends on it). */
int64_t wsi_gemm_workspace_bytes(int32_t op, int32_t precision, const wsi_gemm_group_t* groups, int32_t ngroups);

/* absmax bits (one part per row, see wsi_gemm_group_t.a_absmax) of the rows of X[rows, cols]: for operands that do not change from
 * step to step (the input features of a resident graph, models/HEATNet4.py:202): taken once, handed to every projection as a_absmax */
int wsi_row_absmax(const float* x, int64_t ld, int32_t rows, int32_t cols, uint32_t* out, void* stream);

/* the arithmetic a call with these arguments runs in (resolves WSI_GEMM_AUTO): for
 * callers that account matrix-core work; < 0 on a bad precision */
int32_t wsi_gemm_kernel_precision(int32_t op, int32_t precision, const wsi_gemm_group_t* groups, int32_t ngroups);

int wsi_gemm_grouped(int32_t op, int32_t epilogue, int32_t precision, const wsi_gemm_group_t* groups, int32_t ngroups,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* The packed form of B for WSI_GEMM_FP16X3 NT / NN launches (wsi_gemm_group_t.b_packed): per output column the scale word (absmax over the
 * reduction), then the two scaled fp16 planes in MFMA fragment order.  wsi_gemm_pack_b fills b_packed of every group (fields read: B, B1, B2, ldb,
 * N, K, b_chunk) in ONE launch. */
int64_t wsi_gemm_packed_b_bytes(int32_t N, int32_t K);
int wsi_gemm_pack_b(int32_t op, const wsi_gemm_group_t* groups, int32_t ngroups, void* stream);

/* 1 when a wsi_gemm_grouped call with these arguments fills c_colmax / c_colsum of its groups (the LDS-DMA scaled-fp16 kernel of NT / NN launches
 * does; the other kernels leave the tables untouched), else 0: a caller asks before it hands the tables to a weight-gradient launch */
int32_t wsi_gemm_writes_colstats(int32_t op, int32_t precision, const wsi_gemm_group_t* groups, int32_t ngroups);

/* PARTIAL column statistics of X[rows, cols] in the layout of wsi_gemm_group_t.a_colmax / a_colsum: part p = rows [256 p, 256 p + 256), wsi_col_stats_parts(rows)
 * parts; part_max[p * part_ld + c] = bits(max |X[r, c]|), part_sum[p * part_ld + c] = sum X[r, c] (part_sum may be NULL); part_ld >= cols rounded up to 4,
 * tables 16-byte aligned.  For a weight-gradient operand whose producer leaves no statistics (the attention gradients): the caller runs it on a stream
 * of its own beside the matrix-bound projection that reads the same tensor, instead of letting the weight gradient make the pass in line. */
int32_t wsi_col_stats_parts(int32_t rows);
int wsi_col_stats(const float* x, int64_t ld, int32_t rows, int32_t cols, uint32_t* part_max, float* part_sum, int64_t part_ld, void* stream);

/* absmax bits of every COLUMN of X[rows, cols] over its rows (out[cols]; wsi_gemm_group_t.b_colmax with one part): for a weight-gradient operand
 * that does not change from step to step (the input features of a resident graph).  workspace: wsi_col_absmax_workspace_bytes(rows, cols). */
int64_t wsi_col_absmax_workspace_bytes(int32_t rows, int32_t cols);
int wsi_col_absmax(const float* x, int64_t ld, int32_t rows, int32_t cols, uint32_t* out, void* workspace, int64_t workspace_bytes, void* stream);

/* Both gradients of small Linear layers in ONE launch: dx[i]: dX = dY W (the WSI_GEMM_NN form, M <= 32 rows), dw[i]: dW = dY^T X with the bias
 * gradient in colsum_out (the WSI_GEMM_TN form, K <= 32 rows) - the backward of the classifier head behind the readout (head_2 / head_1 / head,
 * linears_prediction: models/HEATNet4.py:219,243-245; HEATNet2.py:183-190), whose levels are one row per graph.  Same group fields, same
 * fp32 fma chains in a fixed order as wsi_gemm_grouped takes for such shapes; n_dx + n_dw <= 16; epilogues: dx BIAS / ACCUMULATE / SCALE_GATE /
 * ADD_R / R_1MG, dw ACCUMULATE / SCALE_GATE.  WSI_ENOSYS when a group is not small (the caller then makes two wsi_gemm_grouped calls).  Groups
 * are validated as wsi_gemm_grouped validates them (a negative dimension, ADD_R without R: WSI_EINVAL) before anything is launched. */
int wsi_gemm_small_pair(const wsi_gemm_group_t* dx, int32_t n_dx, int32_t dx_epilogue,
                        const wsi_gemm_group_t* dw, int32_t n_dw, int32_t dw_epilogue, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Segmented row reduction: per-(graph, node type) readout and per-type bias gradients.
 *
 * Replaces dgl.readout.{mean,sum,max}_nodes behind
 *   pooling/avg_pooling.py:15-17, pooling/sum_pooling.py:14-16, pooling/max_pooling.py:15-17   (a9)
 * (called from models/HEATNet4.py:219).  Rows of a segment are contiguous.  Chunk tables (built once
 * per graph batch, see wsi-hgnn_amd/ops.py::ReducePlan) make the reduction two-stage and deterministic:
 *   chunk_row[C+1]  : chunk c covers rows [chunk_row[c], chunk_row[c+1]); chunks never straddle segments
 *   seg_chunk[S+1]  : chunks of segment s are [seg_chunk[s], seg_chunk[s+1])
 * op: 0 = sum, 1 = mean (empty segment -> 0), 2 = max (empty segment -> 0; argmax[S,D] receives the row).
 * partial: caller scratch, C*D floats (+ C*D int32 when op == max, placed after the floats).
 */
#define WSI_RED_SUM  0
#define WSI_RED_MEAN 1
#define WSI_RED_MAX  2

int wsi_segment_reduce_fwd(const float* x, int64_t ldx, int32_t D, int32_t op,
                           const int32_t* chunk_row, int32_t num_chunks,
                           const int32_t* seg_chunk, int32_t num_segs,
                           float* partial, float* out, int64_t ldo, int32_t* argmax, void* stream);

/* gx[r,:] = gout[seg(r),:] * (op==mean ? 1/count : 1)   (sum/mean);  max: scatter through argmax.
 * chunk_seg[C]: segment of each chunk.  For max, gx must be zero-filled by the caller. */
int wsi_segment_reduce_bwd(const float* gout, int64_t ldgo, int32_t D, int32_t op,
                           const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks,
                           const int32_t* seg_chunk, int32_t num_segs,
                           const int32_t* argmax, float* gx, int64_t ldgx, void* stream);

/* out[s, j, :] = sum_{r in segment s} w[r, j] * x[r, :]   (J weighted sums of the segment's rows; x [rows, D], w [rows, J] with row
 * stride ldw, out [num_segs, J, D] contiguous).  The weight-gradient side of wsi_attn_pool_t: with x = the layer input h, w = ctab and the
 * (source type, graph) segments this gives sum_u c[u, b, h] * h[u, :], from which dW_v is an [S]-deep product.  Same chunk tables as
 * wsi_segment_reduce_fwd; two-stage, deterministic.  partial: caller scratch, num_chunks * J * D floats. */
int wsi_segment_weighted_sums(const float* x, int64_t ldx, int32_t D, const float* w, int64_t ldw, int32_t J,
                              const int32_t* chunk_row, int32_t num_chunks, const int32_t* seg_chunk, int32_t num_segs,
                              float* partial, float* out, void* stream);

/* Bag softmax pooling (an addition to ABI 26): per segment s and score column c a softmax over the segment's rows, then the weighted sum
 * of the value rows.  Replaces F.softmax(A, dim=1) + torch.mm(A, H) of baselines/ReMix_DSMIL_ABMIL/model/abmil.py:25-28 and
 * F.softmax(A / sqrt(128), 0) + torch.mm(A^T, V) of model/dsmil.py:51-52, for many bags at once:
 *   p[r, c]      = exp(scale * scores[r, c] - lse[seg(r), c])
 *   out[s, c, :] = sum_{r in s} p[r, c] * values[r, :]            [num_segs, C, D] contiguous
 *   lse[s, c]    = logsumexp_{r in s}(scale * scores[r, c])       [num_segs, C]
 * scores [rows, C] with row stride lds, values [rows, D] with row stride ldv; chunk tables as for wsi_segment_reduce_fwd.  An empty segment
 * gives out = 0 and lse = 0.  1 <= C <= 8 (more: WSI_ENOSYS), any D >= 1; 16-byte row loads when values and ldv are 16-byte aligned, a
 * scalar path otherwise.  Two stages (an online softmax over the chunk's rows, then the segment's chunks combined in chunk order): values
 * is read once, no atomics, bit-reproducible.  partial: caller scratch, num_chunks * C * (D + 2) floats.
 * stats [num_segs, C, 2] (may be NULL): the two terms of lse apart - the segment's maximum of scale * scores and the log of the sum rescaled
 * by it (0, 0 for an empty segment).  The backward forms p from these: at scores near -1e4 their float32 sum has an ulp of 1e-3. */
int wsi_bag_softmax_pool_fwd(const float* scores, int64_t lds, int32_t C, float scale,
                             const float* values, int64_t ldv, int32_t D,
                             const int32_t* chunk_row, int32_t num_chunks, const int32_t* seg_chunk, int32_t num_segs,
                             float* partial, float* out, float* lse, float* stats, void* stream);

/* Its gradients, from g_out [num_segs, C, D] and the forward's out and stats (p[r, c] = exp((scale * scores[r, c] - stats[s, c, 0]) - stats[s, c, 1])):
 *   g_values[r, :] = sum_c p[r, c] * g_out[seg(r), c, :]
 *   g_scores[r, c] = scale * p[r, c] * (<g_out[s, c], values[r]> - <g_out[s, c], out[s, c]>)
 * Either gradient pointer may be NULL (that gradient is not computed; out and delta are needed for g_scores only).  values is read once and
 * g_values written once; no atomics, fixed summation order.  A segment whose g_out rows are zero gets exactly zero gradients.
 * delta: caller scratch, num_segs * C floats. */
int wsi_bag_softmax_pool_bwd(const float* g_out, const float* out, const float* scores, int64_t lds, int32_t C, float scale,
                             const float* stats, const float* values, int64_t ldv, int32_t D,
                             const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks, int32_t num_segs,
                             float* delta, float* g_scores, int64_t ldgs, float* g_values, int64_t ldgv, void* stream);

/* DSMIL's score step over many bags (torch.mm(Q, q_max^T), model/dsmil.py:50): scores[r, c] = <x[r, :], t[seg(r), c, :]> with
 * t [num_segs, C, D] contiguous; one launch whatever the number of bags.  1 <= C <= 8. */
int wsi_bag_scores_fwd(const float* x, int64_t ldx, int32_t D, const float* t, int32_t C,
                       const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks,
                       float* scores, int64_t lds, void* stream);

/* Its row gradient: gx[r, :] = sum_c w[r, c] * t[seg(r), c, :]  (+ sum_c w2[r, c] * t2[seg(r), c, :] when w2 and t2 are given: the
 * critical-instance gather's share, w2 = its one-hot rows).  The gradient of t is wsi_segment_weighted_sums(x, w). */
int wsi_bag_scores_bwd(const float* w, int64_t ldw, const float* t, const float* w2, int64_t ldw2, const float* t2,
                       int32_t C, int32_t D, const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks,
                       float* gx, int64_t ldgx, void* stream);

/* Global attention readout (an addition to ABI 26): dgl.nn.GlobalAttentionPooling over the rows of many segments at once - what
 * graph_pooling_type 'att' selects (models/HEATNet4.py:182-187 applied at :219, models/GCN.py), with the one-column gate_nn folded in:
 *   gate[r]   = <x[r, :], w> + bias[0]                                   [rows]
 *   p[r]      = softmax of gate over the rows of r's segment
 *   out[s, :] = sum_{r in s} p[r] * x[r, :]                              [num_segs, D] contiguous
 *   stats[s]  = (the segment's maximum gate, the log of the sum of e^(gate - maximum))   [num_segs, 2], kept apart for the reason
 *               wsi_bag_softmax_pool_fwd gives: at gates near -1e4 their float32 sum has an ulp of 1e-3
 * x [rows, D] with row stride ldx; w [D] and bias [1] are DEVICE pointers (bias may be NULL: 0); chunk tables as for wsi_segment_reduce_fwd
 * (empty chunks nobody owns - the padding of a slot's tables - are fine).  An empty segment gives out = 0 and stats = (0, 0).
 * 1 <= D <= 2048 (more: WSI_ENOSYS); 16-byte row loads when x and ldx are 16-byte aligned, a scalar path otherwise.  Two stages (per chunk an
 * online softmax with the row's dot product taken in the same pass over the row, then the segment's chunks combined in chunk order): x is read
 * once, no atomics, bit-reproducible.  partial: caller scratch, num_chunks * (D + 2) floats. */
int wsi_attn_readout_fwd(const float* x, int64_t ldx, int32_t D, const float* w, const float* bias,
                         const int32_t* chunk_row, int32_t num_chunks, const int32_t* seg_chunk, int32_t num_segs,
                         float* partial, float* out, float* gate, float* stats, void* stream);

/* Its gradients, from g_out [num_segs, D] contiguous and the forward's out, gate and stats (p[r] = exp((gate[r] - stats[s, 0]) - stats[s, 1])):
 *   delta[s]   = <g_out[s], out[s]>
 *   g_gate[r]  = p[r] * (<g_out[s], x[r]> - delta[s])
 *   g_x[r, :]  = p[r] * g_out[s, :] + g_gate[r] * w              [rows, D] with row stride ldgx; may be NULL: not computed, not written
 *   g_wb       = sum_r g_gate[r] * x[r, :]  |  sum_r g_gate[r]   [D + 1]: the gate's weight gradient, then its bias gradient
 * x is read once and g_x written once; g_wb is a per-chunk partial added in chunk order by a second launch - no atomics, fixed summation order.
 * A segment whose g_out row is zero gets exactly zero gradients.  The limits of D and the scalar path are the forward's.
 * scratch: caller scratch, num_segs + num_chunks * (D + 1) floats. */
int wsi_attn_readout_bwd(const float* g_out, const float* out, const float* gate, const float* stats,
                         const float* x, int64_t ldx, int32_t D, const float* w,
                         const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks, int32_t num_segs,
                         float* scratch, float* g_x, int64_t ldgx, float* g_wb, void* stream);

/* ReMix's bag reduction (an addition to ABI 26): ONE Lloyd iteration of a k-means over the rows of many bags at once - what faiss does per slide
 * for baselines/ReMix_DSMIL_ABMIL/reduce.py:18-19 (tools/clustering.py).  x [rows, D] with row stride ldx, the bags one after the other under the
 * chunk tables of wsi_segment_reduce_fwd (chunk_seg as for wsi_segment_reduce_bwd); centroids [num_segs, K, D] contiguous.  Per row
 *   xn    = normalize ? x / (|x|_2 + 1e-10) : x                (tools/clustering.py:42-44; a zero row stays zero)
 *   label = the first minimum over k of sum_c (xn[c] - centroid[k, c])^2
 * labels [rows] int32; objective [num_segs] = the sum of the winning squared distances; new_centroids [num_segs, K, D] = the mean of xn per label,
 * or NULL: assign only.  counts [num_segs, K] int32 = rows per label - with new_centroids given, AFTER the split of the empty clusters; they sum
 * to the bag's rows either way.
 * Empty clusters (faiss's split with a deterministic donor), for k upwards: the donor is the cluster with the largest current count (the lowest
 * index on a tie); centroid[k] = donor * (1 + e) on even columns and donor * (1 - e) on odd ones, the donor's centroid the opposite, e = 1 / 1024;
 * k takes donor_count / 2 of the count, the donor keeps the rest.
 * A bag with fewer than K rows (an empty one included) is legal: its labels are 0 and its counts, objective and new centroids are 0.
 * 1 <= K <= 16 (more: WSI_ENOSYS), any D >= 1; 16-byte row loads when x and ldx are 16-byte aligned, a scalar path otherwise; beyond D = 1024 a
 * slower kernel that re-reads a row from cache.  Two stages (a chunk's rows, then the bag's chunks in chunk order): x is read from memory once,
 * no atomics, bit-reproducible, and a bag's results do not depend on the other bags of the launch.
 * partial: caller scratch, num_chunks * K * (D + 2) floats. */
int wsi_bag_kmeans_step(const float* x, int64_t ldx, int32_t D, const float* centroids, int32_t K, int32_t normalize,
                        const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks,
                        const int32_t* seg_chunk, int32_t num_segs, float* partial,
                        int32_t* labels, int32_t* counts, float* objective, float* new_centroids, void* stream);

/* ReMix's mixing (train_remix_k-fold.py:71-107, mix_aug) over a bank of reduced bags protos [S, K, D] and its shift bank shifts [S, K, V, D]
 * (NULL: no WSI_REMIX_COV row), an addition to ABI 26.
 * wsi_remix_nearest: nearest[b, i] = the first minimum over j of |protos[src[b], i] - protos[tgt[b], j]|^2 for the B mixed bags of a step
 * (np.argmin(cdist(...), axis=1), line 75); 1 <= K <= 16.
 * wsi_remix_rows: out[o, :] for every output row of every mixed bag in ONE launch, from desc [rows, 8] int32 =
 *   [op, slot, src_row, partner, replaced, v, bits(lambda), bits(1 - lambda)]:  c = nearest[slot], tgt = protos[partner, c],
 *   cur = replaced ? tgt : protos.view(S * K, D)[src_row], and
 *     WSI_REMIX_KEEP         cur                                   (a row of the source bag, replaced or not)
 *     WSI_REMIX_APPEND       tgt
 *     WSI_REMIX_INTERPOLATE  (1 - lambda) * cur + lambda * tgt     (two rounded products, one rounded sum)
 *     WSI_REMIX_COV          cur + lambda * shifts[partner, c, v]
 *   A descriptor that points outside the bank gives a row of zeros and reads nothing. */
#define WSI_REMIX_KEEP        0
#define WSI_REMIX_APPEND      1
#define WSI_REMIX_INTERPOLATE 2
#define WSI_REMIX_COV         3
int wsi_remix_nearest(const float* protos, int32_t S, int32_t K, int32_t D, const int32_t* src, const int32_t* tgt, int32_t B,
                      int32_t* nearest, void* stream);
int wsi_remix_rows(const float* protos, const float* shifts, int32_t S, int32_t K, int32_t V, int32_t D,
                   const int32_t* nearest, int32_t num_slots, const int32_t* desc, int32_t rows, float* out, void* stream);

/* Patch dropout of many bags and the fill of a padded bag slot (an addition to ABI 26; mil.dropout_patches, mil.BagSlot).
 * The reference's dropout_patches (baselines/ReMix_DSMIL_ABMIL/train_tcga_k-fold.py:90-96) keeps k = int(n * (1 - p)) rows of a bag of n drawn
 * without replacement and appends m = int(n * p) of the kept rows again; the host computes k and m (mil.patch_counts).  The draw is the
 * project's own, from a 32-bit draw word d per bag, in uint32 arithmetic with fmix32 = MurmurHash3's finaliser and mask = 2^key_bits - 1:
 *   s1 = fmix32(d), s2 = fmix32(d ^ 0x85EBCA6B), key1(i) = fmix32(i * 0x9E3779B1 + s1) & mask, key2(i) = fmix32(i * 0x9E3779B1 + s2) & mask
 *   kept rows: the k rows i of [0, n) with the smallest (key1(i), i), in ascending i;  pad rows: the m kept rows with the smallest (key2(i), i),
 *   in ascending i.  A tie on a key goes to the lower row.  1 <= key_bits <= 32 (the package passes 32; fewer bits make ties common).
 * bag_desc (device): 8 int64 words per bag [src, stride, n, k, m, dst_row, draw, 0] - src = the bag's first source row (fp32, unit column
 * stride, `stride` floats from row to row), dst_row = its first row in the output.  Bags are listed by ascending dst_row, without gaps:
 * dst_row of the next bag = dst_row + k + m.
 * wsi_bag_dropout_select: sel[dst_row + j] = the source row (0-based within its bag) of output row j of every bag, j < k + m; one workgroup per
 * bag, one launch, no allocation, no read-back, the same result run after run, and a bag's rows do not depend on the other bags.  Nothing is
 * written at or beyond sel_rows; k > n and m > k are clamped. */
int wsi_bag_dropout_select(const int64_t* bag_desc, int32_t num_bags, int32_t key_bits, int32_t* sel, int64_t sel_rows, void* stream);

/* wsi_bag_slot_fill: rows[r, :feats] (row stride ld) for EVERY r < num_rows in one launch: the source row sel[r] of the bag that owns r (sel
 * NULL: the bag's rows in order, k = n and m = 0), zeros for a row no bag owns or a source row outside [0, n).  16-byte accesses when rows, ld,
 * feats and the bag's src / stride allow, a scalar path otherwise (per bag).  row_seg (may be NULL): row_seg[r] = the owning bag, filler_seg
 * for the rest.  small_words int32 words are copied from small_src to small_dst (both device; 0: none): the host-built small tables of a slot,
 * which travel behind the descriptors in the same upload. */
int wsi_bag_slot_fill(const int64_t* bag_desc, int32_t num_bags, const int32_t* sel, float* rows, int64_t ld, int32_t feats,
                      int64_t num_rows, int32_t* row_seg, int32_t filler_seg,
                      const int32_t* small_src, int32_t* small_dst, int32_t small_words, void* stream);

/* One Adam step over `count` parameter tensors in ONE launch: the optimizer step of the reference's trainer (torch.optim.Adam(lr, weight_decay),
 * parser.py:33-38; trainer/train_gnn.py:72) with torch's arithmetic, amsgrad = False, maximize = False:
 *   g += weight_decay * p;  m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * `step` = the 1-based step count AFTER this step (torch increments before use).  p, m, v are updated in place; contiguous fp32 tensors.
 * It is wsi_optim_step(WSI_OPTIM_ADAM) below with a host count (s0 = m, s1 = v, no `step` word, host_step = step) under the drop-in signature:
 * the same kernel, 88 non-empty tensors per launch, and like it every tensor is checked before the first launch (WSI_EINVAL leaves nothing stepped). */
typedef struct wsi_adam_tensor { float* p; const float* g; float* m; float* v; int64_t n; } wsi_adam_tensor_t;
int wsi_adam_step(const wsi_adam_tensor_t* tensors, int32_t count, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int64_t step, void* stream);      /* (hyper-parameters in double, as torch holds them: 1 - beta2 is taken in double) */

/* The other optimizers parser.parse_optimizer can build (parser.py:15-46: Adagrad, Adadelta, SGD for anything else) and an Adam whose step
 * count lives on the device, each in ONE launch over all `count` tensors (more than the kernel's table holds: several launches; zero-element
 * tensors are skipped).  fp32 arithmetic per element in torch.optim's order, scalar factors taken in double:
 *   WSI_OPTIM_SGD       g += wd p;  momentum != 0: buf = (flags & WSI_OPTIM_FIRST) ? g : momentum buf + (1 - dampening) g,
 *                       g = nesterov ? g + momentum buf : buf;  p -= lr g                            (s0 = buf; NULL when momentum == 0)
 *   WSI_OPTIM_ADAGRAD   g += wd p;  sum += g^2;  p -= lr / (1 + (t - 1) lr_decay) * g / (sqrt(sum) + eps)                     (s0 = sum)
 *   WSI_OPTIM_ADADELTA  g += wd p;  sq = rho sq + (1 - rho) g^2;  d = sqrt(acc + eps) / sqrt(sq + eps) * g;
 *                       acc = rho acc + (1 - rho) d^2;  p -= lr d                                                  (s0 = sq, s1 = acc)
 *   WSI_OPTIM_ADAM      wsi_adam_step's arithmetic                                                           (s0 = exp_avg, s1 = exp_avg_sq)
 * t is the 1-based count AFTER this step.  A tensor with `step` != NULL keeps it on the device (a 0-dim fp32 word, torch's capturable layout):
 * the launch reads t - 1 from it and leaves t there, which is what lets a captured graph replay the step; `ticket` is an int32 word of the
 * caller's, zero before the first call and left zero by every call (the workgroups of a tensor count themselves through it: the last one
 * stores the new count).  With `step` == NULL, t = hyper->host_step.  SGD and Adadelta never read t but advance a `step` word they are given.
 * `nesterov` is 0 or 1 and needs momentum > 0 and dampening == 0, as torch demands. */
#define WSI_OPTIM_SGD      0
#define WSI_OPTIM_ADAGRAD  1
#define WSI_OPTIM_ADADELTA 2
#define WSI_OPTIM_ADAM     3
#define WSI_OPTIM_FIRST    1   /* flags: this tensor's first step under SGD with momentum (s0 is written, not read) */
typedef struct wsi_optim_tensor {
    float* p; const float* g; float* s0; float* s1;
    float* step; int32_t* ticket; int64_t n; int32_t flags;
} wsi_optim_tensor_t;
typedef struct wsi_optim_hyper {
    double lr, weight_decay, momentum, dampening, nesterov, lr_decay, eps, rho, beta1, beta2, host_step;
} wsi_optim_hyper_t;
int wsi_optim_step(int32_t rule, const wsi_optim_tensor_t* tensors, int32_t count, const wsi_optim_hyper_t* hyper, void* stream);

/* wsi_optim_step with a per-tensor GATE read on the device (an addition to ABI 26; optim._OneLaunch.gate).  gate_index: HOST array
 * of `count` words (NULL: nobody is gated), gate_index[i] = 0: tensor i has no gate, k in 1..gate_len: its gate word is gate_table[k - 1], a
 * DEVICE float table of gate_len <= 255 words that every workgroup of the tensor reads when the launch runs.  A tensor whose gate word is 0.0 is
 * left alone: p, s0, s1, its `step` word and its `ticket` word stay bit for bit as they were (its workgroups return before they load, store or
 * take a ticket) - what torch does to a parameter whose gradient is None.  Any other gate word, or no gate: wsi_optim_step's arithmetic, bit
 * for bit.  wsi_optim_tensor_t and wsi_optim_step are unchanged; a rule that reads t takes a gated tensor with a `step` word only (a host count
 * would advance whether the tensor was stepped or not). */
int wsi_optim_step_gated(int32_t rule, const wsi_optim_tensor_t* tensors, int32_t count, const wsi_optim_hyper_t* hyper,
                         const int32_t* gate_index, const float* gate_table, int32_t gate_len, void* stream);

/* wsi_optim_step_gated with the LEARNING RATE read on the device (an addition to ABI 26; optim.lr_word).  lr_word == NULL: exactly
 * wsi_optim_step_gated.  Otherwise lr_word is an 8-byte aligned DEVICE pointer to one double, read when the launch runs (lane 0 of every
 * workgroup loads it next to the count and forms from it in double, in the host's order, what is made of lr: the (float)lr of SGD and
 * Adadelta, Adam's step_size, Adagrad's clr); hyper->lr is then ignored and not range-checked, and neither host nor kernel checks the word, as
 * torch checks no tensor lr.  With the double v in the word every output bit (p, s0, s1, step and ticket words) equals those of the same
 * call with lr_word == NULL and hyper->lr == v.  A rule that reads t takes a word only with a `step` word per tensor: a host count has its
 * factors taken on the host, which cannot read the word (WSI_EINVAL; torch's tensor lr needs capturable=True for the same reason).  The word
 * is written by the caller on the same stream between launches (a fill_), never by the library.  The gate arguments as above (NULL, NULL, 0:
 * nobody is gated). */
int wsi_optim_step_lr(int32_t rule, const wsi_optim_tensor_t* tensors, int32_t count, const wsi_optim_hyper_t* hyper,
                      const int32_t* gate_index, const float* gate_table, int32_t gate_len, const double* lr_word, void* stream);

/* Mean cross entropy of logits [B, C] against int64 labels and its gradient factor in ONE launch (torch.nn.CrossEntropyLoss() with its
 * defaults, parser.py:182-183, applied at trainer/train_gnn.py:67):  *loss = mean over the VALID rows b of (logsumexp(logits[b]) - logits[b, y_b]);
 * dlogits[b, c] = (softmax(logits[b])[c] - [c == y_b]) / #valid  (the caller multiplies it by the incoming gradient of the loss).
 * A label equal to -100 (torch's default ignore_index) is ignored as torch ignores it: zero gradient row, not counted (no valid row: loss = NaN).
 * Any other label outside [0, C) (torch: a device assert) zeroes its gradient row, turns *loss into NaN and sets *bad_label (optional) to 1 -
 * every element of dlogits is written in every case.  B * C <= 65536. */
int wsi_cross_entropy(const float* logits, const int64_t* labels, int32_t B, int32_t C, float* loss, float* dlogits, int32_t* bad_label, void* stream);

/* out[s] = sum_{r in segment s} sum_c g[r,c] * (a[r,c] - b[r,c])   — the reduction behind d(loss)/d(skip) of
 * the sigmoid-gated residual `alpha*y + (1-alpha)*h` (models/HEATNet4.py:128,135; autograd of torch.sigmoid /
 * broadcasting mul in the reference).  Same chunk tables as wsi_segment_reduce_fwd; two-stage, deterministic.
 * partial: caller scratch, num_chunks * ceil(D/256) floats. */
int wsi_segment_dot_diff(const float* g, int64_t ldg, const float* a, int64_t lda, const float* b, int64_t ldb,
                         int32_t D, const int32_t* chunk_row, int32_t num_chunks,
                         const int32_t* seg_chunk, int32_t num_segs,
                         float* partial, float* out, void* stream);

/* d(loss)/d(skip) of a HEAT layer (models/HEATNet4.py:128,135: `alpha = sigmoid(skip[n_id])`, `alpha * y + (1 - alpha) * h`) in two launches:
 *   g_skip[gate] = (1 - sigmoid(skip[gate])) * sum over the segments s with seg_gate[s] == gate of  sum_{r in s} g[r,:] . (a[r,:] - b[r,:])
 * = wsi_segment_dot_diff followed by the gate map and the sigmoid factor (the alpha factor of d sigmoid is already in g . (a - b) = g . alpha (y - h)).
 * seg_gate[s] < 0: the segment's node type has no gated output (passed through).  Every entry of g_skip [n_gates] is written.  num_segs <= 8192.
 * partial: caller scratch, num_chunks * ceil(D/256) floats. */
int wsi_gate_grad(const float* g, int64_t ldg, const float* a, int64_t lda, const float* b, int64_t ldb,
                  int32_t D, const int32_t* chunk_row, int32_t num_chunks, const int32_t* seg_chunk, int32_t num_segs,
                  const int32_t* seg_gate, const float* skip, int32_t n_gates, float* partial, float* g_skip, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The S-row algebra of a HEAT layer under a sum / mean readout (see wsi_attn_pool_t; no single reference call site: the LAST HEATLayer,
 * models/HEATNet4.py:213-214, together with pools[0] at :219).  T node types, H heads, dk = D / H, Bg graphs, S = T * Bg segments numbered
 * type * Bg + graph.  Plain fp32 sums in a fixed order.
 *
 * wsi_pool_factors: from the per-source coefficients w = ctab [rows, T * H] (column b * H + hh: destination type b, head hh) and x = the layer
 *   input h, over the SOURCE segments (tau, g) of the chunk tables (numbered tau * Bg + g):
 *     hp[b * Bg + g][hh][tau][:] = sum_u w[u, b * H + hh] * x[u, :]          ([S][H][T][D]: the T source types of a destination segment side by side)
 *     csum[tau][b * Bg + g][hh]  = sum_u w[u, b * H + hh]                    ([T][S][H])
 *     x_mean[tau * Bg + g][:]    = the mean of the segment's rows of x   (optional, [S][D]: the same pass with one more weight column of ones - the
 *                                  layer needs mean_seg(h) as well and would otherwise read h once more)
 *   partial: caller scratch, num_chunks * (T * H + 1) * (D + 1) floats.
 * wsi_pool_tmean: t_mean[s, c] = scale[s] * ( sum_tau tpart[tau, s, c] + sum_tau csum[tau, s, c / dk] * bv[tau][c] ) - the segment means of the
 *   aggregate t from the per-source-type partial products tpart [T][S][D] (hp through W_v) and the value biases; bv: HOST array of T device
 *   pointers ([D] each, NULL = no bias); scale [S] or NULL.
 * wsi_pool_bwd_prep: the head of the layer's backward from the gradient of its pooled output g_pool [S, D] (op = WSI_RED_SUM / WSI_RED_MEAN,
 *   counts [S] = rows per segment as floats, z_mean / h_mean [S, D] = segment means of the never-formed output and of the input):
 *     g_row = gradient of every output row of the segment, g_sum = ... summed over the segment's rows,
 *     g_skip[gate] = (1 - sigmoid(skip[gate])) * sum_{s: seg_gate[s] == gate} g_sum[s,:] . (z_mean[s,:] - h_mean[s,:]),
 *     omg[i] = 1 - sigmoid(skip[type_gate[i]]) (1 where type_gate[i] < 0: the layer passes that type through).   S <= 8192.
 * wsi_pool_bwd_bias: beta[tau, s, hh] = gt_seg[s, head hh] . bv[tau][head hh]  and  gbv[tau, c] = sum_s csum[tau, s, c / dk] * gt_seg[s, c]
 *   (wsi_attn_pool_t.beta and the gradient of the value biases); either output may be NULL. */
int wsi_pool_factors(const float* x, int64_t ldx, int32_t D, const float* w, int64_t ldw, int32_t T, int32_t H, int32_t Bg,
                     const int32_t* chunk_row, int32_t num_chunks, const int32_t* seg_chunk,
                     float* partial, float* hp, float* csum, float* x_mean, void* stream);
int wsi_pool_tmean(const float* tpart, int32_t T, int32_t S, int32_t D, int32_t H, const float* csum, const float* const* bv,
                   const float* scale, float* t_mean, void* stream);
int wsi_pool_bwd_prep(const float* g_pool, int32_t S, int32_t D, int32_t op, const float* counts, const float* z_mean, const float* h_mean,
                      const int32_t* seg_gate, const float* skip, int32_t n_gates, const int32_t* type_gate, int32_t T,
                      float* g_row, float* g_sum, float* g_skip, float* omg, void* stream);
int wsi_pool_bwd_bias(const float* gt_seg, int32_t T, int32_t S, int32_t D, int32_t H, const float* const* bv, const float* csum,
                      float* beta, float* gbv, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Segment descriptor tables (csrc/segment_table.hip): tables written from pieces in ONE launch.  desc: DEVICE array of int64, nsegs rows of 10 words
 *   [out, in1, in2, tab_off, key, add, stride, n, mode, block_start]
 * followed by the lookup tables the tab_off's index (in words from desc; tab_off < 0: none).  Segment s writes n elements:
 *   mode 0 (int32 out):  out[i] = (in1 ? in1[i] : 0) + add + i * stride + (tab_off >= 0 ? desc[tab_off + key + (in2 ? in2[i] : 0)] : 0)     (in1, in2: int64)
 *   mode 1  4-byte copy out[i] = in1[i]                                      mode 2  4-byte fill with the low 32 bits of add
 *   mode 3 (int32 out):  out[i] = desc[tab_off + key + i]                    mode 4 (int64 out):  out[i] = desc[tab_off + key + i]
 *   mode 5 (16-byte elements, both pointers 16-byte aligned):  out[i] = in1[i], or zero when in1 is NULL (the feature rows)
 *   modes 10 / 11 / 13 (int32 out): rowptr of the filler's segments / src of its edges / colptr of its sources, for node type `key`, by index
 *   arithmetic from the filler block at desc + tab_off: [T, then per node type: nf, ef, first filler node, first filler CSR edge, source type of
 *   relation slot 0, relation slots, first filler CSC entry] (csrc/slot_math.h; the filler graph: graph.filler_graph)
 *   mode 14 (int32 out): out[i] = add + stride * (local destination of the filler's i-th edge into node type `key`)
 *   mode 12: element i = the filler's i-th edge into node type `key`; writes its CSC entry into the WHOLE tables out (csc_eid) and in1 (csc_dst)
 * block_start = number of 1024-element blocks of the segments before it (segments with n = 0 are not listed); total_blocks = their sum.
 * No allocation, no synchronisation, no read-back; everything on `stream`.  Host side: graph.SegmentTable.
 *
 * wsi_plan_assemble - kernel plan of a block-diagonal batch (`dgl.batch` + `g.to(device)` in front of every step of a loader-fed run:
 * trainer/train_gnn.py:48-65): every table of the batch's plan (rowptr, colptr, src, csc_eid, csc_dst, sim, the processing orders, node_seg,
 * inv_rd) is a concatenation of per-graph pieces with per-piece offsets.  Accepts modes 0-2.
 *
 * wsi_slot_fill - fill of a padded batch slot (data.BatchSlot): plan, readout tables, labels and type-major features of "the real slides, empty
 * graphs up to the slot's capacity, one filler graph" written into caller-owned STATIC buffers, so that a step captured over them replays over
 * every batch that fits.  Accepts every mode. */
int wsi_plan_assemble(const int64_t* desc, int32_t nsegs, int32_t total_blocks, void* stream);
int wsi_slot_fill(const int64_t* desc, int32_t nsegs, int32_t total_blocks, void* stream);

/* Which node types the REAL slides of a filled batch slot hold (an addition to ABI 26; data.BatchSlot(type_mask=...)):
 *   out[t] = 1.0 if seg_nonempty[t * graphs + b] != 0 for some b < b_cap, else 0.0                                    (t < T)
 * seg_nonempty: the slot's readout table, float [T * graphs] with segment t * graphs + b (graphs 0 .. b_cap - 1 are the real slides and the
 * empty graphs behind them, the rest the filler), as wsi_slot_fill and wsi_slot_aug_* have just written it on `stream`.  One wave, plain
 * loads and stores, no atomics, no read-back; every word of out [T] is written.  1 <= T, 0 <= b_cap <= graphs. */
int wsi_type_present(const float* seg_nonempty, int32_t T, int32_t graphs, int32_t b_cap, float* out, void* stream);

/* GraphConv's degree norms of a homogeneous slot (an addition to ABI 26; models/GCN.py: dgl GraphConv(norm='both')), re-derived behind every
 * fill as wsi_type_present is: in_norm[i] = max(rowptr[i + 1] - rowptr[i], 1) ** -0.5 and out_norm[i] = max(colptr[i + 1] - colptr[i], 1) ** -0.5
 * for the n nodes of the slot, the filler's included (rowptr: one segment per node - one relation; colptr: the CSC pointer; n + 1 words each).
 * One launch, no read-back; the reciprocal square root is taken in double and rounded once, which is what ``clamp(min=1).pow(-0.5)`` on a
 * float32 device tensor gives (models/GCN.py HomoPlan): the same bits. */
int wsi_degree_norms(const int32_t* rowptr, const int32_t* colptr, int32_t n, float* in_norm, float* out_norm, void* stream);

/* The live rows of a homogeneous slot (an addition to ABI 26; one node type, so readout segment = graph; models/GIN.py's BatchNorm, DESIGN
 * 3.33), re-derived behind every fill as wsi_type_present is:
 *   live[i] = row_seg[i] < b_cap ? 1.0 : 0.0 for the n rows (the filler's rows are dead; the empty graphs have none), and
 *   live_rows[0] = seg_counts[0] + ... + seg_counts[b_cap - 1], added in index order by one lane (integers below 2^24: exact).
 * row_seg int32 [n] and seg_counts float [graphs]: the slot's readout tables as wsi_slot_fill / wsi_slot_aug_* have just written them on
 * `stream`.  One launch, plain loads and vector stores, no atomics, no read-back; every word of live [n] and live_rows [1] is written, and
 * n == 0 still writes live_rows.  0 <= n, 0 <= b_cap <= graphs. */
int wsi_slot_live_rows(const int32_t* row_seg, const float* seg_counts, int32_t n, int32_t graphs, int32_t b_cap,
                       float* live, float* live_rows, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row-wise kernels of the HGT / GCN siblings of the path.
 *
 * wsi_layernorm_*: torch.nn.LayerNorm(out_dim) per node type, models/HGT.py:57 (creation), :124 (use).
 *   row_param[r] (may be NULL = 0) selects the gamma/beta row (node type -> norms[n_id]); gamma/beta are [P, D].
 *   stats[n,2] receives (mean, rstd) for backward.  bwd also writes xhat_gy = gy * xhat [n,D] whose per-type
 *   column sums are d(gamma) (d(beta) = column sums of gy) — reduce them with wsi_segment_reduce_fwd.
 * wsi_gelu_*: F.gelu after the input projection, models/HGT.py:180, models/HetRGCN.py:98 (exact erf form).
 * wsi_spmm_sum: the copy_u -> sum message passing + degree norms + bias + ReLU of dgl.nn.pytorch.GraphConv
 *   (norm='both'), models/GCN.py:30-33 / models/GCN_NTPool.py:34-37:
 *     out[w] = act(oscale[w] * sum_{e in [ptr[w], ptr[w+1])} edge_w[e] * iscale[idx[e]] * x[idx[e]] + bias)
 *   (edge_w: optional per-edge weight in the order of idx - the explicit edge_weight of PyG's GCNConv / LEConv in pooling/ASAP.py:45-61,157; NULL = 1)
 *   forward: (ptr, idx) = CSR by destination; backward: CSC by source with the scales swapped.  relu_ref
 *   (may be NULL): rows of x are masked by relu_ref[idx] > 0 before being summed (ReLU backward fused in).
 *   Any D <= 1024.
 * wsi_sddmm_dot: the gradient of wsi_spmm_sum's forward with respect to edge_w (GNNExplainer's per-edge message scale through GraphConv,
 *   explainers/gnn_explainer.py:21-33), for every CSR entry e = (u -> w), u = src[e], e in [rowptr[w], rowptr[w+1]):
 *     g_w[e] = oscale[w] * iscale[u] * sum_c gm[w,c] * x[u,c],   gm[w] = g[w] where relu_ref[w] > 0 (relu_ref NULL: gm = g)
 *   g = gradient of spmm_sum's out, x = its input, relu_ref = its out when relu was fused.  One gather of x[u] per edge; g[w] is held by
 *   the lane group that owns w.  g_w[E] fp32 in CSR order; no atomics.  Any D <= 1024. */
int wsi_layernorm_fwd(const float* x, int64_t ldx, int32_t n, int32_t D, float eps,
                      const float* gamma, const float* beta, const int32_t* row_param,
                      float* y, int64_t ldy, float* stats, void* stream);
int wsi_layernorm_bwd(const float* gy, int64_t ldgy, const float* x, int64_t ldx, int32_t n, int32_t D,
                      const float* gamma, const int32_t* row_param, const float* stats,
                      float* gx, int64_t ldgx, float* xhat_gy, int64_t ldp, void* stream);
int wsi_gelu_fwd(const float* x, float* y, int64_t n, void* stream);
int wsi_gelu_bwd(const float* x, const float* gy, float* gx, int64_t n, void* stream);
int wsi_spmm_sum(const float* x, int64_t ldx, int32_t n_out, int32_t D,
                 const int32_t* ptr, const int32_t* idx, const float* edge_w, const float* iscale, const float* oscale,
                 const float* bias, int32_t relu, const float* relu_ref, int64_t ldref,
                 float* out, int64_t ldo, void* stream);
int wsi_sddmm_dot(const float* g, int64_t ldg, const float* x, int64_t ldx, int32_t n, int32_t D,
                  const int32_t* rowptr, const int32_t* src, const float* iscale, const float* oscale,
                  const float* relu_ref, int64_t ldref, float* g_w, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Graph-construction edge step: L2 kNN + per-edge Pearson correlation.  The kNN is an exact
 * re-ranking (wsi_pair_stats) of a shortlist (wsi_knn_select) whose membership is reliable down to neighbour gaps of about
 * slack = 8 e, e = the absolute fp32 error of the key sqnorm[j] - 2 dots[i,j] (a few ulp of |x|^2; about 4e-4 at 1024
 * columns and |x|^2 = 350): a returned distance exceeds the exact one at its position by at most slack.
 *
 * Replaces, behind wsi-hgnn_amd/construct.py::construct_graph,
 *   construct_graph/graph_constructor.py:265-273   Hnsw(space='l2').fit(features); query(features[v], topn=radius)[1:]
 *   construct_graph/graph_constructor.py:276-282   scipy.stats.pearsonr(features[a], features[b])[0] per edge, type = corr > 0
 *
 * wsi_row_sqnorm : out[i] = sum_c x[i,c]^2.
 * wsi_knn_select : `dots` = rows [row0, row0+rows) of X X^T (ld = ldd, N columns; from wsi_gemm_grouped NT).  For every
 *                  row writes the kc (<= 32) columns j != row0+i with the smallest sqnorm[j] - 2 dots[i,j] (i.e. the
 *                  smallest |x_i - x_j|^2 up to the GEMM's rounding), ascending, ties -> smaller j; -1 pads when N-1 < kc.
 *                  A column whose key is +inf (an overflowed norm) is never listed; -1 stands in its place.
 * wsi_pair_stats : for every row i and each of its kc (<= 64) candidates j (entries < 0 are skipped): exact
 *                  d2 = sum (x_i-x_j)^2 and Pearson r from centred sums (NaN if either vector is constant, i.e. every
 *                  element equals the first, as scipy tests it); keeps the `keep` candidates with the smallest (d2, j),
 *                  ascending, into nbr / dist2 / corr [n, keep].  With fewer than `keep` valid candidates the remaining
 *                  slots are not written (caller pre-fills nbr with -1).
 */
int wsi_row_sqnorm(const float* x, int64_t ldx, int32_t n, int32_t F, float* out, void* stream);
int wsi_knn_select(const float* dots, int64_t ldd, const float* sqnorm, int32_t row0, int32_t rows, int32_t N,
                   int32_t kc, int32_t* cand, void* stream);
int wsi_pair_stats(const float* x, int64_t ldx, int32_t n, int32_t F, const int32_t* cand, int32_t kc, int32_t keep,
                   int32_t* nbr, float* dist2, float* corr, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Edge kernels of ASAPPooling (pooling/ASAP.py:142-199).
 *
 * Edges are grouped by the node i that aggregates them: ptr[n+1], idx[E] = gathered node j of each edge in that
 * ("CSR") order; the backward passes that reduce onto j use the CSC of the same edge numbering
 * (colptr[n+1], csc_eid[E] = CSR position, csc_dst[E] = aggregating node).  One wave per node, any D <= 1024,
 * no atomics (replaces torch_scatter's atomic scatter_max / scatter_add and PyG's softmax).
 *
 * wsi_csr_gather_max_fwd : pooling/ASAP.py:158,163  X_q = scatter_max(x_pool[j], i):  out[i,c] = max_e x[idx[e],c],
 *                          arg[i,c] (int32 [n,D]) = CSR position of the first maximum; empty group -> 0 / -1.
 * wsi_csr_gather_max_bwd : gx[j,c] = sum of g_out[i,c] over the edges whose arg[i,c] is that edge.
 * wsi_asap_attend_fwd    : pooling/ASAP.py:167-179 with gat_att(cat(M_q[i], x_pool[j])) pre-split into per-node scalars
 *                          a[i] (includes the bias) and b[j]:  s_e = leaky_relu(a[i] + b[j], negative_slope);
 *                          score[e] = exp(s_e - max_i) / (sum_i exp + 1e-16)   (torch_geometric.utils.softmax);
 *                          out[i,:] = sum_e score[e] * x[idx[e],:].   score is in CSR order.
 * wsi_asap_attend_bwd    : from g_out: g_a[n], g_b[n], gx[n,D]; gpre[E] is caller scratch (receives d loss / d pre-activation).
 */
int wsi_csr_gather_max_fwd(const float* x, int64_t ldx, int32_t n, int32_t D, const int32_t* ptr, const int32_t* idx,
                           float* out, int64_t ldo, int32_t* arg, void* stream);
int wsi_csr_gather_max_bwd(const float* g_out, int64_t ldg, const int32_t* arg, int32_t n_src, int32_t D,
                           const int32_t* colptr, const int32_t* csc_eid, const int32_t* csc_dst,
                           float* gx, int64_t ldgx, void* stream);
int wsi_asap_attend_fwd(const float* a, const float* b, const float* x, int64_t ldx, int32_t n, int32_t D,
                        const int32_t* ptr, const int32_t* idx, float negative_slope,
                        float* score, float* out, int64_t ldo, void* stream);
int wsi_asap_attend_bwd(const float* a, const float* b, const float* x, int64_t ldx, int32_t n, int32_t D,
                        const int32_t* ptr, const int32_t* idx,
                        const int32_t* colptr, const int32_t* csc_eid, const int32_t* csc_dst, float negative_slope,
                        const float* score, const float* g_out, int64_t ldg,
                        float* gpre, float* g_a, float* g_b, float* gx, int64_t ldgx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-head GAT attention (models/GAT.py:17-92, DGL GATConv; H heads of width D, F = H*D, 1 <= H <= 16, 1 <= F <= 4096).
 *
 * Homogeneous edge layout of the relation-attention plan: rowptr[n+1] / src[E] = CSR by destination (edge id = CSR position),
 * colptr[n+1] / csc_eid[E] / csc_dst[E] = CSC by source over the same edge ids; order_dst / order_src (optional, NULL = node
 * order) = the walk orders.  Rows are head-major: column h*D + d.  No atomics, fixed summation orders: bit-reproducible.
 *
 * wsi_gat_scores   : eler[n, 2H] <- el | er,  el[v,h] = sum_d ft[v,h,d] attn_l[h,d],  er likewise with attn_r.
 * wsi_gat_attn_fwd : s_e = leaky_relu(el[u] + er[v], negative_slope);  a = softmax of s over v's in-edges (max-subtracted, NO
 *                    epsilon);  a~ = a * keep(e, h) / (1 - p)  (attn_drop: the counter-based mask of wsi_dropout_apply over an
 *                    [E, H] tensor, row = CSR edge id, column = head; drop_threshold 0 = no dropout);
 *                    out[v] = act(sum_e a~_e ft[u] + bias)  (bias optional; activation 0 none, 1 relu, 2 leaky_relu(act_slope));
 *                    lse[n, 2H] <- the log-sum-exp of the scores in two parts: lse[v, h] = max_e s_e (+inf for a node without
 *                    in-edges: out = act(bias) there), lse[v, H + h] = log sum_e exp(s_e - max); a_e = exp((s_e - max) - log_sum).
 *                    Nothing per edge is stored: the backward recomputes a from eler and lse.
 * wsi_gat_attn_bwd : from g_out (gradient of out) and the forward's eler / lse / out (out read only when activation != 0) and the
 *                    SAME dropout arguments: g_ft[n, F] <- d loss / d ft (both through the aggregation and through el / er),
 *                    g_attn_l[F], g_attn_r[F], g_bias[F] (optional) <- the parameter gradients.  workspace: at least
 *                    wsi_gat_attn_bwd_workspace_bytes(n, E, H, D, activation) bytes (-1 for bad arguments), 16-byte aligned (else WSI_EINVAL).
 * wsi_gat_attn_fwd_scaled / wsi_gat_attn_bwd_scaled : the same with a per-edge message scale edge_scale[E] (fp32, CSR edge order, one value
 *                    for all heads and columns of the edge; any finite value - GNNExplainer passes sigmoid(edge_mask),
 *                    explainers/gnn_explainer.py:21-33).  The scale multiplies the message AFTER the softmax (and after attn_drop):
 *                      out[v] = act(sum_e a~_e s_e ft[u] + bias);  lse as above (the softmax does not see s).
 *                    Backward, with r[e,h] = g_rst[w]_h . ft[u]_h  (g_rst = g_out * act'(out)):
 *                      g_ft[u] = sum_e a~_e s_e g_rst[w] (+ the el / er terms);  d loss / d a~_{e,h} = s_e r[e,h];
 *                      g_edge_scale[e] = sum_h a~_{e,h} r[e,h]   (E fp32, CSR order; heads added in order by one lane: no atomics).
 *                    Same workspace size as the unscaled backward.  The unscaled entry points do not run this code.
 */
int wsi_gat_scores(const float* ft, int64_t ldf, int32_t n, int32_t H, int32_t D, const float* attn_l, const float* attn_r,
                   float* eler, void* stream);
int wsi_gat_attn_fwd(const float* ft, int64_t ldf, const float* eler, int32_t n, int32_t H, int32_t D,
                     const int32_t* rowptr, const int32_t* src, const int32_t* order_dst, float negative_slope,
                     uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_threshold, float drop_scale,
                     const float* bias, int32_t activation, float act_slope, float* out, int64_t ldo, float* lse, void* stream);
int64_t wsi_gat_attn_bwd_workspace_bytes(int32_t n, int32_t E, int32_t H, int32_t D, int32_t activation);
int wsi_gat_attn_bwd(const float* ft, int64_t ldf, const float* eler, const float* lse, const float* out, int64_t ldo,
                     const float* g_out, int64_t ldg, int32_t n, int32_t E, int32_t H, int32_t D,
                     const int32_t* rowptr, const int32_t* src, const int32_t* colptr, const int32_t* csc_eid,
                     const int32_t* csc_dst, const int32_t* order_src, const float* attn_l, const float* attn_r,
                     float negative_slope, uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_threshold,
                     float drop_scale, int32_t activation, float act_slope, void* workspace, int64_t workspace_bytes,
                     float* g_ft, int64_t ldgf, float* g_attn_l, float* g_attn_r, float* g_bias, void* stream);
int wsi_gat_attn_fwd_scaled(const float* ft, int64_t ldf, const float* eler, int32_t n, int32_t H, int32_t D,
                            const int32_t* rowptr, const int32_t* src, const int32_t* order_dst, float negative_slope,
                            uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_threshold, float drop_scale,
                            const float* bias, int32_t activation, float act_slope, const float* edge_scale,
                            float* out, int64_t ldo, float* lse, void* stream);
int wsi_gat_attn_bwd_scaled(const float* ft, int64_t ldf, const float* eler, const float* lse, const float* out, int64_t ldo,
                            const float* g_out, int64_t ldg, int32_t n, int32_t E, int32_t H, int32_t D,
                            const int32_t* rowptr, const int32_t* src, const int32_t* colptr, const int32_t* csc_eid,
                            const int32_t* csc_dst, const int32_t* order_src, const float* attn_l, const float* attn_r,
                            float negative_slope, uint32_t drop_seed, const uint32_t* drop_seed_base, uint32_t drop_threshold,
                            float drop_scale, int32_t activation, float act_slope, const float* edge_scale,
                            void* workspace, int64_t workspace_bytes, float* g_ft, int64_t ldgf, float* g_attn_l, float* g_attn_r,
                            float* g_bias, float* g_edge_scale, void* stream);

/* wsi_graph_topk : pooling/ASAP.py:184  perm = topk(fitness, ratio, batch)  (torch_geometric.nn.pool.topk_pool.topk).
 *                  score[n] fp32, batch[n] int64 graph id of every node (any arrangement; ids in [0, num_graphs)),
 *                  out_start[num_graphs+1] int64 = exclusive prefix of the per-graph counts k_b = ceil(ratio * n_b) (caller),
 *                  perm[out_start[num_graphs]] int64 out: graph by graph, the k_b highest-scoring nodes of graph b in descending
 *                  score order, equal scores in node order.  Rank-by-counting through LDS tiles: exact, deterministic, no sort. */
int wsi_graph_topk(const float* score, const int64_t* batch, int32_t n, int32_t num_graphs,
                   const int64_t* out_start, int32_t* rank_ws /* caller scratch, n int32 */, int64_t* perm, void* stream);

/* wsi_stas : pooling/ASAP.py:68-117  E = S^T A S of graph_connectivity (A = the edge weights, 1 when edge_weight=None - the only way the class
 *            is called), replacing torch_sparse.spspmm x2 + coalesce x4.  Same edge layout as the attention kernels: CSR by centre
 *            (rowptr/idx, score[E] in that order = the attention scores of wsi_asap_attend_fwd) and CSC by neighbour (colptr /
 *            csc_eid / csc_dst).  perm[kN] = selected centres (wsi_graph_topk), n_idx[n] = pooled index of a node or -1.
 *            fill = 0: row_count[kN] <- number of distinct columns c2 != c1 of every row (0 and *overflow = 1 for a row with more
 *                      than 1536 of them: the caller falls back to its sparse-matrix path);
 *            fill = 1: row_start[kN+1] (exclusive prefix of row_count) in, out_col/out_val[row_start[kN]] <- columns ascending and
 *                      values of every row (rows ascending = coalesced COO order); unit self loops are NOT included (:113-115).
 *            Values are sums of score*score products accumulated in 2^-40 fixed point with integer atomics: order-independent,
 *            hence bit-reproducible, and within 2^-41 per term of the exact sum. */
int wsi_stas(int32_t fill, int32_t kN, const int64_t* perm, const int32_t* n_idx,
             const int32_t* rowptr, const int32_t* idx, const float* score, const float* edge_w /* optional [E], CSR order: the values of A (NULL = 1) */,
             const int32_t* colptr, const int32_t* csc_eid, const int32_t* csc_dst,
             int32_t* row_count, const int64_t* row_start, int64_t* out_col, float* out_val, int32_t* overflow, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Train-time graph augmentation (data.py:16-23,116-117: Compose([DropNode(0.5), DropEdge(0.5), NodeShuffle(), FeatMask(0.5, ['feat'])]) through
 * dgl.transforms, applied to every TRAINING graph each time it is loaded).  Host side: wsi-hgnn_amd/transforms.py, ops.augment_graph.
 *
 * The draw contract (beside the dropout contract above; same fmix32, same 16-bit threshold = round(p * 65536), all arithmetic modulo 2^32).
 * One call of a pipeline has ONE 32-bit draw seed.  Transform number k of the pipeline (0 for a transform called on its own), acting on
 * stream j, uses the sub-seed
 *     sub(seed, k, j) = fmix32(fmix32(seed + (k + 1) * 0x9E3779B1) + (j + 1) * 0x85EBCA6B)
 * and element i of that stream the hash  h(i) = fmix32(i * 0x9E3779B1 + sub):
 *     DropNode   stream j = index of the node type in g.ntypes,          i = node id;       node i is REMOVED iff (h(i) & 0xffff) < threshold
 *     DropEdge   stream j = index of the relation in g.canonical_etypes, i = edge position; edge i is REMOVED iff (h(i) & 0xffff) < threshold
 *     NodeShuffle stream j = index of the node type,                     i = node id;       perm = stable argsort of the 32-bit keys h(i)
 *                (equal keys in index order); every node field x becomes x[perm]
 *     FeatMask   stream j = 65536 * (position of the field name in its list) + (32768 for an edge field) + index of the type / relation,
 *                i = feature column;  column i is ZEROED iff (h(i) & 0xffff) < threshold
 * i always counts in the graph THE TRANSFORM RECEIVES: behind DropNode, DropEdge indexes the surviving edges of a relation in their (stable)
 * order and NodeShuffle the surviving nodes.  Probability of removal = threshold / 65536 (p quantised to 1/65536; p = 1 removes everything).
 * A pure function of (seed, k, j, i): the CPU formulation in transforms.py and these kernels produce the same graph bit for bit.
 *
 * Segment descriptors: DEVICE int64 tables, one row per node type / relation, in order.  A segment of n elements owns ceil(n / 1024) TILES;
 * first_tile = tiles of the segments before it; ntiles = their total.  Outputs of a segment are written at its OWN offset `off` (capacity n):
 * no output position depends on another segment's count, and none on an atomic: two-level exclusive scans, stable order, reproducible.
 *
 * wsi_augment_nodes : rows of 6 words [n, off, first_tile, sub-seed, threshold, quota + 1].  new_id[off + i] <- new id of node i of the type
 *                     (survivors keep their order) or -1; kept[off + r] <- old id of the type's r-th survivor; counts[s] <- survivors of
 *                     segment s.  tile_sum: scratch, ntiles + 1 int32.  Last word 0: no quota.  Last word q + 1: of the nodes the draw
 *                     keeps only the first q (node-id order) stay, the others get new_id -1 exactly as if drawn, counts[s] <- min(kept, q);
 *                     the tile sums (and tile_sum[ntiles]) stay those of the DRAW.  A quota the draw does not reach changes nothing.
 * wsi_augment_edges : rows of 14 words [n, off, first_tile, u, v, sim, src_off, dst_off, sub-seed, threshold, mode, n_src, n_dst, quota + 1]; u, v: device
 *                     pointers to the relation's int64 endpoints (local ids), sim: to its fp32 edge scalar or 0; src_off / dst_off: offsets of
 *                     the endpoint types in new_id (new_id NULL: no node was removed).  Stage 1 keeps the edges whose endpoints both survive
 *                     (an endpoint outside [0, n_src) / [0, n_dst) removes the edge) and ranks them; mode 0 draws DropEdge by the edge's
 *                     ORIGINAL position (DropEdge in front of DropNode), mode 1 by that rank (behind it); threshold 0: no DropEdge.
 *                     out_u / out_v [off + r] <- renumbered endpoints of the relation's r-th final survivor, out_sim its sim, out_eid its original
 *                     position; counts[s] <- final survivors.  tile_sum: scratch, 2 * (ntiles + 1) int32; rank1: scratch, one int32 per edge.
 *                     Last word 0: no quota; rank1 keeps the stage-1 rank.  Last word q + 1: only the first q final survivors (input order) are
 *                     written, counts[s] <- min(final, q), and rank1[off + i] ends as -1 for EVERY edge that is not among them (by either
 *                     draw or by the quota), its stage-1 rank otherwise; the second half of tile_sum stays the draw's.
 * wsi_augment_keys  : rows as for wsi_augment_nodes (threshold unused): keys[off + i] <- (segment << 32) | h(i): ONE stable ascending sort of
 *                     keys orders every node type at once.
 * wsi_gather_rows_masked : out[i, c] = zeroed(c) ? 0 : x[row_of[i], c] for i < rows, c < F  (row_of NULL: row i; an index outside
 *                     [0, src_rows) gives a zero row; zeroed(c) = (fmix32(c * 0x9E3779B1 + mask_seed) & 0xffff) < mask_threshold, 0 = no mask):
 *                     DropNode's compaction, NodeShuffle's permutation (composed into row_of) and FeatMask in ONE pass over the surviving
 *                     rows.  One wave per row, 16 bytes per lane and access when F % 4 == 0 and both tables are 16-byte aligned with strides
 *                     that are multiples of 4; any other width / alignment takes an element-per-lane path.
 *                     Traffic: rows * F * 4 bytes read + rows * F * 4 written + rows * 8 of indices. */
int wsi_augment_nodes(const int64_t* desc, int32_t nseg, int32_t ntiles, int32_t* tile_sum, int32_t* new_id, int64_t* kept,
                      int32_t* counts, void* stream);
int wsi_augment_edges(const int64_t* desc, int32_t nseg, int32_t ntiles, const int32_t* new_id, int32_t* tile_sum, int32_t* rank1,
                      int64_t* out_u, int64_t* out_v, float* out_sim, int64_t* out_eid, int32_t* counts, void* stream);
int wsi_augment_keys(const int64_t* desc, int32_t nseg, int32_t ntiles, int64_t* keys, void* stream);
int wsi_gather_rows_masked(const float* x, int64_t ldx, int64_t src_rows, const int64_t* row_of, float* out, int64_t ldo, int64_t rows,
                           int32_t F, uint32_t mask_seed, uint32_t mask_threshold, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Leave-one-node-out batches (explainers/GEM.py:31-50, explainers/gem_het.py:30-39: the model is run on the graph WITHOUT node r, once per node).
 * Host side: graph.leave_one_out_tables / graph.leave_one_out_batch, ops.leave_one_out_batch.  Copy b of the batch is the graph without node r_b
 * of ONE node type t; the result equals graph.batch([graph.remove_nodes(g, [r_b], t) for b]) value for value.  The host knows every copy's
 * surviving edge count in advance (per-node out-degree, in-degree and self-loop count of each relation, read back ONCE per graph and type), so every
 * output offset is exact and a call needs no device->host read.  Entry points added to ABI 26.
 *
 * Descriptors: DEVICE int64 tables with tiles as for wsi_augment_* (a row of n input elements owns ceil(n / 1024) tiles, first_tile = tiles of the
 * rows before it, ntiles = their total).
 *
 * wsi_loo_edges : rows of 12 words [n, off, first_tile, u, v, sim, r_src, r_dst, add_src, add_dst, cap, 0], one per (relation j, copy b), relation-major
 *                 and copy-major inside a relation.  n: edges of the relation; u, v: device pointers to its int64 endpoints (local ids); sim: to its
 *                 fp32 edge scalar or 0; r_src = r_b when the source type is t, else INT64_MAX (never equal, never below an id), r_dst likewise.
 *                 Edge i survives iff u[i] != r_src && v[i] != r_dst.  The row's p-th survivor (input order) is written at off + p:
 *                 out_u <- u - (u > r_src) + add_src, out_v <- v - (v > r_dst) + add_dst (add = b * nodes of that type per copy), out_eid <- i,
 *                 out_sim <- sim[i] (rows with sim only).  cap = the count the host predicted for the row: a survivor with p >= cap is NOT written,
 *                 so a row never leaves its range.  counts[row] <- survivors found (== cap unless the host's tables are wrong).
 *                 tile_sum: scratch, ntiles + 1 int32.  Count per tile, one-block scan, stable scatter: no atomics, bit-reproducible.
 * wsi_loo_rows  : rows of 6 words [n, off, first_tile, per, is_t, 0], one per node type: per = nodes of the type in ONE copy, n = ncopies * per.
 *                 row_of[off + b * per + i] <- i + (is_t && i >= removed[b])   (removed: DEVICE int64 [ncopies], the r_b): the source row of every node
 *                 of the batch, for wsi_gather_rows_masked (threshold 0) and plain indexing. */
int wsi_loo_edges(const int64_t* desc, int32_t nrow, int32_t ntiles, int32_t* tile_sum, int64_t* out_u, int64_t* out_v, float* out_sim,
                  int64_t* out_eid, int32_t* counts, void* stream);
int wsi_loo_rows(const int64_t* desc, int32_t nrow, int32_t ntiles, const int64_t* removed, int32_t ncopies, int64_t* row_of, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fill of a padded batch slot with AUGMENTED slides (data.BatchSlot over a loader with transform=; graph.slot_fill_augmented): the tables
 * wsi_slot_fill writes, for the batch [transform(slide_0, draw_0), .., empty graphs, filler], from survivor counts that stay on the device - no
 * read-back, no synchronisation, no atomics, no allocation; a launch count that depends on neither the draw nor the pipeline.  Entry points
 * added to ABI 26.  A stored slide's plan pieces are in CSR order and DropNode renumbers monotonically, so the augmented slide's pieces are
 * stable compactions of the stored ones; the processing orders are the stored order lists restricted to the survivors (a processing order
 * changes no result), the filler's nodes behind them.
 *
 * Sequence of one fill, all on `stream`: wsi_augment_nodes over the rows at off_node (B * T rows, (slide, type), slide-major; counts = ncnt),
 * wsi_augment_edges over the rows at off_edge (B * R rows, (slide, relation); rank1 = rank1, new_id = new_id), wsi_slot_aug_keys, ONE stable
 * ascending sort of keys whose indices are perm, wsi_slot_aug_scan, wsi_slot_aug_write.
 *
 * desc: ONE device int64 table; the off_* fields are word offsets into it.
 *   off_node   wsi_augment_nodes rows;  off_edge  wsi_augment_edges rows (slide b's rows cover ITS concatenated COO: off = coo_base[b] + ...)
 *   off_flag   nflag rows of 8 words [n, off, first_tile, kind, p0, p1, slide, 0] (tiles of 1024 as for wsi_augment_*; off into frank):
 *              kind 0: p0 = int64 [n], entry i = (relation << 40) | index of the entry's edge in the slide's concatenated COO - kept iff the edge
 *              survives;  kind 1: p0 / p1 = int64 [n] local id / node type of an order list's entry - kept iff the node survives.
 *              Rows, in order: CSR edges into (b, t) at [b T + t], CSC entries out of (b, t) at [B T + b T + t], then per slide its
 *              heavy-destination, light-destination and source order lists at [2 B T + b], [2 B T + B + b], [2 B T + 2 B + b]: nflag = 2 B T + 3 B.
 *   off_push   npush rows of 10 words [n, first_block, kind, slide, type, p0, p1, p2, p3, flag row] (blocks of 1024; rows with n = 0 not listed):
 *              kind 0 nodes of (b, t): p0 = stored rowptr piece (int64 [n R]), p1 = stored colptr piece;  kind 1 CSR edges into (b, t): p0 = src_l,
 *              p1 = src_t, p2 = sim (fp32), p3 = local softmax segment node * R + slot;  kind 2 CSC entries out of (b, t): p0 = eid_l, p1 = ent_t,
 *              p2 = dst_l;  kinds 3 / 4 / 5 the slide's heavy / light / source order list: p0 = local id, p1 = node type (all int64 but sim)
 *   off_feat   B * T rows of 3 words [fp32 feature table of (b, t), its rows, FeatMask's sub-seed]
 *   off_shape  the shape block of csrc/slot_layout.h: [T, B, b_cap, chunk, c_cap, per type: n_cap, e_cap, type_off, ebase, src_type, R, seg_off]
 *   off_misc   noff[B T] (offset of (b, t) in new_id / kept / keys / perm), stored rows [B T], coo_base[B], labels[G], NodeShuffle sub-seeds [B T]
 * ns_mode: 0 no NodeShuffle, 1 in front of DropNode (or no DropNode): perm over the stored nodes, 2 behind it: over the survivors - positions at
 * or beyond the survivors' count carry a key above every real one.  mask_thr: FeatMask's threshold (0: none).  feat_aligned: every feature
 * table is 16-byte aligned (with F % 4 == 0: 16-byte accesses; else the element path).
 * Scratch (caller-owned): new_id int32 / kept int64 / keys int64 / perm int64 [nodes_stored], ncnt int32 [B T], rank1 int32 [COO edges],
 * ftile int32 [flag_tiles + 1], frank int32 [flag entries], fcnt int32 [nflag], L int64 [4 B T + 9 T + 3 B + 2] (slot_layout.h).
 * wsi_slot_aug_scan: flags -> ranks and counts (three launches), then the layout kernel: L, readout_ptr, the readout's chunk tables and
 * segment counts, labels.  wsi_slot_aug_write: the real slides push, the filler and tails are pulled, the features are gathered (three launches);
 * every element of every table is written by every fill (scales: wsi_row_absmax over feat afterwards).
 * Survivor quotas (data.BatchSlot(quota=)): the last word of the rows at off_node / off_edge carries quota + 1.  A kind-0 flag entry
 * whose relation row has a quota is kept iff rank1 >= 0 (the final decision, left there by wsi_augment_edges); without one the by-rank draw is
 * re-derived from rank1 as before.  The slot's capacities may then be below the stored counts: every (slide, type) / (slide, relation) count is
 * clamped where it is produced, and every scattered store of wsi_slot_aug_write is range-checked against its table (N, S, E).
 * wsi_slot_aug_quota(node_rows, nnode, tsum_n, edge_rows, nedge, etiles, tsum_e, overflow): one single-thread launch behind the two
 * augmentation calls of a fill, reading the tile sums they leave (tsum_n [ntiles + 1], tsum_e [2 (etiles + 1)]): the draw's survivors of every
 * row minus its quota.  overflow: DEVICE int64 [3], zeroed by its owner once: [0] += 1 when some quota bound in this fill, [1] / [2] <- max with
 * the largest node / edge excess.  Plain loads and stores, ordered by the stream.  Entry point added to ABI 26.
 * args: a HOST array of 55 int64 words, read during the call (pointers as integers), the same for the three calls:
 *   [0] desc   [1..7] off_node, off_edge, off_flag, off_push, off_feat, off_shape, off_misc   [8..14] B, T, R, N, S, E, G (= b_cap + 1)
 *   [15..23] nflag, flag_tiles, npush, push_blocks, nodes_stored, ns_mode, F, mask_thr, feat_aligned
 *   [24..33] scratch: new_id, kept, ncnt, rank1, ftile, frank, fcnt, keys, perm, L
 *   [34..54] the slot's tables: rowptr, colptr, node_seg, src, csc_eid, csc_dst, order_dst, order_src, sim, inv_rd, readout_ptr, labels, feat,
 *            edge_seg, row_seg, chunk_row, chunk_seg, seg_chunk, seg_counts, seg_inv_counts, seg_nonempty */
int wsi_slot_aug_keys(const int64_t* args, void* stream);
int wsi_slot_aug_scan(const int64_t* args, void* stream);
int wsi_slot_aug_write(const int64_t* args, void* stream);
int wsi_slot_aug_quota(const int64_t* node_rows, int32_t nnode, const int32_t* tsum_n, const int64_t* edge_rows, int32_t nedge, int32_t etiles,
                       const int32_t* tsum_e, int64_t* overflow, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Epoch metrics kept on the device (wsi_hgnn_amd/metrics.py::EpochMetrics): the reference's per-epoch accuracy / precision / recall / F1 / AUC and
 * mean cross entropy (trainer/train_gnn.py:73-79,104-108; evaluator/eval_homo_graph.py:61-95; utils.py:37-47) without a read-back per step.
 * Entry points added to ABI 26.  No allocation, no synchronisation, nothing a hipGraph cannot record; counts are integers and every float sum
 * has one order, so the buffers hold the same bits run after run.
 *
 * The accumulator (caller-owned, zeroed by the caller to reset it):
 *   state       int32 [WSI_METRICS_STATE_HEAD + C * C], 8-byte aligned: [0] cursor n (rows stored), [1] flag bits (WSI_METRICS_*), [2..3] the fp64
 *               sum of the stored rows' cross entropies, then the confusion matrix, conf[label * C + prediction]
 *   probs       fp32 [capacity, C]   row_labels, row_preds  int64 [capacity]
 *
 * wsi_metrics_update: ONE launch, one workgroup.  logits [B, C] fp32, labels int64 [B]; C <= 32, B * C <= 65536 (as wsi_cross_entropy).  For every
 * row in row order: a label of -100 skips the row before its logits are read (a padding graph may carry anything); any other label outside
 * [0, C) skips it and sets WSI_METRICS_BAD_LABEL; a non-finite logit skips it and sets WSI_METRICS_NONFINITE; a row that would land at or past
 * `capacity` is dropped and sets WSI_METRICS_OVERFLOW (nothing is written past the capacity).  A counted row writes, at the cursor, its softmax
 * probabilities (maximum subtracted, precise expf / logf), its label and its prediction (the FIRST maximum of its logits), adds 1 to conf and its
 * cross entropy to the fp64 sum (a fixed tree per 256 rows, those in order), and advances the cursor.
 *
 * wsi_metrics_finalize: two launches over the n stored rows.  pair_partials: scratch, int64 [C * ceil(capacity / 256) * 2].
 *   result      fp64 [WSI_METRICS_RESULT_HEAD + 4 * C]:
 *               [0] n  [1] flag bits  [2] accuracy  [3] mean cross entropy  (n = 0: NaN)
 *               [4..7]   'binary' precision, recall, F1 of class 1 and (TPR + TNR) / 2 of class 1 against the rest from the confusion matrix
 *                        (what roc_curve gives on hard 0 / 1 predictions, utils.py:42-44)
 *               [8..11]  'macro' precision, recall, F1, AUC: unweighted class means
 *               then per class c: precision, recall, F1, one-vs-rest AUC of the stored probabilities' column c
 *   An empty denominator gives 0 for precision / recall / F1; a class without a positive or without a negative row has the AUC NaN (and the
 *   macro AUC is then NaN).  AUC_c is the exact Mann-Whitney statistic by pair counting: over the pairs (i: label c, j: another label),
 *   (2 #(s_ic > s_jc) + #(s_ic == s_jc)) / (2 P N), counted in 64-bit integers, one division in fp64. */
#define WSI_METRICS_STATE_HEAD   4
#define WSI_METRICS_RESULT_HEAD  12
#define WSI_METRICS_BAD_LABEL    1
#define WSI_METRICS_NONFINITE    2
#define WSI_METRICS_OVERFLOW     4
int wsi_metrics_update(const float* logits, const int64_t* labels, int32_t B, int32_t C, int32_t* state, float* probs, int64_t* row_labels,
                       int64_t* row_preds, int32_t capacity, void* stream);
int wsi_metrics_finalize(const int32_t* state, const float* probs, const int64_t* row_labels, int32_t C, int32_t capacity,
                         int64_t* pair_partials, double* result, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Epoch metrics of the multi-label MIL baselines kept on the device (wsi_hgnn_amd/mil/metrics.py::BagEpochMetrics): what the
 * reference's test() computes after every epoch (baselines/ReMix_DSMIL_ABMIL/train_tcga_k-fold.py:98-180, train_remix_k-fold.py:160-232) -
 * sigmoid scores, the ROC-optimal threshold per class (multi_label_roc / optimal_thresh), the hard predictions under it and their counts -
 * without a read-back per bag.  Entry points added to ABI 26.  No allocation, no synchronisation, nothing a hipGraph cannot record, no float
 * atomics; every count is an integer and every float sum has one order: identical calls give identical bits.
 *
 * The accumulator (caller-owned, `state` zeroed by the caller to reset it):
 *   state        int32 [WSI_BAG_METRICS_STATE_HEAD], 8-byte aligned: [0] cursor n (rows stored), [1] flag bits (WSI_BAG_METRICS_*), [2..3] the
 *                fp64 sum of the stored rows' losses
 *   scores       fp32 [capacity, C]: sigmoid(bag_pred)      row_targets  fp32 [capacity, C]
 * Limits: 1 <= C <= WSI_BAG_METRICS_MAX_CLASSES, 0 <= capacity <= WSI_BAG_METRICS_MAX_ROWS (one workgroup sorts a class's rows in LDS),
 * S * C <= 65536.
 *
 * wsi_bag_metrics_update: ONE launch, one workgroup.  bag_pred [S, C] fp32 logits, max_pred [S, C] fp32 logits or NULL (ABMIL), targets
 * [S, C] fp32, weights [S] fp32.  For every segment s in order: weights[s] <= 0 (or NaN) skips it before anything else of it is read (the
 * padding of a mil.BagSlot may carry anything); a non-finite logit (of either prediction) skips it and sets WSI_BAG_METRICS_NONFINITE; a target
 * other than 0 or 1 skips it and sets WSI_BAG_METRICS_BAD_TARGET; a row that would land at or past `capacity` is dropped and sets
 * WSI_BAG_METRICS_OVERFLOW (nothing is written past the capacity).  A counted row writes, at the cursor, 1 / (1 + expf(-x)) of its bag_pred
 * row and its target row, advances the cursor and adds its loss to the fp64 sum (a fixed tree per 256 segments, those in order): the mean over
 * the C classes of max(x, 0) - x t + log1p(exp(-|x|)) in fp64 - BCEWithLogits - of bag_pred, or 0.5 x that + 0.5 x that of max_pred.
 *
 * wsi_bag_metrics_finalize: two launches over the n stored rows (n read from state[0] on the device).
 *   result       int64 [WSI_BAG_METRICS_RESULT_HEAD + 8 * C + K * K], K = C > 1 ? C : 2; the fp64 fields are stored as their bits:
 *                [0] n  [1] flag bits (those of state, and WSI_BAG_METRICS_ONE_LABEL)  [2] fp64 loss sum  [3] rows whose hard prediction row
 *                equals their target row
 *                per class c at HEAD + 8 c: [0] fp64 threshold  [1] tp  [2] fp at it  [3] P  [4] N  [5] gt  [6] eq  [7] fp64 AUC
 *                then conf[true * K + predicted] of the decoded labels
 *   (a) one workgroup per class c sorts (score bits, label bit) descending in LDS - scores lie in [0, 1], so their bit patterns order them as
 *   integers - and takes one ROC point per distinct score, at the last row of its tie group: tps = positives so far, fps = rows so far - tps.
 *   With more than two points it keeps the first, the last and every interior point where the second difference of fps or of tps over its two
 *   neighbours is non-zero (sklearn's drop_intermediate), prepends the point (0, 0) with the threshold +inf, and takes the FIRST minimum of
 *   fps / N - tps / P (fp64, this form; N, P = the last fps, tps) in that order: the threshold is that point's score widened to fp64, tp / fp
 *   its counts.  gt / eq = the pairs (positive i, negative j) with s_i > s_j / s_i == s_j; AUC = (2 gt + eq) / (2 P N), one fp64 division of
 *   integers.  A class with P = 0 or N = 0 (n = 0 included) has threshold and AUC NaN, tp = fp = gt = eq = 0 and sets WSI_BAG_METRICS_ONE_LABEL.
 *   (b) one workgroup walks the rows: prediction[c] = score[c] >= threshold[c] (in fp64); counts the rows equal to their target row and the
 *   confusion matrix of the decoded labels - C > 1: the first c with a 1, 0 for an all-zero row (argmax); C = 1: the value itself. */
#define WSI_BAG_METRICS_STATE_HEAD   4
#define WSI_BAG_METRICS_RESULT_HEAD  4
#define WSI_BAG_METRICS_MAX_ROWS     4096
#define WSI_BAG_METRICS_MAX_CLASSES  32
#define WSI_BAG_METRICS_BAD_TARGET   1
#define WSI_BAG_METRICS_NONFINITE    2
#define WSI_BAG_METRICS_OVERFLOW     4
#define WSI_BAG_METRICS_ONE_LABEL    8
int wsi_bag_metrics_update(const float* bag_pred, const float* max_pred, const float* targets, const float* weights, int32_t S, int32_t C,
                           int32_t* state, float* scores, float* row_targets, int32_t capacity, void* stream);
int wsi_bag_metrics_finalize(const int32_t* state, const float* scores, const float* row_targets, int32_t C, int32_t capacity,
                             int64_t* result, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GTNMIL (wsi_hgnn_amd/gtn, baselines/GTNMIL/models/GraphTransformer.py): the mincut assignment over a sparse adjacency and the attention of
 * its 101-token transformer.  Entry points added to ABI 26.  No atomics, no allocation, no synchronisation: identical calls give identical bits.
 *
 * wsi_mincut_fwd: packed rows of all graphs, one plan segment per graph (chunk tables as for wsi_segment_reduce_fwd).  (ptr, idx, edge_w) = the
 *   adjacency as a CSR by row: A[i, idx[e]] += edge_w[e] for e in [ptr[i], ptr[i + 1]) (edge_w NULL = 1; repeated entries add up; a row may be
 *   empty; nothing is assumed symmetric).  z [n, K] logits with row stride ldz, 1 <= K <= 128 (more: WSI_ENOSYS).  Writes, all dense:
 *     s [n, K] = softmax(z, -1)      t [n, K] = A s      deg [n]: d_i = sum_e edge_w[e]
 *     num [num_segs] = sum_{i in g} <s_i, t_i> = trace(s^T A s)       den [num_segs] = sum_{i in g} d_i |s_i|^2 = trace(s^T D s)
 *   partial: scratch of wsi_mincut_partials(num_chunks) floats.  A segment without rows gets num = den = 0.
 * wsi_mincut_bwd: g_z [n, K] from g_s [n, K] (row stride ldgs), g_num, g_den [num_segs] (each may be NULL = 0) and the forward's s, t, deg:
 *     u_i = g_s_i + g_num[g] (t_i + t'_i) + 2 g_den[g] d_i s_i        g_z_i = s_i * (u_i - <s_i, u_i>)
 *   with t' = A^T s gathered along the CSC side of the same entries (colptr, csc_dst = the row of every entry grouped by its column,
 *   edge_w_csc = the weights in that order).  K = 1 gives exact zeros. */
int32_t wsi_mincut_partials(int32_t num_chunks);
int wsi_mincut_fwd(const float* z, int64_t ldz, int32_t n, int32_t K, const int32_t* ptr, const int32_t* idx, const float* edge_w,
                   const int32_t* chunk_row, int32_t num_chunks, const int32_t* seg_chunk, int32_t num_segs,
                   float* s, float* t, float* deg, float* partial, float* num, float* den, void* stream);
int wsi_mincut_bwd(const float* g_s, int64_t ldgs, const float* g_num, const float* g_den, const float* s, const float* t,
                   const float* deg, int32_t n, int32_t K, const int32_t* colptr, const int32_t* csc_dst, const float* edge_w_csc,
                   const int32_t* chunk_row, const int32_t* chunk_seg, int32_t num_chunks, float* g_z, void* stream);

/* wsi_seq_attn_fwd: multi-head attention over a short sequence (models/ViT.py:183-215).  qkv [B, n, 3 H d] dense, 16-byte aligned, columns in
 *   the reference's (qkv h d) order; out [B, n, H d] in (h d) order; lse [B, H, n] = the log-sum-exp of every row of scale * q k^T over the
 *   keys - all the forward keeps.  1 <= n <= 128 and d in {8, 16}; anything else: WSI_ENOSYS (B = 0 or n = 0: nothing to do).  No dropout.
 * wsi_seq_attn_bwd: g_qkv [B, n, 3 H d] (same layout, every element written) from g_out [B, n, H d], qkv and lse; the probabilities are
 *   recomputed.  One workgroup per (b, h) in both. */
int wsi_seq_attn_fwd(const float* qkv, int32_t B, int32_t n, int32_t H, int32_t d, float scale, float* out, float* lse, void* stream);
int wsi_seq_attn_bwd(const float* g_out, const float* qkv, const float* lse, int32_t B, int32_t n, int32_t H, int32_t d, float scale,
                     float* g_qkv, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GraphCAM of GTNMIL (wsi_hgnn_amd/gtn/graphcam.py): the relevance-propagation rules of baselines/GTNMIL/models/layers.py at alpha = 1, for G
 * slides and C classes per launch.  Entry points added to ABI 26.  fp32; no atomics, no allocation, no synchronisation: identical calls give
 * identical bits.  Every tensor is dense and 16-byte aligned (else WSI_EINVAL).  Forward tensors are [G, n, width], relevances [G, C, n, width].
 *   sd(a, b) = layers.safe_divide: 0 where b == 0, else a / (b + 1e-9f), the denominator 1e-9f where that sum is exactly 0.
 *   x+ = max(x, 0), x- = min(x, 0).
 *
 * wsi_lrp_linear: Linear.relprop.  X [G, n, in], W [out, in], R [G, C, n, out] -> out_rel [G, C, n, in]:
 *     Z = X+ W+^T + X- W-^T  (once per token, shared by the classes; the bias plays no part)     S = sd(R, Z)
 *     out_rel = X+ * (S W+) + X- * (S W-)
 *   in a multiple of 4, 4 <= in <= 256, 1 <= out <= 256; anything else: WSI_ENOSYS.  W+ and W- are taken from one copy of W staged in LDS.
 *
 * wsi_lrp_residual: Clone.relprop of a tensor's two uses, then Add.relprop of the residual below it.  X, A, B [G, n, E]; r1, r2 [G, C, n, E].
 *     R = X * (sd(r1, X) + sd(r2, X))            (r2 NULL: R = r1, X is not read and may be NULL)
 *     S = sd(R, A + B);  a = A S;  b = B S;  a *= sd(sd(|Sa|, |Sa| + |Sb|) * SR, Sa);  b *= sd(sd(|Sb|, |Sa| + |Sb|) * SR, Sb)
 *   with Sa, Sb, SR the sums of a, b, R over the [n, E] tensor of one (slide, class): one workgroup per (slide, class), a fixed order.
 *   E a multiple of 4 (else WSI_ENOSYS), n * E < 2^31.
 *
 * wsi_lrp_attention: Attention.relprop between its two Linear rules, and the block's layer map.  qkv [G, n, 3 H d] and lse [G, H, n] as
 *   wsi_seq_attn_fwd leaves them (the probabilities are recomputed as in wsi_seq_attn_bwd), R [G, C, n, H d] the relevance of the attention
 *   output, g_out [G, C, n, H d] the gradient of the class score with respect to it, or NULL.  Per head, with P = the probabilities:
 *     S2 = sd(R, P v);  cam_attn = P * (S2 v^T) / 2;  cam_v = v * (P^T S2) / 2
 *     S1 = sd(cam_attn, q k^T)  (q k^T unscaled);  cam_q = q * (S1 k) / 2;  cam_k = k * (S1^T q) / 2
 *     cam_qkv [G, C, n, 3 H d] in the (qkv h d) column order, every element written
 *     M [G, C, n, n] = (1 / H) sum_h max(d attn * cam_attn, 0),  d attn = g_out v^T     (g_out NULL: max(cam_attn, 0), the rollout map)
 *   One workgroup per (slide, class, head).  With H > 1 every head writes its term to partial [G * C * H * n * n] floats and a second launch
 *   adds the heads in order; H = 1 writes M directly and partial may be NULL.  1 <= n <= 128 and d in {8, 16}; anything else: WSI_ENOSYS. */
int wsi_lrp_linear(const float* X, const float* W, const float* R, int32_t G, int32_t C, int32_t n, int32_t fan_in, int32_t fan_out,
                   float* out_rel, void* stream);
int wsi_lrp_residual(const float* X, const float* r1, const float* r2, const float* A, const float* B, int32_t G, int32_t C, int32_t n,
                     int32_t E, float* out_a, float* out_b, void* stream);
int wsi_lrp_attention(const float* qkv, const float* lse, const float* R, const float* g_out, int32_t G, int32_t C, int32_t n, int32_t H,
                      int32_t d, float scale, float* partial, float* cam_qkv, float* M, void* stream);

/* ------------------------------------------------------------------------------------------------
 * H2MIL (wsi_hgnn_amd/h2mil, baselines/H2MIL/code): RAConv's two-level attention and IHPool's cluster assignment.  Entry points added to
 * ABI 26.  No atomics, no allocation, no synchronisation, every sum in one fixed order: identical calls give identical bits.
 *
 * Edge layout of both wsi_ra_attn_*: rowptr[n+1] / src[E] = CSR by destination with the SOURCE'S TYPE as the secondary key (a destination's
 * groups (v, t) are contiguous runs; edge id = CSR position), colptr[n+1] / csc_eid[E] / csc_dst[E] = CSC by source over the same edge ids.
 * node_type[n] int32 in {0, 1, 2} (anything else is clamped into that range).  ft [n, C] fp32, 1 <= C <= 4096;
 * sc [n, 4] dense = el | er | pl | pr, the four per-node scalars of RAConv.py:96-97,121-122 (pl, pr through the folded t_lin_l).
 *
 * wsi_ra_attn_fwd: with t(e) = node_type[src[e]], s_e = leaky_relu(el[u_e] + er[v], negative_slope):
 *     a_e = softmax of s over the edges of group (v, t);   q_vt = leaky_relu(mean_{e in (v,t)} pl[u_e] + pr[v], negative_slope);
 *     beta_vt = softmax of q over the groups PRESENT at v;  out[v] = sum_e beta_{v,t(e)} a_e ft[u_e] + bias  (bias optional; a node without
 *     in-edges: out = bias).  Both softmaxes subtract the maximum and add no epsilon.
 *     stat [n, 3, 4] <- per (node, type): max_e s_e (+inf for an absent group) | log sum_e exp(s_e - max) | the group's edge count | beta.
 * wsi_ra_attn_bwd: from g_out and the forward's sc / stat: g_ft [n, C] <- the AGGREGATION term only, sum_e beta a_e g_out[v_e]  (the terms
 *     through sc are the caller's: sc is a projection of the same input);  g_sc [n, 4] <- the gradients of el | er | pl | pr;
 *     g_bias [C] (optional) <- the column sums of g_out.  Scratch, all caller-owned: edge_ws [E] floats, group_ws [3 n] floats,
 *     bias_ws [WSI_RA_BIAS_PARTS * C] floats (read only when g_bias is given).
 *
 * wsi_ihpool_assign (IHPool.py:138-142, 185-189 at dis = 'ou'): xyf [num_nodes, 3] dense = x | y | fitness.  The members of all segments,
 *     grouped by segment: member_node[m] (row of xyf), member_seg[m] (non-decreasing, in [0, num_segs)); the seeds of segment s are
 *     seed_node[seed_ptr[s] .. seed_ptr[s + 1]) (rows of xyf).  assign[i] <- the position within its segment's seed list of the seed nearest
 *     to member i in |xy_s - xy_n|_2 + |f_s - f_n|; equal distances go to the lowest position; a member that is itself a seed gets its own
 *     position; -1 for a member whose segment has no seed.  A segment may be empty.  Indices outside their tables are ignored, never followed. */
#define WSI_RA_BIAS_PARTS 64
int wsi_ra_attn_fwd(const float* ft, int64_t ldf, const float* sc, const int32_t* node_type, int32_t n, int32_t C,
                    const int32_t* rowptr, const int32_t* src, float negative_slope, const float* bias,
                    float* out, int64_t ldo, float* stat, void* stream);
int wsi_ra_attn_bwd(const float* ft, int64_t ldf, const float* sc, const int32_t* node_type, const float* stat,
                    const float* g_out, int64_t ldg, int32_t n, int32_t E, int32_t C,
                    const int32_t* rowptr, const int32_t* src, const int32_t* colptr, const int32_t* csc_eid,
                    const int32_t* csc_dst, float negative_slope, float* edge_ws, float* group_ws, float* bias_ws,
                    float* g_ft, int64_t ldgf, float* g_sc, float* g_bias, void* stream);
int wsi_ihpool_assign(const float* xyf, int32_t num_nodes, const int32_t* member_node, const int32_t* member_seg, int32_t num_members,
                      const int32_t* seed_ptr, const int32_t* seed_node, int32_t num_segs, int32_t num_seeds, int32_t* assign, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Slide graphs from patch grids (wsi_hgnn_amd/construct.py: grid_adjacency, slide_trees).  Entry points added to ABI 26.  Exact look-ups in many
 * small integer point sets: coords [P, 2] int32, all sets of a call packed, set s = the points [set_ptr[s], set_ptr[s + 1]), 1 <= S <= 8192.
 * A valid coordinate is 0 <= c < 2^24; the key of a point is (set << 50) | ((x + 1) << 25) | (y + 1), so the probes at -1 and 2^24 are
 * representable and match nothing.  capacity: a power of two >= 2 P (else WSI_EINVAL).  Every probe loop runs at most `capacity` steps.
 * Look-ups that miss and indices outside their tables are ignored, never followed.  Identical calls give identical outputs, whatever slot a
 * key happened to land in.
 *
 * wsi_grid_index: one open-addressing table (keys int64 [capacity], rows int32 [capacity]) over (set, x, y) -> point, by a 64-bit
 *   compare-and-swap on the key; the winner writes the row.  set_max int32 [S, 2] <- the per-set maxima of x and y (integer atomic max; -1 for
 *   an empty set).  flags int32 [2] <- 0, then flags[0] |= WSI_GRID_BAD_COORD (a coordinate outside [0, 2^24); the point is not stored) |
 *   WSI_GRID_REPEATED (a (set, x, y) given twice) | WSI_GRID_TABLE_FULL (no free slot within `capacity` steps).  It resets all three tables.
 * wsi_grid_count: counts int32 <- the items every node will emit, laid out so that ONE prefix sum over it gives the write offsets.
 * wsi_grid_write: probes again and writes at offsets_incl[i] - counts[i], offsets_incl int64 = the INCLUSIVE prefix sum of counts.  No atomics.
 *
 * mode WSI_GRID_ADJACENCY (GTNMIL, baselines/GTNMIL/feature_extractor/build_graphs.py:78-96): one set per slide, nodes in the caller's order
 *   (the reference: file order).  counts [P].  The entries of node i are (out_a = i, out_b = j) for every j != i of the same set with
 *   |x_i - x_j| <= 1 and |y_i - y_j| <= 1; rows ascend and the columns of a row ascend (the order of adj.nonzero()).  i and j are point
 *   numbers, i.e. global rows of the packed batch.  n1, cover, parent, set_max, node_type, node_tree, x_y_index are not read (NULL).
 *
 * mode WSI_GRID_TREE (H2MIL, baselines/H2MIL/code/github_pretreat.py:94-329): B slides, S = 2 B; the points are the level-1 nodes of all
 *   slides (n1 of them; set b = slide b; (i, j) of a 5x patch name a-b-c-d-i-j) and then the level-2 nodes of all slides (set B + b; a 10x
 *   patch name x-y); cover [n1, 4] = (a, b, c, d) of every level-1 node.  Node rows per slide: the root, its level-1 nodes, its level-2 nodes,
 *   each in the given order; every row below is global.  counts [2 n1 + n2] in [slide][section][node] order, the slide's edges being
 *     section A (:106-133), per level-1 node r: r -> root, root -> r, then for the children (a,c), (b,c), (a,d), (b,d) - each one that exists
 *       among the slide's level-2 coordinates - r -> child, child -> r.  The four slots are independent: a == b or c == d emits a child twice.
 *     section B (:142-170), per level-1 node, for the offsets (0,+1), (0,-1), (+1,0), (-1,0), (+1,+1), (-1,+1), (+1,-1), (-1,-1) in this
 *       order: self -> neighbour where the neighbour exists.       section C (:173-202): the same over the level-2 nodes.
 *   out_a / out_b = source / destination row.  wsi_grid_count also leaves parent int32 [n2]: for every level-2 node the row of the LAST level-1
 *   node in order that covers it (:228-254; an integer atomic max), -1 if none.  wsi_grid_write also writes, for all N = B + P rows,
 *     node_type int64 [N]: 0 / 1 / 2      node_tree int64 [N]: -1 for a root, the root's row for a level-1 node, parent for a level-2 node
 *       (an uncovered one: -2, and flags[1] <- WSI_GRID_UNCOVERED by a plain store)
 *     x_y_index fp64 [N, 2] (:257-315): (0, 0) for a root, else (x / max_x, y / max_y) with the maxima over the node's slide and level: one
 *       IEEE double division per value (a maximum of 0 gives inf / nan).
 *   A slide without level-1 nodes gets no root row written: the caller refuses empty levels.
 * The output buffers hold the largest possible count: 8 P entries (adjacency), 18 n1 + 8 n2 edges (tree). */
#define WSI_GRID_ADJACENCY   0
#define WSI_GRID_TREE        1
#define WSI_GRID_BAD_COORD   1
#define WSI_GRID_REPEATED    2
#define WSI_GRID_TABLE_FULL  4
#define WSI_GRID_UNCOVERED   8
int wsi_grid_index(const int32_t* coords, int32_t num_points, const int32_t* set_ptr, int32_t num_sets, int64_t* keys, int32_t* rows,
                   int32_t capacity, int32_t* set_max, int32_t* flags, void* stream);
int wsi_grid_count(int32_t mode, const int32_t* coords, int32_t num_points, const int32_t* set_ptr, int32_t num_sets, int32_t n1,
                   const int32_t* cover, const int64_t* keys, const int32_t* rows, int32_t capacity, int32_t* counts, int32_t* parent,
                   void* stream);
int wsi_grid_write(int32_t mode, const int32_t* coords, int32_t num_points, const int32_t* set_ptr, int32_t num_sets, int32_t n1,
                   const int32_t* cover, const int64_t* keys, const int32_t* rows, int32_t capacity, const int32_t* counts,
                   const int64_t* offsets_incl, const int32_t* parent, const int32_t* set_max, int64_t* out_a, int64_t* out_b,
                   int64_t* node_type, int64_t* node_tree, double* x_y_index, int32_t* flags, void* stream);

/* The fill of a padded GTNMIL graph slot (an addition to ABI 26; gtn.GraphSlot).  A slot is `cells` cells of `cell_rows` rows;
 * slide i of a batch lies at the head of cell i, every other row is dead.  slide_desc (device): 16 int64 words per slide
 *   [x, x_stride, rowptr, src, edge_w, colptr, csc_dst, edge_w_csc, rows, entries, dst_entry, label, 0, 0, 0, 0]
 * x = the slide's fp32 rows (unit column stride, x_stride floats from row to row); rowptr / colptr int32 [rows + 1] and src / csc_dst int32
 * [entries] = the slide's LOCAL ops.EdgeCSR tables; edge_w / edge_w_csc fp32 [entries] or 0 (every weight 1); dst_entry = the slide's first
 * entry in the slot = the sum of the entries of the slides before it.  rows <= cell_rows, total_entries = the sum of all entries <= entry_cap.
 * Written, in two launches whatever the batch (no atomics, no read-back, no allocation, the same bits run after run):
 *   x [cells * cell_rows, feats] (contiguous): the slides' rows, zero in dead rows;  live [rows] 1 / 0;  cell_live [cells] 1 / 0;
 *   labels int64 [cells]: the descriptor's label, -100 in unused cells;  scalars[0] = inv_cells, scalars[1] = live_rows (passed by the host);
 *   rowptr / colptr int32 [cells * cell_rows + 1]: local value + dst_entry in a live row, the running entry offset in a dead one (an empty
 *     range), total_entries at the end;  src / csc_dst [e] = local value + the cell's first row, edge_w / edge_w_csc [e] the weight or 1.0, for
 *     e < total_entries: nothing at or behind total_entries is written, and nothing that walks rowptr / colptr ever reads there. */
int wsi_graph_slot_fill(const int64_t* slide_desc, int32_t num_slides, int32_t cells, int32_t cell_rows, int32_t feats,
                        int64_t entry_cap, int64_t total_entries, float inv_cells, float live_rows,
                        float* x, float* live, float* cell_live, float* scalars, int64_t* labels,
                        int32_t* rowptr, int32_t* src, float* edge_w, int32_t* colptr, int32_t* csc_dst, float* edge_w_csc, void* stream);

/* BatchNorm1d over the LIVE rows of a padded table (an addition to ABI 26; ops.masked_batch_norm).  x [rows, C] fp32 (row stride
 * ldx), live [rows] fp32 0 / 1, live_rows = ONE device word holding the number of live rows n as fp32 (n >= 2 in training; the host checks).
 * wsi_masked_bn_fwd, training != 0: per column the mean and the biased variance over the live rows - centred (Welford per lane, Chan merges of
 *   (count, mean, M2) across waves, chunks and lanes in one fixed order; never E[x^2] - mean^2) - then stats [2, C] = (mean, 1 / sqrt(var + eps)),
 *   running_mean = (1 - momentum) running_mean + momentum mean and running_var likewise with the unbiased variance M2 / (n - 1) (either may be
 *   NULL: not tracked), and y = (x - mean) rstd gamma + beta in live rows, 0 in dead rows (gamma / beta NULL: 1 / 0).
 *   training == 0: stats = (running_mean, 1 / sqrt(running_var + eps)), the same y; live_rows and partial are not read.
 *   partial: 3 * wsi_masked_bn_chunks(rows) * C floats of workspace.
 * wsi_masked_bn_bwd: dbeta = sum over live rows of g, dgamma = sum of g xhat (xhat = (x - mean) rstd from the saved stats), and
 *   dx = gamma rstd (g - dbeta / n - xhat dgamma / n) in live rows (training == 0: gamma rstd g), 0 in dead rows.
 *   partial: 2 * wsi_masked_bn_chunks(rows) * C floats.
 * No atomics: chunk partials are finished by a second small launch; identical calls give identical bits. */
int32_t wsi_masked_bn_chunks(int32_t rows);
int wsi_masked_bn_fwd(const float* x, int64_t ldx, int32_t rows, int32_t C, const float* live, const float* live_rows,
                      const float* gamma, const float* beta, float* running_mean, float* running_var, int32_t training,
                      float momentum, float eps, float* partial, float* stats, float* y, int64_t ldy, void* stream);
int wsi_masked_bn_bwd(const float* gy, int64_t ldg, const float* x, int64_t ldx, int32_t rows, int32_t C, const float* live,
                      const float* live_rows, const float* gamma, const float* stats, int32_t training, float* partial,
                      float* dgamma, float* dbeta, float* dx, int64_t lddx, void* stream);

/* BatchNorm1d + ReLU over the live rows in the same passes (an addition to ABI 26; ops.masked_batch_norm(relu=True), models/GIN.py, DESIGN
 * 3.33).  With y = fmaf((x - mean) rstd, gamma, beta) exactly as wsi_masked_bn_fwd computes it:
 *   wsi_masked_bn_relu_fwd writes y > 0 ? y : 0 in live rows and 0 in dead rows (y == 0 is on the zero side); statistics, running
 *     statistics, stats, workspace and eval mode are those of wsi_masked_bn_fwd - the ReLU enters no statistic.
 *   wsi_masked_bn_relu_bwd is wsi_masked_bn_bwd with g read as g [y > 0], in the sums and in dx.  It recomputes y from x, the saved stats,
 *     gamma and beta through the one device function the forward calls, so the sign is the forward's bit for bit; no y and no mask is
 *     stored or read.  That is why it takes `beta` (NULL: 0), which wsi_masked_bn_bwd has no use for; dbeta is still an output.
 * Both give the bits of the unfused entry followed / preceded by the elementwise ReLU: the same sums in the same order. */
int wsi_masked_bn_relu_fwd(const float* x, int64_t ldx, int32_t rows, int32_t C, const float* live, const float* live_rows,
                           const float* gamma, const float* beta, float* running_mean, float* running_var, int32_t training,
                           float momentum, float eps, float* partial, float* stats, float* y, int64_t ldy, void* stream);
int wsi_masked_bn_relu_bwd(const float* gy, int64_t ldg, const float* x, int64_t ldx, int32_t rows, int32_t C, const float* live,
                           const float* live_rows, const float* gamma, const float* beta, const float* stats, int32_t training,
                           float* partial, float* dgamma, float* dbeta, float* dx, int64_t lddx, void* stream);

/* The per-relation-source plan derived from a base plan (an addition to ABI 26; graph.plan_by_relation): the plan HGT's
 * attention runs on, whose source rows are numbered per (relation, source node): row(r, u) = rel_lo[r] + (u - type_off[source type of r]).
 * Inputs, all int32 and all of the base plan: src [E] (global source of every CSR edge), colptr [N + 1] / csc_eid [E] / csc_dst [E] (CSC by
 * global source), edge_seg [E] (the softmax segment of every CSR edge, < num_segs), and `header`, header_words = 5 T + 5 NR + 8 words on
 * the device (T = num_types, NR = num_rels; the host knows them and passes them, the table is never read back):
 *   [T, NR, NS, N]  type_off[T+1]  seg_off[T+1]  R[T]  slot_ptr[T+1]  slot_rel[NR]  rel_lo[NR]  rel_src[NR]  rel_k[NR]  srel_ptr[T+1]  srel[NR]
 * R[t] = relations into node type t, slot_rel[slot_ptr[t] + j] = the relation of slot j of type t (segment = seg_off[t] + local node * R[t]
 * + j), rel_lo[r] = first row of relation r, rel_src[r] = its source type, srel[srel_ptr[s] .. srel_ptr[s+1]) = the relations leaving type s,
 * rel_k[r] = r's position in that list.  max_src_rels = the longest such list; above WSI_PLAN_REL_MAX_RELS the call returns WSI_EINVAL.
 * Written (int32, caller-owned): src_rel [E]; colptr_rel [NS + 1], NS = num_src_rows; csc_eid_rel [E]; csc_dst_rel [E] - a row's entries in
 * the order the source's base CSC lists them (a stable partition by relation), which is what a stable sort of the CSR edges by row gives.
 * scratch: wsi_plan_by_relation_scratch_words(NS) int32 words (entry counts and scan partials; smaller: WSI_ENOMEM).
 * Five launches on `stream`, a wave per source node (a source of any out-degree is a strided loop of 64 lanes): no atomics, no floats, no
 * allocation, no synchronisation, no read-back; identical calls give identical bits.  num_edges == 0 (the arrays may then be NULL) writes
 * colptr_rel = 0 and nothing else. */
#define WSI_PLAN_REL_MAX_RELS 32
#define WSI_PLAN_REL_TILE     1024   /* counts per workgroup of the prefix sum */
int64_t wsi_plan_by_relation_scratch_words(int32_t num_src_rows);
int wsi_plan_by_relation(const int32_t* src, const int32_t* colptr, const int32_t* csc_eid, const int32_t* csc_dst,
                         const int32_t* edge_seg, int32_t num_nodes, int32_t num_edges, int32_t num_segs,
                         const int32_t* header, int32_t header_words, int32_t num_types, int32_t num_rels, int32_t num_src_rows,
                         int32_t max_src_rels, int32_t* src_rel, int32_t* colptr_rel, int32_t* csc_eid_rel, int32_t* csc_dst_rel,
                         int32_t* scratch, int64_t scratch_words, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Explanations scored against annotations (wsi_hgnn_amd/localization.py; entry points added to ABI 26): the reference's
 * evaluator/explain_graphs.py:81-119 (patch labels), :179-184 (per-slide AUROC and its NaN-skipping mean) and :136-141 (the heat-map fill).
 * A packed batch of B slides; every table is built by the host, which knows all sizes, and lives on the device:
 *   tiles  int32 [T, 4], 16-byte aligned: (slide, first row, rows <= WSI_LOC_TILE, position of the first row within its slide); the tiles of a
 *          slide are consecutive and cover its rows in order; a slide without rows has no tile.
 *   slides int64 [B, 3]: (first scratch word of the slide, rows of the slide, first tile of the slide).
 * No launch allocates, synchronises or reads back; all run on `stream`; identical calls give identical bits.
 *
 * wsi_loc_labels: labels int32 [N] <- 1 iff centre i (centres fp64 [N, 2]) lies STRICTLY inside at least one ring of its own slide, by the
 *   even-odd rule; a centre on a ring's boundary (an edge or a vertex) is not inside that ring.  Rings are independent.  vertices fp64 [V, 2],
 *   ring r = the vertices [ring_ptr[r], ring_ptr[r + 1]) closed from its last vertex to its first; ring_box fp64 [R, 4] = (min x, min y, max x,
 *   max y) of every ring.  chunks int32 [K, 4], 16-byte aligned: (ring, first edge, edges <= chunk_edges, slide) - every ring cut into runs of
 *   edges, a chunk never spanning two rings, the chunks of a ring consecutive, those of a slide [slide_chunk_ptr[s], slide_chunk_ptr[s + 1]);
 *   max_slide_chunks = the most chunks a slide has (<= WSI_LOC_MAX_SLIDE_CHUNKS).  1 <= chunk_edges <= WSI_LOC_CHUNK_MAX.  All arithmetic is
 *   fp64 without a division: edge (x0, y0) -> (x1, y1) against (x, y): o = (x1 - x0)(y - y0) - (x - x0)(y1 - y0); a crossing iff
 *   (y0 > y) != (y1 > y) and (o > 0) == (y1 > y0); on the boundary iff o == 0 and (x, y) lies in the edge's closed bounding box.  A centre outside
 *   a ring's closed box is outside the ring without an edge being read.  scratch: int32, slide s owning chunks(s) * rows(s) words from
 *   slides[s][0] on (bit 0 = parity of a chunk's crossings, bit 1 = on its boundary); nothing at or beyond scratch_words is touched.  Two
 *   launches, no atomics.
 * wsi_loc_score: scores fp32 [N, C] (dense), labels int32 [N] (0 = negative, anything else positive).  Per slide s and column c, by exact
 *   pair counting within the slide: counts int64 [B, C, 4] = (P, N, gt, eq) - positives, negatives, (positive, negative) pairs with s_pos >
 *   s_neg, pairs with s_pos == s_neg; auc fp64 [B, C] = (2 gt + eq) / (2 P N), one division, NaN when P == 0 or N == 0; flags int32 [B, C] =
 *   WSI_LOC_NONFINITE when a score of (s, c) is not finite, whose auc is NaN.  mean fp64 [C] = the mean over the slides whose auc is not NaN,
 *   summed in the order of numpy's pairwise summation (= numpy.nanmean of the column, to the last bit); NaN when there is none.
 *   partial: int64 [C * T * 5] of workspace.  Three launches, integer partials, no atomics.
 * wsi_loc_owner: owner int32 [height, width] (the caller presets -1) <- max(owner, i) over the pixels x .. x + patch, y .. y + patch
 *   (inclusive: patch + 1 pixels a side, clipped to the image) of every patch i at grid_xy int32 [n, 2] = (x, y): where patches overlap the
 *   highest index owns the pixel, the result of drawing them in order.  One launch; the integer atomic maximum does not depend on the order. */
#define WSI_LOC_TILE              256
#define WSI_LOC_CHUNK_MAX         1024
#define WSI_LOC_MAX_SLIDE_CHUNKS  65535
#define WSI_LOC_MAX_COLUMNS       1024
#define WSI_LOC_MAX_PATCH         4096
#define WSI_LOC_NONFINITE         1
int wsi_loc_labels(const double* centres, int32_t num_centres, const int32_t* tiles, int32_t num_tiles, const int64_t* slides,
                   int32_t num_slides, const double* vertices, int64_t num_vertices, const int64_t* ring_ptr, const double* ring_box,
                   int32_t num_rings, const int32_t* chunks, int32_t num_chunks, const int32_t* slide_chunk_ptr, int32_t max_slide_chunks,
                   int32_t chunk_edges, int32_t* scratch, int64_t scratch_words, int32_t* labels, void* stream);
int wsi_loc_score(const float* scores, int32_t num_rows, int32_t C, const int32_t* labels, const int32_t* tiles, int32_t num_tiles,
                  const int64_t* slides, int32_t num_slides, int64_t* partial, int64_t* counts, int32_t* flags, double* auc, double* mean,
                  void* stream);
int wsi_loc_owner(const int32_t* grid_xy, int32_t num_patches, int32_t patch, int32_t height, int32_t width, int32_t* owner, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GINConv aggregation (an addition to ABI 26; dgl.nn.pytorch.GINConv as models/GIN.py:120-121 constructs it; ops.gin_aggregate).
 *   neigh[w] = reduce_{e: u -> w} (s_e x[u]),  reduce = sum | mean | max (mode),  s_e = edge_s[e] (NULL: 1)
 *   out[w]   = (1 + eps) x[w] + neigh[w] (+ bias)
 * mean divides by the in-degree (the number of messages, not the sum of s_e); a node without in-edges has neigh = 0 under every mode; under
 * max the scale multiplies the message BEFORE the maximum (the reference's update_all hijack, explainers/gnn_explainer.py:21-33).
 * The graph: rowptr [n + 1] / src [E] = CSR by destination, colptr [n + 1] / csc_eid [E] (CSR position) / csc_dst [E] = the CSC of the same edge
 * numbering by source (the [E] arrays may be NULL for a graph without edges: they are never read then).  fp32 throughout, row strides as arguments (>= D), any 1 <= D <= 1024 (beyond: WSI_ENOSYS), n == 0: WSI_OK without a
 * launch.  eps is a DEVICE pointer to one float (the parameter's own storage): nothing about it crosses to the host.  A group of G lanes
 * owns a row and 256 / G rows share a workgroup; 16-byte chunks when D % 4 == 0 and every pointer and stride allows, scalar otherwise; two
 * or four edges' gathers are in flight per group into independent accumulators that are combined in one fixed order.  No atomics: identical
 * calls give identical bits.
 * wsi_gin_aggregate_fwd : out as above.  mode = WSI_GIN_MAX: arg int32 [n, D] (dense; may be NULL) <- the CSR position of the FIRST maximum of
 *   every (row, column), -1 in rows without in-edges.  Other modes never touch arg.
 * wsi_gin_aggregate_bwd : gx[u] = (1 + eps) g[u] + sum_{e: u -> w} s_e c_w m(w, c, e) g[w];  c_w = 1 / indeg(w) under mean (from rowptr), else 1;
 *   m = [arg[w, c] == e] under max (arg required), else 1.
 * wsi_gin_edge_grad     : g_s[e] = c_w sum_c m(w, c, e) g[w, c] x[src[e], c] for every CSR entry e (g_s [E], CSR order): the gradient of edge_s.
 * wsi_gin_eps_grad      : g_eps[0] = sum_{w, c} g[w, c] x[w, c].  A fixed grid writes wsi_gin_eps_partials() floats into `partial`, a second
 *   launch of one workgroup adds them in order.  (n == 0 launches nothing and leaves g_eps as it is.) */
#define WSI_GIN_SUM   0
#define WSI_GIN_MEAN  1
#define WSI_GIN_MAX   2
int wsi_gin_aggregate_fwd(const float* x, int64_t ldx, int32_t n, int32_t D, const int32_t* rowptr, const int32_t* src, const float* edge_s,
                          const float* eps, int32_t mode, const float* bias, float* out, int64_t ldo, int32_t* arg, void* stream);
int wsi_gin_aggregate_bwd(const float* g, int64_t ldg, int32_t n, int32_t D, const int32_t* rowptr, const int32_t* colptr,
                          const int32_t* csc_eid, const int32_t* csc_dst, const float* edge_s, const float* eps, int32_t mode,
                          const int32_t* arg, float* gx, int64_t ldgx, void* stream);
int wsi_gin_edge_grad(const float* g, int64_t ldg, const float* x, int64_t ldx, int32_t n, int32_t D, const int32_t* rowptr,
                      const int32_t* src, int32_t mode, const int32_t* arg, float* g_s, void* stream);
int32_t wsi_gin_eps_partials(void);
int wsi_gin_eps_grad(const float* g, int64_t ldg, const float* x, int64_t ldx, int32_t n, int32_t D, float* partial, float* g_eps,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WSI_HGNN_H */
