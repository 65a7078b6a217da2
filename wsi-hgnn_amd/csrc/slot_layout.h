// Layout of an AUGMENTED padded batch slot (graph.slot_fill_augmented): everything graph.SlotBatch computes on the host from the
// slides' node and edge counts, as one function of counts that live on the DEVICE (the survivors of a draw), shared by the layout kernel
// (csrc/slot_aug.hip, one thread) and by the host program that checks it against a plain re-implementation (tests/slot_aug_check.cpp).
// Plain integer arithmetic, no device intrinsics.
//
// shape (int64 words): [T, B, b_cap, chunk, c_cap, then per node type t: n_cap, e_cap, type_off, ebase, src_type, R, seg_off]
//   B slides are real (B <= b_cap), graphs b in [B, b_cap) are empty, graph b_cap is the filler; chunk = rows per readout chunk,
//   c_cap = the slot's chunk capacity; type_off / ebase / seg_off = first node / CSR edge / softmax segment of the type in the slot.
// ncnt (int32) [B * T]: nodes of (slide b, type t) at [b * T + t]
// fcnt (int32) [2 B T + 3 B]: CSR edges into (b, t), then CSC entries out of (b, t), then per slide the entries kept of its heavy-destination,
//   light-destination and source order lists
// L (int64 words, SLOT_L_WORDS(B, T)): see the SLOT_L_* offsets below; its filler block is the `fp` of csrc/slot_math.h.
#pragma once
#include <stdint.h>

#ifndef WSI_HD
#ifdef __HIPCC__
#define WSI_HD __host__ __device__
#else
#define WSI_HD
#endif
#endif

namespace wsi {

constexpr int SLOT_SHAPE_HEAD = 5;        // T, B, b_cap, chunk, c_cap
constexpr int SLOT_SHAPE_WORDS = 7;       // per node type
enum { SS_NCAP = 0, SS_ECAP = 1, SS_TOFF = 2, SS_EBASE = 3, SS_STYPE = 4, SS_R = 5, SS_SOFF = 6 };

WSI_HD inline const int64_t* slot_shape_type(const int64_t* shape, int64_t t) { return shape + SLOT_SHAPE_HEAD + t * SLOT_SHAPE_WORDS; }

// offsets into L
WSI_HD inline int64_t SLOT_L_NODE(int64_t B, int64_t T) { return 0; }                      // [b * T + t] global id of the first node of (b, t)
WSI_HD inline int64_t SLOT_L_EDGE(int64_t B, int64_t T) { return B * T; }                  // [b * T + t] CSR position of the first edge into (b, t)
WSI_HD inline int64_t SLOT_L_CSC(int64_t B, int64_t T) { return 2 * B * T; }               // [b * T + t] CSC position of the first entry out of (b, t)
WSI_HD inline int64_t SLOT_L_SEG(int64_t B, int64_t T) { return 3 * B * T; }               // [b * T + t] first softmax segment of (b, t)
WSI_HD inline int64_t SLOT_L_N(int64_t B, int64_t T) { return 4 * B * T; }                 // [t] real nodes of the type
WSI_HD inline int64_t SLOT_L_E(int64_t B, int64_t T) { return 4 * B * T + T; }             // [t] real edges into the type
WSI_HD inline int64_t SLOT_L_FILL(int64_t B, int64_t T) { return 4 * B * T + 2 * T; }      // the filler block of slot_math.h: 1 + 7 T words
WSI_HD inline int64_t SLOT_L_ORD(int64_t B, int64_t T) { return 4 * B * T + 9 * T + 1; }   // heavy[b], light[b] (positions in order_dst), so[b] (order_src), nreal
WSI_HD inline int64_t SLOT_L_WORDS(int64_t B, int64_t T) { return 4 * B * T + 9 * T + 1 + 3 * B + 1; }

// Returns 0, or a negative code when the counts do not fit the capacities (nothing the caller may then use; the tables stay inside their bounds).
WSI_HD inline int slot_layout(const int64_t* shape, const int32_t* ncnt, const int32_t* fcnt, int64_t* L, int32_t* readout_ptr, int32_t* chunk_row,
                              int32_t* chunk_seg, int32_t* seg_chunk, float* seg_counts, float* seg_inv_counts, float* seg_nonempty) {
    const int64_t T = shape[0], B = shape[1], b_cap = shape[2], chunk = shape[3], c_cap = shape[4];
    const int64_t G = b_cap + 1, K = T * G;
    int rc = 0;
    int64_t* node = L + SLOT_L_NODE(B, T);
    int64_t* edge = L + SLOT_L_EDGE(B, T);
    int64_t* csc = L + SLOT_L_CSC(B, T);
    int64_t* seg = L + SLOT_L_SEG(B, T);
    int64_t* nn = L + SLOT_L_N(B, T);
    int64_t* ee = L + SLOT_L_E(B, T);
    int64_t* fp = L + SLOT_L_FILL(B, T);
    int64_t* ord = L + SLOT_L_ORD(B, T);
    fp[0] = T;
    int64_t N = 0;
    for (int64_t t = 0; t < T; ++t) {
        const int64_t* s = slot_shape_type(shape, t);
        int64_t pre = 0, epre = 0;
        for (int64_t b = 0; b < B; ++b) {
            node[b * T + t] = s[SS_TOFF] + pre;
            seg[b * T + t] = s[SS_SOFF] + pre * s[SS_R];
            edge[b * T + t] = s[SS_EBASE] + epre;
            pre += ncnt[b * T + t];
            epre += fcnt[b * T + t];
        }
        nn[t] = pre;
        ee[t] = epre;
        if (pre > s[SS_NCAP] - 1 || epre > s[SS_ECAP]) { rc = -1; pre = pre > s[SS_NCAP] - 1 ? s[SS_NCAP] - 1 : pre; epre = epre > s[SS_ECAP] ? s[SS_ECAP] : epre; }
        int64_t* f = fp + 1 + t * 7;
        f[0] = s[SS_NCAP] - pre;                     // nf
        f[1] = s[SS_ECAP] - epre;                    // ef
        f[2] = s[SS_TOFF] + pre;                     // fb
        f[3] = s[SS_EBASE] + epre;                   // feb
        f[4] = s[SS_STYPE];
        f[5] = s[SS_R];
        N += s[SS_NCAP];
    }
    int64_t acc = 0;
    for (int64_t t = 0; t < T; ++t) {
        for (int64_t b = 0; b < B; ++b) {
            csc[b * T + t] = acc;
            acc += fcnt[B * T + b * T + t];
        }
        fp[1 + t * 7 + 6] = acc;                     // cfb
        for (int64_t d = 0; d < T; ++d)
            if (slot_shape_type(shape, d)[SS_STYPE] == t) acc += fp[1 + d * 7 + 1];
    }
    // processing orders: heavy destinations of every slide, then the light ones; sources apart
    acc = 0;
    for (int64_t b = 0; b < B; ++b) { ord[b] = acc; acc += fcnt[2 * B * T + b]; }
    for (int64_t b = 0; b < B; ++b) { ord[B + b] = acc; acc += fcnt[2 * B * T + B + b]; }
    int64_t acc_s = 0;
    for (int64_t b = 0; b < B; ++b) { ord[2 * B + b] = acc_s; acc_s += fcnt[2 * B * T + 2 * B + b]; }
    int64_t nreal = 0;
    for (int64_t t = 0; t < T; ++t) nreal += nn[t];
    ord[3 * B] = nreal;
    if (acc != nreal || acc_s != nreal) rc = rc ? rc : -2;
    // readout: segments (type, graph), their chunks of at most `chunk` rows padded to c_cap with empty chunks nobody owns
    int64_t p = 0, nc = 0;
    readout_ptr[0] = 0;
    seg_chunk[0] = 0;
    for (int64_t t = 0; t < T; ++t) {
        for (int64_t g = 0; g < G; ++g) {
            const int64_t k = t * G + g;
            const int64_t c = g < B ? (int64_t)ncnt[g * T + t] : (g < b_cap ? 0 : fp[1 + t * 7 + 0]);
            for (int64_t r = p; r < p + c; r += chunk) {
                if (nc < c_cap) { chunk_row[nc] = (int32_t)r; chunk_seg[nc] = (int32_t)k; ++nc; } else rc = rc ? rc : -3;
            }
            p += c;
            readout_ptr[k + 1] = (int32_t)p;
            seg_chunk[k + 1] = (int32_t)nc;
            seg_counts[k] = (float)c;
            seg_inv_counts[k] = c > 0 ? (float)(1.0 / (double)c) : 0.0f;
            seg_nonempty[k] = c > 0 ? 1.0f : 0.0f;
        }
    }
    for (int64_t i = nc; i <= c_cap; ++i) chunk_row[i] = (int32_t)N;
    for (int64_t i = nc; i < c_cap; ++i) chunk_seg[i] = (int32_t)(K - 1);
    return rc;
}

}  // namespace wsi
