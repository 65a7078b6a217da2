// Closed forms of the FILLER graph of a padded batch slot (graph.filler_graph), shared by the fill kernel (csrc/segment_table.hip) and by the
// host program that checks them against a sort (tests/slot_math_check.cpp).  Plain integer arithmetic, no device intrinsics.
//
// The filler has nf[t] nodes of every node type t and, for every destination type t with ef[t] > 0, ef[t] edges in relation slot 0 of t, whose
// source type is s = s0[t]: edge j in [0, ef[t]) runs from source j mod nf[s] to destination j mod nf[t].  Its plan follows the repository's
// conventions: CSR by (destination, relation slot) stable in j, CSC by source stable in CSR position.
//
// fp (int64 words): [T, then per type t: nf, ef, fb, feb, s0, R, cfb]
//   fb  global id of the filler's first node of type t          feb  CSR position of the filler's first edge into type t
//   s0  source type of relation slot 0 of t (-1: none)          R    relation slots of t
//   cfb CSC position of the first entry whose source is a filler node of type t
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

constexpr int FILLER_WORDS = 7;
enum { FP_NF = 0, FP_EF = 1, FP_FB = 2, FP_FEB = 3, FP_S0 = 4, FP_R = 5, FP_CFB = 6 };

WSI_HD inline const int64_t* filler_type(const int64_t* fp, int64_t t) { return fp + 1 + t * FILLER_WORDS; }

// first of the edges owned by node i when `e` edges are dealt round-robin to `n` nodes: node i owns q + (i < r) of them, (q, r) = divmod(e, n)
WSI_HD inline int64_t filler_start(int64_t i, int64_t e, int64_t n) {
    const int64_t q = e / n, r = e - q * n;
    return i * q + (i < r ? i : r);
}

// position p among the `e` edges sorted by owner (stable) -> owner i and the rank k among the owner's edges: the edge is j = i + k * n
WSI_HD inline void filler_owner(int64_t p, int64_t e, int64_t n, int64_t* i, int64_t* k) {
    const int64_t q = e / n, r = e - q * n;
    if (p < r * (q + 1)) { *i = p / (q + 1); *k = p - *i * (q + 1); }
    else { const int64_t x = p - r * (q + 1); *i = r + x / q; *k = x - (x / q) * q; }      // (q > 0 here: with q == 0 all e = r edges fall in the first branch)
}

// sum over i in [0, n) of floor((a * i + b) / m), a, b >= 0, m > 0 (the Euclid-like descent: O(log) steps)
WSI_HD inline int64_t floor_sum(int64_t n, int64_t m, int64_t a, int64_t b) {
    int64_t ans = 0;
    while (n > 0) {
        if (a >= m) { ans += (n - 1) * n / 2 * (a / m); a %= m; }
        if (b >= m) { ans += n * (b / m); b %= m; }
        const int64_t y = a * n + b;
        if (y < m) break;
        n = y / m;
        b = y % m;
        const int64_t tmp = m; m = a; a = tmp;
    }
    return ans;
}

// #{ m in [0, M) : (u + a * m) mod b < x },  0 <= x <= b
WSI_HD inline int64_t count_residue_below(int64_t M, int64_t a, int64_t b, int64_t u, int64_t x) {
    return M - (floor_sum(M, b, a, u + b - x) - floor_sum(M, b, a, u));
}

WSI_HD inline int64_t gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

// rowptr entry x in [0, nf * R] of the filler's segments of type t (node i = x / R, slot x mod R; only slot 0 holds edges)
WSI_HD inline int64_t filler_rowptr(const int64_t* fp, int64_t t, int64_t x) {
    const int64_t* f = filler_type(fp, t);
    const int64_t i = x / f[FP_R] + ((x % f[FP_R]) > 0 ? 1 : 0);
    return f[FP_FEB] + filler_start(i, f[FP_EF], f[FP_NF]);
}

// global source id of the filler edge at CSR position feb + p of destination type t
WSI_HD inline int64_t filler_src(const int64_t* fp, int64_t t, int64_t p) {
    const int64_t* f = filler_type(fp, t);
    const int64_t* fs = filler_type(fp, f[FP_S0]);
    int64_t i, k;
    filler_owner(p, f[FP_EF], f[FP_NF], &i, &k);
    return fs[FP_FB] + (i + k * f[FP_NF]) % fs[FP_NF];
}

// CSC entries of the filler sources of type s below source u (+ those of u itself that come from destination types below `upto`)
WSI_HD inline int64_t filler_csc_before(const int64_t* fp, int64_t s, int64_t u, int64_t upto) {
    const int64_t T = fp[0], ns = filler_type(fp, s)[FP_NF];
    int64_t acc = 0;
    for (int64_t t = 0; t < T; ++t) {
        const int64_t* f = filler_type(fp, t);
        if (f[FP_S0] == s && f[FP_EF] > 0) acc += filler_start(u + (t < upto ? 1 : 0), f[FP_EF], ns);
    }
    return acc;
}

// colptr entry of filler source u in [0, nf[s]] of type s
WSI_HD inline int64_t filler_colptr(const int64_t* fp, int64_t s, int64_t u) {
    return filler_type(fp, s)[FP_CFB] + filler_csc_before(fp, s, u, 0);
}

// the filler edge at CSR position feb + p of destination type t: where its CSC entry goes, and the entry (CSR edge id, global destination)
WSI_HD inline void filler_csc(const int64_t* fp, int64_t t, int64_t p, int64_t* slot, int64_t* eid, int64_t* dst) {
    const int64_t* f = filler_type(fp, t);
    const int64_t s = f[FP_S0];
    const int64_t* fs = filler_type(fp, s);
    const int64_t b = f[FP_NF], a = fs[FP_NF], e = f[FP_EF];
    int64_t i, k;
    filler_owner(p, e, b, &i, &k);
    const int64_t j = i + k * b, u = j % a, m = j / a;
    // source u sends the edges u + m' * a of this type, m' in [0, cnt); its CSC entries are ordered by CSR position = (destination, k):
    // ahead of this one are those with a smaller destination, and those with the same destination (m' = m mod P) and a smaller m'
    const int64_t cnt = e / a + (u < e % a ? 1 : 0);
    const int64_t P = b / gcd64(a, b);
    const int64_t rank = count_residue_below(cnt, a, b, u, i) + m / P;
    *slot = fs[FP_CFB] + filler_csc_before(fp, s, u, t) + rank;
    *eid = f[FP_FEB] + p;
    *dst = f[FP_FB] + i;
}

}  // namespace wsi
