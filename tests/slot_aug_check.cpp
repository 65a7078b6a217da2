// Stand-alone host check of csrc/slot_layout.h (the layout of an augmented slot from device-side counts) against a plain re-implementation of
// graph.SlotBatch's host arithmetic on random count tables: zeros, empty (slide, type) segments, B < b_cap, types without incoming relation.
// Built and run by tests/test_batch_slot_augment.py with -fsanitize=address,undefined; exit status 0 = every table agreed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "slot_layout.h"

using namespace wsi;

static uint64_t state = 0x9E3779B97F4A7C15ull;
static int64_t rnd(int64_t n) {           // uniform in [0, n)
    state ^= state << 13; state ^= state >> 7; state ^= state << 17;
    return n > 0 ? (int64_t)(state % (uint64_t)n) : 0;
}

struct Ref {
    std::vector<int64_t> node, edge, csc, seg, n, e, nf, ef, fb, feb, cfb, heavy, light, so, readout_ptr, chunk_row, chunk_seg, seg_chunk;
    std::vector<float> cnt, inv, non;
    int64_t nreal;
};

int main() {
    int bad = 0, cases = 0;
    for (int it = 0; it < 4000; ++it) {
        const int64_t T = 1 + rnd(4), b_cap = 1 + rnd(3), B = 1 + rnd(b_cap), chunk = 1 + rnd(it % 3 == 0 ? 4 : 128), G = b_cap + 1, K = T * G;
        std::vector<int64_t> n_cap(T), e_cap(T), R(T), stype(T), toff(T + 1, 0), ebase(T + 1, 0), soff(T + 1, 0);
        std::vector<int32_t> ncnt(B * T), fcnt(2 * B * T + 3 * B);
        // counts first (zeros with probability 1/4), capacities around them
        for (int64_t t = 0; t < T; ++t) {
            R[t] = rnd(4);                                           // 0: no incoming relation, the type holds no edge
            stype[t] = R[t] ? rnd(T) : -1;
            int64_t ns = 0, es = 0;
            for (int64_t b = 0; b < B; ++b) {
                ncnt[b * T + t] = rnd(4) == 0 ? 0 : (int32_t)rnd(300);
                fcnt[b * T + t] = (R[t] == 0 || rnd(4) == 0) ? 0 : (int32_t)rnd(900);
                ns += ncnt[b * T + t];
                es += fcnt[b * T + t];
            }
            n_cap[t] = ns + 1 + (rnd(3) == 0 ? 0 : rnd(200));
            e_cap[t] = R[t] ? es + (rnd(3) == 0 ? 0 : rnd(500)) : 0;
        }
        for (int64_t t = 0; t < T; ++t) {
            toff[t + 1] = toff[t] + n_cap[t];
            ebase[t + 1] = ebase[t] + e_cap[t];
            soff[t + 1] = soff[t] + n_cap[t] * R[t];
        }
        const int64_t N = toff[T], E = ebase[T];
        // CSC entries out of (b, t): any split of the edges whose source type is t (the filler's come on top); order lists: a split of the nodes
        {
            int64_t total = 0;
            for (int64_t i = 0; i < B * T; ++i) total += fcnt[i];
            for (int64_t i = 0; i < B * T; ++i) { const int64_t c = i + 1 < B * T ? rnd(total + 1) : total; fcnt[B * T + i] = (int32_t)c; total -= c; }
        }
        for (int64_t b = 0; b < B; ++b) {
            int64_t nb = 0;
            for (int64_t t = 0; t < T; ++t) nb += ncnt[b * T + t];
            const int64_t h = rnd(nb + 1);
            fcnt[2 * B * T + b] = (int32_t)h;
            fcnt[2 * B * T + B + b] = (int32_t)(nb - h);
            fcnt[2 * B * T + 2 * B + b] = (int32_t)nb;
        }
        int64_t c_cap = 0;
        for (int64_t t = 0; t < T; ++t) c_cap += (n_cap[t] + chunk - 1) / chunk + G;
        std::vector<int64_t> shape = {T, B, b_cap, chunk, c_cap};
        for (int64_t t = 0; t < T; ++t) { const int64_t w[7] = {n_cap[t], e_cap[t], toff[t], ebase[t], stype[t], R[t], soff[t]}; shape.insert(shape.end(), w, w + 7); }
        // ---- the header under test (guard words around every table)
        const int64_t LW = SLOT_L_WORDS(B, T);
        std::vector<int64_t> L(LW + 2, -77);
        std::vector<int32_t> rp(K + 1 + 2, -77), crow(c_cap + 1 + 2, -77), cseg(c_cap + 2, -77), schunk(K + 1 + 2, -77);
        std::vector<float> cnt(K + 2, -77.f), inv(K + 2, -77.f), non(K + 2, -77.f);
        const int rc = slot_layout(shape.data(), ncnt.data(), fcnt.data(), L.data() + 1, rp.data() + 1, crow.data() + 1, cseg.data() + 1, schunk.data() + 1,
                                   cnt.data() + 1, inv.data() + 1, non.data() + 1);
        // ---- plain re-implementation (graph.SlotBatch)
        Ref r;
        r.node.assign(B * T, 0); r.edge.assign(B * T, 0); r.csc.assign(B * T, 0); r.seg.assign(B * T, 0);
        r.n.assign(T, 0); r.e.assign(T, 0);
        for (int64_t t = 0; t < T; ++t)
            for (int64_t b = 0; b < B; ++b) {
                r.node[b * T + t] = toff[t] + r.n[t];
                r.seg[b * T + t] = soff[t] + r.n[t] * R[t];
                r.edge[b * T + t] = ebase[t] + r.e[t];
                r.n[t] += ncnt[b * T + t];
                r.e[t] += fcnt[b * T + t];
            }
        for (int64_t t = 0; t < T; ++t) { r.nf.push_back(n_cap[t] - r.n[t]); r.ef.push_back(e_cap[t] - r.e[t]); r.fb.push_back(toff[t] + r.n[t]); r.feb.push_back(ebase[t] + r.e[t]); }
        int64_t acc = 0;
        for (int64_t t = 0; t < T; ++t) {
            for (int64_t b = 0; b < B; ++b) { r.csc[b * T + t] = acc; acc += fcnt[B * T + b * T + t]; }
            r.cfb.push_back(acc);
            for (int64_t d = 0; d < T; ++d) if (stype[d] == t) acc += r.ef[d];
        }
        if (acc != E) { std::printf("case %d: the reference's CSC total %lld != E %lld\n", it, (long long)acc, (long long)E); ++bad; continue; }
        int64_t hacc = 0, sacc = 0;
        for (int64_t b = 0; b < B; ++b) { r.heavy.push_back(hacc); hacc += fcnt[2 * B * T + b]; }
        for (int64_t b = 0; b < B; ++b) { r.light.push_back(hacc); hacc += fcnt[2 * B * T + B + b]; }
        for (int64_t b = 0; b < B; ++b) { r.so.push_back(sacc); sacc += fcnt[2 * B * T + 2 * B + b]; }
        r.nreal = 0;
        for (int64_t t = 0; t < T; ++t) r.nreal += r.n[t];
        r.readout_ptr.push_back(0);
        r.seg_chunk.push_back(0);
        for (int64_t t = 0; t < T; ++t)
            for (int64_t g = 0; g < G; ++g) {
                const int64_t c = g < B ? ncnt[g * T + t] : (g == b_cap ? r.nf[t] : 0);
                const int64_t a = r.readout_ptr.back(), e = a + c;
                int64_t row = a;
                while (row < e) { r.chunk_row.push_back(row); r.chunk_seg.push_back(t * G + g); row = row + chunk < e ? row + chunk : e; }
                r.readout_ptr.push_back(e);
                r.seg_chunk.push_back((int64_t)r.chunk_row.size());
                r.cnt.push_back((float)c); r.inv.push_back(c ? (float)(1.0 / (double)c) : 0.f); r.non.push_back(c ? 1.f : 0.f);
            }
        const int64_t pad = c_cap - (int64_t)r.chunk_seg.size();
        if (pad < 0) { std::printf("case %d: chunk capacity exceeded\n", it); ++bad; continue; }
        for (int64_t i = 0; i < pad + 1; ++i) r.chunk_row.push_back(N);
        for (int64_t i = 0; i < pad; ++i) r.chunk_seg.push_back(K - 1);
        // ---- compare
        int miss = rc != 0;
        const int64_t* Lp = L.data() + 1;
        for (int64_t i = 0; i < B * T; ++i)
            miss += Lp[SLOT_L_NODE(B, T) + i] != r.node[i] || Lp[SLOT_L_EDGE(B, T) + i] != r.edge[i] || Lp[SLOT_L_CSC(B, T) + i] != r.csc[i] ||
                    Lp[SLOT_L_SEG(B, T) + i] != r.seg[i];
        const int64_t* fp = Lp + SLOT_L_FILL(B, T);
        miss += fp[0] != T;
        for (int64_t t = 0; t < T; ++t) {
            const int64_t* f = fp + 1 + t * 7;
            miss += Lp[SLOT_L_N(B, T) + t] != r.n[t] || Lp[SLOT_L_E(B, T) + t] != r.e[t] || f[0] != r.nf[t] || f[1] != r.ef[t] || f[2] != r.fb[t] ||
                    f[3] != r.feb[t] || f[4] != stype[t] || f[5] != R[t] || f[6] != r.cfb[t];
        }
        const int64_t* ord = Lp + SLOT_L_ORD(B, T);
        for (int64_t b = 0; b < B; ++b) miss += ord[b] != r.heavy[b] || ord[B + b] != r.light[b] || ord[2 * B + b] != r.so[b];
        miss += ord[3 * B] != r.nreal;
        for (int64_t i = 0; i <= K; ++i) miss += rp[1 + i] != r.readout_ptr[i] || schunk[1 + i] != r.seg_chunk[i];
        for (int64_t i = 0; i <= c_cap; ++i) miss += crow[1 + i] != r.chunk_row[i];
        for (int64_t i = 0; i < c_cap; ++i) miss += cseg[1 + i] != r.chunk_seg[i];
        for (int64_t i = 0; i < K; ++i)
            miss += std::memcmp(&cnt[1 + i], &r.cnt[i], 4) != 0 || std::memcmp(&inv[1 + i], &r.inv[i], 4) != 0 || std::memcmp(&non[1 + i], &r.non[i], 4) != 0;
        // nothing written outside the tables
        miss += L[0] != -77 || L[LW + 1] != -77 || rp[0] != -77 || rp[K + 2] != -77 || crow[0] != -77 || crow[c_cap + 2] != -77 || cseg[0] != -77 ||
                cseg[c_cap + 1] != -77 || schunk[0] != -77 || schunk[K + 2] != -77 || cnt[0] != -77.f || cnt[K + 1] != -77.f || inv[0] != -77.f ||
                inv[K + 1] != -77.f || non[0] != -77.f || non[K + 1] != -77.f;
        if (miss) { std::printf("case %d (T %lld, B %lld of %lld): %d mismatches\n", it, (long long)T, (long long)B, (long long)b_cap, miss); ++bad; }
        ++cases;
    }
    std::printf("%d count tables, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
