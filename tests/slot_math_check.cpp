// Stand-alone host check of csrc/slot_math.h (the filler graph's closed forms) against an explicit stable sort.
// Built and run by tests/test_batch_slot.py with -fsanitize=address,undefined; exit status 0 = every table agreed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "slot_math.h"

using namespace wsi;

static int check(int T, const std::vector<int64_t>& nf, const std::vector<int64_t>& ef, const std::vector<int64_t>& s0, const std::vector<int64_t>& R) {
    // global layout of a graph that is the filler alone, shifted by arbitrary bases so that the offsets are exercised
    std::vector<int64_t> fp(1 + T * FILLER_WORDS), fb(T), feb(T), cfb(T);
    int64_t nb = 5, eb = 11;
    for (int t = 0; t < T; ++t) { fb[t] = nb; nb += nf[t] + 3; feb[t] = eb; eb += ef[t] + 2; }
    // brute force: edges in CSR order (destination type, destination, j), then a stable sort by global source
    struct Edge { int64_t eid, src, dst; };
    std::vector<Edge> edges;
    std::vector<std::vector<int64_t>> rowptr(T);
    for (int t = 0; t < T; ++t) {
        std::vector<int64_t> j(ef[t]);
        std::iota(j.begin(), j.end(), 0);
        std::stable_sort(j.begin(), j.end(), [&](int64_t x, int64_t y) { return x % nf[t] < y % nf[t]; });
        std::vector<int64_t> deg(nf[t], 0);
        for (int64_t p = 0; p < ef[t]; ++p) {
            edges.push_back({feb[t] + p, fb[s0[t]] + j[p] % nf[s0[t]], fb[t] + j[p] % nf[t]});
            deg[j[p] % nf[t]]++;
        }
        int64_t acc = feb[t];
        for (int64_t i = 0; i < nf[t]; ++i)
            for (int64_t sl = 0; sl < R[t]; ++sl) { rowptr[t].push_back(acc); if (sl == 0) acc += deg[i]; }
    }
    std::vector<Edge> csc = edges;
    std::stable_sort(csc.begin(), csc.end(), [](const Edge& x, const Edge& y) { return x.src < y.src; });
    int64_t cb = 7;
    {
        size_t pos = 0;
        for (int s = 0; s < T; ++s) {
            cfb[s] = cb + (int64_t)pos;
            while (pos < csc.size() && csc[pos].src < fb[s] + nf[s]) ++pos;
        }
    }
    fp[0] = T;
    for (int t = 0; t < T; ++t) {
        int64_t* f = fp.data() + 1 + t * FILLER_WORDS;
        f[FP_NF] = nf[t]; f[FP_EF] = ef[t]; f[FP_FB] = fb[t]; f[FP_FEB] = feb[t]; f[FP_S0] = s0[t]; f[FP_R] = R[t]; f[FP_CFB] = cfb[t];
    }
    int bad = 0;
    size_t e0 = 0;
    std::vector<int64_t> got_eid(csc.size(), -1), got_dst(csc.size(), -1);
    for (int t = 0; t < T; ++t) {
        for (int64_t x = 0; x < nf[t] * R[t]; ++x) bad += filler_rowptr(fp.data(), t, x) != rowptr[t][x];
        for (int64_t p = 0; p < ef[t]; ++p) {
            bad += filler_src(fp.data(), t, p) != edges[e0 + p].src;
            int64_t slot, eid, dst;
            filler_csc(fp.data(), t, p, &slot, &eid, &dst);
            slot -= cb;
            if (slot < 0 || slot >= (int64_t)csc.size() || got_eid[slot] != -1) { ++bad; continue; }
            got_eid[slot] = eid; got_dst[slot] = dst;
        }
        e0 += ef[t];
    }
    for (size_t c = 0; c < csc.size(); ++c) bad += (got_eid[c] != csc[c].eid) + (got_dst[c] != csc[c].dst);
    for (int s = 0; s < T; ++s) {
        size_t pos = (size_t)(cfb[s] - cb);
        for (int64_t u = 0; u <= nf[s]; ++u) {
            while (pos < csc.size() && csc[pos].src < fb[s] + u) ++pos;
            bad += filler_colptr(fp.data(), s, u) != cb + (int64_t)pos;
        }
    }
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    // floor_sum against the plain sum
    for (int64_t n = 0; n < 9; ++n) for (int64_t m = 1; m < 8; ++m) for (int64_t a = 0; a < 9; ++a) for (int64_t b = 0; b < 17; ++b) {
        int64_t ref = 0;
        for (int64_t i = 0; i < n; ++i) ref += (a * i + b) / m;
        bad += floor_sum(n, m, a, b) != ref;
    }
    unsigned seed = 12345;
    auto rnd = [&](int lo, int hi) { seed = seed * 1664525u + 1013904223u; return lo + (int)((seed >> 8) % (unsigned)(hi - lo + 1)); };
    const int64_t small[] = {1, 2, 3, 4, 6, 7, 12, 30};
    const int64_t es[] = {0, 1, 2, 5, 6, 11, 12, 29, 60, 211, 600};
    for (int it = 0; it < 4000; ++it) {
        const int T = rnd(1, 3);
        std::vector<int64_t> nf(T), ef(T), s0(T), R(T);
        for (int t = 0; t < T; ++t) { nf[t] = small[rnd(0, 7)]; ef[t] = es[rnd(0, 10)]; s0[t] = rnd(0, T - 1); R[t] = rnd(1, 3); }
        bad += check(T, nf, ef, s0, R);
        ++cases;
    }
    // one filler node carrying every edge, sources spread; and the reverse
    bad += check(2, {1, 40}, {700, 0}, {1, 0}, {2, 1});
    bad += check(2, {40, 1}, {700, 35}, {1, 1}, {2, 2});
    std::printf("slot_math_check: %d cases, %d mismatches\n", cases + 2, bad);
    return bad ? 1 : 0;
}
