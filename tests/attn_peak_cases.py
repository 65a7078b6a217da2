"""Cases, float64 restatement, fp32 emulation and norms for relation attention (csrc/heat_attn.hip) at scores where the softmax MAXIMUM matters:
one score of a segment 96 and more above the rest, whole segments near +100 or -100, stairs of 24.  Every other test of these kernels feeds them
K|Q = 0.5 randn, e_weight 0.7, e_bias 0.3: scores of standard deviation 0.25, where a softmax taken with a wrong maximum (a hub merge with wave
0's M, a dropped exp(m_p - M), an lse without its m) is still right.  No GPU needed; tests/test_attn_peak_cases.py holds every claim made here,
tests/test_attn_peak_kernels_gpu.py runs the kernels against it.

Graph (``graph_case()``): two hand-made slides through ``HeteroGraph.from_coo`` and ``batch``, three node types, the six HEAT relations.  Per
slide and type: control nodes (2 edges per destination and relation among themselves, quadratically skewed destinations), then the patterned
destinations of ``DSTS``, then a pool of dedicated source rows that send into patterned segments only - row p of the pool is edge p of every
segment fed from it (the CSR order is stable in the input order; ``GraphCase`` asserts it from ``oracle.kernel_ref.plan_edge_tables``).  Slide 0
holds the hub destinations (in-degree > 8), slide 1 the light ones.  One graph, two plans as in pooled_cases: ``plan`` (num_heavy == 0) and
``hub_plan`` (graph.HEAVY_DEGREE = 8).

Exact scores (``inputs``): every q and k entry is a multiple of 2^-2, e_weight = 0.5, e_bias = 0.25, sim a multiple of 2^-3, so ea = 0.5 sim +
0.25 is a multiple of 2^-4; with d_k a power of 4, 1/sqrt(d_k) is a power of two and every product and partial sum of a score is a small
integer times a power of two: exact in fp32 under any summation order, fused or not.  Construction: H[m] are the rows of the Sylvester-Hadamard
matrix of order d_k, flipped per head by a fixed +-1 vector.  Patterned destination number j of its slide has q[w]_h = +-(16 H[1+j] + H[8+j]);
a dedicated source has k[u]_h = sum_j +-(KA_j H[1+j] + KB_j H[8+j]) + noise from the rows {0, 15..}: q.k = (16 KA + KB) d_k exactly, and
score = (16 KA + KB) sqrt(d_k) ea.  The coarse part 16 KA carries the level (+-100), KB the fine part, so the mean k row a segment's g_q sums
is small next to its spread.  (512, 4) has d_k = 128: the same K, scores within sqrt(d_k) |ea| / 8 of the nominal ones and inexact in fp32.

Patterns, per (segment, head) (``patterns``): head i % H of segment i carries the segment's primary pattern of ``DSTS``, head (i+1) % H is
ordinary (|score| <= 2), the others rotate through ``FILL``.  'neg' segments (ea = -0.25: sim = -1) carry negative_ea and ordinary heads only.

Norms (``ratios``): bound = (tol + lse_term) * max(floor, largest reference entry); (tol, floor) are the project's.  lse_term, for a and t
only: 2^-23 max|lse_ref| (the stored lse and score - lse each round at 2^-24 |lse|), plus 2^-22 max|score_ref| where d_k is no power of 4.
g_e = (sum gea sim, sum gea) is held to 1e-4 max(1, |ref|) PLUS the same rounding carried to first order through g_s = a (ga - delta)
(``evaluate``: g_e_lse_term).  The saved lse makes every softmax sum to 1 + eps, |eps| <= 2^-23 |lse|, so a segment whose exact g_s vanish (one
peak: a = 1) or cancel (a plateau) leaves eps delta q.k / sqrt(d_k) in gea, with q.k / sqrt(d_k) = score / ea of order 200 - and g_e is ONE
number for the whole graph, so no block of its own scale can be formed for it.  The fp32 emulation is the witness (test_attn_peak_cases.py):
under the plain bound it reaches 29 times the bound ((256, 1)) with lse stored in fp32 and stays under it with lse kept in float64, all else equal."""
import functools
import math
from collections import OrderedDict

import numpy as np
import torch

from pooled_cases import Worst, heavy_degree, hub_mask          # noqa: F401  (shared with the GPU module)

SPECIALISED = [(128, 8), (128, 2), (256, 4), (256, 16), (256, 1), (512, 8), (512, 2), (512, 4)]
GENERIC = [(96, 6), (64, 1)]
CONFIGS = SPECIALISED + GENERIC
HGT_DH = (256, 4)
HUB_DEGREE = 8
E_WEIGHT, E_BIAS = 0.5, 0.25
HGT_E_BIAS = 0.25
OLD_E_WEIGHT, OLD_E_BIAS = 0.7, 0.3
QA = 16.0
GAP = 96.0
COOP_STEP, COOP_U, COOP_PARTS = 32, 4, 8          # kWavesPerBlock * kHeavyUnroll, kHeavyUnroll, kWavesPerBlock

RELATIONS = [("0", "pos", "0"), ("1", "pos", "0"), ("0", "pos", "1"), ("2", "neg", "1"), ("1", "neg", "2"), ("2", "pos", "2")]
REL_IN = {0: ((0, "pos"), (1, "pos")), 1: ((0, "pos"), (2, "neg")), 2: ((1, "neg"), (2, "pos"))}
CONTROL = ((60, 40, 30), (50, 35, 25))            # control nodes per slide and type
CONTROL_EDGES = 2                                 # per control destination and relation: few enough that EVERY node above the hub threshold is in the plan's heavy prefix
# (slide, type, ((length, primary pattern, position of the peak), (...))): the two segments in the order of REL_IN[type]
DSTS = [
    (0, 0, ((40, "peak", 2), (40, "peak", 30))),              # hub: wave 0's share; wave 7's share
    (0, 0, ((40, "peak", 37), (3, "peak", 1))),               # hub: second round; fewer than 4 edges (seven waves see none)
    (0, 0, ((32, "peak", 31), (33, "peak", 32))),             # hub: exactly 32 edges; 33 edges, the peak alone in round two
    (0, 0, ((12, "tie", 0), (9, "plateau_hi", 0))),
    (0, 0, ((20, "plateau_lo", 0), (11, "stairs_up", 0))),
    (0, 0, ((10, "stairs_down", 0), (0, None, 0))),            # hub with an empty segment
    (0, 1, ((16, "plateau_hi", 0), (12, "negative_ea", 9))),
    (1, 0, ((4, "peak", 0), (4, "peak", 3))),                 # light: first edge; last edge
    (1, 0, ((5, "peak", 4), (3, "peak", 2))),                 # light: last edge, length 1 mod 4; last edge, length 3
    (1, 0, ((7, "peak", 6), (1, "peak", 0))),                 # light: last edge, length 3 mod 4 (1 mod 2); a one-edge segment
    (1, 0, ((4, "tie", 0), (4, "plateau_hi", 0))),
    (1, 0, ((4, "plateau_lo", 0), (4, "stairs_up", 0))),
    (1, 1, ((6, "stairs_down", 0), (2, "negative_ea", 1))),
    (1, 2, ((5, "negative_ea", 4), (3, "tie", 0))),
]
FILL = ("plateau_hi", "ordinary", "peak_last", "tie", "plateau_lo", "stairs_down", "peak_first", "stairs_up")
FACTS = ("plain_plan_has_no_heavy", "hub_plan_has_heavy", "patterned_hubs_are_slide_0", "patterned_lights_are_slide_1",
         "dst_without_in_edges", "src_without_out_edges", "empty_segment_on_a_hub", "control_hub", "light_peak_last_len_1_mod_4",
         "light_peak_last_len_3_mod_4", "hub_peak_in_wave_0", "hub_peak_in_wave_7", "hub_peak_in_round_2", "hub_segment_of_32", "hub_segment_of_33",
         "hub_segment_under_4", "dedicated_sources_send_once_per_dst", "at_most_about_400_nodes", "every_node_above_the_threshold_is_a_hub")

# bound = (tol + lse_term) * max(floor, largest float64 entry): the project's (tol, floor) per tensor
BOUNDS = {"t": (1e-5, 0.0), "a": (1e-6, 1.0), "g_q": (1e-4, 0.0), "g_k": (1e-4, 0.0), "g_v": (1e-4, 0.0)}
LSE_TERM = ("a", "t")
G_E_TOL = 1e-4            # |error| <= 1e-4 max(1, |ref|) for each of the two e_linear gradients
LSE_TOL = 1e-6            # |error| <= 1e-6 max(1, |ref|) per entry
BLOCK_FLOOR = 1e-3        # a block's bound is formed from not less than this share of the tensor's largest entry (peaked segments: gradients of order e^-96)


def exact(D, H):
    """d_k a power of 4: 1/sqrt(d_k) a power of two."""
    r = math.isqrt(D // H)
    return r * r == D // H and r & (r - 1) == 0


# ------------------------------------------------------------------------------------------ graph
def _pool_sizes():
    size = [[0] * 3 for _ in CONTROL]
    for b, d, segs in DSTS:
        for (s, _), (L, _, _) in zip(REL_IN[d], segs):
            size[b][s] = max(size[b][s], L)
    return size


def _slide(b, gen):
    from wsi_hgnn_amd.graph import HeteroGraph
    pool = _pool_sizes()[b]
    dsts = [[i for i, x in enumerate(DSTS) if x[0] == b and x[1] == t] for t in range(3)]
    nn = OrderedDict((str(t), CONTROL[b][t] + len(dsts[t]) + pool[t]) for t in range(3))
    edges, sim = OrderedDict(), {}
    for s, kind, d in RELATIONS:
        ns, nd = CONTROL[b][int(s)], CONTROL[b][int(d)]
        u = torch.randint(0, ns, (CONTROL_EDGES * nd,), generator=gen)
        r = torch.rand(CONTROL_EDGES * nd, generator=gen, dtype=torch.float64)
        v = torch.clamp((nd * r * r).floor().long(), max=nd - 1)
        mag = torch.randint(1, 9, (CONTROL_EDGES * nd,), generator=gen).float() / 8
        us, vs = [u], [v]
        for i in dsts[int(d)]:
            for (ss, kk), (L, _, _) in zip(REL_IN[int(d)], DSTS[i][2]):
                if (str(ss), kk) == (s, kind) and L:
                    us.append(CONTROL[b][ss] + len(dsts[ss]) + torch.arange(L))
                    vs.append(torch.full((L,), CONTROL[b][int(d)] + dsts[int(d)].index(i)))
        edges[(s, kind, d)] = (torch.cat(us), torch.cat(vs))
        n_pat = edges[(s, kind, d)][0].numel() - CONTROL_EDGES * nd
        sim[(s, kind, d)] = torch.cat([mag if kind == "pos" else -mag, torch.zeros(n_pat)])       # (patterned edges: set per case, in CSR order)
    return HeteroGraph.from_coo(nn, edges, sim=sim)


class Segment:
    """One patterned softmax segment: ``index`` among them, destination ``w`` (number ``j`` of its slide), relation ``kind``, length ``L``,
    ``primary`` pattern with its peak at ``pos``, ``edges`` [L] CSR positions in segment order, ``seg`` its row of lse."""


class GraphCase:
    def __init__(self):
        from wsi_hgnn_amd import batch
        from wsi_hgnn_amd.graph import _build_plan
        from oracle import kernel_ref
        gen = torch.Generator().manual_seed(9600)
        self.g = g = batch([_slide(b, gen) for b in range(len(CONTROL))])
        self.plan = p = g.plan()
        with heavy_degree(HUB_DEGREE):
            self.hub_plan = _build_plan(g)
        self.rel_plan = _build_plan(g, per_relation_src=True)                    # HGT's layout: K|V rows per (relation, source node)
        self.n, self.E, self.S = p.num_nodes, p.num_edges, p.num_segs
        self.src = p.src.long()
        self.dst, self.seg = kernel_ref.plan_edge_tables(p)
        self.rowptr, self.node_seg = p.rowptr.long(), p.node_seg.long()
        self.seg_len = self.rowptr[1:] - self.rowptr[:-1]
        self.seg_dst = torch.repeat_interleave(torch.arange(self.n), self.node_seg[1:] - self.node_seg[:-1])
        self.inv_rd = p.inv_rd.double()
        self.sim0 = g.cat_edata_csr("sim").clone()
        B = len(CONTROL)
        counts = torch.stack([g.batch_num_nodes(t) for t in g.ntypes])            # [T, B]
        row_seg = torch.repeat_interleave(torch.arange(3 * B), counts.reshape(-1))
        self.type_of, self.slide_of = row_seg // B, row_seg % B
        first = torch.cumsum(counts.reshape(-1), 0) - counts.reshape(-1)          # first global row of (type, slide)
        self.hub = hub_mask(self.hub_plan)
        neg = ((self.type_of[self.dst] == 1) & (self.type_of[self.src] == 2)) | ((self.type_of[self.dst] == 2) & (self.type_of[self.src] == 1))
        self.neg = neg
        assert bool(((self.sim0 < 0) == neg)[self.sim0 != 0].all())
        # the patterned segments, located from the plan's own tables
        self.segments, self.pat_dst, self.pat_src = [], torch.zeros(self.n, dtype=torch.bool), torch.zeros(self.n, dtype=torch.bool)
        slot = [0] * B
        for b, d, segs in DSTS:
            j, slot[b] = slot[b], slot[b] + 1
            local = CONTROL[b][d] + sum(1 for x in DSTS[:DSTS.index((b, d, segs))] if x[0] == b and x[1] == d)
            w = int(first[d * B + b]) + local
            self.pat_dst[w] = True
            for (s, kind), (L, primary, pos) in zip(REL_IN[d], segs):
                if L == 0:
                    continue
                n_dst_s = sum(1 for x in DSTS if x[0] == b and x[1] == s)
                rows = int(first[s * B + b]) + CONTROL[b][s] + n_dst_s + torch.arange(L)
                e = ((self.dst == w) & (self.type_of[self.src] == s)).nonzero().view(-1)
                sg = Segment()
                sg.index, sg.w, sg.j, sg.kind, sg.L, sg.primary, sg.pos, sg.edges = len(self.segments), w, j, kind, L, primary, pos, e
                assert e.numel() == L and torch.equal(e, e[0] + torch.arange(L)), "a patterned segment is one contiguous run of CSR edges"
                sg.seg = int(self.seg[e[0]])
                assert bool((self.seg[e] == sg.seg).all()) and int(self.seg_len[sg.seg]) == L and int(self.rowptr[sg.seg]) == int(e[0])
                assert torch.equal(self.src[e], rows), "edge p of the segment reads row p of the pool"
                assert bool((self.neg[e] == (kind == "neg")).all())
                self.pat_src[rows] = True
                self.segments.append(sg)
        assert max(slot) <= 7, "signal rows 1..7 and 8..14 of the Hadamard matrix"
        self.pat_edge = self.pat_dst[self.dst]

    def facts(self):
        indeg, outdeg = torch.bincount(self.dst, minlength=self.n), torch.bincount(self.src, minlength=self.n)
        sg = self.segments
        hubseg = lambda L, pos=None: any(s.L == L and self.hub[s.w] and (pos is None or (s.primary == "peak" and pos(s.pos))) for s in sg)
        light_last = lambda m: any(s.primary == "peak" and not self.hub[s.w] and s.pos == s.L - 1 and s.L % 4 == m for s in sg)
        per_dst = torch.zeros(self.n, self.n, dtype=torch.long).index_put_((self.src[self.pat_edge], self.dst[self.pat_edge]),
                                                                           torch.ones(int(self.pat_edge.sum()), dtype=torch.long), accumulate=True)
        hubpeak = lambda f: any(s.primary == "peak" and self.hub[s.w] and s.L > COOP_STEP and f(s.pos) for s in sg)
        return {
            "plain_plan_has_no_heavy": self.plan.num_heavy == 0,
            "hub_plan_has_heavy": self.hub_plan.num_heavy > 0 and bool(self.hub.any()),
            "patterned_hubs_are_slide_0": bool(self.hub[self.pat_dst & (self.slide_of == 0)].all()),
            "patterned_lights_are_slide_1": not bool(self.hub[self.pat_dst & (self.slide_of == 1)].any()),
            "dst_without_in_edges": bool((indeg == 0).any()),
            "src_without_out_edges": bool((outdeg == 0).any()),
            "empty_segment_on_a_hub": bool((self.seg_len[self.hub[self.seg_dst]] == 0).any()),
            "control_hub": bool((self.hub & ~self.pat_dst).any()),
            "light_peak_last_len_1_mod_4": light_last(1),
            "light_peak_last_len_3_mod_4": light_last(3),
            "hub_peak_in_wave_0": hubpeak(lambda p: (p % COOP_STEP) // COOP_U == 0 and p < COOP_STEP),
            "hub_peak_in_wave_7": hubpeak(lambda p: (p % COOP_STEP) // COOP_U == COOP_PARTS - 1),
            "hub_peak_in_round_2": hubpeak(lambda p: p >= COOP_STEP),
            "hub_segment_of_32": hubseg(32, lambda p: p == 31),
            "hub_segment_of_33": hubseg(33, lambda p: p == 32),
            "hub_segment_under_4": any(s.L < 4 and self.hub[s.w] and s.primary == "peak" for s in sg),
            "dedicated_sources_send_once_per_dst": int(per_dst.max()) == 1 and not bool(self.pat_src[self.src[~self.pat_edge]].any()),
            "at_most_about_400_nodes": self.n <= 420,
            # (the heavy prefix is a top-k by in-degree: with more candidates than places, ties would decide which are taken)
            "every_node_above_the_threshold_is_a_hub": torch.equal(indeg > HUB_DEGREE, self.hub) and int(self.hub.sum()) < self.hub_plan.num_heavy,
        }


@functools.lru_cache(maxsize=None)
def graph_case():
    return GraphCase()


# ------------------------------------------------------------------------------------------ patterns
def patterns(H, hgt=False):
    """{(segment index, head): (pattern, position of its peak)} - see the module text."""
    out = {}
    for sg in graph_case().segments:
        i, L = sg.index, sg.L
        for h in range(H):
            if h == i % H:
                p, pos = sg.primary, sg.pos
            elif h == (i + 1) % H:
                p, pos = "ordinary", 0
            else:
                p, pos = FILL[(i + 3 * h) % len(FILL)], (5 * i + h) % L
            if sg.kind == "neg" and p != "ordinary" and not hgt:
                p = "negative_ea"
            if p == "peak_first":
                p, pos = "peak", 0
            if p == "peak_last":
                p, pos = "peak", L - 1
            if p == "tie" and L < 3:
                p = "peak"
            if p in ("stairs_up", "stairs_down") and L > 11:            # 11 steps of 24 span -120 .. 120
                p = "plateau_hi" if p == "stairs_up" else "plateau_lo"
            if hgt and p != "ordinary":
                p = "peak" if p in ("peak", "tie", "negative_ea") else "plateau_hi"
            if p in ("peak", "negative_ea") and h != i % H and pos == sg.pos and sg.primary == "peak" and L > 1:
                pos = (pos + 1) % L                                       # heads of a segment peak on different edges
            out[(i, h)] = (p, pos)
    return out


def _nominal(p, pos, sg, rng, step):
    """Nominal scores [L] of one (segment, head)."""
    L, i = sg.L, sg.index
    var = lambda lo, hi: step * rng.integers(math.ceil(lo / step), math.floor(hi / step) + 1, L)
    off = (0.0, 48.0, -48.0)[i % 3]
    if p == "ordinary":
        return var(-2, 2) * 1.0
    if p == "peak":
        s = -32.0 + off + var(-4, 4)
        s[pos] = 72.0 + off
        return s
    if p == "tie":
        s = -32.0 + off + var(-4, 4)
        free = [x for x in range(L) if not (sg.primary == "peak" and x == sg.pos)]      # (the primary's peak edge has another ea)
        s[free[i % (len(free) - 1)]] = s[free[-1]] = 72.0 + off
        return s
    if p == "plateau_hi":
        return 100.0 + var(-2, 2)
    if p == "plateau_lo":
        return -100.0 + var(-2, 2)
    if p == "stairs_up":
        return -120.0 + 24.0 * np.arange(L)
    if p == "stairs_down":
        return 120.0 - 24.0 * np.arange(L)
    if p == "negative_ea":                                                  # ea = -0.25: |q.k| <= 4096 leaves |score| <= 64 at d_k = 256
        s = -44.0 + var(-3, 0)
        s[pos] = 56.0
        return s
    raise KeyError(p)


def hadamard(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    assert h.shape[0] == n
    return h


# ------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def inputs(D, H, layout="heat"):
    """CPU tensors of one case: q [n, D], k [rows, D], v [rows, D], gt [n, D] (fp32, exactly representable where claimed), sim [E], ew, eb,
    the row of the K|V table every edge reads, and ``label`` {(segment, head): (pattern, peak position)}.
    layout 'heat': one row per node, e_weight 0.5;  'hgt': rows per (relation, source node) (``rel_plan``), e_weight 0 (ea = e_bias);
    'old': the inputs of the existing direct tests on this graph (0.5 randn, 0.7, 0.3)."""
    c = graph_case()
    dk = D // H
    hgt = layout == "hgt"
    rows_of_edge = c.rel_plan.src.long() if hgt else c.src
    n_rows = c.rel_plan.num_src_rows if hgt else c.n
    gen = torch.Generator().manual_seed(77000 + 10 * D + H + (5 if hgt else 0))
    rng = np.random.default_rng(88000 + 10 * D + H + (5 if hgt else 0))
    rnd = lambda *s: torch.randn(*s, generator=gen)
    x = {"v": rnd(n_rows, D), "gt": rnd(c.n, D), "rows_of_edge": rows_of_edge, "n_rows": n_rows, "layout": layout}
    if layout == "old":
        mag = torch.rand(c.E, generator=gen)
        x.update(q=rnd(c.n, D) * 0.5, k=rnd(n_rows, D) * 0.5, sim=torch.where(c.neg, -mag, mag), ew=torch.tensor([OLD_E_WEIGHT]),
                 eb=torch.tensor([OLD_E_BIAS]), label={})
        return x
    quant = lambda t: torch.round(t * 4) / 4
    q, k = quant(rnd(c.n, D) * 0.5).double().view(c.n, H, dk), quant(rnd(n_rows, D) * 0.5).double().view(n_rows, H, dk)
    sim = c.sim0.clone().double()
    ew, eb = (0.0, HGT_E_BIAS) if hgt else (E_WEIGHT, E_BIAS)
    had = torch.from_numpy(hadamard(dk))
    flip = torch.from_numpy(rng.choice([-1.0, 1.0], size=(H, dk)))               # the head's fixed +-1 vector
    noise_rows = np.array([0] + list(range(15, dk)))
    rho = math.sqrt(dk)
    label = patterns(H, hgt)
    ded = torch.unique(torch.cat([rows_of_edge[sg.edges] for sg in c.segments]))
    for u in ded.tolist():                                                        # dedicated rows: noise only, then the signals below
        for h in range(H):
            pick = rng.choice(noise_rows, size=min(4, noise_rows.size), replace=False)
            coef = rng.choice([-1.0, -0.75, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0], size=pick.size)
            k[u, h] = (torch.from_numpy(coef).unsqueeze(1) * had[pick]).sum(0)
    for sg in c.segments:
        rows = rows_of_edge[sg.edges]
        if hgt:
            ea = np.full(sg.L, HGT_E_BIAS)
        elif sg.kind == "neg":
            sim[sg.edges] = -1.0
            ea = np.full(sg.L, -0.25)
        else:
            sim[sg.edges] = 0.5
            if sg.primary == "peak":
                sim[sg.edges[sg.pos]] = 1.0                                       # ea = 0.75 on the primary's peak edge
            ea = E_WEIGHT * sim[sg.edges].numpy() + E_BIAS
        step = max(0.5, rho / 8) if exact(D, H) else 1.0
        for h in range(H):
            p, pos = label[(sg.index, h)]
            s = _nominal(p, pos, sg, rng, step)
            ka = np.round(s / (QA * rho * ea) * 4) / 4
            kb = np.round((s - QA * ka * rho * ea) / (rho * ea) * 4) / 4
            sign = 1.0 if (sg.j + h) % 2 == 0 else -1.0
            k[rows, h] += sign * (torch.from_numpy(ka).unsqueeze(1) * had[1 + sg.j] + torch.from_numpy(kb).unsqueeze(1) * had[8 + sg.j])
            q[sg.w, h] = sign * (QA * had[1 + sg.j] + had[8 + sg.j])
    k[ded] = k[ded] * flip
    q[c.pat_dst] = q[c.pat_dst] * flip
    assert bool((q * 4 == torch.round(q * 4)).all()) and bool((k * 4 == torch.round(k * 4)).all()) and bool((sim * 8 == torch.round(sim * 8)).all())
    x.update(q=q.float().reshape(c.n, D), k=k.float().reshape(n_rows, D), sim=sim.float(), ew=torch.tensor([ew]), eb=torch.tensor([eb]), label=label)
    assert torch.equal(x["q"].double().view(c.n, H, dk), q) and torch.equal(x["k"].double().view(n_rows, H, dk), k)
    return x


def pattern_facts(D, H, layout="heat"):
    """What the patterns promise, measured on the float64 scores of the case."""
    c, x = graph_case(), inputs(D, H, layout)
    ev = evaluate(D, H, layout)
    score, qk = ev["score"], ev["qk"]
    out = {"score_within_128": float(score.abs().max()) <= 128.0, "qk_within_4096": float(qk.abs().max()) <= 4096.0,
           "controls_are_near_uniform": float(score[~c.pat_edge].abs().max()) <= 8.0}
    seen = set()
    for sg in c.segments:
        kinds = [x["label"][(sg.index, h)][0] for h in range(H)]
        if H >= 2:
            out[f"segment {sg.index}: an ordinary and a patterned head"] = "ordinary" in kinds and any(p != "ordinary" for p in kinds)
        for h in range(H):
            p, pos = x["label"][(sg.index, h)]
            s = score[sg.edges, h]
            top = torch.sort(s, descending=True).values
            seen.add(p)
            if p in ("peak", "negative_ea"):
                ok = int(s.argmax()) == pos and (sg.L == 1 or float(top[0] - top[1]) >= GAP)
                if p == "negative_ea":
                    ok = ok and float(x["sim"][sg.edges[pos]]) < 0 and float(qk[sg.edges[pos], h]) < 0
            elif p == "tie":
                ok = float(top[0]) == float(top[1]) and float(top[1] - top[2]) >= GAP
            elif p in ("plateau_hi", "plateau_lo"):
                ok = float((s - (100.0 if p == "plateau_hi" else -100.0)).abs().max()) <= 4.0
            elif p in ("stairs_up", "stairs_down"):
                d = s[1:] - s[:-1]
                ok = bool(((d if p == "stairs_up" else -d) - 24.0).abs().max() <= (0.0 if exact(D, H) else 2.0)) if sg.L > 1 else True
            else:
                ok = float(s.abs().max()) <= 4.0
            out[f"segment {sg.index} head {h}: {p}"] = ok
    out["patterns_seen"] = seen
    return out


# ------------------------------------------------------------------------------------------ float64 restatement
def _segment_sum(values, index, size):
    return torch.zeros((size,) + values.shape[1:], dtype=values.dtype).index_add_(0, index, values)


def _backward(c, x, H, dk, f, q, k, ea, isd, qk, a, rows):
    """Everything behind the probabilities ``a`` in their dtype: the header's formulas."""
    n, n_rows = c.n, x["n_rows"]
    v, gt = f(x["v"]).view(n_rows, H, dk), f(x["gt"]).view(n, H, dk)
    inv_r = f(c.inv_rd)[c.dst].unsqueeze(1)
    t = _segment_sum(a.unsqueeze(-1) * v[rows], c.dst, n).reshape(n, -1) * f(c.inv_rd).unsqueeze(1)
    ga = (gt[c.dst] * v[rows]).sum(-1) * inv_r
    g_v = _segment_sum((a * inv_r).unsqueeze(-1) * gt[c.dst], rows, n_rows).reshape(n_rows, -1)
    delta = _segment_sum(a * ga, c.seg, c.S)
    g_s = a * (ga - delta[c.seg])
    gsc = g_s * ea.unsqueeze(1) * isd
    g_q = _segment_sum(gsc.unsqueeze(-1) * k[rows], c.dst, n).reshape(n, -1)
    g_k = _segment_sum(gsc.unsqueeze(-1) * q[c.dst], rows, n_rows).reshape(n_rows, -1)
    gea = (g_s * qk * isd).double()                                               # (the kernels add the fp32 terms in float64)
    g_e = torch.stack([(gea * c_sim(x).unsqueeze(1)).sum(), gea.sum()])
    return {"t": t, "ga": ga, "g_v": g_v, "g_q": g_q, "g_k": g_k, "g_e": g_e, "g_s": g_s}


def c_sim(x):
    return x["sim"].double()


@functools.lru_cache(maxsize=None)
def evaluate(D, H, layout="heat"):
    """The header's formulas in float64: score, lse, a, t, ga, g_q, g_k, g_v, g_e (and q.k)."""
    c, x = graph_case(), inputs(D, H, layout)
    dk, rows = D // H, x["rows_of_edge"]
    f = lambda t: t.double()
    q, k = f(x["q"]).view(c.n, H, dk), f(x["k"]).view(x["n_rows"], H, dk)
    ea = f(x["ew"]) * f(x["sim"]) + f(x["eb"])
    isd = 1.0 / math.sqrt(dk)
    qk = (q[c.dst] * k[rows]).sum(-1)
    score = qk * ea.unsqueeze(1) * isd
    smax = torch.full((c.S, H), -math.inf, dtype=torch.float64).scatter_reduce_(0, c.seg.unsqueeze(1).expand(-1, H), score, "amax")
    live = (c.seg_len > 0).unsqueeze(1)
    smax = torch.where(live, smax, torch.zeros_like(smax))
    lse = torch.where(live, smax + torch.log(_segment_sum(torch.exp(score - smax[c.seg]), c.seg, c.S)), smax)      # (an empty segment has none: 0 here)
    a = torch.exp(score - lse[c.seg])
    out = {"score": score, "qk": qk, "lse": lse, "a": a}
    out.update(_backward(c, x, H, dk, f, q, k, ea, isd, qk, a, rows))
    # what the rounding of the saved lse does to g_e, to first order.  a' = a (1 + eps_s + eta_e): eps_s, |eps_s| <= 2^-24 |lse|, the rounding of the
    # stored lse, common to the segment; eta_e, |eta_e| <= 2^-24 |score_e - lse|, that of the difference.  g_s' - g_s = (eps + eta_e) g_s - a (eps delta +
    # sum_f a_f eta_f ga_f), and g_e adds g_s x, x = q.k / sqrt(d_k) (times sim): the common part gives |eps_s| |G - delta X| per (segment, head) with
    # G = sum g_s x and X = sum a x, the per-edge part at most |eta|_e (|g_s| + a A) |x| with A = sum_f a_f |ga_f|
    xe, A = qk * isd, _segment_sum(a * out["ga"].abs(), c.seg, c.S)
    delta = _segment_sum(a * out["ga"], c.seg, c.S)
    term = []
    for wgt in (x["sim"].double().unsqueeze(1), torch.ones(c.E, 1, dtype=torch.float64)):
        G, X = _segment_sum(out["g_s"] * xe * wgt, c.seg, c.S), _segment_sum(a * xe * wgt, c.seg, c.S)
        common = (2.0 ** -24 * lse.abs() * (G - delta * X).abs()).sum()
        per_edge = (2.0 ** -24 * (score - lse[c.seg]).abs() * (out["g_s"].abs() + a * A[c.seg]) * (xe * wgt).abs()).sum()
        term.append(common + per_edge)
    out["g_e_lse_term"] = torch.stack(term)
    return out


def autograd(D, H, layout="heat"):
    """float64 autograd of oracle.kernel_ref on the same inputs."""
    from oracle import kernel_ref
    c, x = graph_case(), inputs(D, H, layout)
    ewd, ebd = x["ew"].double().requires_grad_(), x["eb"].double().requires_grad_()
    if layout == "hgt":
        qd, kvd = x["q"].double().requires_grad_(), torch.cat([x["k"], x["v"]], 1).double().requires_grad_()
        t = kernel_ref.relation_attention_ref(qd, kvd, ewd, ebd, c.rel_plan, x["sim"].double(), D, H)
        t.backward(x["gt"].double())
        g_q, g_k, g_v = qd.grad, kvd.grad[:, :D], kvd.grad[:, D:]
    else:
        kd = torch.cat([x["k"], x["q"], x["v"]], 1).double().requires_grad_()
        t = kernel_ref.heat_attention_ref(kd, ewd, ebd, c.plan, x["sim"].double(), D, H)
        t.backward(x["gt"].double())
        g_k, g_q, g_v = kd.grad[:, :D], kd.grad[:, D:2 * D], kd.grad[:, 2 * D:]
    return {"t": t.detach(), "g_q": g_q.clone(), "g_k": g_k.clone(), "g_v": g_v.clone(), "g_e": torch.stack([ewd.grad.reshape(()), ebd.grad.reshape(())])}


# ------------------------------------------------------------------------------------------ fp32 emulation
def light_unroll(D):
    """Edges a wave of the one-wave-per-node kernels keeps in flight (heat_attn.hip Unroll): 4 for D in {128, 256}, 2 for D = 512; the
    generic kernels take one edge at a time."""
    return {128: 4, 256: 4, 512: 2}.get(D, 1)


def emulate(D, H, layout="heat", hub=False, max_rule="online", lse_dtype=torch.float32):
    """The same formulas in fp32 as the kernels apply them: lse kept as ONE fp32 number per (segment, head), a = exp(score - lse) from it, the
    softmax walked online in kernel order - a one-wave destination in steps of U edges, a hub destination (``hub``: the hub plan's split) as
    eight parts that take four edges of every 32 and are merged in part order.
    max_rule: 'online' (the kernels);  'first_part' (the merge takes M from part 0);  'none' (no maximum is subtracted anywhere).
    lse_dtype float64: m + log l and score - lse are formed and kept in float64, everything else as before - what the saved FORMAT costs."""
    c, x = graph_case(), inputs(D, H, layout)
    dk, rows = D // H, x["rows_of_edge"]
    f = lambda t: t.float()
    q, k = x["q"].view(c.n, H, dk), x["k"].view(x["n_rows"], H, dk)
    ea = x["ew"] * x["sim"] + x["eb"]
    isd = np.float32(1.0) / np.sqrt(np.float32(dk))
    qk = (q[c.dst] * k[rows]).sum(-1)
    cc = ea * float(isd)
    score = qk * cc.unsqueeze(1)
    sc, vv = score.numpy(), x["v"].view(x["n_rows"], H, dk)[rows].numpy()
    lse = np.zeros((c.S, H), dtype=np.float32 if lse_dtype == torch.float32 else np.float64)
    tseg = np.zeros((c.S, H, dk), dtype=np.float32)
    U = light_unroll(D)
    hubs = c.hub if hub else torch.zeros(c.n, dtype=torch.bool)

    def walk(idx):
        m, l, acc = np.full(H, -np.inf, dtype=np.float32), np.zeros(H, dtype=np.float32), np.zeros((H, dk), dtype=np.float32)
        for e in idx:
            if max_rule == "none":
                mn = np.zeros(H, dtype=np.float32)
                scale = np.ones(H, dtype=np.float32)
            else:
                mn = np.maximum(m, sc[e])
                scale = np.exp(m - mn)
            pr = np.exp(sc[e] - mn)
            l = l * scale + pr
            acc = pr[:, None] * vv[e] + acc * scale[:, None]
            m = mn
        return m, l, acc

    with np.errstate(all="ignore"):
        for s in range(c.S):
            e0, e1 = int(c.rowptr[s]), int(c.rowptr[s + 1])
            if e0 == e1:
                continue
            if not bool(hubs[c.seg_dst[s]]):
                m, l, acc = walk([e + j for e in range(e0, e1, U) for j in range(U) if e + j < e1])
            else:
                parts = [walk([e + j for e in range(e0 + p * COOP_U, e1, COOP_STEP) for j in range(COOP_U) if e + j < e1]) for p in range(COOP_PARTS)]
                if max_rule == "none":
                    M = np.zeros(H, dtype=np.float32)
                elif max_rule == "first_part":
                    M = parts[0][0]
                else:
                    M = np.max(np.stack([pt[0] for pt in parts]), axis=0)
                l, acc = np.zeros(H, dtype=np.float32), np.zeros((H, dk), dtype=np.float32)
                for pm, pl, pa in parts:
                    fac = np.exp(pm - M) if max_rule != "none" else (pl > 0).astype(np.float32)
                    l = pl * fac + l
                    acc = pa * fac[:, None] + acc
                m = M
            lse[s] = m.astype(lse.dtype) + np.log(l.astype(lse.dtype))
            tseg[s] = acc * (np.float32(1.0) / l)[:, None]
    lse_t = torch.from_numpy(lse)
    t = _segment_sum(torch.from_numpy(tseg), c.seg_dst, c.n).reshape(c.n, -1) * c.inv_rd.float().unsqueeze(1)
    a = torch.exp(score.to(lse_dtype) - lse_t[c.seg]).float()
    out = {"score": score, "lse": lse_t, "a": a}
    out.update(_backward(c, x, H, dk, f, q, k, ea, float(isd), qk, a, rows))
    out["t"] = t
    return out


def summation_orders(D, H, layout="heat"):
    """The fp32 scores under forward, reversed and pairwise summation of the d_k products (numpy float32, one operation at a time)."""
    c, x = graph_case(), inputs(D, H, layout)
    dk, rows = D // H, x["rows_of_edge"]
    prod = (x["q"].view(c.n, H, dk)[c.dst] * x["k"].view(x["n_rows"], H, dk)[rows]).numpy().astype(np.float32)          # [E, H, dk]
    cc = ((x["ew"] * x["sim"] + x["eb"]).numpy().astype(np.float32) * (np.float32(1.0) / np.sqrt(np.float32(dk))))[:, None]
    fwd = np.zeros(prod.shape[:2], dtype=np.float32)
    rev = np.zeros(prod.shape[:2], dtype=np.float32)
    for i in range(dk):
        fwd = fwd + prod[:, :, i]
        rev = rev + prod[:, :, dk - 1 - i]
    pair = prod
    while pair.shape[2] > 1:
        pair = pair[:, :, 0::2] + pair[:, :, 1::2]
    return {"forward": torch.from_numpy(fwd * cc), "reversed": torch.from_numpy(rev * cc), "pairwise": torch.from_numpy(pair[:, :, 0] * cc)}


# ------------------------------------------------------------------------------------------ norms
def lse_term(ref, D, H):
    extra = 0.0 if exact(D, H) else 2.0 ** -22 * float(ref["score"].abs().max())
    return 2.0 ** -23 * float(ref["lse"].abs().max()) + extra


def block_ratios(got, ref, row_pat, row_hub, H, tol, floor):
    """{block name: error / bound} of ``got`` [rows, H * x] against float64 ``ref``: the whole tensor, and {patterned rows, other rows} x head x
    {hub rows, other rows}, each under the bound formed from the block's own largest reference entry - but from not less than BLOCK_FLOOR of the
    tensor's largest.  A non-finite entry makes its blocks infinite."""
    got, ref = got.detach().double().cpu().reshape(ref.shape[0], H, -1), ref.reshape(ref.shape[0], H, -1)
    assert got.shape == ref.shape
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf))
    top = float(ref.abs().max()) if ref.numel() else 0.0

    def one(e, r):
        bound = tol * max(floor, r, BLOCK_FLOOR * top)
        return 0.0 if e == 0.0 else (e / bound if bound > 0 else math.inf)
    out = {"all": one(float(err.max()), top) if err.numel() else 0.0}
    for pat in (True, False):
        for hub in (True, False):
            rows = (row_pat == pat) & (row_hub == hub)
            if not bool(rows.any()):
                continue
            e, r = err[rows].amax(dim=(0, 2)), ref[rows].abs().amax(dim=(0, 2))
            for h in range(H):
                out[f"{'patterned' if pat else 'other'} {'hub' if hub else 'light'} head {h}"] = one(float(e[h]), float(r[h]))
    return out


def all_ratios(got, ref, D, H, hub, layout="heat", g_e_term=True):
    """{tensor: {block: error / bound}} for every tensor of ``got`` that BOUNDS, lse or g_e names.  The blocks split by ``case.hub`` whichever plan
    the call ran (``hub``: the cooperative kernels did take those rows), so that the figures of the two plans compare; a K|V row is patterned
    where it feeds a patterned segment and a hub row where it feeds a hub."""
    c = graph_case()
    rows_of_edge = inputs(D, H, layout)["rows_of_edge"]
    term = lse_term(ref, D, H)
    src_pat = torch.zeros(ref["g_k"].shape[0], dtype=torch.bool)
    src_pat[rows_of_edge[c.pat_edge]] = True
    src_hub = torch.zeros(ref["g_k"].shape[0], dtype=torch.bool)
    src_hub[rows_of_edge[c.hub[c.dst]]] = True
    out = {}
    for name, x in got.items():
        if name == "g_e":
            g, r = x.detach().double().cpu().reshape(-1), ref["g_e"]
            out[name] = {"all": max(_scalar_ratio(g[i].item(), r[i].item(), G_E_TOL, ref["g_e_lse_term"][i].item() if g_e_term else 0.0) for i in range(2))}
        elif name == "lse":
            g, r = x.detach().double().cpu()[c.seg_len > 0], ref["lse"][c.seg_len > 0]
            e = torch.where(torch.isfinite(g), (g - r).abs(), torch.full_like(r, math.inf))
            out[name] = {"all": float((e / (LSE_TOL * r.abs().clamp(min=1.0))).max())}
        elif name in BOUNDS:
            tol, floor = BOUNDS[name]
            tol = tol + (term if name in LSE_TERM else 0.0)
            if name == "a":
                out[name] = block_ratios(x, ref[name], c.pat_edge, c.hub[c.dst], H, tol, floor)
            elif name in ("g_k", "g_v"):
                out[name] = block_ratios(x, ref[name], src_pat, src_hub, H, tol, floor)
            else:
                out[name] = block_ratios(x, ref[name], c.pat_dst, c.hub, H, tol, floor)
    return out


def _scalar_ratio(g, r, tol, extra=0.0):
    return abs(g - r) / (tol * max(1.0, abs(r)) + extra) if math.isfinite(g) else math.inf


def ratios(got, ref, D, H, hub, layout="heat", g_e_term=True):
    """{tensor: the largest error / bound over the whole tensor and all its blocks}.  g_e_term False: g_e under the plain 1e-4 max(1, |ref|)."""
    return {name: max(blocks.values()) for name, blocks in all_ratios(got, ref, D, H, hub, layout, g_e_term).items()}


def sum_a_ratio(a, ref):
    """Per (segment, head): |sum a - 1| over 4 * 2^-23 * max(1, |lse|), the largest."""
    c = graph_case()
    s = _segment_sum(a.detach().double().cpu(), c.seg, c.S)
    live = c.seg_len > 0
    return float(((s[live] - 1.0).abs() / (4 * 2.0 ** -23 * ref["lse"][live].abs().clamp(min=1.0))).max())
