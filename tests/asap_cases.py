"""Cases and float64 references for the ASAPPooling kernels of csrc/asap.hip (wsi_csr_gather_max_*, wsi_asap_attend_*, wsi_graph_topk, wsi_stas).

Plain module, no GPU.  The builders live here; tests/test_asap_cases.py proves on the CPU, with the reference formulations only, that each
case has the property it exists for, and tests/test_asap_kernels_gpu.py runs the kernels on them.  Naming follows ops.EdgeCSR(group, other, n):
an edge (i, j) is grouped at the node i that aggregates it (its CSR *segment*, the ``rowptr`` range of i) and gathers node j (the ``colptr``
range of j holds the edges that gather j)."""
import torch

SLOPE = 0.2
AS_WAVES = 4                        # csrc/asap.hip: nodes per workgroup of the edge kernels
TK_TILE, TK_CHUNK = 1024, 8192      # csrc/asap.hip: LDS tile and grid.y chunk of wsi_graph_topk
ST_SMALL_ROWS, ST_LARGE_ROWS = 384, 1536      # csrc/asap.hip: most distinct columns a row may hold in the 512- / 2048-slot launch of wsi_stas

# ------------------------------------------------------------------------------------------------ the edge graph
EDGE_N = 259
LONELY = 0                                                   # only its self loop
LONG = {1: 63, 2: 64, 3: 65, 4: 128, 5: 129}                 # the 64-lane stride of the attention kernels from both sides, one and two full trips
TIED, TIED_SOURCES = 6, 75                                   # 75 sources listed twice each: 150 edges, exact ties in the max
TAIL, TAIL_DEG = EDGE_N - 1, 70                              # the lone node of the last workgroup
NO_SEGMENT = (9, 10, 23, 60, 61, 62, 141, 200, 255)          # nothing grouped at them; 9, 10, 61 sit strictly inside a block of four
NEVER_GATHERED = (7, 12, 33, 64, 65, 99, 128, 129, 191, 230, 257)
NAMED_ROWS = (0, 1, 2, 3, 4, 5, 6, TAIL)                     # rows that also get a bound of their own


def edge_graph(seed=2024):
    """(n, i, j): the edge list of the module docstring's graph, shuffled."""
    gen = torch.Generator().manual_seed(seed)
    n = EDGE_N
    gatherable = torch.tensor([v for v in range(n) if v not in NEVER_GATHERED])
    others = gatherable[gatherable != TAIL]
    ii, jj = [torch.tensor([LONELY])], [torch.tensor([LONELY])]

    def feed(v, k, first=None):                              # k edges grouped at v from k distinct gatherable nodes
        s = others[torch.randperm(others.numel(), generator=gen)[:k]]
        if first is not None:
            s[0] = first
        ii.append(torch.full((s.numel(),), v)); jj.append(s)
        return s

    for v, k in LONG.items():
        feed(v, k, first=TAIL if v in (2, 5) else None)      # the tail node is gathered by others
    s = feed(TIED, TIED_SOURCES)
    ii.append(torch.full((TIED_SOURCES,), TIED)); jj.append(s)
    feed(TAIL, TAIL_DEG)
    rest = torch.tensor([v for v in range(7, n - 1) if v not in NO_SEGMENT])
    d = torch.repeat_interleave(rest, torch.randint(0, 6, (rest.numel(),), generator=gen))
    s = gatherable[torch.randint(0, gatherable.numel(), (d.numel(),), generator=gen)]
    m = d.numel() // 10
    ii += [d, d[:m]]; jj += [s, s[:m]]                       # a tenth of them twice
    i, j = torch.cat(ii), torch.cat(jj)
    o = torch.randperm(i.numel(), generator=gen)
    return n, i[o].contiguous(), j[o].contiguous()


def small_graphs():
    """name -> (n, i, j): one node with a self loop, a directed ring of five, six nodes without an edge."""
    ring = torch.arange(5)
    empty = torch.zeros(0, dtype=torch.int64)
    return {"one_node": (1, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64)),
            "ring5": (5, ring, (ring + 1) % 5),
            "no_edges": (6, empty, empty.clone())}


def degrees(n, i, j):
    """(segment length per node, number of edges that gather each node)"""
    return torch.bincount(i, minlength=n), torch.bincount(j, minlength=n)


def csr_order(i):
    """CSR position -> input edge: ops.EdgeCSR sorts stably, so inside a segment the edges keep their input order."""
    return torch.sort(i, stable=True).indices


REGIMES = ("normal", "peaked", "grid", "grid+4096")


def scores(regime, n, seed=0):
    """(a, b) [n, 1] fp32 of a score regime.  ``grid``: multiples of 2^-10 in [0, 8), every a[i] + b[j] positive and exact in fp32;
    ``grid+4096``: the same values with 4096 added to a - sums (< 2^13 in units of 2^-10: 23 bits) and their differences are still exact,
    so the softmax is that of ``grid`` itself."""
    gen = torch.Generator().manual_seed(77 + seed)
    if regime in ("normal", "peaked"):
        a, b = torch.randn(n, 1, generator=gen), torch.randn(n, 1, generator=gen)
        return (a, b) if regime == "normal" else (30 * a, 30 * b)
    a = torch.randint(0, 8 * 1024, (n, 1), generator=gen).float() / 1024
    b = torch.randint(0, 8 * 1024, (n, 1), generator=gen).float() / 1024
    return (a + 4096.0 if regime == "grid+4096" else a), b


def features(n, D, seed=0):
    """(x, g_max, g_out) [n, D] fp32: the gathered rows and the gradients fed to the two ops."""
    gen = torch.Generator().manual_seed(1000 * D + n + seed)
    return torch.randn(n, D, generator=gen), torch.randn(n, D, generator=gen), torch.randn(n, D, generator=gen)


# ------------------------------------------------------------------------------------------------ references of the edge kernels
def edge_reference(i, j, x, a, b, g_out, slope=SLOPE, dtype=torch.float64):
    """The eager scatter formulation of pooling/ASAP.py:158-179 on the CPU in ``dtype`` (float64: the reference; float32: the yardstick of the
    4x rule), on the SAME fp32 inputs.  The side of leaky_relu's kink comes from the fp32 sum a32[i] + b32[j] - one IEEE add, identical on
    host and device; exactly zero goes to the slope side as in the kernels' leaky().
    Returns a dict: mx [n, D] (0 for an empty segment), out [n, D], score [E] (input edge order), gterm [E] (|score_e * g_out[i_e] . x[j_e]|: the
    size of the per-edge term whose centred sums are g_a and g_b), g_x [n, D], g_a / g_b (the shapes of a / b) for the loss sum(out * g_out)."""
    n, D = x.shape
    xr, ar, br = (t.detach().to(dtype).requires_grad_() for t in (x, a, b))
    xj = xr[j]
    mx = torch.zeros(n, D, dtype=dtype).scatter_reduce(0, i.view(-1, 1).expand(-1, D), xj.detach(), reduce="amax", include_self=False)
    pos = (a.detach().float().view(-1)[i] + b.detach().float().view(-1)[j]) > 0
    pre = (ar.view(-1)[i] + br.view(-1)[j])
    s = torch.where(pos, pre, pre * slope)
    smax = torch.full((n,), float("-inf"), dtype=dtype).scatter_reduce(0, i, s.detach(), reduce="amax", include_self=True)
    ex = torch.exp(s - smax[i])
    den = torch.zeros(n, dtype=dtype).index_add_(0, i, ex)
    p = ex / (den[i] + 1e-16)
    out = torch.zeros(n, D, dtype=dtype).index_add_(0, i, xj * p.view(-1, 1))
    (out * g_out.to(dtype)).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    gterm = (p.detach() * (g_out.to(dtype)[i] * xj.detach()).sum(1)).abs()
    return {"mx": mx, "out": out.detach(), "score": p.detach(), "gterm": gterm,
            "g_x": zero(xr), "g_a": zero(ar), "g_b": zero(br)}


def first_max_arg(n, i, j, x):
    """arg [n, D] of csr_gather_max restated: the CSR position of the FIRST maximum of every (node, column) in CSR order, -1 for an empty
    segment.  Plain loop over the segments; the first position is taken with an explicit minimum, not with argmax's unspecified tie rule."""
    order = csr_order(i)
    src = j[order]
    deg = torch.bincount(i, minlength=n)
    ptr = torch.zeros(n + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(deg, 0)
    arg = torch.full((n, x.shape[1]), -1, dtype=torch.int64)
    for w in range(n):
        e0, e1 = int(ptr[w]), int(ptr[w + 1])
        if e1 > e0:
            xs = x[src[e0:e1]]
            pos = torch.arange(e0, e1).view(-1, 1).expand_as(xs)
            arg[w] = torch.where(xs == xs.max(0).values, pos, torch.full_like(pos, e1)).min(0).values
    return arg, src


def max_backward_from_arg(arg, src, g, rows):
    """g_x of csr_gather_max implied by ``arg``: every (node, column) with an edge routes its gradient to row src[arg] (float64 sums)."""
    n, D = arg.shape
    live = arg >= 0
    cols = torch.arange(D).view(1, -1).expand(n, D)
    gx = torch.zeros(rows, D, dtype=torch.float64)
    gx.index_put_((src[arg[live]], cols[live]), g.double()[live], accumulate=True)
    return gx


def rel_err(got, want):
    """The largest error over the largest reference entry (tests/test_kernels_gpu.py's _relerr with the roles fixed)."""
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.numel() == 0:
        return 0.0
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


# ------------------------------------------------------------------------------------------------ top-k
TOPK_NS = (1, 255, 256, 257, 8192, 8193, 17445, 24575)
TOPK_ARRANGEMENTS = ("grouped", "typed", "shuffled")
TOPK_BS = (1, 4, 7)
TOPK_RATIOS = (1.0, 0.8, 0.33, 1e-4)
TOPK_CASES = [(n, B, arr) for n in TOPK_NS for B in TOPK_BS for arr in TOPK_ARRANGEMENTS]
TOPK_SPECIAL_N = 17445


def topk_case(n, B, arrangement):
    """(score [n], batch [n]): graph ids grouped / grouped inside each of three node types / arbitrary; with B = 7 graph 2 is empty; a quarter
    of the scores (drawn with replacement) share one value."""
    gen = torch.Generator().manual_seed(31 * n + B)
    if arrangement == "grouped":
        batch = torch.sort(torch.randint(0, B, (n,), generator=gen)).values
    elif arrangement == "typed":
        parts = [torch.sort(torch.randint(0, B, (n // 3 + (1 if t < n % 3 else 0),), generator=gen)).values for t in range(3)]
        batch = torch.cat(parts)
    else:
        batch = torch.randint(0, B, (n,), generator=gen)
    if B == 7:
        batch[batch == 2] = 3
    score = torch.rand(n, generator=gen)
    score[torch.randint(0, n, (n // 4,), generator=gen)] = 0.5
    return score, batch


TOPK_SPECIAL_VALUES = (float("nan"), float("inf"), float("-inf"), 0.0, -0.0)


def topk_special_case():
    """n = 17445 in 4 grouped graphs with NaN, +-inf and +-0 sprinkled by a permutation (600 nodes each) across all three chunks."""
    n = TOPK_SPECIAL_N
    gen = torch.Generator().manual_seed(4242)
    batch = torch.sort(torch.randint(0, 4, (n,), generator=gen)).values
    score = torch.randn(n, generator=gen)
    idx = torch.randperm(n, generator=gen)
    for k, v in enumerate(TOPK_SPECIAL_VALUES):
        score[idx[600 * k:600 * (k + 1)]] = v
    return score, batch


def graphs_straddling(batch, step):
    """Graph ids with nodes on both sides of an index that is a positive multiple of ``step``."""
    n = batch.numel()
    hit = set()
    for cut in range(step, n, step):
        hit |= set(batch[:cut].unique().tolist()) & set(batch[cut:].unique().tolist())
    return hit


# ------------------------------------------------------------------------------------------------ S^T A S
STAR_MS = (384, 385, 1536, 1537)


def _looped(ei, N):
    from wsi_hgnn_amd.pooling import ASAP as PA
    return PA.add_remaining_self_loops(ei, None, 1.0, N)[0]


def _edge_values(E, seed, weighted):
    gen = torch.Generator().manual_seed(seed)
    score = torch.rand(E, generator=gen)
    w = torch.pow(10.0, torch.rand(E, generator=gen) * 6 - 3) if weighted else None          # log-uniform in [1e-3, 1e3], fp32 values
    return score, w


def star(m, weighted=False):
    """(N, edge_index with its self loops, score [E], weights [E] or None, perm): nodes 1..m each hold the edge (centre k -> neighbour 0) and a
    self loop, node 0 only its self loop, every node is pooled.  Every row of S^T A S then holds exactly m distinct off-diagonal columns."""
    N = m + 1
    ei = _looped(torch.stack([torch.arange(1, N), torch.zeros(m, dtype=torch.int64)]), N)
    score, w = _edge_values(ei.shape[1], 5 + m, weighted)
    return N, ei, score, w, torch.arange(N)


def random_component(N, E, B, seed):
    """(edge_index, batch) of tests/test_kernels_gpu.py's _asap_case kind: E random edges that stay inside their graph, a tenth of them twice."""
    gen = torch.Generator().manual_seed(seed)
    per = N // B
    src = torch.randint(0, N, (E,), generator=gen)
    dst = ((src // per) * per + torch.randint(0, per, (E,), generator=gen)).clamp(max=N - 1)
    ei = torch.stack([src, dst])
    return torch.cat([ei, ei[:, : E // 10]], dim=1), (torch.arange(N) // per).clamp(max=B - 1)


COMBINED_RANDOM = (600, 3600, 2)


def combined(weighted=False):
    """Disjoint stars with m = 384 and m = 385 plus one random component; perm holds every star node and a fitness-ordered half of the random
    component.  Returns (N, edge_index with self loops, score, weights or None, perm, (rows of star 384, rows of star 385))."""
    from wsi_hgnn_amd.pooling import ASAP as PA
    n1, n2 = 385, 386
    Nr, Er, Br = COMBINED_RANDOM
    s1 = torch.stack([torch.arange(1, n1), torch.zeros(n1 - 1, dtype=torch.int64)])
    s2 = torch.stack([torch.arange(1, n2), torch.zeros(n2 - 1, dtype=torch.int64)]) + n1
    er, br = random_component(Nr, Er, Br, 3)
    N = n1 + n2 + Nr
    ei = _looped(torch.cat([s1, s2, er + n1 + n2], dim=1), N)
    score, w = _edge_values(ei.shape[1], 19, weighted)
    fitness = torch.rand(Nr, generator=torch.Generator().manual_seed(23))
    perm = torch.cat([torch.arange(n1 + n2), n1 + n2 + PA.topk(fitness, 0.5, br)])
    return N, ei, score, w, perm, (range(0, n1), range(n1, n1 + n2))


def stas_reference(N, ei, score, w, perm):
    """graph_connectivity (three sparse products, pooling/ASAP.py:84-117) in float64 on the CPU: (index_E, value_E, distinct off-diagonal columns
    per row)."""
    from wsi_hgnn_amd.pooling import ASAP as PA
    batch = torch.zeros(perm.numel(), dtype=torch.int64)
    idx, val = PA.graph_connectivity(torch.device("cpu"), perm, ei, None if w is None else w.double(), score.double().view(-1, 1), 1.0, batch, N)
    kN = perm.numel()
    rows = torch.bincount(idx[0, : idx.shape[1] - kN], minlength=kN)
    return idx, val, rows
