"""tests/asap_cases.py holds the cases of tests/test_asap_kernels_gpu.py; here, without a GPU and with the reference formulations only, each case
is shown to have the property it exists for - so a change to a builder that loses a path fails here instead of passing silently on the GPU."""
import pytest
import torch

import asap_cases as AC


@pytest.fixture(scope="module")
def graph():
    return AC.edge_graph()


def test_edge_graph_has_the_stated_segments(graph):
    n, i, j = graph
    seg, gathered = AC.degrees(n, i, j)
    assert n == AC.EDGE_N and n % AC.AS_WAVES == 3 and int(i.max()) < n and int(j.max()) < n
    assert seg[:7].tolist() == [1, 63, 64, 65, 128, 129, 150] and int(seg[AC.TAIL]) == 70
    assert j[i == AC.LONELY].tolist() == [AC.LONELY]                                        # its self loop
    assert int(gathered[AC.TAIL]) >= 2 and bool((i[j == AC.TAIL] != AC.TAIL).any())         # the tail is gathered by other nodes
    # nine designed nodes without a segment, one of them strictly inside a block of four consecutive nodes with segments on both sides
    assert len(AC.NO_SEGMENT) == 9 and all(int(seg[v]) == 0 for v in AC.NO_SEGMENT)
    assert any(v % AC.AS_WAVES in (1, 2) and int(seg[v - v % 4]) > 0 and int(seg[v - v % 4 + 3]) > 0 for v in AC.NO_SEGMENT)
    assert len(AC.NEVER_GATHERED) == 11 and all(int(gathered[v]) == 0 for v in AC.NEVER_GATHERED)
    assert not set(AC.NO_SEGMENT) & set(AC.NEVER_GATHERED) and int(seg[list(AC.NEVER_GATHERED)].min()) >= 0
    # every remaining node: 0..5 edges drawn, a tenth of all of them listed twice
    named = set(AC.NAMED_ROWS) | set(AC.NO_SEGMENT)
    rest = torch.tensor([v for v in range(n) if v not in named])
    assert int(seg[rest].max()) <= 10 and 2.0 < float(seg[rest].float().mean()) < 3.5
    # the seven long segments make a second trip of the 64-lane loops; 64 / 65 and 128 / 129 sit on the stride from both sides
    assert sorted(int(d) for d in seg if int(d) >= 63) == [63, 64, 65, 70, 128, 129, 150]


def test_edge_graph_has_duplicates_ties_and_a_shuffled_edge_list(graph):
    n, i, j = graph
    key = i * n + j
    uniq, cnt = torch.unique(key, return_counts=True)
    assert int((cnt > 1).sum()) >= AC.TIED_SOURCES + 10                                     # repeated edges in the softmax
    at_tied = j[i == AC.TIED]
    u, c = torch.unique(at_tied, return_counts=True)
    assert u.numel() == AC.TIED_SOURCES and bool((c == 2).all())                            # 75 sources, twice each
    assert not torch.equal(torch.sort(i, stable=True).values, i)                            # EdgeCSR gets an unsorted list
    # the first-maximum rule is decided by ties: at the tied node every column's maximum occurs exactly twice
    x, _, _ = AC.features(n, 65)
    arg, src = AC.first_max_arg(n, i, j, x)
    order = AC.csr_order(i)
    seg0 = int((i < AC.TIED).sum())
    xs = x[src[seg0:seg0 + 150]]
    assert torch.equal(order[seg0:seg0 + 150], torch.nonzero(i == AC.TIED).view(-1))        # CSR order inside a segment == input order
    assert bool(((xs == xs.max(0).values).sum(0) == 2).all())
    first = arg[AC.TIED] - seg0
    assert bool((xs[first, torch.arange(65)] == xs.max(0).values).all())
    for c in range(65):
        assert not bool((xs[:int(first[c]), c] == xs[:, c].max()).any())
    assert bool((arg[list(AC.NO_SEGMENT)] == -1).all()) and int(arg[AC.LONELY, 0]) == 0 and bool((arg[AC.LONELY] == 0).all())


def test_small_graphs():
    g = AC.small_graphs()
    assert g["one_node"][0] == 1 and g["one_node"][1].tolist() == [0] and g["one_node"][2].tolist() == [0]
    n, i, j = g["ring5"]
    assert n == 5 and i.tolist() == [0, 1, 2, 3, 4] and j.tolist() == [1, 2, 3, 4, 0]
    n, i, j = g["no_edges"]
    assert n == 6 and i.numel() == 0 and j.numel() == 0 and i.dtype == torch.int64
    for n, i, j in g.values():                                                              # the reference runs on all of them
        x, _, g_out = AC.features(n, 3)
        a, b = AC.scores("normal", n)
        ref = AC.edge_reference(i, j, x, a, b, g_out)
        assert ref["out"].shape == (n, 3) and ref["score"].numel() == i.numel() and torch.isfinite(ref["g_x"]).all()
    assert not AC.edge_reference(*g["no_edges"][1:], *AC.features(6, 3)[:1], *AC.scores("normal", 6), AC.features(6, 3)[2])["out"].any()


def _segment_stats(graph, regime):
    n, i, j = graph
    x, _, g_out = AC.features(n, 3)
    a, b = AC.scores(regime, n)
    p = AC.edge_reference(i, j, x, a, b, g_out)["score"]
    top = torch.zeros(n, dtype=torch.float64).scatter_reduce(0, i, p, reduce="amax", include_self=True)
    many = torch.zeros(n, dtype=torch.float64).index_add_(0, i, (p > 0.01).double())
    return AC.degrees(n, i, j)[0], top, many, p


def test_peaked_regime_is_peaked(graph):
    seg, top, many, p = _segment_stats(graph, "peaked")
    multi = seg >= 2
    share = float((top[multi] > 0.999).double().mean())
    print(f"peaked: {share:.3f} of the segments with two or more edges have a largest probability above 0.999")
    assert share >= 0.4
    assert bool(((seg >= 64) & (many >= 2)).any())                                          # a long segment that is NOT one-hot
    # the normal regime is not: no long segment is dominated
    seg_n, top_n, _, _ = _segment_stats(graph, "normal")
    assert float(top_n[seg_n >= 63].max()) < 0.9
    # and without the max subtraction the peaked scores overflow fp32's exp
    n, i, j = graph
    a, b = AC.scores("peaked", n)
    assert float((a[i] + b[j]).max()) > 89.0


def test_grid_regimes_are_exact_in_fp32(graph):
    n, i, j = graph
    a, b = AC.scores("grid", n)
    a2, b2 = AC.scores("grid+4096", n)
    assert torch.equal(b, b2) and torch.equal(a2 - 4096.0, a) and a.dtype == torch.float32
    for t in (a, b):
        assert float(t.min()) >= 0 and float(t.max()) < 8 and torch.equal((t * 1024).round() / 1024, t)
    for aa, bb in ((a, b), (a2, b2)):
        s32 = (aa[i] + bb[j]).view(-1)
        assert torch.equal(s32.double(), (aa.double()[i] + bb.double()[j]).view(-1)) and float(s32.min()) > 0      # sums exact and positive
        top = torch.full((n,), float("-inf")).scatter_reduce(0, i, s32, reduce="amax", include_self=True)
        d32 = s32 - top[i]
        assert torch.equal(d32.double(), s32.double() - top.double()[i])                                           # differences exact
    x, _, g_out = AC.features(n, 3)
    r1, r2 = AC.edge_reference(i, j, x, a, b, g_out), AC.edge_reference(i, j, x, a2, b2, g_out)
    for k in ("out", "score", "g_x", "g_a", "g_b"):
        assert torch.equal(r1[k], r2[k]), k                                                 # the float64 reference itself cannot tell them apart


def test_reference_is_the_scatter_formulation_of_the_module():
    """edge_reference against pooling/ASAP.py's own CPU branch pieces (segment_softmax) and a per-node loop."""
    from wsi_hgnn_amd.pooling import ASAP as PA
    n, i, j = AC.edge_graph()
    x, _, g_out = AC.features(n, 5)
    a, b = AC.scores("normal", n)
    ref = AC.edge_reference(i, j, x, a, b, g_out)
    s = torch.nn.functional.leaky_relu(a.double()[i] + b.double()[j], AC.SLOPE)
    p = PA.segment_softmax(s, i, n).view(-1)
    assert AC.rel_err(ref["score"], p) < 1e-14
    for w in (0, 2, 6, AC.TAIL):
        m = i == w
        assert AC.rel_err(ref["out"][w], (x.double()[j[m]] * p[m].view(-1, 1)).sum(0)) < 1e-13
        assert torch.equal(ref["mx"][w], x.double()[j[m]].max(0).values)
    assert not ref["mx"][list(AC.NO_SEGMENT)].any() and not ref["out"][list(AC.NO_SEGMENT)].any()
    assert not ref["g_x"][list(AC.NEVER_GATHERED)].any() and not ref["g_b"][list(AC.NEVER_GATHERED)].any()
    # the float32 yardstick of the 4x rule is the same composition: it agrees with float64 to fp32 rounding
    r32 = AC.edge_reference(i, j, x, a, b, g_out, dtype=torch.float32)
    assert 0 < AC.rel_err(r32["out"], ref["out"]) < 1e-5


@pytest.mark.parametrize("n,B,arrangement", AC.TOPK_CASES)
def test_topk_cases(n, B, arrangement):
    score, batch = AC.topk_case(n, B, arrangement)
    assert score.numel() == n and batch.numel() == n and int(batch.min()) >= 0 and int(batch.max()) < B
    if n >= 255:
        assert int((score == 0.5).sum()) >= n // 5                                          # the tied value
    if B == 7:
        assert not bool((batch == 2).any())
        if n >= 255:
            assert bool((batch == 3).any()) and bool((batch == 1).any())                    # graph 2 is empty BETWEEN non-empty ones
    if n >= 255:
        sorted_ = bool((batch[1:] >= batch[:-1]).all())
        assert sorted_ == (arrangement == "grouped" or B == 1)
    if n > AC.TK_TILE:
        assert AC.graphs_straddling(batch, AC.TK_TILE)
    if n > AC.TK_CHUNK:
        assert AC.graphs_straddling(batch, AC.TK_CHUNK)                                     # partial ranks of one graph come from two chunks
        assert (n + AC.TK_CHUNK - 1) // AC.TK_CHUNK >= 2


def test_topk_sizes_and_the_special_values():
    assert AC.TOPK_NS == (1, 255, 256, 257, 8192, 8193, 17445, 24575) and 24575 == 3 * AC.TK_CHUNK - 1
    assert set(AC.TOPK_BS) == {1, 4, 7} and AC.TOPK_RATIOS == (1.0, 0.8, 0.33, 1e-4)
    score, batch = AC.topk_special_case()
    n = score.numel()
    assert n == AC.TOPK_SPECIAL_N and (n + AC.TK_CHUNK - 1) // AC.TK_CHUNK == 3
    for c0 in range(0, n, AC.TK_CHUNK):
        s = score[c0:c0 + AC.TK_CHUNK]
        zero = s == 0
        assert bool(torch.isnan(s).any()) and bool((s == float("inf")).any()) and bool((s == float("-inf")).any()), c0
        assert bool((zero & torch.signbit(s)).any()) and bool((zero & ~torch.signbit(s)).any()), c0
    assert AC.graphs_straddling(batch, AC.TK_CHUNK)


@pytest.mark.parametrize("m", AC.STAR_MS)
def test_star_rows_hold_exactly_m_columns(m):
    N, ei, score, w, perm = AC.star(m)
    assert N == m + 1 and ei.shape[1] == 2 * m + 1 and torch.equal(perm, torch.arange(N))
    assert ei[:, :m].tolist() == [list(range(1, N)), [0] * m] and torch.equal(ei[0, m:], ei[1, m:])
    idx, val, rows = AC.stas_reference(N, ei, score, w, perm)
    assert bool((rows == m).all())
    small, large = m <= AC.ST_SMALL_ROWS, AC.ST_SMALL_ROWS < m <= AC.ST_LARGE_ROWS
    assert (small, large) == {384: (True, False), 385: (False, True), 1536: (False, True), 1537: (False, False)}[m]


@pytest.mark.parametrize("weighted", [False, True])
def test_combined_graph_owns_rows_in_both_tables(weighted):
    N, ei, score, w, perm, (star_a, star_b) = AC.combined(weighted)
    idx, val, rows = AC.stas_reference(N, ei, score, w, perm)
    assert perm.unique().numel() == perm.numel() and perm.numel() == 385 + 386 + AC.COMBINED_RANDOM[0] // 2
    assert bool((rows[list(star_a)] == 384).all()) and bool((rows[list(star_b)] == 385).all())
    rnd = rows[385 + 386:]
    assert int(rnd.max()) < AC.ST_SMALL_ROWS and int((rnd > 0).sum()) > 250                  # the random component: small-table rows of many sizes
    assert int(((rows > 0) & (rows <= AC.ST_SMALL_ROWS)).sum()) > 0 and int(((rows > AC.ST_SMALL_ROWS) & (rows <= AC.ST_LARGE_ROWS)).sum()) > 0
    if weighted:
        assert float(w.min()) >= 1e-3 * (1 - 1e-6) and float(w.max()) <= 1e3 and float(w.max()) / float(w.min()) > 1e5 and w.dtype == torch.float32
        assert float(val.abs().max()) > 1.0
    else:
        assert w is None
