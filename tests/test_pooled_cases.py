"""What tests/pooled_cases.py claims, held without a GPU: the float64 restatement of the pooled attention entry points equals autograd of the
plain attention; the graphs have the properties the GPU tests rely on; and float32 rounding alone stays under a quarter of every block-wise
bound tests/test_pooled_kernels_gpu.py applies (so a block over its bound is a wrong kernel, not noise)."""
import pytest
import torch

import pooled_cases as C

RESTATED = [(128, 1), (128, 16), (256, 2), (512, 8)]
# every (T, B) graph and every (T, B, D, H) input set the GPU module uses
GPU_GRAPHS = [(3, 2)] + [(T, B) for T in (1, 2, 4, 5, 8) for B in (1, 3)] + [(1, 2), (8, 2)]
GPU_CASES = [(3, 2, D, H) for D, H in C.ALL_DH] + [(T, B, D, H) for T in (1, 2, 4, 5, 8) for B in (1, 3) for D, H in ((128, 4), (256, 8), (512, 2))]
W = C.Worst()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    W.report("float32 on the CPU")


def _rel(x, y):
    return ((x - y).abs().max() / y.abs().max().clamp(min=1e-300)).item()


@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("D,H", RESTATED)
def test_the_restatement_equals_autograd(D, H, T):
    ev, ag = C.evaluate(T, 2, D, H), C.autograd(T, 2, D, H)
    # g_v[u]_h = sum_b ctab[u, b, h] g_t[seg_b(u)]_h;  r_out = omg g_row[seg] + sum ctab y;  ga from gtab;  then everything behind them
    for name, a, b in [("g_v from ctab", ev["g_v_from_ctab"], ag["g_v"]), ("r_out", ev["r_out"], ag["r_out"]), ("ga from gtab", ev["ga"], ag["ga"]),
                       ("g_q", ev["g_q"], ag["g_q"]), ("g_k", ev["g_k"], ag["g_k"]), ("g_e", ev["g_e"], ag["g_e"])]:
        assert _rel(a, b) < 1e-10, (name, _rel(a, b))
    # the probabilities are the forward's: segment sums of t from ctab and v alone
    c, x = C.graph_case(T, 2), C.inputs(T, 2, D, H)
    S, dk = T * 2, D // H
    want = torch.zeros(S, D, dtype=torch.float64).index_add_(0, c.row_seg, ag["t"])
    got = torch.zeros(S, H, dk, dtype=torch.float64)
    for b in range(T):
        got.index_add_(0, b * 2 + c.graph_of, ev["ctab"][:, b, :].unsqueeze(-1) * x["v64"].view(c.n, H, dk))
    assert _rel(got.view(S, D), want) < 1e-10
    assert float((ev["a"].sum(1) > 0).all()) and _rel(torch.zeros(c.seg_len.numel(), H, dtype=torch.float64).index_add_(0, c.seg, ev["a"])[c.seg_len > 0],
                                                       torch.ones(int((c.seg_len > 0).sum()), H, dtype=torch.float64)) < 1e-12


@pytest.mark.parametrize("T,B", GPU_GRAPHS)
def test_the_graphs_have_the_properties_the_gpu_tests_rely_on(T, B):
    c = C.graph_case(T, B)
    facts = c.facts()
    assert set(facts) == set(C.FACTS)
    assert all(v is not False for v in facts.values()), facts
    # what cannot exist is named, not silently dropped: one type has one source type; one slide, one or two types get no one-row and no empty segment (pooled_cases.structural)
    absent = {k for k, v in facts.items() if v is None}
    want_absent = set()
    one_row, empty = C.structural(T, B)
    assert (one_row, empty) == (T >= 3 and B >= 2,) * 2
    want_absent |= (set() if one_row else {"one_row_segment"}) | (set() if empty else {"empty_segment"})
    if T < 2:
        want_absent |= {"two_source_types_per_dst_type", "segments_of_a_dst_differ_in_source_type"}
    assert absent == want_absent, (absent, want_absent)
    sizes = [sum(x) for x in C.type_counts(T, B)]
    assert sizes == list(C.SLIDE_NODES[:B]) and c.n == sum(sizes) and c.E > 0
    # both plans describe the same CSR / CSC; only the order and the hub prefix differ
    for name in ("src", "rowptr", "node_seg", "colptr", "csc_eid", "csc_dst", "inv_rd"):
        assert torch.equal(getattr(c.plan, name), getattr(c.hub_plan, name)), name
    assert c.hub_plan.heavy_degree == C.HUB_DEGREE and c.plan.num_src_rows == c.n


def test_the_sweeps_cover_every_instantiation_and_every_table_width():
    assert len(C.ALL_DH) == 15 and len(set(C.ALL_DH)) == 15
    js = sorted({T * H for T, H in C.GTAB_TH})
    assert js == [1, 5, 12, 14, 16, 24, 28, 32]
    jp = lambda J: 3 if J <= 12 else (6 if J <= 24 else 8)
    assert {jp(J) for J in js} == {3, 6, 8}
    assert any(J % jp(J) != 0 for J in js) and any(4 * jp(J) - J >= jp(J) for J in js)         # a partly filled j-group; a whole group past J (the clamp)
    assert not C.gtab_fits(8, 4, 512) and C.gtab_fits(8, 4, 256) and not C.gtab_fits(3, 16, 128) and C.gtab_fits(3, 8, 512)
    # the T = 3 sweep reaches the table route at H <= 8 and the refusal at H = 16; JP = 8 is reached by the node-type sweep (T = 8, H = 4: J = 32)
    assert [H for D, H in C.ALL_DH if D == 512 and C.gtab_fits(3, H, D)] == [1, 2, 4, 8]


@pytest.mark.parametrize("T,B,D,H", GPU_CASES)
def test_float32_rounding_stays_under_a_quarter_of_every_bound(T, B, D, H):
    c = C.graph_case(T, B)
    ref, f32 = C.reference(T, B, D, H), C.evaluate(T, B, D, H, torch.float32)
    got = {k: f32[k] for k in ("a", "ctab", "gtab", "r_out", "g_q", "g_k", "g_e", "g_v_from_ctab")}
    W.hold(C.ratios(got, ref, c, c.hub, H), f"T={T} B={B} D={D} H={H}", limit=0.25)
