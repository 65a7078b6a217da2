"""``ops.ra_attention`` (wsi_ra_attn_fwd / _bwd) and ``ops.ihpool_assign`` (wsi_ihpool_assign) on the GPU against float64 on the SAME fp32 inputs.
Tolerance (tests/test_gtn_kernels_gpu.py's norm): error <= 1e-4 x the largest float64 entry of each tensor.

ra_attention: the graph of h2mil_cases.ra_kernel_graph - in-degrees 0, 1, 2, 63, 64, 65 and 200 (a row shorter than, equal to and longer than
a wave's worth of edges for every group width), groups of one edge, destinations with 1, 2 and 3 types present, repeated edges - at
C in {1, 3, 4, 32, 256, 260}; out, g_ft, g_sc and g_bias are each checked.  ihpool_assign: segments of 1, 2, 63, 64, 65 and 300 members under
1, 2, 7 and 65 seeds and an empty segment, inputs under the margin condition: clusters equal the float64 restatement exactly."""
import pytest
import torch

import h2mil_cases as C
from mil_cases import Ratios

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
R = Ratios(TOL)
WIDTHS = (1, 3, 4, 32, 256, 260)


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


@pytest.fixture(scope="module")
def graph():
    from wsi_hgnn_amd import ops
    n, nt, ei = C.ra_kernel_graph()
    ec = ops.edge_csr_by_source_type(ei[0].to(DEV), ei[1].to(DEV), nt.to(DEV), n)
    return n, nt, ei, ec


def _inputs(n, Cw, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(1000 * Cw + seed)
    return (torch.randn(n, Cw, generator=g), torch.randn(n, 4, generator=g) * scale, torch.randn(Cw, generator=g), torch.randn(n, Cw, generator=g))


def _reference(ft, sc, bias, w, ei, nt):
    f, s, b = (t.double().requires_grad_(True) for t in (ft, sc, bias))
    out = C.ra_attention_ref(f, s, b, ei, nt)
    (out * w.double()).sum().backward()
    return out.detach(), f.grad, s.grad, b.grad


def _through_ops(ft, sc, bias, w, ec, nt):
    from wsi_hgnn_amd import ops
    f, s, b = (t.to(DEV).requires_grad_(True) for t in (ft, sc, bias))
    out = ops.ra_attention(f, s, b, ec, nt.to(DEV))
    out.backward(w.to(DEV))
    return out.detach(), f.grad, s.grad, b.grad


NAMES = ("out", "g_ft", "g_sc", "g_bias")


@pytest.mark.parametrize("Cw", WIDTHS)
def test_ra_attention_against_float64(graph, Cw):
    n, nt, ei, ec = graph
    args = _inputs(n, Cw)
    got = _through_ops(*args, ec, nt)
    for name, g, r in zip(NAMES, got, _reference(*args, ei, nt)):
        R.check(g, r, name, f"C={Cw}")
    again = _through_ops(*args, ec, nt)
    for name, a, b in zip(NAMES, got, again):
        assert torch.equal(a, b), f"C={Cw}: {name} differs between identical calls"
    bias = args[2].to(DEV)
    assert torch.equal(got[0][0], bias), "a node without in-edges gives the bias"
    # a softmax of one term has gradient zero: destination 1 has one in-edge, so its er receives exactly nothing
    assert float(got[2][1, 1]) == 0.0


@pytest.mark.parametrize("Cw", (4, 260))
def test_ra_attention_with_nearly_one_hot_rows(graph, Cw):
    n, nt, ei, ec = graph
    args = _inputs(n, Cw, seed=1, scale=30.0)
    for name, g, r in zip(NAMES, _through_ops(*args, ec, nt), _reference(*args, ei, nt)):
        R.check(g, r, name, f"one-hot C={Cw}")


def test_ra_attention_without_bias_and_on_a_strided_projection(graph):
    """bias None; ft as the leading columns of a wider matrix (the layer's own call: ft | pl | pr | 0 | 0 from one GEMM)."""
    from wsi_hgnn_amd import ops
    n, nt, ei, ec = graph
    ft, sc, _, w = _inputs(n, 32, seed=2)
    wide = torch.cat([ft, torch.randn(n, 4)], 1).to(DEV).requires_grad_(True)
    s = sc.to(DEV).requires_grad_(True)
    out = ops.ra_attention(wide[:, :32], s, None, ec, nt.to(DEV))
    out.backward(w.to(DEV))
    f64, s64 = ft.double().requires_grad_(True), sc.double().requires_grad_(True)
    ref = C.ra_attention_ref(f64, s64, None, ei, nt)
    (ref * w.double()).sum().backward()
    R.check(out.detach(), ref.detach(), "out", "strided")
    R.check(wide.grad[:, :32], f64.grad, "g_ft", "strided")
    R.check(s.grad, s64.grad, "g_sc", "strided")
    assert not wide.grad[:, 32:].any()


def test_one_node_type_equals_gat_attention(graph):
    """With every node of one type there is one group per destination and beta = 1: GATConv at one head."""
    from wsi_hgnn_amd import ops
    n, _, ei, _ = graph
    nt = torch.ones(n, dtype=torch.int64)
    ec = ops.edge_csr_by_source_type(ei[0].to(DEV), ei[1].to(DEV), nt.to(DEV), n)
    ec.order_dst = ec.order_src = None
    g = torch.Generator().manual_seed(5)
    Cw = 32
    ft, al, ar, bias = torch.randn(n, Cw, generator=g), torch.randn(1, 1, Cw, generator=g), torch.randn(1, 1, Cw, generator=g), torch.randn(Cw, generator=g)
    ftd = ft.to(DEV)
    sc = torch.stack([ftd @ al.view(Cw).to(DEV), ftd @ ar.view(Cw).to(DEV), torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)], 1)
    ra = ops.ra_attention(ftd, sc, bias.to(DEV), ec, nt.to(DEV), 0.2)
    gat = ops.gat_attention(ftd, al.to(DEV), ar.to(DEV), bias.to(DEV), ec, 0.2)
    ref = C.ra_attention_ref(ft.double(), sc.double().cpu(), bias.double(), ei, nt)
    R.check(ra, ref, "out", "one type")
    R.check(gat, ref, "gat out", "one type")
    R.check(ra, gat.double(), "ra against gat", "one type")


# ------------------------------------------------------------------------------------------------ wsi_ihpool_assign
@pytest.fixture(scope="module")
def assign_case():
    case, _ = C.find_case(C.assign_case, lambda c: float(C.assign_ref(*c)[1].min()))
    return case


def test_ihpool_assign_equals_the_restatement_exactly(assign_case):
    from wsi_hgnn_amd import ops
    sizes = torch.bincount(assign_case[2].long())
    assert sorted(set(sizes.tolist())) == [0, 1, 2, 63, 64, 65, 300]
    want, gaps = C.assign_ref(*assign_case)
    assert float(gaps.min()) >= C.MARGIN
    dev = [t.to(DEV) for t in assign_case]
    got = ops.ihpool_assign(*dev)
    assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), want)
    assert torch.equal(got, ops.ihpool_assign(*dev))
    # every seed sits in its own cluster
    pos = torch.arange(assign_case[4].shape[0]) - assign_case[3].long()[torch.repeat_interleave(torch.arange(len(sizes)), assign_case[3].long().diff())]
    where = {int(nd): i for i, nd in enumerate(assign_case[1].tolist())}
    assert all(int(want[where[int(nd)]]) == int(p) for nd, p in zip(assign_case[4].tolist(), pos.tolist()))


def test_ihpool_assign_ties_and_edges():
    from wsi_hgnn_amd import ops
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device=DEV)
    # segment 0: seeds at nodes 0 and 1, node 2 exactly between them -> the lowest seed; nodes 0 and 1 coincide with seeds 3 and 4 of segment 1,
    # where node 4 is a seed at the very place of seed 3: it still owns its cluster; segment 2 is empty; segment 3 has a member and no seed
    xyf = torch.tensor([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.25, 0.0, 0.0], [0.3, 0.3, 0.1], [0.3, 0.3, 0.1], [0.3, 0.3, 0.1], [0.9, 0.9, 0.9]], device=DEV)
    got = ops.ihpool_assign(xyf, i32(0, 1, 2, 3, 4, 5, 6), i32(0, 0, 0, 1, 1, 1, 3), i32(0, 2, 4, 4, 4), i32(0, 1, 3, 4))
    assert got.tolist() == [0, 1, 0, 0, 1, 0, -1]
    assert ops.ihpool_assign(xyf, i32(), i32(), i32(0), i32()).numel() == 0
