"""Batches built from patch grids on the device go through one training step of their models, at the small sizes of tests/test_gtn_gpu.py and
tests/test_h2mil_gpu.py, and give what the same step gives on the batch built by ``from_dense`` / ``from_slides`` from the restated tensors
(tests/grid_cases.py)."""
import numpy as np
import pytest
import torch

import grid_cases as G
import gtn_cases
from mil_cases import Ratios

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-4
R = Ratios(TOL)
SMALL = dict(n_class=3, in_feats=48, embed_dim=32, node_cluster_num=10, depth=2, num_heads=4)        # tests/test_gtn_gpu.py's


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    R.report()


def test_gtn_step_on_a_from_grid_batch_equals_the_step_on_the_from_dense_batch():
    """The two batches hold the same entries in the same order, but ``from_grid`` leaves ``weight=None`` where ``from_dense`` carries a tensor
    of ones.  That IS a different kernel path: ``wsi_spmm_sum``, ``wsi_mincut_fwd`` and ``wsi_mincut_bwd`` take the branch without an edge_w
    pointer.  So this comparison uses the project's norm - loss and every parameter gradient within 1e-4 x the largest entry of the
    ``from_dense`` result - and prints the ratios; the batches themselves (row, col, sizes) are compared exactly."""
    from wsi_hgnn_amd import gtn, optim
    slides = [G.disc(40, seed=1), G.holed_grid(9, 9, 0.4, seed=G.HOLED_SEED), G.disc(129, seed=2, x0=G.LIMIT - 30)]       # 40, 49 and 129 nodes
    g = torch.Generator().manual_seed(9)
    feats = [torch.randn(len(s), SMALL["in_feats"], generator=g) for s in slides]
    nmax = max(len(s) for s in slides)
    node_feat, adj, mask = torch.zeros(3, nmax, SMALL["in_feats"]), torch.zeros(3, nmax, nmax, dtype=torch.float64), torch.zeros(3, nmax)
    for b, s in enumerate(slides):
        node_feat[b, :len(s)], mask[b, :len(s)] = feats[b], 1
        adj[b, :len(s), :len(s)] = torch.from_numpy(G.dense_adjacency(s))
    dense = gtn.from_dense(node_feat, adj, mask).to(DEV)
    grid = gtn.from_grid([f.to(DEV) for f in feats], [torch.tensor(s, device=DEV) for s in slides])
    assert grid.row.is_cuda and grid.weight is None and dense.weight is not None
    assert grid.sizes == dense.sizes and torch.equal(grid.row, dense.row) and torch.equal(grid.col, dense.col) and torch.equal(grid.x, dense.x)
    base = gtn_cases.classifier_state(SMALL["n_class"], SMALL["in_feats"], SMALL["embed_dim"], SMALL["node_cluster_num"], SMALL["depth"],
                                      SMALL["num_heads"], seed=77)
    labels = torch.tensor([0, 2, 1], device=DEV)
    res = {}
    for name, batch in (("dense", dense), ("grid", grid)):
        m = gtn.Classifier(SMALL["n_class"], SMALL["in_feats"], SMALL["embed_dim"], SMALL["node_cluster_num"], SMALL["depth"], SMALL["num_heads"])
        m.load_state_dict(base, strict=True)
        m = m.to(DEV)
        loss = gtn.train_one_step(m, batch, labels, optim.Adam(m.parameters(), lr=1e-3))
        res[name] = (loss, {k: p.grad.detach().clone() for k, p in m.named_parameters()})
    assert np.isfinite(float(res["grid"][0]))
    R.check(res["grid"][0], res["dense"][0].double(), "loss", "gtn from_grid vs from_dense")
    for k, g_dense in res["dense"][1].items():
        R.check(res["grid"][1][k], g_dense.double(), "g_param", f"gtn from_grid vs from_dense {k}")


def test_h2mil_step_on_a_from_grid_batch_equals_the_step_on_the_from_slides_batch():
    """The two batches are identical tensors (checked field by field first), the kernels are deterministic, so loss and gradients are BIT-equal."""
    from wsi_hgnn_amd import h2mil
    slides = [G.rich_tree(6, 5, feat=12, seed=0), G.small_tree(feat=12, seed=1)]                        # 110 and 16 nodes
    slides[1]["x"] = slides[1]["x"] + 1.5
    want = h2mil.from_slides([G.restated(s) for s in slides]).to(DEV)
    got = h2mil.from_grid([{k: v.to(DEV) for k, v in s.items()} for s in slides])
    assert got.edge_index.is_cuda
    G.same_batches(got, want)
    labels = torch.tensor([0, 1], device=DEV)
    res = []
    for batch in (want, got):
        torch.manual_seed(3)
        m = h2mil.H2MIL(12, 0, 8, 2, drop_out_ratio=0.0).to(DEV)
        loss = h2mil.train_one_step(m, batch, labels, torch.optim.Adam(m.parameters(), lr=1e-2))
        res.append((loss, {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}))
    assert np.isfinite(float(res[0][0])) and torch.equal(res[0][0], res[1][0])
    assert res[0][1] and res[0][1].keys() == res[1][1].keys()
    for k, g in res[0][1].items():
        assert torch.equal(g, res[1][1][k]), k
