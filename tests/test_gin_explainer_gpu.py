"""The explainers on a GIN, on the GPU.  ``GNNExplainer`` over a 60-node graph and a GIN of each neighbour reducer, 3 epochs: ``history``, the
node mask and the trained edge mask against the same loop (tests/test_gnn_explainer_gpu.py's, torch's Adam in float64) run through
``models.GIN`` on the CPU in float64, i.e. through ``ops.gin_aggregate_reference``; the initial masks come from the CPU generator, so they
are equal.  ``GemExplainer`` and ``localization.explain_and_score(..., "GNNExplainer")`` run on a GIN."""
import copy

import numpy as np
import pytest
import torch

from test_gnn_explainer_gpu import LOOP_LR, _close, initial_masks, ref_explainer_loop, trusted_elements

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, IN_DIM, EPOCHS, SEED = 60, 24, 3, 3


def _graph(seed=9):
    """60 nodes: random edges with duplicates, a self loop on every other node, four nodes without in-edges, shuffled edge order."""
    from wsi_hgnn_amd.graph import HeteroGraph
    gen = torch.Generator().manual_seed(seed)
    s = torch.randint(0, N, (300,), generator=gen)
    d = torch.randint(4, N, (300,), generator=gen)
    loop = torch.arange(4, N, 2)
    u, v = torch.cat([s, s[:30], loop]), torch.cat([d, d[:30], loop])
    o = torch.randperm(u.numel(), generator=gen)
    return HeteroGraph.homogeneous(N, u[o], v[o], feat=torch.randn(N, IN_DIM, generator=gen))


def _gin(neigh, layers=3, seed=13):
    from wsi_hgnn_amd.models import GIN
    torch.manual_seed(seed)
    m = GIN(IN_DIM, 16, 2, layers, 2, 0.0, "mean", neigh, True)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith("running_mean"):
                v.copy_(0.3 * torch.randn(v.shape, generator=gen))
            elif k.endswith("running_var"):
                v.copy_(0.5 + torch.rand(v.shape, generator=gen))
            elif k.endswith(".eps"):
                v.fill_(0.3)
    return m.eval()


@pytest.mark.parametrize("neigh", ["sum", "mean", "max"])
def test_explainer_loop_matches_float64_adam(neigh):
    from wsi_hgnn_amd import graph as G
    from wsi_hgnn_amd.explainers import GNNExplainer, ExplainerTags
    g_cpu = _graph()
    g = g_cpu.to(DEV)
    E = g.num_edges()
    m64 = _gin(neigh).double()
    m = copy.deepcopy(m64).float().to(DEV)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ex = GNNExplainer(g, m, num_hops=2, epochs=EPOCHS)
    torch.manual_seed(SEED)
    subgraph, node_mask = ex.explain_node(node_idx=None)
    torch.cuda.synchronize()
    node0, edge0 = initial_masks(N, E, SEED)
    with torch.no_grad():
        pred = m(g).argmax(dim=-1).cpu()
    perm = g._csr_perm().cpu()
    assert torch.equal(perm, g_cpu._csr_perm()) and not torch.equal(perm, torch.arange(E))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(E)

    def forward(h, scale_csr):                                        # the CPU model in float64 under the same message scale (edge order)
        with G.message_scale(g_cpu, scale_csr[inv]):
            return m64(g_cpu, h)

    losses, grads, rnode, redge = ref_explainer_loop(forward, g_cpu.ndata["feat"], node0, edge0, perm, pred, EPOCHS, LOOP_LR)
    assert len(ex.history) == EPOCHS
    for i, (a, b) in enumerate(zip(ex.history, losses)):
        print(f"{neigh} epoch {i}: loss {a:.7f}, float64 {b:.7f}")
        assert abs(a - b) <= 1e-4 * abs(b), f"epoch {i}: loss {a} != {b}"
    keep_n, keep_e = trusted_elements(grads)
    excluded = int((~keep_n).sum()) + int((~keep_e).sum())
    print(f"{neigh}: excluded {excluded} of {N + E} mask elements")
    assert excluded <= 0.02 * (N + E)
    assert isinstance(node_mask, np.ndarray) and node_mask.shape == (N,)
    edge_mask = subgraph.edata[ExplainerTags.EDGE_MASK].detach().cpu()
    _close(torch.from_numpy(node_mask)[keep_n], rnode.sigmoid()[keep_n], "sigmoid(node_mask)")
    _close(edge_mask[keep_e], redge[keep_e], "edge_mask")
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert all(p.grad is None and p.requires_grad for p in m.parameters())


def test_gem_explainer_and_explain_and_score_run_on_a_gin():
    from wsi_hgnn_amd import localization as L
    from wsi_hgnn_amd.explainers import GemExplainer
    g = _graph().to(DEV)
    m = _gin("mean", layers=2).to(DEV)
    label = torch.tensor([1], device=DEV)
    mask = np.asarray(GemExplainer(g, m, label).explain_node(), dtype=np.float32)
    assert mask.shape == (N,) and np.isfinite(mask).all() and float(mask.std()) > 0
    tiles = torch.stack([torch.arange(N) % 10, torch.arange(N) // 10], 1)
    _, centres = L.patch_centres(tiles, 256, 1)
    ann = L.Annotation.from_rings([[(0.0, 0.0), (2560.0, 0.0), (2560.0, 1536.0), (0.0, 1536.0)]])
    torch.manual_seed(SEED)
    score, masks = L.explain_and_score(m, [(g, label, centres.to(DEV), ann)], explainer="GNNExplainer")
    assert len(masks) == 1 and tuple(masks[0].shape) == (N,) and bool(torch.isfinite(masks[0]).all())
    assert score.auc.shape[0] == 1 and np.isfinite(np.asarray(score.auc)).all()
