"""The device path of the graph augmentation (csrc/augment.hip through ops.augment_graph) against the tensor formulation on the CPU, for the same
draw, BIT FOR BIT: counts, edges, ``sim``, ``feat`` and the fields that follow by indexing.  Shapes are the smallest that reach every kernel
path: node types of 0 / 1 / 63 / 64 / 65 nodes (wave boundaries of the ballot scan) and one longer than a 1024-element scan tile, a relation
without edges and one longer than a tile, feature widths 4 (one 16-byte access), 6 (element-per-lane tail path) and 1024 (a wave per row, four
accesses per lane)."""
import importlib.util
import os
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 0x5EED1234
COUNTS = [0, 1, 63, 64, 65, 2500]
RELS = [("5", "a", "5", 3000), ("5", "b", "4", 200), ("4", "c", "5", 300), ("2", "d", "3", 0), ("1", "e", "5", 40), ("0", "f", "5", 0), ("3", "g", "2", 100)]


def _dev():
    return torch.device("cuda:0")


_GRAPHS = {}


def _graph(width):
    """One CPU graph per feature width, built once and never modified (the transforms return new graphs)."""
    if width not in _GRAPHS:
        from wsi_hgnn_amd.graph import HeteroGraph
        gen = torch.Generator().manual_seed(width)
        nn_ = OrderedDict((str(i), c) for i, c in enumerate(COUNTS))
        edges, sim, w = OrderedDict(), {}, {}
        for (s, e, d, m) in RELS:
            edges[(s, e, d)] = (torch.randint(0, max(nn_[s], 1), (m,), generator=gen), torch.randint(0, max(nn_[d], 1), (m,), generator=gen))
            sim[(s, e, d)] = torch.rand(m, generator=gen) - 0.5
        g = HeteroGraph.from_coo(nn_, edges, feat={t: torch.rand(c, width, generator=gen) + 0.5 for t, c in nn_.items()}, sim=sim)
        for t, c in nn_.items():
            g.nodes[t].data["tag"] = torch.arange(c)
        for r in g.canonical_etypes:
            g._eframes[r]["w"] = torch.rand(g.num_edges(r), 3, generator=gen)
        _GRAPHS[width] = g
    return _GRAPHS[width]


def _same(dev_g, cpu_g):
    assert dev_g.ntypes == cpu_g.ntypes and dev_g.canonical_etypes == cpu_g.canonical_etypes
    assert [dev_g.num_nodes(t) for t in dev_g.ntypes] == [cpu_g.num_nodes(t) for t in cpu_g.ntypes]
    for r in cpu_g.canonical_etypes:
        assert dev_g.num_edges(r) == cpu_g.num_edges(r), r
        for a, b in zip(dev_g.edges(r), cpu_g.edges(r)):
            assert a.is_cuda and torch.equal(a.cpu(), b), r
        assert set(dev_g._eframes[r]) == set(cpu_g._eframes[r])
        for k, x in cpu_g._eframes[r].items():
            assert torch.equal(dev_g._eframes[r][k].cpu(), x), (r, k)
    for t in cpu_g.ntypes:
        assert set(dev_g._nframes[t]) == set(cpu_g._nframes[t]), t
        for k, x in cpu_g._nframes[t].items():
            y = dev_g._nframes[t][k]
            assert y.shape == x.shape and torch.equal(y.cpu().view(torch.int32) if x.dtype == torch.float32 else y.cpu(),
                                                      x.view(torch.int32) if x.dtype == torch.float32 else x), (t, k)


def _members(p):
    from wsi_hgnn_amd import transforms as TR
    return {"drop_node": TR.DropNode(p), "drop_edge": TR.DropEdge(p), "node_shuffle": TR.NodeShuffle(),
            "feat_mask": TR.FeatMask(p, node_feat_names=["feat"], edge_feat_names=["w"])}


ALONE = [(k, p) for k in ("drop_node", "drop_edge", "feat_mask") for p in (0.0, 0.5, 1.0)] + [("node_shuffle", 0.5)]   # (NodeShuffle has no probability)


@pytest.mark.parametrize("width", [4, 6, 1024])
@pytest.mark.parametrize("which,p", ALONE)
def test_each_transform_alone_equals_the_cpu_result(which, p, width):
    g = _graph(width)
    t = _members(p)[which]
    _same(t(g.to(_dev()), draw=SEED, index=2), t(g, draw=SEED, index=2))


def test_tile_scan_carries_across_rounds_of_256_tiles():
    """The one-workgroup scan of the tile sums (csrc/segment_table.hip: tile_scan_kernel, shared by the augmentation, the leave-one-out batches,
    the augmented slot fill and the per-relation plan) walks the tiles 256 at a time and carries the total from round to round.  A node type of
    256 * 1024 + 1500 nodes is 258 tiles of 1024: the second round starts from the carry, and the type's kept count is a difference of two
    prefixes that lie in different rounds."""
    from wsi_hgnn_amd import transforms as TR
    from wsi_hgnn_amd.graph import HeteroGraph
    n, m = 256 * 1024 + 1500, 4000
    gen = torch.Generator().manual_seed(258)
    g = HeteroGraph.from_coo(OrderedDict([("0", n)]), OrderedDict([(("0", "a", "0"), (torch.randint(0, n, (m,), generator=gen), torch.randint(0, n, (m,), generator=gen)))]),
                             feat={"0": torch.rand(n, 4, generator=gen) + 0.5}, sim={("0", "a", "0"): torch.rand(m, generator=gen) - 0.5})
    g.nodes["0"].data["tag"] = torch.arange(n)
    t = TR.DropNode(0.5)
    cpu = t(g, draw=SEED, index=2)
    assert 0 < cpu.num_nodes("0") < n and cpu.nodes["0"].data["tag"][-1] >= 256 * 1024     # nodes of the second round survive: their places need the carry
    _same(t(g.to(_dev()), draw=SEED, index=2), cpu)


ORDERS = [("drop_node", "drop_edge", "node_shuffle", "feat_mask"),        # the reference's pipeline: DropEdge by rank, shuffle of the survivors
          ("node_shuffle", "drop_edge", "feat_mask", "drop_node"),        # DropEdge by original position, shuffle in front of the compaction
          ("drop_node", "node_shuffle"), ("drop_edge", "drop_node"), ("feat_mask", "node_shuffle")]


@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("width", [4, 6, 1024])
@pytest.mark.parametrize("order", ORDERS, ids=["-".join(x[:2] for x in o) for o in ORDERS])
def test_fused_pipeline_equals_the_cpu_result(order, width, p):
    from wsi_hgnn_amd import transforms as TR
    g = _graph(width)
    pipe = TR.Compose([_members(p)[k] for k in order])
    _same(pipe(g.to(_dev()), draw=SEED), pipe(g, draw=SEED))


def test_fused_runs_are_bit_identical_and_leave_the_input_alone():
    from wsi_hgnn_amd import transforms as TR
    g = _graph(1024).to(_dev())
    before = {t: g.nodes[t].data["feat"].clone() for t in g.ntypes}
    edges = {r: (g.edges(r)[0].clone(), g.edges(r)[1].clone()) for r in g.canonical_etypes}
    pipe = TR.reference_train_transform()
    a, b = pipe(g, draw=SEED), pipe(g, draw=SEED)
    _same(a, b.to("cpu"))
    c = pipe(g, draw=SEED + 1)
    assert a.num_edges() != c.num_edges() or a.num_nodes() != c.num_nodes()
    assert all(torch.equal(g.nodes[t].data["feat"], before[t]) for t in g.ntypes)
    assert all(torch.equal(g.edges(r)[0], edges[r][0]) and torch.equal(g.edges(r)[1], edges[r][1]) for r in g.canonical_etypes)
    torch.manual_seed(5)
    d = pipe(g)
    torch.manual_seed(5)
    _same(pipe(g), d.to("cpu"))                                  # draw=None: torch.manual_seed replays it


def test_launch_count_does_not_depend_on_the_pipeline_and_a_repeated_kind_starts_a_new_run():
    from wsi_hgnn_amd import _native as N, transforms as TR
    g = _graph(4).to(_dev())
    lib = N.load()
    names = ("wsi_augment_nodes", "wsi_augment_edges", "wsi_augment_keys", "wsi_gather_rows_masked")
    calls = {n: 0 for n in names}
    orig = {n: getattr(lib, n) for n in names}
    try:
        for n in names:
            setattr(lib, n, lambda *a, _n=n: (calls.__setitem__(_n, calls[_n] + 1), orig[_n](*a))[1])
        m = _members(0.5)
        TR.Compose([m["drop_node"], m["node_shuffle"]])(g, draw=SEED)
        two = dict(calls)
        for n in names:
            calls[n] = 0
        TR.Compose([m["feat_mask"], m["drop_node"], m["drop_edge"], m["node_shuffle"]])(g, draw=SEED)
        assert dict(calls) == two == {"wsi_augment_nodes": 1, "wsi_augment_edges": 1, "wsi_augment_keys": 1, "wsi_gather_rows_masked": 6}
        for n in names:
            calls[n] = 0
        twice = TR.Compose([m["drop_node"], m["drop_node"]])
        out = twice(g, draw=SEED)
        assert calls["wsi_augment_nodes"] == 2
    finally:
        for n in names:
            setattr(lib, n, orig[n])
    _same(out, twice(_graph(4), draw=SEED))


def test_gather_refuses_bad_arguments_and_zeroes_rows_outside_the_table():
    from wsi_hgnn_amd import ops
    x = torch.rand(10, 8, device=_dev())
    out = ops.gather_rows_masked(x, torch.tensor([3, 12, 0, -1], device=_dev()))
    assert torch.equal(out[0], x[3]) and torch.equal(out[2], x[0]) and float(out[1].abs().sum()) == 0.0 and float(out[3].abs().sum()) == 0.0
    view = torch.rand(10, 16, device=_dev())[:, 1:7]              # rows that are not 16-byte aligned: the element-per-lane path
    assert torch.equal(ops.gather_rows_masked(view, torch.tensor([9, 2], device=_dev())), view[[9, 2]])
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gather_rows_masked(torch.rand(4, 4), None)


def _headline():
    spec = importlib.util.spec_from_file_location("_headline_path", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_headline_path_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_heatnet4_on_the_augmented_graph_matches_the_oracle():
    """Logits and every gradient on the GPU-augmented graph against the oracle on the CPU-augmented one, with the comparison (and its 1e-4
    tolerance) of tests/test_headline_path_gpu.py."""
    from wsi_hgnn_amd import models, synthetic, transforms as TR
    H = _headline()
    args = (64, 128, 2, 2, 4, H.ND3, 0.0, "mean")
    torch.manual_seed(611)
    m = models.HEATNet4(*args).to(_dev())
    g = synthetic.hetero_graph(600, 64, seed=613, dst_mode="hub")
    pipe = TR.reference_train_transform()
    cpu_g, dev_g = pipe(g, draw=SEED), pipe(g.to(_dev()), draw=SEED)
    _same(dev_g, cpu_g)
    y = torch.tensor([1])
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = {"f32": H._oracle_eval("HEATNet4", args, sd, cpu_g, y, torch.float32), "f64": H._oracle_eval("HEATNet4", args, sd, cpu_g, y, torch.float64)}
    out = m(dev_g)
    loss = torch.nn.functional.cross_entropy(out, y.to(_dev()))
    loss.backward()
    H._compare(m, out, loss, ref)


@pytest.mark.parametrize("resident", [True, False])
def test_loader_with_the_reference_transform_feeds_training_steps(resident):
    from wsi_hgnn_amd import data, models, synthetic, trainer, transforms as TR
    gs = [synthetic.hetero_graph(300 + 20 * i, 64, seed=40 + i) for i in range(4)]
    labels = [0, 1, 1, 0]
    mk = lambda dev, res: data.GraphBatchLoader(gs, labels, 2, dev, shuffle=True, seed=9, resident=res, transform=TR.reference_train_transform())
    torch.manual_seed(611)
    gnn = models.HEATNet4(64, 128, 2, 2, 4, {"0": 0, "1": 1, "2": 2}, 0.2, "mean").to(_dev())
    opt = torch.optim.Adam(gnn.parameters(), lr=1e-4)
    steps = 0
    for (G, y), (Gc, yc) in zip(mk(_dev(), resident), mk("cpu", True)):
        _same(G, Gc)
        assert torch.equal(y.cpu(), yc) and G.batch_size == 2
        loss, *_ = trainer.train_one_step(gnn, opt, torch.nn.CrossEntropyLoss(), G, y, _dev(), sync=True)
        assert loss == loss and abs(loss) < 1e3
        steps += 1
    assert steps == 2
