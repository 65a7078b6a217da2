"""GIN without a GPU: the parser branch against the calls the reference's parser.py:92-102 makes on its two GIN configs, the module surface
(state_dict keys, shapes, parameter creation order, dead parameters) against the reference's own module, the tensor formulation of the
aggregation against plain loops in float64 (values, ``arg`` and every gradient), the float64 restatement of the model against the logits of
the reference's ``GIN.forward`` (tests/golden/gin/, produced by tests/golden/make_reference_gin_fixture.py), the kernels' dispatch rule
and the argument checks of the C-ABI entry points (they return before any HIP call)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import gin_cases as C
import row_group_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gin")
FIX = json.load(open(os.path.join(GOLD, "reference_gin.json")))


# ---------------------------------------------------------------------------------------------------- parser
@pytest.mark.parametrize("rec", FIX["parse_gnn_model"], ids=lambda r: r["config"].split("/")[-1])
def test_parser_makes_the_reference_gin_call(rec, monkeypatch):
    from wsi_hgnn_amd import parser as P
    monkeypatch.setattr(P, "GIN", lambda *a, **k: {"class": "GIN", "args": list(a), "kwargs": k})
    assert P.parse_gnn_model(dict(rec["GNN"])) == rec["constructs"]


@pytest.mark.parametrize("rec", FIX["parse_gnn_model"], ids=lambda r: r["config"].split("/")[-1])
def test_from_config_builds_a_gin(rec):
    from wsi_hgnn_amd import models
    m = models.from_config(dict(rec["GNN"]))
    assert type(m) is models.GIN and m.num_layers == m.n_layers == 2 and m.learn_eps is True
    assert m.drop.p == rec["GNN"]["feat_drop"] and m.graph_pooling_type == rec["GNN"]["graph_pooling_type"]
    assert m.layers[0]._aggregator_type == "mean" and isinstance(m.layers[0].eps, torch.nn.Parameter)
    assert tuple(m.layers[0].apply_func.mlp.linears[0].weight.shape) == (512, 1024)


@pytest.mark.parametrize("key", ["in_dim", "num_mlp_layers", "neighbor_pooling_type", "graph_pooling_type"])
def test_parser_missing_key_is_the_reference_keyerror(key):
    from wsi_hgnn_amd import parser as P
    cfg = dict(FIX["parse_gnn_model"][0]["GNN"])
    del cfg[key]
    with pytest.raises(KeyError) as ei:
        P.parse_gnn_model(cfg)
    assert str(ei.value) == str(KeyError(key)) and isinstance(ei.value, P.MissingGINKey)


# ---------------------------------------------------------------------------------------------------- module surface
@pytest.mark.parametrize("rec", FIX["state_dicts"], ids=lambda r: "mlp{num_mlp_layers}-{graph_pooling_type}-eps{learn_eps}".format(**r["kwargs"]))
def test_state_dict_and_creation_order_match_the_reference(rec):
    from wsi_hgnn_amd.models import GIN
    m = GIN(**rec["kwargs"])
    assert [n for n, _ in m.named_parameters()] == rec["parameters"]
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == rec["state"]
    want = {k: torch.zeros(s, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, s in rec["state"]}
    m.load_state_dict(want, strict=True)


def test_aggregator_and_depth_errors():
    from wsi_hgnn_amd.models.GIN import GIN, GINConv, MLP
    with pytest.raises(KeyError):
        GINConv(None, "median")
    with pytest.raises(ValueError):
        MLP(0, 4, 4, 4)
    with pytest.raises(NotImplementedError):
        GIN(4, 4, 2, 2, 1, 0.0, "median")


def _batch(npz, dtype=torch.float64):
    import wsi_hgnn_amd as W
    src, dst, bnn = (torch.from_numpy(npz[k]).long() for k in ("src", "dst", "batch_num_nodes"))
    x = torch.from_numpy(npz["x"]).to(dtype)
    graphs, off = [], 0
    for n in bnn.tolist():
        keep = (dst >= off) & (dst < off + n)
        g = W.graph.HeteroGraph.homogeneous(n, src[keep] - off, dst[keep] - off)
        g.ndata["feat"] = x[off:off + n]
        graphs.append(g)
        off += n
    return W.batch(graphs), x


@pytest.mark.parametrize("pool", ["sum", "att"])
@pytest.mark.parametrize("layers", [2, 3])
def test_dead_parameters_are_exactly_those_without_a_gradient(pool, layers):
    """With the tensor formulation (CPU, float64): every parameter but the dead ones receives a gradient."""
    from wsi_hgnn_amd.models import GIN
    torch.manual_seed(3)
    m = GIN(12, 8, 3, layers, 2, 0.0, pool, "mean", True).double()
    g, _ = _batch(np.load(os.path.join(GOLD, "reference_gin.npz")))
    m(g).square().sum().backward()
    none = sorted(n for n, p in m.named_parameters() if p.grad is None)
    assert none == sorted(m.dead_parameter_names())
    want = [f"linears_prediction.{layers - 1}.", f"linears_prediction.{layers}."] + ([f"pools.{layers - 1}.gate_nn."] if pool == "att" else [])
    assert none == sorted(p + s for p in want for s in ("weight", "bias"))


# ---------------------------------------------------------------------------------------------------- the aggregation
def _small_case(ties):
    """9 nodes: node 0 without in-edges, node 1 a self loop only, duplicates, a node fed by 5; ``ties``: integer features with many zeros."""
    gen = torch.Generator().manual_seed(17)
    src = [1, 2, 2, 3, 4, 0, 5, 6, 7, 8, 1, 3, 3, 8, 0, 2]
    dst = [1, 3, 3, 3, 3, 3, 4, 4, 5, 5, 6, 7, 7, 8, 2, 2]
    o = torch.randperm(len(src), generator=gen)
    csr = C.csr_of(9, torch.tensor(src)[o], torch.tensor(dst)[o])
    if ties:
        x = torch.randint(0, 3, (9, 4), generator=gen).double() * (torch.rand(9, 4, generator=gen) < 0.6)
        scale = 2.0 ** torch.randint(-1, 2, (len(src),), generator=gen).double()
    else:
        x = torch.randn(9, 4, generator=gen, dtype=torch.float64)
        scale = torch.rand(len(src), generator=gen, dtype=torch.float64) + 0.25
    return csr, x, scale, torch.randn(9, 4, generator=gen, dtype=torch.float64), torch.randn(4, generator=gen, dtype=torch.float64)


@pytest.mark.parametrize("ties", [False, True], ids=["random", "exact-ties"])
@pytest.mark.parametrize("eps", [0.0, 0.3, -1.0])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("mode", C.MODES)
def test_reference_equals_the_loops(mode, scaled, eps, ties):
    from wsi_hgnn_amd import ops
    csr, x, scale, g, bias = _small_case(ties)
    scale = scale if scaled else None
    want, arg = C.loop_forward(x, eps, csr, mode, bias, scale)
    gx, ge, gb, gs = C.loop_backward(g, x, eps, csr, mode, arg, scale)
    xv, ev, bv = x.clone().requires_grad_(), torch.tensor([eps], dtype=torch.float64, requires_grad=True), bias.clone().requires_grad_()
    sv = scale.clone().requires_grad_() if scaled else None
    out, got_arg = ops.gin_aggregate_reference(xv, ev, C.Plan(csr), mode, bv, sv, return_arg=True)
    assert torch.allclose(out, want, rtol=0, atol=1e-12)
    if mode == "max":
        assert torch.equal(got_arg.long(), arg)
        if ties:
            assert int((torch.bincount(C.dst_of(csr)) > 1).sum()) > 0
    (out * g).sum().backward()
    assert torch.allclose(xv.grad, gx, rtol=0, atol=1e-12)
    assert abs(float(ev.grad) - ge) < 1e-12
    assert torch.allclose(bv.grad, gb, rtol=0, atol=1e-12)
    if scaled:
        assert torch.allclose(sv.grad, gs, rtol=0, atol=1e-12)
    # the closed form the GPU tests replay against says the same
    r = C.closed_form(x, eps, csr, mode, bias, scale, g)
    assert torch.allclose(r["out"], want, rtol=0, atol=1e-12) and torch.allclose(r["g_x"], gx, rtol=0, atol=1e-12)
    assert torch.allclose(r["g_scale"], gs, rtol=0, atol=1e-12) and abs(float(r["g_eps"]) - ge) < 1e-12
    if mode == "max":
        assert torch.equal(r["arg"], arg)
    # kernels=False on a CPU tensor is the same function
    assert torch.equal(ops.gin_aggregate(x, ev.detach(), C.Plan(csr), mode, bias, scale, kernels=False), out.detach())


def test_argument_checks_of_the_op():
    from wsi_hgnn_amd import ops
    csr, x, scale, _, bias = _small_case(False)
    plan, eps = C.Plan(csr), torch.zeros(1, dtype=torch.float64)
    with pytest.raises(ValueError, match="mode"):
        ops.gin_aggregate(x, eps, plan, "median")
    with pytest.raises(ValueError, match="one row per node"):
        ops.gin_aggregate(x[:5], eps, plan, "sum")
    with pytest.raises(ValueError, match="edge_scale"):
        ops.gin_aggregate(x, eps, plan, "sum", edge_scale=scale[:3])
    with pytest.raises(ValueError, match="eps"):
        ops.gin_aggregate(x, torch.zeros(2), plan, "sum")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gin_aggregate(x.float(), eps.float(), plan, "sum", kernels=True)
    assert ops.gin_project_first() is True
    ops.set_gin_project_first(False)
    assert ops.gin_project_first() is False
    ops.set_gin_project_first(True)


# ---------------------------------------------------------------------------------------------------- the model against the reference's logits
def _fixture_models():
    npz = np.load(os.path.join(GOLD, "reference_gin.npz"))
    for i, s in enumerate(npz["settings"].tolist()):
        neigh, pool, mlp, learn = s.split("|")
        state = {k.split("/", 2)[2]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(f"{i}/state/")}
        after = {k.split("/", 2)[2]: torch.from_numpy(npz[k]) for k in npz.files if k.startswith(f"{i}/after/")}
        yield npz, i, neigh, pool, int(mlp), learn == "True", state, after


def test_model_restatement_reproduces_the_reference_logits():
    seen = 0
    for npz, i, neigh, pool, mlp, learn, state, after in _fixture_models():
        csr = C.csr_of(12, npz["src"], npz["dst"])
        x, bnn = torch.from_numpy(npz["x"]), torch.from_numpy(npz["batch_num_nodes"])
        for train in (False, True):
            logits, buffers, _ = C.model_ref(state, x, csr, bnn, 2, mlp, neigh, pool, train)
            want = torch.from_numpy(npz[f"{i}/logits_{'train' if train else 'eval'}"])
            assert float((logits - want).abs().max()) < 1e-12, (i, train)
        for k, v in after.items():
            assert float((buffers[k].double() - v.double()).abs().max()) < 1e-12, (i, k)
        seen += 1
    assert seen == 4


def test_cpu_model_reproduces_the_reference_logits():
    """``models.GIN`` itself on the CPU in float64 (the tensor formulation), with the fixture's state loaded strictly."""
    from wsi_hgnn_amd.models import GIN
    for npz, i, neigh, pool, mlp, learn, state, after in _fixture_models():
        m = GIN(12, 8, 3, 2, mlp, 0.0, pool, neigh, learn).double()
        m.load_state_dict(state, strict=True)
        g, _ = _batch(npz)
        m.eval()
        assert float((m(g).detach() - torch.from_numpy(npz[f"{i}/logits_eval"])).abs().max()) < 1e-10
        m.train()
        assert float((m(g).detach() - torch.from_numpy(npz[f"{i}/logits_train"])).abs().max()) < 1e-10
        for k, v in after.items():
            assert float((m.state_dict()[k].double() - v.double()).abs().max()) < 1e-10, (i, k)


def test_train_mode_needs_two_rows():
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd.models import GIN
    m = GIN(4, 4, 2, 2, 1, 0.0, "sum", "sum", True)
    g = W.graph.HeteroGraph.homogeneous(1, torch.tensor([0]), torch.tensor([0]))
    g.ndata["feat"] = torch.ones(1, 4)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        m(g)
    m.eval()
    assert tuple(m(g).shape) == (1, 2)


# ---------------------------------------------------------------------------------------------------- dispatch rule, C ABI, boundary
def test_sweep_reaches_every_instantiation():
    reached = {C.gin_cfg(D, True) for D in C.GIN_SWEEP}
    assert reached == set(C.GIN_INSTANCES)
    assert {1, 3, 4, 32, 200, 512, 1023, 1024} <= set(C.GIN_SWEEP) and max(C.GIN_SWEEP) == 1024
    assert all(C.gin_cfg(D, False)[0] == 1 and C.gin_cfg(D, False) in C.GIN_INSTANCES for D in range(1, 1025))
    assert all(C.gin_cfg(D, True) in C.GIN_INSTANCES for D in range(1, 1025))
    assert {C.gin_cfg(D, True)[1] for D in C.GIN_SWEEP} == {4, 8, 16, 32, 64}
    codes = R.family_codes("gin.hip")
    assert codes == sorted(R.case_lists()[0]) and len(codes) == len(set(codes)) == 16
    assert {(c // 100000, c // 100 % 1000, c % 100) for c in codes} == set(C.GIN_INSTANCES)


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from wsi_hgnn_amd import _native
    return _native.load()


P = ctypes.c_void_p(1 << 40)      # a fake device address: every call below must fail its argument check before touching it
EINVAL, ENOSYS = -22, -38


def test_capi_argument_checks():
    lib = _lib()
    fwd = lambda **k: lib.wsi_gin_aggregate_fwd(k.get("x", P), k.get("ld", 16), k.get("n", 10), k.get("D", 16), k.get("rowptr", P), P, None,
                                                k.get("eps", P), k.get("mode", 0), None, k.get("out", P), 16, None, None)
    bwd = lambda **k: lib.wsi_gin_aggregate_bwd(k.get("g", P), k.get("ld", 16), k.get("n", 10), k.get("D", 16), P, P, P, P, None, k.get("eps", P),
                                                k.get("mode", 0), k.get("arg", None), k.get("gx", P), 16, None)
    edge = lambda **k: lib.wsi_gin_edge_grad(P, k.get("ld", 16), P, 16, k.get("n", 10), k.get("D", 16), P, P, k.get("mode", 0), k.get("arg", None),
                                             k.get("gs", P), None)
    epsg = lambda **k: lib.wsi_gin_eps_grad(P, k.get("ld", 16), P, 16, k.get("n", 10), k.get("D", 16), k.get("partial", P), P, None)
    for f in (fwd, bwd, edge, epsg):
        assert f(D=0) == EINVAL and f(n=-1) == EINVAL and f(ld=15) == EINVAL
        assert f(D=1028, ld=1028) == ENOSYS and f(D=1025, ld=1028) == ENOSYS
        assert b"1024" in lib.wsi_last_error()
        assert f(n=0) == 0
    for f in (fwd, bwd, edge):
        assert f(mode=3) == EINVAL and f(mode=-1) == EINVAL
    assert fwd(x=None) == EINVAL and fwd(rowptr=None) == EINVAL and fwd(eps=None) == EINVAL and fwd(out=None) == EINVAL
    assert bwd(g=None) == EINVAL and bwd(gx=None) == EINVAL and bwd(mode=2, arg=None) == EINVAL and bwd(eps=None) == EINVAL
    assert edge(mode=2, arg=None) == EINVAL
    assert epsg(partial=None) == EINVAL
    assert lib.wsi_gin_eps_partials() == 256


def test_new_code_reads_no_environment_variable():
    for rel in ("wsi-hgnn_amd/models/GIN.py", "wsi-hgnn_amd/csrc/gin.hip", "tools/gin_bench.py"):
        text = open(os.path.join(ROOT, rel)).read()
        assert not re.search(r"os\.environ|\bgetenv\b", text), rel
