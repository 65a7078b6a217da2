#!/usr/bin/env python
"""Fixtures produced by EXECUTING the reference's own H2MIL layers (baselines/H2MIL/code/RAConv.py and IHPool.py) in float64 on seeded inputs.
Data only; no reference source travels.

The reference imports torch_geometric, torch_scatter and torch_sparse, none of which is installed where this runs.  The stand-ins below
implement, from their documented definitions, exactly what the two files call:
  torch_scatter.scatter(src, index, dim, reduce in {sum, add, mean, max}); torch_geometric.utils.softmax (max-subtracted, + 1e-16 in the
  denominator); add_remaining_self_loops; MessagePassing.propagate for node_dim = 0, aggr = 'add' (gathers ``_j`` at edge_index[0] and ``_i`` at
  edge_index[1], passes index = edge_index[1], sums the messages at dim_size = x[1].size(0)); a constructor for LEConv (never called in forward).
Everything else the files import is a name that is never used.

h2mil/reference_raconv.npz: RAConv.forward on a graph of 40 nodes of all three types with nodes without in-edges, a destination with one
group, a destination with three and repeated edges: inputs, state_dict with key order, output, gradients of a seeded linear functional.
h2mil/reference_ihpool.npz: IHPool.forward, a ratio = 0.2 layer followed by a ratio = 4 layer on its output, and a ratio = 0.1 layer: all
nine outputs of each.  The inputs are drawn with consecutive seeds until tests/h2mil_cases.py's margin condition holds for all three layers
(asserted).  Weights and inputs are rounded to float32 first and stored as float32.
Re-run where the reference is checked out: ``python tests/golden/make_reference_h2mil_fixture.py``."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/baselines/H2MIL/code"
sys.path.insert(0, os.path.dirname(HERE))


def scatter(src, index, dim=0, out=None, dim_size=None, reduce="sum"):
    src_m = src.movedim(dim, 0)
    n = int(index.max()) + 1 if dim_size is None else int(dim_size)
    shape = (n,) + tuple(src_m.shape[1:])
    if reduce in ("sum", "add", "mean"):
        res = torch.zeros(shape, dtype=src.dtype).index_add(0, index, src_m)
        if reduce == "mean":
            cnt = torch.zeros(n, dtype=src.dtype).index_add(0, index, torch.ones(index.shape[0], dtype=src.dtype)).clamp(min=1)
            res = res / cnt.view((n,) + (1,) * (src_m.dim() - 1))
    elif reduce == "max":
        idx = index.view((-1,) + (1,) * (src_m.dim() - 1)).expand_as(src_m)
        res = torch.zeros(shape, dtype=src.dtype).scatter_reduce(0, idx, src_m, "amax", include_self=False)
    else:
        raise ValueError(reduce)
    return res.movedim(0, dim)


def pyg_softmax(src, index, ptr=None, num_nodes=None, dim=0):
    n = int(index.max()) + 1 if num_nodes is None else int(num_nodes)
    src_max = scatter(src.detach(), index, dim, dim_size=n, reduce="max")
    out = (src - src_max.index_select(dim, index)).exp()
    out_sum = scatter(out, index, dim, dim_size=n, reduce="sum") + 1e-16
    return out / out_sum.index_select(dim, index)


def add_remaining_self_loops(edge_index, edge_attr=None, fill_value=None, num_nodes=None):
    n = int(edge_index.max()) + 1 if num_nodes is None else num_nodes
    mask = edge_index[0] != edge_index[1]
    loop = torch.arange(n, dtype=edge_index.dtype).unsqueeze(0).repeat(2, 1)
    assert edge_attr is None
    return torch.cat([edge_index[:, mask], loop], 1), None


class MessagePassing(torch.nn.Module):
    def __init__(self, aggr="add", node_dim=0, **kwargs):
        super().__init__()
        assert aggr == "add" and node_dim == 0

    def propagate(self, edge_index, size=None, **kw):
        x, alpha = kw["x"], kw["alpha"]
        j, i = edge_index[0], edge_index[1]
        dim_size = x[1].size(0)
        msg = self.message(x_j=x[0][j], alpha_j=alpha[0][j], alpha_i=alpha[1][i], soft_index=kw["soft_index"], type_edge=kw["type_edge"],
                           node_size=kw["node_size"], index=i, ptr=None, size_i=dim_size)
        return torch.zeros((dim_size,) + tuple(msg.shape[1:]), dtype=msg.dtype).index_add(0, i, msg)


class LEConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__()
        self.lin1 = torch.nn.Linear(in_channels, out_channels, bias=bias)
        self.lin2 = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.lin3 = torch.nn.Linear(in_channels, out_channels, bias=bias)

    def reset_parameters(self):
        for l in (self.lin1, self.lin2, self.lin3):
            l.reset_parameters()


def install_stand_ins():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    unused = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("a stand-in that the two layers never call"))
    mod("torch_scatter", scatter=scatter)
    mod("torch_sparse", SparseTensor=type("SparseTensor", (), {}), set_diag=unused, spspmm=unused)
    pyg = mod("torch_geometric")
    pyg.nn = mod("torch_geometric.nn", LEConv=LEConv)
    pyg.nn.conv = mod("torch_geometric.nn.conv", MessagePassing=MessagePassing)
    pyg.nn.pool = mod("torch_geometric.nn.pool")
    pyg.nn.pool.topk_pool = mod("torch_geometric.nn.pool.topk_pool", topk=unused)
    pyg.utils = mod("torch_geometric.utils", remove_self_loops=unused, add_self_loops=unused, softmax=pyg_softmax,
                    add_remaining_self_loops=add_remaining_self_loops, sort_edge_index=unused)
    any_t = object
    pyg.typing = mod("torch_geometric.typing", OptPairTensor=any_t, Adj=any_t, Size=any_t, NoneType=any_t, OptTensor=any_t)
    for name, attrs in (("sklearn", {}), ("sklearn.cluster", {"KMeans": unused}), ("sklearn.metrics", {}),
                        ("sklearn.metrics.pairwise", {"cosine_similarity": unused}), ("scipy", {}), ("scipy.spatial", {}),
                        ("scipy.spatial.distance", {"cdist": unused})):
        try:
            importlib.import_module(name)
        except Exception:
            mod(name, **attrs)


def raconv_graph(gen):
    """40 nodes: 0 root, 1..12 level 1, 13..39 level 2.  Nodes 36..39 receive no edge; node 20 receives edges from one type only; node 5 from
    all three; the edge 14 -> 15 appears three times."""
    n = 40
    nt = torch.tensor([0] + [1] * 12 + [2] * 27, dtype=torch.int64)
    src = torch.randint(0, n, (150,), generator=gen)
    dst = torch.randint(0, 36, (150,), generator=gen)
    keep = dst != 20
    src, dst = src[keep], dst[keep]
    extra = [(13, 20), (17, 20), (30, 20), (0, 5), (3, 5), (22, 5), (14, 15), (14, 15), (14, 15), (7, 7)]
    src = torch.cat([src, torch.tensor([a for a, _ in extra])])
    dst = torch.cat([dst, torch.tensor([b for _, b in extra])])
    return n, nt, torch.stack([src, dst])


def make_raconv():
    RA = importlib.import_module("RAConv")
    gen = torch.Generator().manual_seed(1911)
    torch.manual_seed(1911)
    cin, cout = 12, 8
    m = RA.RAConv(cin, cout).double()
    with torch.no_grad():
        m.bias.add_(0.1 * torch.randn(cout, generator=gen, dtype=torch.float64))
        for p in m.parameters():
            p.copy_(p.to(torch.float32).to(torch.float64))
    n, nt, ei = raconv_graph(gen)
    x32 = torch.randn(n, cin, generator=gen, dtype=torch.float32)
    w = torch.randn(n, cout, generator=gen, dtype=torch.float64)
    x = x32.double().requires_grad_(True)
    out = m(x, ei, nt)
    (out * w).sum().backward()
    fix = {"x": x32.numpy(), "edge_index": ei.numpy(), "node_type": nt.numpy(), "w": w.numpy(), "out": out.detach().numpy(), "g.x": x.grad.numpy(),
           "keys": np.asarray(list(m.state_dict().keys())), "config": np.asarray([cin, cout], dtype=np.int64)}
    for k, v in m.state_dict().items():
        fix["sd." + k] = v.to(torch.float32).numpy()
    for k, p in m.named_parameters():
        fix["g." + k] = p.grad.numpy()
    return fix


NINE = ("x", "edge_index", "edge_weight", "batch", "cluster", "node_type", "tree", "fitness", "x_y_index")


def make_ihpool():
    import h2mil_cases as C
    IH = importlib.import_module("IHPool")
    cin = 10
    torch.manual_seed(1912)
    layers = {"a": IH.IHPool(cin, ratio=0.2).double(), "b": IH.IHPool(cin, ratio=4).double(), "c": IH.IHPool(cin, ratio=0.1).double()}
    with torch.no_grad():
        for m in layers.values():
            for p in m.parameters():
                p.copy_(p.to(torch.float32).to(torch.float64))

    def run(seed):
        s32 = C.tree_slide(seed, 25, (1, 5), feat=cin)
        s = C.double(s32)
        xy = (s32["x_y_index"] * 2 - 1).double()                    # the float32 coordinates the fixture stores
        args = (s["x"], s["edge_index_tree_8nb"], s["node_type"], s["node_tree"], xy)
        ref = lambda m, a: C.ihpool_ref(a[0], a[1], a[2], a[3], a[4], m.weight_1.detach(), m.weight_2.detach(), m.ratio)
        ra = ref(layers["a"], args)
        rb = ref(layers["b"], (ra["x"], ra["edge_index"], ra["node_type"], ra["tree"], ra["x_y_index"]))
        rc = ref(layers["c"], args)
        return s, args, min(ra["margin"], rb["margin"], rc["margin"])

    for seed in range(C.TRIES):
        s, args, margin = run(seed)
        if margin >= C.MARGIN:
            break
    assert margin >= C.MARGIN, "no input met the margin condition"
    with torch.no_grad():
        oa = layers["a"](x=args[0], edge_index=args[1], node_type=args[2], tree=args[3], x_y_index=args[4])
        ob = layers["b"](x=oa[0], edge_index=oa[1], node_type=oa[5], tree=oa[6], x_y_index=oa[8])
        oc = layers["c"](x=args[0], edge_index=args[1], node_type=args[2], tree=args[3], x_y_index=args[4])
    slide32 = C.tree_slide(seed, 25, (1, 5), feat=cin)
    fix = {"seed": np.asarray(seed), "margin": np.asarray(margin), "config": np.asarray([cin], dtype=np.int64),
           "x": slide32["x"].numpy(), "edge_index": args[1].numpy(), "node_type": args[2].numpy(), "tree": args[3].numpy(),
           "x_y_index": (slide32["x_y_index"] * 2 - 1).numpy(), "keys": np.asarray(list(layers["a"].state_dict().keys()))}
    assert torch.equal((slide32["x_y_index"] * 2 - 1).double(), args[4])
    for name, m, o in (("a", layers["a"], oa), ("b", layers["b"], ob), ("c", layers["c"], oc)):
        fix[f"{name}.ratio"] = np.asarray(float(m.ratio))
        for k, v in m.state_dict().items():
            fix[f"{name}.sd.{k}"] = v.to(torch.float32).numpy()
        for field, v in zip(NINE, o):
            fix[f"{name}.{field}"] = np.zeros(0) if v is None else v.detach().numpy()
    return fix


def main():
    install_stand_ins()
    sys.path.insert(0, REF)
    out_dir = os.path.join(HERE, "h2mil")
    os.makedirs(out_dir, exist_ok=True)
    for name, fix in (("reference_raconv.npz", make_raconv()), ("reference_ihpool.npz", make_ihpool())):
        out = os.path.join(out_dir, name)
        np.savez_compressed(out, **fix)
        print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
