#!/usr/bin/env python
"""Generates tests/golden/gin/reference_gin.json and reference_gin.npz FROM THE REFERENCE ITSELF.

    python tests/golden/make_reference_gin_fixture.py <path of the reference checkout>

The reference is read and executed, never copied: the fixture holds names, shapes and arrays only.

  * ``parser.parse_gnn_model`` (parser.py:48-174) is executed with a recording stand-in bound to ``GIN`` on the ``GNN:`` block of
    configs/COAD/GIN_COAD.yml and GIN_Hover_v2.yml: the recorded keyword arguments go to the JSON file.
  * models/GIN.py is executed as a module.  DGL is absent, so ``dgl.nn.pytorch.conv.GINConv`` and the four ``dgl.nn.pytorch.glob`` poolings
    are stand-ins written here from DGL's documented semantics (rst = (1 + eps) x + reduce over in-neighbours, eps a Parameter of shape [1]
    when learned and a buffer otherwise, the reducer's value 0 for a node without in-edges; sum / mean / max / softmax-gated readouts per
    graph).  Everything else - ApplyNodeFunc, MLP, GIN, their parameter creation order and GIN.forward - is the reference's own code.
  * state_dict key and shape lists of the reference's ``GIN`` for num_mlp_layers in {1, 2} x graph_pooling_type in {sum, att} x learn_eps in
    {True, False} (num_layers = 3, so that the branches for layers beyond the first are taken) go to the JSON file.
  * inputs, state and logits of the reference's own ``GIN.forward`` (num_layers = 2, the only depth it runs: GIN.py:160) on a batch of two
    graphs of 5 and 7 nodes, input_dim 12, hidden 8, 3 classes, float64, in eval and in train mode, go to the npz file.
"""
import ast
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import yaml

REF = sys.argv[1]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gin")
os.makedirs(OUT, exist_ok=True)


# ---------------------------------------------------------------------------------------------------- stand-ins for DGL
class Graph:
    """What the stand-ins need of a batched DGLGraph: edge lists and the node count of every graph."""

    def __init__(self, src, dst, bnn):
        self.src, self.dst, self.bnn = src, dst, bnn
        self.n = int(bnn.sum())
        self.seg = torch.repeat_interleave(torch.arange(bnn.numel()), bnn)


class GINConv(nn.Module):
    def __init__(self, apply_func=None, aggregator_type="sum", init_eps=0, learn_eps=False):
        super().__init__()
        self.apply_func = apply_func
        self._aggregator_type = aggregator_type
        if learn_eps:
            self.eps = nn.Parameter(torch.FloatTensor([init_eps]))
        else:
            self.register_buffer("eps", torch.FloatTensor([init_eps]))

    def forward(self, graph, feat):
        neigh = torch.zeros_like(feat)
        for w in range(graph.n):
            rows = feat[graph.src[graph.dst == w]]
            if rows.shape[0]:
                neigh[w] = {"sum": rows.sum(0), "mean": rows.mean(0), "max": rows.max(0).values}[self._aggregator_type]
        rst = (1 + self.eps) * feat + neigh
        return self.apply_func(rst) if self.apply_func is not None else rst


class _Pool(nn.Module):
    def forward(self, graph, feat):
        return torch.stack([self.one(feat[graph.seg == b]) for b in range(graph.bnn.numel())])


class SumPooling(_Pool):
    one = staticmethod(lambda rows: rows.sum(0))


class AvgPooling(_Pool):
    one = staticmethod(lambda rows: rows.mean(0))


class MaxPooling(_Pool):
    one = staticmethod(lambda rows: rows.max(0).values)


class GlobalAttentionPooling(_Pool):
    def __init__(self, gate_nn):
        super().__init__()
        self.gate_nn = gate_nn

    def one(self, rows):
        return (torch.softmax(self.gate_nn(rows), 0) * rows).sum(0)


def module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


for name in ("dgl", "dgl.nn", "dgl.nn.pytorch"):
    module(name)
module("dgl.nn.pytorch.conv", GINConv=GINConv)
module("dgl.nn.pytorch.glob", SumPooling=SumPooling, AvgPooling=AvgPooling, MaxPooling=MaxPooling, GlobalAttentionPooling=GlobalAttentionPooling)

ref_gin = types.ModuleType("reference_gin")
exec(compile(open(os.path.join(REF, "models", "GIN.py")).read(), "models/GIN.py", "exec"), ref_gin.__dict__)

# ---------------------------------------------------------------------------------------------------- the parser's calls
psrc = open(os.path.join(REF, "parser.py")).read()
fn = next(n for n in ast.parse(psrc).body if isinstance(n, ast.FunctionDef) and n.name == "parse_gnn_model")
ns = {"F": F, "nn": nn, "GIN": lambda *a, **k: {"class": "GIN", "args": list(a), "kwargs": k}}
exec(ast.get_source_segment(psrc, fn), ns)
fixture = {"source": "models/GIN.py, parser.py:48-174 and configs/COAD/GIN_*.yml of the reference, executed with DGL stand-ins", "parse_gnn_model": [],
           "state_dicts": []}
for cfg in ("GIN_COAD.yml", "GIN_Hover_v2.yml"):
    gnn = yaml.safe_load(open(os.path.join(REF, "configs", "COAD", cfg)))["GNN"]
    fixture["parse_gnn_model"].append({"config": f"configs/COAD/{cfg}", "GNN": gnn, "constructs": ns["parse_gnn_model"](gnn)})

# ---------------------------------------------------------------------------------------------------- state_dict keys and shapes
for mlp in (1, 2):
    for pool in ("sum", "att"):
        for learn in (True, False):
            kw = dict(input_dim=12, hidden_dim=8, out_dim=3, num_layers=3, num_mlp_layers=mlp, final_dropout=0.0, graph_pooling_type=pool,
                      neighbor_pooling_type="mean", learn_eps=learn)
            m = ref_gin.GIN(**kw)
            fixture["state_dicts"].append({"kwargs": kw, "parameters": [n for n, _ in m.named_parameters()],
                                           "state": [[k, list(v.shape)] for k, v in m.state_dict().items()]})
json.dump(fixture, open(os.path.join(OUT, "reference_gin.json"), "w"), indent=1)

# ---------------------------------------------------------------------------------------------------- GIN.forward
gen = torch.Generator().manual_seed(2911)
sizes = [5, 7]
src, dst, off = [], [], 0
for n in sizes:
    k = 3 * n
    src.append(torch.randint(0, n, (k,), generator=gen) + off)
    dst.append(torch.randint(1, n, (k,), generator=gen) + off)      # the first node of every graph has no in-edge
    off += n
src, dst = torch.cat(src), torch.cat(dst)
src[1], dst[1] = src[0], dst[0]                                       # a duplicate edge
bnn = torch.tensor(sizes)
x = torch.randn(off, 12, generator=gen, dtype=torch.float64)
graph = Graph(src, dst, bnn)
arrays = {"x": x.numpy(), "src": src.numpy(), "dst": dst.numpy(), "batch_num_nodes": bnn.numpy()}
settings = [("mean", "att", 2, True), ("max", "sum", 1, True), ("sum", "mean", 2, False), ("mean", "max", 1, True)]
arrays["settings"] = np.array(["|".join(map(str, s)) for s in settings])
for i, (neigh, pool, mlp, learn) in enumerate(settings):
    torch.manual_seed(100 + i)
    m = ref_gin.GIN(12, 8, 3, 2, mlp, 0.0, pool, neigh, learn).double()
    with torch.no_grad():
        for k, v in m.state_dict().items():                           # statistics and affine terms away from their initial 0 / 1
            if k.endswith("running_mean") or k.endswith("bn.bias") or ".batch_norms." in k and k.endswith(".bias"):
                v.copy_(0.3 * torch.randn(v.shape, generator=gen, dtype=torch.float64))
            elif k.endswith("running_var") or k.endswith("bn.weight") or ".batch_norms." in k and k.endswith(".weight"):
                v.copy_(0.5 + torch.rand(v.shape, generator=gen, dtype=torch.float64))
            elif k.endswith(".eps"):
                v.fill_(0.3)
    for k, v in m.state_dict().items():
        arrays[f"{i}/state/{k}"] = v.detach().numpy().copy()
    m.eval()
    arrays[f"{i}/logits_eval"] = m(graph, x).detach().numpy()
    m.train()
    arrays[f"{i}/logits_train"] = m(graph, x).detach().numpy()
    for k, v in m.state_dict().items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            arrays[f"{i}/after/{k}"] = v.detach().numpy().copy()
np.savez_compressed(os.path.join(OUT, "reference_gin.npz"), **arrays)
print("wrote", OUT, {f: os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT)})
