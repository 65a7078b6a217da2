"""GAT — drop-in for the reference's ``models/GAT.py:17-92`` (DGL ``GATConv`` + glob poolings).

GATConv = ``fc`` projection on the MFMA GEMM (``ops.linear``: ``set_gemm_precision`` applies), then one HIP edge kernel
(``ops.gat_attention``: per-head edge softmax of leaky_relu(el[src] + er[dst]), weighted neighbour sum, bias and activation
fused; csrc/gat_attn.hip).  ``feat_drop`` / ``attn_drop`` in training mode are counter-based masks (``ops.CounterDropout``):
functions of (seed, element), regenerated in the backward, never stored.  Parameters and ``state_dict`` keys follow DGL >= 0.8's
``GATConv``: ``fc.weight`` [H*D, in], ``attn_l`` / ``attn_r`` [1, H, D], ``bias`` [H*D].
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..graph import message_scale_of
from .heat_net import make_pool


class GatPlan:
    """The homogeneous kernel plan of a graph, checked once for nodes without in-edges."""

    def __init__(self, g):
        p = g.plan()
        n = p.num_nodes
        if n and int((p.rowptr[1:n + 1] - p.rowptr[:n]).min()) == 0:        # one host sync per graph, never per forward
            raise ValueError("GATConv: the graph has nodes with zero in-degree; their output would be invalid (DGL's "
                             "allow_zero_in_degree=False). Add self-loops (the reference datasets do, data.py:119-121).")
        self.rowptr, self.src, self.colptr, self.csc_eid, self.csc_dst = p.rowptr, p.src, p.colptr, p.csc_eid, p.csc_dst
        self.order_dst, self.order_src = p.order_dst, p.order_src
        self.num_nodes, self.num_edges = n, p.num_edges


def gat_plan(g) -> GatPlan:
    if "_gat_plan" not in g.__dict__:
        if len(g.ntypes) != 1 or len(g.canonical_etypes) != 1:
            raise ValueError("GATConv needs a homogeneous graph (use wsi_hgnn_amd.graph.to_homogeneous)")
        g.__dict__["_gat_plan"] = GatPlan(g)
    return g.__dict__["_gat_plan"]


def _fused_activation(fn):
    """The name ``ops.gat_attention`` fuses for ``fn`` (F.relu / F.leaky_relu with its default slope), or False."""
    if fn is None:
        return None
    name = getattr(fn, "__name__", "")
    if name in ("relu", "leaky_relu"):
        return name
    return False


class GATConv(nn.Module):
    """dgl.nn.pytorch.GATConv(in_feats, out_feats, num_heads, feat_drop, attn_drop, negative_slope, residual, activation) with
    DGL's defaults otherwise (bias=True, allow_zero_in_degree=False); parameters created and initialised as DGL does
    (xavier_normal_ with gain calculate_gain('relu'), bias zero).  ``forward(g, feat)`` -> [N, num_heads, out_feats]."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2, residual=False, activation=None):
        super().__init__()
        if residual:
            raise NotImplementedError("GATConv(residual=True) is not implemented (no reference config builds it: parser.py passes "
                                      "residual=False)")
        self._num_heads, self._in_feats, self._out_feats = num_heads, in_feats, out_feats
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.feat_drop = nn.Dropout(feat_drop)
        self.attn_drop = nn.Dropout(attn_drop)
        self.leaky_relu = nn.LeakyReLU(negative_slope)
        self.bias = nn.Parameter(torch.empty(num_heads * out_feats))
        self.register_buffer("res_fc", None)
        self.reset_parameters()
        self.activation = activation

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)
        nn.init.constant_(self.bias, 0)

    def _draw(self, p: float, device):
        if not self.training or p <= 0.0:
            return None
        return ops.CounterDropout(p, ops.next_dropout_seed(), ops.current_dropout_seed_base(device))

    def forward(self, g, feat):
        plan = gat_plan(g)
        x = feat.to(torch.float32)
        drop = self._draw(self.feat_drop.p, x.device)
        if drop is not None:
            x = ops.counter_dropout(x, drop)
        ft = ops.linear(x, self.fc.weight, None)
        act = _fused_activation(self.activation)
        rst = ops.gat_attention(ft, self.attn_l, self.attn_r, self.bias, plan, self.leaky_relu.negative_slope,
                                activation=act or None, attn_drop=self._draw(self.attn_drop.p, x.device),
                                edge_scale=message_scale_of(g))         # graph.message_scale (GNNExplainer): None outside such a block
        if act is False:
            rst = self.activation(rst)
        return rst.view(-1, self._num_heads, self._out_feats)


class GAT(nn.Module):
    def __init__(self, n_layers, in_dim, hidden_dim, out_dim, heads, activation, feat_drop, attn_drop, negative_slope, residual,
                 graph_pooling_type="att"):
        super().__init__()
        self.n_layers = n_layers
        self.layers = nn.ModuleList()
        self.activation = activation
        for l in range(n_layers + 1):                                                   # GAT.py:36-53
            if l == 0:
                self.layers.append(GATConv(in_dim, hidden_dim, heads[0], feat_drop, attn_drop, negative_slope, False, self.activation))
            elif l == n_layers:
                self.layers.append(GATConv(hidden_dim * heads[-2], out_dim, heads[-1], feat_drop, attn_drop, negative_slope, residual, None))
            else:
                self.layers.append(GATConv(hidden_dim * heads[l - 1], hidden_dim, heads[l], feat_drop, attn_drop, negative_slope, residual,
                                           self.activation))
        self.linears_prediction = nn.ModuleList()
        self.pools = nn.ModuleList()
        for layer in range(n_layers + 1):                                               # :57-79
            width = in_dim if layer == 0 else hidden_dim * heads[layer - 1]
            self.linears_prediction.append(nn.Linear(width, out_dim))
            self.pools.append(make_pool(graph_pooling_type, layer, in_dim, width))

    def dead_parameter_names(self):
        """``layers[n_layers]`` is created (GAT.py:42-46) and applied, but its output is never read (:89 stacks the readouts of the
        layer INPUTS only): it never receives a gradient, and ``forward`` here skips it."""
        return [n for n, _ in self.named_parameters() if n.startswith(f"layers.{self.n_layers}.")]

    def forward(self, g, h=None):
        if h is None:
            h = g.ndata["feat"]                                                         # GAT.py:82-83
        h = h.to(torch.float32)
        h_list = []
        for i in range(self.n_layers + 1):                                              # :86-90
            p = self.pools[i](g, h)
            h_list.append(ops.linear(p, self.linears_prediction[i].weight, self.linears_prediction[i].bias))
            if i < self.n_layers:                                                       # the last layer's output is discarded
                h = self.layers[i](g, h).flatten(1)
        return torch.stack(h_list).mean(0)                                              # :92
