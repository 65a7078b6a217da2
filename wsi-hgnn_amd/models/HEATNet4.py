"""HEATNet4 — drop-in for the reference's ``models/HEATNet4.py:141-247`` on the MI355X kernels.

Constructor signature (including the ``dropuout`` spelling), ``forward(G, h=None) -> [B, out_dim]``,
``n_layers`` and every ``state_dict`` key of the reference are kept.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from .heat_layer import HEATLayer
from .heat_net import HEATTrunk, make_pool


class _IdentityZeroGrad(torch.autograd.Function):
    """y = l (no kernel); backward: dl = dy, dw = 0 — what `softmax` over a length-1 axis followed by `a * l` amounts to."""

    @staticmethod
    def forward(ctx, l, w):
        ctx.save_for_backward(w)
        return l.view_as(l)

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return g, torch.zeros_like(w)


class _IdentityZeroGrads(torch.autograd.Function):
    """The same for the concatenated blocks of several LinearAttentionBlocks at once: y = x, zero gradients for all their weights
    (one zero-filled buffer, one view per weight)."""

    @staticmethod
    def forward(ctx, x, *ws):
        ctx.shapes = [w.shape for w in ws]
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        sizes = [int(torch.Size(s).numel()) for s in ctx.shapes]
        z = torch.zeros(sum(sizes), dtype=g.dtype, device=g.device)
        outs, pos = [], 0
        for s, k in zip(ctx.shapes, sizes):
            outs.append(z[pos:pos + k].view(s))
            pos += k
        return (g, *outs)


class LinearAttentionBlock(nn.Module):
    """models/HEATNet4.py:20-42.  For [N,C] inputs the softmax is over a length-1 axis, so the block
    returns ``l`` unchanged and ``op.weight`` gets an exactly-zero gradient; this class
    keeps the parameter (state_dict key ``attn.{k}.op.weight``) and reproduces that behaviour
    without launching the dead Conv1d/softmax."""

    def __init__(self, in_features, normalize_attn=True):
        super().__init__()
        self.normalize_attn = normalize_attn
        self.op = nn.Conv1d(in_channels=in_features, out_channels=1, kernel_size=1, padding=0, bias=False)

    def forward(self, l, g):
        if not self.normalize_attn:
            a = torch.sigmoid(((l + g) * self.op.weight.view(1, -1)).sum(dim=1, keepdim=True))
            return a * l
        return _IdentityZeroGrad.apply(l, self.op.weight)   # identity; zero (not None) gradient for op.weight


class HEATNet4(HEATTrunk):
    def __init__(self, in_dim, hidden_dim, out_dim, n_layers, n_heads, node_dict, dropuout, graph_pooling_type='mean'):
        super().__init__()
        self.node_dict = node_dict
        self.gcs = nn.ModuleList()
        self.n_inp, self.n_hid, self.n_out = in_dim, hidden_dim, out_dim
        self.n_layers, self.n_heads = n_layers, n_heads
        self.adapt_ws = nn.ModuleList()
        self.pools = nn.ModuleList()
        self.linears_prediction = nn.ModuleDict({k: nn.Linear(hidden_dim, 256) for k in node_dict})
        for _ in range(len(node_dict)):
            self.adapt_ws.append(nn.Linear(in_dim, hidden_dim))
        for _ in range(n_layers):
            self.gcs.append(HEATLayer(hidden_dim, hidden_dim, node_dict, n_heads, dropuout))
        self.attn = nn.ModuleDict({a: LinearAttentionBlock(in_features=256, normalize_attn=True) for a in node_dict})
        for layer in range(n_layers + 1):
            self.pools.append(make_pool(graph_pooling_type, layer, in_dim, hidden_dim))
        self.head_2 = nn.Linear(256 * len(node_dict), 256)
        self.head_1 = nn.Linear(256, 64)
        self.head = nn.Linear(64, out_dim)

    def type_gated_parameters(self):
        """Per node-type position (sorted type names) the parameters whose gradient is ``None`` - not zero - when an unpadded batch has no
        node of the type: what a captured step over ``BatchSlot(type_mask=True)`` must keep from the optimizer (``optim.gate``, DESIGN
        3.29).  With every block normalised (the fused path) the absent type's projection is not a group of the GEMM and its block is not
        called: ``linears_prediction[k].weight / .bias`` and ``attn[k].op.weight``.  Otherwise all projections run as one grouped GEMM
        (exact zero gradients for the absent one) and only ``attn[k].op.weight`` is never reached."""
        types = sorted(self.node_dict)
        fused = all(self.attn[t].normalize_attn for t in types)
        return [(list(self.linears_prediction[t].parameters()) if fused else []) + [self.attn[t].op.weight] for t in types]

    def forward(self, G, h=None):
        ctx, hcat, pooled, B = self.encode(G, h, predict=False)
        T = len(ctx.ntypes)
        mask = getattr(G, "_type_present", None)                             # a slot's device-side presence table: the filler
        # gives every type rows, so the host test below is all True there and the table zeroes what belongs to a type the real slides lack
        present = [(b - a) > 0 for (a, b) in ctx.rows]                       # HEATNet4.py:218,230 h[k].shape[0] > 0
        lins = [self.linears_prediction[t] for t in ctx.ntypes]
        width = lins[0].weight.shape[0]
        if any(present) and all(self.attn[t].normalize_attn for t in ctx.ntypes):
            # every block is the identity (the sum `g` of :229-232 is read by nobody): the per-type projections (:219) write
            # their 256 columns of the concatenation of :242 directly - no slices, no cat, and in the backward no copies back
            idx = [i for i in range(T) if present[i]]
            spec = ctx.cache.get(("pred_cat", B, width, tuple(idx)))
            if spec is None:
                spec = ctx.cache[("pred_cat", B, width, tuple(idx))] = ops.LinearSpec(
                    [(i * B, (i + 1) * B) for i in idx], [i * width for i in idx], T * width, T * B,
                    out_rows=[(0, B)] * len(idx), num_out_rows=B)             # absent node types: zero columns (:240)
            g = ops.grouped_linear(pooled, spec, [lins[i].weight for i in idx], [lins[i].bias for i in idx])
            g = _IdentityZeroGrads.apply(g, *[self.attn[ctx.ntypes[i]].op.weight for i in idx])
            if mask is not None:                                             # an absent type: exact zero columns (:240)
                g = (g.view(B, T, width) * mask.view(1, T, 1)).view(B, T * width)
        else:
            spec = ctx.cache.get(("pred", B, width))
            if spec is None:
                spec = ctx.cache[("pred", B, width)] = ops.LinearSpec([(i * B, (i + 1) * B) for i in range(T)], [0] * T, width, T * B)
            out = ops.grouped_linear(pooled, spec, [l.weight for l in lins], [l.bias for l in lins])      # :219
            hg = 0
            for i, t in enumerate(ctx.ntypes):                               # :229-232
                if present[i]:
                    hg = hg + (out[i * B:(i + 1) * B] if mask is None else mask[i] * out[i * B:(i + 1) * B])
            parts = []
            for i, t in enumerate(ctx.ntypes):                               # :236-240
                if present[i]:
                    part = self.attn[t](out[i * B:(i + 1) * B], hg)
                    parts.append(part if mask is None else mask[i] * part)
                else:
                    parts.append(torch.zeros(B, width, dtype=out.dtype, device=out.device))
            g = torch.cat(parts, dim=1)                                      # :242
        g = ops.linear(g, self.head_2.weight, self.head_2.bias)              # :243
        g = ops.linear(g, self.head_1.weight, self.head_1.bias)              # :244
        return ops.linear(g, self.head.weight, self.head.bias)               # :245
