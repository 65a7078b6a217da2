"""RAConv of the H2MIL baseline (``baselines/H2MIL/code/RAConv.py``) at the one configuration the reference builds: heads = 1, one input
tensor, add_self_loops = False, dropout = 0.

The reference projects the per-(destination, source type) means of the RAW features with ``t_lin_l`` (a [3N, in] matrix through a 1024-wide
projection), runs a resolution-level attention over them and throws its aggregation away: only that attention's weights survive, and by
linearity of the mean they need two scalars per node, pl = <x, W_t^T t_att_l> and pr = <x, W_t^T t_att_r>.  Both are two extra output columns
of the one projection (the folded vectors are formed with tensor operations, so autograd carries the gradients of ``t_lin_l`` and the two
``t_att``); the group means are never formed.  ``ops.ra_attention`` does the rest in one kernel each way.
Excluded, not stubbed: ``return_attention_weights``, ``heads > 1``, tuple inputs, SparseTensor adjacencies, attention dropout.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


def _glorot(t: torch.Tensor) -> None:
    stdv = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    t.data.uniform_(-stdv, stdv)


def ra_attention_tensor(ft, sc, bias, src, dst, node_type, negative_slope: float = 0.2):
    """``ops.ra_attention`` in tensor operations, any device and dtype: ``src`` / ``dst`` [E] int64 in any order."""
    n = ft.shape[0]
    el, er, pl, pr = sc.unbind(1)
    grp = dst * 3 + node_type[src]
    s = F.leaky_relu(el[src] + er[dst], negative_slope)
    mx = torch.full((3 * n,), -math.inf, dtype=s.dtype, device=s.device).scatter_reduce(0, grp, s.detach(), "amax", include_self=True)
    ex = torch.exp(s - mx[grp])
    a = ex / torch.zeros(3 * n, dtype=s.dtype, device=s.device).index_add(0, grp, ex)[grp]
    cnt = torch.zeros(3 * n, dtype=s.dtype, device=s.device).index_add(0, grp, torch.ones_like(s))
    mean_pl = torch.zeros(3 * n, dtype=s.dtype, device=s.device).index_add(0, grp, pl[src]) / cnt.clamp(min=1)
    q = F.leaky_relu(mean_pl.view(n, 3) + pr.view(n, 1), negative_slope)
    present = cnt.view(n, 3) > 0
    q = torch.where(present, q, torch.full_like(q, -math.inf))
    qmax = torch.where(present.any(1, keepdim=True), q.detach().max(1, keepdim=True).values, torch.zeros_like(q[:, :1]))
    eq = torch.where(present, torch.exp(q - qmax), torch.zeros_like(q))
    beta = eq / eq.sum(1, keepdim=True).clamp(min=1e-300 if q.dtype == torch.float64 else 1e-30)
    w = beta.reshape(-1)[grp] * a
    out = torch.zeros_like(ft).index_add(0, dst, w.unsqueeze(1) * ft[src])
    return out if bias is None else out + bias


class RAConv(nn.Module):
    """The reference's constructor arguments, defaults and ``state_dict`` keys (``lin_r`` and ``t_lin_r`` are the same modules as ``lin_l`` and
    ``t_lin_l``, as there, so their keys appear too).  ``forward(x, edges, node_type)``: ``edges`` is a ``TreeBatch`` (its cached edge plan is
    used) or an ``edge_index`` [2, E] tensor.  ``kernels=False`` is the same layer in tensor operations."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=False, bias=True,
                 kernels=True, **kwargs):
        super().__init__()
        if not isinstance(in_channels, int):
            raise ValueError("RAConv: one input tensor (in_channels is an int); the reference's tuple form is not built")
        if heads != 1:
            raise ValueError("RAConv: heads = 1 (all the reference builds); multi-head attention is not built")
        if add_self_loops or dropout:
            raise ValueError("RAConv: add_self_loops = False and dropout = 0, as the reference builds it")
        if kwargs:
            raise ValueError(f"RAConv: unknown arguments {sorted(kwargs)}")
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.negative_slope, self.dropout, self.add_self_loops = negative_slope, dropout, add_self_loops
        self.kernels = bool(kernels)
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_r = self.lin_l
        self.t_lin_l = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.t_lin_r = self.t_lin_l
        self.att_l = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_r = nn.Parameter(torch.empty(1, heads, out_channels))
        self.t_att_l = nn.Parameter(torch.empty(1, heads, out_channels))
        self.t_att_r = nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(heads * out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        for t in (self.lin_l.weight, self.att_l, self.att_r, self.t_lin_l.weight, self.t_att_l, self.t_att_r):
            _glorot(t)
        if self.bias is not None:
            self.bias.data.fill_(0)

    def forward(self, x, edges, node_type, size=None, return_attention_weights=None):
        if return_attention_weights is not None:
            raise ValueError("RAConv: return_attention_weights is not built")
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise ValueError("RAConv: x is one [N, in_channels] tensor")
        C = self.out_channels
        fold = torch.cat([self.t_att_l.view(1, C), self.t_att_r.view(1, C)], 0) @ self.t_lin_l.weight              # [2, in]: W_t^T t_att_l | W_t^T t_att_r
        if self.kernels:
            # ft | pl | pr | two zero columns from ONE GEMM: the row stride C + 4 keeps the 16-byte accesses of the attention kernels
            W = torch.cat([self.lin_l.weight, fold, torch.zeros_like(fold)], 0)
            y = ops.linear(x, W, None)
            ft = y[:, :C]
            sc = torch.stack([ft @ self.att_l.view(C), ft @ self.att_r.view(C), y[:, C], y[:, C + 1]], 1)
            ec = edges.ec if hasattr(edges, "ec") else ops.edge_csr_by_source_type(edges[0], edges[1], node_type, x.shape[0])
            return ops.ra_attention(ft, sc, self.bias, ec, node_type, self.negative_slope)
        ei = edges.edge_index if hasattr(edges, "edge_index") else edges
        ft = x @ self.lin_l.weight.t()
        p = x @ fold.t()
        sc = torch.stack([ft @ self.att_l.view(C), ft @ self.att_r.view(C), p[:, 0], p[:, 1]], 1)
        return ra_attention_tensor(ft, sc, self.bias, ei[0], ei[1], node_type, self.negative_slope)

    def __repr__(self):
        return "{}({}, {}, heads={})".format(self.__class__.__name__, self.in_channels, self.out_channels, self.heads)
