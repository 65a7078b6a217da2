"""GCNBlock and the mincut pooling of the GTNMIL baseline over the packed batch (``baselines/GTNMIL/models/gcn.py:328-391``,
torch_geometric's ``dense_mincut_pool`` as ``models/GraphTransformer.py:67`` calls it)."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _native as N
from .. import ops
from .batch import GraphBatch

EPS = 1e-15


def _aggregate(z: torch.Tensor, b: GraphBatch) -> torch.Tensor:
    """A z through tensor operations (the ``kernels=False`` path)."""
    msg = z[b.col] if b.weight is None else z[b.col] * b.weight.to(z.dtype).view(-1, 1)
    return torch.zeros_like(z).index_add_(0, b.row, msg)


class GCNBlock(nn.Module):
    """``y = (A x + x) W + b`` -> L2 row normalisation -> BatchNorm1d over the real rows -> dropout -> relu / lrelu, the reference's block.
    Computed as ``z = x W`` first (the MFMA GEMM, 1024 -> 64) and ``A z + z + b`` second (``wsi_spmm_sum`` over 64 columns): algebraically the
    same, and the aggregation moves 16 times fewer bytes.  ``forward(x, adj)``: ``x`` [N, in] packed rows, ``adj`` the batch (``GraphBatch``);
    the reference's ``mask`` has no meaning in the packed layout and is ignored."""

    def __init__(self, input_dim, output_dim, bn=0, add_self=0, normalize_embedding=0, dropout=0.0, relu=0, bias=True, kernels=True):
        super().__init__()
        self.add_self = add_self
        self.dropout = dropout
        self.relu = relu
        self.bn = bn
        self.kernels = bool(kernels)
        if dropout > 0.001:
            self.dropout_layer = nn.Dropout(p=dropout)
        if self.bn:
            self.bn_layer = torch.nn.BatchNorm1d(output_dim)
        self.normalize_embedding = normalize_embedding
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.weight = nn.Parameter(torch.empty(input_dim, output_dim))
        torch.nn.init.xavier_normal_(self.weight)
        self.bias = nn.Parameter(torch.zeros(output_dim)) if bias else None

    def forward(self, x, adj: GraphBatch, mask=None):
        if self.kernels:
            z = ops.linear(x, self.weight.t().contiguous(), None)
            y = ops.graph_conv_aggregate(z, self.bias, adj.ec, False)
            if self.add_self:
                y = y + z
        else:
            z = x @ self.weight
            y = _aggregate(z, adj)
            if self.add_self:
                y = y + z
            if self.bias is not None:
                y = y + self.bias
        if self.normalize_embedding:
            y = F.normalize(y, p=2, dim=-1)
        if self.bn and getattr(adj, "is_slot", False):
            bn = self.bn_layer               # a padded slot: the statistics of the live rows only, dead rows stay 0 and get no gradient
            y = ops.masked_batch_norm(y, adj.live, adj.live_rows, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.training, bn.momentum,
                                      bn.eps, num_batches_tracked=bn.num_batches_tracked, kernels=self.kernels)
        elif self.bn:
            y = self.bn_layer(y)             # the packed rows ARE the rows the reference gathers in front of its bn_layer (gcn.py:361-375)
        if self.dropout > 0.001:
            y = self.dropout_layer(y)
        if self.relu == "relu":
            y = F.relu(y)
        elif self.relu == "lrelu":
            y = F.leaky_relu(y, 0.1)
        return y


def dense_mincut_pool(x, logits, plan: GraphBatch, return_adj=False, kernels=True):
    """torch_geometric's ``dense_mincut_pool(x, adj, s, mask)`` over the packed batch ``plan`` (the mask is the identity there):

        s = softmax(logits, -1);  out = s^T x;  out_adj = s^T A s
        mincut_loss = mean_g( -trace(out_adj) / trace(s^T D s) ),  D = diag(A.sum(-1))
        ss = s^T s;  ortho_loss = mean_g || ss / ||ss||_F - I_K / ||I_K||_F ||_F
        out_adj[:, i, i] = 0;  d = sqrt(out_adj.sum(-1))[:, None] + 1e-15;  out_adj = out_adj / d / d^T

    Returns (out [G, K, D], out_adj [G, K, K] or None, mincut_loss, ortho_loss).  The traces come from ``ops.mincut_assign`` (no [K, K] matrix
    is formed for them), out and ss from one grouped GEMM; ``out_adj`` - which the model discards - is s^T t from the saved t = A s, without a
    gradient.  A slide without entries has trace(s^T D s) = 0 and gives the reference's 0 / 0 = NaN.

    On a ``gtn.GraphSlot`` every cell is a graph of ``cell_rows`` rows: s is zeroed in dead rows (which have no entries, so num and den are
    those of the live rows already), and both losses are means over the cells that hold a slide, with denominators an unused cell cannot make
    0 - neither its value nor its gradient is NaN; a real slide without entries still gives NaN."""
    G, K = plan.num_graphs, logits.shape[1]
    slot = getattr(plan, "is_slot", False)
    if kernels:
        s, num, den, t = ops.mincut_assign_t(logits, plan.ec, plan.rp)
        out, ss = ops.mincut_pool_products(s * plan.live.view(-1, 1) if slot else s, x, plan.rp)
    else:
        s = torch.softmax(logits, -1)
        if slot:
            s = s * plan.live.to(s.dtype).view(-1, 1)
        t = _aggregate(s, plan)
        seg = plan.segment()
        deg = torch.zeros(s.shape[0], dtype=s.dtype, device=s.device).index_add_(
            0, plan.row, torch.ones_like(plan.row, dtype=s.dtype) if plan.weight is None else plan.weight.to(s.dtype))
        zero = torch.zeros(G, dtype=s.dtype, device=s.device)
        num = zero.index_add(0, seg, (s * t).sum(1))
        den = zero.index_add(0, seg, deg * (s * s).sum(1))
        off = [0]
        for c in plan.sizes:
            off.append(off[-1] + c)
        out = torch.stack([s[a:b].t() @ x[a:b] for a, b in zip(off[:-1], off[1:])])
        ss = torch.stack([s[a:b].t() @ s[a:b] for a, b in zip(off[:-1], off[1:])])
    eye = torch.eye(K, dtype=ss.dtype, device=ss.device)
    if slot:
        used, inv = plan.cell_live.to(ss.dtype), plan.inv_cells.to(ss.dtype).reshape(())
        mincut_loss = (used * -(num / (den + (1 - used)))).sum() * inv
        ss = ss + (1 - used).view(-1, 1, 1) * eye
        ortho_loss = (used * torch.norm(ss / torch.norm(ss, dim=(-1, -2), keepdim=True) - eye / torch.norm(eye), dim=(-1, -2))).sum() * inv
    else:
        mincut_loss = torch.mean(-(num / den))
        ortho_loss = torch.mean(torch.norm(ss / torch.norm(ss, dim=(-1, -2), keepdim=True) - eye / torch.norm(eye), dim=(-1, -2)))
    out_adj = None
    if return_adj:
        with torch.no_grad():
            sd, td = s.detach(), t.detach()
            if kernels:
                out_adj = torch.empty((G, K, K), dtype=torch.float32, device=s.device)
                ops.gemm_tn_fp32([dict(A=N.ptr(sd, a * K * 4), lda=K, B=N.ptr(td, a * K * 4), ldb=K, C=N.ptr(out_adj, g * K * K * 4), ldc=K,
                                       M=K, N=K, K=b - a) for g, (a, b) in enumerate(plan.rp.ranges)], s.device)
            else:
                out_adj = torch.stack([sd[a:b].t() @ td[a:b] for a, b in zip(off[:-1], off[1:])])
            ind = torch.arange(K, device=s.device)
            out_adj[:, ind, ind] = 0
            d = torch.sqrt(out_adj.sum(-1))[:, None] + EPS
            out_adj = (out_adj / d) / d.transpose(1, 2)
    return out, out_adj, mincut_loss, ortho_loss
