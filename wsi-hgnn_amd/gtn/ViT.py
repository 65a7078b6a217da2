"""The transformer of the GTNMIL baseline (``baselines/GTNMIL/models/ViT.py``): pre-norm blocks over the class token and the pooled
cluster tokens, the class token read at index 0.  Same constructor and ``state_dict`` keys as the reference, so its checkpoints load with
``strict=True``.  The reference's stateful ``relprop`` and its attention hooks are not mirrored: ``forward_saving`` returns what relevance
propagation reads and ``gtn.graphcam`` applies the rules to it."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops

# Whether the blocks' attention runs on the fused kernel (``ops.seq_attention``) by default; measured against torch's own attention at the
# reference's shape (tools/gtn_bench.py, leg 3).
FUSED_ATTENTION_DEFAULT = True


def _linear(x, layer: nn.Linear, kernels: bool):
    if not kernels:
        return F.linear(x, layer.weight, layer.bias)
    return ops.linear(x.reshape(-1, x.shape[-1]), layer.weight, layer.bias).reshape(*x.shape[:-1], layer.weight.shape[0])


def _linear_const(x, layer: nn.Linear, kernels: bool):
    """``_linear`` with the layer's parameters as constants (``forward_saving``: a gradient taken through it forms no weight gradient)."""
    w, b = layer.weight.detach(), None if layer.bias is None else layer.bias.detach()
    if not kernels:
        return F.linear(x, w, b)
    return ops.linear(x.reshape(-1, x.shape[-1]), w, b).reshape(*x.shape[:-1], w.shape[0])


def torch_attention(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """The attention of ``models/ViT.py:183-212`` in tensor operations: qkv [B, n, (qkv h d)] -> [B, n, (h d)]."""
    B, n, W = qkv.shape
    d = W // (3 * heads)
    q, k, v = qkv.reshape(B, n, 3, heads, d).permute(2, 0, 3, 1, 4)
    attn = torch.softmax(torch.einsum("bhid,bhjd->bhij", q, k) * d ** -0.5, -1)
    return torch.einsum("bhij,bhjd->bhid", attn, v).permute(0, 2, 1, 3).reshape(B, n, heads * d)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, drop=0., kernels=True):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)
        self.kernels = bool(kernels)

    def forward(self, x):
        x = _linear(x, self.fc1, self.kernels)
        x = ops.gelu(x) if self.kernels else F.gelu(x)          # the exact (erf) form both ways
        x = self.drop(x)
        x = _linear(x, self.fc2, self.kernels)
        return self.drop(x)


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0., kernels=True, fused_attention=None):
        super().__init__()
        if attn_drop:
            raise NotImplementedError("gtn.Attention: attention dropout is not built (the reference runs attn_drop_rate = 0)")
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.kernels = bool(kernels)
        self.fused_attention = FUSED_ATTENTION_DEFAULT if fused_attention is None else bool(fused_attention)

    def forward(self, x):
        qkv = _linear(x, self.qkv, self.kernels)
        d = qkv.shape[-1] // (3 * self.num_heads)
        if self.kernels and self.fused_attention and ops.seq_attention_supported(x.shape[1], d):
            out = ops.seq_attention(qkv, self.num_heads)
        else:
            out = torch_attention(qkv, self.num_heads)
        return self.proj_drop(_linear(out, self.proj, self.kernels))

    def forward_saving(self, x, kernels: bool):
        """``forward`` in eval mode keeping (qkv, lse [B, h, n] - the row log-sum-exp of scale q k^T -, attn_concat, proj_out)."""
        qkv = _linear_const(x, self.qkv, kernels)
        B, n, W = qkv.shape
        d = W // (3 * self.num_heads)
        if kernels and ops.seq_attention_supported(n, d):
            out, lse = ops.seq_attention_lse(qkv, self.num_heads)
        else:
            q, k, _ = qkv.detach().reshape(B, n, 3, self.num_heads, d).permute(2, 0, 3, 1, 4)
            lse = torch.logsumexp(torch.einsum("bhid,bhjd->bhij", q, k) * d ** -0.5, -1)
            out = torch_attention(qkv, self.num_heads)
        return qkv, lse, out, _linear_const(out, self.proj, kernels)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., kernels=True, fused_attention=None):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop, kernels=kernels,
                              fused_attention=fused_attention)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), drop=drop, kernels=kernels)

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.mlp(self.norm2(x))

    def forward_saving(self, x, kernels: bool):
        """(block output, what relevance propagation reads of this block)."""
        s = {"x_in": x, "norm1_out": self.norm1(x)}
        s["qkv"], s["lse"], s["attn_concat"], s["proj_out"] = self.attn.forward_saving(s["norm1_out"], kernels)
        x = s["x_mid"] = x + s["proj_out"]
        s["norm2_out"] = self.norm2(x)
        h = _linear_const(s["norm2_out"], self.mlp.fc1, kernels)
        s["gelu_out"] = ops.gelu(h) if kernels else F.gelu(h)
        s["mlp_out"] = _linear_const(s["gelu_out"], self.mlp.fc2, kernels)
        return x + s["mlp_out"], s


class VisionTransformer(nn.Module):
    """``forward(x)``: x [B, n, embed_dim] (token 0 = the class token) -> [B, num_classes].  ``kernels=False``: tensor operations throughout;
    ``fused_attention``: the blocks' attention on ``ops.seq_attention`` (None = the measured default, ``FUSED_ATTENTION_DEFAULT``)."""

    def __init__(self, num_classes=2, embed_dim=64, depth=3, num_heads=8, mlp_ratio=2., qkv_bias=False, mlp_head=False, drop_rate=0.,
                 attn_drop_rate=0., kernels=True, fused_attention=None):
        super().__init__()
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.kernels = bool(kernels)
        self.blocks = nn.ModuleList([Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, drop=drop_rate,
                                           attn_drop=attn_drop_rate, kernels=kernels, fused_attention=fused_attention) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim)
        if mlp_head:
            self.head = Mlp(embed_dim, int(embed_dim * mlp_ratio), num_classes, kernels=kernels)
        else:
            self.head = nn.Linear(embed_dim, num_classes)

    def forward(self, x):
        for blk in self.blocks:
            x = blk(x)
        x = self.norm(x)[:, 0]
        return self.head(x) if isinstance(self.head, Mlp) else _linear(x, self.head, self.kernels)

    def forward_saving(self, x, kernels=None):
        """``forward`` without dropout (eval mode) that also returns what relevance propagation reads: (logits, per block a dict of x_in,
        norm1_out, qkv, lse, attn_concat, proj_out, x_mid, norm2_out, gelu_out, mlp_out, and the final normed token 0 [B, embed_dim]).
        Nothing is kept on the module; ``kernels`` = None follows the model.  The Linear parameters enter as constants: a gradient with respect
        to an activation is taken without forming weight gradients."""
        if isinstance(self.head, Mlp):
            raise NotImplementedError("gtn.VisionTransformer.forward_saving: mlp_head=True is not built (the reference's Classifier uses the single Linear head)")
        kernels = self.kernels if kernels is None else bool(kernels)
        saved = []
        for blk in self.blocks:
            x, s = blk.forward_saving(x, kernels)
            saved.append(s)
        x0 = self.norm(x)[:, 0]
        return _linear_const(x0, self.head, kernels), saved, x0
