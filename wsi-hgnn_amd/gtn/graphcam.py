"""GraphCAM of the GTNMIL baseline: the per-class heat map over a slide's patches (``baselines/GTNMIL/models/GraphTransformer.py:82-101``,
``models/ViT.py::relprop``, ``models/layers.py``, ``src/vis_graphcam.py:71-101``), for all slides of a batch and all classes in one pass.

The reference works one slide and one class at a time: a backward, then ``relprop``, which re-runs every layer under ``torch.autograd.grad``
to apply its rule.  At alpha = 1 every rule is a closed form (``sd`` = the reference's ``safe_divide``, x+ / x- = the clamps at 0):

    linear    lin(X, W, R)   = X+ * (S W+) + X- * (S W-),  S = sd(R, X+ W+^T + X- W-^T)                 (no bias)
    add       add(A, B, R)   : S = sd(R, A + B), a = A S, b = B S, then a *= sd(sd(|Sa|, |Sa| + |Sb|) SR, Sa), b alike, with the sums
                               Sa, Sb, SR over the whole [n, E] tensor of one (slide, class)
    clone     clone(X, r, s) = X * (sd(r, X) + sd(s, X))
    attention S2 = sd(R, attn v); cam_attn = attn * (S2 v^T) / 2; cam_v = v * (attn^T S2) / 2;
              S1 = sd(cam_attn, q k^T) (unscaled); cam_q = q * (S1 k) / 2; cam_k = k * (S1^T q) / 2
    LayerNorm, GELU, softmax and dropout pass relevance through.

Per block the layer map is M = mean_h max(d attn * cam_attn, 0) (``rollout``: mean_h max(cam_attn, 0)), and the cluster map is row 0 of
(I + M_L) ... (I + M_start) without its first entry.  d attn comes from ``torch.autograd.grad`` of ``prob[c] * softmax(logits)[c]`` with respect
to every block's attention output (one call per class, batched over the slides, no weight gradients); the attention rule forms
d attn = g_out v^T per head itself.  With ``kernels=True`` the rules run on ``wsi_lrp_linear`` / ``wsi_lrp_residual`` / ``wsi_lrp_attention``
(csrc/relprop.hip); ``kernels=False`` is the same closed forms in tensor operations, without autograd inside the rules.  Nothing is read back
to the host.  The relevance of the transformer's input (the last clone of block 0 and its qkv rule) is not computed: no map reads it.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from .. import ops
from .GraphTransformer import Classifier
from .ViT import VisionTransformer
from .batch import as_batch
from .gcn import dense_mincut_pool

METHODS = ("transformer_attribution", "rollout")
REFERENCE_METHODS = ("full", "grad", "last_layer", "last_layer_attn", "second_layer")


@dataclass
class GraphCAM:
    """``prob`` [G, n_class]: softmax of the logits.  ``classes``: the mapped classes C.  ``cluster_cam`` [G, C, K].  ``assign`` [N, K]: softmax
    of the pool logits, packed rows.  ``node_cam`` [N, C] = assign @ cluster_cam^T per slide, raw.  ``node_heat`` [N, C]: node_cam min-max
    normalised per (slide, class), times prob[c], clipped to [0, 1]; a map that is constant over a slide (range exactly 0, where the
    reference divides 0 by 0) is defined as 0.  ``pool_logits`` [N, K], ``tokens`` [G, K + 1, E] (the transformer's input) and ``sizes`` are
    kept for the file writer and the tests.  ``layer_maps``: per block [G, C, K + 1, K + 1], only with ``keep_layer_maps=True``."""
    prob: torch.Tensor
    classes: List[int]
    cluster_cam: torch.Tensor
    assign: torch.Tensor
    node_cam: torch.Tensor
    node_heat: torch.Tensor
    pool_logits: torch.Tensor
    tokens: torch.Tensor
    sizes: List[int]
    layer_maps: Optional[List[torch.Tensor]] = None


# ------------------------------------------------------------------------------------------------ the rules in tensor operations
def sd(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``safe_divide`` of models/layers.py: a / (b + 1e-9), the denominator 1e-9 where that sum is exactly 0, and 0 wherever b == 0."""
    den = b + 1e-9
    den = torch.where(den == 0, torch.full_like(den, 1e-9), den)
    return a / den * (b != 0).to(a.dtype)


def _lin(X, W, R):
    xp, xn, wp, wn = X.clamp(min=0), X.clamp(max=0), W.clamp(min=0), W.clamp(max=0)
    S = sd(R, (xp @ wp.t() + xn @ wn.t()).unsqueeze(1))
    return xp.unsqueeze(1) * (S @ wp) + xn.unsqueeze(1) * (S @ wn)


def _residual(X, r1, r2, A, B):
    """add(A, B, clone(X, r1, r2)); r2 None: add(A, B, r1)."""
    if r2 is not None:
        X = X.unsqueeze(1)
        r1 = X * (sd(r1, X) + sd(r2, X))
    A, B = A.unsqueeze(1), B.unsqueeze(1)
    S = sd(r1, A + B)
    a, b = A * S, B * S
    tot = lambda t: t.sum((-1, -2), keepdim=True)
    sa, sb, sr = tot(a), tot(b), tot(r1)
    return a * sd(sd(sa.abs(), sa.abs() + sb.abs()) * sr, sa), b * sd(sd(sb.abs(), sa.abs() + sb.abs()) * sr, sb)


def _attention(qkv, lse, R, g_out, heads: int):
    """(cam_qkv [G, C, n, 3 H d], M [G, C, n, n]); the probabilities are recomputed from lse as the kernels do."""
    G, n, W = qkv.shape
    C, d = R.shape[1], W // (3 * heads)
    q, k, v = (t.unsqueeze(1) for t in qkv.reshape(G, n, 3, heads, d).permute(2, 0, 3, 1, 4))       # [G, 1, h, n, d]
    z1 = q @ k.transpose(-1, -2)
    attn = torch.exp(z1 * d ** -0.5 - lse.unsqueeze(1).unsqueeze(-1))
    heads_of = lambda t: t.reshape(G, C, n, heads, d).transpose(2, 3)                              # [G, C, h, n, d]
    S2 = sd(heads_of(R), attn @ v)
    vt = v.transpose(-1, -2)
    cam_attn = attn * (S2 @ vt) / 2
    cam_v = v * (attn.transpose(-1, -2) @ S2) / 2
    S1 = sd(cam_attn, z1)
    cam_q = q * (S1 @ k) / 2
    cam_k = k * (S1.transpose(-1, -2) @ q) / 2
    cam_qkv = torch.stack([cam_q, cam_k, cam_v], 2).permute(0, 1, 4, 2, 3, 5).reshape(G, C, n, W)
    if g_out is not None:
        cam_attn = (heads_of(g_out) @ vt) * cam_attn
    return cam_qkv, cam_attn.clamp(min=0).mean(2)


def _rollout_row(maps: Sequence[torch.Tensor], start_layer: int) -> torch.Tensor:
    """Row 0 of (I + M_L) ... (I + M_start), first entry dropped: L - start - 1 batched vector-matrix products."""
    r = maps[-1][:, :, 0, :].clone()
    r[:, :, 0] += 1
    for M in reversed(maps[start_layer:-1]):
        r = r + torch.matmul(r.unsqueeze(-2), M).squeeze(-2)
    return r[:, :, 1:]


def kernels_cover(transformer: VisionTransformer, n: int) -> bool:
    """Whether ``wsi_lrp_*`` cover this model at n tokens (otherwise the tensor-operation form runs)."""
    E, heads = transformer.embed_dim, transformer.blocks[0].attn.num_heads
    widths = [(E, transformer.head.weight.shape[0])]
    for blk in transformer.blocks:
        widths += [tuple(reversed(l.weight.shape)) for l in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2)]
    return (E % heads == 0 and ops.seq_attention_supported(n, E // heads) and ops.lrp_residual_supported(E)
            and all(ops.lrp_linear_supported(i, o) for i, o in widths))


# ------------------------------------------------------------------------------------------------ the transformer's maps
def token_maps(transformer: VisionTransformer, tokens: torch.Tensor, classes=None, method: str = "transformer_attribution",
               start_layer: int = 0, kernels: Optional[bool] = None, keep_layer_maps: bool = False, alpha: float = 1.0):
    """(prob [G, n_class], cluster_cam [G, C, n - 1], layer maps or None) of ``VisionTransformer.relprop`` for ``tokens`` [G, n, E] (token 0 the
    class token), all slides and classes together.  The transformer should be in eval mode (dropout is not applied)."""
    if method in REFERENCE_METHODS:
        raise NotImplementedError(f"gtn.graphcam: method {method!r} of the reference is not built (built: {', '.join(METHODS)})")
    if method not in METHODS:
        raise ValueError(f"gtn.graphcam: unknown method {method!r}")
    if alpha != 1:
        raise NotImplementedError("gtn.graphcam: alpha != 1 is not built (the reference runs alpha = 1)")
    if not isinstance(transformer.head, torch.nn.Linear):
        raise NotImplementedError("gtn.graphcam: mlp_head=True is not built (the reference's Classifier uses the single Linear head)")
    depth = len(transformer.blocks)
    if not 0 <= int(start_layer) < depth:
        raise ValueError(f"gtn.graphcam: start_layer {start_layer} of {depth} blocks")
    heads = transformer.blocks[0].attn.num_heads
    kernels = transformer.kernels if kernels is None else bool(kernels)
    native = kernels and kernels_cover(transformer, tokens.shape[1])
    n_class = transformer.head.weight.shape[0]
    classes = list(range(n_class)) if classes is None else [int(c) for c in classes]
    if not classes or any(not 0 <= c < n_class for c in classes):
        raise ValueError(f"gtn.graphcam: classes {classes} of {n_class}")
    G, n, E = tokens.shape
    C = len(classes)
    with torch.enable_grad():
        x = tokens.detach().requires_grad_(True)           # (as in the reference: the attention outputs then carry a gradient whatever the weights do)
        logits, saved, x0 = transformer.forward_saving(x, kernels)
        out = torch.softmax(logits, -1)
        prob = out.detach()
        g_outs = [None] * depth
        if method == "transformer_attribution":
            concat = [s["attn_concat"] for s in saved]
            per_class = [torch.autograd.grad((prob[:, c] * out[:, c]).sum(), concat, retain_graph=j + 1 < C) for j, c in enumerate(classes)]
            g_outs = [torch.stack([g[l] for g in per_class], 1) for l in range(depth)]                # per block [G, C, n, E]
    with torch.no_grad():
        saved = [{k: v.detach() for k, v in s.items()} for s in saved]
        x0 = x0.detach()
        lin = ops.lrp_linear if native else _lin
        residual = ops.lrp_residual if native else _residual
        attention = ops.lrp_attention if native else _attention
        seed = torch.zeros((G, C, 1, n_class), dtype=tokens.dtype, device=tokens.device)
        for j, c in enumerate(classes):                    # the class seed p * e_c stays on the device (and no index tensor is copied to it)
            seed[:, j, 0, c] = prob[:, c]
        r = lin(x0.unsqueeze(1), transformer.head.weight.detach(), seed)                               # [G, C, 1, E]
        cam = torch.zeros((G, C, n, E), dtype=tokens.dtype, device=tokens.device)
        cam[:, :, :1] = x0[:, None, None, :] * sd(r, x0[:, None, None, :])
        c1, c2, above = cam, None, None
        maps: List[Optional[torch.Tensor]] = [None] * depth
        for i in reversed(range(depth)):
            s, blk = saved[i], transformer.blocks[i]
            c1, c2 = residual(above, c1, c2, s["x_mid"], s["mlp_out"])            # the clone that closes the block above, then this block's add2
            c2 = lin(s["norm2_out"], blk.mlp.fc1.weight.detach(), lin(s["gelu_out"], blk.mlp.fc2.weight.detach(), c2))
            c1, c2 = residual(s["x_mid"], c1, c2, s["x_in"], s["proj_out"])       # clone2, add1
            c2, maps[i] = attention(s["qkv"], s["lse"], lin(s["attn_concat"], blk.attn.proj.weight.detach(), c2), g_outs[i], heads)
            if i == start_layer:
                break                                                              # (no map reads the relevance below this block's attention)
            c2 = lin(s["norm1_out"], blk.attn.qkv.weight.detach(), c2)
            above = s["x_in"]
        cluster_cam = _rollout_row(maps, start_layer)
    return prob, cluster_cam, (maps if keep_layer_maps else None)


def _node_maps(assign: torch.Tensor, b, cluster_cam: torch.Tensor, prob: torch.Tensor, kernels: bool):
    """node_cam [N, C] and node_heat [N, C] over the packed rows (src/vis_graphcam.py:71-101 for every slide and class)."""
    seg = b.segment()
    node_cam = torch.einsum("nk,nck->nc", assign, cluster_cam[seg])
    G, C = prob.shape[0], cluster_cam.shape[1]
    if kernels:
        lo, hi = -ops.segment_reduce(-node_cam, b.rp, "max"), ops.segment_reduce(node_cam, b.rp, "max")
    else:
        idx = seg.view(-1, 1).expand(-1, C)
        lo = torch.full((G, C), float("inf"), dtype=node_cam.dtype, device=node_cam.device).scatter_reduce(0, idx, node_cam, "amin")
        hi = torch.full((G, C), float("-inf"), dtype=node_cam.dtype, device=node_cam.device).scatter_reduce(0, idx, node_cam, "amax")
    rng = hi - lo
    flat = rng > 0
    norm = (node_cam - lo[seg]) / torch.where(flat, rng, torch.ones_like(rng))[seg]
    heat = (torch.where(flat[seg], norm, torch.zeros_like(norm)) * prob[seg]).clamp(0, 1)
    return node_cam, heat


def class_maps(model: Classifier, batch, classes=None, method: str = "transformer_attribution", start_layer: int = 0,
               kernels: Optional[bool] = None, keep_layer_maps: bool = False, alpha: float = 1.0) -> GraphCAM:
    """GraphCAM of every slide of ``batch`` (anything ``as_batch`` takes) for ``classes`` (None: all ``n_class``) in one pass.  The model is
    put in eval mode for the call and restored afterwards; its parameters, buffers and gradients are not touched.  ``kernels`` None follows
    ``model.kernels``; shapes the relevance kernels do not cover run the tensor-operation form.  Methods: ``transformer_attribution`` (the
    reference's GraphCAM) and ``rollout``; the reference's other methods, ``alpha != 1`` and ``mlp_head=True`` raise NotImplementedError.
    ``node_heat`` of a slide whose map is constant (min == max, where the reference computes 0 / 0 = NaN) is 0."""
    if method in REFERENCE_METHODS:
        raise NotImplementedError(f"gtn.graphcam: method {method!r} of the reference is not built (built: {', '.join(METHODS)})")
    kernels = model.kernels if kernels is None else bool(kernels)
    b = as_batch(batch)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            dtype = model.pool1.weight.dtype
            X = _conv_as(model, b, kernels, dtype)
            w, bias = model.pool1.weight, model.pool1.bias
            s = ops.linear(X, w, bias) if kernels else torch.nn.functional.linear(X, w, bias)
            pooled = dense_mincut_pool(X, s, b, kernels=kernels)[0]
            tokens = torch.cat([model.cls_token.repeat(pooled.shape[0], 1, 1), pooled], dim=1)
        prob, cluster_cam, maps = token_maps(model.transformer, tokens, classes, method, start_layer, kernels, keep_layer_maps, alpha)
        with torch.no_grad():
            assign = torch.softmax(s, -1)
            cidx = [int(c) for c in classes] if classes is not None else list(range(prob.shape[1]))
            node_cam, node_heat = _node_maps(assign, b, cluster_cam, torch.stack([prob[:, c] for c in cidx], 1), kernels)
    finally:
        model.train(was_training)
    return GraphCAM(prob=prob, classes=cidx, cluster_cam=cluster_cam, assign=assign, node_cam=node_cam, node_heat=node_heat,
                    pool_logits=s, tokens=tokens, sizes=list(b.sizes), layer_maps=maps)


def _conv_as(model: Classifier, b, kernels: bool, dtype):
    """conv1 under the call's setting of ``kernels`` (the tensor-operation form in the dtype of the parameters)."""
    conv = model.conv1
    keep, conv.kernels = conv.kernels, kernels
    try:
        return conv(b.x if kernels else b.x.to(dtype), b)
    finally:
        conv.kernels = keep


def save_reference_files(result: GraphCAM, graph_index: int, directory: str) -> None:
    """The files ``src/vis_graphcam.py`` loads for one slide, as the reference's ``graphcam_flag`` branch writes them: ``s_matrix.pt`` (argmax
    of the assignment), ``s_matrix_ori.pt`` (the slide's pool logits [n, K]), ``prob.pt`` ([1, n_class]: the reference applies softmax to the
    probabilities once more, GraphTransformer.py:84 - mirrored here and only here) and ``cam_{c}.pt`` [1, K] for every mapped class c."""
    g = int(graph_index)
    if not 0 <= g < len(result.sizes):
        raise IndexError(f"save_reference_files: slide {g} of {len(result.sizes)}")
    os.makedirs(directory, exist_ok=True)
    a = sum(result.sizes[:g])
    logits = result.pool_logits[a:a + result.sizes[g]].detach().cpu()
    torch.save(torch.argmax(logits, dim=1), os.path.join(directory, "s_matrix.pt"))
    torch.save(logits, os.path.join(directory, "s_matrix_ori.pt"))
    torch.save(torch.softmax(result.prob[g:g + 1].detach().cpu(), -1), os.path.join(directory, "prob.pt"))
    for j, c in enumerate(result.classes):
        torch.save(result.cluster_cam[g:g + 1, j].detach().cpu(), os.path.join(directory, f"cam_{c}.pt"))
