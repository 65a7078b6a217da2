"""Restatement of GraphCAM for the GTNMIL baseline (baselines/GTNMIL/models/GraphTransformer.py:82-101, ViT.py:217-240, 266-276, 341-386,
layers.py, src/vis_graphcam.py:71-101) in closed forms, plain torch on the CPU, in the dtype of its inputs (float64 is the yardstick, float32
gives the tests their measured e32').  The reference re-runs every layer under ``torch.autograd.grad`` to apply its rules; with alpha = 1
each of them is one of the few dense forms below.  All slides of a batch and all classes go through together: relevance tensors are
[B, C, n, width], the forward's are [B, n, width], and every whole-tensor sum of the Add rule runs per (slide, class) - which is the reference
run one slide and one class at a time.  Also the seeded inputs of the kernel tests.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gtn", "reference_graphcam.npz")
METHODS = ("transformer_attribution", "rollout")


# ------------------------------------------------------------------------------------------------ the rules
def sd(a, b):
    """layers.safe_divide: a / (b + 1e-9) where b != 0 (the denominator 1e-9 where that sum is exactly 0), 0 where b == 0."""
    den = b + 1e-9
    den = torch.where(den == 0, torch.full_like(den, 1e-9), den)
    return a / den * (b != 0).to(a.dtype)


def lin(X, W, R):
    """layers.Linear.relprop at alpha = 1.  X [B, n, in], W [out, in], R [B, C, n, out] -> [B, C, n, in]; the bias plays no part."""
    xp, xn, wp, wn = X.clamp(min=0), X.clamp(max=0), W.clamp(min=0), W.clamp(max=0)
    S = sd(R, (xp @ wp.t() + xn @ wn.t()).unsqueeze(1))
    return xp.unsqueeze(1) * (S @ wp) + xn.unsqueeze(1) * (S @ wn)


def add(A, B, R):
    """layers.Add.relprop: A, B [B, n, E], R [B, C, n, E] -> (a, b); the three sums run over the [n, E] tensor of every (slide, class)."""
    A, B = A.unsqueeze(1), B.unsqueeze(1)
    S = sd(R, A + B)
    a, b = A * S, B * S
    tot = lambda t: t.sum((-1, -2), keepdim=True)
    sa, sb, sr = tot(a), tot(b), tot(R)
    a = a * sd(sd(sa.abs(), sa.abs() + sb.abs()) * sr, sa)
    b = b * sd(sd(sb.abs(), sa.abs() + sb.abs()) * sr, sb)
    return a, b


def clone(X, r1, r2):
    """layers.Clone.relprop: X [B, n, E] with the relevances of its two uses."""
    X = X.unsqueeze(1)
    return X * (sd(r1, X) + sd(r2, X))


def split_heads(t, heads):
    """[..., n, (h d)] -> [..., h, n, d]."""
    return t.reshape(*t.shape[:-1], heads, t.shape[-1] // heads).transpose(-2, -3)


def attention_rule(qkv, attn, R, heads):
    """ViT.Attention.relprop between the two Linear rules.  qkv [B, n, (qkv h d)], attn [B, h, n, n] (the softmax), R [B, C, n, (h d)] ->
    (cam_qkv [B, C, n, (qkv h d)], cam_attn [B, C, h, n, n] - the saved ``attn_cam``)."""
    B, n, W = qkv.shape
    d = W // (3 * heads)
    q, k, v = (t.unsqueeze(1) for t in qkv.reshape(B, n, 3, heads, d).permute(2, 0, 3, 1, 4))       # [B, 1, h, n, d]
    a = attn.unsqueeze(1)
    Rh = split_heads(R, heads)                                                                     # [B, C, h, n, d]
    S2 = sd(Rh, a @ v)
    cam_attn = a * (S2 @ v.transpose(-1, -2)) / 2
    cam_v = v * (a.transpose(-1, -2) @ S2) / 2
    S1 = sd(cam_attn, q @ k.transpose(-1, -2))
    cam_q = q * (S1 @ k) / 2
    cam_k = k * (S1.transpose(-1, -2) @ q) / 2
    cam_qkv = torch.stack([cam_q, cam_k, cam_v], 2)                                                # [B, C, 3, h, n, d]
    return cam_qkv.permute(0, 1, 4, 2, 3, 5).reshape(B, R.shape[1], n, W), cam_attn


def residual(X, r1, r2, A, B):
    """What ``wsi_lrp_residual`` computes: ``add(A, B, clone(X, r1, r2))``, with r2 = None for a tensor that has one use (R = r1)."""
    return add(A, B, r1 if r2 is None else clone(X, r1, r2))


# ------------------------------------------------------------------------------------------------ the transformer
def forward_saving(sdict, x, heads, prefix=""):
    """models/ViT.py::VisionTransformer.forward keeping what the rules read.  Returns (logits, blocks, x0): per block a dict of x_in,
    norm1_out, qkv, attn (the softmax, in the graph), attn_concat, proj_out, x_mid, norm2_out, gelu_out, mlp_out; x0 the final normed token."""
    p = lambda k: sdict[prefix + k]
    depth = 1 + max(int(k[len(prefix):].split(".")[1]) for k in sdict if k.startswith(prefix + "blocks."))
    E = x.shape[-1]
    B, n, _ = x.shape
    d = E // heads
    blocks = []
    for i in range(depth):
        b = f"blocks.{i}."
        s = {"x_in": x}
        s["norm1_out"] = F.layer_norm(x, (E,), p(b + "norm1.weight"), p(b + "norm1.bias"), 1e-6)
        s["qkv"] = F.linear(s["norm1_out"], p(b + "attn.qkv.weight"), sdict.get(prefix + b + "attn.qkv.bias"))
        q, k, v = s["qkv"].reshape(B, n, 3, heads, d).permute(2, 0, 3, 1, 4)
        s["attn"] = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, -1)
        s["attn_concat"] = (s["attn"] @ v).permute(0, 2, 1, 3).reshape(B, n, E)
        s["proj_out"] = F.linear(s["attn_concat"], p(b + "attn.proj.weight"), p(b + "attn.proj.bias"))
        x = s["x_mid"] = x + s["proj_out"]
        s["norm2_out"] = F.layer_norm(x, (E,), p(b + "norm2.weight"), p(b + "norm2.bias"), 1e-6)
        s["gelu_out"] = F.gelu(F.linear(s["norm2_out"], p(b + "mlp.fc1.weight"), p(b + "mlp.fc1.bias")))
        s["mlp_out"] = F.linear(s["gelu_out"], p(b + "mlp.fc2.weight"), p(b + "mlp.fc2.bias"))
        x = x + s["mlp_out"]
        blocks.append(s)
    x0 = F.layer_norm(x, (E,), p("norm.weight"), p("norm.bias"), 1e-5)[:, 0]
    return F.linear(x0, p("head.weight"), p("head.bias")), blocks, x0


def rollout_row(maps, start_layer=0):
    """Row 0 of (I + M_L) ... (I + M_start) without its first column: maps = [M_1 .. M_L], each [B, C, n, n] -> [B, C, n - 1]."""
    r = maps[-1][:, :, 0, :].clone()
    r[:, :, 0] += 1
    for M in reversed(maps[start_layer:-1]):
        r = r + (r.unsqueeze(-2) @ M).squeeze(-2)
    return r[:, :, 1:]


def vit_graphcam(sdict, x, heads, classes=None, method="transformer_attribution", start_layer=0, prefix=""):
    """The GraphCAM procedure of GraphTransformer.py:82-101 over VisionTransformer.relprop(alpha = 1) for the tokens x [B, n, E] (token 0 the
    class token).  Returns a dict: prob [B, n_class], cluster_cam [B, C, n - 1], layer_maps (per block [B, C, n, n]), attn_cam and attn_grad
    (per block [B, C, h, n, n]; attn_grad only for ``transformer_attribution``)."""
    p = lambda k: sdict[prefix + k].detach()
    with torch.enable_grad():
        logits, blocks, x0 = forward_saving({k: v.detach() for k, v in sdict.items()}, x.detach().requires_grad_(True), heads, prefix)
        out = torch.softmax(logits, -1)
        classes = list(range(out.shape[1])) if classes is None else [int(c) for c in classes]
        prob = out.detach()
        grads = None
        if method == "transformer_attribution":
            per_class = [torch.autograd.grad((prob[:, c] * out[:, c]).sum(), [s["attn"] for s in blocks], retain_graph=True) for c in classes]
            grads = [torch.stack([g[l] for g in per_class], 1) for l in range(len(blocks))]        # per block [B, C, h, n, n]
    blocks = [{k: v.detach() for k, v in s.items()} for s in blocks]
    x0 = x0.detach()
    B, n, E = x.shape
    seed = torch.zeros(B, len(classes), 1, out.shape[1], dtype=x.dtype)
    for j, c in enumerate(classes):
        seed[:, j, 0, c] = prob[:, c]
    r = lin(x0.unsqueeze(1), p("head.weight"), seed)                                              # [B, C, 1, E]
    cam = torch.zeros(B, len(classes), n, E, dtype=x.dtype)
    cam[:, :, :1] = x0[:, None, None, :] * sd(r, x0[:, None, None, :])
    attn_cams = [None] * len(blocks)
    for i in reversed(range(len(blocks))):
        s, b = blocks[i], f"blocks.{i}."
        c1, c2 = add(s["x_mid"], s["mlp_out"], cam)
        c2 = lin(s["norm2_out"], p(b + "mlp.fc1.weight"), lin(s["gelu_out"], p(b + "mlp.fc2.weight"), c2))
        cam = clone(s["x_mid"], c1, c2)
        c1, c2 = add(s["x_in"], s["proj_out"], cam)
        c2, attn_cams[i] = attention_rule(s["qkv"], s["attn"], lin(s["attn_concat"], p(b + "attn.proj.weight"), c2), heads)
        c2 = lin(s["norm1_out"], p(b + "attn.qkv.weight"), c2)
        cam = clone(s["x_in"], c1, c2)
    if method == "transformer_attribution":
        maps = [(g * a).clamp(min=0).mean(2) for g, a in zip(grads, attn_cams)]
    elif method == "rollout":
        maps = [a.clamp(min=0).mean(2) for a in attn_cams]
    else:
        raise NotImplementedError(method)
    return dict(prob=prob, cluster_cam=rollout_row(maps, start_layer), layer_maps=maps, attn_cam=attn_cams, attn_grad=grads, input_cam=cam)


def node_maps(pool_logits, sizes, cluster_cam, prob):
    """src/vis_graphcam.py:71-101 for every slide and class, densely: (assign [N, K], node_cam [N, C], node_heat [N, C]).  ``prob`` [G, C] are
    the probabilities of the mapped classes; the reference's clip of p to [0.4, 1] is a drawing choice and is not part of it.  A constant map
    (range 0; the reference gives NaN) is defined as heat 0."""
    assign = torch.softmax(pool_logits, -1)
    cams, heats, off = [], [], 0
    for g, n in enumerate(sizes):
        cam = assign[off:off + n] @ cluster_cam[g].t()                                             # [n, C]
        lo, hi = cam.min(0, keepdim=True).values, cam.max(0, keepdim=True).values
        rng = hi - lo
        norm = torch.where(rng > 0, (cam - lo) / torch.where(rng > 0, rng, torch.ones_like(rng)), torch.zeros_like(cam))
        cams.append(cam)
        heats.append((norm * prob[g]).clamp(0, 1))
        off += n
    return assign, torch.cat(cams), torch.cat(heats)


# ------------------------------------------------------------------------------------------------ the recorded reference
def load_fixture():
    return np.load(GOLDEN)


def fixture_shapes(fix):
    """[(tag, (n, E, depth, heads, classes), seeds)]."""
    return [(str(t), tuple(int(v) for v in fix[f"{t}.config"]), [int(s) for s in fix[f"{t}.seeds"]]) for t in fix["shapes"]]


def fixture_state(fix, tag, dtype=torch.float64, prefix=""):
    return {prefix + k[len(tag) + 4:]: torch.from_numpy(fix[k]).to(dtype) for k in fix.files if k.startswith(f"{tag}.sd.")}


def fixture_inputs(fix, tag, dtype=torch.float64):
    """[S, n, E]: the recorded inputs of all seeds (each was run alone, batch 1)."""
    return torch.from_numpy(fix[f"{tag}.x"]).to(dtype)


def fixture_e32(fix, tag):
    return float(fix[f"{tag}.e32"].max())


# ------------------------------------------------------------------------------------------------ the model cases
# A Classifier with the recorded transformer weights over a small synthetic packed batch.  The batch seed of each shape is fixed so that the case
# is well conditioned, judged by THIS restatement alone: its float32 CPU run on the case's tokens stays within 1 / MODEL_CONDITION of the tests'
# float32 bound max(1e-4, 4 E32), for the cluster maps and every layer map, both methods (tests/test_gtn_graphcam.py checks it), which leaves
# the bound's factor 4 to the code under test.  The chain divides by signed sums, so it is the tokens, not the code, that decide the float32
# error: over the seeds 1822-1899 the restatement's own error ranges from 4e-6 to 3e-3 at the small shape (to 5e-2 at the reference's).  The chosen seeds measure 4e-6 to
# 9e-6 there (two hosts: the figure moves with the host's matrix products) and 5e-4 at the reference's shape, a tenth of the bound and less,
# because a seed of average conditioning (2e-5) does not carry the comparison of two float32 forms: the forms on the device measured up to
# 4 x the CPU figure of the same case, the comparison of the kernels with the tensor-operation form adds two such errors, and that form's
# aggregation on the device (atomic index_add_) moves its own maps between two identical calls (7e-5 of the largest entry at seed 1824).
MODEL_SIZES = (40, 129, 7)
MODEL_IN_FEATS = 24
MODEL_SEED = 1821
MODEL_BATCH_SEED = {"small": 1878, "ref": 1824}
MODEL_CONDITION = 4


def model_state(fix, tag):
    """float32 state dict under gtn.Classifier's keys: seeded GCN / pooling / class-token parameters, the recorded transformer."""
    import gtn_cases
    n, E, depth, heads, classes = dict((t, c) for t, c, _ in fixture_shapes(fix))[tag]
    sdict = gtn_cases.classifier_state(classes, MODEL_IN_FEATS, E, n - 1, depth, heads, MODEL_SEED)
    sdict.update(fixture_state(fix, tag, torch.float32, prefix="transformer."))
    return sdict


def model_batch(tag="small", sizes=MODEL_SIZES, seed=None):
    """(x [N, F], row, col, weight, sizes) of a packed batch (global row numbers); ``seed`` None: the fixed seed of the shape ``tag``."""
    import gtn_cases
    seed = MODEL_BATCH_SEED[tag] if seed is None else seed
    slides = gtn_cases.slides_case(list(sizes), MODEL_IN_FEATS, seed)
    off, rows, cols = 0, [], []
    for x, r, c, _ in slides:
        rows.append(r + off)
        cols.append(c + off)
        off += x.shape[0]
    return torch.cat([s[0] for s in slides]), torch.cat(rows), torch.cat(cols), torch.cat([s[3] for s in slides]), list(sizes)


def field_errors(got_cam, got_maps, ref, slides, classes):
    """{field: largest error over the largest float64 entry, per (slide, class) tensor} of cluster maps and layer maps against ``ref``."""
    worst = lambda a, b: max(float((a[g, c].double() - b[g, c]).abs().max()) / max(float(b[g, c].abs().max()), 1e-300)
                             for g in range(slides) for c in range(classes))
    out = {"cluster_cam": worst(got_cam, ref["cluster_cam"])}
    for l, (m, r) in enumerate(zip(got_maps, ref["layer_maps"])):
        out[f"layer_map_{l}"] = worst(m, r)
    return out


# ------------------------------------------------------------------------------------------------ kernel inputs
LINEAR_WIDTHS = ((64, 192), (64, 64), (64, 128), (128, 64), (64, 3), (64, 16), (32, 96), (4, 1), (256, 256), (36, 21))   # (in, out)
LINEAR_REFUSED = ((260, 64), (64, 260), (30, 64))                              # too wide, or an input width that is no multiple of 4
SEQ_LENGTHS = (1, 2, 63, 64, 65, 101, 128)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def linear_case(G, C, n, fin, fout, seed, signed=False):
    """X [G, n, in], W [out, in], R [G, C, n, out] fp32.  Coherent: X >= 0 and R >= 0, so Z = X W+^T has one sign; planted: a zero X row (a
    zero Z row: relevance 0), an all-negative W column (an input that feeds nothing at X >= 0), and where ``out`` allows an all-negative W
    row (an exactly zero Z column).  ``signed``: X, W normal - denominators cancel."""
    g = _gen(seed)
    W = torch.randn(fout, fin, generator=g) * fin ** -0.5
    if signed:
        X = torch.randn(G, n, fin, generator=g)
        R = torch.randn(G, C, n, fout, generator=g)
    else:
        X = torch.rand(G, n, fin, generator=g) + 0.1
        R = torch.rand(G, C, n, fout, generator=g)
        W[:, fin // 2] = -W[:, fin // 2].abs() - 0.01
        if fout > 1:
            W[fout - 1] = -W[fout - 1].abs() - 0.01
        X[G - 1, n // 2] = 0
    return X, W, R


def residual_case(G, C, n, E, seed, signed=False, single=False):
    """X, A, B [G, n, E], r1, r2 [G, C, n, E] (r2 None with ``single``).  Coherent: B = sign(A) |.|, relevances >= 0, X away from 0;
    planted: A = -B elements (A + B exactly 0), zero X elements.  ``signed``: everything normal."""
    g = _gen(seed)
    A = torch.randn(G, n, E, generator=g)
    X = torch.randn(G, n, E, generator=g)
    if signed:
        B = torch.randn(G, n, E, generator=g)
        r1 = torch.randn(G, C, n, E, generator=g)
        r2 = torch.randn(G, C, n, E, generator=g)
    else:
        A = torch.sign(A) * (A.abs() + 0.1)
        B = torch.sign(A) * (torch.rand(G, n, E, generator=g) + 0.1)
        X = torch.sign(X) * (X.abs() + 0.1)
        r1 = torch.rand(G, C, n, E, generator=g)
        r2 = torch.rand(G, C, n, E, generator=g)
        B[:, n // 2, ::5] = -A[:, n // 2, ::5]
        X[:, 0, ::7] = 0
    return X, r1, (None if single else r2), A, B


def attention_case(G, C, n, H, d, seed, signed=False, rollout=False):
    """qkv [G, n, 3 H d], R [G, C, n, H d], g_out [G, C, n, H d] or None.  Coherent: q, k, v in [0.1, 1.1], R >= 0; planted: a zero v row
    (cam_v of that key 0) and for n > 2 one zero R row.  ``signed``: all normal (attn v and q k^T cancel)."""
    g = _gen(seed)
    if signed:
        qkv = torch.randn(G, n, 3 * H * d, generator=g)
        R = torch.randn(G, C, n, H * d, generator=g)
    else:
        qkv = torch.rand(G, n, 3 * H * d, generator=g) + 0.1
        R = torch.rand(G, C, n, H * d, generator=g)
        qkv[:, n // 2, 2 * H * d:] = 0
        if n > 2:
            R[:, :, 1] = 0
    g_out = None if rollout else torch.randn(G, C, n, H * d, generator=g)
    return qkv, R, g_out


def attention_reference(qkv, R, g_out, heads):
    """(cam_qkv, M [G, C, n, n], lse [G, h, n]) in the dtype of the inputs: the attention rule and the layer map of one block, with
    d attn = g_out v^T per head (g_out None: the rollout map)."""
    B, n, W = qkv.shape
    d = W // (3 * heads)
    q, k, v = qkv.reshape(B, n, 3, heads, d).permute(2, 0, 3, 1, 4)
    dots = q @ k.transpose(-1, -2) * d ** -0.5
    cam_qkv, cam_attn = attention_rule(qkv, torch.softmax(dots, -1), R, heads)
    if g_out is not None:
        cam_attn = (split_heads(g_out, heads) @ v.unsqueeze(1).transpose(-1, -2)) * cam_attn
    return cam_qkv, cam_attn.clamp(min=0).mean(2), torch.logsumexp(dots, -1)


SIGNED_HEADS = 4


def signed_cases():
    """[(entry point, rule, fp32 inputs)]: one signed case per entry point - X, W, A, B, q, k, v and the relevances all normal, so the
    denominators Z, A + B, attn v and q k^T cancel.  The seeds are fixed so that the rule's own float32 CPU error e32' (``rel_err_f32``) is at
    most 1e-2 (tests/test_gtn_graphcam.py checks it); the GPU tests hold the kernels to max(1e-4, 4 e32')."""
    return [("lrp_linear", lin, linear_case(3, 3, 17, 64, 192, seed=SIGNED_SEEDS["lrp_linear"], signed=True)),
            ("lrp_residual", residual, residual_case(3, 3, 17, 64, seed=SIGNED_SEEDS["lrp_residual"], signed=True)),
            ("lrp_attention", lambda qkv, R, g: attention_reference(qkv, R, g, SIGNED_HEADS)[:2],
             attention_case(3, 3, 33, SIGNED_HEADS, 8, seed=SIGNED_SEEDS["lrp_attention"], signed=True))]


SIGNED_SEEDS = {"lrp_linear": 1, "lrp_residual": 1, "lrp_attention": 1}


def rel_err_f32(fn, *inputs):
    """e32' of a rule on given fp32 inputs: its float32 CPU run against its float64 run, in rel_err's norm, the largest over the outputs."""
    cast = lambda dt: [None if t is None else t.to(dt) for t in inputs]
    outs64, outs32 = fn(*cast(torch.float64)), fn(*cast(torch.float32))
    if torch.is_tensor(outs64):
        outs64, outs32 = (outs64,), (outs32,)
    return max(float((a.double() - b).abs().max()) / max(float(b.abs().max()), 1e-30) for a, b in zip(outs32, outs64))
