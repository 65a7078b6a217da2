"""Float64 restatements of the GTNMIL baseline (baselines/GTNMIL/models/GraphTransformer.py, gcn.py, ViT.py and torch_geometric's
dense_mincut_pool) that the gtn tests compare against.  Plain torch on the CPU, differentiable through autograd; parameters come as a dict
under the reference's state_dict keys.  Two forms of the classifier: ``dense=True`` follows the reference line by line over padded tensors
(dense adjacency, mask, (A x + x) W + b, the rows gathered in front of the BatchNorm), ``dense=False`` is the packed form the package computes.
"""
import math

import torch
import torch.nn.functional as F

EPS = 1e-15


# ------------------------------------------------------------------------------------------------ transformer
def attention_ref(qkv, heads):
    """(out [B, n, (h d)], lse [B, h, n]) of models/ViT.py:183-212 from qkv [B, n, (qkv h d)]."""
    B, n, W = qkv.shape
    d = W // (3 * heads)
    q, k, v = qkv.reshape(B, n, 3, heads, d).permute(2, 0, 3, 1, 4)
    dots = torch.einsum("bhid,bhjd->bhij", q, k) * d ** -0.5
    out = torch.einsum("bhij,bhjd->bhid", torch.softmax(dots, -1), v)
    return out.permute(0, 2, 1, 3).reshape(B, n, heads * d), torch.logsumexp(dots, -1)


def vit_forward(sd, x, heads, prefix=""):
    """Logits [B, classes] of models/ViT.py::VisionTransformer.forward (single-Linear head) with the parameters ``sd[prefix + key]``."""
    p = lambda k: sd[prefix + k]
    depth = 1 + max(int(k[len(prefix):].split(".")[1]) for k in sd if k.startswith(prefix + "blocks."))
    E = x.shape[-1]
    for i in range(depth):
        b = f"blocks.{i}."
        h = F.layer_norm(x, (E,), p(b + "norm1.weight"), p(b + "norm1.bias"), 1e-6)
        qkv = F.linear(h, p(b + "attn.qkv.weight"), sd.get(prefix + b + "attn.qkv.bias"))
        x = x + F.linear(attention_ref(qkv, heads)[0], p(b + "attn.proj.weight"), p(b + "attn.proj.bias"))
        h = F.layer_norm(x, (E,), p(b + "norm2.weight"), p(b + "norm2.bias"), 1e-6)
        h = F.gelu(F.linear(h, p(b + "mlp.fc1.weight"), p(b + "mlp.fc1.bias")))
        x = x + F.linear(h, p(b + "mlp.fc2.weight"), p(b + "mlp.fc2.bias"))
    x = F.layer_norm(x, (E,), p("norm.weight"), p("norm.bias"), 1e-5)[:, 0]
    return F.linear(x, p("head.weight"), p("head.bias"))


# ------------------------------------------------------------------------------------------------ mincut pooling
def mincut_dense(x, adj, logits, mask):
    """torch_geometric.nn.dense_mincut_pool(x, adj, s, mask): (out, out_adj, mincut_loss, ortho_loss) over padded [B, N, .] tensors."""
    s = torch.softmax(logits, -1)
    m = mask.unsqueeze(-1).to(x.dtype)
    x, s = x * m, s * m
    K = s.shape[-1]
    out = s.transpose(1, 2) @ x
    out_adj = s.transpose(1, 2) @ adj @ s
    num = torch.einsum("bii->b", out_adj)
    den = torch.einsum("bii->b", s.transpose(1, 2) @ torch.diag_embed(adj.sum(-1)) @ s)
    mincut_loss = torch.mean(-(num / den))
    ss = s.transpose(1, 2) @ s
    eye = torch.eye(K, dtype=s.dtype)
    ortho_loss = torch.mean(torch.norm(ss / torch.norm(ss, dim=(-1, -2), keepdim=True) - eye / torch.norm(eye), dim=(-1, -2)))
    ind = torch.arange(K)
    out_adj = out_adj.clone()
    out_adj[:, ind, ind] = 0
    d = torch.sqrt(out_adj.sum(-1))[:, None] + EPS
    out_adj = (out_adj / d) / d.transpose(1, 2)
    return out, out_adj, mincut_loss, ortho_loss


def mincut_sparse(z, row, col, w, sizes):
    """(s, t, num [G], den [G]) of ops.mincut_assign from packed logits z [N, K] and the entries A[row, col] += w."""
    s = torch.softmax(z, -1)
    wv = torch.ones(row.shape[0], dtype=z.dtype) if w is None else w.to(z.dtype)
    t = torch.zeros_like(s).index_add(0, row, s[col] * wv.view(-1, 1))
    deg = torch.zeros(z.shape[0], dtype=z.dtype).index_add(0, row, wv)
    seg = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    zero = torch.zeros(len(sizes), dtype=z.dtype)
    return s, t, zero.index_add(0, seg, (s * t).sum(1)), zero.index_add(0, seg, deg * (s * s).sum(1))


def dense_adjacency(n, row, col, w, dtype=torch.float64):
    a = torch.zeros(n, n, dtype=dtype)
    a.index_put_((row, col), torch.ones(row.shape[0], dtype=dtype) if w is None else w.to(dtype), accumulate=True)
    return a


# ------------------------------------------------------------------------------------------------ the classifier
def _batch_norm(y, sd, train):
    """BatchNorm1d over the rows of y; returns (normalised, batch mean, unbiased batch variance) - the latter two None in eval mode."""
    g, b = sd["conv1.bn_layer.weight"], sd["conv1.bn_layer.bias"]
    if not train:
        return (y - sd["conv1.bn_layer.running_mean"]) / torch.sqrt(sd["conv1.bn_layer.running_var"] + 1e-5) * g + b, None, None
    mean, var = y.mean(0), y.var(0, unbiased=False)
    return (y - mean) / torch.sqrt(var + 1e-5) * g + b, mean.detach(), y.var(0, unbiased=True).detach() if y.shape[0] > 1 else None


def classifier_forward(sd, slides, labels, heads, train=True, dense=False):
    """Classifier.forward of models/GraphTransformer.py:33-80.  ``slides``: a list of (x [n, F], row, col, w or None) with local indices;
    ``sd``: float64 tensors under the state_dict keys.  Returns a dict: loss, logits, probs, mincut, ortho, bn_mean, bn_var (unbiased)."""
    sizes = [s[0].shape[0] for s in slides]
    W, bias = sd["conv1.weight"], sd["conv1.bias"]
    if dense:
        B, nmax = len(slides), max(sizes)
        x = torch.zeros(B, nmax, slides[0][0].shape[1], dtype=torch.float64)
        adj = torch.zeros(B, nmax, nmax, dtype=torch.float64)
        mask = torch.zeros(B, nmax, dtype=torch.float64)
        for b, (xb, row, col, w) in enumerate(slides):
            n = xb.shape[0]
            x[b, :n], adj[b, :n, :n], mask[b, :n] = xb, dense_adjacency(n, row, col, w), 1.0
        X = mask.unsqueeze(2) * x
        y = (adj @ X + X) @ W + bias
        y = F.normalize(y, p=2, dim=2)
        packed, mean, var = _batch_norm(torch.cat([y[b, :n] for b, n in enumerate(sizes)], 0), sd, train)
        y = torch.zeros_like(y)
        off = 0
        for b, n in enumerate(sizes):
            y[b, :n] = packed[off:off + n]
            off += n
        s = F.linear(y, sd["pool1.weight"], sd["pool1.bias"])
        pooled, _, mc, ortho = mincut_dense(y, adj, s, mask)
    else:
        off = [0]
        for n in sizes:
            off.append(off[-1] + n)
        x = torch.cat([s[0] for s in slides], 0).to(torch.float64)
        row = torch.cat([s[1] + o for s, o in zip(slides, off)])
        col = torch.cat([s[2] + o for s, o in zip(slides, off)])
        w = None if slides[0][3] is None else torch.cat([s[3] for s in slides]).to(torch.float64)
        z = x @ W
        wv = torch.ones(row.shape[0], dtype=torch.float64) if w is None else w
        y = torch.zeros_like(z).index_add(0, row, z[col] * wv.view(-1, 1)) + z + bias
        y = F.normalize(y, p=2, dim=1)
        y, mean, var = _batch_norm(y, sd, train)
        logits = F.linear(y, sd["pool1.weight"], sd["pool1.bias"])
        s, t, num, den = mincut_sparse(logits, row, col, w, sizes)
        mc = torch.mean(-(num / den))
        K = s.shape[1]
        pooled = torch.stack([s[a:b].t() @ y[a:b] for a, b in zip(off[:-1], off[1:])])
        ss = torch.stack([s[a:b].t() @ s[a:b] for a, b in zip(off[:-1], off[1:])])
        eye = torch.eye(K, dtype=torch.float64)
        ortho = torch.mean(torch.norm(ss / torch.norm(ss, dim=(-1, -2), keepdim=True) - eye / math.sqrt(K), dim=(-1, -2)))
    tokens = torch.cat([sd["cls_token"].repeat(len(slides), 1, 1), pooled], 1)
    out = vit_forward(sd, tokens, heads, prefix="transformer.")
    loss = F.cross_entropy(out, labels) + mc + ortho
    return dict(loss=loss, logits=out, probs=torch.softmax(out, -1), mincut=mc, ortho=ortho, bn_mean=mean, bn_var=var)


# ------------------------------------------------------------------------------------------------ seeded inputs
# graphs of the kernel tests: a single row, the default chunk of 128 rows from both sides, a multi-chunk graph and a short last one
KERNEL_SIZES = (1, 127, 128, 129, 293, 2)
KERNEL_KS = (1, 2, 64, 100, 128)


def kernel_edges(sizes=KERNEL_SIZES, seed=1720):
    """(row, col, w) with global row numbers: a seeded, weighted, non-symmetric list of entries, block-diagonal over the graphs.  It holds self
    loops, repeated (row, col) entries, rows without entries (every row r with r % 7 == 5 of a graph of more than two rows), and in the
    293-row graph one row with 300 entries (local row 11: a long CSR row) and one column with 300 (local column 200: a long CSC row).
    Every graph has an entry; the 1-row graph has its self loop."""
    gen = torch.Generator().manual_seed(seed)
    rows, cols, off = [], [], 0
    for n in sizes:
        if n == 1:
            r, c = torch.tensor([0]), torch.tensor([0])
        else:
            r = torch.randint(0, n, (3 * n,), generator=gen)
            c = torch.randint(0, n, (3 * n,), generator=gen)
            loops = torch.arange(0, n, 4)
            r, c = torch.cat([r, loops, torch.tensor([0])]), torch.cat([c, loops, torch.tensor([1])])
            r, c = torch.cat([r, r[:20]]), torch.cat([c, c[:20]])                      # repeated entries
            if n == 293:
                into = torch.randint(0, n, (300,), generator=gen)
                into = torch.where(into % 7 == 5, into - 1, into)                      # (none of the 300 falls on a row that is emptied below)
                r = torch.cat([r, torch.full((300,), 11), into])
                c = torch.cat([c, torch.randint(0, n, (300,), generator=gen), torch.full((300,), 200)])
            if n > 2:
                keep = r % 7 != 5
                r, c = r[keep], c[keep]
        rows.append(r + off)
        cols.append(c + off)
        off += n
    row, col = torch.cat(rows), torch.cat(cols)
    perm = torch.randperm(row.shape[0], generator=gen)                                 # (the list is in no particular order)
    w = 0.25 + torch.rand(row.shape[0], generator=gen, dtype=torch.float32)
    return row[perm], col[perm], w


def slides_case(sizes, feats, seed, weighted=True, neighbours=4):
    """Seeded slides: x [n, feats] fp32, ``neighbours`` entries per row at random columns plus a self loop each (every slide has an entry),
    positive fp32 weights or None.  Local indices."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        x = torch.randn(n, feats, generator=gen, dtype=torch.float32)
        row = torch.cat([torch.arange(n).repeat_interleave(neighbours), torch.arange(n)])
        col = torch.cat([torch.randint(0, n, (n * neighbours,), generator=gen), torch.arange(n)])
        w = (0.25 + torch.rand(row.shape[0], generator=gen, dtype=torch.float32)) if weighted else None
        out.append((x, row, col, w))
    return out


def classifier_state(n_class, in_feats, embed_dim, clusters, depth, heads, seed, mlp_ratio=2.0):
    """A seeded float32 state dict under gtn.Classifier's keys (values away from the initial ones, so that every term matters)."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape, scale=1.0: torch.randn(*shape, generator=gen, dtype=torch.float32) * scale
    E, Hd = embed_dim, int(embed_dim * mlp_ratio)
    sd = {"cls_token": r(1, 1, E, scale=0.5), "conv1.weight": r(in_feats, E, scale=in_feats ** -0.5), "conv1.bias": r(E, scale=0.1),
          "conv1.bn_layer.weight": 1 + r(E, scale=0.1), "conv1.bn_layer.bias": r(E, scale=0.1),
          "conv1.bn_layer.running_mean": r(E, scale=0.05), "conv1.bn_layer.running_var": 0.5 + torch.rand(E, generator=gen) * 0.5,
          "conv1.bn_layer.num_batches_tracked": torch.tensor(0, dtype=torch.int64),
          "pool1.weight": r(clusters, E, scale=2 * E ** -0.5), "pool1.bias": r(clusters, scale=0.1)}
    t = "transformer."
    for i in range(depth):
        b = f"{t}blocks.{i}."
        sd.update({b + "norm1.weight": 1 + r(E, scale=0.1), b + "norm1.bias": r(E, scale=0.1), b + "attn.qkv.weight": r(3 * E, E, scale=2 * E ** -0.5),
                   b + "attn.proj.weight": r(E, E, scale=E ** -0.5), b + "attn.proj.bias": r(E, scale=0.1),
                   b + "norm2.weight": 1 + r(E, scale=0.1), b + "norm2.bias": r(E, scale=0.1),
                   b + "mlp.fc1.weight": r(Hd, E, scale=E ** -0.5), b + "mlp.fc1.bias": r(Hd, scale=0.1),
                   b + "mlp.fc2.weight": r(E, Hd, scale=Hd ** -0.5), b + "mlp.fc2.bias": r(E, scale=0.1)})
    sd.update({t + "norm.weight": 1 + r(E, scale=0.1), t + "norm.bias": r(E, scale=0.1), t + "head.weight": r(n_class, E, scale=E ** -0.5),
               t + "head.bias": r(n_class, scale=0.1)})
    return sd


def as_float64_leaves(sd):
    """float64 copies that require a gradient (buffers: plain copies)."""
    out = {}
    for k, v in sd.items():
        if v.dtype.is_floating_point and "running_" not in k:
            out[k] = v.detach().to(torch.float64).requires_grad_(True)
        else:
            out[k] = v.detach().to(torch.float64) if v.dtype.is_floating_point else v.clone()
    return out
