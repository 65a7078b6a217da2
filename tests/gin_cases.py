"""What the GIN tests share (no test functions): the kernels' dispatch rule restated, the width table that reaches every instantiation, the
graph builders, float64 restatements of the aggregation - as plain loops (forward, ``arg`` with the first-position rule, every gradient) and
as closed-form tensor expressions that can replay a given ``arg`` - and a float64 restatement of the whole model, train-mode BatchNorm with
its running statistics included."""
import torch

from row_group_cases import row_cfg

TOL = 1e-4                         # the project's norm: of the largest float64 entry of each tensor
N_SINKS = 24                       # nodes without an out-edge
N_EMPTY = 8                        # nodes without an in-edge
MODES = ("sum", "mean", "max")


# ---------------------------------------------------------------------------------------------------- dispatch rule (csrc/row_group.h)
def gin_cfg(D, aligned):
    """(VEC, G, NK) of a row width."""
    return row_cfg(D, D, 1, aligned)


# the instantiations csrc/gin.hip holds: the narrow cases of csrc/row_group.h (ROW_GROUP_DISPATCH_NARROW)
GIN_INSTANCES = [(4, 4, 1), (4, 8, 1), (4, 16, 1), (4, 32, 1), (4, 64, 1), (4, 64, 2), (4, 64, 4),
                 (1, 4, 1), (1, 8, 1), (1, 16, 1), (1, 32, 1), (1, 64, 1), (1, 64, 2), (1, 64, 4), (1, 64, 8), (1, 64, 16)]
# widths that reach each of them through ops (contiguous, allocator-aligned tensors: VEC = 4 exactly when D % 4 == 0)
GIN_SWEEP = [1, 3, 4, 7, 12, 13, 29, 32, 40, 50, 100, 101, 200, 250, 509, 512, 1023, 1024]


# ---------------------------------------------------------------------------------------------------- graphs
def nodes_for(G):
    return 128 * (256 // G) + 37


def sweep_edges(G):
    """(n, src, dst) of the graph of group size G: nodes [0, 8) without in-edges, node 8 in-degree 1 (a self loop), nodes 9..22 in-degrees
    2..15, node 23 in-degree 17, node 24 in-degree 150, the others 0..5 random in-edges plus a self loop on every third; a tenth of the random
    edges twice; the last 24 nodes feed nobody; edge order shuffled."""
    gen = torch.Generator().manual_seed(300 + G)
    n = nodes_for(G)
    R = n - N_SINKS
    src, dst = [torch.tensor([8])], [torch.tensor([8])]

    def feed(v, k):
        src.append(torch.randint(0, R, (k,), generator=gen))
        dst.append(torch.full((k,), v))

    for i in range(14):
        feed(9 + i, 2 + i)
    feed(23, 17)
    feed(24, 150)
    cnt = torch.randint(0, 6, (n - 25,), generator=gen)
    d = torch.repeat_interleave(torch.arange(25, n), cnt)
    s = torch.randint(0, R, (d.numel(),), generator=gen)
    m = d.numel() // 10
    loops = torch.arange(25, R, 3)
    src += [s, s[:m], loops]
    dst += [d, d[:m], loops]
    src, dst = torch.cat(src), torch.cat(dst)
    o = torch.randperm(src.numel(), generator=gen)
    return n, src[o], dst[o]


def check_sweep_graph(G, csr):
    n = nodes_for(G)
    rowptr, s = csr["rowptr"], csr["src"]
    indeg = rowptr[1:] - rowptr[:-1]
    outdeg = torch.bincount(s, minlength=n)
    d = torch.repeat_interleave(torch.arange(n), indeg)
    assert n % (256 // G) != 0 and n > 128 * (256 // G)
    assert int((indeg[:N_EMPTY] == 0).sum()) == N_EMPTY and int(indeg[8]) == 1
    assert indeg[9:23].tolist() == list(range(2, 16)) and int(indeg[23]) == 17 and int(indeg[24]) == 150
    assert int((outdeg[n - N_SINKS:] == 0).sum()) == N_SINKS
    assert torch.unique(s * n + d).numel() < s.numel()                # duplicate edges
    assert bool((s == d).any())                                       # self loops


DEGENERATE = {"one node, no edge": (1, [], []), "one node, a self loop": (1, [0], [0]), "a directed ring of three": (3, [0, 1, 2], [1, 2, 0]),
              "no node": (0, [], [])}


def csr_of(n, src, dst):
    """CSR by destination (a stable sort: edges of one destination keep their order) as int64 CPU tensors, and ``perm`` (CSR position ->
    edge)."""
    src, dst = torch.as_tensor(src, dtype=torch.int64), torch.as_tensor(dst, dtype=torch.int64)
    perm = torch.sort(dst, stable=True).indices if dst.numel() else dst
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    if dst.numel():
        rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
    return {"n": n, "rowptr": rowptr, "src": src[perm], "perm": perm}


def dst_of(csr):
    return torch.repeat_interleave(torch.arange(csr["n"]), csr["rowptr"][1:] - csr["rowptr"][:-1])


# ---------------------------------------------------------------------------------------------------- the aggregation as loops (float64)
def loop_forward(x, eps, csr, mode, bias=None, scale=None):
    """(out, arg) by plain loops; arg [n, D] int64 = the first CSR position of the maximum, -1 in rows without in-edges (and under sum / mean)."""
    n, D = x.shape
    out = torch.zeros((n, D), dtype=torch.float64)
    arg = torch.full((n, D), -1, dtype=torch.int64)
    rowptr, src = csr["rowptr"].tolist(), csr["src"].tolist()
    for w in range(n):
        e0, e1 = rowptr[w], rowptr[w + 1]
        for c in range(D):
            if mode == "max":
                best, at = 0.0, -1
                for e in range(e0, e1):
                    m = float(x[src[e], c]) * (float(scale[e]) if scale is not None else 1.0)
                    if at < 0 or m > best:
                        best, at = m, e
                neigh = best
                arg[w, c] = at
            else:
                neigh = 0.0
                for e in range(e0, e1):
                    neigh += float(x[src[e], c]) * (float(scale[e]) if scale is not None else 1.0)
                if mode == "mean" and e1 > e0:
                    neigh /= (e1 - e0)
            out[w, c] = (1.0 + float(eps)) * float(x[w, c]) + neigh + (float(bias[c]) if bias is not None else 0.0)
    return out, arg


def loop_backward(g, x, eps, csr, mode, arg, scale=None):
    """(g_x, g_eps, g_bias, g_scale) by plain loops, from the definition."""
    n, D = x.shape
    gx = (1.0 + float(eps)) * g.clone()
    gs = torch.zeros(csr["src"].numel(), dtype=torch.float64)
    rowptr, src = csr["rowptr"].tolist(), csr["src"].tolist()
    for w in range(n):
        e0, e1 = rowptr[w], rowptr[w + 1]
        cw = 1.0 / (e1 - e0) if (mode == "mean" and e1 > e0) else 1.0
        for e in range(e0, e1):
            for c in range(D):
                if mode == "max" and int(arg[w, c]) != e:
                    continue
                s = float(scale[e]) if scale is not None else 1.0
                gx[src[e], c] += s * cw * float(g[w, c])
                gs[e] += cw * float(g[w, c]) * float(x[src[e], c])
    return gx, float((g * x).sum()), g.sum(0), gs


# ---------------------------------------------------------------------------------------------------- the same in closed form (float64)
def closed_form(x, eps, csr, mode, bias=None, scale=None, g=None, arg=None):
    """out (and, with ``g``, the gradients) as tensor expressions.  ``arg`` [n, D]: replay these maximum positions (the side of a near-tie is
    decided in fp32 on the GPU); None: the first-position rule in float64.  Returns a dict: out, arg, top (the float64 maximum), and with g:
    g_x, g_eps, g_bias, g_scale."""
    n, D = x.shape
    rowptr, src = csr["rowptr"], csr["src"]
    deg = rowptr[1:] - rowptr[:-1]
    dst = dst_of(csr)
    E = src.numel()
    msg = x[src] * (scale.view(-1, 1) if scale is not None else 1.0)
    res = {}
    pos = torch.arange(E).view(-1, 1).expand(E, D)
    idx = dst.view(-1, 1).expand(E, D)
    if mode == "max":
        top = torch.full((n, D), float("-inf"), dtype=torch.float64).scatter_reduce(0, idx, msg, "amax")
        if arg is None:
            arg = torch.full((n, D), E, dtype=torch.int64).scatter_reduce(0, idx, torch.where(msg == top[dst], pos, E), "amin")
            arg = torch.where(arg < E, arg, -1)
        chosen = (arg.long()[dst] == pos).to(torch.float64)
        coef = chosen
        res["top"] = torch.where(deg.view(-1, 1) > 0, top, torch.zeros(()).double())
    else:
        arg = torch.full((n, D), -1, dtype=torch.int64)
        cw = (1.0 / deg.clamp(min=1).double()) if mode == "mean" else torch.ones(n, dtype=torch.float64)
        coef = cw[dst].view(-1, 1).expand(E, D)
    neigh = torch.zeros((n, D), dtype=torch.float64).index_add(0, dst, msg * coef)
    res["out"] = (1.0 + float(eps)) * x + neigh + (bias if bias is not None else 0.0)
    res["arg"] = arg
    if g is not None:
        gm = g[dst] * coef                                            # d loss / d (scaled message)
        res["g_x"] = (1.0 + float(eps)) * g + torch.zeros((n, D), dtype=torch.float64).index_add(
            0, src, gm * (scale.view(-1, 1) if scale is not None else 1.0))
        res["g_scale"] = (gm * x[src]).sum(1)
        res["g_eps"] = (g * x).sum()
        res["g_eps_bound"] = TOL * float(((g * x) ** 2).sum().sqrt())
        res["g_bias"] = g.sum(0)
    return res


class Plan:
    """GraphPlan's attribute names over a ``csr_of`` table (what ``ops.gin_aggregate`` and its reference take), on ``device``."""

    def __init__(self, csr, device="cpu"):
        n, E = csr["n"], int(csr["src"].numel())
        src, dst = csr["src"], dst_of(csr)
        cperm = torch.sort(src, stable=True).indices if E else src
        colptr = torch.zeros(n + 1, dtype=torch.int64)
        if E:
            colptr[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
        i32 = lambda t: t.to(torch.int32).contiguous().to(device)
        self.num_nodes, self.num_edges = n, E
        self.rowptr, self.src, self.colptr = i32(csr["rowptr"]), i32(src), i32(colptr)
        self.csc_eid, self.csc_dst = i32(cperm), i32(dst[cperm] if E else dst)


# ---------------------------------------------------------------------------------------------------- the whole model (float64)
def _bn(P, R, key, h, train, eps=1e-5, momentum=0.1):
    if train:
        n = h.shape[0]
        mean = h.mean(0)
        var = ((h - mean) ** 2).mean(0)
        R[key + ".running_mean"] = (1 - momentum) * R[key + ".running_mean"] + momentum * mean.detach()
        R[key + ".running_var"] = (1 - momentum) * R[key + ".running_var"] + momentum * var.detach() * n / (n - 1)
        R[key + ".num_batches_tracked"] = R[key + ".num_batches_tracked"] + 1
    else:
        mean, var = R[key + ".running_mean"], R[key + ".running_var"]
    return (h - mean) / torch.sqrt(var + eps) * P[key + ".weight"] + P[key + ".bias"]


def _pool(P, kind, layer, h, bnn, taps=None):
    B = bnn.numel()
    seg = torch.repeat_interleave(torch.arange(B), bnn)
    outs = []
    for b in range(B):
        rows = h[seg == b]
        if rows.shape[0] == 0:
            outs.append(torch.zeros(h.shape[1], dtype=h.dtype))
        elif kind == "sum":
            outs.append(rows.sum(0))
        elif kind == "mean":
            outs.append(rows.mean(0))
        elif kind == "max":
            outs.append(rows.max(0).values)
        else:
            gate = rows @ P[f"pools.{layer}.gate_nn.weight"].t() + P[f"pools.{layer}.gate_nn.bias"]
            _tap(taps, f"pools.{layer}.gate_nn.bias", gate)            # (a softmax does not see a shift: this bias has no gradient)
            outs.append((torch.softmax(gate, 0) * rows).sum(0))
    return torch.stack(outs)


def _tap(taps, name, z):
    if taps is not None and z.requires_grad:
        z.retain_grad()
        taps.setdefault(name, []).append(z)


def cancelling_bounds(taps):
    """For every parameter whose gradient is a sum of terms that cancel EXACTLY - the bias of a Linear in front of a train-mode BatchNorm
    (the mean is subtracted), the bias of an attention gate (a softmax does not see a shift) - the bound its fp32 value is held to: 1e-4 of
    the largest column sum of the MAGNITUDES of the terms (the gradients of the tapped Linear outputs), the scale of the sum's rounding
    error.  1e-4 of the largest float64 entry would be 1e-4 of rounding noise there (the float64 value is 1e-17, not 0)."""
    return {k: TOL * max(float(sum(z.grad.abs().sum(0) for z in zs if z.grad is not None).max()), 1e-30) for k, zs in taps.items()}


def model_ref(state, x, csr, bnn, num_layers, num_mlp_layers, neighbor, readout, train, masks=None, drops=None, scale=None, taps=None):
    """GIN.forward in float64 from a state_dict.  ``state``: name -> float64 tensor (leaves that require grad get gradients).  ``masks``: the
    0 / 1 outcome of every ReLU in execution order, replayed instead of deciding in float64.  ``drops``: the keep-mask * 1 / (1 - p) of every
    inter-layer dropout.  Returns (logits, the buffers after the call, the ReLU pre-activations in execution order).  ``taps``: a dict
    that receives the Linear outputs behind the exactly-cancelling gradients (``cancelling_bounds``)."""
    P = state
    R = {k: v.clone() for k, v in state.items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    pre = []

    def relu(z):
        pre.append(z)
        return z * masks[len(pre) - 1] if masks is not None else torch.relu(z)

    def lin(key, h, into_bn=False):
        z = h @ P[key + ".weight"].t() + P[key + ".bias"]
        if into_bn and train:
            _tap(taps, key + ".bias", z)
        return z

    h = x
    h_list = []
    for i in range(num_layers - 1):
        if i != 0 and drops is not None:
            h = h * drops[i - 1]
        h_list.append(lin(f"linears_prediction.{i}", _pool(P, readout, i, h, bnn, taps)))
        a = f"layers.{i}.apply_func"
        dst = dst_of(csr)
        msg = h[csr["src"]] * (scale.view(-1, 1) if scale is not None else 1.0)
        n, D = h.shape
        if neighbor == "max":
            r = closed_form(h.detach(), 0.0, csr, "max", scale=scale)
            neigh = torch.zeros((n, D), dtype=torch.float64).index_add(0, dst, msg * (r["arg"][dst] == torch.arange(dst.numel()).view(-1, 1)).double())
        else:
            neigh = torch.zeros((n, D), dtype=torch.float64).index_add(0, dst, msg)
            if neighbor == "mean":
                neigh = neigh / (csr["rowptr"][1:] - csr["rowptr"][:-1]).clamp(min=1).double().view(-1, 1)
        h = (1.0 + P[f"layers.{i}.eps"].reshape(())) * h + neigh
        if num_mlp_layers == 1:
            h = lin(a + ".mlp.linear", h, True)
        else:
            for j in range(num_mlp_layers - 1):
                h = relu(_bn(P, R, a + f".mlp.batch_norms.{j}", lin(a + f".mlp.linears.{j}", h, True), train))
            h = lin(a + f".mlp.linears.{num_mlp_layers - 1}", h, True)
        h = relu(_bn(P, R, a + ".bn", h, train))
    h_list.append(lin("classify", _pool(P, readout, num_layers, h, bnn, taps)))
    return torch.stack(h_list).sum(0), R, pre
