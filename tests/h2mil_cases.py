"""Float64 restatements of the H2MIL layers (one slide at a time, plain loops where a loop is clearest) and the seeded cases the H2MIL tests
share.  Written from the specification, independently of wsi_hgnn_amd/h2mil: the tests hold the package against these, and these against the
fixtures recorded from the reference's own code (tests/golden/h2mil).

Margin condition.  Pooling decisions are discrete; a test compares them only on inputs where float32 cannot flip them.  In the float64
restatement, for every segment: at each selected sorted position the fitness differs from both neighbours in the order by >= MARGIN, and for
each node the second-nearest seed is >= MARGIN farther than the nearest.  MARGIN = 1e-3 is ten times the project's tolerance norm of 1e-4 x the
largest entry, and fitness and coordinates lie in [-1, 1], so any upstream result inside the tolerance leaves every decision unchanged.
``ihpool_ref`` returns the smallest such difference it met; ``find_case`` tries seeds in order and asserts one is found within 20."""
import math

import torch
import torch.nn.functional as F

MARGIN = 1e-3
TRIES = 20


# ------------------------------------------------------------------------------------------------ RAConv
def ra_attention_ref(ft, sc, bias, ei, nt, slope=0.2):
    """The two-level softmax of the specification from the projected features ``ft`` [n, C] and ``sc`` [n, 4] = el | er | pl | pr."""
    n, C, E = ft.shape[0], ft.shape[1], ei.shape[1]
    el, er, pl, pr = sc.unbind(1)
    u, v = ei[0], ei[1]
    g = v * 3 + nt[u]
    onehot = torch.zeros(E, 3 * n, dtype=ft.dtype)
    onehot[torch.arange(E), g] = 1
    s = F.leaky_relu(el[u] + er[v], slope)
    smax = torch.where(onehot > 0, s.detach()[:, None], torch.full_like(onehot, -math.inf)).max(0).values if E else torch.zeros(3 * n, dtype=ft.dtype)
    ex = torch.exp(s - smax[g])
    a = ex / (onehot.t() @ ex)[g]
    cnt = onehot.sum(0)
    q = F.leaky_relu(((onehot.t() @ pl[u]) / cnt.clamp(min=1)).view(n, 3) + pr[:, None], slope)
    present = cnt.view(n, 3) > 0
    q = torch.where(present, q, torch.full_like(q, -math.inf))
    q = torch.where(present.any(1, keepdim=True), q, torch.zeros_like(q))
    beta = torch.softmax(q, 1) * present.to(ft.dtype)
    out = torch.zeros(n, C, dtype=ft.dtype).index_add(0, v, (beta.reshape(-1)[g] * a)[:, None] * ft[u])
    return out + bias if bias is not None else out


def raconv_ref(x, ei, nt, p, slope=0.2):
    """RAConv at heads = 1.  ``p``: the layer's state_dict entries (any float dtype = x's)."""
    Wl, Wt = p["lin_l.weight"], p["t_lin_l.weight"]
    C = Wl.shape[0]
    ft, xt = x @ Wl.t(), x @ Wt.t()
    sc = torch.stack([ft @ p["att_l"].reshape(C), ft @ p["att_r"].reshape(C), xt @ p["t_att_l"].reshape(C), xt @ p["t_att_r"].reshape(C)], 1)
    return ra_attention_ref(ft, sc, p.get("bias"), ei, nt, slope)


# ------------------------------------------------------------------------------------------------ IHPool
def reference_step(n, ratio, level):
    """The reference's own expressions for the stride over the sorted members (IHPool.py:128-134 and :176-182); None = 'first and last'."""
    if ratio < 1:
        return int(torch.ceil(torch.tensor(n / (n * ratio))))
    if level == 1:
        return int(torch.ceil(torch.tensor(n / n))) if n < ratio else int(torch.ceil(torch.tensor(n / ratio)))
    return n if n == 1 else n - 1


def _pick_and_assign(xy, f, members, ratio, level):
    """Seeds of one segment and every member's seed.  Returns (positions of the seeds among ``members``, assignment, smallest margin, the
    positions among ``members`` whose FITNESS is too near a selected neighbour's, the positions whose two nearest SEEDS are too nearly
    equidistant)."""
    fm = f[members]
    order = torch.sort(fm, stable=True).indices                  # equal fitness in node order
    n = len(members)
    sel = list(range(0, n, reference_step(n, ratio, level)))
    margin, bad_f = math.inf, set()
    srt = fm[order]
    for pos in sel:
        for nb in (pos - 1, pos + 1):
            if 0 <= nb < n:
                gap = abs(float(srt[pos] - srt[nb]))
                margin = min(margin, gap)
                if gap < MARGIN:
                    bad_f.add(int(order[nb]))
    seeds = order[sel]
    pts, spts = xy[members], xy[members][seeds]
    d = (spts[:, None, :] - pts[None, :, :]).pow(2).sum(-1).sqrt() + (fm[seeds][:, None] - fm[None, :]).abs()      # [seeds, members]
    d[torch.arange(len(sel)), seeds] = -1.0                      # a seed owns its cluster
    rows = torch.arange(len(sel))[:, None].expand_as(d)
    assign = torch.where(d == d.min(0, keepdim=True).values, rows, torch.full_like(rows, len(sel))).min(0).values      # equal distance: the lowest seed
    bad_xy = []
    if len(sel) > 1:
        two = torch.sort(d, 0).values[:2]
        gap = torch.where(two[0] >= 0, two[1] - two[0], two[1])
        margin = min(margin, float(gap.min()))
        bad_xy = (gap < MARGIN).nonzero().view(-1).tolist()
    return seeds, assign, margin, sorted(bad_f), bad_xy


def ihpool_ref(x, ei, nt, tree, xy, w1, w2, ratio):
    """One slide through IHPool at select='inter', dis='ou'.  Returns a dict: x, edge_index, cluster, node_type, tree, fitness, x_y_index,
    margin (the smallest difference met), bad_f and bad_xy (the input rows at which the fitness / the distance half of the margin condition
    fails)."""
    n = x.shape[0]
    i1, i2 = (nt == 1).nonzero().view(-1), (nt == 2).nonzero().view(-1)
    n1 = len(i1)
    xd = x.detach()
    w1, w2 = w1.detach(), w2.detach()
    f1 = torch.tanh((xd[i1] * w1).sum(-1) / w1.norm(p=2, dim=-1))
    f2 = torch.tanh((xd[i2] * w2).sum(-1) / w2.norm(p=2, dim=-1))
    margin, bad_f, bad_xy = math.inf, [], []
    k1 = 0
    cluster = torch.zeros(n, dtype=torch.int64)
    if n1:
        seeds, c1, m, bf, bx = _pick_and_assign(xy[i1], f1, torch.arange(n1), ratio, 1)
        margin, k1 = min(margin, m), len(seeds)
        bad_f += i1[bf].tolist()
        bad_xy += i1[bx].tolist()
        cluster[i1] = 1 + c1
    new_tree, nxt = [-1] + [0] * k1, 1 + k1
    if len(i2):
        seg = c1[tree[i2] - 1]                                   # a level-2 node follows its parent (the level-1 node at row tree)
        for k in range(k1):
            mem = (seg == k).nonzero().view(-1)
            if not len(mem):
                continue                                         # a childless level-1 cluster contributes no level-2 cluster
            seeds, c2, m, bf, bx = _pick_and_assign(xy[i2], f2, mem, ratio, 2)
            margin = min(margin, m)
            bad_f += i2[mem[bf]].tolist()
            bad_xy += i2[mem[bx]].tolist()
            cluster[i2[mem]] = nxt + c2
            new_tree += [k + 1] * len(seeds)
            nxt += len(seeds)
    cnt = torch.zeros(nxt, dtype=x.dtype).index_add(0, cluster, torch.ones(n, dtype=x.dtype))
    x_new = torch.zeros(nxt, x.shape[1], dtype=x.dtype).index_add(0, cluster, x) / cnt[:, None]
    xy_new = torch.zeros(nxt, 2, dtype=xy.dtype).index_add(0, cluster, xy) / cnt.to(xy.dtype)[:, None]
    xy_new[0] = 0
    pairs = {(int(cluster[a]), int(cluster[b])) for a, b in ei.t().tolist()} | {(c, c) for c in range(nxt)}
    fitness = torch.zeros(n, dtype=x.dtype)
    fitness[i1], fitness[i2] = f1, f2
    return {"x": x_new, "edge_index": torch.tensor(sorted(pairs), dtype=torch.int64).t().reshape(2, -1), "cluster": cluster,
            "node_type": torch.tensor([0] + [1] * k1 + [2] * (nxt - 1 - k1), dtype=torch.int64), "tree": torch.tensor(new_tree, dtype=torch.int64),
            "fitness": fitness, "x_y_index": xy_new, "margin": margin, "bad_f": bad_f, "bad_xy": bad_xy}


# ------------------------------------------------------------------------------------------------ the model
def graph_norm(x, w, b, eps=1e-5):
    xc = x - x.mean()
    return xc / (xc.pow(2).mean().sqrt() + eps) * w + b


def _sub(p, prefix):
    return {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix)}


def h2mil_ref(slide, p, ratios=(0.2, 4), mpool="global_mean_pool"):
    """One slide through the model in eval mode / with dropout 0.  ``p``: the state_dict in x's dtype.  Returns (probabilities [1, classes],
    [pool_1 outputs, pool_2 outputs], smallest margin)."""
    x, ei, nt, tree = slide["x"], slide["edge_index_tree_8nb"], slide["node_type"], slide["node_tree"]
    xy = slide["x_y_index"].to(x.dtype) * 2 - 1
    nw, nb = p["norm.weight"], p["norm.bias"]
    read = (lambda t: t.mean(0, keepdim=True)) if mpool == "global_mean_pool" else (lambda t: t.max(0, keepdim=True).values)
    if mpool == "global_att_pool":
        def read(t):
            g = torch.relu(t @ p["mpool.gate_nn.0.weight"].t() + p["mpool.gate_nn.0.bias"]) @ p["mpool.gate_nn.2.weight"].t() + p["mpool.gate_nn.2.bias"]
            return (torch.softmax(g, 0) * t).sum(0, keepdim=True)
    h = graph_norm(x, nw, nb)
    h = graph_norm(torch.relu(raconv_ref(h, ei, nt, _sub(p, "conv1."))), nw, nb)
    o1 = ihpool_ref(h, ei, nt, tree, xy, p["pool_1.weight_1"], p["pool_1.weight_2"], ratios[0])
    x1 = read(o1["x"])
    h = graph_norm(torch.relu(raconv_ref(o1["x"], o1["edge_index"], o1["node_type"], _sub(p, "conv2."))), nw, nb)
    o2 = ihpool_ref(h, o1["edge_index"], o1["node_type"], o1["tree"], o1["x_y_index"], p["pool_2.weight_1"], p["pool_2.weight_2"], ratios[1])
    x2 = read(o2["x"])
    h = graph_norm(torch.relu((x1 + x2) @ p["lin1.weight"].t() + p["lin1.bias"]), nw, nb)
    probs = torch.softmax(h @ p["lin2.weight"].t() + p["lin2.bias"], -1)
    return probs, [o1, o2], min(o1["margin"], o2["margin"])


def reference_run(slides, state, labels, ratios=(0.2, 4), mpool="global_mean_pool"):
    """The slides one at a time through ``h2mil_ref`` under the float64 ``state``: (probabilities [B, classes], the two pools' outputs per
    slide, the loss of a step = the sum over the slides of CrossEntropyLoss applied to the probabilities, its gradient per parameter)."""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in state.items()}
    probs, pools, loss = [], [], 0.0
    for b, s in enumerate(slides):
        pr, po, _ = h2mil_ref(double(s), p, ratios, mpool)
        probs.append(pr)
        pools.append(po)
        loss = loss + F.cross_entropy(pr, labels[b:b + 1])
    loss.backward()
    return torch.cat(probs).detach(), pools, loss.detach(), {k: v.grad for k, v in p.items()}


# ------------------------------------------------------------------------------------------------ cases
def tree_slide(seed, n1, children=(1, 5), feat=16, neighbours=8, dtype=torch.float32):
    """A synthetic three-level slide as the reference's ``Data`` fields: one root, ``n1`` level-1 nodes, ``children`` = (lo, hi) level-2
    children each; every node has up to ``neighbours`` random same-level neighbours plus parent / child edges both ways."""
    g = torch.Generator().manual_seed(seed)
    kids = torch.randint(children[0], children[1] + 1, (n1,), generator=g).tolist() if n1 else []
    n2 = sum(kids)
    n = 1 + n1 + n2
    nt = torch.tensor([0] + [1] * n1 + [2] * n2, dtype=torch.int64)
    tree = torch.tensor([-1] + [0] * n1 + [1 + i for i, k in enumerate(kids) for _ in range(k)], dtype=torch.int64)
    src, dst = [], []
    for lo, hi in ((1, 1 + n1), (1 + n1, n)):
        m = hi - lo
        for i in range(lo, hi):
            if m > 1:
                for j in torch.randint(0, m, (min(neighbours, m - 1),), generator=g).tolist():
                    if lo + j != i:
                        src.append(lo + j); dst.append(i)
    for i in range(1, n):
        par = int(tree[i])
        src += [par, i]; dst += [i, par]
    return {"x": torch.randn(n, feat, generator=g, dtype=torch.float32).to(dtype), "edge_index_tree_8nb": torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1),
            "node_type": nt, "node_tree": tree, "x_y_index": torch.rand(n, 2, generator=g, dtype=torch.float32).to(dtype)}


def find_case(make, margin_of, first_seed=0):
    """The first of TRIES consecutive seeds whose case meets the margin condition: (case, seed).  ``make(seed)`` builds a case,
    ``margin_of(case)`` runs the float64 restatement and returns its smallest margin."""
    for seed in range(first_seed, first_seed + TRIES):
        case = make(seed)
        if margin_of(case) >= MARGIN:
            return case, seed
    raise AssertionError(f"no case met the margin condition within {TRIES} seeds from {first_seed}")


def double(slide):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in slide.items()}


# the three slides of the model tests: about 60, 150 and 400 nodes (level-1 nodes, children per level-1 node)
MODEL_SHAPES = ((9, (4, 7)), (24, (4, 6)), (57, (5, 7)))
MODEL_CFG = dict(in_feats=24, n_hidden=0, out_classes=16, no_of_class=3)


REPAIR_ROUNDS = 40


def make_model(kernels, dtype=torch.float32, drop_out_ratio=0.0, mpool="global_mean_pool", seed=2024):
    """The seeded model of the model tests, its parameters rounded to float32 values.  The shared LayerNorm gets weight 0.4 and bias 0.1: it
    matters in every gradient, and the fitness tanh(<x, w> / |w|) of its output stays out of saturation, where neighbouring values crowd."""
    from wsi_hgnn_amd import h2mil
    torch.manual_seed(seed)
    m = h2mil.H2MIL(**MODEL_CFG, drop_out_ratio=drop_out_ratio, mpool_method=mpool, kernels=kernels).double()
    with torch.no_grad():
        m.norm.weight.fill_(0.4)
        m.norm.bias.fill_(0.1)
        for p in m.parameters():
            p.copy_(p.to(torch.float32).to(torch.float64))
    return m.to(dtype)


def repaired_slide(seed, n1, kids, model_state, ratios, mpool):
    """``tree_slide(seed, ...)`` with the rows at which the margin condition fails adjusted (same seed, a second generator), for at most
    REPAIR_ROUNDS rounds.  Plain rejection cannot work at 400 nodes: with about 80 seeds and 400 assignments a slide has several hundred
    decisions, each within 1e-3 of a tie with probability around 1e-2.  A row whose two nearest seeds are too nearly equidistant gets new
    coordinates, which touch no other row's decision.  A row whose fitness is too near a selected neighbour's gets a nudge to the features of
    its first in-neighbour (RAConv has no self term: a row's fitness comes from its in-neighbours), small enough to leave the slide's LayerNorm
    statistics where they were.  After the second pool a failing cluster stands for its first member.  Whether the result meets the
    condition is decided by ``find_case``, not here."""
    s = tree_slide(seed, n1, kids, feat=MODEL_CFG["in_feats"])
    g = torch.Generator().manual_seed(1_000_003 * (seed + 1))
    src, dst = s["edge_index_tree_8nb"]
    for _ in range(REPAIR_ROUNDS):
        _, pools, margin = h2mil_ref(double(s), model_state, ratios, mpool)
        if margin >= MARGIN:
            break
        member = lambda c: int((pools[0]["cluster"] == c).nonzero()[0])
        for r in sorted(set(pools[0]["bad_xy"]) | {member(c) for c in pools[1]["bad_xy"]}):
            s["x_y_index"][r] = torch.rand(2, generator=g)
        for r in sorted(set(pools[0]["bad_f"]) | {member(c) for c in pools[1]["bad_f"]}):
            s["x"][int(src[(dst == r).nonzero()[0]])] += 0.3 * torch.randn(s["x"].shape[1], generator=g)
    return s


def model_slides(model_state, ratios=(0.2, 4), mpool="global_mean_pool", shapes=MODEL_SHAPES):
    """The three margin-condition slides of the model tests under the float64 state ``model_state``: every slide is drawn on its own (slides of
    a batch do not interact: the LayerNorm statistics are per slide), seeds tried in order from 100 x its index."""
    out = []
    for i, (n1, kids) in enumerate(shapes):
        make = lambda seed: repaired_slide(seed, n1, kids, model_state, ratios, mpool)
        slide, _ = find_case(make, lambda s: h2mil_ref(double(s), model_state, ratios, mpool)[2], first_seed=100 * i)
        out.append(slide)
    return out


# ------------------------------------------------------------------------------------------------ kernel cases
def assign_ref(xyf, member_node, member_seg, seed_ptr, seed_node):
    """wsi_ihpool_assign in float64, segment by segment; returns (assign, the gap between the nearest and the second-nearest seed per member,
    inf where a member has fewer than two seeds)."""
    xyf = xyf.double()
    m = member_node.shape[0]
    out, gaps = torch.full((m,), -1, dtype=torch.int64), torch.full((m,), math.inf, dtype=torch.float64)
    for s in range(seed_ptr.shape[0] - 1):
        mem = (member_seg == s).nonzero().view(-1)
        seeds = seed_node[seed_ptr[s]:seed_ptr[s + 1]].long()
        if not len(mem) or not len(seeds):
            continue
        a, b = xyf[seeds], xyf[member_node[mem].long()]
        d = (a[:, None, :2] - b[None, :, :2]).pow(2).sum(-1).sqrt() + (a[:, None, 2] - b[None, :, 2]).abs()
        d = torch.where(seeds[:, None] == member_node[mem].long()[None, :], torch.full_like(d, -1.0), d)
        rows = torch.arange(len(seeds))[:, None].expand_as(d)
        out[mem] = torch.where(d == d.min(0, keepdim=True).values, rows, torch.full_like(rows, len(seeds))).min(0).values
        if len(seeds) > 1:
            two = torch.sort(d, 0).values[:2]
            gaps[mem] = torch.where(two[0] >= 0, two[1] - two[0], two[1])
    return out, gaps


ASSIGN_MEMBERS = (1, 2, 63, 64, 65, 300)
ASSIGN_SEEDS = (1, 2, 7, 65)


def assign_case(seed):
    """Segments of every size in ASSIGN_MEMBERS under every seed count in ASSIGN_SEEDS (capped by the size) and one empty segment in the middle;
    the members of the segments are scattered over the node table.  A member whose two nearest seeds are within MARGIN of equidistant is drawn
    again (members that are no seeds only, so no other member's distances move), at most 20 times.  Returns (xyf fp32, member_node,
    member_seg, seed_ptr, seed_node)."""
    g = torch.Generator().manual_seed(seed)
    sizes = []
    for m in ASSIGN_MEMBERS:
        for k in ASSIGN_SEEDS:
            sizes.append((m, min(k, m)))
    sizes.insert(len(sizes) // 2, (0, 0))
    total = sum(m for m, _ in sizes)
    xyf = torch.rand(total, 3, generator=g) * 2 - 1
    nodes = torch.randperm(total, generator=g)
    member_node, member_seg, seed_ptr, seed_node, at = [], [], [0], [], 0
    for s, (m, k) in enumerate(sizes):
        mine = nodes[at:at + m]
        at += m
        member_node.append(mine)
        member_seg += [s] * m
        seed_node.append(mine[torch.randperm(m, generator=g)[:k]] if m else mine)
        seed_ptr.append(seed_ptr[-1] + k)
    case = [xyf, torch.cat(member_node).to(torch.int32), torch.tensor(member_seg, dtype=torch.int32), torch.tensor(seed_ptr, dtype=torch.int32),
            torch.cat(seed_node).to(torch.int32)]
    is_seed = torch.zeros(total, dtype=torch.bool)
    is_seed[case[4].long()] = True
    for _ in range(20):
        gaps = assign_ref(*case)[1]
        again = case[1].long()[(gaps < MARGIN) & ~is_seed[case[1].long()]]
        if not len(again):
            break
        xyf[again] = torch.rand(len(again), 3, generator=g) * 2 - 1
    return tuple(case)


def ra_kernel_graph(seed=0):
    """The graph of the ra_attention kernel tests: destinations 0..6 have in-degrees 0, 1, 2, 63, 64, 65 and 200; destination 3 receives from
    one type only, 4 from two, 5 from all three with ONE edge from type 0 (a group of one edge) - as has destination 1; every tenth edge of the
    rest is repeated.  Returns (n, node_type, edge_index)."""
    g = torch.Generator().manual_seed(seed)
    n = 300
    nt = torch.randint(0, 3, (n,), generator=g)
    nt[:9] = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1, 2])
    of = [(nt == t).nonzero().view(-1) for t in range(3)]
    pick = lambda t, k: of[t][torch.randint(0, len(of[t]), (k,), generator=g)]
    src, dst = [], []
    def add(v, us):
        src.append(us); dst.append(torch.full((len(us),), v, dtype=torch.int64))
    add(1, pick(2, 1))
    add(2, torch.cat([pick(0, 1), pick(1, 1)]))
    add(3, pick(2, 63))
    add(4, torch.cat([pick(0, 30), pick(1, 34)]))
    add(5, torch.cat([pick(0, 1), pick(1, 40), pick(2, 24)]))
    add(6, torch.randint(0, n, (200,), generator=g))
    for v in range(7, n):
        k = int(torch.randint(0, 7, (1,), generator=g))
        us = torch.randint(0, n, (k,), generator=g)
        add(v, torch.cat([us, us[:1]]) if v % 10 == 0 and k else us)
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    return n, nt, ei


# ------------------------------------------------------------------------------------------------ the ra_attention dispatch sweep
# One width per (VEC, G, NK) code of csrc/ra_attn.hip's dispatch (all cases of csrc/row_group.h), none on a boundary of row_cfg; the two last of
# each family share a code (a partly filled and a full last chunk).  tests/test_h2mil.py restates row_cfg and checks the coverage without a GPU.
RA_WIDTHS_BEFORE = (1, 3, 4, 32, 256, 260)                   # test_h2mil_kernels_gpu.py's widths before the sweep
RA_SWEEP_VEC4 = (8, 24, 44, 100, 200, 388, 772, 1284, 2052, 4096)
RA_SWEEP_VEC1 = (2, 7, 13, 30, 50, 101, 130, 257, 515, 1025, 2050, 4095)
RA_SWEEP = RA_SWEEP_VEC4 + RA_SWEEP_VEC1
RA_FALLBACK_WIDTHS = (8, 44, 200, 772)                       # multiples of 4 sent down the scalar family by a stride or an offset
RA_ONE_HOT_WIDTHS = (8, 24, 44, 100, 200, 2052, 2050)        # sc x 30: one width per group size G, and the two widest NK of each family
RA_SLOPE_CASES = ((388, 0.05), (101, 0.05), (1284, 0.0), (257, 0.0))      # (width, negative_slope): one width per VEC at each slope
RA_TOL = 1e-4                                                # the kernel tests' norm: error <= RA_TOL x the largest float64 entry
RA_KINK = 1e-5                                               # x the score scale: the least distance of a leaky_relu argument from 0
RA_OUT_ROWS, RA_GFT_ROWS = (3, 4, 5, 6), (10, 11, 12)        # the rows checked against their OWN largest entry
RA_HUBS = ((10, 17), (11, 65), (12, 200))                    # (source, least out-degree)
RA_SINKS = 24


def ra_sweep_graph(seed=0):
    """The graph of the dispatch sweep, n = 333 (no multiple of 256 / G for any G).  Destinations 0..6 as in ``ra_kernel_graph``
    (in-degrees 0, 1, 2, 63, 64, 65, 200; destination 3 fed by one type, 4 by two, 5 by three with ONE edge of type 0, as destination 1).
    Sources 10, 11 and 12 (12 of type 0, as a slide's root) feed at least 17, 65 and 200 edges: more than one trip of a 16-lane and of a
    64-lane stride loop over a source's edges.  The last RA_SINKS nodes are never sources, the very last has no edge at all; every tenth
    destination repeats an edge; node 20 has the only self loop.  Returns (n, node_type, edge_index)."""
    g = torch.Generator().manual_seed(seed)
    n = 333
    R = n - RA_SINKS
    nt = torch.randint(0, 3, (n,), generator=g)
    nt[:9] = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1, 2])
    nt[12] = 0
    of = [(nt[:R] == t).nonzero().view(-1) for t in range(3)]

    def pick(t, k, v):                                           # k sources of type t other than v
        pool = of[t][of[t] != v]
        return pool[torch.randint(0, len(pool), (k,), generator=g)]

    def others(k, v, hi=R):                                      # k sources below hi other than v
        us = torch.randint(0, hi - 1, (k,), generator=g)
        return us + (us >= v)

    src, dst = [], []

    def add(v, us):
        src.append(us); dst.append(torch.full((len(us),), v, dtype=torch.int64))
    add(1, pick(2, 1, 1))
    add(2, torch.cat([pick(0, 1, 2), pick(1, 1, 2)]))
    add(3, pick(2, 63, 3))
    add(4, torch.cat([pick(0, 30, 4), pick(1, 34, 4)]))
    add(5, torch.cat([pick(0, 1, 5), pick(1, 40, 5), pick(2, 24, 5)]))
    add(6, others(200, 6))
    for v in range(7, n - 1):
        k = int(torch.randint(0, 7, (1,), generator=g))
        us = others(k, v)
        add(v, torch.cat([us, us[:1]]) if v % 10 == 0 and k else us)
    for hub, k in RA_HUBS:                                       # the hubs' own edges, to destinations 7 .. n - 2 other than the hub
        vs = 7 + torch.randint(0, n - 9, (k,), generator=g)
        vs = vs + (vs >= hub)
        src.append(torch.full((k,), hub, dtype=torch.int64)); dst.append(vs)
    add(20, torch.tensor([20]))
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    return n, nt, ei


def ra_sweep_facts(n, nt, ei, rowptr, colptr):
    """What ``ra_sweep_graph`` promises, asserted from the edge plan's ``rowptr`` / ``colptr``.  Returns (in-degrees, out-degrees)."""
    indeg, outdeg = rowptr.cpu().long().diff(), colptr.cpu().long().diff()
    assert n == 333 and all(n % (256 // G) for G in (4, 8, 16, 32, 64)) and indeg.numel() == outdeg.numel() == n
    assert torch.equal(indeg, torch.bincount(ei[1], minlength=n)) and torch.equal(outdeg, torch.bincount(ei[0], minlength=n))
    assert indeg[:7].tolist() == [0, 1, 2, 63, 64, 65, 200]
    types_at = lambda v: sorted(nt[ei[0][ei[1] == v]].tolist())
    assert len(set(types_at(3))) == 1 and len(set(types_at(4))) == 2 and len(set(types_at(5))) == 3
    assert types_at(5).count(0) == 1 and len(types_at(1)) == 1                     # groups of a single edge
    for hub, least in RA_HUBS:
        assert int(outdeg[hub]) >= least, (hub, int(outdeg[hub]))
    assert int(nt[12]) == 0
    assert int((outdeg == 0).sum()) >= RA_SINKS and not outdeg[n - RA_SINKS:].any()
    assert int(indeg[n - 1]) == 0 and int(outdeg[n - 1]) == 0                      # a node without any edge
    assert int(indeg[n - RA_SINKS:n - 1].sum()) > 0                                # the other sinks do receive
    assert torch.unique(ei[0] * n + ei[1]).numel() < ei.shape[1]                   # repeated edges
    assert (ei[0] == ei[1]).nonzero().view(-1).numel() == 1 and int(ei[0][ei[0] == ei[1]]) == 20
    return indeg, outdeg


def ra_degenerate_graphs():
    """name -> (n, node_type, edge_index): one node without an edge; a directed ring of three among five nodes (fewer rows than
    WSI_RA_BIAS_PARTS: most column partials of g_bias sum no row; every softmax has one term)."""
    e = lambda *p: torch.tensor(p, dtype=torch.int64).reshape(-1, 2).t().contiguous()
    return {"one-node": (1, torch.tensor([0]), e()), "ring-of-three": (5, torch.tensor([0, 1, 2, 0, 1]), e((0, 1), (1, 2), (2, 0)))}


def ra_inputs(n, Cw, seed=0, scale=1.0):
    """(ft [n, Cw], sc [n, 4] x scale, bias [Cw], the weights of the scalar loss [n, Cw]), fp32, from the seed 1000 Cw + seed."""
    g = torch.Generator().manual_seed(1000 * Cw + seed)
    return (torch.randn(n, Cw, generator=g), torch.randn(n, 4, generator=g) * scale, torch.randn(Cw, generator=g), torch.randn(n, Cw, generator=g))


def ra_run(ft, sc, bias, w, ei, nt, slope=0.2, dtype=torch.float64):
    """``ra_attention_ref`` and its gradients under the loss sum(out * w) in ``dtype``: (out, g_ft, g_sc, g_bias)."""
    f, s, b = (t.detach().to(dtype, copy=True).requires_grad_(True) for t in (ft, sc, bias))
    out = ra_attention_ref(f, s, b, ei, nt, slope)
    (out * w.to(dtype)).sum().backward()
    return out.detach(), f.grad, s.grad, b.grad


def ra_kink_distance(sc, ei, nt):
    """The least |argument| of a leaky_relu in float64: el[u] + er[v] per edge, mean pl + pr per present group (inf without edges)."""
    sc = sc.double()
    u, v = ei[0], ei[1]
    if not u.numel():
        return math.inf
    n = sc.shape[0]
    key = v * 3 + nt[u]
    cnt = torch.zeros(3 * n, dtype=torch.float64).index_add(0, key, torch.ones(u.numel(), dtype=torch.float64))
    mean = torch.zeros(3 * n, dtype=torch.float64).index_add(0, key, sc[u, 2]) / cnt.clamp(min=1)
    q = (mean.view(n, 3) + sc[:, 3:4])[cnt.view(n, 3) > 0]
    return min(float((sc[u, 0] + sc[v, 1]).abs().min()), float(q.abs().min()))


def _ratio(got, want):
    return float((got.double() - want).abs().max()) / max(float(want.abs().max()), 1e-30)


def ra_norms(got, ref):
    """Every figure the kernel tests bound, as name -> error / the largest float64 entry of what the name covers: the four whole tensors,
    the rows RA_OUT_ROWS of out and RA_GFT_ROWS of g_ft (those the graph has) each against its own largest entry, and the four columns of
    g_sc each against its own (g_er and g_pr are cancelling sums; no per-row norm there: the gradients of a one-edge group cancel exactly)."""
    got = [t.detach().cpu() for t in got]
    out = {name: _ratio(g, r) for name, g, r in zip(("out", "g_ft", "g_sc", "g_bias"), got, ref)}
    n = ref[0].shape[0]
    for name, k, rows in (("out", 0, RA_OUT_ROWS), ("g_ft", 1, RA_GFT_ROWS)):
        for r in rows:
            if r < n and float(ref[k][r].abs().max()) > 0:
                out[f"{name}[{r}]"] = _ratio(got[k][r], ref[k][r])
    for c, col in enumerate(("g_el", "g_er", "g_pl", "g_pr")):
        if float(ref[2][:, c].abs().max()) > 0:
            out[col] = _ratio(got[2][:, c], ref[2][:, c])
    return out


_RA_CASES = {}


def ra_case(graph, Cw, scale=1.0, slope=0.2, first_seed=0):
    """The inputs of one kernel comparison with all it is held against, computed once per process: the first of TRIES seeds from
    ``first_seed`` at which (1) every leaky_relu argument is at least RA_KINK x scale from zero in float64, so fp32 cannot take the other
    side of the kink, and (2) the fp32 CPU run of ``ra_attention_ref`` stays within RA_TOL / 4 of the float64 run under every norm of
    ``ra_norms`` - the bound leaves the kernels three quarters of itself.  ``graph`` = (n, node_type, edge_index).  Returns a dict:
    seed, inputs (ft, sc, bias, w), ref (float64 out, g_ft, g_sc, g_bias), e32 (name -> the fp32 run's figure), kink."""
    n, nt, ei = graph
    key = (n, int(ei.shape[1]), Cw, scale, slope, first_seed)
    if key in _RA_CASES:
        return _RA_CASES[key]
    seen = []
    for seed in range(first_seed, first_seed + TRIES):
        inputs = ra_inputs(n, Cw, seed, scale)
        kink = ra_kink_distance(inputs[1], ei, nt)
        if kink < RA_KINK * scale:
            seen.append((seed, "kink", kink))
            continue
        ref = ra_run(*inputs, ei, nt, slope)
        e32 = ra_norms(ra_run(*inputs, ei, nt, slope, torch.float32), ref)
        if max(e32.values()) > RA_TOL / 4:
            seen.append((seed, "e32", max(e32.items(), key=lambda kv: kv[1])))
            continue
        _RA_CASES[key] = {"seed": seed, "inputs": inputs, "ref": ref, "e32": e32, "kink": kink}
        return _RA_CASES[key]
    raise AssertionError(f"C={Cw} scale={scale} slope={slope}: no seed within {TRIES} from {first_seed} met the conditions: {seen}")


def ra_gpu_cases():
    """Every (graph name, width, score scale, negative_slope) tests/test_h2mil_kernels_gpu.py draws through ``ra_case``; tests/test_h2mil.py
    holds each of them to ``ra_case``'s conditions without a GPU.  The fallback and raw-ABI tests reuse sweep cases."""
    cases = [("sweep", Cw, 1.0, 0.2) for Cw in RA_SWEEP]
    cases += [("sweep", Cw, 30.0, 0.2) for Cw in RA_ONE_HOT_WIDTHS]
    cases += [("sweep", Cw, 1.0, slope) for Cw, slope in RA_SLOPE_CASES]
    cases += [(name, Cw, 1.0, 0.2) for name in sorted(ra_degenerate_graphs()) for Cw in RA_DEGENERATE_WIDTHS]
    return cases


RA_DEGENERATE_WIDTHS = (44, 13)
_RA_GRAPHS = {}


def ra_graph(name):
    """(n, node_type, edge_index) of 'sweep' or of a degenerate graph, built once."""
    if not _RA_GRAPHS:
        _RA_GRAPHS.update(ra_degenerate_graphs(), sweep=ra_sweep_graph())
    return _RA_GRAPHS[name]


def ra_stat_ref(sc, ei, nt, slope=0.2):
    """``stat`` [n, 3, 4] of wsi_ra_attn_fwd in float64: per (node, type) the largest score | log sum exp(score - largest) | the edge count
    | beta; an absent group is (+inf, 0, 0, 0)."""
    sc = sc.double()
    n = sc.shape[0]
    stat = torch.zeros(n, 3, 4, dtype=torch.float64)
    stat[:, :, 0] = math.inf
    s = F.leaky_relu(sc[ei[0], 0] + sc[ei[1], 1], slope)
    for v in range(n):
        at = ei[1] == v
        q = torch.full((3,), -math.inf, dtype=torch.float64)
        for t in range(3):
            grp = at & (nt[ei[0]] == t)
            k = int(grp.sum())
            if k:
                m = s[grp].max()
                stat[v, t, 0], stat[v, t, 1], stat[v, t, 2] = m, torch.log(torch.exp(s[grp] - m).sum()), k
                q[t] = F.leaky_relu(sc[ei[0][grp], 2].mean() + sc[v, 3], slope)
        if bool(at.any()):
            stat[v, :, 3] = torch.softmax(q, 0)
    return stat


# ------------------------------------------------------------------------------------------------ wsi_ihpool_assign: indices outside the tables
ASSIGN_TABLE, ASSIGN_LEAD, ASSIGN_ROWS = 100, 50, 200        # num_nodes, the rows of the buffer before xyf, the rows of the buffer


def _redraw_near_ties(xyf, tables, is_seed, g):
    """``assign_case``'s repair, in place: the rows of members that are no seeds and whose two nearest seeds are within MARGIN of
    equidistant are drawn again, at most 20 times."""
    for _ in range(20):
        gaps = assign_ref(xyf, *tables)[1]
        nodes = tables[0].long()
        again = nodes[(gaps < MARGIN) & ~is_seed[nodes]]
        if not len(again):
            return
        xyf[again] = torch.rand(len(again), 3, generator=g) * 2 - 1


ASSIGN_TILE_SEEDS = (128, 129)


def assign_tiles_case(seed):
    """Two segments of 200 members under 128 seeds (two full tiles of ihpool.hip's IH_TILE = 64) and under 129 (a third tile of one seed),
    over a table of 400 nodes; half of every segment's seeds, the last among them, are members too.  Returns ``assign_case``'s tuple."""
    g = torch.Generator().manual_seed(seed)
    total, m = 400, 200
    xyf = torch.rand(total, 3, generator=g) * 2 - 1
    member_node, member_seg, seed_ptr, seed_node = [], [], [0], []
    for s, k in enumerate(ASSIGN_TILE_SEEDS):
        nodes = torch.randperm(total, generator=g)
        mem = torch.cat([nodes[:k // 2 - 1], nodes[k - 1:k + m - k // 2]])
        member_node.append(mem[torch.randperm(m, generator=g)]); member_seg += [s] * m
        seed_node.append(nodes[:k]); seed_ptr.append(seed_ptr[-1] + k)
    tables = (torch.cat(member_node).to(torch.int32), torch.tensor(member_seg, dtype=torch.int32), torch.tensor(seed_ptr, dtype=torch.int32),
              torch.cat(seed_node).to(torch.int32))
    is_seed = torch.zeros(total, dtype=torch.bool)
    is_seed[tables[3].long()] = True
    _redraw_near_ties(xyf, tables, is_seed, g)
    return (xyf,) + tables


def assign_outside_case(seed):
    """A case whose index tables point outside the node table, in a buffer that reaches ASSIGN_LEAD rows before and
    ASSIGN_ROWS - ASSIGN_LEAD - ASSIGN_TABLE rows after it: every index used lies in [-ASSIGN_LEAD, ASSIGN_ROWS - ASSIGN_LEAD), so a kernel that
    followed one would still read allocated memory - and would be found out, because every outside SEED row holds the coordinates of a member
    of its segment (distance 0 if followed) and every outside MEMBER row those of a seed.  Segments (members may belong to several:
    member_node repeats nodes freely):
      0  40 members, 5 seeds, seeds 1 and 3 outside (one below, one above the table)
      1  30 members, 1 seed, outside: every member -1
      2  70 members over 65 seeds (a second tile of one seed), seed 64 - the second tile's only one - outside
      3  20 members, 3 seeds, members 2, 7 and 11 outside the table: -1
    before them 4 members of segment -1 and after them 10 of segments 4 and 5 = num_segs and num_segs + 1: -1.  Members that are no seeds whose two nearest seeds are within
    MARGIN of equidistant are drawn again.  Returns (buffer [ASSIGN_ROWS, 3] fp32, member_node, member_seg, seed_ptr, seed_node, want, the
    smallest gap): ``want`` is ``assign_ref`` on the cleaned case - outside seeds dropped, positions kept - with -1 for what must be
    ignored."""
    g = torch.Generator().manual_seed(seed)
    T, lead = ASSIGN_TABLE, ASSIGN_LEAD
    buf = torch.rand(ASSIGN_ROWS, 3, generator=g) * 2 - 1
    below = iter(range(-lead, 0))
    above = iter(range(T, ASSIGN_ROWS - lead))
    plan = ((40, 5, (1, 3), ()), (30, 1, (0,), ()), (70, 65, (64,), ()), (20, 3, (), (2, 7, 11)))
    member_node, member_seg, seed_ptr, seed_node, lures = [torch.randint(0, T, (4,), generator=g)], [-1] * 4, [0], [], []
    for s, (m, k, bad_seeds, bad_members) in enumerate(plan):
        nodes = torch.randperm(T, generator=g)
        seeds, rest = nodes[:k], nodes[k:]
        mem = torch.cat([seeds[:k // 2], rest[torch.randint(0, len(rest), (m - k // 2,), generator=g)]])     # half of the seeds are members too
        mem = mem[torch.randperm(m, generator=g)]
        for j, p in enumerate(bad_seeds):
            row = next(below) if j % 2 == 0 else next(above)
            lures.append((row, int(rest[j])))                    # rest[j]: a node of this segment's pool that is no seed of it
            mem[-1 - j] = rest[j]                                # ... and is a member
            seeds[p] = row
        for j, p in enumerate(bad_members):
            row = next(above) if j % 2 == 0 else next(below)
            lures.append((row, int(seeds[0])))
            mem[p] = row
        member_node.append(mem); member_seg += [s] * m
        seed_node.append(seeds); seed_ptr.append(seed_ptr[-1] + k)
    member_node.append(torch.randint(0, T, (10,), generator=g)); member_seg += [len(plan)] * 5 + [len(plan) + 1] * 5
    member_node, member_seg = torch.cat(member_node).to(torch.int32), torch.tensor(member_seg, dtype=torch.int32)
    seed_ptr, seed_node = torch.tensor(seed_ptr, dtype=torch.int32), torch.cat(seed_node).to(torch.int32)
    inside = lambda t: (t >= 0) & (t < T)
    keep = inside(seed_node)                                     # the cleaned case: outside seeds dropped, outside members and segments cut
    clean_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), keep.long().cumsum(0)])[seed_ptr.long()].to(torch.int32)
    position = torch.arange(seed_node.numel()) - torch.repeat_interleave(seed_ptr[:-1].long(), seed_ptr.long().diff())
    ok = inside(member_node) & (member_seg >= 0) & (member_seg < len(plan))
    xyf = buf[lead:lead + T]
    is_seed = torch.zeros(T, dtype=torch.bool)
    is_seed[seed_node[keep].long()] = True
    clean = (member_node[ok], member_seg[ok], clean_ptr, seed_node[keep])
    _redraw_near_ties(xyf, clean, is_seed, g)
    got, gaps = assign_ref(xyf, *clean)
    for row, node in lures:                                     # outside the table: the cleaned case does not see these rows
        buf[lead + row] = buf[lead + node]
    original = position[keep]                                   # position in the cleaned seed list -> position in the given one
    first = clean_ptr.long()[member_seg[ok].long()]
    want = torch.full((member_node.numel(),), -1, dtype=torch.int64)
    want[ok] = torch.where(got >= 0, original[(first + got.clamp(min=0)).clamp(max=max(original.numel() - 1, 0))], got)
    return buf, member_node, member_seg, seed_ptr, seed_node, want, float(gaps.min())
