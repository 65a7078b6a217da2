"""What the GTNMIL slot tests share (tests/test_gtn_slot.py on the CPU, tests/test_gtn_slot_kernels_gpu.py and tests/test_gtn_slot_gpu.py on
the GPU): seeded slides whose entries come in no particular order, a host-loop restatement of the tables ``gtn.GraphSlot.load`` writes, the
float64 reference of the model on the UNPADDED slides (``gtn_cases.classifier_forward``) and a float64 masked BatchNorm."""
import torch
import torch.nn.functional as F

import gtn_cases as C

SMALL = dict(n_class=3, in_feats=48, embed_dim=32, node_cluster_num=10, depth=2, num_heads=4)
TABLE_CELLS, TABLE_CELL_ROWS = 3, 140
TABLE_SIZES = (129, 140)                 # one slide short of its cell, one that fills it exactly; the third cell stays unused


def shuffled_slides(sizes, feats, seed, weighted):
    """``gtn_cases.slides_case`` slides (``weighted``: one flag per slide) with 20 repeated entries each and the entry lists permuted, so that
    the stable sorts of ``ops.EdgeCSR`` have something to do."""
    out = []
    for k, (n, wt) in enumerate(zip(sizes, weighted)):
        x, row, col, w = C.slides_case((n,), feats, seed + 7 * k, weighted=wt)[0]
        gen = torch.Generator().manual_seed(seed + 7 * k + 3)
        rep = torch.randint(0, row.shape[0], (min(20, row.shape[0]),), generator=gen)
        row, col = torch.cat([row, row[rep]]), torch.cat([col, col[rep]])
        if w is not None:
            w = torch.cat([w, w[rep]])
        perm = torch.randperm(row.shape[0], generator=gen)
        out.append((x, row[perm], col[perm], None if w is None else w[perm]))
    return out


def table_slides(feats=12, seed=900):
    return shuffled_slides(TABLE_SIZES, feats, seed, (True, False))


def with_unit_weights(slides):
    """The slides with a weight of 1 where they have none (``classifier_forward`` takes all weighted or all unweighted)."""
    return [(x, r, c, torch.ones(r.shape[0], dtype=torch.float32) if w is None else w) for x, r, c, w in slides]


def host_tables(slides, labels, cells, cell_rows):
    """The tables of a slot holding ``slides`` (slide i in cell i) by plain host loops over Python lists: dict of lists.  Entry arrays hold the
    batch's entries only (what lies behind them in a slot is never referenced)."""
    R = cells * cell_rows
    x = [[0.0] * slides[0][0].shape[1] for _ in range(R)]
    live, cell_live, lab = [0.0] * R, [0.0] * cells, [-100] * cells
    rowptr, colptr = [0] * (R + 1), [0] * (R + 1)
    src, edge_w, csc_dst, edge_w_csc = [], [], [], []
    e0 = 0
    for g, (xs, row, col, w) in enumerate(slides):
        n, base = xs.shape[0], g * cell_rows
        ents = [(int(r), int(c), 1.0 if w is None else float(w[k])) for k, (r, c) in enumerate(zip(row.tolist(), col.tolist()))]
        csr = sorted(ents, key=lambda t: t[0])                  # (Python's sort is stable: within a row the original order)
        csc = sorted(csr, key=lambda t: t[1])                   # (within a column the CSR order)
        for j in range(n):
            x[base + j] = xs[j].tolist()
            live[base + j] = 1.0
            rowptr[base + j] = e0 + sum(1 for t in csr if t[0] < j)
            colptr[base + j] = e0 + sum(1 for t in csc if t[1] < j)
        for j in range(n, cell_rows):
            rowptr[base + j] = colptr[base + j] = e0 + len(ents)
        src += [t[1] + base for t in csr]
        edge_w += [t[2] for t in csr]
        csc_dst += [t[0] + base for t in csc]
        edge_w_csc += [t[2] for t in csc]
        cell_live[g], lab[g] = 1.0, int(labels[g])
        e0 += len(ents)
    for r in range(len(slides) * cell_rows, R + 1):
        rowptr[r] = colptr[r] = e0
    total = sum(s[0].shape[0] for s in slides)
    return dict(x=x, live=live, cell_live=cell_live, labels=lab, rowptr=rowptr, colptr=colptr, src=src, edge_w=edge_w, csc_dst=csc_dst,
                edge_w_csc=edge_w_csc, inv_cells=[float(torch.tensor(1.0 / len(slides), dtype=torch.float32))], live_rows=[float(total)])


def slot_tables(slot):
    """The slot's tables on the CPU, entry arrays cut to the loaded batch's entries."""
    E, ec = slot.num_entries, slot.ec
    cpu = lambda t: t.detach().cpu().clone()
    return dict(x=cpu(slot.x), live=cpu(slot.live), cell_live=cpu(slot.cell_live), labels=cpu(slot.labels), rowptr=cpu(ec.rowptr),
                colptr=cpu(ec.colptr), src=cpu(ec.src[:E]), edge_w=cpu(ec.edge_w[:E]), csc_dst=cpu(ec.csc_dst[:E]),
                edge_w_csc=cpu(ec.edge_w_csc[:E]), inv_cells=cpu(slot.inv_cells), live_rows=cpu(slot.live_rows))


def assert_tables_equal(got, want, what=""):
    """Bit for bit: integers and copied floats."""
    assert set(got) == set(want)
    for k in want:
        a = got[k]
        b = torch.as_tensor(want[k], dtype=a.dtype) if not isinstance(want[k], torch.Tensor) else want[k]
        assert a.shape == b.shape, f"{what} {k}: shape {tuple(a.shape)} against {tuple(b.shape)}"
        assert torch.equal(a, b), f"{what} {k}: {int((a != b).sum())} entries differ"


def model_case(sizes, weighted, seed, cfg=SMALL):
    """(slides, labels, float32 state dict) of a seeded model-level case."""
    slides = shuffled_slides(sizes, cfg["in_feats"], seed, weighted)
    labels = [(2 * i + 1) % cfg["n_class"] for i in range(len(sizes))]
    base = C.classifier_state(cfg["n_class"], cfg["in_feats"], cfg["embed_dim"], cfg["node_cluster_num"], cfg["depth"], cfg["num_heads"], seed=seed + 1)
    return slides, labels, base


def reference(slides, labels, base, train, cfg=SMALL):
    """float64 on the unpadded slides: (result dict of ``gtn_cases.classifier_forward`` after ``backward``, the float64 leaves)."""
    sd = C.as_float64_leaves(base)
    ref = C.classifier_forward(sd, with_unit_weights(slides), torch.tensor(labels), cfg["num_heads"], train=train)
    ref["loss"].backward()
    return ref, sd


def build_model(gtn, cfg, base, dev, **kw):
    m = gtn.Classifier(cfg["n_class"], cfg["in_feats"], cfg["embed_dim"], cfg["node_cluster_num"], cfg["depth"], cfg["num_heads"], **kw)
    m.load_state_dict(base, strict=True)
    return m.to(dev)


def run_on_slot(m, slot, train):
    """(loss, logits [cells, n_class]) of the model on a loaded slot, after ``backward``."""
    m.train(train)
    seen = []
    hook = m.transformer.register_forward_hook(lambda _m, _i, out: seen.append(out))
    try:
        _, _, loss, _ = m(slot, None)
    finally:
        hook.remove()
    loss.backward()
    return loss, seen[-1]


def check_against_reference(R, m, loss, logits, ref, sd, base, B, train, case):
    """Loss, logits of the real cells, every parameter gradient and the BatchNorm buffers against the float64 reference."""
    R.check(loss.reshape(1), ref["loss"].reshape(1), "loss", case)
    R.check(logits[:B], ref["logits"], "logits", case)
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        R.check(p.grad, sd[k].grad, "g_param", f"{case} {k}")
    state = m.state_dict()
    rm, rv = state["conv1.bn_layer.running_mean"], state["conv1.bn_layer.running_var"]
    if train:
        R.check(rm, 0.9 * sd["conv1.bn_layer.running_mean"] + 0.1 * ref["bn_mean"], "running_mean", case)
        R.check(rv, 0.9 * sd["conv1.bn_layer.running_var"] + 0.1 * ref["bn_var"], "running_var", case)
        assert int(state["conv1.bn_layer.num_batches_tracked"]) == 1
    else:
        assert torch.equal(rm.cpu(), base["conv1.bn_layer.running_mean"]) and torch.equal(rv.cpu(), base["conv1.bn_layer.running_var"])
        assert int(state["conv1.bn_layer.num_batches_tracked"]) == 0


# ------------------------------------------------------------------------------------------------ masked BatchNorm
def live_mask(cells, cell_rows, live_per_cell):
    """[cells * cell_rows] fp32: the first ``live_per_cell[g]`` rows of cell g are live."""
    m = torch.zeros(cells * cell_rows, dtype=torch.float32)
    for g, n in enumerate(live_per_cell):
        m[g * cell_rows:g * cell_rows + n] = 1.0
    return m


def masked_bn_reference(y, live, gamma, beta, rm, rv, train, g_out, momentum=0.1, eps=1e-5):
    """float64 ``F.batch_norm`` over the live rows ALONE, scattered back: dict of out, g_y, g_gamma, g_beta, running_mean, running_var."""
    idx = live.nonzero().flatten()
    y64 = y.detach().to(torch.float64).requires_grad_(True)
    g64, b64 = gamma.detach().to(torch.float64).requires_grad_(True), beta.detach().to(torch.float64).requires_grad_(True)
    rm64, rv64 = rm.detach().to(torch.float64).clone(), rv.detach().to(torch.float64).clone()
    o = F.batch_norm(y64[idx], rm64, rv64, g64, b64, train, momentum, eps)
    out = torch.zeros_like(y64).index_copy(0, idx, o)
    (out * g_out.to(torch.float64)).sum().backward()
    return dict(out=out.detach(), g_y=y64.grad, g_gamma=g64.grad, g_beta=b64.grad, running_mean=rm64, running_var=rv64)
