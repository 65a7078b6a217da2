"""CPU checks of the GTNMIL baseline: the float64 restatement (tests/gtn_cases.py) against the fixture recorded from the reference's own
transformer, its dense padded form against its packed form (dropping the padding changes nothing), the batch conversion, the module
surface, and the argument errors of the new ops and C entry points - all without a GPU."""
import os

import numpy as np
import pytest
import torch

import gtn_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "gtn", "reference_vit.npz")
EINVAL, ENOSYS = -22, -38

VIT_KEYS = lambda depth: [f"blocks.{i}.{k}" for i in range(depth) for k in (
    "norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias",
    "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")] + ["norm.weight", "norm.bias", "head.weight", "head.bias"]


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


def test_restatement_reproduces_the_reference_transformer():
    f = np.load(FIXTURE)
    heads = int(f["config"][3])
    sd = {k[3:]: torch.from_numpy(f[k]).double().requires_grad_(True) for k in f.files if k.startswith("sd.")}
    x = torch.from_numpy(f["x"]).double().requires_grad_(True)
    out = C.vit_forward(sd, x, heads)
    (out * torch.from_numpy(f["w"])).sum().backward()
    assert _rel(out.detach(), torch.from_numpy(f["logits"])) <= 1e-10
    assert _rel(x.grad, torch.from_numpy(f["g.x"])) <= 1e-10
    names = [k[2:] for k in f.files if k.startswith("g.") and k != "g.x"]
    assert sorted(names) == sorted(sd)
    for k in names:
        assert _rel(sd[k].grad, torch.from_numpy(f["g." + k])) <= 1e-10, k


@pytest.mark.parametrize("train", [True, False])
def test_dense_padded_form_equals_the_packed_form(train):
    """Slides of 1, 40 and 129 nodes padded to 129: loss, logits, every parameter gradient and the BatchNorm batch statistics."""
    slides = C.slides_case((1, 40, 129), 48, seed=11)
    labels = torch.tensor([2, 0, 1])
    base = C.classifier_state(3, 48, 32, 10, 2, 4, seed=5)
    res = {}
    for dense in (True, False):
        sd = C.as_float64_leaves(base)
        r = C.classifier_forward(sd, slides, labels, 4, train=train, dense=dense)
        r["loss"].backward()
        res[dense] = (r, {k: v.grad for k, v in sd.items() if v.requires_grad})
    (rd, gd), (rp, gp) = res[True], res[False]
    for k in ("loss", "logits", "probs", "mincut", "ortho") + (("bn_mean", "bn_var") if train else ()):
        assert _rel(rd[k].detach(), rp[k].detach()) <= 1e-10, k
    assert set(gd) == set(gp) and len(gd) == len(base) - 3
    for k in gd:
        assert gd[k] is not None and float(gd[k].abs().max()) > 0, k
        assert _rel(gd[k], gp[k]) <= 1e-10, k


def test_mincut_sparse_restatement_equals_the_dense_formula():
    """gtn_cases.mincut_sparse (what the kernel tests compare against) against torch_geometric's dense definition on one weighted,
    non-symmetric slide with repeated entries."""
    gen = torch.Generator().manual_seed(3)
    n, K = 37, 6
    row, col = torch.randint(0, n, (150,), generator=gen), torch.randint(0, n, (150,), generator=gen)
    row[:10], col[:10] = row[10:20], col[10:20]                               # repeated entries
    w = torch.rand(150, generator=gen, dtype=torch.float64) + 0.1
    z = torch.randn(n, K, generator=gen, dtype=torch.float64)
    x = torch.randn(n, 5, generator=gen, dtype=torch.float64)
    s, t, num, den = C.mincut_sparse(z, row, col, w, [n])
    adj = C.dense_adjacency(n, row, col, w)
    out, out_adj, mc, ortho = C.mincut_dense(x[None], adj[None], z[None], torch.ones(1, n))
    assert _rel(-(num / den).mean(), mc) <= 1e-12
    assert _rel(s.t() @ x, out[0]) <= 1e-12
    raw = s.t() @ t
    raw.fill_diagonal_(0)
    d = torch.sqrt(raw.sum(-1))[None] + C.EPS
    assert _rel((raw / d.t()) / d, out_adj[0]) <= 1e-12


def test_from_dense_recovers_sizes_edges_and_weights():
    from wsi_hgnn_amd import gtn
    slides = C.slides_case((1, 7, 12), 5, seed=2)
    nmax = 12
    x = torch.zeros(3, nmax, 5)
    adj = torch.zeros(3, nmax, nmax)
    mask = torch.zeros(3, nmax)
    for b, (xb, row, col, w) in enumerate(slides):
        n = xb.shape[0]
        x[b, :n], mask[b, :n] = xb, 1.0
        adj[b, :n, :n] = C.dense_adjacency(n, row, col, w, torch.float32)
    gb = gtn.from_dense(x, adj, mask)
    assert gb.sizes == [1, 7, 12] and gb.num_graphs == 3 and gb.num_rows == 20
    assert torch.equal(gb.x, torch.cat([s[0] for s in slides]))
    off = 0
    for b, n in enumerate(gb.sizes):
        sel = (gb.row >= off) & (gb.row < off + n)
        assert bool(((gb.col[sel] >= off) & (gb.col[sel] < off + n)).all())
        back = C.dense_adjacency(n, gb.row[sel] - off, gb.col[sel] - off, gb.weight[sel], torch.float32)
        assert torch.equal(back, adj[b, :n, :n])
        off += n
    assert int(gb.row.numel()) == int((adj != 0).sum())
    with pytest.raises(ValueError, match="without rows"):
        gtn.from_dense(x, adj, torch.cat([mask[:2], torch.zeros(1, nmax)]))
    with pytest.raises(ValueError, match="without rows"):
        gtn.GraphBatch(torch.zeros(3, 2), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), None, [3, 0])


def test_a_graph_batch_converts_with_the_destination_as_the_row():
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import gtn, synthetic
    g = W.batch([synthetic.homogeneous_graph(9, 4, out_edges=2, seed=1), synthetic.homogeneous_graph(5, 4, out_edges=2, seed=2)])
    gb = gtn.as_batch(g)
    u, v = g.edges()
    assert gb.sizes == [9, 5] and torch.equal(gb.row, v) and torch.equal(gb.col, u) and gb.weight is None
    assert gtn.as_batch(g) is gb and gtn.as_batch(gb) is gb


def test_state_dict_keys_and_shapes():
    from wsi_hgnn_amd import gtn
    f = np.load(FIXTURE)
    n_class, E, depth, heads = (int(v) for v in f["config"])
    vit = gtn.VisionTransformer(num_classes=n_class, embed_dim=E, depth=depth, num_heads=heads)
    assert list(vit.state_dict()) == [str(k) for k in f["keys"]] == VIT_KEYS(depth)
    for k, v in vit.state_dict().items():
        assert tuple(v.shape) == f["sd." + k].shape, k
    vit.load_state_dict({k: torch.from_numpy(f["sd." + k]) for k in vit.state_dict()}, strict=True)
    m = gtn.Classifier(2)
    sd = m.state_dict()
    want = {"cls_token": (1, 1, 64), "conv1.weight": (1024, 64), "conv1.bias": (64,), "conv1.bn_layer.weight": (64,), "conv1.bn_layer.bias": (64,),
            "conv1.bn_layer.running_mean": (64,), "conv1.bn_layer.running_var": (64,), "conv1.bn_layer.num_batches_tracked": (),
            "pool1.weight": (100, 64), "pool1.bias": (100,)}
    want.update({"transformer." + k: None for k in VIT_KEYS(3)})
    assert set(sd) == set(want)
    for k, shape in want.items():
        assert shape is None or tuple(sd[k].shape) == shape, k
    assert tuple(sd["transformer.blocks.2.attn.qkv.weight"].shape) == (192, 64) and tuple(sd["transformer.blocks.0.mlp.fc1.weight"].shape) == (128, 64)
    assert tuple(sd["transformer.head.weight"].shape) == (2, 64)
    assert set(gtn.Classifier(2, kernels=False).state_dict()) == set(sd)
    assert set(C.classifier_state(3, 48, 32, 10, 2, 4, seed=0)) == set(gtn.Classifier(3, 48, 32, 10, 2, 4).state_dict())
    import inspect
    assert list(inspect.signature(gtn.GCNBlock.__init__).parameters)[1:9] == ["input_dim", "output_dim", "bn", "add_self", "normalize_embedding",
                                                                             "dropout", "relu", "bias"]
    assert list(inspect.signature(gtn.VisionTransformer.__init__).parameters)[1:8] == ["num_classes", "embed_dim", "depth", "num_heads", "mlp_ratio",
                                                                                      "qkv_bias", "mlp_head"]


def test_tensor_operation_path_matches_the_restatement_on_the_cpu():
    """``Classifier(kernels=False)`` is plain tensor operations: in float64 on the CPU it is the restatement to rounding."""
    from wsi_hgnn_amd import gtn
    slides = C.slides_case((1, 40, 129), 48, seed=11)
    labels = torch.tensor([2, 0, 1])
    base = C.classifier_state(3, 48, 32, 10, 2, 4, seed=5)
    m = gtn.Classifier(3, 48, 32, 10, 2, 4, kernels=False).double()
    m.load_state_dict({k: (v.double() if v.dtype.is_floating_point else v) for k, v in base.items()}, strict=True)
    off = np.concatenate([[0], np.cumsum([s[0].shape[0] for s in slides])])
    gb = gtn.GraphBatch(torch.cat([s[0] for s in slides]), torch.cat([s[1] + int(o) for s, o in zip(slides, off)]),
                        torch.cat([s[2] + int(o) for s, o in zip(slides, off)]), torch.cat([s[3] for s in slides]), [1, 40, 129])
    gb.x = gb.x.double()
    m.train()
    pred, lab, loss, probs = m(gb, labels)
    loss.backward()
    sd = C.as_float64_leaves(base)
    r = C.classifier_forward(sd, slides, labels, 4, train=True)
    r["loss"].backward()
    assert _rel(loss.detach(), r["loss"].detach()) <= 1e-9 and _rel(probs.detach(), r["probs"].detach()) <= 1e-9
    assert torch.equal(pred, r["logits"].argmax(1)) and lab is labels
    for k, p in m.named_parameters():
        assert _rel(p.grad, sd[k].grad) <= 1e-8, k


def test_new_ops_refuse_cpu_tensors():
    from wsi_hgnn_amd import ops
    n, K = 6, 3
    row, col = torch.tensor([0, 1, 2, 3, 4, 5]), torch.tensor([1, 2, 3, 4, 5, 0])
    ec = ops.EdgeCSR(row, col, n)
    rp = ops.ReducePlan.from_ptr([0, 6], torch.device("cpu"))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.mincut_assign(torch.randn(n, K), ec, rp)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.seq_attention(torch.randn(2, 5, 3 * 2 * 8), 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.mincut_pool_products(torch.randn(n, K), torch.randn(n, 4), rp)
    assert ops.seq_attention_supported(101, 8) and ops.seq_attention_supported(128, 16) and ops.seq_attention_supported(1, 8)
    assert not ops.seq_attention_supported(129, 8) and not ops.seq_attention_supported(64, 32) and not ops.seq_attention_supported(0, 8)


def test_c_entry_points_answer_bad_arguments_without_a_gpu():
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    err = lambda: lib.wsi_last_error().decode()
    nul = [None] * 6
    # mincut: null pointers, negative sizes, more than 128 columns - all answered before any GPU call
    fwd = lambda n, K, chunks, segs, ldz=None: lib.wsi_mincut_fwd(None, K if ldz is None else ldz, n, K, None, None, None, None, chunks, None, segs, *nul, None)
    assert fwd(5, 4, 1, 1) == EINVAL and "null pointer" in err()
    assert fwd(-1, 4, 1, 1) == EINVAL and fwd(5, 0, 1, 1) == EINVAL and fwd(5, 4, -1, 1) == EINVAL and fwd(5, 4, 1, 1, ldz=3) == EINVAL
    assert fwd(5, 129, 1, 1) == ENOSYS and "129" in err()
    assert fwd(5, 128, 1, 1) == EINVAL and fwd(0, 4, 0, 0) == 0
    bwd = lambda n, K, chunks: lib.wsi_mincut_bwd(None, 0, None, None, None, None, None, n, K, None, None, None, None, None, chunks, None, None)
    assert bwd(5, 4, 1) == EINVAL and "null pointer" in err()
    assert bwd(5, 129, 1) == ENOSYS and bwd(-2, 4, 1) == EINVAL and bwd(5, 4, 0) == 0
    assert lib.wsi_mincut_partials(0) == 0 and lib.wsi_mincut_partials(-3) == 0
    assert lib.wsi_mincut_partials(100) == 2 * 100 * 8 and lib.wsi_mincut_partials(1000) == 2 * 1000 * 2 and lib.wsi_mincut_partials(5000) == 2 * 5000
    # attention: the compiled range is 1 <= n <= 128, d in {8, 16}
    af = lambda B, n, H, d: lib.wsi_seq_attn_fwd(None, B, n, H, d, 1.0, None, None, None)
    ab = lambda B, n, H, d: lib.wsi_seq_attn_bwd(None, None, None, B, n, H, d, 1.0, None, None)
    for f in (af, ab):
        assert f(2, 101, 8, 8) == EINVAL and "null pointer" in err()
        assert f(2, 129, 8, 8) == ENOSYS and "129" in err()
        assert f(2, 101, 8, 32) == ENOSYS and f(2, 101, 8, 4) == ENOSYS
        assert f(-1, 101, 8, 8) == EINVAL and f(2, -5, 8, 8) == EINVAL and f(2, 101, 0, 8) == EINVAL
        assert f(0, 101, 8, 8) == 0 and f(2, 0, 8, 8) == 0
