"""GAT without a GPU: the parser branch against the calls the reference's parser.py:51-68 makes, the module surface (parameter
order, state_dict keys and shapes, dead parameters) at the GAT_Kimia_v2 shape, the refused residual form, and the argument checks
of the new C-ABI entry points (they return before any HIP call)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import row_group_cases as R

# configs/COAD/GAT_Kimia_v2.yml, GAT_COAD.yml and GAT_Hover_v2.yml: their ``GNN:`` blocks, inlined
KIMIA_V2 = {"name": "GAT", "negative_slope": 0.2, "num_layers": 2, "in_dim": 1024, "hidden_dim": 512, "residual": True, "in_drop": 0.2,
            "attn_drop": 0.2, "out_dim": 2, "num_heads": 4, "num_out_heads": 1, "feat_drop": 0.2, "graph_pooling_type": "mean"}
NO_POOLING = {"name": "GAT", "negative_slope": 0.2, "num_layers": 2, "in_dim": 1024, "hidden_dim": 8, "residual": True, "in_drop": 0.2,
              "attn_drop": 0.2, "out_dim": 2, "num_heads": 4, "num_out_heads": 1, "feat_drop": 0.2}


class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return "GAT"


def test_parser_makes_the_reference_gat_call(monkeypatch):
    from wsi_hgnn_amd import parser as P
    rec = _Recorder()
    monkeypatch.setattr(P, "GAT", rec)
    assert P.parse_gnn_model(dict(KIMIA_V2)) == "GAT"
    assert rec.calls == [((), dict(n_layers=2, in_dim=1024, hidden_dim=512, out_dim=2, heads=[4, 4, 1], activation=F.leaky_relu,
                                   feat_drop=0.2, attn_drop=0.2, negative_slope=0.2, residual=False, graph_pooling_type="mean"))]


@pytest.mark.parametrize("config", ["GAT_COAD", "GAT_Hover_v2"])
def test_parser_configs_without_pooling_raise_the_reference_keyerror(config, monkeypatch):
    from wsi_hgnn_amd import parser as P
    rec = _Recorder()
    monkeypatch.setattr(P, "GAT", rec)
    with pytest.raises(KeyError) as ei:
        P.parse_gnn_model(dict(NO_POOLING))
    assert str(ei.value) == str(KeyError("graph_pooling_type"))
    assert rec.calls == []


def test_parser_missing_key_is_keyerror_and_notimplementederror():
    from wsi_hgnn_amd import models, parser as P
    with pytest.raises(KeyError) as ei:
        models.from_config({"name": "GAT"})
    assert isinstance(ei.value, NotImplementedError)
    assert str(ei.value) == str(KeyError("num_layers"))
    cfg = dict(KIMIA_V2)
    del cfg["num_out_heads"]
    with pytest.raises(P.MissingGATKey) as ei:
        P.parse_gnn_model(cfg)
    assert str(ei.value) == str(KeyError("num_out_heads"))
    with pytest.raises(NotImplementedError):
        models.from_config({"name": "GIN"})


def test_module_surface_at_gat_kimia_v2():
    from wsi_hgnn_amd import models
    torch.manual_seed(0)
    m = models.from_config(dict(KIMIA_V2))
    assert type(m).__name__ == "GAT" and m.n_layers == 2
    names = [n for n, _ in m.named_parameters()]
    want = []
    for l, (fin, H, D) in enumerate([(1024, 4, 512), (2048, 4, 512), (2048, 1, 2)]):
        want += [f"layers.{l}.attn_l", f"layers.{l}.attn_r", f"layers.{l}.bias", f"layers.{l}.fc.weight"]
    want += [f"linears_prediction.{l}.{p}" for l in range(3) for p in ("weight", "bias")]
    assert names == want
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert list(shapes) == want
    for l, (fin, H, D) in enumerate([(1024, 4, 512), (2048, 4, 512), (2048, 1, 2)]):
        assert shapes[f"layers.{l}.fc.weight"] == (H * D, fin)
        assert shapes[f"layers.{l}.attn_l"] == shapes[f"layers.{l}.attn_r"] == (1, H, D)
        assert shapes[f"layers.{l}.bias"] == (H * D,)
        assert float(m.state_dict()[f"layers.{l}.bias"].abs().max()) == 0.0
    for l, fin in enumerate([1024, 2048, 2048]):
        assert shapes[f"linears_prediction.{l}.weight"] == (2, fin)
    assert m.dead_parameter_names() == ["layers.2.attn_l", "layers.2.attn_r", "layers.2.bias", "layers.2.fc.weight"]
    # xavier_normal_ with gain calculate_gain('relu'): std = sqrt(2) * sqrt(2 / (fan_in + fan_out))
    w = m.layers[0].fc.weight
    std = (2.0 ** 0.5) * (2.0 / (1024 + 2048)) ** 0.5
    assert abs(float(w.std()) / std - 1.0) < 0.02


def test_att_pooling_widths():
    from wsi_hgnn_amd.models import GAT
    m = GAT(2, 16, 8, 3, [2, 3, 1], F.leaky_relu, 0.0, 0.0, 0.2, False, "att")
    assert [tuple(p.gate_nn.weight.shape) for p in m.pools] == [(1, 16), (1, 16), (1, 24)]
    assert [tuple(l.weight.shape) for l in m.linears_prediction] == [(3, 16), (3, 16), (3, 24)]


def test_residual_is_refused():
    from wsi_hgnn_amd.models import GAT
    from wsi_hgnn_amd.models.GAT import GATConv
    with pytest.raises(NotImplementedError, match="residual"):
        GATConv(8, 4, 2, residual=True)
    with pytest.raises(NotImplementedError, match="residual"):
        GAT(2, 8, 4, 2, [2, 2, 1], F.leaky_relu, 0.0, 0.0, 0.2, True, "mean")


def _lib():
    import __graft_entry__
    __graft_entry__.build()
    from wsi_hgnn_amd import _native
    return _native.load()


# a fake device address: every call below must fail its argument check before touching it
P = ctypes.c_void_p(1 << 40)
EINVAL = -22


@pytest.mark.parametrize("H,D", [(0, 8), (17, 8), (1, 0), (4, 1025), (16, 257), (-1, 4)])
def test_capi_rejects_bad_heads_and_widths(H, D):
    lib = _lib()
    assert lib.wsi_gat_scores(P, 4096, 10, H, D, P, P, P, None) == EINVAL
    assert lib.wsi_gat_attn_fwd(P, 4096, P, 10, H, D, P, P, None, 0.2, 0, None, 0, 1.0, None, 0, 0.01, P, 4096, P, None) == EINVAL
    assert lib.wsi_gat_attn_bwd_workspace_bytes(10, 20, H, D, 0) == -1
    assert lib.wsi_gat_attn_bwd(P, 4096, P, P, P, 4096, P, 4096, 10, 20, H, D, P, P, P, P, P, None, P, P, 0.2, 0, None, 0, 1.0, 0, 0.01,
                                P, 1 << 30, P, 4096, P, P, None, None) == EINVAL
    assert "bad shape" in lib.wsi_last_error().decode()


def test_capi_rejects_null_pointers_strides_and_modes():
    lib = _lib()
    H, D = 4, 8
    assert lib.wsi_gat_scores(None, 32, 10, H, D, P, P, P, None) == EINVAL
    assert lib.wsi_gat_scores(P, 31, 10, H, D, P, P, P, None) == EINVAL
    fwd = lambda **kw: lib.wsi_gat_attn_fwd(kw.get("ft", P), kw.get("ld", 32), P, 10, H, D, kw.get("rowptr", P), P, None, 0.2, 0, None,
                                            kw.get("thr", 0), 1.0, None, kw.get("act", 0), 0.01, kw.get("out", P), 32, P, None)
    assert fwd(ft=None) == EINVAL
    assert fwd(rowptr=None) == EINVAL
    assert fwd(out=None) == EINVAL
    assert fwd(ld=16) == EINVAL
    assert fwd(act=3) == EINVAL
    assert fwd(thr=65536) == EINVAL
    ws = lib.wsi_gat_attn_bwd_workspace_bytes(10, 20, H, D, 2)
    assert ws > 0

    def bwd(**kw):
        return lib.wsi_gat_attn_bwd(P, 32, P, P, kw.get("out", P), 32, kw.get("g_out", P), 32, 10, kw.get("E", 20), H, D, P, P, P, P, P, None,
                                    P, P, 0.2, 0, None, 0, 1.0, kw.get("act", 2), 0.01, kw.get("ws", P), kw.get("ws_bytes", ws),
                                    kw.get("g_ft", P), 32, P, P, None, None)
    assert bwd(g_out=None) == EINVAL
    assert bwd(g_ft=None) == EINVAL
    assert bwd(out=None) == EINVAL                  # read for the activation's derivative
    assert bwd(ws=None) == EINVAL
    assert bwd(E=-1) == EINVAL
    assert bwd(act=-1) == EINVAL
    assert bwd(ws_bytes=ws - 1) == -12              # WSI_ENOMEM: workspace too small


def test_capi_rejects_a_misaligned_workspace():
    """g_rst and the column partials are carved out of the workspace and take the 16-byte accesses of the vector-4 kernels: a workspace
    that is not 16-byte aligned is refused before anything is launched (the contract in include/wsi_hgnn.h)."""
    lib = _lib()
    H, D = 4, 8
    ws = lib.wsi_gat_attn_bwd_workspace_bytes(10, 20, H, D, 2)
    for off in (4, 8, 12, 1):                       # offset 0 would pass the check and launch on the fake address: only refusals are made
        w = ctypes.c_void_p((1 << 40) + off)
        assert lib.wsi_gat_attn_bwd(P, 32, P, P, P, 32, P, 32, 10, 20, H, D, P, P, P, P, P, None, P, P, 0.2, 0, None, 0, 1.0, 2, 0.01,
                                    w, ws + 16, P, 32, P, P, None, None) == EINVAL
        assert "16-byte aligned" in lib.wsi_last_error().decode()
        assert lib.wsi_gat_attn_bwd_scaled(P, 32, P, P, P, 32, P, 32, 10, 20, H, D, P, P, P, P, P, None, P, P, 0.2, 0, None, 0, 1.0, 2, 0.01,
                                           P, w, ws + 16, P, 32, P, P, None, P, None) == EINVAL
        assert "16-byte aligned" in lib.wsi_last_error().decode()


# ---------------------------------------------------------------------------------------------------- dispatch coverage
# Every (heads, width, fused activation) the kernel sweep of tests/test_gat_kernels_gpu.py runs, and every width its wsi_sddmm_dot sweep
# runs next to those of tests/test_gnn_explainer_gpu.py.  The lists live here so that the test below, which needs no GPU, sees them.
GA_SWEEP = [(4, 4, None), (8, 4, "relu"), (16, 4, "leaky_relu"), (5, 24, "relu"), (2, 100, "leaky_relu"), (6, 64, None),
            (3, 300, "relu"), (7, 260, "leaky_relu"), (16, 256, "leaky_relu"), (5, 500, "relu"),
            (4, 1, "leaky_relu"), (2, 3, "relu"), (8, 1, None), (16, 1, "relu"), (3, 10, "leaky_relu"), (7, 9, None), (5, 25, "relu"),
            (3, 67, "leaky_relu"), (2, 250, None), (1, 1001, "relu"), (11, 150, "leaky_relu"), (16, 255, "relu")]
SDDMM_WIDTHS = [16, 28, 60, 120, 200, 7, 13, 30, 63, 125, 201, 501, 1001]
SDDMM_WIDTHS_ELSEWHERE = [1, 3, 40, 64, 512, 1000]            # test_gnn_explainer_gpu.py: the aggregate's widths and the direct call's


def ga_cfg(H, D, vec4_ok=True):
    """The dispatch code of csrc/gat_attn.hip's call of row_cfg: VEC * 100000 + G * 100 + NK."""
    return R.code(*R.row_cfg(H * D, D, H, vec4_ok))


def ga_group(H, D, vec4_ok=True):
    return ga_cfg(H, D, vec4_ok) // 100 % 1000


def test_sweeps_reach_every_dispatch_code():
    codes = R.family_codes("gat_attn.hip")
    assert len(codes) == len(set(codes)) == 20 and codes == sorted(sum(R.case_lists(), []))
    reached = {}
    for H, D, _ in GA_SWEEP:
        reached.setdefault(ga_cfg(H, D), []).append((H, D))
    assert sorted(reached) == codes, f"not reached: {sorted(set(codes) - set(reached))}; unknown: {sorted(set(reached) - set(codes))}"
    assert len(set(GA_SWEEP)) == len(GA_SWEEP)
    # the cases the sweep is there for: heads == lanes of a group in both families, the full width, ragged last chunks, every activation
    for H in (8, 16):
        assert any(h == H and ga_group(h, d) == H and d % 4 == 0 for h, d, _ in GA_SWEEP)
        assert any(h == H and ga_group(h, d) == H and d % 4 != 0 for h, d, _ in GA_SWEEP)
    assert any(h * d == 4096 for h, d, _ in GA_SWEEP) and any(ga_cfg(h, d) == 406416 and h * d < 4096 for h, d, _ in GA_SWEEP)
    assert any(ga_cfg(h, d) == 100801 and h < 8 for h, d, _ in GA_SWEEP)
    for vec4 in (True, False):
        acts = {a for h, d, a in GA_SWEEP if (d % 4 == 0) == vec4}
        assert acts == {None, "relu", "leaky_relu"}
    # wsi_sddmm_dot: every code ga_cfg(1, D) produces for a legal width
    want = {ga_cfg(1, D) for D in range(1, 1025)}
    assert want <= set(codes)
    got = {ga_cfg(1, D) for D in SDDMM_WIDTHS + SDDMM_WIDTHS_ELSEWHERE}
    assert got == want, f"wsi_sddmm_dot codes not reached: {sorted(want - got)}"
    assert len({ga_cfg(1, D) for D in SDDMM_WIDTHS}) == len(SDDMM_WIDTHS)          # no width of the new list repeats another's kernel
