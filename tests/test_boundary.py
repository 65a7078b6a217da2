"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/wsi_hgnn.h declares (no compute call without a GPU), the product never touches the oracle,
the nn.Module surface matches the reference's constructor signatures / state_dict keys, and the ops
refuse CPU tensors loudly instead of falling back."""
import ctypes
import inspect
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "wsi-hgnn_amd")


def _native_built():
    import __graft_entry__
    __graft_entry__.build()
    from wsi_hgnn_amd import _native
    return _native


def _gcc(source, *flags, run=False, extra=None):
    """Compile ``source`` (C, sees include/) with gcc; ``run``: link it, run it and return the integers it prints."""
    import subprocess, tempfile
    with tempfile.TemporaryDirectory() as td:
        for name, text in {"t.c": source, **(extra or {})}.items():
            open(os.path.join(td, name), "w").write(text)
        cmd = ["gcc", "-I", td, "-I", os.path.join(ROOT, "include"), *flags, os.path.join(td, "t.c")]
        if not run:
            return subprocess.run(cmd + ["-fsyntax-only"], capture_output=True, text=True)
        subprocess.check_call(cmd + ["-o", os.path.join(td, "t")])
        return [int(x) for x in subprocess.check_output([os.path.join(td, "t")]).split()]


def test_library_exports_every_declared_symbol():
    _native = _native_built()
    header = open(os.path.join(ROOT, "include", "wsi_hgnn.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(wsi_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/wsi_hgnn.h but not exported"
    assert declared == set(_native.EXPORTS), (declared ^ set(_native.EXPORTS))     # (two readings of one file: the C compiler's are below)
    assert _native.load().wsi_abi_version() == _native.WSI_ABI_VERSION


def test_struct_layouts_agree_with_the_header():
    """Every struct the binding derives from include/wsi_hgnn.h (all five today; one added later is covered as it appears) against the C
    compiler's sizeof / offsetof of the same header, and the public class names the host code uses."""
    _native = _native_built()
    assert {c: t.__name__ for c, t in _native.STRUCTS.items()} == {
        "wsi_attn_pool_t": "AttnPool", "wsi_gemm_group_t": "GemmGroup", "wsi_adam_tensor_t": "AdamTensor",
        "wsi_optim_tensor_t": "OptimTensor", "wsi_optim_hyper_t": "OptimHyper"}
    assert [len(_native.STRUCTS[c]._fields_) for c in ("wsi_attn_pool_t", "wsi_gemm_group_t", "wsi_adam_tensor_t", "wsi_optim_tensor_t",
                                                       "wsi_optim_hyper_t")] == [16, 43, 5, 8, 11]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "wsi_hgnn.h"\nint main(void){'
    for cname, ctype in _native.STRUCTS.items():
        assert getattr(_native, ctype.__name__) is ctype
        src += 'printf("%%zu", sizeof(%s));' % cname + "".join('printf(" %%zu", offsetof(%s, %s));' % (cname, f) for f, _ in ctype._fields_)
        src += 'printf("\\n");'
    nums = _gcc(src + "return 0;}", run=True)
    for cname, ctype in _native.STRUCTS.items():
        fields = [f for f, _ in ctype._fields_]
        mine, nums = nums[:1 + len(fields)], nums[1 + len(fields):]
        assert mine[0] == ctypes.sizeof(ctype), cname
        assert mine[1:] == [getattr(ctype, f).offset for f in fields], cname
    assert not nums


_C_SPELLING = {ctypes.c_void_p: "void*", ctypes.c_int64: "int64_t", ctypes.c_int32: "int32_t", ctypes.c_uint32: "uint32_t",
               ctypes.c_float: "float", ctypes.c_double: "double", ctypes.c_int: "int", ctypes.c_char_p: "const char*", None: "void"}


def _prototype_check(exports):
    """One C file with, for every entry, a function-pointer variable whose type is spelled from the derived ctypes signature and which is
    initialised with the address of the declared function: gcc refuses a difference in the number, the order, the class (integer / floating /
    pointer) or the width of any argument or of the result.  C has no initialisation that forgives only WHAT a pointer points to, so the
    file includes the header with every pointer type but ``const char*`` rewritten to ``void*`` (one substitution outside the preprocessor
    lines; it can turn no scalar into a pointer and change no width) - which is all the binding claims of a pointer."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wsi_hgnn.h")).read(), flags=re.S)
    erased = "\n".join(ln if ln.lstrip().startswith("#") else re.sub(r"(?:\bconst\s+)?\b(?!char\b)\w+(?:\s*\*(?:\s*const\b)?)+", "void* ", ln)
                       for ln in header.split("\n"))
    assert "float*" not in erased.replace(" ", "") and "const char*" in erased
    src = '#include "erased.h"\n' + "".join("%s (*p_%s)(%s) = &%s;\n" % (_C_SPELLING[res], name, ", ".join(_C_SPELLING[a] for a in args) or "void", name)
                                           for name, (res, args) in exports.items())
    return _gcc(src, "-Werror=incompatible-pointer-types", "-Werror=int-conversion", extra={"erased.h": erased})


def test_prototypes_agree_with_the_header():
    """restype and argtypes of every entry of _native.EXPORTS against the C compiler's reading of the prototypes (see _prototype_check)."""
    _native = _native_built()
    assert len(_native.EXPORTS) >= 63
    done = _prototype_check(_native.EXPORTS)
    assert done.returncode == 0, done.stderr


def test_prototype_check_sees_a_wrong_width_a_wrong_class_and_a_dropped_argument():
    """The check above is not vacuous: an int64_t typed c_int32, a double typed c_float, a pointer typed as an integer and a dropped argument
    are each refused, with the entry's name in gcc's message."""
    _native = _native_built()
    res, args = _native.EXPORTS["wsi_adam_step"]          # (tensors, int32 count, 5 doubles, int64 step, stream)
    assert args[1] is ctypes.c_int32 and args[2] is ctypes.c_double and args[7] is ctypes.c_int64
    swap = lambda i, t: args[:i] + [t] + args[i + 1:]
    for bad in (swap(7, ctypes.c_int32), swap(2, ctypes.c_float), swap(0, ctypes.c_int64), args[:-1], swap(1, ctypes.c_int64)):
        done = _prototype_check({"wsi_adam_step": (res, bad)})
        assert done.returncode != 0 and "p_wsi_adam_step" in done.stderr, bad
    assert _prototype_check({"wsi_adam_step": (ctypes.c_int64, args)}).returncode != 0
    assert _prototype_check({"wsi_adam_step": (res, args)}).returncode == 0


def test_constants_and_macro_restatements_agree_with_the_header():
    """Every integer constant the binding derives, and the two function-like macros the host code restates by hand
    (_native.gemm_absmax_parts, ops._attn_flags), against the values the C compiler gives the header's own macros."""
    import types
    _native = _native_built()
    from wsi_hgnn_amd import ops
    names = sorted(_native.CONSTANTS)
    assert {"WSI_OK", "WSI_EINVAL", "WSI_ABI_VERSION", "WSI_EPI_GATED_SKIP", "WSI_GEMM_MAX_GROUPS", "WSI_OPTIM_ADAM", "WSI_ATTN_XCD_CONTIGUOUS"} <= set(names)
    assert all(getattr(_native, n) == _native.CONSTANTS[n] for n in names)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wsi_hgnn.h")).read(), flags=re.S)
    assert set(names) == set(re.findall(r"^#define\s+(WSI_\w+)[ \t]+\S", header, flags=re.M))           # none missed; function-like ones skipped
    parts_n, hub_d = (1, 127, 128, 129, 512), (0, 128, 65535)
    exprs = names + ["WSI_GEMM_ABSMAX_PARTS(%d)" % n for n in parts_n] + ["WSI_ATTN_XCD_CONTIGUOUS | WSI_ATTN_HUB_DEGREE(%d)" % d for d in hub_d] + \
        ["WSI_ATTN_HUB_DEGREE(%d)" % d for d in hub_d]
    nums = _gcc('#include <stdio.h>\n#include "wsi_hgnn.h"\nint main(void){' + "".join('printf("%%lld\\n", (long long)(%s));' % e for e in exprs) + "return 0;}",
                run=True)
    assert len(nums) == len(exprs)
    assert dict(zip(names, nums)) == _native.CONSTANTS
    assert _native.WSI_EINVAL == -22 and _native.WSI_EPI_GATED_SKIP == 1 | 4 | 16 | 32
    nums = nums[len(names):]
    assert nums[:5] == [_native.gemm_absmax_parts(n) for n in parts_n]
    plan = lambda d, loc: types.SimpleNamespace(locality=loc, heavy_degree=d)
    assert nums[5:8] == [ops._attn_flags(plan(d, True)) for d in hub_d]
    assert nums[8:] == [ops._attn_flags(plan(d, False)) for d in hub_d]


_BAD_HEADERS = {"an array member": ("int32_t reserved;", "int32_t reserved[2];"),
                "a type outside the table": ("int64_t  ldm;", "size_t  ldm;"),
                "a function pointer": ("void*           b_packed;", "void (*b_packed)(int);"),
                "a nested struct": ("int32_t reserved;", "struct { int a; } reserved;"),
                "two pointer declarators": ("float* r_out; int64_t ldr;", "float *r_out, *r2; int64_t ldr;"),
                "a parameter type outside the table": ("float* y, int64_t n, void* stream);", "float* y, long n, void* stream);"),
                "a return type outside the table": ("int64_t wsi_gemm_packed_b_bytes", "long wsi_gemm_packed_b_bytes"),
                "a division in a constant": ("#define WSI_RED_MAX  2", "#define WSI_RED_MAX  (4 / 2)"),
                "an unknown name in a constant": ("#define WSI_RED_MAX  2", "#define WSI_RED_MAX  WSI_RED_MIN"),
                "an enum": ("#define WSI_RED_MAX  2", "enum wsi_red { WSI_RED_MAX = 2 };"),
                "an unknown directive": ("#define WSI_RED_MAX  2", "#pragma pack(1)")}


@pytest.mark.parametrize("what", sorted(_BAD_HEADERS))
def test_header_parser_refuses_what_it_does_not_know(what, tmp_path):
    """The parser of the binding raises on anything outside the header's idiom and names the line (a nested struct: the line its typedef starts on)."""
    _native = _native_built()
    old, new = _BAD_HEADERS[what]
    header = open(_native.HEADER_PATH).read()
    assert header.count(old) == 1
    line = header[:header.index(old)].count("\n") + 1
    if what == "a nested struct":
        line = header[:header.index("typedef struct wsi_gemm_group {")].count("\n") + 1
    (tmp_path / "bad.h").write_text(header.replace(old, new))
    with pytest.raises(RuntimeError, match=r"bad\.h:%d: " % line):
        _native._parse_header(str(tmp_path / "bad.h"))
    (tmp_path / "good.h").write_text(header)
    assert _native._parse_header(str(tmp_path / "good.h"))[0] == _native.CONSTANTS


def test_product_never_imports_the_oracle():
    bad = []
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                static = re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M)
                dynamic = f.endswith(".py") and re.search(r"(import_module|__import__)\(\s*[fFrRbB]*['\"]oracle", text)
                by_path = f.endswith(".py") and re.search(r"spec_from_file_location\([^)]*oracle", text)
                if static or dynamic or by_path:
                    bad.append(os.path.join(dirpath, f))
    assert not bad, bad


def test_ops_refuse_cpu_tensors():
    from wsi_hgnn_amd import ops
    x = torch.randn(4, 8)
    w = torch.randn(3, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.linear(x, w, None)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.segment_reduce(x, ops.ReducePlan.from_ptr([0, 4], torch.device("cpu")), "mean")


_SURFACE = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_surface.json")))


def _ours(key):
    import importlib
    from wsi_hgnn_amd import models, pooling
    heat_layer, hgt_mod, rgcn_mod, h4_mod, asap_mod = (importlib.import_module(f"wsi_hgnn_amd.{n}") for n in (
        "models.heat_layer", "models.HGT", "models.HetRGCN", "models.HEATNet4", "pooling.ASAP"))
    return {"models/HEATNet4.py:HEATLayer": heat_layer.HEATLayer, "models/HEATNet2.py:HEATLayer": heat_layer.HEATLayer,
            "models/HEATNet4.py:HEATNet4": models.HEATNet4, "models/HEATNet2.py:HEATNet2": models.HEATNet2,
            "models/HEATNet4.py:LinearAttentionBlock": h4_mod.LinearAttentionBlock,
            "models/HGT.py:HGTLayer": hgt_mod.HGTLayer, "models/HGT.py:HGT": models.HGT,
            "models/HetRGCN.py:HeteroRGCNLayer": rgcn_mod.HeteroRGCNLayer, "models/HetRGCN.py:HeteroRGCN": models.HeteroRGCN,
            "models/GCN.py:GCN": models.GCN, "models/GCN_NTPool.py:NTPoolGCN": models.NTPoolGCN,
            "pooling/avg_pooling.py:AvgPooling": pooling.AvgPooling, "pooling/sum_pooling.py:SumPooling": pooling.SumPooling,
            "pooling/max_pooling.py:MaxPooling": pooling.MaxPooling, "pooling/nt_pooling.py:NTPooling": pooling.NTPooling,
            "pooling/ASAP.py:LEConv": asap_mod.LEConv, "pooling/ASAP.py:ASAPPooling": pooling.ASAPPooling}[key]


@pytest.mark.parametrize("key", sorted(_SURFACE["classes"]))
def test_module_surface_matches_reference(key):
    """Constructor and forward signatures of every mirrored class against the REFERENCE'S syntax tree (tests/golden/
    reference_surface.json, made by tests/golden/make_reference_surface_fixture.py from /root/reference): same argument names in
    the same order with the same defaults (incl. the ``dropuout`` spelling)."""
    ref = _SURFACE["classes"][key]
    cls = _ours(key)
    if ref["init"] is not None:
        ps = inspect.signature(cls.__init__).parameters
        names = [a["name"] for a in ref["init"]]
        if list(ps) == ["self", "args", "kwargs"]:          # no constructor of our own (nn.Module's): fine for a reference `__init__(self)`
            assert names == ["self"], key
            return
        # the reference's arguments, in its order; anything we add behind them must be optional
        assert list(ps)[:len(names)] == names, key
        assert all(p.default is not inspect.Parameter.empty for p in list(ps.values())[len(names):]), key
        for a in ref["init"]:
            d = ps[a["name"]].default
            if a["default"] is None:
                assert d is inspect.Parameter.empty, (key, a)
            else:
                assert repr(d) == a["default"] or str(d) == a["default"], (key, a, d)
    if ref["forward"] is not None:
        assert list(inspect.signature(cls.forward).parameters)[:len(ref["forward"])] == ref["forward"], key


def test_parameter_creation_order_matches_reference():
    """The order in which ``__init__`` registers sub-modules / parameters decides both the state_dict key order and which random
    numbers each parameter draws under a fixed seed (the reference seeds with 611, main.py:15): for every model class it must be
    the order of the ``self.X = ...`` statements in the reference's constructor."""
    from wsi_hgnn_amd import models
    nd = {"0": 0, "1": 1}
    ed = {(s, e, d): i for i, (s, e, d) in enumerate((s, e, d) for e in ("pos", "neg") for s in nd for d in nd)}
    built = {"models/HEATNet4.py:HEATNet4": models.HEATNet4(8, 16, 2, 2, 4, nd, 0.2, "att"),
             "models/HEATNet2.py:HEATNet2": models.HEATNet2(8, 16, 3, 1, 2, nd, 0.0, "att"),
             "models/HGT.py:HGT": models.HGT(nd, ed, 8, 16, 2, 2, 4, graph_pooling_type="att"),
             "models/HetRGCN.py:HeteroRGCN": models.HeteroRGCN(8, 16, 2, 2, {et: str(i) for et, i in ed.items()}, nd, "att"),
             "models/GCN.py:GCN": models.GCN(8, 16, 2, 2, torch.relu, 0.0, "att"),
             "models/GCN_NTPool.py:NTPoolGCN": models.NTPoolGCN(8, 16, 2, nd, 2, torch.relu, 0.0, "att")}
    for key, m in built.items():
        ref_order = list(dict.fromkeys(c["attr"] for c in _SURFACE["classes"][key]["created"]))
        ours = list(dict.fromkeys(k.split(".")[0] for k in m.state_dict()))
        assert ours == [a for a in ref_order if a in ours], (key, ours, ref_order)
        assert set(ours) >= {a for a in ref_order if a in dict(m.named_children()) and any(True for _ in getattr(m, a).parameters())}, key


def test_state_dict_keys_of_appendix_a7():
    from wsi_hgnn_amd import models
    nd = {"0": 0, "1": 1}
    m = models.HEATNet4(in_dim=8, hidden_dim=16, out_dim=2, n_layers=2, n_heads=4, node_dict=nd, dropuout=0.2, graph_pooling_type="mean")
    keys = set(m.state_dict().keys())
    for k in ["linears_prediction.0.weight", "adapt_ws.1.bias", "gcs.0.weight.weight", "gcs.1.k_linears.0.weight", "gcs.0.q_linears.1.bias",
              "gcs.0.v_linears.0.weight", "gcs.0.a_linears.1.weight", "gcs.0.e_linear.weight", "gcs.1.skip", "attn.0.op.weight",
              "head_2.weight", "head_1.bias", "head.weight"]:
        assert k in keys, k
    assert m.state_dict()["attn.0.op.weight"].shape == (1, 256, 1)
    assert m.state_dict()["head_2.weight"].shape == (256, 512)
    assert m.n_layers == 2
    m2 = models.HEATNet2(8, 16, 3, 1, 2, nd, 0.0)
    assert m2.state_dict()["linears_prediction.1.weight"].shape == (3, 16)


def test_graph_container_surface():
    import wsi_hgnn_amd as W
    from wsi_hgnn_amd import synthetic
    g = synthetic.hetero_graph(50, 4, seed=1)
    assert g.ntypes == ["0", "1", "2"] and len(g.canonical_etypes) == 6 and not g.is_homogeneous
    assert isinstance(g.edata["sim"], dict) and set(g.edata["sim"]) == set(g.canonical_etypes)
    assert g.nodes["1"].data["feat"].shape == (g.num_nodes("1"), 4)
    with g.local_scope():
        g.ndata["h"] = {t: torch.zeros(g.num_nodes(t), 1) for t in g.ntypes}
        assert "h" in g.ndata
    assert "h" not in g.ndata
    b = W.batch([g, synthetic.hetero_graph(30, 4, seed=2)])
    assert b.batch_size == 2 and b.batch_num_nodes("0").tolist() == [g.num_nodes("0"), 15]
    assert b.num_edges() == g.num_edges() + 8 * 30
    h = synthetic.homogeneous_graph(20, 4)
    assert h.is_homogeneous and h.ndata["feat"].shape == (20, 4)


def test_c_abi_argument_errors_without_a_gpu():
    """Every entry point validates its arguments before it touches the device and reports through the errno-style return code +
    wsi_last_error() (no C++ exception crosses the boundary): exercised here with arguments that must be rejected, so no kernel
    is launched and no GPU is needed."""
    from wsi_hgnn_amd import _native as N
    lib = N.load()
    err = lambda: lib.wsi_last_error().decode()
    EINVAL = -22
    # GEMM: unknown precision / op / epilogue bits, group table problems
    g = (N.GemmGroup * 1)()
    g[0].M, g[0].N, g[0].K = 4, 4, 4
    assert lib.wsi_gemm_grouped(N.WSI_GEMM_NT, 0, 7, g, 1, None, 0, None) == EINVAL and "precision" in err()
    assert lib.wsi_gemm_grouped(9, 0, N.WSI_GEMM_FP32, g, 1, None, 0, None) == EINVAL and "unknown op" in err()
    assert lib.wsi_gemm_grouped(N.WSI_GEMM_NT, 1 << 20, N.WSI_GEMM_FP32, g, 1, None, 0, None) == EINVAL and "epilogue" in err()
    assert lib.wsi_gemm_grouped(N.WSI_GEMM_NT, 0, N.WSI_GEMM_FP32, g, 1, None, 0, None) == EINVAL and "null pointer" in err()
    assert lib.wsi_gemm_grouped(N.WSI_GEMM_NT, 0, N.WSI_GEMM_FP32, g, N.WSI_GEMM_MAX_GROUPS + 1, None, 0, None) == EINVAL
    assert lib.wsi_gemm_grouped(N.WSI_GEMM_TN, N.WSI_EPI_BIAS, N.WSI_GEMM_BF16X6, g, 1, None, 0, None) == EINVAL and "TN accepts" in err()
    assert lib.wsi_gemm_workspace_bytes(N.WSI_GEMM_NT, N.WSI_GEMM_FP32, g, 1) == 0
    # which kernel family a launch runs on: fp16x3 for all three ops (weight gradients: the column-scaled kernel of gemm_tn16.hip); auto only
    # where the launch is large enough (>= 12 GFLOP and K >= 384; a weight gradient: >= 30 GFLOP, >= 2048 rows; a large batch - a group of >= 24576 rows - from 5 / 4 GFLOP; weight gradients at least 192 wide) to amortise the scaled-fp16 pre-pass
    kp = lambda op, prec, M, Nn, K: (setattr(g[0], "M", M), setattr(g[0], "N", Nn), setattr(g[0], "K", K), lib.wsi_gemm_kernel_precision(op, prec, g, 1))[-1]
    assert kp(N.WSI_GEMM_NT, N.WSI_GEMM_FP32, 80000, 512, 512) == N.WSI_GEMM_FP32
    assert kp(N.WSI_GEMM_NT, N.WSI_GEMM_FP16X3, 8, 8, 8) == N.WSI_GEMM_FP16X3 and kp(N.WSI_GEMM_TN, N.WSI_GEMM_FP16X3, 512, 512, 80000) == N.WSI_GEMM_FP16X3
    assert kp(N.WSI_GEMM_NT, N.WSI_GEMM_AUTO, 80000, 1536, 512) == N.WSI_GEMM_FP16X3 and kp(N.WSI_GEMM_NN, N.WSI_GEMM_AUTO, 80000, 512, 1536) == N.WSI_GEMM_FP16X3
    assert kp(N.WSI_GEMM_NT, N.WSI_GEMM_AUTO, 20000, 256, 256) == N.WSI_GEMM_BF16X6 and kp(N.WSI_GEMM_NT, N.WSI_GEMM_AUTO, 10 ** 6, 128, 128) == N.WSI_GEMM_BF16X6
    assert kp(N.WSI_GEMM_NT, N.WSI_GEMM_AUTO, 40000, 768, 256) == N.WSI_GEMM_FP16X3 and kp(N.WSI_GEMM_NN, N.WSI_GEMM_AUTO, 80000, 256, 256) == N.WSI_GEMM_FP16X3
    assert kp(N.WSI_GEMM_NT, N.WSI_GEMM_AUTO, 20000, 768, 256) == N.WSI_GEMM_BF16X6 and kp(N.WSI_GEMM_NT, N.WSI_GEMM_AUTO, 20000, 768, 512) == N.WSI_GEMM_FP16X3   # a small batch keeps the old rule
    assert kp(N.WSI_GEMM_TN, N.WSI_GEMM_AUTO, 1536, 512, 80000) == N.WSI_GEMM_FP16X3 and kp(N.WSI_GEMM_NT, 9, 4, 4, 4) < 0
    assert kp(N.WSI_GEMM_TN, N.WSI_GEMM_AUTO, 512, 512, 1500) == N.WSI_GEMM_BF16X6 and kp(N.WSI_GEMM_TN, N.WSI_GEMM_AUTO, 64, 64, 80000) == N.WSI_GEMM_BF16X6
    assert kp(N.WSI_GEMM_TN, N.WSI_GEMM_AUTO, 256, 256, 40000) == N.WSI_GEMM_FP16X3 and kp(N.WSI_GEMM_TN, N.WSI_GEMM_AUTO, 128, 1024, 80000) == N.WSI_GEMM_BF16X6
    assert kp(N.WSI_GEMM_TN, N.WSI_GEMM_AUTO, 512, 1024, 6000) == N.WSI_GEMM_BF16X6                       # 6.3 GFLOP over a short group
    assert kp(N.WSI_GEMM_TN, N.WSI_GEMM_AUTO, 512, 1536, 20000) == N.WSI_GEMM_FP16X3                      # 31 GFLOP: the small-batch rule
    assert kp(N.WSI_GEMM_TN, N.WSI_GEMM_AUTO, 256, 256, 20000) == N.WSI_GEMM_BF16X6                       # 2.6 GFLOP
    # the scaled-fp16 weight gradient sizes its own workspace (slabs + column statistics); who leaves column statistics
    assert lib.wsi_gemm_workspace_bytes(N.WSI_GEMM_TN, N.WSI_GEMM_FP16X3, g, 1) > 0
    assert lib.wsi_gemm_writes_colstats(N.WSI_GEMM_TN, N.WSI_GEMM_FP16X3, g, 1) == 0 and lib.wsi_gemm_writes_colstats(N.WSI_GEMM_NT, N.WSI_GEMM_FP32, g, 1) == 0
    assert lib.wsi_col_absmax_workspace_bytes(1000, 512) == 4 * 512 * 4 and lib.wsi_col_absmax(None, 0, -1, 4, None, None, 0, None) == EINVAL
    assert lib.wsi_col_absmax(None, 0, 5, 4, None, None, 0, None) == EINVAL and "null pointer" in err()
    assert lib.wsi_gemm_workspace_bytes(N.WSI_GEMM_NT, N.WSI_GEMM_AUTO, g, 1) == 0                 # (g: 4 x 4 x 4 again -> bf16x6)
    g[0].M, g[0].N, g[0].K = 4, 4, 4
    g[0].M = -1
    assert lib.wsi_gemm_grouped(N.WSI_GEMM_NT, 0, N.WSI_GEMM_FP32, g, 1, None, 0, None) == EINVAL and "negative" in err()
    # attention: shape checks come first
    z = [None] * 3
    assert lib.wsi_heat_attn_fwd(None, 0, None, 0, None, 0, 5, 30, 4, None, None, None, None, None, 0, 0, None, None, None, 0, None, None, None, None, None) == EINVAL
    assert "bad shape" in err()                                                             # D % H != 0
    assert lib.wsi_heat_attn_fwd(None, 0, None, 0, None, 0, 0, 32, 4, None, None, None, None, None, 0, 0, None, None, None, 0, None, None, None, None, None) == 0
    assert lib.wsi_heat_attn_fwd(None, 0, None, 0, None, 0, 5, 32, 4, None, None, None, None, None, 0, 0, None, None, None, 0, None, None, None, None, None) == EINVAL
    assert "null pointer" in err()
    # ASAP kernels
    assert lib.wsi_graph_topk(None, None, -1, 1, None, None, None, None) == EINVAL and "bad shape" in err()
    assert lib.wsi_graph_topk(None, None, 10, 1, None, None, None, None) == EINVAL and "null pointer" in err()
    assert lib.wsi_graph_topk(None, None, 0, 0, None, None, None, None) == 0
    assert lib.wsi_stas(0, -3, *([None] * 14), None) == EINVAL and "bad kN" in err()
    assert lib.wsi_stas(0, 4, *([None] * 14), None) == EINVAL and "null pointer" in err()
    assert lib.wsi_stas(0, 0, *([None] * 14), None) == 0
    assert lib.wsi_context_create(None) == EINVAL
    lib.wsi_context_destroy(None)                                                           # NULL is accepted


def test_product_library_reads_no_environment_variable():
    """include/wsi_hgnn.h promises "no global mutable state": no environment variable may change what a call of the product library does.
    The kernel variants / A-B switches of tools/ are compiled only with -DWSI_ABLATE (csrc/common.h::knob) into a SEPARATE shared object;
    the product object does not even import getenv / secure_getenv, no C source calls getenv outside that helper, and the package never
    loads the measurement flavour by itself."""
    import subprocess
    import __graft_entry__
    __graft_entry__.build()
    from wsi_hgnn_amd import _native
    from wsi_hgnn_amd.build import LIB, LIB_ABLATE
    assert os.path.realpath(_native.LIB_PATH) == os.path.realpath(LIB) != os.path.realpath(LIB_ABLATE)
    undefined = subprocess.check_output(["nm", "-D", "--undefined-only", LIB], text=True)
    assert not re.search(r"\b(secure_)?getenv\b", undefined), "libwsi_hgnn.so imports getenv"
    csrc = os.path.join(PKG, "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            text = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, f)).read())
            uses = [m.start() for m in re.finditer(r"\bgetenv\s*\(", text)]
            if f == "common.h":
                assert len(uses) == 1 and "#ifdef WSI_ABLATE" in text[:uses[0]], "getenv outside the WSI_ABLATE helper"
            else:
                assert not uses, f"{f} calls getenv directly"
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py") and f not in ("_native.py", "build.py"):
                assert "use_measurement_library" not in open(os.path.join(dirpath, f)).read(), f
    # ... and since round 6 the same holds for the HOST package: every switch is a call or an argument (README: "Switches of the Python host module");
    # only tools/_knobs.py translates the old WSI_* variables, for the measurement scripts
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if f.endswith(".py"):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"os\.environ|\bgetenv\b", text), f"{os.path.join(dirpath, f)} reads the environment"


def test_side_stream_switches_are_host_state_with_independent_blockers():
    """ops.block_side_streams / block_background_weight_gradients: every blocker (an armed data-parallel bucket, a pinned-host loader
    feeding steps) is independent - the mechanisms come back on only when the LAST one lets go; the side-stream count accepts 1 or 2 only."""
    from wsi_hgnn_amd import ops
    assert not ops._BACKGROUND["blocked"] and not ops._SIDE_STATS["reasons"]
    ops.block_side_streams(True, "loader-1")
    ops.block_background_weight_gradients(True, who="bucket")
    assert ops._BACKGROUND["blocked"] and ops._SIDE_STATS["reasons"] == {"loader-1"}
    ops.block_background_weight_gradients(False, who="bucket")
    assert ops._BACKGROUND["blocked"], "the loader still feeds steps"
    ops.block_side_streams(True, "loader-2")
    ops.block_side_streams(False, "loader-1")
    assert ops._BACKGROUND["blocked"] and ops._SIDE_STATS["reasons"] == {"loader-2"}
    ops.block_side_streams(False, "loader-2")
    assert not ops._BACKGROUND["blocked"] and not ops._SIDE_STATS["reasons"]
    ops.block_side_streams(False, "never-blocked")                     # releasing twice / an unknown blocker is harmless
    assert not ops._BACKGROUND["blocked"]
    before = ops._SIDE_STREAMS["count"]
    with pytest.raises(ValueError):
        ops.set_side_stream_count(3)
    ops.set_side_stream_count(2)
    assert ops._SIDE_STREAMS["count"] == 2
    ops.set_side_stream_count(before)
