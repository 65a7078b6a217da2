"""ctypes binding of csrc/libwsi_hgnn.so (the C-ABI declared in include/wsi_hgnn.h).

There is NO fallback: if the shared object is missing or a symbol is absent, importing fails
loudly — the product path never silently drops to eager PyTorch (or to the CPU oracle).
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_float, c_int32, c_int64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libwsi_hgnn.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "wsi_hgnn.h")

# ------------------------------------------------------------------------------------------------
# The binding is DERIVED from include/wsi_hgnn.h at import: every object-like `#define WSI_* <integer expression>` becomes a module
# attribute, every `typedef struct ... { ... } wsi_x_y_t;` a ctypes.Structure named XY (AttnPool, AdamTensor, OptimTensor, OptimHyper,
# GemmGroup), every prototype an entry of EXPORTS (restype, argtypes).  Any pointer is a c_void_p.  The parser knows the header's own
# idiom and nothing else: whatever it does not understand raises here, with the header's line number - it never guesses.
# tests/test_boundary.py holds every derived layout, signature and value against the C compiler's reading of the same file.
# ------------------------------------------------------------------------------------------------
_SCALARS = {"int": ctypes.c_int, "int32_t": c_int32, "int64_t": c_int64, "uint32_t": ctypes.c_uint32, "float": c_float,
            "double": ctypes.c_double}
_RETURNS = {"int": ctypes.c_int, "int32_t": c_int32, "int64_t": c_int64, "void": None, "const char*": c_char_p}
_DECL = re.compile(r"\s*(?:const\s+)?(\w+)((?:\s*\*(?:\s*const\b)?)*)\s*(\w+(?:\s*,\s*\w+)*)\s*")


def _parse_header(path: str):
    lines_only = lambda m: "\n" * m.group().count("\n")        # what is taken out leaves its newlines: an offset still names its line
    text = re.sub(r"/\*.*?\*/", lines_only, open(path).read(), flags=re.S)
    text = re.sub(r"#ifdef __cplusplus\n.*?#endif", lines_only, text, flags=re.S)          # the extern "C" brackets
    constants, structs, exports, pointees = {}, {}, {}, {"void", "char", *_SCALARS}

    def fail(pos: int, what: str):
        raise RuntimeError(f"{path}:{text.count(chr(10), 0, pos) + 1}: the binding cannot read {' '.join(what.split())[:100]!r} "
                           "(wsi_hgnn_amd/_native.py understands the header's own idiom only and does not guess)")

    def pieces(lo: int, hi: int, sep: str):
        """(offset, text) of the non-blank pieces of text[lo:hi] between ``sep``s."""
        for m in re.compile(f"[^{sep}]*[^{sep}\\s][^{sep}]*").finditer(text, lo, hi):
            yield m.start() + len(m.group()) - len(m.group().lstrip()), m.group()

    def declaration(pos: int, decl: str, many: bool):
        """``[const] T [* [const]]... name[, name...]`` -> (ctype, names): T from _SCALARS, any pointer to a known type a c_void_p."""
        m = _DECL.fullmatch(decl)
        names = re.split(r"\s*,\s*", m.group(3)) if m else []
        if not m or m.group(1) not in (pointees if m.group(2) else _SCALARS) or (len(names) > 1 and (m.group(2) or not many)):
            fail(pos, decl)
        return (c_void_p if m.group(2) else _SCALARS[m.group(1)]), names

    def directive(m):
        d = re.fullmatch(r"\s*#define\s+(WSI_\w+)(\(.*?\))?(.*)", m.group())
        if d and not d.group(2) and d.group(3).strip():         # object-like, with a value (function-like macros and the include guard: skipped)
            try:                                                # earlier constants under operators that mean the same in C and in Python
                ok = re.fullmatch(r"[\w\s()|&<+*-]+", d.group(3)) and eval(d.group(3), {"__builtins__": {}}, dict(constants))
            except Exception:
                ok = None
            if type(ok) is not int:
                fail(m.start(), m.group())
            constants[d.group(1)] = ok
        elif not d and not re.match(r"\s*#(ifndef|include|endif)\b", m.group()):
            fail(m.start(), m.group())
        return ""

    def opaque(m):
        pointees.add(m.group(1))
        return lines_only(m)

    def struct(m):
        name = re.fullmatch(r"wsi_(\w+)_t", m.group(2)) or fail(m.start(2), m.group(2))
        if not m.group(1).rstrip().endswith(";"):
            fail(m.end(1), m.group(1)[-40:])
        fields = [(n, ctype) for pos, decl in pieces(m.start(1), m.end(1), ";") for ctype, names in [declaration(pos, decl, True)] for n in names]
        structs[m.group(2)] = type(name.group(1).title().replace("_", ""), (ctypes.Structure,),
                                   {"_fields_": fields, "__doc__": f"{m.group(2)} (include/wsi_hgnn.h)."})
        pointees.add(m.group(2))
        return lines_only(m)

    text = re.sub(r"^[ \t]*#.*$", directive, text, flags=re.M)
    text = re.sub(r"\btypedef\s+struct\s+\w+\s+(\w+)\s*;", opaque, text)
    text = re.sub(r"\btypedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    if text.rstrip()[-1:] not in ("", ";"):
        fail(len(text.rstrip()), text.rstrip()[-40:])
    for pos, stmt in pieces(0, len(text), ";"):                 # whatever is left must be prototypes
        m = re.fullmatch(r"\s*(const\s+char\s*\*|\w+)\s+(wsi_\w+)\s*\((.*)\)\s*", stmt, flags=re.S)
        ret = m and re.sub(r"\s+", " ", m.group(1)).replace(" *", "*")
        if ret not in _RETURNS or not m.group(3).strip():
            fail(pos, stmt)
        lo = pos - (len(stmt) - len(stmt.lstrip()))
        exports[m.group(2)] = (_RETURNS[ret], [] if m.group(3).strip() == "void" else
                               [declaration(p, decl, False)[0] for p, decl in pieces(lo + m.start(3), lo + m.end(3), ",")])
    return constants, structs, exports


CONSTANTS, STRUCTS, EXPORTS = _parse_header(HEADER_PATH)
globals().update(CONSTANTS)
globals().update({cls.__name__: cls for cls in STRUCTS.values()})


def gemm_absmax_parts(n_cols: int) -> int:
    """WSI_GEMM_ABSMAX_PARTS: slots per row a group of ``n_cols`` output columns writes into c_absmax."""
    return 2 * ((int(n_cols) + 127) // 128)


_lib = None
_ablate = False


def use_measurement_library() -> None:
    """tools/ only: bind the -DWSI_ABLATE flavour of the library (csrc/libwsi_hgnn_ablate.so: the dominant kernel's ablation variants and the
    WSI_* environment knobs of csrc/common.h::knob compiled in) instead of the product library.  Must be called before the first ``load()``;
    the package itself never calls it - the product library reads no environment variable."""
    global _ablate, LIB_PATH
    if _lib is not None:
        raise RuntimeError("use_measurement_library(): the product library is already loaded in this process")
    from .build import LIB_ABLATE
    _ablate, LIB_PATH = True, LIB_ABLATE


def load() -> ctypes.CDLL:
    """Load the shared object and bind every declared symbol; raise RuntimeError when impossible."""
    global _lib
    if _lib is not None:
        return _lib
    try:   # (re)build in-tree when the shared object is missing or older than its sources (hipcc cross-compiles anywhere)
        from .build import build_native
        build_native(force=False, verbose=True, ablate=_ablate)
    except Exception as exc:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing and could not be built ({exc}). Run `python -c 'import __graft_entry__ as g; "
                f"g.build()'`. There is no PyTorch/CPU fallback for the hot path.") from exc
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: the HIP extension is not built; there is no PyTorch/CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:  # pragma: no cover
            raise RuntimeError(f"{LIB_PATH} does not export {name}; rebuild it") from exc
        fn.restype = res
        fn.argtypes = args
    if lib.wsi_abi_version() != WSI_ABI_VERSION:
        raise RuntimeError(f"libwsi_hgnn.so ABI {lib.wsi_abi_version()} != expected {WSI_ABI_VERSION}; rebuild it")
    _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().wsi_last_error()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


_contexts: dict = {}


def context() -> int:
    """The caller-owned wsi_context_t of the current device (side stream of the hub kernels), created on first use and kept
    for the life of the process: the LIBRARY holds no state, this host-side mirror owns one context per device."""
    dev = torch._C._cuda_getDevice()            # (torch.cuda.current_device() re-checks the lazy init on every call: ~10 us)
    h = _contexts.get(dev)
    if h is None:
        out = c_void_p()
        check(load().wsi_context_create(ctypes.byref(out)), "wsi_context_create")
        h = _contexts[dev] = out.value
    return h


def stream() -> int:
    """Raw hipStream_t of torch's current stream on the current device (the C accessors: the torch.cuda wrappers cost ~15 us a call,
    paid once per kernel launch)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def ptr(t, byte_offset: int = 0):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr() + byte_offset


def require_cuda(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("wsi_hgnn_amd ops run on the GPU only (HIP kernels); got a CPU tensor. "
                               "The CPU oracle under oracle/ is test infrastructure, not a fallback.")
