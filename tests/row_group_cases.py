"""What the dispatch tests of the row-group kernels (GAT, RAConv, GIN) share (no test functions): csrc/row_group.h's ``row_cfg`` restated
once, and one reader of its case list and of the dispatch macro a kernel file uses."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wsi-hgnn_amd", "csrc")


def row_cfg(width, unit, min_lanes, vec4_ok):
    """(VEC, G, NK) of a row of ``width`` floats in units of ``unit``: 16-byte chunks when allowed and unit % 4 == 0, the smallest group
    of 4 .. 64 lanes that covers the chunks and ``min_lanes``, the power of two of chunks per lane that covers the rest."""
    vec = 4 if vec4_ok and unit % 4 == 0 else 1
    chunks = width // vec
    G = next(g for g in (4, 8, 16, 32, 64) if g == 64 or (g >= chunks and g >= min_lanes))
    NK = next(k for k in (1, 2, 4, 8, 16, 32, 64, 128) if k * G >= chunks)
    return vec, G, NK


def code(vec, G, NK):                      # the switch value of the dispatch macros
    return vec * 100000 + G * 100 + NK


def case_lists():
    """(narrow, wide): the codes of ROW_GROUP_CASES, in its order"""
    with open(os.path.join(CSRC, "row_group.h")) as f:
        text = f.read()
    table = text[text.index("#define ROW_GROUP_CASES"):text.index("#define ROW_GROUP_CASE_")]
    return tuple([code(int(v), int(g), int(k)) for g, v, k in re.findall(kind + r"\(X, (\d+), (\d+), (\d+)\)", table)] for kind in ("NARROW", "WIDE"))


def family_codes(hip):
    """the sorted codes a kernel file instantiates: the narrow ones, or all, by the dispatch macro it uses"""
    with open(os.path.join(CSRC, hip)) as f:
        uses = set(re.findall(r"ROW_GROUP_DISPATCH_(NARROW|ALL)\(", f.read()))
    assert len(uses) == 1, (hip, uses)
    narrow, wide = case_lists()
    return sorted(narrow + wide if uses == {"ALL"} else narrow)
