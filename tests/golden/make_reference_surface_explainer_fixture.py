#!/usr/bin/env python
"""Generates tests/golden/reference_surface_explainer.json from the reference's ``explainers/gnn_explainer.py``, read with ``ast``
(the module imports DGL, networkx and matplotlib, so it is never imported or executed): the argument names and defaults of
``GNNExplainer.__init__`` and ``GNNExplainer.explain_node``, and the literal ``params`` dict of the class.  Only names and values
are stored.  Usage: python tests/golden/make_reference_surface_explainer_fixture.py <path to the reference checkout>
"""
import ast
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_surface_explainer.json")
REL = "explainers/gnn_explainer.py"


def signature(fn):
    a = fn.args
    names = [x.arg for x in a.args]
    defaults = [None] * (len(names) - len(a.defaults)) + [ast.literal_eval(d) for d in a.defaults]
    return [{"name": n, "default": d, "required": i < len(names) - len(a.defaults)} for i, (n, d) in enumerate(zip(names, defaults))]


def main(ref):
    tree = ast.parse(open(os.path.join(ref, REL)).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GNNExplainer")
    funcs = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    params = next(ast.literal_eval(n.value) for n in cls.body
                  if isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "params" for t in n.targets))
    fixture = {"source": f"HKU-MedAI/WSI-HGNN {REL} (ast only)", "class": "GNNExplainer",
               "init": signature(funcs["__init__"]), "explain_node": signature(funcs["explain_node"]), "params": params}
    json.dump(fixture, open(OUT, "w"), indent=1)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
