#!/usr/bin/env python
"""Fixture produced by EXECUTING the reference's own ``dropout_patches`` (baselines/ReMix_DSMIL_ABMIL/train_tcga_k-fold.py:90-96) over a grid
of bag sizes and rates: mil/reference_dropout_patches.json records, per (n, p), the number of rows of the bag it returned - or null where numpy
refused the second draw ("Cannot take a larger sample than population": more rows to repeat than were kept).  Which rows it drew is not
recorded: numpy's generator is not the project's draw.  Data only; no reference source travels.

The function is taken out of the reference's file by name and executed with numpy alone (the file's other imports - pandas, sklearn, the
models - are not needed for it).  Re-run where the reference is checked out:
``python tests/golden/make_reference_dropout_patches_fixture.py <reference checkout>``."""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (0, 1, 2, 3, 4, 7, 10, 12, 100, 127, 128, 129, 300, 1000, 6000, 9999, 12000)
RATES = (0.0, 0.1, 0.2, 0.25, 0.29, 0.3, 0.5, 0.6, 0.75)


def load(reference: str):
    path = os.path.join(reference, "baselines", "ReMix_DSMIL_ABMIL", "train_tcga_k-fold.py")
    tree = ast.parse(open(path).read(), path)
    fn = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == "dropout_patches"]
    scope = {"np": np}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), scope)
    return scope["dropout_patches"]


def main():
    ref = load(sys.argv[1])
    np.random.seed(2407)
    cases = []
    for n in SIZES:
        for p in RATES:
            feats = np.arange(n * 2, dtype=np.float32).reshape(n, 2)
            try:
                out = ref(feats, p)
                assert out.shape[1] == 2 and all((out[:, 0] % 2 == 0).tolist())
                rows = int(out.shape[0])
            except ValueError:
                rows = None
            cases.append({"n": n, "p": p, "rows": rows})
    os.makedirs(os.path.join(HERE, "mil"), exist_ok=True)
    path = os.path.join(HERE, "mil", "reference_dropout_patches.json")
    with open(path, "w") as f:
        json.dump({"function": "baselines/ReMix_DSMIL_ABMIL/train_tcga_k-fold.py:dropout_patches", "cases": cases}, f, indent=0)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
