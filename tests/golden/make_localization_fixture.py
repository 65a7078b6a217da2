"""Writes tests/golden/localization/labels.npz and auc.json: what two independent libraries say about the cases of tests/localization_cases.py.

labels.npz: lattice points against random rings (most of them self-intersecting), labelled by ``matplotlib.path.Path.contains_points`` per
ring and ORed over the rings of a slide; the points on a ring's boundary (the exact test of localization_cases.ring_contains) are removed
first, since matplotlib does not define them.  auc.json: sklearn's ``auc(*roc_curve(labels, scores)[:2])`` for every slide and column of
localization_cases.auc_cases(), null where sklearn gives NaN or refuses (a one-class slide, a NaN score, an empty slide).

    python tests/golden/make_localization_fixture.py          (needs matplotlib and scikit-learn; the tests read the files only)
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import localization_cases as C  # noqa: E402


def labels_fixture():
    from matplotlib.path import Path
    rng = np.random.RandomState(2016)
    verts, ring_ptr, slide_ring_ptr, points, sizes, labels = [], [0], [0], [], [], []
    for s in range(4):
        rings = []
        for _ in range(3 + s):
            k = int(rng.randint(3, 12))
            cx, cy = rng.randint(-20, 20, size=2) * C.Q * 4
            ring = [(float(cx + a * C.Q), float(cy + b * C.Q)) for a, b in rng.randint(-160, 161, size=(k, 2))]
            rings.append(ring)
        cand = C.lattice_points(160, -55.0, -55.0, 55.0, 55.0, seed=100 + s)
        kept = [p for p in cand if not C.on_any_boundary(rings, *p)]
        inside = np.zeros(len(kept), dtype=bool)
        for ring in rings:
            inside |= Path(np.array(ring + ring[:1]), closed=True).contains_points(np.array(kept))
        for ring in rings:
            verts += ring
            ring_ptr.append(len(verts))
        slide_ring_ptr.append(len(ring_ptr) - 1)
        points += kept
        sizes.append(len(kept))
        labels += inside.astype(np.int32).tolist()
        assert (C.label_loop([(rings, kept)]) == inside.astype(np.int32)).all(), "the loop restatement and matplotlib disagree off the boundary"
    labels = np.array(labels, dtype=np.int32)
    assert 300 <= len(points) <= 700 and 0.1 < labels.mean() < 0.9
    np.savez(os.path.join(C.GOLDEN, "labels.npz"), vertices=np.array(verts, dtype=np.float64), ring_ptr=np.array(ring_ptr, dtype=np.int64),
             slide_ring_ptr=np.array(slide_ring_ptr, dtype=np.int64), points=np.array(points, dtype=np.float64),
             sizes=np.array(sizes, dtype=np.int64), labels=labels)


def auc_fixture():
    from sklearn.metrics import auc, roc_curve
    out = {}
    for name, (scores, labels, sizes) in C.auc_cases().items():
        sc = np.asarray(scores).reshape(len(labels), -1)
        rows, row = [], 0
        for n in sizes:
            cols = []
            for c in range(sc.shape[1]):
                try:
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        fpr, tpr, _ = roc_curve(labels[row:row + n], sc[row:row + n, c])
                        v = float(auc(fpr, tpr))
                except ValueError:
                    v = float("nan")
                cols.append(None if v != v else v)
            rows.append(cols)
            row += n
        out[name] = rows
    json.dump(out, open(os.path.join(C.GOLDEN, "auc.json"), "w"), indent=1)


if __name__ == "__main__":
    os.makedirs(C.GOLDEN, exist_ok=True)
    labels_fixture()
    auc_fixture()
    print("wrote", C.GOLDEN)
