#!/usr/bin/env python
"""Fixture produced by EXECUTING the reference's own ``mix_aug`` (baselines/ReMix_DSMIL_ABMIL/train_remix_k-fold.py:71-107) under
``np.random.seed``: mil/reference_remix.npz holds a small bank of reduced bags (float32, 8 x 512 each, as the reference hard-codes), their
labels, and for every mode and the rates 0.5 and 1.0 the seed, the bag that was trained on and the mixed bag ``mix_aug`` returned.  Each case
replays the draws the reference makes around the call in its order - ``np.random.permutation`` (get_bag_feats_v2, line 36),
``np.random.choice`` over the same-class bags and ``np.random.uniform`` (mix_the_bag_aug, lines 113-116) - and then calls ``mix_aug`` itself.
Data only; no reference source travels.

The shift bank (3.3 MB per bag) is not stored: it is ``RandomState(SHIFT_SEED).standard_normal(...)`` times SHIFT_SCALE rounded to float32,
which a test regenerates; the reference is handed those float32 values (as float64, the dtype np.random.multivariate_normal gives it).
Outputs are stored as float32, which is what the reference's ``torch.Tensor([bag_feats])`` (line 120) makes of them.

Re-run where the reference is checked out (needs /root/reference): ``python tests/golden/make_reference_remix_fixture.py``."""
import importlib.util
import os
import sys

import numpy as np
from scipy.spatial.distance import cdist

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/baselines/ReMix_DSMIL_ABMIL"
S, K, D, V = 4, 8, 512, 200
LABELS = (1, 0, 1, 1)
BANK_SEED, SHIFT_SEED, SHIFT_SCALE = 2207, 2208, 0.25
MODES = ("replace", "append", "interpolate", "cov", "joint")
RATES = (0.5, 1.0)


def load():
    sys.path.insert(0, REF)                     # its own imports: model/, tools/
    spec = importlib.util.spec_from_file_location("ref_remix_train", os.path.join(REF, "train_remix_k-fold.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def shift_bank():
    return (np.random.RandomState(SHIFT_SEED).standard_normal((S, K, V, D)) * SHIFT_SCALE).astype(np.float32)


def main():
    ref = load()
    # bags share K "morphologies" (each bag holds them in an order of its own, plus unit noise), so every prototype has one clear partner
    rs = np.random.RandomState(BANK_SEED)
    base = rs.standard_normal((K, D)) * 2.0
    protos = np.stack([base[rs.permutation(K)] + rs.standard_normal((K, D)) for _ in range(S)]).astype(np.float32)
    labels = np.asarray(LABELS, dtype=np.int64)
    shifts = shift_bank()
    # c(i) must be unambiguous: for every pair of bags, every row's best and second-best partner distances differ by more than 1e-3 relative
    for a in range(S):
        for b in range(S):
            d = np.sort(cdist(protos[a], protos[b]), axis=1)
            assert ((d[:, 1] - d[:, 0]) > 1e-3 * d[:, 1]).all(), (a, b)
    fix = {"prototypes": protos, "labels": labels, "shift_seed": np.int64(SHIFT_SEED), "shift_scale": np.float64(SHIFT_SCALE),
           "shift_shape": np.asarray([S, K, V, D], dtype=np.int64)}
    names = []
    for i, (mode, rate) in enumerate((m, r) for m in MODES for r in RATES):
        # the first seed from 4100 + 10 i on whose partner is another bag (even cases; odd ones take their seed as it comes: 4 of them mix a
        # bag with itself, which the reference allows)
        seed, idx = 4100 + 10 * i, (0, 2, 3, 1)[i % 4]
        same = np.argwhere(labels == labels[idx]).reshape(-1)                            # mix_the_bag_aug, lines 113-116
        while True:
            np.random.seed(seed)
            feats = protos[idx][np.random.permutation(K)]                               # get_bag_feats_v2, line 36
            selected = np.random.choice(same)
            if selected != idx or i % 2 == 1:
                break
            seed += 1
        strength = np.random.uniform(0, 1)
        out = ref.mix_aug(feats, protos[selected], mode=mode, rate=rate, strength=strength,
                          shift=shifts[selected].astype(np.float64) if mode in ("joint", "cov") else None)
        name = f"{mode}.{rate}"
        names.append(name)
        fix[name + ".seed"], fix[name + ".idx"] = np.int64(seed), np.int64(idx)
        fix[name + ".partner"], fix[name + ".strength"] = np.int64(selected), np.float64(strength)      # (recorded for diagnosis; the tests draw their own)
        fix[name + ".out"] = np.asarray(out).astype(np.float32)
        print(name, "seed", seed, "bag", idx, "partner", int(selected), "rows", out.shape[0], out.dtype)
    fix["cases"] = np.asarray(names)
    os.makedirs(os.path.join(HERE, "mil"), exist_ok=True)
    path = os.path.join(HERE, "mil", "reference_remix.npz")
    np.savez_compressed(path, **fix)
    print("wrote", path, os.path.getsize(path), "bytes,", len(fix), "arrays")


if __name__ == "__main__":
    main()
