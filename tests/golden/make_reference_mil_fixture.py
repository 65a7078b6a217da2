#!/usr/bin/env python
"""Fixture produced by EXECUTING the reference's own MIL modules (baselines/ReMix_DSMIL_ABMIL/model/abmil.py, model/dsmil.py) in float64
on seeded inputs, one bag per call as the reference runs them: mil/reference_mil.npz holds the inputs, both full state_dicts, every output and
the gradients of a seeded linear functional of the outputs (summed over the bags; DSMIL's leaves the attention A out).  Data only; no reference source travels.
The file lives in a directory of its own: the *.npz files next to this script are the graph-model vectors that regen_through_reference.py
replays through DGL, and this one is already the reference's own output.

Inputs and weights are rounded to float32 first (and stored as float32), so a float32 model sees exactly the numbers the reference saw.
Re-run where the reference is checked out (needs /root/reference, as make_reference_io_fixture.py does):
``python tests/golden/make_reference_mil_fixture.py``."""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/baselines/ReMix_DSMIL_ABMIL/model"
K, C, SIZES = 16, 3, (1, 40, 129)


def load(name):
    spec = importlib.util.spec_from_file_location("ref_mil_" + name, os.path.join(REF, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def round32(model):
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.to(torch.float32).to(torch.float64))
    return model


def main():
    ab, ds = load("abmil"), load("dsmil")
    torch.manual_seed(1511)
    gen = torch.Generator().manual_seed(1511)
    n = sum(SIZES)
    x32 = torch.randn(n, K, generator=gen, dtype=torch.float32)
    off = np.concatenate([[0], np.cumsum(SIZES)])
    fix = {"sizes": np.asarray(SIZES, dtype=np.int64), "x": x32.numpy()}

    # ---- ABMIL: BClassifier(input_size, num_classes)
    m = round32(ab.BClassifier(K, C).double())
    # the freshly initialised attention is nearly flat: scale its last layer so that the softmax is peaked enough to matter
    with torch.no_grad():
        m.attention[2].weight.mul_(8.0)
    round32(m)
    x = x32.double().requires_grad_(True)
    w_y = torch.randn(len(SIZES), C, generator=gen, dtype=torch.float64)
    ys = [m(x[off[b]:off[b + 1]]) for b in range(len(SIZES))]
    Y = torch.cat(ys, 0)
    (Y * w_y).sum().backward()
    for k, v in m.state_dict().items():
        fix["abmil.sd." + k] = v.to(torch.float32).numpy()
    fix["abmil.order"] = np.asarray([k for k, _ in m.named_parameters()])
    fix["abmil.Y"], fix["abmil.w_Y"], fix["abmil.g.x"] = Y.detach().numpy(), w_y.numpy(), x.grad.numpy()
    for k, p in m.named_parameters():
        fix["abmil.g." + k] = p.grad.numpy()

    # ---- DSMIL: MILNet(FCLayer(K, C), BClassifier(K, C))
    # (as initialised: the critical instance's score of itself already dominates its bag - weights near 0.97 - without saturating the softmax)
    m = round32(ds.MILNet(ds.FCLayer(K, C), ds.BClassifier(K, C, dropout_v=0.0)).double())
    x = x32.double().requires_grad_(True)
    w = {"classes": torch.randn(n, C, generator=gen, dtype=torch.float64), "pred": torch.randn(len(SIZES), C, generator=gen, dtype=torch.float64),
         "B": torch.randn(len(SIZES), C, K, generator=gen, dtype=torch.float64)}
    outs = [m(x[off[b]:off[b + 1]]) for b in range(len(SIZES))]
    classes = torch.cat([o[0] for o in outs], 0)
    pred = torch.cat([o[1] for o in outs], 0)
    A = torch.cat([o[2] for o in outs], 0)
    B = torch.cat([o[3] for o in outs], 0)
    for b in range(len(SIZES)):                       # no two instance scores of a column tie: the critical instance is unambiguous
        c = classes[off[b]:off[b + 1]]
        for j in range(C):
            assert torch.unique(c[:, j]).numel() == c.shape[0], "tied instance scores"
    # (the functional leaves A out: the package returns A detached - the reference's objective never differentiates it)
    ((classes * w["classes"]).sum() + (pred * w["pred"]).sum() + (B * w["B"]).sum()).backward()
    for k, v in m.state_dict().items():
        fix["dsmil.sd." + k] = v.to(torch.float32).numpy()
    fix["dsmil.order"] = np.asarray([k for k, _ in m.named_parameters()])
    for k, v in (("classes", classes), ("pred", pred), ("A", A), ("B", B)):
        fix["dsmil." + k] = v.detach().numpy()
        if k in w:
            fix["dsmil.w_" + k] = w[k].numpy()
    fix["dsmil.g.x"] = x.grad.numpy()
    for k, p in m.named_parameters():
        fix["dsmil.g." + k] = p.grad.numpy()

    os.makedirs(os.path.join(HERE, "mil"), exist_ok=True)
    path = os.path.join(HERE, "mil", "reference_mil.npz")
    np.savez_compressed(path, **fix)
    print("wrote", path, os.path.getsize(path), "bytes,", len(fix), "arrays")


if __name__ == "__main__":
    main()
