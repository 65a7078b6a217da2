#!/usr/bin/env python
"""Fixture produced by EXECUTING the reference's own transformer (baselines/GTNMIL/models/ViT.py::VisionTransformer, with models/layers.py)
in float64 on a seeded input: gtn/reference_vit.npz holds the input, the full state_dict, the logits and the gradients of a seeded linear
functional of the logits with respect to the input and every parameter.  Data only; no reference source travels.

Weights and the input are rounded to float32 first (and stored as float32), so a float32 model sees exactly the numbers the reference saw.
The freshly constructed reference model keeps torch's default initialisation (its ``_init_weights`` is commented out); LayerNorm weights and
biases are perturbed so that they matter.  Re-run where the reference is checked out (needs /root/reference and einops):
``python tests/golden/make_reference_gtn_fixture.py``."""
import importlib
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/baselines/GTNMIL/models"
CONFIG = dict(num_classes=3, embed_dim=32, depth=2, num_heads=4)
SHAPE = (3, 11, 32)


def load_vit():
    """models/ViT.py imported as a member of a stand-in package (its ``from .layers import *`` needs one; the real package's
    GraphTransformer.py needs torch_geometric, which this never touches)."""
    pkg = types.ModuleType("ref_gtn_models")
    pkg.__path__ = [REF]
    pkg.__spec__ = importlib.machinery.ModuleSpec("ref_gtn_models", None, is_package=True)
    pkg.__spec__.submodule_search_locations = [REF]
    sys.modules["ref_gtn_models"] = pkg
    return importlib.import_module("ref_gtn_models.ViT")


def main():
    vit = load_vit()
    torch.manual_seed(1711)
    gen = torch.Generator().manual_seed(1711)
    m = vit.VisionTransformer(**CONFIG).double()
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "norm" in k:
                p.add_(0.1 * torch.randn(p.shape, generator=gen, dtype=torch.float64))
            p.copy_(p.to(torch.float32).to(torch.float64))
    x32 = torch.randn(*SHAPE, generator=gen, dtype=torch.float32)
    w = torch.randn(SHAPE[0], CONFIG["num_classes"], generator=gen, dtype=torch.float64)
    x = x32.double().requires_grad_(True)
    logits = m(x)
    (logits * w).sum().backward()
    fix = {"x": x32.numpy(), "w": w.numpy(), "logits": logits.detach().numpy(), "g.x": x.grad.numpy(),
           "config": np.asarray([CONFIG[k] for k in ("num_classes", "embed_dim", "depth", "num_heads")], dtype=np.int64),
           "keys": np.asarray(list(m.state_dict().keys()))}
    for k, v in m.state_dict().items():
        fix["sd." + k] = v.to(torch.float32).numpy()
    for k, p in m.named_parameters():
        fix["g." + k] = p.grad.numpy()
    out = os.path.join(HERE, "gtn", "reference_vit.npz")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **fix)
    print(out, os.path.getsize(out), "bytes;", len(fix["keys"]), "state_dict keys")


if __name__ == "__main__":
    main()
