#!/usr/bin/env python
"""Fixture produced by EXECUTING the reference's own transformer (baselines/GTNMIL/models/ViT.py::VisionTransformer with models/layers.py,
imported as make_reference_gtn_fixture.py does) through the GraphCAM procedure of models/GraphTransformer.py:82-101: per class c the scalar
``out[c].detach() * out[c]`` of ``out = softmax(logits)`` is back-propagated (the attention hooks keep d/d attn) and
``relprop(one_hot, method="transformer_attribution", start_layer=0, alpha=1)`` returns the cluster map.  gtn/reference_graphcam.npz holds data
only; no reference source travels.

Run in float64, batch 1, weights and inputs rounded to float32 first (and stored as float32), LayerNorm parameters perturbed.  Two shapes
(n, E, depth, heads, classes), one seeded model each (its state_dict is stored once per shape, which keeps the file in the size class of
reference_vit.npz) and six seeded inputs:
  small (11, 32, 2, 4, 3): per seed and class the cluster map [n - 1], every block's ``attn_cam`` and d/d attn [heads, n, n] (these two
        rounded to float32 for the file's size: 6e-8 of an entry, against the tests' bound of 1e-6 of the largest);
  ref   (101, 64, 3, 8, 3), the reference's own shape: the cluster maps only.
``e32`` [seeds, classes]: the same reference code run in float32 on the CPU, as the largest difference of its cluster map from the float64
one over the largest float64 entry - the chain divides by signed sums (attn v, q k^T, A + B), so this is how ill-conditioned float32 is in
the reference itself.  A seed whose e32 exceeds 1e-2 for any class is replaced by the next one.  Re-run where the reference is checked out
(the path make_reference_gtn_fixture.py names; needs einops): ``python tests/golden/make_reference_graphcam_fixture.py``."""
import os

import numpy as np
import torch

from make_reference_gtn_fixture import load_vit

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {"small": (11, 32, 2, 4, 3), "ref": (101, 64, 3, 8, 3)}
MODEL_SEED = {"small": 1801, "ref": 1802}
FIRST_INPUT_SEED = {"small": 100, "ref": 200}
SEEDS = 6
E32_MAX = 1e-2


def graphcam(model, x, classes, keep_blocks):
    """GraphTransformer.py:82-101 on the transformer alone, in the dtype of the model."""
    x = x.clone().requires_grad_(True)                      # (the attention hooks are registered only when the input requires a gradient)
    out = torch.softmax(model(x), -1)
    cams, attn_cams, attn_grads = [], [], []
    for c in range(classes):
        one_hot = torch.zeros(1, classes, dtype=x.dtype)
        one_hot[0, c] = out[0, c].detach()
        model.zero_grad()
        torch.sum(one_hot * out).backward(retain_graph=True)
        cam = model.relprop(one_hot.clone(), method="transformer_attribution", is_ablation=False, start_layer=0, alpha=1)
        cams.append(cam.detach()[0])
        if keep_blocks:
            attn_cams.append(torch.stack([b.attn.get_attn_cam().detach()[0] for b in model.blocks]))
            attn_grads.append(torch.stack([b.attn.get_attn_gradients().detach()[0] for b in model.blocks]))
    return out.detach()[0], torch.stack(cams), (torch.stack(attn_cams), torch.stack(attn_grads)) if keep_blocks else None


def main():
    vit = load_vit()
    fix = {"shapes": np.asarray(list(SHAPES))}
    for tag, (n, E, depth, heads, classes) in SHAPES.items():
        torch.manual_seed(MODEL_SEED[tag])
        gen = torch.Generator().manual_seed(MODEL_SEED[tag])
        m = vit.VisionTransformer(num_classes=classes, embed_dim=E, depth=depth, num_heads=heads).double()
        with torch.no_grad():
            for k, p in m.named_parameters():
                if "norm" in k:
                    p.add_(0.1 * torch.randn(p.shape, generator=gen, dtype=torch.float64))
                p.copy_(p.to(torch.float32).to(torch.float64))
        m32 = vit.VisionTransformer(num_classes=classes, embed_dim=E, depth=depth, num_heads=heads)
        m32.load_state_dict({k: v.to(torch.float32) for k, v in m.state_dict().items()})
        seeds, xs, probs, cams, blocks, e32s = [], [], [], [], [], []
        seed = FIRST_INPUT_SEED[tag]
        while len(seeds) < SEEDS:
            x32 = torch.randn(1, n, E, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)
            prob, cam, kept = graphcam(m, x32.double(), classes, tag == "small")
            _, cam32, _ = graphcam(m32, x32, classes, False)
            e32 = (cam32.double() - cam).abs().amax(1) / cam.abs().amax(1)
            print(f"{tag} seed {seed}: e32 per class {[f'{v:.2e}' for v in e32.tolist()]}")
            if float(e32.max()) <= E32_MAX:
                seeds.append(seed); xs.append(x32[0]); probs.append(prob); cams.append(cam); e32s.append(e32)
                if kept:
                    blocks.append(kept)
            else:
                print("   replaced")
            seed += 1
        fix[f"{tag}.config"] = np.asarray([n, E, depth, heads, classes], dtype=np.int64)
        fix[f"{tag}.seeds"] = np.asarray(seeds, dtype=np.int64)
        fix[f"{tag}.x"] = torch.stack(xs).numpy()
        fix[f"{tag}.prob"] = torch.stack(probs).numpy()
        fix[f"{tag}.cluster_cam"] = torch.stack(cams).numpy()                       # [seeds, classes, n - 1]
        fix[f"{tag}.e32"] = torch.stack(e32s).numpy()
        if blocks:
            fix[f"{tag}.attn_cam"] = torch.stack([b[0] for b in blocks]).to(torch.float32).numpy()    # [seeds, classes, depth, heads, n, n]
            fix[f"{tag}.attn_grad"] = torch.stack([b[1] for b in blocks]).to(torch.float32).numpy()
        for k, v in m.state_dict().items():
            fix[f"{tag}.sd.{k}"] = v.to(torch.float32).numpy()
    out = os.path.join(HERE, "gtn", "reference_graphcam.npz")
    np.savez_compressed(out, **fix)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
