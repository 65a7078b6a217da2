"""``localization.explain_and_score`` end to end on the GPU: two synthetic slides of about 300 patches - ``GemExplainer`` on a 1-layer GCN and
``HetGemExplainer`` on HEATNet2 - with annotation polygons drawn around a known block of patches.  The result equals scoring the returned
masks by hand on the CPU (the loop restatements of localization_cases.py), and after the explainers have run there is one read-back."""
import numpy as np
import pytest
import torch

import localization_cases as C

pytestmark = pytest.mark.gpu

N_PATCHES, COLS, PATCH = 300, 20, 256


def _dev():
    return torch.device("cuda:0")


def _slides():
    """[(graph, label, centres, annotation)] on the device, the models, and the expected labels (a block of the 20-column patch grid lies inside)."""
    import torch.nn.functional as F
    from wsi_hgnn_amd import localization as L, models, synthetic
    tiles = torch.stack([torch.arange(N_PATCHES) % COLS, torch.arange(N_PATCHES) // COLS], 1)
    _, centres = L.patch_centres(tiles, PATCH, 1)                                  # t * 512 + 256
    boxes = [(3, 9, 2, 8), (8, 17, 5, 12)]                                         # tile columns / rows [x0, x1) x [y0, y1) inside the ring
    anns, want = [], []
    for x0, x1, y0, y1 in boxes:
        anns.append(L.Annotation.from_rings([[(x0 * 512.0, y0 * 512.0), (x1 * 512.0, y0 * 512.0), (x1 * 512.0, y1 * 512.0), (x0 * 512.0, y1 * 512.0)],
                                             [(-900.0, -900.0), (-100.0, -900.0), (-500.0, -100.0)]]))
        want.append(((tiles[:, 0] >= x0) & (tiles[:, 0] < x1) & (tiles[:, 1] >= y0) & (tiles[:, 1] < y1)).to(torch.int32))
    torch.manual_seed(611)
    gcn = models.GCN(16, 32, 2, 1, F.relu, 0.0, "mean").to(_dev()).eval()
    heat = models.HEATNet2(16, 32, 2, 2, 4, {"0": 0, "1": 1, "2": 2}, 0.0, "mean").to(_dev()).eval()
    hg = synthetic.homogeneous_graph(N_PATCHES, 16, seed=3)
    het = synthetic.hetero_graph(N_PATCHES, 16, seed=4, dst_mode="hub")
    perm, at = torch.randperm(N_PATCHES, generator=torch.Generator().manual_seed(5)), 0
    for t in het.ntypes:                                                           # which patch every typed node is: a shuffled partition
        het.nodes[t].data["_ID"] = perm[at:at + het.num_nodes(t)]
        at += het.num_nodes(t)
    label = torch.tensor([1], device=_dev())
    slides = [(hg.to(_dev()), label, centres.to(_dev()), anns[0]), (het.to(_dev()), label, centres.to(_dev()), anns[1])]
    return slides, (gcn, heat), torch.cat(want)


def test_explain_and_score_equals_scoring_the_masks_by_hand(monkeypatch):
    from wsi_hgnn_amd import localization as L
    from wsi_hgnn_amd.explainers import GemExplainer, HetGemExplainer
    slides, (gcn, heat), want_labels = _slides()
    got, masks = [], []
    for slide, model in zip(slides, (gcn, heat)):                                  # one model per slide kind: one call each
        score, m = L.explain_and_score(model, [slide], explainer="GemExplainer")
        got.append(score)
        masks += m
    assert all(m.is_cuda and m.dtype == torch.float32 and m.shape == (N_PATCHES,) for m in masks)
    # the masks are the explainers' own, in patch order
    direct = GemExplainer(slides[0][0], gcn, slides[0][1]).explain_node()
    assert np.abs(masks[0].cpu().numpy() - np.asarray(direct, dtype=np.float32)).max() <= 1e-6          # (a second run of the same forwards)
    typed = HetGemExplainer(slides[1][0], heat, slides[1][1]).explain_node()
    for t, m in typed.items():
        assert (masks[1].cpu()[slides[1][0].nodes[t].data["_ID"].cpu()] - m).abs().max().item() <= 1e-6, t
    # scoring them by hand on the CPU
    sizes = [N_PATCHES, N_PATCHES]
    flat = torch.cat(masks).cpu().numpy()
    assert np.isfinite(flat).all() and 0 < want_labels[:N_PATCHES].sum() < N_PATCHES
    want = C.pair_loop(flat, want_labels.numpy(), sizes)
    auc = C.auc_of(want)
    for s in range(2):
        assert not got[s].auc.is_cuda
        assert [got[s].pos.item(), got[s].neg.item(), got[s].gt.item(), got[s].eq.item(), got[s].flags.item()] == want[s, 0].tolist()
        assert got[s].auc.item() == auc[s, 0] == got[s].mean.item()
    # both slides in one call over precomputed scores: one labelling, one scoring, and exactly one read-back
    reads = []
    for name in ("cpu", "item", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda orig, name: lambda self, *a, **k: (reads.append(name) if self.is_cuda else None, orig(self, *a, **k))[1])(orig, name))
    orig_to = torch.Tensor.to

    def to(self, *a, **k):
        out = orig_to(self, *a, **k)
        if self.is_cuda and not out.is_cuda:
            reads.append("to")
        return out
    monkeypatch.setattr(torch.Tensor, "to", to)
    both, _ = L.explain_and_score(None, slides, explainer=None, scores=masks)
    monkeypatch.undo()
    assert reads == ["cpu"], reads
    assert both.auc.tolist() == [auc[0, 0], auc[1, 0]] and both.mean.item() == C.nanmean_columns(auc)[0]
    labels = L.patch_labels(torch.cat([s[2] for s in slides]), sizes, [s[3] for s in slides])
    assert torch.equal(labels.cpu(), want_labels)


def test_graphcam_style_columns_are_scored_per_class():
    """[n, C] scores in place of an explainer (GraphCAM's ``node_heat`` has a column per class)."""
    from wsi_hgnn_amd import localization as L
    slides, _, want_labels = _slides()
    rng = np.random.RandomState(7)
    heat = [torch.from_numpy((np.floor(rng.rand(N_PATCHES, 2) * 16) / 16).astype(np.float32)).to(_dev()) for _ in slides]
    got, _ = L.explain_and_score(None, [(None, s[1], s[2], s[3]) for s in slides], explainer=None, scores=heat)
    want = C.pair_loop(torch.cat(heat).cpu().numpy(), want_labels.numpy(), [N_PATCHES] * 2)
    assert got.auc.shape == (2, 2) and np.array_equal(got.gt.numpy(), want[..., 2]) and np.array_equal(got.eq.numpy(), want[..., 3])
    assert np.array_equal(got.auc.numpy().view(np.int64), C.auc_of(want).view(np.int64))
