"""ABMIL and DSMIL over many bags restated in plain float64 torch, one bag at a time so that it is obviously the reference's arithmetic
(baselines/ReMix_DSMIL_ABMIL/model/abmil.py:23-30, model/dsmil.py:41-57), plus the shape tables the MIL tests share.

The functions take a ``state_dict`` with the reference's keys; everything is differentiable, so autograd through them gives the
reference gradients.  An empty bag has no rows to attend over: its pooled vector is 0 and its prediction the last layer's bias."""
import numpy as np
import torch
import torch.nn.functional as F

# tests/golden/mil/reference_mil.npz
FIXTURE_K, FIXTURE_C, FIXTURE_SIZES = 16, 3, (1, 40, 129)

# kernel tests: a single row, the chunk boundary (default chunk 128), two empty bags (one between non-empty ones), multi-chunk combines, a short last bag
KERNEL_SIZES = (1, 127, 128, 129, 0, 293, 0, 1061, 2)
KERNEL_CS = (1, 2, 3, 5, 8)
KERNEL_DS = (1, 3, 4, 50, 128, 512, 1024)

# model tests: empty bags in the middle and at the end
MODEL_K, MODEL_CS, MODEL_SIZES = 64, (1, 2, 5), (300, 0, 1, 129, 0)

SCALE_128 = 1.0 / float(np.sqrt(np.float32(128)))      # the reference divides by a float32 sqrt(128)


def offsets(sizes):
    o = [0]
    for n in sizes:
        o.append(o[-1] + int(n))
    return o


def to64(sd):
    return {k: torch.as_tensor(np.asarray(v), dtype=torch.float64).clone().requires_grad_(True) for k, v in sd.items()}


def softmax_pool(scores, values, sizes, scale=1.0):
    """(out [S, C, D], lse [S, C], p [N, C]) of the bag softmax pooling, bag by bag."""
    o = offsets(sizes)
    C, D = scores.shape[1], values.shape[1]
    outs, lses, ps = [], [], []
    for a, b in zip(o[:-1], o[1:]):
        if a == b:
            outs.append(values.new_zeros(C, D)); lses.append(values.new_zeros(C))
            continue
        s = scores[a:b] * scale
        lse = torch.logsumexp(s, 0)
        p = torch.exp(s - lse)
        outs.append(p.t() @ values[a:b]); lses.append(lse); ps.append(p)
    p_all = torch.cat(ps, 0) if ps else scores.new_zeros(0, C)
    return torch.stack(outs), torch.stack(lses), p_all


def abmil_forward(sd, x, sizes, scores_out=None):
    """[S, classes].  ``scores_out``: a list that receives every non-empty bag's attention scores [n, 1] with their gradient retained."""
    o = offsets(sizes)
    ys = []
    for a, b in zip(o[:-1], o[1:]):
        H = x[a:b]
        if a == b:
            ys.append(sd["classifier.0.bias"].view(1, -1))
            continue
        A = F.linear(torch.relu(F.linear(H, sd["attention.0.weight"], sd["attention.0.bias"])), sd["attention.2.weight"], sd["attention.2.bias"])
        if scores_out is not None:
            A.retain_grad()
            scores_out.append(A)
        A = F.softmax(A.t(), dim=1)
        ys.append(F.linear(A @ H, sd["classifier.0.weight"], sd["classifier.0.bias"]))
    return torch.cat(ys, 0)


def dsmil_forward(sd, x, sizes):
    """(classes [N, C], prediction_bag [S, C], A [N, C], B [S, C, K]) of MILNet(FCLayer, BClassifier)."""
    o = offsets(sizes)
    W = sd["b_classifier.fcc.weight"]
    C, K = W.shape[0], W.shape[2]
    classes, preds, As, Bs = [], [], [], []
    for a, b in zip(o[:-1], o[1:]):
        feats = x[a:b]
        if a == b:
            Bs.append(x.new_zeros(C, K)); preds.append(sd["b_classifier.fcc.bias"].view(1, -1))
            continue
        c = F.linear(feats, sd["i_classifier.fc.0.weight"], sd["i_classifier.fc.0.bias"])
        V = F.linear(feats, sd["b_classifier.v.1.weight"], sd["b_classifier.v.1.bias"])
        Q = F.linear(feats, sd["b_classifier.q.weight"], sd["b_classifier.q.bias"])
        m_idx = torch.stack([first_argmax(c[:, j]) for j in range(C)])
        q_max = F.linear(feats[m_idx], sd["b_classifier.q.weight"], sd["b_classifier.q.bias"])
        A = F.softmax((Q @ q_max.t()) * SCALE_128, 0)
        B = A.t() @ V
        preds.append((F.conv1d(B.unsqueeze(0), W, sd["b_classifier.fcc.bias"])).view(1, -1))
        classes.append(c); As.append(A); Bs.append(B)
    cat = lambda ts, w: torch.cat(ts, 0) if ts else x.new_zeros(0, w)
    return cat(classes, C), torch.cat(preds, 0), cat(As, C), torch.stack(Bs)


def first_argmax(v):
    """The first row holding the column's maximum (what a strict '>' scan keeps)."""
    return torch.nonzero(v == v.max())[0, 0]


def dsmil_loss(outputs, labels, num_classes, sizes):
    """train_tcga_k-fold.py:76-80 per bag, averaged over the non-empty bags."""
    classes, pred = outputs[0], outputs[1]
    o = offsets(sizes)
    total, live, row = 0.0, 0, 0
    for s, (a, b) in enumerate(zip(o[:-1], o[1:])):
        if a == b:
            continue
        t = target_row(labels[s], num_classes).to(pred.dtype)
        n = b - a
        mx = classes[row:row + n].max(0)[0]
        row += n
        total = total + 0.5 * F.binary_cross_entropy_with_logits(pred[s].view(1, -1), t.view(1, -1)) \
            + 0.5 * F.binary_cross_entropy_with_logits(mx.view(1, -1), t.view(1, -1))
        live += 1
    return total / max(live, 1)


def abmil_loss(pred, labels, num_classes, sizes):
    total, live = 0.0, 0
    for s, n in enumerate(sizes):
        if n == 0:
            continue
        t = target_row(labels[s], num_classes).to(pred.dtype)
        total = total + F.binary_cross_entropy_with_logits(pred[s].view(1, -1), t.view(1, -1))
        live += 1
    return total / max(live, 1)


def target_row(label, num_classes):
    """train_tcga_k-fold.py:28-35"""
    t = torch.zeros(num_classes)
    if num_classes == 1:
        t[0] = float(label)
    elif int(label) <= num_classes - 1:
        t[int(label)] = 1
    return t


def rel_err(got, want):
    """tests/test_gat_gpu.py's norm: the largest error over the largest float64 entry of the tensor."""
    want = want.detach().to(torch.float64).cpu()
    got = got.detach().to(torch.float64).cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.numel() == 0:
        return 0.0
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-30)


class Ratios:
    """Checks tensors against float64 in rel_err's norm and keeps the largest error / bound ratio per tensor name (printed by the module that
    owns it, quoted in DESIGN.md)."""

    def __init__(self, tol):
        self.tol, self.worst = tol, {}

    def check(self, got, want, what, case=""):
        ratio = rel_err(got, want) / self.tol
        print(f"{case} {what}: error / bound {ratio:.3e}")
        if ratio > self.worst.get(what, (-1.0, None))[0]:
            self.worst[what] = (ratio, case)
        assert torch.isfinite(got).all(), f"{case} {what}: not finite"
        assert ratio <= 1.0, f"{case} {what}: error {ratio:.3e} x the bound of {self.tol} x the largest reference entry"

    def report(self):
        for name, (r, case) in sorted(self.worst.items()):
            print(f"\nlargest error / bound, {name}: {r:.3e} ({case})", end="")
        print()
