"""What the GIN slot tests share (no test functions): nine small homogeneous slides (one node type, one relation, self-loops; 16-d features),
their loader, and slot capacities.

Slides 0-5: 40, 90, 55, 70, 62 and 48 nodes, four random in-edges per node and a self-loop.  Slide 6 is ONE node with a self-loop (a
train-mode BatchNorm cannot run on it), slides 7 and 8 have 37 and 38 nodes: at node drop probability 0.5 fewer than two of n nodes
survive with probability (n + 1) / 2^n, which is above 2^-32 at 37 and below it at 38."""
import torch

IN_DIM, HIDDEN, CLASSES = 16, 8, 2
SIZES = [40, 90, 55, 70, 62, 48, 1, 37, 38]
LABELS = [1, 0, 1, 1, 0, 0, 1, 0, 1]
ONE, N37, N38 = 6, 7, 8
WIDE = ((400,), (2000,), 2)                   # a slot in which the filler holds more rows than any batch of two slides
SETTINGS = [("sum", "sum"), ("mean", "att"), ("max", "mean")]          # (neighbour reducer, readout)


def slides():
    from wsi_hgnn_amd.graph import HeteroGraph
    out = []
    for i, n in enumerate(SIZES):
        gen = torch.Generator().manual_seed(4100 + i)
        dst = torch.arange(n).repeat_interleave(4) if n > 1 else torch.zeros(0, dtype=torch.int64)
        src = torch.randint(0, n, (dst.numel(),), generator=gen)
        loops = torch.arange(n)
        g = HeteroGraph.homogeneous(n, torch.cat([src, loops]), torch.cat([dst, loops]))
        g.ndata["feat"] = torch.randn(n, IN_DIM, generator=gen)
        out.append(g)
    return out


def loader(device, augment=False, batch_size=2):
    from wsi_hgnn_amd import transforms
    from wsi_hgnn_amd.data import GraphBatchLoader
    return GraphBatchLoader(slides(), LABELS, batch_size, device, shuffle=False, resident=True, seed=5,
                            transform=transforms.reference_train_transform() if augment else None)


def model(neighbor, readout, learn_eps, dropout=0.0, seed=3):
    """GIN of the tests' shape - 2 layers, 2-layer MLPs - with BatchNorm statistics, affine terms and eps away from their initial values."""
    from wsi_hgnn_amd.models import GIN
    torch.manual_seed(seed)
    m = GIN(IN_DIM, HIDDEN, CLASSES, 2, 2, dropout, readout, neighbor, learn_eps)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            norm = "bn" in k or "batch_norms" in k
            if k.endswith("running_mean") or (norm and k.endswith(".bias")):
                v.copy_(0.3 * torch.randn(v.shape, generator=gen))
            elif k.endswith("running_var") or (norm and k.endswith(".weight")):
                v.copy_(0.5 + torch.rand(v.shape, generator=gen))
            elif k.endswith(".eps"):
                v.fill_(0.3)
    return m


def cancelling(name: str, train: bool) -> bool:
    """Parameters whose gradient is 0 in exact arithmetic - what is computed is rounding noise without a scale of its own: the bias of an
    attention gate (a softmax ignores a shift) and, in train mode, the bias of every Linear in front of a BatchNorm (the mean is
    subtracted) - all of the MLPs' Linears here."""
    return name.endswith("gate_nn.bias") or (train and ".mlp.linears." in name and name.endswith(".bias"))
