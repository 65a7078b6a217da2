"""wsi-hgnn_amd: MI355X-native hot path of HKU-MedAI/WSI-HGNN (HEAT message passing + readout).

Import as ``wsi_hgnn_amd`` (alias package at the repo root).  Layout:
  graph.py      HeteroGraph container + CSR/CSC kernel plan (replaces the DGLGraph argument)
  synthetic.py  synthetic WSI patch graphs of the BASELINE shapes
  csrc/         hand-written HIP kernels for gfx950 + the C-ABI (include/wsi_hgnn.h)
  _native.py    ctypes loader of csrc/libwsi_hgnn.so (fails loudly when missing)
  ops.py        torch.autograd.Function wrappers calling the C-ABI
  models/, pooling/   nn.Module mirror of the reference's models/* and pooling/* API
  mil/          the multiple-instance-learning baselines (ABMIL, DSMIL) over batches of bags: bag softmax pooling in HIP
  gtn/          the graph-transformer baseline (GTNMIL) over a packed batch: mincut assignment over a sparse adjacency and short-sequence attention in HIP
  h2mil/        the hierarchical baseline (H2MIL) over packed slide trees: RAConv's two-level attention and IHPool's cluster assignment in HIP
  metrics.py    per-epoch classification metrics accumulated on the device (one recordable launch per step, one read-back per epoch)
  dist.py       WSI-sharded data parallelism (RCCL gradient all-reduce)
"""
from .graph import HeteroGraph, GraphPlan, batch, to_homogeneous, permute_nodes, remove_nodes, locality_order, apply_locality_order, leave_one_out_batch, leave_one_out_tables  # noqa: F401
