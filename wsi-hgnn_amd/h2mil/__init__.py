"""The H2MIL baseline of the reference (``baselines/H2MIL``): RAConv -> IHPool -> RAConv -> IHPool over three-level slide trees, as a PACKED batch.

The reference needs torch_geometric, torch_scatter and torch_sparse to execute one layer, handles one slide at a time, matches every edge
against every (destination, source type) group with an [E, groups] broadcast, coarsens through a dense [N, N] adjacency and loops in Python
over the level-1 clusters.  Here the slides of a batch lie one after the other (``TreeBatch``; ``from_slides`` builds one from tensors named as
the reference's ``Data`` fields, ``from_grid`` from patch features and grid tables, the trees made on the device), RAConv's two-level
attention is ``ops.ra_attention`` (``wsi_ra_attn_fwd`` / ``_bwd``) behind one projection
GEMM, and IHPool assigns every node of every substructure of every slide in one launch per level (``wsi_ihpool_assign``) with one small
read-back per layer.  ``kernels=False`` runs the same model through tensor operations, on any device and in any dtype.
Not built, and not stubbed: ``return_attention_weights``, ``heads > 1``, the k-fold / staging / typing scripts (the same model under another
``no_of_class``) and ``WSI_processing/``.
"""
from .batch import TreeBatch, from_grid, from_slides, tables_from_names
from .RAConv import RAConv, ra_attention_tensor
from .IHPool import IHPool, level1_step, seed_count
from .model import H2MIL, GraphLayerNorm, loss_fn, train_one_step

__all__ = ["TreeBatch", "from_slides", "from_grid", "tables_from_names", "RAConv", "ra_attention_tensor", "IHPool", "level1_step", "seed_count", "H2MIL", "GraphLayerNorm",
           "loss_fn", "train_one_step"]
