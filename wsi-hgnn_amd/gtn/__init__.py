"""The graph-transformer baseline of the reference (``baselines/GTNMIL``): GCNBlock -> mincut pooling -> transformer, over a PACKED batch.

The reference pads every slide to the largest one and multiplies a dense [B, Nmax, Nmax] adjacency twice; here the rows of all slides lie one
after the other and the adjacency is a list of entries (``GraphBatch``; ``from_dense`` converts the reference's padded tensors, ``from_grid``
builds the reference's grid adjacency from patch coordinates on the device).  The
projection runs on the MFMA GEMM, the aggregation on ``wsi_spmm_sum``, the assignment with its two regularisers on ``ops.mincut_assign``, the
pooled products on one grouped GEMM, the transformer's attention on ``ops.seq_attention``.  ``graphcam.class_maps`` is the method's explainer,
GraphCAM: the reference's ``relprop`` as batched closed-form rules on ``wsi_lrp_*``.  ``GraphSlot`` / ``CapturedGraphStep`` (``slots``) hold a
batch in padded tables of one shape and replay one recorded training step over new slides.  Not built: the attention hooks, the k-fold scripts, the
feature extractor, drawing the maps over the slide.
"""
from .batch import GraphBatch, as_batch, from_dense, from_grid, read_coords
from .gcn import GCNBlock, dense_mincut_pool
from .ViT import VisionTransformer
from .GraphTransformer import Classifier, train_one_step
from . import graphcam
from .graphcam import GraphCAM, class_maps, save_reference_files
from .slots import SlideSet, GraphSlot, slot_step, CapturedGraphStep

__all__ = ["GraphBatch", "as_batch", "from_dense", "from_grid", "read_coords", "GCNBlock", "dense_mincut_pool", "VisionTransformer", "Classifier",
           "train_one_step", "graphcam", "GraphCAM", "class_maps", "save_reference_files", "SlideSet", "GraphSlot", "slot_step", "CapturedGraphStep"]
