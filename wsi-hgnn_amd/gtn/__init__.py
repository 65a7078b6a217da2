"""The graph-transformer baseline of the reference (``baselines/GTNMIL``): GCNBlock -> mincut pooling -> transformer, over a PACKED batch.

The reference pads every slide to the largest one and multiplies a dense [B, Nmax, Nmax] adjacency twice; here the rows of all slides lie one
after the other and the adjacency is a list of entries (``GraphBatch``; ``from_dense`` converts the reference's padded tensors).  The
projection runs on the MFMA GEMM, the aggregation on ``wsi_spmm_sum``, the assignment with its two regularisers on ``ops.mincut_assign``, the
pooled products on one grouped GEMM, the transformer's attention on ``ops.seq_attention``.  Not built: ``relprop`` / GraphCAM, the attention
hooks, the k-fold scripts, the feature extractor.
"""
from .batch import GraphBatch, as_batch, from_dense
from .gcn import GCNBlock, dense_mincut_pool
from .ViT import VisionTransformer
from .GraphTransformer import Classifier, train_one_step

__all__ = ["GraphBatch", "as_batch", "from_dense", "GCNBlock", "dense_mincut_pool", "VisionTransformer", "Classifier", "train_one_step"]
