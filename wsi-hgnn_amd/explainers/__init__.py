"""The reference's explainers (``explainers/__init__.py``): GNNExplainer's learnable edge and node masks (``gnn_explainer.py``) through
the HIP aggregation kernels, and the leave-one-node-out explainers (``GEM.py``, ``gem_het.py``) on the batched engine."""
from .gnn_explainer import GNNExplainer, ExplainerTags  # noqa: F401
from .gem import GemExplainer, HetGemExplainer  # noqa: F401

__all__ = ["GNNExplainer", "ExplainerTags", "GemExplainer", "HetGemExplainer"]
