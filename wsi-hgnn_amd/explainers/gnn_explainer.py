"""GNNExplainer (https://arxiv.org/abs/1903.03894) as the reference implements it (``explainers/gnn_explainer.py``): a per-edge mask
and a per-node mask are trained through the FROZEN model so that the masked graph keeps the model's prediction while the masks
shrink (size and entropy regularisers).

The reference swaps the graph's class for one whose ``update_all`` multiplies every message by ``sigmoid(edge_mask)``
(gnn_explainer.py:21-33).  Here the same factor is attached to the graph with ``graph.message_scale`` and applied inside the HIP
aggregation kernels (``wsi_spmm_sum`` + ``wsi_sddmm_dot`` for GraphConv, ``wsi_gat_attn_fwd_scaled`` / ``_bwd_scaled`` for GATConv),
which also return its gradient: one epoch is one forward and one backward over the whole slide, nothing per edge goes through
eager tensors.  Same constructor, ``params``, method names and return values as the reference class.

Differences, all deliberate:
* ``explain_node`` takes ``node_idx=None`` only (graph classification, the evaluator's only call, evaluator/explain_graphs.py);
  the mirrored models return one row per graph, so there is no per-node logit to explain (gnn_explainer.py:125-136 is omitted).
* the model's parameters are frozen (``requires_grad_(False)``, restored afterwards) while the masks train: their gradients are never
  computed, where the reference computes and ignores them.  The masks do not depend on it.
* the constructor's ``edge_size`` / ``feat_size`` go into a per-instance copy of ``params`` (the reference writes them into the class
  attribute, gnn_explainer.py:64-65, so one explainer's arguments leak into the next).
* ``history`` (the loss of every epoch) replaces the progress bar; it is read from the device once, after the loop.
* omitted: ``_visualize`` / ``visualize`` (networkx + matplotlib plotting, gnn_explainer.py:229-276).
"""
from __future__ import annotations

from math import sqrt
from typing import Dict, List

import torch
import torch.nn as nn

from ..graph import HeteroGraph, message_scale


class ExplainerTags:                                        # gnn_explainer.py:15-18
    ORIGINAL_ID = '_explainer_original_id'
    EDGE_MASK = '_explainer_edge_mast'
    NODE_FEATURES = 'feat'


def _mean_entropy(m: torch.Tensor, eps: float) -> torch.Tensor:
    """Mean binary entropy of a mask whose values lie in [0, 1]; ``eps`` inside both logarithms keeps 0 and 1 finite."""
    keep, drop = m, 1.0 - m
    return -(keep * (keep + eps).log() + drop * (drop + eps).log()).mean()


def mask_loss(pred_loss: torch.Tensor, edge_prob: torch.Tensor, node_prob: torch.Tensor, params: Dict[str, float]) -> torch.Tensor:
    """The prediction loss plus the four regularisers of gnn_explainer.py:91-101 on the two masks AFTER their sigmoid: the edge
    size is a SUM over edges (:93), the node size and both entropies are means (:95, :99, :101)."""
    eps = params['eps']
    edge_terms = params['edge_size'] * edge_prob.sum() + params['edge_ent'] * _mean_entropy(edge_prob, eps)
    node_terms = params['feat_size'] * node_prob.mean() + params['feat_ent'] * _mean_entropy(node_prob, eps)
    return pred_loss + edge_terms + node_terms


class GNNExplainer:
    # hyper parameters, taken from the original paper (gnn_explainer.py:38-44)
    params = {
        'edge_size': 0.005,
        'feat_size': 0.5,
        'edge_ent': 1.0,
        'feat_ent': 0.1,
        'eps': 1e-15
    }

    def __init__(self, graph: HeteroGraph, model: nn.Module, num_hops: int,
                 epochs: int = 100, lr: float = 0.01,
                 mask_threshold: float = 0.5, edge_size: float = 0.005, feat_size: float = 0.1):
        self.g = graph
        self.model = model
        self.epochs = epochs
        self.lr = lr
        self.threshold = mask_threshold
        self.num_hops = num_hops
        self.node_mask = None
        self.params = dict(type(self).params)               # :64-65, on a copy (module doc)
        self.params['edge_size'] = edge_size
        self.params['feat_size'] = feat_size
        self.nfeat = ExplainerTags.NODE_FEATURES
        self.history: List[float] = []
        for module in self.model.modules():                 # :67-69
            if hasattr(module, '_allow_zero_in_degree'):
                module._allow_zero_in_degree = True

    def __set_masks__(self, g: HeteroGraph):
        """Fresh masks (gnn_explainer.py:71-77).  Draw order and placement are part of the behaviour: N normals for the node mask
        first, then E for the edge mask, both from the CPU generator and only then moved, so ``torch.manual_seed`` gives the draws it
        gives there.  Node mask: std 0.1.  Edge mask: std gain('relu') * sqrt(2 / (2 N)); it lives in ``g.edata[EDGE_MASK]``."""
        dev = self.g.device
        n, e = g.num_nodes(), g.num_edges()
        node_draw = torch.randn(n)
        edge_draw = torch.randn(e)
        edge_std = nn.init.calculate_gain('relu') * sqrt(2.0 / (2 * n))
        self.node_mask = nn.Parameter(node_draw.to(dev) * 0.1)
        g.edata[ExplainerTags.EDGE_MASK] = nn.Parameter(edge_draw.to(dev) * edge_std)

    @staticmethod
    def __apply_feature_mask__(feat, mask):
        """Soft node mask (:79-82): row i of ``feat`` times sigmoid(mask[i])."""
        return torch.sigmoid(mask).unsqueeze(-1) * feat

    def __loss__(self, g, node_idx, log_logits, pred_label):
        """:84-103 for graph classification: minus the logit of the predicted class, plus ``mask_loss``'s regularisers."""
        if node_idx is not None:
            raise NotImplementedError(_NODE_IDX)
        pred_loss = -log_logits.view(-1)[pred_label]
        return mask_loss(pred_loss, torch.sigmoid(g.edata[ExplainerTags.EDGE_MASK]), torch.sigmoid(self.node_mask), self.params)

    def _predict(self, graph, model, node_id, feat_mask=None):
        """(logits, predicted class) of ``model`` in eval mode without gradients, on ``graph``'s features times ``feat_mask`` when
        one is given (:105-117).  ``explain_node`` returns one value per node, so a 1-d mask multiplies rows."""
        if node_id is not None:
            raise NotImplementedError(_NODE_IDX)
        x = graph.ndata[self.nfeat]
        if feat_mask is not None:
            w = torch.as_tensor(feat_mask, device=x.device)
            x = x * (w.unsqueeze(-1) if w.dim() == 1 else w)
        model.eval()
        with torch.no_grad():
            logits = model(graph, x)
        return logits, logits.argmax(dim=-1)

    def _create_subgraph(self, node_idx):
        """:119-123: for graph classification the "subgraph" is a copy of the whole graph (own frames; the index and feature tensors are
        shared, nothing writes into them) with the original node ids attached."""
        if node_idx is not None:
            raise NotImplementedError(_NODE_IDX)
        g = self.g
        sub_g = HeteroGraph(g._num_nodes, g._edges, g._batch_num_nodes)
        for t in g.ntypes:
            sub_g._nframes[t].update(g._nframes[t])
        for r in g.canonical_etypes:
            sub_g._eframes[r].update(g._eframes[r])
        sub_g.ndata[ExplainerTags.ORIGINAL_ID] = torch.arange(g.num_nodes(), dtype=torch.int, device=g.device)
        return sub_g

    def explain_node(self, node_idx):
        """:138-200 for ``node_idx=None``.  Returns (subgraph, node_mask): the graph copy with the trained raw edge mask in
        ``edata[ExplainerTags.EDGE_MASK]`` and the ids in ``ndata[ExplainerTags.ORIGINAL_ID]``, and sigmoid(node mask) as a NumPy array."""
        if node_idx is not None:
            raise NotImplementedError(_NODE_IDX)
        self.model.eval()
        with torch.no_grad():                                               # :141-144, the class to preserve, taken once from model(g)
            target = self.model(self.g).argmax(dim=-1)
        subgraph = self._create_subgraph(None)
        self.__set_masks__(subgraph)
        edge_mask = subgraph.edata[ExplainerTags.EDGE_MASK]
        feat = subgraph.ndata[self.nfeat]
        optimizer = torch.optim.Adam([self.node_mask, edge_mask], lr=self.lr)           # :167
        frozen = [p for p in self.model.parameters() if p.requires_grad]
        for p in frozen:
            p.requires_grad_(False)
        losses = []
        try:
            for _ in range(self.epochs):                                    # :172-178
                optimizer.zero_grad()
                with message_scale(subgraph, torch.sigmoid(edge_mask)):
                    logits = self.model(subgraph, self.__apply_feature_mask__(feat, self.node_mask))
                loss = self.__loss__(subgraph, None, logits, target)
                loss.backward()
                optimizer.step()
                losses.append(loss.detach().reshape(-1))
        finally:
            for p in frozen:
                p.requires_grad_(True)
        self.history = torch.cat(losses).cpu().tolist() if losses else []   # one read-back, after the loop
        return subgraph, torch.sigmoid(self.node_mask.detach()).cpu().numpy()           # :199

    def test_explanation(self, node_id, subgraph, feat_mask):
        """Print what the explanation kept and whether the prediction survived it (the report of gnn_explainer.py:202-227, in
        our own wording): graph size, how much of ``feat_mask`` is kept, and logits and label of the model on the original graph
        and on ``subgraph`` with ``feat_mask`` applied.  Returns nothing, as there."""
        full_logits, full_label = self._predict(self.g, self.model, node_id)
        kept_logits, kept_label = self._predict(subgraph, self.model, node_id, feat_mask)
        mask = torch.as_tensor(feat_mask)
        report = [
            ("original graph", f"{self.g.num_nodes()} nodes, {self.g.num_edges()} edges"),
            ("explanation subgraph", f"{subgraph.num_nodes()} nodes, {subgraph.num_edges()} edges"),
            ("feature mask", f"{mask.numel()} entries, total weight {float(mask.sum()):.4g}"),
            ("logits, original", full_logits.tolist()),
            ("logits, explanation", kept_logits.tolist()),
            ("label, original", full_label.tolist()),
            ("label, explanation", kept_label.tolist()),
        ]
        for name, value in report:
            print(f"{name:>22}: {value}")


_NODE_IDX = ("GNNExplainer explains graph classification only (node_idx=None): the mirrored models return one row of logits per "
             "graph, so there is no per-node prediction to explain")
