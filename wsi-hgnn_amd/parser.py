"""Config -> objects, mirroring the reference's ``parser.py`` (same function names, same config keys, same error behaviour):

  parse_gnn_model(cfg["GNN"])      parser.py:48-174   the in-scope branches: GAT, GCN, GCN_NTPool, GIN, HetRGCN, HGT, HEAT2, HEAT4
  parse_optimizer(cfg["optim"], m) parser.py:15-46    adagrad / adadelta / adam / anything else -> SGD (native=True: wsi_hgnn_amd.optim's)
  parse_loss(cfg["train"])         parser.py:176-184  BCE / CE

``node_dict`` and the etype-major enumeration of ``edge_dict`` / ``etypes`` are built exactly as :107-113,122-129; a config
without a key the reference reads raises the same ``KeyError``; names the reference does not know (``HEAT``, ``HEAT3`` of
configs/COAD/HEAT*_staging.yml: orphan configs) raise its ``NotImplementedError``.  ``GAT`` (:51-68) reads its
keys in the reference's order (num_layers, num_heads, num_out_heads, in_dim, hidden_dim, out_dim, feat_drop, attn_drop,
negative_slope, graph_pooling_type) and always passes ``F.leaky_relu`` and ``residual=False``; a missing key raises
``MissingGATKey``, a ``KeyError`` with the reference's message that is also a ``NotImplementedError`` (the package refused GAT
with the latter before it had the model).  ``GIN`` (:92-102) reads in_dim, hidden_dim, out_dim, num_layers, num_mlp_layers, feat_drop,
graph_pooling_type and neighbor_pooling_type in that order and leaves ``learn_eps`` at the class default; a missing key raises
``MissingGINKey``, built the same way (tests/golden/gin/reference_gin.json holds the reference's recorded calls on its two GIN
configs).  tests/test_parser.py replays the calls the REFERENCE function makes on its own configs (tests/golden/
reference_surface.json, produced by executing parser.py:48-174 with recording stand-ins for the classes).
"""
from __future__ import annotations

import torch.nn.functional as F
from torch import nn, optim

from .models import GAT, GCN, GIN, HGT, HEATNet2, HEATNet4, HeteroRGCN, NTPoolGCN


def parse_optimizer(config_optim, model, native=False, device_lr=False):
    """parser.py:15-46.  ``native=False``: the ``torch.optim`` classes, as the reference builds them.  ``native=True``: the same branch with the
    same arguments from ``wsi_hgnn_amd.optim`` - every parameter of the model stepped in one HIP launch.  ``device_lr=True`` (with
    ``native=True`` only): the rate is ``optim.lr_word(lr, device of the model's parameters)``, read by the launch on the device, and Adam and
    Adagrad are built ``capturable=True`` - what a captured step needs to follow a ``torch.optim.lr_scheduler`` without being recorded again."""
    opt_method = config_optim["opt_method"].lower()
    alpha = config_optim["lr"]
    weight_decay = config_optim["weight_decay"]
    if native:
        from . import optim as O
    else:
        O = optim
    counts = {}
    if device_lr:
        if not native:
            raise ValueError("parse_optimizer: device_lr=True builds wsi_hgnn_amd.optim's classes (native=True); torch.optim's own optimizers "
                             "take a tensor lr themselves (lr=torch.tensor(...), capturable=True)")
        first = next(iter(model.parameters()), None)
        alpha = O.lr_word(alpha, None if first is None else first.device)
        counts = {"capturable": True}                               # (the rules that read the count take a word with a device count only)
    if opt_method == "adagrad":
        return O.Adagrad(model.parameters(), lr=alpha, lr_decay=weight_decay, weight_decay=weight_decay, **counts)    # (lr_decay = weight_decay: parser.py:23)
    if opt_method == "adadelta":
        return O.Adadelta(model.parameters(), lr=alpha, weight_decay=weight_decay)
    if opt_method == "adam":
        return O.Adam(model.parameters(), lr=alpha, weight_decay=weight_decay, **counts)
    return O.SGD(model.parameters(), lr=alpha, weight_decay=weight_decay)


def _typed_schema(config_gnn):
    n_node_types = config_gnn["n_node_types"]
    etypes = config_gnn["edge_types"]
    canonical_etypes = [(str(s), r, str(t)) for r in etypes for s in range(n_node_types) for t in range(n_node_types)]   # etype-major
    node_dict = {str(i): i for i in range(n_node_types)}
    return node_dict, canonical_etypes


class MissingGATKey(KeyError, NotImplementedError):
    """A key the reference's GAT branch reads is missing: the reference's ``KeyError`` (same message), and a ``NotImplementedError``
    as the package's earlier refusal of GAT was."""


class MissingGINKey(KeyError, NotImplementedError):
    """The same for the GIN branch: the reference's ``KeyError``, and the ``NotImplementedError`` with which the package refused GIN before it
    had the model."""


class _Config:
    def __init__(self, config_gnn, missing):
        self._cfg, self._missing = config_gnn, missing

    def __getitem__(self, key):
        try:
            return self._cfg[key]
        except KeyError:
            raise self._missing(key) from None


def _parse_gat(config_gnn):
    c = _Config(config_gnn, MissingGATKey)                          # parser.py:51-68, keys read in this order
    n_layers = c["num_layers"]
    n_heads = c["num_heads"]
    n_out_heads = c["num_out_heads"]
    heads = ([n_heads] * n_layers) + [n_out_heads]
    return GAT(n_layers=c["num_layers"], in_dim=c["in_dim"], hidden_dim=c["hidden_dim"], out_dim=c["out_dim"], heads=heads,
               activation=F.leaky_relu, feat_drop=c["feat_drop"], attn_drop=c["attn_drop"], negative_slope=c["negative_slope"],
               residual=False, graph_pooling_type=c["graph_pooling_type"])


def parse_gnn_model(config_gnn):
    gnn_name = config_gnn["name"]
    if gnn_name == "GAT":
        return _parse_gat(config_gnn)
    if gnn_name == "GIN":
        c = _Config(config_gnn, MissingGINKey)                      # parser.py:92-102, keys read in this order
        return GIN(input_dim=c["in_dim"], hidden_dim=c["hidden_dim"], out_dim=c["out_dim"], num_layers=c["num_layers"],
                   num_mlp_layers=c["num_mlp_layers"], final_dropout=c["feat_drop"], graph_pooling_type=c["graph_pooling_type"],
                   neighbor_pooling_type=c["neighbor_pooling_type"])
    if gnn_name == "GCN":
        return GCN(in_dim=config_gnn["in_dim"], hidden_dim=config_gnn["hidden_dim"], out_dim=config_gnn["out_dim"],
                   n_layers=config_gnn["num_layers"], activation=F.relu, dropout=config_gnn["feat_drop"],
                   graph_pooling_type=config_gnn["graph_pooling_type"])
    if gnn_name == "GCN_NTPool":
        node_dict = {str(i): i for i in range(config_gnn["n_node_types"])}
        return NTPoolGCN(in_dim=config_gnn["in_dim"], hidden_dim=config_gnn["hidden_dim"], out_dim=config_gnn["out_dim"],
                         node_dict=node_dict, n_layers=config_gnn["num_layers"], activation=F.relu, dropout=config_gnn["feat_drop"],
                         graph_pooling_type=config_gnn["graph_pooling_type"])
    if gnn_name == "HetRGCN":
        node_dict, canonical_etypes = _typed_schema(config_gnn)
        etypes = {et: str(i) for i, et in enumerate(canonical_etypes)}
        return HeteroRGCN(in_dim=config_gnn["in_dim"], hidden_dim=config_gnn["hidden_dim"], out_dim=config_gnn["out_dim"],
                          n_layers=config_gnn["num_layers"], etypes=etypes, node_dict=node_dict,
                          graph_pooling_type=config_gnn["graph_pooling_type"])
    if gnn_name == "HGT":
        node_dict, canonical_etypes = _typed_schema(config_gnn)
        edge_dict = {et: i for i, et in enumerate(canonical_etypes)}
        return HGT(node_dict, edge_dict, in_dim=config_gnn["in_dim"], hidden_dim=config_gnn["hidden_dim"], out_dim=config_gnn["out_dim"],
                   n_layers=config_gnn["num_layers"], n_heads=config_gnn["num_heads"])
    if gnn_name in ("HEAT2", "HEAT4"):
        node_dict = {str(i): i for i in range(config_gnn["n_node_types"])}
        cls = HEATNet2 if gnn_name == "HEAT2" else HEATNet4
        return cls(in_dim=config_gnn["in_dim"], hidden_dim=config_gnn["hidden_dim"], out_dim=config_gnn["out_dim"],
                   n_layers=config_gnn["num_layers"], n_heads=config_gnn["n_heads"], node_dict=node_dict,
                   dropuout=config_gnn["feat_drop"], graph_pooling_type=config_gnn["graph_pooling_type"])
    raise NotImplementedError("This GNN model is not implemented")


def parse_loss(config_train):
    loss_name = config_train["loss"]
    if loss_name == "BCE":
        return nn.BCELoss()
    if loss_name == "CE":
        return nn.CrossEntropyLoss()
    raise NotImplementedError("This Loss is not implemented")
