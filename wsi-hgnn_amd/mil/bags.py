"""Bag plans: which contiguous rows of a [N, L] feature table belong to which bag (``ops.ReducePlan`` chunk tables, built once per batch)."""
from __future__ import annotations

from typing import Optional, Sequence, Union

import torch

from .. import ops
from ..graph import HeteroGraph


def _graph_sizes(g: HeteroGraph):
    if len(g.ntypes) != 1:
        raise ValueError("a bag batch needs a homogeneous graph batch (one node type): its graphs are the bags")
    return [int(c) for c in g.batch_num_nodes(g.ntypes[0]).tolist()]


def bag_plan(bags: Union[Sequence[int], torch.Tensor, HeteroGraph], device, chunk: int = 128) -> ops.ReducePlan:
    """The plan of a batch of bags laid out one after the other: ``bags`` = the row count of every bag (empty bags allowed), or a
    homogeneous ``HeteroGraph`` batch whose graphs are the bags (edges are ignored).  ``chunk`` = rows per workgroup of the pooling kernels."""
    if isinstance(bags, HeteroGraph):
        sizes = _graph_sizes(bags)
    else:
        sizes = [int(c) for c in (bags.tolist() if isinstance(bags, torch.Tensor) else bags)]
    if any(c < 0 for c in sizes):
        raise ValueError("bag_plan: negative bag size")
    ptr = [0]
    for c in sizes:
        ptr.append(ptr[-1] + c)
    return ops.ReducePlan.from_ptr(ptr, device, chunk)


def rows_and_plan(x, bags: Optional[ops.ReducePlan]):
    """(rows [N, L] fp32, plan) of a forward's input: a tensor alone is one bag; a graph batch brings its own bags."""
    if isinstance(x, HeteroGraph):
        h = x.ndata["feat"].to(torch.float32)
        if bags is None:
            cache = x.__dict__.setdefault("_bag_plans", {})
            bags = cache.get(str(h.device))
            if bags is None:
                bags = cache[str(h.device)] = bag_plan(x, h.device)
    else:
        h = x.to(torch.float32)
        if h.dim() != 2:
            h = h.reshape(h.shape[0], -1)
        if bags is None:
            bags = bag_plan([h.shape[0]], h.device)
    if bags.first_row != 0 or bags.num_rows != h.shape[0]:
        raise ValueError(f"the bag plan covers {bags.num_rows} rows, the input has {h.shape[0]}")
    return h, bags
