"""``search_depth`` (hironaka/util/search.py:9-32): against a deterministic host, how long can an adversarial agent
make the game last?  Every agent choice is enumerated depth first, on the GPU (hk_search_depth): one tree per root,
any number of roots per call.

The reference's ``search_tree`` / ``search_tree_morin`` (treelib output) and the JAX ``search_tree_fix_host`` are
not built here.
"""
from typing import NamedTuple, Optional

import torch

from .. import _abi as A
from .. import ops
from ..host import AllCoordHost, WeakSpivakovsky, WeakSpivakovskyMinHitting, Zeillinger, ZeillingerLex

DEFAULT_MAX_DEPTH = 1 << 20
DEFAULT_MAX_NODES = 1 << 24
DEFAULT_STACK_NODES = 1 << 16  # per root, for one root (the 5552-deep reference tree peaks at a few hundred)
DEFAULT_BATCH_STACK_NODES = 1 << 12  # per root of a batch; ops.search_depth splits a batch to bound the workspace

_LIMITS = ((A.HK_SEARCH_DEPTH_LIMIT, "max_depth"), (A.HK_SEARCH_NODE_LIMIT, "max_nodes"),
           (A.HK_SEARCH_STACK_LIMIT, "stack_nodes"),
           (A.HK_SEARCH_INEXACT, "the exact integer range of the dtype (2^24 for float32, 2^53 for float64)"))


class SearchDepthResult(NamedTuple):
    depth: torch.Tensor   # int32 [B]: 1 + the largest depth of a visited node (the reference's return value)
    nodes: torch.Tensor   # int64 [B]: visited nodes, root included (the reference's host.select_coord calls)
    status: torch.Tensor  # int32 [B]: 0 = exact, else an OR of A.HK_SEARCH_* bits


_SEARCH_HOSTS = {Zeillinger: "zeillinger", AllCoordHost: "all_coord", ZeillingerLex: "zeillinger_lex",
                 WeakSpivakovsky: "weak_spivakovsky", WeakSpivakovskyMinHitting: "weak_spivakovsky_min_hitting"}


def _host_name(host) -> str:
    # exact types: a subclass may override select_coord, which the kernel would not see
    name = _SEARCH_HOSTS.get(type(host))
    if name is None:
        raise TypeError("search_depth runs the host inside the GPU search: supported hosts are "
                        "hironaka_amd.host.Zeillinger and hironaka_amd.host.AllCoordHost, plus ZeillingerLex, "
                        f"WeakSpivakovsky and WeakSpivakovskyMinHitting. Got {type(host).__name__}.")
    return name


def _roots(points, dtype: Optional[torch.dtype]) -> torch.Tensor:
    if hasattr(points, "points") and isinstance(points.points, torch.Tensor):  # HipPoints
        t = points.points
    elif isinstance(points, torch.Tensor):
        t = points
    else:  # nested lists, one root [[x, ...], ...] or a batch [[[x, ...], ...]]: float32, as HipPoints
        t = torch.as_tensor(points, dtype=torch.float32 if dtype is None else dtype)
    if dtype is not None:
        t = t.to(dtype)
    elif t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float32)
    if not t.is_cuda:
        t = t.to("cuda")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    return t


def search_depths(points, host, *, max_depth: int = DEFAULT_MAX_DEPTH, max_nodes: int = DEFAULT_MAX_NODES,
                  stack_nodes: int = DEFAULT_BATCH_STACK_NODES, dtype: Optional[torch.dtype] = None) -> SearchDepthResult:
    """``search_depth`` for a batch of roots [B, m, d] (tensor, HipPoints or nested lists); the reference asserts a
    batch of one.  ``dtype`` converts the roots (nested lists default to float32; float64 keeps integers exact up to
    2^53 instead of 2^24).  Nothing is raised for a non-zero status: read ``status``."""
    depth, nodes, status = ops.search_depth(_roots(points, dtype), _host_name(host), max_depth=max_depth,
                                            max_nodes=max_nodes, stack_nodes=stack_nodes)
    return SearchDepthResult(depth, nodes, status)


def search_depth(points, host, debug=False, *, max_depth: Optional[int] = None,
                 max_nodes: Optional[int] = None, stack_nodes: Optional[int] = None) -> int:
    """The reference's ``search_depth(points, host)``: the maximal length of the game an agent can achieve against
    ``host``.  ``points``: a HipPoints of batch 1, a [m, d] or [1, m, d] tensor, or nested lists.  Raises
    RuntimeError naming the limit when the search did not finish exactly, ValueError for a root with fewer than
    2 points (the reference asserts).  ``debug`` is accepted for the reference's signature and prints nothing."""
    roots = _roots(points, None)
    if roots.shape[0] != 1:
        raise ValueError(f"search_depth searches one root (the reference asserts batch_size == 1); got a batch of "
                         f"{roots.shape[0]}: use search_depths")
    res = search_depths(roots, host, max_depth=DEFAULT_MAX_DEPTH if max_depth is None else max_depth,
                        max_nodes=DEFAULT_MAX_NODES if max_nodes is None else max_nodes,
                        stack_nodes=DEFAULT_STACK_NODES if stack_nodes is None else stack_nodes)
    status = int(res.status[0])
    if status & A.HK_SEARCH_ROOT_ENDED:
        raise ValueError("the root has fewer than 2 points: the game has already ended")
    hit = [name for bit, name in _LIMITS if status & bit]
    if hit:
        raise RuntimeError(f"search_depth did not finish exactly (status {status}): limited by {', '.join(hit)}; "
                           f"depth >= {int(res.depth[0])}, nodes >= {int(res.nodes[0])}")
    return int(res.depth[0])
