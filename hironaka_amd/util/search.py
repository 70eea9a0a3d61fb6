"""``search_depth`` (hironaka/util/search.py:9-32): against a deterministic host, how long can an adversarial agent
make the game last?  Every agent choice is enumerated depth first, on the GPU (hk_search_depth): one tree per root,
any number of roots per call.

``search_tree`` (hironaka/util/search.py:35-50): the same game tree with every node kept, in the reference's node
order, built on the GPU (hk_search_game_tree) and handed to any tree object with ``size()`` and ``create_node``
(treelib's ``Tree`` among them).  ``search_trees`` returns the trees of a batch of roots as tensors.

``search_tree_morin`` (hironaka/util/search.py:53-93): the Morin game tree, where every node also carries integer
weights and a distinguished point; actions are pruned by weight and a child that loses the point is a
"No contribution" leaf.  Built on the GPU (hk_search_morin_tree, dim 2..7) and handed over like ``search_tree``,
with the reference's "...more..." nodes added where it stops at ``max_size``.  ``search_trees_morin`` returns the
trees of a batch of roots as tensors.

The JAX ``search_tree_fix_host`` (any callable host, level by level) lives in ``hironaka_amd.host_tree``.
"""
from collections import namedtuple
from typing import NamedTuple, Optional

import numpy as np

import torch

from .. import _abi as A
from .. import ops
from ..host import AllCoordHost, WeakSpivakovsky, WeakSpivakovskyMinHitting, Zeillinger, ZeillingerLex

DEFAULT_MAX_DEPTH = 1 << 20
DEFAULT_MAX_NODES = 1 << 24
DEFAULT_STACK_NODES = 1 << 16  # per root, for one root (the 5552-deep reference tree peaks at a few hundred)
DEFAULT_BATCH_STACK_NODES = 1 << 12  # per root of a batch; ops.search_depth splits a batch to bound the workspace
DEFAULT_TREE_NODES = 1 << 21  # search_tree: one root; the 5552-deep reference tree has 1 128 897 nodes
DEFAULT_BATCH_TREE_NODES = 1 << 14  # search_trees: per root of a batch
DEFAULT_MORIN_NODES = 1 << 18  # search_tree_morin: one root; weight pruning keeps the Thom trees in the hundreds

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


def _one_root(points, fn: str, why: str = "") -> torch.Tensor:
    # the root of search_depth / search_tree, a batch of one; fn + "s" takes a batch
    roots = _roots(points, None)
    if roots.shape[0] != 1:
        raise ValueError(f"{fn} searches one root{why}; got a batch of {roots.shape[0]}: use {fn}s")
    return roots


def _limit_message(fn: str, status: int, ignore: int = 0) -> Optional[str]:
    # the limits a status names, None when there are none
    hit = [name for bit, name in _LIMITS if status & bit & ~ignore]
    return f"{fn} did not finish exactly (status {status}): limited by {', '.join(hit)}" if hit else None


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
    roots = _one_root(points, "search_depth", " (the reference asserts batch_size == 1)")
    res = search_depths(roots, host, max_depth=DEFAULT_MAX_DEPTH if max_depth is None else max_depth,
                        max_nodes=DEFAULT_MAX_NODES if max_nodes is None else max_nodes,
                        stack_nodes=DEFAULT_STACK_NODES if stack_nodes is None else stack_nodes)
    status = int(res.status[0])
    if status & A.HK_SEARCH_ROOT_ENDED:
        raise ValueError("the root has fewer than 2 points: the game has already ended")
    msg = _limit_message("search_depth", status)
    if msg:
        raise RuntimeError(f"{msg}; depth >= {int(res.depth[0])}, nodes >= {int(res.nodes[0])}")
    return int(res.depth[0])


class SearchTreeResult(NamedTuple):
    parent: torch.Tensor       # int32 [B, max_nodes]: the parent's id, -1 for the root; ids are preorder
    child_index: torch.Tensor  # int32 [B, max_nodes]: the position in the parent's host list, -1 for the root
    axis: torch.Tensor         # int32 [B, max_nodes]: the agent's axis that made the node, -1 for the root
    depth: torch.Tensor        # int32 [B, max_nodes]: the root has depth 0
    num_points: torch.Tensor   # int32 [B, max_nodes]
    host_class: torch.Tensor   # int32 [B, max_nodes]: an expanded node's host subset (class id), else -1
    states: Optional[torch.Tensor]  # [B, max_nodes, m, d]: list semantics, padding -1; None unless states=True
    count: torch.Tensor        # int32 [B]: the nodes; slots from count on hold -1
    status: torch.Tensor       # int32 [B]: 0, or an OR of A.HK_SEARCH_* bits


def search_trees(points, host, *, max_size: Optional[int] = None, max_depth: int = DEFAULT_MAX_DEPTH,
                 max_nodes: int = DEFAULT_BATCH_TREE_NODES, stack_nodes: int = DEFAULT_BATCH_STACK_NODES,
                 states: bool = True, dtype: Optional[torch.dtype] = None) -> SearchTreeResult:
    """The reference's ``search_tree`` for a batch of roots [B, m, d] (tensor, HipPoints or nested lists), as padded
    tensors.  ``max_size`` counts as in the reference with the root alone in the tree (tree.size() == 1): nodes
    numbered <= max_size - 1 are expanded; None expands the whole tree.  A root with ``max_size`` < 1 is refused
    here (the reference adds nothing).  Nothing is raised for a non-zero status: read ``status``."""
    if max_size is not None and max_size < 1:
        raise ValueError(f"max_size must be None or >= 1 (the root is in the tree). Got {max_size}.")
    res = ops.search_game_tree(_roots(points, dtype), _host_name(host),
                               expand_limit=None if max_size is None else max_size - 1, max_depth=max_depth,
                               max_nodes=max_nodes, stack_nodes=stack_nodes, states=states)
    return SearchTreeResult(*res)


class TreeNodeData:
    """The ``data`` of a node made by ``search_tree``: a light stand-in for the reference's ListPoints of one game.
    ``points`` is the nested list [[[x, ...], ...]] of a batch of one, ``str()`` prints it as ListPoints does."""
    __slots__ = ("points",)
    batch_size = 1

    def __init__(self, points):
        self.points = points

    @property
    def ended(self) -> bool:
        return len(self.points[0]) <= 1

    def __repr__(self) -> str:
        return str(self.points)


def _node_points(state) -> list:
    # the rows with coordinate 0 >= 0, as Python ints (the states are exact integers)
    return [[[int(x) for x in row] for row in state if row[0] >= 0]]


def search_tree(points, tree, curr_node, host, max_size=100, *, max_depth: Optional[int] = None,
                max_nodes: Optional[int] = None, stack_nodes: Optional[int] = None):
    """The reference's ``search_tree(points, tree, curr_node, host, max_size=100)``: builds the game tree under
    ``host`` below ``curr_node``, which the caller has already created in ``tree``, and adds its nodes with
    ``tree.create_node(node_id, node_id, parent=..., data=...)`` in the reference's order, node_id = tree.size().
    ``tree`` is any object with ``size()`` and ``create_node`` (a treelib Tree works).  Returns ``tree``, or None
    when the root has fewer than 2 points or ``tree.size() > max_size`` (nothing is added then).  ``max_size``
    None builds the whole tree.  ``points``: a HipPoints of batch 1, a [m, d] or [1, m, d] tensor, or nested lists.
    The tree is built on the GPU first and handed over afterwards; RuntimeError names the limit when it did not
    fit (``max_nodes``, ``stack_nodes``) or left the exact integer range.  A node's ``data`` is a TreeNodeData."""
    name = _host_name(host)
    roots = _one_root(points, "search_tree")
    s0 = tree.size()
    if max_size is not None and s0 > max_size:
        return None
    res = ops.search_game_tree(roots, name, expand_limit=None if max_size is None else max_size - s0,
                               max_depth=DEFAULT_MAX_DEPTH if max_depth is None else max_depth,
                               max_nodes=DEFAULT_TREE_NODES if max_nodes is None else max_nodes,
                               stack_nodes=DEFAULT_STACK_NODES if stack_nodes is None else stack_nodes)
    parent, _, _, _, _, _, st, count, status = res
    status, count = int(status[0]), int(count[0])
    if status & A.HK_SEARCH_ROOT_ENDED:
        return None
    msg = _limit_message("search_tree", status, ignore=A.HK_SEARCH_DEPTH_LIMIT)
    if msg:
        raise RuntimeError(msg)
    par = parent[0, :count].tolist()
    states = st[0, :count].cpu().numpy()
    ident = [curr_node] + [s0 + j - 1 for j in range(1, count)]
    for j in range(1, count):
        tree.create_node(ident[j], ident[j], parent=ident[par[j]], data=TreeNodeData(_node_points(states[j])))
    return tree


class MorinTreeResult(NamedTuple):
    parent: torch.Tensor         # int32 [B, max_nodes]: as SearchTreeResult
    child_index: torch.Tensor    # int32 [B, max_nodes]: the position in the parent's host list; pruned actions are gaps
    axis: torch.Tensor           # int32 [B, max_nodes]
    depth: torch.Tensor          # int32 [B, max_nodes]
    num_points: torch.Tensor     # int32 [B, max_nodes]
    host_class: torch.Tensor     # int32 [B, max_nodes]: an expanded node's host subset (class id), else -1
    kind: torch.Tensor           # int32 [B, max_nodes]: 0 a contributing node, 1 "No contribution"
    distinguished: torch.Tensor  # int32 [B, max_nodes]: the distinguished point's row in states, -1 for kind 1
    weights: torch.Tensor        # int32 [B, max_nodes, d]
    states: Optional[torch.Tensor]  # [B, max_nodes, m, d]: list semantics, padding -1; None unless states=True
    count: torch.Tensor          # int32 [B]: the nodes; slots from count on hold -1
    status: torch.Tensor         # int32 [B]: 0, or an OR of A.HK_SEARCH_* bits


MorinNode = namedtuple("Node", ["points"])  # a node's data, as the reference's namedtuple Node(points=str)
NO_CONTRIBUTION = "No contribution"
MORE = "...more..."


def _int_vector(values, name: str) -> list:
    # a list of Python ints; integral floats are accepted, anything else is a ValueError
    if isinstance(values, torch.Tensor):
        values = values.tolist()
    arr = np.asarray(values)
    if arr.ndim != 1 or arr.dtype.kind not in "iuf" or (arr.dtype.kind == "f" and not np.all(arr == np.floor(arr))):
        raise ValueError(f"{name} must be a list or array of integers. Got {values!r}.")
    return [int(v) for v in arr.tolist()]


def search_trees_morin(points, weights, distinguished, host, *, max_size: Optional[int] = None,
                       max_depth: int = DEFAULT_MAX_DEPTH, max_nodes: int = DEFAULT_BATCH_TREE_NODES,
                       stack_nodes: int = DEFAULT_BATCH_STACK_NODES, states: bool = True,
                       dtype: Optional[torch.dtype] = None) -> MorinTreeResult:
    """The reference's ``search_tree_morin`` for a batch of roots [B, m, d] with weights [B, d] and distinguished row
    indices [B] (tensors or nested lists), as padded tensors.  ``max_size`` counts as in ``search_trees``.  The
    result holds the kernel's nodes only, no "...more..." nodes.  Nothing is raised for a non-zero status: read
    ``status`` (A.HK_SEARCH_ROOT_INVALID: the index addresses no point, or a weight is negative)."""
    name = _host_name(host)
    if max_size is not None and max_size < 1:
        raise ValueError(f"max_size must be None or >= 1 (the root is in the tree). Got {max_size}.")
    roots = _roots(points, dtype)
    wts = torch.as_tensor(weights).to(roots.device)
    dist = torch.as_tensor(distinguished).to(roots.device)
    if wts.dim() == 1:
        wts = wts.unsqueeze(0)
    if dist.dim() == 0:
        dist = dist.unsqueeze(0)
    res = ops.search_morin_tree(roots, wts, dist, name, expand_limit=None if max_size is None else max_size - 1,
                                max_depth=max_depth, max_nodes=max_nodes, stack_nodes=stack_nodes, states=states)
    return MorinTreeResult(*res)


def search_tree_morin(points, tree, curr_node, curr_weights, host, max_size=100, *, distinguished: Optional[int] = None,
                      max_depth: Optional[int] = None, max_nodes: Optional[int] = None,
                      stack_nodes: Optional[int] = None):
    """The reference's ``search_tree_morin(points, tree, curr_node, curr_weights, host, max_size=100)``: builds the
    Morin game tree under ``host`` below ``curr_node``, which the caller has already created in ``tree``, and adds
    its nodes with ``tree.create_node(node_id, node_id, parent=..., data=Node(points=str))`` in the reference's
    order, node_id = tree.size().  A node's data string is ``str([state]) + ", [dist]"``, "No contribution" where the
    distinguished point was lost, or "...more..." below every contributing node that the reference reaches with
    ``tree.size() > max_size``.  Always returns ``tree``.  ``max_size`` None builds the whole tree.
    ``points``: a HipPoints of batch 1 whose ``distinguished_points[0]`` names the point, or a [m, d] / [1, m, d]
    tensor or nested lists with ``distinguished=``.  ``curr_weights``: a list or numpy array of non-negative integers.
    ValueError when no index is given or it addresses no point; RuntimeError names the limit when the tree did not
    fit (``max_nodes``, ``stack_nodes``) or left the exact integer range.  ``max_nodes`` bounds the nodes the traversal
    records, which with a ``max_size`` exceed the nodes kept: up to one node per lane and iteration is expanded before
    the ones beyond ``max_size`` are dropped (23 018 records for the 151 nodes of the Thom N = 4 root under
    AllCoordHost at max_size=100)."""
    name = _host_name(host)
    weights = _int_vector(curr_weights, "curr_weights")
    if distinguished is None:
        given = getattr(points, "distinguished_points", None)
        distinguished = given[0] if given else None
    if distinguished is None or isinstance(distinguished, bool) or int(distinguished) != distinguished:
        raise ValueError("search_tree_morin needs the distinguished point's row index: a HipPoints with "
                         f"distinguished_points, or distinguished=. Got {distinguished!r}.")
    distinguished = int(distinguished)
    roots = _one_root(points, "search_tree_morin")
    if len(weights) != roots.shape[2]:
        raise ValueError(f"curr_weights must have one weight per coordinate ({roots.shape[2]}). Got {len(weights)}.")
    if min(weights) < 0:
        raise ValueError(f"curr_weights must not be negative. Got {weights}.")
    s0 = tree.size()
    if max_size is not None and s0 > max_size:
        tree.create_node(s0, s0, parent=curr_node, data=MorinNode(MORE))
        return tree
    if not 0 <= distinguished < roots.shape[1]:
        raise ValueError(f"distinguished must address a point of the root. Got {distinguished}.")
    dev = roots.device
    res = ops.search_morin_tree(roots, torch.tensor([weights], dtype=torch.int64, device=dev),
                                torch.tensor([distinguished], dtype=torch.int64, device=dev), name,
                                expand_limit=None if max_size is None else max_size - s0,
                                max_depth=DEFAULT_MAX_DEPTH if max_depth is None else max_depth,
                                max_nodes=DEFAULT_MORIN_NODES if max_nodes is None else max_nodes,
                                stack_nodes=DEFAULT_STACK_NODES if stack_nodes is None else stack_nodes)
    res = MorinTreeResult(*res)
    status, count = int(res.status[0]), int(res.count[0])
    if status & A.HK_SEARCH_ROOT_INVALID:
        raise ValueError(f"distinguished must address a point of the root. Got {distinguished}.")
    if status & A.HK_SEARCH_ROOT_ENDED:
        return tree
    msg = _limit_message("search_tree_morin", status, ignore=A.HK_SEARCH_DEPTH_LIMIT)
    if msg:
        raise RuntimeError(msg)
    par = res.parent[0, :count].tolist()
    kind = res.kind[0, :count].tolist()
    dist = res.distinguished[0, :count].tolist()
    states = res.states[0, :count].cpu().numpy()
    limit = None if max_size is None else max_size - s0  # kernel ids above it are reached with tree.size() > max_size
    ident = [curr_node] + [None] * (count - 1)
    for j in range(1, count):
        ident[j] = tree.size()
        if kind[j]:
            tree.create_node(ident[j], ident[j], parent=ident[par[j]], data=MorinNode(NO_CONTRIBUTION))
            continue
        tree.create_node(ident[j], ident[j], parent=ident[par[j]],
                         data=MorinNode(str(_node_points(states[j])) + f", {[dist[j]]}"))
        if limit is not None and j > limit:
            more = tree.size()
            tree.create_node(more, more, parent=ident[j], data=MorinNode(MORE))
    return tree
