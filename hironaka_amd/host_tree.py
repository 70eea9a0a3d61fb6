"""The game tree under ANY host, level by level: the counterpart of ``hironaka/jax/search.py`` (``TreeNode``,
``default_label_fn``, ``search_tree_fix_host``).

The search operators of ``hironaka_amd.util.search`` run one of five fixed hosts inside the kernel.  A host that is a
Python callable -- a network, ``players.random_host_fn``, anything a user writes -- cannot run there, but it can run
once per tree level on the whole frontier.  Between two host calls everything is environment work, done by ONE launch
of hk_tree_expand per level (``ops.tree_expand``): one child per coordinate of each node's subset, stepped, tested for
the end of the game and packed in parent order.

``search_trees_fix_host`` walks a batch of roots that way and returns the trees as flat tensors in the reference's
recursion order (preorder: a node, then the subtree of each child in ascending axis).  ``search_tree_fix_host`` has
the reference's signature and fills ``TreeNode`` objects from one such walk.  ``hironaka_amd.search`` is the MCTS
driver and has nothing to do with this module.
"""
from collections import deque
from dataclasses import dataclass
from typing import Any, Callable, List, NamedTuple, Optional, Tuple

import torch

from . import _abi as A
from . import ops

DEFAULT_MAX_NODES = 1 << 20  # over the whole batch of roots: it bounds what a walk allocates
DEPTH_LIMIT, NODE_LIMIT = A.HK_SEARCH_DEPTH_LIMIT, A.HK_SEARCH_NODE_LIMIT


class HostTreeResult(NamedTuple):
    parent: torch.Tensor      # int32 [T]: the parent's id within its root's tree, -1 for a root; ids are preorder
    axis: torch.Tensor        # int32 [T]: the agent's axis that made the node, -1 for a root
    depth: torch.Tensor       # int32 [T]: a root has depth 0
    num_points: torch.Tensor  # int32 [T]: rows with coordinate 0 >= 0
    done: torch.Tensor        # bool [T]: the game has ended at the node (it is never expanded)
    host_class: torch.Tensor  # int32 [T]: an expanded node's host subset (class id), else -1
    states: torch.Tensor      # [T, m, d]
    root: torch.Tensor        # int32 [T]: the root the node belongs to; the nodes of root b are a contiguous run
    count: torch.Tensor       # int32 [B]: the nodes of every root's tree (they sum to T)
    status: torch.Tensor      # int32 [B]: 0, or an OR of DEPTH_LIMIT (a node that is not done sits below max_depth
    #                           and was not expanded) and NODE_LIMIT (max_nodes kept a node from being made or expanded)


def level_key(key, level: int):
    """The key of a level's host call: ``key + level`` for an int key; a torch.Generator (whose state advances by
    itself) and None are passed through unchanged."""
    if key is None or isinstance(key, torch.Generator):
        return key
    return int(key) + level


def host_classes(out: torch.Tensor, n: int, d: int, device) -> torch.Tensor:
    """A host's answer for n nodes as int32 class ids [n]: one-hot rows or logits [n, 2^d - d - 1] are decoded with
    the first maximum (get_batch_decode_from_one_hot), an integer vector [n] is taken as class ids."""
    ncls = (1 << d) - d - 1
    if not isinstance(out, torch.Tensor):
        out = torch.as_tensor(out)
    out = out.to(device)
    if out.dim() == 2 and tuple(out.shape) == (n, ncls):
        return torch.argmax(out if out.dtype != torch.bool else out.to(torch.uint8), dim=1).to(torch.int32)
    if out.dim() == 1 and out.shape[0] == n and out.dtype in (torch.int32, torch.int64):
        return out.to(torch.int32)
    raise ValueError(f"the host must return one-hot rows or logits of shape {(n, ncls)}, or int32/int64 class ids of "
                     f"shape {(n,)}. Got {out.dtype} {tuple(out.shape)}.")


def host_from_object(host) -> Callable:
    """A ``hironaka_amd.host.Host`` as a callable for ``host_input="points"``: ``select_coord``'s mask encoded as class
    ids, -1 where the subset has fewer than two coordinates."""
    def fn(points: torch.Tensor, key=None) -> torch.Tensor:
        mask = host.select_coord(points).to(torch.int64)
        d = mask.shape[1]
        value = (mask << torch.arange(d, device=mask.device)).sum(1)
        top = torch.zeros_like(value)
        for j in range(1, d):
            top = torch.where(value >> j != 0, torch.full_like(value, j), top)
        return torch.where(mask.sum(1) >= 2, value - top - 2, torch.full_like(value, -1)).to(torch.int32)
    return fn


def _root_records(roots, m: int, d: int, dtype: Optional[torch.dtype]) -> torch.Tensor:
    # [B, m*d + d] records on the device; states without a tail get a zero tail
    t = roots if isinstance(roots, torch.Tensor) else torch.as_tensor(roots, dtype=torch.float32)
    if dtype is not None:
        t = t.to(dtype)
    elif t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float32)
    if not t.is_cuda:
        t = t.to("cuda")
    n = m * d
    if t.dim() == 3 and tuple(t.shape[1:]) == (m, d):
        t = t.reshape(-1, n)
    if t.dim() == 2 and t.shape[1] == n:
        return torch.cat([t, t.new_zeros((t.shape[0], d))], dim=1)
    if t.dim() == 2 and t.shape[1] == n + d:
        return t.contiguous()
    raise ValueError(f"roots must be observations [B, {n + d}] or states [B, {m}, {d}]. Got shape {tuple(t.shape)}.")


def _flag(status: torch.Tensor, roots: torch.Tensor, bit: int) -> None:
    hit = torch.zeros_like(status, dtype=torch.bool)
    hit[roots.long()] = True
    status |= hit.to(torch.int32) * bit


def search_trees_fix_host(roots, spec: Tuple[int, int], host: Callable, *, key=0, max_depth: int = 1000,
                          max_nodes: int = DEFAULT_MAX_NODES, sem: str = "jax", reposition: bool = True,
                          host_input: str = "obs", dtype: Optional[torch.dtype] = None) -> HostTreeResult:
    """The trees ``search_tree_fix_host`` builds below a batch of roots, as flat tensors in preorder.

    roots: observations [B, m*d + d] (the reference's node data) or states [B, m, d], spec = (m, d).
    host: called once per level on the whole frontier, ended nodes included (their answer is ignored), as
        ``host(frontier, key=level_key(key, level))``; the frontier is [N, m*d + d] with ``host_input="obs"`` and
        [N, m, d] with ``host_input="points"`` (``host_from_object`` adapts a ``hironaka_amd.host.Host`` to that form).
        It returns one-hot rows or logits [N, 2^d - d - 1], decoded with the first maximum, or int class ids [N]; an
        id < 0 gives the node no children.
    key: an int (level L gets ``key + L``), a torch.Generator (passed through) or None.
    A node is expanded when it is not done and its depth is <= max_depth, so leaves exist at depth max_depth + 1
    (search.py:90).  sem / reposition: the step, as in ``ops.tree_expand`` (the reference: "jax", True).  A node is
    done, under "jax", when at most d entries of its state are >= 0 (get_done_from_flatten) and, under "list", when it
    has fewer than 2 points.
    max_nodes bounds the nodes of all the trees together, and with them what the walk allocates: children without
    room are dropped, nothing is expanded any more, and NODE_LIMIT is set for the roots concerned.
    Every level costs one launch of hk_tree_expand and one 4-byte readback, the size of the next level."""
    m, d = (int(v) for v in spec)
    n = m * d
    if host_input not in ("obs", "points"):
        raise ValueError(f"host_input must be 'obs' or 'points'. Got {host_input!r}.")
    if sem not in ("jax", "list"):
        raise ValueError(f"sem must be 'jax' or 'list'. Got {sem!r}.")
    rec = _root_records(roots, m, d, dtype)
    b, dev = rec.shape[0], rec.device
    if max_nodes < b:
        raise ValueError(f"max_nodes must hold the {b} roots at least. Got {max_nodes}.")
    status = torch.zeros(b, dtype=torch.int32, device=dev)
    state = rec[:, :n]
    num_points = (state.reshape(b, m, d)[:, :, 0] >= 0).sum(1).to(torch.int32)
    done = num_points < 2 if sem == "list" else (state >= 0).sum(1) <= d
    minus = torch.full((b,), -1, dtype=torch.int32, device=dev)
    # per level: records, parent (index into the level above), axis, num_points, done, root, host class
    levels = [[rec, minus, minus, num_points, done, torch.arange(b, dtype=torch.int32, device=dev), None]]
    nodes, level = b, 0
    while b:
        cur = levels[-1]
        rec, done, root = cur[0], cur[4], cur[5]
        size = rec.shape[0]
        if level > max_depth or nodes >= max_nodes:
            cur[6] = torch.full((size,), -1, dtype=torch.int32, device=dev)
            _flag(status, root[~done], DEPTH_LIMIT if level > max_depth else NODE_LIMIT)
            break
        frontier = rec if host_input == "obs" else rec.as_strided((size, m, d), (n + d, d, 1))
        cls = host_classes(host(frontier, key=level_key(key, level)), size, d, dev)
        cls = torch.where(done, torch.full_like(cls, -1), cls)
        cur[6] = cls
        capacity = min(size * d, max_nodes - nodes)
        res = ops.tree_expand(rec, cls, spec=(m, d), sem=sem, reposition=reposition, capacity=capacity, zero_tail=True)
        total = int(res.total)  # the readback: the loop's exit test, and the bound of the next allocation
        if total == 0:
            break
        if total > capacity:  # the parents that lost a child
            sizes = ops._class_sizes(d, dev)
            ok = (cls >= 0) & (cls < sizes.numel())
            ends = torch.cumsum(torch.where(ok, sizes[cls.long().clamp(0, sizes.numel() - 1)], 0), 0)
            _flag(status, root[ends > capacity], NODE_LIMIT)
        kept = min(total, capacity)
        parent = res.child_parent[:kept]
        levels.append([res.children[:kept], parent, res.child_axis[:kept], res.child_num_points[:kept],
                       res.child_done[:kept], root[parent.long()], None])
        nodes += kept
        level += 1
    if not b:
        empty = torch.zeros(0, dtype=torch.int32, device=dev)
        return HostTreeResult(empty, empty, empty, empty, empty.bool(), empty, rec[:, :n].reshape(0, m, d), empty,
                              empty, status)
    # preorder ids from the level arrays: subtree sizes bottom-up, then top-down a node's id is its parent's, plus
    # one, plus the subtrees of its earlier siblings (the children of a parent are adjacent, in ascending axis)
    sub = [torch.ones(lv[0].shape[0], dtype=torch.int64, device=dev) for lv in levels]
    for k in range(len(levels) - 1, 0, -1):
        sub[k - 1].index_add_(0, levels[k][1].long(), sub[k])
    pre = [torch.cumsum(sub[0], 0) - sub[0]]
    for k in range(1, len(levels)):
        par = levels[k][1].long()
        before = torch.cumsum(sub[k], 0) - sub[k]
        first = torch.ones_like(par, dtype=torch.bool)
        first[1:] = par[1:] != par[:-1]
        start = torch.cummax(torch.where(first, before, torch.zeros_like(before)), 0).values
        pre.append(pre[k - 1][par] + 1 + before - start)
    where = torch.cat(pre)
    base = pre[0]  # the id of every root's first node

    def gather(column, dtype):
        flat = torch.cat([lv[column] for lv in levels]).to(dtype)
        return torch.empty_like(flat).index_copy_(0, where, flat)

    root_of = gather(5, torch.int32)
    local = [minus] + [(pre[k - 1][levels[k][1].long()] - base[levels[k][5].long()]).to(torch.int32)
                       for k in range(1, len(levels))]
    parent = torch.empty(nodes, dtype=torch.int32, device=dev).index_copy_(0, where, torch.cat(local))
    depth = torch.cat([torch.full((lv[0].shape[0],), k, dtype=torch.int32, device=dev)
                       for k, lv in enumerate(levels)])
    depth = torch.empty_like(depth).index_copy_(0, where, depth)
    states = torch.cat([lv[0][:, :n] for lv in levels])
    states = torch.empty_like(states).index_copy_(0, where, states).reshape(nodes, m, d)
    return HostTreeResult(parent, gather(2, torch.int32), depth, gather(3, torch.int32), gather(4, torch.bool),
                          gather(6, torch.int32), states, root_of, sub[0].to(torch.int32), status)


# ---- the reference's names (hironaka/jax/search.py:24-113) ----------------------------------------------------------

@dataclass(eq=False, repr=False)
class TreeNode:
    children: Optional[List["TreeNode"]] = None
    parent: Optional["TreeNode"] = None
    action_from_parent: Optional[int] = None
    data: Any = None

    def _walk(self, max_depth: Optional[int]):
        """the reference's breadth-first walk: (id, node, parent id) of every node it adds, ids in that order"""
        yield 0, self, None
        num_nodes = 1
        queue = deque([(self, 0, 0)])
        while queue:
            node, depth, ident = queue.popleft()
            if node.children is None or (max_depth is not None and depth >= max_depth):
                continue
            for child in node.children:
                queue.append((child, depth + 1, num_nodes))
                yield num_nodes, child, ident
                num_nodes += 1

    def to_dot(self, max_depth: Optional[int] = None, label_fn: Optional[Callable] = None) -> str:
        """The subtree below this node as DOT text, by the walk of ``to_graphviz``: node ids in breadth-first order,
        a node's label ``label_fn(node)`` (default its id), an edge's label the child's ``action_from_parent``."""
        def quote(text) -> str:
            return '"' + str(text).replace("\\", "\\\\").replace('"', '\\"').replace("\n", "\\n") + '"'
        lines = ["strict graph {"]
        for ident, node, parent_id in self._walk(max_depth):
            lines.append(f"  {ident} [label={quote(label_fn(node) if label_fn is not None else ident)}];")
            if parent_id is not None:
                lines.append(f"  {parent_id} -- {ident} [label={quote(node.action_from_parent)}];")
        return "\n".join(lines + ["}"]) + "\n"

    def to_graphviz(self, max_depth: Optional[int] = None, label_fn: Optional[Callable] = None):
        """The subtree below this node as a pygraphviz AGraph (breadth-first, so that the depth can be bounded)."""
        try:
            import pygraphviz as pgv
        except ImportError as err:
            raise ImportError("TreeNode.to_graphviz needs pygraphviz, which is not installed; TreeNode.to_dot "
                              "returns the same graph as DOT text without it.") from err
        graph = pgv.AGraph()
        for ident, node, parent_id in self._walk(max_depth):
            self.add_node(graph, id=ident, node=node, parent_id=parent_id, label_fn=label_fn,
                          edge_label=None if parent_id is None else str(node.action_from_parent))
        return graph

    @staticmethod
    def add_node(graph, id, node, parent_id=None, label_fn=None, edge_label=None):
        label = label_fn(node) if label_fn is not None else str(id)
        graph.add_node(id, label=label)
        if parent_id is not None:
            graph.add_edge(parent_id, id, label=edge_label)


def default_label_fn(node: TreeNode, spec: Tuple[int, int]) -> str:
    """the node's points, rows with coordinate 0 >= 0 (search.py:67-70)"""
    points = node.data[:, :-spec[1]].reshape(spec)
    points = points[points[:, 0] >= 0]
    return str(points.cpu().numpy() if isinstance(points, torch.Tensor) else points)


def search_tree_fix_host(node: TreeNode, spec: Tuple[int, int], host: Callable, depth: int, key,
                         scale_observation=True, max_depth=1000) -> TreeNode:
    """The reference's ``search_tree_fix_host(node, spec, host, depth, key, scale_observation=True, max_depth=1000)``.
    ``node.data`` is a [1, (m+1)*d] tensor; ``host(obs, key=...)`` returns policy logits or one-hot rows over the
    host classes for a batch of such observations (it is called once per tree level, not once per node).  Children
    are appended to ``node.children`` as TreeNodes whose ``data`` are [1, (m+1)*d] device tensors with a zero tail.
    A node is expanded when it is not done and ``depth`` plus its level below ``node`` is <= max_depth.
    ``scale_observation`` is accepted and unused, as in the reference.  ``key``: an int or a torch.Generator.  The
    tree is built on the GPU by one ``search_trees_fix_host`` walk and handed over with one device-to-host copy;
    RuntimeError when it exceeds DEFAULT_MAX_NODES nodes."""
    if node.children is None:
        node.children = []
    m, d = (int(v) for v in spec)
    data = node.data if isinstance(node.data, torch.Tensor) else torch.as_tensor(node.data, dtype=torch.float32)
    if tuple(data.shape) != (1, (m + 1) * d):
        raise ValueError(f"node.data must have shape {(1, (m + 1) * d)}. Got {tuple(data.shape)}.")
    res = search_trees_fix_host(data, (m, d), host, key=key, max_depth=max_depth - depth)
    links = torch.stack([res.parent, res.axis, res.status.expand_as(res.parent)]).cpu()  # the one copy
    parent, axis = links[0].tolist(), links[1].tolist()
    if int(links[2, 0]) & NODE_LIMIT:
        raise RuntimeError(f"search_tree_fix_host: the tree has more than {DEFAULT_MAX_NODES} nodes; bound it with "
                           "max_depth, or walk it with search_trees_fix_host(max_nodes=...)")
    total = len(parent)
    obs = torch.cat([res.states.reshape(total, m * d), res.states.new_zeros((total, d))], dim=1)
    made = [node] + [None] * (total - 1)
    for j in range(1, total):  # preorder: a parent comes before its children, siblings in ascending axis
        made[j] = TreeNode(children=[], parent=made[parent[j]], action_from_parent=axis[j], data=obs[j:j + 1])
        made[parent[j]].children.append(made[j])
    return node
