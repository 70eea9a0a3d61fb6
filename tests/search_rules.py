"""The fixed-host search operators restated in plain Python and numpy on exact integers: the five deterministic hosts
of hironaka/host.py as ordered lists, the list-semantics child, and the three walks of hironaka/util/search.py
(search_depth, search_tree, search_tree_morin) in the form hk_search_depth, hk_search_game_tree and
hk_search_morin_tree define their outputs.  Nothing here comes from hironaka_amd, and nothing here knows how the
kernels traverse a tree: test_search_rules.py pins this module to the fixtures made by running the reference, and the
GPU tests compare the kernels with it.

A state is an [n, d] array whose rows with coordinate 0 >= 0 are the points, in row order, holes anywhere: a root is
taken as given.  Every state made here is an int64 array of live rows only."""
import sys
from collections import namedtuple
from functools import lru_cache
from itertools import combinations

import numpy as np

HOSTS = ("all_coord", "zeillinger", "zeillinger_lex", "weak_spivakovsky", "weak_spivakovsky_min_hitting")
DEPTH_LIMIT = 1  # HK_SEARCH_DEPTH_LIMIT
NO_CONTRIBUTION = "No contribution"
MORE = "...more..."
KIND_NODE, KIND_LOST, KIND_MORE = 0, 1, 2


# ---- the hosts (row order, holes anywhere) -------------------------------------------------------------------------

def _points(state):
    return [r for r in state if r[0] >= 0]


@lru_cache(maxsize=None)
def _pairs(n):
    return np.triu_indices(n, 1)  # the order of combinations(range(n), 2)


def zeillinger_pair(state, lex):
    """Zeillinger (host.py:70-95) and ZeillingerLex (host.py:116-127) as the ordered pair [argmin v, argmax v] of the
    chosen difference v = P_i - P_j, i < j in row order; [0, 1] when the two coincide; None below 2 points"""
    state = np.asarray(state)
    pts = state[state[:, 0] >= 0]
    if len(pts) < 2:
        return None
    i, j = _pairs(len(pts))
    v = pts[i] - pts[j]
    mx, mn = v.max(1), v.min(1)
    big = mx - mn
    cnt = (v == mx[:, None]).sum(1) + (v == mn[:, None]).sum(1)
    best = np.lexsort((cnt, big))[0]  # stable: the first pair of the smallest (L, S)
    tied = [best] if not lex else np.nonzero((big == big[best]) & (cnt == cnt[best]))[0]
    r = [(int(v[k].argmin()), int(v[k].argmax())) for k in tied]
    return list(min((0, 1) if lo == hi else (lo, hi) for lo, hi in r))


def rule_zeillinger(state, lex):
    pair = zeillinger_pair(state, lex)
    return None if pair is None else set(pair)


def _supports(state):
    return {frozenset(np.nonzero(p)[0].tolist()) for p in _points(state)}


def rule_weak(state):
    pts, sup = _points(state), _supports(state)
    U = sorted(set().union(*sup)) if sup else []
    if len(pts) < 2:
        return None
    for size in range(2, len(U) + 1):
        for c in combinations(U, size):  # sorted tuples in lexicographic order
            if all(set(c) & s for s in sup):
                return set(c)
    return None


def rule_min_hitting(state, d):
    pts, sup = _points(state), _supports(state)
    if len(pts) < 2:
        return None
    for c in sorted(range(1 << d), key=lambda c: (bin(c).count("1"), c)):
        cs = {k for k in range(d) if (c >> k) & 1}
        if len(cs) >= 2 and all(cs & s for s in sup):
            return cs
    return None


def host_list(host, state):
    """the host's list for one game, in the reference's order; None where it has none (fewer than 2 points, or the
    hitting-set hosts' zero row / |U| < 2, where the reference misbehaves)"""
    state = np.asarray(state)
    d = state.shape[1]
    if host == "all_coord":
        return list(range(d)) if len(_points(state)) >= 2 else None
    if host in ("zeillinger", "zeillinger_lex"):
        return zeillinger_pair(state, host == "zeillinger_lex")
    got = rule_weak(state) if host == "weak_spivakovsky" else rule_min_hitting(state, d)
    return None if got is None else sorted(got)


def class_id(coords, d):
    """the class id of a subset: its rank among the masks with >= 2 bits in ascending order (hk_step's coords codec)"""
    mask = sum(1 << k for k in coords)
    return sum(1 for v in range(mask) if bin(v).count("1") >= 2)


# ---- one move in list semantics ------------------------------------------------------------------------------------

def live(state):
    state = np.asarray(state)
    return np.ascontiguousarray(state[state[:, 0] >= 0]).astype(np.int64)


def shift(pts, coords, a):
    out = pts.copy()
    out[:, a] = pts[:, list(coords)].sum(1)
    return out


def newton(pts):
    """duplicates and dominated rows dropped, the rest sorted descending (get_newton_polytope_approx_lst)"""
    u = pts[np.lexsort(pts.T[::-1])]  # ascending, lexicographic
    u = u[np.concatenate(([True], (u[1:] != u[:-1]).any(1)))]
    below = (u[:, None, :] <= u[None, :, :]).all(2)  # [j, i]: u_j <= u_i
    return u[below.sum(0) == 1][::-1].copy()


def child(pts, coords, a):
    return newton(shift(pts, coords, a))


def moves(host, pts):
    """(the host's list, the child of every axis of it) at a state of live rows"""
    coords = host_list(host, pts)
    return coords, [child(pts, coords, a) for a in coords or []]


def morin_child(pts, coords, a, dist):
    """shift, reposition, Newton; returns (state, row of the distinguished point or None, lost to an identical row?)"""
    new = shift(pts, coords, a)
    new -= new.min(0)
    p = new[dist]
    others = np.delete(new, dist, axis=0)
    under = (others <= p).all(1)
    kept = newton(new)
    if under.any():
        return kept, None, bool((others[under] == p).all(1).any())
    return kept, int(np.nonzero((kept == p).all(1))[0][0]), False


# ---- search_depth (util/search.py:9-32) as hk_search_depth counts it -------------------------------------------------

def depth_nodes(root, host, max_depth=None):
    """(depth, nodes, status): 1 + the largest depth of a visited node, the visited nodes (select_coord calls), and
    DEPTH_LIMIT when a node at max_depth was visited, whose children are not made.  (0, 0, None) for an ended root."""
    root = live(root)
    if len(root) < 2:
        return 0, 0, None
    stack, deepest, nodes, status = [(root, 0)], 0, 0, 0
    while stack:
        cur, dep = stack.pop()
        deepest = max(deepest, dep)
        nodes += 1
        if max_depth is not None and dep >= max_depth:
            status |= DEPTH_LIMIT
            continue
        for nxt in moves(host, cur)[1]:
            if len(nxt) >= 2:
                stack.append((nxt, dep + 1))
    return deepest + 1, nodes, status


# ---- search_tree (util/search.py:35-50) ------------------------------------------------------------------------------

Tree = namedtuple("Tree", "parent child_index axis depth num_points states hosts status")
# per node, in creation order with the root as node 0: parent (-1 for the root), position in the parent's host list,
# the agent's axis, depth, number of points, state; hosts: the host's list at every node that is expanded, else None;
# status: DEPTH_LIMIT when max_depth kept a node from being expanded that the reference would have expanded


class _recursion:
    def __enter__(self):
        self.old = sys.getrecursionlimit()
        sys.setrecursionlimit(max(self.old, 100000))

    def __exit__(self, *exc):
        sys.setrecursionlimit(self.old)


def tree(root, host, max_size=None, max_depth=None, s0=1):
    """the nodes search_tree creates below a root that is the s0-th node of the caller's tree (tree.size() == s0 at the
    call), in creation order; node j is created as identifier s0 + j - 1"""
    t = Tree([-1], [-1], [-1], [0], [], [], [None], 0)
    status = 0

    def rec(pts, node, dep):
        nonlocal status
        if len(pts) <= 1 or (max_size is not None and s0 - 1 + len(t.parent) > max_size):
            return
        if max_depth is not None and dep >= max_depth:
            status |= DEPTH_LIMIT
            return
        coords, children = moves(host, pts)
        if coords is None:
            return
        t.hosts[node] = coords
        for ci, (a, new) in enumerate(zip(coords, children)):
            ident = len(t.parent)
            t.parent.append(node), t.child_index.append(ci), t.axis.append(a), t.depth.append(dep + 1)
            t.num_points.append(len(new)), t.states.append(new), t.hosts.append(None)
            rec(new, ident, dep + 1)

    pts = live(root)
    t.num_points.append(len(pts)), t.states.append(pts)
    with _recursion():
        rec(pts, 0, 0)
    return t._replace(status=status)


# ---- search_tree_morin (util/search.py:53-93) ------------------------------------------------------------------------

MorinTree = namedtuple("MorinTree", "parent child_index axis depth num_points states hosts status kind dist weights")
# Tree's fields, then per node: kind (KIND_NODE, KIND_LOST for "No contribution", KIND_MORE for "...more..."), the row
# of the distinguished point in the state (-1 unless KIND_NODE) and the weights.  KIND_MORE nodes are the reference's
# alone: hk_search_morin_tree's outputs are this tree without them (without_more).


def morin_tree(root, weights, dist, host, max_size=None, max_depth=None, s0=1, stats=None):
    """the nodes search_tree_morin creates, as tree() lists them.  dist: the distinguished point's row in `root`.  host:
    a name of HOSTS, or select(state) -> the host's list.  stats, when given, counts [nodes lost to an identical row,
    nodes lost to a strictly smaller row, pruned actions, "...more..." nodes below an ended node]."""
    select = host if callable(host) else (lambda st: host_list(host, st))
    stats = [0, 0, 0, 0] if stats is None else stats
    t = MorinTree([-1], [-1], [-1], [0], [], [], [None], 0, [KIND_NODE], [], [])
    status = 0

    def create(node, ci, a, dep, new, kind, nd, w):
        t.parent.append(node), t.child_index.append(ci), t.axis.append(a), t.depth.append(dep)
        t.num_points.append(len(new)), t.states.append(new), t.hosts.append(None)
        t.kind.append(kind), t.dist.append(nd), t.weights.append(w)
        return len(t.parent) - 1

    def rec(pts, dist, w, node, dep):
        nonlocal status
        over = max_size is not None and s0 - 1 + len(t.parent) > max_size
        if len(pts) <= 1 or over:
            if over:
                stats[3] += len(pts) <= 1
                create(node, -1, -1, dep + 1, pts[:0], KIND_MORE, -1, w)
            return
        if max_depth is not None and dep >= max_depth:
            status |= DEPTH_LIMIT
            return
        coords = select(pts)
        if coords is None:
            return
        coords = [int(c) for c in coords]
        t.hosts[node] = coords
        for ci, a in enumerate(coords):
            if w[a] > min(w[i] for i in coords):
                stats[2] += 1
                continue
            w2 = [w[i] - w[a] if i in coords and i != a else w[i] for i in range(len(w))]
            new, nd, identical = morin_child(pts, coords, a, dist)
            if nd is None:
                stats[0] += identical
                stats[1] += not identical
                create(node, ci, a, dep + 1, new, KIND_LOST, -1, w2)
                continue
            rec(new, nd, w2, create(node, ci, a, dep + 1, new, KIND_NODE, nd, w2), dep + 1)

    state = np.asarray(root)
    pts = live(state)
    t.num_points.append(len(pts)), t.states.append(pts)
    t.dist.append(int(dist)), t.weights.append([int(v) for v in weights])
    with _recursion():
        rec(pts, int((state[:dist, 0] >= 0).sum()), t.weights[0], 0, 0)
    return t._replace(status=status)


def without_more(t):
    """the tree hk_search_morin_tree returns: the KIND_MORE nodes dropped, the others renumbered in order"""
    keep = [j for j, k in enumerate(t.kind) if k != KIND_MORE]
    new = {j: i for i, j in enumerate(keep)}
    cols = [[col[j] for j in keep] for col in t[:7]] + [t.status] + [[col[j] for j in keep] for col in t[8:]]
    out = MorinTree(*cols)
    out.parent[:] = [-1 if p < 0 else new[p] for p in out.parent]
    return out


def rows_of(state):
    return [[int(x) for x in r] for r in state]


def morin_data(t, j):
    """the data string of node j, as the reference writes it"""
    if t.kind[j] != KIND_NODE:
        return NO_CONTRIBUTION if t.kind[j] == KIND_LOST else MORE
    return str([rows_of(t.states[j])]) + f", {[t.dist[j]]}"


def created(t, s0=1, curr=0):
    """the create_node calls behind a Tree or MorinTree as (identifier, parent identifier) per node after the root"""
    ident = [curr] + [s0 + j - 1 for j in range(1, len(t.parent))]
    return [(ident[j], ident[t.parent[j]]) for j in range(1, len(t.parent))]
