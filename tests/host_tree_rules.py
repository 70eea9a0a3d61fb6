"""hironaka/jax/search.py:73-113 search_tree_fix_host restated as a plain recursion in numpy: what hk_tree_expand,
hironaka_amd.ops.tree_expand and hironaka_amd.host_tree define their outputs by.  The step is oracle.np_oracle.step
under JAX semantics and the list-semantics child of tests/search_rules.py under list semantics; the host is a Python
function of one state that returns a class id (or -1 / None for "no children").  Nothing here comes from hironaka_amd,
and nothing here knows of levels, offsets or slots: test_host_tree_rules.py pins this module to the reference's recorded
trees, and the GPU tests compare the kernel and the level loop with it.

A state is a padded [m, d] array: rows with coordinate 0 >= 0 are the points."""
import sys
from collections import namedtuple

import numpy as np

import search_rules as R
from oracle import np_oracle as NO


def subset(cls, d):
    """the coordinates of a host class in ascending order; [] for an id outside the dimension's classes"""
    table = NO.decode_table(d)
    if cls is None or not 0 <= cls < len(table):
        return []
    return [k for k in range(d) if table[cls][k]]


def num_points(state):
    return int((np.asarray(state)[:, 0] >= 0).sum())


def is_done(state, sem, d):
    """get_done_from_flatten on the state's m*d entries under "jax" (at most d of them >= 0); fewer than 2 points
    under "list" """
    return bool((np.asarray(state) >= 0).sum() <= d) if sem == "jax" else num_points(state) < 2


def child(state, coords, a, sem, reposition):
    """the step of `state` with the subset `coords` and the agent's axis a, as a padded array of the state's shape"""
    state = np.asarray(state)
    m, d = state.shape
    if sem == "jax":
        mask = np.zeros((1, d), state.dtype)
        mask[0, list(coords)] = 1
        return NO.step(state[None], mask, np.asarray([a]), sem="jax", do_reposition=reposition)[0].astype(state.dtype)
    pts = R.live(state)
    new = R.shift(pts, coords, a)
    if reposition and len(new):
        new = new - new.min(0)
    kept = R.newton(new) if len(new) else new
    out = np.full((m, d), -1, state.dtype)
    out[:len(kept)] = kept
    return out


def expand(state, cls, sem, reposition):
    """[(axis, child state)] of one node under the host class cls, in ascending axis (search.py:102)"""
    coords = subset(cls, np.asarray(state).shape[1])
    return [(a, child(state, coords, a, sem, reposition)) for a in coords]


Tree = namedtuple("Tree", "parent axis depth num_points done host_class states")
# per node in the recursion's order (preorder), the root as node 0: parent id (-1 for the root), the agent's axis
# (-1), depth below the root, points, done, the host's class where the node was expanded else -1, the padded state


def tree(root, host, sem="jax", reposition=True, max_depth=1000, depth=0):
    """the nodes search_tree_fix_host(root, spec, host, depth, key, max_depth=max_depth) makes, root included"""
    root = np.asarray(root)
    d = root.shape[1]
    t = Tree([], [], [], [], [], [], [])

    def rec(state, parent, axis, dep):
        ident = len(t.parent)
        t.parent.append(parent), t.axis.append(axis), t.depth.append(dep - depth)
        t.num_points.append(num_points(state)), t.done.append(is_done(state, sem, d))
        t.host_class.append(-1), t.states.append(state)
        if t.done[ident] or dep > max_depth:  # search.py:90
            return
        cls = host(state)
        if not subset(cls, d):
            return
        t.host_class[ident] = int(cls)
        for a, new in expand(state, cls, sem, reposition):
            rec(new, ident, a, dep + 1)

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 100000))
    try:
        rec(root, -1, -1, depth)
    finally:
        sys.setrecursionlimit(old)
    return t


def list_host(name):
    """a host of search_rules.py (an ascending-list host: all_coord, weak_spivakovsky, weak_spivakovsky_min_hitting)
    as a function state -> class id, -1 where it has no list"""
    def fn(state):
        coords = R.host_list(name, state)
        return -1 if coords is None else R.class_id(coords, np.asarray(state).shape[1])
    return fn
