"""hk_search_depth, hk_search_game_tree and hk_search_morin_tree at the largest roots they accept, where a wave has
fewer lanes than pending nodes: (64,2), (64,3), (33,4), (48,5), (64,6), and for the Morin operator (33,4), (64,6),
(24,7), (64,7); all five hosts, float32 and float64.  Expected values: tests/search_rules.py, the plain restatement
that test_search_rules.py pins to the reference, computed here on the CPU; and tests/golden/search_sizes.npz, the
reference's own runs at these shapes, for the tree wrappers.  Every comparison is exact."""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import search_rules as R
from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import _lib
from hironaka_amd import ops
from hironaka_amd.host import AllCoordHost, WeakSpivakovsky, WeakSpivakovskyMinHitting, Zeillinger, ZeillingerLex
from hironaka_amd.util import search_depths, search_tree, search_tree_morin, search_trees, search_trees_morin

pytestmark = pytest.mark.gpu

HOSTS = {"all_coord": AllCoordHost, "zeillinger": Zeillinger, "zeillinger_lex": ZeillingerLex,
         "weak_spivakovsky": WeakSpivakovsky, "weak_spivakovsky_min_hitting": WeakSpivakovskyMinHitting}
DTYPES = {"f32": torch.float32, "f64": torch.float64}
# (operator, shape) -> the max_depth cap under the all-coordinates host, whose trees do not end.  Chosen from the
# restatement so that its tree holds more than 2 * lanes nodes to expand in float32, the dtype with more lanes
# (test_narrow_regime_and_tree_parity asserts it).  At dim 2 every host's list is both axes and the staircase's tree is
# at most 36 nodes wide, so depth gets it there, for every host.  The other hosts run under FINITE_CAP.
ALL_COORD_CAP = {("tree", (64, 2)): 16, ("tree", (64, 3)): 8, ("tree", (33, 4)): 5, ("tree", (48, 5)): 4,
                 ("tree", (64, 6)): 4, ("morin", (33, 4)): 8, ("morin", (64, 6)): 4, ("morin", (24, 7)): 4,
                 ("morin", (64, 7)): 4}
FINITE_CAP = 7
CASES = [(op, shape, dt) for (op, shape) in ALL_COORD_CAP for dt in DTYPES]
IDS = [f"{op}-{m}x{d}-{dt}" for op, (m, d), dt in CASES]
TREE_FIELDS = ("parent", "child_index", "axis", "depth", "num_points", "host_class", "states")
MORIN_FIELDS = TREE_FIELDS + ("kind", "distinguished", "weights")
SPARE = 3  # output slots behind the expected tree, which must stay -1


def lanes(op, m, d, dtype):
    """launch_search's lanes per wave: the LDS slices that fit into 64 KiB"""
    extra = 2 * d if op == "morin" else 0
    return min(64, 65536 // (((2 * m * d + 2 * d + extra) | 1) * (4 if dtype == torch.float32 else 8)))


def cap_of(op, shape, host):
    return ALL_COORD_CAP[op, shape] if host == "all_coord" or shape[1] == 2 else FINITE_CAP


def sizes_of(op, shape):
    """three finite max_size values: below the lanes of either dtype, between the two, above both"""
    return 5, lanes(op, *shape, torch.float64) + 3, lanes(op, *shape, torch.float32) + 5


@lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "search_sizes.npz"))


@lru_cache(maxsize=None)
def root_of(op, shape, which):
    """(root [m, d], weights, distinguished row) of which = "full", "sparse", "tail", "one_first", "one_last"; the
    last two have a single point and are ended"""
    m, d = shape
    g = golden()
    full = g[f"root_{m}x{d}"]
    if which.startswith("one"):
        root = np.full((m, d), -1, np.int64)
        row = 0 if which == "one_first" else m - 1
        root[row] = full[row]
        return root, [1] * d, row
    kind = "" if which == "full" else "_" + which
    if op == "tree":
        return g[f"root_{m}x{d}{kind}"], None, None
    return g[f"root_{m}x{d}{kind}"], g[f"morin_{m}x{d}_weights{kind}"].tolist(), int(g[f"morin_{m}x{d}_dist{kind}"])


@lru_cache(maxsize=None)
def expected(op, shape, host, which="full", max_size=None):
    """the expected outputs of one root as arrays (the fields of TREE_FIELDS / MORIN_FIELDS, count, status)"""
    m, d = shape
    root, weights, dist = root_of(op, shape, which)
    cap = cap_of(op, shape, host)
    if op == "tree":
        t = R.tree(root, host, max_size, cap)
    else:
        t = R.without_more(R.morin_tree(root, weights, dist, host, max_size, cap))
    n = len(t.parent)
    out = {f: np.asarray(getattr(t, f), np.int64) for f in ("parent", "child_index", "axis", "depth", "num_points")}
    out["host_class"] = np.asarray([-1 if c is None else R.class_id(c, d) for c in t.hosts], np.int64)
    states = np.full((n, m, d), -1, np.int64)
    states[0] = root  # the root is kept as given, padding rows included
    for j in range(1, n):
        states[j, :len(t.states[j])] = t.states[j]
    out["states"] = states
    if op == "morin":
        out["kind"] = np.asarray(t.kind, np.int64)
        out["distinguished"] = np.asarray(t.dist, np.int64)
        out["weights"] = np.asarray(t.weights, np.int64)
    ended = t.num_points[0] < 2
    out["count"] = n
    out["status"] = A.HK_SEARCH_ROOT_ENDED if ended else t.status
    out["expandable"] = sum(c is not None for c in t.hosts)
    return out


def run(op, shape, host, dtype, which, max_size=None, max_nodes=None, stack_nodes=None):
    """one call over the roots `which` (a tuple of names)"""
    m, d = shape
    roots = [root_of(op, shape, w) for w in which]
    pts = torch.as_tensor(np.stack([r[0] for r in roots]), dtype=dtype, device="cuda")
    kw = dict(max_size=max_size, max_depth=cap_of(op, shape, host), max_nodes=max_nodes, stack_nodes=stack_nodes)
    if op == "tree":
        return search_trees(pts, HOSTS[host](), **kw)
    return search_trees_morin(pts, torch.tensor([r[1] for r in roots]), torch.tensor([r[2] for r in roots]),
                              HOSTS[host](), **kw)


def budget(op, shape, host, which):
    """max_nodes and stack_nodes for a call: every record of a traversal, at any max_size, is a node of the tree at
    max_size = None under the same cap, and so is every pending node"""
    n = max(expected(op, shape, host, w)["count"] for w in which)
    return n + SPARE, n


def check_root(res, b, exp, fields, msg):
    n = exp["count"]
    assert int(res.count[b]) == n, msg
    assert int(res.status[b]) == exp["status"] and not exp["status"] & A.HK_SEARCH_INEXACT, msg
    for f in fields:
        got = getattr(res, f)[b].cpu().numpy()
        assert np.array_equal(got[:n], exp[f]), (msg, f)
        assert got.shape[0] > n and (got[n:] == -1).all(), (msg, f, "slots from count on")


@pytest.mark.parametrize("op,shape,dt", CASES, ids=IDS)
def test_narrow_regime_and_tree_parity(op, shape, dt):
    """A condition first: the expected trees are larger than a wave.  Then the tree operator against the restatement at
    max_size = None under the cap and at three finite sizes, every field of every node."""
    dtype = DTYPES[dt]
    n_lanes = lanes(op, *shape, dtype)
    full = {h: expected(op, shape, h) for h in HOSTS}
    assert n_lanes < 64
    assert max(e["expandable"] for e in full.values()) > 2 * n_lanes
    assert all(e["count"] >= 8 for e in full.values())
    assert max(int(e["states"].max()) for e in full.values()) < 2 ** 15  # far below 2^24
    small, mid, big = sizes_of(op, shape)
    assert small < n_lanes < big and (mid < n_lanes) == (dtype == torch.float32)
    fields = TREE_FIELDS if op == "tree" else MORIN_FIELDS
    for host in HOSTS:
        max_nodes, stack_nodes = budget(op, shape, host, ("full",))
        for max_size in (None, small, mid, big):
            exp = expected(op, shape, host, "full", max_size)
            res = run(op, shape, host, dtype, ("full",), max_size, max_nodes, stack_nodes)
            check_root(res, 0, exp, fields, (host, max_size))
            print(f"{op} {shape} {dt} lanes {n_lanes} {host} max_size {max_size}: {exp['count']} nodes, "
                  f"{exp['expandable']} expanded")


@pytest.mark.parametrize("op,shape,dt", [c for c in CASES if c[0] == "tree"], ids=[i for i in IDS if i[0] == "t"])
def test_depth_parity_and_agreement_with_the_tree(op, shape, dt):
    """search_depths under the cap against the restatement, full and sparse roots and an ended one in one call; and
    against search_trees.  hk_search_depth visits the nodes at depth max_depth without expanding them, so at one cap
    its nodes are the tree's nodes with >= 2 points; the tree's expanded nodes are its nodes one cap lower."""
    dtype = DTYPES[dt]
    which = ("full", "one_first", "sparse", "one_last", "tail")
    pts = torch.as_tensor(np.stack([root_of(op, shape, w)[0] for w in which]), dtype=dtype, device="cuda")
    for host in HOSTS:
        cap = cap_of(op, shape, host)
        want = [R.depth_nodes(root_of(op, shape, w)[0], host, cap) for w in which]
        stack_nodes = max(w[1] for w in want) + 1
        res = search_depths(pts, HOSTS[host](), max_depth=cap, max_nodes=1 << 20, stack_nodes=stack_nodes)
        assert res.depth.tolist() == [w[0] for w in want], host
        assert res.nodes.tolist() == [w[1] for w in want], host
        assert res.status.tolist() == [A.HK_SEARCH_ROOT_ENDED if w[2] is None else w[2] for w in want], host
        max_nodes, tree_stack = budget(op, shape, host, ("full",))
        tree = run(op, shape, host, dtype, ("full",), None, max_nodes, tree_stack)
        n = int(tree.count[0])
        dep, npts, cls = (x[0, :n].cpu().numpy() for x in (tree.depth, tree.num_points, tree.host_class))
        assert int(res.nodes[0]) == int((npts >= 2).sum()) and int(res.depth[0]) == 1 + dep[npts >= 2].max(), host
        lower = search_depths(pts[:1], HOSTS[host](), max_depth=cap - 1, max_nodes=1 << 20, stack_nodes=stack_nodes)
        assert int(lower.nodes[0]) == int((cls >= 0).sum()) and int(lower.depth[0]) == 1 + dep[cls >= 0].max(), host


@pytest.mark.parametrize("op,shape,dt", CASES, ids=IDS)
def test_several_roots_in_one_call(op, shape, dt):
    """five roots of one shape in one call: 64, 32 and 3 points (or what the shape holds), one of them between two
    ended roots.  Every root's outputs equal the restatement's and its single-root call's.  The trees differ in size
    under the hosts whose trees the cap does not fill: under the cap the hitting-set hosts' trees are complete binary
    trees at every root of dim >= 3."""
    dtype = DTYPES[dt]
    which = ("full", "one_first", "sparse", "one_last", "tail")
    fields = TREE_FIELDS if op == "tree" else MORIN_FIELDS
    sizes = {h: [expected(op, shape, h, w)["count"] for w in which] for h in HOSTS}
    assert all(v[1] == v[3] == 1 and min(v[0], v[2], v[4]) >= 8 for v in sizes.values())
    assert any(len(set(v)) >= 3 for v in sizes.values()), sizes
    for host in HOSTS:
        exp = [expected(op, shape, host, w) for w in which]
        max_nodes, stack_nodes = budget(op, shape, host, which)
        res = run(op, shape, host, dtype, which, None, max_nodes, stack_nodes)
        for b, w in enumerate(which):
            check_root(res, b, exp[b], fields, (host, w))
        for b in (1, 2):
            one = run(op, shape, host, dtype, which[b:b + 1], None, max_nodes, stack_nodes)
            for f in fields + ("count", "status"):
                assert torch.equal(getattr(res, f)[b], getattr(one, f)[0]), (host, which[b], f)


class DuckTree:
    """size() and create_node(tag, identifier, parent=, data=), as treelib's Tree"""

    def __init__(self, n0=0):
        self.nodes = [(i, i - 1 if i else None, None) for i in range(n0)]

    def size(self):
        return len(self.nodes)

    def create_node(self, tag=None, identifier=None, parent=None, data=None):
        assert tag == identifier
        self.nodes.append((identifier, parent, data))


# the wrappers' max_nodes bounds the records of a traversal, not the nodes kept: fewer than (max_size + 1) iterations
# of at most 64 popped nodes with at most 7 children each, 18 368 for max_size = 40
WRAPPER_NODES = 1 << 15


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("case", ["tree_64x6", "morin_64x6", "morin_64x7"])
def test_wrappers_match_the_reference_runs(case, dt):
    """search_tree and search_tree_morin into a duck tree at the fixture's (64,6) and (64,7) cases: identifiers,
    parents and data as the reference created them, the "...more..." nodes included"""
    g = golden()
    names = [str(c) for c in g["cases"]]
    more = 0
    for host in HOSTS:
        i = names.index(f"{case}_{host}")
        root = torch.as_tensor(g[f"c{i}_root"], dtype=DTYPES[dt], device="cuda")
        max_size = int(g[f"c{i}_max_size"])
        tree = DuckTree(1)
        if case.startswith("tree"):
            out = search_tree(root, tree, 0, HOSTS[host](), max_size=max_size, max_nodes=WRAPPER_NODES,
                              stack_nodes=WRAPPER_NODES)
            data = [c[2].points for c in tree.nodes[1:]]
            want = [[[r for r in st.tolist() if r[0] >= 0]] for st in g[f"c{i}_states"]]
        else:
            out = search_tree_morin(root, tree, 0, g[f"c{i}_weights"].tolist(), HOSTS[host](), max_size=max_size,
                                    distinguished=int(g[f"c{i}_dist"]), max_nodes=WRAPPER_NODES,
                                    stack_nodes=WRAPPER_NODES)
            data = [c[2].points for c in tree.nodes[1:]]
            want = [str(s) for s in g[f"c{i}_data"]]
            more += want.count(R.MORE)
        assert out is tree, host
        assert [c[0] for c in tree.nodes[1:]] == g[f"c{i}_ident"].tolist(), host
        assert [c[1] for c in tree.nodes[1:]] == g[f"c{i}_parent"].tolist(), host
        assert data == want, host
    assert more >= 1 or case.startswith("tree")


LIMIT_SHAPE = (64, 6)


def _least(passes, lo, hi):
    """the least value in (lo, hi] at which passes() holds, given that it fails at lo, holds at hi and is monotone"""
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if passes(mid) else (mid, hi)
    return hi


@pytest.mark.parametrize("op", ["tree", "morin"])
def test_tree_limits_at_a_narrow_shape(op):
    """(64,6) in float64, 10 lanes: max_nodes one below the recorded nodes sets NODE_LIMIT, at them it does not;
    stack_nodes one below the peak sets STACK_LIMIT.  Both thresholds come from runs with generous limits."""
    host, dtype = "all_coord", torch.float64
    exp = expected(op, LIMIT_SHAPE, host)
    fields = TREE_FIELDS if op == "tree" else MORIN_FIELDS
    n = exp["count"]
    generous = run(op, LIMIT_SHAPE, host, dtype, ("full",), None, 2 * n, 2 * n)
    assert int(generous.count[0]) == n and int(generous.status[0]) == A.HK_SEARCH_DEPTH_LIMIT
    below = run(op, LIMIT_SHAPE, host, dtype, ("full",), None, n - 1, 2 * n)
    assert int(below.status[0]) == A.HK_SEARCH_NODE_LIMIT and int(below.count[0]) <= n - 1
    at = run(op, LIMIT_SHAPE, host, dtype, ("full",), None, n, 2 * n)
    assert int(at.status[0]) == A.HK_SEARCH_DEPTH_LIMIT
    for f in fields:
        assert torch.equal(getattr(at, f)[0], getattr(generous, f)[0, :n]), f

    def fits(stack_nodes):
        r = run(op, LIMIT_SHAPE, host, dtype, ("full",), None, n, stack_nodes)
        assert int(r.status[0]) in (A.HK_SEARCH_DEPTH_LIMIT, A.HK_SEARCH_STACK_LIMIT)
        return int(r.status[0]) == A.HK_SEARCH_DEPTH_LIMIT

    assert not fits(1) and fits(exp["expandable"])  # the pending nodes are nodes that get expanded
    peak = _least(fits, 1, exp["expandable"])
    assert peak >= LIMIT_SHAPE[1]  # the root's children, all pending at once
    r = run(op, LIMIT_SHAPE, host, dtype, ("full",), None, n, peak - 1)
    assert int(r.status[0]) == A.HK_SEARCH_STACK_LIMIT
    check_root(run(op, LIMIT_SHAPE, host, dtype, ("full",), None, n + SPARE, peak), 0, exp, fields, "at the peak")


def test_depth_limits_at_a_narrow_shape():
    host, cap = "all_coord", cap_of("tree", LIMIT_SHAPE, "all_coord")
    root = root_of("tree", LIMIT_SHAPE, "full")[0]
    depth, nodes, status = R.depth_nodes(root, host, cap)
    pts = torch.as_tensor(root[None], dtype=torch.float64, device="cuda")

    def go(max_nodes, stack_nodes):
        r = search_depths(pts, HOSTS[host](), max_depth=cap, max_nodes=max_nodes, stack_nodes=stack_nodes)
        return int(r.depth[0]), int(r.nodes[0]), int(r.status[0])

    assert go(2 * nodes, 2 * nodes) == (depth, nodes, status)
    assert go(nodes, 2 * nodes) == (depth, nodes, status)
    got = go(nodes - 1, 2 * nodes)
    assert got[2] == status | A.HK_SEARCH_NODE_LIMIT and got[1] == nodes - 1
    assert go(nodes, 1)[2] & A.HK_SEARCH_STACK_LIMIT
    peak = _least(lambda s: not go(nodes, s)[2] & A.HK_SEARCH_STACK_LIMIT, 1, nodes)
    assert peak >= LIMIT_SHAPE[1]
    assert go(nodes, peak - 1)[2] & A.HK_SEARCH_STACK_LIMIT
    assert go(nodes, peak) == (depth, nodes, status)


CHUNK_SHAPE = (33, 4)
CHUNK_ROOTS = ("full", "one_first", "sparse", "tail", "sparse", "one_last", "full", "tail")


@pytest.mark.parametrize("op", ["depth", "tree", "morin"])
def test_chunked_launches(op, monkeypatch):
    """a batch of 8 roots split into launches of 3, 3 and 2 roots that share one workspace gives the unsplit call's
    results: ops._search_launch for search_depth and search_game_tree, and the loop of ops.search_morin_tree"""
    m, d = CHUNK_SHAPE
    host, dtype = "zeillinger_lex", torch.float32
    kind = "tree" if op == "depth" else op
    max_nodes, stack_nodes = budget(kind, CHUNK_SHAPE, host, CHUNK_ROOTS)
    L = _lib.lib()
    if op == "depth":
        per_root = L.hk_search_depth_workspace_bytes(1, m, d, A.HK_F32, stack_nodes)
        pts = torch.as_tensor(np.stack([root_of(kind, CHUNK_SHAPE, w)[0] for w in CHUNK_ROOTS]), dtype=dtype,
                              device="cuda")

        def call():
            return search_depths(pts, HOSTS[host](), max_depth=FINITE_CAP, max_nodes=1 << 20, stack_nodes=stack_nodes)
    else:
        fn = L.hk_search_game_tree_workspace_bytes if op == "tree" else L.hk_search_morin_tree_workspace_bytes
        per_root = fn(1, m, d, A.HK_F32, max_nodes, stack_nodes)

        def call():
            return run(op, CHUNK_SHAPE, host, dtype, CHUNK_ROOTS, None, max_nodes, stack_nodes)

    assert per_root > 0
    whole = call()
    launches = []
    check = ops.check
    monkeypatch.setattr(ops, "check", lambda status, name: (launches.append(name), check(status, name))[1])
    monkeypatch.setattr(ops, "_SEARCH_WORKSPACE_BYTES", 3 * per_root + per_root // 2)
    split = call()
    assert len(launches) == 3
    for x, y in zip(whole, split):
        assert torch.equal(x, y)
    if op != "depth":
        fields = TREE_FIELDS if op == "tree" else MORIN_FIELDS
        for b, w in enumerate(CHUNK_ROOTS):
            check_root(split, b, expected(op, CHUNK_SHAPE, host, w), fields, w)
