"""tests/search_rules.py, the plain restatement of search_depth, search_tree and search_tree_morin that the GPU tests
of the large shapes compare the kernels with, pinned to the reference: node for node against the fixtures made by
running the reference's own functions (search_tree.npz, search_morin.npz, search_depth.npz, the depth groups of
hosts.npz) and against search_sizes.npz, the reference's runs at the largest shapes the operators accept
(tests/golden/make_search_sizes_golden.py)."""
import os

import numpy as np
import pytest

import search_rules as R
from conftest import GOLDEN

NODE_BOUND = 20000  # depth roots above it are left to the GPU tests (the 5552 root among them)
SHAPES = ((64, 2), (64, 3), (33, 4), (48, 5), (64, 6))
MORIN_SHAPES = ((33, 4), (64, 6), (24, 7), (64, 7))


def _load(name):
    return np.load(os.path.join(GOLDEN, name))


def _states_equal(t, j, want):
    return R.rows_of(t.states[j]) == [r for r in np.asarray(want).tolist() if r[0] >= 0]


def test_search_tree_fixture():
    g = _load("search_tree.npz")
    assert len(g["cases"]) >= 100
    for i, name in enumerate(g["cases"]):
        max_size, n0, curr = (int(v) for v in g[f"c{i}_meta"])
        t = R.tree(g[f"c{i}_root"], str(g[f"c{i}_host"]), None if max_size < 0 else max_size, s0=n0)
        calls = R.created(t, n0, curr)
        assert [c[0] for c in calls] == g[f"c{i}_ident"].tolist(), name
        assert [c[1] for c in calls] == g[f"c{i}_parent"].tolist(), name
        assert all(_states_equal(t, j + 1, st) for j, st in enumerate(g[f"c{i}_states"])), name
        assert t.status == 0


def test_search_morin_fixture():
    g = _load("search_morin.npz")
    stats = [0, 0, 0, 0]
    for i, name in enumerate(g["cases"]):
        max_size, n0, curr, dist = (int(v) for v in g[f"c{i}_meta"])
        t = R.morin_tree(g[f"c{i}_root"], g[f"c{i}_weights"], dist, str(g[f"c{i}_host"]),
                         None if max_size < 0 else max_size, s0=n0, stats=stats)
        calls = R.created(t, n0, curr)
        assert [c[0] for c in calls] == g[f"c{i}_ident"].tolist(), name
        assert [c[1] for c in calls] == g[f"c{i}_parent"].tolist(), name
        assert [R.morin_data(t, j) for j in range(1, len(t.parent))] == [str(s) for s in g[f"c{i}_data"]], name
    assert stats == g["stats"].tolist()


def _depth_groups():
    dep = _load("search_depth.npz")
    for g in dep["groups"]:
        yield str(g), str(dep[f"{g}_host"]), dep[f"{g}_roots"], dep[f"{g}_depth"], dep[f"{g}_nodes"]
    hosts = _load("hosts.npz")
    for host in ("zeillinger_lex", "weak_spivakovsky", "weak_spivakovsky_min_hitting"):
        for d in (3, 4):
            g = f"depth_{host}{d}"
            yield g, host, hosts[f"{g}_roots"], hosts[f"{g}_depth"], hosts[f"{g}_nodes"]


def test_search_depth_fixtures():
    seen = left = 0
    for g, host, roots, depth, nodes in _depth_groups():
        for root, dp, nd in zip(roots, depth, nodes):
            if nd > NODE_BOUND:
                left += 1
                continue
            assert R.depth_nodes(root, host) == (dp, nd, 0), (g, root.tolist())
            seen += 1
    assert seen >= 300 and left >= 1


def test_depth_cap_counts_the_tree_cut_there():
    # hk_search_depth visits the nodes at max_depth without expanding them; search_tree's nodes with >= 2 points are
    # search_depth's nodes, at any cap
    g = _load("search_depth.npz")
    root = g["z4_roots"][int(np.argmax(g["z4_nodes"] * (g["z4_nodes"] < 2000)))]
    full = R.tree(root, "zeillinger")
    for cap in (0, 1, 3, max(full.depth) + 1):
        dp, nd, status = R.depth_nodes(root, "zeillinger", cap)
        t = R.tree(root, "zeillinger", max_depth=cap)
        assert nd == sum(n >= 2 for n in t.num_points)
        assert dp == 1 + max(dep for dep, n in zip(t.depth, t.num_points) if n >= 2)
        assert status == t.status == (R.DEPTH_LIMIT if cap <= max(full.depth) - 1 else 0)
        assert len(t.parent) == sum(dep <= cap for dep in full.depth)


@pytest.fixture(scope="module")
def sizes():
    return _load("search_sizes.npz")


def test_sizes_fixture_covers_every_operator_shape_and_host(sizes):
    seen = set()
    for i, name in enumerate(sizes["cases"]):
        root = sizes[f"c{i}_root"]
        seen.add((str(sizes[f"c{i}_op"]), root.shape, str(sizes[f"c{i}_host"])))
        assert int(sizes[f"c{i}_max_size"]) >= 1
        # all rows live and pairwise incomparable: neither the reference nor a kernel changes such a root
        assert (root >= 0).all() and len(R.newton(root)) == len(root), name
    assert seen == ({("tree", s, h) for s in SHAPES for h in R.HOSTS} |
                    {("morin", s, h) for s in MORIN_SHAPES for h in R.HOSTS})
    assert os.path.getsize(os.path.join(GOLDEN, "search_sizes.npz")) < 1000000
    for m, d in set(SHAPES) | set(MORIN_SHAPES):
        for kind in ("sparse", "tail"):
            r = sizes[f"root_{m}x{d}_{kind}"]
            pts = R.live(r)
            assert r.shape == (m, d) and 2 <= len(pts) < m and len(R.newton(pts)) == len(pts)
        assert (sizes[f"root_{m}x{d}_sparse"][::2, 0] < 0).any()  # padding between the points


def test_sizes_fixture(sizes):
    for i, name in enumerate(sizes["cases"]):
        root, host, max_size = sizes[f"c{i}_root"], str(sizes[f"c{i}_host"]), int(sizes[f"c{i}_max_size"])
        ident, parent = sizes[f"c{i}_ident"].tolist(), sizes[f"c{i}_parent"].tolist()
        if str(sizes[f"c{i}_op"]) == "tree":
            t = R.tree(root, host, max_size)
            assert all(_states_equal(t, j + 1, st) for j, st in enumerate(sizes[f"c{i}_states"])), name
        else:
            t = R.morin_tree(root, sizes[f"c{i}_weights"], int(sizes[f"c{i}_dist"]), host, max_size)
            assert [R.morin_data(t, j) for j in range(1, len(t.parent))] == [str(s) for s in sizes[f"c{i}_data"]], name
        assert len(ident) >= 3, name
        assert R.created(t) == list(zip(ident, parent)), name


def test_without_more_drops_the_reference_only_nodes(sizes):
    i = [str(c) for c in sizes["cases"]].index("morin_64x7_all_coord")
    t = R.morin_tree(sizes[f"c{i}_root"], sizes[f"c{i}_weights"], int(sizes[f"c{i}_dist"]), "all_coord",
                     int(sizes[f"c{i}_max_size"]))
    k = R.without_more(t)
    assert R.KIND_MORE in t.kind and R.KIND_MORE not in k.kind and len(k.parent) == sum(v != R.KIND_MORE for v in t.kind)
    assert all(0 <= p < j for j, p in enumerate(k.parent) if j) and k.parent[0] == -1
    assert [R.morin_data(k, j) for j in range(len(k.parent))] == [R.morin_data(t, j) for j in range(len(t.parent))
                                                                 if t.kind[j] != R.KIND_MORE]
