"""hk_search_morin_tree / hironaka_amd.util.search_tree_morin on the GPU: exact parity with the reference's own
search_tree_morin (tests/golden/search_morin.npz, tests/golden/make_search_morin_golden.py), the tensor form's
structure, the loss rules on hand-made roots, truncation and the limits."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import _lib
from hironaka_amd import ops
from hironaka_amd.core import HipPoints
from hironaka_amd.host import AllCoordHost, WeakSpivakovsky, WeakSpivakovskyMinHitting, Zeillinger, ZeillingerLex
from hironaka_amd.util import search_tree_morin, search_trees, search_trees_morin

pytestmark = pytest.mark.gpu

HOSTS = {"zeillinger": Zeillinger, "all_coord": AllCoordHost, "zeillinger_lex": ZeillingerLex,
         "weak_spivakovsky": WeakSpivakovsky, "weak_spivakovsky_min_hitting": WeakSpivakovskyMinHitting}
# max_nodes bounds the records, not the nodes kept.  A full fixture tree holds <= 3000 nodes.  With max_size the
# traversal runs L + 1 <= 101 iterations (the 10000 case ends at 37 nodes), each popping at most 64 nodes that make at
# most 7 children: fewer than 1 + 101 * 64 * 7 = 45 249 records, which the all-coordinates host's endless trees approach.
NODES = 1 << 16


class DuckTree:
    """size() and create_node(tag, identifier, parent=, data=), as treelib's Tree"""

    def __init__(self, n0=0):
        self.nodes = [(i, i - 1 if i else None, None) for i in range(n0)]

    def size(self):
        return len(self.nodes)

    def create_node(self, tag=None, identifier=None, parent=None, data=None):
        assert tag == identifier
        self.nodes.append((identifier, parent, data))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "search_morin.npz"))


def _case(golden, i):
    max_size, n0, curr, dist = (int(v) for v in golden[f"c{i}_meta"])
    return (golden[f"c{i}_root"], golden[f"c{i}_weights"].tolist(), dist, str(golden[f"c{i}_host"]),
            None if max_size < 0 else max_size, n0, curr)


def _index(golden, name):
    return [str(c) for c in golden["cases"]].index(name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fixture_parity(golden, dtype):
    for i, name in enumerate(golden["cases"]):
        root, weights, dist, host, max_size, n0, curr = _case(golden, i)
        tree = DuckTree(n0)
        out = search_tree_morin(torch.as_tensor(root, dtype=dtype, device="cuda"), tree, curr, weights, HOSTS[host](),
                                max_size=max_size, distinguished=dist, max_nodes=NODES)
        assert out is tree, name
        new = tree.nodes[n0:]
        assert [c[0] for c in new] == golden[f"c{i}_ident"].tolist(), name
        assert [c[1] for c in new] == golden[f"c{i}_parent"].tolist(), name
        assert [c[2].points for c in new] == [str(s) for s in golden[f"c{i}_data"]], name
        assert all(type(c[2]).__name__ == "Node" and c[2]._fields == ("points",) for c in new), name


def test_thom_tree_original_as_in_test_thom(golden):
    # test/testThom.py:94-114, called as there; the root is the fixture's array (the reference makes it with sympy)
    points = golden[f"c{_index(golden, 'thom_original')}_root"].tolist()
    dimension = len(points[0])
    assert dimension == 7 and len(points) == 19
    initial_points = HipPoints([points], max_num_points=len(points), distinguished_points=[len(points) - 1])
    tree = DuckTree()
    tree.create_node(0, 0, data=initial_points)
    host = WeakSpivakovsky()
    weights = [1, 1, 2, 3, 2, 3, 3]
    out = search_tree_morin(initial_points, tree, 0, weights, host, max_size=10000)
    assert out is tree
    assert tree.size() == 37
    # numpy weights, as the reference accepts them
    again = DuckTree(1)
    search_tree_morin(initial_points, again, 0, np.asarray(weights), host, max_size=10000)
    assert [(c[0], c[1], c[2].points) for c in again.nodes[1:]] == [(c[0], c[1], c[2].points) for c in tree.nodes[1:]]


def _mask(cls, d):
    # the subset of a class id (hk_step's coords codec): ids count the masks with >= 2 bits in ascending order
    masks = [v for v in range(1 << d) if bin(v).count("1") >= 2]
    return masks[cls]


def test_tensor_form_matches_per_root_calls_and_the_rules(golden):
    # the full-tree fixture roots of one dimension and host in one call, padded with -1 rows to one shape
    groups = {}
    for i in range(len(golden["cases"])):
        root, weights, dist, host, max_size, n0, curr = _case(golden, i)
        if max_size is None and n0 == 1:
            groups.setdefault((root.shape[1], host), []).append(i)
    assert {k[0] for k in groups} == {2, 3, 4, 5, 6, 7}
    assert {k[0] for k, v in groups.items() if len(v) >= 2} == {2, 3, 4, 5, 6, 7}
    seen_gap = False
    for (d, host), idx in groups.items():
        m = max(golden[f"c{i}_root"].shape[0] for i in idx)
        padded = np.full((len(idx), m, d), -1, np.int64)
        for b, i in enumerate(idx):
            padded[b, :golden[f"c{i}_root"].shape[0]] = golden[f"c{i}_root"]
        roots = torch.as_tensor(padded, dtype=torch.float64, device="cuda")
        wts = torch.as_tensor(np.stack([golden[f"c{i}_weights"] for i in idx]), device="cuda")
        dst = torch.as_tensor(np.asarray([int(golden[f"c{i}_meta"][3]) for i in idx]), device="cuda")
        res = search_trees_morin(roots, wts, dst, HOSTS[host](), max_nodes=NODES)
        assert (res.status == 0).all()
        for b, i in enumerate(idx):
            n = int(res.count[b])
            assert n == len(golden[f"c{i}_ident"]) + 1  # no "...more..." in a full tree
            one = search_trees_morin(roots[b:b + 1], wts[b:b + 1], dst[b:b + 1], HOSTS[host](), max_nodes=NODES)
            for f in ("parent", "child_index", "axis", "depth", "num_points", "host_class", "kind", "distinguished",
                      "weights", "states"):
                assert torch.equal(getattr(res, f)[b, :n], getattr(one, f)[0, :n]), (f, i)
                assert (getattr(res, f)[b, n:] == -1).all(), (f, i)
            par, chd, ax = res.parent[b, :n].tolist(), res.child_index[b, :n].tolist(), res.axis[b, :n].tolist()
            cls, kind, dist = res.host_class[b, :n].tolist(), res.kind[b, :n].tolist(), res.distinguished[b, :n].tolist()
            w, npts = res.weights[b, :n].tolist(), res.num_points[b, :n].tolist()
            states = res.states[b, :n].cpu().numpy()
            data = ["root"] + [str(s) for s in golden[f"c{i}_data"]]
            children = {}
            for j in range(1, n):
                p = par[j]
                assert cls[p] >= 0 and kind[p] == 0
                coords = [k for k in range(d) if (_mask(cls[p], d) >> k) & 1]
                assert ax[j] in coords
                assert w[j] == [w[p][k] - w[p][ax[j]] if k in coords and k != ax[j] else w[p][k] for k in range(d)]
                assert w[p][ax[j]] == min(w[p][k] for k in coords)  # not pruned
                children.setdefault(p, []).append(chd[j])
                live = states[j][states[j][:, 0] >= 0].astype(np.int64).tolist()
                assert len(live) == npts[j]
                if kind[j] == 0:
                    assert 0 <= dist[j] < npts[j]
                    assert data[j] == str([live]) + f", {[dist[j]]}"
                else:
                    assert kind[j] == 1 and dist[j] == -1 and cls[j] == -1 and data[j] == "No contribution"
            for p, got in children.items():
                coords = [k for k in range(d) if (_mask(cls[p], d) >> k) & 1]
                if host not in ("zeillinger", "zeillinger_lex"):  # their lists are [argmin, argmax], often descending
                    lowest = min(w[p][k] for k in coords)
                    want = [pos for pos, k in enumerate(coords) if w[p][k] == lowest]
                    assert got == want, (i, p)
                    seen_gap |= len(want) < len(coords)
                else:
                    assert got == sorted(got) and set(got) <= {0, 1}
    assert seen_gap


def _one(rows, dist, weights, host=AllCoordHost, **kw):
    tree = DuckTree(1)
    search_tree_morin(rows, tree, 0, weights, host(), distinguished=dist, **kw)
    return [(c[0], c[1], c[2].points) for c in tree.nodes[1:]]


def test_loss_to_an_identical_row_to_a_smaller_row_and_the_kept_case():
    # max_size=1 with the caller's root in the tree: the root alone is expanded.  Weights [1, 2]: the all-coordinates
    # host's action 1 is pruned, action 0 makes x0 <- x0 + x1.
    # identical: the distinguished row has a twin, so the marked row sorts first and is removed as contained
    assert _one([[1, 2], [1, 2], [3, 0]], 0, [1, 2], max_size=1) == [(1, 0, "No contribution")]
    assert _one([[1, 2], [1, 2], [3, 0]], 1, [1, 2], max_size=1) == [(1, 0, "No contribution")]
    # strictly smaller: (0, 3) -> (3, 3), (2, 0) -> (2, 0), (1, 1) -> (2, 1); after the reposition by (2, 0) the
    # distinguished (1, 3) lies above (0, 0)
    assert _one([[0, 3], [2, 0], [1, 1]], 0, [1, 2], max_size=1) == [(1, 0, "No contribution")]
    # kept: the same root with the distinguished point (2, 0) -> (0, 0), the only vertex left; the ended node is
    # reached with tree.size() > max_size and gets its "...more..."
    assert _one([[0, 3], [2, 0], [1, 1]], 1, [1, 2], max_size=1) == [(1, 0, "[[[0, 0]]], [0]"), (2, 1, "...more...")]
    # kept among several: (0, 3) -> (3, 3), (4, 0) -> (4, 0), (1, 1) -> (2, 1); repositioned by (2, 0) and sorted:
    # (2, 0), (1, 3), (0, 1), of which (1, 3) lies above (0, 1).  The distinguished (0, 1) ends at row 1.
    assert _one([[0, 3], [4, 0], [1, 1]], 2, [1, 2], max_size=1) == [(1, 0, "[[[2, 0], [0, 1]]], [1]"),
                                                                    (2, 1, "...more...")]
    # equal weights: both actions, in list order
    assert _one([[0, 3], [4, 0], [1, 1]], 2, [1, 1], max_size=1) == [
        (1, 0, "[[[2, 0], [0, 1]]], [1]"), (2, 1, "...more..."), (3, 0, "[[[1, 0], [0, 1]]], [0]"), (4, 3, "...more...")]


def test_truncation_on_the_thom_root(golden):
    i_full = _index(golden, "thom4_weak_spivakovsky_full")
    root, weights, dist, host, _, _, _ = _case(golden, i_full)
    for size in (0, 1):
        i = _index(golden, f"thom4_weak_spivakovsky_{size}")
        tree = DuckTree(1)
        search_tree_morin(root.tolist(), tree, 0, weights, WeakSpivakovsky(), max_size=size, distinguished=dist)
        assert [(c[0], c[1], c[2].points) for c in tree.nodes[1:]] == list(zip(
            golden[f"c{i}_ident"].tolist(), golden[f"c{i}_parent"].tolist(), [str(s) for s in golden[f"c{i}_data"]]))
    # a call that starts with tree.size() > max_size adds exactly one "...more..." below curr_node
    tree = DuckTree(4)
    assert search_tree_morin(root.tolist(), tree, 2, weights, WeakSpivakovsky(), max_size=3, distinguished=dist) is tree
    assert [(c[0], c[1], c[2].points) for c in tree.nodes[4:]] == [(4, 2, "...more...")]
    tree = DuckTree(4)  # even for an ended root
    search_tree_morin([[1, 2, 3]], tree, 2, [1, 1, 1], WeakSpivakovsky(), max_size=3, distinguished=0)
    assert [(c[0], c[1], c[2].points) for c in tree.nodes[4:]] == [(4, 2, "...more...")]
    tree = DuckTree(1)  # an ended root within max_size adds nothing
    assert search_tree_morin([[1, 2, 3]], tree, 0, [1, 1, 1], WeakSpivakovsky(), distinguished=0) is tree
    assert tree.size() == 1
    tree = DuckTree(1)
    search_tree_morin(root.tolist(), tree, 0, weights, WeakSpivakovsky(), max_size=None, distinguished=dist)
    assert [(c[0], c[1], c[2].points) for c in tree.nodes[1:]] == list(zip(
        golden[f"c{i_full}_ident"].tolist(), golden[f"c{i_full}_parent"].tolist(),
        [str(s) for s in golden[f"c{i_full}_data"]]))


def test_limits(golden):
    root, weights, dist, _, _, _, _ = _case(golden, _index(golden, "thom4_weak_spivakovsky_full"))
    n_full = len(golden[f"c{_index(golden, 'thom4_weak_spivakovsky_full')}_ident"]) + 1
    host = WeakSpivakovsky()
    res = search_trees_morin([root.tolist()], [weights], [dist], host, max_nodes=n_full - 1)
    assert int(res.status[0]) == A.HK_SEARCH_NODE_LIMIT
    res = search_trees_morin([root.tolist()], [weights], [dist], host, max_nodes=n_full)
    assert int(res.status[0]) == 0 and int(res.count[0]) == n_full
    branching = [[0, 3], [4, 0], [1, 1]]  # with equal weights both children of the root can be expanded
    res = search_trees_morin([branching], [[1, 1]], [2], AllCoordHost(), stack_nodes=1)
    assert int(res.status[0]) == A.HK_SEARCH_STACK_LIMIT
    res = search_trees_morin([branching], [[1, 1]], [2], AllCoordHost(), stack_nodes=2)
    assert int(res.status[0]) == 0
    with pytest.raises(RuntimeError, match="stack_nodes"):
        search_tree_morin(branching, DuckTree(1), 0, [1, 1], AllCoordHost(), distinguished=2, stack_nodes=1)
    with pytest.raises(RuntimeError, match="max_nodes"):
        search_tree_morin(root.tolist(), DuckTree(1), 0, weights, host, distinguished=dist, max_nodes=8)
    # float32 leaves its exact integers at 2^24: x0 <- x0 + x1 = 2^24 at the first shift; float64 holds it
    big = [[2 ** 24 - 2, 2, 0], [0, 0, 5], [1, 7, 1]]
    res = search_trees_morin([big], [[1, 1, 1]], [2], AllCoordHost(), dtype=torch.float32, max_size=3, max_nodes=64)
    assert int(res.status[0]) == A.HK_SEARCH_INEXACT
    res = search_trees_morin([big], [[1, 1, 1]], [2], AllCoordHost(), dtype=torch.float64, max_size=3, max_nodes=64)
    assert int(res.status[0]) == 0
    # a bad distinguished index (a padding row, out of range, negative) or a negative weight: that root only
    roots = [[[0, 3], [4, 0], [1, 1], [-1, -1]]] * 6
    dists = [2, 3, 4, -1, 2, 2]
    wts = [[1, 2]] * 4 + [[1, -1]] + [[1, 2]]
    res = search_trees_morin(roots, wts, dists, AllCoordHost(), max_nodes=64)
    assert res.status.tolist() == [0] + [A.HK_SEARCH_ROOT_INVALID] * 4 + [0]
    assert res.count[1:5].tolist() == [1] * 4
    one = search_trees_morin(roots[:1], wts[:1], dists[:1], AllCoordHost(), max_nodes=64)
    for b in (0, 5):
        for f in ("parent", "child_index", "kind", "distinguished", "weights", "states", "count"):
            assert torch.equal(getattr(res, f)[b], getattr(one, f)[0]), f
    assert int(one.count[0]) > 1
    with pytest.raises(ValueError):
        search_tree_morin(roots[0], DuckTree(1), 0, [1, 2], AllCoordHost(), distinguished=3)
    with pytest.raises(ValueError):
        search_tree_morin(roots[0], DuckTree(1), 0, [1, 2], AllCoordHost(), distinguished=7)
    # fewer than 2 points
    res = search_trees_morin([[[1, 2], [-1, -1]]], [[1, 1]], [0], AllCoordHost(), max_nodes=8)
    assert int(res.status[0]) == A.HK_SEARCH_ROOT_ENDED and int(res.count[0]) == 1


def test_other_search_operators_still_refuse_dim_7(golden):
    root = torch.as_tensor(golden[f"c{_index(golden, 'thom4_weak_spivakovsky_full')}_root"], dtype=torch.float32,
                           device="cuda")
    assert root.shape == (19, 7)
    with pytest.raises(_lib.HironakaHipError) as e:
        search_trees(root, WeakSpivakovsky(), max_nodes=64)
    assert e.value.status == A.HK_ERR_UNSUPPORTED
    with pytest.raises(_lib.HironakaHipError):
        ops.search_depth(root.unsqueeze(0), "weak_spivakovsky", max_depth=8, max_nodes=64, stack_nodes=16)
