"""hk_search_game_tree / hironaka_amd.util.search_tree on the GPU: exact parity with the reference's own search_tree
(tests/golden/search_tree.npz, tests/golden/make_search_tree_golden.py), consistency with the pinned search_depth
numbers, the tree's structure, and the limits."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import ops
from hironaka_amd.host import AllCoordHost, WeakSpivakovsky, WeakSpivakovskyMinHitting, Zeillinger, ZeillingerLex
from hironaka_amd.util import search_depths, search_tree, search_trees

pytestmark = pytest.mark.gpu

HOSTS = {"zeillinger": Zeillinger, "all_coord": AllCoordHost, "zeillinger_lex": ZeillingerLex,
         "weak_spivakovsky": WeakSpivakovsky, "weak_spivakovsky_min_hitting": WeakSpivakovskyMinHitting}
LITERAL = [(0, 0, 4), (5, 0, 1), (1, 5, 1), (0, 25, 0)]


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
    return np.load(os.path.join(GOLDEN, "search_tree.npz"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fixture_parity(golden, dtype):
    for i, name in enumerate(golden["cases"]):
        root = torch.as_tensor(golden[f"c{i}_root"], dtype=dtype, device="cuda")
        max_size, n0, curr = (int(v) for v in golden[f"c{i}_meta"])
        tree = DuckTree(n0)
        out = search_tree(root, tree, curr, HOSTS[str(golden[f"c{i}_host"])](),
                          max_size=None if max_size < 0 else max_size)
        ident, parent, states = golden[f"c{i}_ident"], golden[f"c{i}_parent"], golden[f"c{i}_states"]
        assert (out is None) == (len(ident) == 0), name
        new = tree.nodes[n0:]
        assert [c[0] for c in new] == ident.tolist(), name
        assert [c[1] for c in new] == parent.tolist(), name
        for j, c in enumerate(new):
            want = [r for r in states[j].tolist() if r[0] >= 0]
            assert c[2].points == [want], (name, j)


def test_reference_literal_as_in_test_search(golden):
    # test/testSearch.py:42-50, called exactly as there
    host = Zeillinger()
    points = [list(r) for r in LITERAL]
    tree = DuckTree()
    tree.create_node(0, 0, data=points)
    out = search_tree(points, tree, 0, host)
    assert out is tree and tree.size() == 107
    assert [c[0] for c in tree.nodes] == list(range(107))
    assert [c[1] for c in tree.nodes[1:]] == golden["c0_parent"].tolist()
    assert [str(c[2]) for c in tree.nodes[1:]] == golden["lit_str"].tolist()
    for c in tree.nodes[1:]:
        assert c[2].batch_size == 1 and c[2].ended == (len(c[2].points[0]) <= 1)


def test_root_ended_and_oversized_tree_add_nothing():
    tree = DuckTree(1)
    assert search_tree([[1, 2, 3]], tree, 0, Zeillinger()) is None
    assert search_tree([[1, 2, 3], [-1, -1, -1]], tree, 0, Zeillinger()) is None
    assert tree.size() == 1
    tree = DuckTree(5)
    assert search_tree(LITERAL, tree, 0, Zeillinger(), max_size=4) is None
    assert tree.size() == 5
    r = search_trees([[[1, 2, 3], [-1, -1, -1]]], Zeillinger(), max_nodes=8)
    assert int(r.status[0]) == A.HK_SEARCH_ROOT_ENDED and int(r.count[0]) == 1
    assert int(r.parent[0, 0]) == -1 and int(r.host_class[0, 0]) == -1 and int(r.num_points[0, 0]) == 1


def _depth_groups():
    dep = np.load(os.path.join(GOLDEN, "search_depth.npz"))
    for g in dep["groups"]:
        yield str(g), str(dep[f"{g}_host"]), dep[f"{g}_roots"], dep[f"{g}_depth"], dep[f"{g}_nodes"]
    hosts = np.load(os.path.join(GOLDEN, "hosts.npz"))
    for host in ("zeillinger_lex", "weak_spivakovsky", "weak_spivakovsky_min_hitting"):
        for d in (3, 4):
            g = f"depth_{host}{d}"
            if len(hosts[f"{g}_roots"]):
                yield g, host, hosts[f"{g}_roots"], hosts[f"{g}_depth"], hosts[f"{g}_nodes"]


def test_consistent_with_search_depth():
    """expanded nodes == search_depth's nodes, 1 + their largest depth == its depth; Zeillinger: count = 1 + 2 nodes"""
    for g, host, roots, depth, nodes in _depth_groups():
        sel = np.nonzero(nodes <= 100000)[0]  # the 5552 root: test_the_5552_root
        if len(sel):
            cap = int(1 + roots.shape[2] * nodes[sel].max())
            r = search_trees(torch.as_tensor(roots[sel], device="cuda"), HOSTS[host](), max_nodes=cap,
                             stack_nodes=1 << 16, states=False)
            assert (r.status.cpu().numpy() == 0).all(), g
            cls = r.host_class.cpu().numpy()
            dep = r.depth.cpu().numpy()
            expanded = cls >= 0
            assert np.array_equal(expanded.sum(1), nodes[sel]), g
            assert np.array_equal(np.where(expanded, dep, -1).max(1) + 1, depth[sel]), g
            if host == "zeillinger":
                assert np.array_equal(r.count.cpu().numpy(), 1 + 2 * nodes[sel]), g


def test_the_5552_root():
    dep = np.load(os.path.join(GOLDEN, "search_depth.npz"))
    r = search_trees(dep["lit4_roots"][:1], Zeillinger(), max_nodes=1 << 21, stack_nodes=1 << 16, states=False)
    assert int(r.status[0]) == 0
    assert int(r.count[0]) == 1128897
    assert int((r.host_class[0] >= 0).sum()) == 564448
    assert int(r.depth[0].max()) == 5552


def _check_structure(r, b):
    n = int(r.count[b])
    par = r.parent[b, :n].cpu().numpy()
    ci = r.child_index[b, :n].cpu().numpy()
    assert par[0] == -1 and (par[1:] < np.arange(1, n)).all() and (par[1:] >= 0).all()
    size = np.ones(n, np.int64)
    for j in range(n - 1, 0, -1):
        size[par[j]] += size[j]
    # preorder: the first child follows its parent, each later sibling follows the previous one's subtree, siblings
    # in host-list order; so the subtree of j is [j, j + size_j)
    last = {}
    for j in range(1, n):
        p = par[j]
        if p in last:
            k = last[p]
            assert j == k + size[k] and ci[j] == ci[k] + 1
        else:
            assert j == p + 1 and ci[j] == 0
        last[p] = j
        assert j < p + size[p]
    assert size[0] == n
    return par


@pytest.mark.parametrize("host", list(HOSTS))
def test_structure_and_one_step_per_edge(host):
    """the tree is in preorder with siblings in host order, and every child is its parent after one list-semantics
    step with the parent's host class and the child's axis (one batched hk_step over all edges)"""
    dep = np.load(os.path.join(GOLDEN, "search_depth.npz"))
    roots = torch.as_tensor(dep["z4_roots"] if host != "all_coord" else dep["a2_roots"], device="cuda")
    if host in ("weak_spivakovsky", "weak_spivakovsky_min_hitting"):
        hosts = np.load(os.path.join(GOLDEN, "hosts.npz"))
        roots = torch.as_tensor(hosts[f"depth_{host}4_roots"], device="cuda")
    r0 = search_depths(roots, HOSTS[host]())
    b = int(torch.argmax(r0.nodes * (r0.nodes < 20000)))  # the largest tree below 20 000 expanded nodes
    r = search_trees(roots[b:b + 1], HOSTS[host](), max_nodes=1 + 4 * 20000)
    assert int(r.status[0]) == 0
    par = _check_structure(r, 0)
    n = len(par)
    assert n >= 3
    st = r.states[0, :n]
    cls = r.host_class[0, :n]
    kids = torch.arange(1, n, device="cuda")
    p = r.parent[0, 1:n].long()
    assert (cls[p] >= 0).all()
    flags = A.HK_SEM_LIST | A.HK_FLAG_COMPACT_SORTED
    child = ops.step(st[p].contiguous(), cls[p].contiguous(), r.axis[0, 1:n].contiguous(),
                     stages=A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON, flags=flags)["points"]
    assert torch.equal(child, st[kids])
    assert torch.equal(r.num_points[0, :n], ops.get_num_points(st).to(torch.int32))
    assert torch.equal(r.depth[0, 1:n], r.depth[0, p] + 1)


def test_truncation_keeps_the_full_trees_prefix():
    """at every expand_limit L the first L+2 nodes are the full tree's; the rest are trailing siblings"""
    root = torch.as_tensor([LITERAL], dtype=torch.float32, device="cuda")
    full = ops.search_game_tree(root, "zeillinger", expand_limit=None, max_depth=1 << 20, max_nodes=4096,
                                stack_nodes=4096)
    nf = int(full[7][0])
    assert nf == 1583
    for L in (0, 1, 5, 63, 64, 65, 99, 500, 1581, 1582, 5000):
        t = ops.search_game_tree(root, "zeillinger", expand_limit=L, max_depth=1 << 20, max_nodes=4096,
                                 stack_nodes=4096)
        n = int(t[7][0])
        k = min(L + 2, nf)
        for i in (0, 1, 2, 3, 4, 6):  # parent, child_index, axis, depth, num_points, states
            assert torch.equal(full[i][0, :k], t[i][0, :k]), (L, i)
        assert torch.equal(full[5][0, :min(L + 1, nf)], t[5][0, :min(L + 1, nf)]), L
        assert n >= k and (n == nf) == (L + 2 >= nf)
        expanded = t[5][0, :n] >= 0
        assert not expanded[L + 1:].any()


def test_limits_set_their_bits():
    root = [LITERAL]
    r = search_trees(root, Zeillinger(), max_depth=3, max_nodes=4096)
    assert int(r.status[0]) == A.HK_SEARCH_DEPTH_LIMIT
    full = search_trees(root, Zeillinger(), max_nodes=4096)
    keep = (full.depth[0, :int(full.count[0])] <= 3).cpu().numpy()
    assert int(r.count[0]) == int(keep.sum())
    assert int(r.depth[0, :int(r.count[0])].max()) == 3
    assert int(search_trees(root, Zeillinger(), max_nodes=100).status[0]) & A.HK_SEARCH_NODE_LIMIT
    assert int(search_trees(root, Zeillinger(), max_nodes=4096, stack_nodes=1).status[0]) & A.HK_SEARCH_STACK_LIMIT
    big = [[[2 ** 24 - 1, 1, 5], [1, 2 ** 24 - 1, 0]]]  # a shift of axis 0 reaches 2^24
    r = search_trees(big, Zeillinger(), max_nodes=64, dtype=torch.float32)
    assert int(r.status[0]) & A.HK_SEARCH_INEXACT
    assert int(search_trees(big, Zeillinger(), max_nodes=64, dtype=torch.float64).status[0]) & A.HK_SEARCH_INEXACT == 0
    with pytest.raises(RuntimeError, match="max_nodes"):
        search_tree(root, DuckTree(1), 0, Zeillinger(), max_size=None, max_nodes=100)
    with pytest.raises(RuntimeError, match="stack_nodes"):
        search_tree(root, DuckTree(1), 0, Zeillinger(), max_size=None, stack_nodes=1)
