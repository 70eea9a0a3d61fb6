"""hk_search_depth on the MI355X: exact integer parity with the reference's own search_depth (fixture made by
tests/golden/make_search_depth_golden.py), with a level-by-level search composed from the existing operators, and
the limits.  Every check is exact equality."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import ops
from hironaka_amd.host import AllCoordHost, RandomHost, Zeillinger
from hironaka_amd.util import SearchDepthResult, search_depth, search_depths

pytestmark = pytest.mark.gpu

HOSTS = {"zeillinger": Zeillinger, "all_coord": AllCoordHost}
ROOT_5552 = [[7, 5, 3, 8], [8, 1, 8, 18], [8, 3, 17, 8], [11, 11, 1, 19], [11, 12, 18, 6], [16, 11, 5, 6]]
ROOT_6 = [[0, 1, 0, 1], [0, 2, 0, 0], [1, 0, 0, 1], [1, 0, 1, 0], [1, 1, 0, 0], [2, 0, 0, 0]]


@pytest.fixture(scope="module")
def fixture():
    f = np.load(os.path.join(GOLDEN, "search_depth.npz"))
    return {str(g): (str(f[f"{g}_host"]), f[f"{g}_roots"], f[f"{g}_depth"], f[f"{g}_nodes"]) for g in f["groups"]}


def _run(roots, host, dtype=torch.float32, **kw):
    r = search_depths(torch.as_tensor(roots, dtype=dtype, device="cuda"), HOSTS[host](), **kw)
    return r.depth.cpu().numpy(), r.nodes.cpu().numpy(), r.status.cpu().numpy()


def test_search_depth_small():
    assert search_depth(ROOT_6, Zeillinger()) == 6                 # test/testSearch.py:27-33
    r = search_depths([ROOT_6], Zeillinger())
    assert isinstance(r, SearchDepthResult) and r.nodes.tolist() == [14] and r.status.tolist() == [0]


def test_search_depth_5552():
    """test/testSearch.py:13-24, disabled in the reference (35.7 s there)"""
    assert search_depth(torch.tensor(ROOT_5552, dtype=torch.float32, device="cuda"), Zeillinger()) == 5552
    r = search_depths([ROOT_5552], Zeillinger())
    assert r.depth.tolist() == [5552] and r.nodes.tolist() == [564448] and r.status.tolist() == [0]


def test_search_depth_accepts_hip_points():
    from hironaka_amd.core import HipPoints
    p = HipPoints([ROOT_6], max_num_points=8, semantics="list")
    assert search_depth(p, Zeillinger()) == 6


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fixture_parity_batched(fixture, dtype):
    for g, (host, roots, depth, nodes) in fixture.items():
        d, n, s = _run(roots, host, dtype)
        assert (s == 0).all(), (g, np.nonzero(s)[0])
        assert np.array_equal(d, depth), g
        assert np.array_equal(n, nodes), g


def test_fixture_parity_one_root_per_call(fixture):
    for g, (host, roots, depth, nodes) in fixture.items():
        for i in range(len(roots)):
            if nodes[i] > 100000:
                continue  # the 5552 tree has a test of its own
            d, n, s = _run(roots[i:i + 1], host)
            assert (d[0], n[0], s[0]) == (depth[i], nodes[i], 0), (g, i)


def test_fixture_parity_padded_and_permuted(fixture):
    rng = np.random.default_rng(7)
    for g, (host, roots, depth, nodes) in fixture.items():
        b, m, dim = roots.shape
        M = m + 5
        tail = np.full((b, M, dim), -1.0)
        tail[:, :m] = roots
        mixed = np.full((b, M, dim), -1.0)
        for i in range(b):  # padding rows interleaved between the points, row order of the points kept
            slots = np.sort(rng.choice(M, m, replace=False))
            mixed[i, slots] = roots[i]
            if rng.random() < 0.5:  # a padding row with other negative entries, not only -1
                free = [j for j in range(M) if j not in set(slots.tolist())]
                mixed[i, free[0]] = -rng.integers(1, 5, dim)
        perm = rng.permutation(b)
        for arr, want_d, want_n in ((tail, depth, nodes), (mixed, depth, nodes), (mixed[perm], depth[perm],
                                                                                   nodes[perm])):
            d, n, s = _run(arr, host)
            assert (s == 0).all() and np.array_equal(d, want_d) and np.array_equal(n, want_n), g


# ---- a level-by-level search composed from the existing operators -------------------------------------------------

def _composed(roots: torch.Tensor, host: str, cap: int):
    """BFS over whole levels with ops.zeillinger(list) / decode_host_class / step(list, compact-sorted, shift+Newton)
    / get_num_points.  Nodes at depth `cap` are visited, not expanded.  Returns depth, nodes, status (DEPTH_LIMIT,
    INEXACT as the kernel defines them, over the whole truncated tree) per root."""
    b, m, d = roots.shape
    dev = roots.device
    limit = 2.0 ** 24 if roots.dtype == torch.float32 else 2.0 ** 53
    depth = torch.zeros(b, dtype=torch.int64, device=dev)
    nodes = torch.zeros(b, dtype=torch.int64, device=dev)
    status = torch.zeros(b, dtype=torch.int32, device=dev)
    states, owner = roots, torch.arange(b, device=dev)
    flags = A.HK_SEM_LIST | A.HK_FLAG_COMPACT_SORTED
    for level in range(cap + 1):
        if states.shape[0] == 0:
            break
        nodes += torch.bincount(owner, minlength=b)
        depth[owner] = level + 1
        if level == cap:
            status[owner] |= A.HK_SEARCH_DEPTH_LIMIT
            break
        if host == "zeillinger":
            cls = ops.zeillinger(states, sem="list")
            mask = ops.decode_host_class(cls.clamp(min=0), d, torch.int32)
        else:
            mask = torch.ones((states.shape[0], d), dtype=torch.int32, device=dev)
        nxt, nown = [], []
        for a in range(d):  # per axis: the kernel's child order does not matter to depth and nodes
            sel = torch.nonzero(mask[:, a]).squeeze(1)
            if sel.numel() == 0:
                continue
            ax = torch.full((sel.numel(),), a, dtype=torch.int32, device=dev)
            shifted = ops.step(states[sel], mask[sel], ax, stages=A.HK_STAGE_SHIFT, flags=flags)["points"]
            big = ((shifted[:, :, a] >= limit) & (shifted[:, :, 0] >= 0)).any(1)
            status[owner[sel][big]] |= A.HK_SEARCH_INEXACT
            child = ops.step(states[sel], mask[sel], ax, stages=A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON,
                             flags=flags)["points"]
            keep = ops.get_num_points(child) >= 2
            nxt.append(child[keep])
            nown.append(owner[sel][keep])
        states = torch.cat(nxt) if nxt else states[:0]
        owner = torch.cat(nown) if nown else owner[:0]
    return depth.cpu().numpy(), nodes.cpu().numpy(), status.cpu().numpy()


def _random_roots(seed, b, m, d, max_value=20, dtype=torch.float32):
    rng = np.random.default_rng(seed)
    roots = rng.integers(0, max_value + 1, (b, m, d)).astype(np.float64)
    count = rng.integers(2, m + 1, b)
    for i in range(b):
        roots[i, count[i]:] = -1.0
    return torch.as_tensor(roots, dtype=dtype, device="cuda")


@pytest.mark.parametrize("host,b,m,d,cap", [("zeillinger", 512, 10, 4, 48), ("zeillinger", 512, 20, 3, 48),
                                            ("all_coord", 256, 6, 3, 8)])
def test_matches_composed_search(host, b, m, d, cap):
    roots = _random_roots(1000 * m + d, b, m, d)
    want_d, want_n, want_s = _composed(roots, host, cap)
    r = search_depths(roots, HOSTS[host](), max_depth=cap, max_nodes=1 << 30)
    got_d, got_n, got_s = r.depth.cpu().numpy(), r.nodes.cpu().numpy(), r.status.cpu().numpy()
    exact = (want_s & A.HK_SEARCH_INEXACT) == 0
    assert exact.mean() > 0.9
    assert np.array_equal(got_s[~exact] & A.HK_SEARCH_INEXACT, want_s[~exact] & A.HK_SEARCH_INEXACT)
    assert np.array_equal(got_s[exact], want_s[exact])
    assert np.array_equal(got_d[exact], want_d[exact])
    assert np.array_equal(got_n[exact], want_n[exact])
    assert (want_s & A.HK_SEARCH_DEPTH_LIMIT).any()


# ---- limits -------------------------------------------------------------------------------------------------------

def test_node_limit():
    r = search_depths([ROOT_5552], Zeillinger(), max_nodes=1000)
    assert r.status.tolist() == [A.HK_SEARCH_NODE_LIMIT]
    assert int(r.nodes[0]) >= 1000 and 1 <= int(r.depth[0]) <= 5552
    again = search_depths([ROOT_5552], Zeillinger(), max_nodes=1000)
    for x, y in zip(r, again):
        assert torch.equal(x, y)
    # exactly the tree's size is no limit
    r = search_depths([ROOT_6], Zeillinger(), max_nodes=14)
    assert (r.depth.tolist(), r.nodes.tolist(), r.status.tolist()) == ([6], [14], [0])


def test_stack_limit():
    r = search_depths([ROOT_6], Zeillinger(), stack_nodes=1)
    assert r.status.tolist() == [A.HK_SEARCH_STACK_LIMIT] and int(r.nodes[0]) <= 14


def test_depth_limit():
    r = search_depths([ROOT_6], Zeillinger(), max_depth=0)
    assert (r.depth.tolist(), r.nodes.tolist(), r.status.tolist()) == ([1], [1], [A.HK_SEARCH_DEPTH_LIMIT])
    r = search_depths([ROOT_6], Zeillinger(), max_depth=5)  # the deepest node sits at depth 5: visited, no children
    assert (r.depth.tolist(), r.nodes.tolist(), r.status.tolist()) == ([6], [14], [A.HK_SEARCH_DEPTH_LIMIT])


BIG = [[9000000, 8000000], [8000000, 9000000], [5000000, 9500000]]


def test_inexact_in_float32_exact_in_float64():
    r32 = search_depths([BIG], Zeillinger(), dtype=torch.float32)
    assert int(r32.status[0]) & A.HK_SEARCH_INEXACT
    r64 = search_depths([BIG], Zeillinger(), dtype=torch.float64)
    assert r64.status.tolist() == [0]
    d, n, s = _composed(torch.tensor([BIG], dtype=torch.float64, device="cuda"), "zeillinger", 64)
    assert (r64.depth.tolist(), r64.nodes.tolist(), s.tolist()) == (d.tolist(), n.tolist(), [0])
    assert search_depth(torch.tensor(BIG, dtype=torch.float64, device="cuda"), Zeillinger()) == d[0]


def test_root_ended_and_empty_batch():
    r = search_depths([[[3, 4, 5], [-1, -1, -1]], [[1, 2, 3], [3, 2, 1]]], Zeillinger())
    assert r.status.tolist() == [A.HK_SEARCH_ROOT_ENDED, 0] and r.depth[0] == 0 and r.nodes[0] == 0
    with pytest.raises(ValueError, match="fewer than 2 points"):
        search_depth([[3, 4, 5]], Zeillinger())
    d, n, s = ops.search_depth(torch.zeros((0, 6, 4), device="cuda"), "zeillinger", max_depth=8, max_nodes=8,
                               stack_nodes=8)
    assert d.shape == n.shape == s.shape == (0,)


def test_search_depth_raises_on_every_limit():
    with pytest.raises(RuntimeError, match="max_depth"):
        search_depth(ROOT_6, Zeillinger(), max_depth=2)
    with pytest.raises(RuntimeError, match="max_nodes"):
        search_depth(ROOT_6, Zeillinger(), max_nodes=3)
    with pytest.raises(RuntimeError, match="stack_nodes"):
        search_depth(ROOT_6, Zeillinger(), stack_nodes=1)
    with pytest.raises(RuntimeError, match="exact integer range"):
        search_depth(BIG, Zeillinger())


def test_bad_roots_and_hosts_are_refused():
    for bad in ([[0.5, 1, 2], [1, 2, 3]], [[float("nan"), 1, 2], [1, 2, 3]], [[2.0 ** 24, 1, 2], [1, 2, 3]],
                [[1, -2, 2], [1, 2, 3]]):
        with pytest.raises(ValueError):
            search_depth(bad, Zeillinger())
    with pytest.raises(TypeError, match="Zeillinger"):
        search_depth(ROOT_6, RandomHost(seed=0))
    with pytest.raises(ValueError):
        search_depth([ROOT_6, ROOT_6], Zeillinger())
