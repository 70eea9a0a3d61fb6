"""hk_search_depth with ZeillingerLex, WeakSpivakovsky and WeakSpivakovskyMinHitting: exact parity with the
reference's own search_depth (tests/golden/hosts.npz, tests/golden/make_host_golden.py), and a depth-capped
comparison with a level-by-level search composed from ops.host_select and the list-semantics step operators."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import ops
from hironaka_amd.host import WeakSpivakovsky, WeakSpivakovskyMinHitting, ZeillingerLex
from hironaka_amd.util import search_depth, search_depths

pytestmark = pytest.mark.gpu

HOSTS = {"zeillinger_lex": ZeillingerLex, "weak_spivakovsky": WeakSpivakovsky,
         "weak_spivakovsky_min_hitting": WeakSpivakovskyMinHitting}


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "hosts.npz"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("host", list(HOSTS))
def test_fixture_parity(fixture, host, dtype):
    for d in (3, 4):
        g = f"depth_{host}{d}"
        roots, depth, nodes = fixture[f"{g}_roots"], fixture[f"{g}_depth"], fixture[f"{g}_nodes"]
        if len(roots) == 0:
            continue
        r = search_depths(torch.as_tensor(roots, dtype=dtype, device="cuda"), HOSTS[host]())
        assert (r.status.cpu().numpy() == 0).all(), g
        assert np.array_equal(r.depth.cpu().numpy(), depth), g
        assert np.array_equal(r.nodes.cpu().numpy(), nodes), g
    # one root through the reference's signature
    roots, depth = fixture[f"depth_{host}3_roots"], fixture[f"depth_{host}3_depth"]
    live = roots[0][roots[0][:, 0] >= 0]
    assert search_depth(live.tolist(), HOSTS[host]()) == depth[0]


def _composed(roots: torch.Tensor, host: str, cap: int, max_nodes: int):
    """BFS over whole levels with ops.host_select / decode_host_class / ops.shift(list) /
    ops.get_newton_polytope(list, compact_sorted); nodes at depth `cap` are visited, not expanded.  Returns depth,
    nodes and whether some node sat at depth `cap`, per root; `max_nodes` only guards the test's memory."""
    b, m, d = roots.shape
    dev = roots.device
    depth = torch.zeros(b, dtype=torch.int64, device=dev)
    nodes = torch.zeros(b, dtype=torch.int64, device=dev)
    capped = torch.zeros(b, dtype=torch.bool, device=dev)
    states, owner = roots, torch.arange(b, device=dev)
    for level in range(cap + 1):
        if states.shape[0] == 0:
            break
        assert states.shape[0] <= max_nodes
        nodes += torch.bincount(owner, minlength=b)
        depth[owner] = level + 1
        if level == cap:
            capped[owner] = True
            break
        cls = ops.host_select(states, host)
        mask = ops.decode_host_class(cls.clamp(min=0), d, torch.int32) * (cls >= 0).unsqueeze(1).to(torch.int32)
        nxt, nown = [], []
        for a in range(d):
            sel = torch.nonzero(mask[:, a]).squeeze(1)
            if sel.numel() == 0:
                continue
            ax = torch.full((sel.numel(),), a, dtype=torch.int32, device=dev)
            child = ops.shift(states[sel], mask[sel], ax, sem="list")
            child = ops.get_newton_polytope(child, sem="list", compact_sorted=True)
            keep = ops.get_num_points(child) >= 2
            nxt.append(child[keep])
            nown.append(owner[sel][keep])
        states = torch.cat(nxt) if nxt else states[:0]
        owner = torch.cat(nown) if nown else owner[:0]
    return depth.cpu().numpy(), nodes.cpu().numpy(), capped.cpu().numpy()


@pytest.mark.parametrize("host,cap", [("zeillinger_lex", 6), ("weak_spivakovsky", 5),
                                      ("weak_spivakovsky_min_hitting", 4)])
def test_depth_capped_matches_composed_search(host, cap):
    rng = np.random.default_rng(cap)
    b, m, d = 64, 8, 4
    roots = rng.integers(0, 21, (b, m, d)).astype(np.float32)
    count = rng.integers(3, m + 1, b)
    for i in range(b):
        roots[i, count[i]:] = -1.0
    roots = torch.as_tensor(roots, device="cuda")
    want_d, want_n, want_cap = _composed(roots, host, cap, 1 << 22)
    r = search_depths(roots, HOSTS[host](), max_depth=cap, max_nodes=1 << 30)
    got_s = r.status.cpu().numpy()
    assert np.array_equal(got_s, np.where(want_cap, A.HK_SEARCH_DEPTH_LIMIT, 0))
    assert np.array_equal(r.depth.cpu().numpy(), want_d)
    assert np.array_equal(r.nodes.cpu().numpy(), want_n)
    if host != "zeillinger_lex":
        assert want_cap.mean() > 0.5  # the weak hosts: most of these trees do not end within the cap


@pytest.mark.parametrize("host", list(HOSTS))
def test_node_limit_on_the_weak_hosts(host):
    root = [[3, 5, 8, 1], [5, 2, 6, 0], [1, 3, 6, 2], [7, 3, 3, 9]]
    r = search_depths([root], HOSTS[host](), max_nodes=2000)
    assert r.status.tolist()[0] in (0, A.HK_SEARCH_NODE_LIMIT)
    if r.status.tolist()[0]:
        assert int(r.nodes[0]) >= 2000
        with pytest.raises(RuntimeError, match="max_nodes"):
            search_depth([root], HOSTS[host](), max_nodes=2000)


def test_a_root_without_a_subset_is_a_leaf():
    """a zero row (not Newton-reduced): the hitting-set hosts return no subset, so the root has no children"""
    root = [[0, 0, 0], [1, 2, 3], [4, 0, 1]]
    for host in ("weak_spivakovsky", "weak_spivakovsky_min_hitting"):
        r = search_depths([root], HOSTS[host]())
        assert (r.depth.tolist(), r.nodes.tolist(), r.status.tolist()) == ([1], [1], [0]), host
