"""CPU-side checks of hk_search_depth / hironaka_amd.util.search_depth: the fixture made by running the reference's own
search_depth (tests/golden/make_search_depth_golden.py) holds the reference's known answers, and bad arguments are
refused on the host before any launch."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import _lib


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "search_depth.npz"))


def test_fixture_holds_the_reference_literals(fixture):
    # test/testSearch.py:13-24 (the disabled `== 5552`), :27-33 (`== 6`), :35-40 (no assert)
    assert fixture["lit4_roots"][0].tolist() == [[7, 5, 3, 8], [8, 1, 8, 18], [8, 3, 17, 8], [11, 11, 1, 19],
                                                 [11, 12, 18, 6], [16, 11, 5, 6]]
    assert fixture["lit4_depth"].tolist() == [5552, 6]
    assert fixture["lit4_nodes"].tolist() == [564448, 14]
    assert fixture["lit3_depth"].tolist() == [8] and fixture["lit3_nodes"].tolist() == [26]


def test_fixture_groups_are_consistent(fixture):
    hosts = set()
    for g in fixture["groups"]:
        roots, depth, nodes = fixture[f"{g}_roots"], fixture[f"{g}_depth"], fixture[f"{g}_nodes"]
        hosts.add(str(fixture[f"{g}_host"]))
        assert roots.ndim == 3 and len(roots) == len(depth) == len(nodes) > 0, g
        avail = roots[:, :, 0] >= 0
        assert (avail.sum(1) >= 2).all(), g
        assert (roots[avail] == np.floor(roots[avail])).all() and (roots[avail] >= 0).all(), g
        assert (roots[~avail] == -1).all(), g
        assert (depth >= 1).all() and (nodes >= depth).all(), g
    assert hosts == {"zeillinger", "all_coord"}
    assert len(fixture["z3_depth"]) + len(fixture["z4_depth"]) >= 200 and len(fixture["a2_depth"]) >= 40


def _call(L, points=1, batch=4, m=6, d=4, dtype=A.HK_F32, host=A.HK_HOST_ZEILLINGER, max_depth=8, max_nodes=64,
          stack_nodes=16, workspace=1, workspace_bytes=None, depth=1, nodes=1, status=1):
    buf = (ctypes.c_uint64 * 4096)()
    addr = ctypes.addressof(buf)
    if workspace_bytes is None:
        workspace_bytes = L.hk_search_depth_workspace_bytes(batch, m, d, dtype, stack_nodes)
    ptr = lambda flag: addr if flag else None  # noqa: E731
    return L.hk_search_depth(ptr(points), batch, m, d, dtype, host, max_depth, max_nodes, stack_nodes, ptr(workspace),
                             workspace_bytes, ptr(depth), ptr(nodes), ptr(status), None)


def test_search_depth_argument_validation_without_gpu():
    """every status for bad arguments is decided on the host, before any launch"""
    L = _lib.lib()
    assert L.hk_search_depth_workspace_bytes(4, 6, 4, A.HK_F32, 16) == 4 * 16 * (6 * 4 * 4 + 4)
    assert L.hk_search_depth_workspace_bytes(3, 10, 3, A.HK_F64, 100) == 3 * 100 * (10 * 3 * 8 + 4)
    assert L.hk_search_depth_workspace_bytes(4, 6, 1, A.HK_F32, 16) == 0
    assert L.hk_search_depth_workspace_bytes(4, 6, 4, A.HK_I32, 16) == 0
    assert _call(L, points=0) == A.HK_ERR_NULL
    assert _call(L, depth=0) == A.HK_ERR_NULL
    assert _call(L, nodes=0) == A.HK_ERR_NULL
    assert _call(L, status=0) == A.HK_ERR_NULL
    assert _call(L, workspace=0) == A.HK_ERR_NULL
    assert _call(L, workspace_bytes=4 * 16 * 100 - 1) == A.HK_ERR_SHAPE   # workspace too small
    assert _call(L, d=1, workspace_bytes=1 << 20) == A.HK_ERR_SHAPE
    assert _call(L, m=0, workspace_bytes=1 << 20) == A.HK_ERR_SHAPE
    assert _call(L, batch=-1, workspace_bytes=1 << 20) == A.HK_ERR_SHAPE
    assert _call(L, max_depth=-1) == A.HK_ERR_SHAPE
    assert _call(L, max_nodes=0) == A.HK_ERR_SHAPE
    assert _call(L, stack_nodes=0, workspace_bytes=1 << 20) == A.HK_ERR_SHAPE
    assert _call(L, host=A.HK_HOST_RANDOM) == A.HK_ERR_UNSUPPORTED
    assert _call(L, host=7) == A.HK_ERR_UNSUPPORTED
    assert _call(L, dtype=A.HK_I32, workspace_bytes=1 << 20) == A.HK_ERR_UNSUPPORTED
    assert _call(L, d=7, workspace_bytes=1 << 20) == A.HK_ERR_UNSUPPORTED
    assert _call(L, m=65, workspace_bytes=1 << 20) == A.HK_ERR_UNSUPPORTED
    assert _call(L, batch=0, points=0, workspace=0, depth=0, nodes=0, status=0, workspace_bytes=0) == A.HK_OK


def test_search_depth_hosts_are_checked_without_gpu():
    from hironaka_amd.host import PolicyHost, RandomHost
    from hironaka_amd.util import search
    assert search._host_name(search.Zeillinger()) == "zeillinger"
    assert search._host_name(search.AllCoordHost()) == "all_coord"
    for h in (RandomHost(seed=0), PolicyHost(policy=None), object()):
        with pytest.raises(TypeError, match="Zeillinger and hironaka_amd.host.AllCoordHost"):
            search._host_name(h)
