"""CPU-side checks of hk_search_game_tree / hironaka_amd.util.search_tree: the symbols are exported and bound, the
workspace formula holds, bad arguments are refused on the host before any launch, and the fixture made by running the
reference's own search_tree (tests/golden/make_search_tree_golden.py) is consistent."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import _lib


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    for name in ("hk_search_game_tree_workspace_bytes", "hk_search_game_tree"):
        assert name in A.PROTOTYPES
        fn = getattr(L, name)
        assert fn.argtypes == A.PROTOTYPES[name][1]
    assert A.HK_ABI_VERSION == 6 and L.hk_abi_version() == 6


def _ws(batch, m, d, es, max_nodes, stack_nodes):
    return batch * (max_nodes * m * d * es + 4 * (10 * max_nodes + 1 + stack_nodes))


def test_workspace_formula():
    L = _lib.lib()
    f = L.hk_search_game_tree_workspace_bytes
    assert f(4, 6, 4, A.HK_F32, 100, 16) == _ws(4, 6, 4, 4, 100, 16)
    assert f(3, 10, 3, A.HK_F64, 1000, 64) == _ws(3, 10, 3, 8, 1000, 64)
    assert f(1, 64, 6, A.HK_F64, 1 << 21, 1 << 16) == _ws(1, 64, 6, 8, 1 << 21, 1 << 16)
    assert f(0, 6, 4, A.HK_F32, 100, 16) == 0
    assert f(4, 6, 1, A.HK_F32, 100, 16) == 0
    assert f(4, 6, 7, A.HK_F32, 100, 16) == 0
    assert f(4, 65, 4, A.HK_F32, 100, 16) == 0
    assert f(4, 6, 4, A.HK_I32, 100, 16) == 0
    assert f(4, 6, 4, A.HK_F32, 0, 16) == 0
    assert f(4, 6, 4, A.HK_F32, 100, 0) == 0


def _call(L, points=1, batch=4, m=6, d=4, dtype=A.HK_F32, host=A.HK_HOST_ZEILLINGER, expand_limit=-1, max_depth=8,
          max_nodes=64, stack_nodes=16, workspace=1, workspace_bytes=None, outs=(1,) * 9, offset=0):
    buf = (ctypes.c_uint64 * 4096)()
    addr = ctypes.addressof(buf)
    if workspace_bytes is None:
        workspace_bytes = L.hk_search_game_tree_workspace_bytes(batch, m, d, dtype, max_nodes, stack_nodes)
    ptr = lambda flag: addr + offset if flag else None  # noqa: E731
    return L.hk_search_game_tree(ptr(points), batch, m, d, dtype, host, expand_limit, max_depth, max_nodes,
                                 stack_nodes, ptr(workspace), workspace_bytes, *[ptr(o) for o in outs], None)


def test_argument_validation_without_gpu():
    """every status for bad arguments is decided on the host, before any launch"""
    L = _lib.lib()
    assert _call(L, points=0) == A.HK_ERR_NULL
    assert _call(L, workspace=0) == A.HK_ERR_NULL
    for i in range(9):
        if i == 6:  # states_out may be NULL
            continue
        outs = [1] * 9
        outs[i] = 0
        assert _call(L, outs=outs) == A.HK_ERR_NULL, i
    assert _call(L, d=1, workspace_bytes=1 << 20) == A.HK_ERR_SHAPE
    assert _call(L, d=7, workspace_bytes=1 << 20) == A.HK_ERR_UNSUPPORTED
    assert _call(L, m=65, workspace_bytes=1 << 20) == A.HK_ERR_UNSUPPORTED
    assert _call(L, m=0, workspace_bytes=1 << 20) == A.HK_ERR_SHAPE
    assert _call(L, dtype=A.HK_I32, workspace_bytes=1 << 20) == A.HK_ERR_UNSUPPORTED
    assert _call(L, host=0) == A.HK_ERR_UNSUPPORTED
    assert _call(L, host=6) == A.HK_ERR_UNSUPPORTED
    assert _call(L, max_nodes=0, workspace_bytes=1 << 20) == A.HK_ERR_SHAPE
    assert _call(L, stack_nodes=0, workspace_bytes=1 << 20) == A.HK_ERR_SHAPE
    assert _call(L, max_depth=-1) == A.HK_ERR_SHAPE
    assert _call(L, batch=-1, workspace_bytes=1 << 20) == A.HK_ERR_SHAPE
    assert _call(L, workspace_bytes=_ws(4, 6, 4, 4, 64, 16) - 1) == A.HK_ERR_SHAPE  # workspace too small
    assert _call(L, offset=2) == A.HK_ERR_ALIGN
    assert _call(L, batch=0, points=0, workspace=0, outs=(0,) * 9, workspace_bytes=0) == A.HK_OK


def test_hosts_are_checked_without_gpu():
    from hironaka_amd.host import PolicyHost, RandomHost
    from hironaka_amd.util import search, search_tree
    for h in (RandomHost(seed=0), PolicyHost(policy=None), object()):
        with pytest.raises(TypeError):
            search_tree([[1, 2], [2, 1]], None, 0, h)
    assert search.TreeNodeData([[[1, 2], [3, 4]]]).__repr__() == "[[[1, 2], [3, 4]]]"
    assert search.TreeNodeData([[[1, 2]]]).ended and not search.TreeNodeData([[[1, 2], [3, 4]]]).ended


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "search_tree.npz"))


def test_fixture_is_consistent(golden):
    cases = [str(c) for c in golden["cases"]]
    lit = {c: i for i, c in enumerate(cases)}
    # test/testSearch.py:42-50: 107 nodes at max_size=100 (the root made by the caller + 106), 1 583 in full
    assert len(golden[f"c{lit['literal_100']}_ident"]) == 106
    assert len(golden[f"c{lit['literal_full']}_ident"]) == 1582
    assert len(golden["lit_str"]) == 106
    hosts, sizes = set(), set()
    for i, name in enumerate(cases):
        root = golden[f"c{i}_root"]
        max_size, n0, curr = (int(v) for v in golden[f"c{i}_meta"])
        ident, parent, states = golden[f"c{i}_ident"], golden[f"c{i}_parent"], golden[f"c{i}_states"]
        hosts.add(str(golden[f"c{i}_host"]))
        sizes.add(max_size)
        n = len(ident)
        assert ident.tolist() == list(range(n0, n0 + n)), name
        assert (parent < ident).all() and (parent >= 0).all(), name
        assert all(p == curr or p >= n0 for p in parent), name
        assert states.shape == (n,) + root.shape, name
        if max_size >= 0:
            assert (n == 0) == (n0 > max_size or (root[:, 0] >= 0).sum() < 2), name
    assert hosts == {"zeillinger", "all_coord", "zeillinger_lex", "weak_spivakovsky", "weak_spivakovsky_min_hitting"}
    assert sizes == {-1, 0, 1, 7, 100}
    assert any(int(golden[f"c{i}_meta"][1]) > 1 and int(golden[f"c{i}_meta"][2]) != 0 for i in range(len(cases)))
    assert {golden[f"c{i}_root"].shape[1] for i in range(len(cases))} == {2, 3, 4, 5}
