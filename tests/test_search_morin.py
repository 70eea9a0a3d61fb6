"""CPU-side checks of hk_search_morin_tree / hironaka_amd.util.search_tree_morin: the symbols are exported and bound,
the workspace formula holds, bad arguments are refused on the host before any launch, and the fixture made by running
the reference's own search_tree_morin (tests/golden/make_search_morin_golden.py) is consistent, including against a
plain restatement of the rules for the all-coordinates host."""
import ast
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import _lib

HOST_KEYS = {"zeillinger", "all_coord", "zeillinger_lex", "weak_spivakovsky", "weak_spivakovsky_min_hitting"}


def test_symbols_are_exported_and_bound():
    L = _lib.lib()
    for name in ("hk_search_morin_tree_workspace_bytes", "hk_search_morin_tree"):
        assert name in A.PROTOTYPES
        fn = getattr(L, name)
        assert fn.argtypes == A.PROTOTYPES[name][1]
    assert A.HK_SEARCH_ROOT_INVALID == 32
    assert A.HK_ABI_VERSION == 6 and L.hk_abi_version() == 6
    from hironaka_amd import util
    for name in ("search_tree_morin", "search_trees_morin", "MorinTreeResult"):
        assert name in util.__all__ and hasattr(util, name)


def _ws(batch, m, d, es, max_nodes, stack_nodes):
    # search_tree's words, then child count, sibling rank, kind, distinguished and d weights per record
    return batch * (max_nodes * m * d * es + 4 * (10 * max_nodes + 1 + stack_nodes + (4 + d) * max_nodes))


def test_workspace_formula():
    f = _lib.lib().hk_search_morin_tree_workspace_bytes
    assert f(4, 6, 4, A.HK_F32, 100, 16) == _ws(4, 6, 4, 4, 100, 16)
    assert f(3, 10, 3, A.HK_F64, 1000, 64) == _ws(3, 10, 3, 8, 1000, 64)
    assert f(2, 19, 7, A.HK_F32, 100, 16) == _ws(2, 19, 7, 4, 100, 16) != 0
    assert f(1, 64, 7, A.HK_F64, 1 << 18, 1 << 16) == _ws(1, 64, 7, 8, 1 << 18, 1 << 16)
    assert f(0, 6, 4, A.HK_F32, 100, 16) == 0
    assert f(4, 6, 1, A.HK_F32, 100, 16) == 0
    assert f(4, 6, 8, A.HK_F32, 100, 16) == 0
    assert f(4, 65, 4, A.HK_F32, 100, 16) == 0
    assert f(4, 6, 4, A.HK_I32, 100, 16) == 0
    assert f(4, 6, 4, A.HK_F32, 0, 16) == 0
    assert f(4, 6, 4, A.HK_F32, 100, 0) == 0


N_OUT = 12  # parent .. status; index 9 is states_out


def _call(L, points=1, weights=1, distinguished=1, batch=4, m=6, d=4, dtype=A.HK_F32, host=A.HK_HOST_ZEILLINGER,
          expand_limit=-1, max_depth=8, max_nodes=64, stack_nodes=16, workspace=1, workspace_bytes=None,
          outs=(1,) * N_OUT, offset=0):
    buf = (ctypes.c_uint64 * 8192)()
    addr = ctypes.addressof(buf)
    if workspace_bytes is None:
        workspace_bytes = L.hk_search_morin_tree_workspace_bytes(batch, m, d, dtype, max_nodes, stack_nodes)
    ptr = lambda flag: addr + offset if flag else None  # noqa: E731
    return L.hk_search_morin_tree(ptr(points), ptr(weights), ptr(distinguished), batch, m, d, dtype, host, expand_limit,
                                  max_depth, max_nodes, stack_nodes, ptr(workspace), workspace_bytes,
                                  *[ptr(o) for o in outs], None)


def test_argument_validation_without_gpu():
    """every status for bad arguments is decided on the host, before any launch: none of these calls reaches one (the
    last status a valid call could get without a device is not HK_OK either, so only refusals are asserted)"""
    L = _lib.lib()
    assert _call(L, points=0) == A.HK_ERR_NULL
    assert _call(L, weights=0) == A.HK_ERR_NULL
    assert _call(L, distinguished=0) == A.HK_ERR_NULL
    assert _call(L, workspace=0) == A.HK_ERR_NULL
    for i in range(N_OUT):
        if i == 9:  # states_out may be NULL
            continue
        outs = [1] * N_OUT
        outs[i] = 0
        assert _call(L, outs=outs) == A.HK_ERR_NULL, i
    assert _call(L, d=1, workspace_bytes=1 << 20) == A.HK_ERR_SHAPE
    assert _call(L, d=8, workspace_bytes=1 << 20) == A.HK_ERR_UNSUPPORTED
    assert _call(L, d=7, points=0) == A.HK_ERR_NULL  # dim 7 passes the shape checks
    assert _call(L, d=7, workspace_bytes=_ws(4, 6, 7, 4, 64, 16) - 1) == A.HK_ERR_SHAPE
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
    assert _call(L, dtype=A.HK_F64, offset=4) == A.HK_ERR_ALIGN
    assert _call(L, batch=0, points=0, weights=0, distinguished=0, workspace=0, outs=(0,) * N_OUT,
                 workspace_bytes=0) == A.HK_OK
    # the other fixed-host operators still stop at dim 6
    assert L.hk_search_game_tree_workspace_bytes(4, 6, 7, A.HK_F32, 100, 16) == 0
    assert L.hk_search_depth_workspace_bytes(4, 6, 7, A.HK_F32, 16) == 0


def test_hosts_and_weights_are_checked_without_gpu():
    from hironaka_amd.host import PolicyHost, RandomHost, Zeillinger
    from hironaka_amd.util import search_tree_morin, search_trees_morin
    root = [[1, 2], [2, 1]]
    for h in (RandomHost(seed=0), PolicyHost(policy=None), object()):
        with pytest.raises(TypeError):
            search_tree_morin(root, None, 0, [1, 1], h, distinguished=0)
        with pytest.raises(TypeError):
            search_trees_morin([root], [[1, 1]], [0], h)
    for bad in ([1, 1.5], ["a", 1], [[1, 1]], None, [1, float("nan")]):
        with pytest.raises(ValueError):
            search_tree_morin(root, None, 0, bad, Zeillinger(), distinguished=0)
    with pytest.raises(ValueError):  # no index from anywhere
        search_tree_morin(root, None, 0, [1, 1], Zeillinger())
    with pytest.raises(ValueError):
        search_tree_morin(root, None, 0, np.asarray([1.0, 2.0]), Zeillinger(), distinguished=0.5)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "search_morin.npz"))


def _depth(ident, parent, curr):
    dep = {curr: 0}
    for i, p in zip(ident, parent):
        dep[i] = dep[p] + 1
    return max(dep.values())


def test_fixture_is_consistent(golden):
    cases = [str(c) for c in golden["cases"]]
    index = {c: i for i, c in enumerate(cases)}
    hosts, sizes, dims, deep7 = set(), set(), set(), set()
    total = more_below_ended = 0
    for i, name in enumerate(cases):
        root, weights = golden[f"c{i}_root"], golden[f"c{i}_weights"]
        max_size, n0, curr, dist = (int(v) for v in golden[f"c{i}_meta"])
        ident, parent, data = golden[f"c{i}_ident"].tolist(), golden[f"c{i}_parent"].tolist(), golden[f"c{i}_data"]
        host = str(golden[f"c{i}_host"])
        hosts.add(host)
        sizes.add(max_size)
        dims.add(root.shape[1])
        total += len(ident)
        assert weights.shape == (root.shape[1],) and (weights >= 0).all() and 0 <= dist < len(root), name
        assert ident == list(range(n0, n0 + len(ident))), name
        assert all(p < c and (p == curr or p >= n0) for p, c in zip(parent, ident)), name
        assert len(data) == len(ident), name
        text = {c: str(s) for c, s in zip(ident, data)}
        for c, p in zip(ident, parent):
            if p != curr:  # only contributing nodes have children
                assert text[p] not in ("No contribution", "...more..."), name
            if text[c] == "...more..." and p != curr and len(ast.literal_eval(text[p].rsplit(", [", 1)[0])[0]) <= 1:
                more_below_ended += 1
        if max_size >= 0 and n0 > max_size:
            assert [text[c] for c in ident] == ["...more..."], name
        if root.shape[1] == 7 and ident and _depth(ident, parent, curr) >= 3:
            deep7.add(host)
    assert hosts == deep7 == HOST_KEYS
    assert sizes == {-1, 0, 1, 7, 100, 10000}
    assert dims == {2, 3, 4, 5, 6, 7}
    assert total <= 40000
    assert any(int(golden[f"c{i}_meta"][1]) > 1 and int(golden[f"c{i}_meta"][2]) != 0 for i in range(len(cases)))
    # test/testThom.py:94-114: 37 nodes with the caller's root
    assert len(golden[f"c{index['thom_original']}_ident"]) == 36
    assert golden[f"c{index['thom4_weak_spivakovsky_full']}_root"].shape == (19, 7)
    # the generator's coverage: identical-row losses, strictly-smaller losses, pruned actions, "...more..." below an
    # ended node
    assert (golden["stats"] >= 1).all() and more_below_ended >= 1 and more_below_ended == int(golden["stats"][3])
    assert len(golden["thom4_ref_seconds"]) == len(golden["thom4_hosts"]) == 4


def _walk(rows, dist, weights, max_size, nodes, curr, stats):
    """The issue's rules restated for the all-coordinates host, whose list is every axis in ascending order.  nodes:
    the (identifier, parent, data) list that stands for the tree."""
    d = len(rows[0])
    coords = list(range(d))

    def create(parent, data):
        nodes.append((len(nodes), parent, data))
        return len(nodes) - 1

    def rec(state, dist, w, node):
        if len(state) <= 1 or len(nodes) > max_size:
            if len(nodes) > max_size:
                create(node, "...more...")
            return
        for a in coords:
            if w[a] > min(w):
                stats["pruned"] += 1
                continue
            w2 = [w[i] if i == a else w[i] - w[a] for i in coords]
            new = [[sum(x) if i == a else x[i] for i in coords] for x in state]
            low = [min(x[i] for x in new) for i in coords]
            new = [[x[i] - low[i] for i in coords] for x in new]
            p = new[dist]
            below = [x for j, x in enumerate(new) if j != dist and all(x[k] <= p[k] for k in coords)]
            if below:
                stats["identical" if p in below else "smaller"] += 1
                create(node, "No contribution")
                continue
            kept = sorted((x for x in new if not any(y != x and all(y[k] <= x[k] for k in coords) for y in new)),
                          reverse=True)
            kept = [x for j, x in enumerate(kept) if x not in kept[:j]]
            nd = kept.index(p)
            rec(kept, nd, w2, create(node, str([kept]) + f", {[nd]}"))

    rec([list(r) for r in rows], dist, list(weights), curr)


def test_restated_rules_reproduce_the_all_coord_cases(golden):
    stats = {"pruned": 0, "identical": 0, "smaller": 0}
    seen = 0
    for i, name in enumerate(golden["cases"]):
        if str(golden[f"c{i}_host"]) != "all_coord":
            continue
        max_size, n0, curr, dist = (int(v) for v in golden[f"c{i}_meta"])
        nodes = [(j, j - 1 if j else None, None) for j in range(n0)]
        _walk(golden[f"c{i}_root"].tolist(), dist, golden[f"c{i}_weights"].tolist(), 10 ** 9 if max_size < 0 else max_size,
              nodes, curr, stats)
        new = nodes[n0:]
        assert [c[0] for c in new] == golden[f"c{i}_ident"].tolist(), name
        assert [c[1] for c in new] == golden[f"c{i}_parent"].tolist(), name
        assert [c[2] for c in new] == [str(s) for s in golden[f"c{i}_data"]], name
        seen += 1
    assert seen >= 40 and stats["pruned"] and stats["identical"] and stats["smaller"]
