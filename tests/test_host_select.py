"""CPU-side checks of hk_host_select and the hosts it serves (ZeillingerLex, WeakSpivakovsky,
WeakSpivakovskyMinHitting): the header's constants, argument validation before any launch, a numpy restatement of the
three selection rules against the fixture made by running the reference's own classes
(tests/golden/make_host_golden.py), and search_depth's host mapping."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import _lib
from hironaka_amd import host as H
from hironaka_amd.util import search as S
from search_rules import rule_min_hitting, rule_weak, rule_zeillinger

HOSTS = ("zeillinger_lex", "weak_spivakovsky", "weak_spivakovsky_min_hitting", "zeillinger")
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "hironaka_hip.h")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "hosts.npz"))


def test_constants_match_the_header():
    text = open(HEADER).read()
    for name in ("HK_HOST_ZEILLINGER_LEX", "HK_HOST_WEAK_SPIVAKOVSKY", "HK_HOST_MIN_HITTING", "HK_ABI_VERSION"):
        got = re.search(rf"#define {name} (\d+)", text)
        assert got and int(got.group(1)) == getattr(A, name), name
    assert (A.HK_HOST_ZEILLINGER_LEX, A.HK_HOST_WEAK_SPIVAKOVSKY, A.HK_HOST_MIN_HITTING) == (3, 4, 5)
    assert A.HK_ABI_VERSION == 6 and _lib.lib().hk_abi_version() == 6
    assert '#include "hironaka_hip_hosts.h"' in text


def test_hosts_header_entry_points_are_bound():
    """include/hironaka_hip_hosts.h declares exactly DEVICE_PROTOTYPES (the entry points without an oracle twin), the
    library exports them, and PROTOTYPES (what the oracle restates) stays apart"""
    text = open(os.path.join(INCLUDE, "hironaka_hip_hosts.h")).read()
    declared = set(re.findall(r"^(?:int|uint64_t)\s+(hk_\w+)\(", text, flags=re.M))
    assert declared == set(A.DEVICE_PROTOTYPES) == {"hk_host_select"}
    assert not declared & set(A.PROTOTYPES)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name


def _call(L, points=1, stride=None, out=1, batch=4, m=6, d=3, dtype=A.HK_F32, host=A.HK_HOST_ZEILLINGER_LEX,
          offset=0):
    buf = (ctypes.c_uint64 * 512)()
    addr = ctypes.addressof(buf)
    ptr = lambda flag: addr + offset if flag else None  # noqa: E731
    return L.hk_host_select(ptr(points), m * d if stride is None else stride, ptr(out), batch, m, d, dtype, host, None)


def test_host_select_argument_validation_without_gpu():
    """every status for bad arguments is decided on the host, before any launch"""
    L = _lib.lib()
    assert _call(L, points=0) == A.HK_ERR_NULL
    assert _call(L, out=0) == A.HK_ERR_NULL
    assert _call(L, stride=17) == A.HK_ERR_SHAPE
    assert _call(L, batch=0, points=0, out=0) == A.HK_OK
    assert _call(L, batch=-1) == A.HK_ERR_SHAPE
    assert _call(L, m=0) == A.HK_ERR_SHAPE
    assert _call(L, d=1) == A.HK_ERR_SHAPE
    assert _call(L, d=7) == A.HK_ERR_UNSUPPORTED
    assert _call(L, m=65) == A.HK_ERR_UNSUPPORTED
    for dt in (A.HK_I32, A.HK_I64, A.HK_U8, 7):  # f16 has no dtype code: anything but f32 / f64
        assert _call(L, dtype=dt) == A.HK_ERR_UNSUPPORTED
    for h in (A.HK_HOST_RANDOM, 6, 7, -1):
        assert _call(L, host=h) == A.HK_ERR_UNSUPPORTED
    assert _call(L, offset=2) == A.HK_ERR_ALIGN
    assert _call(L, offset=4, dtype=A.HK_F64) == A.HK_ERR_ALIGN


def test_search_depth_accepts_the_new_host_codes_only():
    L = _lib.lib()
    buf = (ctypes.c_uint64 * 4096)()
    a = ctypes.addressof(buf)
    ws = L.hk_search_depth_workspace_bytes(1, 4, 3, A.HK_F32, 4)
    for h, want in ((A.HK_HOST_RANDOM, A.HK_ERR_UNSUPPORTED), (6, A.HK_ERR_UNSUPPORTED), (7, A.HK_ERR_UNSUPPORTED)):
        assert L.hk_search_depth(a, 1, 4, 3, A.HK_F32, h, 4, 8, 4, a, ws, a, a, a, None) == want, h
    for h in (A.HK_HOST_ZEILLINGER_LEX, A.HK_HOST_WEAK_SPIVAKOVSKY, A.HK_HOST_MIN_HITTING):
        # accepted: the next check that fails is the null workspace
        assert L.hk_search_depth(a, 1, 4, 3, A.HK_F32, h, 4, 8, 4, None, ws, a, a, a, None) == A.HK_ERR_NULL, h
        assert L.hk_search_depth(a, 1, 4, 7, A.HK_F32, h, 4, 8, 4, a, ws, a, a, a, None) == A.HK_ERR_UNSUPPORTED, h


# ---- the selection rules, restated in numpy (tests/search_rules.py: row order, holes anywhere) --------------------

def rule(host, state, d):
    if host == "zeillinger_lex":
        return rule_zeillinger(state, True)
    if host == "zeillinger":
        return rule_zeillinger(state, False)
    if host == "weak_spivakovsky":
        return rule_weak(state)
    return rule_min_hitting(state, d)


def test_fixture_covers_the_issue(fixture):
    for d in range(2, 7):
        st = fixture[f"sel{d}_states"]
        assert st.shape[1:] == (20, d) and len(st) >= 160
        red = fixture[f"sel{d}_reduced"]
        assert red.any() and (~red).any()
        assert (st[..., 0] >= 0).sum(1).min() >= 2
    assert fixture["sel3_states"][0, :2].tolist() == [[0, 1, 2], [2, 1, 0]]
    # test/testGame.py:45-52: Zeillinger picks [0, 2]; WeakSpivakovsky returns a subset of >= 2 coordinates
    assert fixture["sel3_zeillinger"][0].tolist() == [1, 0, 1]
    assert fixture["sel3_weak_spivakovsky"][0].sum() >= 2


@pytest.mark.parametrize("host", HOSTS)
def test_numpy_rules_reproduce_the_reference(fixture, host):
    for d in range(2, 7):
        states, masks = fixture[f"sel{d}_states"], fixture[f"sel{d}_{host}"]
        for g, (st, mk) in enumerate(zip(states, masks)):
            got = rule(host, st, d)
            want = None if mk[0] < 0 else set(np.nonzero(mk)[0].tolist())
            assert got == want, (d, g, st[st[:, 0] >= 0].tolist(), got, want)


def test_numpy_rules_on_the_no_subset_cases():
    z = np.array([[0, 0, 0], [1, 2, 0], [-1, -1, -1]], float)
    assert rule_weak(z) is None and rule_min_hitting(z, 3) is None  # a zero row: nothing meets its empty support
    one_axis = np.array([[2, 0, 0], [5, 0, 0]], float)
    assert rule_weak(one_axis) is None  # |U| = 1
    assert rule_min_hitting(one_axis, 3) == {0, 1}  # the reference's subset_route is defined there
    single = np.array([[1, 2, 3], [-1, -1, -1]], float)
    assert all(rule(h, single, 3) is None for h in HOSTS)


def test_depth_groups_are_consistent(fixture):
    for host in ("zeillinger_lex", "weak_spivakovsky", "weak_spivakovsky_min_hitting"):
        for d in (3, 4):
            g = f"depth_{host}{d}"
            roots, depth, nodes = fixture[f"{g}_roots"], fixture[f"{g}_depth"], fixture[f"{g}_nodes"]
            assert len(roots) == len(depth) == len(nodes) <= int(fixture[f"{g}_tried"]), g
            assert (depth >= 1).all() and (nodes >= depth).all(), g
    assert len(fixture["depth_zeillinger_lex3_depth"]) >= 40


def test_search_depth_maps_the_new_hosts():
    assert S._host_name(H.ZeillingerLex()) == "zeillinger_lex"
    assert S._host_name(H.WeakSpivakovsky()) == "weak_spivakovsky"
    assert S._host_name(H.WeakSpivakovskyMinHitting(dim=16)) == "weak_spivakovsky_min_hitting"
    assert S._host_name(H.Zeillinger()) == "zeillinger" and S._host_name(H.AllCoordHost()) == "all_coord"

    class Sub(H.ZeillingerLex):
        pass

    for bad in (Sub(), H.RandomHost(seed=0)):
        with pytest.raises(TypeError, match="Zeillinger and hironaka_amd.host.AllCoordHost"):
            S._host_name(bad)
