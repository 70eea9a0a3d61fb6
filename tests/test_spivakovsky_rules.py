"""CPU-side checks of hk_spivakovsky_select and the hosts it serves (Spivakovsky, RandomSpivakovsky): the plain-Python
rules of tests/spivakovsky_rules.py against the fixture made by running the reference's own classes
(tests/golden/make_spivakovsky_golden.py), what those rules reach, the header's constants and entry point, and argument
validation before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import _lib
from spivakovsky_rules import (random_spivakovsky_candidates, rule_random_spivakovsky, rule_spivakovsky,
                               three_row_states)

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE, "hironaka_hip_spivakovsky.h")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "spivakovsky.npz"))


# ---- the fixture -------------------------------------------------------------------------------------------------------

def test_fixture_covers_the_issue(fixture):
    for d in range(2, 7):
        st, kind = fixture[f"sel{d}_states"], fixture[f"sel{d}_kind"]
        assert st.shape[1:] == (20, d) and len(st) >= 160 and st.dtype == np.float64
        assert set(kind.tolist()) == {0, 1, 2}  # reduced, raw, rescaled reduced
        assert (st[..., 0] >= 0).sum(1).min() >= 2
        assert fixture[f"sel{d}_spivakovsky"].shape == (len(st), d)
        assert st[kind == 2].max() == 1.0 and st[kind != 2].max() == 20.0
    assert os.path.getsize(os.path.join(GOLDEN, "spivakovsky.npz")) <= os.path.getsize(os.path.join(GOLDEN, "hosts.npz"))
    states, masks = fixture["game_states"], fixture["game_masks"]
    assert states.shape[1:] == (16, 10, 3) and len(states) == len(masks) + 1 and states.max() < 2.0 ** 53
    live = (states[:-1, :, :, 0] >= 0).sum(2) >= 2
    single = live & (masks.sum(2) < 2)
    assert single.any()  # a game meets a one-coordinate subset, and the reference leaves its state as it is
    assert all(np.array_equal(states[t + 1, g], states[t, g]) for t, g in np.argwhere(single))


def test_rules_reproduce_the_reference(fixture):
    for d in range(2, 7):
        states, masks = fixture[f"sel{d}_states"], fixture[f"sel{d}_spivakovsky"]
        cands = fixture[f"sel{d}_random_candidates"]
        for g, st in enumerate(states):
            want = sum(1 << k for k in np.nonzero(masks[g])[0].tolist())
            assert rule_spivakovsky(st) == want, (d, g, st[st[:, 0] >= 0].tolist())
            assert random_spivakovsky_candidates(st) == [c for c in cands[g].tolist() if c >= 0], (d, g)


def test_rules_replay_the_reference_game(fixture):
    states, masks = fixture["game_states"], fixture["game_masks"]
    for t in range(len(masks)):
        for g in range(states.shape[1]):
            got = rule_spivakovsky(states[t, g])
            assert [(got >> k) & 1 for k in range(3)] == masks[t, g].tolist(), (t, g)


# ---- what the rules reach ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def reached(fixture):
    """per dim: the (subset size, levels, last step, alive emptied) of every state of the fixture, of the 3-row states
    at dims 2 and 3, and of seeded random games at dims 4..6"""
    rng = np.random.default_rng(7)
    out = {}
    for d in range(2, 7):
        states = list(fixture[f"sel{d}_states"])
        if d == 2:
            states += list(three_row_states(2))
        elif d == 3:
            states += list(three_row_states(3, every=7))
        else:
            states += [rng.integers(0, 3, (int(rng.integers(2, 6)), d)).astype(float) for _ in range(300)]
        seen = set()
        for st in states:
            trace = {}
            mask = rule_spivakovsky(st, trace)
            seen.add((bin(mask).count("1"), min(trace["levels"], 3), trace["last"], trace["emptied"]))
        out[d] = seen
    return out


def test_rules_reach_every_branch(reached):
    for d in range(2, 7):
        sizes = {s[0] for s in reached[d]}
        assert set(range(2, d + 1)) <= sizes, (d, sizes)
    assert 1 in {s[0] for s in reached[2]} and 1 in {s[0] for s in reached[3]}
    everything = set().union(*reached.values())
    assert 0 in {s[0] for s in everything}
    assert {s[1] for s in everything} == {0, 1, 2, 3}  # 3 stands for >= 3 levels
    assert {s[2] for s in everything} == {"none", "set", "empty"}
    assert {s[3] for s in everything} == {True, False}


def test_rules_on_the_small_cases():
    single = np.array([[1, 2, 3], [-1, -1, -1]], float)
    assert rule_spivakovsky(single) == 0 and random_spivakovsky_candidates(single) == []
    zero_row = np.array([[0, 0, 0], [1, 2, 0], [-1, -1, -1]], float)
    assert rule_spivakovsky(zero_row) == 0  # the zero row ends the levels, and no subset is permissible on it
    assert random_spivakovsky_candidates(zero_row) == [] and rule_random_spivakovsky(zero_row, 2 ** 32 - 1) == 0
    pair = np.array([[0, 1, 2], [2, 1, 0]], float)  # test/testGame.py:45-52
    assert rule_spivakovsky(pair) == 0b101
    assert random_spivakovsky_candidates(pair) == [0b011, 0b101, 0b110]  # supports {1, 2} and {0, 1}
    assert random_spivakovsky_candidates(np.array([[1, 0, 0], [0, 1, 1]], float)) == [0b011, 0b101]
    assert rule_random_spivakovsky(np.array([[1, 0, 0], [0, 1, 1]], float), 2 ** 31) == 0b101


# ---- the header and the entry point --------------------------------------------------------------------------------------

def test_constants_match_the_header():
    text = open(HEADER).read()
    for name in ("HK_HOST_SPIVAKOVSKY", "HK_HOST_RANDOM_SPIVAKOVSKY"):
        got = re.search(rf"#define {name} (\d+)", text)
        assert got and int(got.group(1)) == getattr(A, name), name
    assert (A.HK_HOST_SPIVAKOVSKY, A.HK_HOST_RANDOM_SPIVAKOVSKY) == (6, 7)
    assert '#include "hironaka_hip_spivakovsky.h"' in open(os.path.join(INCLUDE, "hironaka_hip.h")).read()


def test_header_entry_point_is_bound():
    """include/hironaka_hip_spivakovsky.h declares exactly SPIVAKOVSKY_PROTOTYPES, the library exports them and they
    are bound by default"""
    text = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|uint64_t)\s+(hk_\w+)\(", text, flags=re.M))
    assert declared == set(A.SPIVAKOVSKY_PROTOTYPES) == {"hk_spivakovsky_select"}
    assert not declared & (set(A.PROTOTYPES) | set(A.DEVICE_PROTOTYPES))
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
        assert getattr(_lib.lib(), name).argtypes == A.SPIVAKOVSKY_PROTOTYPES[name][1], name


def _call(L, points=1, stride=None, out=1, batch=4, m=6, d=3, dtype=A.HK_F32, host=A.HK_HOST_SPIVAKOVSKY, offset=0):
    buf = (ctypes.c_uint64 * 512)()
    addr = ctypes.addressof(buf)
    ptr = lambda flag: addr + offset if flag else None  # noqa: E731
    return L.hk_spivakovsky_select(ptr(points), m * d if stride is None else stride, ptr(out), batch, m, d, dtype, host,
                                   0, 0, 0, None)


@pytest.mark.parametrize("host", (A.HK_HOST_SPIVAKOVSKY, A.HK_HOST_RANDOM_SPIVAKOVSKY))
def test_spivakovsky_select_argument_validation_without_gpu(host):
    """every status for bad arguments is decided on the host, before any launch, as hk_host_select decides them"""
    L = _lib.lib()
    call = lambda **kw: _call(L, host=host, **kw)  # noqa: E731
    assert call(points=0) == A.HK_ERR_NULL
    assert call(out=0) == A.HK_ERR_NULL
    assert call(stride=17) == A.HK_ERR_SHAPE
    assert call(batch=0, points=0, out=0) == A.HK_OK
    assert call(batch=-1) == A.HK_ERR_SHAPE
    assert call(m=0) == A.HK_ERR_SHAPE
    assert call(d=1) == A.HK_ERR_SHAPE
    assert call(d=7) == A.HK_ERR_UNSUPPORTED
    assert call(m=65) == A.HK_ERR_UNSUPPORTED
    for dt in (A.HK_I32, A.HK_I64, A.HK_U8, 7):  # f16 has no dtype code: anything but f32 / f64
        assert call(dtype=dt) == A.HK_ERR_UNSUPPORTED
    assert call(offset=2) == A.HK_ERR_ALIGN
    assert call(offset=4, dtype=A.HK_F64) == A.HK_ERR_ALIGN
    # the order of hk_host_select: shape before dtype before host before the limits, all before batch == 0 and NULL
    assert call(d=1, dtype=7) == A.HK_ERR_SHAPE
    assert call(batch=0, d=7, points=0, out=0) == A.HK_ERR_UNSUPPORTED


def test_other_host_codes_are_unsupported():
    L = _lib.lib()
    for h in (0, 1, 2, 3, 4, 5, 8, -1):
        assert _call(L, host=h) == A.HK_ERR_UNSUPPORTED, h
        assert _call(L, host=h, batch=0, points=0, out=0) == A.HK_ERR_UNSUPPORTED, h
