"""CPU-side checks of hk_search_morin_play / hironaka_amd.ops.morin_play: tests/morin_rules.py, the plain restatement
the GPU tests compare the kernel with, is pinned move for move to the fixture made by running the reference's own
GameMorin and AgentMorin (tests/golden/make_morin_game_golden.py); the symbol, the descriptor and the constants are
bound; bad arguments are refused on the host before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_cases
import morin_rules as M
import search_rules as R
from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import _lib


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "morin_game.npz"))


@pytest.fixture(scope="module")
def games(golden):
    return M.load_games(golden)


def test_fixture_covers_the_issue(games):
    assert {g.host for g in games} == set(R.HOSTS)
    assert {g.root.shape[1] for g in games} == {2, 3, 4, 5, 6, 7}
    assert len({g.seed for g in games}) >= 3
    assert sum(g.raised for g in games) * 20 <= len(games)
    names = {g.name.rsplit("_s", 1)[0] for g in games}
    for root in ("thom3", "thom4", "thom_original"):
        assert {f"{root}_{h}" for h in R.HOSTS} <= names
    thom4 = next(g for g in games if g.name == "thom4_weak_spivakovsky_s0")
    assert thom4.root.shape == (19, 7) and thom4.dist == 18 and 0 < len(thom4.axes) <= 100 and thom4.stopped
    assert any(g.stopped == 1 for g in games) and any(g.stopped == 2 and g.axes for g in games)
    assert any(g.root_dist < 0 for g in games) and max(len(g.axes) for g in games) > 3
    # a twin of the distinguished row loses it at the root
    twins = [g for g in games if "twin" in g.name]
    assert twins and all(g.root_dist < 0 and not g.axes for g in twins)


def test_every_recorded_tie_break_lies_in_the_subset(games):
    ties = chosen_not_lowest = 0
    for g in games:
        w = [1] * g.root.shape[1]
        for coords, a, w2 in zip(g.lists, g.axes, g.weights):
            assert a in coords, g.name
            rule = M.morin_axis(coords, w, "random")
            if rule is None:
                ties += 1
                chosen_not_lowest += a != min(coords)
            else:  # no tie: the smaller weight of the two lowest coordinates, which are the reference's coords[0:2]
                assert rule == a and set(sorted(coords)[:2]) == set(coords[:2]), g.name
            assert w2 == M.next_weights(coords, w, a, "agent"), g.name
            w = w2
    assert ties >= 100 and chosen_not_lowest >= 10


def test_restatement_follows_every_recorded_game(games):
    """the restated hosts, agent rule, weights, child and tracking against the reference, move for move"""
    for g in games:
        state, dist = M.tracked_newton(g.root, g.dist)
        assert R.rows_of(state) == g.root_state.tolist() and dist == g.root_dist, g.name
        _, axes = M.forced_moves(g)
        got = M.play(g.root, [1] * g.root.shape[1], g.dist, g.host, len(g.axes), axes=axes, tie="random",
                     reduce_root=True)
        assert got.length == len(g.axes) and got.axes == g.axes, g.name
        assert got.classes == [R.class_id(c, g.root.shape[1]) for c in g.lists], g.name
        for (state, w, dist), want, w2, d2 in zip(got.history, g.states, g.weights, g.dists):
            assert R.rows_of(state) == want.tolist() and w == w2 and dist == d2, g.name
        assert got.outcome == {0: M.RUNNING, 1: M.ENDED, 2: M.NO_CONTRIBUTION}[g.stopped], g.name
        # the same game with every move forced and no host
        classes, _ = M.forced_moves(g)
        again = M.play(g.root, [1] * g.root.shape[1], g.dist, None, len(g.axes), classes=classes, axes=g.axes,
                       reduce_root=True)
        assert again.outcome == got.outcome and again.weights == got.weights and again.dist == got.dist, g.name
        assert R.rows_of(again.state) == R.rows_of(got.state), g.name


def test_restated_edge_rules():
    root = np.asarray([[2, 0], [0, 2], [-1, -1]])
    # no reduction: an index that addresses no point is "lost", a game below 2 points has ended, both copied through
    assert M.play(root, [1, 1], 2, "zeillinger", 5).outcome == M.NO_CONTRIBUTION
    one = M.play(root[1:], [1, 1], 0, "zeillinger", 5)
    assert (one.outcome, one.length, one.untouched) == (M.ENDED, 0, True)
    # with the reduction a game that enters with -1 plays untracked and is never "no contribution"
    free = M.play(root, [1, 1], -1, "zeillinger", 5, reduce_root=True)
    assert free.outcome == M.ENDED and free.dist == -1 and free.length >= 1
    # forced moves: a class the dimension does not have, an axis outside the subset, no host
    assert M.play(root, [1, 1], 0, None, 5, classes=[1]).outcome == M.NO_MOVE
    assert M.play(root, [1, 1], 0, None, 5).outcome == M.NO_MOVE
    three = np.asarray([[2, 0, 1], [0, 2, 1]])
    assert M.play(three, [1, 1, 1], 0, None, 5, classes=[0], axes=[2]).outcome == M.NO_MOVE
    # the weight rules and the tie modes
    lo = M.play(three, [1, 1, 1], 0, "all_coord", 1, tie="lowest")
    hi = M.play(three, [1, 1, 1], 0, "all_coord", 1, tie="highest", weight_rule="search")
    assert (lo.axes, lo.weights) == ([0], [1, 0, 0]) and (hi.axes, hi.weights) == ([2], [0, 0, 1])
    assert M.play(three, [2, 1, 1], 0, "all_coord", 1, weight_rule="search").weights == [1, 1, 0]
    # a shifted coordinate at the limit
    big = np.asarray([[2 ** 23, 2 ** 23], [0, 2 ** 24]])
    assert M.play(big, [1, 1], 0, "zeillinger", 3, limit=2 ** 24).outcome == M.INEXACT
    with pytest.raises(ValueError):
        M.play(three, [1, 1, 1], 0, "all_coord", 1, tie="random")


def test_distinguished_elements_record(golden):
    """test/testPoints.py:152-172 as the reference ran it, and the restated tracking on the same sequence"""
    counts, dists = golden["de_counts"].tolist(), golden["de_dists"].tolist()
    states = np.split(golden["de_states"].reshape(-1, 4), np.cumsum(counts)[:-1])
    assert tuple(states[0][dists[0]]) == (8, 3, 17, 8) and tuple(states[1][dists[1]]) == (11, 3, 17, 8)
    assert dists[2] == -1
    state, dist = M.tracked_newton(golden["de_root"].astype(np.int64), 2)
    assert state.tolist() == states[0].tolist() and dist == dists[0]
    shifts = golden["de_shifts"].tolist()
    for group, want, nd in (([shifts[0]], states[1], dists[1]), (shifts[1:], states[2], dists[2])):
        for *mask, a in group:
            state = R.shift(state, [k for k in range(4) if mask[k]], a)
        state, dist = M.tracked_newton(state, dist)
        assert state.tolist() == want.tolist() and dist == nd


# ---- the ABI entry and the wrapper, without a GPU --------------------------------------------------------------------

def test_symbol_descriptor_and_constants():
    L = _lib.lib()
    assert "hk_search_morin_play" in A.PROTOTYPES
    assert L.hk_search_morin_play.argtypes == A.PROTOTYPES["hk_search_morin_play"][1]
    assert A.HK_ABI_VERSION == 6 and L.hk_abi_version() == 6
    text = abi_cases.header()
    for name in ("HK_MORIN_RUNNING", "HK_MORIN_ENDED", "HK_MORIN_NO_CONTRIBUTION", "HK_MORIN_NO_MOVE",
                 "HK_MORIN_INEXACT", "HK_MORIN_TIE_LOWEST", "HK_MORIN_TIE_HIGHEST", "HK_MORIN_TIE_RANDOM",
                 "HK_MORIN_WEIGHTS_AGENT", "HK_MORIN_WEIGHTS_SEARCH", "HK_MORIN_REDUCE_ROOT", "HK_MORIN_HOST_FORCED"):
        got = re.search(rf"#define {name} \(?(-?\d+)u?\)?", text)
        assert got and int(got.group(1)) == getattr(A, name), name
    assert len({A.HK_MORIN_RUNNING, A.HK_MORIN_ENDED, A.HK_MORIN_NO_CONTRIBUTION, A.HK_MORIN_NO_MOVE,
                A.HK_MORIN_INEXACT}) == 5
    assert (M.RUNNING, M.ENDED, M.NO_CONTRIBUTION, M.NO_MOVE, M.INEXACT) == (
        A.HK_MORIN_RUNNING, A.HK_MORIN_ENDED, A.HK_MORIN_NO_CONTRIBUTION, A.HK_MORIN_NO_MOVE, A.HK_MORIN_INEXACT)


def test_descriptor_layout_matches_c(tmp_path):
    """sizeof/offsetof as the C compiler sees them == ctypes"""
    abi_cases.assert_layouts_match_c({"hk_morin_play_desc": A.hk_morin_play_desc}, tmp_path)


REQUIRED = ("points_in", "points_out", "weights_in", "weights_out", "distinguished_in", "distinguished_out", "length_out",
            "outcome_out")
OPTIONAL = ("class_in", "axis_in", "class_out", "axis_out")


def _call(L, null=(), offset=0, offset_of=REQUIRED + OPTIONAL, **fields):
    buf = (ctypes.c_uint64 * 8192)()
    addr = ctypes.addressof(buf)
    q = A.hk_morin_play_desc()
    q.batch, q.max_points, q.dim, q.dtype, q.host, q.max_steps = 4, 6, 4, A.HK_F32, A.HK_HOST_ZEILLINGER, 8
    q.in_stride = q.out_stride = 24
    for name in REQUIRED + OPTIONAL:
        setattr(q, name, None if name in null else addr + (offset if name in offset_of else 0))
    for name, value in fields.items():
        setattr(q, name, value)
    return L.hk_search_morin_play(ctypes.byref(q), None)


def test_argument_validation_without_gpu():
    """every status for bad arguments is decided on the host, before any launch: none of these calls reaches one"""
    L = _lib.lib()
    assert L.hk_search_morin_play(None, None) == A.HK_ERR_NULL
    for name in REQUIRED:
        assert _call(L, null=(name,)) == A.HK_ERR_NULL, name
    assert _call(L, null=("class_in",), host=A.HK_MORIN_HOST_FORCED) == A.HK_ERR_NULL  # no host and no forced classes
    assert _call(L, dim=1) == A.HK_ERR_SHAPE
    assert _call(L, dim=8) == A.HK_ERR_UNSUPPORTED
    assert _call(L, dim=7, in_stride=42, out_stride=42, null=("points_in",)) == A.HK_ERR_NULL  # dim 7 passes the shape checks
    assert _call(L, max_points=0) == A.HK_ERR_SHAPE
    assert _call(L, max_points=65) == A.HK_ERR_UNSUPPORTED
    assert _call(L, max_points=64, in_stride=256, out_stride=256, null=("points_out",)) == A.HK_ERR_NULL
    assert _call(L, dtype=A.HK_I32) == A.HK_ERR_UNSUPPORTED
    assert _call(L, batch=-1) == A.HK_ERR_SHAPE
    assert _call(L, max_steps=-1) == A.HK_ERR_SHAPE
    assert _call(L, host=A.HK_HOST_RANDOM) == A.HK_ERR_UNSUPPORTED
    assert _call(L, host=6) == A.HK_ERR_UNSUPPORTED
    assert _call(L, host=-2) == A.HK_ERR_UNSUPPORTED
    assert _call(L, tie=3) == A.HK_ERR_UNSUPPORTED
    assert _call(L, tie=-1) == A.HK_ERR_UNSUPPORTED
    assert _call(L, weight_rule=2) == A.HK_ERR_UNSUPPORTED
    assert _call(L, flags=2) == A.HK_ERR_UNSUPPORTED
    assert _call(L, in_stride=23) == A.HK_ERR_SHAPE
    assert _call(L, out_stride=23) == A.HK_ERR_SHAPE
    assert _call(L, in_stride=25) == A.HK_ERR_SHAPE  # in place needs equal strides
    for off in (8, 24 * 4 * 4 - 4):  # other than in place, the records of points_in and points_out do not overlap
        assert _call(L, offset=off, offset_of=("points_out",)) == A.HK_ERR_SHAPE
        assert _call(L, offset=off, offset_of=("points_in",)) == A.HK_ERR_SHAPE
    # strided records that interleave without sharing an element
    assert _call(L, offset=24 * 4, offset_of=("points_out",), in_stride=48, out_stride=48) == A.HK_ERR_SHAPE
    assert _call(L, offset=24 * 4, offset_of=("points_in",), in_stride=48, out_stride=48) == A.HK_ERR_SHAPE
    assert _call(L, out_stride=25) == A.HK_ERR_SHAPE  # the same pointer, different strides
    # records that span more than 2^63 bytes (the byte count would wrap): refused, in place too, behind the null checks
    far = dict(offset=32768, offset_of=("points_out",))
    for bad in (dict(in_stride=1 << 62), dict(out_stride=1 << 62), dict(in_stride=1 << 62, out_stride=1 << 62),
                dict(batch=5, in_stride=1 << 60)):  # 4 rows x 2^60 elements x 4 bytes: exactly 2^64
        assert _call(L, **far, **bad) == A.HK_ERR_SHAPE, bad
    assert _call(L, in_stride=1 << 62, out_stride=1 << 62) == A.HK_ERR_SHAPE  # in place
    for name in REQUIRED:
        assert _call(L, null=(name,), in_stride=1 << 62, out_stride=1 << 62) == A.HK_ERR_NULL, name
    assert _call(L, offset=2) == A.HK_ERR_ALIGN
    assert _call(L, offset=2, offset_of=("points_in", "points_out")) == A.HK_ERR_ALIGN
    assert _call(L, dtype=A.HK_F64, offset=4, offset_of=("points_in", "points_out")) == A.HK_ERR_ALIGN
    assert _call(L, offset=2, offset_of=("axis_out",)) == A.HK_ERR_ALIGN
    assert _call(L, batch=0, null=REQUIRED + OPTIONAL) == A.HK_OK


def test_wrapper_refuses_bad_arguments_without_gpu():
    import torch
    from hironaka_amd import ops
    pts, w, dist = torch.zeros(2, 4, 3), torch.ones(2, 3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.morin_play(pts, w, dist, host="zeillinger", max_steps=1)
    with pytest.raises(TypeError):
        ops.morin_play(pts.tolist(), w, dist, host="zeillinger", max_steps=1)
    # names and scalars are refused before the tensors are looked at
    for bad in (dict(host="spivakovsky"), dict(host="random"), dict(tie="middle"), dict(weight_rule="tree"),
                dict(max_steps=-1), dict(max_steps=2 ** 31), dict(seed=-1), dict(game_offset=2 ** 64),
                dict(step_offset=2 ** 32 - 1)):
        with pytest.raises(ValueError):
            ops.morin_play(pts, w, dist, **{"host": "zeillinger", "max_steps": 1, **bad})
    assert set(ops.MORIN_TIES) == {"lowest", "highest", "random"} and set(ops.MORIN_WEIGHT_RULES) == {"agent", "search"}
    assert set(ops.MORIN_OUTCOMES) == {0, 1, 2, 3, 4}
    from hironaka_amd.agent import AgentMorin
    from hironaka_amd.game import GameMorin  # noqa: F401
    with pytest.raises(ValueError):
        AgentMorin(tie="middle")
    assert AgentMorin.USE_WEIGHTS and AgentMorin.USE_REPOSITION
    with pytest.raises(Exception):
        AgentMorin().move(None, None)  # missing weights raise, as in the reference


def test_wrapper_range_check_without_gpu():
    """ops.morin_play's only guard of the device data, on CPU tensors: the C entry cannot look at them"""
    import torch
    from hironaka_amd.ops import _morin_range_error as refused
    m = 4
    w, dist = torch.ones(2, 3, dtype=torch.int32), torch.tensor([0, m - 1], dtype=torch.int32)
    moves = torch.full((2, 5), -1, dtype=torch.int64)
    for rule in ("agent", "search"):
        assert refused(w, dist, None, None, m, rule) is None
        assert refused(w, torch.tensor([-1, 0]), moves, moves, m, rule) is None  # -1: lost / none
        assert refused(torch.zeros(2, 3, dtype=torch.int64) + 2 ** 31 - 1, dist, None, None, m, rule) is None
        for bad in (torch.tensor([0, m]), torch.tensor([-2, 0])):
            assert "distinguished" in refused(w, bad, None, None, m, rule), (rule, bad)
        heavy = w.to(torch.int64)
        heavy[1, 2] = 2 ** 31
        assert "weights" in refused(heavy, dist, None, None, m, rule)
        wide = moves.clone()
        wide[1, 4] = 2 ** 31
        assert refused(w, dist, wide, None, m, rule) and refused(w, dist, None, wide, m, rule)
    negative = w.clone()
    negative[1, 2] = -1
    assert "weights" in refused(negative, dist, None, None, m, "agent")
    # the search rule leaves such weights itself (w[i] -= w[axis] with w[i] < w[axis]) and takes them back
    assert M.next_weights([0, 1, 2], [2, 3, 1], 0, "search") == [2, 1, -1]
    assert refused(negative, dist, None, None, m, "search") is None
    below = w.to(torch.int64)
    below[0, 0] = -2 ** 31 - 1
    assert "weights" in refused(below, dist, None, None, m, "search")
