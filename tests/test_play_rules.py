"""CPU-side checks of hk_game_play / hironaka_amd.ops.game_play: tests/play_rules.py, the plain restatement the GPU tests
compare the kernel with, is pinned move for move to the fixture made by running the reference's own GameHironaka and
HironakaValidator (tests/golden/make_play_golden.py); the product's playoff bookkeeping is pinned to the same records;
the symbol, the descriptor and the constants are bound; bad arguments are refused on the host before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_cases
import play_rules as P
import search_rules as R
from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import _lib


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "play_game.npz"))


@pytest.fixture(scope="module")
def games(golden):
    return P.load_games(golden)


@pytest.fixture(scope="module")
def playoffs(golden):
    return P.load_playoffs(golden)


def test_fixture_covers_the_issue(games, playoffs):
    assert {g.host for g in games} == set(R.HOSTS) and {g.agent for g in games} == {"choose_first", "random"}
    assert {g.scale for g in games} == {False, True}
    assert {g.root.shape[1] for g in games} == {2, 3, 4, 5, 6, 7}
    assert max(len(g.root) for g in games) == 20 and min(len(g.root) for g in games) <= 5
    assert sum(g.raised for g in games) * 50 <= len(games)
    assert any(g.stopped for g in games) and any(not g.stopped for g in games)
    assert max(len(g.axes) for g in games) == 40
    # the random agent did not always take the lowest coordinate
    assert sum(a != min(c) for g in games if g.agent == "random" for a, c in zip(g.axes, g.lists)) >= 50
    assert {(p.host, p.agent) for p in playoffs} == (
        {(h, a) for h in ("zeillinger", "zeillinger_lex", "all_coord") for a in ("choose_first", "random")}
        | {(h, "choose_first") for h in ("weak_spivakovsky", "weak_spivakovsky_min_hitting")})
    assert {p.scale for p in playoffs} == {False, True} and any(p.value_threshold == 1e3 for p in playoffs)
    assert all(p.step_threshold == 25 and p.num_steps == 300 for p in playoffs)
    assert any(25 in p.len_history for p in playoffs)  # the step threshold cut games off


def test_restatement_follows_every_recorded_game(games):
    """the restated hosts, agents, move, rescale and stops against the reference, move for move and bit for bit"""
    for g in games:
        dtype = np.float64 if g.scale else np.int64
        d = g.root.shape[1]
        first = P.play(g.root, g.host, "choose_first", 0, reduce_root=True, rescale_root=g.scale, dtype=dtype)
        assert np.array_equal(P.points_of(first.state), g.root_state), g.name
        axes = g.axes if g.agent == "random" else None
        got = P.play(g.root, g.host, g.agent if axes is None else "choose_first", len(g.axes), axes=axes,
                     rescaled=g.scale, reduce_root=True, rescale_root=g.scale, dtype=dtype)
        assert got.length == len(g.axes) and got.lists == g.lists and got.axes == g.axes, g.name
        assert got.classes == [R.class_id(c, d) for c in g.lists], g.name
        for mine, want in zip(got.history, g.states):
            assert mine.dtype == dtype and np.array_equal(P.points_of(mine), want), g.name
        if not g.raised:
            assert (got.outcome == P.ENDED) == bool(g.stopped), g.name
            assert got.outcome in (P.ENDED, P.RUNNING), g.name


def test_float64_restatement_equals_the_exact_one_without_rescale(games):
    for g in games[::7]:
        if g.scale:
            continue
        exact = P.play(g.root, g.host, "choose_first", len(g.axes), axes=g.axes, reduce_root=True)
        for dtype in (np.float32, np.float64):
            got = P.play(g.root, g.host, "choose_first", len(g.axes), axes=g.axes, reduce_root=True, dtype=dtype)
            assert got.outcome == exact.outcome and np.array_equal(got.state, exact.state), g.name


def test_restated_playoff_equals_the_recorded_len_history(playoffs):
    for p in playoffs:
        got, used = P.playoff(p.states, p.num_steps, p.host, "choose_first", p.step_threshold, p.scale,
                              p.value_threshold, axes=p.axes if p.agent == "random" else None)
        assert got == p.len_history and used == len(p.states), p.name
        assert sum(got) + len(got) - 1 == p.num_steps, p.name  # every iteration either counts or records


def test_stops_of_the_restatement():
    root = [[3, 0], [0, 3]]
    assert P.play(root, "all_coord", "choose_first", 5).outcome == P.ENDED
    assert P.play([[1, 1], [-1, -1]], "all_coord", "choose_first", 5).length == 0
    # neither point of `full` ever lies below the other (the first is larger in x0 and x1, which sums of the two keep, and
    # smaller in x2, which a {0, 1} move does not touch), and their supports are full: a weak host offers {0, 1} for
    # ever.  An agent that alternates makes the values grow like Fibonacci numbers until they leave the exact integers
    full = [[5, 3, 1], [1, 1, 2]]
    alternate = lambda coords, t: sorted(coords)[t % 2]  # noqa: E731
    for dtype in (np.float32, np.float64):
        got = P.play(full, "weak_spivakovsky", alternate, 200, dtype=dtype)
        assert got.outcome == P.INEXACT and got.lists == [[0, 1]] * got.length, dtype
        assert got.history[-1].max() >= P.LIMITS[np.dtype(dtype)] > got.history[-2].max(), dtype
    assert P.play(full, "weak_spivakovsky", alternate, 30, dtype=np.float64).outcome == P.RUNNING
    assert P.play(full, "weak_spivakovsky", alternate, 200, rescaled=True, dtype=np.float64).outcome == P.RUNNING
    got = P.play(full, "weak_spivakovsky", alternate, 200, value_threshold=1e3, dtype=np.float64)
    assert got.outcome == P.VALUE_LIMIT and got.history[-1].max() > 1e3 >= got.history[-2].max()
    zero_row = [[0, 0, 0], [1, 2, 3], [3, 2, 1]]
    assert P.play(zero_row, "weak_spivakovsky_min_hitting", "choose_first", 3).outcome == P.NO_MOVE
    forced = P.play(full, "all_coord", "choose_first", 3, classes=[0], axes=[2])  # class 0 = {0, 1}
    assert forced.outcome == P.NO_MOVE and forced.length == 0 and np.array_equal(forced.state, full)
    assert P.play(full, "zeillinger", "choose_last", 1).axes == [max(R.host_list("zeillinger", np.asarray(full)))]
    with pytest.raises(TypeError):
        P.play(full, "zeillinger", "choose_first", 1, rescaled=True)  # the exact dtype has no rescale


# ---- the product's bookkeeping (no GPU: hironaka_amd.validator.playoff_history works on arrays) ----------------------

def _lengths_and_outcomes(p):
    """every reset state of a recorded playoff played by the restatement as the kernel would: step_threshold moves"""
    if p.agent == "random":
        return None  # (its draws are the reference's own: only the literal loop above can follow them)
    out = []
    for st in p.states:
        g = P.play(st, p.host, "choose_first", p.step_threshold, rescaled=p.scale, rescale_root=p.scale,
                   value_threshold=p.value_threshold, dtype=np.float64)
        out.append((g.length, g.outcome))
    return np.asarray(out, np.int64)


def test_playoff_history_equals_the_recorded_len_history(playoffs):
    from hironaka_amd.validator import playoff_history
    checked = 0
    for p in playoffs:
        lo = _lengths_and_outcomes(p)
        if lo is None:
            continue
        got, left = playoff_history(lo[:, 0], lo[:, 1], p.num_steps, p.step_threshold)
        assert got == p.len_history and left == 0, p.name
        # a budget that ends exactly on a reset records a trailing 0; one that the games do not fill is handed back
        ended_at = int(np.where(lo[0, 1] == P.ENDED, max(lo[0, 0], 1), lo[0, 0] + 1))
        got, left = playoff_history(lo[:1, 0], lo[:1, 1], ended_at, p.step_threshold)
        assert got == [p.len_history[0], 0] and left == 0, p.name
        got, left = playoff_history(lo[:1, 0], lo[:1, 1], ended_at + 5, p.step_threshold)
        assert got == [p.len_history[0]] and left == 5, p.name
        checked += 1
    assert checked >= 10


def test_playoff_history_refuses_games_without_a_length():
    from hironaka_amd.validator import playoff_history
    with pytest.raises(RuntimeError, match="game 7"):
        playoff_history([3, 4], [P.ENDED, P.INEXACT], 100, 25, first_game=6)
    with pytest.raises(RuntimeError, match="game 0"):
        playoff_history([0, 4], [P.NO_MOVE, P.ENDED], 100, 25)
    # a game the budget never reaches is not looked at
    assert playoff_history([3, 4], [P.ENDED, P.INEXACT], 2, 25) == ([2], 0)


# ---- the C boundary ------------------------------------------------------------------------------------------------

def test_symbol_constants_and_descriptor_are_bound(tmp_path):
    handle = ctypes.CDLL(_lib.build())
    assert hasattr(handle, "hk_game_play") and set(A.PLAY_PROTOTYPES) == {"hk_game_play"}
    text = abi_cases.header("hironaka_hip_play.h")
    assert re.search(r"^int hk_game_play\(const hk_game_play_desc\* desc, void\* stream\);", text, flags=re.M)
    found = re.findall(r"#define\s+(HK_PLAY_\w+)\s+\(?(-?\d+)u?\)?\s", text)
    assert len(found) == 10
    for name, value in found:
        assert getattr(A, name) == int(value), name
    assert (A.HK_PLAY_RUNNING, A.HK_PLAY_ENDED, A.HK_PLAY_NO_MOVE, A.HK_PLAY_INEXACT) == (
        A.HK_MORIN_RUNNING, A.HK_MORIN_ENDED, A.HK_MORIN_NO_MOVE, A.HK_MORIN_INEXACT)
    assert (P.RUNNING, P.ENDED, P.NO_MOVE, P.INEXACT, P.VALUE_LIMIT) == (
        A.HK_PLAY_RUNNING, A.HK_PLAY_ENDED, A.HK_PLAY_NO_MOVE, A.HK_PLAY_INEXACT, A.HK_PLAY_VALUE_LIMIT)
    assert A.HK_ABI_VERSION == 6
    # sizeof / offsetof as the C compiler sees them
    abi_cases.assert_layouts_match_c({"hk_game_play_desc": A.hk_game_play_desc}, tmp_path)


def _desc(buf, ints, **kw):
    q = A.hk_game_play_desc()
    q.points_in = q.points_out = ctypes.addressof(buf)
    q.length_out = q.outcome_out = ctypes.addressof(ints)
    q.batch, q.max_points, q.dim, q.dtype, q.max_steps = 4, 5, 3, A.HK_F32, 3
    q.in_stride = q.out_stride = 15
    q.host, q.agent = A.HK_HOST_ZEILLINGER, A.HK_AGENT_CHOOSE_FIRST
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def test_argument_validation_without_gpu():
    """every refusal is decided on the host, before any launch (no GPU here: a launch would be HK_ERR_LAUNCH or worse)"""
    L = _lib.lib()
    buf, ints = (ctypes.c_double * 4096)(), (ctypes.c_int32 * 64)()
    call = lambda **kw: L.hk_game_play(ctypes.byref(_desc(buf, ints, **kw)), None)  # noqa: E731
    assert L.hk_game_play(None, None) == A.HK_ERR_NULL
    assert call(batch=0) == A.HK_OK  # an empty batch: nothing to do
    assert call(batch=0, points_in=None) == A.HK_OK
    for bad in (dict(dtype=A.HK_I32), dict(dim=8), dict(max_points=65), dict(host=A.HK_HOST_RANDOM), dict(host=6),
                dict(host=-2), dict(agent=A.HK_AGENT_RANDOM), dict(agent=4), dict(flags=16),
                dict(value_threshold=float("nan"))):
        assert call(**bad) == A.HK_ERR_UNSUPPORTED, bad
    for bad in (dict(batch=-1), dict(max_points=0), dict(dim=1), dict(max_steps=-1), dict(in_stride=14),
                dict(out_stride=14), dict(out_stride=16)):  # in place needs equal strides
        assert call(**bad) == A.HK_ERR_SHAPE, bad
    for bad in (dict(points_in=None), dict(points_out=None), dict(length_out=None), dict(outcome_out=None),
                dict(host=A.HK_PLAY_HOST_FORCED)):  # forced classes need class_in
        assert call(**bad) == A.HK_ERR_NULL, bad
    base = ctypes.addressof(buf)
    # records that overlap without being the same buffer
    assert call(points_out=base + 4 * 15) == A.HK_ERR_SHAPE  # the output starts inside the input's span
    assert call(points_in=base + 4 * 15) == A.HK_ERR_SHAPE  # the input starts inside the output's span
    assert call(points_out=base + 4 * 8, in_stride=16, out_stride=16) == A.HK_ERR_SHAPE
    assert call(points_out=base + 4 * 15, in_stride=30, out_stride=30) == A.HK_ERR_SHAPE  # interleaved, no element shared
    # records that span more than 2^63 bytes (the byte count would wrap): refused, in place too, behind the null checks
    far = base + 16384
    for bad in (dict(in_stride=1 << 62), dict(out_stride=1 << 62), dict(in_stride=1 << 62, out_stride=1 << 62),
                dict(batch=5, in_stride=1 << 60)):  # 4 rows x 2^60 elements x 4 bytes: exactly 2^64
        assert call(points_out=far, **bad) == A.HK_ERR_SHAPE, bad
    assert call(in_stride=1 << 62, out_stride=1 << 62) == A.HK_ERR_SHAPE  # in place
    assert call(in_stride=1 << 62, out_stride=1 << 62, points_out=None) == A.HK_ERR_NULL
    assert call(in_stride=1 << 62, out_stride=1 << 62, length_out=None) == A.HK_ERR_NULL
    for bad in (dict(points_in=base + 2, points_out=base + 2), dict(length_out=ctypes.addressof(ints) + 2),
                dict(class_in=ctypes.addressof(ints) + 1), dict(axis_out=ctypes.addressof(ints) + 3),
                dict(dtype=A.HK_F64, points_in=base + 4, points_out=base + 4)):
        assert call(**bad) == A.HK_ERR_ALIGN, bad


def test_wrappers_refuse_what_cannot_run():
    import torch
    from hironaka_amd import ops
    from hironaka_amd.agent import ChooseFirstAgent, PolicyAgent, RandomAgent
    from hironaka_amd.game import GameHironaka
    from hironaka_amd.host import RandomHost, Zeillinger
    from hironaka_amd.validator import HironakaValidator
    with pytest.raises(TypeError):
        ops.game_play(torch.zeros(2, 4, 3), host="zeillinger", max_steps=1)  # a CPU tensor
    with pytest.raises(ValueError):
        ops.game_play(torch.zeros(2, 4, 3), host="random", max_steps=1)
    with pytest.raises(ValueError):
        ops.game_play(torch.zeros(2, 4, 3), host="zeillinger", agent="policy", max_steps=1)
    assert set(ops.PLAY_OUTCOMES) == {0, 1, 3, 4, 5}
    for host, agent in ((RandomHost(), ChooseFirstAgent()), (Zeillinger(), PolicyAgent(None))):
        with pytest.raises(TypeError, match=r"step\(\)"):
            GameHironaka(None, host, agent).play(3)
        with pytest.raises(TypeError):
            HironakaValidator(host, agent)
    v = HironakaValidator(Zeillinger(), RandomAgent(3), {"dimension": 4}, step_threshold=7)
    assert (v.max_num_points, v.dimension, v.max_value, v.value_threshold, v.step_threshold, v.scale_observation) == (
        10, 4, 50, None, 7, True)
