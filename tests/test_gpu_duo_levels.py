"""The two-lane rollout's levels, pair tests and action window against the C oracle, bit for bit.

The staircase of hk::duo_kernel has a level of seven slots per lane, and its domination test keeps the verdicts of a row as
sign bits of a word.  What decides the level is the widest game of a wave, so the batches here place one game of exactly
n live rows -- first in a wave of narrow games, and a whole wave of them -- for every n around the levels' edges (6, 7, 8
and 10 slots per lane at 20 rows; the top levels of the other shapes).  Rows past a game's count hold the fill value, so
every wave stays on the exact path.  The pair tests see ties in every position two rows can have to each other (same
lane, the two lanes of a slot, across slots), games of 0, 1 and 2 rows and rows of zeros; the action window is crossed at
its edge and at a refill by a wave whose first game outlasts step 16.  Every launch runs forced onto two lanes and as
routed; the state sits between two sentinel games that must come back untouched.  States are compared as int32 views."""
import numpy as np
import pytest
import torch

import level_cases as LC
from hironaka_amd import _abi as A
from hironaka_amd import ops
from oracle import c_oracle as CO
from test_gpu_step_loops import CONFIGS

pytestmark = pytest.mark.gpu

ROUTES = (("two", A.HK_FLAG_FORCE_TWO_LANES), ("routed", 0))
WIDTHS = {(20, 3): (11, 12, 13, 14, 15, 16, 20), (16, 3): (13, 14, 15, 16), (20, 4): (13, 14)}
BATCHES = (1, 32, 33, 65)
CFGS = ("jax7", "torch7", "jax15")  # the two compiled-in configurations and a run-time one
SENTINEL = np.float32(-12345.0)
GAMES = 32  # per wave
SUM = 11    # rows are compositions of 11: 78 of them in three parts


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def same(what, got, want, tag):
    got, want = bits(got), bits(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    where = ""
    if got.shape == want.shape and got.ndim >= 1 and what != "done_count":
        axis = 1 if what in ("host_class", "axis", "done", "reward") else 0
        bad = np.moveaxis(got != want, axis, 0).reshape(got.shape[axis], -1).any(axis=1)
        where = f", first at game {int(np.argwhere(bad)[0, 0])}"
    raise AssertionError(f"{tag}: {what} differs from the oracle{where}")


def fenced(p0):
    """the state on the device between two sentinel games: (whole buffer, view of the state)"""
    b, m, d = p0.shape
    buf = torch.full((b + 2, m, d), float(SENTINEL), dtype=torch.float32, device="cuda")
    buf[1:b + 1] = torch.as_tensor(p0).cuda()
    return buf, buf[1:b + 1]


def fence_ok(buf, tag):
    ends = buf[[0, -1]].cpu().numpy()
    assert (ends == SENTINEL).all(), f"{tag}: a sentinel game was written"


def wide_batch(m, d, b, n, whole, seed, pad=-1.0):
    """b games: the first of every wave (`whole`: every game) holds exactly n antichain rows at scattered indices, the
    others 0..3 rows"""
    rng = np.random.default_rng(seed)
    p = np.full((b, m, d), pad, dtype=np.float32)
    for g in range(b):
        LC.place(rng, p[g], n if (whole or g % GAMES == 0) else int(rng.integers(0, 4)), SUM)
    assert max(LC.widest_per_wave(p, "two")) == n and LC.widest_per_wave(p, "two")[0] == n
    return p


def roll_both(p0, T, seed, cfg, tag, step_offset=0, record=("game_length",)):
    flags, host_policy, agent, stages, pad = CONFIGS[cfg]
    small = tuple(k for k in record if k != "game_length")
    want_p, want = CO.rollout(p0, T, seed, game_offset=3, step_offset=step_offset, host_policy=host_policy,
                              agent_policy=agent, stages=stages, flags=flags, padding_value=pad, record=bool(small))
    for route, force in ROUTES:
        buf, P = fenced(p0)
        got = ops.rollout(P, T, seed, game_offset=3, step_offset=step_offset, host_policy=host_policy, agent_policy=agent,
                          stages=stages, padding_value=pad, flags=flags | force, record=record)
        t = f"{tag} ({route})"
        same("final state", P.cpu().numpy(), want_p, t)
        for k in record:
            same(k, got[k].cpu().numpy(), want[k], t)
        same("done_count", got["done_count"].cpu().numpy().astype(np.uint64), want["done_count"], t)
        fence_ok(buf, t)
    return want


# ---- the widest game of the wave ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("shape", list(WIDTHS), ids=lambda s: f"{s[0]}x{s[1]}")
def test_rollouts_by_widest_game(shape, cfg):
    """rollouts of 1, 2 and 20 steps from waves that enter on each of the top levels"""
    m, d = shape
    slots = set()
    for n in WIDTHS[shape]:
        slots.add((n + 1) // 2)
        for b in BATCHES:
            for whole in (False, True):
                p0 = wide_batch(m, d, b, n, whole, 1000 * m + 10 * n + b)
                for T in (1, 2, 20):
                    roll_both(p0, T, 7 + n, cfg, f"{shape} {cfg} widest {n} rows, b={b}, whole wave={whole}, T={T}")
    if shape == (20, 3):
        assert slots == {6, 7, 8, 10}


@pytest.mark.parametrize("shape", list(WIDTHS), ids=lambda s: f"{s[0]}x{s[1]}")
def test_steps_by_widest_game(shape):
    """hk_step with the caller's actions at each width"""
    m, d = shape
    rng = np.random.default_rng(5 * m + d)
    for n in WIDTHS[shape]:
        for b, whole in ((33, False), (65, True)):
            p0 = wide_batch(m, d, b, n, whole, 2000 * m + 10 * n + b)
            cls = rng.integers(0, 2 ** d - d - 1, b).astype(np.int32)
            ax = rng.integers(0, d, b).astype(np.int32)
            for sem in ("jax", "torch"):
                fo = CO.flags_of(sem=sem, noop_if_invalid=sem != "jax", ignore_ended=sem == "torch")
                want = CO.step(p0, cls, ax, stages=7, flags=fo)
                for route, force in ROUTES:
                    buf, P = fenced(p0)
                    out = torch.full_like(buf, float(SENTINEL))
                    got = ops.step(P, torch.as_tensor(cls).cuda(), torch.as_tensor(ax).cuda(), stages=7,
                                   flags=ops.make_flags(sem, sem != "jax", sem == "torch") | force, out=out[1:b + 1],
                                   want=("done", "prev_done", "reward", "num_points"))
                    t = f"hk_step {shape} {sem} widest {n} rows, b={b} ({route})"
                    for k in ("points", "done", "prev_done", "reward", "num_points"):
                        same(k, got[k].cpu().numpy(), want[k], t)
                    fence_ok(out, t)
                    same("the input", P.cpu().numpy(), p0, t)


# ---- ties and holes ---------------------------------------------------------------------------------------------------
def tie_batch(m, d, pad=-1.0):
    """games whose live rows (in row order: the compact rank) repeat a row at rank distance 1 from an even rank (the two
    lanes of one slot), 1 from an odd rank and 3 (across slots), and 2 (one lane); games of 0, 1 and 2 rows, of equal rows
    only, of rows of zeros; every pattern at scattered and at leading row indices"""
    rng = np.random.default_rng(99)
    base = LC.compositions(rng, 8, SUM, d)
    patterns = []
    for i, j in ((0, 1), (2, 3), (1, 2), (3, 4), (0, 2), (1, 3), (0, 3), (1, 4), (0, 7), (6, 7)):
        rows = base.copy()
        rows[j] = rows[i]
        patterns.append(rows)
    patterns.append(np.repeat(base[:1], 8, axis=0))               # eight equal rows
    patterns.append(np.concatenate([base[:4], base[:4]]))         # every row twice, four ranks apart
    patterns.append(np.repeat(base[:4], 2, axis=0))               # every slot's two lanes equal
    zeros = np.zeros((1, d), dtype=np.float32)
    patterns += [np.zeros((0, d), np.float32), base[:1], zeros, base[:2], np.repeat(base[:1], 2, axis=0),
                 np.concatenate([zeros, zeros]), np.concatenate([zeros, base[:1]]), np.concatenate([base[:1], zeros, zeros])]
    games = []
    for rows in patterns:
        for scattered in (False, True):
            g = np.full((m, d), pad, dtype=np.float32)
            idx = np.sort(rng.choice(m, size=len(rows), replace=False)) if scattered else np.arange(len(rows))
            g[idx] = rows
            games.append(g)
    return np.stack(games)


@pytest.mark.parametrize("shape", [(20, 3), (16, 3), (20, 4), (8, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_ties_and_holes(shape):
    m, d = shape
    p0 = tie_batch(m, d)
    assert not np.signbit(p0[p0 >= 0]).any()  # (+0 throughout)
    for cfg in CFGS + ("list",):
        for T in (1, 2, 5):
            roll_both(p0, T, 11, cfg, f"{shape} {cfg} ties, T={T}")
    # newton alone on the duplicates as they stand, through hk_step
    cls, ax = np.zeros(len(p0), np.int32), np.zeros(len(p0), np.int32)
    for stages in (4, 7):
        want = CO.step(p0, cls, ax, stages=stages, flags=CO.flags_of(sem="jax"))
        for route, force in ROUTES:
            got = ops.step(torch.as_tensor(p0).cuda(), torch.as_tensor(cls).cuda(), torch.as_tensor(ax).cuda(), stages=stages,
                           flags=ops.make_flags("jax") | force, want=("num_points",))
            same("points", got["points"].cpu().numpy(), want["points"], f"hk_step {shape} ties stages={stages} ({route})")
            same("num_points", got["num_points"].cpu().numpy(), want["num_points"], f"hk_step {shape} ties ({route})")


def test_step_that_makes_two_rows_equal():
    """rows (1,2,5) and (9,2,5): the subset {1, 2} with axis 0 sends both to (7,2,5) -- the earlier one survives.  Every
    class and axis, the two rows at ranks (0,1), (1,2), (0,2) and (2,3) among other rows"""
    m, d = 20, 3
    a, c = np.array([1, 2, 5], np.float32), np.array([9, 2, 5], np.float32)
    far = np.array([[0, 30, 0], [0, 0, 30], [0, 29, 1]], np.float32)  # incomparable with both, before and after
    games, cls, ax = [], [], []
    for rows in ([a, c], [far[0], a, c], [a, far[0], c], [far[0], far[1], a, c], [a, far[0], far[1], far[2], c]):
        for k in range(2 ** d - d - 1):
            for axis in range(d):
                g = np.full((m, d), -1.0, dtype=np.float32)
                g[2:2 + len(rows)] = np.stack(rows)
                games.append(g)
                cls.append(k)
                ax.append(axis)
    p0, cls, ax = np.stack(games), np.array(cls, np.int32), np.array(ax, np.int32)
    want = CO.step(p0, cls, ax, stages=5, flags=CO.flags_of(sem="jax"))
    merged = [(want["points"][g] == np.array([7, 2, 5], np.float32)).all(axis=-1).sum() for g in range(len(p0))]
    assert merged.count(1) >= 5 and 2 not in merged, "the oracle keeps one of the two equal rows, in every arrangement"
    for stages in (5, 7):
        want = CO.step(p0, cls, ax, stages=stages, flags=CO.flags_of(sem="jax"))
        for route, force in ROUTES:
            got = ops.step(torch.as_tensor(p0).cuda(), torch.as_tensor(cls).cuda(), torch.as_tensor(ax).cuda(), stages=stages,
                           flags=ops.make_flags("jax") | force, want=("num_points",))
            same("points", got["points"].cpu().numpy(), want["points"], f"equal rows by a step, stages={stages} ({route})")
            same("num_points", got["num_points"].cpu().numpy(), want["num_points"], f"equal rows by a step ({route})")


# ---- the action window ------------------------------------------------------------------------------------------------
# (configuration, step offset) -> seed of the policies under which the batch's first game lasts 19 steps and more (chosen
# with the oracle; every test asserts it again)
LONG_SEEDS = {("jax7", 0): 124, ("jax7", 3): 11, ("torch7", 0): 32, ("torch7", 3): 130, ("jax15", 0): 124, ("jax15", 3): 11}


def long_batch(b):
    """(20,3): the batch's first game holds 20 antichain rows of sum 60; the others are small"""
    m, d = 20, 3
    rng = np.random.default_rng(8)
    p = np.full((b, m, d), -1.0, dtype=np.float32)
    LC.place(rng, p[0], m, 60)
    for g in range(1, b):
        LC.place(rng, p[g], int(rng.integers(0, 6)), SUM)
    return p


def lasts(want):
    first = want["game_length"][0]
    assert first < 0 or first > 17, f"the wave's first game ends at step {first}"


@pytest.mark.parametrize("offset", (0, 3))
@pytest.mark.parametrize("cfg", ("jax7", "torch7", "jax15"))
def test_episodes_across_the_action_window(cfg, offset):
    """20, 24 and 25 steps: inside the window of 24, up to its edge, past it (a refill); from a step offset of 3 the window's
    first block is entered in its last step and the refill comes at step 21"""
    p0 = long_batch(33)
    for T in (20, 24, 25):
        lasts(roll_both(p0, T, LONG_SEEDS[cfg, offset], cfg, f"(20, 3) {cfg} T={T} from step {offset}", step_offset=offset))


@pytest.mark.parametrize("cfg", ("jax7", "torch7"))
def test_small_records_across_the_action_window(cfg):
    keys = ("host_class", "axis", "done", "reward", "game_length")
    p0 = long_batch(33)
    for offset in (0, 3):
        for T in (20, 25):
            lasts(roll_both(p0, T, LONG_SEEDS[cfg, offset], cfg, f"(20, 3) {cfg} records T={T} from step {offset}",
                            step_offset=offset, record=keys))
