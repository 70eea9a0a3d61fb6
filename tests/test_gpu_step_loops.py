"""The step loops of the two-lane rollout: their bookkeeping against the C oracle.

`hk::duo_kernel` keeps a game's first finished step as a counter of the steps after which the game was not finished,
votes on scalar masks restricted to the lanes that speak for a game, leaves the one-slot level at the wave's fixed point,
raises its priority between two loops at step 10, and refills the action window between two passes over its levels.
These cases aim at that bookkeeping: last waves of one game and of one game more than a full wave (lanes without a
game), episodes of 1, 2, 11 (across step 10), 20, 25 and 30 steps (25 and 30 refill the window), step offsets 0, 3 and 22
(the window starts inside a Philox block; the first pass is short), batches whose games are all finished at entry (the
wave leaves at the fixed point on step 1) -- and compare, np.array_equal, the final states, `game_length_out`, the
finished-game counts both direct and deferred, and the small per-step records with the oracle.  Every case runs forced
onto the two-lane kernel and once as `pick` routes it.

The (20,3) batches of 193 games are checked on the ORACLE's output to contain a game of length 0, one that is not
finished after 20 steps, one of length 20 and a whole wave (32 consecutive games from a multiple of 32) whose games
all end before step 10: the seeds below were chosen on the CPU for that, so that none of the counter's corner cases drops
out unnoticed."""
import numpy as np
import pytest
import torch

from hironaka_amd import _abi as A
from hironaka_amd import ops
from oracle import c_oracle as CO

pytestmark = pytest.mark.gpu

F2 = A.HK_FLAG_FORCE_TWO_LANES
FORCE = ((F2, "two_lanes"), (0, "default"))
STAGES7 = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON

# name -> (flags, host policy, agent policy, stages, padding value): the configurations of tests/test_gpu_publish.py
# and Zeillinger's host
CONFIGS = {
    "jax7": (CO.flags_of(sem="jax"), A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM, STAGES7, -1.0),
    "jax15": (CO.flags_of(sem="jax"), A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM, STAGES7 | A.HK_STAGE_RESCALE, -1.0),
    "torch7": (CO.flags_of(sem="torch", noop_if_invalid=True, ignore_ended=True), A.HK_HOST_RANDOM,
               A.HK_AGENT_RANDOM_LEGAL, STAGES7, -1.0),
    "torch15_pad7": (CO.flags_of(sem="torch", noop_if_invalid=True, ignore_ended=True), A.HK_HOST_RANDOM,
                     A.HK_AGENT_RANDOM_LEGAL, STAGES7 | A.HK_STAGE_RESCALE, -7.0),
    "torch7_pad0p5": (CO.flags_of(sem="torch"), A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM, STAGES7, -0.5),
    "list": (CO.flags_of(sem="list", noop_if_invalid=True), A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM, STAGES7, -1.0),
    "list_compact": (CO.flags_of(sem="list", noop_if_invalid=True, compact_sorted=True), A.HK_HOST_RANDOM,
                     A.HK_AGENT_RANDOM, A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON, -1.0),
    "zeillinger": (0, A.HK_HOST_ZEILLINGER, A.HK_AGENT_RANDOM, STAGES7, -1.0),
}
SHAPES = [(20, 3), (5, 3), (8, 4), (20, 4)]
BATCHES = (1, 33, 193)
STEPS = (1, 2, 11, 20, 25, 30)
OFFSETS = (0, 3, 22)
QUICK_WAVE = 2  # games 64 .. 95 of a batch of 193: few rows of small values

# (configuration, step offset) -> seed of the policies, chosen with the oracle (see the module's docstring)
SEEDS = {
    ("jax7", 0): 368, ("jax7", 3): 197, ("jax7", 22): 477,
    ("jax15", 0): 368, ("jax15", 3): 197, ("jax15", 22): 477,
    ("torch7", 0): 525, ("torch7", 3): 171, ("torch7", 22): 5,
    ("torch15_pad7", 0): 401, ("torch15_pad7", 3): 138, ("torch15_pad7", 22): 5,
    ("torch7_pad0p5", 0): 368, ("torch7_pad0p5", 3): 197, ("torch7_pad0p5", 22): 477,
    ("list", 0): 1, ("list", 3): 3, ("list", 22): 17,
    ("list_compact", 0): 1, ("list_compact", 3): 3, ("list_compact", 22): 17,
    ("zeillinger", 0): 538, ("zeillinger", 3): 1067, ("zeillinger", 22): 1152,
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


def dev(x):
    return torch.as_tensor(np.array(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def placed_states(m, d, b, pad, seed):
    """[b, m, d] float32, placed as in tests/test_gpu_publish.py: the padding row everywhere, and per game a set of live
    rows of small integers at chosen row indices -- by game index modulo 8: the first row only, the last row only, first
    and last, the first k, the last k, k scattered rows, every row, none.  The values' range goes by game index modulo 4
    (3, 6, 21, 300: ties and dominated rows end a game early, a wide range keeps it going past 20 steps); the games of
    wave QUICK_WAVE keep at most three of their rows, with values below 3."""
    rng = np.random.default_rng(seed)
    p = np.full((b, m, d), pad, dtype=np.float32)
    for g in range(b):
        k = int(rng.integers(2, m + 1))
        kind = g % 8
        rows = {0: [0], 1: [m - 1], 2: [0, m - 1], 3: list(range(k)), 4: list(range(m - k, m)),
                5: sorted(rng.choice(m, size=k, replace=False).tolist()), 6: list(range(m)), 7: []}[kind]
        hi = (3, 6, 21, 300)[g % 4]
        if g // 32 == QUICK_WAVE:
            rows, hi = rows[:3], 3
        p[g, rows] = rng.integers(0, hi, (len(rows), d)).astype(np.float32)
    return p


def finished_states(m, d, b, pad, seed):
    """every game finished at entry: no row, one row somewhere, or one row at the origin (by game index modulo 3)"""
    rng = np.random.default_rng(seed)
    p = np.full((b, m, d), pad, dtype=np.float32)
    for g in range(b):
        if g % 3 == 1:
            p[g, int(rng.integers(0, m))] = rng.integers(0, 9, d).astype(np.float32)
        elif g % 3 == 2:
            p[g, int(rng.integers(0, m))] = 0.0
    return p


def corner_cases_present(length, steps):
    """the counter's corner cases in a batch's game lengths (see the module's docstring)"""
    waves = [length[w:w + 32] for w in range(0, len(length) - 31, 32)]
    return ((length == 0).any() and (length == -1).any() and (length == steps).any()
            and any(((w >= 0) & (w < 10)).all() for w in waves))


_oracle = {}


def check_case(kind, p0, T, cfg, force, seed, step_offset):
    flags, host_policy, agent, stages, pad = CONFIGS[cfg]
    kw = dict(game_offset=3, step_offset=step_offset, host_policy=host_policy, agent_policy=agent, stages=stages,
              padding_value=pad)
    b, m, d = p0.shape
    key = (kind, m, d, b, T, cfg, step_offset)
    if key not in _oracle:  # (the same expectation serves both routes)
        _oracle[key] = CO.rollout(p0, T, seed, flags=flags, record=True, **kw)
    want_p, want = _oracle[key]
    if kind == "finished":
        assert (want["game_length"] == 0).all()
    elif (m, d) == (20, 3) and b == 193 and T == 20:
        assert corner_cases_present(want["game_length"], T), "the oracle's lengths miss a corner case: choose another seed"
    # the plain rollout: final states, lengths, the counts reduced by the launch itself
    P = dev(p0)
    got = ops.rollout(P, T, seed, flags=flags | force, record=("game_length",), **kw)
    assert np.array_equal(host(P).view(np.int32), want_p.view(np.int32))
    assert np.array_equal(host(got["game_length"]), want["game_length"])
    assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"])
    # with the small records, the counts deferred to a reduction of their own
    P = dev(p0)
    ws = ops.rollout_workspace(b, T, (m, d), flags=flags | force)
    rec = ops.rollout(P, T, seed, flags=flags | force, record=("game_length", "host_class", "axis", "done", "reward"),
                      defer_counts=True, workspace=ws, **kw)
    counts = ops.reduce_counts(ws, torch.zeros(T + 1, dtype=torch.int64, device="cuda"), b, T, (m, d),
                               flags=flags | force)
    assert np.array_equal(host(P).view(np.int32), want_p.view(np.int32))
    assert np.array_equal(host(rec["game_length"]), want["game_length"])
    assert np.array_equal(host(counts).astype(np.uint64), want["done_count"])
    for key in ("host_class", "axis", "done", "reward"):
        assert np.array_equal(host(rec[key]), want[key]), key


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_placed_states(shape, cfg, force):
    """placed live rows; every batch, episode length and step offset"""
    m, d = shape
    pad = CONFIGS[cfg][4]
    for b in BATCHES:
        p0 = placed_states(m, d, b, pad, 7)
        for T in STEPS:
            for so in OFFSETS:
                try:
                    check_case("placed", p0, T, cfg, force[0], SEEDS[(cfg, so)], so)
                except AssertionError as err:
                    raise AssertionError(f"{shape} {cfg} {force[1]} b={b} T={T} step_offset={so}") from err


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_game_finished_at_entry(shape, cfg, force):
    """length 0 everywhere: the counter never moves and the wave leaves at the fixed point on step 1"""
    m, d = shape
    pad = CONFIGS[cfg][4]
    for b in BATCHES:
        p0 = finished_states(m, d, b, pad, 11)
        for T in STEPS:
            for so in OFFSETS:
                try:
                    check_case("finished", p0, T, cfg, force[0], SEEDS[(cfg, so)], so)
                except AssertionError as err:
                    raise AssertionError(f"{shape} {cfg} {force[1]} b={b} T={T} step_offset={so}") from err
