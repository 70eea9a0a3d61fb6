"""The two-lane kernel's finished-game counts, action window and padding rows against the C oracle.

Plain rollouts of `hk::duo_kernel` on the exact path count their finished games in closed form when the episode has at
most 63 steps: a histogram of the games' first finished steps in LDS, a prefix sum across the lanes, one atomic per step
from lane `step` -- step 0 (the games finished at entry) included.  Longer episodes, the whole-wave slow path and the
recording loop keep their own counting.  The decoded actions of a window of steps are computed before the first step and
refilled between two passes over the step loops; the small per-step records are read from the window after a refill.
The publish pads the rows that died in straight line over the slots per lane at entry.  These cases aim at exactly that:

* (20,3) with batches of 1, 31, 32, 33 and 65 games -- a wave of one game, a wave one game short, a full wave, a wave of
  one game behind a full one -- and one case each at (10,3) and (20,4), which share the counts;
* episodes of 1, 15, 16, 17, 20, 24 and 25 steps (the window's edge, a refill of one block, a refill at the last step),
  63 and 64 (the last length the histogram serves, the first one the ballots serve) and 70, at step offsets 0 and 3 (an
  offset of 3 puts the window's blocks across the first step); the first game of every wave lasts 23 steps or more;
* jax, torch and list semantics, and Zeillinger's host (no window, the same counts);
* the small records (host class, axis, done, reward) at 20 and 25 steps;
* placed states: every game finished at entry (the whole wave in the histogram's first word); one step from dense
  states (no game finished: nothing is added anywhere); one non-representable row (the slow path's own counts beside a
  neighbouring wave's histogram);
* deferred counts accumulated over three launches with different seeds into one workspace, reduced once: the sum of the
  oracle's three histograms, and a workspace that is all zero afterwards;
* a sentinel row before and after every output, so that a padding store past a game's rows shows.

Everything is compared with np.array_equal -- final states as bit patterns, `game_length`, `done_count` direct and
deferred -- forced onto two lanes and as `pick` routes it."""
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
SENTINEL = 0x7FC0BEEF  # a quiet NaN

# name -> (flags, host policy, agent policy, stages, padding value)
CONFIGS = {
    "jax": (CO.flags_of(sem="jax"), A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM, STAGES7, -1.0),
    "torch": (CO.flags_of(sem="torch", noop_if_invalid=True, ignore_ended=True), A.HK_HOST_RANDOM,
              A.HK_AGENT_RANDOM_LEGAL, STAGES7, -1.0),
    "list": (CO.flags_of(sem="list", noop_if_invalid=True), A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM, STAGES7, -1.0),
    "zeillinger": (0, A.HK_HOST_ZEILLINGER, A.HK_AGENT_RANDOM, STAGES7, -1.0),
}
BATCHES = (1, 31, 32, 33, 65)
WINDOW_STEPS = (1, 15, 16, 17, 20, 24, 25)
LONG_STEPS = (63, 64, 70)
OFFSETS = (0, 3)
SMALL_RECORDS = ("host_class", "axis", "done", "reward")

# Random play ends a game after 5 steps on average, and a wave stops once its games sit at their fixed points: a wave
# that is still playing when the action window ends takes a game that lasts.  (configuration, step offset) -> (seed,
# ((position, game of the generator's stream LONG_GEN, its length), ...)): dense (20,3) states that last at least 23
# steps at that position of the batch -- positions 0, 32 and 64, the first game of each wave of a batch of 65 -- under
# that seed's policy stream at game offset 3.  Found by playing 30 000 drawn states through the oracle per seed; the
# lengths are asserted below.  Zeillinger's host has no window: no placed games.
LONG_GEN = dict(max_value=1000, seed=9000)
LONG = {
    ("jax", 0): (3, ((0, 9121, 30), (32, 17072, 23), (64, 24154, 23))),
    ("jax", 3): (11, ((0, 9284, 32), (32, 19088, 35), (64, 20066, 24))),
    ("torch", 0): (15, ((0, 9427, 28), (32, 11903, 28), (64, 21037, 29))),
    ("torch", 3): (36, ((0, 6976, 29), (32, 13315, 30), (64, 23128, 37))),
    ("list", 0): (26, ((0, 8451, 38), (32, 11927, 34), (64, 20943, 36))),
    ("list", 3): (12, ((0, 1749, 38), (32, 14291, 40), (64, 25816, 38))),
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


def dev(x):
    return torch.as_tensor(np.array(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def mixed_states(m, d, b, seed):
    """[b, m, d] float32: Newton-reduced states as the generator draws them, every fourth game dense (all m rows live)"""
    p = CO.generate_points(b, m, d, 20, seed)
    dense = CO.generate_points(b, m, d, 20, seed + 1, stages=0)
    p[3::4] = dense[3::4]
    return p


def lasting_states(b, gen_seed, cfg, step_offset):
    """(20,3): mixed states with the games of LONG at their positions; returns (states, seed, {position: length})"""
    p = mixed_states(20, 3, b, gen_seed)
    if (cfg, step_offset) not in LONG:
        return p, 11, {}
    seed, placed = LONG[(cfg, step_offset)]
    lengths = {}
    for pos, game, length in placed:
        if pos < b:
            p[pos] = CO.generate_points(1, 20, 3, LONG_GEN["max_value"], LONG_GEN["seed"], stages=0, game_offset=game)[0]
            lengths[pos] = length
    return p, seed, lengths


def assert_lengths(want, T, lengths):
    """the placed games last as long as the table says (the episode's T steps permitting)"""
    for pos, length in lengths.items():
        assert want["game_length"][pos] == (length if length <= T else -1), (pos, length, T)


def guarded_output(p0):
    """a [b, m, d] output holding the initial states, with a sentinel row before and after it"""
    b, m, d = p0.shape
    n, row = b * m * d, m * d
    raw = torch.empty(n + 2 * row + 64, dtype=torch.float32, device="cuda")
    base = (-raw.data_ptr() % 256) // 4
    flat = raw[base:base + n + 2 * row]
    flat.view(torch.int32).fill_(SENTINEL)
    out = flat[row:row + n].view(b, m, d)
    out.copy_(dev(p0))
    return flat, out


def guard_rows_intact(flat, out):
    bits = host(flat.view(torch.int32))
    row = out.shape[1] * out.shape[2]
    return bool((bits[:row] == SENTINEL).all() and (bits[row + out.numel():] == SENTINEL).all())


_oracle = {}


def expectation(tag, p0, T, cfg, seed, step_offset, record=False):
    """the oracle's (final states, records) of one rollout: computed once, shared by both routes, never written to"""
    flags, host_policy, agent, stages, pad = CONFIGS[cfg]
    b, m, d = p0.shape
    key = (tag, m, d, b, T, cfg, seed, step_offset, record)
    if key not in _oracle:
        _oracle[key] = CO.rollout(p0, T, seed, flags=flags, record=record, game_offset=3, step_offset=step_offset,
                                  host_policy=host_policy, agent_policy=agent, stages=stages, padding_value=pad)
    return _oracle[key]


def rollout_kw(cfg, step_offset):
    flags, host_policy, agent, stages, pad = CONFIGS[cfg]
    return flags, dict(game_offset=3, step_offset=step_offset, host_policy=host_policy, agent_policy=agent,
                       stages=stages, padding_value=pad)


def check_rollout(tag, p0, T, cfg, force, *, seed=11, step_offset=0):
    flags, kw = rollout_kw(cfg, step_offset)
    b, m, d = p0.shape
    want_p, want = expectation(tag, p0, T, cfg, seed, step_offset)
    # final states, lengths, the counts reduced by the launch itself
    flat, out = guarded_output(p0)
    got = ops.rollout(out, T, seed, flags=flags | force, record=("game_length",), **kw)
    assert np.array_equal(host(out).view(np.int32), want_p.view(np.int32))
    assert guard_rows_intact(flat, out)
    assert np.array_equal(host(got["game_length"]), want["game_length"])
    assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"])
    # the counts deferred to a reduction of their own
    flat, out = guarded_output(p0)
    ws = ops.rollout_workspace(b, T, (m, d), flags=flags | force)
    got = ops.rollout(out, T, seed, flags=flags | force, record=("game_length",), defer_counts=True, workspace=ws, **kw)
    counts = ops.reduce_counts(ws, torch.zeros(T + 1, dtype=torch.int64, device="cuda"), b, T, (m, d),
                               flags=flags | force)
    assert np.array_equal(host(out).view(np.int32), want_p.view(np.int32))
    assert guard_rows_intact(flat, out)
    assert np.array_equal(host(got["game_length"]), want["game_length"])
    assert np.array_equal(host(counts).astype(np.uint64), want["done_count"])
    assert not host(ws).any()
    return want


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_window_edges_at_20x3(cfg, force):
    """episodes that end before, at and behind the edge of a window of 16 or 24 steps, from step offsets 0 and 3; every
    wave's first game lasts 23 steps or more (LONG), so the waves play on past the window's edge and refill it"""
    for b in BATCHES:
        for so in OFFSETS:
            p0, seed, lengths = lasting_states(b, 100 + b, cfg, so)
            for T in WINDOW_STEPS:
                try:
                    want = check_rollout("lasting", p0, T, cfg, force[0], seed=seed, step_offset=so)
                except AssertionError as err:
                    raise AssertionError(f"{cfg} {force[1]} b={b} T={T} step_offset={so}") from err
                assert_lengths(want, T, lengths)
                assert want["done_count"][-1] == (want["game_length"] >= 0).sum()


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_histogram_and_ballots_at_20x3(cfg, force):
    """63 steps: the last episode the histogram serves (lane 63 adds the last step's count); 64 and 70: the ballots, with
    the entry count of their own"""
    for b in (1, 33, 65):
        for so in OFFSETS:
            p0, seed, lengths = lasting_states(b, 150 + b, cfg, so)
            for T in LONG_STEPS if so == 0 else (70,):
                try:
                    want = check_rollout("lasting_long", p0, T, cfg, force[0], seed=seed, step_offset=so)
                except AssertionError as err:
                    raise AssertionError(f"{cfg} {force[1]} b={b} T={T} step_offset={so}") from err
                assert_lengths(want, T, lengths)


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("shape", [(10, 3), (20, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_other_instantiations(shape, cfg, force):
    """(10,3) and (20,4): the counts are shared; (20,4) keeps the slot-by-slot deal and the refill of the whole image"""
    m, d = shape
    p0 = mixed_states(m, d, 33, 400)
    for T in (20, 25):
        try:
            check_rollout("mixed", p0, T, cfg, force[0], step_offset=3)
        except AssertionError as err:
            raise AssertionError(f"{shape} {cfg} {force[1]} T={T}") from err


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", ["jax", "torch"])
def test_small_records(cfg, force):
    """host class, axis, done and reward of every step at 20 and 25 steps: the records' flush reads the action window
    and the games' lengths behind the counts, window by window"""
    for b in (33, 65):
        for so in OFFSETS:
            p0, seed, lengths = lasting_states(b, 250 + b, cfg, so)
            for T in (20, 25):
                flags, kw = rollout_kw(cfg, so)
                want_p, want = expectation("lasting_rec", p0, T, cfg, seed, so, record=True)
                assert_lengths(want, T, lengths)
                flat, out = guarded_output(p0)
                got = ops.rollout(out, T, seed, flags=flags | force[0], record=SMALL_RECORDS + ("game_length",), **kw)
                where = f"{cfg} {force[1]} b={b} T={T} step_offset={so}"
                assert np.array_equal(host(out).view(np.int32), want_p.view(np.int32)), where
                assert guard_rows_intact(flat, out), where
                for key in SMALL_RECORDS + ("game_length",):
                    assert np.array_equal(host(got[key]), want[key]), f"{where} {key}"
                assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"]), where


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_every_game_finished_at_entry(cfg, force):
    """no row, or one row somewhere: every game of every wave counts at step 0 and at every step after it"""
    m, d = 20, 3
    rng = np.random.default_rng(6)
    for b in (32, 33, 65):
        p0 = np.full((b, m, d), CONFIGS[cfg][4], dtype=np.float32)
        for g in range(1, b, 2):
            p0[g, int(rng.integers(0, m))] = rng.integers(0, 9, d).astype(np.float32)
        for T in (1, 20, 63):
            want = check_rollout("finished", p0, T, cfg, force[0], step_offset=3)
            assert (want["game_length"] == 0).all() and (want["done_count"] == b).all()


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_no_game_finished(cfg, force):
    """one step from dense states: no game is finished, no slot of the workspace takes anything"""
    m, d = 20, 3
    for b in (1, 33, 65):
        # (a dense game can end at once; what a game does depends on its state and its position's policy stream alone:
        # every position takes the first of four drawn states that its stream leaves open)
        drawn = [CO.generate_points(b, m, d, 20, 600 + b + 100 * k, stages=0) for k in range(4)]
        open_ = [expectation(f"dense_{k}", p, 1, cfg, 7, 0)[1]["game_length"] == -1 for k, p in enumerate(drawn)]
        assert np.any(open_, axis=0).all()
        pick = np.argmax(open_, axis=0)
        p0 = np.stack([drawn[pick[g]][g] for g in range(b)])
        want = check_rollout("dense_open", p0, 1, cfg, force[0], seed=7)
        assert (want["game_length"] == -1).all() and not want["done_count"].any()


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", ["jax", "torch", "zeillinger"])
def test_slow_path_beside_the_histogram(cfg, force):
    """a row that is not representable sends its game's whole wave down the generic routines, with their own counts; the
    waves around it keep the histogram"""
    m, d = 20, 3
    for game, row, bad in ((3, 1, (2.0, -1.0, 3.0)), (40, 12, (1.0, -2.5, 0.0)), (64, 19, (0.0, 5.0, -1.0))):
        p0 = mixed_states(m, d, 65, 800)
        p0[game, row] = bad
        for T in (20, 25):
            try:
                check_rollout(f"bad_{game}", p0, T, cfg, force[0], step_offset=3)
            except AssertionError as err:
                raise AssertionError(f"{cfg} {force[1]} game {game} row {row} = {bad} T={T}") from err


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_deferred_counts_over_three_launches(cfg, force):
    """three launches with seeds of their own add to one workspace; one reduction gives the sum of the three histograms
    and leaves the workspace zeroed"""
    m, d = 20, 3
    for b in (33, 65):
        p0, first, _ = lasting_states(b, 700 + b, cfg, 0)
        for T in (20, 25, 64):
            flags, kw = rollout_kw(cfg, 0)
            ws = ops.rollout_workspace(b, T, (m, d), flags=flags | force[0])
            total = np.zeros(T + 1, dtype=np.uint64)
            for seed in (first, 122, 123):
                want_p, want = expectation("lasting_sum", p0, T, cfg, seed, 0)
                total += want["done_count"]
                flat, out = guarded_output(p0)
                got = ops.rollout(out, T, seed, flags=flags | force[0], record=("game_length",), defer_counts=True,
                                  workspace=ws, **kw)
                where = f"{cfg} {force[1]} b={b} T={T} seed={seed}"
                assert np.array_equal(host(out).view(np.int32), want_p.view(np.int32)), where
                assert guard_rows_intact(flat, out), where
                assert np.array_equal(host(got["game_length"]), want["game_length"]), where
            counts = ops.reduce_counts(ws, torch.zeros(T + 1, dtype=torch.int64, device="cuda"), b, T, (m, d),
                                       flags=flags | force[0])
            assert np.array_equal(host(counts).astype(np.uint64), total), f"{cfg} {force[1]} b={b} T={T}"
            assert not host(ws).any()
