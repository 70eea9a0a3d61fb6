"""tests/env_rules.py pinned to the reference's own gym environments: every game of tests/golden/env_game.npz
(make_env_golden.py: recorded by running hironaka/gym_env's HironakaHostEnv / HironakaAgentEnv) is followed move for
move, bit for bit, and the conditions that keep the fixture from being vacuous are asserted again from its arrays."""
import os

import numpy as np
import pytest

import env_rules as E
import play_rules as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "env_game.npz")


@pytest.fixture(scope="module")
def games():
    return E.load_games(np.load(GOLDEN))


def mask_of(vec):
    return E.coords_mask(np.nonzero(vec)[0])


def test_every_recorded_game_bit_for_bit(games):
    steps = 0
    for g in games:
        for t, env, reward, stopped in E.follow(g):
            want = g.reset_state if t < 0 else g.states[t]
            assert env.state.dtype == np.float64
            assert np.array_equal(R.points_of(env.state), want), (g.name, t)
            assert np.array_equal(env.obs_points(), R.padded(want, g.m).astype(np.float32)), (g.name, t)
            if t < 0:
                assert env.current_step == g.reset_step and int(env.exceed_threshold) == g.reset_exceed, g.name
                assert g.mode == 1 or mask_of(env.obs_coords()) == g.reset_coords, g.name
                continue
            steps += 1
            assert env.current_step == g.reset_step + t + 1, (g.name, t)
            assert reward == g.reward[t] and stopped == g.stopped[t], (g.name, t, reward, g.reward[t])
            assert env.exceed_threshold == g.exceed[t], (g.name, t)
            if g.mode == 0:
                assert mask_of(env.obs_coords()) == g.coords[t], (g.name, t)
                assert E.coords_mask(env.last_action_taken) == g.last[t], (g.name, t)
            else:
                assert (-1 if env.last_action_taken is None else env.last_action_taken) == g.last[t], (g.name, t)
    assert steps == sum(g.steps for g in games) > 2000


def test_float32_follows_the_same_games_in_its_own_arithmetic(games):
    """float32 is the restatement's second dtype: on the games without a rescale every value is a small integer, so
    float32 must give the recorded states exactly"""
    seen = 0
    for g in games:
        if g.scale or g.raised:
            continue
        for t, env, reward, stopped in E.follow(g, np.float32):
            want = g.reset_state if t < 0 else g.states[t]
            assert env.state.dtype == np.float32
            assert np.array_equal(R.points_of(env.state).astype(np.float64), want), (g.name, t)
            if t >= 0:
                assert reward == g.reward[t] and stopped == g.stopped[t] and env.exceed_threshold == g.exceed[t]
                seen += 1
    assert seen > 500


def test_an_illegal_host_move_touches_nothing(games):
    """the reference's rule the product had wrong: the state after an illegal host-mode move is the state before it,
    also where Newton would have changed it"""
    kept = 0
    for g in games:
        if g.mode != 0:
            continue
        state, coords = g.reset_state, g.reset_coords
        for t in range(g.steps):
            a = g.action[t]
            if not (0 <= a < g.d and (coords >> a) & 1):
                assert np.array_equal(g.states[t], state), (g.name, t)
                kept += g.scale and E.unreduced(R.padded(state, g.m))
            state, coords = g.states[t], g.last[t]
    assert kept >= 10


def test_threshold_zero_exceeds_at_the_reset(games):
    zero = [g for g in games if g.has_threshold and g.value_threshold == 0.0]
    assert len(zero) > 20
    for g in zero:
        positive = bool((g.reset_state > 0).any())
        if g.mode == 0:
            assert g.reset_exceed == int(positive) and (not positive or g.reset_coords == 0), g.name
        elif g.steps:
            assert g.exceed[0] == bool((g.states[0] > 0).any()), g.name


def test_fixture_is_not_vacuous(games):
    c = E.coverage(games)
    assert c["illegal_on_unreduced"] >= 10 and c["post_reset_on_unreduced"] >= 3, c
    assert c["dim7_hosts"] == {"zeillinger", "all_coord", "zeillinger_lex", "weak_spivakovsky",
                               "weak_spivakovsky_min_hitting"}, c
    # host mode has no step threshold and agent mode no invalid move: each mode shows its three stop causes
    assert c["causes"][0] == {"ended", "value", "invalid"} and c["causes"][1] == {"ended", "value", "steps"}, c
    assert c["raised"] * 50 <= c["games"], c
    assert c["after_stop"] > 100 and c["outside_range"] > 100 and min(c["subsets"].values()) > 10, c
    assert {g.d for g in games} == {2, 3, 4, 5, 6, 7}
    assert {(64, 7), (19, 7), (20, 3)} <= {(g.m, g.d) for g in games}
    assert os.path.getsize(GOLDEN) <= 512 * 1024
    host, agent = [g for g in games if g.mode == 0], [g for g in games if g.mode == 1]
    for key in ("scale", "stop_invalid", "improve"):
        assert {getattr(g, key) for g in host} == {0, 1}, key
    for key in ("scale", "improve", "discrete", "stop_at_threshold", "fixed_penalty", "point_reduction"):
        assert {getattr(g, key) for g in agent} == {0, 1}, key
    assert {g.step_threshold for g in agent} == {3, 4, 5, 6}
    assert {g.player_name for g in agent} == {"choose_first", "random"}
    for group in (host, agent):  # None, 0.0 and a value that trips after the first step
        assert any(not g.has_threshold for g in group) and any(g.value_threshold == 0.0 for g in group)
        assert any(g.has_threshold and g.value_threshold > 0 and any(g.exceed) and not g.exceed[0] for g in group)


def test_vec_env_rule_episodes_and_counters():
    """VecEnv's own rule on the CPU: episode e of game b is game game_offset + e * world_games + b of the generator's
    stream reduced as reset does; final_* only for a game that stopped"""
    m, d, n = 5, 3, 6
    cfg = dict(scale_observation=True, stop_after_invalid_move=True)
    vec = E.VecEnv(lambda b: E.HostEnv("zeillinger", m, d, **cfg), n, max_value=4, seed=3, game_offset=10, world_games=100)
    vec.reset()
    assert (vec.episode == 0).all() and (vec.step_count == 1).all()
    for b in range(n):
        one = E.HostEnv("zeillinger", m, d, **cfg)
        one.reset(E.generator_root(m, d, 4, 3, 10 + b))
        assert np.array_equal(vec.state[b], one.state)
    before = vec.final_points.copy()
    act = np.asarray([-1, 0, 9, 1, -1, 2], np.int32)
    vec.step(act)
    assert vec.stopped[[0, 2, 4]].all() and (vec.episode[[0, 2, 4]] == 1).all() and (vec.step_count[[0, 2, 4]] == 1).all()
    for b in (0, 2, 4):
        one = E.HostEnv("zeillinger", m, d, **cfg)
        one.reset(E.generator_root(m, d, 4, 3, 10 + 100 + b))
        assert np.array_equal(vec.state[b], one.state) and vec.final_written[b]
    keep = ~vec.stopped
    assert np.array_equal(vec.final_points[keep], before[keep]) and not vec.final_written[keep].any()
    assert (vec.step_count[keep] == 2).all() and (vec.episode[keep] == 0).all()
