"""gym_env, ops.env_step and hk_env_step against tests/env_rules.py, the plain restatement that test_env_rules.py pins to
the reference's own environments (tests/golden/env_game.npz).  Everything is bit for bit.

  * the fixture's games through gym_env's batched environments and through ops.env_step (float64, no auto reset),
    the steps after `stopped` included;
  * the branches of hk_env_step no other test executes, against env_rules.VecEnv: reposition, dim 4..6, every host at
    (19,7) and (64,7), improve_efficiency in agent mode, float32 over several episodes; the random agent's axes come
    from the numpy oracle's Philox (env_rules.philox_axis);
  * which lanes of a wave reset, forced per game;
  * game indices past 32 bits in both counter words of Philox.

Every case computes what the rules expect first and asserts from it that the case is not vacuous."""
import os

import numpy as np
import pytest
import torch

import env_rules as E
import play_rules as R
from hironaka_amd import ops
from hironaka_amd.agent import Agent, ChooseFirstAgent
from hironaka_amd.gym_env import HironakaAgentEnv, HironakaHostEnv
from hironaka_amd.host import MAX_HOST_DIM
from oracle import c_oracle as CO
from test_gpu_vec_env import HOSTS, cu, env_buffers, games_per_wave, guarded, guards_intact, mask_bits

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "env_game.npz")
TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}
DTYPES = [np.float64, np.float32]
SELECT_HOSTS = ("zeillinger_lex", "weak_spivakovsky", "weak_spivakovsky_min_hitting")  # served by hk_host_select


@pytest.fixture(scope="module")
def games():
    return E.load_games(np.load(GOLDEN))


def host(t):
    return t.cpu().numpy()


# ---- the fixture ----------------------------------------------------------------------------------------------------

class Group:
    """the games of one (shape, configuration) side by side; a game whose recording is over goes on with a filler
    action and is no longer looked at"""

    def __init__(self, gs):
        self.gs, self.g0 = gs, gs[0]
        self.n, self.m, self.d = len(gs), gs[0].m, gs[0].d
        self.steps = max(g.steps for g in gs)
        self.roots = np.full((self.n, self.m, self.d), -1.0)
        for i, g in enumerate(gs):
            self.roots[i, :g.root_rows] = g.root
        self.reset_points = np.stack([R.padded(g.reset_state, self.m) for g in gs])

    def live(self, t):
        return np.asarray([t < g.steps for g in self.gs])

    def actions(self, t):
        fill = -1 if self.g0.mode == 0 else 0
        a = [g.action[t] if t < g.steps else fill for g in self.gs]
        return np.asarray([-1 if x == E.NONE_ACTION else x for x in a], np.int32)

    def column(self, name, t, fill=0):
        return np.asarray([getattr(g, name)[t] if t < g.steps else fill for g in self.gs])

    def points(self, t):
        return np.stack([R.padded(g.states[t], self.m) if t < g.steps else np.full((self.m, self.d), -1.0)
                         for g in self.gs])


def groups_of(games, mode, d, keep=lambda g: True):
    out = {}
    for g in games:
        if g.mode == mode and g.d == d and keep(g):
            out.setdefault(g.key(), []).append(g)
    return [Group(gs) for gs in out.values()]


def coords_bits(masks, d):
    return mask_bits(np.asarray(masks, np.int64), d).astype(np.float64)


class RecordedAgent(Agent):
    """the axes the reference's RandomAgent drew, in order"""

    def __init__(self, group):
        self.group, self.t = group, 0

    def _get_actions(self, points, coords):
        axes = self.group.column("last", self.t)
        self.t += 1
        return cu(np.maximum(axes, 0).astype(np.int32))


@pytest.mark.parametrize("d", [2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("mode", [0, 1])
def test_fixture_through_gym_env(games, mode, d):
    """every recorded game on gym_env's batched environments: reset(points=roots), then step for step"""
    groups = groups_of(games, mode, d)
    assert groups
    checked = refused = 0
    for gr in groups:
        g0, n = gr.g0, gr.n
        kw = {k: v for k, v in g0.config().items() if k != "dtype"}
        kw.update(dimension=d, max_num_points=gr.m, num_envs=n)
        if mode == 0:
            env = HironakaHostEnv(HOSTS[g0.player_name](), **kw)
        else:
            agent = ChooseFirstAgent() if g0.player_name == "choose_first" else RecordedAgent(gr)
            env = HironakaAgentEnv(agent, use_discrete_actions_for_host=bool(g0.discrete), compressed_host_output=False,
                                   **kw)
        if mode == 0 and d > MAX_HOST_DIM and g0.player_name in SELECT_HOSTS:
            # gym_env asks hk_host_select for these hosts, which serves dim <= 6 and says so; hk_env_step runs them
            # in the kernel at dim 7: test_fixture_through_env_step plays these games
            with pytest.raises(ValueError, match="hk_host_select"):
                env.reset(points=gr.roots)
            refused += 1
            continue
        obs = env.reset(points=gr.roots)
        pts = obs["points"] if mode == 0 else obs
        assert pts.dtype == torch.float32 and np.array_equal(host(pts), gr.reset_points.astype(np.float32)), g0.name
        assert env.current_step == g0.reset_step
        assert host(env.exceed_threshold).tolist() == [bool(g.reset_exceed) for g in gr.gs], g0.name
        if mode == 0:
            assert np.array_equal(host(obs["coords"]), coords_bits([g.reset_coords for g in gr.gs], d)), g0.name
        for t in range(gr.steps):
            live, a = gr.live(t), gr.actions(t)
            action = cu(a) if mode == 0 or g0.discrete else cu(mask_bits(a, d))
            obs, reward, stopped, info = env.step(action)
            pts = obs["points"] if mode == 0 else obs
            label = (g0.name, t)
            assert np.array_equal(host(pts)[live], gr.points(t).astype(np.float32)[live]), label
            assert np.array_equal(host(env._points)[live], gr.points(t)[live]), label
            assert np.array_equal(host(reward)[live], gr.column("reward", t, 0.0)[live]), label
            assert np.array_equal(host(stopped)[live], gr.column("stopped", t)[live]), label
            assert np.array_equal(host(env.exceed_threshold)[live], gr.column("exceed", t)[live]), label
            if mode == 0:
                assert np.array_equal(host(obs["coords"])[live], coords_bits(gr.column("coords", t), d)[live]), label
                assert np.array_equal(host(env.last_action_taken)[live], coords_bits(gr.column("last", t), d)[live]), label
            else:
                assert np.array_equal(host(env.last_action_taken)[live], gr.column("last", t)[live]), label
            checked += int(live.sum())
    played = [gr for gr in groups if not (mode == 0 and d > MAX_HOST_DIM and gr.g0.player_name in SELECT_HOSTS)]
    assert checked == sum(g.steps for gr in played for g in gr.gs) > 0 and refused == len(groups) - len(played)
    if mode == 0 and d == 7:  # Zeillinger and AllCoordHost play dim 7 on gym_env, the unreduced (19,7) games included
        assert {gr.g0.player_name for gr in played} == {"zeillinger", "all_coord"}
        assert any(g.name.startswith("unreduced") for gr in played for g in gr.gs)


def launch_kwargs(mode, player, cfg, **more):
    """ops.env_step's keywords of an env_rules configuration"""
    kw = dict(mode="host" if mode == 0 else "agent", scale_observation=cfg.get("scale_observation", True),
              improve_efficiency=cfg.get("improve_efficiency", False), value_threshold=cfg.get("value_threshold"))
    if mode == 0:
        kw.update(host=player, invalid_move_penalty=cfg.get("invalid_move_penalty", -1e-3),
                  stop_after_invalid=cfg.get("stop_after_invalid_move", False))
    else:
        limit, fixed = cfg.get("step_threshold", 1000), cfg.get("fixed_penalty_crossing_threshold")
        kw.update(agent=player, step_threshold=limit, threshold_penalty=-float(limit) if fixed is None else float(fixed),
                  stop_at_threshold=cfg.get("stop_at_threshold", True),
                  point_reduction_reward=cfg.get("reward_based_on_point_reduction", False))
    kw.update(more)
    return kw


@pytest.mark.parametrize("d", [2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("mode", [0, 1])
def test_fixture_through_env_step(games, mode, d):
    """every recorded game on ops.env_step, float64, auto_reset=False, from the rules' reset state with class_io,
    step_count and episode set by hand.  Left out: value_threshold 0.0 (ops.env_step refuses it) and the reference's
    RandomAgent (the kernel draws its own axes; its rule is tested against Philox below)"""
    groups = groups_of(games, mode, d, lambda g: g.value_threshold != 0.0 and g.player_name != "random")
    assert groups
    checked = 0
    for gr in groups:
        g0, n, m = gr.g0, gr.n, gr.m
        envs = [g.make() for g in gr.gs]
        for env, g in zip(envs, gr.gs):
            env.reset(g.root)
        whole, v = env_buffers(n, m, d, torch.float64, mode == 0)
        bufs = {k: t for k, t in v.items() if k != "points"}
        v["points"].copy_(cu(np.stack([env.state for env in envs])))
        v["step_count"].fill_(g0.reset_step)
        v["episode"].zero_()
        if mode == 0:
            v["class_io"].copy_(cu(np.asarray([env.pending_class for env in envs], np.int32)))
        kw = launch_kwargs(mode, g0.player_name, {k: v_ for k, v_ in g0.config().items() if k != "dtype"},
                           auto_reset=False)
        for t in range(gr.steps):
            live, label = gr.live(t), (g0.name, t)
            v["action"].copy_(cu(gr.actions(t)))
            ops.env_step(v["points"], **bufs, **kw)
            assert np.array_equal(host(v["points"])[live], gr.points(t)[live]), label
            assert np.array_equal(host(v["obs_points"])[live], gr.points(t).astype(np.float32)[live]), label
            assert np.array_equal(host(v["reward"])[live], gr.column("reward", t, 0.0)[live]), label
            assert np.array_equal(host(v["stopped"])[live], gr.column("stopped", t)[live]), label
            assert np.array_equal(host(v["exceed"])[live], gr.column("exceed", t)[live]), label
            assert (v["step_count"] == g0.reset_step + t + 1).all() and (v["episode"] == 0).all(), label
            if mode == 0:
                assert np.array_equal(host(v["obs_coords"])[live], coords_bits(gr.column("coords", t), d)[live]), label
                cls = [E.class_id(E.mask_coords(c, d), d) if c else -1 for c in gr.column("last", t)]
                assert np.array_equal(host(v["class_io"])[live], np.asarray(cls)[live]), label
            else:
                assert np.array_equal(host(v["agent_axis"])[live], gr.column("last", t)[live]), label
            checked += int(live.sum())
        assert (v["final_points"] == 7.5).all()  # no auto reset: never written
        for name, (buf, fill) in whole.items():
            assert guards_intact(buf, fill), (g0.name, name)
    assert checked > 30


# ---- hk_env_step against env_rules.VecEnv ---------------------------------------------------------------------------

def philox_pick(agent_seed, d):
    def pick(coords, env):
        return E.philox_axis(agent_seed, env.gg, env.current_step - 1, E.coords_mask(coords), d)
    return pick


class Case:
    """one configuration of hk_env_step and its restatement.  player: a host key, "choose_first" or "random" """

    def __init__(self, mode, m, d, player, dtype, n, max_value, cfg=None, reposition=False, seed=7, agent_seed=4242,
                 game_offset=0, world_games=None, auto_reset=True):
        self.mode, self.m, self.d, self.player, self.dtype, self.n = mode, m, d, player, np.dtype(dtype), n
        self.max_value, self.cfg, self.reposition = max_value, dict(cfg or {}), reposition
        self.seed, self.agent_seed, self.game_offset, self.world_games = seed, agent_seed, game_offset, world_games
        self.auto_reset = auto_reset

    def make_env(self, b):
        if self.mode == 0:
            return E.HostEnv(self.player, self.m, self.d, dtype=self.dtype, **self.cfg)
        pick = "choose_first" if self.player == "choose_first" else philox_pick(self.agent_seed, self.d)
        return E.AgentEnv(pick, self.m, self.d, reposition=self.reposition, dtype=self.dtype, **self.cfg)

    def rules(self):
        return E.VecEnv(self.make_env, self.n, self.max_value, self.seed, self.game_offset, self.world_games,
                        self.auto_reset)

    def kwargs(self):
        more = dict(seed=self.seed, max_value=self.max_value, game_offset=self.game_offset,
                    world_games=self.world_games, auto_reset=self.auto_reset)
        if self.mode == 1:
            more.update(agent_seed=self.agent_seed, reposition=self.reposition)
        return launch_kwargs(self.mode, self.player, self.cfg, **more)

    def buffers(self):
        whole, v = env_buffers(self.n, self.m, self.d, TORCH[self.dtype], self.mode == 0)
        return whole, v, {k: t for k, t in v.items() if k != "points"}


def draw_actions(vec, rng):
    """host mode: mostly an axis of the game's pending list, a fifth of the time one of [-1, d]; agent mode: mostly a
    subset of 2 or more coordinates, a fifth of the time any mask"""
    d, out = vec.d, np.zeros(vec.batch, np.int32)
    legal = [v for v in range(1 << d) if bin(v).count("1") >= 2]
    for b, env in enumerate(vec.envs):
        wild = rng.random() < 0.2
        if vec.host_mode:
            out[b] = rng.integers(-1, d + 1) if wild or not env.coords else env.coords[rng.integers(len(env.coords))]
        else:
            out[b] = rng.integers(0, 1 << d) if wild else legal[rng.integers(len(legal))]
    return out


def compare(v, vec, label, prev_final=None):
    for key, want in (("points", vec.state), ("obs_points", vec.obs_points), ("step_count", vec.step_count),
                      ("episode", vec.episode), ("reward", vec.reward), ("stopped", vec.stopped.astype(np.uint8)),
                      ("exceed", vec.exceed.astype(np.uint8))):
        got = host(v[key])
        assert got.dtype == want.dtype, (label, key)
        bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
        assert not len(bad), (label, key, bad[:5], got[bad[0]], want[bad[0]])
    if vec.host_mode:
        assert np.array_equal(host(v["class_io"]), vec.pending), (label, host(v["class_io"]), vec.pending)
        assert np.array_equal(host(v["obs_coords"]), vec.obs_coords), label
    else:
        assert np.array_equal(host(v["agent_axis"]), vec.agent_axis), (label, host(v["agent_axis"]), vec.agent_axis)
    if prev_final is not None:  # the terminal observation of the games that stopped and were reset, and of no other
        w = vec.final_written
        assert np.array_equal(w, vec.stopped & vec.auto_reset)
        assert np.array_equal(host(v["final_points"])[w], vec.final_points[w]), label
        assert np.array_equal(host(v["final_points"])[~w], prev_final[0][~w]), label
        if vec.host_mode:
            assert (host(v["final_coords"])[w] == 0).all(), label
            assert np.array_equal(host(v["final_coords"])[~w], prev_final[1][~w]), label


def finals(v, host_mode):
    return host(v["final_points"]).copy(), host(v["final_coords"]).copy() if host_mode else None


def step_both(case, vec, v, bufs, actions, in_place, label):
    """one launch and one step of the rules on the same actions, compared"""
    v["action"].copy_(cu(actions))
    prev = finals(v, vec.host_mode)
    if in_place:
        ops.env_step(v["points"], **bufs, **case.kwargs())
    else:
        before = v["points"].clone()
        out_whole, out = guarded(tuple(v["points"].shape), v["points"].dtype, 7)
        ops.env_step(v["points"], out=out, **bufs, **case.kwargs())
        assert torch.equal(v["points"], before) and guards_intact(out_whole, 7), label
        v["points"].copy_(out)
    vec.step(actions)
    compare(v, vec, label, prev)


def run_case(case, steps, episode=-1, rng_seed=1):
    """reset_all, then `steps` steps alternating in place and with out=; returns the rules' VecEnv and the stops seen"""
    vec = case.rules()
    whole, v, bufs = case.buffers()
    v["episode"].copy_(cu(np.broadcast_to(np.asarray(episode, np.int32), (case.n,)).copy()))
    v["step_count"].zero_()
    ops.env_step(v["points"], reset_all=True, **{k: t for k, t in bufs.items() if k != "action"}, **case.kwargs())
    vec.reset(episode)
    compare(v, vec, "reset")
    assert (v["final_points"] == 7.5).all()
    rng, stops = np.random.default_rng(rng_seed), 0
    for t in range(steps):
        step_both(case, vec, v, bufs, draw_actions(vec, rng), t % 2 == 0, ("step", t))
        stops += int(vec.stopped.sum())
    for name, (buf, fill) in whole.items():
        assert guards_intact(buf, fill), name
    return vec, stops


def batch_of(m, d, dtype):
    return 3 * games_per_wave(m, d, np.dtype(dtype).itemsize) + 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("agent", ["choose_first", "random"])
@pytest.mark.parametrize("m,d,max_value", [(5, 3, 6), (19, 7, 4)])
def test_agent_reposition(m, d, max_value, agent, dtype):
    """HK_ENV_AGENT_REPOSITION: shift, reposition, Newton; also on a subset without an axis, as Agent.move does"""
    cfg = dict(step_threshold=4, scale_observation=d == 3, reward_based_on_point_reduction=True)
    case = Case(1, m, d, agent, dtype, batch_of(m, d, dtype), max_value, cfg, reposition=True)
    plain = Case(1, m, d, agent, dtype, case.n, max_value, cfg, reposition=False).rules()
    vec, stops = run_case(case, 6)
    plain.reset()
    rng = np.random.default_rng(1)
    plain.step(draw_actions(plain, rng))
    moved = case.rules()
    moved.reset()
    moved.step(draw_actions(moved, np.random.default_rng(1)))
    assert not np.array_equal(plain.state, moved.state)  # the flag matters on these games' first move
    assert stops > 0 and vec.episode.max() >= 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("d,host_name", [(4, "zeillinger_lex"), (5, "weak_spivakovsky"),
                                         (6, "weak_spivakovsky_min_hitting")])
def test_dims_four_to_six(d, host_name, mode, dtype):
    m = 7
    cfg = dict(scale_observation=True, value_threshold=1.5) if mode == 0 else \
        dict(step_threshold=5, fixed_penalty_crossing_threshold=-7)
    case = Case(mode, m, d, host_name if mode == 0 else "random", dtype, batch_of(m, d, dtype), 5, cfg)
    vec, stops = run_case(case, 6)
    assert stops > 0 and vec.episode.max() >= 1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("host_name", sorted(HOSTS))
@pytest.mark.parametrize("m,d,max_value", [(19, 7, 4), (64, 7, 3)])
def test_every_host_at_dim_seven(m, d, max_value, host_name, dtype):
    """the Bits128 instantiation and m = 64 under each of the five hosts"""
    cfg = dict(scale_observation=True, invalid_move_penalty=-0.125, value_threshold=1.75)
    case = Case(0, m, d, host_name, dtype, batch_of(m, d, dtype), max_value, cfg)
    vec, stops = run_case(case, 5)
    assert (vec.pending >= 0).any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,d,max_value", [(5, 3, 3), (20, 3, 20)])
def test_agent_improve_efficiency(m, d, max_value, dtype):
    """the fresh state without its second Newton, in agent mode"""
    cfg = dict(step_threshold=3, improve_efficiency=True, scale_observation=True)
    case = Case(1, m, d, "choose_first", dtype, batch_of(m, d, dtype), max_value, cfg)
    vec, stops = run_case(case, 7)
    assert stops > 0 and vec.episode.max() >= 2


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scale,thr", [(True, 1.25), (False, 3.0)])
def test_float32_several_episodes(scale, thr, mode):
    """float32 over 8 steps and at least 3 episodes, with a value threshold that trips"""
    m, d = 5, 3
    cfg = dict(scale_observation=scale, value_threshold=thr)
    if mode == 1:
        cfg.update(step_threshold=6)
    case = Case(mode, m, d, "zeillinger" if mode == 0 else "random", np.float32, batch_of(m, d, np.float32), 3, cfg)
    vec, stops = run_case(case, 8)
    assert vec.episode.max() >= 2 and stops > 0


# ---- which lanes of a wave reset -------------------------------------------------------------------------------------

def reset_pattern(gpb, tail):
    """blocks: no game, every game, lane 0, the last lane, alternating lanes; then a partial block whose last game
    resets"""
    want = np.zeros(5 * gpb + tail, bool)
    want[gpb:2 * gpb] = True
    want[2 * gpb] = True
    want[4 * gpb - 1] = True
    want[4 * gpb:5 * gpb:2] = True
    want[-1] = True
    return want


def pattern_setup(mode, m, d, max_value, dtype):
    """(case, the rules loaded with its inputs, states, step_count, pending, actions, the games meant to reset).  The
    states are fresh states of the generator's stream in which only the intended games stop: at least 2 points, and in
    host mode a legal axis that does not end the game.  Agent mode: step_count is one below step_threshold where a
    game shall reset, and no game gets a subset.  Host mode: axis -1 under stop_after_invalid where it shall reset"""
    gpb = games_per_wave(m, d, np.dtype(dtype).itemsize)
    want = reset_pattern(gpb, 3)
    n = len(want)
    cfg = dict(step_threshold=5, scale_observation=True) if mode == 1 else \
        dict(scale_observation=True, invalid_move_penalty=-0.125)
    player = "choose_first" if mode == 1 else "zeillinger"
    pool = Case(mode, m, d, player, dtype, 4 * n, max_value, cfg).rules()
    case = Case(mode, m, d, player, dtype, n, max_value, cfg if mode == 1 else dict(cfg, stop_after_invalid_move=True))
    pool.reset()
    picked, axes = [], []
    for b, env in enumerate(pool.envs):
        if len(picked) == n or E.num_points(env.state) < 2:
            continue
        if mode == 0:
            trial = case.make_env(0)
            trial.load(env.state, 1)
            trial.set_pending_class(pool.pending[b])
            axis = trial.coords[0] if trial.coords else -1
            if axis < 0 or trial.step(axis)[2]:
                continue
            axes.append(axis)
        picked.append(b)
    assert len(picked) == n
    states = pool.state[picked]
    if mode == 1:
        step_count, pending, actions = np.where(want, 4, 0).astype(np.int32), None, np.zeros(n, np.int32)
    else:
        step_count, pending = np.ones(n, np.int32), pool.pending[picked]
        actions = np.where(want, -1, np.asarray(axes)).astype(np.int32)
    vec = case.rules()
    vec.load(states, step_count, 0, pending)
    return case, vec, states, step_count, pending, actions, want


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("m,d,max_value,dtype,per_block", [(5, 3, 20, np.float64, 64), (64, 7, 3, np.float64, 17),
                                                            (64, 7, 3, np.float32, 35)])
def test_reset_patterns(m, d, max_value, dtype, per_block, mode):
    """which lanes of a wave reset is chosen per game, and the rules' outcome shows that every pattern occurred: no
    game of a block, every game, lane 0 only, the last lane only, alternating lanes, the last game of a partial block"""
    assert games_per_wave(m, d, np.dtype(dtype).itemsize) == per_block
    case, vec, states, step_count, pending, actions, want = pattern_setup(mode, m, d, max_value, dtype)
    whole, v, bufs = case.buffers()
    v["points"].copy_(cu(states))
    v["step_count"].copy_(cu(step_count))
    v["episode"].zero_()
    if mode == 0:
        v["class_io"].copy_(cu(pending))
    step_both(case, vec, v, bufs, actions, True, "pattern")
    assert np.array_equal(vec.stopped, want), np.nonzero(vec.stopped != want)[0]
    assert np.array_equal(vec.episode, want.astype(np.int32))
    assert (host(v["final_points"])[~want] == 7.5).all()
    for name, (buf, fill) in whole.items():
        assert guards_intact(buf, fill), name


# ---- game indices past 32 bits ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("game_offset,world_games,episode", [
    (2 ** 32 - 3, None, -1), ((1 << 33) + 5, None, -1), (0, 2 ** 31 + 1, [-1, 0, 1, 2, -1, 0, 1, 2])])
def test_game_indices_past_32_bits(game_offset, world_games, episode, mode):
    """both counter words of Philox carry the game index: fresh states against the C oracle's generator at that index,
    reduced by the rules; the random agent's axes against the numpy oracle's Philox"""
    m, d, n, max_value, seed = 5, 3, 8, 6, 13
    cfg = dict(scale_observation=True) if mode == 0 else dict(step_threshold=3)
    case = Case(mode, m, d, "zeillinger" if mode == 0 else "random", np.float64, n, max_value, cfg, seed=seed,
                game_offset=game_offset, world_games=world_games)
    vec, stops = run_case(case, 5, episode=episode)
    assert stops > 0
    # the states of the first reset straight from the C oracle's stream
    fresh = case.rules()
    fresh.reset(episode)
    index = [fresh.game_index(b, fresh.episode[b]) for b in range(n)]
    assert max(index) >= 2 ** 32 and (world_games is None or min(index[2:4]) >= 2 ** 32)
    high = 0
    for b, gg in enumerate(index):
        raw = CO.generate_points(1, m, d, max_value, seed, game_offset=gg, dtype=np.float64, stages=0)[0]
        assert np.array_equal(raw, E.generator_root(m, d, max_value, seed, gg))
        env = case.make_env(b)
        env.reset(raw)
        assert np.array_equal(env.state, fresh.state[b]), b
        high += gg >= 2 ** 32 and not np.array_equal(raw, E.generator_root(m, d, max_value, seed, gg % 2 ** 32))
    assert high > 0  # the high word is not ignored


@pytest.mark.parametrize("thr", [0.0, -0.5])
def test_value_threshold_at_or_below_zero(thr):
    """the environments test `is not None`: gym_env stops at its reset as the reference does, and hk_env_step, which
    would read the value as "none", refuses it"""
    env = HironakaHostEnv(HOSTS["zeillinger"](), num_envs=3, dimension=3, max_num_points=5, max_value=6,
                          value_threshold=thr)
    obs = env.reset(points=np.asarray([[[1, 2, 3], [3, 2, 1], [2, 2, 2], [0, 5, 1], [4, 0, 4]]] * 3))
    assert env.exceed_threshold.all() and (obs["coords"] == 0).all()
    rule = E.HostEnv("zeillinger", 5, 3, value_threshold=thr)
    rule.reset(np.asarray([[1, 2, 3], [3, 2, 1]]))
    assert rule.exceed_threshold and not rule.coords
    _, v = env_buffers(3, 5, 3, torch.float64, True)
    bufs = {k: t for k, t in v.items() if k != "points"}
    with pytest.raises(ValueError, match="gym_env"):
        ops.env_step(v["points"], **bufs, mode="host", host="zeillinger", max_value=6, value_threshold=thr)
