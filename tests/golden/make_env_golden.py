"""
Generate tests/golden/env_game.npz by RUNNING the reference's own gym environments (hironaka/gym_env/hironaka_base.py,
hironaka_host_env.py, hironaka_agent_env.py) with its own hosts, `ChooseFirstAgent` / `RandomAgent` and ListPoints.  Runs
only where the reference checkout exists; the resulting .npz is what travels, and it holds data only.

The files are loaded one by one as make_golden.py does.  `gym` is not installed: the stand-in below (an `Env` to
inherit from, the four spaces as attribute holders, a version below 0.22) is put into sys.modules before the three
environment files load.  The registration glue of gym_env/__init__.py is not loaded.

Every game starts from reset(points=root): the reference draws roots with numpy's global generator, which is not what
is under test.  `RandomAgent` draws from `random`, seeded per game; its axes are recorded.

Layout (G games, S steps in all; tests/env_rules.py load_games unpacks it, META names the columns of `meta`):
    names      [G] str
    hosts      [5] str      the host keys;  agents [2] str
    meta       [G, 22] int64
    thresholds [G] float64  value_threshold where meta's has_threshold is 1
    roots      flat float64 the roots as given, root_rows * d each
    points     flat float64 the state behind every observation, rows * d each: after the reset, then after every
                            step.  The observation's points are this state cast to float32 and padded with -1 to m
                            rows; the generator checks that for every observation before it drops them
    rows       [S]          the points after the step
    action     [S]          host mode: the axis fed in (NONE_ACTION for None); agent mode: the subset as a bit mask
    coords     [S]          host mode: the observation's coords as a bit mask
    reward     [S] float64; stopped, exceed [S] uint8
    last       [S]          info["last_action_taken"]: host mode the pending list as a bit mask, agent mode the agent's
                            axis (-1 for None)

Games: seeded roots of dim 2..7 with 2..11 points, (10,3), (20,3), (19,7) and one (64,7).  Host mode: the five
deterministic hosts, configurations cycling through scale_observation x stop_after_invalid_move x improve_efficiency x
value_threshold in {None, 0.0, one that trips}; a quarter of the axes are illegal (None, -1, beyond d, outside the
pending list).  Agent mode: both agents, configurations cycling through MultiBinary / discrete actions x
stop_at_threshold x fixed penalty None / -7 x reward_based_on_point_reduction x improve_efficiency x scale_observation
x value_threshold, step_threshold 3..6; a fifth of the subsets are arbitrary masks, 0 and 1 coordinates included.
Every game goes on for a few steps after it stopped.  Targeted games: tests/env_rules.py searches for scaled states
that Newton would change (the rescale merged coordinates an ulp apart) and the reference is then fed illegal axes on
them, or reset onto them with improve_efficiency.

tests/env_rules.py follows every game move for move, bit for bit, before anything is written, and the coverage
conditions at the end of main() hold.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_env_golden.py
"""
import os
import random
import sys
import time
import types
import warnings

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from make_golden import OUT, _load, _pkg, load_reference  # noqa: E402
import env_rules as E  # noqa: E402
import play_rules as R  # noqa: E402

HOSTS = {"zeillinger": "Zeillinger", "all_coord": "AllCoordHost", "zeillinger_lex": "ZeillingerLex",
         "weak_spivakovsky": "WeakSpivakovsky", "weak_spivakovsky_min_hitting": "WeakSpivakovskyMinHitting"}
AGENTS = {"choose_first": "ChooseFirstAgent", "random": "RandomAgent"}
AFTER_STOP = 3


def install_gym():
    """a stand-in for the parts of gym the three environment files touch"""
    gym = types.ModuleType("gym")
    gym.__version__ = "0.21.0"
    spaces = types.ModuleType("gym.spaces")

    class Env:
        pass

    class Space:
        def __init__(self, *args, **kwargs):
            self.args, self.kwargs = args, kwargs

        def __class_getitem__(cls, item):
            return cls

    class Dict(Space, dict):
        def __init__(self, entries):
            dict.__init__(self, entries)

    gym.Env, gym.spaces = Env, spaces
    spaces.Space, spaces.Dict = Space, Dict
    for name in ("Box", "Discrete", "MultiBinary"):
        setattr(spaces, name, type(name, (Space,), {}))
    sys.modules["gym"], sys.modules["gym.spaces"] = gym, spaces


def load_envs():
    ref = load_reference()
    install_gym()
    _pkg("hironaka.gym_env")
    _load("hironaka.gym_env.hironaka_base", "hironaka/gym_env/hironaka_base.py")
    host = _load("hironaka.gym_env.hironaka_host_env", "hironaka/gym_env/hironaka_host_env.py")
    agent = _load("hironaka.gym_env.hironaka_agent_env", "hironaka/gym_env/hironaka_agent_env.py")
    return ref, host.HironakaHostEnv, agent.HironakaAgentEnv


def state_of(env):
    return np.asarray(env._points.points[0], np.float64).reshape(-1, env.dimension)


def check_obs(env, points, m):
    want = R.padded(state_of(env), m).astype(np.float32)
    assert points.dtype == np.float32 and np.array_equal(points, want)


def run_host(ref, HostEnv, g, choose):
    """g: an env_rules.Game with its configuration set; choose(t, coords, stopped) -> the action of step t"""
    env = HostEnv(getattr(ref.host, HOSTS[g.player_name])(), dimension=g.d, max_num_points=g.m, **reference_kwargs(g))
    try:
        obs, info = env.reset(points=[g.root.tolist()], return_info=True)
    except Exception:  # noqa: BLE001 -- a host without a move at the root
        return False
    check_obs(env, obs["points"], g.m)
    g.reset_state, g.reset_coords = state_of(env), E.coords_mask(np.nonzero(obs["coords"])[0])
    assert g.improve or (info["current_step"], info["exceed_threshold"]) == (env.current_step, env.exceed_threshold)
    g.reset_step, g.reset_exceed = env.current_step, int(env.exceed_threshold)
    left, t = None, 0
    while left is None or left > 0:
        a = choose(t, [int(c) for c in env._coords], left is not None)
        try:
            obs, reward, stopped, info = env.step(a)
        except Exception:  # noqa: BLE001 -- the reference's own failures: a host without a move
            g.raised, g.raised_action = 1, E.NONE_ACTION if a is None else a
            break
        check_obs(env, obs["points"], g.m)
        g.action.append(E.NONE_ACTION if a is None else a)
        g.states.append(state_of(env))
        g.coords.append(E.coords_mask(np.nonzero(obs["coords"])[0]))
        g.reward.append(float(reward)), g.stopped.append(bool(stopped)), g.exceed.append(bool(env.exceed_threshold))
        g.last.append(E.coords_mask(env.last_action_taken))
        if not g.improve:
            assert info["last_action_taken"] is env.last_action_taken and info["current_step"] == t + 2
        t += 1
        if left is not None:
            left -= 1
        elif stopped or t >= g.max_steps:
            left = AFTER_STOP if stopped else 0
    return True


def run_agent(ref, AgentEnv, g, masks):
    random.seed(g.seed)
    env = AgentEnv(getattr(ref.agent, AGENTS[g.player_name])(), dimension=g.d, max_num_points=g.m,
                   use_discrete_actions_for_host=bool(g.discrete), compressed_host_output=False, **reference_kwargs(g))
    obs = env.reset(points=[g.root.tolist()])
    check_obs(env, obs, g.m)
    g.reset_state, g.reset_coords, g.reset_step, g.reset_exceed = state_of(env), 0, env.current_step, 0
    left, t = None, 0
    while left is None or left > 0:
        mask = int(masks[t])
        action = mask if g.discrete else np.asarray([(mask >> k) & 1 for k in range(g.d)])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # `None in array` of shift_lst
            obs, reward, stopped, info = env.step(action)
        check_obs(env, obs, g.m)
        g.action.append(mask)
        g.states.append(state_of(env))
        g.coords.append(0)
        g.reward.append(float(reward)), g.stopped.append(bool(stopped)), g.exceed.append(bool(env.exceed_threshold))
        g.last.append(-1 if env.last_action_taken[0] is None else int(env.last_action_taken[0]))
        t += 1
        if left is not None:
            left -= 1
        elif stopped or t >= g.max_steps:
            left = AFTER_STOP if stopped else 0
    return True


def reference_kwargs(g):
    kw = g.config()
    kw.pop("dtype")
    return kw


def new_game(name, mode, player, root, m, cfg, seed, max_steps):
    g = E.Game()
    g.name, g.mode, g.player_name, g.seed, g.max_steps = name, mode, player, seed, max_steps
    g.root = np.asarray(root, np.float64)
    g.m, g.d, g.root_rows = m, g.root.shape[1], len(g.root)
    for k in ("scale", "improve", "stop_invalid", "stop_at_threshold", "fixed_penalty", "point_reduction", "discrete"):
        setattr(g, k, int(cfg.get(k, 0)))
    g.step_threshold = cfg.get("step_threshold", 1000)
    g.value_threshold = cfg.get("value_threshold")
    g.has_threshold = int(g.value_threshold is not None)
    g.raised, g.raised_action = 0, 0
    g.action, g.states, g.coords, g.reward, g.stopped, g.exceed, g.last = [], [], [], [], [], [], []
    return g


def check_follow(g):
    """the restatement must give the same game bit for bit, in float64"""
    g.steps, g.rows = len(g.action), [len(s) for s in g.states]
    for t, env, reward, stopped in E.follow(g):
        want = g.reset_state if t < 0 else g.states[t]
        assert np.array_equal(R.points_of(env.state), want), (g.name, t, R.points_of(env.state), want)
        if t < 0:
            assert env.current_step == g.reset_step and int(env.exceed_threshold) == g.reset_exceed, g.name
            if g.mode == 0:
                assert E.coords_mask(np.nonzero(env.obs_coords())[0]) == g.reset_coords, g.name
            continue
        assert reward == g.reward[t] and stopped == g.stopped[t] and env.exceed_threshold == g.exceed[t], (g.name, t)
        if g.mode == 0:
            assert E.coords_mask(np.nonzero(env.obs_coords())[0]) == g.coords[t], (g.name, t)
            assert E.coords_mask(env.last_action_taken) == g.last[t], (g.name, t)
        else:
            assert (-1 if env.last_action_taken is None else env.last_action_taken) == g.last[t], (g.name, t)


def host_chooser(rng, d, script=()):
    """scripted actions first; then an axis of the pending list, a quarter of the time an illegal one"""
    def choose(t, coords, stopped):
        if t < len(script):
            return script[t]
        if coords and rng.random() >= 0.25:
            return coords[int(rng.integers(len(coords)))]
        outside = [a for a in range(d) if a not in coords]
        pool = [None, -1, d, d + 3] + outside + outside
        return pool[int(rng.integers(len(pool)))]
    return choose


def agent_masks(rng, d, steps):
    legal = [v for v in range(1 << d) if bin(v).count("1") >= 2]
    masks = [int(rng.integers(0, 1 << d)) if rng.random() < 0.2 else legal[int(rng.integers(len(legal)))]
             for _ in range(steps)]
    if rng.random() < 0.3:
        masks[int(rng.integers(steps))] = 1 << int(rng.integers(d))
    if rng.random() < 0.15:
        masks[int(rng.integers(steps))] = 0
    return masks


def find_unreduced(rng, m, d, max_value, host, want):
    """(root, the legal axes that lead there, the state before its rescale) of games whose scaled state Newton would
    change, found with the restatement"""
    out = []
    while len(out) < want:
        root = rng.integers(0, max_value, (m, d))
        env = E.HostEnv(host, m, d, scale_observation=True)
        axes = []
        try:
            env.reset(root)
            for _ in range(14):
                if not env.coords:
                    break
                a = env.coords[int(rng.integers(len(env.coords)))]
                prev, coords = env.state, env.coords
                env.step(a)
                axes.append(a)
                if env.coords and E.unreduced(env.state):
                    out.append((root, list(axes), R.points_of(R.move(prev, coords, a)[0])))
                    break
        except E.NoMove:
            continue
    return out


def main():
    t0 = time.time()
    ref, HostEnv, AgentEnv = load_envs()
    host_keys, agent_keys = list(HOSTS), list(AGENTS)
    rng = np.random.default_rng(20261019)
    games, skipped = [], 0

    host_cfgs = [dict(scale=s, stop_invalid=i, improve=e, thr=t) for t in ("none", "zero", "trip") for e in (0, 1)
                 for i in (0, 1) for s in (1, 0)]
    agent_cfgs = [dict(discrete=a, stop_at_threshold=b, fixed_penalty=c, point_reduction=r, improve=e, scale=s, thr=t)
                  for t in ("none", "trip", "zero") for e in (0, 1) for r in (0, 1) for c in (0, 1) for b in (1, 0)
                  for a in (0, 1) for s in (1, 0)]
    counter = {"host": 0, "agent": 0, "seed": 0}

    def threshold(cfg, max_value):
        if cfg["thr"] == "none":
            return None
        if cfg["thr"] == "zero":
            return 0.0
        return 1.25 if cfg["scale"] else 1.5 * max_value

    def add_host(name, root, m, host, cfg, max_value, script=(), max_steps=7):
        nonlocal skipped
        cfg = dict(cfg, value_threshold=threshold(cfg, max_value)) if "thr" in cfg else cfg
        g = new_game(f"{name}_{host}_h{len(games)}", 0, host, root, m, cfg, 0, max_steps)
        if not run_host(ref, HostEnv, g, host_chooser(rng, g.d, script)):
            skipped += 1
            return None
        check_follow(g)
        games.append(g)
        return g

    def add_agent(name, root, m, agent, cfg, max_value, max_steps=7):
        cfg = dict(cfg, value_threshold=threshold(cfg, max_value), step_threshold=3 + counter["agent"] % 4)
        counter["seed"] += 1
        g = new_game(f"{name}_{agent}_a{len(games)}", 1, agent, root, m, cfg, counter["seed"], max_steps)
        run_agent(ref, AgentEnv, g, agent_masks(rng, g.d, max_steps + AFTER_STOP + 1))
        check_follow(g)
        games.append(g)

    def add(name, root, max_value, per_host, per_agent):
        m = len(root)
        for host in HOSTS:
            for _ in range(per_host):
                add_host(name, root, m, host, host_cfgs[counter["host"] % len(host_cfgs)], max_value)
                counter["host"] += 5  # coprime to 24: every configuration under every host
        for agent in AGENTS:
            for _ in range(per_agent):
                add_agent(name, root, m, agent, agent_cfgs[counter["agent"] % len(agent_cfgs)], max_value)
                counter["agent"] += 7

    for d in (2, 3, 4, 5, 6, 7):
        for j in range(2):
            add(f"d{d}_{j}", rng.integers(0, 10, (int(rng.integers(2, 12)), d)), 10, 3, 6)
    for j in range(2):
        add(f"m10_d3_{j}", rng.integers(0, 10, (10, 3)), 10, 2, 4)
        add(f"m20_d3_{j}", rng.integers(0, 30, (20, 3)), 30, 2, 4)
        add(f"m19_d7_{j}", rng.integers(0, 4, (19, 7)), 4, 2, 4)
    add("m64_d7", rng.integers(0, 3, (64, 7)), 3, 1, 2)

    # targeted: illegal axes on, and resets onto, scaled states that Newton would change
    for (m, d, max_value) in ((19, 7, 4), (10, 3, 10)):
        for j, host in enumerate(("zeillinger", "zeillinger_lex", "all_coord", "weak_spivakovsky",
                                  "weak_spivakovsky_min_hitting")):
            for k, (root, axes, pre) in enumerate(find_unreduced(rng, m, d, max_value, host, 2)):
                illegal = [[-1, None, d + 1], [None, d, -1]][k]
                add_host(f"unreduced_m{m}_d{d}_{k}", root, m, host, dict(scale=1, stop_invalid=k), max_value,
                         script=axes + illegal, max_steps=len(axes) + 5)
                if j < 3:
                    add_host(f"reset_unreduced_m{m}_d{d}_{k}", pre, m, host, dict(scale=1, improve=1, stop_invalid=0),
                             max_value, max_steps=4)

    # ---- the conditions that keep the fixture from being vacuous ----
    for g in games:
        g.player = (host_keys if g.mode == 0 else agent_keys).index(g.player_name)
        g.reset_rows = len(g.reset_state)
    c = E.coverage(games)
    print(c)
    assert c["illegal_on_unreduced"] >= 10 and c["post_reset_on_unreduced"] >= 3, c
    assert c["dim7_hosts"] == set(HOSTS), c
    # host mode has no step threshold and agent mode no invalid move: each mode shows its three causes
    assert c["causes"][0] == {"ended", "value", "invalid"} and c["causes"][1] == {"ended", "value", "steps"}, c
    assert (c["raised"] + skipped) * 50 <= len(games), (c["raised"], skipped)
    assert c["after_stop"] > 100 and c["outside_range"] > 100 and min(c["subsets"].values()) > 10, c
    assert {g.d for g in games} == {2, 3, 4, 5, 6, 7} and (64, 7) in {(g.m, g.d) for g in games}

    meta = np.asarray([[getattr(g, k) for k in E.META] for g in games], np.int64)
    cat = lambda rows, dt: np.asarray([v for r in rows for v in r], dt)  # noqa: E731
    rec = dict(
        names=np.asarray([g.name for g in games]), hosts=np.asarray(host_keys), agents=np.asarray(agent_keys), meta=meta,
        thresholds=np.asarray([g.value_threshold or 0.0 for g in games], np.float64),
        roots=np.concatenate([g.root.reshape(-1) for g in games]),
        points=np.concatenate([s.reshape(-1) for g in games for s in [g.reset_state] + g.states]),
        rows=cat([g.rows for g in games], np.int32), action=cat([g.action for g in games], np.int32),
        coords=cat([g.coords for g in games], np.int32), reward=cat([g.reward for g in games], np.float64),
        stopped=cat([g.stopped for g in games], np.uint8), exceed=cat([g.exceed for g in games], np.uint8),
        last=cat([g.last for g in games], np.int32))
    path = os.path.join(OUT, "env_game.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) <= 512 * 1024, os.path.getsize(path)
    print(f"wrote env_game.npz: {len(games)} games ({skipped} skipped at the root), {c['steps']} steps, "
          f"{os.path.getsize(path)} bytes in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
