"""The gym environments restated in plain numpy, one environment per game: hironaka/gym_env/hironaka_base.py:86-114
(reset), hironaka_host_env.py:41-74 and hironaka_agent_env.py:44-80 (step) followed line by line, on top of
tests/play_rules.py (move, reduce, rescale, exceeds) and tests/search_rules.py (the five deterministic hosts).  Nothing
here comes from hironaka_amd: test_env_rules.py pins this module to the fixture made by running the reference's own
environments (tests/golden/make_env_golden.py), and the GPU tests compare gym_env, vec_env and hk_env_step with it.

Everything runs in the dtype it is given, float64 (the reference's python floats) or float32.  A state is play_rules':
an [m, d] array, the points sorted descending and packed to the front, padding -1.

What the reference does and this module keeps:
  * a host-mode move whose axis is not in the pending list (None, an axis outside [0, d), any axis once the game has
    stopped) touches nothing: no shift and no Newton.  The state is looked at as it is, then rescaled;
  * an agent-mode subset of fewer than 2 coordinates gives no axis, yet Agent.move still runs its Newton;
  * value_threshold is tested with `is not None`: at 0.0 every state with a positive coordinate exceeds;
  * the thresholds are tested on the state before the step's rescale.

The one rule that is vec_env's own (VecEnv below): episode e of game b is game game_offset + e * world_games + b of the
generator's stream (oracle/np_oracle.py random_ints), reduced as reset does; a game that stopped hands out its
terminal observation and starts its next episode within the same step, as include/hironaka_hip_env.h states."""
import numpy as np

import play_rules as R
from search_rules import class_id, host_list

STREAM_PLAY_AGENT = 3


class NoMove(Exception):
    """the host has no list for a state that is still running (where the reference's hitting-set hosts misbehave)"""


def mask_coords(mask, d):
    return [k for k in range(d) if (int(mask) >> k) & 1]


def coords_mask(coords):
    return sum(1 << int(k) for k in coords)


def num_points(state):
    return int((np.asarray(state)[:, 0] >= 0).sum())


def philox_axis(agent_seed, gg, t, mask, d):
    """hk_env_step's random agent: word 0 of Philox4x32-10 keyed by agent_seed at counter (gg low, gg high, t, stream 3)
    picks the j-th coordinate of the subset in ascending order, j = (word * |subset|) >> 32"""
    from oracle import np_oracle as NO
    sub = mask_coords(mask, d)
    word = NO.philox4x32(gg & 0xFFFFFFFF, (gg >> 32) & 0xFFFFFFFF, t, STREAM_PLAY_AGENT, agent_seed)[0]
    return sub[(int(word) * len(sub)) >> 32]


def generator_root(m, d, max_value, seed, gg):
    """the integers the generator draws for game gg of its stream, [m, d]"""
    from oracle import np_oracle as NO
    return NO.random_ints(1, m, d, max_value, seed, game_offset=gg)[0]


class Base:
    def __init__(self, m, d, dtype=np.float64, value_threshold=None, step_threshold=1000,
                 fixed_penalty_crossing_threshold=None, stop_at_threshold=True, improve_efficiency=False,
                 scale_observation=True, reward_based_on_point_reduction=False):
        self.m, self.d, self.dtype = m, d, np.dtype(dtype)
        self.value_threshold, self.step_threshold = value_threshold, step_threshold
        self.fixed_penalty_crossing_threshold = fixed_penalty_crossing_threshold
        self.stop_at_threshold, self.improve_efficiency = stop_at_threshold, improve_efficiency
        self.scale_observation = scale_observation
        self.reward_based_on_point_reduction = reward_based_on_point_reduction
        self.state, self.coords = None, []
        self.current_step, self.exceed_threshold, self.last_action_taken = 0, False, None

    @property
    def ended(self):
        return num_points(self.state) <= 1

    def _exceeds(self):
        return self.value_threshold is not None and R.exceeds(self.state, self.value_threshold)

    def reset(self, points):
        """hironaka_base.py:86-114 with `points` given: rows with a negative first coordinate are padding"""
        pts = R.points_of(np.asarray(points, dtype=self.dtype))
        self.state = R.reduce(R.padded(pts, self.m))
        if self.scale_observation:
            self.state = R.rescale(self.state)
        self.current_step, self.exceed_threshold, self.last_action_taken = 0, False, None
        if not self.improve_efficiency:
            self.state = R.reduce(self.state)
        self._post_reset_update()
        return self.obs()

    def load(self, state, current_step=0):
        """take a state as it is (what ops.env_step is handed)"""
        self.state = np.array(state, dtype=self.dtype)
        self.current_step = current_step

    def obs_points(self):
        return self.state.astype(np.float32)


class HostEnv(Base):
    def __init__(self, host, m, d, invalid_move_penalty=-1e-3, stop_after_invalid_move=False, **kwargs):
        super().__init__(m, d, **kwargs)
        self.host, self.raise_no_move = host, True  # (hk_env_step: a host without a list leaves no pending subset)
        self.invalid_move_penalty, self.stop_after_invalid_move = invalid_move_penalty, stop_after_invalid_move

    def _post_reset_update(self):
        self.step(None)

    def step(self, action):
        self.current_step += 1
        stopped, reward = False, 0.0
        if action is not None and int(action) in self.coords:
            self.state, _ = R.move(self.state, self.coords, int(action))
            reward += 1.0 if not self.ended else 0.0
        else:
            stopped |= bool(self.stop_after_invalid_move)
            reward += self.invalid_move_penalty
        stopped |= self.ended
        self.exceed_threshold = self._exceeds()
        stopped |= self.exceed_threshold
        if stopped:
            self.coords = []
        else:
            got = host_list(self.host, self.state)
            if got is None and self.raise_no_move:
                raise NoMove(self.host)
            self.coords = [int(c) for c in got or []]
        if self.scale_observation:
            self.state = R.rescale(self.state)
        self.last_action_taken = self.coords
        return self.obs(), float(reward), bool(stopped)

    def obs_coords(self):
        out = np.zeros(self.d)
        if not self.ended and len(self.coords) >= 2:
            out[self.coords] = 1
        return out

    def obs(self):
        return self.obs_points(), self.obs_coords()

    @property
    def pending_class(self):
        return class_id(self.coords, self.d) if len(self.coords) >= 2 else -1

    def set_pending_class(self, cls):
        self.coords = R.subset_of_class(int(cls), self.d) or []


class AgentEnv(Base):
    """agent: "choose_first", or pick(coords, env) -> axis (a recorded or a Philox random agent)"""

    def __init__(self, agent, m, d, reposition=False, **kwargs):
        super().__init__(m, d, **kwargs)
        self.pick = (lambda coords, env: min(coords)) if agent == "choose_first" else agent
        self.reposition = reposition

    def _post_reset_update(self):
        pass

    def step(self, mask):
        """mask: the host's subset as a bit mask (MultiBinary read as bits, a discrete code as it is)"""
        self.current_step += 1
        stopped, reward = False, 0.0
        coords = mask_coords(mask, self.d)
        before = num_points(self.state)
        axis = int(self.pick(coords, self)) if len(coords) > 1 else None
        if axis is not None:
            self.state, _ = R.move(self.state, coords, axis, self.reposition)
        else:  # Agent.move: shift_lst skips the game, reposition and Newton run
            pts = R.points_of(self.state)
            if self.reposition:
                pts = pts - pts.min(0)
            self.state = R.reduce(R.padded(pts, self.m))
        self.last_action_taken = axis
        stopped |= self.ended
        self.exceed_threshold = self._exceeds()
        if self.stop_at_threshold and (self.current_step >= self.step_threshold or self.exceed_threshold):
            stopped = True
            if self.fixed_penalty_crossing_threshold is None:
                reward -= self.step_threshold
            else:
                reward += self.fixed_penalty_crossing_threshold
        if self.scale_observation:
            self.state = R.rescale(self.state)
        if self.reward_based_on_point_reduction:
            reward += before - num_points(self.state)
        reward += 1 if self.ended else 0
        return self.obs(), float(reward), bool(stopped)

    def obs(self):
        return self.obs_points()


# ---- vec_env's own rule: per-game episodes from the generator's stream ------------------------------------------------

class VecEnv:
    """B environments stepped together as hk_env_step steps them (include/hironaka_hip_env.h).  make(b) -> a HostEnv or
    an AgentEnv; an AgentEnv's pick may read env.gg (the game's index in both streams) and env.current_step.  Arrays
    hold what the launch leaves: state, obs_points, obs_coords / agent_axis, reward, stopped, exceed, step_count,
    episode, pending (host mode: the class id, -1 for none), final_points / final_coords (written only for a game that
    stopped and was reset)."""

    def __init__(self, make, batch, max_value, seed, game_offset=0, world_games=None, auto_reset=True):
        self.envs = [make(b) for b in range(batch)]
        for env in self.envs:
            env.raise_no_move = False
        e0 = self.envs[0]
        self.host_mode = isinstance(e0, HostEnv)
        self.batch, self.m, self.d, self.dtype = batch, e0.m, e0.d, e0.dtype
        self.max_value, self.seed, self.game_offset = max_value, seed, game_offset
        self.world_games = batch if world_games is None else world_games
        self.auto_reset = auto_reset
        n, m, d = batch, self.m, self.d
        self.episode = np.full(n, -1, np.int32)
        self.step_count = np.zeros(n, np.int32)
        self.reward, self.stopped, self.exceed = np.zeros(n), np.zeros(n, bool), np.zeros(n, bool)
        self.state = np.full((n, m, d), -1, self.dtype)
        self.obs_points = np.full((n, m, d), -1, np.float32)
        self.obs_coords, self.final_coords = np.zeros((n, d)), np.zeros((n, d))
        self.final_points = np.zeros((n, m, d), np.float32)
        self.final_written = np.zeros(n, bool)  # by the latest step
        self.agent_axis = np.full(n, -1, np.int32)
        self.pending = np.full(n, -1, np.int32)

    def game_index(self, b, episode):
        return (self.game_offset + int(episode) * self.world_games + b) % (1 << 64)

    def load(self, states, step_count, episode, pending=None):
        """the inputs of an ops.env_step launch, taken as they are"""
        self.step_count[:], self.episode[:] = step_count, episode
        for b, env in enumerate(self.envs):
            env.load(states[b], int(self.step_count[b]))
            if self.host_mode:
                env.set_pending_class(-1 if pending is None else pending[b])
            self._collect(b)

    def _collect(self, b):
        env = self.envs[b]
        self.state[b], self.obs_points[b] = env.state, env.obs_points()
        self.step_count[b] = env.current_step
        if self.host_mode:
            self.obs_coords[b], self.pending[b] = env.obs_coords(), env.pending_class

    def _fresh(self, b):
        self.episode[b] += 1
        env = self.envs[b]
        gg = self.game_index(b, self.episode[b])
        env.gg = gg
        env.reset(generator_root(self.m, self.d, self.max_value, self.seed, gg))

    def reset(self, episode=-1):
        """HK_ENV_RESET_ALL: every game starts the episode after `episode` (per game, or one number)"""
        self.episode[:] = episode
        for b in range(self.batch):
            self._fresh(b)
            self._collect(b)
        self.reward[:], self.stopped[:], self.exceed[:] = 0, False, False
        self.final_written[:] = False

    def step(self, actions):
        self.final_written[:] = False
        for b, env in enumerate(self.envs):
            env.gg = self.game_index(b, self.episode[b])
            _, self.reward[b], self.stopped[b] = env.step(int(actions[b]))
            self.exceed[b] = env.exceed_threshold
            if not self.host_mode:
                self.agent_axis[b] = -1 if env.last_action_taken is None else env.last_action_taken
            self._collect(b)
            if self.stopped[b] and self.auto_reset:
                self.final_points[b] = self.obs_points[b]
                self.final_coords[b] = 0.0
                self.final_written[b] = True
                self._fresh(b)
                self._collect(b)


# ---- the fixture tests/golden/env_game.npz (make_env_golden.py) -------------------------------------------------------

META = ("mode", "m", "d", "player", "scale", "improve", "stop_invalid", "stop_at_threshold", "fixed_penalty",
        "point_reduction", "step_threshold", "discrete", "seed", "has_threshold", "root_rows", "steps", "raised",
        "reset_step", "reset_exceed", "reset_rows", "reset_coords", "raised_action")
PENALTY = -0.125  # invalid_move_penalty of every recorded host game
NONE_ACTION = -(1 << 20)  # the recorded code of step(None)


class Game:
    """one recorded game: the META fields, value_threshold (None or a float), root [root_rows, d] float64,
    reset_state [reset_rows, d] and per step: action, state, coords (the observation's subset as a bit mask, host mode),
    reward, stopped, exceed, last (host mode: last_action_taken as a bit mask; agent mode: the agent's axis, -1 for
    None)"""

    def config(self, dtype=np.float64):
        kw = dict(dtype=dtype, value_threshold=self.value_threshold, step_threshold=self.step_threshold,
                  fixed_penalty_crossing_threshold=-7 if self.fixed_penalty else None,
                  stop_at_threshold=bool(self.stop_at_threshold), improve_efficiency=bool(self.improve),
                  scale_observation=bool(self.scale), reward_based_on_point_reduction=bool(self.point_reduction))
        if self.mode == 0:
            kw.update(invalid_move_penalty=PENALTY, stop_after_invalid_move=bool(self.stop_invalid))
        return kw

    def key(self):
        """games with the same key can share one batched environment"""
        return tuple(getattr(self, k) for k in META[:12]) + (self.value_threshold,)

    def make(self, dtype=np.float64):
        if self.mode == 0:
            return HostEnv(self.player_name, self.m, self.d, **self.config(dtype))
        pick = "choose_first"
        if self.player_name == "random":  # the recorded axis of the step
            axes = list(self.last) + [-1]
            pick = lambda coords, env: axes[env.current_step - 1]  # noqa: E731
        return AgentEnv(pick, self.m, self.d, **self.config(dtype))


def load_games(npz):
    hosts, agents = [str(h) for h in npz["hosts"]], [str(a) for a in npz["agents"]]
    at = {"roots": 0, "points": 0}

    def take(key, rows, d):
        out = npz[key][at[key]: at[key] + rows * d].reshape(rows, d)
        at[key] += rows * d
        return out

    games, s = [], 0
    for name, row, thr in zip(npz["names"], npz["meta"].tolist(), npz["thresholds"].tolist()):
        g = Game()
        g.name = str(name)
        for k, v in zip(META, row):
            setattr(g, k, v)
        g.player_name = (hosts if g.mode == 0 else agents)[g.player]
        g.value_threshold = thr if g.has_threshold else None
        g.root = take("roots", g.root_rows, g.d)
        g.reset_state = take("points", g.reset_rows, g.d)
        n = g.steps
        g.action = npz["action"][s: s + n].tolist()
        g.rows = npz["rows"][s: s + n].tolist()
        g.states = [take("points", c, g.d) for c in g.rows]
        g.coords = npz["coords"][s: s + n].tolist()
        g.reward = npz["reward"][s: s + n].tolist()
        g.stopped = npz["stopped"][s: s + n].astype(bool).tolist()
        g.exceed = npz["exceed"][s: s + n].astype(bool).tolist()
        g.last = npz["last"][s: s + n].tolist()
        s += n
        games.append(g)
    assert s == len(npz["action"]) and at["roots"] == len(npz["roots"]) and at["points"] == len(npz["points"])
    return games


def follow(g, dtype=np.float64):
    """play a recorded game with this module and yield per step (t, env, obs, reward, stopped); t = -1 is the reset.
    The game ends where the reference raised: there this module must raise NoMove"""
    env = g.make(dtype)
    env.reset(g.root)
    yield -1, env, None, None
    for t in range(g.steps):
        a = g.action[t]
        _, reward, stopped = env.step(None if a == NONE_ACTION else a)
        yield t, env, reward, stopped
    if g.raised:
        a = g.raised_action
        try:
            env.step(None if a == NONE_ACTION else a)
        except NoMove:
            return
        raise AssertionError(f"{g.name}: the reference raised at step {g.steps}, the rules did not")


def unreduced(state):
    """whether Newton would change this state: its rescale merged coordinates that were an ulp apart"""
    return not np.array_equal(R.reduce(state), np.asarray(state))


def coverage(games):
    """the counts make_env_golden.py asserts before it writes, from the recorded arrays alone"""
    c = dict(games=len(games), steps=sum(g.steps for g in games), raised=sum(g.raised for g in games),
             illegal_on_unreduced=0, post_reset_on_unreduced=0, dim7_hosts=set(), causes={0: set(), 1: set()},
             after_stop=0, outside_range=0, subsets={0: 0, 1: 0, 2: 0})
    for g in games:
        if g.mode == 0 and g.d == 7:
            c["dim7_hosts"].add(g.player_name)
        state, coords, was_stopped = R.padded(g.reset_state.copy(), g.m), g.reset_coords, False
        if g.mode == 0 and g.scale and g.improve:
            # reset: Newton, rescale, then step(None) on that state
            pre = R.rescale(R.reduce(R.padded(R.points_of(g.root.copy()), g.m)))
            c["post_reset_on_unreduced"] += unreduced(pre)
        for t in range(g.steps):
            a, new = g.action[t], R.padded(g.states[t], g.m)
            rows = len(g.states[t])
            if g.mode == 0:
                legal = 0 <= a < g.d and (coords >> a) & 1
                c["outside_range"] += not 0 <= a < g.d
                if not legal and g.scale and unreduced(state):
                    c["illegal_on_unreduced"] += 1
                if g.stopped[t]:
                    c["causes"][0].add("ended" if rows < 2 else "value" if g.exceed[t] else "invalid")
                coords = g.last[t]
            else:
                c["subsets"][min(2, bin(a & ((1 << g.d) - 1)).count("1"))] += 1
                if g.stopped[t]:
                    cause = "ended" if rows < 2 else "value" if g.exceed[t] else "steps"
                    c["causes"][1].add(cause)
            c["after_stop"] += was_stopped
            was_stopped = was_stopped or g.stopped[t]
            state = new
    return c
