"""Vectorised gym-style environments whose every game resets itself: ``HironakaHostVecEnv`` and
``HironakaAgentVecEnv``, the per-game forms of ``gym_env.HironakaHostEnv`` / ``HironakaAgentEnv`` with the same
constructor keywords, observation / action spaces and reward conventions.

``step(actions)`` is ONE launch (hk_env_step, ``ops.env_step``) into buffers allocated once: it plays every game's
move, and a game that stopped gets its next episode inside the same launch (``auto_reset=True``), with its terminal
observation in ``info["final_observation"]``.  Every game carries its own ``current_step`` and ``episode``, so no game
waits for another.  Episode e of game b is game ``game_offset + e * world_games + b`` of the generator's stream under
the environment's seed -- the state ``gym_env``'s (e + 1)-th ``reset()`` gives row b of a batch of ``world_games`` --
so shards of a larger batch (``game_offset``, ``world_games``) reproduce it.

The host and the agent run inside the kernel: the hosts are the five of ``util.search`` (Zeillinger, AllCoordHost,
ZeillingerLex, WeakSpivakovsky, WeakSpivakovskyMinHitting), the agents ``ChooseFirstAgent`` and ``RandomAgent``, whose
draws come from Philox keyed by the agent's seed, the game and the move number (as in ``RandomAgent.play``), not from
``torch.rand``.  Any other host or agent is a TypeError: ``gym_env``'s environments take those.

The tensors ``step`` and ``reset`` return are the environment's own buffers: the next ``step`` overwrites them.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Union

import numpy as np
import torch

from . import ops
from .agent import Agent, ChooseFirstAgent, RandomAgent
from .gym_env import spaces
from .host import Host
from .util.search import _SEARCH_HOSTS

_FALLBACK = "use hironaka_amd.gym_env.HironakaHostEnv / HironakaAgentEnv for any other host or agent"
_FALLBACK_THRESHOLD = "use hironaka_amd.gym_env.HironakaHostEnv / HironakaAgentEnv for such a threshold"


class HironakaVecBase:
    metadata = {"render_modes": ["ansi"]}
    _MODE = ""

    def __init__(self, num_envs: int, dimension: int = 3, max_num_points: int = 10, max_value: int = 10,
                 padding_value: float = -1.0, value_threshold: Optional[float] = None, step_threshold: int = 1000,
                 fixed_penalty_crossing_threshold: Optional[int] = None, stop_at_threshold: bool = True,
                 improve_efficiency: bool = False, scale_observation: bool = True,
                 reward_based_on_point_reduction: bool = False, device: Union[str, torch.device] = "cuda",
                 seed: int = 0, auto_reset: bool = True, game_offset: int = 0, world_games: Optional[int] = None,
                 **kwargs):
        if num_envs is None or int(num_envs) < 1:
            raise ValueError(f"num_envs must be a positive number of games. Got {num_envs}.")
        if padding_value != -1.0:
            raise ValueError(f"hk_env_step pads with -1. Got padding_value {padding_value}.")
        if value_threshold is not None and value_threshold <= 0:
            raise ValueError(f"hk_env_step reads a value_threshold <= 0 as none, while the environments test any "
                             f"threshold that is not None. Got {value_threshold}; {_FALLBACK_THRESHOLD}.")
        self.dimension, self.max_num_points, self.max_value = dimension, max_num_points, max_value
        self.padding_value = padding_value
        self.value_threshold, self.step_threshold = value_threshold, step_threshold
        self.fixed_penalty_crossing_threshold = fixed_penalty_crossing_threshold
        self.stop_at_threshold = stop_at_threshold
        self.improve_efficiency = improve_efficiency
        self.scale_observation = scale_observation
        self.reward_based_on_point_reduction = reward_based_on_point_reduction
        self.num_envs = int(num_envs)
        self.auto_reset = bool(auto_reset)
        self.game_offset = int(game_offset)
        self.world_games = self.num_envs if world_games is None else int(world_games)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TypeError("the environments run on a HIP device")
        self._seed = int(seed)
        high = np.inf if self.scale_observation else 1.0  # (as gym_env: the bounds are swapped in the reference too)
        self.point_observation_space = spaces.Box(low=-1.0, high=high, shape=(max_num_points, dimension),
                                                  dtype=np.float32)
        n, m, d = self.num_envs, max_num_points, dimension
        new = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=self.device)  # noqa: E731
        self._points = new((n, m, d), torch.float64)  # list semantics, like gym_env's state
        self.current_step = new((n,), torch.int32)
        self.episode = new((n,), torch.int32)
        self._action = new((n,), torch.int32)
        self._reward = new((n,), torch.float64)
        self._stopped = new((n,), torch.uint8)
        self._exceed = new((n,), torch.uint8)
        self._obs_points = new((n, m, d), torch.float32)
        self._final_points = new((n, m, d), torch.float32)
        self.exceed_threshold = self._exceed.view(torch.bool)
        self._stopped_bool = self._stopped.view(torch.bool)
        self._buffers: Dict[str, Any] = {}
        self._started = False

    # ---- what the two environments differ in ------------------------------------------------------
    def _observation(self):
        raise NotImplementedError

    def _final_observation(self):
        raise NotImplementedError

    def _launch(self, reset_all: bool) -> None:
        penalty = -float(self.step_threshold) if self.fixed_penalty_crossing_threshold is None \
            else float(self.fixed_penalty_crossing_threshold)
        ops.env_step(self._points, mode=self._MODE, step_count=self.current_step, episode=self.episode,
                     reward=self._reward, stopped=self._stopped, exceed=self._exceed, obs_points=self._obs_points,
                     final_points=self._final_points, action=self._action, seed=self._seed,
                     game_offset=self.game_offset, world_games=self.world_games, max_value=self.max_value,
                     value_threshold=self.value_threshold, step_threshold=self.step_threshold,
                     threshold_penalty=penalty, scale_observation=self.scale_observation,
                     stop_at_threshold=self.stop_at_threshold,
                     point_reduction_reward=self.reward_based_on_point_reduction,
                     improve_efficiency=self.improve_efficiency, auto_reset=self.auto_reset, reset_all=reset_all,
                     **self._buffers)

    def _info(self) -> Dict[str, Any]:
        return {"final_observation": self._final_observation(), "episode": self.episode,
                "current_step": self.current_step, "exceed_threshold": self.exceed_threshold,
                "step_threshold": self.step_threshold}

    # ---- gym protocol ---------------------------------------------------------------------------
    def reset(self, seed: Optional[int] = None, return_info: bool = False, options=None) -> Any:
        """Episode 0 of every game (with ``seed``: under that seed from now on), through hk_env_step's reset path: the
        states are those of ``gym_env``'s first ``reset()``."""
        if seed is not None:
            self._seed = int(seed)
        self.episode.fill_(-1)
        self.current_step.zero_()
        self._launch(reset_all=True)
        self._started = True
        return (self._observation(), self._info()) if return_info else self._observation()

    def _step(self):
        if not self._started:
            raise RuntimeError("call reset() before step().")
        self._launch(reset_all=False)
        return self._observation(), self._reward, self._stopped_bool, self._info()

    def render(self, mode="ansi"):
        print(self._points)

    def close(self):
        pass


class HironakaHostVecEnv(HironakaVecBase):
    """The environment fixes a Host; it receives one axis per game (int [N]).  obs = {"points": [N, m, d] float32,
    "coords": [N, d] float64}; reward +1 per legal move that does not end the game, 0 on the one that does,
    ``invalid_move_penalty`` on an axis outside the host's subset."""
    _MODE = "host"

    def __init__(self, host: Host, num_envs: int, invalid_move_penalty: float = -1e-3,
                 stop_after_invalid_move: bool = False, config_kwargs: Optional[Dict[str, Any]] = None, **kwargs):
        name = _SEARCH_HOSTS.get(type(host))  # exact types: a subclass may override select_coord
        if name is None:
            raise TypeError(f"HironakaHostVecEnv runs the host inside the step kernel: supported hosts are "
                            f"{', '.join(t.__name__ for t in _SEARCH_HOSTS)}. Got {type(host).__name__}; {_FALLBACK}.")
        config_kwargs = dict() if config_kwargs is None else config_kwargs
        super().__init__(num_envs, **{**config_kwargs, **kwargs})
        self.host = host
        self.invalid_move_penalty = invalid_move_penalty
        self.stop_after_invalid_move = stop_after_invalid_move
        self.observation_space = spaces.Dict({"points": self.point_observation_space,
                                              "coords": spaces.MultiBinary(self.dimension)})
        self.action_space = spaces.Discrete(self.dimension)
        n, d = self.num_envs, self.dimension
        self._class = torch.full((n,), -1, dtype=torch.int32, device=self.device)
        self._obs_coords = torch.zeros((n, d), dtype=torch.float64, device=self.device)
        self._final_coords = torch.zeros((n, d), dtype=torch.float64, device=self.device)
        self._buffers = dict(host=name, class_io=self._class, obs_coords=self._obs_coords,
                             final_coords=self._final_coords, invalid_move_penalty=float(invalid_move_penalty),
                             stop_after_invalid=bool(stop_after_invalid_move))

    def _observation(self):
        return {"points": self._obs_points, "coords": self._obs_coords}

    def _final_observation(self):
        return {"points": self._final_points, "coords": self._final_coords}

    def step(self, action):
        """action: one axis per game, int [N] (an int32 tensor on the device is used as it is).  Returns
        (obs, reward float64 [N], stopped bool [N], info)."""
        act = torch.as_tensor(action, device=self.device).reshape(self.num_envs)
        self._action = act.to(torch.int32).contiguous()
        return self._step()


class HironakaAgentVecEnv(HironakaVecBase):
    """The environment fixes an Agent; it receives one coordinate subset per game: MultiBinary [N, d], or with
    ``use_discrete_actions_for_host`` an int [N] decoded as its raw binary expansion (like gym_env).  obs = [N, m, d]
    float32; reward +1 when the game ends, the threshold penalty when a threshold trips, optionally the points
    removed.  ``info["agent_axis"]`` is the axis the agent chose, -1 where the subset had fewer than 2 coordinates."""
    _MODE = "agent"

    def __init__(self, agent: Agent, num_envs: int, use_discrete_actions_for_host: Optional[bool] = False,
                 compressed_host_output: Optional[bool] = True, config_kwargs: Optional[Dict[str, Any]] = None,
                 **kwargs):
        if type(agent) is ChooseFirstAgent:  # exact types: a subclass may override the choice
            name, agent_seed = "choose_first", 0
        elif type(agent) is RandomAgent:
            name, agent_seed = "random", agent.play_seed()
        else:
            raise TypeError(f"HironakaAgentVecEnv runs the agent inside the step kernel: supported agents are "
                            f"ChooseFirstAgent and RandomAgent. Got {type(agent).__name__}; {_FALLBACK}.")
        config = kwargs if config_kwargs is None else {**kwargs, **config_kwargs}
        config = dict(config)
        self.use_discrete_actions_for_host = config.pop("use_discrete_actions_for_host", use_discrete_actions_for_host)
        super().__init__(num_envs, **config)
        self.agent = agent
        self.compressed_host_output = compressed_host_output
        self.observation_space = self.point_observation_space
        d = self.dimension
        if self.use_discrete_actions_for_host:
            self.action_space = spaces.Discrete(2 ** d - d - 1 if compressed_host_output else 2 ** d)
        else:
            self.action_space = spaces.MultiBinary(d)
        self._agent_axis = torch.full((self.num_envs,), -1, dtype=torch.int32, device=self.device)
        self._bit = (1 << torch.arange(d, device=self.device)).to(torch.int32)
        self._buffers = dict(agent=name, agent_seed=agent_seed, agent_axis=self._agent_axis,
                             reposition=bool(agent.USE_REPOSITION))

    def _observation(self):
        return self._obs_points

    def _final_observation(self):
        return self._final_points

    def _info(self):
        info = super()._info()
        info["agent_axis"] = self._agent_axis
        return info

    def step(self, action):
        """action: MultiBinary [N, d] subsets, or with use_discrete_actions_for_host int [N] codes (an int32 tensor on the
        device is used as it is: the code is the subset's bit mask).  Returns (obs, reward float64 [N], stopped bool
        [N], info)."""
        n, d = self.num_envs, self.dimension
        action = torch.as_tensor(action, device=self.device)
        if self.use_discrete_actions_for_host:
            mask = action.reshape(n).to(torch.int32)  # the kernel looks at the low d bits only
        else:
            mask = ((action.reshape(n, d) == 1).to(torch.int32) * self._bit).sum(dim=1, dtype=torch.int32)
        self._action = mask.contiguous()
        return self._step()
