"""Fixed agents for the gym / game surfaces, vectorised -- the counterparts of ``hironaka/agent.py``
(`Agent.move`, `RandomAgent`, `ChooseFirstAgent`, `AgentMorin`).

``move(points, coords)`` takes a ``HipPoints``-like container (``.points`` [B, m, d]) and the host's
subsets as a multi-binary mask [B, d]; it chooses one axis per game (-1 = "None": the host offered
fewer than two coordinates, agent.py:89,97), and -- with ``inplace`` -- applies
shift -> [reposition] -> Newton polytope to the container in ONE fused launch (agent.py:69-72).
"""
import abc
import random
from typing import Optional, Union

import torch

from . import _abi as A
from . import ops
from .host_action_preprocess import encode_host_class


class Agent(abc.ABC):
    USE_REPOSITION: bool = False

    def move(self, points, coords: torch.Tensor, inplace: bool = True, sem: str = "list") -> torch.Tensor:
        pts = points.points if hasattr(points, "points") else points
        coords = coords.to(pts.device)
        actions = self._get_actions(pts, coords)
        actions = torch.where(coords.sum(dim=1) > 1, actions, torch.full_like(actions, -1))
        if not inplace:
            return actions
        flags = ops.make_flags(getattr(points, "semantics", sem), noop_if_invalid=True)
        stages = ops.make_stages(True, self.USE_REPOSITION, True, False)
        pad = getattr(points, "padding_value", -1.0)
        res = ops.step(pts, coords, actions, stages=stages, flags=flags, padding_value=pad, out=pts)
        if hasattr(points, "points"):
            points.points = res["points"]
        return actions

    @abc.abstractmethod
    def _get_actions(self, points: torch.Tensor, coords: torch.Tensor) -> torch.Tensor:
        ...

    def _play(self, agent: str, points, **kwargs):
        """ops.game_play with this agent's rule and USE_REPOSITION (RandomAgent.play, ChooseFirstAgent.play)"""
        pts = points.points if hasattr(points, "points") else points
        return ops.game_play(pts, agent=agent, reposition=self.USE_REPOSITION, **kwargs)


class RandomAgent(Agent):
    """agent.py:85-90 -- uniform over the host's subset."""

    def __init__(self, seed: Optional[Union[int, torch.Generator]] = None):
        self._gen = seed if isinstance(seed, torch.Generator) else None
        self._seed = seed if isinstance(seed, int) else None
        self._play_seed = None
        self.moves = 0  # moves play() may have drawn for: the move number in the random agent's counter

    def play_seed(self) -> int:
        """the Philox key of the draws made on the device (play, vec_env.HironakaAgentVecEnv): the generator's initial
        seed, or the agent's, or a fresh one when the agent has none"""
        if self._play_seed is None:
            given = self._gen.initial_seed() if self._gen is not None else self._seed
            self._play_seed = (random.getrandbits(63) if given is None else int(given)) % 2 ** 64
        return self._play_seed

    def play(self, points, **kwargs):
        """whole games in one launch (ops.game_play, agent="random"): the draws come from Philox keyed by this agent's
        seed (the generator's initial seed, or a fresh one when the agent has none), the game and the move number"""
        kwargs.setdefault("seed", self.play_seed())
        kwargs.setdefault("step_offset", self.moves)
        res = self._play("random", points, **kwargs)
        self.moves += kwargs["max_steps"]
        return res

    def _get_actions(self, points, coords):
        if self._gen is None and self._seed is not None:
            self._gen = torch.Generator(device=points.device)
            self._gen.manual_seed(self._seed)
        noise = torch.rand(coords.shape, device=points.device, generator=self._gen) + 1e-6
        return torch.argmax(noise * (coords > 0), dim=1).to(torch.int32)


class ChooseFirstAgent(Agent):
    """agent.py:93-98 -- the lowest coordinate of the subset."""

    def _get_actions(self, points, coords):
        return torch.argmax((coords > 0).to(torch.int32), dim=1).to(torch.int32)

    def play(self, points, **kwargs):
        """whole games in one launch (ops.game_play, agent="choose_first")"""
        return self._play("choose_first", points, **kwargs)


class PolicyAgent(Agent):
    """agent.py:101-111 -- an agent that asks a policy object: ``policy.predict((features, coords))`` returns
    one axis per game."""

    def __init__(self, policy, **kwargs):
        self._policy = policy

    def move(self, points, coords: torch.Tensor, inplace: bool = True, sem: str = "list") -> torch.Tensor:
        self._features = points.get_features() if hasattr(points, "get_features") else None
        return super().move(points, coords, inplace, sem)

    def _get_actions(self, points, coords):
        features = points if self._features is None else self._features
        return torch.as_tensor(self._policy.predict((features, coords)), device=points.device).to(torch.int32)


class AgentMorin(Agent):
    """agent.py:114-136, batched -- of the two lowest coordinates of the host's subset the one with the smaller weight;
    when they weigh the same, ``tie`` decides: "random" (the reference: uniform over the whole subset, drawn on the
    device from Philox keyed by ``seed``, the game and the number of moves this agent has made), "lowest" or
    "highest".  The other coordinates of the subset get weight 0.  ``move`` applies shift -> reposition -> Newton
    polytope and the weights in ONE launch (hk_search_morin_play) and, when the container tracks distinguished points,
    moves them: a game whose point is lost keeps the new state and gets ``None`` / -1."""
    USE_WEIGHTS = True
    USE_REPOSITION = True

    def __init__(self, tie: str = "random", seed: Optional[int] = None):
        if tie not in ops.MORIN_TIES:
            raise ValueError(f"tie must be one of {sorted(ops.MORIN_TIES)}. Got {tie!r}.")
        self.tie = tie
        self.seed = random.getrandbits(63) if seed is None else int(seed)
        self.moves = 0  # launches so far: the move number in the random tie's counter

    def _get_actions(self, points, coords):
        raise NotImplementedError("AgentMorin chooses inside hk_search_morin_play: call move() with the weights.")

    def play(self, points, weights: torch.Tensor, distinguished: torch.Tensor, **kwargs):
        """ops.morin_play with this agent's tie mode and seed; counts the moves it may draw for"""
        res = ops.morin_play(points, weights, distinguished, tie=self.tie, seed=self.seed, step_offset=self.moves,
                             **kwargs)
        self.moves += kwargs["max_steps"]
        return res

    def move(self, points, coords: torch.Tensor, weights=None, inplace: bool = True):
        if weights is None:
            raise Exception("Please specify weights in the parameters.")
        pts = points.points if hasattr(points, "points") else points
        as_list = not isinstance(weights, torch.Tensor)
        w = torch.tensor(weights, dtype=torch.int32, device=pts.device) if as_list else weights
        given = getattr(points, "distinguished_points", None)
        if given is None:  # nothing to track: the game is played on the reduced state
            dist = torch.full((pts.shape[0],), -1, dtype=torch.int32, device=pts.device)
        elif isinstance(given, torch.Tensor):
            dist = given
        else:
            dist = torch.tensor([-1 if v is None else int(v) for v in given], dtype=torch.int32, device=pts.device)
        work = pts if pts.dtype in (torch.float32, torch.float64) else pts.float()
        res = self.play(work, w, dist, max_steps=1, classes=encode_host_class(coords.to(pts.device)).unsqueeze(1),
                        reduce_root=given is None, record=True, out=work if inplace else None)
        actions = res.axes[:, 0]
        if not inplace:
            return actions, (res.weights.tolist() if as_list else res.weights)
        if as_list:
            weights[:] = res.weights.tolist()
        else:
            weights.copy_(res.weights)
        if work is not pts:
            pts.copy_(work)
        if isinstance(given, torch.Tensor):
            given.copy_(res.distinguished)
        elif given is not None:
            given[:] = [None if v < 0 else v for v in res.distinguished.tolist()]
        return actions
