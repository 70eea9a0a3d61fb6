"""Autonomous games between a fixed host and a fixed agent, vectorised over the batch -- the counterpart of
``hironaka/game.py`` (`Game`, `GameHironaka`, `GameMorin`; BASELINE config 1's plumbing).

The state is a ``HipPoints`` container; one ``step()`` is: the host picks a coordinate subset per game
(`Host.select_coord`, one launch for Zeillinger's), the agent picks an axis and applies shift -> Newton
polytope in ONE fused launch (`Agent.move`, agent.py:69-72), then the optional rescale (game.py:107-108).
``coord_history`` holds the hosts' multi-binary masks [B, d] and ``move_history`` the agents' axes [B]
(-1 where the reference records ``None``), one entry per step, as device tensors.
"""
import abc
import logging
from typing import Optional

import torch

from . import _abi as A
from . import ops
from .agent import Agent, AgentMorin, ChooseFirstAgent, RandomAgent
from .core import HipPoints
from .host import AllCoordHost, Host, WeakSpivakovsky, WeakSpivakovskyMinHitting, Zeillinger, ZeillingerLex
from .host_action_preprocess import encode_host_class

_KERNEL_HOSTS = {Zeillinger: "zeillinger", AllCoordHost: "all_coord", ZeillingerLex: "zeillinger_lex",
                 WeakSpivakovsky: "weak_spivakovsky", WeakSpivakovskyMinHitting: "weak_spivakovsky_min_hitting"}


class Game(abc.ABC):
    """game.py:11-81"""

    def __init__(self, state: Optional[HipPoints], host: Host, agent: Agent,
                 scale_observation: Optional[bool] = True, **kwargs):
        self.logger = logging.getLogger(type(self).__name__)
        self.state = state
        self.dimension = state.dimension if state is not None else None
        self.host = host
        self.agent = agent
        self.coord_history = []
        self.move_history = []
        self.scale_observation = scale_observation
        if self.state is not None:
            self.state.get_newton_polytope()  # clear up the extra points (game.py:46)
            self.stopped = self.state.ended
            if self.scale_observation:
                self.state.rescale()
        else:
            self.stopped = True

    @abc.abstractmethod
    def step(self, verbose: int = 0) -> bool:
        """one move of every game; True if the games go on, False if they had stopped or stop now"""

    def _show(self, coords, action, weights, ended):
        lines = [f"Host move: {coords}", f"Agent move: {action}"]
        if weights is not None:
            lines.append(f"Weights: {weights}")
        for line in lines + [f"Game Ended: {ended}"]:
            self.logger.info(line)

    def print_history(self):
        for title, history in (("Coordinate history (host choices):", self.coord_history),
                               ("Move history (agent choices):", self.move_history)):
            self.logger.info(title)
            self.logger.info(history)


class GameHironaka(Game):
    """game.py:84-119.  ``step()`` is one move of every game in up to three launches (the host's, the agent's fused
    move, the rescale).  ``play(n)`` runs up to n further moves of every game in ONE launch of hk_game_play when the
    host is one of the five deterministic hosts and the agent a `RandomAgent` or a `ChooseFirstAgent`, on a state in
    list semantics with padding -1; it is also the only way the hitting-set hosts play at dimension 7.  It appends the
    ``coord_history`` / ``move_history`` entries that ``step()`` would (zeros / -1 for a game that did not move) and
    keeps, per game, ``length`` [B] (the moves ``play`` has made), ``outcome`` [B] (the HK_PLAY_* code,
    ops.PLAY_OUTCOMES) and ``stopped_batch`` [B]; ``stopped`` is true once every game has stopped."""

    def __init__(self, state: Optional[HipPoints], host: Host, agent: Agent, **kwargs):
        super().__init__(state, host, agent, **kwargs)
        self.stopped_batch = self.outcome = self.length = None
        self._host_name = _KERNEL_HOSTS.get(type(self.host))  # exact types: a subclass may override select_coord
        self._may_hold_frozen = False  # a game stopped by something other than its end: play() must not touch it again

    def play(self, max_steps: int) -> bool:
        """up to max_steps further moves of every game in one launch; True if games go on"""
        if self._host_name is None or type(self.agent) not in (RandomAgent, ChooseFirstAgent):
            raise TypeError("play() runs the host and the agent inside the launch: it needs one of the five "
                            "deterministic hosts and a RandomAgent or a ChooseFirstAgent. Got "
                            f"{type(self.host).__name__} and {type(self.agent).__name__}; use step().")
        if self.state is None or self.stopped or max_steps < 1:
            return not self.stopped
        if getattr(self.state, "semantics", None) != "list" or self.state.padding_value != -1.0:
            raise ValueError("play() needs a HipPoints with semantics='list' and padding_value=-1; use step().")
        pts = self.state.points
        b, _, d = pts.shape
        if self.outcome is None:
            self.outcome = torch.zeros(b, dtype=torch.int32, device=pts.device)
            self.length = torch.zeros(b, dtype=torch.int32, device=pts.device)
        work = pts if pts.dtype in (torch.float32, torch.float64) else pts.float()
        frozen = (self.outcome != A.HK_PLAY_RUNNING) & (self.outcome != A.HK_PLAY_ENDED)
        classes = None
        if self._may_hold_frozen and bool(frozen.any()):
            # a class id beyond the dimension's classes: the launch leaves such a game as it is
            classes = torch.where(frozen, (1 << d) - d - 1, -1).to(torch.int32).unsqueeze(1).repeat(1, max_steps)
        res = self.agent.play(work, host=self._host_name, max_steps=max_steps, classes=classes,
                              rescale=bool(self.scale_observation), record=True, out=work)
        if work is not pts:
            pts.copy_(work)
        self.outcome = torch.where(frozen, self.outcome, res.outcome)
        self.length = self.length + res.length
        self.stopped_batch = self.outcome != A.HK_PLAY_RUNNING
        for t in range(int(res.length.max())):  # (the one synchronisation of a fused run)
            played = res.classes[:, t] >= 0
            mask = ops.decode_host_class(res.classes[:, t].clamp(min=0), d, torch.int32)
            self.coord_history.append(mask * played.unsqueeze(1).to(torch.int32))
            self.move_history.append(res.axes[:, t])
        self._may_hold_frozen = bool(((self.outcome != A.HK_PLAY_RUNNING) & (self.outcome != A.HK_PLAY_ENDED)).any())
        self.stopped = bool(self.stopped_batch.all())
        return not self.stopped

    def step(self, verbose: int = 0) -> bool:
        if self.stopped:
            return False
        if verbose:
            self.logger.info(self.state)
        coords = self.host.select_coord(self.state)
        action = self.agent.move(self.state, coords)
        if self.scale_observation:
            self.state.rescale()
        if verbose:
            self._show(coords, action, None, self.state.ended)
        self.coord_history.append(coords)
        self.move_history.append(action)
        if self.state.ended:
            self.stopped = True
            return False
        return True


class GameMorin(Game):
    """game.py:122-154, vectorised -- the agent is Thom's (`AgentMorin`: of the two lowest coordinates the host offers,
    the one with the smaller weight), and a game stops with "no contribution" when its distinguished point is no
    longer a vertex of the Newton polytope after a move.

    The state is a ``HipPoints`` in list semantics with ``distinguished_points``; ``weights`` starts as ones [B, d]
    (int32, on the device).  One ``step()`` is one launch of hk_search_morin_play for all games when the host is one
    of the five deterministic hosts -- the host's choice, the agent's, the weights, shift -> reposition -> Newton
    polytope and the tracking all happen inside it, which is also the only way the hitting-set hosts play at
    dimension 7.  Any other host is asked through ``select_coord`` and its subsets are forced on the same launch.
    ``stopped_batch`` [B] marks the games that have stopped (they are not touched again), ``no_contribution`` [B]
    those whose point was lost, ``outcome`` [B] holds the HK_MORIN_* code of each game (ops.MORIN_OUTCOMES), and
    ``stopped`` is true once every game has stopped.  ``coord_history`` / ``move_history`` are `GameHironaka`'s: the
    hosts' masks [B, d] and the agents' axes [B] per step, zeros / -1 for a game that did not move.  ``play(n)`` runs
    up to n further moves of every game in one launch and appends the same histories.  ``scale_observation`` is
    honoured at construction as `Game` does and, as in the reference's GameMorin.step, not applied in ``step``."""

    def __init__(self, state: Optional[HipPoints], host: Host, agent: Agent, **kwargs):
        if state is not None and (getattr(state, "semantics", None) != "list" or state.distinguished_points is None):
            raise ValueError("GameMorin needs a HipPoints with semantics='list' and distinguished_points.")
        if not isinstance(agent, AgentMorin):
            raise TypeError(f"GameMorin plays with an AgentMorin. Got {type(agent).__name__}.")
        super().__init__(state, host, agent, **kwargs)
        self.weights = self.stopped_batch = self.no_contribution = self.outcome = None
        self._host_name = _KERNEL_HOSTS.get(type(self.host))  # exact types: a subclass may override select_coord
        if state is None:
            return
        pts = state.points
        b, _, d = pts.shape
        self.weights = torch.ones((b, d), dtype=torch.int32, device=pts.device)
        given = state.distinguished_points
        self._dist_as_list = not isinstance(given, torch.Tensor)
        self._dist = (torch.tensor([-1 if v is None else int(v) for v in given], dtype=torch.int32, device=pts.device)
                      if self._dist_as_list else given.to(torch.int32))
        self.no_contribution = self._dist < 0
        ended = state.ended_batch_in_tensor.to(torch.bool)
        self.stopped_batch = ended | self.no_contribution
        self.outcome = torch.where(self.no_contribution, A.HK_MORIN_NO_CONTRIBUTION,
                                   torch.where(ended, A.HK_MORIN_ENDED, A.HK_MORIN_RUNNING)).to(torch.int32)
        self.stopped = bool(self.stopped_batch.all())

    def _advance(self, max_steps: int, classes=None):
        """up to max_steps moves of every game that has not stopped, in one launch"""
        pts = self.state.points
        work = pts if pts.dtype in (torch.float32, torch.float64) else pts.float()
        live = ~self.stopped_batch
        res = self.agent.play(work, self.weights, torch.where(live, self._dist, -1), max_steps=max_steps,
                              host=None if classes is not None else self._host_name, classes=classes, record=True,
                              out=work, validate=False)
        if work is not pts:
            pts.copy_(work)
        self.weights = res.weights
        self._dist = torch.where(live, res.distinguished, self._dist)
        self.outcome = torch.where(live, res.outcome, self.outcome)
        self.no_contribution = self.outcome == A.HK_MORIN_NO_CONTRIBUTION
        self.stopped_batch = self.outcome != A.HK_MORIN_RUNNING
        d = pts.shape[2]
        for t in range(1 if max_steps == 1 else int(res.length.max())):  # (one synchronisation for a fused run)
            played = res.classes[:, t] >= 0
            mask = ops.decode_host_class(res.classes[:, t].clamp(min=0), d, torch.int32)
            self.coord_history.append(mask * played.unsqueeze(1).to(torch.int32))
            self.move_history.append(res.axes[:, t])
        self.state.distinguished_points = ([None if v < 0 else v for v in self._dist.tolist()] if self._dist_as_list
                                           else self._dist)
        self.stopped = bool(self.stopped_batch.all())
        return res

    def step(self, verbose: int = 0) -> bool:
        if self.stopped:
            return False
        if verbose:
            self.logger.info(self.state)
        classes = None
        if self._host_name is None:
            classes = encode_host_class(self.host.select_coord(self.state)).unsqueeze(1)
        self._advance(1, classes)
        if verbose:
            self._show(self.coord_history[-1], self.move_history[-1], self.weights, self.stopped_batch)
        return not self.stopped

    def play(self, max_steps: int) -> bool:
        """up to max_steps further moves of every game in one launch (kernel hosts only); True if games go on"""
        if self._host_name is None:
            raise TypeError("play() runs the host inside the launch: it needs one of the five deterministic hosts. "
                            f"Got {type(self.host).__name__}; use step().")
        if self.stopped or max_steps < 1:
            return not self.stopped
        self._advance(max_steps)
        return not self.stopped
