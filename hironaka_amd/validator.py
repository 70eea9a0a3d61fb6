"""A fixed host measured against a fixed agent -- the counterpart of ``hironaka/validator/hironaka_validator.py``
(`HironakaValidator`, the source of the reference README's rho tables).

The reference plays one game at a time and counts loop iterations; here a batch of games is played to the end in one
launch of hk_game_play (``play_games``), and ``playoff`` does the reference's bookkeeping on the (length, outcome) pairs
that come back: what hironaka_validator.py:30-48 returns when its ``reset`` hands out the same states in the same order.
"""
from typing import Any, Dict, Optional

import numpy as np
import torch

from . import _abi as A
from .agent import ChooseFirstAgent, RandomAgent
from .game import _KERNEL_HOSTS

_PLAYOFF_BATCH = 16384  # games per launch of a playoff without reset_states


def playoff_history(lengths, outcomes, num_steps: int, step_threshold: int, first_game: int = 0):
    """The reference's bookkeeping (hironaka_validator.py:33-48) over games given as (length, outcome) arrays, in the
    order ``reset`` handed them out, for a budget of ``num_steps`` loop iterations.  A game that ended at move k costs k
    iterations and records k - 1; one that passed the value threshold at move k costs k + 1 and records k; one still
    running after step_threshold = T moves costs T + 1 and records T.  The game that the budget cuts off records the
    iterations it got; a budget that ends exactly on a reset records a trailing 0.  Returns (len_history, the
    iterations left over when the games ran out)."""
    lengths, outcomes = np.asarray(lengths, np.int64), np.asarray(outcomes, np.int64)
    ended = outcomes == A.HK_PLAY_ENDED
    cost = np.where(ended, np.maximum(lengths, 1), lengths + 1)
    record = np.where(ended, np.maximum(lengths - 1, 0), lengths)
    cum = np.cumsum(cost)
    k = int(np.searchsorted(cum, num_steps, side="left"))  # the game in which the budget runs out
    used = min(k + 1, len(cost))
    bad = np.nonzero((outcomes[:used] == A.HK_PLAY_INEXACT) | (outcomes[:used] == A.HK_PLAY_NO_MOVE))[0]
    if len(bad):
        g = int(bad[0])
        raise RuntimeError(f"game {first_game + g} stopped after {int(lengths[g])} moves with outcome "
                           f"{int(outcomes[g])} (HK_PLAY_INEXACT: a coordinate left the exact integers; HK_PLAY_NO_MOVE: "
                           f"the host had no move): it has no length to count.")
    still = (outcomes[:used] == A.HK_PLAY_RUNNING) & (lengths[:used] != step_threshold)
    assert not still.any(), "a running game was played for step_threshold moves"
    if k >= len(cost):
        return record.tolist(), num_steps - (int(cum[-1]) if len(cum) else 0)
    if cum[k] == num_steps:
        return record[: k + 1].tolist() + [0], 0
    return record[:k].tolist() + [num_steps - (int(cum[k - 1]) if k else 0)], 0


class HironakaValidator:
    """hironaka_validator.py:8-54 on the GPU.  ``host``: one of the five deterministic hosts; ``agent``: a
    `RandomAgent` or a `ChooseFirstAgent` (exact types: the launch plays both sides).  Configuration keys (in
    ``config_kwargs`` or as keywords), with the reference's defaults: max_num_points 10, dimension 3, max_value 50,
    value_threshold None, step_threshold 1000, scale_observation True; and seed 0 (of the reset states), dtype
    torch.float64, device "cuda".  Reset states are raw ``randint[0, max_value)`` draws, not reduced, as in the
    reference; they are rescaled when scale_observation is set."""

    def __init__(self, host, agent, config_kwargs: Optional[Dict[str, Any]] = None, **kwargs):
        config = {**(config_kwargs or {}), **kwargs}
        if type(host) not in _KERNEL_HOSTS or type(agent) not in (RandomAgent, ChooseFirstAgent):
            raise TypeError("HironakaValidator plays whole games inside one launch: it needs one of the five "
                            "deterministic hosts and a RandomAgent or a ChooseFirstAgent. Got "
                            f"{type(host).__name__} and {type(agent).__name__}.")
        self.host, self.agent = host, agent
        self._host_name = _KERNEL_HOSTS[type(host)]
        self.max_num_points = int(config.get("max_num_points", 10))
        self.dimension = int(config.get("dimension", 3))
        self.max_value = int(config.get("max_value", 50))
        self.value_threshold = config.get("value_threshold", None)
        if self.value_threshold is not None and not self.value_threshold > 0:
            raise ValueError(f"value_threshold must be positive or None. Got {self.value_threshold}.")
        self.step_threshold = int(config.get("step_threshold", 1000))
        self.scale_observation = bool(config.get("scale_observation", True))
        self.seed = int(config.get("seed", 0))
        self.dtype = config.get("dtype", torch.float64)
        self.device = torch.device(config.get("device", "cuda"))
        self._gen = None
        self.games_played = 0  # the number of the next game in the random agent's counter

    def _reset_states(self, num_games: int) -> torch.Tensor:
        if self._gen is None:
            self._gen = torch.Generator(device=self.device)
            self._gen.manual_seed(self.seed)
        return torch.randint(0, self.max_value, (num_games, self.max_num_points, self.dimension), device=self.device,
                             generator=self._gen).to(self.dtype)

    def play_games(self, num_games: int, reset_states: Optional[torch.Tensor] = None):
        """num_games games from fresh reset states (or from ``reset_states`` [num_games, m, d]) played until they
        stop or reach step_threshold moves, in one launch: (lengths [N], outcomes [N]) int32 device tensors, outcomes
        in the HK_PLAY_* codes (ops.PLAY_OUTCOMES)."""
        if reset_states is None:
            states = self._reset_states(num_games)
        else:
            states = torch.as_tensor(reset_states).to(device=self.device, dtype=self.dtype).clone()
            if states.dim() != 3 or states.shape[0] != num_games:
                raise ValueError(f"reset_states must be [{num_games}, max_points, dim]. Got {tuple(states.shape)}.")
        over = None
        if self.value_threshold is not None:
            # the reference tests the threshold before every move, the first included: on the reset state as it plays it
            top = states.amax(dim=(1, 2), keepdim=True)
            root = torch.where(top > 0, states / top, states) if self.scale_observation else states
            over = (root > self.value_threshold).flatten(1).any(1)
        res = self.agent.play(states, host=self._host_name, max_steps=self.step_threshold,
                              rescale=self.scale_observation, rescale_root=self.scale_observation,
                              value_threshold=self.value_threshold, game_offset=self.games_played, step_offset=0,
                              out=states)
        self.games_played += num_games
        if over is None:
            return res.length, res.outcome
        return (torch.where(over, 0, res.length).to(torch.int32),
                torch.where(over, A.HK_PLAY_VALUE_LIMIT, res.outcome).to(torch.int32))

    def playoff(self, num_steps: int, verbose: int = 0, reset_states: Optional[torch.Tensor] = None):
        """the reference's ``len_history`` for a budget of num_steps loop iterations"""
        history, left, first = [], int(num_steps), 0
        if reset_states is not None:
            reset_states = torch.as_tensor(reset_states)
        while True:
            if reset_states is not None:
                if first >= reset_states.shape[0]:
                    raise ValueError(f"reset_states holds {first} games, which last for {num_steps - left} of the "
                                     f"{num_steps} steps.")
                n = reset_states.shape[0]
                lengths, outcomes = self.play_games(n, reset_states)
            else:
                n = max(1, min(left, _PLAYOFF_BATCH))
                lengths, outcomes = self.play_games(n)
            got, left = playoff_history(lengths.cpu().numpy(), outcomes.cpu().numpy(), left, self.step_threshold, first)
            history += got
            first += n
            if left == 0:
                return history
