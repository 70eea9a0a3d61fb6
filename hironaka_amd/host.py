"""Fixed hosts for the gym / game surfaces, vectorised over a batch of games -- the counterparts of
``hironaka/host.py`` (`Host.select_coord`, `RandomHost`, `AllCoordHost`, `Zeillinger`, `ZeillingerLex`,
`WeakSpivakovsky`, `WeakSpivakovskyMinHitting`, `Spivakovsky`, `RandomSpivakovsky`).

``select_coord(points)`` takes the padded state ``[B, m, d]`` (device tensor or a container with a
``.points`` attribute) and returns the chosen coordinate subsets as a multi-binary mask ``[B, d]``
(int32).  A game with fewer than two points gets the empty subset (all zeros), the vectorised form of
the reference's ``[]`` (host.py:78-80).
"""
import abc
import random
from typing import Optional, Union

import torch

from . import ops


def _as_points(points) -> torch.Tensor:
    return points.points if hasattr(points, "points") else points


class Host(abc.ABC):
    def select_coord(self, points, debug=False) -> torch.Tensor:
        pts = _as_points(points)
        mask = self._select_coord(pts)
        alive = ops.get_num_points(pts) >= 2
        return mask * alive.unsqueeze(1).to(mask.dtype)

    @abc.abstractmethod
    def _select_coord(self, points: torch.Tensor) -> torch.Tensor:
        ...


class RandomHost(Host):
    """host.py:42-45 -- two distinct coordinates, uniformly."""

    def __init__(self, seed: Optional[Union[int, torch.Generator]] = None):
        self._gen = seed if isinstance(seed, torch.Generator) or seed is None else None
        self._seed = seed if isinstance(seed, int) else None

    def _generator(self, device):
        if self._gen is None and self._seed is not None:
            self._gen = torch.Generator(device=device)
            self._gen.manual_seed(self._seed)
        return self._gen

    def _select_coord(self, points: torch.Tensor) -> torch.Tensor:
        b, _, d = points.shape
        keys = torch.rand((b, d), device=points.device, generator=self._generator(points.device))
        pick = keys.argsort(dim=1)[:, :2]
        mask = torch.zeros((b, d), dtype=torch.int32, device=points.device)
        return mask.scatter_(1, pick, 1)


class AllCoordHost(Host):
    """host.py:48-51"""

    def _select_coord(self, points: torch.Tensor) -> torch.Tensor:
        b, _, d = points.shape
        return torch.ones((b, d), dtype=torch.int32, device=points.device)


class Zeillinger(Host):
    """host.py:54-95 -- characteristic vector (L, S) over the pairs of points, smallest first;
    the subset is {argmin, argmax} of that pair's difference (hk_zeillinger, list semantics)."""

    @staticmethod
    def get_char_vector(vt):
        mx, mn = max(vt), min(vt)
        return mx - mn, sum(v == mx for v in vt) + sum(v == mn for v in vt)

    def _select_coord(self, points: torch.Tensor) -> torch.Tensor:
        d = points.shape[2]
        cls = ops.zeillinger(points, sem="list")
        mask = ops.decode_host_class(cls.clamp(min=0), d, torch.int32)
        return mask * (cls >= 0).unsqueeze(1).to(torch.int32)


MAX_HOST_DIM = 6  # hk_host_select: the hitting-set hosts keep one bit per possible support


def _hk_host(points: torch.Tensor, host: str) -> torch.Tensor:
    """select_coord of a host of hk_host_select (list semantics): the decoded mask, empty where the class is -1"""
    d = points.shape[2]
    if d > MAX_HOST_DIM:
        raise ValueError(f"{host} runs on the GPU for dimensions up to {MAX_HOST_DIM} (hk_host_select). Got {d}.")
    cls = ops.host_select(points, host)
    mask = ops.decode_host_class(cls.clamp(min=0), d, torch.int32)
    return mask * (cls >= 0).unsqueeze(1).to(torch.int32)


class ZeillingerLex(Zeillinger):
    """host.py:116-127 -- Zeillinger's key (L, S); among the pairs of the smallest key, the lexicographically
    smallest [argmin, argmax] of P_i - P_j (hk_host_select)."""

    def _select_coord(self, points: torch.Tensor) -> torch.Tensor:
        return _hk_host(points, "zeillinger_lex")


class WeakSpivakovsky(Host):
    """host.py:357-378 -- a minimal hitting set of the points' supports (sets of nonzero coordinates), the first in
    lexicographic order of its sorted coordinates (hk_host_select)."""

    def _select_coord(self, points: torch.Tensor) -> torch.Tensor:
        return _hk_host(points, "weak_spivakovsky")


class WeakSpivakovskyMinHitting(Host):
    """host.py:381-427 -- a minimal hitting set of the points' supports, the smallest as an integer
    (hk_host_select).  ``dim`` (the width of the reference's subset table) is accepted and ignored."""

    def __init__(self, dim=16):
        self.dim = dim

    def _select_coord(self, points: torch.Tensor) -> torch.Tensor:
        return _hk_host(points, "weak_spivakovsky_min_hitting")


def _hk_mask_host(points: torch.Tensor, host: str, **draw) -> torch.Tensor:
    """select_coord of a host of hk_spivakovsky_select (list semantics): its bit masks as a multi-binary mask"""
    d = points.shape[2]
    if d > MAX_HOST_DIM:
        raise ValueError(f"{host} runs on the GPU for dimensions up to {MAX_HOST_DIM} (hk_spivakovsky_select). Got {d}.")
    bits = ops.spivakovsky_select(points, host, **draw)
    return (bits.unsqueeze(1) >> torch.arange(d, dtype=torch.int32, device=bits.device)) & 1


class Spivakovsky(Host):
    """host.py:130-290 -- Spivakovsky's host, the one the game was solved with (hk_spivakovsky_select): levels of
    "move to the origin, take the coordinates of the nearest points, project", then a minimal permissible set.  The
    subset may hold 0 or 1 coordinates, as the reference's does.  ``dim`` is accepted and ignored."""

    def __init__(self, dim=16):
        self.dim = dim

    def _select_coord(self, points: torch.Tensor) -> torch.Tensor:
        return _hk_mask_host(points, "spivakovsky")


class RandomSpivakovsky(Host):
    """host.py:293-354 -- one of the smallest hitting sets (>= 2 coordinates) of the points' supports, uniformly
    (hk_spivakovsky_select).  The draws come from Philox keyed by ``seed`` (a fresh key when None), the game's number
    ``game_offset + g`` and the number of the call, ``moves``, which every ``select_coord`` advances.  ``dim`` (the
    width of the reference's subset table) is accepted and ignored: the candidates lie within the game's coordinates."""

    def __init__(self, dim=16, seed: Optional[int] = None, game_offset: int = 0):
        self.dim = dim
        self.seed = (random.getrandbits(63) if seed is None else int(seed)) % 2 ** 64
        self.game_offset = game_offset
        self.moves = 0  # calls made: the move number in the host's counter

    def _select_coord(self, points: torch.Tensor) -> torch.Tensor:
        mask = _hk_mask_host(points, "random_spivakovsky", seed=self.seed, game_offset=self.game_offset,
                             step=self.moves)
        self.moves += 1
        return mask


class PolicyHost(Host):
    """host.py:98-113 -- a host that asks a policy object: ``policy.predict(features)`` on the container's
    features (``get_features()``) returns the multi-binary subsets [B, d]."""

    def __init__(self, policy, use_discrete_actions_for_host: Optional[bool] = False, **kwargs):
        self._policy = policy
        self.use_discrete_actions_for_host = kwargs.get("use_discrete_actions_for_host", use_discrete_actions_for_host)

    def select_coord(self, points, debug=False) -> torch.Tensor:
        self._features = points.get_features() if hasattr(points, "get_features") else _as_points(points)
        return super().select_coord(points, debug)

    def _select_coord(self, points: torch.Tensor) -> torch.Tensor:
        coords = torch.as_tensor(self._policy.predict(self._features), device=points.device)
        return (coords == 1).to(torch.int32)
