"""``ReplayBuffer`` -- the DQN trainers' replay buffer, the counterpart of ``hironaka/trainer/replay_buffer.py:6-176``
(same constructor, attributes, forced types, ``add`` / ``sample`` / ``reset``), kept on the device whole: the ring, its
cursor and the index draws.

The reference keeps ``pos`` and ``full`` as Python ints, copies 5 to 7 slices per ``add`` (twice that at the wrap) and
draws the sample's indices on the CPU.  Here ``add`` is ONE launch of ``hk_replay_push`` and ``sample`` ONE launch of
``hk_replay_sample`` (include/hironaka_hip_replay.h); the cursor is a block of device memory that the kernels read and
advance, so neither call synchronises and both can be captured into a graph.  ``add`` also takes a mask ``keep``: the
uncompacted tensors of a roll-out step go in as they are and only the kept rows enter, in batch order
(``FusedGame.collect``).

Deviation: the sample's indices are Philox words keyed by ``seed`` and the number of samples drawn so far, not
``torch.randint``'s stream -- the deviation ``vec_env.RandomAgent`` makes for the same reason.
"""
from typing import Dict, Optional, Tuple, Type, Union

import torch

from . import _abi as A
from . import ops


class ReplayBuffer:
    """An experience is (order matters): observations (self.dtype), actions (torch.int32), rewards (torch.float32),
    dones (torch.bool), next_observations (self.dtype)."""

    def __init__(self, input_shape: Union[Dict, Tuple], output_dim: int, buffer_size: int,
                 device: Union[str, torch.device], dtype: Union[Type, torch.dtype] = torch.float32, seed: int = 0,
                 **kwargs):
        self.input_shape = input_shape
        self.output_dim = output_dim
        self.buffer_size = buffer_size
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise TypeError(f"ReplayBuffer lives on a HIP device (there is no CPU path). Got {self.device}.")
        self.dtype = dtype
        self.seed = seed

        def storage():
            if isinstance(self.input_shape, dict):
                return {key: torch.zeros((self.buffer_size, *shape), device=self.device, dtype=self.dtype)
                        for key, shape in self.input_shape.items()}
            return torch.zeros((self.buffer_size, *self.input_shape), device=self.device, dtype=self.dtype)

        self.observations = storage()
        self.next_observations = storage()
        self.actions = torch.zeros((self.buffer_size, 1), device=self.device, dtype=torch.int32)
        self.rewards = torch.zeros((self.buffer_size, 1), device=self.device, dtype=torch.float32)
        self.dones = torch.zeros((self.buffer_size, 1), device=self.device, dtype=torch.bool)
        # the raw device block hk_replay_push / hk_replay_sample read and advance (_abi.HK_REPLAY_* name its words)
        self.cursor = ops.replay_cursor(self.device)
        self._offered = 0  # rows handed to add() since the last reset, kept or not

    # ---- the columns, in the experience's order; a dict observation is one column per key --------------------------
    def _split(self, value, name: str) -> list:
        if isinstance(self.input_shape, dict):
            if not isinstance(value, dict):
                raise TypeError(f"{name} must be a dict with keys {list(self.input_shape)}. Got {type(value)}.")
            return [value[key] for key in self.input_shape]
        if not isinstance(value, torch.Tensor):
            raise TypeError(f"Unsupported type. Got {type(value)}.")
        return [value]

    def _join(self, cols: list):
        if isinstance(self.input_shape, dict):
            return dict(zip(self.input_shape, cols))
        return cols[0]

    def _rings(self) -> list:
        return (self._split(self.observations, "observations") + [self.actions, self.rewards, self.dones]
                + self._split(self.next_observations, "next_observations"))

    def _fix(self, t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """the reference's forced type, on the buffer's device, every row contiguous"""
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"Unsupported type. Got {type(t)}.")
        t = t.to(self.device)
        t = t if t.dtype == dtype else t.type(dtype)
        return t if t.shape[0] == 0 or t[0].is_contiguous() else t.contiguous()

    def add(self, obs: Union[torch.Tensor, Dict], action: torch.Tensor, reward: torch.Tensor, done: torch.Tensor,
            next_obs: Union[torch.Tensor, Dict], clone=True, keep: Optional[torch.Tensor] = None):
        """Add a batch of experiences, in one launch.  The inputs are forced into the types above.  With ``keep`` (bool
        or uint8 [B]) only the rows it marks enter, in batch order, as if the inputs had been compacted first; how many
        those are is decided on the device.  ``clone`` is accepted for the reference's signature: the rows are always
        copied.  Raises where the reference asserts: the shapes, and buffer_size > the number of input rows."""
        assert action.shape[1:] == torch.Size([1])
        assert reward.shape[1:] == torch.Size([1])
        assert done.shape[1:] == torch.Size([1])
        length = action.shape[0]
        assert self.buffer_size > length, f"{length} samples are more than the buffer size."
        rows = ([self._fix(t, self.dtype) for t in self._split(obs, "obs")]
                + [self._fix(action, torch.int32), self._fix(reward, torch.float32), self._fix(done, torch.bool)]
                + [self._fix(t, self.dtype) for t in self._split(next_obs, "next_obs")])
        if keep is not None:
            keep = keep.to(self.device).reshape(-1)
        ops.replay_push(self._rings(), rows, self.cursor, keep=keep)
        self._offered += length

    def sample(self, batch_size: int, device: torch.device = None, clone: bool = True) -> Tuple:
        """batch_size experiences drawn uniformly (with repetition) from what the buffer holds, in one launch; the
        indices drawn stay in ``last_sample_index``.  Raises if no row was ever handed to ``add``; where rows were
        offered and ``keep`` let none in, the indices are -1 and the experiences zero."""
        assert self._offered > 0
        cols, self.last_sample_index = ops.replay_sample(self._rings(), self.cursor, batch_size, self.seed)
        if device is not None:
            cols = [c.to(device) for c in cols]
        k = (len(cols) - 3) // 2  # the columns of an observation
        return (self._join(cols[:k]), cols[k], cols[k + 1], cols[k + 2], self._join(cols[k + 3:]))

    def reset(self):
        self.cursor.zero_()
        self._offered = 0

    @property
    def pos(self) -> int:
        """the slot the next experience goes to.  Reads the cursor back: synchronises with the device."""
        return int(self.cursor[A.HK_REPLAY_POS].item())

    @property
    def full(self) -> bool:
        """whether every slot has been written.  Reads the cursor back: synchronises with the device."""
        return bool(self.cursor[A.HK_REPLAY_FULL].item())
