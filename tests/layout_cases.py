"""Games, actions and oracle expectations shared by tests/test_gpu_layouts.py (the kernels on strided, offset and
record layouts) and the oracle's own layout consistency in tests/test_oracle.py.  numpy only: the results of every
operator are independent of the memory layout, so the expectation is the C oracle on the plain contiguous batch,
computed once per (shape, batch, dtype, configuration) and shared by every layout and kernel family."""
import functools

import numpy as np

from hironaka_amd import _abi as A
from oracle import c_oracle as CO
from oracle import np_oracle as NO

# (max_points, dim, dtype): every vector width W of the slab I/O (4, 2, 1 by m*d % 4, % 2) and every kernel family
SHAPES = [(20, 3, np.float32), (20, 4, np.float32), (10, 3, np.float32), (5, 3, np.float32), (8, 4, np.float32),
          (50, 4, np.float32), (7, 3, np.float32), (9, 7, np.float32), (20, 3, np.float64)]
BATCHES = (1, 33, 64, 193, 1000)  # partial waves of 16 / 32 / 64 games, one full wave, several workgroups

# name -> (semantics, noop_if_invalid, ignore_ended, compact_sorted, stages)
STEP_CONFIGS = {
    "jax7": ("jax", False, False, False, 7),
    "jax15": ("jax", False, False, False, 15),
    "torch7": ("torch", True, True, False, 7),
    "torch15": ("torch", True, True, False, 15),
    "list": ("list", True, False, True, A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON),  # sorted + compacted: the StepAux kernels
}


def config_flags(name):
    sem, noop, ign, compact, _ = STEP_CONFIGS[name]
    return CO.flags_of(sem=sem, noop_if_invalid=noop, ignore_ended=ign, compact_sorted=compact)


def shape_id(shape):
    m, d, dtype = shape
    return f"{m}x{d}" + ("_f64" if dtype == np.float64 else "")


@functools.lru_cache(maxsize=None)
def states(m, d, b, dtype):
    """[b, m, d]: even games Newton-reduced (the generator's output), odd games random small integers with holes
    (ties, padding rows anywhere); from three games on: game 0 holds one point, game 1 none, game 2 is dense."""
    rng = np.random.default_rng(1000 * m + 10 * d + b)
    p = CO.generate_points(b, m, d, 20, 17, dtype=dtype)
    odd = rng.integers(0, 6, (b, m, d)).astype(dtype)
    odd[rng.random((b, m)) < 0.3] = -1.0
    p[1::2] = odd[1::2]
    if b >= 3:
        p[0, 1:] = -1.0
        p[0, 0] = rng.integers(1, 6, d)
        p[1] = -1.0
        p[2] = rng.integers(0, 20, (m, d))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def actions(m, d, b):
    """(class ids int32 [b], axis int32 [b], the classes' 0/1 masks float32 [b, d])"""
    rng = np.random.default_rng(77 * m + d + 3 * b)
    cls = rng.integers(0, 2 ** d - d - 1, b).astype(np.int32)
    ax = rng.integers(0, d, b).astype(np.int32)
    mask = NO.decode_class(cls, d).astype(np.float32)
    for a in (cls, ax, mask):
        a.setflags(write=False)
    return cls, ax, mask


@functools.lru_cache(maxsize=None)
def expected_step(m, d, b, dtype, name):
    """hk_step under STEP_CONFIGS[name] on the contiguous batch with class-id coords: points [b, m, d] + the side outputs"""
    cls, ax, _ = actions(m, d, b)
    return CO.step(states(m, d, b, dtype), cls, ax, stages=STEP_CONFIGS[name][4], flags=config_flags(name),
                   reward_sign=-1.0)


def records(p, tail):
    """[b, m*d + d] agent observations: the points followed by `tail` ([b, d]), as functional.make_agent_obs lays them out"""
    b = p.shape[0]
    return np.concatenate([p.reshape(b, -1), tail.astype(p.dtype)], axis=1)
