"""Torch-tensor front end of the HIP operators (``include/hironaka_hip.h``).

Tensors are used for device memory and streams only; every function validates its arguments,
fills a C descriptor, calls the C ABI on the current HIP stream and raises on a non-zero status.
There is no CPU path: a non-CUDA tensor is a TypeError.

Operator names follow the reference's operator layer (hironaka/src/__init__.py:22-46):
``shift``, ``get_newton_polytope``, ``reposition``, ``rescale`` with ``sem`` selecting which
sibling's semantics is reproduced ("jax" = _jax_ops.py, "torch" = _torch_ops.py, "list" =
_list_ops.py on padded arrays).
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _abi as A
from ._lib import check, lib

_TORCH2HK = {torch.float32: A.HK_F32, torch.float64: A.HK_F64, torch.int32: A.HK_I32,
             torch.int64: A.HK_I64, torch.uint8: A.HK_U8, torch.bool: A.HK_U8}
ALL_STAGES = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON | A.HK_STAGE_RESCALE


# kernel-selection flags OR-ed into every step / rollout descriptor (tests: `with ops.forced(...)`)
_forced_flags = 0


@contextlib.contextmanager
def forced(flags: int):
    """Run the enclosed calls with kernel-selection flags (HK_FLAG_FORCE_ONE_LANE / _TEAM / _GENERIC) added to
    every step and rollout launch -- the results must not depend on them."""
    global _forced_flags
    before, _forced_flags = _forced_flags, _forced_flags | flags
    try:
        yield
    finally:
        _forced_flags = before


def make_flags(sem: str = "jax", noop_if_invalid: bool = False, ignore_ended: bool = False,
               compact_sorted: bool = False, force_generic: bool = False, force_team: bool = False) -> int:
    if sem not in A.SEMANTICS:
        raise ValueError(f"sem must be one of {sorted(A.SEMANTICS)}. Got {sem}.")
    f = A.SEMANTICS[sem]
    if noop_if_invalid:
        f |= A.HK_FLAG_AXIS_NOOP_IF_INVALID
    if ignore_ended:
        f |= A.HK_FLAG_IGNORE_ENDED
    if compact_sorted:
        f |= A.HK_FLAG_COMPACT_SORTED
    if force_generic:
        f |= A.HK_FLAG_FORCE_GENERIC
    if force_team:
        f |= A.HK_FLAG_FORCE_TEAM
    return f


def make_stages(shift=False, reposition=False, newton=False, rescale=False) -> int:
    return ((A.HK_STAGE_SHIFT if shift else 0) | (A.HK_STAGE_REPOSITION if reposition else 0)
            | (A.HK_STAGE_NEWTON if newton else 0) | (A.HK_STAGE_RESCALE if rescale else 0))


def _require_device(t: torch.Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor on a HIP device. Got {type(t)}.")
    if not t.is_cuda:
        raise TypeError(f"{name} must live on a HIP device (hironaka_amd has no CPU path). Got {t.device}.")


def _state(points: torch.Tensor, name="points") -> Tuple[torch.Tensor, torch.dtype]:
    """contiguous f32/f64 view of the state + the dtype to hand back"""
    _require_device(points, name)
    orig = points.dtype
    if orig in (torch.float16, torch.bfloat16):
        points = points.float()
    elif orig not in (torch.float32, torch.float64):
        raise TypeError(f"{name} must be a floating tensor. Got {orig}.")
    return points.contiguous(), orig


def _batch_spec(pts: torch.Tensor, spec: Optional[Tuple[int, int]]) -> Tuple[int, int, int, int]:
    """(B, m, d, stride) of states given as [B, m, d], or as [B, stride] records together with spec=(m, d)"""
    if pts.dim() == 3:
        b, m, d = pts.shape
        return b, m, d, m * d
    if pts.dim() == 2 and spec is not None:
        m, d = spec
        return pts.shape[0], m, d, pts.shape[1]
    raise ValueError("points must be [B, m, d], or [B, stride] together with spec=(m, d)")


def _stream(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _aux(t: Optional[torch.Tensor], like: torch.Tensor, name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t, device=like.device)
    _require_device(t, name)
    if t.device != like.device:
        raise ValueError(f"{name} is on {t.device}, points on {like.device}")
    if t.dtype in (torch.float16, torch.bfloat16):
        t = t.float()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype not in _TORCH2HK:
        raise TypeError(f"{name}: unsupported dtype {t.dtype}")
    return t.contiguous()


def step(points: torch.Tensor, coords=None, axis=None, *, stages: int, flags: int = 0,
         padding_value: float = -1.0, reward_sign: float = 1.0, spec: Optional[Tuple[int, int]] = None,
         coords_in_record: bool = False, out: Optional[torch.Tensor] = None,
         want: Sequence[str] = (), features_out: Optional[torch.Tensor] = None,
         scale_observation: bool = True) -> Dict[str, torch.Tensor]:
    """One fused transition (hk_step).

    points: [B, m, d] state, or a [B, stride] record matrix with ``spec=(m, d)`` (flattened host
        observation, or agent observation whose last d columns are the subset mask --
        ``coords_in_record=True``; jax/util.py:58-74).
    coords: [B, d] multi-binary mask (any numeric dtype) or [B] class ids (int32/int64).
    axis: [B] int or float; or [B, d] float32 logits of the agent (with class-id coords): its move is the argmax over
        the subset's coordinates, decoded inside the kernel (shapes with a four-lane step kernel only).
    want: any of "done", "prev_done", "reward", "num_points".
    features_out: [B, m*d] contiguous float32 -- the observation features of the RESULT (get_features of the new
        points, rescaled first if `scale_observation`) written by the same launch (hk_step_features: shapes with a
        four-lane step kernel, class-id coords; HironakaHipError(HK_ERR_UNSUPPORTED) otherwise).
    Returns {"points": [B, m, d] (or `out`), ...}."""
    pts, orig = _state(points)
    b, m, d, in_stride = _batch_spec(pts, spec)
    dev = pts.device
    s = A.hk_step_desc()
    if out is None:
        out_t = torch.empty((b, m, d), dtype=pts.dtype, device=dev)
        out_stride = m * d
    else:
        _require_device(out, "out")
        if out.dtype != pts.dtype or not out.is_contiguous() or out.shape[0] != b:
            raise ValueError("out must be contiguous, of the state dtype and batch")
        out_t = out
        out_stride = out.numel() // max(b, 1)
    keep = [pts, out_t]
    s.points_in, s.points_out = pts.data_ptr(), out_t.data_ptr()
    s.in_stride, s.out_stride = in_stride, out_stride
    s.coords_kind = A.HK_COORDS_NONE
    if stages & A.HK_STAGE_SHIFT:
        ax = _aux(axis, pts, "axis")
        if ax is not None and ax.dim() == 2:
            # [B, d] float32 logits of the agent: its move is the argmax over the subset's coordinates
            # (HK_AXIS_MASKED_LOGITS; four-lane step kernel only -- HironakaHipError(HK_ERR_UNSUPPORTED) otherwise)
            if ax.shape != (b, d) or ax.dtype != torch.float32 or not ax.is_contiguous():
                raise ValueError(f"agent logits must be a contiguous float32 tensor of shape ({b}, {d})")
            keep.append(ax)
            s.axis, s.axis_dtype = ax.data_ptr(), A.HK_AXIS_MASKED_LOGITS
        else:
            if ax is None or ax.shape != (b,):
                raise ValueError(f"axis must have shape ({b},)")
            if ax.dtype == torch.uint8:
                ax = ax.to(torch.int32)
            keep.append(ax)
            s.axis, s.axis_dtype = ax.data_ptr(), _TORCH2HK[ax.dtype]
        if coords_in_record:
            s.coords_kind = A.HK_COORDS_IN_RECORD
        else:
            co = _aux(coords, pts, "coords")
            if co is None:
                raise ValueError("coords is required for the shift stage")
            keep.append(co)
            if co.dim() == 1:
                if co.shape != (b,) or co.dtype not in (torch.int32, torch.int64):
                    raise ValueError("class-id coords must be int32/int64 of shape (B,)")
                s.coords_kind = A.HK_COORDS_CLASS_I32 if co.dtype == torch.int32 else A.HK_COORDS_CLASS_I64
            elif co.shape == (b, d):
                s.coords_kind = _TORCH2HK[co.dtype]
                s.coords_stride = d
            else:
                raise ValueError(f"coords must have shape ({b}, {d}) or ({b},)")
            s.coords = co.data_ptr()
    res: Dict[str, torch.Tensor] = {}
    for key in want:
        if key in ("done", "prev_done"):
            res[key] = torch.empty(b, dtype=torch.bool, device=dev)  # the kernel stores 0/1 bytes
        elif key == "reward":
            res[key] = torch.empty(b, dtype=torch.float32, device=dev)
        elif key == "num_points":
            res[key] = torch.empty(b, dtype=torch.int32, device=dev)
        else:
            raise ValueError(f"unknown output {key}")
    s.done_out = res["done"].data_ptr() if "done" in res else None
    s.prev_done_out = res["prev_done"].data_ptr() if "prev_done" in res else None
    s.reward_out = res["reward"].data_ptr() if "reward" in res else None
    s.num_points_out = res["num_points"].data_ptr() if "num_points" in res else None
    s.padding_value, s.reward_sign = float(padding_value), float(reward_sign)
    s.batch, s.max_points, s.dim, s.dtype = b, m, d, _TORCH2HK[pts.dtype]
    s.stages, s.flags = stages, flags | _forced_flags
    with torch.cuda.device(dev):
        if features_out is not None:
            if (not features_out.is_cuda or features_out.dtype != torch.float32 or not features_out.is_contiguous()
                    or tuple(features_out.shape) != (b, m * d)):
                raise ValueError(f"features_out must be a contiguous float32 [{b}, {m * d}] tensor on the device")
            check(lib().hk_step_features(C.byref(s), features_out.data_ptr(), int(bool(scale_observation)),
                                         _stream(pts)), "hk_step_features")
            res["features"] = features_out
        else:
            check(lib().hk_step(C.byref(s), _stream(pts)), "hk_step")
    if out is None and orig != out_t.dtype:
        out_t = out_t.to(orig)
    res["points"] = out_t
    return res


def shift(points, coords, axis, padding_value: float = -1.0, sem: str = "jax", noop_if_invalid=False,
          ignore_ended=False, **kw) -> torch.Tensor:
    """shift_jax / shift_torch / shift_lst (see include/hironaka_hip.h)."""
    return step(points, coords, axis, stages=A.HK_STAGE_SHIFT, padding_value=padding_value,
                flags=make_flags(sem, noop_if_invalid, ignore_ended, **kw))["points"]


def reposition(points, padding_value: float = -1.0, sem: str = "jax", **kw) -> torch.Tensor:
    return step(points, stages=A.HK_STAGE_REPOSITION, padding_value=padding_value,
                flags=make_flags(sem, **kw))["points"]


def get_newton_polytope(points, padding_value: float = -1.0, sem: str = "jax", compact_sorted=False,
                        **kw) -> torch.Tensor:
    return step(points, stages=A.HK_STAGE_NEWTON, padding_value=padding_value,
                flags=make_flags(sem, compact_sorted=compact_sorted, **kw))["points"]


def rescale(points, padding_value: float = -1.0, sem: str = "jax", **kw) -> torch.Tensor:
    return step(points, stages=A.HK_STAGE_RESCALE, padding_value=padding_value,
                flags=make_flags(sem, **kw))["points"]


def _counts(points: torch.Tensor, spec, fn_name: str, out_dtype) -> torch.Tensor:
    pts, _ = _state(points)
    b, m, d, stride = _batch_spec(pts, spec)
    out = torch.empty(b, dtype=out_dtype, device=pts.device)
    with torch.cuda.device(pts.device):
        check(getattr(lib(), fn_name)(pts.data_ptr(), stride, out.data_ptr(), b, m, d,
                                      _TORCH2HK[pts.dtype], _stream(pts)), fn_name)
    return out


def get_dones(points: torch.Tensor, spec=None) -> torch.Tensor:
    """(#rows with x_0 >= 0) < 2 -- jax/util.py:34-35."""
    return _counts(points, spec, "hk_get_dones", torch.bool)  # 0/1 bytes


def get_num_points(points: torch.Tensor, spec=None) -> torch.Tensor:
    """core/tensor_points.py:65-70."""
    return _counts(points, spec, "hk_get_num_points", torch.int32)


def decode_host_class(cls: torch.Tensor, dim: int, dtype=torch.float32) -> torch.Tensor:
    """class ids -> multi-binary masks (jax/host_action_preprocess.py:59-65)."""
    _require_device(cls, "cls")
    ids = cls.to(torch.int32).contiguous()
    n_cls = 2 ** dim - dim - 1
    out = torch.empty((ids.numel(), dim), dtype=dtype, device=ids.device)
    if dtype not in _TORCH2HK:
        raise TypeError(f"unsupported mask dtype {dtype}")
    with torch.cuda.device(ids.device):
        check(lib().hk_decode_host_class(ids.data_ptr(), out.data_ptr(), _TORCH2HK[dtype], ids.numel(), dim,
                                         _stream(ids)), "hk_decode_host_class")
    return out.reshape(*cls.shape, dim)


def zeillinger(points: torch.Tensor, sem: str = "jax", spec=None, force_generic: bool = False,
               force_team: bool = False) -> torch.Tensor:
    """Zeillinger host: class id per game.  sem="jax": jax/players.py:84-109 (degenerate -> 0);
    sem="list": host.py:70-95 on padded rows (-1 for a game with fewer than 2 points).
    points: [B, m, d], or [B, stride] records with spec=(m, d) (e.g. agent observations)."""
    if sem not in ("jax", "list"):
        raise ValueError(f"sem must be 'jax' or 'list'. Got {sem}.")
    pts, _ = _state(points)
    b, m, d, stride = _batch_spec(pts, spec)
    out = torch.empty(b, dtype=torch.int32, device=pts.device)
    flags = (A.SEMANTICS[sem] | (A.HK_FLAG_FORCE_GENERIC if force_generic else 0)
             | (A.HK_FLAG_FORCE_TEAM if force_team else 0))
    with torch.cuda.device(pts.device):
        check(lib().hk_zeillinger(pts.data_ptr(), stride, out.data_ptr(), b, m, d, _TORCH2HK[pts.dtype],
                                  flags, _stream(pts)), "hk_zeillinger")
    return out


# the fixed hosts, under the two names their operators grew up with
HOSTS = SEARCH_HOSTS = {"all_coord": A.HK_HOST_ALL_COORD, "zeillinger": A.HK_HOST_ZEILLINGER,
                        "zeillinger_lex": A.HK_HOST_ZEILLINGER_LEX, "weak_spivakovsky": A.HK_HOST_WEAK_SPIVAKOVSKY,
                        "weak_spivakovsky_min_hitting": A.HK_HOST_MIN_HITTING}


def host_select(points: torch.Tensor, host: str, spec=None) -> torch.Tensor:
    """The class id a deterministic host of hironaka/host.py picks per game, in list semantics (hk_host_select):
    "all_coord", "zeillinger" (== zeillinger(sem="list")), "zeillinger_lex", "weak_spivakovsky",
    "weak_spivakovsky_min_hitting".  -1 = no subset (fewer than 2 points; a zero row or fewer than 2 nonzero
    coordinates in all for the hitting-set hosts, see include/hironaka_hip_hosts.h).  dim 2..6, up to 64 points.
    points: [B, m, d], or [B, stride] records with spec=(m, d)."""
    if host not in HOSTS:
        raise ValueError(f"host must be one of {sorted(HOSTS)}. Got {host!r}.")
    pts, _ = _state(points)
    b, m, d, stride = _batch_spec(pts, spec)
    out = torch.empty(b, dtype=torch.int32, device=pts.device)
    with torch.cuda.device(pts.device):
        check(lib().hk_host_select(pts.data_ptr(), stride, out.data_ptr(), b, m, d, _TORCH2HK[pts.dtype], HOSTS[host],
                                   _stream(pts)), "hk_host_select")
    return out


# the hosts of hk_spivakovsky_select, which answers with bit masks: their subsets may hold fewer than 2 coordinates
SPIVAKOVSKY_HOSTS = {"spivakovsky": A.HK_HOST_SPIVAKOVSKY, "random_spivakovsky": A.HK_HOST_RANDOM_SPIVAKOVSKY}


def spivakovsky_select(points: torch.Tensor, host: str, spec=None, seed: int = 0, game_offset: int = 0,
                       step: int = 0) -> torch.Tensor:
    """The subset Spivakovsky's host (hironaka/host.py:130-290) or RandomSpivakovsky (host.py:293-354) picks per game,
    in list semantics (hk_spivakovsky_select), as an int32 bit mask [B] (bit k <-> coordinate k).  "spivakovsky" may
    give 0 or 1 coordinates, as the reference does; fewer than 2 points give 0, and so does "random_spivakovsky" on a
    zero row.  "random_spivakovsky" draws candidate number (word * n) >> 32, word = the first word of the Philox block
    (game_offset + g, step, stream 5) under seed; "spivakovsky" ignores the three.  dim 2..6, up to 64 points.
    points: [B, m, d], or [B, stride] records with spec=(m, d)."""
    if host not in SPIVAKOVSKY_HOSTS:
        raise ValueError(f"host must be one of {sorted(SPIVAKOVSKY_HOSTS)}. Got {host!r}.")
    if not (0 <= seed < 2 ** 64 and 0 <= game_offset < 2 ** 64 and 0 <= step < 2 ** 32):
        raise ValueError(f"seed and game_offset must fit 64 bits, step 32. Got {seed}, {game_offset}, {step}.")
    pts, _ = _state(points)
    b, m, d, stride = _batch_spec(pts, spec)
    out = torch.empty(b, dtype=torch.int32, device=pts.device)
    with torch.cuda.device(pts.device):
        check(lib().hk_spivakovsky_select(pts.data_ptr(), stride, out.data_ptr(), b, m, d, _TORCH2HK[pts.dtype],
                                          SPIVAKOVSKY_HOSTS[host], seed, game_offset, step, _stream(pts)),
              "hk_spivakovsky_select")
    return out


def get_features(points: torch.Tensor, scale_observation: bool = True, padding_value: float = -1.0,
                 spec=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """order_and_rescale (jax/util.py:186-197): [B, m*d] rows sorted descending, last coordinate
    primary, optionally rescaled first."""
    pts, orig = _state(points)
    b, m, d, in_stride = _batch_spec(pts, spec)
    if out is None:
        out = torch.empty((b, m * d), dtype=pts.dtype, device=pts.device)
    elif (not out.is_cuda or out.dtype != pts.dtype or tuple(out.shape) != (b, m * d) or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous [{b}, {m * d}] {pts.dtype} tensor on the device")
    with torch.cuda.device(pts.device):
        check(lib().hk_get_features(pts.data_ptr(), in_stride, out.data_ptr(), m * d, b, m, d,
                                    _TORCH2HK[pts.dtype], int(bool(scale_observation)), float(padding_value),
                                    _stream(pts)), "hk_get_features")
    return out if orig == out.dtype else out.to(orig)


def get_features_torch(points: torch.Tensor, padding_value: float = -1.0) -> torch.Tensor:
    """TensorPoints.get_features (core/tensor_points.py:72-74): [B, m, d] rows ordered by coordinate 0,
    descending (unavailable rows last); rows with equal coordinate 0 keep their order."""
    pts, orig = _state(points)
    if pts.dim() != 3:
        raise ValueError(f"points must be [B, m, d]. Got {tuple(pts.shape)}.")
    b, m, d = pts.shape
    out = torch.empty_like(pts)
    with torch.cuda.device(pts.device):
        check(lib().hk_get_features_torch(pts.data_ptr(), m * d, out.data_ptr(), m * d, b, m, d,
                                          _TORCH2HK[pts.dtype], float(padding_value), _stream(pts)),
              "hk_get_features_torch")
    return out if orig == out.dtype else out.to(orig)


def generate_points(batch: int, max_points: int, dim: int, max_value: int, seed: int, *,
                    game_offset: int = 0, dtype=torch.float32, device=None, newton=True, reposition=True,
                    rescale=False, padding_value: float = -1.0, flags: int = 0,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """generate_pts (jax/util.py:385-392): randint[0, max_value) -> newton -> [reposition] ->
    [rescale], Philox-keyed by (seed, game_offset + game index)."""
    if out is None:
        device = torch.device("cuda") if device is None else torch.device(device)
        if device.type != "cuda":
            raise TypeError("generate_points needs a HIP device")
        out = torch.empty((batch, max_points, dim), dtype=dtype, device=device)
    else:
        _require_device(out, "out")
    stages = make_stages(False, reposition, newton, rescale)
    with torch.cuda.device(out.device):
        check(lib().hk_generate_points(out.data_ptr(), batch, max_points, dim, _TORCH2HK[out.dtype], max_value,
                                       seed, game_offset, stages, float(padding_value), flags, _stream(out)),
              "hk_generate_points")
    return out


class _WorkspaceCache:
    """Per-(device, stream) zeroed uint8 memory for the kernels' counters and tickets, grown on demand (the C ABI never
    allocates); the key is the device's current stream, on which launches follow each other, and every launch leaves
    its workspace zero again.  A buffer that a larger request outgrows is retired, not freed: a hipGraph captured
    earlier may still hold its address.  Growing DURING a capture is refused with `refuse`; where that is None the
    request is served from the capture's own pool instead (its zero fill is captured with it): exactly `nbytes`,
    neither kept nor retiring anything."""

    def __init__(self, floor: int, refuse: Optional[str] = None):
        self.floor, self.refuse = floor, refuse
        self.live: Dict[Tuple[torch.device, int], torch.Tensor] = {}
        self.retired: list = []

    def get(self, dev: torch.device, nbytes: int) -> torch.Tensor:
        key = (dev, torch.cuda.current_stream(dev).cuda_stream)
        ws = self.live.get(key)
        if ws is None or ws.numel() < nbytes:
            if torch.cuda.is_current_stream_capturing():
                if self.refuse is not None:
                    raise RuntimeError(self.refuse)
                return torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            if ws is not None:
                self.retired.append(ws)
            ws = self.live[key] = torch.zeros(max(nbytes, self.floor), dtype=torch.uint8, device=dev)
        return ws


# hk_rollout's per-workgroup counters: allocate before capturing (one eager call of the same shape, or the caller's own
# `rollout_workspace` + `defer_counts`)
_ROLLOUT_WORKSPACES = _WorkspaceCache(1 << 16, "hk_rollout's counter workspace would have to be (re)allocated inside a "
                                      "stream capture: run the same rollout once eagerly on this stream first, or pass "
                                      "workspace=ops.rollout_workspace(...) with defer_counts=True")


def _geometry_desc(batch: int, steps: int, spec: Tuple[int, int], dtype, flags: int) -> "A.hk_rollout_desc":
    r = A.hk_rollout_desc()
    r.batch, r.max_points, r.dim, r.dtype, r.steps = batch, spec[0], spec[1], _TORCH2HK[dtype], steps
    r.host_policy, r.agent_policy, r.flags = A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM, flags | _forced_flags
    r.stages = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON
    return r


def rollout_workspace(batch: int, steps: int, spec: Tuple[int, int], dtype=torch.float32, device=None,
                      flags: int = 0) -> torch.Tensor:
    """A zeroed counter workspace of the caller's own, for rollouts with `defer_counts=True`."""
    dev = torch.device("cuda") if device is None else torch.device(device)
    r = _geometry_desc(batch, steps, spec, dtype, flags)
    probe = torch.empty(8, dtype=torch.uint8, device=dev)
    r.points = probe.data_ptr()
    need = lib().hk_rollout_workspace_bytes(C.byref(r))
    return torch.zeros(max(int(need), 8), dtype=torch.uint8, device=dev)


def reduce_counts(workspace: torch.Tensor, done_count: torch.Tensor, batch: int, steps: int,
                  spec: Tuple[int, int], dtype=torch.float32, flags: int = 0) -> torch.Tensor:
    """done_count += the partial counts that rollouts with `defer_counts=True` left in `workspace`
    (hk_rollout_reduce_counts); the workspace is zero afterwards."""
    _require_device(workspace, "workspace")
    _require_device(done_count, "done_count")
    if done_count.dtype != torch.int64 or done_count.numel() != steps + 1:
        raise ValueError("done_count must be an int64 device tensor of steps+1 elements")
    r = _geometry_desc(batch, steps, spec, dtype, flags)
    r.done_count = done_count.data_ptr()
    r.workspace, r.workspace_bytes = workspace.data_ptr(), workspace.numel()
    with torch.cuda.device(workspace.device):
        check(lib().hk_rollout_reduce_counts(C.byref(r), _stream(workspace)), "hk_rollout_reduce_counts")
    return done_count


def _rollout_counts(r: "A.hk_rollout_desc", res: Dict[str, torch.Tensor], batch: int, steps: int, dev: torch.device,
                    flags: int, game_ids: Optional[torch.Tensor], done_count: Optional[torch.Tensor],
                    defer_counts: bool, workspace: Optional[torch.Tensor]) -> int:
    """What rollout and rollout_generated share ahead of their descriptors: game_ids, and where the finished-game counts
    go -- deferred into the caller's workspace, or into done_count (a new one unless given), which then joins res.
    Fills r.game_ids and r.done_count; returns the flags."""
    if game_ids is not None:
        _require_device(game_ids, "game_ids")
        if (game_ids.dtype != torch.int32 or game_ids.shape != (batch,) or not game_ids.is_contiguous()
                or game_ids.device != dev):
            raise ValueError("game_ids must be a contiguous int32 [B] tensor on the device of the games")
        r.game_ids = game_ids.data_ptr()
    if defer_counts:
        if workspace is None:
            raise ValueError("defer_counts=True needs the caller's own workspace (ops.rollout_workspace)")
        _require_device(workspace, "workspace")
        flags |= A.HK_FLAG_DEFER_COUNTS
    elif done_count is None:
        done_count = torch.zeros(steps + 1, dtype=torch.int64, device=dev)
    elif done_count.dtype != torch.int64 or done_count.numel() != steps + 1 or not done_count.is_cuda:
        raise ValueError("done_count must be an int64 device tensor of steps+1 elements")
    if done_count is not None:
        res["done_count"] = done_count
    r.done_count = done_count.data_ptr() if (done_count is not None and not defer_counts) else None
    return flags


def _rollout_launch(r: "A.hk_rollout_desc", dev: torch.device, defer_counts: bool,
                    workspace: Optional[torch.Tensor]) -> None:
    """hk_rollout on the filled descriptor, with the caller's workspace or this stream's own"""
    with torch.cuda.device(dev):
        ws = workspace if defer_counts else _ROLLOUT_WORKSPACES.get(dev, lib().hk_rollout_workspace_bytes(C.byref(r)))
        r.workspace, r.workspace_bytes = ws.data_ptr(), ws.numel()
        check(lib().hk_rollout(C.byref(r), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "hk_rollout")


def rollout(points: torch.Tensor, steps: int, seed: int, *, game_offset: int = 0, step_offset: int = 0,
            host_policy: int = A.HK_HOST_RANDOM, agent_policy: int = A.HK_AGENT_RANDOM,
            stages: int = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON, flags: int = 0,
            padding_value: float = -1.0, reward_sign: float = 1.0, record: Sequence[str] = (),
            done_count: Optional[torch.Tensor] = None,
            initial: Optional[torch.Tensor] = None, defer_counts: bool = False,
            workspace: Optional[torch.Tensor] = None,
            game_ids: Optional[torch.Tensor] = None, episodes: int = 1) -> Dict[str, torch.Tensor]:
    """T fused steps with in-kernel policies (hk_rollout); `points` is updated IN PLACE.
    record: any of "obs", "host_class", "axis", "done", "reward", "game_length".
    done_count: optional uint64-as-int64 [steps+1] accumulator (zeroed by the caller).
    initial: optional tensor like `points` holding the starting state; it is left untouched and
        `points` only receives the final state (an episode restart without a device copy).
    defer_counts: leave the finished-game counts as partial sums in `workspace` (from `rollout_workspace`;
        they accumulate over launches) and skip the reduce kernel; `reduce_counts` adds them to a
        done_count later -- one reduction for many rollouts.
    game_ids: optional int32 [B]: the policy stream of the game at position g is keyed by game_offset + game_ids[g]
        (a batch re-ordered by `bin_by_live_rows` rolls out game by game as the original order would).
    episodes: E > 1 (needs `initial`, no per-step records): E episodes back to back, each from `initial` with seed + e;
        the counts accumulate, `points` and game_length are the last episode's (hk_rollout_desc.episodes: one launch
        where the four-lane kernel's waves are all resident, else one launch per episode inside the library)."""
    _require_device(points, "points")
    if points.dtype not in (torch.float32, torch.float64) or not points.is_contiguous() or points.dim() != 3:
        raise ValueError("rollout updates a contiguous [B, m, d] float32/float64 tensor in place")
    b, m, d = points.shape
    dev = points.device
    if initial is not None:
        _require_device(initial, "initial")
        if (initial.shape != points.shape or initial.dtype != points.dtype or not initial.is_contiguous()
                or initial.device != dev):
            raise ValueError("initial must match points in shape, dtype, device and be contiguous")
    r = A.hk_rollout_desc()
    res: Dict[str, torch.Tensor] = {}
    flags = _rollout_counts(r, res, b, steps, dev, flags, game_ids, done_count, defer_counts, workspace)
    for key in record:
        if key == "obs":
            res[key] = torch.empty((steps, b, m, d), dtype=points.dtype, device=dev)
        elif key in ("host_class", "axis"):
            res[key] = torch.empty((steps, b), dtype=torch.int32, device=dev)
        elif key == "done":
            res[key] = torch.empty((steps, b), dtype=torch.bool, device=dev)  # 0/1 bytes
        elif key == "reward":
            res[key] = torch.empty((steps, b), dtype=torch.float32, device=dev)
        elif key == "game_length":
            res[key] = torch.empty(b, dtype=torch.int32, device=dev)
        else:
            raise ValueError(f"unknown record {key}")
    ptr = lambda k: res[k].data_ptr() if k in res else None
    r.points = points.data_ptr()
    r.points_in = initial.data_ptr() if initial is not None else None
    r.obs_out, r.host_class_out, r.axis_out = ptr("obs"), ptr("host_class"), ptr("axis")
    r.done_out, r.reward_out, r.game_length_out = ptr("done"), ptr("reward"), ptr("game_length")
    r.seed, r.game_offset, r.step_offset = seed, game_offset, step_offset
    r.padding_value, r.reward_sign = float(padding_value), float(reward_sign)
    r.batch, r.max_points, r.dim, r.dtype, r.steps = b, m, d, _TORCH2HK[points.dtype], steps
    r.host_policy, r.agent_policy, r.stages, r.flags = host_policy, agent_policy, stages, flags | _forced_flags
    r.episodes = int(episodes)
    _rollout_launch(r, dev, defer_counts, workspace)
    res["points"] = points
    return res


def rollout_generated(batch: int, spec: Tuple[int, int], steps: int, seed: int, *, max_value: int,
                      gen_seed: Optional[int] = None, newton: bool = True, reposition: bool = True, rescale: bool = False,
                      episodes: int = 1, game_offset: int = 0, step_offset: int = 0,
                      host_policy: int = A.HK_HOST_RANDOM, agent_policy: int = A.HK_AGENT_RANDOM,
                      stages: int = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON, flags: int = 0,
                      padding_value: float = -1.0, dtype=torch.float32, device=None,
                      out: Optional[torch.Tensor] = None, record: Sequence[str] = (),
                      done_count: Optional[torch.Tensor] = None, defer_counts: bool = False,
                      workspace: Optional[torch.Tensor] = None,
                      game_ids: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """hk_rollout from initial states drawn INSIDE the launch (hk_rollout_desc.gen_max_value, ABI 4): what
    `generate_points(batch, m, d, max_value, gen_seed, ...)` followed by `rollout(..., steps, seed)` computes, without
    the state ever touching memory -- the loop body of JAXTrainer.compute_rho (jax_trainer.py:502-555), `episodes` of them
    back to back (episode e: seed + e, gen_seed + e; the counts accumulate).  `out`: optional [B, m, d] tensor for the
    final state of the last episode (None: "counts only").  record: "game_length" (the last episode's).
    Requests the fused kernel does not serve (other shapes / dtypes / flags) run as generate + rollout per episode
    inside the library and then need `out`; without it they raise HironakaHipError(HK_ERR_UNSUPPORTED)."""
    m, d = spec
    dev = out.device if out is not None else (torch.device("cuda") if device is None else torch.device(device))
    if dev.type != "cuda":
        raise TypeError("rollout_generated needs a HIP device")
    if out is not None:
        _require_device(out, "out")
        if out.shape != (batch, m, d) or not out.is_contiguous():
            raise ValueError("out must be a contiguous [B, m, d] tensor")
        dtype = out.dtype
    r = A.hk_rollout_desc()
    res: Dict[str, torch.Tensor] = {}
    flags = _rollout_counts(r, res, batch, steps, dev, flags, game_ids, done_count, defer_counts, workspace)
    for key in record:
        if key != "game_length":
            raise ValueError(f"rollout_generated records game_length only. Got {key}.")
        res[key] = torch.empty(batch, dtype=torch.int32, device=dev)
    r.points = out.data_ptr() if out is not None else None
    r.game_length_out = res["game_length"].data_ptr() if "game_length" in res else None
    r.seed, r.game_offset, r.step_offset = seed, game_offset, step_offset
    r.padding_value, r.reward_sign = float(padding_value), 1.0
    r.batch, r.max_points, r.dim, r.dtype, r.steps = batch, m, d, _TORCH2HK[dtype], steps
    r.host_policy, r.agent_policy, r.stages, r.flags = host_policy, agent_policy, stages, flags | _forced_flags
    r.gen_max_value, r.gen_seed = int(max_value), int(seed if gen_seed is None else gen_seed)
    r.gen_stages, r.episodes = make_stages(False, reposition, newton, rescale), int(episodes)
    _rollout_launch(r, dev, defer_counts, workspace)
    if out is not None:
        res["points"] = out
    return res


def bin_group(max_points: int, dim: int, dtype=torch.float32) -> Tuple[int, int]:
    """(games per group, games per unit) of the on-device binning for a shape; (0, 0): no binning kernel."""
    code = _TORCH2HK.get(dtype, -1)
    return int(lib().hk_bin_group_games(max_points, dim, code)), int(lib().hk_bin_unit_games(max_points, dim, code))


def bin_by_live_rows(points: torch.Tensor, out: Optional[torch.Tensor] = None,
                     want_num_points: bool = False):
    """Games re-ordered by their number of live rows and the permutation as int32 `game_ids` (position -> original
    index) for `rollout(..., game_ids=)`: a wave of the rollout kernels then holds games of one size -- its slots per lane
    are the widest game's -- and every game keeps its policy stream, so the re-ordered batch rolls out exactly as the
    original one, game by game (the reference's batches carry no order: jax/util.py:385-392 draws them at random).
    ONE launch (hk_bin_by_live_rows, ABI 4) on the shapes with a four-lane kernel: the order is local to groups of
    `bin_group(...)[0]` consecutive games -- widest first, equal games in their order --, and the k-th sixteen games of
    all groups lie together in the output, the widest stratum first (include/hironaka_hip.h).  Other shapes / dtypes: a
    global stable sort with the tensor library.
    Returns (binned points, game_ids) or, with want_num_points, (binned points, game_ids, live rows per position)."""
    _require_device(points, "points")
    if points.dim() != 3:
        raise ValueError("points must be [B, m, d]")
    b, m, d = points.shape
    if points.is_contiguous() and bin_group(m, d, points.dtype)[0]:
        out = torch.empty_like(points) if out is None else out
        if out.data_ptr() == points.data_ptr():
            raise ValueError("bin_by_live_rows cannot work in place: a group's games leave for every stratum")
        ids = torch.empty(b, dtype=torch.int32, device=points.device)
        npts = torch.empty(b, dtype=torch.int32, device=points.device) if want_num_points else None
        with torch.cuda.device(points.device):
            check(lib().hk_bin_by_live_rows(points.data_ptr(), out.data_ptr(), ids.data_ptr(),
                                            npts.data_ptr() if npts is not None else None, b, m, d,
                                            _TORCH2HK[points.dtype], _stream(points)), "hk_bin_by_live_rows")
        return (out, ids, npts) if want_num_points else (out, ids)
    counts = get_num_points(points)
    order = torch.argsort(counts, descending=True, stable=True)
    binned = points.index_select(0, order).contiguous()
    if out is not None:
        out.copy_(binned)
        binned = out
    ids = order.to(torch.int32)
    return (binned, ids, counts.index_select(0, order)) if want_num_points else (binned, ids)


def generate_points_binned(batch: int, max_points: int, dim: int, max_value: int, seed: int, *, game_offset: int = 0,
                           device=None, newton=True, reposition=True, rescale=False, padding_value: float = -1.0,
                           flags: int = 0, out: Optional[torch.Tensor] = None, want_num_points: bool = False):
    """generate_points + bin_by_live_rows as ONE launch (hk_generate_points_binned): the generator has every game's
    rows in registers when it knows their count.  float32, the shapes with a four-lane kernel (HironakaHipError
    otherwise: generate_points + bin_by_live_rows).  Returns (points, game_ids[, live rows per position])."""
    dev = out.device if out is not None else (torch.device("cuda") if device is None else torch.device(device))
    if out is None:
        out = torch.empty((batch, max_points, dim), dtype=torch.float32, device=dev)
    else:
        _require_device(out, "out")
    ids = torch.empty(batch, dtype=torch.int32, device=dev)
    npts = torch.empty(batch, dtype=torch.int32, device=dev) if want_num_points else None
    stages = make_stages(False, reposition, newton, rescale)
    with torch.cuda.device(dev):
        check(lib().hk_generate_points_binned(out.data_ptr(), ids.data_ptr(), npts.data_ptr() if npts is not None else None,
                                              batch, max_points, dim, _TORCH2HK[out.dtype], max_value, seed, game_offset,
                                              stages, float(padding_value), flags | _forced_flags, _stream(out)),
              "hk_generate_points_binned")
    return (out, ids, npts) if want_num_points else (out, ids)


def has_fast_path(max_points: int, dim: int, dtype=torch.float32) -> bool:
    return bool(lib().hk_has_fast_path(max_points, dim, _TORCH2HK.get(dtype, -1)))


_SEARCH_WORKSPACE_BYTES = 4 << 30  # per launch; a larger batch runs as several launches


def _search_roots(points: torch.Tensor) -> torch.Tensor:
    """the roots of hk_search_depth / hk_search_game_tree, contiguous; their points must be exact integers"""
    pts = points.contiguous()
    limit = 2.0 ** 24 if pts.dtype == torch.float32 else 2.0 ** 53
    avail = (pts[:, :, 0] >= 0).unsqueeze(2).expand_as(pts)
    vals = pts[avail]
    if vals.numel() and not bool(((vals >= 0) & (vals < limit) & (vals == torch.floor(vals))).all()):
        raise ValueError(f"the points of a root (rows with coordinate 0 >= 0) must be integers in [0, {int(limit)}) "
                         f"for {pts.dtype}")
    return pts


def _search_checks(points: torch.Tensor, host: str, max_depth: int, max_nodes: int, stack_nodes: int, node_bits: int,
                   expand_limit: Optional[int] = None) -> torch.Tensor:
    """the argument checks of search_depth / search_game_tree (max_nodes < 2^node_bits); returns the roots"""
    _require_device(points, "points")
    if points.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"points must be float32 or float64. Got {points.dtype}.")
    if points.dim() != 3:
        raise ValueError(f"points must be [B, max_points, dim]. Got shape {tuple(points.shape)}.")
    if host not in SEARCH_HOSTS:
        raise ValueError(f"host must be one of {sorted(SEARCH_HOSTS)}. Got {host!r}.")
    if expand_limit is not None and not 0 <= expand_limit < 2 ** 63:
        raise ValueError(f"expand_limit must be None or in [0, 2^63). Got {expand_limit}.")
    if not (0 <= max_depth < 2 ** 31 and 1 <= max_nodes < 2 ** node_bits and 1 <= stack_nodes < 2 ** 31):
        raise ValueError(f"need 0 <= max_depth < 2^31, 1 <= max_nodes < 2^{node_bits}, 1 <= stack_nodes < 2^31. Got "
                         f"{max_depth}, {max_nodes}, {stack_nodes}.")
    return _search_roots(points)


def _search_launch(fn, name: str, pts: torch.Tensor, host: str, params: tuple, per_root: int, outs: list,
                   extra: Sequence[torch.Tensor] = ()) -> list:
    """fn(points, *extra, batch, m, d, dtype, host, *params, workspace, workspace_bytes, *outs, stream) over the roots,
    in chunks that share one workspace of at most _SEARCH_WORKSPACE_BYTES.  per_root == 0: the C entry refuses the
    arguments; one call with batch 1 and no buffers raises its status.  outs: (shape, dtype, fill or None) of each
    output, batch first, or None for an output not wanted; they are made once the arguments pass, and returned.
    extra: further inputs per root, batch first."""
    b, m, d = pts.shape
    head = (m, d, _TORCH2HK[pts.dtype], SEARCH_HOSTS[host], *params)
    if per_root == 0:
        check(fn(*([None] * (1 + len(extra))), 1, *head, None, 0, *([None] * len(outs)), None), name)
    outs = [None if o is None else torch.empty(o[0], dtype=o[1], device=pts.device) if o[2] is None else
            torch.full(o[0], o[2], dtype=o[1], device=pts.device) for o in outs]
    chunk = max(1, min(b, _SEARCH_WORKSPACE_BYTES // max(per_root, 1)))
    with torch.cuda.device(pts.device):
        ws = torch.empty(per_root * chunk if b else 0, dtype=torch.uint8, device=pts.device)
        for lo in range(0, b, chunk):
            ptrs = [None if t is None else t[lo].data_ptr() for t in outs]
            ins = [t[lo].data_ptr() for t in (pts, *extra)]
            check(fn(*ins, min(chunk, b - lo), *head, ws.data_ptr(), ws.numel(), *ptrs, _stream(pts)), name)
    return outs


def search_depth(points: torch.Tensor, host: str, *, max_depth: int, max_nodes: int,
                 stack_nodes: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Exhaustive worst-case game length under a fixed host, one tree per root (hironaka/util/search.py:9-32,
    hk_search_depth).  points: [B, m, d] float32/float64 roots in list semantics, used as given (rows with
    coordinate 0 >= 0 are points; padding rows may sit anywhere).  host: a key of SEARCH_HOSTS.
    Returns (depth int32[B], nodes int64[B], status int32[B]); status 0 = finished and exact, else an OR of
    HK_SEARCH_* bits (the numbers are then bounds, see include/hironaka_hip.h)."""
    pts = _search_checks(points, host, max_depth, max_nodes, stack_nodes, 63)
    b, m, d = pts.shape
    per_root = lib().hk_search_depth_workspace_bytes(1, m, d, _TORCH2HK[pts.dtype], stack_nodes)
    outs = [((b,), torch.int32, None), ((b,), torch.int64, None), ((b,), torch.int32, None)]
    depth, nodes, status = _search_launch(lib().hk_search_depth, "hk_search_depth", pts, host,
                                          (max_depth, max_nodes, stack_nodes), per_root, outs)
    return depth, nodes, status


def search_game_tree(points: torch.Tensor, host: str, *, expand_limit: Optional[int], max_depth: int, max_nodes: int,
                     stack_nodes: int, states: bool = True) -> Tuple[torch.Tensor, ...]:
    """The game tree under a fixed host, every node kept in the reference's preorder (hironaka/util/search.py:35-50
    search_tree, hk_search_game_tree).  points: [B, m, d] float32/float64 roots as for search_depth.  host: a key of
    SEARCH_HOSTS.  expand_limit: None for the whole tree, else L >= 0: only nodes numbered <= L are expanded (the
    reference's max_size - tree.size()).  Returns (parent, child_index, axis, depth, num_points, host_class) int32
    [B, max_nodes], states [B, max_nodes, m, d] of the roots' dtype (None unless ``states``), count int32 [B] and
    status int32 [B].  Slots from count on hold -1.  A status other than 0 / HK_SEARCH_ROOT_ENDED /
    HK_SEARCH_DEPTH_LIMIT leaves only count and status meaningful (include/hironaka_hip.h)."""
    pts = _search_checks(points, host, max_depth, max_nodes, stack_nodes, 31, expand_limit)
    b, m, d = pts.shape
    lim = -1 if expand_limit is None else int(expand_limit)
    per_root = lib().hk_search_game_tree_workspace_bytes(1, m, d, _TORCH2HK[pts.dtype], max_nodes, stack_nodes)
    outs = ([((b, max_nodes), torch.int32, -1)] * 6 + [((b, max_nodes, m, d), pts.dtype, -1) if states else None] +
            [((b,), torch.int32, 0)] * 2)
    return tuple(_search_launch(lib().hk_search_game_tree, "hk_search_game_tree", pts, host,
                                (lim, max_depth, max_nodes, stack_nodes), per_root, outs))


def search_morin_tree(points: torch.Tensor, weights: torch.Tensor, distinguished: torch.Tensor, host: str, *,
                      expand_limit: Optional[int], max_depth: int, max_nodes: int, stack_nodes: int,
                      states: bool = True) -> Tuple[torch.Tensor, ...]:
    """The Morin game tree under a fixed host (hironaka/util/search.py:53-93 search_tree_morin,
    hk_search_morin_tree): search_game_tree's tree with integer weights and a distinguished point per node, actions
    pruned by weight and "No contribution" leaves where the point is lost.  points: [B, m, d] float32/float64 roots
    as for search_game_tree, d in 2..7.  weights: [B, d] integers >= 0.  distinguished: [B] row indices.  Returns
    (parent, child_index, axis, depth, num_points, host_class, kind, distinguished) int32 [B, max_nodes], weights
    int32 [B, max_nodes, d], states [B, max_nodes, m, d] (None unless ``states``), count int32 [B] and status int32
    [B].  Slots from count on hold -1.  HK_SEARCH_ROOT_INVALID marks a root whose distinguished index addresses no
    point or that has a negative weight (count 1)."""
    pts = _search_checks(points, host, max_depth, max_nodes, stack_nodes, 31, expand_limit)
    b, m, d = pts.shape
    for t, name, shape in ((weights, "weights", (b, d)), (distinguished, "distinguished", (b,))):
        _require_device(t, name)
        if t.dtype not in (torch.int32, torch.int64) or tuple(t.shape) != shape or t.device != pts.device:
            raise ValueError(f"{name} must be an int32/int64 tensor of shape {shape} on the roots' device. Got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}.")
        if t.numel() and int(t.abs().max()) >= 2 ** 31:
            raise ValueError(f"{name} must fit int32.")
    wts = weights.to(torch.int32).contiguous()
    dist = distinguished.to(torch.int32).contiguous()
    lim = -1 if expand_limit is None else int(expand_limit)
    per_root = lib().hk_search_morin_tree_workspace_bytes(1, m, d, _TORCH2HK[pts.dtype], max_nodes, stack_nodes)
    outs = ([((b, max_nodes), torch.int32, -1)] * 8 + [((b, max_nodes, d), torch.int32, -1)] +
            [((b, max_nodes, m, d), pts.dtype, -1) if states else None] + [((b,), torch.int32, 0)] * 2)
    return tuple(_search_launch(lib().hk_search_morin_tree, "hk_search_morin_tree", pts, host,
                                (lim, max_depth, max_nodes, stack_nodes), per_root, outs, extra=(wts, dist)))


MORIN_TIES = {"lowest": A.HK_MORIN_TIE_LOWEST, "highest": A.HK_MORIN_TIE_HIGHEST, "random": A.HK_MORIN_TIE_RANDOM}
MORIN_WEIGHT_RULES = {"agent": A.HK_MORIN_WEIGHTS_AGENT, "search": A.HK_MORIN_WEIGHTS_SEARCH}
MORIN_OUTCOMES = {A.HK_MORIN_RUNNING: "running", A.HK_MORIN_ENDED: "ended",
                  A.HK_MORIN_NO_CONTRIBUTION: "no contribution", A.HK_MORIN_NO_MOVE: "no move",
                  A.HK_MORIN_INEXACT: "inexact"}

MorinPlayResult = collections.namedtuple("MorinPlayResult", "points weights distinguished length outcome classes axes")


def _record_stride(t: torch.Tensor) -> Optional[int]:
    """the element stride between the games of a [B, m, d] tensor whose games are contiguous records, else None"""
    b, m, d = t.shape
    if t.stride(2) != 1 or (m > 1 and t.stride(1) != d):
        return None
    if b > 1:
        return t.stride(0) if t.stride(0) >= m * d else None
    return m * d


def _records_overlap(x: torch.Tensor, y: torch.Tensor) -> bool:
    """whether the byte ranges that the records of two [B, m, d] record tensors span meet"""
    def span(t):
        b, m, d = t.shape
        return t.data_ptr(), t.data_ptr() + ((b - 1) * _record_stride(t) + m * d) * t.element_size()
    if not x.numel() or not y.numel():
        return False
    (x0, x1), (y0, y1) = span(x), span(y)
    return x0 < y1 and y0 < x1


def _play_checks(points: torch.Tensor, host: Optional[str], max_steps: int, seed: int, game_offset: int,
                 step_offset: int) -> None:
    """what game_play and morin_play ask of their host, their counters and their points"""
    if host is not None and host not in SEARCH_HOSTS:
        raise ValueError(f"host must be None or one of {sorted(SEARCH_HOSTS)}. Got {host!r}.")
    if not (0 <= max_steps < 2 ** 31 and 0 <= seed < 2 ** 64 and 0 <= game_offset < 2 ** 64
            and 0 <= step_offset < 2 ** 32 - max_steps):
        raise ValueError(f"need 0 <= max_steps < 2^31, seed and game_offset in [0, 2^64), step_offset + max_steps < 2^32. "
                         f"Got {max_steps}, {seed}, {game_offset}, {step_offset}.")
    _require_device(points, "points")
    if points.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"points must be float32 or float64. Got {points.dtype}.")
    if points.dim() != 3:
        raise ValueError(f"points must be [B, max_points, dim]. Got shape {tuple(points.shape)}.")


def _int_input(t: torch.Tensor, name: str, shape: tuple, dev: torch.device) -> None:
    _require_device(t, name)
    if t.dtype not in (torch.int32, torch.int64) or tuple(t.shape) != shape or t.device != dev:
        raise ValueError(f"{name} must be an int32/int64 tensor of shape {shape} on the points' device. Got "
                         f"{t.dtype} {tuple(t.shape)} on {t.device}.")


def _forced_moves(classes: Optional[torch.Tensor], axes: Optional[torch.Tensor], host: Optional[str], batch: int,
                  max_steps: int, dev: torch.device, clamp: bool) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """The forced classes / axes [B, max_steps] of game_play and morin_play as contiguous int32, None where not given.
    The two differ in what a value beyond int32 becomes, on purpose.  game_play never synchronises, so it clamps: such a
    value stays beyond every class and axis, and the game stops with "no move" as it would unclamped.  morin_play pays
    one synchronisation for the range of its weights under validate=True and refuses such a value there with the rest,
    so it converts as is (clamp=False)."""
    moves = []
    for t, name in ((classes, "classes"), (axes, "axes")):
        if t is not None:
            _int_input(t, name, (batch, max_steps), dev)
            t = (t.clamp(-1, 2 ** 31 - 1) if clamp else t).to(torch.int32).contiguous()
        moves.append(t)
    if host is None and classes is None and max_steps > 0:
        raise ValueError("without a host every move needs a forced class: pass classes.")
    return moves[0], moves[1]


def _play_records(points: torch.Tensor, out: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(src, dst) of game_play and morin_play: the [B, m, d] record tensors the launch reads and writes.  Games that are
    contiguous records at any stride are used in place, any other view through a copy (_play_result copies dst back)."""
    if out is not None:
        _require_device(out, "out")
        if out.shape != points.shape or out.dtype != points.dtype or out.device != points.device:
            raise ValueError(f"out must match points: {tuple(points.shape)} {points.dtype} on {points.device}. Got "
                             f"{tuple(out.shape)} {out.dtype} on {out.device}.")
    src = points if _record_stride(points) is not None else points.contiguous()
    dst = out if out is not None and _record_stride(out) is not None else torch.empty(
        tuple(points.shape), dtype=points.dtype, device=points.device)
    if _records_overlap(src, dst) and not (dst.data_ptr() == src.data_ptr() and dst.stride() == src.stride()):
        src = src.clone()  # only an exact in-place call may share memory: workgroups write back while others still read
    return src, dst


def _play_result(out: Optional[torch.Tensor], dst: torch.Tensor) -> torch.Tensor:
    """the final points where the caller wants them"""
    if out is not None and dst is not out:
        out.copy_(dst)
        return out
    return dst


def _morin_range_error(weights: torch.Tensor, distinguished: torch.Tensor, classes: Optional[torch.Tensor],
                       axes: Optional[torch.Tensor], max_points: int, weight_rule: str) -> Optional[str]:
    """morin_play's range check: the message of what it refuses, else None.  Weights lie in [0, 2^31) under the
    agent's rule; the search rule can leave a negative weight (a coordinate of the subset lighter than the axis), so
    under it, as for classes and axes, any value that fits int32 is taken.  distinguished lies in [-1, max_points).
    One synchronisation when the tensors are on a device."""
    w64, d64 = weights.to(torch.int64), distinguished.to(torch.int64)
    low = -2 ** 31 if weight_rule == "search" else 0
    bad = (w64 < low).any() | (w64 >= 2 ** 31).any() | (d64 < -1).any() | (d64 >= max_points).any()
    for t in (classes, axes):
        if t is not None and t.numel():
            bad = bad | (t.to(torch.int64).abs() >= 2 ** 31).any()
    if bool(bad):
        return (f"weights must lie in [{low}, 2^31) under weight_rule={weight_rule!r}, distinguished in "
                f"[-1, {max_points}), classes and axes must fit int32.")
    return None


def morin_play(points: torch.Tensor, weights: torch.Tensor, distinguished: torch.Tensor, *, host: Optional[str] = None,
               max_steps: int, classes: Optional[torch.Tensor] = None, axes: Optional[torch.Tensor] = None,
               tie: str = "lowest", weight_rule: str = "agent", seed: int = 0, game_offset: int = 0,
               step_offset: int = 0, reduce_root: bool = False, record: bool = False, out: Optional[torch.Tensor] = None,
               validate: bool = True) -> MorinPlayResult:
    """Morin games played forward, one game per lane, up to ``max_steps`` moves in one launch (hk_search_morin_play;
    hironaka/game.py:122-154 GameMorin with hironaka/agent.py:114-136 AgentMorin).  points: [B, m, d] float32/float64
    in list semantics (padding -1), d in 2..7, m <= 64; games that are contiguous records at any stride are read in
    place, any other view through a copy.  weights: [B, d] integers, >= 0 under weight_rule="agent"; the search rule
    can leave a negative weight, and a game that continues under it may bring any int32.  distinguished: [B] row
    indices, -1 for lost / none.  host: a key of SEARCH_HOSTS, or None when ``classes`` forces every move.  classes /
    axes: [B, max_steps] forced class ids / axes, entries < 0 leave the move to the host / the agent's rule.  tie: a
    key of MORIN_TIES (the agent's choice when the two lowest coordinates of the subset weigh the same; "random" draws
    from Philox keyed by (seed, game_offset + b, step_offset + move), so shards and launches that continue a game
    reproduce one launch).  weight_rule: a key of MORIN_WEIGHT_RULES.  reduce_root: Newton with the row tracked before
    any move (with max_steps=0: the tracked get_newton_polytope).  record: return the moves played as classes / axes
    [B, max_steps], -1 from length on.  out: where the final points go; default a new tensor.  It may be ``points``
    itself (in place); an ``out`` that shares memory with ``points`` in any other way is served through a copy of
    ``points``.  validate=False skips the range checks of weights and distinguished, which cost a synchronisation.
    Returns MorinPlayResult(points, weights, distinguished, length, outcome, classes, axes); outcome holds the
    HK_MORIN_* codes of include/hironaka_hip.h (MORIN_OUTCOMES names them)."""
    if tie not in MORIN_TIES or weight_rule not in MORIN_WEIGHT_RULES:
        raise ValueError(f"tie must be one of {sorted(MORIN_TIES)} and weight_rule one of {sorted(MORIN_WEIGHT_RULES)}. "
                         f"Got {tie!r}, {weight_rule!r}.")
    _play_checks(points, host, max_steps, seed, game_offset, step_offset)
    b, m, d = points.shape
    dev = points.device
    _int_input(weights, "weights", (b, d), dev)
    _int_input(distinguished, "distinguished", (b,), dev)
    c_in, a_in = _forced_moves(classes, axes, host, b, max_steps, dev, clamp=False)
    if validate and b:
        refused = _morin_range_error(weights, distinguished, classes, axes, m, weight_rule)
        if refused:
            raise ValueError(refused)
    w_in, d_in = weights.to(torch.int32).contiguous(), distinguished.to(torch.int32).contiguous()
    src, dst = _play_records(points, out)
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    w_out, d_out, length, outcome = new(b, d), new(b), new(b), new(b)
    c_out, a_out = (new(b, max_steps), new(b, max_steps)) if record else (None, None)
    q = A.hk_morin_play_desc()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    q.points_in, q.points_out = src.data_ptr(), dst.data_ptr()
    q.in_stride, q.out_stride = _record_stride(src), _record_stride(dst)
    q.weights_in, q.weights_out = w_in.data_ptr(), w_out.data_ptr()
    q.distinguished_in, q.distinguished_out = d_in.data_ptr(), d_out.data_ptr()
    q.class_in, q.axis_in, q.class_out, q.axis_out = ptr(c_in), ptr(a_in), ptr(c_out), ptr(a_out)
    q.length_out, q.outcome_out = length.data_ptr(), outcome.data_ptr()
    q.seed, q.game_offset, q.step_offset = seed, game_offset, step_offset
    q.batch, q.max_points, q.dim, q.dtype = b, m, d, _TORCH2HK[points.dtype]
    q.host = A.HK_MORIN_HOST_FORCED if host is None else SEARCH_HOSTS[host]
    q.max_steps, q.tie, q.weight_rule = max_steps, MORIN_TIES[tie], MORIN_WEIGHT_RULES[weight_rule]
    q.flags = A.HK_MORIN_REDUCE_ROOT if reduce_root else 0
    with torch.cuda.device(dev):
        check(lib().hk_search_morin_play(C.byref(q), _stream(points)), "hk_search_morin_play")
    return MorinPlayResult(_play_result(out, dst), w_out, d_out, length, outcome, c_out, a_out)


PLAY_AGENTS = {"random": A.HK_AGENT_RANDOM_LEGAL, "choose_first": A.HK_AGENT_CHOOSE_FIRST,
               "choose_last": A.HK_AGENT_CHOOSE_LAST}
PLAY_OUTCOMES = {A.HK_PLAY_RUNNING: "running", A.HK_PLAY_ENDED: "ended", A.HK_PLAY_NO_MOVE: "no move",
                 A.HK_PLAY_INEXACT: "inexact", A.HK_PLAY_VALUE_LIMIT: "value limit"}

GamePlayResult = collections.namedtuple("GamePlayResult", "points length outcome classes axes")


def game_play(points: torch.Tensor, *, host: Optional[str] = None, agent: str = "choose_first", max_steps: int,
              classes: Optional[torch.Tensor] = None, axes: Optional[torch.Tensor] = None, reposition: bool = False,
              rescale: bool = False, reduce_root: bool = False, rescale_root: bool = False,
              value_threshold: Optional[float] = None, seed: int = 0, game_offset: int = 0, step_offset: int = 0,
              record: bool = False, out: Optional[torch.Tensor] = None) -> GamePlayResult:
    """Plain Hironaka games played forward, one game per lane, up to ``max_steps`` moves in one launch (hk_game_play;
    hironaka/game.py:84-119 GameHironaka with hironaka/agent.py:85-98 RandomAgent / ChooseFirstAgent).  points:
    [B, m, d] float32/float64 in list semantics (padding -1), d in 2..7, m <= 64; games that are contiguous records at
    any stride are read in place, any other view through a copy.  host: a key of SEARCH_HOSTS, or None when ``classes``
    forces every move.  agent: a key of PLAY_AGENTS ("random" draws from Philox keyed by (seed, game_offset + b,
    step_offset + move), so shards and launches that continue a game reproduce one launch).  classes / axes:
    [B, max_steps] forced class ids / axes, entries < 0 leave the move to the host / the agent.  reposition: the stage
    between shift and Newton that Agent.USE_REPOSITION stands for.  rescale: the list rescale after every move
    (scale_observation).  reduce_root / rescale_root: Newton sorted + compacted, then the rescale, before any move (with
    max_steps=0 the call is just these); a root that is not reduced is played as given.  value_threshold: a game one of
    whose coordinates exceeds it after a move stops with HK_PLAY_VALUE_LIMIT; None or <= 0 for none.  record: return the
    moves played as classes / axes [B, max_steps], -1 from length on.  out: where the final points go; default a new
    tensor.  It may be ``points`` itself (in place); an ``out`` that shares memory with ``points`` in any other way is
    served through a copy of ``points``.  Returns GamePlayResult(points, length, outcome, classes, axes); outcome holds
    the HK_PLAY_* codes of include/hironaka_hip_play.h (PLAY_OUTCOMES names them)."""
    if agent not in PLAY_AGENTS:
        raise ValueError(f"agent must be one of {sorted(PLAY_AGENTS)}. Got {agent!r}.")
    if value_threshold is not None and value_threshold != value_threshold:
        raise ValueError("value_threshold must be a number or None. Got NaN.")
    _play_checks(points, host, max_steps, seed, game_offset, step_offset)
    b, m, d = points.shape
    dev = points.device
    c_in, a_in = _forced_moves(classes, axes, host, b, max_steps, dev, clamp=True)
    src, dst = _play_records(points, out)
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)  # noqa: E731
    length, outcome = new(b), new(b)
    c_out, a_out = (new(b, max_steps), new(b, max_steps)) if record else (None, None)
    q = A.hk_game_play_desc()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    q.points_in, q.points_out = src.data_ptr(), dst.data_ptr()
    q.in_stride, q.out_stride = _record_stride(src), _record_stride(dst)
    q.class_in, q.axis_in, q.class_out, q.axis_out = ptr(c_in), ptr(a_in), ptr(c_out), ptr(a_out)
    q.length_out, q.outcome_out = length.data_ptr(), outcome.data_ptr()
    q.seed, q.game_offset, q.step_offset = seed, game_offset, step_offset
    q.value_threshold = 0.0 if value_threshold is None else float(value_threshold)
    q.batch, q.max_points, q.dim, q.dtype = b, m, d, _TORCH2HK[points.dtype]
    q.host = A.HK_PLAY_HOST_FORCED if host is None else SEARCH_HOSTS[host]
    q.agent, q.max_steps = PLAY_AGENTS[agent], max_steps
    q.flags = ((A.HK_PLAY_REPOSITION if reposition else 0) | (A.HK_PLAY_RESCALE if rescale else 0)
               | (A.HK_PLAY_REDUCE_ROOT if reduce_root else 0) | (A.HK_PLAY_RESCALE_ROOT if rescale_root else 0))
    with torch.cuda.device(dev):
        check(lib().hk_game_play(C.byref(q), _stream(points)), "hk_game_play")
    return GamePlayResult(_play_result(out, dst), length, outcome, c_out, a_out)


# ---- one move of a vectorised environment, resets included (hk_env_step) ---------------------------------------------

ENV_MODES = {"host": A.HK_ENV_MODE_HOST, "agent": A.HK_ENV_MODE_AGENT}
ENV_AGENTS = {"random": A.HK_AGENT_RANDOM_LEGAL, "choose_first": A.HK_AGENT_CHOOSE_FIRST}


def _env_buffer(t, name: str, dtype, shape, dev, optional: bool = False) -> Optional[int]:
    """the address of a buffer hk_env_step reads or writes in place: exactly this dtype and shape, contiguous, on dev"""
    if t is None:
        if optional:
            return None
        raise ValueError(f"{name} is required.")
    _require_device(t, name)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}. Got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}, contiguous: {t.is_contiguous()}.")
    return t.data_ptr()


def env_step(points: torch.Tensor, *, mode: str, step_count: torch.Tensor, episode: torch.Tensor, reward: torch.Tensor,
             stopped: torch.Tensor, obs_points: torch.Tensor, action: Optional[torch.Tensor] = None,
             class_io: Optional[torch.Tensor] = None, obs_coords: Optional[torch.Tensor] = None,
             final_points: Optional[torch.Tensor] = None, final_coords: Optional[torch.Tensor] = None,
             agent_axis: Optional[torch.Tensor] = None, exceed: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None, host: Optional[str] = None, agent: Optional[str] = None, seed: int = 0,
             agent_seed: int = 0, game_offset: int = 0, world_games: Optional[int] = None, max_value: int = 0,
             value_threshold: Optional[float] = None, step_threshold: int = 2 ** 31 - 1,
             invalid_move_penalty: float = -1e-3, threshold_penalty: float = 0.0, scale_observation: bool = True,
             stop_after_invalid: bool = False, stop_at_threshold: bool = True, point_reduction_reward: bool = False,
             improve_efficiency: bool = False, reposition: bool = False, auto_reset: bool = True,
             reset_all: bool = False) -> None:
    """One move of every game of a vectorised environment in one launch, the next episode of a stopped game included
    (hk_env_step, include/hironaka_hip_env.h: the step of gym_env.HironakaHostEnv / HironakaAgentEnv per game).  Every
    tensor is a buffer the caller owns, read and written in place: nothing is copied or converted, so each must have
    exactly the dtype and shape below, be contiguous and live on the points' device.

    points [B, m, d] float32/float64, list semantics, d in 2..7, m <= 64; out: where the new state goes, default
    ``points`` itself (otherwise the two must not share memory).  mode "host": ``host`` is a key of SEARCH_HOSTS,
    action int32 [B] the agent's axis, class_io int32 [B] the pending subset as a class id (in and out), obs_coords
    float64 [B, d].  mode "agent": ``agent`` is a key of ENV_AGENTS, action int32 [B] the host's subset as a bit mask,
    agent_axis int32 [B] (optional) the axis chosen.  step_count, episode int32 [B] (in and out); reward float64 [B];
    stopped, exceed (optional) uint8 [B]; obs_points float32 [B, m, d]; final_points float32 [B, m, d] and final_coords
    float64 [B, d] (optional) receive the terminal observation of the games that stopped and were reset.  seed keys the
    generator, agent_seed the random agent; the game index of both streams is game_offset + episode * world_games + b
    (world_games: default B).  reset_all: play no move and give every game a fresh episode (episode += 1)."""
    if mode not in ENV_MODES:
        raise ValueError(f"mode must be one of {sorted(ENV_MODES)}. Got {mode!r}.")
    host_mode = mode == "host"
    if host_mode and host not in SEARCH_HOSTS:
        raise ValueError(f"host must be one of {sorted(SEARCH_HOSTS)}. Got {host!r}.")
    if not host_mode and agent not in ENV_AGENTS:
        raise ValueError(f"agent must be one of {sorted(ENV_AGENTS)}. Got {agent!r}.")
    _require_device(points, "points")
    if points.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"points must be float32 or float64. Got {points.dtype}.")
    if points.dim() != 3 or not points.is_contiguous():
        raise ValueError(f"points must be a contiguous [B, max_points, dim]. Got shape {tuple(points.shape)}, "
                         f"strides {points.stride()}.")
    b, m, d = points.shape
    dev = points.device
    if not (2 <= d <= 7 and 1 <= m <= 64 and b < 2 ** 31):
        raise ValueError(f"hk_env_step serves dim 2..7, max_points 1..64 and fewer than 2^31 games. Got {(b, m, d)}.")
    world_games = b if world_games is None else world_games
    if not (0 <= seed < 2 ** 64 and 0 <= agent_seed < 2 ** 64 and 0 <= game_offset < 2 ** 64
            and 0 <= world_games < 2 ** 64):
        raise ValueError(f"seed, agent_seed, game_offset and world_games must be in [0, 2^64). Got {seed}, {agent_seed}, "
                         f"{game_offset}, {world_games}.")
    if not (0 <= max_value < 2 ** 31 and -2 ** 31 <= step_threshold < 2 ** 31):
        raise ValueError(f"max_value and step_threshold must fit an int32. Got {max_value}, {step_threshold}.")
    if (auto_reset or reset_all) and max_value < 1:
        raise ValueError(f"a reset draws integers in [0, max_value): max_value must be at least 1. Got {max_value}.")
    for v, name in ((value_threshold, "value_threshold"), (invalid_move_penalty, "invalid_move_penalty"),
                    (threshold_penalty, "threshold_penalty")):
        if v is not None and v != v:
            raise ValueError(f"{name} must be a number. Got NaN.")
    if value_threshold is not None and value_threshold <= 0:
        raise ValueError(f"hk_env_step reads a value_threshold <= 0 as none, while the environments test any threshold "
                         f"that is not None. Got {value_threshold}; use hironaka_amd.gym_env's environments for it.")
    q = A.hk_env_step_desc()
    q.points_in = points.data_ptr()
    q.points_out = q.points_in if out is None or out is points else _env_buffer(out, "out", points.dtype, (b, m, d), dev)
    if q.points_out != q.points_in and _records_overlap(points, out):
        raise ValueError("out must be points itself or share no memory with it.")
    i32, f64, f32, u8 = torch.int32, torch.float64, torch.float32, torch.uint8
    q.step_count = _env_buffer(step_count, "step_count", i32, (b,), dev)
    q.episode = _env_buffer(episode, "episode", i32, (b,), dev)
    q.action = _env_buffer(action, "action", i32, (b,), dev, optional=reset_all)
    q.reward = _env_buffer(reward, "reward", f64, (b,), dev)
    q.stopped = _env_buffer(stopped, "stopped", u8, (b,), dev)
    q.exceed = _env_buffer(exceed, "exceed", u8, (b,), dev, optional=True)
    q.obs_points = _env_buffer(obs_points, "obs_points", f32, (b, m, d), dev)
    q.final_points = _env_buffer(final_points, "final_points", f32, (b, m, d), dev, optional=True)
    if host_mode:
        q.class_io = _env_buffer(class_io, "class_io", i32, (b,), dev)
        q.obs_coords = _env_buffer(obs_coords, "obs_coords", f64, (b, d), dev)
        q.final_coords = _env_buffer(final_coords, "final_coords", f64, (b, d), dev, optional=True)
        q.host = SEARCH_HOSTS[host]
    else:
        q.agent_axis = _env_buffer(agent_axis, "agent_axis", i32, (b,), dev, optional=True)
        q.agent = ENV_AGENTS[agent]
    q.seed, q.agent_seed, q.game_offset, q.world_games = seed, agent_seed, game_offset, world_games
    q.value_threshold = 0.0 if value_threshold is None else float(value_threshold)
    q.invalid_move_penalty, q.threshold_penalty = float(invalid_move_penalty), float(threshold_penalty)
    q.batch, q.max_points, q.dim, q.dtype, q.mode = b, m, d, _TORCH2HK[points.dtype], ENV_MODES[mode]
    q.max_value, q.step_threshold = max_value, step_threshold
    q.flags = ((A.HK_ENV_SCALE_OBSERVATION if scale_observation else 0)
               | (A.HK_ENV_STOP_AFTER_INVALID if stop_after_invalid else 0)
               | (A.HK_ENV_STOP_AT_THRESHOLD if stop_at_threshold else 0)
               | (A.HK_ENV_POINT_REDUCTION_REWARD if point_reduction_reward else 0)
               | (A.HK_ENV_IMPROVE_EFFICIENCY if improve_efficiency else 0)
               | (A.HK_ENV_AGENT_REPOSITION if reposition else 0) | (A.HK_ENV_AUTO_RESET if auto_reset else 0)
               | (A.HK_ENV_RESET_ALL if reset_all else 0))
    with torch.cuda.device(dev):
        check(lib().hk_env_step(C.byref(q), _stream(points)), "hk_env_step")


# ---- one greedy move of the DQN evaluation (hk_dqn_host_move / hk_dqn_agent_move) -------------------------------------

DQN_MOVE_MAX_DIM, DQN_MOVE_MAX_POINTS = 7, 64


def _q_rows(q: torch.Tensor, name: str, rows: int, width: int, dev) -> int:
    """the row stride of the Q-values [rows, width] of a network: float32/float64, rows of unit stride any distance
    apart (a slice of a wider output is read in place)"""
    _require_device(q, name)
    if q.dtype not in (torch.float32, torch.float64) or tuple(q.shape) != (rows, width) or q.device != dev:
        raise ValueError(f"{name} must be a float32/float64 tensor of shape ({rows}, {width}) on {dev}. Got {q.dtype} "
                         f"{tuple(q.shape)} on {q.device}.")
    if q.stride(1) != 1 or (rows > 1 and q.stride(0) < width):
        raise ValueError(f"{name} must have rows of unit stride that do not overlap. Got strides {q.stride()}.")
    return q.stride(0) if rows > 1 else width


def _shares_memory(x: Optional[torch.Tensor], y: Optional[torch.Tensor]) -> bool:
    """whether the byte ranges from the first to the last element of two tensors meet"""
    def span(t):
        last = sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
        return t.data_ptr(), t.data_ptr() + (last + 1) * t.element_size()
    if x is None or y is None or not x.numel() or not y.numel():
        return False
    (x0, x1), (y0, y1) = span(x), span(y)
    return x0 < y1 and y0 < x1


def _no_shared_memory(written: Dict[str, Optional[torch.Tensor]], read: Dict[str, Optional[torch.Tensor]]) -> None:
    names = list(written)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if _shares_memory(written[a], written[b]):
                raise ValueError(f"{a} and {b} are both written and must not share memory.")
        for b, t in read.items():
            if _shares_memory(written[a], t):
                raise ValueError(f"{a} is written and must not share memory with {b}.")


def dqn_host_move(q: torch.Tensor, class_out: torch.Tensor, coords_out: torch.Tensor, *,
                  prev_done: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None) -> None:
    """The host's greedy move from its Q-values in one launch (hk_dqn_host_move, include/hironaka_hip_dqn_move.h):
    class_out[b] = torch.argmax(q[b]) (the first maximum; the first NaN wins) and coords_out[b] = the class's subset as
    0/1 values, what FusedGame.host_move returns with exploration off.  Every tensor is a buffer the caller owns, used in
    place; nothing is allocated.

    q [B, 2^d - d - 1] float32/float64, rows of unit stride at any distance; class_out int32 [B]; coords_out [B, d]
    float32/float64, contiguous; d in 2..7.  prev_done uint8 [B] and counts int32 [2^d - d - 1], both or neither:
    counts[class_out[b]] += 1 for every b with prev_done[b] == 0."""
    _require_device(coords_out, "coords_out")
    if coords_out.dim() != 2 or coords_out.dtype not in (torch.float32, torch.float64) or not coords_out.is_contiguous():
        raise ValueError(f"coords_out must be a contiguous float32/float64 [B, dim] tensor. Got {coords_out.dtype} "
                         f"{tuple(coords_out.shape)}, contiguous: {coords_out.is_contiguous()}.")
    b, d = coords_out.shape
    dev = coords_out.device
    if not (2 <= d <= DQN_MOVE_MAX_DIM and b < 2 ** 31):
        raise ValueError(f"hk_dqn_host_move serves dim 2..{DQN_MOVE_MAX_DIM} and fewer than 2^31 games. Got {(b, d)}.")
    classes = 2 ** d - d - 1
    if (prev_done is None) != (counts is None):
        raise ValueError("prev_done and counts go together: pass both or neither.")
    s = A.hk_dqn_host_move_desc()
    s.q_stride = _q_rows(q, "q", b, classes, dev)
    s.q = q.data_ptr()
    s.class_out = _env_buffer(class_out, "class_out", torch.int32, (b,), dev)
    s.coords_out = coords_out.data_ptr()
    s.prev_done = _env_buffer(prev_done, "prev_done", torch.uint8, (b,), dev, optional=True)
    s.counts = _env_buffer(counts, "counts", torch.int32, (classes,), dev, optional=True)
    _no_shared_memory({"class_out": class_out, "coords_out": coords_out, "counts": counts},
                      {"q": q, "prev_done": prev_done})
    s.batch, s.dim, s.q_dtype, s.coords_dtype = b, d, _TORCH2HK[q.dtype], _TORCH2HK[coords_out.dtype]
    with torch.cuda.device(dev):
        check(lib().hk_dqn_host_move(C.byref(s), _stream(coords_out)), "hk_dqn_host_move")


def dqn_agent_move(points: torch.Tensor, q: torch.Tensor, class_id: torch.Tensor, *, axis_out: torch.Tensor,
                   features_out: torch.Tensor, done_out: torch.Tensor, lengths: torch.Tensor,
                   counts: Optional[torch.Tensor] = None, masked: bool = True, rescale: bool = True,
                   padding_value: float = -1.0) -> None:
    """The agent's greedy move from its Q-values, the move itself and the next observation in one launch
    (hk_dqn_agent_move, include/hironaka_hip_dqn_move.h): what FusedGame.agent_move does with exploration off
    (``masked``: the argmax over the host's subset by fused_game's expression), then ``get_features`` and ``get_dones``
    of the new state.  Every tensor is a buffer the caller owns, used in place; nothing is allocated.

    points [B, m, d] float32/float64, contiguous, moved in place (torch semantics: shift unless the axis lies outside the
    subset or the game is over, Newton polytope, ``rescale``); q [B, d] float32/float64, rows of unit stride at any
    distance; class_id int32 [B], the host's class; axis_out int32 [B]; features_out [B, m, d] of the points' dtype;
    done_out uint8 [B]; lengths int32 [B], += 1 for every game that was not over before the move; counts int32 [d]
    (optional), += 1 at the axis of each such game.  d in 2..7, m <= 64, padding_value negative."""
    _require_device(points, "points")
    if points.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"points must be float32 or float64. Got {points.dtype}.")
    if points.dim() != 3 or not points.is_contiguous():
        raise ValueError(f"points must be a contiguous [B, max_points, dim]. Got shape {tuple(points.shape)}, "
                         f"strides {points.stride()}.")
    b, m, d = points.shape
    dev = points.device
    if not (2 <= d <= DQN_MOVE_MAX_DIM and 1 <= m <= DQN_MOVE_MAX_POINTS and b < 2 ** 31):
        raise ValueError(f"hk_dqn_agent_move serves dim 2..{DQN_MOVE_MAX_DIM}, max_points 1..{DQN_MOVE_MAX_POINTS} and "
                         f"fewer than 2^31 games. Got {(b, m, d)}.")
    if not padding_value < 0:
        raise ValueError(f"padding_value must be negative. Got {padding_value}.")
    s = A.hk_dqn_agent_move_desc()
    s.points = points.data_ptr()
    s.q_stride = _q_rows(q, "q", b, d, dev)
    s.q = q.data_ptr()
    s.class_id = _env_buffer(class_id, "class_id", torch.int32, (b,), dev)
    s.axis_out = _env_buffer(axis_out, "axis_out", torch.int32, (b,), dev)
    s.features_out = _env_buffer(features_out, "features_out", points.dtype, (b, m, d), dev)
    s.done_out = _env_buffer(done_out, "done_out", torch.uint8, (b,), dev)
    s.lengths = _env_buffer(lengths, "lengths", torch.int32, (b,), dev)
    s.counts = _env_buffer(counts, "counts", torch.int32, (d,), dev, optional=True)
    _no_shared_memory({"points": points, "features_out": features_out, "axis_out": axis_out, "done_out": done_out,
                       "lengths": lengths, "counts": counts}, {"q": q, "class_id": class_id})
    s.padding_value = float(padding_value)
    s.batch, s.max_points, s.dim = b, m, d
    s.dtype, s.q_dtype = _TORCH2HK[points.dtype], _TORCH2HK[q.dtype]
    s.flags = (A.HK_DQN_MOVE_MASKED if masked else 0) | (A.HK_DQN_MOVE_RESCALE if rescale else 0)
    with torch.cuda.device(dev):
        check(lib().hk_dqn_agent_move(C.byref(s), _stream(points)), "hk_dqn_agent_move")


# ---- the replay buffer as a ring on the device (hk_replay_push / hk_replay_sample) ---------------------------------

REPLAY_TILE_ROWS = A.HK_REPLAY_TILE_ROWS


def replay_cursor(device) -> torch.Tensor:
    """a zeroed cursor block: an empty buffer (int64 [8]; the words are the HK_REPLAY_* indices of _abi)"""
    return torch.zeros(A.HK_REPLAY_CURSOR_WORDS, dtype=torch.int64, device=device)


def _row_bytes(t: torch.Tensor) -> int:
    n = t.element_size()
    for k in t.shape[1:]:
        n *= k
    return n


def _rows_of(t: torch.Tensor, ring: torch.Tensor, name: str, rows: int) -> int:
    """checks the batch side of a column against its ring; returns its row stride in bytes"""
    _require_device(t, name)
    if t.device != ring.device or t.dtype != ring.dtype or tuple(t.shape[1:]) != tuple(ring.shape[1:]) or t.dim() < 1:
        raise ValueError(f"{name} must hold rows of the ring's kind ({ring.dtype} {tuple(ring.shape[1:])} on "
                         f"{ring.device}). Got {t.dtype} {tuple(t.shape)} on {t.device}.")
    if t.shape[0] != rows:
        raise ValueError(f"{name} must have {rows} rows. Got {t.shape[0]}.")
    row = _row_bytes(ring)
    if rows == 0:
        return row
    stride = t.stride(0) * t.element_size() if rows > 1 else row
    if not t[0].is_contiguous() or stride < row:
        raise ValueError(f"the rows of {name} must each be contiguous and must not overlap. Got strides {t.stride()}.")
    return stride


def _replay_desc(ring_cols: Sequence[torch.Tensor], cursor: torch.Tensor) -> "A.hk_replay_desc":
    if not 1 <= len(ring_cols) <= A.HK_REPLAY_MAX_COLS:
        raise ValueError(f"a replay buffer has 1..{A.HK_REPLAY_MAX_COLS} columns. Got {len(ring_cols)}.")
    _require_device(cursor, "cursor")
    if cursor.dtype != torch.int64 or tuple(cursor.shape) != (A.HK_REPLAY_CURSOR_WORDS,) or not cursor.is_contiguous():
        raise ValueError(f"cursor must be a contiguous int64 [{A.HK_REPLAY_CURSOR_WORDS}]. Got {cursor.dtype} "
                         f"{tuple(cursor.shape)}.")
    q = A.hk_replay_desc()
    capacity = None
    for c, ring in enumerate(ring_cols):
        _require_device(ring, f"ring_cols[{c}]")
        if ring.dim() < 1 or not ring.is_contiguous() or ring.device != cursor.device:
            raise ValueError(f"ring_cols[{c}] must be a contiguous [capacity, ...] tensor on {cursor.device}.")
        capacity = ring.shape[0] if capacity is None else capacity
        if ring.shape[0] != capacity:
            raise ValueError(f"every ring has the same number of rows. Got {capacity} and {ring.shape[0]}.")
        q.col[c].ring = ring.data_ptr()
        q.col[c].row_bytes = _row_bytes(ring)
    if not 1 <= capacity < 2 ** 31:
        raise ValueError(f"the capacity must be in [1, 2^31). Got {capacity}.")
    q.ncols, q.capacity, q.cursor = len(ring_cols), capacity, cursor.data_ptr()
    return q


def replay_push(ring_cols: Sequence[torch.Tensor], row_cols: Sequence[torch.Tensor], cursor: torch.Tensor,
                keep: Optional[torch.Tensor] = None) -> None:
    """Push a batch of experiences into the rings in one launch (hk_replay_push, include/hironaka_hip_replay.h).

    ring_cols: 1..8 contiguous tensors [capacity, ...], one per column.  row_cols: the batch, one tensor [B, ...] per
    column with its ring's dtype and trailing shape; the rows may be strided (a slice of wider records), each row
    contiguous.  keep: bool or uint8 [B], the rows to push (None: all).  The kept rows go, in batch order, to the slots
    the cursor points at and the cursor moves on, all on the device: nothing here synchronises.  B < capacity."""
    q = _replay_desc(ring_cols, cursor)
    if len(row_cols) != len(ring_cols):
        raise ValueError(f"{len(ring_cols)} rings but {len(row_cols)} columns of rows.")
    batch = row_cols[0].shape[0] if isinstance(row_cols[0], torch.Tensor) and row_cols[0].dim() else 0
    for c, (ring, rows) in enumerate(zip(ring_cols, row_cols)):
        q.col[c].rows_stride_bytes = _rows_of(rows, ring, f"row_cols[{c}]", batch)
        q.col[c].rows = rows.data_ptr()
    if batch >= q.capacity:
        raise ValueError(f"a push must be smaller than the buffer. Got {batch} rows for a capacity of {q.capacity}.")
    if keep is not None:
        _require_device(keep, "keep")
        if keep.dtype not in (torch.bool, torch.uint8) or tuple(keep.shape) != (batch,) or keep.device != cursor.device:
            raise ValueError(f"keep must be a bool or uint8 [{batch}] on {cursor.device}. Got {keep.dtype} "
                             f"{tuple(keep.shape)} on {keep.device}.")
        keep = keep.contiguous()
        q.keep = keep.data_ptr()
    q.batch = batch
    with torch.cuda.device(cursor.device):
        check(lib().hk_replay_push(C.byref(q), _stream(cursor)), "hk_replay_push")


def replay_sample(ring_cols: Sequence[torch.Tensor], cursor: torch.Tensor, batch_size: int, seed: int,
                  out: Optional[Sequence[torch.Tensor]] = None) -> Tuple[list, torch.Tensor]:
    """Draw batch_size rows uniformly from the filled part of the rings in one launch (hk_replay_sample).

    Returns (cols, index): cols[c] [batch_size, ...] holds row index[j] of ring_cols[c] at row j (``out``: tensors to
    write into instead of fresh ones), index int64 [batch_size].  The indices are Philox words keyed by ``seed`` and the
    cursor's samples_drawn, which the launch advances.  An empty buffer gives index -1 and leaves the rows as they
    are (fresh ones: zero)."""
    q = _replay_desc(ring_cols, cursor)
    if not (0 <= batch_size < 2 ** 31 and 0 <= seed < 2 ** 64):
        raise ValueError(f"batch_size must be in [0, 2^31) and seed in [0, 2^64). Got {batch_size}, {seed}.")
    if out is None:
        out = [torch.zeros((batch_size,) + tuple(r.shape[1:]), dtype=r.dtype, device=r.device) for r in ring_cols]
    elif len(out) != len(ring_cols):
        raise ValueError(f"{len(ring_cols)} rings but {len(out)} output columns.")
    for c, (ring, rows) in enumerate(zip(ring_cols, out)):
        q.col[c].rows_stride_bytes = _rows_of(rows, ring, f"out[{c}]", batch_size)
        q.col[c].rows = rows.data_ptr()
    index = torch.full((batch_size,), -1, dtype=torch.int64, device=cursor.device)
    with torch.cuda.device(cursor.device):
        check(lib().hk_replay_sample(C.byref(q), batch_size, seed, index.data_ptr(), _stream(cursor)),
              "hk_replay_sample")
    return list(out), index


# ---- the DQN fit step: TD target + Huber loss + dQ in one launch, Polyak update of a parameter list in one ----------

DQN_TILE_ROWS = A.HK_DQN_TILE_ROWS
DqnTdResult = collections.namedtuple("DqnTdResult", "loss dq target row_loss status")
_DQN_WORKSPACES = _WorkspaceCache(1 << 12)  # of dqn_td calls that bring no workspace


def dqn_td_workspace(batch: int, device) -> torch.Tensor:
    """a zeroed workspace of the caller's own for dqn_td launches of up to `batch` rows (uint8; the ticket and one slot
    per workgroup).  Launches that share one belong on one stream."""
    need = int(lib().hk_dqn_td_workspace_bytes(int(batch)))
    if need == 0:
        raise ValueError(f"batch must be in [0, 2^31). Got {batch}.")
    return torch.zeros(need, dtype=torch.uint8, device=device)


def _dqn_rows(t: torch.Tensor, name: str, dtype=None) -> torch.Tensor:
    """a [B, A] float32 / float64 block whose rows are contiguous (the rows themselves may be strided)"""
    _require_device(t, name)
    if t.dim() != 2 or t.dtype not in (torch.float32, torch.float64) or (dtype is not None and t.dtype != dtype):
        raise TypeError(f"{name} must be a [B, A] {dtype or 'float32 or float64'} tensor. Got {t.dtype} "
                        f"{tuple(t.shape)}.")
    ok = (t.shape[1] == 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])
    return t if ok else t.contiguous()


def _dqn_stride(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _dqn_column(t: torch.Tensor, name: str, like: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """[B] or [B, 1], as ReplayBuffer.sample returns it, forced into the kernel's type"""
    _require_device(t, name)
    if t.device != like.device:
        raise ValueError(f"{name} is on {t.device}, q on {like.device}")
    if t.numel() != like.shape[0] or t.dim() not in (1, 2):
        raise ValueError(f"{name} must be [B] or [B, 1] with B = {like.shape[0]}. Got {tuple(t.shape)}.")
    t = t.reshape(-1)
    if dtype == torch.uint8:
        t = t.view(torch.uint8) if t.dtype == torch.bool else (t if t.dtype == torch.uint8 else (t != 0).view(torch.uint8))
    elif t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def dqn_td(q: torch.Tensor, next_q: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor, dones: torch.Tensor,
           gamma: float, *, workspace: Optional[torch.Tensor] = None, out: Optional[dict] = None,
           want: Sequence[str] = ("target", "row_loss")) -> DqnTdResult:
    """The 1-step TD target, the Huber loss and its gradient with respect to q in one launch (hk_dqn_td,
    include/hironaka_hip_dqn.h; dqn_trainer.py:68-88 and the backward pass of its loss).

    q, next_q: [B, A] float32 or float64, rows possibly strided; actions int32, rewards float32, dones bool, each [B] or
    [B, 1] (other types are converted).  Returns DqnTdResult(loss [] , dq [B, A], target [B] or None, row_loss [B] or
    None, status int32 [1]): `want` names the optional outputs, `out` may bring tensors for any of "loss", "dq",
    "target", "row_loss", "status" (a status brought along is OR-ed into, not cleared).  An action outside [0, A) gives a
    zero row and sets HK_DQN_BAD_ACTION in status.  workspace: dqn_td_workspace(...) of the caller's own; None: one per
    device and stream.  Nothing here synchronises."""
    q = _dqn_rows(q, "q")
    next_q = _dqn_rows(next_q, "next_q", q.dtype)
    if next_q.shape != q.shape or next_q.device != q.device:
        raise ValueError(f"q and next_q must have one shape and device. Got {tuple(q.shape)} on {q.device} and "
                         f"{tuple(next_q.shape)} on {next_q.device}.")
    batch, nact = q.shape
    if not (1 <= nact <= A.HK_DQN_MAX_ACTIONS and batch < 2 ** 31):
        raise ValueError(f"A must be in [1, {A.HK_DQN_MAX_ACTIONS}] and B below 2^31. Got B = {batch}, A = {nact}.")
    actions = _dqn_column(actions, "actions", q, torch.int32)
    rewards = _dqn_column(rewards, "rewards", q, torch.float32)
    dones = _dqn_column(dones, "dones", q, torch.uint8)
    out = dict(out or {})
    unknown = (set(out) | set(want)) - set(DqnTdResult._fields)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")
    dev = q.device

    def given(name, shape, dtype):
        t = out.get(name)
        if t is None:
            return None
        _require_device(t, name)
        if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev:
            raise ValueError(f"out[{name!r}] must be {dtype} {shape} on {dev}. Got {t.dtype} {tuple(t.shape)}.")
        return t

    dq = given("dq", (batch, nact), q.dtype)
    if dq is None:
        dq = torch.empty((batch, nact), dtype=q.dtype, device=dev)
    elif not ((nact == 1 or dq.stride(1) == 1) and (batch <= 1 or dq.stride(0) >= nact)):
        raise ValueError(f"the rows of out['dq'] must each be contiguous. Got strides {dq.stride()}.")
    loss = given("loss", (), q.dtype)
    if loss is None:
        loss = torch.full((), float("nan"), dtype=q.dtype, device=dev) if batch == 0 else \
            torch.empty((), dtype=q.dtype, device=dev)
    status = given("status", (1,), torch.int32)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    extra = {}
    for name in ("target", "row_loss"):
        t = given(name, (batch,), q.dtype)
        if t is None and name in want:
            t = torch.empty(batch, dtype=q.dtype, device=dev)
        if t is not None and not t.is_contiguous():
            raise ValueError(f"out[{name!r}] must be contiguous.")
        extra[name] = t
    if workspace is None:
        workspace = _DQN_WORKSPACES.get(dev, int(lib().hk_dqn_td_workspace_bytes(batch)))
    else:
        _require_device(workspace, "workspace")
        if (workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != dev
                or workspace.numel() < lib().hk_dqn_td_workspace_bytes(batch)):
            raise ValueError("workspace must be what dqn_td_workspace(batch, device) returns (or a larger one).")
    d = A.hk_dqn_td_desc()
    d.q, d.next_q, d.actions, d.rewards, d.dones = (q.data_ptr(), next_q.data_ptr(), actions.data_ptr(),
                                                    rewards.data_ptr(), dones.data_ptr())
    d.target = extra["target"].data_ptr() if extra["target"] is not None else None
    d.row_loss = extra["row_loss"].data_ptr() if extra["row_loss"] is not None else None
    d.dq, d.loss, d.workspace, d.status = dq.data_ptr(), loss.data_ptr(), workspace.data_ptr(), status.data_ptr()
    d.q_stride, d.next_q_stride, d.dq_stride = _dqn_stride(q), _dqn_stride(next_q), _dqn_stride(dq)
    d.gamma, d.batch, d.num_actions, d.dtype = float(gamma), batch, nact, _TORCH2HK[q.dtype]
    with torch.cuda.device(dev):
        check(lib().hk_dqn_td(C.byref(d), _stream(q)), "hk_dqn_td")
    return DqnTdResult(loss, dq, extra["target"], extra["row_loss"], status)


def polyak_update(srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor], tau: float) -> None:
    """dst = tau * src + (1 - tau) * dst for every pair, in place, HK_POLYAK_MAX_TENSORS pairs per launch
    (hk_polyak_update: the reference's polyak_update, _borrowed_fn.py:25-49, to the bit: a rounded multiply, then a fused
    multiply-add).  Every tensor is a contiguous float32 or float64 tensor on one HIP device, all of one dtype (anything
    else is a TypeError); a pair has one number of elements.  Nothing here synchronises."""
    srcs, dsts = list(srcs), list(dsts)
    if len(srcs) != len(dsts):
        raise ValueError(f"{len(srcs)} sources but {len(dsts)} destinations.")
    if not srcs:
        return
    first = dsts[0]
    _require_device(first, "dsts[0]")
    dtype, dev = first.dtype, first.device
    flat = []  # src, dst, numel of every pair: the descriptor's entries as they lie in memory
    for k, (s, t) in enumerate(zip(srcs, dsts)):
        for name, x in (("srcs", s), ("dsts", t)):
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == dtype and x.device == dev
                    and x.is_contiguous() and dtype in (torch.float32, torch.float64)):
                _require_device(x, f"{name}[{k}]")
                raise TypeError(f"every tensor must be a contiguous float32 or float64 tensor of one dtype on one "
                                f"device ({dtype} on {dev}). {name}[{k}] is {x.dtype} on {x.device} with strides "
                                f"{x.stride()}.")
        n = s.numel()
        if n != t.numel():
            raise ValueError(f"pair {k}: {n} source elements but {t.numel()} destination elements.")
        flat += (s.data_ptr(), t.data_ptr(), n)
    per = 3 * A.HK_POLYAK_MAX_TENSORS
    with torch.cuda.device(dev):
        stream = _stream(first)
        for at in range(0, len(flat), per):
            part = flat[at:at + per]
            d = A.hk_polyak_desc()
            (C.c_int64 * len(part)).from_address(C.addressof(d))[:] = part  # d.tensor[k] = {src, dst, numel}
            d.tau, d.ntensors, d.dtype = float(tau), len(part) // 3, _TORCH2HK[dtype]
            check(lib().hk_polyak_update(C.byref(d), stream), "hk_polyak_update")


# ---- the MCTS trainer's loss: policy_value_loss with its gradient, the sampled target rows gathered, in one launch ----

PVLOSS_TILE_ROWS = A.HK_PVLOSS_TILE_ROWS
PvLossResult = collections.namedtuple("PvLossResult", "loss dlogits dvalue row_loss status")
_PVLOSS_WORKSPACES = _WorkspaceCache(1 << 12)  # of pv_loss calls that bring no workspace


def pv_loss_workspace(batch: int, device) -> torch.Tensor:
    """a zeroed workspace of the caller's own for pv_loss launches of up to `batch` rows (uint8; the ticket and one slot
    per workgroup).  Launches that share one belong on one stream."""
    need = int(lib().hk_pv_loss_workspace_bytes(int(batch)))
    if need == 0:
        raise ValueError(f"batch must be in [0, 2^31). Got {batch}.")
    return torch.zeros(need, dtype=torch.uint8, device=device)


def _pvloss_rows(t: torch.Tensor, name: str, dev=None) -> torch.Tensor:
    """a [rows, A] float32 block whose rows are contiguous (the rows themselves may be strided)"""
    _require_device(t, name)
    if t.dim() != 2 or t.dtype != torch.float32 or (dev is not None and t.device != dev):
        raise TypeError(f"{name} must be a [rows, A] float32 tensor{f' on {dev}' if dev is not None else ''}. Got "
                        f"{t.dtype} {tuple(t.shape)} on {t.device}.")
    ok = (t.shape[1] == 1 or t.stride(1) == 1) and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1])
    return t if ok else t.contiguous()


def _pvloss_column(t: torch.Tensor, name: str, rows: int, dev, dtype=torch.float32, strided: bool = False):
    """[rows] or [rows, 1] of `dtype` on `dev` as a 1-d view; contiguous unless `strided` (then: a positive stride)"""
    _require_device(t, name)
    if t.dtype != dtype or t.device != dev or t.dim() not in (1, 2) or t.numel() != rows or t.shape[0] != rows:
        raise TypeError(f"{name} must be [{rows}] or [{rows}, 1] {dtype} on {dev}. Got {t.dtype} {tuple(t.shape)} on "
                        f"{t.device}.")
    t = t[:, 0] if t.dim() == 2 else t
    if rows > 1 and (t.stride(0) < 1 or (not strided and t.stride(0) != 1)):
        t = t.contiguous()
    return t


def pv_loss(logits: torch.Tensor, value: torch.Tensor, target_policy: torch.Tensor, target_value: torch.Tensor,
            weight: Optional[torch.Tensor] = None, index: Optional[torch.Tensor] = None, *,
            workspace: Optional[torch.Tensor] = None, out: Optional[dict] = None,
            want: Sequence[str] = ("row_loss",)) -> PvLossResult:
    """policy_value_loss (hironaka/jax/loss.py:12-24) and its gradient with respect to logits and value in one launch
    (hk_pv_loss; the rule is in include/hironaka_hip_pvloss.h).

    logits [B, A] and value [B] or [B, 1]: float32, the network's outputs, rows possibly strided.  target_policy [N, A],
    target_value [N] and weight [N] (or None: 1): float32, the N samples; index [B] int64 (or None: N == B, row b takes
    sample b) says which sample a row takes.  Returns PvLossResult(loss [], dlogits [B, A], dvalue of value's shape,
    row_loss [B] or None, status int32 [1]): `want` names the optional output, `out` may bring tensors for any of "loss",
    "dlogits", "dvalue", "row_loss", "status" (a status brought along is OR-ed into, not cleared).  An index outside
    [0, N) gives a zero row and sets HK_PVLOSS_BAD_INDEX in status.  workspace: pv_loss_workspace(...) of the caller's
    own; None: one per device and stream.  Nothing here synchronises."""
    logits = _pvloss_rows(logits, "logits")
    dev = logits.device
    batch, nact = logits.shape
    target_policy = _pvloss_rows(target_policy, "target_policy", dev)
    samples = target_policy.shape[0]
    if not (1 <= nact <= A.HK_PVLOSS_MAX_ACTIONS and batch < 2 ** 31) or target_policy.shape[1] != nact:
        raise ValueError(f"A must be in [1, {A.HK_PVLOSS_MAX_ACTIONS}], the same for logits and target_policy, and B "
                         f"below 2^31. Got logits {tuple(logits.shape)}, target_policy {tuple(target_policy.shape)}.")
    value_shape = tuple(value.shape)
    value = _pvloss_column(value, "value", batch, dev, strided=True)
    target_value = _pvloss_column(target_value, "target_value", samples, dev)
    if weight is not None:
        weight = _pvloss_column(weight, "weight", samples, dev)
    if index is not None:
        index = _pvloss_column(index, "index", batch, dev, dtype=torch.int64)
    elif samples != batch:
        raise ValueError(f"without an index the targets have one row per batch row. Got {samples} samples, B = {batch}.")
    out = dict(out or {})
    unknown = (set(out) | set(want)) - set(PvLossResult._fields)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}")

    def given(name, shape, dtype):
        t = out.get(name)
        if t is None:
            return None
        _require_device(t, name)
        if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev:
            raise ValueError(f"out[{name!r}] must be {dtype} {shape} on {dev}. Got {t.dtype} {tuple(t.shape)}.")
        return t

    dlogits = given("dlogits", (batch, nact), torch.float32)
    if dlogits is None:
        dlogits = torch.empty((batch, nact), dtype=torch.float32, device=dev)
    elif not ((nact == 1 or dlogits.stride(1) == 1) and (batch <= 1 or dlogits.stride(0) >= nact)):
        raise ValueError(f"the rows of out['dlogits'] must each be contiguous. Got strides {dlogits.stride()}.")
    dvalue = given("dvalue", value_shape, torch.float32)
    if dvalue is None:
        dvalue = torch.empty(value_shape, dtype=torch.float32, device=dev)
    dvalue_1d = dvalue[:, 0] if dvalue.dim() == 2 else dvalue
    if batch > 1 and dvalue_1d.stride(0) < 1:
        raise ValueError(f"out['dvalue'] must have a positive stride. Got {dvalue.stride()}.")
    loss = given("loss", (), torch.float32)
    if loss is None:
        loss = torch.full((), float("nan"), dtype=torch.float32, device=dev) if batch == 0 else \
            torch.empty((), dtype=torch.float32, device=dev)
    status = given("status", (1,), torch.int32)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    row_loss = given("row_loss", (batch,), torch.float32)
    if row_loss is None and "row_loss" in want:
        row_loss = torch.empty(batch, dtype=torch.float32, device=dev)
    if row_loss is not None and not row_loss.is_contiguous():
        raise ValueError("out['row_loss'] must be contiguous.")
    need = int(lib().hk_pv_loss_workspace_bytes(batch))
    if workspace is None:
        workspace = _PVLOSS_WORKSPACES.get(dev, need)
    else:
        _require_device(workspace, "workspace")
        if (workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != dev
                or workspace.numel() < need):
            raise ValueError("workspace must be what pv_loss_workspace(batch, device) returns (or a larger one).")
    d = A.hk_pv_loss_desc()
    d.logits, d.value, d.target_policy, d.target_value = (logits.data_ptr(), value.data_ptr(), target_policy.data_ptr(),
                                                         target_value.data_ptr())
    d.weight = weight.data_ptr() if weight is not None else None
    d.index = index.data_ptr() if index is not None else None
    d.dlogits, d.dvalue, d.loss = dlogits.data_ptr(), dvalue_1d.data_ptr(), loss.data_ptr()
    d.row_loss = row_loss.data_ptr() if row_loss is not None else None
    d.workspace, d.status = workspace.data_ptr(), status.data_ptr()
    d.logits_stride, d.target_policy_stride, d.dlogits_stride = _dqn_stride(logits), _dqn_stride(target_policy), \
        _dqn_stride(dlogits)
    d.value_stride = value.stride(0) if batch > 1 else 1
    d.dvalue_stride = dvalue_1d.stride(0) if batch > 1 else 1
    d.num_samples, d.batch, d.actions, d.dtype, d.flags = samples, batch, nact, A.HK_F32, 0
    with torch.cuda.device(dev):
        check(lib().hk_pv_loss(C.byref(d), _stream(logits)), "hk_pv_loss")
    return PvLossResult(loss, dlogits, dvalue, row_loss, status)


# ---- the optimiser step: gradient clipping + Adam / SGD of a parameter list in two launches per 64 tensors ----------

OPTIM_KINDS = {"scale": A.HK_OPTIM_SCALE, "sgd": A.HK_OPTIM_SGD, "adam": A.HK_OPTIM_ADAM}
_OPTIM_WORKSPACES = _WorkspaceCache(  # of optim_prepare calls that bring no workspace
    1 << 12, "optim_prepare needs a larger workspace than this stream has, inside a stream capture: "
             "run one step before capturing, or bring workspace=ops.optim_workspace(...)")
_OPTIM_STATE_FIELDS = tuple(name for name, _ in A.hk_optim_state._fields_)


def optim_workgroups(numels: Sequence[int], dtype: torch.dtype) -> int:
    """the workgroups of hk_optim_prepare over gradients of these sizes: one per HK_OPTIM_CHUNK_BYTES of each"""
    esz = 8 if dtype == torch.float64 else 4
    return sum((int(n) * esz + A.HK_OPTIM_CHUNK_BYTES - 1) // A.HK_OPTIM_CHUNK_BYTES for n in numels)


def optim_workspace(total_workgroups: int, device) -> torch.Tensor:
    """a zeroed workspace of the caller's own for optim_prepare chains of up to `total_workgroups` workgroups (uint8; the
    ticket and one slot per workgroup).  Launches that share one belong on one stream."""
    need = int(lib().hk_optim_workspace_bytes(int(total_workgroups)))
    if need == 0:
        raise ValueError(f"total_workgroups must be in [0, 2^31). Got {total_workgroups}.")
    return torch.zeros(need, dtype=torch.uint8, device=device)


def optim_state(device, step: int = 0, beta1_pow: float = 1.0, beta2_pow: float = 1.0) -> torch.Tensor:
    """the 64-byte state block of one parameter group on the device (hk_optim_state as 8 float64 words; word 0 holds the
    int64 step count)"""
    block = torch.zeros(len(_OPTIM_STATE_FIELDS), dtype=torch.float64)
    block[1], block[2] = beta1_pow, beta2_pow
    block.view(torch.int64)[0] = int(step)
    return block.to(device)


def optim_state_read(state: torch.Tensor) -> dict:
    """the state block's fields as Python numbers (a copy to the host: synchronises)"""
    host = state.detach().cpu()
    out = {name: float(host[k]) for k, name in enumerate(_OPTIM_STATE_FIELDS)}
    out["step"] = int(host.view(torch.int64)[0])
    return out


class OptimChain:
    """The descriptors of one parameter list for optim_prepare / optim_apply: HK_OPTIM_MAX_TENSORS entries per launch,
    the launches of a chain one after the other on the current stream.  Built once per set of addresses (the optimisers
    keep theirs while the addresses stay); it holds the tensors alive.

    kind: "scale", "sgd" or "adam".  grads, and where the kind uses them params, state1 (exp_avg / momentum buffer) and
    state2 (exp_avg_sq): contiguous float32 or float64 tensors of one dtype on one HIP device (anything else is a
    TypeError), entry by entry of one size.  state: what optim_state(...) returns.  workspace: optim_workspace(...) of
    the caller's own; None: one per device and stream.  hold_grads=False: the chain does not keep the gradient tensors
    alive: bring them with set_grads(...) before every use."""

    def __init__(self, kind: str, grads: Sequence[torch.Tensor], params: Optional[Sequence[torch.Tensor]] = None,
                 state1: Optional[Sequence[torch.Tensor]] = None, state2: Optional[Sequence[torch.Tensor]] = None, *,
                 state: torch.Tensor, workspace: Optional[torch.Tensor] = None, hold_grads: bool = True):
        if kind not in OPTIM_KINDS:
            raise ValueError(f"kind must be one of {sorted(OPTIM_KINDS)}. Got {kind!r}.")
        grads = list(grads)
        columns = [("grads", grads)]
        for name, col in (("params", params), ("state1", state1), ("state2", state2)):
            col = list(col) if col is not None else None
            if col is not None and len(col) != len(grads):
                raise ValueError(f"{len(grads)} gradients but {len(col)} {name}.")
            columns.append((name, col))
        _require_device(state, "state")
        if state.dtype != torch.float64 or state.numel() != len(_OPTIM_STATE_FIELDS) or not state.is_contiguous():
            raise ValueError("state must be what optim_state(device) returns.")
        dev = state.device
        dtype = grads[0].dtype if grads else torch.float32
        for name, col in columns:
            for k, x in enumerate(col or ()):
                if not (isinstance(x, torch.Tensor) and x.is_cuda and x.layout == torch.strided and x.dtype == dtype
                        and x.device == dev and x.is_contiguous() and dtype in (torch.float32, torch.float64)):
                    _require_device(x, f"{name}[{k}]")
                    raise TypeError(f"every tensor must be a contiguous float32 or float64 tensor of one dtype on one "
                                    f"device ({dtype} on {dev}). {name}[{k}] is {x.dtype} on {x.device}, layout "
                                    f"{x.layout}, strides {x.stride() if x.layout == torch.strided else None}.")
                if x.numel() != grads[k].numel():
                    raise ValueError(f"entry {k}: {grads[k].numel()} gradient elements but {x.numel()} in {name}.")
        if workspace is not None:
            _require_device(workspace, "workspace")
            if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.device != dev:
                raise ValueError("workspace must be what optim_workspace(total_workgroups, device) returns.")
        self.kind, self.device, self.dtype, self.state, self.workspace = kind, dev, dtype, state, workspace
        # hold_grads=False: the caller brings the gradients on every use (set_grads): backward allocates new ones after
        # zero_grad(set_to_none=True), and held here the old ones would stay alive next to them
        self.keep = columns if hold_grads else columns[1:]
        self.numels = [g.numel() for g in grads]
        self.total_workgroups = optim_workgroups([g.numel() for g in grads], dtype)
        if workspace is not None and workspace.numel() < lib().hk_optim_workspace_bytes(self.total_workgroups):
            raise ValueError(f"workspace is smaller than optim_workspace({self.total_workgroups}, device).")
        self.descs = []
        per, slot_base = A.HK_OPTIM_MAX_TENSORS, 0
        cols = dict(columns)
        for at in range(0, max(len(grads), 1), per):
            d = A.hk_optim_desc()
            flat = []  # param, grad, state1, state2, numel of every entry as they lie in memory
            for k in range(at, min(at + per, len(grads))):
                flat += [cols[name][k].data_ptr() if cols[name] is not None else 0
                         for name in ("params", "grads", "state1", "state2")]
                flat.append(grads[k].numel())
            if flat:
                (C.c_int64 * len(flat)).from_address(C.addressof(d))[:] = flat
            d.ntensors, d.dtype, d.kind, d.slot_base = len(flat) // 5, _TORCH2HK[dtype], OPTIM_KINDS[kind], slot_base
            d.state = state.data_ptr()
            slot_base += optim_workgroups([grads[k].numel() for k in range(at, min(at + per, len(grads)))], dtype)
            self.descs.append(d)
        # the descriptors' tables as int64 words, five per entry: word 1 of an entry is its gradient's address
        self._words = [(C.c_int64 * (5 * d.ntensors)).from_address(C.addressof(d)) for d in self.descs]
        self._lr_dev = None

    def set_grads(self, grads: Sequence[torch.Tensor]) -> None:
        """point the descriptors at these gradients: the same number, sizes, dtype and device as the chain was built
        with, each contiguous (anything else is a TypeError / ValueError); everything else of the chain stays"""
        if len(grads) != len(self.numels):
            raise ValueError(f"the chain has {len(self.numels)} entries. Got {len(grads)} gradients.")
        dtype, dev = self.dtype, self.device
        for k, g in enumerate(grads):
            if not (g.dtype == dtype and g.device == dev and g.layout == torch.strided and g.is_contiguous()):
                raise TypeError(f"grads[{k}] must be a contiguous {dtype} tensor on {dev}. Got {g.dtype} on {g.device}, "
                                f"layout {g.layout}.")
            if g.numel() != self.numels[k]:
                raise ValueError(f"entry {k}: the chain has {self.numels[k]} elements, the gradient {g.numel()}.")
        per = A.HK_OPTIM_MAX_TENSORS
        for at, words in zip(range(0, len(grads), per), self._words):
            words[1::5] = [g.data_ptr() for g in grads[at:at + per]]
        if self.keep[0][0] == "grads":
            self.keep[0] = ("grads", list(grads))


def optim_prepare(chain: OptimChain, *, max_norm: float = float("inf"), lr=0.0, beta1: float = 0.0, beta2: float = 0.0,
                  advance: bool = False, clip: bool = True) -> None:
    """hk_optim_prepare over the chain (include/hironaka_hip_optim.h): one pass over the gradients that leaves
    total_norm, clip_coef = min(1, max_norm / (total_norm + 1e-6)) (clip=False: 1 whatever the norm is) and, with
    `advance`, the next step's count, running powers of the betas, -lr / (1 - beta1^step) and sqrt(1 - beta2^step) in the
    chain's state block.  lr: a float, or a one-element tensor on the device (a learning-rate schedule under graph
    replay): a float64 one is read where it lies, one of another dtype is converted first, which costs a launch and an
    allocation per call.  Nothing here synchronises."""
    dev = chain.device
    lr_dev = None
    if isinstance(lr, torch.Tensor):
        _require_device(lr, "lr")
        if lr.numel() != 1 or lr.device != dev:
            raise ValueError(f"lr must be a float or a one-element tensor on {dev}. Got {tuple(lr.shape)} on {lr.device}.")
        lr_dev = lr.detach().reshape(1)
        if lr_dev.dtype != torch.float64:
            lr_dev = lr_dev.to(torch.float64)
        chain._lr_dev = lr_dev  # alive until the next call
    with torch.cuda.device(dev):
        ws = chain.workspace
        if ws is None:
            ws = _OPTIM_WORKSPACES.get(dev, int(lib().hk_optim_workspace_bytes(chain.total_workgroups)))
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for k, d in enumerate(chain.descs):
            d.workspace = ws.data_ptr()
            d.lr_dev = lr_dev.data_ptr() if lr_dev is not None else None
            d.lr = 0.0 if lr_dev is not None else float(lr)
            d.beta1, d.beta2, d.max_norm = float(beta1), float(beta2), float(max_norm)
            d.flags = ((A.HK_OPTIM_LAST if k == len(chain.descs) - 1 else 0) | (A.HK_OPTIM_ADVANCE if advance else 0)
                       | (0 if clip else A.HK_OPTIM_NO_CLIP))
            check(lib().hk_optim_prepare(C.byref(d), stream), "hk_optim_prepare")


def optim_apply(chain: OptimChain, *, eps: float = 1e-8, weight_decay: float = 0.0, momentum: float = 0.0,
                dampening: float = 0.0, nesterov: bool = False, beta1: float = 0.9, beta2: float = 0.999,
                keep_grads: bool = False) -> None:
    """hk_optim_apply over the chain with the scalars optim_prepare left in its state block: "scale" grad *= clip_coef;
    "sgd" / "adam" clip, then torch.optim.SGD's / Adam's update (the rules: include/hironaka_hip_optim.h).  The clipped
    gradient is written back unless keep_grads.  Nothing here synchronises."""
    with torch.cuda.device(chain.device):
        stream = C.c_void_p(torch.cuda.current_stream(chain.device).cuda_stream)
        for d in chain.descs:
            d.eps, d.weight_decay, d.momentum, d.dampening = float(eps), float(weight_decay), float(momentum), float(dampening)
            d.beta1, d.beta2 = float(beta1), float(beta2)
            d.flags = (A.HK_OPTIM_KEEP_GRADS if keep_grads else 0) | (A.HK_OPTIM_NESTEROV if nesterov else 0)
            check(lib().hk_optim_apply(C.byref(d), stream), "hk_optim_apply")


# ---- one level of a game tree under any host (hk_tree_expand) -------------------------------------------------------

TreeExpandResult = collections.namedtuple(
    "TreeExpandResult", "children child_parent child_axis child_num_points child_done total status")
_class_sizes_cache: Dict[Tuple[int, torch.device], torch.Tensor] = {}


def _class_sizes(d: int, device: torch.device) -> torch.Tensor:
    """int64 [2^d - d - 1]: the number of coordinates of every host class of dimension d"""
    key = (d, device)
    if key not in _class_sizes_cache:
        sizes = [bin(v).count("1") for v in range(1, 1 << d) if v & (v - 1)]
        _class_sizes_cache[key] = torch.tensor(sizes, dtype=torch.int64, device=device)
    return _class_sizes_cache[key]


def _tree_records(t: torch.Tensor, m: int, d: int, name: str) -> torch.Tensor:
    """the [N, m, d] view of states given as [N, m, d], [N, m*d] or records [N, m*d + d]: a view where the states
    are contiguous records at any stride and offset, else a copy"""
    if t.dim() == 3 and tuple(t.shape[1:]) == (m, d):
        v = t
    elif t.dim() == 2 and t.shape[1] in (m * d, m * d + d):
        if t.stride(1) == 1:
            v = t.as_strided((t.shape[0], m, d), (t.stride(0), d, 1), t.storage_offset())
        else:
            v = t[:, :m * d].contiguous().view(-1, m, d)
    else:
        raise ValueError(f"{name} must be [N, {m}, {d}], [N, {m * d}] or records [N, {m * d + d}]. "
                         f"Got shape {tuple(t.shape)}.")
    return v if _record_stride(v) is not None else v.contiguous()


def tree_expand(parents: torch.Tensor, class_id: torch.Tensor, *, spec: Tuple[int, int], sem: str = "jax",
                reposition: bool = True, out: Optional[torch.Tensor] = None, capacity: Optional[int] = None,
                zero_tail: bool = False) -> TreeExpandResult:
    """One level of hironaka/jax/search.py:73-113 search_tree_fix_host over a whole frontier, in one launch
    (hk_tree_expand).  parents: N states of spec=(m, d) as [N, m, d], [N, m*d] or records [N, m*d + d], float32 or
    float64; contiguous records at any stride and offset are read in place, any other view through a copy.  class_id:
    int32/int64 [N], the host's subset per parent; an id < 0 (or beyond the dimension's classes) means "do not
    expand".  A parent has one child per coordinate of its subset in ascending order; the children are packed in
    parent order.  sem: "jax" (shift, [reposition], Newton polytope; rows keep their places) or "list" (the same,
    then sorted and compacted).  out: the children's buffer, [capacity, m, d], [capacity, m*d] or records
    [capacity, m*d + d] of contiguous records; default a new one, records when ``zero_tail`` else [capacity, m, d],
    uninitialised from ``total`` on.  capacity: the child slots that exist, default all of ``out``, or N*d.  A child
    without a slot is dropped and HK_TREE_OVERFLOW is set in ``status``.  zero_tail: write d zeros behind every child's
    state (``out`` must be records then); otherwise only the states are written.  Returns TreeExpandResult(children,
    child_parent, child_axis, child_num_points, child_done, total, status): the per-child tensors have ``capacity``
    entries, ``total`` (int64 scalar on the device) of which are children when nothing was dropped; status is an int32
    scalar on the device.  Nothing here synchronises."""
    if sem not in ("jax", "list"):
        raise ValueError(f"sem must be 'jax' or 'list'. Got {sem!r}.")
    m, d = (int(v) for v in spec)
    _require_device(parents, "parents")
    _require_device(class_id, "class_id")
    if parents.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"parents must be float32 or float64. Got {parents.dtype}.")
    dev = parents.device
    src = _tree_records(parents, m, d, "parents")
    n = src.shape[0]
    if class_id.dtype not in (torch.int32, torch.int64) or tuple(class_id.shape) != (n,) or class_id.device != dev:
        raise ValueError(f"class_id must be an int32/int64 tensor of shape {(n,)} on the parents' device. Got "
                         f"{class_id.dtype} {tuple(class_id.shape)} on {class_id.device}.")
    sizes = _class_sizes(d, dev)
    cls64 = class_id.to(torch.int64)
    valid = (cls64 >= 0) & (cls64 < sizes.numel())
    cls = torch.where(valid, cls64, cls64.new_full((), -1)).to(torch.int32)
    counts = torch.where(valid, sizes[cls64.clamp(0, sizes.numel() - 1)], cls64.new_zeros(()))
    ends = torch.cumsum(counts, 0)
    offsets = (ends - counts).contiguous()
    total = ends[-1] if n else torch.zeros((), dtype=torch.int64, device=dev)
    if out is not None:
        _require_device(out, "out")
        if out.dtype != parents.dtype or out.device != dev:
            raise ValueError(f"out must be {parents.dtype} on {dev}. Got {out.dtype} on {out.device}.")
        if zero_tail and not (out.dim() == 2 and out.shape[1] == m * d + d):
            raise ValueError(f"zero_tail needs out as records [capacity, {m * d + d}]. Got shape {tuple(out.shape)}.")
        dst = _tree_records(out, m, d, "out")
        if out.numel() and dst.data_ptr() != out.data_ptr():
            raise ValueError("out must hold contiguous records (any stride between them): the children are written "
                             "in place.")
        capacity = out.shape[0] if capacity is None else capacity
        if not 0 <= capacity <= out.shape[0]:
            raise ValueError(f"capacity must lie in [0, {out.shape[0]}] (the records of out). Got {capacity}.")
        children = out
    else:
        capacity = n * d if capacity is None else capacity
        if not 0 <= capacity < 2 ** 31:
            raise ValueError(f"capacity must lie in [0, 2^31). Got {capacity}.")
        children = torch.empty((capacity, m * d + d) if zero_tail else (capacity, m, d), dtype=parents.dtype, device=dev)
        dst = _tree_records(children, m, d, "out")
    if n >= 2 ** 31:
        raise ValueError(f"at most 2^31 - 1 parents per call. Got {n}.")
    new = lambda dtype: torch.empty(capacity, dtype=dtype, device=dev)  # noqa: E731
    c_par, c_ax, c_np, c_done = new(torch.int32), new(torch.int32), new(torch.int32), new(torch.bool)
    status = torch.zeros((), dtype=torch.int32, device=dev)
    q = A.hk_tree_expand_desc()
    q.parents_in, q.children_out = src.data_ptr(), dst.data_ptr()
    q.in_stride = _record_stride(src)
    # (a buffer of one record has no stride between records: with a tail, the tail belongs to the record)
    q.out_stride = m * d + d if zero_tail and dst.shape[0] <= 1 else _record_stride(dst)
    q.class_id, q.child_offset = cls.data_ptr(), offsets.data_ptr()
    q.child_parent, q.child_axis = c_par.data_ptr(), c_ax.data_ptr()
    q.child_num_points, q.child_done, q.status = c_np.data_ptr(), c_done.data_ptr(), status.data_ptr()
    q.n_parents, q.capacity, q.max_points, q.dim = n, capacity, m, d
    q.dtype, q.sem = _TORCH2HK[parents.dtype], A.SEMANTICS[sem]
    q.flags = (A.HK_TREE_REPOSITION if reposition else 0) | (A.HK_TREE_ZERO_TAIL if zero_tail else 0)
    with torch.cuda.device(dev):
        check(lib().hk_tree_expand(C.byref(q), _stream(parents)), "hk_tree_expand")
    return TreeExpandResult(children, c_par, c_ax, c_np, c_done, total, status)


# ---- the eval-mode forward of a create_mlp stack in one launch ---------------------------------------------------------

MlpLayer = collections.namedtuple("MlpLayer", "weight bias bn_mean bn_var bn_weight bn_bias eps relu",
                                  defaults=(None, None, None, None, None, 1e-5, False))
MlpLayer.__doc__ = """One `Linear [-> BatchNorm1d (eval)] [-> ReLU]` block of mlp_forward: weight [n, k] as nn.Linear
keeps it, bias [n] or None, the batch norm's running_mean / running_var [n] (both None: no batch norm) with its weight /
bias [n] or None (affine=False) and eps, relu: whether a ReLU follows."""
_MLP_TILES = {None: 0, A.HK_MLP_TILE_SMALL: A.HK_MLP_FORCE_TILE_SMALL, A.HK_MLP_TILE_LARGE: A.HK_MLP_FORCE_TILE_LARGE}


def _mlp_tensor(x, name: str, dev: Optional[torch.device], shape=None) -> Optional[int]:
    """the address of a contiguous float32 tensor on `dev` (of `shape`, if given); None for None"""
    if x is None:
        return None
    _require_device(x, name)
    if x.dtype != torch.float32 or x.layout != torch.strided or not x.is_contiguous() or (dev is not None
                                                                                          and x.device != dev):
        raise TypeError(f"{name} must be a contiguous float32 tensor on {dev}. Got {x.dtype} on {x.device}, "
                        f"strides {x.stride() if x.layout == torch.strided else None}.")
    if shape is not None and tuple(x.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}. Got {tuple(x.shape)}.")
    return x.data_ptr()


def _mlp_widths(weight, table: str, i: int, field: str, width: Optional[int]):
    """(n, k) of the weight [n, k] of entry i of a plan's `table` ("layers" / "blocks"): k is the `width` the entry before
    gives (None: the first entry), and both lie within the limit"""
    if not isinstance(weight, torch.Tensor) or weight.dim() != 2:
        raise TypeError(f"{table}[{i}].{field} must be a [n, k] tensor.")
    n, k = weight.shape
    if width is not None and k != width:
        raise ValueError(f"{table}[{i}] takes {k} inputs but {table}[{i - 1}] gives {width}.")
    if not (1 <= k <= A.HK_MLP_MAX_WIDTH and 1 <= n <= A.HK_MLP_MAX_WIDTH):
        raise ValueError(f"{table}[{i}]: widths must lie in 1..{A.HK_MLP_MAX_WIDTH}. Got [{n}, {k}].")
    return n, k


def _mlp_tile_flag(tile: Optional[int]) -> int:
    """the descriptor flag that forces the row tile `tile` (None: 0, the library picks)"""
    if tile not in _MLP_TILES:
        raise ValueError(f"tile must be None, {A.HK_MLP_TILE_SMALL} or {A.HK_MLP_TILE_LARGE}. Got {tile!r}.")
    return _MLP_TILES[tile]


def _mlp_batch_limit(batch: int) -> None:
    if batch >= 2 ** 31:
        raise ValueError(f"at most 2^31 - 1 rows per call. Got {batch}.")


def _mlp_given_out(out: torch.Tensor, name: str, dev: torch.device, shape) -> None:
    """an output tensor the caller gave: float32 on `dev`, of `shape` ([B, n] or [B]), the elements of a row adjacent and
    the rows at least a row apart"""
    _require_device(out, name)
    if out.dtype != torch.float32 or out.device != dev:
        raise TypeError(f"{name} must be a float32 tensor on {dev}. Got {out.dtype} on {out.device}.")
    n = shape[1] if len(shape) > 1 else 1
    if tuple(out.shape) != tuple(shape) or (n > 1 and out.stride(1) != 1) or (shape[0] > 1 and out.stride(0) < n):
        raise ValueError(f"{name} must be {list(shape)} with adjacent elements in a row and rows that do not overlap. "
                         f"Got shape {tuple(out.shape)}, strides {out.stride()}.")


class _MlpTable:
    """What MlpPlan and MlpTrainPlan share: the walk over `layers` (entries of LAYER, or tuples in its order) that
    checks them and fills the layer table of a DESC, whose fields STATS take a batch norm's running statistics.  It
    leaves `desc`, `device`, `k_in`, `n_out` and `tensors` (what the table points at, held alive); _own adds what a
    plan keeps of a layer besides."""
    LAYER = DESC = STATS = None

    def _fill(self, layers, input_relu: bool):
        layers = [l if isinstance(l, self.LAYER) else self.LAYER(*l) for l in layers]
        if not 1 <= len(layers) <= A.HK_MLP_MAX_LAYERS:
            raise ValueError(f"1 to {A.HK_MLP_MAX_LAYERS} layers. Got {len(layers)}.")
        _require_device(layers[0].weight, "layers[0].weight")
        self.device = dev = layers[0].weight.device
        self.desc = d = self.DESC()
        self.tensors = []
        width = None
        for i, l in enumerate(layers):
            n, k = _mlp_widths(l.weight, "layers", i, "weight", width)
            bn = l.bn_mean is not None
            # (bn_weight, bn_bias and, where LAYER has one, num_batches_tracked belong to a batch norm)
            if bn != (l.bn_var is not None) or (not bn and any(t is not None for t in l[4:6] + l[9:])):
                raise ValueError(f"layers[{i}]: a batch norm needs both bn_mean and bn_var.")
            width = n
            e = d.layer[i]
            e.weight = _mlp_tensor(l.weight, f"layers[{i}].weight", dev)
            for field, name in zip(("bias",) + self.STATS + ("bn_weight", "bn_bias"), self.LAYER._fields[1:6]):
                setattr(e, field, _mlp_tensor(getattr(l, name), f"layers[{i}].{name}", dev, (n,)))
            e.eps, e.k, e.n, e.flags = float(l.eps), k, n, A.HK_MLP_RELU if l.relu else 0
            self.tensors += [t for t in l[:6] if t is not None]
            self._own(i, l, e, bn)
        d.nlayers, d.dtype, d.flags = len(layers), A.HK_F32, A.HK_MLP_INPUT_RELU if input_relu else 0
        self.k_in, self.n_out = layers[0].weight.shape[1], width

    def _own(self, i: int, l, e, bn: bool):
        """what a plan adds for layer i: l of LAYER, its table entry e, whether it has a batch norm"""


class MlpPlan(_MlpTable):
    """The layer table of mlp_forward, built once per set of parameter addresses (it holds the tensors alive):
    `layers` is a sequence of MlpLayer (or tuples in its order).  The table points at the tensors it was given: whoever
    swaps a tensor for another builds a new plan (hironaka_amd.nets.FusedSequential does, by the addresses of the
    tensors its modules hold at each call)."""
    LAYER, DESC, STATS = MlpLayer, A.hk_mlp_desc, ("bn_mean", "bn_var")

    def __init__(self, layers: Sequence[MlpLayer], input_relu: bool = False, input_bn: Optional[MlpLayer] = None):
        self._fill(layers, input_relu)
        if input_bn is not None:  # an MlpLayer whose batch-norm fields alone count: the batch norm on the input
            if input_bn.bn_mean is None or input_bn.bn_var is None:
                raise ValueError("input_bn needs both bn_mean and bn_var.")
            for name in ("bn_mean", "bn_var", "bn_weight", "bn_bias"):
                setattr(self.desc, "in_" + name,
                        _mlp_tensor(getattr(input_bn, name), f"input_bn.{name}", self.device, (self.k_in,)))
            self.desc.in_eps = float(input_bn.eps)
            self.tensors += [t for t in input_bn[2:6] if t is not None]


def _mlp_rows(x: torch.Tensor, name: str, dev: torch.device) -> torch.Tensor:
    """x as [B, k] float32 rows on `dev` whose elements are adjacent (the rows may lie any number of elements apart)"""
    _require_device(x, name)
    if x.dtype != torch.float32 or x.device != dev:
        raise TypeError(f"{name} must be a float32 tensor on {dev}. Got {x.dtype} on {x.device}.")
    if x.dim() < 2:
        raise ValueError(f"{name} must have a batch dimension and at least one more. Got shape {tuple(x.shape)}.")
    if x.dim() > 2:
        x = x.flatten(1)
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    return x


def _mlp_inputs(plan: _MlpTable, x0: torch.Tensor, x1: Optional[torch.Tensor]):
    """x0 and x1 (or None) as rows (_mlp_rows) that together are the plan's input"""
    x0 = _mlp_rows(x0, "x0", plan.device)
    batch, k0 = x0.shape
    k1 = 0
    if x1 is not None:
        x1 = _mlp_rows(x1, "x1", plan.device)
        k1 = x1.shape[1]
        if x1.shape[0] != batch:
            raise ValueError(f"x0 has {batch} rows but x1 has {x1.shape[0]}.")
    if k0 + k1 != plan.k_in:
        raise ValueError(f"the first layer takes {plan.k_in} inputs. Got {k0}{' + ' + str(k1) if x1 is not None else ''}.")
    return x0, x1


def _mlp_fill_inputs(d, x0: torch.Tensor, x1: Optional[torch.Tensor]) -> None:
    """the input's fields of a descriptor: the rows of _mlp_inputs and their count"""
    batch, k0 = x0.shape
    k1 = x1.shape[1] if x1 is not None else 0
    d.x0, d.x0_stride, d.k0 = x0.data_ptr(), x0.stride(0) if batch > 1 else k0, k0
    d.x1, d.x1_stride, d.k1 = (x1.data_ptr(), x1.stride(0) if batch > 1 else k1, k1) if k1 else (None, 0, 0)
    d.batch = batch


def mlp_forward(x0: torch.Tensor, layers, x1: Optional[torch.Tensor] = None, input_relu: bool = False,
                out: Optional[torch.Tensor] = None, tile: Optional[int] = None,
                input_bn: Optional[MlpLayer] = None) -> torch.Tensor:
    """The forward of `Linear [-> BatchNorm1d (eval)] [-> ReLU]` blocks in ONE launch (hk_mlp_forward; the rule, to the
    bit, is in include/hironaka_hip_mlp.h).  Row b of the input is x0[b] flattened, followed by x1[b] flattened if x1 is
    given; input_bn (an MlpLayer whose batch-norm fields alone count) applies an eval-mode batch norm to it first,
    input_relu a ReLU after that.  `layers`: a sequence of MlpLayer, or an MlpPlan built from one (its own input_relu
    and input_bn count then).  out: a [B, n] float32 tensor with adjacent elements in a row to write into (rows any
    number of elements >= n apart); None: a new one.  tile: None, or the row tile (16 / 64) to force -- same bits.
    Everything is float32 on one HIP device (a TypeError otherwise).  Nothing here synchronises."""
    plan = layers if isinstance(layers, MlpPlan) else MlpPlan(layers, input_relu, input_bn)
    tile_flag = _mlp_tile_flag(tile)
    dev = plan.device
    x0, x1 = _mlp_inputs(plan, x0, x1)
    batch = x0.shape[0]
    _mlp_batch_limit(batch)
    if out is None:
        out = torch.empty((batch, plan.n_out), dtype=torch.float32, device=dev)
    else:
        _mlp_given_out(out, "out", dev, (batch, plan.n_out))
    if batch == 0:
        return out
    d = plan.desc
    _mlp_fill_inputs(d, x0, x1)
    d.out, d.out_stride = out.data_ptr(), out.stride(0) if batch > 1 else plan.n_out
    d.flags = (d.flags & A.HK_MLP_INPUT_RELU) | tile_flag
    with torch.cuda.device(dev):
        check(lib().hk_mlp_forward(C.byref(d), _stream(out)), "hk_mlp_forward")
    return out


# ---- the gradient-free forward of a DenseResNet / DenseNet policy-value network in one launch ------------------------------

PvnetDense = collections.namedtuple("PvnetDense", "weight bias gn_scale gn_bias", defaults=(None, None, None))
PvnetDense.__doc__ = """One `Dense [-> GroupNorm(32)]` of pvnet_forward: weight [n, k] as nn.Linear keeps it, bias [n] or
None, the group norm's scale / bias [n] or None (a dense block has no norm: both are ignored)."""
PvnetBlock = collections.namedtuple("PvnetBlock", "kind dense1 dense2 proj eps", defaults=(None, None, 1e-6))
PvnetBlock.__doc__ = """One block of pvnet_forward's trunk: kind "dense" (`relu(Dense1(h))`) or "residue"
(`relu(o + GN2(Dense2(relu(GN1(Dense1(h))))))` with o = h, or GNp(Densep(h)) where the block changes the width); dense1,
dense2, proj: PvnetDense (or tuples in its order); eps: the group norms' (flax's default)."""
_PVNET_KINDS = {"dense": A.HK_PVNET_DENSE, "residue": A.HK_PVNET_RESIDUE}
PVNET_NORMED_WIDTHS = A.PVNET_NORMED_WIDTHS


class PvnetPlan:
    """The block table of pvnet_forward, built once per set of parameter addresses (it holds the tensors alive): `blocks`
    is a sequence of PvnetBlock, `policy` and `value` are the heads' (weight [A, n], bias [A] or None) and (weight [1, n],
    bias [1] or None).  The table points at the tensors it was given: whoever swaps a tensor for another builds a new plan
    (hironaka_amd.net.DenseResNet does, by the addresses of the tensors its modules hold at each call)."""

    def __init__(self, blocks: Sequence[PvnetBlock], policy, value, *, _head_extra: int = 0):
        # (_head_extra: CustomnetPlan's heads, which read that many features behind the trunk's result)
        blocks = [b if isinstance(b, PvnetBlock) else PvnetBlock(*b) for b in blocks]
        if not 1 <= len(blocks) <= A.HK_PVNET_MAX_BLOCKS:
            raise ValueError(f"1 to {A.HK_PVNET_MAX_BLOCKS} blocks. Got {len(blocks)}.")
        first = PvnetDense(*blocks[0].dense1).weight
        _require_device(first, "blocks[0].dense1.weight")
        self.device = dev = first.device
        self.desc = d = A.hk_pvnet_desc()
        self.tensors = []
        # the parameters in module order -- per block dense1, dense2, proj (those it has), per Dense weight, bias, gn_scale,
        # gn_bias (those that exist), then the policy head's and the value head's: the order of pvnet_backward's gradients;
        # grad_fields says where each one's gradient goes in an hk_pvgrad_desc: (block or "policy" / "value", Dense, field)
        self.params, self.grad_fields = [], []
        width = None

        def fill(i, which, dense, n, k, normed=True):
            e, name = getattr(d.block[i], which), f"blocks[{i}].{which}"
            dense = PvnetDense(*dense)
            if not isinstance(dense.weight, torch.Tensor) or tuple(dense.weight.shape) != (n, k):
                raise ValueError(f"{name}.weight must be a [{n}, {k}] tensor.")
            e.weight = _mlp_tensor(dense.weight, f"{name}.weight", dev)
            for field in ("bias", "gn_scale", "gn_bias"):
                setattr(e, field, _mlp_tensor(getattr(dense, field), f"{name}.{field}", dev, (n,)))
            self.tensors += [t for t in dense if t is not None]
            for field, t in zip(("d_weight", "d_bias", "d_gn_scale", "d_gn_bias"), dense if normed else dense[:2]):
                if t is not None:
                    self.params.append(t)
                    self.grad_fields.append((i, which, field))

        for i, b in enumerate(blocks):
            if b.kind not in _PVNET_KINDS:
                raise ValueError(f'blocks[{i}].kind must be "dense" or "residue". Got {b.kind!r}.')
            n, k = _mlp_widths(PvnetDense(*b.dense1).weight, "blocks", i, "dense1.weight", width)
            width = n
            e = d.block[i]
            e.k, e.n, e.kind, e.eps = k, n, _PVNET_KINDS[b.kind], float(b.eps)
            fill(i, "dense1", b.dense1, n, k, b.kind == "residue")
            if b.kind == "residue":
                if n not in PVNET_NORMED_WIDTHS:
                    raise ValueError(f"blocks[{i}]: a normed width must be one of {PVNET_NORMED_WIDTHS}. Got {n}.")
                if b.dense2 is None or (k != n and b.proj is None):
                    raise ValueError(f"blocks[{i}]: a residue block needs dense2, and proj where it changes the width.")
                fill(i, "dense2", b.dense2, n, n)
                if k != n:
                    fill(i, "proj", b.proj, n, k)
        actions = policy[0].shape[0] if isinstance(policy[0], torch.Tensor) and policy[0].dim() == 2 else 0
        if not 1 <= actions <= A.HK_PVNET_MAX_WIDTH - 1:
            raise ValueError(f"the policy head must have 1 to {A.HK_PVNET_MAX_WIDTH - 1} outputs. Got {actions}.")
        self.n_last, width = width, width + int(_head_extra)
        for name, (weight, bias), n in (("policy", policy, actions), ("value", value, 1)):
            if not isinstance(weight, torch.Tensor) or tuple(weight.shape) != (n, width):
                raise ValueError(f"{name}[0] must be a [{n}, {width}] tensor.")
            setattr(d, name + "_weight", _mlp_tensor(weight, f"{name}[0]", dev))
            setattr(d, name + "_bias", _mlp_tensor(bias, f"{name}[1]", dev, (n,)))
            self.tensors += [t for t in (weight, bias) if t is not None]
            for field, t in (("d_weight", weight), ("d_bias", bias)):
                if t is not None:
                    self.params.append(t)
                    self.grad_fields.append((name, None, field))
        d.nblocks, d.actions, d.dtype = len(blocks), actions, A.HK_F32
        self.k_in, self.actions = PvnetDense(*blocks[0].dense1).weight.shape[1], actions


def pvnet_forward(x: torch.Tensor, plan: PvnetPlan, tile: Optional[int] = None, raw_value: bool = False,
                  policy: Optional[torch.Tensor] = None, value: Optional[torch.Tensor] = None, *,
                  gate: Optional[Tuple[torch.Tensor, int]] = None,
                  out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """The forward of a trunk of dense / residue blocks with a policy head and a tanh value head in ONE launch
    (hk_pvnet_forward; the rule, to the bit, is in include/hironaka_hip_pvnet.h).  x: [B, ...] float32 rows (flattened
    behind the batch dimension; the rows may lie any number of elements apart).  Returns (policy [B, A], value [B]).
    policy / value: float32 tensors of these shapes to write into (policy with adjacent elements in a row, rows >= A
    apart; value at any element stride >= 1); None: new ones.  out: the two as a pair.  tile: None, or the row tile
    (16 / 64) to force -- same bits.  raw_value: store the value head before the tanh.  gate: (word, want) -- an int32
    tensor of one element on the device and an int: the launch computes only where the word holds `want` when the
    kernel runs (hk_unified_pvnet_forward, include/hironaka_hip_unified.h), otherwise it leaves policy and value as they
    are; the decision is the device's, nothing is read back.  Everything is float32 on one HIP device (a TypeError
    otherwise).  Nothing here synchronises."""
    if not isinstance(plan, PvnetPlan):
        raise TypeError(f"plan must be a PvnetPlan. Got {type(plan).__name__}.")
    if out is not None:
        if policy is not None or value is not None:
            raise ValueError("give the outputs as out=(policy, value) or as policy= / value=, not both.")
        policy, value = out
    if gate is not None:
        word, want = gate
        _require_device(word, "gate[0]")
        if word.dtype != torch.int32 or word.numel() != 1 or word.device != plan.device:
            raise TypeError(f"gate[0] must be an int32 tensor of one element on {plan.device}. "
                            f"Got {word.dtype} {tuple(word.shape)} on {word.device}.")
    tile_flag = _mlp_tile_flag(tile)
    dev = plan.device
    x = _mlp_rows(x, "x", dev)
    batch, k0 = x.shape
    if k0 != plan.k_in:
        raise ValueError(f"the first block takes {plan.k_in} inputs. Got {k0}.")
    _mlp_batch_limit(batch)
    a = plan.actions
    for name, out, shape in (("policy", policy, (batch, a)), ("value", value, (batch,))):
        if out is not None:
            _mlp_given_out(out, name, dev, shape)
    if policy is None:
        policy = torch.empty((batch, a), dtype=torch.float32, device=dev)
    if value is None:
        value = torch.empty((batch,), dtype=torch.float32, device=dev)
    if batch == 0:
        return policy, value
    d = plan.desc
    d.x, d.x_stride, d.k0, d.batch = x.data_ptr(), x.stride(0) if batch > 1 else k0, k0, batch
    d.policy, d.policy_stride = policy.data_ptr(), policy.stride(0) if batch > 1 else a
    d.value, d.value_stride = value.data_ptr(), value.stride(0) if batch > 1 else 1
    d.flags = tile_flag | (A.HK_PVNET_RAW_VALUE if raw_value else 0)
    with torch.cuda.device(dev):
        if gate is None:
            check(lib().hk_pvnet_forward(C.byref(d), _stream(policy)), "hk_pvnet_forward")
        else:
            check(lib().hk_unified_pvnet_forward(C.byref(d), word.data_ptr(), int(want), _stream(policy)),
                  "hk_unified_pvnet_forward")
    return policy, value


# ---- the gradient-free forward of CustomNet: one tower per row, chosen by its point count (hironaka_hip_customnet.h) --------

class CustomnetPlan:
    """The tower table of customnet_forward in device memory, the heads and the workspace, built once per set of parameter
    addresses (it holds the tensors alive).  `towers`: m sequences of PvnetBlock, tower t for the rows with t points -- its
    first block takes (t + 1) * d + e inputs, every tower has the same number of blocks, kinds and output widths; `policy`
    / `value`: the heads' (weight [A, n_last + e], bias or None) and (weight [1, n_last + e], bias or None); `spec`:
    (m, d); `extra_dim`: e.  Every record is checked against pvnet_forward's rules here, once: the library cannot read
    the table (include/hironaka_hip_customnet.h).  The workspace grows with the batches the plan is called on."""

    def __init__(self, towers, policy, value, spec: Tuple[int, int], extra_dim: int):
        m, d = (int(v) for v in spec)
        e = int(extra_dim)
        towers = [list(t) for t in towers]
        if not 1 <= m <= A.HK_CUSTOMNET_MAX_POINTS or d < 2 or e < 0 or m * d + e > A.HK_PVNET_MAX_WIDTH:
            raise ValueError(f"1 to {A.HK_CUSTOMNET_MAX_POINTS} points of at least 2 coordinates and m * d + e <= "
                             f"{A.HK_PVNET_MAX_WIDTH}. Got m={m}, d={d}, e={e}.")
        if len(towers) != m:
            raise ValueError(f"one tower per point count: {m}. Got {len(towers)}.")
        plans = [PvnetPlan(t, policy, value, _head_extra=e) for t in towers]
        shapes = [[(b.kind, b.n) for b in p.desc.block[: p.desc.nblocks]] for p in plans]
        if any(s != shapes[0] for s in shapes):
            raise ValueError("every tower must have the same blocks: kinds and output widths.")
        for t, p in enumerate(plans):
            if p.k_in != (t + 1) * d + e:
                raise ValueError(f"towers[{t}] must take {(t + 1) * d + e} inputs. Got {p.k_in}.")
        first = plans[0]
        if first.n_last + e > A.HK_PVNET_MAX_WIDTH:
            raise ValueError(f"n_last + e must be at most {A.HK_PVNET_MAX_WIDTH}. Got {first.n_last} + {e}.")
        self.device = dev = first.device
        self.tensors = [t for p in plans for t in p.tensors]
        self.m, self.d, self.e, self.k_in, self.actions = m, d, e, m * d + e, first.actions
        nblocks = first.desc.nblocks
        table = (A.hk_pvnet_block * (m * nblocks))()
        for t, p in enumerate(plans):
            for l in range(nblocks):
                table[t * nblocks + l] = p.desc.block[l]
        # (the copy is ordered with the stream that is current now, as every later launch on it is)
        self.table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        self.desc = q = A.hk_customnet_desc()
        q.towers = self.table.data_ptr()
        for name in ("policy_weight", "policy_bias", "value_weight", "value_bias"):
            setattr(q, name, getattr(first.desc, name))
        q.m, q.d, q.e, q.nblocks, q.n_last, q.actions, q.dtype = m, d, e, nblocks, first.n_last, first.actions, A.HK_F32
        self.workspace, self._retired = None, []
        # the gradients of customnet_backward (include/hironaka_hip_customgrad.h): `params` in module order -- tower after
        # tower, block after block (PvnetPlan.params' order inside a tower), then the policy head's and the value head's --
        # and where each one's gradient begins in ONE flat buffer of `grad_floats` floats.  The gradient table, parallel to
        # the tower table, holds those offsets; it is written here, once, and nobody can read it back: every offset is this
        # loop's, inside the buffer, and no two gradients share a float
        self.params, self.grad_starts, floats = [], [], 0
        gtable = (A.hk_customgrad_block * (m * nblocks))()
        for rec in gtable:
            for which in ("dense1", "dense2", "proj"):
                for field in ("d_weight", "d_bias", "d_gn_scale", "d_gn_bias"):
                    setattr(getattr(rec, which), field, A.HK_CUSTOMGRAD_NONE)
        self.grad_desc = g = A.hk_customgrad_desc()
        for head in (g.policy, g.value):
            for field in ("d_weight", "d_bias", "d_gn_scale", "d_gn_bias"):
                setattr(head, field, A.HK_CUSTOMGRAD_NONE)

        def place(param, record, field):
            nonlocal floats
            setattr(record, field, floats)
            self.params.append(param)
            self.grad_starts.append(floats)
            floats += (param.numel() + 3) & ~3

        for t, p in enumerate(plans):
            for param, (block, which, field) in zip(p.params, p.grad_fields):
                if which is not None:
                    place(param, getattr(gtable[t * nblocks + block], which), field)
        for param, (block, which, field) in zip(first.params, first.grad_fields):
            if which is None:
                place(param, getattr(g, block), field)
        self.grad_floats = floats
        self.grad_table = torch.frombuffer(bytearray(bytes(gtable)), dtype=torch.uint8).to(dev)
        g.grad_table, g.grad_floats = self.grad_table.data_ptr(), floats
        for l in range(nblocks):
            g.n[l], g.kind[l] = first.desc.block[l].n, first.desc.block[l].kind

    def workspace_for(self, batch: int) -> torch.Tensor:
        """the workspace for a call on `batch` rows, allocated (for twice the rows) and zeroed where the one at hand is
        too small -- not inside a graph capture: call this, or the forward, once before"""
        need = int(lib().hk_customnet_workspace_bytes(batch, self.m))
        if self.workspace is None or self.workspace.numel() * 8 < need:
            # room for twice the rows: a batch that grows a little does not allocate again.  A workspace that is replaced
            # stays alive with the plan: a captured graph may still point at it
            if self.workspace is not None:
                self._retired.append(self.workspace)
            words = (int(lib().hk_customnet_workspace_bytes(2 * batch, self.m)) + 15) // 16
            # (zeroed once: the library's counters at its head, which every call leaves zero)
            self.workspace = torch.zeros((words, 2), dtype=torch.int64, device=self.device)
        return self.workspace


def customnet_forward(x: torch.Tensor, plan: CustomnetPlan, tile: Optional[int] = None, raw_value: bool = False,
                      gate: Optional[Tuple[torch.Tensor, int]] = None,
                      out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """The forward of CustomNet in two launches (hk_customnet_forward; the rule, to the bit, is in
    include/hironaka_hip_customnet.h): the rows are grouped by their point count and every row runs the ONE tower its count
    names, then the heads.  x: [B, ...] float32 rows of m * d + e features (flattened behind the batch dimension; the rows
    may lie any number of elements apart -- a column slice of a wider buffer).  Returns (policy [B, A], value [B]).  out:
    (policy, value) to write into, as pvnet_forward's; tile, raw_value and gate as pvnet_forward's.  The plan's workspace
    is used by the call: calls on one plan belong on one stream.  Inside a graph capture a call must find the plan built and
    its workspace large enough: building a plan copies the table to the device and a batch that outgrows the workspace
    allocates and zeroes a new one, neither of which belongs in a capture -- make a call of the largest batch (or
    `plan.workspace_for(batch)`) before capturing, as the search loops' warm-up does.  That no TOWER parameter shares a
    byte with policy or value is not checked (the library checks x, the heads, the table and the workspace against them).
    Everything is float32 on one HIP device (a TypeError otherwise).  Nothing here synchronises."""
    if not isinstance(plan, CustomnetPlan):
        raise TypeError(f"plan must be a CustomnetPlan. Got {type(plan).__name__}.")
    policy, value = out if out is not None else (None, None)
    word, want = None, 0
    if gate is not None:
        word, want = gate
        _require_device(word, "gate[0]")
        if word.dtype != torch.int32 or word.numel() != 1 or word.device != plan.device:
            raise TypeError(f"gate[0] must be an int32 tensor of one element on {plan.device}. "
                            f"Got {word.dtype} {tuple(word.shape)} on {word.device}.")
    tile_flag = _mlp_tile_flag(tile)
    dev = plan.device
    x = _mlp_rows(x, "x", dev)
    batch, k = x.shape
    if k != plan.k_in:
        raise ValueError(f"the rows have {plan.k_in} features ({plan.m} points of {plan.d} and {plan.e} more). Got {k}.")
    _mlp_batch_limit(batch)
    a = plan.actions
    for name, given, shape in (("policy", policy, (batch, a)), ("value", value, (batch,))):
        if given is not None:
            _mlp_given_out(given, name, dev, shape)
    if policy is None:
        policy = torch.empty((batch, a), dtype=torch.float32, device=dev)
    if value is None:
        value = torch.empty((batch,), dtype=torch.float32, device=dev)
    if batch == 0:
        return policy, value
    workspace = plan.workspace_for(batch)
    q = plan.desc
    q.x, q.x_stride, q.batch = x.data_ptr(), x.stride(0) if batch > 1 else k, batch
    q.policy, q.policy_stride = policy.data_ptr(), policy.stride(0) if batch > 1 else a
    q.value, q.value_stride = value.data_ptr(), value.stride(0) if batch > 1 else 1
    q.workspace, q.workspace_bytes = workspace.data_ptr(), workspace.numel() * 8
    q.gate, q.want = (word.data_ptr(), int(want)) if word is not None else (None, 0)
    q.flags = tile_flag | (A.HK_CUSTOMNET_RAW_VALUE if raw_value else 0)
    with torch.cuda.device(dev):
        check(lib().hk_customnet_forward(C.byref(q), _stream(policy)), "hk_customnet_forward")
    return policy, value


# ---- one expansion of the role-agnostic search tree: kind of the batch, expansion, prior (hironaka_hip_unified.h) ----------

def _unified_array(t: torch.Tensor, name: str, dtype, shape, dev) -> int:
    _require_device(t, name)
    if t.dtype != dtype or t.device != dev or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}. "
                         f"Got {t.dtype} {tuple(t.shape)} on {t.device}.")
    return t.data_ptr()


def unified_expand(embeddings: torch.Tensor, parent: torch.Tensor, action: torch.Tensor, node: torch.Tensor,
                   kind: torch.Tensor, *, spec: Tuple[int, int], discount: float, scale_observation: bool = True,
                   reposition: bool = False, net_in: Optional[torch.Tensor] = None,
                   subset: Optional[torch.Tensor] = None, reward: Optional[torch.Tensor] = None,
                   discount_out: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """One expansion of a role-agnostic tree (hk_unified_expand; include/hironaka_hip_unified.h states the rule).
    embeddings: the contiguous float32 table [B, N, m*d + d], read at `parent` and written at `node` (both [B] int32);
    action: [B] int32; kind: an int32 tensor of one element that holds 0 -- it receives 1 when a parent is a host
    state.  Returns {"net_in": [B, m*d + d], "subset": [B] int32, "reward": [B], "discount": [B]} (the tensors given, or
    new ones).  Nothing here synchronises."""
    _require_device(embeddings, "embeddings")
    m, d = spec
    dev = embeddings.device
    if embeddings.dim() != 3 or embeddings.shape[2] != m * d + d:
        raise ValueError(f"embeddings must be [B, N, {m * d + d}]. Got {tuple(embeddings.shape)}.")
    b, n, w = embeddings.shape
    q = A.hk_unified_expand_desc()
    q.embeddings = _unified_array(embeddings, "embeddings", torch.float32, (b, n, w), dev)
    for name, t in (("parent", parent), ("action", action), ("node", node)):
        setattr(q, name, _unified_array(t, name, torch.int32, (b,), dev))
    _require_device(kind, "kind")
    if kind.dtype != torch.int32 or kind.numel() != 1 or kind.device != dev:
        raise ValueError(f"kind must be an int32 tensor of one element on {dev}.")
    q.kind = kind.data_ptr()
    res = {}
    for name, t, dtype, shape in (("net_in", net_in, torch.float32, (b, w)), ("subset", subset, torch.int32, (b,)),
                                  ("reward", reward, torch.float32, (b,)), ("discount", discount_out, torch.float32, (b,))):
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        setattr(q, "discount_out" if name == "discount" else name, _unified_array(t, name, dtype, shape, dev))
        res[name] = t
    q.discount = float(discount)
    q.batch, q.num_nodes, q.max_points, q.dim, q.dtype = b, n, m, d, A.HK_F32
    q.flags = (A.HK_UNIFIED_REPOSITION if reposition else 0) | (A.HK_UNIFIED_SCALE_OBSERVATION if scale_observation else 0)
    with torch.cuda.device(dev):
        check(lib().hk_unified_expand(C.byref(q), _stream(embeddings)), "hk_unified_expand")
    return res


def unified_prior(kind: torch.Tensor, agent_logits: torch.Tensor, agent_value: torch.Tensor, host_logits: torch.Tensor,
                  host_value: torch.Tensor, subset: torch.Tensor, *, dim: int, prior: Optional[torch.Tensor] = None,
                  value: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(prior [B, 2^dim - dim - 1], value [B]) of the node a role-agnostic expansion made (hk_unified_prior): where `kind`
    holds 1 the agent's logits behind the bits of `subset`, padded with -inf, and the agent's value; where it holds 0
    the host's.  The side that is not selected is not read.  Nothing here synchronises."""
    _require_device(agent_logits, "agent_logits")
    dev = agent_logits.device
    b = agent_logits.shape[0]
    a = 2 ** dim - dim - 1
    if prior is None:
        prior = torch.empty((b, a), dtype=torch.float32, device=dev)
    if value is None:
        value = torch.empty((b,), dtype=torch.float32, device=dev)
    _require_device(kind, "kind")
    if kind.dtype != torch.int32 or kind.numel() != 1 or kind.device != dev:
        raise ValueError(f"kind must be an int32 tensor of one element on {dev}.")
    ptrs = [_unified_array(t, name, dtype, shape, dev) for name, t, dtype, shape in (
        ("agent_logits", agent_logits, torch.float32, (b, dim)), ("agent_value", agent_value, torch.float32, (b,)),
        ("host_logits", host_logits, torch.float32, (b, a)), ("host_value", host_value, torch.float32, (b,)),
        ("subset", subset, torch.int32, (b,)), ("prior", prior, torch.float32, (b, a)),
        ("value", value, torch.float32, (b,)))]
    with torch.cuda.device(dev):
        check(lib().hk_unified_prior(kind.data_ptr(), *ptrs, b, dim, _stream(prior)), "hk_unified_prior")
    return prior, value


# ---- the training-mode forward of a create_mlp stack and its backward, one launch per layer each way ---------------------

MlpTrainLayer = collections.namedtuple(
    "MlpTrainLayer", "weight bias bn_mean bn_var bn_weight bn_bias eps relu momentum num_batches_tracked",
    defaults=(None, None, None, None, None, 1e-5, False, 0.1, None))
MlpTrainLayer.__doc__ = """One `Linear [-> BatchNorm1d (training)] [-> ReLU]` block of mlp_train_forward: MlpLayer's
fields, where bn_mean / bn_var are the running statistics the forward UPDATES (both None: no batch norm), then the batch
norm's momentum (a float) and its num_batches_tracked (a 0-dim int64 tensor the forward increments, or None)."""


def _align4(n: int) -> int:
    return (n + 3) & ~3


class MlpTrainPlan(_MlpTable):
    """The layer table of mlp_train_forward / mlp_backward, built once per set of parameter addresses (it holds the
    tensors alive).  `params` lists the parameters in module order -- per layer weight, bias, bn_weight, bn_bias, those
    that exist -- which is the order of mlp_backward's gradients."""
    LAYER, DESC, STATS = MlpTrainLayer, A.hk_mlp_train_desc, ("running_mean", "running_var")

    def __init__(self, layers: Sequence[MlpTrainLayer], input_relu: bool = False):
        self.params, self.shapes, self.bn = [], [], []
        self._fill(layers, input_relu)
        self.widest = max([n for n, *_ in self.shapes[1:]], default=0)
        # the gradients of one backward, in floats from the start of its buffer: (d_weight, d_bias, d_bn_weight, d_bn_bias)
        self.grad_at, at = [], 0
        for n, k, bias, gamma, beta in self.shapes:
            row = [at]
            at += _align4(n * k)
            for present in (bias, gamma, beta):
                row.append(at if present else None)
                at += _align4(n) if present else 0
            self.grad_at.append(row)
        self.grad_floats = at
        self._saved_at = {}

    def _own(self, i: int, l, e, bn: bool):
        if bn and not isinstance(l.momentum, float):
            raise TypeError(f"layers[{i}]: momentum must be a float. Got {l.momentum!r}.")
        nbt = l.num_batches_tracked
        if nbt is not None:
            _require_device(nbt, f"layers[{i}].num_batches_tracked")
            if nbt.dtype != torch.int64 or nbt.numel() != 1 or nbt.device != self.device:
                raise TypeError(f"layers[{i}].num_batches_tracked must be one int64 on {self.device}.")
            e.num_batches_tracked = nbt.data_ptr()
            self.tensors.append(nbt)
        e.momentum = float(l.momentum) if bn else 0.0
        e.flags |= A.HK_MLP_TRAIN_BN if bn else 0
        n, k = l.weight.shape
        self.params += [t for t in (l.weight, l.bias, l.bn_weight, l.bn_bias) if t is not None]
        self.shapes.append((n, k, l.bias is not None, l.bn_weight is not None, l.bn_bias is not None))
        self.bn.append(bn)

    def saved_at(self, batch: int):
        """where one forward's saved tensors lie, in floats from the start of its buffer: per layer (act, z, mean, inv),
        and the buffer's length.  The last layer's act is a tensor of its own (the result)."""
        got = self._saved_at.get(batch)
        if got is None:
            rows, at = [], 0
            for i, ((n, *_), bn) in enumerate(zip(self.shapes, self.bn)):
                row = [None] * 4
                if i + 1 < len(self.shapes):
                    row[0], at = at, at + _align4(batch * n)
                if bn:
                    row[1], at = at, at + _align4(batch * n)
                    row[2], at = at, at + _align4(n)
                    row[3], at = at, at + _align4(n)
                rows.append(row)
            got = self._saved_at[batch] = (rows, at)
        return got


class MlpTrainSaved:
    """what mlp_backward needs of one mlp_train_forward: the plan, the inputs, the result and the buffer that holds
    every layer's act, z, mean and inv"""

    def __init__(self, plan, x0, x1, out, buf):
        self.plan, self.x0, self.x1, self.out, self.buf = plan, x0, x1, out, buf

    def layer(self, i: int):
        """(act, z, mean, inv) of layer i as tensors (None where the layer has none)"""
        rows, _ = self.plan.saved_at(self.out.shape[0])
        n, batch = self.plan.shapes[i][0], self.out.shape[0]
        act, z, mean, inv = rows[i]
        view = lambda at, *shape: None if at is None else self.buf[at:at + math.prod(shape)].view(*shape)  # noqa: E731
        return (self.out if act is None else view(act, batch, n), view(z, batch, n), view(mean, n), view(inv, n))


def _mlp_train_fill(plan: MlpTrainPlan, x0, x1, out, buf):
    """the descriptor's fields that belong to one call"""
    d = plan.desc
    _mlp_fill_inputs(d, x0, x1)
    d.grad_out, d.workspace, d.workspace_bytes = None, None, 0
    rows, _ = plan.saved_at(x0.shape[0])
    base = buf.data_ptr()
    for i, (act, z, mean, inv) in enumerate(rows):
        e = d.layer[i]
        e.act = out.data_ptr() if act is None else base + 4 * act
        if z is not None:
            e.z, e.mean, e.inv = base + 4 * z, base + 4 * mean, base + 4 * inv


def mlp_train_forward(x0: torch.Tensor, plan, x1: Optional[torch.Tensor] = None, input_relu: bool = False):
    """The training-mode forward of `Linear [-> BatchNorm1d] [-> ReLU]` blocks, one launch per layer
    (hk_train_mlp_forward; the rule, to the bit, is in include/hironaka_hip_mlp_train.h): batch statistics, the running
    statistics and num_batches_tracked updated in place.  `plan`: an MlpTrainPlan, or a sequence of MlpTrainLayer (with
    input_relu).  Row b of the input is x0[b] flattened, followed by x1[b] flattened if x1 is given.  Returns (out [B, n],
    saved): `saved` (an MlpTrainSaved) is what mlp_backward takes.  The buffers are new per call, so a plan may run
    forward any number of times before a backward.  At most HK_MLP_TRAIN_MAX_BATCH rows, at least 2 with a batch norm.
    Nothing here synchronises."""
    if not isinstance(plan, MlpTrainPlan):
        plan = MlpTrainPlan(plan, input_relu)
    dev = plan.device
    x0, x1 = _mlp_inputs(plan, x0, x1)
    batch = x0.shape[0]
    if batch > A.HK_MLP_TRAIN_MAX_BATCH or (batch == 1 and any(plan.bn)):
        raise ValueError(f"2 to {A.HK_MLP_TRAIN_MAX_BATCH} rows with a batch norm, 0 to {A.HK_MLP_TRAIN_MAX_BATCH} "
                         f"without. Got {batch}.")
    out = torch.empty((batch, plan.n_out), dtype=torch.float32, device=dev)
    buf = torch.empty(plan.saved_at(batch)[1], dtype=torch.float32, device=dev)
    # (an alias without autograd's marks: where `out` becomes the result of an autograd.Function whose context holds
    # `saved`, holding `out` itself would tie the graph into a cycle that only the garbage collector ends)
    saved = MlpTrainSaved(plan, x0, x1, out.detach(), buf)
    if batch == 0:
        return out, saved
    _mlp_train_fill(plan, x0, x1, out, buf)
    with torch.cuda.device(dev):
        check(lib().hk_train_mlp_forward(C.byref(plan.desc), _stream(out)), "hk_train_mlp_forward")
    return out, saved


def mlp_backward(saved: MlpTrainSaved, grad_out: torch.Tensor, grads: Optional[Sequence[torch.Tensor]] = None):
    """The backward of one mlp_train_forward, one launch per layer (hk_train_mlp_backward): grad_out [B, n] is the
    gradient with respect to the forward's result; returns the gradients of the plan's `params`, in that order (new
    tensors, views of one buffer).  grads: contiguous float32 tensors of the parameters' shapes, in that order, to write
    the gradients into instead (views of one flat buffer, say: any 4-byte boundary will do); they are what is returned.
    The input gets none.  The parameters must be what they were in the forward.  Nothing here synchronises."""
    plan, out = saved.plan, saved.out
    dev = plan.device
    _require_device(grad_out, "grad_out")
    if grad_out.dtype != torch.float32 or grad_out.device != dev or tuple(grad_out.shape) != tuple(out.shape):
        raise TypeError(f"grad_out must be a float32 tensor of shape {tuple(out.shape)} on {dev}. "
                        f"Got {grad_out.dtype} {tuple(grad_out.shape)} on {grad_out.device}.")
    batch = out.shape[0]
    if plan.n_out > 1 and grad_out.stride(1) != 1:
        grad_out = grad_out.contiguous()
    ws_floats = 2 * batch * plan.widest
    if grads is not None:
        grads = list(grads)
        if len(grads) != len(plan.params):
            raise ValueError(f"grads must hold one tensor per parameter ({len(plan.params)}). Got {len(grads)}.")
        at = [_mlp_tensor(g, f"grads[{i}]", dev, p.shape) for i, (g, p) in enumerate(zip(grads, plan.params))]
        buf, ws_at, rows, given = torch.empty(ws_floats, dtype=torch.float32, device=dev), 0, [], iter(at)
        for n, k, bias, gamma, beta in plan.shapes:
            rows.append([next(given)] + [next(given) if present else None for present in (bias, gamma, beta)])
    else:
        buf, ws_at = torch.empty(plan.grad_floats + ws_floats, dtype=torch.float32, device=dev), plan.grad_floats
        base = buf.data_ptr()
        rows = [[None if at is None else base + 4 * at for at in row] for row in plan.grad_at]
        grads = []
        for (n, k, *_), (w, b, g, be) in zip(plan.shapes, plan.grad_at):
            grads.append(buf[w:w + n * k].view(n, k))
            grads += [buf[at:at + n] for at in (b, g, be) if at is not None]
    if batch == 0:
        for g in ([buf[:plan.grad_floats]] if ws_at else grads):  # (ws_at == 0: the caller's tensors)
            g.zero_()
        return grads
    _mlp_train_fill(plan, saved.x0, saved.x1, out, saved.buf)
    d = plan.desc
    d.grad_out, d.grad_stride = grad_out.data_ptr(), grad_out.stride(0) if batch > 1 else plan.n_out
    d.workspace, d.workspace_bytes = (buf.data_ptr() + 4 * ws_at, 4 * ws_floats) if ws_floats else (None, 0)
    for i, row in enumerate(rows):
        e = d.layer[i]
        e.d_weight, e.d_bias, e.d_bn_weight, e.d_bn_bias = row
    with torch.cuda.device(dev):
        check(lib().hk_train_mlp_backward(C.byref(d), _stream(out)), "hk_train_mlp_backward")
    return grads


# ---- the training-mode forward of a DenseResNet / DenseNet policy-value network and its backward -------------------------

class PvnetSaved:
    """what pvnet_backward needs of one pvnet_train_forward: the plan, the input rows, the results (value as the kernel
    stored it) and the workspace that holds every block's saved arrays"""

    def __init__(self, plan, x, policy, value, workspace, raw_value):
        self.plan, self.x, self.policy, self.value, self.workspace, self.raw_value = plan, x, policy, value, workspace, raw_value


def _pvgrad_desc(plan: PvnetPlan, x, policy, value, workspace, raw_value: bool):
    """the plan's hk_pvgrad_desc with the fields of one call filled in"""
    g = plan.__dict__.get("_grad_desc")
    if g is None:
        g = plan.__dict__["_grad_desc"] = A.hk_pvgrad_desc()
    batch, k0, a = x.shape[0], x.shape[1], plan.actions
    g.net = plan.desc
    d = g.net
    d.x, d.x_stride, d.k0, d.batch = x.data_ptr(), x.stride(0) if batch > 1 else k0, k0, batch
    d.policy, d.policy_stride = policy.data_ptr(), policy.stride(0) if batch > 1 else a
    d.value, d.value_stride = value.data_ptr(), value.stride(0) if batch > 1 else 1
    d.flags = A.HK_PVNET_RAW_VALUE if raw_value else 0
    g.workspace, g.workspace_bytes = workspace.data_ptr(), 4 * workspace.numel()
    g.grad_policy = g.grad_value = None
    return g


def pvnet_train_forward(x: torch.Tensor, plan: PvnetPlan, raw_value: bool = False):
    """pvnet_forward with what the backward needs saved, in one launch (hk_pvgrad_forward; the rule is in
    include/hironaka_hip_pvgrad.h).  Returns (policy [B, A], value [B], saved): policy and value have pvnet_forward's bits,
    `saved` (a PvnetSaved) is what pvnet_backward takes.  The buffers are new per call.  At most HK_PVGRAD_MAX_BATCH rows.
    Nothing here synchronises."""
    if not isinstance(plan, PvnetPlan):
        raise TypeError(f"plan must be a PvnetPlan. Got {type(plan).__name__}.")
    dev = plan.device
    x = _mlp_rows(x, "x", dev)
    batch, k0 = x.shape
    if k0 != plan.k_in:
        raise ValueError(f"the first block takes {plan.k_in} inputs. Got {k0}.")
    if batch > A.HK_PVGRAD_MAX_BATCH:
        raise ValueError(f"at most {A.HK_PVGRAD_MAX_BATCH} rows. Got {batch}.")
    policy = torch.empty((batch, plan.actions), dtype=torch.float32, device=dev)
    value = torch.empty((batch,), dtype=torch.float32, device=dev)
    g = _pvgrad_desc(plan, x, policy, value, policy, raw_value)
    g.workspace, g.workspace_bytes = None, 0
    floats = lib().hk_pvgrad_workspace_bytes(C.byref(g)) // 4 if batch else 0
    workspace = torch.empty(max(floats, 1), dtype=torch.float32, device=dev)
    # (aliases without autograd's marks: see mlp_train_forward)
    saved = PvnetSaved(plan, x, policy.detach(), value.detach(), workspace, bool(raw_value))
    if batch == 0:
        return policy, value, saved
    g.workspace, g.workspace_bytes = workspace.data_ptr(), 4 * workspace.numel()
    with torch.cuda.device(dev):
        check(lib().hk_pvgrad_forward(C.byref(g), _stream(policy)), "hk_pvgrad_forward")
    return policy, value, saved


def pvnet_backward(saved: PvnetSaved, grad_policy: torch.Tensor, grad_value: torch.Tensor,
                   grads: Optional[Sequence[torch.Tensor]] = None):
    """The backward of one pvnet_train_forward (hk_pvgrad_backward: one launch for the rows, one per HK_PVGRAD_TABLE Denses
    for the parameters): grad_policy [B, A] and grad_value [B] or [B, 1] are the gradients with respect to the forward's
    policy and value (the tanh's result, or the raw value where the forward ran with raw_value); their rows may lie any
    number of elements apart.  Returns the gradients of the plan's `params`, in that order (new tensors, views of one
    buffer).  grads: contiguous float32 tensors of the parameters' shapes, in that order, to write into instead.  The input
    gets none.  The parameters must be what they were in the forward.  Nothing here synchronises."""
    plan = saved.plan
    dev = plan.device
    batch, a = saved.policy.shape
    for name, t, shapes in (("grad_policy", grad_policy, ((batch, a),)), ("grad_value", grad_value, ((batch,), (batch, 1)))):
        _require_device(t, name)
        if t.dtype != torch.float32 or t.device != dev or tuple(t.shape) not in shapes:
            raise TypeError(f"{name} must be a float32 tensor of shape {' or '.join(map(str, shapes))} on {dev}. "
                            f"Got {t.dtype} {tuple(t.shape)} on {t.device}.")
    if (a > 1 and grad_policy.stride(1) != 1) or (batch > 1 and grad_policy.stride(0) < a):
        grad_policy = grad_policy.contiguous()
    if batch > 1 and grad_value.stride(0) < 1:
        grad_value = grad_value.contiguous()
    if grads is not None:
        grads = list(grads)
        if len(grads) != len(plan.params):
            raise ValueError(f"grads must hold one tensor per parameter ({len(plan.params)}). Got {len(grads)}.")
        at = [_mlp_tensor(t, f"grads[{i}]", dev, p.shape) for i, (t, p) in enumerate(zip(grads, plan.params))]
    else:
        starts, floats = [], 0
        for p in plan.params:
            starts.append(floats)
            floats += _align4(p.numel())
        buf = torch.empty(floats, dtype=torch.float32, device=dev)
        grads = [buf[s:s + p.numel()].view(p.shape) for s, p in zip(starts, plan.params)]
        at = [buf.data_ptr() + 4 * s for s in starts]
    if batch == 0:
        for t in grads:
            t.zero_()
        return grads
    g = _pvgrad_desc(plan, saved.x, saved.policy, saved.value, saved.workspace, saved.raw_value)
    g.grad_policy, g.grad_policy_stride = grad_policy.data_ptr(), grad_policy.stride(0) if batch > 1 else a
    g.grad_value, g.grad_value_stride = grad_value.data_ptr(), grad_value.stride(0) if batch > 1 else 1
    for (block, which, field), ptr in zip(plan.grad_fields, at):
        setattr(getattr(g, block) if which is None else getattr(g.block[block], which), field, ptr)
    with torch.cuda.device(dev):
        check(lib().hk_pvgrad_backward(C.byref(g), _stream(saved.policy)), "hk_pvgrad_backward")
    return grads


# ---- the training-mode forward of CustomNet and its backward: one tower per row both ways (hironaka_hip_customgrad.h) -------

class CustomnetSaved:
    """what customnet_backward needs of one customnet_train_forward: the plan, the input rows, the results (value as the
    kernel stored it) and the workspace that holds the grouping and every saved array"""

    def __init__(self, plan, x, policy, value, workspace, raw_value):
        self.plan, self.x, self.policy, self.value, self.workspace, self.raw_value = plan, x, policy, value, workspace, raw_value


def _customgrad_desc(plan: CustomnetPlan, x, policy, value, workspace, raw_value: bool):
    """the plan's hk_customgrad_desc with the fields of one call filled in"""
    g = plan.grad_desc
    batch, k, a = x.shape[0], x.shape[1], plan.actions
    g.net = plan.desc
    q = g.net
    q.x, q.x_stride, q.batch = x.data_ptr(), x.stride(0) if batch > 1 else k, batch
    q.policy, q.policy_stride = policy.data_ptr(), policy.stride(0) if batch > 1 else a
    q.value, q.value_stride = value.data_ptr(), value.stride(0) if batch > 1 else 1
    q.gate, q.want = None, 0
    q.flags = A.HK_CUSTOMNET_RAW_VALUE if raw_value else 0
    q.workspace, q.workspace_bytes = (workspace.data_ptr(), 4 * workspace.numel()) if workspace is not None else (None, 0)
    g.grads = g.grad_policy = g.grad_value = None
    return g


def customnet_train_forward(x: torch.Tensor, plan: CustomnetPlan, raw_value: bool = False):
    """customnet_forward with what the backward needs saved, in two launches (hk_customgrad_forward; the rule is in
    include/hironaka_hip_customgrad.h): a stable grouping of the rows by their point count, then every row through the ONE
    tower its count names.  Returns (policy [B, A], value [B], saved): policy and value have customnet_forward's bits,
    `saved` (a CustomnetSaved) is what customnet_backward takes.  The buffers are new per call (the plan's workspace is
    not used).  At most HK_PVGRAD_MAX_BATCH rows.  Nothing here synchronises."""
    if not isinstance(plan, CustomnetPlan):
        raise TypeError(f"plan must be a CustomnetPlan. Got {type(plan).__name__}.")
    dev = plan.device
    x = _mlp_rows(x, "x", dev)
    batch, k = x.shape
    if k != plan.k_in:
        raise ValueError(f"the rows have {plan.k_in} features ({plan.m} points of {plan.d} and {plan.e} more). Got {k}.")
    if batch > A.HK_PVGRAD_MAX_BATCH:
        raise ValueError(f"at most {A.HK_PVGRAD_MAX_BATCH} rows. Got {batch}.")
    policy = torch.empty((batch, plan.actions), dtype=torch.float32, device=dev)
    value = torch.empty((batch,), dtype=torch.float32, device=dev)
    g = _customgrad_desc(plan, x, policy, value, None, raw_value)
    floats = lib().hk_customgrad_workspace_bytes(C.byref(g)) // 4 if batch else 0
    workspace = torch.empty(max(floats, 4), dtype=torch.float32, device=dev)
    # (aliases without autograd's marks: see mlp_train_forward)
    saved = CustomnetSaved(plan, x, policy.detach(), value.detach(), workspace, bool(raw_value))
    if batch == 0:
        return policy, value, saved
    g.net.workspace, g.net.workspace_bytes = workspace.data_ptr(), 4 * workspace.numel()
    with torch.cuda.device(dev):
        check(lib().hk_customgrad_forward(C.byref(g), _stream(policy)), "hk_customgrad_forward")
    return policy, value, saved


def customnet_backward(saved: CustomnetSaved, grad_policy: torch.Tensor, grad_value: torch.Tensor,
                       out: Optional[torch.Tensor] = None):
    """The backward of one customnet_train_forward in two launches (hk_customgrad_backward: the row chain, then the
    parameter gradients of every tower over its own rows and of the heads over all): grad_policy [B, A] and grad_value [B]
    or [B, 1] are the gradients with respect to the forward's policy and value (the tanh's result, or the raw value where
    the forward ran with raw_value); their rows may lie any number of elements apart.  Returns the gradients of the plan's
    `params`, in that order: views of ONE flat float32 buffer of `plan.grad_floats` floats -- `out`, where it is given (a
    contiguous float32 tensor of that many elements on the device), a new one otherwise.  A tower that saw no row gets
    zeros.  The input gets no gradient.  The parameters must be what they were in the forward.  Nothing here
    synchronises."""
    if not isinstance(saved, CustomnetSaved):
        raise TypeError(f"saved must be a CustomnetSaved. Got {type(saved).__name__}.")
    plan = saved.plan
    dev = plan.device
    batch, a = saved.policy.shape
    for name, t, shapes in (("grad_policy", grad_policy, ((batch, a),)), ("grad_value", grad_value, ((batch,), (batch, 1)))):
        _require_device(t, name)
        if t.dtype != torch.float32 or t.device != dev or tuple(t.shape) not in shapes:
            raise TypeError(f"{name} must be a float32 tensor of shape {' or '.join(map(str, shapes))} on {dev}. "
                            f"Got {t.dtype} {tuple(t.shape)} on {t.device}.")
    if (a > 1 and grad_policy.stride(1) != 1) or (batch > 1 and grad_policy.stride(0) < a):
        grad_policy = grad_policy.contiguous()
    if batch > 1 and grad_value.stride(0) < 1:
        grad_value = grad_value.contiguous()
    if out is not None:
        _require_device(out, "out")
        if out.dtype != torch.float32 or out.device != dev:
            raise TypeError(f"out must be a float32 tensor on {dev}. Got {out.dtype} on {out.device}.")
        if out.dim() != 1 or out.numel() != plan.grad_floats or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous tensor of {plan.grad_floats} floats. Got {tuple(out.shape)}.")
        buf = out
    else:
        buf = torch.empty(plan.grad_floats, dtype=torch.float32, device=dev)
    grads = [buf[s:s + p.numel()].view(p.shape) for s, p in zip(plan.grad_starts, plan.params)]
    if batch == 0:
        buf.zero_()
        return grads
    g = _customgrad_desc(plan, saved.x, saved.policy, saved.value, saved.workspace, saved.raw_value)
    g.grads = buf.data_ptr()
    g.grad_policy, g.grad_policy_stride = grad_policy.data_ptr(), grad_policy.stride(0) if batch > 1 else a
    g.grad_value, g.grad_value_stride = grad_value.data_ptr(), grad_value.stride(0) if batch > 1 else 1
    with torch.cuda.device(dev):
        check(lib().hk_customgrad_backward(C.byref(g), _stream(saved.policy)), "hk_customgrad_backward")
    return grads
