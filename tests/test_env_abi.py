"""CPU-side checks of hk_env_step's boundary (include/hironaka_hip_env.h): the library exports it, the python mirror of
the header agrees with it, and bad arguments are refused on the host, before any launch."""
import ctypes
import re

import abi_cases
from hironaka_amd import _abi as A
from hironaka_amd import _lib


def _header():
    return abi_cases.header("hironaka_hip_env.h")


def test_library_exports_hk_env_step():
    _lib.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    declared = abi_cases.declared("hironaka_hip_env.h")
    assert declared == set(A.ENV_PROTOTYPES) == {"hk_env_step"}
    for name in declared:
        assert hasattr(handle, name), name
    assert not declared & set(A.PROTOTYPES)
    assert '#include "hironaka_hip_env.h"' in abi_cases.header()
    assert _lib.lib().hk_abi_version() == A.HK_ABI_VERSION == 6


def test_env_constants_match_header():
    found = re.findall(r"#define\s+(HK_ENV_\w+)\s+\(?(-?\d+)u?\)?\s", _header())
    assert len(found) == 10
    for name, value in found:
        assert getattr(A, name) == int(value), name


def test_env_descriptor_layout_matches_c(tmp_path):
    """sizeof/offsetof as the C compiler sees them (gcc on the header) == ctypes"""
    abi_cases.assert_layouts_match_c({"hk_env_step_desc": A.hk_env_step_desc}, tmp_path)


def _desc(**over):
    """a descriptor that passes every check up to the launch, but for what `over` changes"""
    buf = (ctypes.c_double * 64)()
    at = ctypes.addressof(buf)
    q = A.hk_env_step_desc()
    for name in ("points_in", "points_out", "class_io", "step_count", "episode", "action", "reward", "stopped",
                 "obs_points", "obs_coords"):
        setattr(q, name, at)
    q.batch, q.max_points, q.dim, q.dtype = 4, 5, 3, A.HK_F64
    q.mode, q.host, q.agent, q.max_value = A.HK_ENV_MODE_HOST, A.HK_HOST_ZEILLINGER, A.HK_AGENT_CHOOSE_FIRST, 10
    q.flags = A.HK_ENV_AUTO_RESET | A.HK_ENV_SCALE_OBSERVATION
    for name, v in over.items():
        setattr(q, name, v)
    q._keep = buf
    return q


def test_env_step_validation_without_gpu():
    L = _lib.lib()
    call = lambda **over: L.hk_env_step(ctypes.byref(_desc(**over)), None)  # noqa: E731
    assert L.hk_env_step(None, None) == A.HK_ERR_NULL
    assert call(batch=0) == A.HK_OK  # a valid descriptor, nothing to do
    assert call(dim=1) == A.HK_ERR_SHAPE
    assert call(dim=8) == A.HK_ERR_UNSUPPORTED
    assert call(max_points=0) == A.HK_ERR_SHAPE
    assert call(max_points=65) == A.HK_ERR_UNSUPPORTED
    assert call(batch=-1) == A.HK_ERR_SHAPE
    assert call(points_in=None) == A.HK_ERR_NULL
    assert call(points_out=None) == A.HK_ERR_NULL
    assert call(mode=2) == A.HK_ERR_UNSUPPORTED
    assert call(mode=-1) == A.HK_ERR_UNSUPPORTED
    for host in (A.HK_HOST_RANDOM, 6, -1):
        assert call(host=host) == A.HK_ERR_UNSUPPORTED, host
    for agent in (A.HK_AGENT_RANDOM, A.HK_AGENT_CHOOSE_LAST, 4, -1):
        assert call(mode=A.HK_ENV_MODE_AGENT, agent=agent) == A.HK_ERR_UNSUPPORTED, agent
    assert call(dtype=A.HK_I32) == A.HK_ERR_UNSUPPORTED
    assert call(flags=256) == A.HK_ERR_UNSUPPORTED
    assert call(max_value=0) == A.HK_ERR_SHAPE  # a reset needs something to draw from
    assert call(max_value=0, flags=0, batch=0) == A.HK_OK
    for name in ("step_count", "episode", "action", "reward", "stopped", "obs_points", "class_io", "obs_coords"):
        assert call(**{name: None}) == A.HK_ERR_NULL, name
    # agent mode has no use for the host's buffers; RESET_ALL none for the state coming in and the actions
    agent = dict(mode=A.HK_ENV_MODE_AGENT, class_io=None, obs_coords=None, host=0)
    assert call(batch=0, **agent) == A.HK_OK
    assert call(step_count=None, **agent) == A.HK_ERR_NULL
    # points_in and points_out that overlap without being equal
    q = _desc()
    q.points_out = q.points_in + 8
    assert L.hk_env_step(ctypes.byref(q), None) == A.HK_ERR_SHAPE
    q = _desc()
    q.points_in = q.points_out + 8  # the input starts inside the output's span
    assert L.hk_env_step(ctypes.byref(q), None) == A.HK_ERR_SHAPE
    for dtype, off in ((A.HK_F64, 4), (A.HK_F32, 2)):  # a pointer misaligned for its type
        q = _desc(dtype=dtype)
        q.points_in = q.points_out = q.points_in + off
        assert L.hk_env_step(ctypes.byref(q), None) == A.HK_ERR_ALIGN
    q = _desc()
    q.step_count = q.step_count + 2
    assert L.hk_env_step(ctypes.byref(q), None) == A.HK_ERR_ALIGN
