"""CPU-side checks of the boundary of hk_dqn_host_move / hk_dqn_agent_move (include/hironaka_hip_dqn_move.h): the
library exports them, the python mirror of the header agrees with it, and bad arguments are refused on the host, before
any launch."""
import ctypes
import os
import re

import abi_cases
from hironaka_amd import _abi as A
from hironaka_amd import _lib

HEADER = "hironaka_hip_dqn_move.h"


def test_library_exports_the_entry_points():
    _lib.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    declared = abi_cases.declared(HEADER)
    assert declared == set(A.DQN_MOVE_PROTOTYPES) == {"hk_dqn_host_move", "hk_dqn_agent_move"}
    for name in declared:
        assert hasattr(handle, name), name
        assert getattr(_lib.lib(), name).argtypes == A.DQN_MOVE_PROTOTYPES[name][1], name
    assert not declared & set(A.PROTOTYPES)
    assert '#include "%s"' % HEADER in abi_cases.header()
    assert _lib.lib().hk_abi_version() == A.HK_ABI_VERSION == 6
    with open(os.path.join(_lib.CSRC, "Makefile")) as f:
        assert re.search(r"^SINGLES :=.*\bdqn_move\b", f.read(), flags=re.M)


def test_constants_match_header():
    found = re.findall(r"#define\s+(HK_DQN_MOVE_\w+)\s+\(?(-?\d+)u?\)?\s", abi_cases.header(HEADER))
    assert len(found) == 2
    for name, value in found:
        assert getattr(A, name) == int(value), name


def test_descriptor_layouts_match_c(tmp_path):
    """sizeof/offsetof as the C compiler sees them (gcc on the header) == ctypes"""
    abi_cases.assert_layouts_match_c({"hk_dqn_host_move_desc": A.hk_dqn_host_move_desc,
                                      "hk_dqn_agent_move_desc": A.hk_dqn_agent_move_desc}, tmp_path)


def _buffers(count=8):
    """`count` disjoint 4 KiB host ranges, 8-byte aligned"""
    buf = (ctypes.c_double * (512 * count))()
    return buf, [ctypes.addressof(buf) + 4096 * i for i in range(count)]


def _host_desc(**over):
    """a descriptor that passes every check up to the launch, but for what `over` changes"""
    buf, at = _buffers()
    q = A.hk_dqn_host_move_desc()
    q.q, q.class_out, q.coords_out, q.prev_done, q.counts = at[:5]
    q.batch, q.dim, q.q_dtype, q.coords_dtype, q.q_stride = 4, 3, A.HK_F32, A.HK_F64, 4
    for name, v in over.items():
        setattr(q, name, v)
    q._keep = buf
    return q


def _agent_desc(**over):
    buf, at = _buffers()
    q = A.hk_dqn_agent_move_desc()
    q.points, q.q, q.class_id, q.axis_out, q.features_out, q.done_out, q.lengths, q.counts = at
    q.batch, q.max_points, q.dim, q.dtype, q.q_dtype, q.q_stride = 4, 5, 3, A.HK_F64, A.HK_F32, 3
    q.padding_value, q.flags = -1.0, A.HK_DQN_MOVE_MASKED | A.HK_DQN_MOVE_RESCALE
    for name, v in over.items():
        setattr(q, name, v)
    q._keep = buf
    return q


def test_host_move_validation_without_gpu():
    L = _lib.lib()
    call = lambda **over: L.hk_dqn_host_move(ctypes.byref(_host_desc(**over)), None)  # noqa: E731
    assert L.hk_dqn_host_move(None, None) == A.HK_ERR_NULL
    assert call(batch=0) == A.HK_OK  # a valid descriptor, nothing to do
    assert call(batch=-1) == A.HK_ERR_SHAPE
    assert call(dim=1) == A.HK_ERR_SHAPE
    assert call(dim=8) == A.HK_ERR_UNSUPPORTED
    assert call(q_stride=3) == A.HK_ERR_SHAPE  # rows of 4 classes would overlap
    for name in ("q_dtype", "coords_dtype"):
        for dtype in (A.HK_I32, A.HK_U8, -1):
            assert call(**{name: dtype}) == A.HK_ERR_UNSUPPORTED, (name, dtype)
    for name in ("q", "class_out", "coords_out"):
        assert call(**{name: None}) == A.HK_ERR_NULL, name
    assert call(batch=0, prev_done=None, counts=None) == A.HK_OK
    q = _host_desc()
    q.coords_out = q.coords_out + 4  # a double off its alignment
    assert L.hk_dqn_host_move(ctypes.byref(q), None) == A.HK_ERR_ALIGN
    q = _host_desc()
    q.class_out = q.class_out + 2
    assert L.hk_dqn_host_move(ctypes.byref(q), None) == A.HK_ERR_ALIGN
    q = _host_desc()
    q.class_out = q.q + 8  # an output inside the Q-values
    assert L.hk_dqn_host_move(ctypes.byref(q), None) == A.HK_ERR_SHAPE
    q = _host_desc()
    q.counts = q.class_out + 4  # two outputs that meet
    assert L.hk_dqn_host_move(ctypes.byref(q), None) == A.HK_ERR_SHAPE


def test_agent_move_validation_without_gpu():
    L = _lib.lib()
    call = lambda **over: L.hk_dqn_agent_move(ctypes.byref(_agent_desc(**over)), None)  # noqa: E731
    assert L.hk_dqn_agent_move(None, None) == A.HK_ERR_NULL
    assert call(batch=0) == A.HK_OK
    assert call(batch=-1) == A.HK_ERR_SHAPE
    assert call(dim=1) == A.HK_ERR_SHAPE
    assert call(dim=8) == A.HK_ERR_UNSUPPORTED
    assert call(max_points=0) == A.HK_ERR_SHAPE
    assert call(max_points=65) == A.HK_ERR_UNSUPPORTED
    assert call(q_stride=2) == A.HK_ERR_SHAPE
    assert call(flags=4) == A.HK_ERR_UNSUPPORTED
    for pad in (0.0, 1.0, float("nan")):
        assert call(padding_value=pad) == A.HK_ERR_UNSUPPORTED, pad
    for name in ("dtype", "q_dtype"):
        for dtype in (A.HK_I32, A.HK_U8, -1):
            assert call(**{name: dtype}) == A.HK_ERR_UNSUPPORTED, (name, dtype)
    for name in ("points", "q", "class_id", "axis_out", "features_out", "done_out", "lengths"):
        assert call(**{name: None}) == A.HK_ERR_NULL, name
    assert call(batch=0, counts=None) == A.HK_OK
    q = _agent_desc()
    q.points = q.points + 4
    assert L.hk_dqn_agent_move(ctypes.byref(q), None) == A.HK_ERR_ALIGN
    q = _agent_desc()
    q.lengths = q.lengths + 2
    assert L.hk_dqn_agent_move(ctypes.byref(q), None) == A.HK_ERR_ALIGN
    q = _agent_desc()
    q.features_out = q.points + 8  # the features inside the state
    assert L.hk_dqn_agent_move(ctypes.byref(q), None) == A.HK_ERR_SHAPE
    q = _agent_desc()
    q.features_out = q.points
    assert L.hk_dqn_agent_move(ctypes.byref(q), None) == A.HK_ERR_SHAPE
    q = _agent_desc()
    q.axis_out = q.class_id  # an output over an input
    assert L.hk_dqn_agent_move(ctypes.byref(q), None) == A.HK_ERR_SHAPE
