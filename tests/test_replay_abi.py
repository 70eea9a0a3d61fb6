"""CPU-side checks of the boundary of hk_replay_push / hk_replay_sample (include/hironaka_hip_replay.h): the library
exports them, the python mirror of the header agrees with it, and bad arguments are refused on the host, before any
launch."""
import ctypes
import re

import abi_cases
from hironaka_amd import _abi as A
from hironaka_amd import _lib


def _header():
    return abi_cases.header("hironaka_hip_replay.h")


def test_library_exports_the_replay_entry_points():
    _lib.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    declared = abi_cases.declared("hironaka_hip_replay.h")
    assert declared == set(A.REPLAY_PROTOTYPES) == {"hk_replay_push", "hk_replay_sample"}
    for name in declared:
        assert hasattr(handle, name), name
    assert not declared & set(A.PROTOTYPES)
    assert '#include "hironaka_hip_replay.h"' in abi_cases.header()
    assert _lib.lib().hk_abi_version() == A.HK_ABI_VERSION == 6
    assert _lib.lib().hk_replay_push.argtypes == A.REPLAY_PROTOTYPES["hk_replay_push"][1]  # bound by default


def test_replay_constants_match_header():
    found = re.findall(r"#define\s+(HK_REPLAY_\w+)\s+(\d+)\s", _header())
    assert len(found) == 10
    for name, value in found:
        assert getattr(A, name) == int(value), name


def test_replay_descriptor_layout_matches_c(tmp_path):
    """sizeof/offsetof as the C compiler sees them (gcc on the header) == ctypes"""
    abi_cases.assert_layouts_match_c({"hk_replay_col": A.hk_replay_col, "hk_replay_desc": A.hk_replay_desc}, tmp_path)


def _desc(ncols=2, col=None, **over):
    """a descriptor that passes every check up to the launch, but for what `over` (and `col`, for column 1) changes"""
    buf = (ctypes.c_int64 * 64)()
    at = ctypes.addressof(buf)
    q = A.hk_replay_desc()
    for c in range(A.HK_REPLAY_MAX_COLS):
        q.col[c].ring, q.col[c].rows, q.col[c].row_bytes, q.col[c].rows_stride_bytes = at, at, 12, 16
    q.keep, q.cursor, q.ncols, q.batch, q.capacity = at, at, ncols, 4, 10
    for name, v in (col or {}).items():
        setattr(q.col[1], name, v)
    for name, v in over.items():
        setattr(q, name, v)
    q._keep = buf
    return q


def test_replay_validation_without_gpu():
    L = _lib.lib()
    push = lambda **over: L.hk_replay_push(ctypes.byref(_desc(**over)), None)  # noqa: E731
    sample = lambda n=0, **over: L.hk_replay_sample(ctypes.byref(_desc(**over)), n, 7, None, None)  # noqa: E731
    assert L.hk_replay_push(None, None) == A.HK_ERR_NULL
    assert L.hk_replay_sample(None, 4, 7, None, None) == A.HK_ERR_NULL
    assert push(batch=0) == A.HK_OK  # a valid descriptor, nothing to do
    assert push(batch=0, ncols=8, keep=None) == A.HK_OK
    assert sample() == A.HK_OK
    for call in (lambda **over: push(batch=0, **over), sample):
        assert call(ncols=0) == A.HK_ERR_SHAPE
        assert call(ncols=9) == A.HK_ERR_SHAPE
        assert call(capacity=0) == A.HK_ERR_SHAPE
        assert call(cursor=None) == A.HK_ERR_NULL
        assert call(col=dict(ring=None)) == A.HK_ERR_NULL
        assert call(col=dict(row_bytes=0)) == A.HK_ERR_SHAPE
        assert call(col=dict(rows_stride_bytes=11)) == A.HK_ERR_SHAPE  # a stride below the row size
        assert call(col=dict(row_bytes=(1 << 20) + 1, rows_stride_bytes=1 << 21)) == A.HK_ERR_UNSUPPORTED
        assert call(col=dict(row_bytes=1, rows_stride_bytes=1)) == A.HK_OK
        assert call(ncols=1, col=dict(ring=None, row_bytes=0)) == A.HK_OK  # column 1 is not looked at
        q = _desc(batch=0)
        q.cursor = q.cursor + 4
        assert (L.hk_replay_push(ctypes.byref(q), None) if call is not sample
                else L.hk_replay_sample(ctypes.byref(q), 0, 7, None, None)) == A.HK_ERR_ALIGN
    assert push(batch=-1) == A.HK_ERR_SHAPE
    assert push(batch=10) == A.HK_ERR_SHAPE  # batch >= capacity: the reference asserts buffer_size > length
    assert push(batch=11) == A.HK_ERR_SHAPE
    assert push(batch=1, capacity=1) == A.HK_ERR_SHAPE
    assert push(col=dict(rows=None)) == A.HK_ERR_NULL
    assert sample(-1) == A.HK_ERR_SHAPE
    assert sample(3, col=dict(rows=None)) == A.HK_ERR_NULL
    assert sample(0, batch=99) == A.HK_OK  # a sample does not look at the push's batch
