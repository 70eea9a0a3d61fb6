"""CPU-side checks of the boundary of hk_dqn_td / hk_polyak_update (include/hironaka_hip_dqn.h): the library exports
them, the python mirror of the header agrees with it, and bad arguments are refused on the host, before any launch."""
import ctypes
import os
import re

import abi_cases
from conftest import ROOT
from hironaka_amd import _abi as A
from hironaka_amd import _lib


def _header():
    return abi_cases.header("hironaka_hip_dqn.h")


def test_library_exports_the_dqn_entry_points():
    _lib.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    declared = abi_cases.declared("hironaka_hip_dqn.h")
    assert declared == set(A.DQN_PROTOTYPES) == {"hk_dqn_td", "hk_dqn_td_workspace_bytes", "hk_polyak_update"}
    for name in declared:
        assert hasattr(handle, name), name
    assert not declared & set(A.PROTOTYPES)
    text = abi_cases.header()
    assert '#include "hironaka_hip_dqn.h"' in text
    assert not re.search(r"#define\s+HK_(DQN|POLYAK)_", text)  # the feature's defines live in its own header
    assert _lib.lib().hk_abi_version() == A.HK_ABI_VERSION == 6
    assert _lib.lib().hk_dqn_td.argtypes == A.DQN_PROTOTYPES["hk_dqn_td"][1]  # bound by default
    with open(os.path.join(ROOT, "hironaka_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SINGLES :=.*\bdqn\b", f.read(), flags=re.M)


def test_dqn_constants_match_header():
    defines = re.findall(r"#define\s+(HK_\w+)\s+(\d+)u?\s", _header())
    assert len(defines) == 5 and all(re.match(r"HK_(DQN|POLYAK)_", name) for name, _ in defines)
    for name, value in defines:
        assert getattr(A, name) == int(value), name
    assert A.HK_DQN_TILE_ROWS % 64 == 0 and A.HK_POLYAK_CHUNK_BYTES == 256 * 4 * 16


def test_dqn_descriptor_layouts_match_c(tmp_path):
    """sizeof/offsetof as the C compiler sees them (gcc on the header) == ctypes"""
    abi_cases.assert_layouts_match_c({"hk_dqn_td_desc": A.hk_dqn_td_desc, "hk_polyak_tensor": A.hk_polyak_tensor,
                                      "hk_polyak_desc": A.hk_polyak_desc}, tmp_path)


def test_workspace_bytes():
    L = _lib.lib()
    R = A.HK_DQN_TILE_ROWS
    assert L.hk_dqn_td_workspace_bytes(-1) == 0
    assert L.hk_dqn_td_workspace_bytes(0) == L.hk_dqn_td_workspace_bytes(1) == L.hk_dqn_td_workspace_bytes(R) == 24
    assert L.hk_dqn_td_workspace_bytes(R + 1) == 32 and L.hk_dqn_td_workspace_bytes(40 * R + 3) == 16 + 41 * 8
    assert L.hk_dqn_td_workspace_bytes(2 ** 31 - 1) == 16 + 8 * (2 ** 31 // R)


_POINTERS = ("q", "next_q", "actions", "rewards", "dones", "target", "row_loss", "dq", "loss", "workspace", "status")


def _td(**over):
    """a descriptor that passes every check up to the launch, but for what `over` changes: 4 rows of 3 actions, float64,
    every array in a region of its own of one host block"""
    buf = (ctypes.c_int64 * 512)()
    at = ctypes.addressof(buf)
    d = A.hk_dqn_td_desc()
    for k, name in enumerate(_POINTERS):
        setattr(d, name, at + 256 * k)
    d.q_stride, d.next_q_stride, d.dq_stride = 3, 4, 5
    d.gamma, d.batch, d.num_actions, d.dtype = 0.99, 4, 3, A.HK_F64
    for name, v in over.items():
        setattr(d, name, v + getattr(d, name) if isinstance(v, _Shift) else
                getattr(d, v[0]) + v[1] if isinstance(v, _At) else v)
    d._keep = buf
    return d


class _Shift(int):
    """move a pointer by this many bytes instead of replacing it"""


class _At(tuple):
    """(field, bytes): the pointer of another field of the same descriptor, moved by so many bytes"""


def test_dqn_td_validation_without_gpu():
    L = _lib.lib()
    td = lambda **over: L.hk_dqn_td(ctypes.byref(_td(**over)), None)  # noqa: E731
    assert L.hk_dqn_td(None, None) == A.HK_ERR_NULL
    assert td(batch=0) == A.HK_OK  # a valid descriptor, nothing to do
    assert td(batch=0, q=None, dq=None, workspace=None) == A.HK_OK  # a batch of no rows has no arrays
    assert td(batch=0, num_actions=65536, q_stride=65536, next_q_stride=65536, dq_stride=65536) == A.HK_OK
    assert td(batch=-1) == A.HK_ERR_SHAPE
    for dtype in (A.HK_I32, A.HK_I64, A.HK_U8, 7, -1):
        assert td(dtype=dtype) == A.HK_ERR_UNSUPPORTED and td(batch=0, dtype=dtype) == A.HK_ERR_UNSUPPORTED
    for batch in (0, 4):
        assert td(batch=batch, num_actions=0) == A.HK_ERR_SHAPE
        assert td(batch=batch, num_actions=-3) == A.HK_ERR_SHAPE
        assert td(batch=batch, num_actions=65537, q_stride=1 << 20, next_q_stride=1 << 20,
                  dq_stride=1 << 20) == A.HK_ERR_SHAPE
        for stride in ("q_stride", "next_q_stride", "dq_stride"):
            assert td(batch=batch, **{stride: 2}) == A.HK_ERR_SHAPE  # a stride below A
            assert td(batch=batch, **{stride: 0}) == A.HK_ERR_SHAPE
            assert td(batch=batch, **{stride: -5}) == A.HK_ERR_SHAPE
    assert td(q_stride=1 << 62) == A.HK_ERR_SHAPE  # the rows would span more than the address space
    for name in _POINTERS:
        if name not in ("target", "row_loss"):
            assert td(**{name: None}) == A.HK_ERR_NULL, name
    for name in ("q", "next_q", "dq", "loss", "target", "row_loss"):
        assert td(**{name: _Shift(4)}) == A.HK_ERR_ALIGN, name  # float64 elements off by four bytes
    for name in ("actions", "rewards", "status"):
        assert td(**{name: _Shift(2)}) == A.HK_ERR_ALIGN, name
    assert td(workspace=_Shift(4)) == A.HK_ERR_ALIGN
    # dq on top of q or next_q, or reaching into them: 4 rows of stride 5 span (3 * 5 + 3) * 8 = 144 bytes
    assert td(dq=_At(("q", 0))) == A.HK_ERR_UNSUPPORTED
    assert td(dq=_At(("next_q", 0))) == A.HK_ERR_UNSUPPORTED
    assert td(dq=_At(("q", -136))) == A.HK_ERR_UNSUPPORTED and td(dq=_At(("next_q", 112))) == A.HK_ERR_UNSUPPORTED
    assert td(dq=_At(("q", 88))) == A.HK_ERR_UNSUPPORTED  # q's rows span (3 * 3 + 3) * 8 = 96 bytes


def _polyak(n=3, numel=5, dtype=A.HK_F32, tau=0.3, **entry1):
    """n entries of `numel` elements, every src and dst a region of its own; `entry1` changes entry 1 (_At((k, field,
    bytes)): to where that field of entry k points, moved by so many bytes)"""
    buf = (ctypes.c_int64 * (64 * 2 * A.HK_POLYAK_MAX_TENSORS))()
    at = ctypes.addressof(buf)
    d = A.hk_polyak_desc()
    for k in range(A.HK_POLYAK_MAX_TENSORS):
        d.tensor[k].src, d.tensor[k].dst, d.tensor[k].numel = at + 1024 * k, at + 1024 * k + 512, numel
    for name, v in entry1.items():
        setattr(d.tensor[1], name, v + getattr(d.tensor[1], name) if isinstance(v, _Shift) else
                getattr(d.tensor[v[0]], v[1]) + v[2] if isinstance(v, _At) else v)
    d.tau, d.ntensors, d.dtype = tau, n, dtype
    d._keep = buf
    return d


def test_polyak_validation_without_gpu():
    L = _lib.lib()
    run = lambda **kw: L.hk_polyak_update(ctypes.byref(_polyak(**kw)), None)  # noqa: E731
    assert L.hk_polyak_update(None, None) == A.HK_ERR_NULL
    assert run(n=0) == A.HK_OK
    assert run(numel=0) == A.HK_OK and run(n=64, numel=0) == A.HK_OK  # nothing to do: no launch
    assert run(numel=0, src=None, dst=None) == A.HK_OK  # an entry without elements has no arrays
    assert run(n=-1) == A.HK_ERR_SHAPE and run(n=65) == A.HK_ERR_SHAPE
    for dtype in (A.HK_I32, A.HK_U8, 9):
        assert run(dtype=dtype) == A.HK_ERR_UNSUPPORTED and run(n=0, dtype=dtype) == A.HK_ERR_UNSUPPORTED
    assert run(numel=-1) == A.HK_ERR_SHAPE
    assert run(src=None) == A.HK_ERR_NULL and run(dst=None) == A.HK_ERR_NULL
    assert run(src=_Shift(2)) == A.HK_ERR_ALIGN and run(dst=_Shift(1)) == A.HK_ERR_ALIGN
    assert run(dtype=A.HK_F64, dst=_Shift(4)) == A.HK_ERR_ALIGN
    assert run(dst=_At((1, "src", 0))) == A.HK_ERR_UNSUPPORTED  # src == dst
    assert run(dst=_At((1, "src", 16))) == A.HK_ERR_UNSUPPORTED  # 20-byte ranges 16 bytes apart
    assert run(dst=_At((1, "src", -16))) == A.HK_ERR_UNSUPPORTED
    assert run(dst=_At((2, "src", 0))) == A.HK_ERR_UNSUPPORTED  # written by one entry, read by another
    assert run(dst=_At((0, "dst", 4))) == A.HK_ERR_UNSUPPORTED  # two entries write the same bytes
