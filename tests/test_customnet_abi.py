"""CPU-side checks of the boundary of hk_customnet_forward (include/hironaka_hip_customnet.h): the library exports it, the
python mirror of the header agrees with it, and bad arguments are refused on the host, before any launch.  The tower
table lies in device memory and is not read by the host: its contents are ops.CustomnetPlan's to check."""
import ctypes
import os
import re
import subprocess

import abi_cases
from conftest import ROOT
from hironaka_amd import _abi as A
from hironaka_amd import _lib

HEADER = "hironaka_hip_customnet.h"
ENTRIES = {"hk_customnet_forward", "hk_customnet_workspace_bytes"}


def test_library_exports_the_customnet_entry_points():
    _lib.build()
    declared = abi_cases.declared(HEADER)
    assert declared == set(A.CUSTOMNET_PROTOTYPES) == ENTRIES
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r"\bT (hk_customnet_\w+)", exported)) == declared  # exactly what the header declares
    assert not declared & (set(A.PROTOTYPES) | set(A.PVNET_PROTOTYPES))
    text = abi_cases.header()
    assert text.index('#include "hironaka_hip_pvnet.h"') < text.index(f'#include "{HEADER}"')
    assert not re.search(r"#define\s+HK_CUSTOMNET_", text)  # the feature's defines live in its own header
    assert not re.search(r"#define\s+HK_CUSTOMNET_", abi_cases.header("hironaka_hip_pvnet.h"))
    assert _lib.lib().hk_abi_version() == A.HK_ABI_VERSION == 6
    for name in ENTRIES:
        assert getattr(_lib.lib(), name).argtypes == A.CUSTOMNET_PROTOTYPES[name][1], name  # bound by default
    with open(os.path.join(ROOT, "hironaka_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SINGLES :=.*\bcustomnet\b", f.read(), flags=re.M)


def test_customnet_constants_match_header():
    defines = re.findall(r"#define\s+(HK_\w+)\s+(\d+)u?\s", abi_cases.header(HEADER))
    assert len(defines) == 4 and all(name.startswith("HK_CUSTOMNET_") for name, _ in defines)
    for name, value in defines:
        assert getattr(A, name) == int(value), name
    assert (A.HK_CUSTOMNET_RAW_VALUE, A.HK_CUSTOMNET_FORCE_TILE_SMALL, A.HK_CUSTOMNET_FORCE_TILE_LARGE) == \
        (A.HK_PVNET_RAW_VALUE, A.HK_MLP_FORCE_TILE_SMALL, A.HK_MLP_FORCE_TILE_LARGE)
    assert ctypes.sizeof(A.hk_customnet_desc) == 10 * 8 + 4 * 8 + 10 * 4 <= 4096 - 64  # the kernels' argument


def test_customnet_descriptor_layout_matches_c(tmp_path):
    """sizeof/offsetof as the C compiler sees them (gcc on the header) == ctypes"""
    abi_cases.assert_layouts_match_c({"hk_customnet_desc": A.hk_customnet_desc}, tmp_path)


def test_workspace_bytes():
    L = _lib.lib()
    words = lambda batch, m: 72 + 4 * ((batch + 15) // 16 + m + 1) + 2 * batch  # noqa: E731  (72: the counters)
    for batch, m in ((0, 1), (1, 5), (16, 5), (17, 20), (100, 64), (1 << 20, 20), ((1 << 31) - 1, 64)):
        assert L.hk_customnet_workspace_bytes(batch, m) == (4 * words(batch, m) + 15) // 16 * 16, (batch, m)
    assert L.hk_customnet_workspace_bytes(-1, 5) == 0 and L.hk_customnet_workspace_bytes(8, 0) == 0
    assert L.hk_customnet_workspace_bytes(8, 65) == 0


_PTRS = ("x", "policy", "value", "towers", "policy_weight", "policy_bias", "value_weight", "value_bias", "workspace", "gate")


def _desc(m=5, d=3, e=3, nblocks=2, n_last=32, batch=4, actions=3, **top):
    """a descriptor whose every array is a region of its own of one host block; `top` changes the descriptor's fields:
    ("shift", bytes) moves a pointer, ("at", output, bytes) points it at that output.  (The pointers are the host's: every
    call below returns before a launch.)"""
    region = 512 * 1024
    buf = (ctypes.c_char * (region * (len(_PTRS) + 1)))()
    at = (ctypes.addressof(buf) + 63) // 64 * 64
    q = A.hk_customnet_desc()
    for j, name in enumerate(_PTRS):
        setattr(q, name, at + j * region)
    q.gate = None
    q.m, q.d, q.e, q.nblocks, q.n_last, q.batch, q.actions, q.dtype = m, d, e, nblocks, n_last, batch, actions, A.HK_F32
    q.x_stride, q.policy_stride, q.value_stride = m * d + e, actions, 1
    q.workspace_bytes = _lib.lib().hk_customnet_workspace_bytes(max(batch, 0), min(max(m, 1), 64))
    for name, v in top.items():
        if isinstance(v, tuple) and v[0] == "shift":
            v = getattr(q, name) + v[1]
        elif isinstance(v, tuple) and v[0] == "at":
            v = getattr(q, v[1]) + v[2]
        setattr(q, name, v)
    q._keep = buf
    return q


def test_customnet_validation_without_gpu():
    L = _lib.lib()
    run = lambda **kw: L.hk_customnet_forward(ctypes.byref(_desc(**kw)), None)  # noqa: E731
    # what is accepted is asked with batch=0 (HK_OK comes after every other check): a batch > 0 that passes would launch
    ok = lambda **kw: L.hk_customnet_forward(ctypes.byref(_desc(batch=0, **kw)), None)  # noqa: E731
    assert L.hk_customnet_forward(None, None) == A.HK_ERR_NULL
    assert ok() == A.HK_OK and ok(e=0) == A.HK_OK and ok(m=1, d=2, e=0) == A.HK_OK and ok(m=64, d=4, e=0) == A.HK_OK
    assert ok(m=20, d=3, e=3, nblocks=32, n_last=253, actions=255, policy_stride=255) == A.HK_OK
    assert ok(e=5) == A.HK_OK  # any e >= 0
    # dtype and flags come first
    for dtype in (A.HK_F64, A.HK_I32, 9, -1):
        assert run(dtype=dtype) == A.HK_ERR_UNSUPPORTED and run(dtype=dtype, m=0) == A.HK_ERR_UNSUPPORTED
    assert run(flags=8) == A.HK_ERR_UNSUPPORTED
    assert run(flags=A.HK_CUSTOMNET_FORCE_TILE_SMALL | A.HK_CUSTOMNET_FORCE_TILE_LARGE) == A.HK_ERR_UNSUPPORTED
    for flags in (A.HK_CUSTOMNET_RAW_VALUE, A.HK_CUSTOMNET_FORCE_TILE_SMALL, A.HK_CUSTOMNET_FORCE_TILE_LARGE | A.HK_CUSTOMNET_RAW_VALUE):
        assert ok(flags=flags) == A.HK_OK
    # the scalars
    assert run(d=1) == A.HK_ERR_SHAPE and run(m=0) == A.HK_ERR_SHAPE and run(m=65, d=2) == A.HK_ERR_SHAPE and run(e=-1) == A.HK_ERR_SHAPE
    assert run(m=64, d=4, e=1) == A.HK_ERR_SHAPE and run(m=20, d=13, e=0) == A.HK_ERR_SHAPE      # m d + e > 256
    assert run(n_last=254) == A.HK_ERR_SHAPE and run(n_last=0) == A.HK_ERR_SHAPE and ok(n_last=253) == A.HK_OK  # n_last + e
    assert run(nblocks=0) == A.HK_ERR_SHAPE and run(nblocks=33) == A.HK_ERR_SHAPE
    assert run(actions=0) == A.HK_ERR_SHAPE and run(actions=256, policy_stride=256) == A.HK_ERR_SHAPE
    assert run(batch=-1) == A.HK_ERR_SHAPE and run(x_stride=-1) == A.HK_ERR_SHAPE
    assert run(policy_stride=2) == A.HK_ERR_SHAPE and run(value_stride=0) == A.HK_ERR_SHAPE
    assert ok(x_stride=0) == A.HK_OK and ok(x_stride=40) == A.HK_OK and ok(policy_stride=7, value_stride=5) == A.HK_OK
    assert run(d=1, x=None) == A.HK_ERR_SHAPE  # the scalars before the pointers
    # pointers that are used
    for name in ("x", "policy", "value", "towers", "policy_weight", "value_weight", "workspace"):
        assert run(**{name: None}) == A.HK_ERR_NULL, name
    assert ok(policy_bias=None, value_bias=None) == A.HK_OK and ok(gate=("at", "x", 4096)) == A.HK_OK
    assert run(x=None, policy=("shift", 2)) == A.HK_ERR_NULL  # NULL before alignment
    # alignment: 4 bytes, the table 8, the workspace 16
    for name in ("x", "policy", "value", "policy_weight", "policy_bias", "value_weight", "value_bias"):
        assert run(**{name: ("shift", 2)}) == A.HK_ERR_ALIGN, name
        assert ok(**{name: ("shift", 4)}) == A.HK_OK, name
    assert run(gate=("at", "x", 4098)) == A.HK_ERR_ALIGN
    assert run(towers=("shift", 4)) == A.HK_ERR_ALIGN and ok(towers=("shift", 8)) == A.HK_OK
    assert run(workspace=("shift", 8)) == A.HK_ERR_ALIGN and ok(workspace=("shift", 16)) == A.HK_OK
    # spans and the workspace's size: after alignment, before the overlaps
    assert run(batch=2, x_stride=1 << 62) == A.HK_ERR_SHAPE and run(batch=2, policy_stride=1 << 62) == A.HK_ERR_SHAPE
    assert run(batch=2, value_stride=1 << 62) == A.HK_ERR_SHAPE
    assert run(batch=2, x_stride=1 << 62, x=("shift", 2)) == A.HK_ERR_ALIGN
    need = L.hk_customnet_workspace_bytes(4, 5)
    assert run(workspace_bytes=need - 1) == A.HK_ERR_SHAPE and run(workspace_bytes=0) == A.HK_ERR_SHAPE
    assert ok(workspace_bytes=L.hk_customnet_workspace_bytes(0, 5)) == A.HK_OK
    assert ok(workspace_bytes=L.hk_customnet_workspace_bytes(0, 5) - 1) == A.HK_ERR_SHAPE
    assert run(workspace_bytes=need - 1, x=("at", "policy", 0)) == A.HK_ERR_SHAPE
    # an output may share no byte with the input, a head parameter, the table or the workspace: 4 rows of 3 floats are
    # 48 bytes, 4 values 16
    for out, last in (("policy", 44), ("value", 12)):
        for name in ("x", "policy_weight", "policy_bias", "value_weight", "value_bias"):
            assert run(**{name: ("at", out, 0)}) == A.HK_ERR_UNSUPPORTED, (out, name)
            assert run(**{name: ("at", out, last)}) == A.HK_ERR_UNSUPPORTED, (out, name)
        assert run(towers=("at", out, 8)) == A.HK_ERR_UNSUPPORTED and run(workspace=("at", out, 0)) == A.HK_ERR_UNSUPPORTED
    assert run(x=("at", "policy", -4 * (4 * 18) + 4)) == A.HK_ERR_UNSUPPORTED        # x's last element on policy's first
    assert run(towers=("at", "value", -5 * 2 * 112 + 8)) == A.HK_ERR_UNSUPPORTED     # the table's last 8 bytes
    assert run(value_weight=("at", "policy", -4 * 35 + 4)) == A.HK_ERR_UNSUPPORTED   # [1, n_last + e]
    assert ok(x=("at", "policy", 0)) == A.HK_OK  # no rows: nothing to share
