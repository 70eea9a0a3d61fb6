"""CPU-side checks of the boundary of hk_optim_prepare / hk_optim_apply (include/hironaka_hip_optim.h): the library
exports them, the python mirror of the header agrees with it, and bad arguments are refused on the host, before any
launch."""
import ctypes
import os
import re
import subprocess

import abi_cases
from conftest import ROOT
from hironaka_amd import _abi as A
from hironaka_amd import _lib


def _header():
    return abi_cases.header("hironaka_hip_optim.h")


def test_library_exports_the_optim_entry_points():
    _lib.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    declared = abi_cases.declared("hironaka_hip_optim.h")
    assert declared == set(A.OPTIM_PROTOTYPES) == {"hk_optim_workspace_bytes", "hk_optim_prepare", "hk_optim_apply"}
    for name in declared:
        assert hasattr(handle, name), name
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r"\bT (hk_optim_\w+)", exported)) == declared  # exactly what the header declares
    assert not declared & (set(A.PROTOTYPES) | set(A.DQN_PROTOTYPES))
    text = abi_cases.header()
    assert text.index('#include "hironaka_hip_dqn.h"') < text.index('#include "hironaka_hip_optim.h"')
    assert not re.search(r"#define\s+HK_OPTIM_", text)  # the feature's defines live in its own header
    assert "optim" not in abi_cases.header("hironaka_hip_dqn.h").lower()
    assert _lib.lib().hk_abi_version() == A.HK_ABI_VERSION == 6
    assert _lib.lib().hk_optim_apply.argtypes == A.OPTIM_PROTOTYPES["hk_optim_apply"][1]  # bound by default
    with open(os.path.join(ROOT, "hironaka_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SINGLES :=.*\boptim\b", f.read(), flags=re.M)


def test_optim_constants_match_header():
    defines = re.findall(r"#define\s+(HK_\w+)\s+(\d+)u?\s", _header())
    assert len(defines) == 11 and all(name.startswith("HK_OPTIM_") for name, _ in defines)
    for name, value in defines:
        assert getattr(A, name) == int(value), name
    assert A.HK_OPTIM_CHUNK_BYTES == 256 * 4 * 16 and A.HK_OPTIM_STATE_BYTES == ctypes.sizeof(A.hk_optim_state) == 64
    assert ctypes.sizeof(A.hk_optim_tensor) == 40
    # the table travels as the kernel's argument, next to the first-workgroup table and the scalars
    assert ctypes.sizeof(A.hk_optim_desc) + 4 * (A.HK_OPTIM_MAX_TENSORS + 1) + A.HK_OPTIM_MAX_TENSORS < 4096


def test_optim_descriptor_layouts_match_c(tmp_path):
    """sizeof/offsetof as the C compiler sees them (gcc on the header) == ctypes"""
    abi_cases.assert_layouts_match_c({"hk_optim_tensor": A.hk_optim_tensor, "hk_optim_state": A.hk_optim_state,
                                      "hk_optim_desc": A.hk_optim_desc}, tmp_path)


def test_workspace_bytes():
    L = _lib.lib()
    assert L.hk_optim_workspace_bytes(-1) == 0 and L.hk_optim_workspace_bytes(2 ** 31) == 0
    assert L.hk_optim_workspace_bytes(0) == L.hk_optim_workspace_bytes(1) == 24
    assert L.hk_optim_workspace_bytes(2) == 32
    assert L.hk_optim_workspace_bytes(2 ** 31 - 1) == 16 + 8 * (2 ** 31 - 1)


class _Shift(int):
    """move a pointer by this many bytes instead of replacing it"""


class _At(tuple):
    """(entry, field, bytes): to where that field of entry k points, moved by so many bytes"""


_FIELDS = ("param", "grad", "state1", "state2")


def _desc(n=3, numel=5, dtype=A.HK_F32, kind=A.HK_OPTIM_ADAM, top=None, **entry1):
    """n entries of `numel` elements, every array a region of its own of one host block; `entry1` changes entry 1, `top`
    the descriptor's own fields.  (The pointers are the host's: every call below returns before a launch.)"""
    buf = (ctypes.c_int64 * (32 * 4 * A.HK_OPTIM_MAX_TENSORS + 64))()
    at = ctypes.addressof(buf)
    d = A.hk_optim_desc()
    for k in range(A.HK_OPTIM_MAX_TENSORS):
        for j, name in enumerate(_FIELDS):
            setattr(d.tensor[k], name, at + 1024 * k + 256 * j)
        d.tensor[k].numel = numel
    end = at + 1024 * A.HK_OPTIM_MAX_TENSORS
    d.state, d.workspace, d.lr_dev = end, end + 128, None
    d.lr, d.beta1, d.beta2, d.eps, d.max_norm = 1e-3, 0.9, 0.999, 1e-8, 1.0
    d.ntensors, d.dtype, d.kind = n, dtype, kind
    for name, v in entry1.items():
        setattr(d.tensor[1], name, v + getattr(d.tensor[1], name) if isinstance(v, _Shift) else
                getattr(d.tensor[v[0]], v[1]) + v[2] if isinstance(v, _At) else v)
    for name, v in (top or {}).items():
        setattr(d, name, v + getattr(d, name) if isinstance(v, _Shift) else v)
    d._keep = buf
    return d


def test_optim_validation_without_gpu():
    L = _lib.lib()
    prepare = lambda **kw: L.hk_optim_prepare(ctypes.byref(_desc(**kw)), None)  # noqa: E731
    apply = lambda **kw: L.hk_optim_apply(ctypes.byref(_desc(**kw)), None)  # noqa: E731
    assert L.hk_optim_prepare(None, None) == A.HK_ERR_NULL and L.hk_optim_apply(None, None) == A.HK_ERR_NULL
    for run in (prepare, apply):
        # nothing to do: no launch
        assert run(n=0) == A.HK_OK
        assert run(numel=0) == A.HK_OK and run(n=64, numel=0) == A.HK_OK
        assert run(numel=0, param=None, grad=None, state1=None, state2=None) == A.HK_OK
        assert run(n=0, top=dict(flags=A.HK_OPTIM_LAST | A.HK_OPTIM_ADVANCE)) == A.HK_OK
        # counts
        assert run(n=-1) == A.HK_ERR_SHAPE and run(n=65) == A.HK_ERR_SHAPE
        assert run(numel=-1) == A.HK_ERR_SHAPE
        assert run(top=dict(slot_base=-1)) == A.HK_ERR_SHAPE
        # kind, dtype, flags
        for dtype in (A.HK_I32, A.HK_U8, 9, -1):
            assert run(dtype=dtype) == A.HK_ERR_UNSUPPORTED and run(n=0, dtype=dtype) == A.HK_ERR_UNSUPPORTED
        for kind in (-1, 3, 17):
            assert run(kind=kind) == A.HK_ERR_UNSUPPORTED and run(n=0, kind=kind) == A.HK_ERR_UNSUPPORTED
        assert run(top=dict(flags=32)) == A.HK_ERR_UNSUPPORTED
        # pointers
        assert run(top=dict(state=None)) == A.HK_ERR_NULL
        assert run(top=dict(state=_Shift(4))) == A.HK_ERR_ALIGN
        assert run(grad=None) == A.HK_ERR_NULL
        assert run(grad=_Shift(2)) == A.HK_ERR_ALIGN
        assert run(dtype=A.HK_F64, grad=_Shift(4)) == A.HK_ERR_ALIGN
    # prepare: the workspace and lr_dev; only the gradients are looked at
    assert prepare(top=dict(workspace=None)) == A.HK_ERR_NULL
    assert prepare(top=dict(workspace=_Shift(4))) == A.HK_ERR_ALIGN
    assert prepare(top=dict(lr_dev=12)) == A.HK_ERR_ALIGN
    assert prepare(n=0, top=dict(workspace=None)) == A.HK_ERR_NULL
    assert prepare(numel=0, param=None, state1=None, state2=None) == A.HK_OK
    assert prepare(numel=1 << 59) == A.HK_ERR_SHAPE  # more workgroups than a grid has
    # apply: what the kind uses
    assert apply(numel=0, top=dict(workspace=None)) == A.HK_OK
    for name in ("param", "state1", "state2"):
        assert apply(**{name: None}) == A.HK_ERR_NULL, name
        assert apply(**{name: _Shift(1)}) == A.HK_ERR_ALIGN, name
        assert apply(dtype=A.HK_F64, **{name: _Shift(4)}) == A.HK_ERR_ALIGN, name
        assert apply(kind=A.HK_OPTIM_SCALE, numel=0, **{name: None}) == A.HK_OK, name
    assert apply(kind=A.HK_OPTIM_SGD, state1=None, top=dict(momentum=0.9)) == A.HK_ERR_NULL
    assert apply(kind=A.HK_OPTIM_SCALE, top=dict(flags=A.HK_OPTIM_KEEP_GRADS)) == A.HK_ERR_UNSUPPORTED  # nothing to do
    # overlapping ranges between any two of param / grad / state, within an entry and across entries
    for name in _FIELDS:
        for other in _FIELDS:
            if name != other:
                assert apply(**{name: _At((1, other, 0))}) == A.HK_ERR_UNSUPPORTED, (name, other)
                assert apply(**{name: _At((1, other, 16))}) == A.HK_ERR_UNSUPPORTED  # 20-byte ranges 16 bytes apart
                assert apply(**{name: _At((1, other, -16))}) == A.HK_ERR_UNSUPPORTED
            assert apply(**{name: _At((2, other, 4))}) == A.HK_ERR_UNSUPPORTED, (name, other)
            assert apply(**{name: _At((0, other, -4))}) == A.HK_ERR_UNSUPPORTED, (name, other)
    # ranges that a kind does not use may coincide
    assert apply(kind=A.HK_OPTIM_SGD, numel=0, state1=_At((1, "param", 0))) == A.HK_OK
