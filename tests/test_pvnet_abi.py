"""CPU-side checks of the boundary of hk_pvnet_forward (include/hironaka_hip_pvnet.h): the library exports it, the python
mirror of the header agrees with it, and bad arguments are refused on the host, before any launch."""
import ctypes
import os
import re
import subprocess

import abi_cases
from conftest import ROOT
from hironaka_amd import _abi as A
from hironaka_amd import _lib


def test_library_exports_the_pvnet_entry_point():
    _lib.build()
    declared = abi_cases.declared("hironaka_hip_pvnet.h")
    assert declared == set(A.PVNET_PROTOTYPES) == {"hk_pvnet_forward"}
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r"\bT (hk_pvnet_\w+)", exported)) == declared  # exactly what the header declares
    text = abi_cases.header()
    assert text.index('#include "hironaka_hip_mlp_train.h"') < text.index('#include "hironaka_hip_pvnet.h"')
    assert not re.search(r"#define\s+HK_PVNET_", text)  # the feature's defines live in its own header
    assert _lib.lib().hk_abi_version() == A.HK_ABI_VERSION == 6
    assert _lib.lib().hk_pvnet_forward.argtypes == A.PVNET_PROTOTYPES["hk_pvnet_forward"][1]  # bound by default
    with open(os.path.join(ROOT, "hironaka_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SINGLES :=.*\bpvnet\b", f.read(), flags=re.M)


def test_pvnet_constants_match_header():
    defines = re.findall(r"#define\s+(HK_\w+)\s+(\d+)u?\s", abi_cases.header("hironaka_hip_pvnet.h"))
    assert len(defines) == 7 and all(name.startswith("HK_PVNET_") for name, _ in defines)
    for name, value in defines:
        assert getattr(A, name) == int(value), name
    assert (A.HK_PVNET_FORCE_TILE_SMALL, A.HK_PVNET_FORCE_TILE_LARGE) == (A.HK_MLP_FORCE_TILE_SMALL, A.HK_MLP_FORCE_TILE_LARGE)
    assert A.HK_PVNET_MAX_WIDTH == A.HK_MLP_MAX_WIDTH
    assert ctypes.sizeof(A.hk_pvnet_dense) == 32 and ctypes.sizeof(A.hk_pvnet_block) == 112
    assert ctypes.sizeof(A.hk_pvnet_desc) == 104 + 112 * A.HK_PVNET_MAX_BLOCKS <= 4096 - 64  # the kernel's argument


def test_pvnet_descriptor_layouts_match_c(tmp_path):
    """sizeof/offsetof as the C compiler sees them (gcc on the header) == ctypes"""
    abi_cases.assert_layouts_match_c({"hk_pvnet_dense": A.hk_pvnet_dense, "hk_pvnet_block": A.hk_pvnet_block,
                                      "hk_pvnet_desc": A.hk_pvnet_desc}, tmp_path)


_DENSE_PTRS = ("weight", "bias", "gn_scale", "gn_bias")
_TOP_PTRS = ("x", "policy", "value", "policy_weight", "policy_bias", "value_weight", "value_bias")


def _desc(widths=(18, 64, 64, 32), kinds=None, batch=4, actions=3, block1=None, dense=None, **top):
    """a net of the given widths (residue blocks unless `kinds` says otherwise), every array a region of its own of one
    host block; `block1` changes block 1's scalars, `dense` = (block, which, {field: value}) one of its Denses, `top` the
    descriptor's own fields; ("shift", bytes) moves a pointer, ("at", output, bytes) points it at that output.
    (The pointers are the host's: every call below returns before a launch.)"""
    region = 512 * 1024  # more than 256 x 256 floats
    nblocks = len(widths) - 1
    buf = (ctypes.c_char * (region * (8 + 12 * nblocks)))()
    at = (ctypes.addressof(buf) + 63) // 64 * 64
    d = A.hk_pvnet_desc()
    for j, name in enumerate(_TOP_PTRS):
        setattr(d, name, at + j * region)
    d.k0, d.batch, d.nblocks, d.actions, d.dtype = widths[0], batch, nblocks, actions, A.HK_F32
    d.x_stride, d.policy_stride, d.value_stride = widths[0], actions, 1
    for i in range(nblocks):
        e = d.block[i]
        e.k, e.n, e.eps = widths[i], widths[i + 1], 1e-6
        e.kind = A.HK_PVNET_RESIDUE if kinds is None else kinds[i]
        for w, which in enumerate(("dense1", "dense2", "proj")):
            used = w == 0 or (e.kind == A.HK_PVNET_RESIDUE and (w == 1 or e.k != e.n))
            for j, name in enumerate(_DENSE_PTRS):
                setattr(getattr(e, which), name, at + (8 + 12 * i + 4 * w + j) * region if used else None)

    def change(obj, fields):
        for name, v in fields.items():
            if isinstance(v, tuple) and v[0] == "shift":
                v = getattr(obj, name) + v[1]
            elif isinstance(v, tuple) and v[0] == "at":
                v = getattr(d, v[1]) + v[2]
            setattr(obj, name, v)
    change(d.block[1], block1 or {})
    if dense:
        change(getattr(d.block[dense[0]], dense[1]), dense[2])
    change(d, top)
    d._keep = buf
    return d


def test_pvnet_validation_without_gpu():
    L = _lib.lib()
    run = lambda **kw: L.hk_pvnet_forward(ctypes.byref(_desc(**kw)), None)  # noqa: E731
    # what is accepted is asked with batch=0 (HK_OK comes after every other check): a batch > 0 that passes would launch
    ok = lambda **kw: L.hk_pvnet_forward(ctypes.byref(_desc(batch=0, **kw)), None)  # noqa: E731
    D, R = A.HK_PVNET_DENSE, A.HK_PVNET_RESIDUE
    assert L.hk_pvnet_forward(None, None) == A.HK_ERR_NULL
    assert ok() == A.HK_OK and ok(widths=(256,) * 33) == A.HK_OK and ok(widths=(1, 32)) == A.HK_OK
    assert ok(widths=(1, 1, 17, 256, 33), kinds=(D, D, D, D)) == A.HK_OK and ok(widths=(60, 128, 7), kinds=(R, D)) == A.HK_OK
    assert ok(policy=None) == A.HK_ERR_NULL and ok(dtype=A.HK_F64) == A.HK_ERR_UNSUPPORTED
    # counts and widths
    assert run(batch=-1) == A.HK_ERR_SHAPE
    assert run(nblocks=0) == A.HK_ERR_SHAPE and run(nblocks=33) == A.HK_ERR_SHAPE and run(nblocks=-1) == A.HK_ERR_SHAPE
    assert run(widths=(257, 32)) == A.HK_ERR_SHAPE and run(widths=(3, 257), kinds=(D,)) == A.HK_ERR_SHAPE
    assert run(block1=dict(k=0)) == A.HK_ERR_SHAPE and run(block1=dict(n=0)) == A.HK_ERR_SHAPE
    assert run(block1=dict(k=32)) == A.HK_ERR_SHAPE and run(block1=dict(n=128)) == A.HK_ERR_SHAPE  # the chain of widths
    assert run(k0=17) == A.HK_ERR_SHAPE and run(k0=0) == A.HK_ERR_SHAPE
    assert run(actions=0) == A.HK_ERR_SHAPE and run(actions=256, policy_stride=256) == A.HK_ERR_SHAPE
    assert ok(actions=255, policy_stride=255) == A.HK_OK
    assert run(x_stride=-1) == A.HK_ERR_SHAPE and run(policy_stride=2) == A.HK_ERR_SHAPE and run(value_stride=0) == A.HK_ERR_SHAPE
    assert ok(x_stride=0) == A.HK_OK and ok(policy_stride=7, value_stride=5) == A.HK_OK
    # a normed width: a multiple of 32 (a shape), and one of the four the kernel serves
    assert run(widths=(18, 48)) == A.HK_ERR_SHAPE and run(widths=(18, 33)) == A.HK_ERR_SHAPE
    for n in (96, 160, 192, 224):
        assert run(widths=(18, n)) == A.HK_ERR_UNSUPPORTED, n
        assert ok(widths=(18, n), kinds=(D,)) == A.HK_OK, n
    for n in (32, 64, 128, 256):
        assert ok(widths=(18, n)) == A.HK_OK and ok(widths=(n, n)) == A.HK_OK, n
    # dtype, flags and kinds
    for dtype in (A.HK_F64, A.HK_I32, 9, -1):
        assert run(dtype=dtype) == A.HK_ERR_UNSUPPORTED
    assert run(flags=8) == A.HK_ERR_UNSUPPORTED and run(block1=dict(kind=2)) == A.HK_ERR_UNSUPPORTED
    assert run(block1=dict(kind=-1)) == A.HK_ERR_UNSUPPORTED
    assert run(flags=A.HK_PVNET_FORCE_TILE_SMALL | A.HK_PVNET_FORCE_TILE_LARGE) == A.HK_ERR_UNSUPPORTED
    for flags in (A.HK_PVNET_RAW_VALUE, A.HK_PVNET_FORCE_TILE_SMALL, A.HK_PVNET_FORCE_TILE_LARGE | A.HK_PVNET_RAW_VALUE):
        assert ok(flags=flags) == A.HK_OK
    # pointers that are used
    for name in ("x", "policy", "value", "policy_weight", "value_weight"):
        assert run(**{name: None}) == A.HK_ERR_NULL, name
    assert ok(policy_bias=None, value_bias=None) == A.HK_OK
    assert run(dense=(1, "dense1", dict(weight=None))) == A.HK_ERR_NULL
    assert run(dense=(1, "dense2", dict(weight=None))) == A.HK_ERR_NULL
    assert run(dense=(0, "proj", dict(weight=None))) == A.HK_ERR_NULL  # block 0 is 18 -> 64: no projection to add
    assert ok(dense=(1, "proj", dict(weight=None))) == A.HK_OK  # block 1 is 64 -> 64: h itself
    for which in ("dense1", "dense2"):
        assert ok(dense=(1, which, dict(bias=None, gn_scale=None, gn_bias=None))) == A.HK_OK
    assert ok(widths=(18, 7), kinds=(D,), dense=(0, "dense2", dict(weight=2))) == A.HK_OK  # a dense block's are not looked at
    # alignment: 4 bytes, every pointer
    for name in _TOP_PTRS:
        assert run(**{name: ("shift", 2)}) == A.HK_ERR_ALIGN, name
        assert ok(**{name: ("shift", 4)}) == A.HK_OK, name
    for block, which in ((0, "proj"), (1, "dense1"), (1, "dense2")):
        for name in _DENSE_PTRS:
            assert run(dense=(block, which, {name: ("shift", 2)})) == A.HK_ERR_ALIGN, (which, name)
            assert ok(dense=(block, which, {name: ("shift", 4)})) == A.HK_OK, (which, name)
    # an output may share no byte with the input or a parameter: 4 rows of 3 floats are 48 bytes, 4 values 16
    for out, last in (("policy", 44), ("value", 12)):
        for name in ("x", "policy_weight", "policy_bias", "value_weight", "value_bias"):
            assert run(**{name: ("at", out, 0)}) == A.HK_ERR_UNSUPPORTED, (out, name)
            assert run(**{name: ("at", out, last)}) == A.HK_ERR_UNSUPPORTED, (out, name)
        for block, which in ((0, "proj"), (1, "dense1"), (1, "dense2")):
            for name in _DENSE_PTRS:
                assert run(dense=(block, which, {name: ("at", out, last)})) == A.HK_ERR_UNSUPPORTED, (out, which, name)
    assert run(x=("at", "policy", -4 * 4 * 18 + 4)) == A.HK_ERR_UNSUPPORTED  # x's last element on policy's first
    assert run(dense=(1, "dense2", dict(weight=("at", "value", -4 * 64 * 64 + 4)))) == A.HK_ERR_UNSUPPORTED
    assert run(value_bias=("at", "policy", -4 + 4)) == A.HK_ERR_UNSUPPORTED
    assert run(value_weight=("at", "policy", -4 * 32 + 4)) == A.HK_ERR_UNSUPPORTED  # [1, 32]


def test_pvnet_row_span_beyond_63_bits_is_refused():
    """two rows 2^62 floats apart span 2^64 bytes: refused as a shape where the spans are computed (after the pointer and
    alignment checks), not wrapped into a span that passes the overlap check"""
    L = _lib.lib()
    run = lambda **kw: L.hk_pvnet_forward(ctypes.byref(_desc(batch=2, **kw)), None)  # noqa: E731
    assert run(x_stride=1 << 62) == A.HK_ERR_SHAPE
    assert run(policy_stride=1 << 62) == A.HK_ERR_SHAPE and run(value_stride=1 << 62) == A.HK_ERR_SHAPE
    assert run(x_stride=1 << 62, policy=None) == A.HK_ERR_NULL and run(x_stride=1 << 62, x=("shift", 2)) == A.HK_ERR_ALIGN
