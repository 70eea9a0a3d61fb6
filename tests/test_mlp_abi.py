"""CPU-side checks of the boundary of hk_mlp_forward (include/hironaka_hip_mlp.h): the library exports it, the python
mirror of the header agrees with it, and bad arguments are refused on the host, before any launch."""
import ctypes
import os
import re
import subprocess

import abi_cases
from conftest import ROOT
from hironaka_amd import _abi as A
from hironaka_amd import _lib


def _header():
    return abi_cases.header("hironaka_hip_mlp.h")


def test_library_exports_the_mlp_entry_points():
    _lib.build()
    declared = abi_cases.declared("hironaka_hip_mlp.h")
    assert declared == set(A.MLP_PROTOTYPES) == {"hk_mlp_row_tile", "hk_mlp_forward"}
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r"\bT (hk_mlp_\w+)", exported)) == declared  # exactly what the header declares
    text = abi_cases.header()
    assert text.index('#include "hironaka_hip_optim.h"') < text.index('#include "hironaka_hip_mlp.h"')
    assert not re.search(r"#define\s+HK_MLP_", text)  # the feature's defines live in its own header
    assert _lib.lib().hk_abi_version() == A.HK_ABI_VERSION == 6
    assert _lib.lib().hk_mlp_forward.argtypes == A.MLP_PROTOTYPES["hk_mlp_forward"][1]  # bound by default
    with open(os.path.join(ROOT, "hironaka_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SINGLES :=.*\bmlp\b", f.read(), flags=re.M)


def test_mlp_constants_match_header():
    defines = re.findall(r"#define\s+(HK_\w+)\s+(\d+)u?\s", _header())
    assert len(defines) == 9 and all(name.startswith("HK_MLP_") for name, _ in defines)
    for name, value in defines:
        assert getattr(A, name) == int(value), name
    assert ctypes.sizeof(A.hk_mlp_layer) == 64
    assert ctypes.sizeof(A.hk_mlp_desc) == 112 + 64 * A.HK_MLP_MAX_LAYERS < 4096 - 64  # the kernel's argument
    L = _lib.lib()
    for batch in (0, 1, A.HK_MLP_TILE_CROSSOVER):
        assert L.hk_mlp_row_tile(batch) == A.HK_MLP_TILE_SMALL
    assert L.hk_mlp_row_tile(A.HK_MLP_TILE_CROSSOVER + 1) == L.hk_mlp_row_tile(2 ** 31 - 1) == A.HK_MLP_TILE_LARGE


def test_mlp_descriptor_layouts_match_c(tmp_path):
    """sizeof/offsetof as the C compiler sees them (gcc on the header) == ctypes"""
    abi_cases.assert_layouts_match_c({"hk_mlp_layer": A.hk_mlp_layer, "hk_mlp_desc": A.hk_mlp_desc}, tmp_path)


_LAYER_PTRS = ("weight", "bias", "bn_mean", "bn_var", "bn_weight", "bn_bias")
_IN_BN = ("in_bn_mean", "in_bn_var", "in_bn_weight", "in_bn_bias")


def _desc(widths=(5, 7, 3), batch=4, k1=0, bn=True, in_bn=False, layer1=None, **top):
    """a net of the given widths, every array a region of its own of one host block; `layer1` changes layer 1, `top` the
    descriptor's own fields; ("shift", field, bytes) moves a pointer, ("at", field) points it at the descriptor's `out`.
    (The pointers are the host's: every call below returns before a launch.)"""
    region = 512 * 1024  # more than 256 x 256 floats
    buf = (ctypes.c_char * (region * (8 + 6 * len(widths))))()
    at = (ctypes.addressof(buf) + 63) // 64 * 64
    d = A.hk_mlp_desc()
    d.x0, d.x1, d.out = at, (at + region if k1 else None), at + 2 * region
    if in_bn:
        for j, name in enumerate(_IN_BN):
            setattr(d, name, at + (3 + j) * region)
    d.k0, d.k1, d.batch, d.nlayers, d.dtype = widths[0] - k1, k1, batch, len(widths) - 1, A.HK_F32
    d.x0_stride, d.x1_stride, d.out_stride = widths[0] - k1, k1, widths[-1]
    for i in range(len(widths) - 1):
        e = d.layer[i]
        for j, name in enumerate(_LAYER_PTRS):
            setattr(e, name, at + (8 + 6 * i + j) * region if bn or j < 2 else None)
        e.k, e.n, e.eps, e.flags = widths[i], widths[i + 1], 1e-5, A.HK_MLP_RELU if i + 2 < len(widths) else 0

    def change(obj, fields):
        for name, v in fields.items():
            if isinstance(v, tuple) and v[0] == "shift":
                v = getattr(obj, name) + v[1]
            elif isinstance(v, tuple) and v[0] == "at":
                v = d.out + v[1]
            setattr(obj, name, v)
    change(d.layer[1], layer1 or {})
    change(d, top)
    d._keep = buf
    return d


def test_mlp_validation_without_gpu():
    L = _lib.lib()
    run = lambda **kw: L.hk_mlp_forward(ctypes.byref(_desc(**kw)), None)  # noqa: E731
    # what is accepted is asked with batch=0 (HK_OK comes after every other check): a batch > 0 that passes would launch
    ok = lambda **kw: L.hk_mlp_forward(ctypes.byref(_desc(batch=0, **kw)), None)  # noqa: E731
    assert L.hk_mlp_forward(None, None) == A.HK_ERR_NULL
    # nothing to do: no launch -- but only after every other check
    assert ok() == A.HK_OK and ok(k1=2, in_bn=True) == A.HK_OK
    assert ok(widths=(256,) * 33) == A.HK_OK and ok(widths=(1, 1)) == A.HK_OK
    assert ok(out=None) == A.HK_ERR_NULL and ok(dtype=A.HK_F64) == A.HK_ERR_UNSUPPORTED
    # counts and widths
    assert run(batch=-1) == A.HK_ERR_SHAPE
    assert run(nlayers=0) == A.HK_ERR_SHAPE and run(nlayers=33) == A.HK_ERR_SHAPE and run(nlayers=-1) == A.HK_ERR_SHAPE
    assert run(widths=(257, 3)) == A.HK_ERR_SHAPE and run(widths=(3, 257)) == A.HK_ERR_SHAPE
    assert run(layer1=dict(k=0)) == A.HK_ERR_SHAPE and run(layer1=dict(n=0)) == A.HK_ERR_SHAPE
    assert run(layer1=dict(k=6)) == A.HK_ERR_SHAPE and run(layer1=dict(n=4)) == A.HK_ERR_SHAPE  # n=4: out_stride is 3
    assert run(k0=4) == A.HK_ERR_SHAPE and run(k0=0) == A.HK_ERR_SHAPE and ok(k1=1) == A.HK_OK
    assert run(k1=-1, k0=6) == A.HK_ERR_SHAPE
    assert run(x0_stride=-1) == A.HK_ERR_SHAPE and run(k1=2, x1_stride=-1) == A.HK_ERR_SHAPE
    assert run(out_stride=2) == A.HK_ERR_SHAPE and ok(x0_stride=0) == A.HK_OK and ok(out_stride=5) == A.HK_OK
    # dtype and flags
    for dtype in (A.HK_F64, A.HK_I32, 9, -1):
        assert run(dtype=dtype) == A.HK_ERR_UNSUPPORTED
    assert run(flags=8) == A.HK_ERR_UNSUPPORTED and run(layer1=dict(flags=2)) == A.HK_ERR_UNSUPPORTED
    assert run(flags=A.HK_MLP_FORCE_TILE_SMALL | A.HK_MLP_FORCE_TILE_LARGE) == A.HK_ERR_UNSUPPORTED
    for flags in (A.HK_MLP_INPUT_RELU, A.HK_MLP_FORCE_TILE_SMALL, A.HK_MLP_FORCE_TILE_LARGE | A.HK_MLP_INPUT_RELU):
        assert ok(flags=flags) == A.HK_OK
    # pointers that are used
    assert run(x0=None) == A.HK_ERR_NULL and run(out=None) == A.HK_ERR_NULL
    assert run(k1=2, x1=None) == A.HK_ERR_NULL and ok(x1=None) == A.HK_OK
    assert run(layer1=dict(weight=None)) == A.HK_ERR_NULL
    assert ok(layer1=dict(bias=None)) == A.HK_OK
    assert run(layer1=dict(bn_mean=None)) == A.HK_ERR_NULL and run(layer1=dict(bn_var=None)) == A.HK_ERR_NULL
    assert ok(layer1=dict(bn_weight=None, bn_bias=None)) == A.HK_OK  # affine=False
    assert ok(bn=False) == A.HK_OK and run(bn=False, layer1=dict(bn_bias=("at", 4096))) == A.HK_ERR_NULL
    assert ok(in_bn=True) == A.HK_OK and run(in_bn=True, in_bn_var=None) == A.HK_ERR_NULL
    assert ok(in_bn=True, in_bn_weight=None, in_bn_bias=None) == A.HK_OK
    # alignment: 4 bytes, every pointer
    for name in ("x0", "out") + _IN_BN:
        assert run(in_bn=True, **{name: ("shift", 2)}) == A.HK_ERR_ALIGN, name
        assert ok(in_bn=True, **{name: ("shift", 4)}) == A.HK_OK, name
    assert run(k1=2, x1=("shift", 1)) == A.HK_ERR_ALIGN
    for name in _LAYER_PTRS:
        assert run(layer1={name: ("shift", 2)}) == A.HK_ERR_ALIGN, name
        assert ok(layer1={name: ("shift", 4)}) == A.HK_OK, name
    # out may share no byte with an input or a parameter: 4 rows of 3 floats are 48 bytes
    for name in ("x0",) + _IN_BN:
        assert run(in_bn=True, **{name: ("at", 0)}) == A.HK_ERR_UNSUPPORTED, name
        assert run(in_bn=True, **{name: ("at", 44)}) == A.HK_ERR_UNSUPPORTED, name
    assert run(k1=2, x1=("at", 44)) == A.HK_ERR_UNSUPPORTED
    assert run(x0=("at", -4 * 4 * 5 + 4)) == A.HK_ERR_UNSUPPORTED
    for name in _LAYER_PTRS:
        assert run(layer1={name: ("at", 44)}) == A.HK_ERR_UNSUPPORTED, name
    assert run(layer1=dict(weight=("at", -4 * 21 + 4))) == A.HK_ERR_UNSUPPORTED  # layer 1's weight: 3 x 7 floats
    assert run(layer1=dict(bias=("at", -12 + 4))) == A.HK_ERR_UNSUPPORTED
    # records: out and x0 as columns of rows of one stride have to keep apart inside a record (k0 = 5, n = 3)
    rec = dict(x0_stride=16, out_stride=16)
    assert run(x0=("at", -4 * 4), **rec) == A.HK_ERR_UNSUPPORTED  # out begins on x0's last element
    assert run(x0=("at", -4 * 14), **rec) == A.HK_ERR_UNSUPPORTED  # out runs into the next record's x0
    assert run(x0=("at", 4 * 2), **rec) == A.HK_ERR_UNSUPPORTED  # x0 begins on out's last element
    # (ranges that only touch are accepted: test_gpu_mlp.py runs views of one storage side by side)


def test_mlp_row_span_beyond_63_bits_is_refused():
    """two rows 2^62 floats apart span 2^64 bytes: refused as a shape, where the spans are first computed (after the
    pointer and alignment checks), not wrapped into a span that passes the overlap check"""
    L = _lib.lib()
    run = lambda **kw: L.hk_mlp_forward(ctypes.byref(_desc(batch=2, **kw)), None)  # noqa: E731
    assert run(x0_stride=1 << 62) == A.HK_ERR_SHAPE
    assert run(out_stride=1 << 62) == A.HK_ERR_SHAPE
    assert run(x0_stride=1 << 62, out_stride=1 << 62) == A.HK_ERR_SHAPE
    assert run(x0_stride=1 << 62, out=None) == A.HK_ERR_NULL and run(x0_stride=1 << 62, x0=("shift", 2)) == A.HK_ERR_ALIGN
