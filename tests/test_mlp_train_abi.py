"""CPU-side checks of the boundary of hk_train_mlp_forward / hk_train_mlp_backward (include/hironaka_hip_mlp_train.h):
the library exports them, the python mirror of the header agrees with it, and bad arguments are refused on the host,
before any launch."""
import ctypes
import os
import re
import subprocess

import abi_cases
from conftest import ROOT
from hironaka_amd import _abi as A
from hironaka_amd import _lib

NAMES = {"hk_train_mlp_rows", "hk_train_mlp_workspace_bytes", "hk_train_mlp_forward", "hk_train_mlp_backward"}


def _header():
    return abi_cases.header("hironaka_hip_mlp_train.h")


def test_library_exports_the_entry_points():
    _lib.build()
    declared = abi_cases.declared("hironaka_hip_mlp_train.h")
    assert declared == set(A.MLP_TRAIN_PROTOTYPES) == NAMES
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r"\bT (hk_train_\w+)", exported)) == declared  # exactly what the header declares
    text = abi_cases.header()
    assert text.index('#include "hironaka_hip_mlp.h"') < text.index('#include "hironaka_hip_mlp_train.h"')
    assert _lib.lib().hk_abi_version() == A.HK_ABI_VERSION == 6
    assert _lib.lib().hk_train_mlp_backward.argtypes == A.MLP_TRAIN_PROTOTYPES["hk_train_mlp_backward"][1]  # bound by default
    with open(os.path.join(ROOT, "hironaka_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SINGLES :=.*\bmlp_train\b", f.read(), flags=re.M)


def test_constants_match_header():
    defines = dict(re.findall(r"#define\s+(HK_\w+)\s+(\d+)u?\s", _header()))
    assert set(defines) == {"HK_MLP_TRAIN_MAX_BATCH", "HK_MLP_TRAIN_ROWS_SMALL", "HK_MLP_TRAIN_BN"}
    for name, value in defines.items():
        assert getattr(A, name) == int(value), name
    assert 256 <= A.HK_MLP_TRAIN_ROWS_SMALL <= A.HK_MLP_TRAIN_MAX_BATCH == 1024  # never below the reference's fit batch
    assert not A.HK_MLP_TRAIN_BN & A.HK_MLP_RELU
    L = _lib.lib()
    for batch in (0, 1, A.HK_MLP_TRAIN_ROWS_SMALL):
        assert L.hk_train_mlp_rows(batch) == A.HK_MLP_TRAIN_ROWS_SMALL
    assert L.hk_train_mlp_rows(A.HK_MLP_TRAIN_ROWS_SMALL + 1) == L.hk_train_mlp_rows(A.HK_MLP_TRAIN_MAX_BATCH) == 1024


def test_descriptor_layouts_match_c(tmp_path):
    """sizeof/offsetof as the C compiler sees them (gcc on the header, as C) == ctypes"""
    abi_cases.assert_layouts_match_c({"hk_mlp_train_layer": A.hk_mlp_train_layer,
                                      "hk_mlp_train_desc": A.hk_mlp_train_desc}, tmp_path)
    assert ctypes.sizeof(A.hk_mlp_train_layer) == 144


_READ = ("weight", "bias", "bn_weight", "bn_bias")
_FWD_OUT = ("running_mean", "running_var", "num_batches_tracked", "z", "act", "mean", "inv")
_BWD_OUT = ("d_weight", "d_bias", "d_bn_weight", "d_bn_bias")
_PTRS = _READ + _FWD_OUT + _BWD_OUT
_BN_ONLY = ("bn_weight", "bn_bias", "running_mean", "running_var", "num_batches_tracked", "d_bn_weight", "d_bn_bias")


def _desc(widths=(5, 7, 3), batch=4, k1=0, bn=True, layer1=None, **top):
    """a net of the given widths, every array a region of its own of one host block; `layer1` changes layer 1, `top` the
    descriptor's own fields; ("shift", bytes) moves a pointer, ("of", field, bytes) points it into layer 1's `field`,
    ("x0", bytes) into x0.  (The pointers are the host's: every call below returns before a launch.)"""
    region = 1024 * 1024 + 4096  # more than 1024 x 256 floats
    buf = (ctypes.c_char * (region * (5 + len(_PTRS) * (len(widths) - 1))))()
    at = (ctypes.addressof(buf) + 63) // 64 * 64
    d = A.hk_mlp_train_desc()
    d.x0, d.x1, d.grad_out, d.workspace = at, (at + region if k1 else None), at + 2 * region, at + 3 * region
    d.k0, d.k1, d.batch, d.nlayers, d.dtype = widths[0] - k1, k1, batch, len(widths) - 1, A.HK_F32
    d.x0_stride, d.x1_stride, d.grad_stride = widths[0] - k1, k1, widths[-1]
    for i in range(len(widths) - 1):
        e = d.layer[i]
        for j, name in enumerate(_PTRS):
            keep = bn or name in ("weight", "bias", "act", "d_weight", "d_bias")
            setattr(e, name, at + (5 + len(_PTRS) * i + j) * region if keep else None)
        e.k, e.n, e.eps, e.momentum = widths[i], widths[i + 1], 1e-5, 0.1
        e.flags = (A.HK_MLP_RELU if i + 2 < len(widths) else 0) | (A.HK_MLP_TRAIN_BN if bn else 0)
    d.workspace_bytes = 2 * region

    def change(obj, fields):
        for name, v in fields.items():
            if isinstance(v, tuple) and v[0] == "shift":
                v = getattr(obj, name) + v[1]
            elif isinstance(v, tuple) and v[0] == "of":
                v = getattr(d.layer[1], v[1]) + v[2]
            elif isinstance(v, tuple) and v[0] == "x0":
                v = d.x0 + v[1]
            setattr(obj, name, v)
    change(d.layer[1], layer1 or {})
    change(d, top)
    d._keep = buf
    return d


def test_workspace_bytes():
    L = _lib.lib()
    ws = lambda **kw: L.hk_train_mlp_workspace_bytes(ctypes.byref(_desc(**kw)))  # noqa: E731
    assert L.hk_train_mlp_workspace_bytes(None) == 0
    assert ws() == 2 * 4 * 3 * 4  # dz of two consecutive layers: the widest output behind the first layer
    assert ws(widths=(5, 256, 9, 3), batch=1024) == 2 * 1024 * 9 * 4
    assert ws(widths=(5, 3)) == 0 and ws(batch=0) == 0


def test_validation_without_gpu():
    L = _lib.lib()
    for entry, backward in ((L.hk_train_mlp_forward, False), (L.hk_train_mlp_backward, True)):
        run = lambda **kw: entry(ctypes.byref(_desc(**kw)), None)  # noqa: E731
        # what is accepted is asked with batch=0 (HK_OK comes after every other check): a batch > 0 that passes would launch
        ok = lambda **kw: entry(ctypes.byref(_desc(batch=0, **kw)), None)  # noqa: E731
        assert entry(None, None) == A.HK_ERR_NULL
        assert ok() == A.HK_OK and ok(k1=2) == A.HK_OK and ok(bn=False) == A.HK_OK
        assert ok(widths=(256,) * 33) == A.HK_OK and ok(widths=(1, 1)) == A.HK_OK
        assert ok(x0=None) == A.HK_ERR_NULL and ok(dtype=A.HK_F64) == A.HK_ERR_UNSUPPORTED
        # counts and widths
        assert run(batch=-1) == A.HK_ERR_SHAPE and run(batch=A.HK_MLP_TRAIN_MAX_BATCH + 1) == A.HK_ERR_SHAPE
        assert run(batch=1) == A.HK_ERR_SHAPE  # a batch norm over one row
        assert run(batch=A.HK_MLP_TRAIN_MAX_BATCH + 1, bn=False) == A.HK_ERR_SHAPE
        assert run(nlayers=0) == A.HK_ERR_SHAPE and run(nlayers=33) == A.HK_ERR_SHAPE and run(nlayers=-1) == A.HK_ERR_SHAPE
        assert run(widths=(257, 3)) == A.HK_ERR_SHAPE and run(widths=(3, 257)) == A.HK_ERR_SHAPE
        assert run(layer1=dict(k=0)) == A.HK_ERR_SHAPE and run(layer1=dict(n=0)) == A.HK_ERR_SHAPE
        assert run(layer1=dict(k=6)) == A.HK_ERR_SHAPE
        assert run(k0=4) == A.HK_ERR_SHAPE and run(k0=0) == A.HK_ERR_SHAPE and ok(k1=1) == A.HK_OK
        assert run(k1=-1, k0=6) == A.HK_ERR_SHAPE
        assert run(x0_stride=-1) == A.HK_ERR_SHAPE and run(k1=2, x1_stride=-1) == A.HK_ERR_SHAPE
        assert ok(x0_stride=0) == A.HK_OK
        # dtype and flags
        for dtype in (A.HK_F64, A.HK_I32, 9, -1):
            assert run(dtype=dtype) == A.HK_ERR_UNSUPPORTED
        assert run(flags=2) == A.HK_ERR_UNSUPPORTED and run(layer1=dict(flags=4)) == A.HK_ERR_UNSUPPORTED
        assert ok(flags=A.HK_MLP_INPUT_RELU) == A.HK_OK
        # pointers that are used
        assert run(x0=None) == A.HK_ERR_NULL and run(k1=2, x1=None) == A.HK_ERR_NULL and ok(x1=None) == A.HK_OK
        for name in ("weight", "act", "z", "mean", "inv", "running_mean", "running_var"):
            assert run(layer1={name: None}) == A.HK_ERR_NULL, name
        for name in ("bias", "bn_weight", "bn_bias", "num_batches_tracked", "d_bias", "d_bn_weight", "d_bn_bias"):
            assert ok(layer1={name: None}) == A.HK_OK, name
        assert ok(bn=False, layer1=dict(z=None, mean=None, inv=None)) == A.HK_OK
        # a batch norm's pointers without the flag
        for name in _BN_ONLY:
            assert run(bn=False, layer1={name: ("x0", 1 << 19)}) == A.HK_ERR_UNSUPPORTED, name
        # alignment: 4 bytes, every pointer; the counter 8
        for name in ("x0", "grad_out", "workspace"):
            assert run(**{name: ("shift", 2)}) == A.HK_ERR_ALIGN, name
            assert ok(**{name: ("shift", 4)}) == A.HK_OK, name
        assert run(k1=2, x1=("shift", 1)) == A.HK_ERR_ALIGN
        for name in _PTRS:
            assert run(layer1={name: ("shift", 2)}) == A.HK_ERR_ALIGN, name
            assert ok(layer1={name: ("shift", 8)}) == A.HK_OK, name
        assert run(layer1=dict(num_batches_tracked=("shift", 4))) == A.HK_ERR_ALIGN
        # what is written shares no byte with what is read or with something else that is written
        # (layer 1: 3 x 7 weights, vectors of 3, 4 rows of 3 floats)
        written = _BWD_OUT if backward else _FWD_OUT
        for name in written:
            for target, off in (("weight", 4 * 20), ("bias", 8), ("bn_weight", 0), ("bn_bias", 8)):
                assert run(layer1={name: ("of", target, off)}) == A.HK_ERR_UNSUPPORTED, (name, target)
            assert run(layer1={name: ("x0", 4 * 18)}) == A.HK_ERR_UNSUPPORTED, name  # x0: 4 rows of 5 floats
            other = next(o for o in written if o != name)
            assert run(layer1={name: ("of", other, 0)}) == A.HK_ERR_UNSUPPORTED, (name, other)
        if backward:
            assert run(grad_out=None) == A.HK_ERR_NULL and run(workspace=None) == A.HK_ERR_NULL
            assert ok(widths=(5, 3), workspace=None) == A.HK_OK  # one layer: nothing is handed down
            assert run(layer1=dict(d_weight=None)) == A.HK_ERR_NULL
            assert run(grad_stride=-1) == A.HK_ERR_SHAPE and ok(grad_stride=0) == A.HK_OK
            assert run(workspace_bytes=2 * 4 * 3 * 4 - 1) == A.HK_ERR_SHAPE
            for name in ("act", "z", "mean", "inv"):  # the saved tensors are read now
                assert run(layer1=dict(d_bias=("of", name, 0))) == A.HK_ERR_UNSUPPORTED, name
            assert run(workspace=("x0", 0)) == A.HK_ERR_UNSUPPORTED
            assert run(layer1=dict(d_weight=("of", "weight", 0))) == A.HK_ERR_UNSUPPORTED
        else:
            assert ok(grad_out=None, workspace=None, workspace_bytes=0) == A.HK_OK  # the backward's alone
            assert ok(layer1=dict(d_weight=None)) == A.HK_OK


def test_row_span_beyond_63_bits_is_refused():
    """two rows 2^62 floats apart span 2^64 bytes: refused as a shape, where the spans are first computed (after the
    pointer and alignment checks), not wrapped into a span that passes the overlap check"""
    L = _lib.lib()
    for entry, backward in ((L.hk_train_mlp_forward, False), (L.hk_train_mlp_backward, True)):
        run = lambda **kw: entry(ctypes.byref(_desc(batch=2, **kw)), None)  # noqa: E731
        assert run(x0_stride=1 << 62) == A.HK_ERR_SHAPE
        assert run(x0_stride=1 << 62, x0=None) == A.HK_ERR_NULL and run(x0_stride=1 << 62, x0=("shift", 2)) == A.HK_ERR_ALIGN
        if backward:
            assert run(grad_stride=1 << 62) == A.HK_ERR_SHAPE
            assert run(x0_stride=1 << 62, grad_stride=1 << 62) == A.HK_ERR_SHAPE
