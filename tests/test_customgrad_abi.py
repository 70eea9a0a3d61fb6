"""CPU-side checks of the boundary of hk_customgrad_forward / hk_customgrad_backward (include/hironaka_hip_customgrad.h):
the library exports them, the python mirror of the header agrees with it, and bad arguments are refused on the host, before
any launch."""
import ctypes
import os
import re
import subprocess

import abi_cases
from conftest import ROOT
from hironaka_amd import _abi as A
from hironaka_amd import _lib

HEADER = "hironaka_hip_customgrad.h"
ENTRIES = {"hk_customgrad_forward", "hk_customgrad_backward", "hk_customgrad_workspace_bytes"}


def test_library_exports_the_customgrad_entry_points():
    _lib.build()
    declared = abi_cases.declared(HEADER)
    assert declared == set(A.CUSTOMGRAD_PROTOTYPES) == ENTRIES
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r"\bT (hk_customgrad_\w+)", exported)) == declared  # exactly what the header declares
    text = abi_cases.header()
    assert text.index('#include "hironaka_hip_pvgrad.h"') < text.index('#include "hironaka_hip_customgrad.h"')
    assert not re.search(r"#define\s+HK_CUSTOMGRAD_", text)  # the feature's defines live in its own header
    assert _lib.lib().hk_abi_version() == A.HK_ABI_VERSION == 6
    for name in ENTRIES:
        assert getattr(_lib.lib(), name).argtypes == A.CUSTOMGRAD_PROTOTYPES[name][1], name  # bound by default
    with open(os.path.join(ROOT, "hironaka_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SINGLES :=.*\bcustomgrad\b", f.read(), flags=re.M)


def test_customgrad_constants_match_header():
    text = abi_cases.header(HEADER)
    defines = re.findall(r"#define\s+(HK_\w+)\s+\(?(-?\d+)\)?u?\s", text)
    assert len(defines) == 4 and all(name.startswith("HK_CUSTOMGRAD_") for name, _ in defines)
    for name, value in defines:
        assert getattr(A, name) == int(value), name
    assert A.HK_CUSTOMGRAD_NONE < 0
    # first[c] and R_c for c = 0 .. 64 fit the header's words
    assert A.HK_CUSTOMGRAD_FIRST + A.HK_CUSTOMNET_MAX_POINTS + 1 <= A.HK_CUSTOMGRAD_SIZE
    assert A.HK_CUSTOMGRAD_SIZE + A.HK_CUSTOMNET_MAX_POINTS + 1 <= A.HK_CUSTOMGRAD_HEADER and A.HK_CUSTOMGRAD_HEADER % 4 == 0
    assert ctypes.sizeof(A.hk_customgrad_dense) == 32 and ctypes.sizeof(A.hk_customgrad_block) == 96
    assert ctypes.sizeof(A.hk_customgrad_desc) == ctypes.sizeof(A.hk_customnet_desc) + 56 + 64 + 8 * A.HK_PVNET_MAX_BLOCKS


def test_customgrad_descriptor_layouts_match_c(tmp_path):
    abi_cases.assert_layouts_match_c({"hk_customgrad_dense": A.hk_customgrad_dense, "hk_customgrad_block": A.hk_customgrad_block,
                                      "hk_customgrad_desc": A.hk_customgrad_desc}, tmp_path)


_NET_PTRS = ("x", "policy", "value", "towers", "policy_weight", "policy_bias", "value_weight", "value_bias", "workspace")
_TOP_PTRS = ("grad_table", "grads", "grad_policy", "grad_value")
REGION = 512 * 1024  # more than any array of the cases below
R, D = A.HK_PVNET_RESIDUE, A.HK_PVNET_DENSE


def _desc(spec=(5, 3, 3), widths=(64, 32), kinds=None, batch=4, actions=3, net=None, top=None, heads=None):
    """a CustomNet of the shape, every array a region of its own of one host block.  `net` changes fields of the
    hk_customnet_desc, `top` of the descriptor itself, `heads` = {"policy" / "value": {field: offset}}.  ("shift", bytes)
    moves a pointer, ("at", name, bytes) points it at the region of that name.  workspace_bytes is what the library asks for
    unless `net` says otherwise.  (The pointers are the host's: every call below returns before a launch.)"""
    m, d, e = spec
    buf = (ctypes.c_char * (REGION * (len(_NET_PTRS) + len(_TOP_PTRS) + 1)))()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    g = A.hk_customgrad_desc()
    q = g.net
    where = {}
    for i, name in enumerate(_NET_PTRS + _TOP_PTRS):
        where[name] = base + i * REGION
        setattr(q if name in _NET_PTRS else g, name, where[name])
    q.batch, q.m, q.d, q.e, q.nblocks, q.n_last, q.actions, q.dtype = batch, m, d, e, len(widths), widths[-1], actions, A.HK_F32
    q.x_stride, q.policy_stride, q.value_stride = m * d + e, actions, 1
    g.grad_policy_stride, g.grad_value_stride = actions, 1
    for l, n in enumerate(widths):
        g.n[l], g.kind[l] = n, R if kinds is None else kinds[l]
    kh = widths[-1] + e
    g.policy.d_weight, g.policy.d_bias, g.value.d_weight, g.value.d_bias = 0, actions * kh, actions * kh + actions, actions * kh + actions + kh
    g.grad_floats = actions * kh + actions + kh + 1
    for head in (g.policy, g.value):
        head.d_gn_scale = head.d_gn_bias = A.HK_CUSTOMGRAD_NONE

    def change(obj, fields):
        for name, v in fields.items():
            if isinstance(v, tuple) and v[0] == "shift":
                v = getattr(obj, name) + v[1]
            elif isinstance(v, tuple) and v[0] == "at":
                v = where[v[1]] + v[2]
            setattr(obj, name, v)
    for head, fields in (heads or {}).items():
        change(getattr(g, head), fields)
    q.workspace_bytes = _lib.lib().hk_customgrad_workspace_bytes(ctypes.byref(g))
    change(g, top or {})
    change(q, net or {})
    g._keep = buf
    return g


def test_workspace_bytes():
    L = _lib.lib()
    need = lambda **kw: L.hk_customgrad_workspace_bytes(ctypes.byref(_desc(**kw)))  # noqa: E731
    assert L.hk_customgrad_workspace_bytes(None) == 0 and need(batch=0) == 0 and need(batch=-1) == 0
    assert need(net=dict(nblocks=0)) == 0 and need(net=dict(nblocks=33)) == 0 and need(actions=0) == 0
    assert need(spec=(65, 2, 0)) == 0 and need(spec=(5, 1, 0)) == 0 and need(widths=(64, 48)) == 0
    assert need(batch=A.HK_PVGRAD_MAX_BATCH + 1) == 0 and need(net=dict(n_last=64)) == 0

    def words(batch, m, kin, arrays, kh, actions):
        ints = A.HK_CUSTOMGRAD_HEADER + 4 * (-(-batch // 16) + m + 1) + (batch + 3) // 4 * 4
        return (4 * (ints + batch * (kin + arrays + kh + actions + 1)) + 15) // 16 * 16
    # ? -> 64 (the first block always has a projection's arrays: 13), 64 -> 32 (13), z [4, 35], dzh [4, 4]
    assert need() == words(4, 5, 18, 13 * 64 + 13 * 32, 35, 3)
    # 64 -> 64 has no projection: 10 arrays; dense blocks have 2
    assert need(widths=(64, 64), batch=21) == words(21, 5, 18, 13 * 64 + 10 * 64, 67, 3)
    assert need(spec=(64, 2, 0), widths=(17, 33), kinds=(D, D), batch=70, actions=9) == words(70, 64, 128, 2 * (17 + 33), 33, 9)


def test_customgrad_validation_without_gpu():
    L = _lib.lib()
    fwd, bwd = L.hk_customgrad_forward, L.hk_customgrad_backward
    run = lambda fn, **kw: fn(ctypes.byref(_desc(**kw)), None)  # noqa: E731
    # what is accepted is asked with batch=0 (HK_OK comes after every other check): a batch > 0 that passes would launch
    ok = lambda fn, **kw: fn(ctypes.byref(_desc(batch=0, **kw)), None)  # noqa: E731
    for fn in (fwd, bwd):
        assert fn(None, None) == A.HK_ERR_NULL
        assert ok(fn) == A.HK_OK and ok(fn, spec=(64, 2, 0), widths=(32,), kinds=(D,)) == A.HK_OK
        assert ok(fn, spec=(1, 2, 0), widths=(256,) * 32) == A.HK_OK and ok(fn, net=dict(flags=A.HK_CUSTOMNET_RAW_VALUE)) == A.HK_OK
        # everything hk_customnet_forward refuses, with its code
        assert run(fn, net=dict(dtype=A.HK_F64)) == A.HK_ERR_UNSUPPORTED and run(fn, net=dict(flags=8)) == A.HK_ERR_UNSUPPORTED
        assert run(fn, spec=(5, 1, 0)) == A.HK_ERR_SHAPE and run(fn, spec=(65, 2, 0)) == A.HK_ERR_SHAPE
        assert run(fn, spec=(5, 3, -1)) == A.HK_ERR_SHAPE and run(fn, spec=(64, 4, 1)) == A.HK_ERR_SHAPE
        assert run(fn, net=dict(nblocks=0)) == A.HK_ERR_SHAPE and run(fn, net=dict(nblocks=33)) == A.HK_ERR_SHAPE
        assert run(fn, actions=0) == A.HK_ERR_SHAPE and run(fn, actions=256) == A.HK_ERR_SHAPE and run(fn, batch=-1) == A.HK_ERR_SHAPE
        assert run(fn, net=dict(x_stride=-1)) == A.HK_ERR_SHAPE and run(fn, net=dict(policy_stride=2)) == A.HK_ERR_SHAPE
        assert run(fn, net=dict(value_stride=0)) == A.HK_ERR_SHAPE
        for name in ("x", "policy", "value", "towers", "policy_weight", "value_weight", "workspace"):
            assert run(fn, net={name: None}) == A.HK_ERR_NULL, name
        for name in ("x", "policy", "value", "policy_weight", "policy_bias", "value_weight", "value_bias"):
            assert run(fn, net={name: ("shift", 2)}) == A.HK_ERR_ALIGN, name
        assert run(fn, net=dict(towers=("shift", 4))) == A.HK_ERR_ALIGN and run(fn, net=dict(workspace=("shift", 8))) == A.HK_ERR_ALIGN
        # this header's own: a gate, either FORCE flag, the widths and kinds, the batch, the workspace
        assert run(fn, net=dict(gate=("at", "x", 0))) == A.HK_ERR_UNSUPPORTED
        for flag in (A.HK_CUSTOMNET_FORCE_TILE_SMALL, A.HK_CUSTOMNET_FORCE_TILE_LARGE | A.HK_CUSTOMNET_RAW_VALUE):
            assert run(fn, net=dict(flags=flag)) == A.HK_ERR_UNSUPPORTED, flag
        assert run(fn, widths=(0, 32)) == A.HK_ERR_SHAPE and run(fn, widths=(257, 32)) == A.HK_ERR_SHAPE
        assert run(fn, widths=(48, 32)) == A.HK_ERR_SHAPE and ok(fn, widths=(48, 32), kinds=(D, R)) == A.HK_OK
        assert run(fn, kinds=(R, 7)) == A.HK_ERR_SHAPE and run(fn, net=dict(n_last=64)) == A.HK_ERR_SHAPE
        assert run(fn, batch=A.HK_PVGRAD_MAX_BATCH + 1) == A.HK_ERR_SHAPE
        need = L.hk_customgrad_workspace_bytes(ctypes.byref(_desc()))
        assert run(fn, net=dict(workspace_bytes=need - 1)) == A.HK_ERR_SHAPE and run(fn, net=dict(workspace_bytes=0)) == A.HK_ERR_SHAPE
        assert ok(fn, net=dict(workspace_bytes=1 << 40)) == A.HK_OK
        # the workspace may share no byte with anything read, nor with another thing written
        for name in ("x", "policy_weight", "value_bias", "towers", "policy", "value"):
            assert run(fn, net=dict(workspace=("at", name, 0))) == A.HK_ERR_UNSUPPORTED, name
        assert run(fn, net=dict(x=("at", "workspace", need - 4))) == A.HK_ERR_UNSUPPORTED  # x's first float on its last
        # two rows 2^62 floats apart span 2^64 bytes
        assert run(fn, batch=2, net=dict(x_stride=1 << 62)) == A.HK_ERR_SHAPE
    # the forward looks at no gradient, at neither table nor buffer, at neither grad_policy nor grad_value
    assert ok(fwd, top=dict(grad_table=None, grads=None, grad_policy=None, grad_value=None, grad_policy_stride=0,
                            grad_value_stride=0, grad_floats=0)) == A.HK_OK
    assert ok(fwd, heads=dict(policy=dict(d_weight=A.HK_CUSTOMGRAD_NONE))) == A.HK_OK
    # the backward's own
    for name in _TOP_PTRS:
        assert run(bwd, top={name: None}) == A.HK_ERR_NULL, name
    assert run(bwd, top=dict(grad_policy_stride=2)) == A.HK_ERR_SHAPE and run(bwd, top=dict(grad_value_stride=0)) == A.HK_ERR_SHAPE
    assert ok(bwd, top=dict(grad_policy_stride=7, grad_value_stride=5)) == A.HK_OK
    assert run(bwd, batch=2, top=dict(grad_policy_stride=1 << 62)) == A.HK_ERR_SHAPE
    for head in ("policy", "value"):
        assert run(bwd, heads={head: dict(d_weight=A.HK_CUSTOMGRAD_NONE)}) == A.HK_ERR_NULL, head
        assert ok(bwd, heads={head: dict(d_bias=A.HK_CUSTOMGRAD_NONE)}) == A.HK_OK, head
    assert run(bwd, top=dict(grad_table=("shift", 4))) == A.HK_ERR_ALIGN
    for name in ("grads", "grad_policy", "grad_value"):
        assert run(bwd, top={name: ("shift", 2)}) == A.HK_ERR_ALIGN and ok(bwd, top={name: ("shift", 4)}) == A.HK_OK
    # a head's gradient ends inside the buffer
    floats = _desc().grad_floats
    assert run(bwd, top=dict(grad_floats=floats - 1)) == A.HK_ERR_SHAPE and run(bwd, heads=dict(value=dict(d_bias=floats))) == A.HK_ERR_SHAPE
    assert run(bwd, heads=dict(policy=dict(d_weight=floats))) == A.HK_ERR_SHAPE
    # the gradient buffer may share no byte with anything read, nor with the workspace
    for name in ("x", "value", "policy", "grad_policy", "grad_value", "policy_weight", "towers", "grad_table", "workspace"):
        assert run(bwd, top=dict(grads=("at", name, 0))) == A.HK_ERR_UNSUPPORTED, name
    assert run(bwd, top=dict(grads=("at", "x", -4 * floats + 4))) == A.HK_ERR_UNSUPPORTED  # its last float on x's first
