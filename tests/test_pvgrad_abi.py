"""CPU-side checks of the boundary of hk_pvgrad_forward / hk_pvgrad_backward (include/hironaka_hip_pvgrad.h): the library
exports them, the python mirror of the header agrees with it, and bad arguments are refused on the host, before any launch."""
import ctypes
import os
import re
import subprocess

import abi_cases
from conftest import ROOT
from hironaka_amd import _abi as A
from hironaka_amd import _lib

HEADER = "hironaka_hip_pvgrad.h"
ENTRIES = {"hk_pvgrad_forward", "hk_pvgrad_backward", "hk_pvgrad_workspace_bytes"}


def test_library_exports_the_pvgrad_entry_points():
    _lib.build()
    declared = abi_cases.declared(HEADER)
    assert declared == set(A.PVGRAD_PROTOTYPES) == ENTRIES
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r"\bT (hk_pvgrad_\w+)", exported)) == declared  # exactly what the header declares
    text = abi_cases.header()
    assert text.index('#include "hironaka_hip_pvloss.h"') < text.index('#include "hironaka_hip_pvgrad.h"')
    assert not re.search(r"#define\s+HK_PVGRAD_", text)  # the feature's defines live in its own header
    assert not re.search(r"#define\s+HK_PVGRAD_", abi_cases.header("hironaka_hip_pvnet.h"))
    assert _lib.lib().hk_abi_version() == A.HK_ABI_VERSION == 6
    for name in ENTRIES:
        assert getattr(_lib.lib(), name).argtypes == A.PVGRAD_PROTOTYPES[name][1], name  # bound by default
    with open(os.path.join(ROOT, "hironaka_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SINGLES :=.*\bpvgrad\b", f.read(), flags=re.M)


def test_pvgrad_constants_match_header():
    defines = re.findall(r"#define\s+(HK_\w+)\s+(\d+)u?\s", abi_cases.header(HEADER))
    assert len(defines) == 2 and all(name.startswith("HK_PVGRAD_") for name, _ in defines)
    for name, value in defines:
        assert getattr(A, name) == int(value), name
    assert A.HK_PVGRAD_MAX_BATCH == A.HK_MLP_TILE_CROSSOVER
    assert ctypes.sizeof(A.hk_pvgrad_dense) == 32 and ctypes.sizeof(A.hk_pvgrad_block) == 96
    assert ctypes.sizeof(A.hk_pvgrad_desc) == ctypes.sizeof(A.hk_pvnet_desc) + 48 + 64 + 96 * A.HK_PVNET_MAX_BLOCKS
    # the launches the header promises: [n] x 8 needs one for the parameters, 32 projecting blocks three
    per = A.HK_PVGRAD_TABLE
    assert -(-(16 + 2) // per) == 1 and -(-(96 + 2) // per) == 3


def test_pvgrad_descriptor_layouts_match_c(tmp_path):
    abi_cases.assert_layouts_match_c({"hk_pvgrad_dense": A.hk_pvgrad_dense, "hk_pvgrad_block": A.hk_pvgrad_block,
                                      "hk_pvgrad_desc": A.hk_pvgrad_desc}, tmp_path)


_DENSE_PTRS = ("weight", "bias", "gn_scale", "gn_bias")
_GRAD_PTRS = ("d_weight", "d_bias", "d_gn_scale", "d_gn_bias")
_NET_PTRS = ("x", "policy", "value", "policy_weight", "policy_bias", "value_weight", "value_bias")
_TOP_PTRS = ("grad_policy", "grad_value", "workspace")
REGION = 512 * 1024  # more than 256 x 256 floats


def _desc(widths=(18, 64, 64, 32), kinds=None, batch=4, actions=3, net=None, top=None, grad=None, dense=None, ws_region=16):
    """a net of the given widths (residue blocks unless `kinds` says otherwise), every array a region of its own of one host
    block.  `net` changes fields of the hk_pvnet_desc, `top` of the descriptor itself, `grad` = (block or "policy" / "value",
    which, {field: value}) a gradient table's entry, `dense` = (block, which, {field: value}) a Dense of the net.  ("shift",
    bytes) moves a pointer, ("at", name, bytes) points it at the region of that name (a field of the net, of the descriptor,
    or "g:block:which:field").  workspace_bytes is what the library asks for unless `top` says otherwise.  (The pointers are
    the host's: every call below returns before a launch.)"""
    nblocks = len(widths) - 1
    regions = 7 + 3 + ws_region + 8 + 24 * nblocks
    buf = (ctypes.c_char * (REGION * (regions + 1)))()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    g = A.hk_pvgrad_desc()
    d = g.net
    where, at = {}, [0]

    def region(name, count=1):
        where[name] = base + at[0] * REGION
        at[0] += count
        return where[name]

    for name in _NET_PTRS:
        setattr(d, name, region(name))
    for name in _TOP_PTRS:
        setattr(g, name, region(name, ws_region if name == "workspace" else 1))
    for head in ("policy", "value"):
        for name in _GRAD_PTRS:
            setattr(getattr(g, head), name, region(f"g:{head}::{name}"))
    d.k0, d.batch, d.nblocks, d.actions, d.dtype = widths[0], batch, nblocks, actions, A.HK_F32
    d.x_stride, d.policy_stride, d.value_stride = widths[0], actions, 1
    g.grad_policy_stride, g.grad_value_stride = actions, 1
    for i in range(nblocks):
        e = d.block[i]
        e.k, e.n, e.eps = widths[i], widths[i + 1], 1e-6
        e.kind = A.HK_PVNET_RESIDUE if kinds is None else kinds[i]
        for w, which in enumerate(("dense1", "dense2", "proj")):
            used = w == 0 or (e.kind == A.HK_PVNET_RESIDUE and (w == 1 or e.k != e.n))
            for name, gname in zip(_DENSE_PTRS, _GRAD_PTRS):
                setattr(getattr(e, which), name, region(f"n:{i}:{which}:{name}") if used else None)
                setattr(getattr(g.block[i], which), gname, region(f"g:{i}:{which}:{gname}") if used else None)
    assert at[0] <= regions

    def change(obj, fields):
        for name, v in fields.items():
            if isinstance(v, tuple) and v[0] == "shift":
                v = getattr(obj, name) + v[1]
            elif isinstance(v, tuple) and v[0] == "at":
                v = (where[v[1]] if v[1] in where else getattr(d, v[1])) + v[2]
            setattr(obj, name, v)
    if dense:
        change(getattr(d.block[dense[0]], dense[1]), dense[2])
    if grad:
        change(getattr(g, grad[0]) if grad[1] is None else getattr(g.block[grad[0]], grad[1]), grad[2])
    change(d, net or {})
    g.workspace_bytes = _lib.lib().hk_pvgrad_workspace_bytes(ctypes.byref(g))
    change(g, top or {})
    g._keep = buf
    return g


def test_workspace_bytes():
    L = _lib.lib()
    need = lambda **kw: L.hk_pvgrad_workspace_bytes(ctypes.byref(_desc(**kw)))  # noqa: E731
    assert L.hk_pvgrad_workspace_bytes(None) == 0 and need(batch=0) == 0 and need(batch=-1) == 0
    assert need(net=dict(nblocks=0)) == 0 and need(net=dict(nblocks=33)) == 0 and need(actions=0) == 0
    # 18 -> 64 (a projection: 13 arrays), 64 -> 64 (10), 64 -> 32 (13), and dzh [4, actions + 1]
    assert need() == 4 * (4 * (13 * 64 + 10 * 64 + 13 * 32) + 4 * 4)
    D = A.HK_PVNET_DENSE
    assert need(widths=(7, 17, 33), kinds=(D, D), batch=5, actions=9) == 4 * (5 * 2 * (17 + 33) + 5 * 10)


def test_pvgrad_validation_without_gpu():
    L = _lib.lib()
    both = (L.hk_pvgrad_forward, L.hk_pvgrad_backward)
    run = lambda fn, **kw: fn(ctypes.byref(_desc(**kw)), None)  # noqa: E731
    # what is accepted is asked with batch=0 (HK_OK comes after every other check): a batch > 0 that passes would launch
    ok = lambda fn, **kw: fn(ctypes.byref(_desc(batch=0, **kw)), None)  # noqa: E731
    D, R = A.HK_PVNET_DENSE, A.HK_PVNET_RESIDUE
    fwd, bwd = both
    for fn in both:
        assert fn(None, None) == A.HK_ERR_NULL
        assert ok(fn) == A.HK_OK and ok(fn, widths=(256,) * 33) == A.HK_OK and ok(fn, widths=(1, 32)) == A.HK_OK
        assert ok(fn, widths=(1, 1, 17, 256, 33), kinds=(D, D, D, D)) == A.HK_OK
        assert ok(fn, net=dict(flags=A.HK_PVNET_RAW_VALUE)) == A.HK_OK
        # everything hk_pvnet_forward refuses, with its code
        assert run(fn, batch=-1) == A.HK_ERR_SHAPE and run(fn, net=dict(nblocks=0)) == A.HK_ERR_SHAPE
        assert run(fn, net=dict(nblocks=33)) == A.HK_ERR_SHAPE and run(fn, widths=(257, 32)) == A.HK_ERR_SHAPE
        assert run(fn, net=dict(k0=17)) == A.HK_ERR_SHAPE and run(fn, actions=0) == A.HK_ERR_SHAPE
        assert run(fn, net=dict(x_stride=-1)) == A.HK_ERR_SHAPE and run(fn, net=dict(policy_stride=2)) == A.HK_ERR_SHAPE
        assert run(fn, net=dict(value_stride=0)) == A.HK_ERR_SHAPE
        assert run(fn, widths=(18, 48)) == A.HK_ERR_SHAPE and run(fn, widths=(18, 96)) == A.HK_ERR_UNSUPPORTED
        assert run(fn, net=dict(dtype=A.HK_F64)) == A.HK_ERR_UNSUPPORTED and run(fn, net=dict(flags=8)) == A.HK_ERR_UNSUPPORTED
        for name in ("x", "policy", "value", "policy_weight", "value_weight"):
            assert run(fn, net={name: None}) == A.HK_ERR_NULL, name
        assert run(fn, dense=(1, "dense2", dict(weight=None))) == A.HK_ERR_NULL
        assert run(fn, dense=(0, "proj", dict(weight=None))) == A.HK_ERR_NULL
        for name in _NET_PTRS:
            assert run(fn, net={name: ("shift", 2)}) == A.HK_ERR_ALIGN, name
        assert run(fn, dense=(1, "dense1", dict(gn_scale=("shift", 2)))) == A.HK_ERR_ALIGN
        # this header's own: either FORCE flag, the batch, the workspace
        for flag in (A.HK_PVNET_FORCE_TILE_SMALL, A.HK_PVNET_FORCE_TILE_LARGE, A.HK_PVNET_FORCE_TILE_LARGE | A.HK_PVNET_RAW_VALUE):
            assert run(fn, net=dict(flags=flag)) == A.HK_ERR_UNSUPPORTED, flag
        assert run(fn, widths=(3, 32), batch=A.HK_PVGRAD_MAX_BATCH + 1, ws_region=40) == A.HK_ERR_SHAPE
        need = L.hk_pvgrad_workspace_bytes(ctypes.byref(_desc()))
        assert run(fn, top=dict(workspace_bytes=need - 1)) == A.HK_ERR_SHAPE and run(fn, top=dict(workspace_bytes=0)) == A.HK_ERR_SHAPE
        assert ok(fn, top=dict(workspace_bytes=1 << 40)) == A.HK_OK
        assert run(fn, top=dict(workspace=None)) == A.HK_ERR_NULL and ok(fn, top=dict(workspace=None)) == A.HK_ERR_NULL
        assert run(fn, top=dict(workspace=("shift", 2))) == A.HK_ERR_ALIGN and ok(fn, top=dict(workspace=("shift", 4))) == A.HK_OK
        # the workspace may share no byte with anything read, nor with another thing written
        for name in ("x", "policy_weight", "value_bias", "n:0:proj:weight", "n:1:dense2:gn_bias", "n:2:dense1:bias"):
            assert run(fn, top=dict(workspace=("at", name, 0))) == A.HK_ERR_UNSUPPORTED, name
        assert run(fn, net=dict(x=("at", "workspace", need - 4))) == A.HK_ERR_UNSUPPORTED  # x's first float on its last
        assert run(fn, net=dict(x=("at", "workspace", -4 * 4 * 18 + 4))) == A.HK_ERR_UNSUPPORTED
        # two rows 2^62 floats apart span 2^64 bytes
        assert run(fn, batch=2, net=dict(x_stride=1 << 62)) == A.HK_ERR_SHAPE
    # the forward writes policy and value; the backward reads value and does not look at policy
    assert run(fwd, top=dict(workspace=("at", "policy", 0))) == A.HK_ERR_UNSUPPORTED
    assert run(fwd, top=dict(workspace=("at", "value", 0))) == A.HK_ERR_UNSUPPORTED
    assert run(bwd, top=dict(workspace=("at", "value", 0))) == A.HK_ERR_UNSUPPORTED
    # the forward looks at no gradient and at neither grad_policy nor grad_value
    assert ok(fwd, top=dict(grad_policy=None, grad_value=None, grad_policy_stride=0, grad_value_stride=0)) == A.HK_OK
    assert ok(fwd, grad=(1, "dense1", dict(d_weight=None))) == A.HK_OK and ok(fwd, grad=("policy", None, dict(d_weight=2))) == A.HK_OK
    # the backward's own
    assert run(bwd, top=dict(grad_policy=None)) == A.HK_ERR_NULL and run(bwd, top=dict(grad_value=None)) == A.HK_ERR_NULL
    assert run(bwd, top=dict(grad_policy_stride=2)) == A.HK_ERR_SHAPE and run(bwd, top=dict(grad_value_stride=0)) == A.HK_ERR_SHAPE
    assert ok(bwd, top=dict(grad_policy_stride=7, grad_value_stride=5)) == A.HK_OK
    assert run(bwd, batch=2, top=dict(grad_policy_stride=1 << 62)) == A.HK_ERR_SHAPE
    for block, which in ((0, "dense1"), (0, "proj"), (1, "dense2"), ("policy", None), ("value", None)):
        assert run(bwd, grad=(block, which, dict(d_weight=None))) == A.HK_ERR_NULL, (block, which)
        for name in _GRAD_PTRS[1:]:
            assert ok(bwd, grad=(block, which, {name: None})) == A.HK_OK, (block, which, name)
    assert ok(bwd, grad=(1, "proj", dict(d_weight=None))) == A.HK_OK  # block 1 is 64 -> 64: no projection
    assert ok(bwd, widths=(18, 7), kinds=(D,), grad=(0, "dense2", dict(d_weight=2))) == A.HK_OK  # not looked at
    for name in ("grad_policy", "grad_value"):
        assert run(bwd, top={name: ("shift", 2)}) == A.HK_ERR_ALIGN and ok(bwd, top={name: ("shift", 4)}) == A.HK_OK
    for block, which in ((0, "proj"), (1, "dense1"), ("value", None)):
        for name in _GRAD_PTRS[:2] if which is None else _GRAD_PTRS:
            assert run(bwd, grad=(block, which, {name: ("shift", 2)})) == A.HK_ERR_ALIGN, (block, which, name)
            assert ok(bwd, grad=(block, which, {name: ("shift", 4)})) == A.HK_OK, (block, which, name)
    # a gradient may share no byte with anything read, with the workspace or with another gradient
    for target in ("x", "value", "grad_policy", "grad_value", "policy_weight", "n:1:dense1:weight", "n:0:proj:gn_scale",
                   "workspace", "g:1:dense2:d_weight", "g:policy::d_bias"):
        assert run(bwd, grad=(1, "dense1", dict(d_bias=("at", target, 0)))) == A.HK_ERR_UNSUPPORTED, target
        assert run(bwd, grad=("value", None, dict(d_weight=("at", target, 0)))) == A.HK_ERR_UNSUPPORTED, target
    assert run(bwd, grad=(1, "dense1", dict(d_weight=("at", "x", -4 * 64 * 64 + 4)))) == A.HK_ERR_UNSUPPORTED  # last on first
