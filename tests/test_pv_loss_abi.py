"""CPU-side checks of the boundary of hk_pv_loss (include/hironaka_hip_pvloss.h): the library exports it, the python
mirror of the header agrees with it, and bad arguments are refused on the host, before any launch."""
import ctypes
import os
import re

import abi_cases
from conftest import ROOT
from hironaka_amd import _abi as A
from hironaka_amd import _lib


def _header():
    return abi_cases.header("hironaka_hip_pvloss.h")


def test_library_exports_the_pv_loss_entry_points():
    _lib.build()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    declared = abi_cases.declared("hironaka_hip_pvloss.h")
    assert declared == set(A.PVLOSS_PROTOTYPES) == {"hk_pv_loss", "hk_pv_loss_workspace_bytes"}
    for name in declared:
        assert hasattr(handle, name), name
    assert not declared & set(A.PROTOTYPES)
    text = abi_cases.header()
    assert text.index('#include "hironaka_hip_pvnet.h"') < text.index('#include "hironaka_hip_pvloss.h"')
    assert not re.search(r"#define\s+HK_PVLOSS_", text)  # the feature's defines live in its own header
    assert _lib.lib().hk_abi_version() == A.HK_ABI_VERSION == 6
    assert _lib.lib().hk_pv_loss.argtypes == A.PVLOSS_PROTOTYPES["hk_pv_loss"][1]  # bound by default
    with open(os.path.join(ROOT, "hironaka_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SINGLES :=.*\bpvloss\b", f.read(), flags=re.M)


def test_pv_loss_constants_match_header():
    defines = re.findall(r"#define\s+(HK_\w+)\s+(\d+)u?\s", _header())
    assert len(defines) == 3 and all(name.startswith("HK_PVLOSS_") for name, _ in defines)
    for name, value in defines:
        assert getattr(A, name) == int(value), name
    assert 64 % A.HK_PVLOSS_TILE_ROWS == 0  # a wave's share of a tile is a whole number of rows
    assert A.HK_PVLOSS_MAX_ACTIONS == A.HK_PVNET_MAX_WIDTH - 1  # the policy head's range


def test_pv_loss_descriptor_layout_matches_c(tmp_path):
    """sizeof/offsetof as the C compiler sees them (gcc on the header) == ctypes"""
    abi_cases.assert_layouts_match_c({"hk_pv_loss_desc": A.hk_pv_loss_desc}, tmp_path)


def test_workspace_bytes():
    L = _lib.lib()
    R = A.HK_PVLOSS_TILE_ROWS
    assert L.hk_pv_loss_workspace_bytes(-1) == 0
    assert L.hk_pv_loss_workspace_bytes(0) == L.hk_pv_loss_workspace_bytes(1) == L.hk_pv_loss_workspace_bytes(R) == 24
    assert L.hk_pv_loss_workspace_bytes(R + 1) == 32 and L.hk_pv_loss_workspace_bytes(40 * R + 3) == 16 + 41 * 8
    assert L.hk_pv_loss_workspace_bytes(2 ** 31 - 1) == 16 + 8 * (2 ** 31 // R)


_INPUTS = ("logits", "value", "target_policy", "target_value", "weight", "index")
_OUTPUTS = ("dlogits", "dvalue", "row_loss", "loss")
_POINTERS = _INPUTS + _OUTPUTS + ("workspace", "status")
_OPTIONAL = ("weight", "index", "row_loss")


class _Shift(int):
    """move a pointer by this many bytes instead of replacing it"""


class _At(tuple):
    """(field, bytes): the pointer of another field of the same descriptor, moved by so many bytes"""


def _desc(**over):
    """a descriptor that passes every check up to the launch, but for what `over` changes: 4 rows of 3 actions out of 6
    samples, every array in a region of its own of one host block"""
    buf = (ctypes.c_int64 * 512)()
    at = ctypes.addressof(buf)
    d = A.hk_pv_loss_desc()
    for k, name in enumerate(_POINTERS):
        setattr(d, name, at + 256 * k)
    d.logits_stride, d.value_stride, d.target_policy_stride, d.dlogits_stride, d.dvalue_stride = 3, 1, 4, 5, 2
    d.num_samples, d.batch, d.actions, d.dtype, d.flags = 6, 4, 3, A.HK_F32, 0
    for name, v in over.items():
        setattr(d, name, v + getattr(d, name) if isinstance(v, _Shift) else
                getattr(d, v[0]) + v[1] if isinstance(v, _At) else v)
    d._keep = buf
    return d


def test_pv_loss_validation_without_gpu():
    L = _lib.lib()
    run = lambda **over: L.hk_pv_loss(ctypes.byref(_desc(**over)), None)  # noqa: E731
    wide = dict(logits_stride=255, target_policy_stride=255, dlogits_stride=255)
    assert L.hk_pv_loss(None, None) == A.HK_ERR_NULL
    assert run(batch=0) == A.HK_OK  # a valid descriptor, nothing to do
    assert run(batch=0, logits=None, dlogits=None, workspace=None, num_samples=0) == A.HK_OK  # no rows, no arrays
    assert run(batch=0, actions=255, **wide) == A.HK_OK
    assert run(batch=-1) == A.HK_ERR_SHAPE
    for dtype in (A.HK_F64, A.HK_I32, A.HK_I64, A.HK_U8, 7, -1):
        assert run(dtype=dtype) == A.HK_ERR_UNSUPPORTED and run(batch=0, dtype=dtype) == A.HK_ERR_UNSUPPORTED
    for flags in (1, 2, 1 << 30, -1):
        assert run(flags=flags) == A.HK_ERR_UNSUPPORTED and run(batch=0, flags=flags) == A.HK_ERR_UNSUPPORTED
    for batch in (0, 4):
        assert run(batch=batch, actions=0) == A.HK_ERR_SHAPE
        assert run(batch=batch, actions=-3) == A.HK_ERR_SHAPE
        assert run(batch=batch, actions=256, logits_stride=256, target_policy_stride=256,
                   dlogits_stride=256) == A.HK_ERR_SHAPE
        assert run(batch=batch, num_samples=-1) == A.HK_ERR_SHAPE
        for stride in ("logits_stride", "target_policy_stride", "dlogits_stride"):
            assert run(batch=batch, **{stride: 2}) == A.HK_ERR_SHAPE  # a stride below A
            assert run(batch=batch, **{stride: 0}) == A.HK_ERR_SHAPE
            assert run(batch=batch, **{stride: -5}) == A.HK_ERR_SHAPE
        for stride in ("value_stride", "dvalue_stride"):
            assert run(batch=batch, **{stride: 0}) == A.HK_ERR_SHAPE
            assert run(batch=batch, **{stride: -1}) == A.HK_ERR_SHAPE
    assert run(num_samples=0) == A.HK_ERR_SHAPE
    assert run(index=None, num_samples=3) == A.HK_ERR_SHAPE  # without an index row b takes sample b: 4 rows need 4
    for stride in ("logits_stride", "dlogits_stride", "value_stride", "dvalue_stride"):
        assert run(**{stride: 1 << 62}) == A.HK_ERR_SHAPE  # the rows would span more than the address space
    assert run(target_policy_stride=1 << 61, num_samples=9) == A.HK_ERR_SHAPE
    assert run(num_samples=1 << 62) == A.HK_ERR_SHAPE
    for name in _POINTERS:
        if name not in _OPTIONAL:
            assert run(**{name: None}) == A.HK_ERR_NULL, name
    for name in _INPUTS[:5] + _OUTPUTS + ("status",):
        assert run(**{name: _Shift(2)}) == A.HK_ERR_ALIGN, name
    assert run(index=_Shift(4)) == A.HK_ERR_ALIGN and run(workspace=_Shift(4)) == A.HK_ERR_ALIGN
    # an output on top of an input, or reaching into it: dlogits spans (3 * 5 + 3) * 4 = 72 bytes, dvalue (3 * 2 + 1) * 4
    # = 28, row_loss 16, loss 4; logits (3 * 3 + 3) * 4 = 48, value 16, target_policy (5 * 4 + 3) * 4 = 92, target_value
    # and weight 24, index 32
    spans = {"logits": 48, "value": 16, "target_policy": 92, "target_value": 24, "weight": 24, "index": 32}
    for out, own in (("dlogits", 72), ("dvalue", 28), ("row_loss", 16), ("loss", 4)):
        for inp, span in spans.items():
            assert run(**{out: _At((inp, 0))}) == A.HK_ERR_UNSUPPORTED, (out, inp)
            assert run(**{out: _At((inp, span - 4))}) == A.HK_ERR_UNSUPPORTED, (out, inp)  # its first element on the last
            assert run(**{out: _At((inp, 4 - own))}) == A.HK_ERR_UNSUPPORTED, (out, inp)   # its last element on the first
