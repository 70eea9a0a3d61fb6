"""Every kernel family on the memory layouts include/hironaka_hip.h allows: records at pointers that are only
element-aligned, strides beyond max_points*dim, agent observations with the mask in the record's tail, separate
layouts for input and output, and in place.

Every record batch is carved out of a larger device buffer (`arena`) with at least 4 KiB of the test's own memory on
both sides: gaps and margins of an input hold 0.0 (a row of zeros dominates every row, so reading a gap as a point
changes the result), those of an output a recognisable NaN pattern that must survive bit for bit.  The expectation is
always the C oracle on the plain contiguous batch (tests/layout_cases.py; its independence of the layout is pinned by
tests/test_oracle.py), compared with np.array_equal: no tolerance anywhere.

A kernel family that cannot take a layout is no error: `pick` falls through to the next one and the result is the
same.  The requests that are refused are listed with their status in EXPECTED_STATUS; everything else is served."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import layout_cases as LC
from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import ops
from hironaka_amd._lib import HironakaHipError, lib
from oracle import c_oracle as CO

pytestmark = pytest.mark.gpu

MARGIN_BYTES = 4096
GUARD = {1: 0xA5, 4: 0x7FC0BEEF, 8: 0x7FF8BEEF0BADF00D}  # per element size; a quiet NaN for float32 / float64
BITS = {1: torch.uint8, 4: torch.int32, 8: torch.int64}

F1, F2, F4 = A.HK_FLAG_FORCE_ONE_LANE, A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_FOUR_LANES
FT, FG = A.HK_FLAG_FORCE_TEAM, A.HK_FLAG_FORCE_GENERIC
FLAG_NAMES = {0: "default", F1: "one_lane", F2: "two_lanes", F4: "four_lanes", FT: "team", FG: "generic"}
# the families a shape has (flag 0 is the team kernel at (7,3) and the generic one at (9,7) / float64)
FAMILIES = {"20x3": (0, F1, F2, F4, FT, FG), "20x4": (0, F1, F2, F4, FT, FG), "10x3": (0, F1, F2, F4, FT, FG),
            "5x3": (0, F1, F2, FT, FG), "8x4": (0, F1, F2, FT, FG), "50x4": (0, F4, FT, FG), "7x3": (0, FG),
            "9x7": (0,), "20x3_f64": (0,)}

# id -> (base offset in elements, stride beyond m*d: a number of elements or "d")
LAYOUTS = {"plain": (0, 0), "off1": (1, 0), "off2": (2, 0), "rec": (0, "d"), "pad4": (0, 4), "pad1": (0, 1),
           "off1pad1": (1, 1)}
# (input, output) at 193 games; output None = in place (points_out == points_in)
STEP_PAIRS = [(k, k) for k in LAYOUTS] + [("plain", "pad4"), ("pad4", "plain"), ("rec", "plain"), ("plain", "off1"),
                                         ("off1", "pad4"), ("off2", "plain"),  # (the team kernel's vec_in != vec_out)
                                         ("plain", None), ("pad4", None), ("pad1", None)]
# config -> how the host's subset is handed over ("rec" inputs also run with HK_COORDS_IN_RECORD)
COORDS_OF = {"jax7": "class", "jax15": "mask", "torch7": "mask", "torch15": "class", "list": "class"}

# (operator, shape, input layout) -> status of the requests that are refused; every other request is served.
# hk_step_features and HK_AXIS_MASKED_LOGITS exist on the four-lane kernel only: contiguous records aligned to its
# vector width (16 bytes, 8 at (10,3)).  The binning kernels want 16 bytes.
EXPECTED_STATUS = {}
for _s in ("10x3", "20x3", "20x4"):
    for _op in ("step_features", "masked_logits"):
        EXPECTED_STATUS[(_op, _s, "off1")] = A.HK_ERR_UNSUPPORTED
        EXPECTED_STATUS[(_op, _s, "pad4")] = A.HK_ERR_UNSUPPORTED
        if _s != "10x3":
            EXPECTED_STATUS[(_op, _s, "off2")] = A.HK_ERR_UNSUPPORTED
for _op in ("bin_by_live_rows", "generate_points_binned"):
    EXPECTED_STATUS[(_op, "20x3", "off1")] = A.HK_ERR_ALIGN

STEP_SHAPES = LC.SHAPES
SIDE = ("done", "prev_done", "reward", "num_points")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


def tdtype(np_dtype):
    return {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32,
            np.dtype(np.uint8): torch.uint8}[np.dtype(np_dtype)]


def dev(x):
    return torch.as_tensor(np.array(x)).cuda()  # (a copy: the shared cases are read-only)


def host(t):
    return t.detach().cpu().numpy()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def arena(b, n, stride, offset_elems, dtype=torch.float32, fill="guard", spec=None):
    """`b` records of `stride` elements carved out of a larger device buffer: returns (flat buffer, view), the view
    [b, stride] -- [b, m, d] when stride == n and `spec` is given -- starting `offset_elems` elements after a 256-byte
    aligned address, with MARGIN_BYTES of the buffer before the first record and after the last.  fill: 0 (inputs) or
    "guard" (outputs: GUARD's bit pattern)."""
    es = torch.empty((), dtype=dtype).element_size()
    margin = MARGIN_BYTES // es
    total = margin + offset_elems + b * stride + margin
    raw = torch.empty(total + 256 // es, dtype=dtype, device="cuda")
    skip = (-raw.data_ptr() % 256) // es
    flat = raw[skip:skip + total]
    if fill == 0:
        flat.zero_()
    else:
        flat.view(BITS[es]).fill_(GUARD[es])
    start = margin + offset_elems
    view = flat[start:start + b * stride].view(b, stride)
    if stride == n and spec is not None:
        view = view.view(b, *spec)
    assert (view.data_ptr() - offset_elems * es) % 256 == 0 and view.is_contiguous()
    return flat, view


def outside_unchanged(flat, view, n, fill="guard"):
    """every element of the arena that is not among the first n of a record still holds the fill, bit for bit"""
    es = flat.element_size()
    bits = host(flat.view(BITS[es]))
    b = view.shape[0]
    stride = view.numel() // b
    start = (view.data_ptr() - flat.data_ptr()) // es
    keep = np.ones(bits.shape, dtype=bool)
    keep[(start + np.arange(b)[:, None] * stride + np.arange(n)[None, :]).ravel()] = False
    return bool((bits[keep] == (0 if fill == 0 else GUARD[es])).all())


def first_n(view, n):
    return host(view.reshape(view.shape[0], -1)[:, :n])


def layout_arena(layout, b, m, d, dtype, fill):
    off, extra = LAYOUTS[layout]
    n = m * d
    return arena(b, n, n + (d if extra == "d" else extra), off, tdtype(dtype), fill, spec=(m, d))


def input_arena(layout, p, tail=None):
    """the games `p` [b, m, d] in a zero-filled arena of the layout; "rec": `tail` [b, d] behind the points"""
    b, m, d = p.shape
    flat, view = layout_arena(layout, b, m, d, p.dtype, 0)
    view.reshape(b, -1)[:, :m * d] = dev(p.reshape(b, -1))
    if tail is not None:
        view[:, m * d:m * d + d] = dev(tail.astype(p.dtype))
    return flat, view


def status_of(call):
    try:
        call()
    except HironakaHipError as err:
        return err.status
    return A.HK_OK


# ------------------------------------------------------------------------------------------------------------------
# hk_step
# ------------------------------------------------------------------------------------------------------------------

def check_step(shape, b, in_layout, out_layout, flags_list, configs):
    m, d, dtype = shape
    n = m * d
    p = LC.states(m, d, b, dtype)
    cls, ax, mask = LC.actions(m, d, b)
    g_cls, g_ax, g_mask = dev(cls), dev(ax), dev(mask)
    in_flat, in_view = input_arena(in_layout, p, mask if in_layout == "rec" else None)
    before = in_flat.clone()
    for name in configs:
        want = LC.expected_step(m, d, b, dtype, name)
        cfg = LC.STEP_CONFIGS[name]
        modes = [COORDS_OF[name]] + (["record"] if in_layout == "rec" else [])
        for flag in flags_list:
            for mode in modes:
                tag = (LC.shape_id(shape), b, in_layout, out_layout, name, FLAG_NAMES[flag], mode)
                if out_layout is None:  # in place: a fresh copy of the input, which must keep its zeros
                    out_flat, out_view = input_arena(in_layout, p)
                    src, fill = out_view, 0
                else:
                    out_flat, out_view = layout_arena(out_layout, b, m, d, dtype, "guard")
                    src, fill = in_view, "guard"
                coords = {"class": g_cls, "mask": g_mask, "record": None}[mode]
                got = ops.step(src, coords, g_ax, stages=cfg[4], flags=LC.config_flags(name) | flag, reward_sign=-1.0,
                               spec=(m, d), coords_in_record=mode == "record", out=out_view, want=SIDE)
                assert np.array_equal(first_n(out_view, n), want["points"].reshape(b, n)), tag
                assert outside_unchanged(out_flat, out_view, n, fill), tag
                for k in SIDE:
                    assert np.array_equal(host(got[k]), want[k]), (k, tag)
    assert torch.equal(in_flat.view(BITS[in_flat.element_size()]), before.view(BITS[in_flat.element_size()]))


@pytest.mark.parametrize("pair", STEP_PAIRS, ids=lambda pr: f"{pr[0]}-{pr[1] or 'inplace'}")
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=LC.shape_id)
def test_step_layouts_families_semantics(shape, pair):
    """stages 7 and 15 with the four side outputs in JAX and torch semantics, the sorted + compacted step of the
    list semantics, under every kernel family of the shape"""
    check_step(shape, 193, pair[0], pair[1], FAMILIES[LC.shape_id(shape)], tuple(LC.STEP_CONFIGS))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("b", [x for x in LC.BATCHES if x != 193])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=LC.shape_id)
def test_step_batch_tails(shape, b, layout):
    """partial waves of every family, one full wave and several workgroups, input and output in the same layout"""
    fam = FAMILIES[LC.shape_id(shape)]
    check_step(shape, b, layout, layout, fam, ("jax7",))
    check_step(shape, b, layout, layout, (0,), ("torch15", "list"))


@pytest.mark.parametrize("layout", ["pad4", "off1"])
@pytest.mark.parametrize("shape", STEP_SHAPES, ids=LC.shape_id)
def test_single_stage_operators(shape, layout):
    """shift / reposition / Newton polytope / rescale one at a time: as hk_step with one stage on the layout, and
    through the C wrappers (which take no stride) at the layout's pointers"""
    m, d, dtype = shape
    n, b = m * d, 193
    p = LC.states(m, d, b, dtype)
    cls, ax, mask = LC.actions(m, d, b)
    want = {A.HK_STAGE_SHIFT: CO.shift(p, cls, ax), A.HK_STAGE_REPOSITION: CO.reposition(p),
            A.HK_STAGE_NEWTON: CO.get_newton_polytope(p), A.HK_STAGE_RESCALE: CO.rescale(p)}
    in_flat, in_view = input_arena(layout, p)
    L, code = lib(), CO._NP2HK[np.dtype(dtype)]
    for flag in FAMILIES[LC.shape_id(shape)]:
        for stage, exp in want.items():
            out_flat, out_view = layout_arena(layout, b, m, d, dtype, "guard")
            ops.step(in_view, dev(cls), dev(ax), stages=stage, flags=flag, spec=(m, d), out=out_view)
            assert np.array_equal(first_n(out_view, n), exp.reshape(b, n)), (stage, layout, FLAG_NAMES[flag])
            assert outside_unchanged(out_flat, out_view, n), (stage, layout, FLAG_NAMES[flag])
        if LAYOUTS[layout][1] == 0:  # contiguous at an offset: the wrappers' own layout
            g_cls, g_ax = dev(cls), dev(ax)
            calls = {
                A.HK_STAGE_SHIFT: lambda o: L.hk_shift(in_view.data_ptr(), o, g_cls.data_ptr(), A.HK_COORDS_CLASS_I32,
                                                       g_ax.data_ptr(), A.HK_I32, b, m, d, code, -1.0, flag, stream()),
                A.HK_STAGE_REPOSITION: lambda o: L.hk_reposition(in_view.data_ptr(), o, b, m, d, code, -1.0, flag, stream()),
                A.HK_STAGE_NEWTON: lambda o: L.hk_get_newton_polytope(in_view.data_ptr(), o, b, m, d, code, -1.0, flag,
                                                                      stream()),
                A.HK_STAGE_RESCALE: lambda o: L.hk_rescale(in_view.data_ptr(), o, b, m, d, code, -1.0, flag, stream())}
            for stage, call in calls.items():
                out_flat, out_view = layout_arena(layout, b, m, d, dtype, "guard")
                assert call(out_view.data_ptr()) == A.HK_OK
                assert np.array_equal(first_n(out_view, n), want[stage].reshape(b, n)), (stage, FLAG_NAMES[flag])
                assert outside_unchanged(out_flat, out_view, n), (stage, FLAG_NAMES[flag])


def step_desc(in_view, out_view, b, m, d, dtype, stages, flags, in_stride=None, out_stride=None):
    s = A.hk_step_desc()
    s.points_in, s.points_out = in_view.data_ptr(), out_view.data_ptr()
    s.in_stride = in_view.numel() // b if in_stride is None else in_stride
    s.out_stride = out_view.numel() // b if out_stride is None else out_stride
    s.coords_kind = A.HK_COORDS_NONE
    s.padding_value, s.reward_sign = -1.0, -1.0
    s.batch, s.max_points, s.dim, s.dtype = b, m, d, CO._NP2HK[np.dtype(dtype)]
    s.stages, s.flags = stages, flags
    return s


@pytest.mark.parametrize("shape", STEP_SHAPES, ids=LC.shape_id)
def test_mask_coords_with_their_own_stride(shape):
    """[batch, dim] masks with coords_stride > dim (float32), and a uint8 mask whose rows start at odd byte addresses"""
    m, d, dtype = shape
    n, b = m * d, 193
    p = LC.states(m, d, b, dtype)
    cls, ax, mask = LC.actions(m, d, b)
    g_ax = dev(ax)
    masks = []
    for mdtype, stride, off in ((torch.float32, d + 3, 1), (torch.uint8, d + (d % 2 == 0), 1)):
        _, mv = arena(b, d, stride, off, mdtype, 0)
        mv[:, :d] = dev(mask).to(mdtype)
        assert mdtype != torch.uint8 or (mv.data_ptr() % 2 == 1 and stride % 2 == 1)
        masks.append((mv, A.HK_F32 if mdtype == torch.float32 else A.HK_U8, stride))
    L = lib()
    for layout in ("plain", "pad1"):
        in_flat, in_view = input_arena(layout, p)
        for name in ("jax7", "torch15"):
            want = LC.expected_step(m, d, b, dtype, name)
            for flag in FAMILIES[LC.shape_id(shape)]:
                for mv, kind, stride in masks:
                    out_flat, out_view = layout_arena(layout, b, m, d, dtype, "guard")
                    s = step_desc(in_view, out_view, b, m, d, dtype, LC.STEP_CONFIGS[name][4], LC.config_flags(name) | flag)
                    s.coords, s.coords_kind, s.coords_stride = mv.data_ptr(), kind, stride
                    s.axis, s.axis_dtype = g_ax.data_ptr(), A.HK_I32
                    done = torch.empty(b, dtype=torch.uint8, device="cuda")
                    s.done_out = done.data_ptr()
                    tag = (layout, name, FLAG_NAMES[flag], kind)
                    assert L.hk_step(C.byref(s), stream()) == A.HK_OK, tag
                    assert np.array_equal(first_n(out_view, n), want["points"].reshape(b, n)), tag
                    assert outside_unchanged(out_flat, out_view, n), tag
                    assert np.array_equal(host(done).astype(bool), want["done"]), tag


# ------------------------------------------------------------------------------------------------------------------
# hk_step_features / HK_AXIS_MASKED_LOGITS: the four-lane kernel only
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["plain", "off2", "off1", "pad4"])
@pytest.mark.parametrize("shape", [s for s in LC.SHAPES if LC.shape_id(s) in ("10x3", "20x3", "20x4")], ids=LC.shape_id)
def test_step_features_and_agent_logits(shape, layout):
    """served on contiguous records aligned to the kernel's vector width (8 bytes at (10,3): "off2"), refused with
    HK_ERR_UNSUPPORTED elsewhere, and then nothing is written"""
    m, d, dtype = shape
    n, b, sid = m * d, 193, LC.shape_id(shape)
    p = LC.states(m, d, b, dtype)
    cls, ax, _ = LC.actions(m, d, b)
    rng = np.random.default_rng(5)
    lg = rng.standard_normal((b, d)).astype(np.float32)
    lg[rng.random((b, d)) < 0.1] = np.nan
    lg[rng.random((b, d)) < 0.15] = 0.25
    in_flat, in_view = input_arena(layout, p)
    for name in ("jax7", "torch7", "jax15"):
        cfg, fo = LC.STEP_CONFIGS[name], LC.config_flags(name)
        for axis, is_logits in ((ax, False), (lg, True)):
            for features in (True, None):
                if features is None and not is_logits:
                    continue  # (the plain step: test_step_layouts_families_semantics)
                op = "step_features" if features else "masked_logits"
                for flag in (0, F4):
                    want = CO.step(p, cls, axis, stages=cfg[4], flags=fo, axis_logits=is_logits, features=features,
                                   reward_sign=-1.0)
                    out_flat, out_view = layout_arena("plain", b, m, d, dtype, "guard")
                    f_flat, f_view = arena(b, n, n, 0, torch.float32, "guard")
                    st = status_of(lambda: ops.step(in_view, dev(cls), dev(axis), stages=cfg[4], flags=fo | flag,
                                                    reward_sign=-1.0, spec=(m, d), out=out_view,
                                                    features_out=f_view if features else None))
                    tag = (sid, layout, name, op, is_logits, FLAG_NAMES[flag])
                    assert st == EXPECTED_STATUS.get((op, sid, layout), A.HK_OK), tag
                    if st == A.HK_OK:
                        assert np.array_equal(first_n(out_view, n), want["points"].reshape(b, n), equal_nan=True), tag
                        if features:
                            assert np.array_equal(host(f_view), want["features"], equal_nan=True), tag
                    else:
                        assert outside_unchanged(out_flat, out_view, 0) and outside_unchanged(f_flat, f_view, 0), tag
                    assert outside_unchanged(out_flat, out_view, n) and outside_unchanged(f_flat, f_view, n if features else 0)


def test_step_features_into_a_slot_of_the_search_tables():
    """HostExpander's call at (10,3) with 33 games: out and features_out are slot 1 of [N, 33, 30] tables, 8 bytes off
    a 16-byte boundary -- what the shape's four-lane kernel stores to (8-byte chunks), so it is served"""
    m, d, b, n = 10, 3, 33, 30
    p = LC.states(m, d, b, np.float32)
    cls, ax, _ = LC.actions(m, d, b)
    want = CO.step(p, cls, ax, stages=7, features=True)
    p_flat, table = arena(2 * b, n, n, 0, torch.float32, "guard")
    f_flat, ftable = arena(2 * b, n, n, 0, torch.float32, "guard")
    P, F = table.view(2, b, n), ftable.view(2, b, n)
    assert P[1].data_ptr() % 16 == 8 and F[1].data_ptr() % 16 == 8
    got = ops.step(dev(p), dev(cls), dev(ax), stages=7, out=P[1], features_out=F[1], want=SIDE)
    assert np.array_equal(host(P[1]), want["points"].reshape(b, n))
    assert np.array_equal(host(F[1]), want["features"])
    for k in SIDE:
        assert np.array_equal(host(got[k]), want[k]), k
    assert outside_unchanged(p_flat, P[1], n) and outside_unchanged(f_flat, F[1], n)  # slot 0 and the margins


def test_step_features_pointer_the_kernel_cannot_store_to_is_unsupported():
    """(20,3) stores its features in 16-byte chunks: a features_out one element off is element-aligned, so it is no
    HK_ERR_ALIGN, and the four-lane kernel declines it: HK_ERR_UNSUPPORTED (the caller's cue for hk_step +
    hk_get_features)"""
    m, d, b, n = 20, 3, 33, 60
    p = LC.states(m, d, b, np.float32)
    cls, ax, _ = LC.actions(m, d, b)
    o_flat, out = arena(b, n, n, 0, torch.float32, "guard")
    f_flat, feat = arena(b, n, n, 1, torch.float32, "guard")
    assert feat.data_ptr() % 16 == 4
    with pytest.raises(HironakaHipError) as err:
        ops.step(dev(p), dev(cls), dev(ax), stages=7, out=out, features_out=feat)
    assert err.value.status == A.HK_ERR_UNSUPPORTED
    assert outside_unchanged(o_flat, out, 0) and outside_unchanged(f_flat, feat, 0)


# ------------------------------------------------------------------------------------------------------------------
# the strided read-only operators
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["plain", "rec", "pad4", "pad1", "off1"])
@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.shape_id)
def test_zeillinger_layouts(shape, layout):
    m, d, dtype = shape
    L, code = lib(), CO._NP2HK[np.dtype(dtype)]
    for b in (193, 1000):
        p = LC.states(m, d, b, dtype)
        _, view = input_arena(layout, p, np.full((b, d), 7.0) if layout == "rec" else None)
        for sem in ("jax", "list"):
            want = CO.zeillinger(p, sem)
            for flag in (FAMILIES[LC.shape_id(shape)] if b == 193 else (0,)):
                c_flat, c_view = arena(b, 1, 1, 1, torch.int32, "guard")
                st = L.hk_zeillinger(view.data_ptr(), view.numel() // b, c_view.data_ptr(), b, m, d, code,
                                     A.SEMANTICS[sem] | flag, stream())
                assert st == A.HK_OK, (b, sem, FLAG_NAMES[flag])
                assert np.array_equal(host(c_view).ravel(), want), (b, sem, FLAG_NAMES[flag])
                assert outside_unchanged(c_flat, c_view, 1)


@pytest.mark.parametrize("out_layout", ["plain", "pad4", "pad1", "off1"])
@pytest.mark.parametrize("in_layout", ["plain", "rec", "pad4", "pad1", "off1"])
@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.shape_id)
def test_features_layouts(shape, in_layout, out_layout):
    """hk_get_features (with and without rescaling) and hk_get_features_torch, strided on both sides"""
    m, d, dtype = shape
    n, L, code = m * d, lib(), CO._NP2HK[np.dtype(dtype)]
    for b in (193, 1000):
        p = LC.states(m, d, b, dtype)
        _, view = input_arena(in_layout, p, np.full((b, d), 7.0) if in_layout == "rec" else None)
        calls = [(CO.get_features(p, bool(s)),
                  lambda o, os_, s=s: L.hk_get_features(view.data_ptr(), view.numel() // b, o, os_, b, m, d, code, s, -1.0,
                                                        stream())) for s in (0, 1)]
        calls.append((CO.get_features_torch(p).reshape(b, n),
                      lambda o, os_: L.hk_get_features_torch(view.data_ptr(), view.numel() // b, o, os_, b, m, d, code,
                                                             -1.0, stream())))
        for i, (want, call) in enumerate(calls):
            out_flat, out_view = layout_arena(out_layout, b, m, d, dtype, "guard")
            assert call(out_view.data_ptr(), out_view.numel() // b) == A.HK_OK, (b, i)
            assert np.array_equal(first_n(out_view, n), want), (b, i)
            assert outside_unchanged(out_flat, out_view, n), (b, i)


@pytest.mark.parametrize("layout", ["plain", "rec", "off1pad1"])
@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.shape_id)
def test_counts_layouts(shape, layout):
    m, d, dtype = shape
    for b in LC.BATCHES:
        p = LC.states(m, d, b, dtype)
        _, view = input_arena(layout, p, np.full((b, d), 7.0) if layout == "rec" else None)
        assert np.array_equal(host(ops.get_dones(view, spec=(m, d))), CO.get_dones(p)), b
        assert np.array_equal(host(ops.get_num_points(view, spec=(m, d))), CO.get_num_points(p)), b


def _encode(masks):
    """[N, d] 0/1 masks (all -1 = no subset) -> class ids, -1 kept"""
    v = (masks.clip(0).astype(np.int64) << np.arange(masks.shape[1])).sum(1)
    lg = np.floor(np.log2(np.maximum(v, 1))).astype(np.int64)
    return np.where(masks[:, 0] < 0, -1, v - lg - 2)


@pytest.mark.parametrize("layout", ["off1", "off2"])
def test_host_select_pointers(layout):
    """the deterministic hosts at pointers that are only 4- / 8-byte aligned: the recorded answers of the reference's
    hosts (tests/golden/hosts.npz), and Zeillinger's against the oracle on the layouts' own games"""
    fixture = np.load(os.path.join(GOLDEN, "hosts.npz"))
    for dtype in (np.float32, np.float64):
        for d in (3, 4):
            st = fixture[f"sel{d}_states"].astype(dtype)
            _, view = input_arena(layout, st)
            for hname in ("zeillinger_lex", "weak_spivakovsky", "weak_spivakovsky_min_hitting", "zeillinger"):
                got = host(ops.host_select(view, hname))
                assert np.array_equal(got, _encode(fixture[f"sel{d}_{hname}"])), (hname, d, dtype)
    for m, d, dtype in ((20, 3, np.float32), (7, 3, np.float32), (20, 3, np.float64)):
        p = LC.states(m, d, 193, dtype)
        _, view = input_arena(layout, p)
        assert np.array_equal(host(ops.host_select(view, "zeillinger")), CO.zeillinger(p, "list")), (m, d, dtype)


# ------------------------------------------------------------------------------------------------------------------
# the generators (no stride: the pointers vary)
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["plain", "off1", "off2"])
@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.shape_id)
def test_generate_points_pointers(shape, layout):
    """the four-lane generator declines a pointer it cannot store to; the other generators give the same draws"""
    m, d, dtype = shape
    n = m * d
    for b in (193, 1000):
        want = CO.generate_points(b, m, d, 20, 5, game_offset=9, dtype=dtype)
        for flag in (FAMILIES[LC.shape_id(shape)] if b == 193 else (0,)):
            flat, view = layout_arena(layout, b, m, d, dtype, "guard")
            ops.generate_points(b, m, d, 20, seed=5, game_offset=9, flags=flag, out=view)
            assert np.array_equal(host(view), want), (b, FLAG_NAMES[flag])
            assert outside_unchanged(flat, view, n), (b, FLAG_NAMES[flag])


def test_binning_needs_sixteen_bytes():
    """hk_bin_by_live_rows / hk_generate_points_binned: HK_ERR_ALIGN before any launch, nothing written"""
    m, d, b, n = 20, 3, 193, 60
    L = lib()
    _, src = input_arena("plain", LC.states(m, d, b, np.float32))
    _, src1 = input_arena("off1", LC.states(m, d, b, np.float32))
    for name, make in (("bin_by_live_rows", lambda o, i: L.hk_bin_by_live_rows(src.data_ptr(), o, i, None, b, m, d, A.HK_F32,
                                                                               stream())),
                       ("generate_points_binned", lambda o, i: L.hk_generate_points_binned(o, i, None, b, m, d, A.HK_F32, 20,
                                                                                           5, 0, 6, -1.0, 0, stream()))):
        for layout in ("plain", "off1"):
            flat, view = layout_arena(layout, b, m, d, np.float32, "guard")
            i_flat, ids = arena(b, 1, 1, 0, torch.int32, "guard")
            st = make(view.data_ptr(), ids.data_ptr())
            assert st == EXPECTED_STATUS.get((name, "20x3", layout), A.HK_OK), (name, layout)
            if st != A.HK_OK:
                assert outside_unchanged(flat, view, 0) and outside_unchanged(i_flat, ids, 0), (name, layout)
            else:
                assert outside_unchanged(flat, view, n) and outside_unchanged(i_flat, ids, 1), (name, layout)
    flat, view = layout_arena("plain", b, m, d, np.float32, "guard")
    i_flat, ids = arena(b, 1, 1, 0, torch.int32, "guard")
    assert L.hk_bin_by_live_rows(src1.data_ptr(), view.data_ptr(), ids.data_ptr(), None, b, m, d, A.HK_F32, stream()) \
        == A.HK_ERR_ALIGN
    assert outside_unchanged(flat, view, 0) and outside_unchanged(i_flat, ids, 0)


# ------------------------------------------------------------------------------------------------------------------
# hk_rollout (no stride: the pointers vary)
# ------------------------------------------------------------------------------------------------------------------

STEPS = 5
ROLL_STAGES = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON


def run_rollout(shape, b, seed, *, points_off, flags=0, obs_off=None, small=False, host_policy=A.HK_HOST_RANDOM,
                initial_off=None, episodes=1, gen=0):
    """hk_rollout through the raw descriptor with every buffer in an arena of its own; checks the guards and that the
    initial states stay untouched; returns the products as numpy arrays"""
    m, d, dtype = shape
    n, L = m * d, lib()
    p = LC.states(m, d, b, dtype)
    r = A.hk_rollout_desc()
    keep = {}
    if initial_off is not None:
        keep["in"] = arena(b, n, n, initial_off, tdtype(dtype), 0, spec=(m, d))
        keep["in"][1].copy_(dev(p))
        keep["pts"] = arena(b, n, n, points_off, tdtype(dtype), "guard", spec=(m, d))
        r.points_in = keep["in"][1].data_ptr()
        before = keep["in"][0].clone()
    elif gen:
        keep["pts"] = arena(b, n, n, points_off, tdtype(dtype), "guard", spec=(m, d))
    else:
        keep["pts"] = arena(b, n, n, points_off, tdtype(dtype), 0, spec=(m, d))
        keep["pts"][1].copy_(dev(p))
    r.points = keep["pts"][1].data_ptr()
    if obs_off is not None:
        keep["obs"] = arena(STEPS * b, n, n, obs_off, tdtype(dtype), "guard")
        r.obs_out = keep["obs"][1].data_ptr()
    if small or obs_off is not None:
        for key, field, dt in (("host_class", "host_class_out", torch.int32), ("axis", "axis_out", torch.int32),
                               ("done", "done_out", torch.uint8), ("reward", "reward_out", torch.float32)):
            keep[key] = arena(STEPS, b, b, 0, dt, "guard")
            setattr(r, field, keep[key][1].data_ptr())
    keep["game_length"] = arena(1, b, b, 1, torch.int32, "guard")
    r.game_length_out = keep["game_length"][1].data_ptr()
    dc = torch.zeros(STEPS + 1, dtype=torch.int64, device="cuda")
    r.done_count = dc.data_ptr()
    r.seed, r.padding_value, r.reward_sign = seed, -1.0, 1.0
    r.batch, r.max_points, r.dim, r.dtype, r.steps = b, m, d, CO._NP2HK[np.dtype(dtype)], STEPS
    r.host_policy, r.agent_policy, r.stages, r.flags = host_policy, A.HK_AGENT_RANDOM, ROLL_STAGES, flags
    r.episodes = episodes
    if gen:
        r.gen_max_value, r.gen_seed, r.gen_stages = gen, seed + 100, A.HK_STAGE_NEWTON | A.HK_STAGE_REPOSITION
    need = int(L.hk_rollout_workspace_bytes(C.byref(r)))  # (asked with the pointers the launch gets)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    r.workspace, r.workspace_bytes = ws.data_ptr(), need
    st = L.hk_rollout(C.byref(r), stream())
    assert st == A.HK_OK, f"hk_rollout status {st}"
    res = {"points": host(keep["pts"][1]), "done_count": host(dc).astype(np.uint64),
           "game_length": host(keep["game_length"][1]).ravel()}
    assert outside_unchanged(*keep["pts"], n, 0 if (initial_off is None and not gen) else "guard")
    assert outside_unchanged(*keep["game_length"], b)
    assert not bool(ws.any()), "the reduction leaves the workspace zero"
    if initial_off is not None:
        assert torch.equal(keep["in"][0].view(BITS[before.element_size()]), before.view(BITS[before.element_size()]))
    if obs_off is not None:
        res["obs"] = host(keep["obs"][1]).reshape(STEPS, b, m, d)
        assert outside_unchanged(*keep["obs"], n)
    for key in ("host_class", "axis", "done", "reward"):
        if key in keep:
            res[key] = host(keep[key][1])
            assert outside_unchanged(*keep[key], b)
    return res


_roll_cache = {}


def expected_rollout(shape, b, seed, host_policy=A.HK_HOST_RANDOM):
    key = (shape, b, seed, host_policy)
    if key not in _roll_cache:
        m, d, dtype = shape
        _roll_cache[key] = CO.rollout(LC.states(m, d, b, dtype), STEPS, seed, host_policy=host_policy, record=True)
    return _roll_cache[key]


def check_rollout(got, want_p, want, tag):
    assert np.array_equal(got["points"], want_p), tag
    assert np.array_equal(got["done_count"], want["done_count"]), tag
    assert np.array_equal(got["game_length"], want["game_length"]), tag
    for key in ("obs", "host_class", "axis", "reward"):
        if key in got:
            assert np.array_equal(got[key], want[key]), (key, tag)
    if "done" in got:
        assert np.array_equal(got["done"].astype(bool), want["done"]), tag


@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.shape_id)
def test_rollout_plain_and_small_records_pointers(shape):
    b = 193
    want_p, want = expected_rollout(shape, b, 11)
    for flag in FAMILIES[LC.shape_id(shape)]:
        for off in (0, 1, 2):
            for small in (False, True):
                got = run_rollout(shape, b, 11, points_off=off, flags=flag, small=small)
                check_rollout(got, want_p, want, (FLAG_NAMES[flag], off, small))


@pytest.mark.parametrize("offs", [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)], ids=lambda o: f"points{o[0]}-obs{o[1]}")
@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.shape_id)
def test_rollout_observations_pointers(shape, offs):
    """recording rollouts with `points` and `obs_out` aligned independently: an obs_out the four-lane rollout cannot
    store to makes it decline, and the next family serves the request"""
    for b in (193, 1000):
        want_p, want = expected_rollout(shape, b, 12)
        for flag in (FAMILIES[LC.shape_id(shape)] if b == 193 else (0,)):
            got = run_rollout(shape, b, 12, points_off=offs[0], obs_off=offs[1], flags=flag)
            check_rollout(got, want_p, want, (b, FLAG_NAMES[flag]))


@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.shape_id)
def test_rollout_zeillinger_host_pointers(shape):
    b = 193
    want_p, want = expected_rollout(shape, b, 13, A.HK_HOST_ZEILLINGER)
    for flag in FAMILIES[LC.shape_id(shape)]:
        for off in (0, 1, 2):
            got = run_rollout(shape, b, 13, points_off=off, flags=flag, host_policy=A.HK_HOST_ZEILLINGER)
            check_rollout(got, want_p, want, (FLAG_NAMES[flag], off))


@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.shape_id)
def test_rollout_episodes_from_points_in_pointers(shape):
    """points_in + episodes = 3: the counts accumulate, `points` and game_length are the last episode's"""
    m, d, dtype = shape
    b = 193
    total = np.zeros(STEPS + 1, dtype=np.uint64)
    for e in range(3):
        want_p, want = CO.rollout(LC.states(m, d, b, dtype), STEPS, 20 + e, record=False)
        total += want["done_count"]
    for flag in FAMILIES[LC.shape_id(shape)]:
        for in_off, out_off in ((0, 0), (1, 0), (0, 1), (2, 2), (1, 2)):
            got = run_rollout(shape, b, 20, points_off=out_off, initial_off=in_off, episodes=3, flags=flag)
            tag = (FLAG_NAMES[flag], in_off, out_off)
            assert np.array_equal(got["points"], want_p), tag
            assert np.array_equal(got["done_count"], total), tag
            assert np.array_equal(got["game_length"], want["game_length"]), tag


@pytest.mark.parametrize("shape", LC.SHAPES, ids=LC.shape_id)
def test_rollout_generated_pointers(shape):
    """gen_max_value > 0 into a buffer the fused kernel cannot store to: hk_generate_points + plain rollouts serve it"""
    m, d, dtype = shape
    b = 193
    want_p, want = CO.rollout_generated(b, (m, d), STEPS, 30, max_value=20, gen_seed=130, dtype=dtype)
    for flag in FAMILIES[LC.shape_id(shape)]:
        for off in (0, 1, 2):
            got = run_rollout(shape, b, 30, points_off=off, gen=20, flags=flag)
            check_rollout(got, want_p, want, (FLAG_NAMES[flag], off))


# ------------------------------------------------------------------------------------------------------------------
# validation: decided before any launch
# ------------------------------------------------------------------------------------------------------------------

def test_layouts_the_header_forbids_are_refused_before_any_launch():
    m, d, b, n = 20, 3, 8, 60
    L = lib()
    flat, view = arena(b, n, n + d, 0, torch.float32, 0)
    o_flat, out = arena(b, n, n + d, 0, torch.float32, "guard")
    cls = torch.zeros(b, dtype=torch.int32, device="cuda")
    mask = torch.ones((b, d), dtype=torch.float32, device="cuda")

    def desc(**over):
        s = step_desc(view, out, b, m, d, np.float32, 7, 0)
        s.coords, s.coords_kind, s.coords_stride = mask.data_ptr(), A.HK_F32, d
        s.axis, s.axis_dtype = cls.data_ptr(), A.HK_I32
        for k, v in over.items():
            setattr(s, k, v)
        return s

    assert L.hk_step(C.byref(desc()), stream()) == A.HK_OK  # the control: only the change below is refused
    o_flat.view(torch.int32).fill_(GUARD[4])
    assert L.hk_step(C.byref(desc(points_in=view.data_ptr() + 2)), stream()) == A.HK_ERR_ALIGN
    assert L.hk_step(C.byref(desc(points_out=out.data_ptr() + 2)), stream()) == A.HK_ERR_ALIGN
    assert L.hk_step(C.byref(desc(in_stride=n - 1)), stream()) == A.HK_ERR_SHAPE
    assert L.hk_step(C.byref(desc(out_stride=n - 1)), stream()) == A.HK_ERR_SHAPE
    assert L.hk_step(C.byref(desc(coords_kind=A.HK_COORDS_IN_RECORD, in_stride=n + d - 1)), stream()) == A.HK_ERR_SHAPE
    assert L.hk_step(C.byref(desc(coords_kind=A.HK_COORDS_IN_RECORD, in_stride=n + d)), stream()) == A.HK_OK
    o_flat.view(torch.int32).fill_(GUARD[4])
    assert L.hk_step(C.byref(desc(coords_stride=d - 1)), stream()) == A.HK_ERR_SHAPE
    feat = torch.empty((b, n), dtype=torch.float32, device="cuda")
    assert L.hk_step_features(C.byref(desc(coords=cls.data_ptr(), coords_kind=A.HK_COORDS_CLASS_I32, in_stride=n,
                                           out_stride=n)), feat.data_ptr() + 2, 1, stream()) == A.HK_ERR_ALIGN
    r = A.hk_rollout_desc()
    counts = torch.zeros(STEPS + 2, dtype=torch.int64, device="cuda")
    pts = torch.zeros((b, m, d), dtype=torch.float32, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    r.points, r.done_count = pts.data_ptr(), counts.data_ptr() + 4
    r.workspace, r.workspace_bytes = ws.data_ptr(), ws.numel()
    r.padding_value, r.reward_sign = -1.0, 1.0
    r.batch, r.max_points, r.dim, r.dtype, r.steps = b, m, d, A.HK_F32, STEPS
    r.stages = ROLL_STAGES
    assert L.hk_rollout(C.byref(r), stream()) == A.HK_ERR_ALIGN
    torch.cuda.synchronize()
    assert outside_unchanged(o_flat, out, 0) and not bool(counts.any()) and not bool(pts.any())
