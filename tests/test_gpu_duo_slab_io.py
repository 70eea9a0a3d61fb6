"""The two-lane kernel's slab I/O, scan and wave maximum against the C oracle.

`hk::duo_kernel` loads its 32 games by LDS-DMA where its image is the contiguous slab -- (20,3): 16-byte chunks, no row
padding, contiguous 16-byte aligned records, no game ids -- with a branch of whole requests for a full wave and lanes that
sit out on the batch's last slab; every other layout keeps the loads through registers.  The exactness guard of the scan is
a word per lane, and the wave's widest game is a DPP reduction.  These cases aim at exactly that:

* batches of 1, 4, 5, 17, 31, 32, 33 and 65 games at (20,3) -- 15 chunks per game, 64 per request: a request that is
  empty, partial or exactly full, and a partial last slab behind full ones -- for 1, 2 and 20 steps at step offsets 0 and 3;
* jax, torch and list semantics and Zeillinger's host, which share the slab I/O;
* layouts that must stay on the register path and stay right: the initial states a view offset by one float, and by one
  game, of a larger tensor; in place; steps from records with a stride above m * d and into strided records;
* the shapes with 8-byte and 4-byte chunks and with padded images: (10,3), (5,3), (8,4), (16,3), (20,4);
* a sentinel row before and after the output of a batch of 33;
* placed states: every game finished at entry; 20 live rows per game (the wave maximum's upper bound: dense states
  before any Newton pass); one row that is not representable, which sends its wave down the generic routines (the guard).

Everything is compared with np.array_equal -- final states as bit patterns, `game_length`, `done_count` direct and
deferred -- forced onto two lanes and as `pick` routes it."""
import numpy as np
import pytest
import torch

from hironaka_amd import _abi as A
from hironaka_amd import ops
from oracle import c_oracle as CO

pytestmark = pytest.mark.gpu

F2 = A.HK_FLAG_FORCE_TWO_LANES
FORCE = ((F2, "two_lanes"), (0, "default"))
STAGES7 = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON
SENTINEL = 0x7FC0BEEF  # a quiet NaN

# name -> (flags, host policy, agent policy, stages, padding value)
CONFIGS = {
    "jax": (CO.flags_of(sem="jax"), A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM, STAGES7, -1.0),
    "torch": (CO.flags_of(sem="torch", noop_if_invalid=True, ignore_ended=True), A.HK_HOST_RANDOM,
              A.HK_AGENT_RANDOM_LEGAL, STAGES7, -1.0),
    "list": (CO.flags_of(sem="list", noop_if_invalid=True), A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM, STAGES7, -1.0),
    "zeillinger": (0, A.HK_HOST_ZEILLINGER, A.HK_AGENT_RANDOM, STAGES7, -1.0),
}
BATCHES = (1, 4, 5, 17, 31, 32, 33, 65)
STEPS = (1, 2, 20)
OFFSETS = (0, 3)
OTHER_SHAPES = [(10, 3), (5, 3), (8, 4), (16, 3), (20, 4)]
LAYOUTS = ("in_place", "separate", "offset_float", "offset_game")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


def dev(x):
    return torch.as_tensor(np.array(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def mixed_states(m, d, b, seed):
    """[b, m, d] float32: Newton-reduced states as the generator draws them, every fourth game dense (all m rows live)"""
    p = CO.generate_points(b, m, d, 20, seed)
    dense = CO.generate_points(b, m, d, 20, seed + 1, stages=0)
    p[3::4] = dense[3::4]
    return p


def initial_view(p0, layout):
    """the initial states on the device as `layout` places them: None (in place), a tensor of their own, or a contiguous
    view one float / one game into a larger tensor (16-byte aligned base: one float in is not); and a check that the
    larger tensor's other words still hold the sentinel"""
    b, m, d = p0.shape
    n = b * m * d
    if layout == "in_place":
        return None, lambda: True
    if layout == "separate":
        return dev(p0), lambda: True
    skip = 1 if layout == "offset_float" else m * d
    raw = torch.empty(n + m * d + 64, dtype=torch.float32, device="cuda")
    base = (-raw.data_ptr() % 256) // 4
    raw.view(torch.int32).fill_(SENTINEL)
    view = raw[base + skip:base + skip + n].view(b, m, d)
    view.copy_(dev(p0))
    assert view.is_contiguous() and (layout == "offset_game" or view.data_ptr() % 16 != 0)

    def around_intact():
        bits = host(raw.view(torch.int32))
        return bool((bits[:base + skip] == SENTINEL).all() and (bits[base + skip + n:] == SENTINEL).all())

    return view, around_intact


def guarded_output(p0, in_place):
    """a [b, m, d] output with a sentinel row before and after it (holding the initial states when `in_place`)"""
    b, m, d = p0.shape
    n, row = b * m * d, m * d
    raw = torch.empty(n + 2 * row + 64, dtype=torch.float32, device="cuda")
    base = (-raw.data_ptr() % 256) // 4
    flat = raw[base:base + n + 2 * row]
    flat.view(torch.int32).fill_(SENTINEL)
    out = flat[row:row + n].view(b, m, d)
    if in_place:
        out.copy_(dev(p0))
    return flat, out


def guard_rows_intact(flat, out):
    bits = host(flat.view(torch.int32))
    row = out.shape[1] * out.shape[2]
    return bool((bits[:row] == SENTINEL).all() and (bits[row + out.numel():] == SENTINEL).all())


_oracle = {}


def check_rollout(tag, p0, T, cfg, force, *, seed=11, step_offset=0, layout="in_place", game_ids=None):
    flags, host_policy, agent, stages, pad = CONFIGS[cfg]
    kw = dict(game_offset=3, step_offset=step_offset, host_policy=host_policy, agent_policy=agent, stages=stages,
              padding_value=pad)
    b, m, d = p0.shape
    key = (tag, m, d, b, T, cfg, seed, step_offset)
    if key not in _oracle:  # (one expectation for both routes and every layout)
        _oracle[key] = CO.rollout(p0, T, seed, flags=flags, record=False, game_ids=game_ids, **kw)
    want_p, want = _oracle[key]
    if game_ids is not None:
        kw["game_ids"] = dev(game_ids)
    # final states, lengths, the counts reduced by the launch itself
    src, around_intact = initial_view(p0, layout)
    before = None if src is None else src.clone()
    flat, out = guarded_output(p0, in_place=src is None)
    got = ops.rollout(out, T, seed, flags=flags | force, initial=src, record=("game_length",), **kw)
    assert np.array_equal(host(out).view(np.int32), want_p.view(np.int32))
    assert guard_rows_intact(flat, out)
    if src is not None:
        assert torch.equal(src.view(torch.int32), before.view(torch.int32))
    assert around_intact()
    assert np.array_equal(host(got["game_length"]), want["game_length"])
    assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"])
    # the counts deferred to a reduction of their own
    src, around_intact = initial_view(p0, layout)
    flat, out = guarded_output(p0, in_place=src is None)
    ws = ops.rollout_workspace(b, T, (m, d), flags=flags | force)
    got = ops.rollout(out, T, seed, flags=flags | force, initial=src, record=("game_length",), defer_counts=True,
                      workspace=ws, **kw)
    counts = ops.reduce_counts(ws, torch.zeros(T + 1, dtype=torch.int64, device="cuda"), b, T, (m, d),
                               flags=flags | force)
    assert np.array_equal(host(out).view(np.int32), want_p.view(np.int32))
    assert guard_rows_intact(flat, out)
    assert np.array_equal(host(got["game_length"]), want["game_length"])
    assert np.array_equal(host(counts).astype(np.uint64), want["done_count"])
    assert around_intact()
    return want


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_batch_sizes_at_20x3(cfg, force):
    """requests that are empty, partial and exactly full; a partial last slab behind full ones; 1, 2 and 20 steps from
    step offsets 0 and 3; in place and from a separate tensor"""
    for b in BATCHES:
        p0 = mixed_states(20, 3, b, 100 + b)
        for T in STEPS:
            for so in OFFSETS:
                layout = "separate" if (b + T + so) % 2 else "in_place"
                try:
                    check_rollout("mixed", p0, T, cfg, force[0], step_offset=so, layout=layout)
                except AssertionError as err:
                    raise AssertionError(f"{cfg} {force[1]} b={b} T={T} step_offset={so} {layout}") from err


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_input_layouts_at_20x3(layout, cfg, force):
    """the initial states in place, in a tensor of their own, and as views one float (not 16-byte aligned: the register
    path) and one game into a larger tensor; the view is unchanged, the larger tensor's other words keep their sentinel,
    and so do the guard rows of the output"""
    for b in (1, 32, 33, 65):
        p0 = mixed_states(20, 3, b, 200 + b)
        for T in (1, 20):
            try:
                check_rollout("mixed_layout", p0, T, cfg, force[0], step_offset=3, layout=layout)
            except AssertionError as err:
                raise AssertionError(f"{layout} {cfg} {force[1]} b={b} T={T}") from err


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("shape", [(20, 3)] + OTHER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_steps_from_and_into_strided_records(shape, force):
    """hk_step (rollouts take contiguous states only): records with a stride above m * d on the way in, on the way out and
    both; the gaps between the records and the sentinel rows around the output survive"""
    m, d = shape
    n = m * d
    for b in (1, 33, 65):
        p0 = mixed_states(m, d, b, 300 + b)
        rng = np.random.default_rng(b)
        cls = rng.integers(0, 2 ** d - d - 1, b).astype(np.int32)
        ax = rng.integers(0, d, b).astype(np.int32)
        want = CO.step(p0, cls, ax, stages=7)["points"].reshape(b, n)
        for in_stride, out_stride in ((n + 4, n), (n, n + 4), (n + 3, n + 5)):
            src = torch.full((b, in_stride), 7.0, dtype=torch.float32, device="cuda")
            src[:, :n] = dev(p0.reshape(b, n))
            raw = torch.empty((b + 2) * out_stride + 64, dtype=torch.float32, device="cuda")
            base = (-raw.data_ptr() % 256) // 4
            flat = raw[base:base + (b + 2) * out_stride]
            flat.view(torch.int32).fill_(SENTINEL)
            out = flat[out_stride:(b + 1) * out_stride].view(b, out_stride)
            ops.step(src, dev(cls), dev(ax), stages=7, flags=force[0], spec=(m, d), out=out)
            where = f"{shape} {force[1]} b={b} strides {in_stride} -> {out_stride}"
            assert np.array_equal(host(out[:, :n]).view(np.int32), want.view(np.int32)), where
            bits = host(flat.view(torch.int32)).reshape(b + 2, out_stride)
            assert (bits[0] == SENTINEL).all() and (bits[-1] == SENTINEL).all(), where
            assert (bits[1:-1, n:] == SENTINEL).all(), where


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("shape", OTHER_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_other_chunk_widths_and_padded_images(shape, cfg, force):
    """(10,3) and (5,3): chunks of 8 and 4 bytes; (8,4), (16,3), (20,4): images with row padding -- the register path"""
    m, d = shape
    for b in (1, 33):
        p0 = mixed_states(m, d, b, 400 + b)
        for T in STEPS:
            for so in OFFSETS:
                layout = "separate" if (b + T + so) % 2 else "in_place"
                try:
                    check_rollout("mixed", p0, T, cfg, force[0], step_offset=so, layout=layout)
                except AssertionError as err:
                    raise AssertionError(f"{shape} {cfg} {force[1]} b={b} T={T} step_offset={so} {layout}") from err


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("shape", [(20, 3), (10, 3), (20, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_rows_around_a_batch_of_33(shape, cfg, force):
    """a full wave and a wave of one game: nothing lands before the first or behind the last game (check_rollout asserts
    the sentinel rows on both sides of every output; here with the initial states at every layout)"""
    m, d = shape
    p0 = mixed_states(m, d, 33, 500)
    for layout in LAYOUTS:
        check_rollout("guard", p0, 20, cfg, force[0], layout=layout)


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_every_game_finished_at_entry(cfg, force):
    """no row, or one row somewhere: the widest game of every wave has at most one row"""
    m, d = 20, 3
    rng = np.random.default_rng(6)
    for b in (32, 33, 65):
        p0 = np.full((b, m, d), CONFIGS[cfg][4], dtype=np.float32)
        for g in range(1, b, 2):
            p0[g, int(rng.integers(0, m))] = rng.integers(0, 9, d).astype(np.float32)
        for T in (1, 20):
            want = check_rollout("finished", p0, T, cfg, force[0], step_offset=3)
            assert (want["game_length"] == 0).all()


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_twenty_live_rows_per_game(cfg, force):
    """dense states before any Newton pass: every row of every game is live, the wave maximum is at its upper bound"""
    m, d = 20, 3
    for b in (1, 33, 65):
        p0 = CO.generate_points(b, m, d, 20, 600 + b, stages=0)
        assert (p0 >= 0).all()  # every row available
        for T in (1, 2, 20):
            check_rollout("dense", p0, T, cfg, force[0], seed=7)
    # one dense game among finished ones: the maximum comes from a single pair of lanes, wherever it sits in the wave
    for at in (0, 15, 16, 31, 32, 47, 48, 64):
        p0 = np.full((65, m, d), -1.0, dtype=np.float32)
        p0[at] = CO.generate_points(1, m, d, 20, 700 + at, stages=0)[0]
        check_rollout(f"dense_at_{at}", p0, 2, cfg, force[0], seed=7)


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", ["jax", "torch", "zeillinger"])
def test_a_row_that_is_not_representable(cfg, force):
    """a partly padded row or a negative coordinate that is not the padding, in one game: the game's whole wave takes the
    generic routines, the waves around it stay on the exact path.  The row sits in the first and in the second lane's
    half of the game, first and last in the game."""
    m, d = 20, 3
    bad_rows = ((2.0, -1.0, 3.0), (1.0, -2.5, 0.0), (0.0, 5.0, -1.0), (-1.0, -1.0, 0.0))
    for case, (game, row) in enumerate(((3, 1), (40, 12), (64, 19), (31, 0))):
        p0 = mixed_states(m, d, 65, 800)
        p0[game, row] = bad_rows[case]
        assert not ((p0[game, row] >= 0).all() or (p0[game, row] == -1.0).all())
        for T in (1, 20):
            try:
                check_rollout(f"bad_{case}", p0, T, cfg, force[0], step_offset=3)
            except AssertionError as err:
                raise AssertionError(f"{cfg} {force[1]} game {game} row {row} = {bad_rows[case]} T={T}") from err


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_game_ids_at_20x3(cfg, force):
    """a permutation as game ids: these launches keep the loads through registers (the id's load in flight ahead of the
    slab's) on the shape that otherwise takes LDS-DMA; the policy stream of position g is that of game ids[g]"""
    for b in (1, 32, 33, 65):
        p0 = mixed_states(20, 3, b, 900 + b)
        ids = np.random.default_rng(b).permutation(b).astype(np.int32)
        for T in (1, 20):
            for layout in ("in_place", "separate", "offset_float"):
                try:
                    check_rollout("ids", p0, T, cfg, force[0], step_offset=3, layout=layout, game_ids=ids)
                except AssertionError as err:
                    raise AssertionError(f"{cfg} {force[1]} b={b} T={T} {layout}") from err
