"""The two-lane rollout's publish: only what changed goes back into the image it loaded.

A plain rollout on the exact path of `hk::duo_kernel` no longer refills its image with the padding row before it writes
the live rows back: it relies on every row of the loaded image being either live or exactly the padding row, on the
re-deals writing live slots only, and it overwrites just the rows that were live at the start and are dead at the end.
These cases put the live rows where that could go wrong -- the first row, the last row, scattered rows, none, all --
let them die at different steps, end the episode in wide levels, in the one-slot level and after the fixed-point exit,
and compare the final states, the game lengths and the finished-game counts with the C oracle: np.array_equal, no
tolerance.  Every case runs forced onto the two-lane kernel and once as `pick` routes it.

List semantics (rows move: sorted + compacted at the end) and a wave with a game off the exact path keep the
fill-then-scatter publish; they are here so that the choice between the two stays right."""
import zlib

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
GUARD = 0x7FC0BEEF  # a quiet NaN
MARGIN = 1024       # elements on both sides of an output

# name -> (flags, agent policy, stages, padding value)
CONFIGS = {
    "jax7": (CO.flags_of(sem="jax"), A.HK_AGENT_RANDOM, STAGES7, -1.0),  # the compiled headline configuration
    "jax15": (CO.flags_of(sem="jax"), A.HK_AGENT_RANDOM, STAGES7 | A.HK_STAGE_RESCALE, -1.0),
    "torch7": (CO.flags_of(sem="torch", noop_if_invalid=True, ignore_ended=True), A.HK_AGENT_RANDOM_LEGAL, STAGES7, -1.0),
    "torch15_pad7": (CO.flags_of(sem="torch", noop_if_invalid=True, ignore_ended=True), A.HK_AGENT_RANDOM_LEGAL,
                     STAGES7 | A.HK_STAGE_RESCALE, -7.0),
    "torch7_pad0p5": (CO.flags_of(sem="torch"), A.HK_AGENT_RANDOM, STAGES7, -0.5),
    "list": (CO.flags_of(sem="list", noop_if_invalid=True), A.HK_AGENT_RANDOM, STAGES7, -1.0),  # the old publish
    "list_compact": (CO.flags_of(sem="list", noop_if_invalid=True, compact_sorted=True), A.HK_AGENT_RANDOM,
                     A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON, -1.0),
}
SHAPES = [(20, 3), (10, 3), (5, 3), (16, 3), (8, 4), (20, 4)]
BATCHES = (33, 193, 1000)  # none a multiple of the 32 games of a wave
STEPS = (1, 2, 3, 20)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


def dev(x):
    return torch.as_tensor(np.array(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def placed_states(m, d, b, pad, seed):
    """[b, m, d] float32: the padding row everywhere, and per game a set of live rows of small integers at chosen row
    indices -- by game index modulo 8: the first row only, the last row only, first and last, the first k, the last k,
    k scattered rows, every row, none.  Small values (ties, dominated rows) make the rows die over several steps."""
    rng = np.random.default_rng(seed)
    p = np.full((b, m, d), pad, dtype=np.float32)
    for g in range(b):
        k = int(rng.integers(2, m + 1))
        kind = g % 8
        rows = {0: [0], 1: [m - 1], 2: [0, m - 1], 3: list(range(k)), 4: list(range(m - k, m)),
                5: sorted(rng.choice(m, size=k, replace=False).tolist()), 6: list(range(m)), 7: []}[kind]
        hi = (3, 6, 21)[g % 3]
        p[g, rows] = rng.integers(0, hi, (len(rows), d)).astype(np.float32)
    return p


def guarded(b, m, d, offset):
    """a [b, m, d] float32 view `offset` elements (a multiple of 4: 16 bytes) into a NaN-patterned buffer"""
    n = b * m * d
    raw = torch.empty(2 * MARGIN + n + 64, dtype=torch.float32, device="cuda")
    skip = (-raw.data_ptr() % 256) // 4
    flat = raw[skip:skip + 2 * MARGIN + n]
    flat.view(torch.int32).fill_(GUARD)
    view = flat[MARGIN + offset:MARGIN + offset + n].view(b, m, d)
    return flat, view


def margins_intact(flat, view):
    bits = host(flat.view(torch.int32))
    start = (view.data_ptr() - flat.data_ptr()) // 4
    return bool((bits[:start] == GUARD).all() and (bits[start + view.numel():] == GUARD).all())


_oracle = {}


def run_case(p0, T, cfg, force, *, separate, seed=5):
    flags, agent, stages, pad = CONFIGS[cfg]
    kw = dict(game_offset=3, step_offset=1, agent_policy=agent, stages=stages, padding_value=pad)
    key = (cfg, T, seed, p0.shape, zlib.crc32(p0.tobytes()))
    if key not in _oracle:  # (the same expectation serves both routes and both output layouts)
        _oracle[key] = CO.rollout(p0, T, seed, flags=flags, record=False, **kw)
    want_p, want = _oracle[key]
    b, m, d = p0.shape
    if separate:  # the initial states stay where they are; the final states land inside a guarded buffer
        src = dev(p0)
        before = src.clone()
        flat, out = guarded(b, m, d, 4 * (b % 3))
        got = ops.rollout(out, T, seed, flags=flags | force, initial=src, record=("game_length",), **kw)
        assert margins_intact(flat, out)
        assert torch.equal(src.view(torch.int32), before.view(torch.int32))
    else:
        out = dev(p0)
        got = ops.rollout(out, T, seed, flags=flags | force, record=("game_length",), **kw)
    # (bit patterns: the padding value and the zeros of a repositioned point included)
    assert np.array_equal(host(out).view(np.int32), want_p.view(np.int32))
    assert np.array_equal(host(got["game_length"]), want["game_length"])
    assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"])


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_placed_rows_every_episode_length(shape, cfg, force):
    """live rows at the first, last and scattered indices; episodes of 1, 2, 3 and 20 steps; ragged last waves; in
    place and into a separate guarded buffer"""
    m, d = shape
    pad = CONFIGS[cfg][3]
    for b in BATCHES:
        p0 = placed_states(m, d, b, pad, 100 * m + d + b)
        for T in STEPS:
            for separate in (False, True):
                try:
                    run_case(p0, T, cfg, force[0], separate=separate)
                except AssertionError as err:
                    raise AssertionError(f"{shape} {cfg} {force[1]} b={b} T={T} separate={separate}") from err


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", ["jax7", "torch15_pad7", "list"])
def test_generated_states_and_no_steps(cfg, force):
    """Newton-reduced states as the generator draws them (the headline's input), dense states (the widest levels), and
    an episode of no steps at all: the publish writes back exactly what it loaded"""
    m, d = 20, 3
    pad = CONFIGS[cfg][3]
    gen = CO.generate_points(32 * 7 + 5, m, d, 20, 21)
    dense = CO.generate_points(61, m, d, 20, 22, stages=0)
    p0 = np.concatenate([gen, dense])
    p0[p0 < 0] = pad
    for T in (0, 1, 7, 20, 30):  # (30: past the action window of 24 steps)
        for separate in (False, True):
            run_case(p0, T, cfg, force[0], separate=separate, seed=9)


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
@pytest.mark.parametrize("cfg", ["jax7", "torch7", "torch15_pad7"])
def test_one_game_off_the_exact_path(cfg, force):
    """a partly padded row in one game: its whole wave takes the generic routines (and the old publish); the waves
    around it stay on the exact path"""
    m, d = 20, 3
    pad = CONFIGS[cfg][3]
    p0 = placed_states(m, d, 32 * 4 + 11, pad, 77)
    p0[70, 1] = (2.0, pad, 3.0)
    p0[70, 5] = (1.0, 4.0, 0.0)
    for T in (1, 3, 20):
        for separate in (False, True):
            run_case(p0, T, cfg, force[0], separate=separate)


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
def test_zeillinger_host_keeps_the_full_publish(force):
    """Zeillinger's host parks rows by rank in the image between two deals, so its rollouts refill the image"""
    m, d = 20, 3
    p0 = np.concatenate([placed_states(m, d, 100, -1.0, 5), CO.generate_points(41, m, d, 20, 6, stages=0)])
    for T in (1, 3, 20):
        want_p, want = CO.rollout(p0, T, 13, host_policy=A.HK_HOST_ZEILLINGER, record=False)
        P = dev(p0)
        got = ops.rollout(P, T, 13, host_policy=A.HK_HOST_ZEILLINGER, flags=force[0], record=("game_length",))
        assert np.array_equal(host(P).view(np.int32), want_p.view(np.int32)), T
        assert np.array_equal(host(got["game_length"]), want["game_length"]), T
        assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"]), T


@pytest.mark.parametrize("force", FORCE, ids=lambda f: f[1])
def test_step_into_strided_records(force):
    """hk_step of the two-lane kernel into records with a stride of their own inside a guarded buffer: the gaps
    between the records and the margins survive.  A step, not a rollout: hk_rollout takes no stride (its states are
    contiguous), so the strided branch of the slab store is reached by steps only and the rollout's final store always
    runs its contiguous branch -- the one the cases above cover."""
    m, d, b = 20, 3, 193
    n, stride = m * d, m * d + 4
    p0 = placed_states(m, d, b, -1.0, 3)
    rng = np.random.default_rng(4)
    cls = rng.integers(0, 4, b).astype(np.int32)
    ax = rng.integers(0, d, b).astype(np.int32)
    want = CO.step(p0, cls, ax, stages=7)
    raw = torch.empty(2 * MARGIN + b * stride + 64, dtype=torch.float32, device="cuda")
    skip = (-raw.data_ptr() % 256) // 4
    flat = raw[skip:skip + 2 * MARGIN + b * stride]
    flat.view(torch.int32).fill_(GUARD)
    out = flat[MARGIN:MARGIN + b * stride].view(b, stride)
    ops.step(dev(p0), dev(cls), dev(ax), stages=7, flags=force[0], spec=(m, d), out=out)
    assert np.array_equal(host(out[:, :n]).view(np.int32), want["points"].reshape(b, n).view(np.int32))
    bits = host(flat.view(torch.int32))
    assert (bits[:MARGIN] == GUARD).all() and (bits[MARGIN + b * stride:] == GUARD).all()
    assert (bits[MARGIN:MARGIN + b * stride].reshape(b, stride)[:, n:] == GUARD).all()
