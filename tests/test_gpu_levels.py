"""Every level of the rollout and step staircases, bit for bit against the C oracle.

A register-resident kernel has one straight-line body per bucket of slots per lane -- a level: its own stages, its own
re-deal, its own image build.  Which level a wave runs on follows from the live rows of its widest game, so the inputs
decide what is tested.  The batches of tests/level_cases.py hold every width 1..m as some wave's widest game, with rows
on a hyperplane (an antichain: nothing is dominated at entry), so the waves come down the stairs a level or two at a
time; tests/test_level_cases.py shows on the oracle alone that they step on, publish on and re-deal between all levels.
Every test here asserts the coverage of its own inputs again before it looks at the device, so a changed seed cannot
drop a level unnoticed.  States are compared as int32 views."""
import numpy as np
import pytest
import torch

import level_cases as LC
from hironaka_amd import _abi as A
from hironaka_amd import ops
from oracle import c_oracle as CO
from test_gpu_step_loops import CONFIGS

pytestmark = pytest.mark.gpu

FORCE = {"four": A.HK_FLAG_FORCE_FOUR_LANES, "two": A.HK_FLAG_FORCE_TWO_LANES, "one": A.HK_FLAG_FORCE_ONE_LANE}
ROUTES = ("forced", "default")
CASES = [(f, s) for f in ("four", "two", "one") for s in LC.ROLLOUT_SHAPES[f]]
QUAD_SHAPES = LC.ROLLOUT_SHAPES["four"]
shape_id = lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


def dev(x):
    return torch.as_tensor(np.array(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def check(what, got, want, tag, family, paths=None):
    """np.array_equal on bit patterns; the message names the first game that differs, its wave and the wave's path"""
    got, want = bits(got), bits(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    where = ""
    if got.shape == want.shape and what != "done_count":
        games = LC.FAMILIES[family][1]
        axis = 1 if what in ("obs", "host_class", "axis", "done", "reward") else 0  # ([T, B, ...] records)
        per_game = np.moveaxis(got != want, axis, 0).reshape(got.shape[axis], -1).any(axis=1)
        g = int(np.argwhere(per_game)[0, 0])
        where = f", first at game {g}: " + (LC.describe(paths, g // games) if paths else f"wave {g // games}")
    raise AssertionError(f"{tag}: {what} differs from the oracle{where}")


def batch_of(shape, S):
    """the four-lane family's placed-width batch of a shape and S, as the rollout cases use it"""
    seed = [c for c in LC.rollout_cases("four", shape) if c[0] == S][0][2]
    return LC.batch(shape[0], shape[1], "four", S, seed)


# ---- rollouts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("cfg", LC.CONFIG_NAMES)
@pytest.mark.parametrize("family,shape", CASES, ids=shape_id)
def test_rollouts_on_every_level(family, shape, cfg, route):
    """plain rollouts of T = 0, 1, 2, 3, 5 steps from the placed-width batches, forced onto the family and as `pick`
    routes them: final states, game lengths, finished-game counts"""
    m, d = shape
    flags, host_policy, agent, stages, pad = CONFIGS[cfg]
    paths, by_sum = LC.family_paths(family, shape, cfg, CONFIGS[cfg])
    miss = LC.missing(LC.coverage(paths), family, m)
    if family == "four" and shape == (50, 4):
        miss += LC.missing_at_50_4(paths, by_sum)
    assert not miss, f"{family} lanes {shape} {cfg}: the inputs do not reach: {', '.join(miss)}"
    force = FORCE[family] if route == "forced" else 0
    for case in LC.rollout_cases(family, shape):
        S, T, _, seed = case
        p0, want_p, want, case_paths = LC.trace(family, shape, cfg, CONFIGS[cfg], case)
        P = dev(p0)
        got = ops.rollout(P, T, seed, game_offset=3, host_policy=host_policy, agent_policy=agent, stages=stages,
                          padding_value=pad, flags=flags | force, record=("game_length",))
        tag = f"{family} lanes ({route}) {shape} {cfg} S={S} T={T}"
        check("final state", host(P), want_p, tag, family, case_paths)
        check("game_length", host(got["game_length"]), want["game_length"], tag, family, case_paths)
        check("done_count", host(got["done_count"]).astype(np.uint64), want["done_count"], tag, family)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=shape_id)
def test_recording_rollout_on_every_level(shape, route):
    """the four-lane kernel's recording run: the image is rebuilt on the step's level every step -- observations and
    the small records of a 5-step episode whose waves enter on every level"""
    m, d = shape
    flags, host_policy, agent, stages, pad = CONFIGS["jax7"]
    case = [c for c in LC.rollout_cases("four", shape) if c[:2] == (40, 5)][0]
    p0, want_p, want, paths = LC.trace("four", shape, "jax7", CONFIGS["jax7"], case)
    cov = LC.coverage(paths)
    assert cov["stepped"] == set(LC.ladder("four", m)), f"{shape}: an image is never built on {set(LC.ladder('four', m)) - cov['stepped']}"
    assert any(hi != lo for hi, lo in cov["redeals"])
    P = dev(p0)
    keys = ("obs", "host_class", "axis", "done", "reward", "game_length")
    got = ops.rollout(P, 5, case[3], game_offset=3, host_policy=host_policy, agent_policy=agent, stages=stages,
                      padding_value=pad, flags=flags | (FORCE["four"] if route == "forced" else 0), record=keys)
    tag = f"four lanes ({route}) {shape} jax7 recording S=40 T=5"
    check("final state", host(P), want_p, tag, "four", paths)
    for k in keys:
        check(k, host(got[k]), want[k], tag, "four", paths)
    check("done_count", host(got["done_count"]).astype(np.uint64), want["done_count"], tag, "four")


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=shape_id)
def test_episodes_climb_back_to_the_top(shape, route):
    """episodes=3 from `initial`: every episode of a wave starts on its entry level again, after the last one's descent"""
    m, d = shape
    flags, host_policy, agent, stages, pad = CONFIGS["jax7"]
    S, T, batch_seed, seed = [c for c in LC.rollout_cases("four", shape) if c[:2] == (12, 5)][0]
    p0 = LC.batch(m, d, "four", S, batch_seed)
    total, paths = np.zeros(T + 1, dtype=np.uint64), []
    for e in range(3):
        want_p, want = CO.rollout(p0, T, seed + e, game_offset=3, host_policy=host_policy, agent_policy=agent,
                                  stages=stages, flags=flags, padding_value=pad, record=True)
        total += want["done_count"]
        states = np.concatenate([want["obs"], want_p[None]], axis=0)
        ep = LC.level_path(LC.live_rows(states), "four", m, T, LC.at_fixed_point(states))
        assert {p["entered"] for p in ep} == set(LC.ladder("four", m))
        assert any(p["publish"] < p["entered"] for p in ep), "no wave comes down: nothing to climb back from"
        paths = ep
    P = torch.empty((len(p0), m, d), device="cuda")
    got = ops.rollout(P, T, seed, game_offset=3, host_policy=host_policy, agent_policy=agent, stages=stages,
                      padding_value=pad, flags=flags | (FORCE["four"] if route == "forced" else 0), initial=dev(p0),
                      episodes=3, record=("game_length",))
    tag = f"four lanes ({route}) {shape} jax7 episodes=3 S={S} T={T}"
    check("final state", host(P), want_p, tag, "four", paths)
    check("game_length", host(got["game_length"]), want["game_length"], tag, "four", paths)
    check("done_count", host(got["done_count"]).astype(np.uint64), total, tag, "four")


@pytest.mark.parametrize("route", ROUTES)
def test_game_off_the_exact_path_in_a_wave_entering_on_10(route):
    """(50,4): a partly padded row in one game of a wave whose widest game holds 33..40 rows"""
    m, d = 50, 4
    for cfg in ("jax7", "torch7"):
        flags, host_policy, agent, stages, pad = CONFIGS[cfg]
        p0 = batch_of((m, d), 40).copy()
        w = LC.first_wave_of_width(p0, "four", 33, 40)
        n = LC.live_rows(p0[16 * w:16 * w + 16])
        assert LC.level_of("four", m, n.max()) == 10
        g = 16 * w + int(np.argwhere((n >= 2) & (n < n.max()))[0, 0])  # (not the widest game: the wave's width stays)
        row = int(np.argwhere((p0[g] >= 0).all(axis=-1))[0, 0])
        p0[g, row, 1] = pad
        for T in (1, 3):
            want_p, want = CO.rollout(p0, T, 5, game_offset=3, host_policy=host_policy, agent_policy=agent, stages=stages,
                                      flags=flags, padding_value=pad, record=False)
            P = dev(p0)
            got = ops.rollout(P, T, 5, game_offset=3, host_policy=host_policy, agent_policy=agent, stages=stages,
                              padding_value=pad, flags=flags | (FORCE["four"] if route == "forced" else 0),
                              record=("game_length",))
            tag = f"four lanes ({route}) (50, 4) {cfg} partly padded row in game {g} (wave {w}) T={T}"
            check("final state", host(P), want_p, tag, "four")
            check("game_length", host(got["game_length"]), want["game_length"], tag, "four")
            check("done_count", host(got["done_count"]).astype(np.uint64), want["done_count"], tag, "four")


# ---- single launches ----------------------------------------------------------------------------------------------------
def single_launch_batches(shape):
    """(name, states): the placed-width batches of the four-lane family; at (50,4) also S = 500 and a batch with one
    fractional coordinate in the wave of width 36 (from the packed test to the float test)"""
    m, d = shape
    out = [(f"S={S}", batch_of(shape, S)) for S in LC.sums_for(m)]
    if shape == (50, 4):
        p = batch_of(shape, 40).copy()
        w = LC.first_wave_of_width(p, "four", 36, 36)
        n = LC.live_rows(p[16 * w:16 * w + 16])
        g = 16 * w + int(n.argmax())
        row = int(np.argwhere((p[g] >= 0).all(axis=-1))[3, 0])
        p[g, row, 2] += 0.5
        assert LC.widest_per_wave(p, "four")[w] == 36
        out.append((f"S=40, a fractional coordinate in wave {w}", p))
    return out


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=shape_id)
def test_single_launches_on_every_bucket(shape, route):
    """hk_step (stages 4, 7, 15; JAX, torch and list semantics), the feature sorts in both key orders (hk_get_features:
    last coordinate first; the compacted sorted polytope: first coordinate first), hk_get_features_torch,
    hk_step_features and hk_zeillinger on batches in which every bucket is some wave's dispatch level"""
    m, d = shape
    force = FORCE["four"] if route == "forced" else 0
    rng = np.random.default_rng(17 * m + d)
    for name, p in single_launch_batches(shape):
        b = len(p)
        widest = LC.widest_per_wave(p, "four")
        assert {LC.level_of("four", m, n) for n in widest} == set(LC.ladder("four", m)), "a bucket is never dispatched"
        assert set(range(1, m + 1)) <= set(widest)
        where = lambda g: f"wave {g // 16} (widest game {widest[g // 16]} rows, bucket {LC.level_of('four', m, widest[g // 16])})"

        def same(what, got, want):
            got, want = bits(got), bits(want)
            if not np.array_equal(got, want):
                g = int(np.argwhere((got != want).reshape(b, -1).any(axis=1))[0, 0])
                raise AssertionError(f"four lanes ({route}) {shape} {name}: {what} differs from the oracle, first at game {g}, {where(g)}")

        P = dev(p)
        cls = rng.integers(0, 2 ** d - d - 1, b).astype(np.int32)
        ax = rng.integers(0, d, b).astype(np.int32)
        for sem in ("jax", "torch", "list"):
            fo = CO.flags_of(sem=sem, noop_if_invalid=sem != "jax", ignore_ended=sem == "torch")
            fp = ops.make_flags(sem, sem != "jax", sem == "torch") | force
            for stages in (4, 7, 15):
                want = CO.step(p, cls, ax, stages=stages, flags=fo)
                got = ops.step(P, dev(cls), dev(ax), stages=stages, flags=fp, want=("done", "prev_done", "reward", "num_points"))
                for k in ("points", "done", "prev_done", "reward", "num_points"):
                    same(f"hk_step {sem} stages={stages}: {k}", host(got[k]), want[k])
                if sem == "list" or shape == (50, 4) or not stages & A.HK_STAGE_SHIFT:
                    continue  # (hk_step_features: a shift by class id, JAX / torch semantics, the small games)
                for scale in (True, False):
                    want = CO.step(p, cls, ax, stages=stages, flags=fo, features=scale)
                    feat = torch.empty((b, m * d), dtype=torch.float32, device="cuda")
                    got = ops.step(P, dev(cls), dev(ax), stages=stages, flags=fp, want=("num_points",), features_out=feat,
                                   scale_observation=scale)
                    same(f"hk_step_features {sem} stages={stages} scale={scale}: points", host(got["points"]), want["points"])
                    same(f"hk_step_features {sem} stages={stages} scale={scale}: features", host(feat), want["features"])
                    same(f"hk_step_features {sem} stages={stages}: num_points", host(got["num_points"]), want["num_points"])
        for scale in (True, False):
            same(f"hk_get_features scale={scale}", host(ops.get_features(P, scale)), CO.get_features(p, scale))
        same("hk_get_features_torch", host(ops.get_features_torch(P)), CO.get_features_torch(p))
        with ops.forced(force):
            for sem in ("jax", "torch"):
                same(f"compact sorted polytope {sem}", host(ops.get_newton_polytope(P, sem=sem, compact_sorted=True)),
                     CO.get_newton_polytope(p, sem=sem, compact_sorted=True))
        for sem in ("jax", "list"):
            same(f"hk_zeillinger {sem}", host(ops.zeillinger(P, sem)), CO.zeillinger(p, sem))
