"""GPU parity tests: the HIP path (through the C ABI) against the oracle, the hand-typed
known answers and the committed outputs of the reference's torch / list siblings.

Bit-exact (np.array_equal) everywhere except where the reference itself only pins a tolerance
(rescale vs 4-digit printouts) -- stated at the assertion.
"""
import numpy as np
import pytest
import torch

from hironaka_amd import _abi as A
from hironaka_amd import ops
from oracle import c_oracle as CO
from oracle import np_oracle as NO

pytestmark = pytest.mark.gpu

FAST_SPECS = [(4, 3), (5, 3), (10, 3), (16, 3), (20, 3), (8, 4), (20, 4)]   # register-resident kernels
TEAM_SPECS = [(50, 4), (7, 3), (5, 2), (6, 5), (12, 6), (3, 3), (64, 3), (33, 4), (2, 2)]  # team kernel (f32, four lanes per game)
GENERIC_SPECS = [(7, 3), (5, 2), (6, 5), (12, 6), (3, 3), (64, 3), (70, 3), (9, 7)]


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def host(t):
    return t.detach().cpu().numpy()


def f32(x):
    return np.array(x, dtype=np.float32)


def rand_state(rng, b, m, d, dtype=np.float32, pad=-1.0, maxv=6, holes=0.3):
    p = rng.integers(0, maxv, (b, m, d)).astype(dtype)
    p[rng.random((b, m)) < holes] = pad
    return p


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


# ------------------------------------------------------------------------------------------
# known answers from the reference's tests, through both kernel families
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("force_generic", [False, True])
@pytest.mark.parametrize("sem", ["jax", "torch"])
def test_reference_sequence(golden, sem, force_generic):
    kw = dict(sem=sem, force_generic=force_generic)
    r = ops.get_newton_polytope(dev(f32(golden["newton_r"]["points"])), **kw)
    assert np.array_equal(host(r), f32(golden["newton_r"]["expected"]))
    e = golden["shift_then_newton_r2"]
    r2 = ops.get_newton_polytope(ops.shift(r, dev(np.array(e["coords"])), dev(np.array(e["axis"])), **kw), **kw)
    assert np.array_equal(host(r2), f32(e["expected"]))
    r3 = ops.reposition(r2, **kw)
    assert np.array_equal(host(r3), f32(golden["reposition_r3"]["expected"]))
    rs = ops.rescale(r3, **kw)
    # the reference pins rs only to isclose / 4 printed digits (test/testJAX.py:172)
    assert np.allclose(host(rs), f32(golden["rescale_rs"]["expected"]), atol=1e-6)
    assert np.array_equal(host(rs), CO.rescale(host(r3), sem=sem))  # and bit-exact vs the oracle


@pytest.mark.parametrize("force_generic", [False, True])
def test_reference_edge_cases(golden, force_generic):
    for key in ("newton_extreme", "torch_functions_2", "torch_remove_repeated"):
        e = golden[key]
        for sem in ("jax", "torch"):
            out = ops.get_newton_polytope(dev(f32(e["points"])), sem=sem, force_generic=force_generic)
            assert np.array_equal(host(out), f32(e["expected"])), key
    e = golden["rescale_s"]
    assert np.array_equal(host(ops.rescale(dev(f32(e["points"])), force_generic=force_generic)), f32(e["expected"]))
    e = golden["shift_fractional"]
    out = ops.shift(dev(f32(e["points"])), dev(np.array(e["coords"])), dev(np.array(e["axis"])),
                    force_generic=force_generic)
    assert np.array_equal(host(out), f32(e["expected"]))
    e = golden["torch_rescale_by_0"]
    assert np.isfinite(host(ops.rescale(dev(f32(e["points"])), sem="torch", force_generic=force_generic))).all()
    # torch semantics: illegal axis / finished game are no-ops (test/testTensorPoints.py:84-103)
    e = golden["torch_invalid_actions"]
    out = ops.shift(dev(f32(e["points"])), dev(np.array([[0, 1, 0, 0], [1, 0, 1, 1]])), dev(np.array(e["axis"])),
                    sem="torch", noop_if_invalid=True, ignore_ended=True, force_generic=force_generic)
    assert np.array_equal(host(out), f32(e["expected"]))
    e = golden["torch_ended_game"]
    for ign, key in ((True, "expected_ignore_ended"), (False, "expected_forced")):
        out = ops.shift(dev(f32(e["points"])), dev(np.array([[1, 1, 0, 0]])), dev(np.array(e["axis"])),
                        sem="torch", noop_if_invalid=True, ignore_ended=ign, force_generic=force_generic)
        assert np.array_equal(host(out), f32(e[key]))


def test_take_actions_composition(golden):
    """test/testJAX.py:461-488 through hk_step, host role and agent role (mask in the record)."""
    e = golden["take_actions_inputs"]
    p, c, a = f32(e["points"]), np.array(e["coords"]), f32(e["axis"])
    st = A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON | A.HK_STAGE_RESCALE
    out = ops.step(dev(p.reshape(2, -1)), dev(c), dev(a), stages=st, spec=(4, 3))["points"]
    assert np.array_equal(host(out), NO.rescale(NO.get_newton_polytope(NO.shift(p, c, a))))
    obs = NO.make_agent_obs(p, c)
    res = ops.step(dev(obs), None, dev(a), stages=A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON, spec=(4, 3),
                   coords_in_record=True, reward_sign=-1.0, want=("done", "prev_done", "reward"))
    assert np.array_equal(host(res["points"]), NO.get_newton_polytope(NO.shift(p, c, a)))
    assert np.array_equal(host(res["reward"]), NO.reward(host(res["done"]), host(res["prev_done"]), "agent"))


def test_features_zeillinger_codec(golden):
    e = golden["features_host"]
    assert np.array_equal(host(ops.get_features(dev(f32(e["points"])), True)), f32(e["expected"]))
    for key in ("features_agent_unscaled", "features_agent_scaled"):
        e = golden[key]
        obs = f32(e["obs"])
        feat = host(ops.get_features(dev(obs), e["scale_observation"], spec=tuple(e["spec"])))
        assert np.array_equal(np.concatenate([feat, obs[:, 9:]], axis=1), f32(e["expected"])), key
    for key in ("zeillinger_slice", "zeillinger_padded"):
        e = golden[key]
        assert host(ops.zeillinger(dev(f32(e["points"])))).tolist() == e["expected_class"]
    e = golden["zeillinger_batch"]
    cls = ops.zeillinger(dev(f32(e["points"])))
    assert np.array_equal(host(ops.decode_host_class(cls, 4, torch.int32)), np.array(e["expected_mask"]))
    e = golden["codec_d3"]
    assert np.array_equal(host(ops.decode_host_class(dev(np.arange(4, dtype=np.int32)), 3, torch.int32)),
                          np.array(e["decode_table"]))


# ------------------------------------------------------------------------------------------
# committed outputs of the reference's torch and list siblings
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("force_generic", [False, True])
def test_live_torch(live_torch, force_generic):
    tags = sorted({k.split("/")[0] for k in live_torch.files if k.startswith("m")})
    for tag in tags:
        g = lambda k: live_torch[f"{tag}/{k}"]
        pad = -1.0 if tag.endswith("pad1") else -1e-8
        kw = dict(sem="torch", padding_value=pad, force_generic=force_generic)
        p = dev(g("points"))
        assert np.array_equal(host(ops.get_newton_polytope(p, **kw)), g("newton")), tag
        assert np.array_equal(host(ops.reposition(p, **kw)), g("reposition")), tag
        assert np.array_equal(host(ops.rescale(p, **kw)), g("rescale")), tag
        mask, axis, cls = dev(g("mask")), dev(g("axis")), dev(g("class"))
        for ign in (0, 1):
            out = ops.shift(p, mask, axis, noop_if_invalid=True, ignore_ended=bool(ign), **kw)
            assert np.array_equal(host(out), g(f"shift_ign{ign}")), (tag, ign)
        # FusedGame.agent_move (trainer/fused_game.py:150-163) as ONE fused launch per variant
        start = ops.get_newton_polytope(p, **kw)
        fl = ops.make_flags("torch", True, True, force_generic=force_generic)
        res = ops.step(start, cls, axis, stages=A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON, flags=fl, padding_value=pad,
                       want=("done", "num_points"))
        assert np.array_equal(host(res["points"]), g("game_unscaled")), tag
        assert np.array_equal(host(res["done"]), g("game_ended")), tag
        assert np.array_equal(host(res["num_points"]), g("game_num_points")), tag
        res = ops.step(start, mask, axis.double(), flags=fl, padding_value=pad,
                       stages=A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON | A.HK_STAGE_RESCALE)
        assert np.array_equal(host(res["points"]), g("game_scaled")), tag


def test_live_list(live_list):
    for tag in ("m6_d4", "m10_d3", "m20_d3", "m5_d2"):
        g = lambda k: live_list[f"{tag}/{k}"]
        p = dev(g("points"))
        assert np.array_equal(host(ops.get_newton_polytope(p, sem="list")), g("newton")), tag
        assert np.array_equal(host(ops.reposition(p, sem="list")), g("reposition")), tag
        assert np.array_equal(host(ops.rescale(p, sem="list")), g("rescale")), tag
        sh = ops.shift(p, dev(g("shift_mask")), dev(g("shift_axis")), sem="list", noop_if_invalid=True)
        assert np.array_equal(host(sh), g("shift")), tag
        assert np.array_equal(host(ops.get_newton_polytope(sh, sem="list")), g("shift_newton")), tag


@pytest.mark.parametrize("scale", [0, 1])
def test_live_config1_trajectory(live_list, scale):
    """BASELINE config 1 (dim 3, 10 points, 32 games, Zeillinger vs recorded random agent):
    every state of the reference's GameHironaka run, replayed with one fused launch per move."""
    states = live_list[f"game_scale{scale}/states"]
    masks, axes = live_list[f"game_scale{scale}/masks"], live_list[f"game_scale{scale}/axes"]
    p = ops.get_newton_polytope(dev(live_list[f"game_scale{scale}/start"]), sem="list")
    if scale:
        p = ops.rescale(p, sem="list")
    assert np.array_equal(host(p), states[0])
    st = A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON | (A.HK_STAGE_RESCALE if scale else 0)
    fl = ops.make_flags("list", noop_if_invalid=True)
    for t in range(len(masks)):
        res = ops.step(p, dev(masks[t]), dev(axes[t]), stages=st, flags=fl, want=("done",))
        p = res["points"]
        assert np.array_equal(host(p), states[t + 1]), t
    assert host(res["done"]).all()


# ------------------------------------------------------------------------------------------
# seeded random inputs against the C oracle: every mode, both kernel families
# ------------------------------------------------------------------------------------------

def _check_all_ops(rng, m, d, dtype, force_generic, b=97, force_team=False):
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    for sem in ("jax", "torch", "list"):
        for pad in (-1.0, -1e-8, -2.5):
            p = rand_state(rng, b, m, d, dtype, pad)
            if m >= 3:
                p[3, 1] = [-3.0] * d  # irregular padding rows, incl. a duplicated one
                p[3, 2] = [-3.0] * d
            if d > 1:
                p[4, 0, 0] = -0.5  # a mixed-sign row
            P = dev(p)
            kw = dict(sem=sem, padding_value=pad, force_generic=force_generic, force_team=force_team)
            for compact in (False, True):
                got = host(ops.get_newton_polytope(P, compact_sorted=compact, **kw))
                assert np.array_equal(got, CO.get_newton_polytope(p, pad, sem=sem, compact_sorted=compact)), (sem, pad, compact)
            assert np.array_equal(host(ops.reposition(P, **kw)), CO.reposition(p, pad, sem=sem))
            assert np.array_equal(host(ops.rescale(P, **kw)), CO.rescale(p, pad, sem=sem))
            cls = rng.integers(0, 2 ** d - d - 1, b).astype(np.int32)
            ax = rng.integers(0, d, b).astype(np.int32)
            for noop in (False, True):
                for ign in (False, True):
                    want = CO.shift(p, cls, ax, pad, sem=sem, noop_if_invalid=noop, ignore_ended=ign)
                    got = ops.shift(P, dev(cls), dev(ax), noop_if_invalid=noop, ignore_ended=ign, **kw)
                    assert np.array_equal(host(got), want), (sem, pad, noop, ign)
            fl = ops.make_flags(sem, force_generic=force_generic, force_team=force_team)
            for stages in (A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON, 7, 15):
                want = CO.step(p, cls, ax, stages=stages, flags=CO.flags_of(sem=sem), padding_value=pad, reward_sign=-1.0)
                got = ops.step(P, dev(cls), dev(ax).to(tdt), stages=stages, flags=fl, padding_value=pad,
                               reward_sign=-1.0, want=("done", "prev_done", "reward", "num_points"))
                assert np.array_equal(host(got["points"]), want["points"]), (sem, pad, stages)
                for k in ("done", "prev_done", "reward", "num_points"):
                    assert np.array_equal(host(got[k]), want[k]), (k, sem, stages)
    q = rand_state(rng, b, m, d, dtype, -1.0)
    assert np.array_equal(host(ops.get_dones(dev(q))), CO.get_dones(q))
    assert np.array_equal(host(ops.get_num_points(dev(q))), CO.get_num_points(q))


@pytest.mark.parametrize("spec", FAST_SPECS)
def test_random_vs_oracle_fast_specs(spec):
    m, d = spec
    assert ops.has_fast_path(m, d)
    rng = np.random.default_rng(100 * m + d)
    _check_all_ops(rng, m, d, np.float32, force_generic=False, b=97 if m < 50 else 70)  # the default kernels
    for lanes in (A.HK_FLAG_FORCE_ONE_LANE, A.HK_FLAG_FORCE_TWO_LANES):
        with ops.forced(lanes):
            _check_all_ops(rng, m, d, np.float32, force_generic=False, b=97 if m < 50 else 70)


QUAD_SPECS = [(10, 3), (20, 3), (20, 4), (50, 4)]  # hk::quad_kernel (four lanes per game): hk_step


@pytest.mark.parametrize("spec", QUAD_SPECS)
def test_random_vs_oracle_four_lane_step(spec):
    """hk::quad_kernel forced for every hk_step it can serve: all semantics / stage masks / paddings of
    _check_all_ops, then the compiled action layouts (f32 mask + i32 / i64 / f32 axis, class ids) with out-of-range and
    non-integral axes, dense states (every row live: the many-slot paths), and batches that end inside a wave."""
    m, d = spec
    rng = np.random.default_rng(7 * m + d)
    with ops.forced(A.HK_FLAG_FORCE_FOUR_LANES):
        _check_all_ops(rng, m, d, np.float32, force_generic=False, b=97 if m < 50 else 70)
    for b in (1, 17, 1000):
        for dense in (False, True):
            p = CO.generate_points(b, m, d, 20, 5) if not dense else \
                rng.integers(0, 20, (b, m, d)).astype(np.float32)
            cls = rng.integers(0, 2 ** d - d - 1, b).astype(np.int32)
            ax = rng.integers(0, d, b).astype(np.int32)
            if b > 8:
                ax[3], ax[5] = d, -1
            mask = NO.decode_class(cls, d).astype(np.float32)
            for sem in ("jax", "torch", "list"):
                fl_o = CO.flags_of(sem=sem, noop_if_invalid=sem != "jax", ignore_ended=sem == "torch")
                fl_p = ops.make_flags(sem, sem != "jax", sem == "torch") | A.HK_FLAG_FORCE_FOUR_LANES
                for stages in (7, 15):
                    want = CO.step(p, cls, ax, stages=stages, flags=fl_o)
                    axes = [dev(ax), dev(ax).long(), dev(ax).float()]
                    if b > 8:
                        axes[2] = axes[2].clone()
                        axes[2][7] = 0.5  # a non-integral axis matches nothing
                        want_f = CO.step(p, cls, np.where(np.arange(b) == 7, -1, ax).astype(np.int32), stages=stages, flags=fl_o)
                    else:
                        want_f = want
                    for coords in (dev(cls), dev(mask)):
                        for ai, a in enumerate(axes):
                            got = ops.step(dev(p), coords, a, stages=stages, flags=fl_p,
                                           want=("done", "prev_done", "reward", "num_points"))
                            ref = want_f if ai == 2 else want
                            for k in ("points", "done", "prev_done", "reward", "num_points"):
                                assert np.array_equal(host(got[k]), ref[k]), (k, spec, b, dense, sem, stages, ai)


@pytest.mark.parametrize("spec", [(20, 3), (10, 3), (8, 4), (4, 3)])
def test_random_vs_oracle_team_kernel_on_fast_specs(spec):
    """the team kernel forced onto shapes that normally run register-resident"""
    m, d = spec
    rng = np.random.default_rng(17 * m + d)
    _check_all_ops(rng, m, d, np.float32, force_generic=False, b=97, force_team=True)
    P = ops.generate_points(3000, m, d, 20, seed=2)
    cls = torch.randint(0, 2 ** d - d - 1, (3000,), device="cuda", dtype=torch.int32)
    ax = torch.randint(0, d, (3000,), device="cuda", dtype=torch.int32)
    a = ops.step(P, cls, ax, stages=7)["points"]
    assert torch.equal(a, ops.step(P, cls, ax, stages=7, flags=A.HK_FLAG_FORCE_TEAM)["points"])
    Q1, Q2 = P.clone(), P.clone()
    r1 = ops.rollout(Q1, 15, 4, record=("axis", "done"))
    r2 = ops.rollout(Q2, 15, 4, record=("axis", "done"), flags=A.HK_FLAG_FORCE_TEAM)
    assert torch.equal(Q1, Q2) and torch.equal(r1["done"], r2["done"]) and torch.equal(r1["done_count"], r2["done_count"])
    g1 = ops.generate_points(500, m, d, 20, seed=8)
    assert torch.equal(g1, ops.generate_points(500, m, d, 20, seed=8, flags=A.HK_FLAG_FORCE_TEAM))


@pytest.mark.parametrize("spec", TEAM_SPECS)
def test_random_vs_oracle_team_specs(spec):
    """f32 shapes without a register specialisation run on the team kernel (four lanes per game,
    hk_team_kernel.h)"""
    m, d = spec
    assert not ops.has_fast_path(m, d)
    rng = np.random.default_rng(31 * m + d)
    _check_all_ops(rng, m, d, np.float32, force_generic=False, b=70 if m < 50 else 67)


@pytest.mark.parametrize("spec", [(50, 4), (33, 4), (64, 3), (12, 6), (7, 3), (2, 2)])
def test_team_kernel_rollout_generate_match_other_kernels(spec):
    """fused rollouts (with the squeeze of the register rows), per-step observations and the generator on
    the team kernel against the generic kernel and the C oracle"""
    m, d = spec
    b = 1000
    P = ops.generate_points(b, m, d, 20, seed=5)
    assert torch.equal(P, ops.generate_points(b, m, d, 20, seed=5, flags=A.HK_FLAG_FORCE_TEAM))
    assert torch.equal(P, ops.generate_points(b, m, d, 20, seed=5, flags=A.HK_FLAG_FORCE_GENERIC))
    assert np.array_equal(host(P), CO.generate_points(b, m, d, 20, 5))
    rec = ("obs", "host_class", "axis", "done", "reward", "game_length")
    outs = []
    for fl in (0, A.HK_FLAG_FORCE_TEAM, A.HK_FLAG_FORCE_GENERIC):
        Q = P.clone()
        r = ops.rollout(Q, 12, 9, record=rec, flags=fl)
        outs.append((Q, r))
    for Q, r in outs[1:]:
        assert torch.equal(outs[0][0], Q)
        for k in rec + ("done_count",):
            assert torch.equal(outs[0][1][k], r[k]), k
    want, wrec = CO.rollout(host(P), 12, 9, record=True)
    assert np.array_equal(host(outs[0][0]), want)
    assert np.array_equal(host(outs[0][1]["obs"]), wrec["obs"])
    assert np.array_equal(host(outs[0][1]["done_count"]), wrec["done_count"])
    # ragged tail: the last wave holds fewer than 16 games
    for bb in (1, 15, 17, 63):
        Pb = P[:bb].contiguous()
        cls = torch.randint(0, 2 ** d - d - 1, (bb,), device="cuda", dtype=torch.int64)
        ax = torch.randint(0, d, (bb,), device="cuda", dtype=torch.int64)
        got = ops.step(Pb, cls, ax, stages=15, want=("done", "reward"))
        ref = CO.step(host(Pb), host(cls), host(ax), stages=15)
        assert np.array_equal(host(got["points"]), ref["points"]) and np.array_equal(host(got["done"]), ref["done"])


@pytest.mark.parametrize("spec", GENERIC_SPECS + [(20, 3), (10, 3)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_random_vs_oracle_generic(spec, dtype):
    m, d = spec
    rng = np.random.default_rng(7 * m + d)
    _check_all_ops(rng, m, d, dtype, force_generic=True, b=70 if m < 64 else 40)


def test_fast_equals_generic_on_dense_games():
    """all 20 points alive, distinct and mutually non-dominating is the worst case of the pair loop"""
    rng = np.random.default_rng(1)
    b, m, d = 256, 20, 3
    base = np.stack([np.arange(m), m - 1 - np.arange(m), np.zeros(m)], axis=1).astype(np.float32)  # antichain
    p = np.repeat(base[None], b, 0)
    for g in range(b):
        p[g] = p[g][rng.permutation(m)]
        p[g, :, 2] = rng.integers(0, 3, m)
    a = host(ops.get_newton_polytope(dev(p)))
    assert np.array_equal(a, host(ops.get_newton_polytope(dev(p), force_generic=True)))
    assert np.array_equal(a, CO.get_newton_polytope(p))


def test_large_values_and_float_axis():
    """values near 2^24 (exact f32 integers) and float-typed axis (test/testJAX.py:474)"""
    rng = np.random.default_rng(3)
    p = (rng.integers(0, 1 << 22, (200, 20, 3))).astype(np.float32)
    cls = rng.integers(0, 4, 200).astype(np.int64)
    ax = rng.integers(0, 3, 200).astype(np.float32)
    want = CO.step(p, cls, ax, stages=7)
    got = ops.step(dev(p), dev(cls), dev(ax), stages=7)
    assert np.array_equal(host(got["points"]), want["points"])


# ------------------------------------------------------------------------------------------
# generator, fused rollout, sharding
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec,force_generic", [((20, 3), False), ((20, 3), True), ((10, 3), False), ((50, 4), False),
                                                ((7, 3), True), ((7, 3), False), ((12, 6), False)])
def test_generate_matches_oracle(spec, force_generic):
    m, d = spec
    fl = A.HK_FLAG_FORCE_GENERIC if force_generic else 0
    for resc in (False, True):
        got = ops.generate_points(300, m, d, 20, seed=42, game_offset=11, rescale=resc, flags=fl)
        want = CO.generate_points(300, m, d, 20, 42, 11, stages=A.HK_STAGE_NEWTON | A.HK_STAGE_REPOSITION | (A.HK_STAGE_RESCALE if resc else 0))
        assert np.array_equal(host(got), want)
    raw = ops.generate_points(300, m, d, 7, seed=1, newton=False, reposition=False, flags=fl)
    assert np.array_equal(host(raw), NO.random_ints(300, m, d, 7, 1).astype(np.float32))


@pytest.mark.parametrize("spec", [(10, 3), (20, 3), (20, 4), (50, 4)])
def test_generate_families_match_oracle(spec):
    """hk_generate_points on the shapes with a four-lane generator (hk::quadgen_kernel, the default) against the oracle
    and against the one-lane / team / generic kernels forced by flag: batches that leave a wave partly empty, one
    game, value ranges that make many duplicate rows (max_value 2) and none (max_value 1000), every stage subset, torch
    semantics, a game offset beyond 2^32, and a padding value the four-lane kernel declines under JAX semantics
    (_jax_ops.py:65 fills duplicates with -1.0 whatever the padding is: the exact generic routines take it)."""
    m, d = spec
    N, R, S = A.HK_STAGE_NEWTON, A.HK_STAGE_REPOSITION, A.HK_STAGE_RESCALE
    families = (0, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_ONE_LANE, A.HK_FLAG_FORCE_TEAM, A.HK_FLAG_FORCE_GENERIC)
    cases = [dict(b=b, mv=20, st=N | R, off=3, pad=-1.0, sem="jax") for b in (1, 15, 16, 17, 63, 65, 300)]
    cases += [dict(b=200, mv=mv, st=N | R, off=0, pad=-1.0, sem="jax") for mv in (1, 2, 3, 1000, 2 ** 31 - 1)]
    cases += [dict(b=130, mv=20, st=st, off=(1 << 33) + 5, pad=-1.0, sem="jax") for st in (0, N, R, S, N | S, N | R | S)]
    cases += [dict(b=130, mv=20, st=st, off=7, pad=pad, sem="torch") for st in (N, N | R | S) for pad in (-1.0, -2.5)]
    cases += [dict(b=130, mv=20, st=N | R, off=7, pad=-2.5, sem="jax")]
    for c in cases:
        fo = CO.flags_of(sem=c["sem"])
        want = CO.generate_points(c["b"], m, d, c["mv"], 9, c["off"], stages=c["st"], padding_value=c["pad"], flags=fo)
        for fam in families:
            got = ops.generate_points(c["b"], m, d, c["mv"], seed=9, game_offset=c["off"], newton=bool(c["st"] & N),
                                      reposition=bool(c["st"] & R), rescale=bool(c["st"] & S), padding_value=c["pad"],
                                      flags=ops.make_flags(c["sem"]) | fam)
            assert np.array_equal(host(got), want), (c, fam)


@pytest.mark.parametrize("max_value", [64, 65, 127, 128])
@pytest.mark.parametrize("spec", [(20, 3), (50, 4)])
def test_generate_value_edges_match_oracle(spec, max_value):
    """hk_generate_points on both sides of the generator's two value edges, on every family: max_value 64 | 65 (eight
    against four elements per Philox block) and 127 | 128 (largest draw 126 | 127: the packed byte test against the
    float loop of the Newton stage) -- a batch that ends inside a wave and one of several workgroups"""
    m, d = spec
    N, R, S = A.HK_STAGE_NEWTON, A.HK_STAGE_REPOSITION, A.HK_STAGE_RESCALE
    families = (0, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_ONE_LANE, A.HK_FLAG_FORCE_TEAM, A.HK_FLAG_FORCE_GENERIC)
    for b in (17, 200):
        raw = CO.generate_points(b, m, d, max_value, 9, 3, stages=0)
        assert raw.max() == max_value - 1, "the batch does not draw the largest value"
        for st in (0, N, N | R, N | R | S):
            want = CO.generate_points(b, m, d, max_value, 9, 3, stages=st)
            for fam in families:
                got = ops.generate_points(b, m, d, max_value, seed=9, game_offset=3, newton=bool(st & N),
                                          reposition=bool(st & R), rescale=bool(st & S), flags=fam)
                assert np.array_equal(host(got).view(np.int32), want.view(np.int32)), (spec, max_value, b, st, fam)


@pytest.mark.parametrize("spec,force_generic", [((20, 3), False), ((20, 3), True), ((10, 3), False), ((8, 4), False),
                                                ((6, 5), True), ((50, 4), False), ((7, 3), False), ((6, 5), False)])
def test_rollout_matches_oracle(spec, force_generic):
    m, d = spec
    p0 = CO.generate_points(333, m, d, 20, 5)
    # (the recording rollouts of every family that serves the shape: default, four lanes, two lanes / team)
    families = (A.HK_FLAG_FORCE_GENERIC,) if force_generic else (0, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_TWO_LANES,
                                                                  A.HK_FLAG_FORCE_TEAM)
    for hp in (A.HK_HOST_RANDOM, A.HK_HOST_ALL_COORD, A.HK_HOST_ZEILLINGER):
        for ap in (A.HK_AGENT_RANDOM, A.HK_AGENT_RANDOM_LEGAL, A.HK_AGENT_CHOOSE_FIRST, A.HK_AGENT_CHOOSE_LAST):
            for T, so in ((9, 3), (27, 0)):
                want_p, want = CO.rollout(p0, T, 99, game_offset=17, step_offset=so, host_policy=hp, agent_policy=ap)
                for fl in families:
                    P = dev(p0.copy())
                    got = ops.rollout(P, T, 99, game_offset=17, step_offset=so, host_policy=hp, agent_policy=ap, flags=fl,
                                      record=("obs", "host_class", "axis", "done", "reward", "game_length"))
                    assert np.array_equal(host(P), want_p), (hp, ap, T, fl)
                    for k in ("obs", "host_class", "axis", "done", "reward", "game_length"):
                        assert np.array_equal(host(got[k]), want[k]), (k, hp, ap, T, fl)
                    assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"])


@pytest.mark.parametrize("spec", [(20, 3), (10, 3), (8, 4), (20, 4), (50, 4)])
def test_small_records_without_observations_match_oracle(spec):
    """The small per-step records alone (host class, axis, done, reward): the two-lane plain rollout writes them from
    its action window and the games' first finished steps (`duo_kernel<..., ACTS>`), the four-lane kernel likewise; the
    one-lane kernel stores them per step.  Episodes inside one window of 24 steps, across windows (50 steps from an odd
    offset), a ragged last wave, one game off the exact path (a partly padded row: whole-wave slow path), both the
    compiled JAX configuration and a run-time configured one."""
    m, d = spec
    p0 = CO.generate_points(32 * 5 + 7, m, d, 20, 11)
    p0[40, 1, 0] = -1.0  # partly padded row: the wave of game 40 takes the generic routines
    fields = ("host_class", "axis", "done", "reward", "game_length")
    stages = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON
    for hp, ap, st in ((A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM, stages), (A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM_LEGAL, None),
                       (A.HK_HOST_ALL_COORD, A.HK_AGENT_CHOOSE_LAST, None)):
        kw = dict(host_policy=hp, agent_policy=ap, **({"stages": st} if st is not None else {}))
        for T, so in ((9, 3), (24, 0), (50, 5)):
            want_p, want = CO.rollout(p0, T, 7, game_offset=3, step_offset=so, **kw)
            for fl in (0, A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_ONE_LANE):
                if fl == A.HK_FLAG_FORCE_TWO_LANES and m > 32:
                    continue
                P = dev(p0.copy())
                got = ops.rollout(P, T, 7, game_offset=3, step_offset=so, flags=fl, record=fields, **kw)
                assert np.array_equal(host(P), want_p), (hp, ap, T, fl)
                for k in fields:
                    assert np.array_equal(host(got[k]), want[k]), (k, hp, ap, T, fl)
                assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"])
    if spec == (20, 3):  # the default route above 32 768 games: the two-lane kernel takes the small records
        big = CO.generate_points(40000, m, d, 20, 12)
        want_p, want = CO.rollout(big, 20, 7)
        P = dev(big.copy())
        got = ops.rollout(P, 20, 7, record=fields)
        assert np.array_equal(host(P), want_p)
        for k in fields:
            assert np.array_equal(host(got[k]), want[k]), k


@pytest.mark.parametrize("spec", [(20, 3), (10, 3), (4, 3), (5, 3), (16, 3), (8, 4), (20, 4), (50, 4)])
def test_zeillinger_host_plain_rollouts_match_oracle(spec):
    """Plain rollouts against Zeillinger's host (jax/players.py:55-109) on the two-lane kernel (`duo_kernel<..., ZEIL>`:
    the pair test split over the two lanes of a game, ties by the explicit pair index), the four-lane kernel
    (`quadroll_kernel<..., ZEIL>`: the default at (50,4) and for small batches) and the one-lane kernel, against the oracle: wide states (every bucket of the staircase), states of small integers (many equal
    characteristic vectors: the first pair in row-major order must win), ragged waves, a step offset inside a Philox
    block, one game off the exact path."""
    m, d = spec
    for max_value, seed in ((20, 31), (3, 32), (2, 33)):
        p0 = CO.generate_points(32 * 6 + 9, m, d, max_value, seed)
        if max_value == 20:
            dense = CO.generate_points(64, m, d, 20, 34, stages=0)  # every row live: the widest buckets
            p0 = np.concatenate([p0, dense])
            p0[70, 1, 0] = -1.0  # partly padded row: whole-wave slow path
        for ap in (A.HK_AGENT_RANDOM, A.HK_AGENT_RANDOM_LEGAL, A.HK_AGENT_CHOOSE_FIRST):
            for T, so in ((20, 0), (11, 6)):
                want_p, want = CO.rollout(p0, T, 13, game_offset=9, step_offset=so, host_policy=A.HK_HOST_ZEILLINGER,
                                          agent_policy=ap, record=False)
                for fl in (0, A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_ONE_LANE):
                    if m > 32 and fl in (A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_ONE_LANE):
                        continue
                    P = dev(p0.copy())
                    got = ops.rollout(P, T, 13, game_offset=9, step_offset=so, host_policy=A.HK_HOST_ZEILLINGER,
                                      agent_policy=ap, flags=fl, record=("game_length",))
                    assert np.array_equal(host(P), want_p), (max_value, ap, T, fl)
                    assert np.array_equal(host(got["game_length"]), want["game_length"]), (max_value, ap, T, fl)
                    assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"])


@pytest.mark.parametrize("spec", [(20, 3), (50, 4), (5, 3)])
def test_tiny_batches_and_degenerate_episodes(spec):
    """One game, a wave plus one game, no steps at all, one step, one step past an action window -- with game ids, every
    family, plain / small records / everything recorded."""
    m, d = spec
    small = ("host_class", "axis", "done", "reward", "game_length")
    for b in (1, 17, 65):
        p0 = CO.generate_points(b, m, d, 20, 8)
        ids = np.random.default_rng(b).permutation(b).astype(np.int32)
        for T in (0, 1, 25):
            for hp in (A.HK_HOST_RANDOM, A.HK_HOST_ZEILLINGER):
                want_p, want = CO.rollout(p0, T, 5, step_offset=2, host_policy=hp, agent_policy=A.HK_AGENT_RANDOM, game_ids=ids)
                for fl in (0, A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_ONE_LANE):
                    if m > 32 and fl not in (0, A.HK_FLAG_FORCE_FOUR_LANES):
                        continue
                    for rec in (("game_length",), small, ("obs",) + small):
                        P = dev(p0.copy())
                        got = ops.rollout(P, T, 5, step_offset=2, host_policy=hp, agent_policy=A.HK_AGENT_RANDOM, flags=fl,
                                          record=rec, game_ids=dev(ids))
                        assert np.array_equal(host(P), want_p), (b, T, hp, fl, rec)
                        for k in rec:
                            assert np.array_equal(host(got[k]), want[k].reshape(got[k].shape)), (k, b, T, hp, fl)
                        assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"])


@pytest.mark.parametrize("spec", [(20, 3), (50, 4), (8, 4)])
def test_long_episodes_match_oracle(spec):
    """Episodes of more than 64 steps (the finished-game counts go out 64 steps per atomic instruction, the action windows
    and the small records window by window): every family, plain and with the small records, random and Zeillinger's host."""
    m, d = spec
    p0 = CO.generate_points(32 * 3 + 5, m, d, 20, 3)
    small = ("host_class", "axis", "done", "reward", "game_length")
    for T, so in ((130, 0), (67, 3)):
        for hp in (A.HK_HOST_RANDOM, A.HK_HOST_ZEILLINGER):
            want_p, want = CO.rollout(p0, T, 5, step_offset=so, host_policy=hp, agent_policy=A.HK_AGENT_RANDOM_LEGAL)
            for fl in (0, A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_ONE_LANE):
                if m > 32 and fl in (A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_ONE_LANE):
                    continue
                for rec in (("game_length",), small):
                    P = dev(p0.copy())
                    got = ops.rollout(P, T, 5, step_offset=so, host_policy=hp, agent_policy=A.HK_AGENT_RANDOM_LEGAL,
                                      flags=fl, record=rec)
                    assert np.array_equal(host(P), want_p), (T, hp, fl, rec)
                    for k in rec:
                        assert np.array_equal(host(got[k]), want[k]), (k, T, hp, fl)
                    assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"]), (T, hp, fl)


@pytest.mark.parametrize("spec", [(20, 3), (8, 4), (50, 4), (7, 3)])
def test_reordered_batch_with_game_ids_rolls_out_like_the_original(spec):
    """`hk_rollout_desc.game_ids` (round 3): a batch binned by live rows (`ops.bin_by_live_rows`) with the permutation as
    game ids gives, game by game, what the original order gives -- against the oracle with the same ids, and as the
    permutation of the plain run; every family (four lanes, two lanes, one lane, team, generic),
    records included."""
    m, d = spec
    p0 = CO.generate_points(32 * 9 + 5, m, d, 20, 21)
    P0 = dev(p0.copy())
    binned, ids = ops.bin_by_live_rows(P0)
    idn = host(ids)
    assert sorted(idn.tolist()) == list(range(p0.shape[0]))
    cnt = (p0[:, :, 0] >= 0).sum(1)
    assert np.array_equal(host(binned), p0[idn])
    group, rot = ops.bin_group(m, d)
    if group:  # the on-device order: local to groups, strata of sixteen (include/hironaka_hip.h) -- the oracle's
        assert np.array_equal(idn, CO.bin_by_live_rows(p0, group, rot)[1])
    else:      # the tensor library's global stable sort
        assert np.all(np.diff(cnt[idn]) <= 0)
    fields = ("host_class", "axis", "done", "reward", "game_length")
    for hp, ap in ((A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM), (A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM_LEGAL),
                   (A.HK_HOST_ZEILLINGER, A.HK_AGENT_CHOOSE_FIRST)):
        for T, so in ((20, 0), (30, 6)):
            plain_p, plain = CO.rollout(p0, T, 5, game_offset=100, step_offset=so, host_policy=hp, agent_policy=ap)
            want_p, want = CO.rollout(p0[idn], T, 5, game_offset=100, step_offset=so, host_policy=hp, agent_policy=ap,
                                      game_ids=idn)
            # the oracle itself: the re-ordered run is the permutation of the plain one
            assert np.array_equal(want_p, plain_p[idn]) and np.array_equal(want["game_length"], plain["game_length"][idn])
            assert np.array_equal(want["done_count"], plain["done_count"])
            for fl in (0, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_ONE_LANE, A.HK_FLAG_FORCE_TEAM,
                       A.HK_FLAG_FORCE_GENERIC):
                if fl == A.HK_FLAG_FORCE_TWO_LANES and m > 32:
                    continue
                for rec in (fields, ("obs",) + fields, ("game_length",)):
                    Q = binned.clone()
                    got = ops.rollout(Q, T, 5, game_offset=100, step_offset=so, host_policy=hp, agent_policy=ap, flags=fl,
                                      record=rec, game_ids=ids)
                    assert np.array_equal(host(Q), want_p), (hp, ap, T, fl, rec)
                    for k in rec:
                        assert np.array_equal(host(got[k]), want[k]), (k, hp, ap, T, fl)
                    assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"])


@pytest.mark.parametrize("spec", [(50, 4), (40, 3), (33, 4)])
def test_dense_states_of_large_games_packed_and_float_tests_match_oracle(spec):
    """hk_step on states no Newton pass has thinned (more than 8 slots per lane): integral rows whose coordinates stay
    below 127 after the shift and the reposition take the domination test on packed rows (`qg_newton_on_packed`),
    anything else -- a coordinate of 127 and more, fractional rows, a mix inside one wave -- the float tests.  Every
    variant against the oracle: value ranges around the packing limit, duplicates (small ranges), holes, every stage
    subset with a Newton stage, three semantics."""
    m, d = spec
    rng = np.random.default_rng(11 * m + d)
    b = 16 * 5 + 3
    cls = rng.integers(0, 2 ** d - d - 1, b).astype(np.int32)
    ax = rng.integers(0, d, b).astype(np.int32)
    cases = {}
    for maxv in (2, 4, 20, 32, 43, 64, 127, 128, 1000):
        cases[f"int{maxv}"] = rng.integers(0, maxv, (b, m, d)).astype(np.float32)
    cases["at_the_limit"] = rng.integers(120, 128, (b, m, d)).astype(np.float32)
    cases["fractional"] = (rng.integers(0, 40, (b, m, d)) / np.float32(8)).astype(np.float32)
    mixed = rng.integers(0, 20, (b, m, d)).astype(np.float32)
    mixed[5, 3, 1] = 0.5       # one fractional coordinate in the batch: its wave takes the float test
    mixed[40, 7, 0] = 300.0    # one coordinate past the limit
    cases["mixed"] = mixed
    holes = rng.integers(0, 20, (b, m, d)).astype(np.float32)
    holes[rng.random((b, m)) < 0.15] = -1.0
    cases["holes"] = holes
    for name, p in cases.items():
        for sem in ("jax", "torch", "list"):
            fl_o = CO.flags_of(sem=sem, noop_if_invalid=sem != "jax", ignore_ended=sem == "torch")
            fl_p = ops.make_flags(sem, sem != "jax", sem == "torch")
            for stages in (4, 6, 7, 15):
                want = CO.step(p, cls, ax, stages=stages, flags=fl_o)
                for fam in (0, A.HK_FLAG_FORCE_FOUR_LANES):
                    if fam and (m, d) != (50, 4):  # (the shapes without a four-lane step kernel: the default route only)
                        continue
                    got = ops.step(dev(p), dev(cls), dev(ax), stages=stages, flags=fl_p | fam, want=("done", "num_points"))
                    assert np.array_equal(host(got["points"]), want["points"]), (name, sem, stages, fam)
                    assert np.array_equal(host(got["num_points"]), want["num_points"]), (name, sem, stages, fam)


@pytest.mark.parametrize("spec", [(10, 3), (20, 3), (20, 4), (50, 4)])
def test_sorted_plain_rollouts_on_four_lanes_match_oracle(spec):
    """list semantics / COMPACT_SORTED on the four-lane rollout kernel (`quadroll_kernel<..., kHotList>`): the state is
    ranked once, when it is published -- at whatever level of the staircase the episode ends (one step from dense
    states: the widest level's rolled ranking; long episodes: the DPP ranking), before a pending rescale.  Against the
    oracle and the other families, from generated, dense, fractional and partly finished states, with a ragged last
    wave and one game off the exact path."""
    m, d = spec
    rng = np.random.default_rng(5 * m + d)
    b = 16 * 9 + 5
    starts = {"generated": CO.generate_points(b, m, d, 20, 4),
              "dense": rng.integers(0, 30, (b, m, d)).astype(np.float32),
              "fractional": (rng.integers(0, 9, (b, m, d)) / np.float32(9)).astype(np.float32)}
    starts["holes"] = np.where(rng.random((b, m, 1)) < 0.5, np.float32(-1.0), starts["dense"]).astype(np.float32)
    starts["irregular"] = starts["generated"].copy()
    starts["irregular"][21, 1, 0] = -1.0
    for name, p0 in starts.items():
        for sem, compact in (("list", False), ("jax", True), ("torch", True)):
            fo = CO.flags_of(sem=sem, noop_if_invalid=sem != "jax", ignore_ended=sem == "torch", compact_sorted=compact)
            fp = ops.make_flags(sem, sem != "jax", sem == "torch", compact_sorted=compact)
            for stages in (7, 15):
                for T in (0, 1, 2, 7, 30):
                    for hp, ap in ((A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM_LEGAL), (A.HK_HOST_ALL_COORD, A.HK_AGENT_CHOOSE_LAST)):
                        want_p, want = CO.rollout(p0, T, 3, game_offset=9, host_policy=hp, agent_policy=ap, stages=stages,
                                                  flags=fo, record=False)
                        for fam in (0, A.HK_FLAG_FORCE_FOUR_LANES):
                            Q = dev(p0.copy())
                            got = ops.rollout(Q, T, 3, game_offset=9, host_policy=hp, agent_policy=ap, stages=stages,
                                              flags=fp | fam, record=("game_length",))
                            assert np.array_equal(host(Q), want_p), (name, sem, compact, stages, T, hp, fam)
                            assert np.array_equal(host(got["game_length"]), want["game_length"])
                            assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"])


@pytest.mark.parametrize("spec", [(10, 3), (20, 3), (20, 4), (50, 4)])
def test_binning_on_the_device_matches_oracle(spec):
    """hk_bin_by_live_rows / hk_generate_points_binned (ABI 4): the order local to groups of games (widest first, equal
    games in their order, the k-th sixteen games of all full groups together, a partial last group in place) equals
    the oracle's on batches of one game, one wave, one group +- one game, several groups and a ragged tail; the
    generator's binned output is the binned output of the plain generator; the counts per position."""
    m, d = spec
    group, rot = ops.bin_group(m, d)
    assert group in (64, 256) and rot == 16
    for b in (1, 15, 16, 17, group - 1, group, group + 1, 3 * group, 3 * group + 77):
        p0 = CO.generate_points(b, m, d, 20, 13, 5)
        want_p, want_ids, want_np = CO.bin_by_live_rows(p0, group, rot)
        got_p, got_ids, got_np = ops.bin_by_live_rows(dev(p0.copy()), want_num_points=True)
        assert np.array_equal(host(got_ids), want_ids), b
        assert np.array_equal(host(got_p), want_p) and np.array_equal(host(got_np), want_np), b
        gen_p, gen_ids, gen_np = ops.generate_points_binned(b, m, d, 20, 13, game_offset=5, want_num_points=True)
        assert np.array_equal(host(gen_ids), want_ids) and np.array_equal(host(gen_p), want_p), b
        assert np.array_equal(host(gen_np), want_np), b
    # states with holes in the middle, rescaled values, other stage subsets, torch semantics
    p0 = CO.generate_points(2 * group + 9, m, d, 20, 3)
    p0[::3] = CO.rollout(p0[::3], 3, 8, record=False)[0]
    want_p, want_ids, _ = CO.bin_by_live_rows(p0, group, rot)
    got_p, got_ids = ops.bin_by_live_rows(dev(p0.copy()))
    assert np.array_equal(host(got_ids), want_ids) and np.array_equal(host(got_p), want_p)
    for kw, st, sem in ((dict(rescale=True), A.HK_STAGE_NEWTON | A.HK_STAGE_REPOSITION | A.HK_STAGE_RESCALE, "jax"),
                        (dict(reposition=False), A.HK_STAGE_NEWTON, "torch")):
        raw = CO.generate_points(group + 40, m, d, 9, 2, stages=st, flags=CO.flags_of(sem=sem))
        want_p, want_ids, _ = CO.bin_by_live_rows(raw, group, rot)
        gen_p, gen_ids = ops.generate_points_binned(group + 40, m, d, 9, 2, flags=ops.make_flags(sem), **kw)
        assert np.array_equal(host(gen_ids), want_ids) and np.array_equal(host(gen_p), want_p), kw


@pytest.mark.parametrize("spec", [(20, 3), (10, 3), (4, 3), (8, 4), (20, 4), (50, 4)])
def test_compiled_rollout_configurations_match_oracle(spec):
    """The two rollout configurations the register-resident kernels carry as compile-time constants (SURVEY
    8d's protocols: JAX semantics + uniform axis; torch semantics + an axis among the host's coordinates,
    illegal / finished games not shifted) without records -- the launches bench.py times -- against the
    oracle, and the same requests with one flag more (which the runtime-configured kernel serves)"""
    m, d = spec
    p0 = CO.generate_points(1111, m, d, 20, 6)
    stages = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON
    torch_flags = ops.make_flags("torch", noop_if_invalid=True, ignore_ended=True)
    for flags_p, flags_o, ap in (
            (0, 0, A.HK_AGENT_RANDOM),
            (torch_flags, CO.flags_of(sem="torch", noop_if_invalid=True, ignore_ended=True), A.HK_AGENT_RANDOM_LEGAL),
            (ops.make_flags("torch", noop_if_invalid=True), CO.flags_of(sem="torch", noop_if_invalid=True),
             A.HK_AGENT_RANDOM_LEGAL)):
        for T in (1, 20):
            want_p, want = CO.rollout(p0, T, 31, game_offset=5, host_policy=A.HK_HOST_RANDOM, agent_policy=ap,
                                      stages=stages, flags=flags_o, record=False)
            # hk::duo_kernel / hk::fast_kernel / hk::quadroll_kernel (where they exist; elsewhere the flags change nothing)
            for lanes in (0, A.HK_FLAG_FORCE_ONE_LANE, A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_FOUR_LANES):
                P = dev(p0.copy())
                got = ops.rollout(P, T, 31, game_offset=5, host_policy=A.HK_HOST_RANDOM, agent_policy=ap,
                                  stages=stages, flags=flags_p | lanes, record=("game_length",))
                assert np.array_equal(host(P), want_p), (flags_p, T, lanes)
                assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"]), (flags_p, T)
                assert np.array_equal(host(got["game_length"]), want["game_length"]), (flags_p, T, lanes)


@pytest.mark.parametrize("family,spec", [("two", s) for s in ((20, 3), (10, 3), (5, 3), (16, 3), (8, 4), (20, 4))] +
                         [("quad", s) for s in ((20, 3), (10, 3), (20, 4), (50, 4))])
def test_forced_rollout_families_match_oracle(family, spec):
    """hk::duo_kernel (two lanes per game) and hk::quadroll_kernel (four lanes per game), both with decoded action
    windows of 24 steps, forced at every batch size, against the oracle: episode lengths
    on both sides of every round / window boundary, a step offset that is not a multiple of a Philox block, batches
    that leave waves / workgroups partly or wholly empty, the run-time configured variant (other policies, rescale, no
    reposition), a padding value that sends a workgroup down the exact generic path, and non-canonical games in one
    workgroup only"""
    m, d = spec
    force = A.HK_FLAG_FORCE_TWO_LANES if family == "two" else A.HK_FLAG_FORCE_FOUR_LANES
    stages = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON
    torch_flags = ops.make_flags("torch", noop_if_invalid=True, ignore_ended=True)
    torch_flags_o = CO.flags_of(sem="torch", noop_if_invalid=True, ignore_ended=True)
    cases = []
    for T in (0, 1, 2, 3, 4, 5, 6, 8, 9, 12, 13, 20, 24, 25, 41, 49):
        cases.append(dict(b=700, T=T, so=0, fp=0, fo=0, hp=A.HK_HOST_RANDOM, ap=A.HK_AGENT_RANDOM, st=stages, pad=-1.0))
    for b in (1, 31, 33, 255, 257, 513, 1500):
        cases.append(dict(b=b, T=20, so=3, fp=0, fo=0, hp=A.HK_HOST_RANDOM, ap=A.HK_AGENT_RANDOM, st=stages, pad=-1.0))
    cases.append(dict(b=900, T=20, so=5, fp=torch_flags, fo=torch_flags_o, hp=A.HK_HOST_RANDOM,
                      ap=A.HK_AGENT_RANDOM_LEGAL, st=stages, pad=-1.0))
    for hp, ap, st in ((A.HK_HOST_ALL_COORD, A.HK_AGENT_CHOOSE_FIRST, stages),
                       (A.HK_HOST_RANDOM, A.HK_AGENT_CHOOSE_LAST, stages | A.HK_STAGE_RESCALE),
                       (A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM, A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON),
                       (A.HK_HOST_RANDOM, A.HK_AGENT_RANDOM_LEGAL, A.HK_STAGE_SHIFT)):
        cases.append(dict(b=600, T=11, so=2, fp=0, fo=0, hp=hp, ap=ap, st=st, pad=-1.0))
    cases.append(dict(b=600, T=9, so=0, fp=ops.make_flags("torch"), fo=CO.flags_of(sem="torch"), hp=A.HK_HOST_RANDOM,
                      ap=A.HK_AGENT_RANDOM, st=stages, pad=-2.5))
    cases.append(dict(b=600, T=9, so=0, fp=0, fo=0, hp=A.HK_HOST_RANDOM, ap=A.HK_AGENT_RANDOM, st=stages, pad=-2.5))
    cases.append(dict(b=600, T=9, so=1, fp=0, fo=0, hp=A.HK_HOST_RANDOM, ap=A.HK_AGENT_RANDOM, st=stages, pad=-1.0,
                      poison=True))
    for i, c in enumerate(cases):
        p0 = CO.generate_points(c["b"], m, d, 20, 11 + i, padding_value=c["pad"],
                                flags=c["fo"] & 3)
        if c.get("poison"):  # non-canonical games (a negative coordinate in a live row) in the second workgroup only
            p0[300:310, 0, 0] = -0.5
        want_p, want = CO.rollout(p0, c["T"], 77, game_offset=9, step_offset=c["so"], host_policy=c["hp"],
                                  agent_policy=c["ap"], stages=c["st"], flags=c["fo"], padding_value=c["pad"],
                                  record=False)
        P = dev(p0.copy())
        got = ops.rollout(P, c["T"], 77, game_offset=9, step_offset=c["so"], host_policy=c["hp"], agent_policy=c["ap"],
                          stages=c["st"], flags=c["fp"] | force, padding_value=c["pad"],
                          record=("game_length",))
        assert np.array_equal(host(P), want_p), c
        assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"]), c
        assert np.array_equal(host(got["game_length"]), want["game_length"]), c


def test_rollout_equals_stepwise_launches():
    """T fused steps == T single-step launches fed the recorded actions (the two bench paths)"""
    P = ops.generate_points(4096, 20, 3, 20, seed=42)
    Q = P.clone()
    rec = ops.rollout(P, 12, 7, record=("host_class", "axis", "done"))
    for t in range(12):
        res = ops.step(Q, rec["host_class"][t], rec["axis"][t], stages=7, out=Q, want=("done",))
        assert torch.equal(res["done"], rec["done"][t])
    assert torch.equal(P, Q)
    # out-of-place variant: the initial state is read from `initial` and left untouched
    fresh = ops.generate_points(4096, 20, 3, 20, seed=42)
    keep = fresh.clone()
    R = torch.empty_like(fresh)
    ops.rollout(R, 12, 7, initial=fresh)
    assert torch.equal(R, P) and torch.equal(fresh, keep)
    for fl in (0, A.HK_FLAG_FORCE_GENERIC):
        R.zero_()
        ops.rollout(R, 12, 7, initial=fresh, flags=fl)
        assert torch.equal(R, P)


def test_shard_invariance():
    full = ops.generate_points(1000, 20, 3, 20, seed=3)
    parts = [ops.generate_points(250, 20, 3, 20, seed=3, game_offset=250 * r) for r in range(4)]
    assert torch.equal(full, torch.cat(parts))
    ops.rollout(full, 10, 5)
    for r in range(4):
        ops.rollout(parts[r], 10, 5, game_offset=250 * r)
    assert torch.equal(full, torch.cat(parts))


def test_config4_shards_equal_the_whole_batch():
    """BASELINE configs[3] at full size on one device: 524 288 games as 8 rank shards of 65 536 (generation and
    a 20-step rollout each with its rank's game_offset) == the unsharded batch, state for state, and the
    shards' finished-game histograms add up to the whole batch's (what all_reduce_counts sums across ranks)"""
    world, b = 8, 65536
    full = ops.generate_points(world * b, 20, 3, 20, seed=42)
    rec_full = ops.rollout(full, 20, 7, record=("game_length",))
    total = torch.zeros_like(rec_full["done_count"])
    for r in range(world):
        part = ops.generate_points(b, 20, 3, 20, seed=42, game_offset=r * b)
        rec = ops.rollout(part, 20, 7, game_offset=r * b, record=("game_length",))
        assert torch.equal(part, full[r * b:(r + 1) * b]), r
        assert torch.equal(rec["game_length"], rec_full["game_length"][r * b:(r + 1) * b]), r
        total += rec["done_count"]
    assert torch.equal(total, rec_full["done_count"])


@pytest.mark.parametrize("spec", [(10, 3), (20, 3), (20, 4), (50, 4), (8, 4), (7, 3)])
def test_generated_rollouts_match_oracle(spec):
    """hk_rollout_desc.gen_max_value / episodes (ABI 4): the initial states drawn inside the launch, counts only or with
    the final state, one episode or several (seed + e, gen_seed + e; the counts accumulate, the last episode's state and
    lengths are kept) -- the fused kernel (hk::quadroll_kernel<..., GEN>) on the shapes that have one, the library's
    generate + rollout composition elsewhere and under forced families; against the oracle's generated rollouts and
    against generate_points + rollout on the device."""
    m, d = spec
    torch_flags = ops.make_flags("torch", noop_if_invalid=True, ignore_ended=True)
    torch_flags_o = CO.flags_of(sem="torch", noop_if_invalid=True, ignore_ended=True)
    stages = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON
    fused = spec in ((10, 3), (20, 3), (20, 4), (50, 4))
    cases = [dict(b=b, T=T, E=1, hp=A.HK_HOST_RANDOM, ap=A.HK_AGENT_RANDOM, fp=0, fo=0, st=stages, mv=20, rs=False)
             for b, T in ((1, 5), (16, 0), (17, 1), (250, 20), (301, 27))]
    cases += [dict(b=200, T=20, E=E, hp=A.HK_HOST_RANDOM, ap=A.HK_AGENT_RANDOM, fp=0, fo=0, st=stages, mv=20, rs=False)
              for E in (2, 5)]
    cases += [dict(b=150, T=12, E=2, hp=A.HK_HOST_RANDOM, ap=A.HK_AGENT_RANDOM_LEGAL, fp=torch_flags, fo=torch_flags_o,
                   st=stages, mv=20, rs=False),
              dict(b=150, T=12, E=1, hp=A.HK_HOST_ALL_COORD, ap=A.HK_AGENT_CHOOSE_LAST, fp=0, fo=0,
                   st=stages | A.HK_STAGE_RESCALE, mv=9, rs=True),
              dict(b=150, T=9, E=3, hp=A.HK_HOST_ZEILLINGER, ap=A.HK_AGENT_RANDOM_LEGAL, fp=0, fo=0, st=stages, mv=20,
                   rs=False),
              dict(b=150, T=9, E=1, hp=A.HK_HOST_RANDOM, ap=A.HK_AGENT_RANDOM, fp=0, fo=0, st=stages, mv=300, rs=False)]
    for c in cases:
        gst = A.HK_STAGE_NEWTON | A.HK_STAGE_REPOSITION | (A.HK_STAGE_RESCALE if c["rs"] else 0)
        want_p, want = CO.rollout_generated(c["b"], spec, c["T"], 31, max_value=c["mv"], gen_seed=77, gen_stages=gst,
                                            episodes=c["E"], game_offset=9, step_offset=2, host_policy=c["hp"],
                                            agent_policy=c["ap"], stages=c["st"], flags=c["fo"])
        for fam in (0, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_ONE_LANE, A.HK_FLAG_FORCE_GENERIC):
            out = torch.empty((c["b"], m, d), device="cuda")
            got = ops.rollout_generated(c["b"], spec, c["T"], 31, max_value=c["mv"], gen_seed=77, rescale=c["rs"],
                                        episodes=c["E"], game_offset=9, step_offset=2, host_policy=c["hp"],
                                        agent_policy=c["ap"], stages=c["st"], flags=c["fp"] | fam, out=out,
                                        record=("game_length",))
            assert np.array_equal(host(out), want_p), (c, fam)
            assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"]), (c, fam)
            assert np.array_equal(host(got["game_length"]), want["game_length"]), (c, fam)
        # counts only: no state buffer at all (the fused kernel; elsewhere the library says so)
        zeil_small = c["hp"] == A.HK_HOST_ZEILLINGER and m <= 32
        if fused and not zeil_small:
            got = ops.rollout_generated(c["b"], spec, c["T"], 31, max_value=c["mv"], gen_seed=77, rescale=c["rs"],
                                        episodes=c["E"], game_offset=9, step_offset=2, host_policy=c["hp"],
                                        agent_policy=c["ap"], stages=c["st"], flags=c["fp"])
            assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"]), c
        else:
            from hironaka_amd._lib import HironakaHipError
            with pytest.raises(HironakaHipError):
                ops.rollout_generated(c["b"], spec, c["T"], 31, max_value=c["mv"], gen_seed=77, rescale=c["rs"],
                                      episodes=c["E"], host_policy=c["hp"], agent_policy=c["ap"], stages=c["st"],
                                      flags=c["fp"])
    # one episode == generate_points + rollout on the device; with game ids (fused kernel only)
    P = ops.generate_points(300, m, d, 20, seed=5, game_offset=3)
    rec = ops.rollout(P, 15, 8, game_offset=3, record=("game_length",))
    out = torch.empty_like(P)
    got = ops.rollout_generated(300, spec, 15, 8, max_value=20, gen_seed=5, game_offset=3, out=out, record=("game_length",))
    assert torch.equal(out, P) and torch.equal(got["done_count"], rec["done_count"])
    assert torch.equal(got["game_length"], rec["game_length"])
    if fused:
        ids = np.random.default_rng(1).permutation(300).astype(np.int32)
        want_p, want = CO.rollout_generated(300, spec, 15, 8, max_value=20, gen_seed=5, game_offset=3, game_ids=ids)
        got = ops.rollout_generated(300, spec, 15, 8, max_value=20, gen_seed=5, game_offset=3, out=out,
                                    record=("game_length",), game_ids=dev(ids))
        assert np.array_equal(host(out), want_p)
        assert np.array_equal(host(got["game_length"]), want["game_length"])
        assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"])


def test_episodes_from_resident_states_match_oracle():
    """hk_rollout_desc.episodes with the initial states in memory (`initial`): every episode restarts from them with
    seed + e; the counts accumulate, `points` keeps the last episode's final state"""
    p0 = CO.generate_points(500, 20, 3, 20, 4)
    total = np.zeros(21, dtype=np.uint64)
    for e in range(3):
        want_p, want = CO.rollout(p0, 20, 60 + e, record=False)
        total += want["done_count"]
    for fam in (0, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_ONE_LANE, A.HK_FLAG_FORCE_TWO_LANES):
        P0, P = dev(p0.copy()), torch.empty((500, 20, 3), device="cuda")
        r = A.hk_rollout_desc()
        dc = torch.zeros(21, dtype=torch.int64, device="cuda")
        gl = torch.empty(500, dtype=torch.int32, device="cuda")
        r.points, r.points_in, r.done_count, r.game_length_out = P.data_ptr(), P0.data_ptr(), dc.data_ptr(), gl.data_ptr()
        r.seed, r.padding_value, r.reward_sign, r.episodes = 60, -1.0, 1.0, 3
        r.batch, r.max_points, r.dim, r.dtype, r.steps = 500, 20, 3, A.HK_F32, 20
        r.stages, r.flags = 7, fam
        import ctypes as C
        from hironaka_amd._lib import check, lib
        ws = ops.rollout_workspace(500, 20, (20, 3))
        r.workspace, r.workspace_bytes = ws.data_ptr(), ws.numel()
        check(lib().hk_rollout(C.byref(r), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "hk_rollout")
        assert np.array_equal(host(P), want_p), fam
        assert np.array_equal(host(dc).astype(np.uint64), total), fam
        assert np.array_equal(host(gl), want["game_length"]), fam
    # through ops.rollout, with a game off the exact path in one wave (its episodes restart on the generic routines too)
    p1 = p0.copy()
    p1[37, 1, 0] = -1.0  # a partly padded row
    tot = np.zeros(21, dtype=np.uint64)
    for e in range(4):
        want_p, want = CO.rollout(p1, 20, 9 + e, record=False)
        tot += want["done_count"]
    for fam in (0, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_GENERIC):
        P = torch.empty((500, 20, 3), device="cuda")
        got = ops.rollout(P, 20, 9, initial=dev(p1.copy()), episodes=4, flags=fam, record=("game_length",))
        assert np.array_equal(host(P), want_p), fam
        assert np.array_equal(host(got["done_count"]).astype(np.uint64), tot), fam
        assert np.array_equal(host(got["game_length"]), want["game_length"]), fam


# ------------------------------------------------------------------------------------------
# BASELINE sizes: oracle on a slice + size-independent properties on the whole batch
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b,m,d", [(65536, 20, 3), (262144, 50, 4)])
def test_baseline_sizes(b, m, d):
    n_cls = 2 ** d - d - 1
    P = ops.generate_points(b, m, d, 20, seed=42)
    # generator output is a fixed point of newton and reposition (idempotence)
    assert torch.equal(ops.get_newton_polytope(P), P)
    assert torch.equal(ops.reposition(P), P)
    npts = ops.get_num_points(P)
    assert int(npts.min()) >= 1 and int(npts.max()) <= m
    g = torch.Generator(device="cuda").manual_seed(0)
    cls = torch.randint(0, n_cls, (b,), device="cuda", generator=g, dtype=torch.int32)
    ax = torch.randint(0, d, (b,), device="cuda", generator=g, dtype=torch.int32)
    res = ops.step(P, cls, ax, stages=7, want=("done", "prev_done", "reward", "num_points"))
    Q = res["points"]
    # oracle on the first / last 2048 games
    for sl in (slice(0, 2048), slice(b - 2048, b)):
        want = CO.step(host(P[sl]), host(cls[sl]), host(ax[sl]), stages=7)
        assert np.array_equal(host(Q[sl]), want["points"])
        assert np.array_equal(host(res["reward"][sl]), want["reward"])
    # properties over the whole batch
    assert torch.equal(ops.get_newton_polytope(Q), Q)           # result is reduced
    assert torch.equal(res["num_points"], ops.get_num_points(Q))
    assert torch.equal(res["done"], ops.get_dones(Q))
    assert bool((res["num_points"] >= 1).all())                   # a game never loses its last point
    assert bool((res["reward"] == (res["done"] & ~res["prev_done"]).float()).all())
    # the specialised (two lanes per game / one lane per game) and the generic kernels agree on every game
    assert torch.equal(Q, ops.step(P, cls, ax, stages=7, flags=A.HK_FLAG_FORCE_GENERIC)["points"])
    assert torch.equal(Q, ops.step(P, cls, ax, stages=7, flags=A.HK_FLAG_FORCE_ONE_LANE)["points"])
    R1, R2 = P.clone(), P.clone()
    r1 = ops.rollout(R1, 20, 3, record=("game_length",))
    r2 = ops.rollout(R2, 20, 3, flags=A.HK_FLAG_FORCE_ONE_LANE, record=("game_length",))
    assert torch.equal(R1, R2) and torch.equal(r1["done_count"], r2["done_count"])
    assert torch.equal(r1["game_length"], r2["game_length"])
    # the fused rollout at size against the ORACLE: the Philox stream is keyed by the global game index, so the oracle
    # rolls out a slice with its offset -- final states, game lengths and the slice's share of the finished-game counts,
    # for the default route (the headline instantiation at (20,3) x 65 536) and the forced families
    for sl in (slice(0, 2048), slice(b - 2048, b)):
        want_p, want = CO.rollout(host(P[sl]), 20, 3, game_offset=sl.start, record=False)
        for R, r in ((R1, r1), (R2, r2)):
            assert np.array_equal(host(R[sl]), want_p)
            gl = host(r["game_length"][sl])
            assert np.array_equal(gl, want["game_length"])
            share = np.array([((gl >= 0) & (gl <= t)).sum() for t in range(21)], dtype=np.uint64)
            assert np.array_equal(share, want["done_count"])
    for fam in ((A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_FOUR_LANES) if m <= 32 else (A.HK_FLAG_FORCE_TEAM,)):
        R3 = P.clone()
        r3 = ops.rollout(R3, 20, 3, flags=fam, record=("game_length",))
        assert torch.equal(R1, R3) and torch.equal(r1["done_count"], r3["done_count"]), fam
        assert torch.equal(r1["game_length"], r3["game_length"]), fam
    # ... and from initial states drawn inside the launch (hk_rollout_desc.gen_max_value): counts only, then with the state
    gen = ops.rollout_generated(b, (m, d), 20, 3, max_value=20, gen_seed=42)
    assert torch.equal(gen["done_count"], r1["done_count"])
    G1 = torch.empty_like(P)
    gen = ops.rollout_generated(b, (m, d), 20, 3, max_value=20, gen_seed=42, out=G1, record=("game_length",))
    assert torch.equal(G1, R1) and torch.equal(gen["game_length"], r1["game_length"])
    # ... and binned on the device: the same games, game by game, at their new positions
    Bn, ids = ops.generate_points_binned(b, m, d, 20, 42)
    assert torch.equal(Bn, P[ids.long()])
    rb = ops.rollout(Bn, 20, 3, game_ids=ids, record=("game_length",))
    assert torch.equal(Bn, R1[ids.long()]) and torch.equal(rb["game_length"], r1["game_length"][ids.long()])
    assert torch.equal(rb["done_count"], r1["done_count"])
    # fused rollout: monotone done counts, every game that ends stays ended
    rec = ops.rollout(P, 20, 1, record=("game_length",))
    dc = host(rec["done_count"])
    assert (np.diff(dc) >= 0).all() and dc[-1] == int(ops.get_dones(P).sum())
    gl = host(rec["game_length"])
    assert ((gl >= 0).sum() == dc[-1])


@pytest.mark.parametrize("b,m,d", [(65536, 20, 3), (262144, 50, 4)])
def test_baseline_sizes_other_operators(b, m, d):
    """The state-reading operators and the other rollout configurations at BASELINE.json's sizes: oracle slices (first
    and last 1 024 games, the policy streams keyed by the global index) and size-independent properties over the whole
    batch -- the sorted features are sorted and idempotent, Zeillinger's class is a legal subset, a list-semantics
    rollout leaves a compacted, descending state with the same games finished as the JAX-semantics one."""
    P = ops.generate_points(b, m, d, 20, seed=7)
    D = ops.generate_points(b, m, d, 20, seed=8, newton=False, reposition=False)
    n_cls = 2 ** d - d - 1
    slices = (slice(0, 1024), slice(b - 1024, b))
    for pts in (P, D):
        f = ops.get_features(pts)
        ft = ops.get_features_torch(pts)
        z = ops.zeillinger(pts)
        for sl in slices:
            hp = host(pts[sl])
            assert np.array_equal(host(f[sl]), CO.get_features(hp))
            assert np.array_equal(host(ft[sl]), CO.get_features_torch(hp))
            assert np.array_equal(host(z[sl]), CO.zeillinger(hp))
        assert int(z.min()) >= 0 and int(z.max()) < n_cls
        f3 = f.reshape(b, m, d)
        assert torch.equal(ops.get_features(f3), f)                       # sorted + rescaled once is a fixed point
        key = f3[:, :, d - 1]
        assert bool((key[:, :-1] >= key[:, 1:]).all())                    # last coordinate (primary key) descending
        assert bool((ft[:, :-1, 0] >= ft[:, 1:, 0]).all())                # coordinate 0 descending, padding last
        assert torch.equal(ops.get_num_points(ft), ops.get_num_points(pts))
    g = torch.Generator(device="cuda").manual_seed(1)
    cls = torch.randint(0, n_cls, (b,), device="cuda", generator=g, dtype=torch.int32)
    ax = torch.randint(0, d, (b,), device="cuda", generator=g, dtype=torch.int32)
    dense_next = ops.step(D, cls, ax, stages=7)["points"]                 # (50,4): the packed-row test
    for sl in slices:
        assert np.array_equal(host(dense_next[sl]), CO.step(host(D[sl]), host(cls[sl]), host(ax[sl]), stages=7)["points"])
    assert torch.equal(ops.get_newton_polytope(dense_next), dense_next)
    fl_o, fl_p = CO.flags_of(sem="list", noop_if_invalid=True), ops.make_flags("list", noop_if_invalid=True)
    L = P.clone()
    rl = ops.rollout(L, 20, 5, flags=fl_p, agent_policy=A.HK_AGENT_RANDOM_LEGAL, record=("game_length",))
    Zs = P.clone()
    rz = ops.rollout(Zs, 20, 5, host_policy=A.HK_HOST_ZEILLINGER, record=("game_length",))
    for sl in slices:
        want_p, want = CO.rollout(host(P[sl]), 20, 5, game_offset=sl.start, flags=fl_o, agent_policy=A.HK_AGENT_RANDOM_LEGAL,
                                  record=False)
        assert np.array_equal(host(L[sl]), want_p) and np.array_equal(host(rl["game_length"][sl]), want["game_length"])
        want_p, want = CO.rollout(host(P[sl]), 20, 5, game_offset=sl.start, host_policy=A.HK_HOST_ZEILLINGER, record=False)
        assert np.array_equal(host(Zs[sl]), want_p) and np.array_equal(host(rz["game_length"][sl]), want["game_length"])
    live = L[:, :, 0] >= 0
    assert bool((live[:, :-1] | ~live[:, 1:]).all())                     # compacted: no live row behind a padding row
    both = live[:, :-1] & live[:, 1:]
    assert bool((L[:, :-1, 0][both] >= L[:, 1:, 0][both]).all())           # coordinate 0 descending among the live rows
    assert int(rl["done_count"][-1]) == int(ops.get_dones(L).sum())


# ------------------------------------------------------------------------------------------
# error behaviour at the boundary
# ------------------------------------------------------------------------------------------

def test_error_behaviour():
    from hironaka_amd._lib import HironakaHipError
    P = torch.zeros(4, 5, 3, device="cuda")
    with pytest.raises(ValueError):
        ops.shift(P, torch.zeros(4, 2, device="cuda"), torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError):
        ops.get_newton_polytope(P, sem="numpy")
    with pytest.raises(TypeError):
        ops.get_newton_polytope(P.int())
    with pytest.raises(HironakaHipError) as ei:
        ops.step(P.reshape(4, 15), None, None, stages=A.HK_STAGE_NEWTON, spec=(5, 4))
    assert ei.value.status == A.HK_ERR_SHAPE
    assert ops.get_newton_polytope(torch.zeros(0, 5, 3, device="cuda")).shape == (0, 5, 3)  # empty batch
    h = torch.zeros(4, 5, 3, device="cuda", dtype=torch.float16)
    assert ops.get_newton_polytope(h).dtype == torch.float16


# ------------------------------------------------------------------------------------------
# ragged batches, degenerate shapes, high dimensions
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", [1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 1000])
def test_ragged_batch_sizes(b):
    """batches that do not fill the last wave (or even one wave), every kernel family, step + rollout +
    generate; also checks nothing is written past the batch (guard rows after the tensors)."""
    for (m, d), flag_sets in (((20, 3), (0, A.HK_FLAG_FORCE_ONE_LANE, A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_FOUR_LANES,
                                        A.HK_FLAG_FORCE_TEAM, A.HK_FLAG_FORCE_GENERIC)),
                              ((10, 3), (0, A.HK_FLAG_FORCE_FOUR_LANES)),
                              ((50, 4), (0, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_GENERIC)),
                              ((7, 5), (0, A.HK_FLAG_FORCE_GENERIC))):
        p0 = CO.generate_points(b, m, d, 20, 3, game_offset=9)
        rng = np.random.default_rng(b)
        cls = rng.integers(0, 2 ** d - d - 1, b).astype(np.int32)
        ax = rng.integers(0, d, b).astype(np.int32)
        want = CO.step(p0, cls, ax, stages=7)
        want_roll, want_rec = CO.rollout(p0, 5, 11, game_offset=9)
        for fl in flag_sets:
            guard = torch.full((b + 2, m, d), 123.0, device="cuda")
            guard[:b] = dev(p0)
            out = torch.full((b + 2, m, d), 456.0, device="cuda")
            res = ops.step(guard[:b], dev(cls), dev(ax), stages=7, flags=fl, out=out[:b], want=("done", "reward"))
            assert np.array_equal(host(out[:b]), want["points"]), (m, d, fl)
            assert bool((out[b:] == 456.0).all()) and bool((guard[b:] == 123.0).all())
            assert np.array_equal(host(res["done"]), want["done"])
            roll = guard.clone()
            rec = ops.rollout(roll[:b], 5, 11, game_offset=9, flags=fl, record=("axis", "game_length"))
            assert np.array_equal(host(roll[:b]), want_roll) and bool((roll[b:] == 123.0).all()), (m, d, fl)
            assert np.array_equal(host(rec["axis"]), want_rec["axis"])
            assert np.array_equal(host(rec["game_length"]), want_rec["game_length"])
            assert np.array_equal(host(rec["done_count"]).astype(np.uint64), want_rec["done_count"])
            plain = guard.clone()  # without per-step records: the plain rollout kernels (two lanes / one lane)
            prec = ops.rollout(plain[:b], 5, 11, game_offset=9, flags=fl, record=("game_length",))
            assert np.array_equal(host(plain[:b]), want_roll) and bool((plain[b:] == 123.0).all()), (m, d, fl)
            assert np.array_equal(host(prec["game_length"]), want_rec["game_length"])
            assert np.array_equal(host(prec["done_count"]).astype(np.uint64), want_rec["done_count"])
            gen = torch.full((b + 1, m, d), 7.0, device="cuda")
            ops.generate_points(b, m, d, 20, seed=3, game_offset=9, flags=fl, out=gen[:b])
            assert np.array_equal(host(gen[:b]), p0) and bool((gen[b:] == 7.0).all())


@pytest.mark.parametrize("spec", [(1, 3), (1, 2), (2, 10), (5, 10), (3, 8), (64, 2), (40, 6)])
def test_degenerate_and_high_dim_shapes(spec):
    """one-row games (always finished), dim up to the codec's limit of 10, 64 rows"""
    m, d = spec
    rng = np.random.default_rng(m * 100 + d)
    b = 130
    for dtype in (np.float32, np.float64):
        p = rand_state(rng, b, m, d, dtype, -1.0, maxv=4, holes=0.2)
        cls = rng.integers(0, 2 ** d - d - 1, b).astype(np.int32)
        ax = rng.integers(0, d, b).astype(np.int32)
        for sem in ("jax", "torch", "list"):
            want = CO.step(p, cls, ax, stages=15, flags=CO.flags_of(sem=sem, noop_if_invalid=(sem != "jax")))
            got = ops.step(dev(p), dev(cls), dev(ax), stages=15, flags=ops.make_flags(sem, noop_if_invalid=(sem != "jax")),
                           want=("done", "num_points"))
            assert np.array_equal(host(got["points"]), want["points"]), (spec, dtype, sem)
            assert np.array_equal(host(got["done"]), want["done"])
            assert np.array_equal(host(got["num_points"]), want["num_points"])
    q = CO.generate_points(b, m, d, 9, 1)
    assert np.array_equal(host(ops.generate_points(b, m, d, 9, seed=1)), q)
    wp, wr = CO.rollout(q, 4, 2, agent_policy=A.HK_AGENT_RANDOM_LEGAL)
    Q = dev(q)
    gr = ops.rollout(Q, 4, 2, agent_policy=A.HK_AGENT_RANDOM_LEGAL, record=("host_class", "axis"))
    assert np.array_equal(host(Q), wp) and np.array_equal(host(gr["host_class"]), wr["host_class"])
    assert np.array_equal(host(gr["axis"]), wr["axis"])


def test_non_finite_and_negative_zero_inputs_match_oracle():
    """inf / NaN / -0.0 entries are outside the shortcut's exactness guard: the wave takes the generic routines, which
    follow the C restatement operation for operation (the NaN-aware minimum of `reposition`, the domination test as the
    reference's subtraction: inf - inf dominates nothing) -- so EVERY game, the non-finite ones included, equals the
    oracle, on every kernel family, under JAX and torch semantics, for single steps with every stage subset and for
    rollouts.  (Round 3 found the HIP paths and the oracle apart on such a game -- tests/golden/nonfinite_regression.json
    -- and narrowed this test to the finite games; list semantics -- ragged Python lists -- stay finite-only.)"""
    import json
    import os
    rng = np.random.default_rng(4)
    for (m, d) in ((20, 3), (6, 3), (50, 4), (7, 5)):
        b = 300
        p = rand_state(rng, b, m, d, np.float32, -1.0)
        rows = rng.integers(0, min(m, 4), 40)
        games = rng.choice(b, 40, replace=False)
        for n, (g, r) in enumerate(zip(games, rows)):
            k = rng.integers(0, d)
            if p[g, r, 0] < 0:
                continue
            p[g, r, k] = (np.inf, np.nan, -0.0, np.inf)[n % 4]
            if n % 8 == 7:
                p[g, (r + 1) % m] = p[g, r]  # a duplicate of a non-finite row
        cls = rng.integers(0, 2 ** d - d - 1, b).astype(np.int32)
        ax = rng.integers(0, d, b).astype(np.int32)
        fams = (0, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_ONE_LANE, A.HK_FLAG_FORCE_TEAM,
                A.HK_FLAG_FORCE_GENERIC)
        for sem in ("jax", "torch"):
            fo = CO.flags_of(sem=sem, noop_if_invalid=(sem == "torch"))
            fp = ops.make_flags(sem, noop_if_invalid=(sem == "torch"))
            for st in (1, 2, 4, 8, 3, 7, 15):
                want = CO.step(p, cls, ax, stages=st, flags=fo)
                for fam in fams:
                    got = ops.step(dev(p), dev(cls), dev(ax), stages=st, flags=fp | fam, want=("done", "reward"))
                    assert np.array_equal(host(got["points"]), want["points"], equal_nan=True), (m, d, sem, st, fam)
                    assert np.array_equal(host(got["done"]), want["done"]), (m, d, sem, st, fam)
            want_p, want = CO.rollout(p, 6, 3, flags=fo, record=False)
            for fam in fams:
                P = dev(p.copy())
                got = ops.rollout(P, 6, 3, flags=fp | fam, record=("game_length",))
                assert np.array_equal(host(P), want_p, equal_nan=True), (m, d, sem, fam)
                assert np.array_equal(host(got["game_length"]), want["game_length"]), (m, d, sem, fam)
                assert np.array_equal(host(got["done_count"]).astype(np.uint64), want["done_count"]), (m, d, sem, fam)
    # the game round 3 tripped over (gpurun_out/r3_dbg1.log, game 259), as a committed fixture
    with open(os.path.join(os.path.dirname(__file__), "golden", "nonfinite_regression.json")) as f:
        fx = json.load(f)
    conv = lambda rows: np.array([[float(v) for v in r] for r in rows], dtype=np.float32)[None]
    pin, pexp = conv(fx["points_in"]), conv(fx["points_out"])
    c1, a1 = np.array([fx["host_class"]], dtype=np.int32), np.array([fx["axis"]], dtype=np.int32)
    assert np.array_equal(CO.step(pin, c1, a1, stages=7)["points"], pexp, equal_nan=True)
    for fam in (0, A.HK_FLAG_FORCE_FOUR_LANES, A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_TEAM, A.HK_FLAG_FORCE_GENERIC):
        got = ops.step(dev(pin), dev(c1), dev(a1), stages=7, flags=fam)["points"]
        assert np.array_equal(host(got), pexp, equal_nan=True), fam


@pytest.mark.parametrize("spec", [(20, 3), (50, 4), (9, 7)])
def test_deferred_counts_equal_per_launch_counts(spec):
    """HK_FLAG_DEFER_COUNTS: the per-workgroup partial counts of several launches accumulate in the caller's
    workspace and one hk_rollout_reduce_counts equals the sum of the per-launch done_counts; the workspace is
    zero afterwards (fast, team and generic kernels)."""
    m, d = spec
    b, T = 3000, 9
    P = ops.generate_points(b, m, d, 20, seed=11)
    want = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    finals = []
    for k in range(4):
        Q = P.clone()
        want += ops.rollout(Q, T, 100 + k)["done_count"]
        finals.append(Q)
    ws = ops.rollout_workspace(b, T, spec)
    assert int(ws.sum()) == 0
    for k in range(4):
        Q = P.clone()
        res = ops.rollout(Q, T, 100 + k, defer_counts=True, workspace=ws)
        assert "done_count" not in res and torch.equal(Q, finals[k])
    got = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    ops.reduce_counts(ws, got, b, T, spec)
    assert torch.equal(got, want)
    assert int(ws.sum()) == 0
    ops.reduce_counts(ws, got, b, T, spec)  # nothing pending: a no-op
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        ops.rollout(P.clone(), T, 1, defer_counts=True)
    # launches served by different kernel variants (two lanes / one lane per game, team, Zeillinger's host, and
    # a recording rollout) meet in ONE workspace: its rows have the same length for all of them
    variants = [dict(), dict(flags=A.HK_FLAG_FORCE_ONE_LANE), dict(flags=A.HK_FLAG_FORCE_TEAM),
                dict(host_policy=A.HK_HOST_ZEILLINGER), dict(record=("axis",))]
    if d > 6:
        variants = [dict(), dict(host_policy=A.HK_HOST_ZEILLINGER), dict(record=("axis",))]
    want = torch.zeros(T + 1, dtype=torch.int64, device="cuda")
    for kw in variants:
        want += ops.rollout(P.clone(), T, 7, **kw)["done_count"]
    for kw in variants:
        ops.rollout(P.clone(), T, 7, defer_counts=True, workspace=ws, **kw)
    got.zero_()
    ops.reduce_counts(ws, got, b, T, spec)
    assert torch.equal(got, want) and int(ws.sum()) == 0


@pytest.mark.parametrize("spec", [(20, 3), (20, 4), (10, 3), (8, 4), (4, 3), (50, 4), (33, 4), (64, 3), (12, 6), (7, 3), (9, 7)])
def test_features_match_oracle(spec):
    """hk_get_features (jax/util.py:186-197: rescale + rows in descending order, last coordinate primary) on the
    register-resident, team and generic kernels: game states, duplicate rows, ties on the primary coordinate,
    all-padding games, irregular input (exact path) and record strides (agent observations)"""
    m, d = spec
    rng = np.random.default_rng(1000 * m + d)
    b = 300
    p = rand_state(rng, b, m, d, np.float32, -1.0, maxv=4, holes=0.5)   # small values: many ties and duplicates
    p[0] = -1.0                                                          # an empty game
    p[1, :, :] = 2.0                                                     # all rows equal
    q = host(ops.step(dev(p), dev(rng.integers(0, 2 ** d - d - 1, b).astype(np.int32)),
                      dev(rng.integers(0, d, b).astype(np.int32)), stages=7)["points"])
    for states in (p, q):
        for scale in (True, False):
            want = CO.get_features(states, scale)
            assert np.array_equal(host(ops.get_features(dev(states), scale)), want), (spec, scale)
    r = p.copy()
    if m >= 3:
        r[5, 1] = -3.0          # irregular padding row: the wave takes the exact generic routines
        r[6, 0, 0] = -0.5
    assert np.array_equal(host(ops.get_features(dev(r), True)), CO.get_features(r, True))
    # agent observation records: the subset mask trails the points and is not part of the features
    rec = np.concatenate([q.reshape(b, m * d), rng.integers(0, 2, (b, d)).astype(np.float32)], axis=1)
    got = host(ops.get_features(dev(rec), True, spec=spec))
    assert np.array_equal(got, CO.get_features(q, True))
    # big batch, ragged tail
    big = host(ops.generate_points(5003, m, d, 20, seed=3))
    assert np.array_equal(host(ops.get_features(dev(big), True)), CO.get_features(big, True))
    # fractional coordinates (dyadic fractions: exact sums, many equal keys after the rescale) -- the class of input
    # behind the round-2 development mismatch at (20,4), b = 63 (tests/golden/fuzz_regression_features_20_4.npz)
    for bb in (63, 300):
        f = (rng.integers(0, 33, (bb, m, d)) / 8.0).astype(np.float32)
        f[rng.random((bb, m)) < 0.4] = -1.0
        for scale in (True, False):
            assert np.array_equal(host(ops.get_features(dev(f), scale)), CO.get_features(f, scale)), (spec, bb, scale)


def test_features_fuzz_regression_20_4():
    """the configuration of the round-2 development mismatch (fuzz_parity: m=20, d=4, b=63, dyadic fractions,
    scale=True) as a committed fixture: inputs + the oracle's features"""
    import os
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "fuzz_regression_features_20_4.npz"))
    for scale, key in ((True, "features_scaled"), (False, "features_unscaled")):
        assert np.array_equal(CO.get_features(fx["points"], scale), fx[key])  # (the fixture pins the oracle too)
        assert np.array_equal(host(ops.get_features(dev(fx["points"]), scale)), fx[key])


@pytest.mark.parametrize("spec", [(20, 3), (10, 3), (8, 4), (20, 4), (4, 3), (7, 3), (50, 4), (64, 6), (9, 7)])
def test_zeillinger_operator_matches_oracle(spec):
    """hk_zeillinger (jax/players.py:55-109): on shapes with a register-resident specialisation the class comes
    from the rows in registers, elsewhere from the generic kernel; both against the C oracle -- game states,
    tiny values (ties in (L, S)), empty / one-point games, irregular padding (exact path)"""
    m, d = spec
    rng = np.random.default_rng(77 * m + d)
    b = 500
    p = rand_state(rng, b, m, d, np.float32, -1.0, maxv=3, holes=0.6)
    p[0] = -1.0
    p[1, 1:] = -1.0
    g = host(ops.generate_points(b, m, d, 20, seed=9))
    frac = np.where(g >= 0, g / np.float32(7.0), g).astype(np.float32)
    for sem in ("jax", "list"):
        for states in (p, g, frac):
            want = CO.zeillinger(states, sem)
            assert np.array_equal(host(ops.zeillinger(dev(states), sem)), want), sem
            assert np.array_equal(host(ops.zeillinger(dev(states), sem, force_generic=True)), want), sem
            if d <= 6 and m <= 64:
                assert np.array_equal(host(ops.zeillinger(dev(states), sem, force_team=True)), want), sem
    r = p.copy()
    if m >= 3:
        r[7, 1] = -3.0
        r[8, 0, 0] = -0.5
    for sem in ("jax", "list"):
        assert np.array_equal(host(ops.zeillinger(dev(r), sem)), CO.zeillinger(r, sem)), sem
    # records with a stride (agent observations) and a ragged batch
    rec = np.concatenate([g.reshape(b, m * d), np.ones((b, d), np.float32)], axis=1)[:333]
    assert np.array_equal(host(ops.zeillinger(dev(rec), spec=spec)), CO.zeillinger(g[:333], "jax"))


@pytest.mark.parametrize("spec", [(20, 3), (5, 3), (8, 4), (20, 4), (7, 3), (33, 6), (50, 4), (9, 7)])
def test_features_torch_matches_oracle(spec, live_fused):
    """hk_get_features_torch (core/tensor_points.py:72-74) on the register-resident, team and generic kernels
    against the C oracle -- ties in coordinate 0 (stable), empty games, irregular rows (exact path), f64 --
    and against the reference's own outputs where a fixture has this shape"""
    m, d = spec
    rng = np.random.default_rng(5 * m + d)
    b = 777
    p = rand_state(rng, b, m, d, np.float32, -1.0, maxv=4, holes=0.4)
    p[0] = -1.0
    frac = np.where(p >= 0, p / np.float32(3.0), p).astype(np.float32)
    r = p.copy()
    if m >= 3:
        r[7, 1] = -3.0
        r[8, 0, 0] = -0.5
    for states in (p, frac, r, p.astype(np.float64)):
        want = CO.get_features_torch(states)
        got = host(ops.get_features_torch(torch.as_tensor(states).cuda()))
        assert np.array_equal(got, want) and got.dtype == want.dtype
    tag = f"features_m{m}_d{d}"
    if f"{tag}/points" in live_fused.files:
        got = host(ops.get_features_torch(torch.as_tensor(live_fused[f"{tag}/points"]).cuda()))
        assert np.array_equal(got, live_fused[f"{tag}/features"])


def test_step_with_agent_logits_equals_masked_argmax_then_step():
    """HK_AXIS_MASKED_LOGITS (the agent's move decoded inside hk_step from its logits and the host's class id) against
    hk_search_masked_argmax followed by a plain step, on the shapes with a four-lane kernel; elsewhere the status is
    HK_ERR_UNSUPPORTED"""
    from hironaka_amd._lib import HironakaHipError, check, lib
    rng = np.random.default_rng(5)
    for (m, d) in ((20, 3), (10, 3), (20, 4)):
        for b in (1, 33, 1000):
            for stages in (A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON,
                           A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON | A.HK_STAGE_RESCALE):
                P = ops.generate_points(b, m, d, 20, seed=3)
                cls = torch.tensor(rng.integers(0, 2 ** d - d - 1, b), dtype=torch.int32, device="cuda")
                lg = rng.standard_normal((b, d)).astype(np.float32)
                lg[rng.random((b, d)) < 0.1] = np.nan
                lg[rng.random((b, d)) < 0.15] = 0.25
                logits = torch.tensor(lg, device="cuda")
                axis = torch.empty(b, dtype=torch.int32, device="cuda")
                check(lib().hk_search_masked_argmax(logits.data_ptr(), cls.data_ptr(), axis.data_ptr(), b, d, None), "argmax")
                want = ("done", "prev_done", "reward", "num_points")
                ref = ops.step(P, cls, axis, stages=stages, want=want)
                got = ops.step(P, cls, logits, stages=stages, want=want)
                for k in ref:
                    assert torch.equal(ref[k], got[k]), (m, d, b, stages, k)
    P = ops.generate_points(8, 16, 3, 20, seed=3)  # no four-lane kernel for (16,3)
    with pytest.raises(HironakaHipError) as err:
        ops.step(P, torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros((8, 3), device="cuda"),
                 stages=A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON)
    assert err.value.status == A.HK_ERR_UNSUPPORTED


@pytest.mark.parametrize("spec", [(20, 3), (10, 3), (20, 4)])
def test_step_features_and_agent_logits_match_oracle(spec):
    """hk_step_features and HK_AXIS_MASKED_LOGITS DIRECTLY against the oracle (hko_step_features = hko_step +
    hko_get_features; the masked argmax of jax/util.py:287-327 inside hko_step): generated and dense states, NaN / tied
    logits, with and without rescaling, JAX and torch semantics -- and non-canonical (finite) games (a negative
    coordinate in a live row, a partly padded row, an irregular padding row) in some waves only: those waves take the
    exact generic path, which must produce the features too"""
    m, d = spec
    rng = np.random.default_rng(31 * m + d)
    for b in (1, 17, 1000, 4099):
        for stages, sem in ((7, "jax"), (5, "jax"), (7, "torch"), (15, "jax")):
            for kind in ("generated", "dense", "poisoned"):
                p = host(ops.generate_points(b, m, d, 20, seed=b + m, newton=kind != "dense", reposition=kind != "dense"))
                if kind == "poisoned":
                    for g in range(0, b, 37):       # one game in (roughly) every other wave of 16
                        if g % 3 == 0:
                            p[g, 0, 0] = -0.5       # a negative coordinate in a live row
                        elif g % 3 == 1:
                            p[g, 0] = 2.0
                            p[g, 0, d - 1] = -1.0   # a partly padded row
                        else:
                            p[g, m - 1] = -3.0      # an irregular padding row
                cls = rng.integers(0, 2 ** d - d - 1, b).astype(np.int32)
                ax = rng.integers(0, d, b).astype(np.int32)
                lg = rng.standard_normal((b, d)).astype(np.float32)
                lg[rng.random((b, d)) < 0.1] = np.nan
                lg[rng.random((b, d)) < 0.15] = 0.25
                fo = CO.flags_of(sem=sem, noop_if_invalid=sem != "jax", ignore_ended=sem == "torch")
                fp = ops.make_flags(sem, sem != "jax", sem == "torch")
                for axis, is_logits in ((ax, False), (lg, True)):
                    for scale in (True, False):
                        want = CO.step(p, cls, axis, stages=stages, flags=fo, axis_logits=is_logits, features=scale)
                        feat = torch.empty((b, m * d), dtype=torch.float32, device="cuda")
                        got = ops.step(dev(p), dev(cls), dev(axis), stages=stages, flags=fp,
                                       want=("done", "prev_done", "reward", "num_points"), features_out=feat,
                                       scale_observation=scale)
                        tag = (spec, b, stages, sem, kind, is_logits, scale)
                        assert np.array_equal(host(got["points"]), want["points"], equal_nan=True), tag
                        assert np.array_equal(host(feat), want["features"], equal_nan=True), tag
                        for k in ("done", "prev_done", "reward", "num_points"):
                            assert np.array_equal(host(got[k]), want[k]), (k, tag)
                    if is_logits:  # the plain step with the agent's logits as its axis
                        want = CO.step(p, cls, axis, stages=stages, flags=fo, axis_logits=True)
                        got = ops.step(dev(p), dev(cls), dev(axis), stages=stages, flags=fp, want=("done", "reward"))
                        assert np.array_equal(host(got["points"]), want["points"], equal_nan=True), (spec, b, stages, sem, kind)
                        assert np.array_equal(host(got["reward"]), want["reward"])


def test_step_features_equals_step_then_get_features():
    """hk_step_features (the step and the observation features of its result in one launch) against hk_step followed
    by hk_get_features: class-id subsets with an int32 axis or the agent's logits, with and without rescaling, JAX and
    torch semantics, hot and run-time configured stage masks; unsupported shapes / layouts say so"""
    from hironaka_amd._lib import HironakaHipError
    rng = np.random.default_rng(9)
    for (m, d) in ((20, 3), (10, 3), (20, 4)):
        for b in (1, 17, 1000, 4099):
            for stages, sem in ((7, "jax"), (5, "jax"), (7, "torch"), (15, "jax")):
                for dense in (False, True):
                    P = ops.generate_points(b, m, d, 20, seed=b + m, newton=not dense, reposition=not dense)
                    cls = torch.tensor(rng.integers(0, 2 ** d - d - 1, b), dtype=torch.int32, device="cuda")
                    ax = torch.tensor(rng.integers(0, d, b), dtype=torch.int32, device="cuda")
                    logits = torch.tensor(rng.standard_normal((b, d)).astype(np.float32), device="cuda")
                    fl = ops.make_flags(sem, sem != "jax", sem == "torch")
                    for axis in (ax, logits):
                        for scale in (True, False):
                            ref = ops.step(P, cls, axis, stages=stages, flags=fl, want=("done", "reward"))
                            want = ops.get_features(ref["points"], scale)
                            feat = torch.empty((b, m * d), dtype=torch.float32, device="cuda")
                            got = ops.step(P, cls, axis, stages=stages, flags=fl, want=("done", "reward"),
                                           features_out=feat, scale_observation=scale)
                            assert torch.equal(got["points"], ref["points"]) and torch.equal(got["done"], ref["done"])
                            assert torch.equal(got["reward"], ref["reward"])
                            assert torch.equal(feat, want), (m, d, b, stages, sem, dense, scale)
    P = ops.generate_points(8, 20, 3, 20, seed=1)
    feat = torch.empty((8, 60), dtype=torch.float32, device="cuda")
    # a float mask with an int32 axis: the JAX trainer's stage mask only (the agent-role tree of the search)
    mask = ops.decode_host_class(torch.tensor(rng.integers(0, 4, 8), dtype=torch.int32, device="cuda"), 3, torch.float32)
    ax = torch.tensor(rng.integers(0, 3, 8), dtype=torch.int32, device="cuda")
    ref = ops.step(P, mask, ax, stages=7)
    got = ops.step(P, mask, ax, stages=7, features_out=feat)
    assert torch.equal(got["points"], ref["points"]) and torch.equal(feat, ops.get_features(ref["points"], True))
    with pytest.raises(HironakaHipError) as err:
        ops.step(P, mask, ax, stages=5, features_out=feat)
    assert err.value.status == A.HK_ERR_UNSUPPORTED
