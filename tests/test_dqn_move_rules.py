"""tests/dqn_move_rules.py pinned in two ways, without a GPU: its argmax rules against torch on the CPU (the expression
of fused_game.py:143-146 followed by torch.argmax), and the whole of `evaluate` against tests/golden/dqn_trainer.npz,
which tests/golden/make_dqn_trainer_golden.py recorded from the reference's own Trainer.get_rho_for_pair and
count_actions.  The schedulers and the dummy player modules are compared with the same recording."""
import itertools
import os

import numpy as np
import pytest
import torch

import dqn_move_rules as R
from hironaka_amd import player_modules, scheduler

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dqn_trainer.npz")
TAGS = ("m5_d2", "m20_d3", "m8_d4")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def odd_rows(d, dtype):
    """every row over a small alphabet of awkward values, for d <= 3; a random sample of them beyond"""
    dt = np.dtype(dtype).type
    alphabet = [dt(np.nan), dt(np.inf), dt(-np.inf), dt(-0.0), dt(0.0), np.finfo(dtype).min, np.finfo(dtype).max,
                dt(1.5), dt(-1.5)]
    rows = np.array(list(itertools.product(alphabet, repeat=d)) if d <= 3 else [], dtype).reshape(-1, d)
    if d > 3:
        rng = np.random.default_rng(d)
        rows = np.array(alphabet, dtype)[rng.integers(0, len(alphabet), (4000, d))]
    return rows


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=("f32", "f64"))
@pytest.mark.parametrize("d", (2, 3, 5))
def test_axis_rule_is_torchs(d, dtype):
    """masked: q * mask + (1 - mask) * finfo.min, then argmax, on rows of ties, infinities, NaNs inside and outside the
    subset, -0.0 and finfo.min itself, against every subset; unmasked: argmax alone.  The mask comes in q's dtype or, for
    a float32 q, in float64 (torch then promotes q, exactly).  A float64 q under a float32 mask is not covered by the
    rule: there torch forms (1 - mask) * finfo(float64).min in float32, where it overflows"""
    q = odd_rows(d, dtype)
    masks = R.O.decode_table(d)
    for mask, mask_dtype in itertools.product(masks, {torch.from_numpy(q).dtype, torch.float64}):
        coords = np.broadcast_to(mask, q.shape)
        tq, tm = torch.from_numpy(q), torch.from_numpy(np.ascontiguousarray(coords)).to(mask_dtype)
        masked = tq * tm + (1 - tm) * torch.finfo(tq.dtype).min
        assert (R.agent_axis(q, coords, True) == torch.argmax(masked, dim=1).numpy()).all(), mask
    assert (R.agent_axis(q, None, False) == torch.argmax(torch.from_numpy(q), dim=1).numpy()).all()


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=("f32", "f64"))
def test_host_pick_is_torchs_argmax_and_decode(dtype):
    for d in (2, 3, 4):
        q = odd_rows(R.num_classes(d), dtype)[:20000]
        cls, coords = R.host_pick(q, d, dtype)
        assert (cls == torch.argmax(torch.from_numpy(q), dim=1).numpy()).all()
        assert coords.dtype == dtype and (coords == R.O.decode_table(d)[cls]).all()
        assert ((coords == 0) | (coords == 1)).all() and (coords.sum(1) >= 2).all()


def set_nets(g, tag):
    """the recording's SetNet players as numpy callables: rows summed, times the weights, plus the bias, in float32"""
    hw, hb, aw, av, ab = (g[f"{tag}/{k}"] for k in ("host_w", "host_b", "agent_w", "agent_v", "agent_b"))
    host = lambda feats: feats.sum(1, dtype=np.float32) @ hw + hb  # noqa: E731
    agent = lambda feats, coords: feats.sum(1, dtype=np.float32) @ aw + coords.astype(np.float32) @ av + ab  # noqa: E731
    return host, agent


@pytest.mark.parametrize("tag", TAGS)
def test_evaluate_reproduces_the_reference_trainer(golden, tag):
    """rho, the lengths and both roles' action counts of the reference's get_rho_for_pair / count_actions(er=0.0)"""
    host, agent = set_nets(golden, tag)
    start, max_steps = golden[f"{tag}/start"], int(golden[f"{tag}/max_steps"])
    for count_for in ("host", "agent"):
        lengths, initial_done, counts, rho, _ = R.evaluate(start, host, agent, max_steps, scale_observation=False,
                                                           count_for=count_for)
        assert (lengths == golden[f"{tag}/lengths"]).all()
        assert (initial_done == golden[f"{tag}/initial_done"]).all()
        assert (counts == golden[f"{tag}/{count_for}_counts"]).all()
        assert rho.dtype == np.float32 and rho == golden[f"{tag}/rho"]
    assert R.evaluate(start, host, agent, max_steps, scale_observation=False)[2] is None


def test_evaluate_of_nothing_is_nan():
    """0 / 0: every game over at the start"""
    start = np.full((3, 4, 2), -1, np.float32)
    lengths, initial_done, _, rho, _ = R.evaluate(start, lambda f: np.zeros((3, 1), np.float32),
                                                  lambda f, c: np.zeros((3, 2), np.float32), 5)
    assert (lengths == 0).all() and initial_done.all() and np.isnan(rho)


def test_schedulers_match_the_reference(golden):
    value, initial, rate, inverse_rate, er, initial_er = golden["sched/params"]
    made = {
        "constant": scheduler.ConstantScheduler(value),
        "exponential_lr": scheduler.ExponentialLRScheduler(value, mode="exponential", initial_lr=initial, rate=rate),
        "inverse_lr": scheduler.InverseLRScheduler(value, mode="inverse", initial_lr=initial, rate=inverse_rate),
        "exponential_er": scheduler.ExponentialERScheduler(er, mode="exponential", initial_er=initial_er, rate=rate),
    }
    assert tuple(golden["sched/steps"]) == (0, 1, 10, 1000)
    for name, s in made.items():
        got = np.array([s(int(step)) for step in golden["sched/steps"]], np.float64)
        np.testing.assert_allclose(got, golden[f"sched/{name}"], rtol=1e-12, atol=0, err_msg=name)
    for cls, key in ((scheduler.ExponentialLRScheduler, "initial_lr"), (scheduler.InverseLRScheduler, "initial_lr"),
                     (scheduler.ExponentialERScheduler, "initial_er")):
        assert cls.mandatory_keys == [key, "rate"]
        with pytest.raises(AssertionError):
            cls(0.1, rate=0.5)
        with pytest.raises(AssertionError):
            cls(0.1, **{key: 0.5})


def test_dummy_modules_match_the_reference(golden):
    d, m, dev = 3, 20, torch.device("cpu")
    obs = {"points": torch.from_numpy(golden["dummy/points"]), "coords": torch.from_numpy(golden["dummy/coords"])}
    for name, module, x in (("choose_first", player_modules.ChooseFirstAgentModule(d, m, dev), obs),
                            ("choose_last", player_modules.ChooseLastAgentModule(d, m, dev), obs),
                            ("all_coord", player_modules.AllCoordHostModule(d, m, dev), obs["points"])):
        out = module(x)
        assert isinstance(module, player_modules.DummyModule) and out.dtype == torch.float32
        assert (out.numpy() == golden[f"dummy/{name}"]).all(), name
    # the random ones: one-hot float32, the agent's inside the subset
    out = player_modules.RandomAgentModule(d, m, dev)(obs)
    assert out.dtype == torch.float32 and (out.sum(1) == 1).all() and ((out * obs["coords"]).sum(1) == 1).all()
    out = player_modules.RandomHostModule(d, m, dev)(obs["points"])
    assert out.dtype == torch.float32 and out.shape == (16, 4) and (out.sum(1) == 1).all()
