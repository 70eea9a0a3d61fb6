"""tests/optim_rules.py (the rules of hk_optim_prepare / hk_optim_apply, include/hironaka_hip_optim.h) against what
torch's own clip_grad_norm_, Adam and SGD computed on the CPU (tests/golden/optim_step.npz, written by
tests/golden/make_optim_golden.py).  Bit for bit: the clipping coefficient from torch's norm, the clipped gradients,
Adam's exp_avg and exp_avg_sq, all of SGD.  Within a reasoned bound: the total norm (torch adds in another order).  Within
the fixture's measured tolerance: Adam's parameters (torch's vectorised addcdiv_ has no scalar formulation)."""
import os

import numpy as np
import pytest
import torch

import dqn_rules as D
import optim_rules as R
from conftest import GOLDEN

same_bits = R.same_bits


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "optim_step.npz"))


def shapes_of(net_kind):
    return [tuple(p.shape) for p in D.build_net(net_kind, R.NUM_ACTIONS, torch.float32).parameters()]


def test_fixture_holds_every_case(fix):
    keys = R.case_keys()
    assert len(keys) == len(R.CASES) * 6
    for key, _, kind, hyper, dtype, net in keys:
        n = sum(int(np.prod(s)) for s in shapes_of(net))
        assert fix[f"{key}_p"].shape == (R.STEPS + 1, n) and fix[f"{key}_p"].dtype == dtype
        assert fix[f"{key}_grad"].shape == fix[f"{key}_clipped"].shape == (R.STEPS, n)
        assert (f"{key}_s2" in fix) == (kind == R.ADAM)
        assert (f"{key}_p64" in fix) == (kind == R.ADAM and dtype == np.float32)
        assert (f"{key}_s1" in fix) == (kind == R.ADAM or bool(hyper.get("momentum")))
        bites = fix[f"{key}_norm"].astype(np.float64) + 1e-6 > float(fix[f"{key}_max_norm"])
        assert bites.any() and not bites.all(), key  # clipping bites in some steps and not in others
    assert float(fix["adam_p_tolerance"]) == 2.0 * float(fix["adam_p_yardstick"]) > 0.0


def test_total_norm_and_clip_coef(fix):
    """the norm: float32 within 1 ulp of torch's; float64 within n * 2^-52 relative (n double additions of rounded
    squares in either order).  The coefficient from torch's norm and the clipped gradients: torch's bits."""
    for key, _, _, _, dtype, net in R.case_keys():
        shapes = shapes_of(net)
        max_norm = float(fix[f"{key}_max_norm"])
        for s in range(R.STEPS):
            grad, want = fix[f"{key}_grad"][s], fix[f"{key}_norm"][s]
            got = R.total_norm(R.split(grad, shapes), dtype)
            assert got.dtype == dtype
            if dtype == np.float32:
                assert abs(float(got) - float(want)) <= float(np.spacing(want)), (key, s)
            else:
                assert abs(float(got) - float(want)) <= grad.size * 2.0 ** -52 * float(want), (key, s)
            t = torch.from_numpy(np.array(want))
            theirs = torch.clamp(max_norm / (t + 1e-6), max=1.0).numpy()
            coef = R.clip_coef(want, max_norm, dtype)
            assert same_bits(np.array(coef), theirs), (key, s)
            assert same_bits(R.scale(grad, coef), fix[f"{key}_clipped"][s]), (key, s)
    assert R.clip_coef(np.float32(3.0), np.inf, np.float32) == 1.0
    assert np.isnan(R.clip_coef(np.float32(np.inf), np.inf, np.float32))
    assert np.isnan(R.clip_coef(np.float32(np.nan), 1.0, np.float32))
    assert R.clip_coef(np.float32(np.inf), 1.0, np.float32) == 0.0


def torch_state(fix, key, s, dtype, hyper):
    """the state block as the rules would have left it, but with torch's norm: its coefficient is torch's"""
    st = R.new_state()
    for k in range(s + 1):
        st = R.prepare(st, [], dtype, lr=float(fix["lr"]), advance=True,
                       beta1=hyper.get("betas", (0, 0))[0], beta2=hyper.get("betas", (0, 0))[1])
    st["clip_coef"] = float(R.clip_coef(fix[f"{key}_norm"][s], float(fix[f"{key}_max_norm"]), dtype))
    return st


def test_sgd_is_torch_bit_for_bit(fix):
    seen = 0
    for key, _, kind, hyper, dtype, _ in R.case_keys():
        if kind != R.SGD:
            continue
        for s in range(R.STEPS):
            st = torch_state(fix, key, s, dtype, hyper)
            buf = fix[f"{key}_s1"][s - 1] if hyper.get("momentum") and s > 0 else None
            p, g, buf = R.sgd(fix[f"{key}_p"][s], fix[f"{key}_grad"][s], buf, st, **hyper)
            assert same_bits(p, fix[f"{key}_p"][s + 1]), (key, s)
            assert same_bits(g, fix[f"{key}_clipped"][s]), (key, s)
            if hyper.get("momentum"):
                assert same_bits(buf, fix[f"{key}_s1"][s]), (key, s)
            seen += 1
    assert seen == 5 * 6 * R.STEPS


def test_adam_state_is_torch_bit_for_bit_and_parameters_within_the_measured_tolerance(fix):
    tolerance, yardstick = float(fix["adam_p_tolerance"]), float(fix["adam_p_yardstick"])
    worst = {np.float32: [0.0, 0.0], np.float64: [0.0, 0.0]}  # the rule's and torch's distance from the reference
    exact = total = 0
    from_torch64 = 0.0
    for key, _, kind, hyper, dtype, _ in R.case_keys():
        if kind != R.ADAM:
            continue
        for s in range(R.STEPS):
            st = torch_state(fix, key, s, dtype, hyper)
            n = fix[f"{key}_p"].shape[1]
            m0 = fix[f"{key}_s1"][s - 1] if s > 0 else np.zeros(n, dtype)
            v0 = fix[f"{key}_s2"][s - 1] if s > 0 else np.zeros(n, dtype)
            p0 = fix[f"{key}_p"][s]
            kw = dict(beta1=hyper["betas"][0], beta2=hyper["betas"][1], weight_decay=hyper.get("weight_decay", 0.0))
            p, g, m, v = R.adam(p0, fix[f"{key}_grad"][s], m0, v0, st, **kw)
            assert same_bits(g, fix[f"{key}_clipped"][s]), (key, s)
            assert same_bits(m, fix[f"{key}_s1"][s]), (key, s)
            assert same_bits(v, fix[f"{key}_s2"][s]), (key, s)
            ref = R.adam_reference(p0, fix[f"{key}_clipped"][s], m0, v0, st, hyper["betas"],
                                   weight_decay=hyper.get("weight_decay", 0.0))
            ours, theirs = R.adam_distance(p, ref, p0, dtype), R.adam_distance(fix[f"{key}_p"][s + 1], ref, p0, dtype)
            worst[dtype] = [max(worst[dtype][0], ours), max(worst[dtype][1], theirs)]
            assert ours <= tolerance, (key, s, ours, tolerance)
            if dtype == np.float32:  # and from torch's own float64 Adam, which the yardstick was measured from
                direct = R.adam_distance(p, fix[f"{key}_p64"][s], p0, dtype)
                from_torch64 = max(from_torch64, direct)
                assert direct <= tolerance, (key, s, direct, tolerance)
            exact += int((p == fix[f"{key}_p"][s + 1]).sum())
            total += n
    print(f"float32 rule from torch's float64 Adam: {from_torch64:.3f} units")
    print(f"Adam's parameters, units of max(ulp(p), ulp(update)) from the reference: float32 rule {worst[np.float32][0]:.3f}"
          f" torch {worst[np.float32][1]:.3f}; float64 rule {worst[np.float64][0]:.3f} torch {worst[np.float64][1]:.3f}; "
          f"yardstick {yardstick:.3f}, tolerance {tolerance:.3f}; {exact} of {total} elements equal torch's bits")
    assert exact > 0.9 * total


def test_state_block_advances():
    st = R.new_state()
    for k in range(1, 4):
        st = R.prepare(st, [np.array([3.0, 4.0], np.float32)], np.float32, max_norm=1.0, lr=0.1, beta1=0.9, beta2=0.999,
                       advance=True)
        assert st["step"] == k and st["total_norm"] == 5.0
        assert abs(st["beta1_pow"] - 0.9 ** k) <= k * 2.0 ** -53 * 0.9 ** k
        assert abs(st["beta2_pow"] - 0.999 ** k) <= k * 2.0 ** -53 * 0.999 ** k
        assert st["neg_step_size"] == -(0.1 / (1.0 - st["beta1_pow"])) and st["bias2_sqrt"] == (1.0 - st["beta2_pow"]) ** 0.5
    assert st["clip_coef"] == float(np.float32(1.0) / (np.float32(5.0) + np.float32(1e-6)) * np.float32(1.0))
    kept = R.prepare(st, [], np.float64, lr=0.5)
    assert kept["step"] == 3 and kept["lr"] == 0.5 and kept["total_norm"] == 0.0 and kept["clip_coef"] == 1.0


def test_slots_follow_the_chunks():
    """one slot per 16 KiB of every gradient; a sum of ones is exact whatever the order"""
    for dtype in R.DTYPES:
        per = R.CHUNK_BYTES // np.dtype(dtype).itemsize
        sizes = [0, 1, per, per + 1, 2 * per + 3]
        grads = [np.ones(n, dtype) for n in sizes]
        assert R.workgroups(sizes, dtype) == 0 + 1 + 1 + 2 + 3
        assert R.slots(grads) == [1.0, float(per), float(per), 1.0, float(per), float(per), 3.0]
        assert R.sum_squares(grads) == float(sum(sizes))
