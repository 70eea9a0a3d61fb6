"""tests/dqn_rules.py (the rules of hk_dqn_td / hk_polyak_update, include/hironaka_hip_dqn.h) against what the
reference's own DQNTrainer._fit_network / _update_target_net / polyak_update computed on torch CPU
(tests/golden/dqn_fit.npz, written by tests/golden/make_dqn_golden.py).  eps_T is the machine epsilon of the case's
dtype.  Targets and Polyak results are compared bit for bit; a gradient entry within 2 eps_T relative (either side
rounds at most twice after x); the loss within B eps_T relative (the any-order bound of a sum of non-negative terms)."""
import os

import numpy as np
import pytest
import torch

import dqn_rules as R
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fit():
    return np.load(os.path.join(GOLDEN, "dqn_fit.npz"))


def _cases(fit):
    return range(len(fit["case_B"]))


same_bits = R.same_bits


def test_fixture_covers_what_it_should(fit):
    n = len(fit["case_B"])
    assert n == 12 and {(int(b), int(a)) for b, a in zip(fit["case_B"], fit["case_A"])} == {
        (b, a) for b in (1, 5, 259) for a in (1, 3, 11, 120)}
    single = []
    for f64 in (0, 1):
        mine = [k for k in range(n) if fit["case_f64"][k] == f64]
        assert {int(fit["case_B"][k]) for k in mine} == {1, 5, 259}
        assert {int(fit["case_A"][k]) for k in mine} == {1, 3, 11, 120}
        assert {int(fit["case_net"][k]) for k in mine} == {0, 1, 2} and {int(fit["case_dones"][k]) for k in mine} == {0, 1, 2}
    for k in range(n):
        dtype = np.float64 if fit["case_f64"][k] else np.float32
        assert fit[f"c{k}_next_q"].dtype == fit[f"c{k}_current_q"].dtype == fit[f"c{k}_target"].dtype == dtype
        assert fit[f"c{k}_rewards"].dtype == np.float32 and set(np.unique(fit[f"c{k}_rewards"])) <= {-1.0, 0.0, 1.0}
        x, _ = R.td_error(fit[f"c{k}_current_q"], fit[f"c{k}_target"], fit[f"c{k}_actions"])
        if fit["case_B"][k] > 1:
            assert np.abs(x).min() < 1 < np.abs(x).max() and np.abs(x).max() > 3, k  # both branches, one far out
        else:
            single.append(abs(float(x[0])))
    assert min(single) < 1 < max(single)


def test_target_matches_the_reference_bit_for_bit(fit):
    for k in _cases(fit):
        got = R.td_target(fit[f"c{k}_next_q"], fit[f"c{k}_rewards"], fit[f"c{k}_dones"], float(fit["case_gamma"][k]))
        assert same_bits(got, fit[f"c{k}_target"]), k


def test_gradient_and_loss_match_the_reference(fit):
    worst_grad = worst_loss = 0.0
    for k in _cases(fit):
        q, target, actions = fit[f"c{k}_current_q"], fit[f"c{k}_target"], fit[f"c{k}_actions"]
        eps, B = np.finfo(q.dtype).eps, q.shape[0]
        got, want = R.td_grad(q, target, actions).astype(np.float64), fit[f"c{k}_dq"].astype(np.float64)
        assert ((want == 0) == (got == 0)).all(), k  # the same zeros, one entry per row
        nz = want != 0
        err = np.abs(got[nz] - want[nz]) / np.abs(want[nz]) / eps
        worst_grad = max(worst_grad, float(err.max()))
        assert err.max() <= 2.0, (k, err.max())
        loss, ref = float(R.td_loss(q, target, actions)), float(fit[f"c{k}_loss"])
        worst_loss = max(worst_loss, abs(loss - ref) / abs(ref) / eps)
        assert abs(loss - ref) <= B * eps * abs(ref), (k, loss, ref)
    print(f"worst gradient error {worst_grad:.2f} eps, worst loss error {worst_loss:.2f} eps")


def test_polyak_matches_the_reference_bit_for_bit(fit):
    for k in _cases(fit):
        names = [key[len(f"c{k}_t1_"):] for key in fit.files if key.startswith(f"c{k}_t1_")]
        assert names and (fit["case_net"][k] != 2 or any("running_var" in n for n in names))
        for j, tau in enumerate(R.TAUS):
            for name in names:
                src, dst, want = fit[f"c{k}_q1_{name}"], fit[f"c{k}_t1_{name}"], fit[f"c{k}_tau{j}_{name}"]
                assert same_bits(R.polyak(src, dst, tau), want), (k, tau, name)
                if tau == 1.0:
                    assert same_bits(want, src)
                if tau == 0.0:
                    assert same_bits(want, dst)


def test_unfused_polyak_is_not_the_rule():
    """the rounded multiply + fused multiply-add is what the reference computes; two roundings are not"""
    rng = np.random.default_rng(3)
    src, dst = (rng.standard_normal(4096).astype(np.float32) for _ in range(2))
    t = torch.from_numpy(dst.copy())
    t.mul_(1 - 0.3)
    torch.add(t, torch.from_numpy(src), alpha=0.3, out=t)
    assert same_bits(R.polyak(src, dst, 0.3), t.numpy())
    unfused = np.float32(0.3) * src + dst * np.float32(1.0 - 0.3)
    assert not same_bits(unfused, t.numpy())


def test_fma_exact_rounds_once():
    f = np.float32
    # a * b + c lies just above a float32 tie: a float64 sum would hit the tie exactly and round to even
    a, b, c = f(1 + 2.0 ** -12), f(1 + 2.0 ** -12), f(2.0 ** -60)
    exact = R.fma_exact(a, b, c, np.float32)
    twice = f(np.float64(a) * np.float64(b) + np.float64(c))
    assert exact == f(1 + 2.0 ** -11 + 2.0 ** -23) and twice == f(1 + 2.0 ** -11) and exact != twice
    assert R.fma_exact(f(3), f(5), f(-15), np.float32) == 0 and not np.signbit(R.fma_exact(f(3), f(5), f(-15), np.float32))
    assert R.fma_exact(f(2.0 ** -100), f(2.0 ** -49), f(0), np.float32) == f(2.0 ** -149)  # the smallest subnormal
    assert R.fma_exact(f(3e38), f(2), f(1), np.float32) == np.inf
    assert R.fma_exact(np.float64(0.1), np.float64(10), np.float64(-1), np.float64) == 2.0 ** -54
    assert np.isnan(R.fma_exact(f(np.inf), f(0), f(1), np.float32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_nonfinite_rows_match_torch(dtype):
    """NaN, +inf and -inf rows against the reference's three lines on torch CPU; a done row whose max is inf is NaN"""
    gamma = 0.99
    inf, nan = float("inf"), float("nan")
    next_q = torch.tensor([[1.0, nan, 3.0], [nan, nan, nan], [1.0, inf, -2.0], [-inf, -inf, -inf], [inf, 0.5, 1.0],
                           [-inf, 2.0, -inf], [-inf, -inf, -inf], [0.25, -0.5, 0.125]], dtype=dtype)
    rewards = torch.tensor([[1.0], [0.0], [-1.0], [1.0], [0.0], [1.0], [0.0], [-1.0]], dtype=torch.float32)
    dones = torch.tensor([[False], [True], [False], [False], [True], [True], [True], [False]])
    mx, _ = next_q.max(dim=1)
    want = (rewards + (~dones) * gamma * mx.reshape(-1, 1)).reshape(-1)
    assert want.dtype == dtype
    got = R.td_target(next_q.numpy(), rewards.numpy(), dones.numpy(), gamma)
    assert same_bits(got, want.numpy())
    assert np.isnan(got[[0, 1, 4, 6]]).all() and got[2] == np.inf and got[3] == -np.inf and got[5] == 1.0
    q = torch.tensor(np.random.default_rng(0).standard_normal((8, 3)), dtype=dtype, requires_grad=True)
    actions = torch.tensor([[0], [1], [2], [0], [1], [2], [0], [1]])
    picked = torch.gather(q, dim=1, index=actions)
    rows = torch.nn.functional.smooth_l1_loss(picked, want.reshape(-1, 1), reduction="none")
    rows.sum().backward()
    mine = R.td_loss_rows(q.detach().numpy(), got, actions.numpy())
    assert same_bits(mine, rows.detach().numpy().reshape(-1))
    # the gradient's direction: torch's clamp of x, NaN where x is NaN (here without the 1 / B of the mean)
    x, _ = R.td_error(q.detach().numpy(), got, actions.numpy())
    clamped = np.where(x < -1, -1, np.where(x > 1, 1, x))
    picked_grad = q.grad.numpy()[np.arange(8), actions.numpy().reshape(-1)]
    assert same_bits(clamped.astype(picked_grad.dtype), picked_grad)
    assert np.isnan(R.td_grad(q.detach().numpy(), got, actions.numpy())[0, 0])


def test_bad_actions_give_zero_rows():
    q = np.arange(12, dtype=np.float32).reshape(4, 3)
    target = np.array([0.5, 0.5, 0.5, 0.5], dtype=np.float32)
    actions = np.array([-1, 3, 0, 2])
    assert R.td_status(actions, 3) == R.BAD_ACTION and R.td_status(actions[2:], 3) == 0
    rows, grad = R.td_loss_rows(q, target, actions), R.td_grad(q, target, actions)
    assert rows[0] == rows[1] == 0 and rows[2] > 0 and not grad[:2].any() and grad[2, 0] != 0 and grad[3, 2] != 0
