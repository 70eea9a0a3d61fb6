"""tests/pv_loss_rules.py, the numpy statement of hk_pv_loss's rule, against torch's own operators on the CPU in float64:
F.softmax / F.log_softmax / abs / mean as hironaka/jax/loss.py:12-24 composes them, and autograd for both gradients.
Two float64 evaluations of the same formula in different orders: they agree to a few units of 2^-52 of the largest term."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pv_loss_rules as R

SHAPES = [(1, 1), (2, 3), (7, 4), (33, 26), (5, 120), (3, 255)]


def _torch_loss(logits, value, target_policy, target_value, weight):
    """loss.py:12-24 with torch's operators; the product is masked where the target's softmax is 0, as the rule says"""
    q = F.softmax(target_policy, dim=-1)
    logp = F.log_softmax(logits, dim=-1)
    policy_loss = torch.where(q == 0, torch.zeros_like(q), -q * logp).mean(dim=-1)
    value_loss = (value - target_value).abs()
    weight = torch.ones_like(value) if weight is None else weight
    return ((policy_loss + value_loss) * weight).mean(), (policy_loss + value_loss) * weight


def _close(got, want, scale):
    return np.abs(np.asarray(got) - np.asarray(want)).max() <= 64 * np.finfo(np.float64).eps * scale


@pytest.mark.parametrize("weight", [False, True])
@pytest.mark.parametrize("index", [False, True])
def test_rule_matches_torch_float64_and_autograd(weight, index):
    rng = np.random.default_rng(11)
    for B, A in SHAPES:
        logits, value, tp, tv, w, idx = R.case(rng, B, A, weight=weight, index=index)
        got = R.pv_loss(logits, value, tp, tv, w, idx)
        assert got.status == 0 and got.dlogits.shape == (B, A) and got.dvalue.shape == (B,)
        gather = (lambda a: a) if idx is None else (lambda a: a[idx])
        x = torch.from_numpy(logits).double().requires_grad_()
        v = torch.from_numpy(value).double().requires_grad_()
        loss, rows = _torch_loss(x, v, torch.from_numpy(gather(tp)).double(), torch.from_numpy(gather(tv)).double(),
                                 torch.from_numpy(gather(w)).double() if w is not None else None)
        loss.backward()
        scale = max(1.0, float(rows.detach().abs().max()))
        assert _close(got.loss, loss.item(), scale), (B, A)
        assert _close(got.row_loss, rows.detach().numpy(), scale), (B, A)
        assert _close(got.dlogits, x.grad.numpy(), 1.0), (B, A)
        assert _close(got.dvalue, v.grad.numpy(), 1.0), (B, A)  # torch multiplies by a rounded 1 / B, the rule divides
        if w is None:
            assert np.array_equal(got.dvalue, v.grad.numpy()), (B, A)  # +-1 / B or 0: no rounding to differ in


def test_hard_inputs_are_what_they_claim():
    """the shared case really holds a masked target, logits that overflow without the max-subtraction, a value on its
    target, a zero weight and a repeated index -- and the rule stays finite on them"""
    rng = np.random.default_rng(12)
    logits, value, tp, tv, w, idx = R.case(rng, 9, 4)
    assert np.isneginf(tp[idx]).any() and np.abs(logits).max() == 1e4 and (w[idx] == 0).any()
    assert (value == tv[idx]).any() and len(set(idx.tolist())) < len(idx) and not (np.sort(idx) == idx).all()
    got = R.pv_loss(logits, value, tp, tv, w, idx)
    assert all(np.isfinite(a).all() for a in (got.loss, got.row_loss, got.dlogits, got.dvalue))
    assert (got.dvalue[value == tv[idx]] == 0).all() and (got.dlogits[w[idx] == 0] == 0).all()
    q_zero = np.isneginf(tp[idx])
    assert (got.dlogits[q_zero & (w[idx] != 0)[:, None]] >= 0).all()  # p * sum(q) / (A * B): nothing subtracted
    with np.errstate(all="ignore"):
        assert not np.isfinite(np.exp(logits.astype(np.float64)).sum(axis=1)).all()


def test_repeated_rows_give_repeated_results_and_bad_index_zeroes_its_row():
    rng = np.random.default_rng(13)
    logits, value, tp, tv, w, _ = R.case(rng, 6, 5, N=8, index=False, hard=False)
    logits[3], value[3] = logits[0], value[0]
    idx = np.array([2, 7, 7, 2, 0, 1], dtype=np.int64)
    got = R.pv_loss(logits, value, tp, tv, w, idx)
    assert np.array_equal(got.dlogits[0], got.dlogits[3]) and got.row_loss[0] == got.row_loss[3]
    plain = R.pv_loss(logits, value, tp[idx], tv[idx], w[idx], None)
    assert all(np.array_equal(a, b) for a, b in zip(got[:4], plain[:4]))
    for bad in (-1, 8, 2 ** 40):
        idx2 = idx.copy()
        idx2[4] = bad
        out = R.pv_loss(logits, value, tp, tv, w, idx2)
        assert out.status == R.BAD_INDEX and out.row_loss[4] == 0 and out.dvalue[4] == 0 and (out.dlogits[4] == 0).all()
        keep = np.arange(6) != 4
        assert np.array_equal(out.dlogits[keep], got.dlogits[keep]) and np.array_equal(out.row_loss[keep], got.row_loss[keep])
        assert abs(out.loss - got.row_loss[keep].sum() / 6) <= 8 * np.finfo(np.float64).eps * np.abs(got.row_loss).sum()


def test_nan_stays_in_its_row():
    rng = np.random.default_rng(14)
    logits, value, tp, tv, w, idx = R.case(rng, 5, 3, hard=False)
    clean = R.pv_loss(logits, value, tp, tv, w, idx)
    logits[2, 1] = np.nan
    got = R.pv_loss(logits, value, tp, tv, w, idx)
    keep = np.arange(5) != 2
    assert np.isnan(got.loss) and np.isnan(got.row_loss[2]) and np.isnan(got.dlogits[2]).all()
    assert np.array_equal(got.dlogits[keep], clean.dlogits[keep]) and np.array_equal(got.dvalue, clean.dvalue)


def test_within_is_one_ulp():
    want = np.array([1.0, -3.0, 0.0, np.inf, np.nan, 2.0 ** -10])
    exact = want.astype(np.float32)
    assert R.within(exact, want)
    assert R.within(np.nextafter(exact, np.float32(np.inf)), want)
    two = np.nextafter(np.nextafter(exact, np.float32(np.inf)), np.float32(np.inf))
    assert not R.within(two[[0]], want[[0]]) and not R.within(two[[5]], want[[5]])
    assert R.within(two[[0]], want[[0]], extra=2.0 ** -22)
    assert not R.within(np.float32([np.nan]), want[[0]]) and not R.within(np.float32([-np.inf]), want[[3]])
