"""The rule of hk_pv_loss (include/hironaka_hip_pvloss.h) restated in plain numpy float64: what test_pv_loss_rules.py
pins to torch's own softmax / log_softmax / abs / mean and to autograd, and test_gpu_pv_loss.py holds the kernel to.
Inputs are float32 or float64 arrays; every operation below is a float64 one, in the order the header writes it; the
outputs are float64 (the kernel's float32 outputs are these, rounded once)."""
import collections

import numpy as np

BAD_INDEX = 1
PvLoss = collections.namedtuple("PvLoss", "loss row_loss dlogits dvalue status")


def _quiet(fn):
    def wrapped(*args, **kw):
        with np.errstate(all="ignore"):
            return fn(*args, **kw)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


def rows_of(index, batch, num_samples):
    """(r [B] int64 with the out-of-range entries at 0, ok [B] bool)"""
    r = np.arange(batch, dtype=np.int64) if index is None else np.asarray(index).reshape(-1).astype(np.int64)
    ok = (r >= 0) & (r < num_samples)
    return np.where(ok, r, 0), ok


@_quiet
def pv_loss(logits, value, target_policy, target_value, weight=None, index=None):
    """PvLoss(loss, row_loss [B], dlogits [B, A], dvalue [B], status), all float64; a row whose index is out of range
    is zero in row_loss, dlogits and dvalue and sets BAD_INDEX"""
    x = np.asarray(logits, dtype=np.float64)
    B, A = x.shape
    r, ok = rows_of(index, B, np.asarray(target_policy).shape[0])
    t = np.asarray(target_policy, dtype=np.float64)[r]
    v = np.asarray(value, dtype=np.float64).reshape(B)
    tv = np.asarray(target_value, dtype=np.float64).reshape(-1)[r]
    w = np.ones(B) if weight is None else np.asarray(weight, dtype=np.float64).reshape(-1)[r]
    et = np.exp(t - t.max(axis=1, keepdims=True))
    q = et / et.sum(axis=1, keepdims=True)
    dx = x - x.max(axis=1, keepdims=True)
    logp = dx - np.log(np.exp(dx).sum(axis=1, keepdims=True))
    p = np.exp(logp)
    sum_q = q.sum(axis=1, keepdims=True)
    cross = np.where(q == 0, 0.0, q * logp).sum(axis=1)  # no 0 * inf; a NaN q is not 0
    d = v - tv
    row = (-cross / A + np.abs(d)) * w
    dlogits = w[:, None] * (p * sum_q - q) / (float(A) * float(B))
    dvalue = w * np.sign(d) / B
    row, dvalue, dlogits = np.where(ok, row, 0.0), np.where(ok, dvalue, 0.0), np.where(ok[:, None], dlogits, 0.0)
    total = 0.0
    for one in row:
        total += float(one)
    return PvLoss(np.float64(total / B), row, dlogits, dvalue, 0 if ok.all() else BAD_INDEX)


def ulp32(x):
    """the float32 unit in the last place at |x| (of a float64 array), the smallest subnormal at 0"""
    x = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    with np.errstate(all="ignore"):
        return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def within(got, want, extra=0.0):
    """got (float32) within one float32 ulp of want (float64) plus `extra` absolute; NaN and inf have to sit in the same
    places, with the same sign"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    with np.errstate(all="ignore"):
        want32 = want.astype(np.float32).astype(np.float64)  # overflow to inf as the single rounding does
    finite = np.isfinite(want32)
    if not np.array_equal(got[~finite], want32[~finite], equal_nan=True):
        return False
    slack = ulp32(want[finite]) + np.broadcast_to(np.asarray(extra, dtype=np.float64), want.shape)[finite]
    return bool((np.abs(got[finite] - want[finite]) <= slack).all())


# ---- the cases both test files share -----------------------------------------------------------------------------------

def case(rng, B, A, N=None, weight=True, index=True, hard=True):
    """float32 inputs (logits, value [B], target_policy [N, A], target_value [N], weight [N] or None, index [B] or None).
    With `hard` (and room for it): -inf target entries, logits of +-1e4, value == target_value, a zero weight, a
    repeated and a permuted index."""
    N = (B + 5 if index else B) if N is None else N
    logits = (2.0 * rng.standard_normal((B, A))).astype(np.float32)
    value = np.tanh(rng.standard_normal(B)).astype(np.float32)
    target_policy = (3.0 * rng.standard_normal((N, A))).astype(np.float32)
    target_value = rng.integers(-4, 5, N).astype(np.float32) / 4
    w = rng.uniform(0.25, 2.0, N).astype(np.float32) if weight else None
    idx = rng.permutation(N)[:B].astype(np.int64) if index else None
    if idx is not None and B > 2:
        idx[1] = idx[0]  # a sample taken twice
    if hard:
        r = idx if idx is not None else np.arange(B)
        if A > 1:
            target_policy[r[0], rng.integers(0, A)] = -np.inf  # a masked action
            logits[B - 1, 0], logits[B - 1, A - 1] = 1e4, -1e4  # the max-subtraction matters
        if A > 2 and B > 1:
            target_policy[r[B - 1], : A - 1] = -np.inf  # all but one masked
        value[B // 2] = target_value[r[B // 2]]  # sign(0) = 0
        if w is not None:
            w[r[B // 3]] = 0.0
    return logits, value, target_policy, target_value, w, idx
