"""The rules of hk_dqn_td / hk_polyak_update (include/hironaka_hip_dqn.h) restated in plain numpy: what
test_dqn_rules.py pins to the reference's own DQNTrainer (tests/golden/dqn_fit.npz) and test_gpu_dqn.py holds the
kernels to.  T is np.float32 or np.float64; every operation below rounds once, to T."""
import math

import numpy as np

BAD_ACTION = 1
_FORMAT = {np.dtype(np.float32): (24, -126, 127), np.dtype(np.float64): (53, -1022, 1023)}  # bits, emin, emax


def _quiet(fn):
    def wrapped(*args, **kw):
        with np.errstate(all="ignore"):
            return fn(*args, **kw)
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


@_quiet
def td_target(next_q, rewards, dones, gamma):
    """[B] T: (T)reward + (done ? 0 : (T)(float)gamma) * max(next_q row); np.max gives NaN for a row with a NaN"""
    T = next_q.dtype.type
    g = T(np.float32(gamma))
    mx = np.max(next_q, axis=1)
    coef = np.where(np.asarray(dones).reshape(-1) != 0, T(0), g).astype(T)
    return np.asarray(rewards).reshape(-1).astype(T) + coef * mx


def _valid(actions, num_actions):
    a = np.asarray(actions).reshape(-1).astype(np.int64)
    return a, (a >= 0) & (a < num_actions)


@_quiet
def td_error(q, target, actions):
    """x [B] T = q[b, a_b] - target (0 where the action is out of range), and which rows are in range"""
    T = q.dtype.type
    a, ok = _valid(actions, q.shape[1])
    picked = q[np.arange(q.shape[0]), np.where(ok, a, 0)]
    return np.where(ok, picked - target, T(0)).astype(T), ok


@_quiet
def td_loss_rows(q, target, actions):
    """[B] T: |x| < 1 ? 0.5 * x * x : |x| - 0.5; 0 for an action out of range"""
    T = q.dtype.type
    x, ok = td_error(q, target, actions)
    ax = np.abs(x)
    rows = np.where(ax < T(1), T(0.5) * x * x, ax - T(0.5)).astype(T)
    return np.where(ok, rows, T(0)).astype(T)


@_quiet
def td_grad(q, target, actions):
    """[B, A] T: clamp(x, -1, 1) / (T)B at the action's column (NaN stays NaN), 0 elsewhere"""
    T = q.dtype.type
    x, ok = td_error(q, target, actions)
    a, _ = _valid(actions, q.shape[1])
    clamped = np.where(x < T(-1), T(-1), np.where(x > T(1), T(1), x)).astype(T)
    out = np.zeros(q.shape, dtype=T)
    rows = np.arange(q.shape[0])[ok]
    out[rows, a[ok]] = (clamped / T(q.shape[0]))[ok]
    return out


@_quiet
def td_loss(q, target, actions):
    """(T)(the sum of the rows in double, in row order / B)"""
    T = q.dtype.type
    total = 0.0
    for v in td_loss_rows(q, target, actions).astype(np.float64):
        total += float(v)
    return T(total / q.shape[0])


def same_bits(a, b):
    """equal bit for bit, but for NaNs, which only have to sit in the same places (a NaN's payload is no rule)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    return bool((nan == np.isnan(b)).all()) and a[~nan].tobytes() == b[~nan].tobytes()


def td_status(actions, num_actions):
    return 0 if _valid(actions, num_actions)[1].all() else BAD_ACTION


# ---- a single-rounding fma in either format -------------------------------------------------------------------------

def _parts(x):
    """a finite float as (integer, exponent): x == integer * 2^exponent exactly"""
    m, e = math.frexp(x)
    return int(m * (1 << 53)), e - 53


def _round(n, e, bits, emin, emax):
    """n * 2^e rounded to nearest, ties to even, in the format of `bits` significant bits (n != 0), as a float"""
    sign = -1.0 if n < 0 else 1.0
    n = abs(n)
    top = n.bit_length() + e - 1              # 2^top <= |value| < 2^(top + 1)
    unit = max(top, emin) - (bits - 1)        # the exponent of the last place (subnormals share emin's)
    shift = unit - e
    if shift > 0:
        q, r = n >> shift, n & ((1 << shift) - 1)
        half = 1 << (shift - 1)
        if r > half or (r == half and (q & 1)):
            q += 1
    else:
        q = n << -shift
    if q.bit_length() + unit - 1 > emax:
        return sign * math.inf
    return sign * math.ldexp(q, unit)          # exact: q has at most `bits` bits (+ a carry into the next binade)


def fma_exact(a, b, c, dtype):
    """round(a * b + c) with ONE rounding to dtype; a, b, c are values of dtype.  (A float64 fma emulated as
    float32(a * b + c in float64) would round twice; Python has math.fma from 3.13 on only.)"""
    dtype = np.dtype(dtype)
    bits, emin, emax = _FORMAT[dtype]
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        with np.errstate(all="ignore"):
            return dtype.type(dtype.type(a) * dtype.type(b) + dtype.type(c))  # inf / NaN: no rounding is involved
    if a == 0.0 or b == 0.0 or c == 0.0:
        with np.errstate(all="ignore"):
            return dtype.type(dtype.type(a) * dtype.type(b) + dtype.type(c))  # a zero term: at most one rounding
    (ma, ea), (mb, eb), (mc, ec) = _parts(a), _parts(b), _parts(c)
    mp, ep = ma * mb, ea + eb
    e = min(ep, ec)
    n = (mp << (ep - e)) + (mc << (ec - e))
    if n == 0:
        return dtype.type(0.0)  # an exact cancellation of nonzero terms is +0 under round-to-nearest
    return dtype.type(_round(n, e, bits, emin, emax))


def polyak(src, dst, tau):
    """fma((T)tau, src, round(dst * (T)(1 - tau))) element by element; 1 - tau is computed in double"""
    dtype = dst.dtype
    T = dtype.type
    t, rest = T(tau), T(1.0 - float(tau))
    with np.errstate(all="ignore"):
        scaled = (dst * rest).astype(dtype)
    flat_s, flat_d = np.asarray(src, dtype=dtype).reshape(-1), scaled.reshape(-1)
    out = np.empty(flat_d.shape, dtype=dtype)
    for i in range(flat_d.size):
        out[i] = fma_exact(t, flat_s[i], flat_d[i], dtype)
    return out.reshape(dst.shape)


# ---- the cases of tests/golden/dqn_fit.npz (make_dqn_golden.py writes them, the tests rebuild the same nets) ----------

TAUS = (0.0, 0.005, 0.3, 1.0)
OBS_DIM, HIDDEN = 6, 8
NET_KINDS = ("two_layer", "three_layer", "batch_norm")


def build_net(kind, num_actions, dtype):
    """the fixture's nets (torch is imported here only: the rules above are plain numpy)"""
    from torch import nn
    if kind == "two_layer":
        layers = [nn.Linear(OBS_DIM, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, num_actions)]
    elif kind == "three_layer":
        layers = [nn.Linear(OBS_DIM, HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, HIDDEN), nn.ReLU(),
                  nn.Linear(HIDDEN, num_actions)]
    else:
        layers = [nn.Linear(OBS_DIM, HIDDEN), nn.BatchNorm1d(HIDDEN), nn.ReLU(), nn.Linear(HIDDEN, num_actions)]
    return nn.Sequential(*layers).to(dtype)


def net_state(net):
    """{name: tensor} of the parameters and the floating buffers (the BatchNorm running statistics), in order"""
    out = dict(net.named_parameters())
    out.update({k: v for k, v in net.named_buffers() if v.is_floating_point()})
    return out
