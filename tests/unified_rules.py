"""The rule of one expansion of the role-agnostic search tree (include/hironaka_hip_unified.h; the reference's
hironaka/jax/recurrent_fn.py:126-199 and jax/util.py:240-257), restated in plain numpy on float32 -- every operation an
array operation of that type, so every result is rounded once, as the kernels round.  tests/test_unified_rules.py pins
the pieces to the oracle's composition; the GPU kernels and the CPU build of the lane body are compared with `expand`
and `prior` bit for bit.

A state is m * d points (row-major) followed by a tail of d floats."""
import numpy as np

F = np.float32
CLOSE = np.float32(1e-8)  # isclose(x, 0): |x| <= atol, in float


def masks_of(d):
    """the subsets of >= 2 coordinates as bit masks, in class order"""
    return np.array([v for v in range(1 << d) if v & (v - 1)], np.int64)


def num_actions(d):
    return 2 ** d - d - 1


def is_host_state(states, d):
    """every tail entry close to zero; a NaN is not close"""
    with np.errstate(invalid="ignore"):
        return (np.abs(states[..., -d:]) <= CLOSE).all(-1)


def batch_kind(parents, d):
    """1 when any game's parent is a host state: the decision is the batch's, not the game's"""
    return int(is_host_state(parents, d).any())


def subset_of(action, d):
    """the bit mask of the class id `action`, clamped as hk_decode_host_class clamps"""
    return masks_of(d)[np.clip(np.asarray(action, np.int64), 0, num_actions(d) - 1)]


def bits_of(subset, d, dtype=F):
    return ((np.asarray(subset)[..., None] >> np.arange(d)) & 1).astype(dtype)


def shift(p, c, axis):
    """_jax_ops.py:76-90: x_axis <- sum_k x_k c_k (coordinate order, one rounding per operation) on every row with a
    non-negative entry, the other rows become -1; an axis outside [0, d) matches no coordinate"""
    b, m, d = p.shape
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros((b, m), F)
        for k in range(d):
            s = s + p[:, :, k] * c[:, None, k]
        out = p.copy()
        for k in range(d):
            out[:, :, k] = np.where((np.asarray(axis) == k)[:, None], s, p[:, :, k])
        return np.where((p >= 0).any(-1)[..., None], out, F(-1))


def reposition(p):
    """_jax_ops.py:114-123: per coordinate, the minimum over the rows with an unavailable entry standing in as the
    column's maximum; subtracted unless it is <= 0"""
    b, m, d = p.shape
    with np.errstate(invalid="ignore", over="ignore"):
        colmax = p[:, 0].copy()
        for i in range(1, m):
            colmax = np.where(p[:, i] > colmax, p[:, i], colmax)
        mn = np.where(p[:, 0] >= 0, p[:, 0], colmax)
        for i in range(1, m):
            v = np.where(p[:, i] >= 0, p[:, i], colmax)
            mn = np.where(v < mn, v, mn)
        moved = np.where(p >= 0, p - mn[:, None], F(-1))
        return np.where((mn <= 0)[:, None], p, moved)


def newton(p):
    """_jax_ops.py:32-73: repeated rows become -1 (against the rows as they came), then a row is removed when another
    available row lies below it in every coordinate -- the reference's subtraction, P_i - P_j >= 0"""
    b, m, d = p.shape
    with np.errstate(invalid="ignore", over="ignore"):
        tmp = p.copy()
        for i in range(1, m):
            rep = np.zeros(b, bool)
            for j in range(i):
                rep |= (p[:, i] == p[:, j]).all(-1)
            tmp[rep, i] = F(-1)
        avail = (tmp >= 0).all(-1)
        out = tmp.copy()
        for i in range(m):
            removed = np.zeros(b, bool)
            for j in range(m):
                if j != i:
                    removed |= avail[:, j] & (tmp[:, i] - tmp[:, j] >= 0).all(-1)
            out[removed & avail[:, i], i] = F(-1)
        return out


def step_points(p, c, axis, repos):
    """hk_step in JAX semantics: shift, [reposition], Newton, no rescale"""
    p = shift(p, c, axis)
    if repos:
        p = reposition(p)
    return newton(p)


def count_points(p):
    return (p[:, :, 0] >= 0).sum(1)


def rescale(p):
    """_jax_ops.py:93-111: divide by the maximum over all entries unless it is <= 1e-8; rows without a non-negative
    entry become -1"""
    b, m, d = p.shape
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        flat = p.reshape(b, -1)
        mx = flat[:, 0].copy()
        for e in range(1, m * d):
            mx = np.where(flat[:, e] > mx, flat[:, e], mx)
        skip = mx <= CLOSE
        scaled = np.where(skip[:, None, None], p, p / mx[:, None, None])
        return np.where((p >= 0).any(-1)[..., None], scaled, F(-1))


def _sorts_before(a, b):
    """row a goes before row b: descending, last coordinate primary"""
    for k in range(len(a) - 1, -1, -1):
        if a[k] > b[k]:
            return True
        if a[k] < b[k]:
            return False
    return False


def _insertion_sort(g):
    """the stable insertion sort itself, for rows that are not totally ordered (NaN)"""
    g = g.copy()
    for i in range(1, len(g)):
        row, pos = g[i].copy(), i
        while pos > 0 and _sorts_before(row, g[pos - 1]):
            g[pos] = g[pos - 1]
            pos -= 1
        g[pos] = row
    return g


def feature_sort(p):
    """jax/util.py:186-197: the rows in descending order, last coordinate primary, ties in row order"""
    b, m, d = p.shape
    # rank of row i: the rows that sort before it, and its equals above it
    before = np.zeros((b, m, m), bool)  # before[:, j, i]: row j sorts before row i
    tied = np.ones((b, m, m), bool)
    for k in range(d - 1, -1, -1):
        a, c = p[:, :, None, k], p[:, None, :, k]
        before |= tied & (a > c)
        tied &= a == c
    before |= tied & (np.arange(m)[:, None] < np.arange(m)[None, :])
    rank = before.sum(1)
    out = np.empty_like(p)
    np.put_along_axis(out, np.repeat(rank[..., None], d, -1), p, 1)
    for g in np.nonzero(np.isnan(p).any((1, 2)))[0]:
        out[g] = _insertion_sort(p[g])
    return out


def features(p, scale):
    """hk_get_features: [rescale,] the sort"""
    b, m, d = p.shape
    return feature_sort(rescale(p) if scale else p).reshape(b, m * d)


def expand(parents, action, m, d, *, reposition_points=False, scale_observation=True, discount=0.99):
    """one expansion of a batch: parents [B, m*d + d] float32, action [B] int.  Returns kind, next_state [B, m*d + d],
    net_in [B, m*d + d], subset [B] int32, reward [B], discount [B], prev_done, done"""
    parents = np.ascontiguousarray(parents, F)
    action = np.asarray(action, np.int64)
    b, n = len(parents), m * d
    points, tail = parents[:, :n].reshape(b, m, d), parents[:, n:]
    kind = batch_kind(parents, d)
    if kind:
        subset = subset_of(action, d)
        next_points, next_tail = points.copy(), bits_of(subset, d)
    else:
        axis = np.where((action >= 0) & (action < d), action, -1)
        subset = np.zeros(b, np.int64)
        next_points, next_tail = step_points(points, tail, axis, reposition_points), np.zeros((b, d), F)
    prev_done, done = count_points(points) < 2, count_points(next_points) < 2
    return dict(kind=kind,
                next_state=np.concatenate([next_points.reshape(b, n), next_tail], 1),
                net_in=np.concatenate([features(next_points, scale_observation), next_tail], 1),
                subset=subset.astype(np.int32),
                reward=F(-1) * (done & ~prev_done).astype(F),
                discount=np.full(b, -F(discount), F), prev_done=prev_done, done=done)


def prior(kind, agent_logits, agent_value, host_logits, host_value, subset, d):
    """hk_unified_prior: kind 1 the agent's logits behind its mask, padded with -inf, and its value; kind 0 the host's"""
    if not kind:
        return np.array(host_logits, F), np.array(host_value, F)
    b, k = len(agent_logits), min(d, num_actions(d))  # (d = 2 has one class: the reference's pad by -1 crops the logits)
    out = np.full((b, num_actions(d)), -np.inf, F)
    out[:, :k] = np.where(bits_of(subset, d, bool), agent_logits, F(-np.inf))[:, :k]
    return out, np.array(agent_value, F)
