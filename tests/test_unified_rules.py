"""tests/unified_rules.py, the numpy restatement of one expansion of the role-agnostic tree, pinned to the oracle's
composition: oracle.c_oracle.step with stages 7 (shift, reposition, Newton) or 5 (shift, Newton) in JAX semantics with
the tail as the float mask, oracle.np_oracle.decode_class, the oracle's get_features -- on every state of 3 rows over
{hole, 0..2}^d, d = 2, 3, with every class and every axis, those out of range included.  Bit patterns, no tolerances
(one NaN is as good as another; -0.0 and +0.0 stay apart).  No GPU is involved."""
import itertools

import numpy as np
import pytest

import unified_rules as U
from hironaka_amd import _abi as A
from oracle import c_oracle as CO
from oracle import np_oracle as NO

F = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    return np.where(np.isnan(a), np.array(np.nan, a.dtype), a).view(np.uint32)


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, "%s: %d differ, the first at %s: got %r, want %r" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def small_states(d):
    """every state of 3 rows, each a hole or coordinates in 0..2: (1 + 3^d)^3 of them, [count, 3, d] float32"""
    rows = np.array([[-1] * d] + list(itertools.product(range(3), repeat=d)), F)
    return rows[np.array(list(itertools.product(range(len(rows)), repeat=3)))]


def with_tail(points, tail):
    return np.concatenate([points.reshape(len(points), -1), np.asarray(tail, F)], 1)


def test_the_codec_and_its_clamp():
    for d in range(2, 6):
        ncls = U.num_actions(d)
        cls = np.arange(-3, ncls + 4)
        want = NO.decode_class(np.clip(cls, 0, ncls - 1), d)
        assert_bits(U.bits_of(U.subset_of(cls, d), d, np.int32), want, "decode d=%d" % d)
        inside = np.arange(ncls)  # (the oracle refuses an id outside; the device's decode_kernel clamps to the ends)
        assert_bits(U.bits_of(U.subset_of(inside, d), d, np.int32), CO.decode_host_class(inside, d), "the oracle d=%d" % d)
        assert (U.subset_of(cls[:3], d) == U.subset_of(0, d)).all() and (U.subset_of(cls[-4:], d) == (1 << d) - 1).all()
        assert (U.bits_of(U.subset_of(cls, d), d).sum(1) >= 2).all()


def test_host_state_is_isclose_to_zero():
    d = 3
    eps = np.float32(1e-8)
    tails = np.array([[0, 0, 0], [eps, -eps, 0], [-0.0, 0, 0], [2e-8, 0, 0], [0, 0, np.nan], [1, 1, 0],
                      [np.nextafter(eps, F(1)), 0, 0], [0, -2e-8, 0]], F)
    want = np.array([1, 1, 1, 0, 0, 0, 0, 0], bool)
    states = with_tail(np.ones((len(tails), 2, d), F), tails)
    assert (U.is_host_state(states, d) == want).all()
    with np.errstate(invalid="ignore"):
        assert (np.isclose(tails, F(0), rtol=0, atol=eps).all(1) == want).all()  # numpy's own isclose, in float
    assert U.batch_kind(states[3:], d) == 0 and U.batch_kind(states[2:], d) == 1 and U.batch_kind(states[:1], d) == 1


@pytest.mark.parametrize("repos", (False, True))
@pytest.mark.parametrize("d", (2, 3))
def test_agent_kind_is_the_oracle_step_on_every_small_state_class_and_axis(d, repos):
    """kind 0: the tail is the float mask, the action the axis; axes -1, d and d + 1 match nothing"""
    states = small_states(d)
    assert len(states) == {2: 1000, 3: 21952}[d]
    masks = U.masks_of(d)
    axes = np.arange(-1, d + 2)
    s, c, a = np.meshgrid(np.arange(len(states)), np.arange(len(masks)), axes, indexing="ij")
    p, tail, action = states[s.ravel()], U.bits_of(masks[c.ravel()], d), a.ravel()
    m = 3
    got = U.expand(with_tail(p, tail), action, m, d, reposition_points=repos, scale_observation=True)
    assert got["kind"] == 0  # no subset has fewer than 2 coordinates: no zero tail
    stages = A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON | (A.HK_STAGE_REPOSITION if repos else 0)
    assert stages == (7 if repos else 5)
    want = CO.step(p, tail, action.astype(np.int32), stages=stages, flags=A.HK_SEM_JAX, reward_sign=-1.0)
    n = m * d
    assert_bits(got["next_state"][:, :n], want["points"].reshape(len(p), n), "next points")
    assert_bits(got["next_state"][:, n:], np.zeros((len(p), d), F), "next tail")
    assert_bits(got["reward"], want["reward"], "reward")
    assert (got["done"] == want["done"]).all() and (got["prev_done"] == want["prev_done"]).all()
    assert_bits(got["net_in"][:, :n], CO.get_features(want["points"], scale_observation=True), "features")
    assert_bits(got["net_in"][:, n:], np.zeros((len(p), d), F), "the network's tail")
    assert (got["subset"] == 0).all() and got["subset"].dtype == np.int32
    assert_bits(got["discount"], np.full(len(p), -F(0.99), F), "discount")
    # reached, from the oracle alone: games that end on the move, ended games, rows Newton removes, axes off the subset
    assert (want["reward"] == -1).any() and want["prev_done"].any() and (~want["done"]).any()
    assert ((want["points"][:, :, 0] >= 0).sum(1) < (p[:, :, 0] >= 0).sum(1)).any()
    off = (action < 0) | (action >= d) | (tail[np.arange(len(p)), np.clip(action, 0, d - 1)] == 0)
    assert off.any() and (~off).any()
    assert np.signbit(want["reward"]).all()  # -1 * 0 is -0.0


@pytest.mark.parametrize("scale", (False, True))
@pytest.mark.parametrize("d", (2, 3))
def test_host_kind_keeps_the_points_and_decodes_the_class(d, scale):
    """kind 1 on every small state and every class id from -2 to two beyond the last: the points stay, the tail is the
    subset, the features are the oracle's of the same points"""
    states = small_states(d)
    ncls = U.num_actions(d)
    s, c = np.meshgrid(np.arange(len(states)), np.arange(-2, ncls + 2), indexing="ij")
    p, action = states[s.ravel()], c.ravel()
    m, n = 3, 3 * d
    got = U.expand(with_tail(p, np.zeros((len(p), d), F)), action, m, d, scale_observation=scale)
    assert got["kind"] == 1
    tail = NO.decode_class(np.clip(action, 0, ncls - 1), d).astype(F)
    assert_bits(got["next_state"], with_tail(p, tail), "next state")
    assert_bits(got["net_in"], np.concatenate([CO.get_features(p, scale_observation=scale), tail], 1), "network input")
    assert_bits(U.bits_of(got["subset"], d), tail, "subset")
    assert_bits(got["reward"], np.full(len(p), -0.0, F), "reward: nothing ends where nothing moves")
    assert (got["done"] == got["prev_done"]).all() and got["done"].any() and (~got["done"]).any()


def test_one_host_state_makes_the_batch_a_host_batch():
    """the decision is the batch's: an agent parent in a host-kind batch keeps its points and takes the class's subset"""
    d, m = 3, 3
    rng = np.random.default_rng(5)
    p = small_states(d)[rng.integers(0, 21952, 64)]
    tail = U.bits_of(U.masks_of(d)[rng.integers(0, 4, 64)], d)
    action = rng.integers(-1, 6, 64)
    agent = U.expand(with_tail(p, tail), action, m, d)
    assert agent["kind"] == 0
    for at in (0, 63):
        mixed_tail = tail.copy()
        mixed_tail[at] = 0
        got = U.expand(with_tail(p, mixed_tail), action, m, d)
        assert got["kind"] == 1
        want = U.expand(with_tail(p, np.zeros_like(tail)), action, m, d)  # as if every parent were a host state
        for name in ("next_state", "net_in", "subset", "reward"):
            assert_bits(got[name], want[name], name)
        assert (bits(got["next_state"]) != bits(agent["next_state"])).any()


def test_features_with_nan_follow_the_insertion_sort():
    """a NaN tail in an agent-kind batch reaches the points; the sort is then the kernel's insertion sort, as the oracle's"""
    d, m = 3, 5
    rng = np.random.default_rng(9)
    p = rng.integers(0, 4, (200, m, d)).astype(F)
    p[rng.random((200, m)) < 0.2] = -1
    tail = np.ones((200, d), F)
    tail[::2, 1] = np.nan
    action = rng.integers(0, d, 200)
    got = U.expand(with_tail(p, tail), action, m, d)
    want = CO.step(p, tail, action.astype(np.int32), stages=5, flags=A.HK_SEM_JAX, reward_sign=-1.0)
    assert np.isnan(want["points"]).any()
    assert_bits(got["next_state"][:, : m * d], want["points"].reshape(200, -1), "points")
    assert_bits(got["net_in"][:, : m * d], CO.get_features(want["points"], scale_observation=True), "features")


def test_prior_selects_masks_and_pads():
    d, b = 3, 7
    rng = np.random.default_rng(1)
    al, av = rng.standard_normal((b, d)).astype(F), rng.standard_normal(b).astype(F)
    hl, hv = rng.standard_normal((b, 4)).astype(F), rng.standard_normal(b).astype(F)
    subset = U.subset_of(rng.integers(0, 4, b), d).astype(np.int32)
    p1, v1 = U.prior(1, al, av, hl, hv, subset, d)
    mask = U.bits_of(subset, d, bool)
    assert p1.shape == (b, 4) and np.isneginf(p1[:, 3]).all() and np.isneginf(p1[:, :3][~mask]).all()
    assert_bits(p1[:, :3][mask], al[mask], "open logits")
    assert_bits(v1, av, "value")
    p0, v0 = U.prior(0, al, av, hl, hv, subset, d)
    assert_bits(p0, hl, "host logits")
    assert_bits(v0, hv, "host value")
