"""hk_search_morin_play on the GPU and the surfaces on top of it (ops.morin_play, HipPoints' tracked
get_newton_polytope, AgentMorin, GameMorin): the reference's own games replayed bit for bit
(tests/golden/morin_game.npz, made by tests/golden/make_morin_game_golden.py), the in-kernel hosts and agent against
the plain restatement tests/morin_rules.py, random ties, agreement with search_trees_morin, layouts."""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import morin_rules as M
import search_rules as R
from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import ops
from hironaka_amd._lib import HironakaHipError
from hironaka_amd.agent import AgentMorin
from hironaka_amd.core import HipPoints
from hironaka_amd.game import GameMorin
from hironaka_amd.host import RandomHost, WeakSpivakovsky, Zeillinger
from hironaka_amd.host_action_preprocess import batch_encode, encode_host_class
from hironaka_amd.util import search_trees_morin

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float64)
NP = {torch.float32: np.float32, torch.float64: np.float64}
HITTING = ("weak_spivakovsky", "weak_spivakovsky_min_hitting")


@lru_cache(maxsize=None)
def fixture_games():
    return M.load_games(np.load(os.path.join(GOLDEN, "morin_game.npz")))


def thom4_root():
    return next(g for g in fixture_games() if g.name == "thom4_weak_spivakovsky_s0").root


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else torch.as_tensor(
        np.ascontiguousarray(a), device="cuda").to(dtype)


def launch(roots, weights, dist, dtype, **kw):
    return ops.morin_play(dev(roots, dtype), dev(np.asarray(weights, np.int32)), dev(np.asarray(dist, np.int32)), **kw)


def pad_moves(rows, steps):
    return np.asarray([list(r[:steps]) + [-1] * (steps - len(r[:steps])) for r in rows], np.int32).reshape(len(rows), steps)


def check(res, roots, want, dtype, steps, label):
    """every output field of a launch against the restatement's games"""
    npd = NP[dtype]
    got = res.points.cpu().numpy()
    for b, (root, p) in enumerate(zip(roots, want)):
        assert got[b].tobytes() == M.final_state(root, p, npd).tobytes(), (label, b)
    assert res.weights.tolist() == [p.weights for p in want], label
    assert res.distinguished.tolist() == [p.dist for p in want], label
    assert res.length.tolist() == [p.length for p in want], label
    assert res.outcome.tolist() == [p.outcome for p in want], label
    if res.classes is not None:
        assert res.classes.cpu().numpy().tolist() == pad_moves([p.classes for p in want], steps).tolist(), label
        assert res.axes.cpu().numpy().tolist() == pad_moves([p.axes for p in want], steps).tolist(), label


# ---- 1. replay of the reference ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_replay_of_the_reference(dtype):
    """every fixture game with forced classes and axes, one launch per (m, d) and prefix length t: states, weights,
    distinguished, length and outcome after every move equal the reference's"""
    groups = {}
    for g in fixture_games():
        groups.setdefault(g.root.shape, []).append(g)
    assert len(groups) >= 12
    for (m, d), games in groups.items():
        roots = np.stack([g.root for g in games])
        dist = [g.dist for g in games]
        forced = [M.forced_moves(g) for g in games]
        longest = max(len(g.axes) for g in games)
        for t in range(longest + 1):
            res = launch(roots, np.ones((len(games), d)), dist, dtype, max_steps=t, reduce_root=True, record=True,
                         classes=dev(pad_moves([f[0] for f in forced], t)) if t else None,
                         axes=dev(pad_moves([f[1] for f in forced], t)) if t else None)
            pts, w, nd = res.points.cpu().numpy(), res.weights.tolist(), res.distinguished.tolist()
            length, outcome = res.length.tolist(), res.outcome.tolist()
            for b, g in enumerate(games):
                n = min(t, len(g.axes))
                state = g.states[n - 1] if n else g.root_state
                assert pts[b].tobytes() == M.padded(state, m, NP[dtype]).tobytes(), (g.name, t)
                assert w[b] == (g.weights[n - 1] if n else [1] * d), (g.name, t)
                assert nd[b] == (g.dists[n - 1] if n else g.root_dist), (g.name, t)
                assert length[b] == n, (g.name, t)
                if n == len(g.axes) and g.stopped:
                    want = {1: M.ENDED, 2: M.NO_CONTRIBUTION}[g.stopped]
                elif t > len(g.axes):  # the record breaks off (the host raised, or a cap): no class is forced and
                    want = M.NO_MOVE   # the launch has no host
                else:
                    want = M.RUNNING
                assert outcome[b] == want, (g.name, t)
                assert res.axes[b, :n].tolist() == g.axes[:n] if t else True, (g.name, t)


def test_replay_move_by_move_without_the_reduction():
    """a T = 1 loop that feeds every launch the previous one's outputs, the in-kernel host choosing: the Thom N = 4
    game under WeakSpivakovsky at dimension 7 with the reference's tie-breaks"""
    g = next(g for g in fixture_games() if g.name == "thom4_weak_spivakovsky_s1")
    _, axes = M.forced_moves(g)
    res = launch(g.root[None], [[1] * 7], [g.dist], torch.float32, max_steps=0, reduce_root=True)
    for t, a in enumerate(axes):
        res = ops.morin_play(res.points, res.weights, res.distinguished, host="weak_spivakovsky", max_steps=1,
                             axes=dev(np.asarray([[a]], np.int32)), record=True)
        assert res.classes.tolist() == [[R.class_id(g.lists[t], 7)]] and res.axes.tolist() == [[g.axes[t]]]
        assert res.points[0].cpu().numpy().tolist() == M.padded(g.states[t], 19).tolist()
        assert res.weights.tolist() == [g.weights[t]] and res.distinguished.tolist() == [g.dists[t]]
    assert res.outcome.tolist() == [{1: M.ENDED, 2: M.NO_CONTRIBUTION}[g.stopped]]
    again = ops.morin_play(res.points, res.weights, res.distinguished, host="weak_spivakovsky", max_steps=1)
    assert again.length.tolist() == [0] and torch.equal(again.points, res.points)  # a stopped game is copied through


# ---- 2. HipPoints tracking -----------------------------------------------------------------------------------------

DE_ROOT = [(7, 5, 3, 8), (8, 1, 8, 18), (8, 3, 17, 8), (11, 11, 1, 19), (11, 12, 18, 6), (16, 11, 5, 6)]


def _shift(points, coords, axis):
    mask = torch.zeros((1, 4), device="cuda")
    mask[0, coords] = 1
    points.shift(mask, torch.tensor([axis], device="cuda"))


@pytest.mark.parametrize("as_tensor", [False, True])
def test_distinguished_elements(as_tensor):
    """test/testPoints.py:152-172"""
    given = torch.tensor([2], dtype=torch.int32, device="cuda") if as_tensor else [2]
    points = HipPoints([[list(r) for r in DE_ROOT]], max_num_points=6, distinguished_points=given, semantics="list")
    index = lambda: int(points.distinguished_points[0]) if as_tensor else points.distinguished_points[0]  # noqa: E731
    copy = points.get_newton_polytope(inplace=False)
    assert (points.distinguished_points.tolist() if as_tensor else points.distinguished_points) == [2]
    assert tuple(copy.points[0][int(copy.distinguished_points[0])].tolist()) == (8, 3, 17, 8)
    points.get_newton_polytope()
    assert torch.equal(copy.points, points.points)
    assert tuple(points.points[0][index()].tolist()) == (8, 3, 17, 8)
    _shift(points, [0, 1], 0)
    points.get_newton_polytope()
    assert tuple(points.points[0][index()].tolist()) == (11, 3, 17, 8)
    _shift(points, [0, 2], 0)
    _shift(points, [2, 3], 2)
    _shift(points, [0, 1], 1)
    probe = points.copy()
    probe.reposition().rescale()  # these do not reorder rows and leave the index alone
    assert (probe.distinguished_points.tolist() if as_tensor else probe.distinguished_points) == [index()]
    points.get_newton_polytope()
    assert (index() == -1) if as_tensor else (index() is None)
    if as_tensor:
        assert points.distinguished_points.dtype == torch.int32 and points.distinguished_points.is_cuda


def test_untracked_containers_are_unchanged():
    rng = np.random.default_rng(5)
    raw = rng.integers(0, 9, (33, 7, 3)).astype(np.float32)
    for sem in ("list", "torch"):
        plain = HipPoints(raw.copy(), semantics=sem)
        want = ops.get_newton_polytope(dev(raw), sem=sem)
        assert plain.get_newton_polytope() is plain and plain.distinguished_points is None
        assert torch.equal(plain.points, want)
    marked = HipPoints(raw.copy(), semantics="torch", distinguished_points=[0] * 33)
    marked.get_newton_polytope()
    assert marked.distinguished_points == [0] * 33
    assert torch.equal(marked.points, ops.get_newton_polytope(dev(raw), sem="torch"))
    # list semantics with marks: the same states as without, indices as the restatement's
    listed = HipPoints(raw.copy(), semantics="list", distinguished_points=[b % 7 for b in range(33)])
    listed.get_newton_polytope()
    assert torch.equal(listed.points, ops.get_newton_polytope(dev(raw), sem="list"))
    want = [M.tracked_newton(raw[b].astype(np.int64), b % 7)[1] for b in range(33)]
    assert listed.distinguished_points == [None if v < 0 else v for v in want]
    assert None in listed.distinguished_points and any(v is not None for v in listed.distinguished_points)


def test_containers_beyond_the_tracked_sizes_are_reduced_as_before():
    """m > 64 or d > 7: no tracking there; the container is reduced as one without marks, with a warning"""
    rng = np.random.default_rng(6)
    for m, d in ((65, 3), (5, 8)):
        raw = rng.integers(0, 9, (3, m, d)).astype(np.float32)
        marked = HipPoints(raw.copy(), semantics="list", distinguished_points=[0, 1, 2])
        with pytest.warns(UserWarning, match="distinguished_points are tracked"):
            assert marked.get_newton_polytope() is marked
        assert marked.distinguished_points == [0, 1, 2]
        assert torch.equal(marked.points, ops.get_newton_polytope(dev(raw), sem="list"))
        with pytest.warns(UserWarning):
            copy = marked.get_newton_polytope(inplace=False)
        assert torch.equal(copy.points, marked.points)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_tracking_keeps_the_padding_value(dtype):
    rng = np.random.default_rng(7)
    raw = rng.integers(0, 9, (33, 7, 3)).astype(np.float32)
    raw[::3, 4:] = -2.0
    marks = [b % 4 for b in range(33)]
    plain = HipPoints(raw.copy(), semantics="list", padding_value=-2.0, dtype=dtype)
    plain.get_newton_polytope()
    assert bool((plain.points == -2).any()) and not bool((plain.points == -1).any())
    marked = HipPoints(raw.copy(), semantics="list", padding_value=-2.0, distinguished_points=list(marks), dtype=dtype)
    copy = marked.get_newton_polytope(inplace=False)
    assert marked.distinguished_points == marks and torch.equal(marked.points, dev(raw, dtype))
    marked.get_newton_polytope()
    assert marked.points.dtype == dtype
    assert torch.equal(marked.points, plain.points) and torch.equal(copy.points, plain.points)
    want = [M.tracked_newton(np.where(raw[b] < 0, -1, raw[b]).astype(np.int64), marks[b])[1] for b in range(33)]
    assert marked.distinguished_points == copy.distinguished_points == [None if v < 0 else v for v in want]


def test_encode_host_class_is_batch_encode_with_no_move():
    masks = ops.decode_host_class(torch.arange(2 ** 7 - 8, dtype=torch.int32, device="cuda"), 7, torch.int32)
    assert encode_host_class(masks).tolist() == batch_encode(masks).tolist() == list(range(2 ** 7 - 8))
    assert encode_host_class(masks.float() * 3).tolist() == list(range(2 ** 7 - 8))
    few = torch.tensor([[0, 0, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0], [1, 0, 0, 1]], device="cuda")
    assert encode_host_class(few).tolist() == [-1, -1, -1, batch_encode(few[3:]).tolist()[0]]
    assert encode_host_class(few).dtype == torch.int32


# ---- 3. in-kernel hosts and agent against the restatement ------------------------------------------------------------

STEPS = 6
SHAPES = [(2, 2), (20, 3), (19, 7), (64, 6)]
CASES = [(m, d, h) for m, d in SHAPES for h in R.HOSTS] + [(64, 7, h) for h in HITTING]


def games_per_wave(m, d, dtype):
    """the kernel's launch shape: a slice holds parent, child, 2 d scratch and 2 d for weights and the saved row"""
    stride = (2 * m * d + 4 * d) | 1
    return min(64, 65536 // (stride * (4 if dtype == torch.float32 else 8)))


@lru_cache(maxsize=None)
def seeded_roots(m, d, count):
    """full, padded and already-ended games and games with a hole, with and without a distinguished row"""
    rng = np.random.default_rng(1000 * m + d)
    roots = np.full((count, m, d), -1, np.int64)
    dist, weights = [], []
    for b in range(count):
        n = m if b % 3 == 0 else int(rng.integers(1, m + 1))
        if b % 11 == 10:
            n = 1
        high = int(rng.choice([3, 50, 3000, 100000] if m == 2 else [3, 6, 12, 40]))  # two points play Euclid's game
        roots[b, :n] = rng.integers(0, high, (n, d))
        rows = list(range(n))
        if n >= 3 and b % 7 == 3:  # a hole before the last point
            roots[b, n - 2] = -1
            rows.remove(n - 2)
        lightest = min(rows, key=lambda i: int(roots[b, i].sum()))
        dist.append(-1 if b % 9 == 4 else lightest if b % 4 else int(rng.choice(rows)))
        weights.append(rng.integers(0, 4, d).tolist() if b % 2 else [1] * d)
    if (m, d) == (19, 7):
        roots[0], dist[0], weights[0] = thom4_root(), 18, [1] * 7
    return roots, dist, weights


@lru_cache(maxsize=None)
def expected(m, d, host, tie, rule):
    count = 3 * games_per_wave(m, d, torch.float32) + 1
    roots, dist, weights = seeded_roots(m, d, count)
    return [M.play(roots[b], weights[b], dist[b], host, STEPS, tie=tie, weight_rule=rule, reduce_root=True)
            for b in range(count)]


@pytest.mark.parametrize("m,d,host", CASES)
def test_hosts_and_agent_against_the_restatement(m, d, host):
    for tie in ("lowest", "highest"):
        for rule in ("agent", "search"):
            want = expected(m, d, host, tie, rule)
            outcomes = {p.outcome for p in want}
            assert {M.ENDED, M.NO_CONTRIBUTION, M.RUNNING} <= outcomes, (tie, rule, outcomes)
            assert max(p.length for p in want) > 3 and any(p.length == 0 for p in want)
            assert any(p.dist < 0 and p.outcome == M.RUNNING for p in want) or d == 2  # an untracked game goes on
            for dtype in DTYPES:
                count = 3 * games_per_wave(m, d, dtype) + 1  # three workgroups and a partial fourth
                roots, dist, weights = (v[:count] for v in seeded_roots(m, d, len(want)))
                res = launch(roots, weights, dist, dtype, host=host, max_steps=STEPS, tie=tie, weight_rule=rule,
                             reduce_root=True, record=True)
                check(res, roots, want[:count], dtype, STEPS, (m, d, host, tie, rule, dtype))


def test_forced_moves_stop_where_they_are_not_legal():
    roots = np.asarray([[[2, 0, 1], [0, 2, 1], [-1, -1, -1]]] * 4)
    classes = np.asarray([[0, 3], [4, 0], [3, -1], [-1, -1]], np.int32)  # class 4 does not exist at dimension 3
    axes = np.asarray([[2, 0], [0, 0], [-1, -1], [-1, -1]], np.int32)   # axis 2 is outside class 0 = {0, 1}
    res = launch(roots, np.ones((4, 3)), [0] * 4, torch.float32, max_steps=2, classes=dev(classes), axes=dev(axes),
                 record=True)
    want = [M.play(roots[b], [1] * 3, 0, None, 2, classes=classes[b], axes=axes[b]) for b in range(4)]
    assert [p.outcome for p in want[:2]] == [M.NO_MOVE] * 2 and want[3].outcome == M.NO_MOVE and want[2].length >= 1
    check(res, roots, want, torch.float32, 2, "forced")


def test_inexact_stops_the_game():
    roots = np.asarray([[[2 ** 23, 2 ** 23], [0, 2 ** 24 - 1]], [[3, 0], [0, 3]]])
    res = launch(roots, np.ones((2, 2)), [0, 0], torch.float32, host="zeillinger", max_steps=3)
    assert res.outcome.tolist() == [A.HK_MORIN_INEXACT, M.play(roots[1], [1, 1], 0, "zeillinger", 3).outcome]
    assert res.length.tolist()[0] == 1
    res = launch(roots, np.ones((2, 2)), [0, 0], torch.float64, host="zeillinger", max_steps=3)
    assert res.outcome.tolist()[0] == M.play(roots[0], [1, 1], 0, "zeillinger", 3).outcome != A.HK_MORIN_INEXACT


def test_wrapper_refuses_what_the_c_entry_cannot_see():
    """ops.morin_play's checks of device data and of the arguments that go with it"""
    roots, dist, weights = (v[:5] for v in seeded_roots(9, 3, 5))
    pts, w, nd = dev(roots, torch.float32), dev(np.asarray(weights, np.int32)), dev(np.asarray(dist, np.int32))
    nd = nd.clamp(min=0)
    kw = dict(host="zeillinger", max_steps=2)
    assert ops.morin_play(pts, w, nd, **kw).length.shape == (5,)

    def changed(t, index, value):
        t = t.clone()
        t[index] = value
        return t

    moves = torch.full((5, 2), -1, dtype=torch.int64, device="cuda")
    for bad in (dict(weights=changed(w, (3, 1), -1)),                       # a negative weight under the agent's rule
                dict(weights=changed(w.to(torch.int64), (0, 0), 2 ** 31)),
                dict(weights=changed(w.to(torch.int64), (0, 0), -2 ** 31 - 1), weight_rule="search"),
                dict(distinguished=changed(nd, 4, 9)),                      # = m
                dict(distinguished=changed(nd, 0, -2)),
                dict(classes=changed(moves, (2, 1), 2 ** 31)),
                dict(axes=changed(moves, (2, 1), -2 ** 31 - 1)),
                dict(weights=w[:, :2]), dict(weights=w[:4]), dict(weights=w.float()),   # shape and dtype
                dict(distinguished=nd[:4]), dict(distinguished=nd.unsqueeze(1)),
                dict(classes=moves[:, :1]), dict(axes=moves[:4]),
                dict(host=None),                                            # no host and no classes
                dict(host="spivakovsky"), dict(tie="middle"), dict(weight_rule="tree"),
                dict(out=torch.empty((5, 9, 4), device="cuda")), dict(out=torch.empty((5, 9, 3), device="cuda").double()),
                dict(points=pts[0])):
        args = {"points": pts, "weights": w, "distinguished": nd, **kw, **bad}
        with pytest.raises(ValueError):
            ops.morin_play(args.pop("points"), args.pop("weights"), args.pop("distinguished"), **args)
    for bad in (dict(points=pts.half()), dict(out=torch.empty((5, 9, 3))), dict(weights=w.cpu())):
        args = {"points": pts, "weights": w, "distinguished": nd, **kw, **bad}
        with pytest.raises(TypeError):
            ops.morin_play(args.pop("points"), args.pop("weights"), args.pop("distinguished"), **args)
    # what validate=False skips is the range check alone, and the kernel reads an index that addresses no point as -1
    loose = ops.morin_play(pts, w, changed(nd, 4, 9), validate=False, **kw)
    assert loose.outcome.tolist()[4] == A.HK_MORIN_NO_CONTRIBUTION and loose.length.tolist()[4] == 0
    # host=None with classes is served, and with max_steps=0 needs neither
    assert ops.morin_play(pts, w, nd, max_steps=0).length.tolist() == [0] * 5
    with pytest.raises(HironakaHipError) as refused:  # a status of the C entry is raised
        ops.morin_play(pts[:, :0], w, nd, validate=False, **kw)
    assert refused.value.status == A.HK_ERR_SHAPE


def test_search_rule_continues_with_the_negative_weights_it_leaves():
    """w[i] -= w[axis] goes below zero where a third coordinate of the subset is lighter than the axis; a second launch
    takes those weights back under the same rule"""
    roots, dist, _ = (v[:40] for v in seeded_roots(12, 5, 40))
    weights = [[2, 3, 1, 1, 2]] * 40
    kw = dict(host="all_coord", tie="lowest", weight_rule="search")
    want = [M.play(roots[b], weights[b], dist[b], "all_coord", 5, tie="lowest", weight_rule="search", reduce_root=True)
            for b in range(40)]
    assert any(p.length >= 3 for p in want)
    whole = launch(roots, weights, dist, torch.float32, max_steps=5, reduce_root=True, record=True, **kw)
    check(whole, roots, want, torch.float32, 5, "search")
    head = launch(roots, weights, dist, torch.float32, max_steps=1, reduce_root=True, record=True, **kw)
    going = head.outcome == A.HK_MORIN_RUNNING
    assert bool((head.weights[going] < 0).any())
    with pytest.raises(ValueError):
        ops.morin_play(head.points, head.weights, head.distinguished, max_steps=4, host="all_coord")
    tail = ops.morin_play(head.points, head.weights, torch.where(going, head.distinguished, -1), max_steps=4,
                          record=True, **kw)
    # (a game the first launch played untracked stays "running" with -1: the tail stops it, as it should a lost one)
    tracked = going & (head.distinguished >= 0)
    assert int(tracked.sum()) >= 5
    for field in ("points", "weights", "distinguished", "outcome"):
        assert torch.equal(getattr(tail, field)[tracked], getattr(whole, field)[tracked]), field
    assert torch.equal(torch.cat([head.axes, tail.axes], 1)[tracked], whole.axes[tracked])


# ---- 4. random ties ------------------------------------------------------------------------------------------------

def test_random_ties():
    rng = np.random.default_rng(11)
    b, m, d, steps = 256, 8, 4, 8
    roots = rng.integers(0, 9, (b, m, d))
    dist = [int(roots[i].sum(1).argmin()) for i in range(b)]
    run = lambda seed, lo=0, hi=b, off=0: launch(roots[lo:hi], np.ones((hi - lo, d)), dist[lo:hi], torch.float32,  # noqa: E731
                                                 host="all_coord", max_steps=steps, tie="random", seed=seed,
                                                 game_offset=off, reduce_root=True, record=True)
    res = run(7)
    classes, axes = res.classes.tolist(), res.axes.tolist()
    playing = [i for i in range(b) if res.length[i] > 0]
    assert len(playing) > b // 2
    for i in range(b):
        n = int(res.length[i])
        p = M.play(roots[i], [1] * d, dist[i], "all_coord", steps, axes=axes[i][:n], tie="random", reduce_root=True)
        assert (p.length, p.outcome, p.classes, p.weights, p.dist) == (
            n, int(res.outcome[i]), classes[i][:n], res.weights[i].tolist(), int(res.distinguished[i])), i
        assert res.points[i].cpu().numpy().tolist() == M.final_state(roots[i], p).tolist(), i
        w = [1] * d
        for t in range(n):  # every axis is legal under the rule: the lighter of the two lowest, anything at a tie
            rule = M.morin_axis(list(range(d)), w, "random")
            assert axes[i][t] in range(d) and rule in (None, axes[i][t]), (i, t)
            w = M.next_weights(list(range(d)), w, axes[i][t], "agent")
    first = {axes[i][0] for i in playing}  # weights all 1: every game ties at move 0
    assert {0, 1} <= first and first <= set(range(d))
    same = run(7)
    assert all(torch.equal(x, y) for x, y in zip(res, same))
    other = run(8)
    assert not torch.equal(other.axes, res.axes)
    halves = [run(7, 0, b // 2), run(7, b // 2, b, b // 2)]
    for k, field in enumerate(res._fields):
        assert torch.equal(torch.cat([h[k] for h in halves]), res[k]), field
    # two launches that continue the games with step_offset reproduce the one launch
    head = launch(roots, np.ones((b, d)), dist, torch.float32, host="all_coord", max_steps=3, tie="random", seed=7,
                  reduce_root=True, record=True)
    tail = ops.morin_play(head.points, head.weights, torch.where(head.outcome == 0, head.distinguished, -1),
                          host="all_coord", max_steps=steps - 3, tie="random", seed=7, step_offset=3, record=True)
    going = head.outcome == 0
    assert torch.equal(tail.points[going], res.points[going]) and torch.equal(tail.weights[going], res.weights[going])
    assert torch.equal(torch.cat([head.axes, tail.axes], 1)[going], res.axes[going])


# ---- 5. agreement with the tree ------------------------------------------------------------------------------------

def test_played_games_are_paths_of_the_morin_tree():
    rng = np.random.default_rng(3)
    b, m, d, steps = 6, 6, 4, 32
    roots = rng.integers(0, 7, (b, m, d))
    weights = rng.integers(1, 4, (b, d))
    dist = [int(roots[i].sum(1).argmin()) for i in range(b)]
    # the tree's roots are used as given: reduce them first, as Game.__init__ does
    start = launch(roots, weights, dist, torch.float64, max_steps=0, reduce_root=True)
    assert (start.distinguished >= 0).all()
    tree = search_trees_morin(start.points, start.weights, start.distinguished, Zeillinger())
    assert (tree.status == 0).all()
    for tie in ("lowest", "highest"):
        res = ops.morin_play(start.points, start.weights, start.distinguished, host="zeillinger", max_steps=steps,
                             tie=tie, weight_rule="search", record=True)
        assert (res.outcome != A.HK_MORIN_RUNNING).all() and int(res.length.max()) >= 2
        parent, axis = tree.parent.tolist(), tree.axis.tolist()
        for i in range(b):
            node = 0
            for t in range(int(res.length[i])):
                below = [j for j in range(int(tree.count[i])) if parent[i][j] == node and axis[i][j] == res.axes[i, t]]
                assert len(below) == 1, (i, t)  # the agent's axis is never one the search prunes
                node = below[0]
            assert torch.equal(tree.states[i, node], res.points[i]) and torch.equal(tree.weights[i, node], res.weights[i])
            assert int(tree.distinguished[i, node]) == int(res.distinguished[i])
            assert int(tree.kind[i, node]) == int(res.outcome[i] == A.HK_MORIN_NO_CONTRIBUTION)
            assert not any(p == node for p in parent[i][: int(tree.count[i])])  # a leaf


# ---- 6. layouts ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_layouts(dtype):
    b, m, d = 70, 9, 3
    roots, dist, weights = seeded_roots(m, d, b)
    kw = dict(host="weak_spivakovsky", max_steps=4, reduce_root=True, record=True)
    base = launch(roots, weights, dist, dtype, **kw)
    w, nd = dev(np.asarray(weights, np.int32)), dev(np.asarray(dist, np.int32))

    def views():
        flat = torch.full((5 + b * m * d,), 7.0, dtype=dtype, device="cuda")
        offset = flat[5:].view(b, m, d)
        record = torch.full((b, m * d + 5), 7.0, dtype=dtype, device="cuda")
        transposed = torch.empty((m, b, d), dtype=dtype, device="cuda").transpose(0, 1)
        for name, v, whole in (("offset", offset, flat), ("record", record[:, : m * d].view(b, m, d), record),
                               ("transposed", transposed, transposed)):
            v.copy_(dev(roots, dtype))
            yield name, v, whole

    for name, v, whole in views():
        assert name != "transposed" or not v.is_contiguous()
        keep = v.clone()
        res = ops.morin_play(v, w, nd, **kw)
        assert torch.equal(v, keep), name  # out of place leaves the input alone
        assert all(torch.equal(x, y) for x, y in zip(res, base)), name
    for name, v, whole in views():
        res = ops.morin_play(v, w, nd, out=v, **kw)
        assert res.points is v and torch.equal(v, base.points), name
        assert all(torch.equal(x, y) for x, y in zip(res[1:], base[1:])), name
        if name == "offset":
            assert (whole[:5] == 7).all()
        if name == "record":
            assert (whole[:, m * d:] == 7).all()
    for name, v, whole in views():  # into another layout
        out = torch.zeros((b, d, m), dtype=dtype, device="cuda").transpose(1, 2)
        assert ops.morin_play(v, w, nd, out=out, **kw).points is out and torch.equal(out, base.points), name
    # an out that shares memory with the points other than in place: games shifted by one, by a row, and the records
    # of one buffer read at one stride and written at another
    buf = torch.full(((b + 1) * m * d + d,), 7.0, dtype=dtype, device="cuda")
    for lo_in, lo_out in ((0, m * d), (m * d, 0), (0, d), (d, 0)):
        src, out = (buf[lo:lo + b * m * d].view(b, m, d) for lo in (lo_in, lo_out))
        src.copy_(dev(roots, dtype))
        assert ops.morin_play(src, w, nd, out=out, **kw).points is out and torch.equal(out, base.points), (lo_in, lo_out)
    wide = torch.full((b, 2 * m * d), 7.0, dtype=dtype, device="cuda")
    src, out = wide[:, : m * d].view(b, m, d), wide.view(-1)[: b * m * d].view(b, m, d)
    src.copy_(dev(roots, dtype))
    assert ops.morin_play(src, w, nd, out=out, **kw).points is out and torch.equal(out, base.points)


# ---- 7. surfaces ---------------------------------------------------------------------------------------------------

def _thom_game(tie="lowest", host=None, dtype=torch.float32):
    root = thom4_root()
    state = HipPoints([root.tolist()], max_num_points=19, distinguished_points=[18], semantics="list", dtype=dtype)
    return GameMorin(state, host or WeakSpivakovsky(), AgentMorin(tie=tie), scale_observation=False)


def test_game_morin_on_the_thom_root():
    """test/testThom.py:15-76 with the tie broken towards the lowest coordinate"""
    want = M.play(thom4_root(), [1] * 7, 18, "weak_spivakovsky", 100, tie="lowest", reduce_root=True)
    assert want.outcome in (M.ENDED, M.NO_CONTRIBUTION) and 0 < want.length < 100
    game = _thom_game()
    assert game.weights.tolist() == [[1] * 7] and not game.stopped
    for i in range(100):
        game.step()
        if game.stopped:
            break
    assert game.stopped and len(game.move_history) == want.length == i + 1
    assert [int(a[0]) for a in game.move_history] == want.axes
    assert [encode_host_class(c).tolist() for c in game.coord_history] == [[c] for c in want.classes]
    assert game.weights.tolist() == [want.weights] and game.outcome.tolist() == [want.outcome]
    assert game.state.points[0].cpu().numpy().tolist() == M.padded(want.state, 19).tolist()
    assert game.state.distinguished_points == [None if want.dist < 0 else want.dist]
    assert game.no_contribution.tolist() == [want.outcome == M.NO_CONTRIBUTION]
    assert game.step() is False and len(game.move_history) == want.length
    fused = _thom_game()
    assert fused.play(100) is False
    assert torch.equal(fused.state.points, game.state.points) and torch.equal(fused.weights, game.weights)
    assert len(fused.move_history) == len(game.move_history)
    assert all(torch.equal(x, y) for x, y in zip(fused.move_history + fused.coord_history,
                                                 game.move_history + game.coord_history))
    assert torch.equal(fused.outcome, game.outcome)


def test_game_morin_without_a_state_has_stopped():
    game = GameMorin(None, WeakSpivakovsky(), AgentMorin(tie="lowest"))
    assert game.stopped and game.step() is False and game.play(5) is False and game.weights is None
    with pytest.raises(TypeError):
        GameMorin(None, RandomHost(seed=1), AgentMorin()).play(5)


def test_game_morin_batch_keeps_stopped_games_untouched():
    b, m, d = 40, 12, 5
    roots, _, _ = seeded_roots(m, d, b)
    roots = roots.copy()
    roots[roots[:, :, 0] < 0] = -1
    dist = [int(np.where(r[:, 0] >= 0, r.sum(1), 10 ** 6).argmin()) for r in roots]
    want = [M.play(roots[i], [1] * d, dist[i], "weak_spivakovsky_min_hitting", 50, tie="highest", reduce_root=True)
            for i in range(b)]
    lengths = sorted({p.length for p in want})
    assert len(lengths) >= 3 and lengths[0] == 0  # games stop at different moves
    state = HipPoints(roots.astype(np.float32), distinguished_points=dev(np.asarray(dist, np.int32)), semantics="list")
    from hironaka_amd.host import WeakSpivakovskyMinHitting
    game = GameMorin(state, WeakSpivakovskyMinHitting(), AgentMorin(tie="highest"), scale_observation=False)
    seen = []
    for _ in range(50):  # one game of this batch never stops: the restatement's 50 moves are the cap here too
        going = game.step()
        seen.append((game.state.points.clone(), game.weights.clone(), game.stopped_batch.clone()))
        if not going:
            break
    assert M.RUNNING in {p.outcome for p in want} and bool(seen[0][2].any()) and not game.stopped
    assert len(game.move_history) == lengths[-1]
    for (p0, w0, s0), (p1, w1, _) in zip(seen, seen[1:]):
        assert torch.equal(p0[s0], p1[s0]) and torch.equal(w0[s0], w1[s0])
    assert game.outcome.tolist() == [p.outcome for p in want]
    assert game.weights.tolist() == [p.weights for p in want]
    assert game.state.distinguished_points.tolist() == [p.dist for p in want]
    assert game.state.points.cpu().numpy().tolist() == [M.padded(p.state, m).tolist() for p in want]
    assert torch.stack(game.move_history, 1).tolist() == pad_moves([p.axes for p in want], lengths[-1]).tolist()


def test_game_morin_with_a_forced_host():
    b, m, d = 32, 6, 4
    roots, _, _ = seeded_roots(m, d, b)
    dist = [int(np.where(r[:, 0] >= 0, r.sum(1), 10 ** 6).argmin()) for r in roots]
    state = HipPoints(roots.astype(np.float32), distinguished_points=list(dist), semantics="list")
    game = GameMorin(state, RandomHost(seed=3), AgentMorin(tie="random", seed=5), scale_observation=False)
    start = game.state.points.cpu().numpy().astype(np.int64)
    start_dist = [-1 if v is None else v for v in game.state.distinguished_points]
    for _ in range(200):
        if not game.step():
            break
    assert game.stopped and len(game.move_history) >= 2
    with pytest.raises(TypeError):
        game.play(5)
    masks, moves = torch.stack(game.coord_history, 1).tolist(), torch.stack(game.move_history, 1).tolist()
    for i in range(b):
        n = sum(a >= 0 for a in moves[i])
        assert all(a < 0 for a in moves[i][n:]) and all(sum(c) == 0 for c in masks[i][n:])
        assert all(sum(c) == 2 and c[a] == 1 for c, a in zip(masks[i][:n], moves[i][:n])), i  # every move is legal
        classes = [R.class_id([k for k in range(d) if c[k]], d) for c in masks[i][:n]]
        p = M.play(start[i], [1] * d, start_dist[i], None, n, classes=classes, axes=moves[i][:n])
        assert p.length == n and p.outcome == int(game.outcome[i]) and p.weights == game.weights[i].tolist(), i
        assert game.state.points[i].cpu().numpy().tolist() == M.final_state(start[i], p).tolist(), i
