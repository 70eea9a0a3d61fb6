"""hk_game_play / ops.game_play on the GPU: replay of the reference's recorded GameHironaka games, in-kernel hosts and
agents against the plain restatement tests/play_rules.py, roots as given, every outcome code, the random agent, layouts,
and the surfaces built on it (RandomAgent.play / ChooseFirstAgent.play, GameHironaka.play, HironakaValidator)."""
import os
from functools import lru_cache

import numpy as np
import pytest
import torch

import play_rules as P
import search_rules as R
from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import ops
from hironaka_amd._lib import HironakaHipError
from hironaka_amd.agent import ChooseFirstAgent, RandomAgent
from hironaka_amd.core import HipPoints
from hironaka_amd.game import GameHironaka
from hironaka_amd.host import (AllCoordHost, WeakSpivakovsky, WeakSpivakovskyMinHitting, Zeillinger, ZeillingerLex)
from hironaka_amd.validator import HironakaValidator

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float64)
NP = {torch.float32: np.float32, torch.float64: np.float64}
HOST_TYPES = {"zeillinger": Zeillinger, "all_coord": AllCoordHost, "zeillinger_lex": ZeillingerLex,
              "weak_spivakovsky": WeakSpivakovsky, "weak_spivakovsky_min_hitting": WeakSpivakovskyMinHitting}


@lru_cache(maxsize=None)
def fixture():
    npz = np.load(os.path.join(GOLDEN, "play_game.npz"))
    return P.load_games(npz), P.load_playoffs(npz)


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    return t if dtype is None else t.to(dtype)


def launch(roots, dtype, **kw):
    return ops.game_play(dev(roots, dtype), **kw)


def pad_moves(rows, steps):
    return np.asarray([list(r[:steps]) + [-1] * (steps - len(r[:steps])) for r in rows], np.int32).reshape(len(rows), steps)


def check(res, want, dtype, steps, label):
    """every output field of a launch against the restatement's games (run in the launch's dtype)"""
    got = res.points.cpu().numpy()
    assert got.dtype == NP[dtype]
    for b, p in enumerate(want):
        assert p.state.dtype == got.dtype and np.array_equal(got[b], p.state), (label, b, got[b], p.state)
    assert res.length.tolist() == [p.length for p in want], label
    assert res.outcome.tolist() == [p.outcome for p in want], label
    if res.classes is not None:
        assert res.classes.cpu().numpy().tolist() == pad_moves([p.classes for p in want], steps).tolist(), label
        assert res.axes.cpu().numpy().tolist() == pad_moves([p.axes for p in want], steps).tolist(), label


# ---- 1. replay of the reference ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,scale", [(torch.float64, True), (torch.float64, False), (torch.float32, False)])
def test_replay_of_the_reference(dtype, scale):
    """every recorded game of the reference, hosts in the kernel: with every axis forced, and with the in-kernel
    ChooseFirst agent where the reference played that agent.  A game is stopped behind its last recorded move by a
    forced class that does not exist, which leaves it untouched."""
    games = [g for g in fixture()[0] if g.scale == scale]
    groups = {}
    for g in games:
        groups.setdefault((g.root.shape[1], g.host), []).append(g)
    assert len(groups) == 30
    for (d, host), group in groups.items():
        m = max(len(g.root) for g in group)
        steps = max(len(g.axes) for g in group) + 1
        roots = np.stack([P.padded(g.root, m) for g in group])
        stop = np.full((len(group), steps), -1, np.int32)
        for b, g in enumerate(group):
            stop[b, len(g.axes)] = (1 << d) - d - 1
        for own_agent in (False, True):
            axes = pad_moves([[] if own_agent and g.agent == "choose_first" else g.axes for g in group], steps)
            res = launch(roots, dtype, host=host, agent="choose_first", max_steps=steps, classes=dev(stop),
                         axes=dev(axes), rescale=scale, reduce_root=True, rescale_root=scale, record=True)
            got = res.points.cpu().numpy()
            for b, g in enumerate(group):
                label = (g.name, own_agent)
                n = len(g.axes)
                last = g.states[-1] if n else g.root_state
                assert int(res.length[b]) == n, label
                assert res.axes[b, :n].tolist() == g.axes and (res.axes[b, n:] == -1).all(), label
                assert res.classes[b, :n].tolist() == [R.class_id(c, d) for c in g.lists], label
                assert np.array_equal(got[b], P.padded(last.astype(NP[dtype]), m)), label
                if not g.raised:
                    assert int(res.outcome[b]) == (A.HK_PLAY_ENDED if g.stopped else A.HK_PLAY_NO_MOVE), label


def test_replay_move_by_move_continues_a_game():
    """one launch per move on the states the launch before left (scaled, float64) equals the recorded game"""
    g = next(g for g in fixture()[0] if g.scale and g.agent == "random" and g.host == "zeillinger" and len(g.axes) >= 5)
    pts = launch(g.root[None], torch.float64, host=g.host, max_steps=0, reduce_root=True, rescale_root=True).points
    for t, a in enumerate(g.axes):
        res = ops.game_play(pts, host=g.host, max_steps=1, axes=dev(np.asarray([[a]], np.int32)), rescale=True, out=pts)
        assert res.points is pts and res.length.tolist() == [1]
        assert np.array_equal(P.points_of(pts[0].cpu().numpy()), g.states[t]), t


# ---- 2. in-kernel hosts and agents against the restatement -----------------------------------------------------------

STEPS = 5
SHAPES = [(2, 2), (20, 3), (19, 7), (64, 6), (64, 7)]
CONFIGS = [(False, False), (True, False), (False, True)]  # (reposition, rescale)


def games_per_wave(m, d, dtype):
    """the kernel's launch shape: a slice holds parent, child and 2 d elements of scratch"""
    stride = (2 * m * d + 2 * d) | 1
    return min(64, 65536 // (stride * (4 if dtype == torch.float32 else 8)))


@lru_cache(maxsize=None)
def seeded_roots(m, d, count):
    """full, padded and already-ended games and games with a hole"""
    rng = np.random.default_rng(2000 * m + d)
    roots = np.full((count, m, d), -1, np.int64)
    for b in range(count):
        n = m if b % 3 == 0 else int(rng.integers(1, m + 1))
        if b % 11 == 10:
            n = 1
        high = int(rng.choice([3, 50, 3000, 100000] if m == 2 else [3, 6, 12, 40]))  # two points play Euclid's game
        roots[b, :n] = rng.integers(0, high, (n, d))
        if n >= 3 and b % 7 == 3:  # a hole before the last point
            roots[b, n - 2] = -1
    return roots


@lru_cache(maxsize=None)
def expected(m, d, host, agent, reposition, rescaled, dtype):
    count = 3 * games_per_wave(m, d, dtype) + 1  # three workgroups and a partial fourth
    return [P.play(root, host, agent, STEPS, reposition=reposition, rescaled=rescaled, reduce_root=True,
                   rescale_root=rescaled, dtype=NP[dtype]) for root in seeded_roots(m, d, count)]


@pytest.mark.parametrize("host", R.HOSTS)
@pytest.mark.parametrize("m,d", SHAPES)
def test_hosts_and_agents_against_the_restatement(m, d, host):
    assert games_per_wave(64, 7, torch.float64) < 16 and games_per_wave(20, 3, torch.float64) == 64
    for k, (reposition, rescaled) in enumerate(CONFIGS):
        agent = ("choose_first", "choose_last")[k % 2]
        for dtype in DTYPES:
            want = expected(m, d, host, agent, reposition, rescaled, dtype)
            if (m, d) != (2, 2):
                assert {P.ENDED, P.RUNNING} <= {p.outcome for p in want} and any(p.length == 0 for p in want)
                assert max(p.length for p in want) == STEPS
            res = launch(seeded_roots(m, d, len(want)), dtype, host=host, agent=agent, max_steps=STEPS,
                         reposition=reposition, rescale=rescaled, reduce_root=True, rescale_root=rescaled, record=True)
            check(res, want, dtype, STEPS, (m, d, host, agent, reposition, rescaled, dtype))


# ---- 3. roots as given ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_unreduced_roots_with_holes(dtype):
    """HironakaValidator.reset does not reduce: rows in row order, duplicates and dominated rows included, holes anywhere"""
    rng = np.random.default_rng(5)
    b, m, d = 70, 9, 4
    roots = rng.integers(0, 5, (b, m, d))
    roots[rng.random((b, m)) < 0.3] = -1
    roots[0, 1:] = -1  # one point
    roots[1] = -1      # none
    roots[2, 3] = roots[2, 0]  # a twin
    for host in ("zeillinger", "zeillinger_lex", "all_coord"):
        for reduce_root in (False, True):
            for steps in (0, 1, 4):
                want = [P.play(r, host, "choose_first", steps, reduce_root=reduce_root, dtype=NP[dtype]) for r in roots]
                res = launch(roots, dtype, host=host, max_steps=steps, reduce_root=reduce_root, record=True)
                check(res, want, dtype, steps, (host, reduce_root, steps))
    # max_steps 0 without a root stage is a copy; with them it is Game.__init__
    res = launch(roots, dtype, host="zeillinger", max_steps=0)
    assert torch.equal(res.points, dev(roots, dtype)) and res.length.tolist() == [0] * b
    assert res.outcome.tolist() == [int((r[:, 0] >= 0).sum() < 2) for r in roots]
    want = [P.play(r, "zeillinger", "choose_first", 0, reduce_root=True, rescale_root=True, dtype=NP[dtype]) for r in roots]
    check(launch(roots, dtype, host="zeillinger", max_steps=0, reduce_root=True, rescale_root=True), want, dtype, 0, "init")
    want = [P.play(r, "zeillinger", "choose_first", 0, rescale_root=True, dtype=NP[dtype]) for r in roots]
    check(launch(roots, dtype, host="zeillinger", max_steps=0, rescale_root=True), want, dtype, 0, "rescale only")
    assert ops.game_play(dev(roots, dtype), max_steps=0).length.tolist() == [0] * b  # no host needed


# ---- 4. every outcome ----------------------------------------------------------------------------------------------

FULL = [[5, 3, 1], [1, 1, 2]]  # test_play_rules.py test_stops_of_the_restatement: a weak host offers {0, 1} for ever


def test_every_outcome_code():
    assert set(ops.PLAY_OUTCOMES) == {A.HK_PLAY_RUNNING, A.HK_PLAY_ENDED, A.HK_PLAY_NO_MOVE, A.HK_PLAY_INEXACT,
                                      A.HK_PLAY_VALUE_LIMIT}
    steps = 200
    alternate = [t % 2 for t in range(steps)]  # forced on both sides: Fibonacci growth under {0, 1}
    forced = dev(np.asarray([alternate], np.int32))
    roots = np.asarray([FULL])
    for host in ("weak_spivakovsky", "weak_spivakovsky_min_hitting"):
        for dtype in DTYPES:
            kw = dict(host=host, max_steps=steps, axes=forced, record=True)
            play = lambda **rules: P.play(FULL, host, "choose_first", steps, axes=alternate, dtype=NP[dtype], **rules)  # noqa: E731
            want = play()
            assert want.outcome == P.INEXACT and 20 < want.length < steps
            check(launch(roots, dtype, **kw), [want], dtype, steps, (host, dtype, "inexact"))
            want = play(value_threshold=1e3)
            assert want.outcome == P.VALUE_LIMIT
            check(launch(roots, dtype, value_threshold=1e3, **kw), [want], dtype, steps, (host, dtype, "value limit"))
            want = play(rescaled=True, rescale_root=True)
            assert want.outcome == P.RUNNING and want.length == steps  # the rescale keeps the values in [0, 1]
            check(launch(roots, dtype, rescale=True, rescale_root=True, **kw), [want], dtype, steps, (host, dtype, "scaled"))
            want = play(reposition=True)  # (the subsets change: a forced axis outside one stops the game where it is)
            check(launch(roots, dtype, reposition=True, **kw), [want], dtype, steps, (host, dtype, "reposition"))
    # the threshold of float32 is not that of float64
    edge = np.asarray([[[2 ** 23, 2 ** 23], [0, 2 ** 24 - 1]], [[3, 0], [0, 3]]])
    res = launch(edge, torch.float32, host="zeillinger", max_steps=3)
    assert res.outcome.tolist() == [A.HK_PLAY_INEXACT, A.HK_PLAY_ENDED] and res.length.tolist()[0] == 1
    res = launch(edge, torch.float64, host="zeillinger", max_steps=3)
    assert res.outcome.tolist()[0] == P.play(edge[0], "zeillinger", "choose_first", 3, dtype=np.float64).outcome
    assert res.outcome.tolist()[0] != A.HK_PLAY_INEXACT


def test_no_move():
    # a zero row has no support for a hitting set to meet
    zero_row = np.asarray([[[0, 0, 0], [1, 2, 3], [3, 2, 1]], [[1, 0, 2], [1, 2, 0], [0, 2, 1]]])
    for host in ("weak_spivakovsky", "weak_spivakovsky_min_hitting"):
        want = [P.play(r, host, "choose_first", 3, dtype=np.float32) for r in zero_row]
        assert want[0].outcome == P.NO_MOVE and want[0].length == 0 and want[1].length > 0
        check(launch(zero_row, torch.float32, host=host, max_steps=3, record=True), want, torch.float32, 3, host)
    roots = np.asarray([[[2, 0, 1], [0, 2, 1], [-1, -1, -1]]] * 4)
    classes = np.asarray([[0, 3], [4, 0], [3, -1], [-1, -1]], np.int32)  # class 4 does not exist at dimension 3
    axes = np.asarray([[2, 0], [0, 0], [-1, -1], [-1, -1]], np.int32)   # axis 2 is outside class 0 = {0, 1}
    res = launch(roots, torch.float32, max_steps=2, classes=dev(classes), axes=dev(axes), record=True)
    want = [P.play(roots[b], None, "choose_first", 2, classes=classes[b], axes=axes[b], dtype=np.float32) for b in range(4)]
    assert [p.outcome for p in want[:2]] == [P.NO_MOVE] * 2 and want[3].outcome == P.NO_MOVE and want[2].length >= 1
    check(res, want, torch.float32, 2, "forced")
    assert torch.equal(res.points[0], dev(roots[0], torch.float32))  # untouched


def test_wrapper_refusals():
    pts = dev(seeded_roots(9, 3, 5), torch.float32)
    kw = dict(host="zeillinger", max_steps=2)
    moves = torch.full((5, 2), -1, dtype=torch.int64, device="cuda")
    for bad in (dict(classes=moves[:, :1]), dict(axes=moves[:4]), dict(axes=moves.float()), dict(host=None),
                dict(host="spivakovsky"), dict(agent="policy"), dict(max_steps=-1), dict(step_offset=2 ** 32 - 1),
                dict(value_threshold=float("nan")), dict(out=torch.empty((5, 9, 4), device="cuda")),
                dict(out=torch.empty((5, 9, 3), device="cuda").double()), dict(points=pts[0])):
        args = {"points": pts, **kw, **bad}
        with pytest.raises(ValueError):
            ops.game_play(args.pop("points"), **args)
    for bad in (dict(points=pts.half()), dict(out=torch.empty((5, 9, 3))), dict(axes=moves.cpu())):
        args = {"points": pts, **kw, **bad}
        with pytest.raises(TypeError):
            ops.game_play(args.pop("points"), **args)
    with pytest.raises(HironakaHipError) as refused:  # a status of the C entry is raised
        ops.game_play(pts[:, :0], **kw)
    assert refused.value.status == A.HK_ERR_SHAPE
    with pytest.raises(HironakaHipError) as refused:
        ops.game_play(torch.zeros((2, 4, 8), device="cuda"), **kw)
    assert refused.value.status == A.HK_ERR_UNSUPPORTED


# ---- 5. the random agent -------------------------------------------------------------------------------------------

def test_random_agent():
    rng = np.random.default_rng(11)
    b, m, d, steps = 256, 8, 4, 8
    roots = rng.integers(0, 9, (b, m, d))
    run = lambda seed, lo=0, hi=b, off=0: launch(roots[lo:hi], torch.float32, host="all_coord", agent="random",  # noqa: E731
                                                 max_steps=steps, seed=seed, game_offset=off, reduce_root=True,
                                                 record=True)
    res = run(7)
    axes = res.axes.tolist()
    want = [P.play(roots[i], "all_coord", "choose_first", steps, axes=axes[i][: int(res.length[i])], reduce_root=True,
                   dtype=np.float32) for i in range(b)]  # (an axis outside the subset would stop the restatement)
    check(res, want, torch.float32, steps, "random")
    playing = [i for i in range(b) if res.length[i] > 0]
    assert len(playing) > b // 2 and {axes[i][0] for i in playing} == set(range(d))
    # legal under a host that offers two coordinates
    two = launch(roots, torch.float64, host="zeillinger", agent="random", max_steps=steps, seed=3, reduce_root=True,
                 record=True)
    pairs = ops.decode_host_class(two.classes.clamp(min=0).flatten(), d, torch.int32).view(b, steps, d)
    played = two.axes >= 0
    assert bool(pairs.gather(2, two.axes.clamp(min=0).unsqueeze(2).long()).squeeze(2)[played].all())
    assert bool((two.axes[played] != ops.game_play(dev(roots, torch.float64), host="zeillinger", max_steps=steps,
                                                   reduce_root=True, record=True).axes[played]).any())
    same = run(7)
    assert all(torch.equal(x, y) for x, y in zip(res, same))
    assert not torch.equal(run(8).axes, res.axes)
    halves = [run(7, 0, b // 2), run(7, b // 2, b, b // 2)]
    for k, field in enumerate(res._fields):
        assert torch.equal(torch.cat([h[k] for h in halves]), res[k]), field
    # two launches that continue the games with step_offset reproduce the one launch
    head = launch(roots, torch.float32, host="all_coord", agent="random", max_steps=3, seed=7, reduce_root=True,
                  record=True)
    tail = ops.game_play(head.points, host="all_coord", agent="random", max_steps=steps - 3, seed=7, step_offset=3,
                         record=True)
    going = head.outcome == A.HK_PLAY_RUNNING
    assert int(going.sum()) > b // 4 and torch.equal(tail.points[going], res.points[going])
    assert torch.equal(torch.cat([head.axes, tail.axes], 1)[going], res.axes[going])
    assert torch.equal((head.length + tail.length)[going], res.length[going])


def test_random_agent_is_uniform():
    """65 536 draws at a 3-coordinate subset: each axis within 5 sigma of n / 3, sigma = sqrt(n * 2 / 9)"""
    n = 65536
    roots = np.tile(np.asarray([[[1, 2, 3], [3, 2, 1], [2, 3, 1]]]), (n, 1, 1))
    res = launch(roots, torch.float32, host="all_coord", agent="random", max_steps=1, seed=2026, record=True)
    assert res.length.tolist() == [1] * n
    counts = torch.bincount(res.axes[:, 0], minlength=3).tolist()
    sigma = (n * 2 / 9) ** 0.5
    assert len(counts) == 3 and sum(counts) == n and all(abs(c - n / 3) <= 5 * sigma for c in counts), counts


# ---- 6. layouts ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_layouts(dtype):
    b, m, d = 70, 9, 3
    roots = seeded_roots(m, d, b)
    kw = dict(host="weak_spivakovsky", max_steps=4, reduce_root=True, record=True)
    base = launch(roots, dtype, **kw)

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
        res = ops.game_play(v, **kw)
        assert torch.equal(v, keep), name  # out of place leaves the input alone
        assert all(torch.equal(x, y) for x, y in zip(res, base)), name
    for name, v, whole in views():
        res = ops.game_play(v, out=v, **kw)
        assert res.points is v and torch.equal(v, base.points), name
        assert all(torch.equal(x, y) for x, y in zip(res[1:], base[1:])), name
        if name == "offset":
            assert (whole[:5] == 7).all()
        if name == "record":
            assert (whole[:, m * d:] == 7).all()
    for name, v, whole in views():  # into another layout
        out = torch.zeros((b, d, m), dtype=dtype, device="cuda").transpose(1, 2)
        assert ops.game_play(v, out=out, **kw).points is out and torch.equal(out, base.points), name
    # an out that shares memory with the points other than in place: games shifted by one, by a row, and the records
    # of one buffer read at one stride and written at another
    buf = torch.full(((b + 1) * m * d + d,), 7.0, dtype=dtype, device="cuda")
    for lo_in, lo_out in ((0, m * d), (m * d, 0), (0, d), (d, 0)):
        src, out = (buf[lo:lo + b * m * d].view(b, m, d) for lo in (lo_in, lo_out))
        src.copy_(dev(roots, dtype))
        assert ops.game_play(src, out=out, **kw).points is out and torch.equal(out, base.points), (lo_in, lo_out)
    wide = torch.full((b, 2 * m * d), 7.0, dtype=dtype, device="cuda")
    src, out = wide[:, : m * d].view(b, m, d), wide.view(-1)[: b * m * d].view(b, m, d)
    src.copy_(dev(roots, dtype))
    assert ops.game_play(src, out=out, **kw).points is out and torch.equal(out, base.points)


def test_c_entry_rejects_overlaps():
    """the C entry itself: records that overlap without being the same buffer are HK_ERR_SHAPE, nothing is launched"""
    import ctypes
    from hironaka_amd._lib import lib
    b, m, d = 8, 5, 3
    buf = torch.full(((b + 2) * m * d,), 7.0, device="cuda")
    ints = torch.zeros((2, b), dtype=torch.int32, device="cuda")
    q = A.hk_game_play_desc()
    q.points_in = buf.data_ptr()
    q.in_stride = q.out_stride = m * d
    q.length_out, q.outcome_out = ints[0].data_ptr(), ints[1].data_ptr()
    q.batch, q.max_points, q.dim, q.dtype, q.max_steps = b, m, d, A.HK_F32, 2
    q.host, q.agent = A.HK_HOST_ZEILLINGER, A.HK_AGENT_CHOOSE_FIRST
    for shift in (4, 4 * m * d, 4 * (b - 1) * m * d + 4 * (m * d - 1)):
        q.points_out = buf.data_ptr() + shift
        assert lib().hk_game_play(ctypes.byref(q), None) == A.HK_ERR_SHAPE, shift
    q.points_out, q.out_stride = buf.data_ptr(), m * d + 1
    assert lib().hk_game_play(ctypes.byref(q), None) == A.HK_ERR_SHAPE
    torch.cuda.synchronize()
    assert (buf == 7).all() and (ints == 0).all()


# ---- 7. surfaces ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", (3, 6))
@pytest.mark.parametrize("host", R.HOSTS)
def test_game_play_equals_steps(host, d):
    """GameHironaka.play(n) against n calls of step(): states, histories, stopped"""
    rng = np.random.default_rng(100 + d)
    b, m, n = 40, 8, 6
    roots = rng.integers(0, 7, (b, m, d)).astype(np.float64)
    roots[rng.random((b, m)) < 0.3] = -1
    roots[:, :2] = np.abs(roots[:, :2])  # at least two rows
    roots[5, 1:] = -1                    # a game that has ended
    for scale in (False, True):
        for dtype in DTYPES:
            make = lambda: GameHironaka(HipPoints(dev(roots, dtype), dtype=dtype, semantics="list"),  # noqa: E731
                                        HOST_TYPES[host](), ChooseFirstAgent(), scale_observation=scale)
            stepped, played = make(), make()
            assert torch.equal(stepped.state.points, played.state.points)
            for _ in range(n):
                stepped.step()
            going = played.play(n)
            label = (host, d, scale, dtype)
            assert torch.equal(stepped.state.points, played.state.points), label
            assert going == (not stepped.stopped) and played.stopped == stepped.stopped, label
            assert len(played.coord_history) == len(stepped.coord_history) == len(played.move_history) > 2, label
            for x, y in zip(stepped.coord_history + stepped.move_history, played.coord_history + played.move_history):
                assert x.dtype == y.dtype and torch.equal(x, y), label
            ended = stepped.state.ended_batch_in_tensor.to(torch.bool)
            assert torch.equal(played.stopped_batch, ended) and int(played.length[5]) == 0, label
            assert torch.equal(played.outcome == A.HK_PLAY_ENDED, ended), label
            assert torch.equal(played.length, torch.stack(played.move_history, 1).ge(0).sum(1).to(torch.int32)), label
            # play() goes on from where it stopped, as further steps do
            for _ in range(3):
                stepped.step()
            played.play(3)
            assert torch.equal(stepped.state.points, played.state.points), label
            assert len(played.move_history) == len(stepped.move_history), label


def test_game_play_surfaces():
    roots = dev(seeded_roots(10, 7, 50), torch.float32)
    # a weak host plays the plain game at dimension 7: select_coord cannot, the launch can
    game = GameHironaka(HipPoints(roots.clone(), semantics="list"), WeakSpivakovsky(), RandomAgent(5),
                        scale_observation=False)
    with pytest.raises(ValueError):
        game.step()
    game.play(4)
    want = ops.game_play(roots, host="weak_spivakovsky", agent="random", max_steps=4, seed=5, reduce_root=True)
    assert torch.equal(game.state.points, want.points) and torch.equal(game.length, want.length)
    assert int(game.length.max()) == 4 and len(game.move_history) == 4
    # an agent with USE_REPOSITION passes it on

    class Repositioning(ChooseFirstAgent):
        USE_REPOSITION = True

    res = Repositioning().play(roots, host="weak_spivakovsky", max_steps=4, reduce_root=True)
    want = ops.game_play(roots, host="weak_spivakovsky", max_steps=4, reduce_root=True, reposition=True)
    assert all(torch.equal(x, y) for x, y in zip(res[:3], want[:3]))
    assert not torch.equal(res.points, ChooseFirstAgent().play(roots, host="weak_spivakovsky", max_steps=4,
                                                               reduce_root=True).points)
    with pytest.raises(TypeError, match=r"step\(\)"):  # exact types only
        GameHironaka(HipPoints(roots.clone(), semantics="list"), Zeillinger(), Repositioning()).play(2)
    with pytest.raises(ValueError):  # torch semantics is another game
        GameHironaka(HipPoints(roots.clone()), Zeillinger(), ChooseFirstAgent()).play(2)
    # a game stopped by something other than its end stays as it is when play() is called again
    edge = dev(np.asarray([[[2 ** 23, 2 ** 23], [0, 2 ** 24 - 1]], [[5, 0], [0, 3]]]), torch.float32)
    game = GameHironaka(HipPoints(edge, semantics="list"), Zeillinger(), ChooseFirstAgent(), scale_observation=False)
    game.play(1)
    assert game.outcome.tolist() == [A.HK_PLAY_INEXACT, A.HK_PLAY_RUNNING] and not game.stopped
    frozen = game.state.points[0].clone()
    game.play(20)
    assert torch.equal(game.state.points[0], frozen) and game.outcome.tolist() == [A.HK_PLAY_INEXACT, A.HK_PLAY_ENDED]
    assert game.length.tolist()[0] == 1 and game.stopped


def test_validator_equals_the_recorded_playoffs():
    checked = 0
    for p in fixture()[1]:
        if p.agent != "choose_first":
            continue
        cfg = dict(step_threshold=p.step_threshold, scale_observation=p.scale, value_threshold=p.value_threshold)
        v = HironakaValidator(HOST_TYPES[p.host](), ChooseFirstAgent(), cfg)
        states = torch.as_tensor(p.states)
        assert v.playoff(p.num_steps, reset_states=states) == p.len_history, p.name
        lengths, outcomes = v.play_games(len(p.states), states)
        want = [P.play(st, p.host, "choose_first", p.step_threshold, rescaled=p.scale, rescale_root=p.scale,
                       value_threshold=p.value_threshold, dtype=np.float64) for st in p.states]
        assert lengths.tolist() == [g.length for g in want] and outcomes.tolist() == [g.outcome for g in want], p.name
        assert lengths.dtype == torch.int32 and lengths.is_cuda
        if p.value_threshold:
            assert A.HK_PLAY_VALUE_LIMIT in outcomes.tolist(), p.name
        with pytest.raises(ValueError):  # too few states for the budget
            v.playoff(p.num_steps, reset_states=states[:2])
        checked += 1
    assert checked >= 10


def test_validator_on_its_own_states():
    """seeded reset states on the device; the random agent; the bookkeeping adds up; games without a length raise"""
    for agent in (ChooseFirstAgent, lambda: RandomAgent(4)):
        runs = []
        for _ in range(2):
            v = HironakaValidator(Zeillinger(), agent(), dimension=4, max_num_points=12, step_threshold=30, seed=9,
                                  dtype=torch.float32)
            runs.append(v.playoff(2000))
        assert runs[0] == runs[1] and len(runs[0]) > 20
        assert sum(runs[0]) + len(runs[0]) - 1 == 2000  # every iteration either counts or records
    other = HironakaValidator(Zeillinger(), ChooseFirstAgent(), dimension=4, max_num_points=12, step_threshold=30, seed=10,
                              dtype=torch.float32).playoff(2000)
    assert other != runs[0]
    lengths, outcomes = v.play_games(300)
    assert lengths.shape == (300,) and set(outcomes.tolist()) <= {A.HK_PLAY_ENDED, A.HK_PLAY_RUNNING}
    # FULL never ends under a weak host, and a random agent makes its values grow until they leave the integers: such a
    # game has no length to count
    v = HironakaValidator(WeakSpivakovsky(), RandomAgent(1), step_threshold=1000, scale_observation=False,
                          dtype=torch.float32)
    with pytest.raises(RuntimeError, match="game 0 "):
        v.playoff(5000, reset_states=torch.as_tensor([FULL] * 4))
