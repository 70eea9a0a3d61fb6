"""hk_replay_push / hk_replay_sample, ReplayBuffer and FusedGame.collect on the device against tests/replay_rules.py
(which test_replay_rules.py pins to the reference's own ReplayBuffer), byte for byte.

T is the number of batch rows one workgroup owns: the sizes below are the smallest that put a push below, at and
beyond one tile, with a ragged last tile."""
import os
import warnings

import numpy as np
import pytest
import torch

import replay_rules as RR
from conftest import GOLDEN
from hironaka_amd import _abi as A

pytestmark = pytest.mark.gpu

T = A.HK_REPLAY_TILE_ROWS
AGENT_ROW_BYTES = [240, 12, 4, 4, 1, 240, 12]  # the agent role's experience at (20, 3) float32
SENTINEL = 0xA5
KEEPS = ["null", "none", "one", "alternating", "random", "tile_first", "tile_last"]


def _ops():
    from hironaka_amd import ops
    return ops


def _keep(pattern, batch, rng, move):
    j = np.arange(batch)
    if pattern == "null":
        return None
    return {"none": np.zeros(batch), "one": j == (move * 3) % batch, "alternating": (j + move) % 2,
            "random": rng.integers(0, 2, batch), "tile_first": j % T == 0,
            "tile_last": (j % T == T - 1) | (j == batch - 1)}[pattern].astype(np.uint8)


class _Pair:
    """a buffer of byte columns on the device, and the rules' copy of it on the host"""

    def __init__(self, row_bytes, capacity):
        self.capacity = capacity
        self.host = [np.full((capacity, rb), SENTINEL, dtype=np.uint8) for rb in row_bytes]
        self.dev = [torch.full((capacity, rb), SENTINEL, dtype=torch.uint8, device="cuda") for rb in row_bytes]
        self.cur_host = RR.new_cursor()
        self.cursor = _ops().replay_cursor("cuda")

    def set_cursor(self, **words):
        for name, v in words.items():
            self.cur_host[getattr(RR, name)] = v
        self.cursor.copy_(torch.from_numpy(self.cur_host))

    def push(self, rows, keep):
        RR.push(self.host, rows, self.cur_host, keep=keep)
        _ops().replay_push(self.dev, [torch.from_numpy(r).cuda() for r in rows], self.cursor,
                           keep=None if keep is None else torch.from_numpy(keep).cuda())

    def check(self, where):
        assert self.cursor.cpu().numpy().tolist() == self.cur_host.tolist(), where
        for c, (d, h) in enumerate(zip(self.dev, self.host)):
            assert d.cpu().numpy().tobytes() == h.tobytes(), (where, c)  # the slots not written keep the sentinel


def _rows(rng, batch, row_bytes):
    return [rng.integers(0, 255, (batch, rb)).astype(np.uint8) for rb in row_bytes]


@pytest.mark.parametrize("pattern", KEEPS)
@pytest.mark.parametrize("roomy", [False, True])
@pytest.mark.parametrize("batch", [1, 5, T, 2 * T + 3])
def test_push_matches_rules(batch, roomy, pattern):
    capacity = 3 * batch + 7 if roomy else batch + 1
    rng = np.random.default_rng(batch * 7 + roomy)
    pair = _Pair(AGENT_ROW_BYTES, capacity)
    for move in range(4):
        keep = _keep(pattern, batch, rng, move)
        if keep is not None and move == 2:
            keep = keep * 255  # any nonzero byte keeps
        pair.push(_rows(rng, batch, AGENT_ROW_BYTES), keep)
        pair.check((move, pair.cur_host.tolist()))
    if pattern == "null":
        assert pair.cur_host[RR.TOTAL_PUSHED] == 4 * batch
        assert pair.cur_host[RR.FULL] == (4 * batch >= capacity) and (pair.cur_host[RR.FULL] or batch < 7)


@pytest.mark.parametrize("pattern", ["null", "random", "tile_last"])
@pytest.mark.parametrize("back", ["tile", "batch", "one", "tile_minus", "tile_plus"])
def test_push_wrap_positions(back, pattern):
    """the wrap on a tile boundary, exactly at the end of the push, and a row to either side of those"""
    batch = 2 * T + 3
    capacity = 3 * batch + 7
    rng = np.random.default_rng(11)
    pair = _Pair(AGENT_ROW_BYTES, capacity)
    start = capacity - {"tile": T, "batch": batch, "one": 1, "tile_minus": T - 1, "tile_plus": T + 1}[back]
    pair.set_cursor(POS=start, TOTAL_PUSHED=start)
    pair.push(_rows(rng, batch, AGENT_ROW_BYTES), _keep(pattern, batch, rng, 0))
    pair.check(back)
    if pattern == "null":
        assert pair.cur_host[RR.FULL] == 1 and pair.cur_host[RR.POS] == (start + batch) % capacity
        assert (back == "batch") == (pair.cur_host[RR.POS] == 0)
    pair.push(_rows(rng, batch, AGENT_ROW_BYTES), _keep(pattern, batch, rng, 1))
    pair.check(back)


@pytest.mark.parametrize("row,stride,offset", [(6, 10, 2), (8, 16, 4), (16, 48, 16)])
def test_push_and_sample_strided_rows(row, stride, offset):
    """rows inside wider records that start off the allocation's alignment: 6-byte rows 2 bytes in go byte by byte,
    8-byte rows 4 bytes in as dwords, 16-byte rows of 48-byte records 16 bytes at a time"""
    ops = _ops()
    batch, capacity = T + 5, 2 * T + 1
    rng = np.random.default_rng(row)
    pair = _Pair([row], capacity)
    for move in range(3):
        rec = rng.integers(0, 255, offset + batch * stride).astype(np.uint8)
        keep = _keep("random", batch, rng, move)
        view = lambda flat: flat[offset:offset + batch * stride].reshape(batch, stride)[:, :row]  # noqa: E731
        RR.push(pair.host, [view(rec)], pair.cur_host, keep=keep)
        rows = view(torch.from_numpy(rec).cuda())
        assert rows.data_ptr() % 16 == offset % 16 and rows.stride(0) == stride
        ops.replay_push(pair.dev, [rows], pair.cursor, keep=torch.from_numpy(keep).cuda())
        pair.check(move)
    n = T + 3
    flat = torch.full((offset + n * stride,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = flat[offset:].reshape(n, stride)[:, :row]
    _, index = ops.replay_sample(pair.dev, pair.cursor, n, seed=9, out=[out])
    want = np.full(offset + n * stride, SENTINEL, dtype=np.uint8)
    idx = RR.sample_indices(pair.cur_host, capacity, n, seed=9)
    want[offset:].reshape(n, stride)[:, :row] = pair.host[0][idx]
    assert index.cpu().numpy().tolist() == idx.tolist()
    assert flat.cpu().numpy().tobytes() == want.tobytes()  # the bytes between the rows are left alone


@pytest.mark.parametrize("n", [1, T, 2 * T + 3])
def test_sample_matches_rules(n):
    ops = _ops()
    batch, capacity = T + 9, 2 * T + 40
    rng = np.random.default_rng(n)
    pair = _Pair(AGENT_ROW_BYTES, capacity)
    # an empty buffer: every index -1, the outputs untouched, and the draw still counts
    out = [torch.full((n, rb), 0x3C, dtype=torch.uint8, device="cuda") for rb in AGENT_ROW_BYTES]
    _, index = ops.replay_sample(pair.dev, pair.cursor, n, seed=5, out=out)
    assert (RR.sample_indices(pair.cur_host, capacity, n, seed=5) == -1).all()
    assert (index.cpu().numpy() == -1).all() and all(bool((o == 0x3C).all()) for o in out)
    pair.check("empty")
    seen = []
    for move in range(3):  # not full after the first two pushes, full after the third
        pair.push(_rows(rng, batch, AGENT_ROW_BYTES), _keep("alternating" if move == 0 else "null", batch, rng, move))
        for again in range(2):
            cols, index = ops.replay_sample(pair.dev, pair.cursor, n, seed=5)
            idx = RR.sample_indices(pair.cur_host, capacity, n, seed=5)
            assert index.dtype == torch.int64 and index.cpu().numpy().tolist() == idx.tolist(), (move, again)
            if not pair.cur_host[RR.FULL]:
                assert idx.max() < pair.cur_host[RR.POS]
            for c, col in enumerate(cols):
                assert col.cpu().numpy().tobytes() == pair.host[c][idx].tobytes(), (move, again, c)
            seen.append(idx)
        pair.check(move)
    assert pair.cur_host[RR.FULL] == 1 and pair.cur_host[RR.SAMPLES_DRAWN] == 7
    if n > 1:
        assert (seen[0] != seen[1]).any() and (seen[4] != seen[5]).any()  # samples_drawn moves on: two calls differ
    with pytest.raises(TypeError):
        ops.replay_sample([d.cpu() for d in pair.dev], pair.cursor, n, seed=5)
    with pytest.raises(TypeError):
        ops.replay_push(pair.dev, [torch.zeros(2, rb, dtype=torch.uint8) for rb in AGENT_ROW_BYTES], pair.cursor)
    with pytest.raises(ValueError):
        ops.replay_push(pair.dev, [torch.zeros(capacity, rb, dtype=torch.uint8, device="cuda")
                                   for rb in AGENT_ROW_BYTES], pair.cursor)


# ---- ReplayBuffer: the reference's sequence on the device --------------------------------------------------------

def _experience(fixture, tag, a):
    t = {c: torch.from_numpy(fixture[f"{tag}_a{a}_in_{c}"]).cuda() for c in RR.COLUMNS[tag]}
    if tag == "dict":
        obs = {k: t[f"obs_{k}"] for k in RR.SHAPES[tag]}
        nxt = {k: t[f"next_{k}"] for k in RR.SHAPES[tag]}
    else:
        obs, nxt = t["obs"], t["next"]
    return obs, t["action"], t["reward"], t["done"], nxt


def _storage(buf, tag):
    if tag == "dict":
        obs = [buf.observations[k] for k in RR.SHAPES[tag]]
        nxt = [buf.next_observations[k] for k in RR.SHAPES[tag]]
    else:
        obs, nxt = [buf.observations], [buf.next_observations]
    return obs + [buf.actions, buf.rewards, buf.dones] + nxt


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("tag", ["tuple", "dict"])
def test_replay_buffer_replays_the_reference(tag, dtype):
    import hironaka_amd
    from hironaka_amd.replay_buffer import ReplayBuffer
    assert hironaka_amd.ReplayBuffer is ReplayBuffer
    fixture = np.load(os.path.join(GOLDEN, "replay_buffer.npz"))
    buf = ReplayBuffer(RR.SHAPES[tag], 3, 10, "cuda", dtype=dtype, seed=3)
    with pytest.raises(AssertionError):
        buf.sample(4)  # nothing was ever added
    for a, n in enumerate(fixture[f"{tag}_lengths"]):
        if fixture[f"{tag}_asserts"][a]:
            with pytest.raises(AssertionError):
                buf.add(*_experience(fixture, tag, a))
        else:
            buf.add(*_experience(fixture, tag, a))
        for c, got in zip(RR.COLUMNS[tag], _storage(buf, tag)):
            want = torch.from_numpy(fixture[f"{tag}_a{a}_buf_{c}"])
            if c not in RR.DTYPES:
                want = want.to(dtype)  # an observation: quarters of small integers: exact in float16 too
            assert got.dtype == want.dtype and got.shape == want.shape, (a, c)
            assert torch.equal(got.cpu(), want), (a, c)
        assert buf.pos == fixture[f"{tag}_pos"][a] and buf.full == bool(fixture[f"{tag}_full"][a]), a
    obs, act, rew, done, nxt = buf.sample(64)
    idx = buf.last_sample_index
    cur = RR.new_cursor()
    cur[RR.FULL] = 1
    assert idx.cpu().numpy().tolist() == RR.sample_indices(cur, 10, 64, seed=3).tolist()
    assert act.dtype == torch.int32 and rew.dtype == torch.float32 and done.dtype == torch.bool
    assert torch.equal(act, buf.actions[idx]) and torch.equal(rew, buf.rewards[idx])
    assert torch.equal(done, buf.dones[idx])
    if tag == "dict":
        assert sorted(obs) == sorted(nxt) == ["coords", "points"] and obs["points"].dtype == dtype
        assert torch.equal(obs["coords"], buf.observations["coords"][idx])
        assert torch.equal(nxt["points"], buf.next_observations["points"][idx])
    else:
        assert obs.dtype == dtype and obs.shape == (64, 4, 3)
        assert torch.equal(obs, buf.observations[idx]) and torch.equal(nxt, buf.next_observations[idx])
    buf.reset()
    assert buf.pos == 0 and not buf.full and not bool(buf.cursor.any())
    with pytest.raises(TypeError):
        ReplayBuffer(RR.SHAPES[tag], 3, 10, "cpu")


def test_replay_buffer_add_with_keep():
    """uncompacted inputs with a mask == the compacted inputs without one"""
    from hironaka_amd.replay_buffer import ReplayBuffer
    rng = np.random.default_rng(2)
    masked, plain = (ReplayBuffer(RR.SHAPES["dict"], 3, T + 8, "cuda") for _ in range(2))
    for move in range(3):
        b = T + 7
        keep = torch.from_numpy(rng.integers(0, 2, b).astype(bool)).cuda()
        obs, nxt = ({"points": torch.rand(b, 4, 3, device="cuda"), "coords": torch.rand(b, 3, device="cuda")}
                    for _ in range(2))
        act = torch.randint(0, 3, (b, 1), device="cuda")
        rew, done = torch.rand(b, 1, device="cuda"), torch.rand(b, 1, device="cuda") < 0.5
        masked.add(obs, act, rew, done, nxt, keep=keep if move else keep.to(torch.uint8))
        pick = lambda x: {k: v[keep] for k, v in x.items()}  # noqa: E731
        plain.add(pick(obs), act[keep], rew[keep], done[keep], pick(nxt))
        for x, y in zip(_storage(masked, "dict"), _storage(plain, "dict")):
            assert torch.equal(x, y), move
        assert torch.equal(masked.cursor, plain.cursor)
    assert masked.full


# ---- FusedGame.collect ---------------------------------------------------------------------------------------------

class _SumNet(torch.nn.Module):
    """a deterministic player: a fixed linear map of the column sums (and of the host's subset, for the agent)"""

    def __init__(self, d, outputs, seed, agent=False):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = torch.nn.Parameter(torch.randn(d, outputs, generator=g), requires_grad=False)
        self.v = torch.nn.Parameter(torch.randn(d, outputs, generator=g), requires_grad=False) if agent else None

    def forward(self, x):
        if isinstance(x, dict):
            return x["points"].sum(dim=1) @ self.w + x["coords"] @ self.v
        return x.sum(dim=1) @ self.w


@pytest.mark.parametrize("role", ["host", "agent"])
def test_collect_fills_the_buffer_as_step_and_add_do(role):
    from hironaka_amd.core import HipPoints
    from hironaka_amd.fused_game import FusedGame
    from hironaka_amd.replay_buffer import ReplayBuffer
    b, m, d, capacity = 70, 6, 3, 100
    start = torch.randint(0, 6, (b, m, d), generator=torch.Generator().manual_seed(4)).float()
    shape = (m, d) if role == "host" else {"points": (m, d), "coords": (d,)}
    states, buffers, finished = [], [], []
    for way in ("step", "collect"):
        game = FusedGame(_SumNet(d, 2 ** d - d - 1, 1), _SumNet(d, d, 2, agent=True), log_time=(way == "collect"))
        pts = HipPoints(start.clone())
        pts.get_newton_polytope()
        buf = ReplayBuffer(shape, d if role == "agent" else 2 ** d - d - 1, capacity, "cuda")
        torch.manual_seed(0)
        for t in range(3):
            if way == "step":
                finished.append(int(pts.ended_batch_in_tensor.sum()))
                buf.add(*game.step(pts, role, exploration_rate=0.0))
            else:
                mode = torch.cuda.get_sync_debug_mode()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # "a prototype feature"
                    torch.cuda.set_sync_debug_mode("error")  # a synchronising torch call inside collect raises
                    try:
                        assert game.collect(pts, role, buf, exploration_rate=0.0) is None
                    finally:
                        torch.cuda.set_sync_debug_mode(mode)
        assert game.log_time == (way == "collect")
        states.append(pts.points.clone())
        buffers.append(buf)
    assert 0 <= finished[0] < finished[2] < b, finished  # games finish on the way, and not all of them
    assert torch.equal(states[0], states[1])
    by_step, by_collect = buffers
    for c, (x, y) in enumerate(zip(_storage(by_step, "tuple" if role == "host" else "dict"),
                                   _storage(by_collect, "tuple" if role == "host" else "dict"))):
        assert torch.equal(x, y), c
    assert torch.equal(by_step.cursor, by_collect.cursor)
    assert by_step.full and by_step.cursor[A.HK_REPLAY_TOTAL_PUSHED] == 3 * b - sum(finished)  # it wrapped


# ---- graph capture ---------------------------------------------------------------------------------------------------

def test_push_and_sample_replay_from_a_graph():
    """one push + one sample on one stream, captured: three replays == three eager calls (the cursor is device state)"""
    ops = _ops()
    batch, capacity, n = T + 3, 3 * T, 40
    rng = np.random.default_rng(8)
    rows = [torch.from_numpy(r).cuda() for r in _rows(rng, batch, AGENT_ROW_BYTES)]
    keep = torch.from_numpy(_keep("random", batch, rng, 0)).cuda()

    def fresh():
        return ([torch.full((capacity, rb), SENTINEL, dtype=torch.uint8, device="cuda") for rb in AGENT_ROW_BYTES],
                ops.replay_cursor("cuda"))

    eager_rings, eager_cursor = fresh()
    eager = []
    for _ in range(3):
        ops.replay_push(eager_rings, rows, eager_cursor, keep=keep)
        cols, index = ops.replay_sample(eager_rings, eager_cursor, n, seed=6)
        eager.append((index.clone(), [c.clone() for c in cols]))
    rings, cursor = fresh()
    out = [torch.zeros((n, rb), dtype=torch.uint8, device="cuda") for rb in AGENT_ROW_BYTES]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.replay_push(rings, rows, cursor, keep=keep)
        _, index = ops.replay_sample(rings, cursor, n, seed=6, out=out)
    assert not bool(cursor.any())  # capturing runs nothing
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(index, eager[k][0]), k
        for x, y in zip(out, eager[k][1]):
            assert torch.equal(x, y), k
    assert not torch.equal(eager[0][0], eager[1][0])
    assert torch.equal(cursor, eager_cursor) and int(cursor[A.HK_REPLAY_SAMPLES_DRAWN]) == 3
    for x, y in zip(rings, eager_rings):
        assert torch.equal(x, y)
