"""hk_dqn_host_move and hk_dqn_agent_move (include/hironaka_hip_dqn_move.h) on the GPU against tests/dqn_move_rules.py,
bit for bit, and against the composition of the operators they replace (HipPoints.step + ops.get_dones +
ops.get_features_torch); then FusedGame.evaluate: the kernels' path, the forced torch path and the rules on the same
create_mlp nets, the recording of the reference's Trainer (tests/golden/dqn_trainer.npz), and the captured move."""
import os

import numpy as np
import pytest
import torch

import dqn_move_rules as R
from test_dqn_move_lane import bits, games, odd_values

pytestmark = pytest.mark.gpu

SHAPES = ((5, 2), (20, 3), (12, 5), (6, 7), (64, 3))
DTYPES = {np.float32: torch.float32, np.float64: torch.float64}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dqn_trainer.npz")
LDS_BYTES = 64 * 1024


def dev():
    return torch.device("cuda")


def on_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def assert_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    if got.dtype == np.bool_:
        got = got.astype(np.uint8)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, "%s: %d differ, the first at %s: got %r, want %r" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def batches(m, d, itemsize):
    """around a wave, and around the games a workgroup takes at this shape (lane_geometry)"""
    per_block = min(64, LDS_BYTES // (((2 * m * d + 2 * d) | 1) * itemsize))
    return sorted({1, 63, 64, 65, 130, max(per_block - 1, 1), per_block, per_block + 1, 2 * per_block + 1})


def q_view(q, pad_cols, offset):
    """q's values as a strided view: columns offset .. offset + width of a wider tensor"""
    wide = torch.full((q.shape[0], q.shape[1] + pad_cols), float("nan"), dtype=q.dtype, device=q.device)
    view = wide[:, offset: offset + q.shape[1]]
    view.copy_(q)
    return view


@pytest.mark.parametrize("dtype", (np.float32, np.float64), ids=("f32", "f64"))
@pytest.mark.parametrize("m,d", SHAPES)
def test_agent_move_matches_rules_and_the_operators_it_replaces(m, d, dtype):
    from hironaka_amd import ops
    from hironaka_amd.core import HipPoints
    rng = np.random.default_rng(100 * m + d)
    for k, b in enumerate(batches(m, d, np.dtype(dtype).itemsize)):
        qdtype = (np.float32, np.float64)[k % 2]
        masked, rescale, strided = bool(k & 1) or k == 0, bool(k & 2) or k == 0, k % 3 != 0
        points = np.concatenate([games(rng, m, d, dtype)] * (b // 48 + 1))[:b]
        cls = rng.integers(-1, R.num_classes(d) + 1, b)
        sub = R.O.decode_class(R.clamp_class(cls, d), d)
        q = odd_values(rng.normal(size=(b, d)).astype(qdtype), rng, sub if b >= 8 else None)
        what = "(%d,%d) B=%d q=%s masked=%d rescale=%d strided=%d" % (m, d, b, np.dtype(qdtype).name, masked, rescale, strided)

        pts, tq, tcls = on_gpu(points), on_gpu(q), on_gpu(cls.astype(np.int32))
        if strided:
            tq = q_view(tq, 5, 3)
        axis = torch.full((b,), -7, dtype=torch.int32, device=dev())
        feats = torch.full_like(pts, -7)
        done = torch.full((b,), 7, dtype=torch.uint8, device=dev())
        lengths = on_gpu(np.arange(b, dtype=np.int32))
        counts = on_gpu(np.arange(d, dtype=np.int32))
        want_lengths, want_counts = np.arange(b), np.arange(d)
        for _ in range(2):  # a second launch on the moved state: lengths and counts accumulate
            before = pts.clone()
            ops.dqn_agent_move(pts, tq, tcls, axis_out=axis, features_out=feats, done_out=done, lengths=lengths,
                               counts=counts, masked=masked, rescale=rescale)
            new, want_axis, want_feats, want_done, prev_done = R.agent_move(points, q, cls, masked=masked, rescale=rescale)
            assert_bits(pts, new, what + " points")
            assert_bits(axis, want_axis, what + " axis")
            assert_bits(feats, want_feats, what + " features")
            assert_bits(done, want_done.astype(np.uint8), what + " done")
            # the operators it replaces, given the kernel's axis
            hp = HipPoints(before, dtype=DTYPES[dtype])
            hp.step(on_gpu(sub.astype(dtype)), axis.to(torch.int64), rescale=rescale)
            assert torch.equal(hp.points.view(torch.uint8), pts.view(torch.uint8)), what
            assert torch.equal(ops.get_dones(pts).to(torch.uint8), done), what
            assert torch.equal(ops.get_features_torch(pts).view(torch.uint8), feats.view(torch.uint8)), what
            want_lengths = want_lengths + ~prev_done
            want_counts = want_counts + np.bincount(want_axis[~prev_done], minlength=d)
            assert_bits(lengths, want_lengths.astype(np.int32), what + " lengths")
            assert_bits(counts, want_counts.astype(np.int32), what + " counts")
            points = new
        # without counts, nothing else changes
        pts2, lengths2 = on_gpu(points), torch.zeros(b, dtype=torch.int32, device=dev())
        ops.dqn_agent_move(pts2, tq, tcls, axis_out=axis, features_out=feats, done_out=done, lengths=lengths2,
                           masked=masked, rescale=rescale)
        assert_bits(pts2, R.agent_move(points, q, cls, masked=masked, rescale=rescale)[0], what + " no counts")


@pytest.mark.parametrize("d", (2, 3, 5, 7))
def test_host_move_matches_rules(d):
    from hironaka_amd import ops
    rng = np.random.default_rng(d)
    classes = R.num_classes(d)
    for k, b in enumerate((1, 63, 64, 65, 130, 255, 256, 257, 600)):
        qdtype, cdtype = (np.float32, np.float64)[k % 2], (np.float32, np.float64)[(k // 2) % 2]
        q = odd_values(rng.normal(size=(b, classes)).astype(qdtype), rng)
        what = "d=%d B=%d q=%s coords=%s" % (d, b, np.dtype(qdtype).name, np.dtype(cdtype).name)
        tq = on_gpu(q) if k % 3 == 0 else q_view(on_gpu(q), 7, 2)
        cls = torch.full((b,), -7, dtype=torch.int32, device=dev())
        coords = torch.full((b, d), -7, dtype=DTYPES[cdtype], device=dev())
        prev_done = rng.random(b) < 0.3
        counts = on_gpu(np.arange(classes, dtype=np.int32))
        want_cls, want_coords = R.host_pick(q, d, cdtype)
        for launch in (1, 2):
            ops.dqn_host_move(tq, cls, coords, prev_done=on_gpu(prev_done.astype(np.uint8)), counts=counts)
            assert_bits(cls, want_cls, what + " class")
            assert_bits(coords, want_coords, what + " coords")
            assert torch.equal(coords, ops.decode_host_class(cls, d, dtype=DTYPES[cdtype])), what
            want = np.arange(classes) + launch * np.bincount(want_cls[~prev_done], minlength=classes)
            assert_bits(counts, want.astype(np.int32), what + " counts after launch %d" % launch)
        ops.dqn_host_move(tq, cls, coords)  # nothing counted
        assert_bits(counts, want.astype(np.int32), what + " counts untouched")


def test_wrappers_refuse_bad_arguments():
    from hironaka_amd import ops
    b, m, d = 4, 5, 3
    pts = torch.zeros((b, m, d), device=dev())
    good = dict(axis_out=torch.zeros(b, dtype=torch.int32, device=dev()), features_out=torch.zeros_like(pts),
                done_out=torch.zeros(b, dtype=torch.uint8, device=dev()),
                lengths=torch.zeros(b, dtype=torch.int32, device=dev()))
    q, cls = torch.zeros((b, d), device=dev()), torch.zeros(b, dtype=torch.int32, device=dev())
    ops.dqn_agent_move(pts, q, cls, **good)
    with pytest.raises(TypeError):
        ops.dqn_agent_move(pts.cpu(), q, cls, **good)
    with pytest.raises(ValueError):
        ops.dqn_agent_move(pts, q, cls, **{**good, "features_out": pts})
    with pytest.raises(ValueError):
        ops.dqn_agent_move(pts, q.to(torch.float16), cls, **good)
    with pytest.raises(ValueError):
        ops.dqn_agent_move(pts, q.t().contiguous().t(), cls, **good)
    with pytest.raises(ValueError):
        ops.dqn_agent_move(pts, q, cls.to(torch.int64), **good)
    with pytest.raises(ValueError):
        ops.dqn_agent_move(pts, q, cls, **{**good, "lengths": good["lengths"][:3]})
    with pytest.raises(ValueError):
        ops.dqn_agent_move(pts, q, cls, padding_value=0.0, **good)
    with pytest.raises(ValueError):
        ops.dqn_agent_move(torch.zeros((b, m, 8), device=dev()), q, cls, **good)
    coords = torch.zeros((b, d), device=dev())
    with pytest.raises(ValueError):
        ops.dqn_host_move(torch.zeros((b, 5), device=dev()), cls, coords)
    with pytest.raises(ValueError):
        ops.dqn_host_move(torch.zeros((b, 4), device=dev()), cls, coords, counts=torch.zeros(4, dtype=torch.int32, device=dev()))
    with pytest.raises(ValueError):
        ops.dqn_host_move(torch.zeros((b, 4), device=dev()), cls, coords[:, :2])


# ---- FusedGame.evaluate ------------------------------------------------------------------------------------------------

def mlp_players(m, d, seed):
    from hironaka_amd.nets import AgentFeatureExtractor, HostFeatureExtractor, create_mlp
    torch.manual_seed(seed)
    host = create_mlp(HostFeatureExtractor(m * d), [16, "b", 32, "b"], m * d, R.num_classes(d))
    agent = create_mlp(AgentFeatureExtractor(m * d + d), [16, "b", 32, "b"], m * d + d, d)
    for net in (host, agent):
        for mod in net.modules():  # running statistics that are not the identity
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.uniform_(-0.5, 0.5)
                mod.running_var.uniform_(0.5, 2.0)
    return host.to(dev()).eval(), agent.to(dev()).eval()


def start_states(b, m, d, max_value, seed):
    from hironaka_amd.core import HipPoints
    gen = torch.Generator(device="cuda").manual_seed(seed)
    pts = torch.randint(max_value + 1, (b, m, d), device=dev(), generator=gen).to(torch.float32)
    pts[0, 1:] = -1.0  # a game that is over at the start
    points = HipPoints(pts)
    points.get_newton_polytope()
    points.rescale()
    return points.points.clone()


def assert_same_result(got, want, what):
    assert torch.equal(got.lengths, want.lengths) and got.lengths.dtype == torch.int32, what
    assert torch.equal(got.initial_done, want.initial_done) and got.initial_done.dtype == torch.bool, what
    assert (got.counts is None) == (want.counts is None), what
    if got.counts is not None:
        assert torch.equal(got.counts, want.counts) and got.counts.dtype == torch.int32, what
    assert got.rho.dim() == 0 and torch.equal(got.rho, want.rho), what


@pytest.mark.parametrize("count_for", (None, "host", "agent"))
def test_evaluate_kernels_torch_path_and_rules_agree(count_for):
    """scale_observation on, create_mlp players: the two paths ask the same launches for Q on bit-identical features,
    so the trajectories are identical; the rules are given Q by the same nets"""
    from hironaka_amd.core import HipPoints
    from hironaka_amd.fused_game import FusedGame
    from hironaka_amd.nets import FusedSequential
    b, m, d, max_steps = 65, 20, 3, 6
    host, agent = mlp_players(m, d, 5)
    with torch.inference_mode():  # as evaluate calls them
        assert isinstance(host, FusedSequential) and host.fused_reason is None and agent.fused_reason is None
    start = start_states(b, m, d, 20, 9)
    game = FusedGame(host, agent, log_time=True)
    fused_points, torch_points = HipPoints(start.clone()), HipPoints(start.clone())
    fused = game.evaluate(fused_points, max_steps, count_for=count_for)
    assert fused.fused and game.fused_eval_last_reason is None and host.fused_last_reason is None
    plain = game.evaluate(torch_points, max_steps, count_for=count_for, force_torch=True)
    assert not plain.fused and game.fused_eval_last_reason == "force_torch" and game.log_time is True
    assert_same_result(fused, plain, count_for)
    assert torch.equal(fused_points.points.view(torch.uint8), torch_points.points.view(torch.uint8))

    with torch.inference_mode():
        host_q = lambda f: host(on_gpu(f)).cpu().numpy()  # noqa: E731
        agent_q = lambda f, c: agent({"points": on_gpu(f), "coords": on_gpu(c)}).cpu().numpy()  # noqa: E731
        lengths, initial_done, counts, rho, final = R.evaluate(start.cpu().numpy(), host_q, agent_q, max_steps,
                                                               count_for=count_for)
    assert_bits(fused.lengths, lengths, "lengths")
    assert_bits(fused.initial_done.to(torch.uint8), initial_done.astype(np.uint8), "initial_done")
    if count_for:
        assert_bits(fused.counts, counts, "counts")
    assert_bits(fused.rho, np.asarray(rho), "rho")
    assert_bits(fused_points.points, final, "final points")
    assert initial_done[0] and 0 < lengths.max() and lengths.sum() > b


@pytest.mark.parametrize("tag", ("m5_d2", "m20_d3", "m8_d4"))
def test_evaluate_reproduces_the_reference_trainer(tag):
    """the SetNet players of the recording run as they are between the two kernels"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_golden import SetNet
    from hironaka_amd.core import HipPoints
    from hironaka_amd.fused_game import FusedGame
    g = np.load(GOLDEN)
    host = SetNet(g[f"{tag}/host_w"], g[f"{tag}/host_b"])
    agent = SetNet(g[f"{tag}/agent_w"], g[f"{tag}/agent_b"], g[f"{tag}/agent_v"])
    game = FusedGame(host, agent, log_time=False)
    for count_for in ("host", "agent"):
        for force_torch in (False, True):
            res = game.evaluate(HipPoints(g[f"{tag}/start"]), int(g[f"{tag}/max_steps"]), scale_observation=False,
                                count_for=count_for, force_torch=force_torch)
            assert res.fused != force_torch
            assert_bits(res.lengths, g[f"{tag}/lengths"], tag)
            assert_bits(res.initial_done.to(torch.uint8), g[f"{tag}/initial_done"].astype(np.uint8), tag)
            assert_bits(res.counts.to(torch.int64), g[f"{tag}/{count_for}_counts"], tag)
            assert_bits(res.rho, g[f"{tag}/rho"], tag)


def test_evaluate_from_a_graph_equals_eager():
    from hironaka_amd.core import HipPoints
    from hironaka_amd.fused_game import FusedGame
    b, m, d, max_steps = 65, 20, 3, 10
    host, agent = mlp_players(m, d, 6)
    start = start_states(b, m, d, 20, 10)
    game = FusedGame(host, agent, log_time=False)
    eager_points, graph_points = HipPoints(start.clone()), HipPoints(start.clone())
    eager = game.evaluate(eager_points, max_steps, count_for="agent")
    graph = game.evaluate(graph_points, max_steps, count_for="agent", use_graph=True)
    assert eager.fused and graph.fused
    assert_same_result(graph, eager, "graph")
    assert torch.equal(eager_points.points.view(torch.uint8), graph_points.points.view(torch.uint8))
    assert int(eager.lengths.max()) > 2  # moves that only the replays played


def test_evaluate_falls_back_where_the_kernels_cannot_serve():
    from hironaka_amd.core import HipPoints
    from hironaka_amd.fused_game import FusedGame
    from hironaka_amd.player_modules import AllCoordHostModule, ChooseFirstAgentModule
    for m, d, pad, why in ((4, 8, -1.0, "dimension"), (65, 3, -1.0, "points per game"), (5, 3, 0.0, "padding")):
        game = FusedGame(AllCoordHostModule(d, m, dev()), ChooseFirstAgentModule(d, m, dev()), log_time=False)
        pts = torch.randint(0, 5, (6, m, d), device=dev()).to(torch.float32)
        points = HipPoints(pts, padding_value=pad)
        points.get_newton_polytope()
        res = game.evaluate(points, 3, scale_observation=False, count_for="agent")
        assert not res.fused and why in game.fused_eval_last_reason, game.fused_eval_last_reason
        assert res.lengths.shape == (6,) and int(res.counts.sum()) == int(res.lengths.sum())
