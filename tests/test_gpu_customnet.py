"""hk_customnet_forward, hironaka_amd.net.CustomNet and HipTrainer(custom_net=True) on the device against
tests/customnet_rules.py (which test_customnet_rules.py pins by hand and to the reference's own formula).

Everything the kernels write is compared with the rule bit for bit under HK_CUSTOMNET_RAW_VALUE; with the tanh the value
stays within the bound test_gpu_pvnet.py::test_the_tanh documents.  Every case asserts that its inputs hold the point
counts it claims to cover.  The shapes are the smallest that reach every path: both block kinds, widths that are no
multiple of 16 (a head width of 24 + 3), a width change, more groups than full tiles (21 groups in 64 rows), batches on
both sides of the 16-row tile, every row in one group, every row with no tower at all."""
import numpy as np
import pytest
import torch

import customnet_rules as C
from hironaka_amd import _abi as A
from test_gpu_mlp import SENTINEL, Guarded, dev
from test_gpu_pvnet import TANH_BOUND_UNITS, randomised, to_numpy

pytestmark = pytest.mark.gpu
same_bits = C.same_bits
F32 = np.float32
TILES = (A.HK_MLP_TILE_SMALL, A.HK_MLP_TILE_LARGE)  # (below the crossover the library's own choice is the small one)

# (name, m, d, e, block widths, kind, actions)
SHAPES = [
    ("test_host", 5, 3, 0, [32, 32], "residue", 4),
    ("test_agent", 5, 3, 3, [32, 32], "residue", 3),
    ("dense_agent", 5, 3, 3, [128, 128], "dense", 3),
    ("odd_dense_agent", 5, 3, 3, [40, 24], "dense", 3),
    ("twenty_agent", 20, 3, 3, [64, 32], "residue", 3),
    ("two_host", 2, 2, 0, [32], "residue", 1),
]


def _ops():
    from hironaka_amd import ops
    return ops


def _net():
    from hironaka_amd import net
    return net


def device_plan(net, m, d, e):
    ops = _ops()
    dn = lambda t: None if t is None else ops.PvnetDense(*(dev(a) for a in t))  # noqa: E731
    towers = [[ops.PvnetBlock(b.kind, dn(b.dense1), dn(b.dense2), dn(b.proj), b.eps) for b in tower] for tower in net.towers]
    return ops.CustomnetPlan(towers, tuple(dev(a) for a in net.policy), tuple(dev(a) for a in net.value), (m, d), e)


def batches(rng, m, d, e):
    """{name: (rows, the counts the case claims to cover)}"""
    every = np.arange(m + 1)
    cases = {
        "one row": [m // 2],
        "16 rows": rng.integers(0, m + 1, 16),
        "17 rows": np.concatenate([every, rng.integers(0, m + 1, 17)])[:17],
        "100 rows": np.concatenate([every, rng.integers(0, m + 1, 100)])[:100],
        "64 rows over every count": np.arange(64) % (m + 1),
        "one group": np.full(37, m - 1),
        "no tower": np.full(19, m),
        "no point": np.full(33, 0),
    }
    out = {name: (C.rows_with_counts(rng, np.asarray(cs), m, d, e), sorted(set(int(c) for c in cs))) for name, cs in cases.items()}
    cs = np.concatenate([every[1:], rng.integers(1, m, 20)]) if m > 1 else np.ones(8, int)
    out["holes"] = (C.rows_with_counts(rng, cs, m, d, e, holes=True), sorted(set(int(c) for c in cs)))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_kernels_match_the_rule(shape):
    name, m, d, e, arch, kind, actions = shape
    rng = np.random.default_rng(sum(map(ord, name)))
    net = C.random_net(rng, m, d, e, arch, actions, kind)
    cases = batches(rng, m, d, e)
    everything = np.concatenate([x for x, _ in cases.values()])
    want_p, want_v = C.forward(everything, net, m, d, e)  # the rule once: a row's result is its own
    plan = device_plan(net, m, d, e)
    at = 0
    for case, (x, claimed) in cases.items():
        assert sorted(set(C.counts(x, m, d))) == claimed, case
        if case == "64 rows over every count":
            assert claimed == list(range(m + 1)) and len(x) == 64
        if case == "holes":  # a point behind a -1 row
            pts = x[:, : m * d].reshape(len(x), m, d)[:, :, 0] >= 0
            assert (pts[:, 1:] & ~pts[:, :-1]).any()
        p, v = want_p[at: at + len(x)], want_v[at: at + len(x)]
        at += len(x)
        for tile in (None,) + TILES:
            got = _ops().customnet_forward(dev(x), plan, tile=tile, raw_value=True)
            assert got[0].shape == (len(x), actions) and got[1].shape == (len(x),)
            assert same_bits(got[0].cpu().numpy(), p), (case, tile, "policy")
            assert same_bits(got[1].cpu().numpy(), v), (case, tile, "value")
    # with the tanh: the same policy, the value within the documented bound of float64's tanh
    x = cases["100 rows"][0]
    want = C.forward(x, net, m, d, e)
    p, v = _ops().customnet_forward(dev(x), plan)
    assert same_bits(p.cpu().numpy(), want[0])
    assert float(np.abs(v.cpu().numpy().astype(np.float64) - np.tanh(want[1].astype(np.float64))).max()) <= TANH_BOUND_UNITS * C.M.UNIT
    assert _ops().customnet_forward(dev(x[:0]), plan)[0].shape == (0, actions)


@pytest.fixture(scope="module")
def agent():
    """the (5, 3) agent of the test config with its rule results on 37 rows of every count"""
    m, d, e = 5, 3, 3
    rng = np.random.default_rng(50)
    net = C.random_net(rng, m, d, e, [64, 32], 3)
    x = C.rows_with_counts(rng, np.arange(37) % (m + 1), m, d, e)
    other = C.rows_with_counts(rng, rng.integers(0, m + 1, 53), m, d, e)
    return dict(m=m, d=d, e=e, net=net, x=x, want=C.forward(x, net, m, d, e), other=other,
                other_want=C.forward(other, net, m, d, e), plan=device_plan(net, m, d, e))


@pytest.mark.parametrize("tile", TILES)
def test_layouts_and_guards(agent, tile):
    """x as a column slice of a wider buffer (x_stride > K) at an element offset, policy at a row stride, value at an
    element stride, between sentinels that must stay; policy and value as columns of one record"""
    ops, x, want, plan = _ops(), agent["x"], agent["want"], agent["plan"]
    batch, k, a = len(x), x.shape[1], 3
    for case, (ox, sx, op, sp, ov, sv) in enumerate([(0, k, 0, a, 0, 1), (1, k + 7, 1, a, 3, 1), (2, k + 3, 3, a + 7, 1, 3)]):
        gx, p, v = Guarded(batch, k, ox, sx, x), Guarded(batch, a, op, sp), Guarded(batch, 1, ov, sv)
        got = ops.customnet_forward(gx.view, plan, tile=tile, raw_value=True, out=(p.view, v.view[:, 0]))
        assert got[0] is p.view and got[1].data_ptr() == v.view.data_ptr()
        assert p.holds(want[0]) and v.holds(want[1]) and gx.holds(), case
    rec = torch.full((batch, a + 3), SENTINEL, dtype=torch.float32, device="cuda")
    ops.customnet_forward(dev(x), plan, tile=tile, raw_value=True, out=(rec[:, :a], rec[:, a]))
    expect = np.full((batch, a + 3), SENTINEL, F32)
    expect[:, :a], expect[:, a] = want
    assert same_bits(rec.cpu().numpy(), expect)
    # the host's rows as the expander passes them: the first m * d columns of the agent's buffer
    m, d = agent["m"], agent["d"]
    host = C.random_net(np.random.default_rng(51), m, d, 0, [32], 4)
    got = ops.customnet_forward(dev(x)[:, : m * d], device_plan(host, m, d, 0), tile=tile, raw_value=True)
    host_want = C.forward(x[:, : m * d], host, m, d, 0)
    assert same_bits(got[0].cpu().numpy(), host_want[0]) and same_bits(got[1].cpu().numpy(), host_want[1])


def test_the_gate(agent):
    ops, x, want, plan = _ops(), agent["x"], agent["want"], agent["plan"]
    word = torch.tensor([1], dtype=torch.int32, device="cuda")
    p = torch.full((len(x), 3), SENTINEL, dtype=torch.float32, device="cuda")
    v = torch.full((len(x),), SENTINEL, dtype=torch.float32, device="cuda")
    ops.customnet_forward(dev(x), plan, raw_value=True, gate=(word, 0), out=(p, v))
    assert bool((p == SENTINEL).all()) and bool((v == SENTINEL).all())  # *gate != want: as they were
    ops.customnet_forward(dev(x), plan, raw_value=True, gate=(word, 1), out=(p, v))
    assert same_bits(p.cpu().numpy(), want[0]) and same_bits(v.cpu().numpy(), want[1])
    with pytest.raises(TypeError):
        ops.customnet_forward(dev(x), plan, gate=(word.long(), 1))


def test_calls_in_a_row_and_graph_replay(agent):
    """the workspace needs nothing of the caller: a call on another batch between two calls on the same one changes
    nothing, and a captured sequence of three forwards replays to the eager bits"""
    ops, plan = _ops(), agent["plan"]
    x, other = dev(agent["x"]), dev(agent["other"])
    first = [t.clone() for t in ops.customnet_forward(x, plan, raw_value=True)]
    between = [t.clone() for t in ops.customnet_forward(other, plan, raw_value=True)]
    again = ops.customnet_forward(x, plan, raw_value=True)
    assert same_bits(first[0].cpu().numpy(), agent["want"][0]) and same_bits(first[1].cpu().numpy(), agent["want"][1])
    assert same_bits(between[0].cpu().numpy(), agent["other_want"][0]) and same_bits(between[1].cpu().numpy(), agent["other_want"][1])
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    static_x, static_other = x.clone(), other.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.customnet_forward(static_other, plan, raw_value=True)  # (the workspace has its size before the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # sequential: one stream, no branches
        a = ops.customnet_forward(static_x, plan, raw_value=True)
        b = ops.customnet_forward(static_other, plan, raw_value=True)
        c = ops.customnet_forward(static_x, plan, raw_value=True)
    for _ in range(2):
        for t in a + b + c:
            t.fill_(SENTINEL)
        graph.replay()
        assert torch.equal(a[0], first[0]) and torch.equal(a[1], first[1])
        assert torch.equal(b[0], between[0]) and torch.equal(b[1], between[1])
        assert torch.equal(c[0], first[0]) and torch.equal(c[1], first[1])
    static_x.copy_(x.flip(0))
    graph.replay()
    assert torch.equal(a[0], first[0].flip(0)) and torch.equal(c[1], first[1].flip(0)) and torch.equal(b[0], between[0])


def test_front_end_refuses(agent):
    ops, plan, x = _ops(), agent["plan"], dev(agent["x"])
    with pytest.raises(TypeError):
        ops.customnet_forward(x.cpu(), plan)
    with pytest.raises(TypeError):
        ops.customnet_forward(x, [plan])
    with pytest.raises(ValueError):
        ops.customnet_forward(x[:, :15], plan)
    with pytest.raises(ValueError):
        ops.customnet_forward(x, plan, tile=32)
    net, m, d, e = agent["net"], agent["m"], agent["d"], agent["e"]
    with pytest.raises(ValueError, match="tower"):
        device_plan(net._replace(towers=net.towers[:-1]), m, d, e)
    with pytest.raises(ValueError, match="inputs"):
        device_plan(net._replace(towers=net.towers[::-1]), m, d, e)
    with pytest.raises(ValueError):
        device_plan(net, m, d, e + 1)


# ---- more than 1 024 rows: the group launch's workgroups hand over through the counters in memory ------------------------

# (name, m, d, e, block widths, kind, actions, rows): neither batch is a multiple of 1 024 (3 and 5 workgroups of the group
# launch); 5 000 rows lie above the row tile's crossover, so tile=None is the 64-row tile there and the 16-row one at 2 500
LARGE = [
    ("large_agent", 5, 3, 3, [64, 32], "residue", 3, 2500),
    ("large_twenty_agent", 20, 3, 3, [64, 32], "residue", 3, 5000),
]


def counters(plan):
    """the ticket and the histogram at the head of the plan's workspace (words 1 and 4 .. 68)"""
    return plan.workspace.view(torch.int32).reshape(-1)[:72].cpu().numpy()[[1] + list(range(4, 69))]


@pytest.mark.parametrize("shape", LARGE, ids=[s[0] for s in LARGE])
def test_batches_of_several_group_workgroups(shape):
    """the rule's bits with every tile; the counters in memory are zero after every call; a gated-off call leaves outputs
    and counters alone and the ungated one behind it is right; large, small, large on one plan, eagerly and from a graph
    replayed twice"""
    name, m, d, e, arch, kind, actions, rows = shape
    ops = _ops()
    assert rows > 2 * 1024 and rows % 1024 and (rows > A.HK_MLP_TILE_CROSSOVER) == (rows == 5000)
    rng = np.random.default_rng(sum(map(ord, name)))
    net = C.random_net(rng, m, d, e, arch, actions, kind)
    cs = np.concatenate([np.arange(m + 1), rng.integers(0, m + 1, rows)])[:rows]
    cs[-3:] = (m, 0, m - 1)  # (the last, partial workgroup holds rows too)
    large = C.rows_with_counts(rng, cs, m, d, e)
    small = C.rows_with_counts(rng, np.arange(45) % (m + 1), m, d, e)
    assert sorted(set(C.counts(large, m, d))) == list(range(m + 1)) == sorted(set(C.counts(small, m, d)))
    want = C.forward(np.concatenate([large, small]), net, m, d, e)
    want_large, want_small = (want[0][:rows], want[1][:rows]), (want[0][rows:], want[1][rows:])
    plan = device_plan(net, m, d, e)
    x, y = dev(large), dev(small)

    def right(got, expect, where):
        assert same_bits(got[0].cpu().numpy(), expect[0]) and same_bits(got[1].cpu().numpy(), expect[1]), where
        assert not counters(plan).any(), where  # the ticket and the histogram: zero again

    for tile in (None,) + TILES:
        right(ops.customnet_forward(x, plan, tile=tile, raw_value=True), want_large, tile)
    # the gate: off, then on, at this size
    word = torch.tensor([0], dtype=torch.int32, device="cuda")
    p = torch.full((rows, actions), SENTINEL, dtype=torch.float32, device="cuda")
    v = torch.full((rows,), SENTINEL, dtype=torch.float32, device="cuda")
    ops.customnet_forward(x, plan, raw_value=True, gate=(word, 1), out=(p, v))
    assert bool((p == SENTINEL).all()) and bool((v == SENTINEL).all()) and not counters(plan).any()
    right(ops.customnet_forward(x, plan, raw_value=True, gate=(word, 0), out=(p, v)), want_large, "gated on")
    right(ops.customnet_forward(x, plan, raw_value=True), want_large, "behind the gated calls")
    # large, small, large on one plan
    right(ops.customnet_forward(y, plan, raw_value=True), want_small, "small between")
    right(ops.customnet_forward(x, plan, raw_value=True), want_large, "large again")
    static_x, static_y = x.clone(), y.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # sequential: one stream, no branches; the workspace has its size already
        a = ops.customnet_forward(static_x, plan, raw_value=True)
        b = ops.customnet_forward(static_y, plan, raw_value=True)
        c = ops.customnet_forward(static_x, plan, raw_value=True)
    for replay in range(2):
        for t in a + b + c:
            t.fill_(SENTINEL)
        graph.replay()
        right(a, want_large, ("replay", replay, "first"))
        right(b, want_small, ("replay", replay, "small"))
        right(c, want_large, ("replay", replay, "third"))
    static_x.copy_(x.flip(0))  # other rows in every workgroup of the group launch
    graph.replay()
    right((a[0].flip(0), a[1].flip(0)), want_large, "flipped")
    right((c[0].flip(0), c[1].flip(0)), want_large, "flipped, third")


# ---- through hironaka_amd.net -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("role,block", [("host", "DenseResidueBlock"), ("agent", "DenseBlock")])
def test_the_module_takes_the_kernels_path(role, block):
    N = _net()
    m, d = 5, 3
    net = randomised(N.CustomNet(4 if role == "host" else 3, [64, 32], (m, d), block_cls=getattr(N, block), role=role, seed=1), 2).cuda()
    e = net.extra_dim
    x = C.rows_with_counts(np.random.default_rng(52), np.arange(41) % (m + 1), m, d, e)
    rule = C.module_net(net, to_numpy)
    want = C.forward(x, rule, m, d, e)
    with torch.no_grad():
        assert net.fused_reason is None
        p, v = net(dev(x))
        assert net.fused_last_reason is None and p.shape == (41, net.output_size) and v.shape == (41, 1)
        raw = _ops().customnet_forward(dev(x), net._cached_plan(), raw_value=True)
        assert same_bits(p.cpu().numpy(), want[0]) and same_bits(raw[1].cpu().numpy(), want[1])
        tanh = np.tanh(want[1].astype(np.float64))
        assert float(np.abs(v[:, 0].cpu().numpy() - tanh).max()) <= TANH_BOUND_UNITS * C.M.UNIT
        plan = net.__dict__["_fused_plan"]
        assert net(dev(x).view(41, -1, d))[0].equal(p) and net.__dict__["_fused_plan"] is plan
        # torch's path on the same rows: within the CPU test's criterion of the reference's formula
        net.fused_enabled = False
        off = net(dev(x))
        assert net.fused_last_reason == "fused_enabled is False"
        net.fused_enabled = True
        p64, v64 = C.forward64(x, rule, m, d, e)
        e_torch = max(C.units(off[0].cpu().numpy(), p64), C.units(off[1][:, 0].cpu().numpy(), v64))
        e_rule = max(C.units(p.cpu().numpy(), p64), C.units(v[:, 0].cpu().numpy(), v64))
        print(f"{role}: E_torch {e_torch:.3g} E_fused {e_rule:.3g}")
        assert e_rule <= 2 * e_torch
    # with gradients on: torch's path, and backward fills the towers that had rows, and the heads
    rows = dev(x[(C.counts(x, m, d) == 1) | (C.counts(x, m, d) == 3) | (C.counts(x, m, d) == m)])
    p, v = net(rows)
    assert net.fused_last_reason == "gradients are on" and p.requires_grad
    (p.square().sum() + v.sum()).backward()
    for t, tower in enumerate(net.towers):
        got = any(bool(q.grad.abs().sum() > 0) for b in tower for q in b.parameters())
        assert got == (t in (1, 3)), t
    assert all(bool(q.grad.abs().sum() > 0) for q in list(net.Dense_0.parameters()) + list(net.Dense_1.parameters()))
    # in-place steps keep the table, a moved module builds a new one
    with torch.no_grad():
        for q in net.parameters():
            q.mul_(1.25)
        moved = net.cpu().cuda()
        p2 = moved(dev(x))[0]
        assert moved.__dict__["_fused_plan"] is not plan and moved.fused_last_reason is None
        assert same_bits(p2.cpu().numpy(), C.forward(x, C.module_net(moved, to_numpy), m, d, e)[0])


# ---- through HipTrainer -----------------------------------------------------------------------------------------------

def trainer_config(net_type):
    """the reference's test config (test/jax_config.yml: 5 points in dimension 3, [32, 32], adamw) shrunk to 8 games,
    4 evaluations and 3 moves"""
    section = {"batch_size": 8, "net_arch": [32, 32], "optim": {"name": "adamw", "args": {"learning_rate": 1e-3}}}
    return {"use_cuda": True, "scale_observation": True, "reposition": True, "gumbel_scale": 0.3, "version_string": "mcts",
            "net_type": net_type, "dimension": 3, "max_num_points": 5, "max_length_game": 3, "max_value": 20,
            "max_grad_norm": 1, "eval_batch_size": 8, "num_evaluations": 4, "num_evaluations_as_opponent": 2,
            "eval_on_cpu": False, "max_num_considered_actions": 10, "discount": 0.99,
            "host": dict(section), "agent": dict(section)}


@pytest.mark.parametrize("net_type", ["custom", "custom_dense"])
def test_trainer_simulates_and_trains(net_type):
    from hironaka_amd.functional import rollout_sanity_tests
    from hironaka_amd.trainer_api import HipTrainer
    N = _net()
    with pytest.raises(ValueError, match="CustomNet"):
        HipTrainer(42, trainer_config(net_type))
    t = HipTrainer(42, trainer_config(net_type), custom_net=True)
    u = HipTrainer(42, trainer_config(net_type), custom_net=True, fused_expand=False)
    block = N.DenseResidueBlock if net_type == "custom" else N.DenseBlock
    for role, (e, a) in {"host": (0, 4), "agent": (3, 3)}.items():
        net = t.built_nets[role]
        assert type(net) is N.CustomNet and all(type(b) is block for b in net.blocks) and len(net.blocks) == 10
        assert (net.extra_dim, net.output_size, net.net_arch) == (e, a, [32, 32]) and net.Dense_0.weight.is_cuda
        assert t.models[role].module is net
    rollouts = {}
    for role in ("host", "agent"):
        for unified in (False, True):
            exp = t.simulate(7, role, use_unified_tree=unified)
            # (the unified tree's states carry the agent's tail and its actions are the host's, whatever the role)
            in_dim = 18 if unified else t.input_dim[role]
            acts = 4 if unified else t.output_dim[role]
            assert exp[0].shape == (8 * 3, in_dim) and exp[1].shape == (8 * 3, acts) and exp[2].shape == (8 * 3,)
            assert rollout_sanity_tests(exp, (5, 3)) and torch.isfinite(exp[2]).all()
            for x, y in zip(exp, u.simulate(7, role, use_unified_tree=unified)):  # the fused expansions change nothing
                assert torch.equal(torch.nan_to_num(x, neginf=-1e30), torch.nan_to_num(y, neginf=-1e30)), (role, unified)
            if not unified:
                rollouts[role] = tuple(x.clone() for x in exp)
        assert t.built_nets[role].fused_last_reason is None
    for role in ("host", "agent"):
        params = list(t.built_nets[role].parameters())
        before = [p.detach().clone() for p in params]
        at = [p.data_ptr() for p in params]
        losses = t.train(5, role, 1, rollouts[role])
        assert losses.shape == (1,) and bool(torch.isfinite(losses).all())
        assert t.built_nets[role].fused_last_reason == "gradients are on"
        assert [p.data_ptr() for p in params] == at and any(not torch.equal(p, q) for p, q in zip(params, before))
