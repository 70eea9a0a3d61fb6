"""tests/customnet_rules.py, the rule of hk_customnet_forward in numpy: the choice of the tower pinned by hand, the rule
pinned to the reference's own formula (hironaka/jax/net.py:84-103: all towers, one-hot, product, sum) within torch's own
distance of a float64 evaluation; and hironaka_amd.net.CustomNet on the CPU."""
import numpy as np
import pytest
import torch

import customnet_rules as C
import pvnet_rules as R
from test_pvnet_rules import torch_forward as torch_trunk_forward

F32 = np.float32


def test_point_count_and_tower_by_hand():
    """a (3, 2) net with e = 2: rows with 0, 1, 2 and 3 points, a hole, and a NaN in a coordinate 0"""
    m, d, e = 3, 2, 2
    rng = np.random.default_rng(0)
    net = C.random_net(rng, m, d, e, [64, 64], 3)  # (groups of two columns: a width of 32 gives the bias alone)
    nan = np.nan
    x = np.array([[-1, -1, -1, -1, -1, -1, .5, .25],     # no point: tower 0 on (-1, -1) ++ extra
                  [.9, .1, -1, -1, -1, -1, .5, .25],     # one point: tower 1 on two points
                  [.9, .1, .4, .3, -1, -1, .5, .25],     # two points: tower 2 on all three
                  [.9, .1, .4, .3, .2, .7, .5, .25],     # three points: c == m, no tower
                  [.9, .1, -1, .3, .2, .7, .5, .25],     # a hole in the middle: c = 2, whatever the order
                  [nan, .1, .4, .3, -1, -1, .5, .25],    # a NaN does not count: c = 1
                  [0.0, .1, -0.0, .3, -1, -1, .5, .25]], F32)  # 0 and -0 are >= 0: c = 2
    assert list(C.counts(x, m, d)) == [0, 1, 2, 3, 2, 1, 2]
    p, v = C.forward(x, net, m, d, e)
    for b, t in ((0, 0), (1, 1), (2, 2), (4, 2), (5, 1), (6, 2)):
        u = np.concatenate([x[b: b + 1, : (t + 1) * d], x[b: b + 1, m * d:]], axis=1)
        z = np.concatenate([R.trunk(u, net.towers[t]), x[b: b + 1, m * d:]], axis=1)
        assert C.same_bits(p[b], R.M.linear(z, net.policy[0], net.policy[1])[0]), b
        assert C.same_bits(v[b], R.M.linear(z, net.value[0], net.value[1])[0, 0]), b
    # the row with every point: the heads on 0 ++ extra
    z = np.concatenate([np.zeros((1, 64), F32), x[3: 4, m * d:]], axis=1)
    assert C.same_bits(p[3], R.M.linear(z, net.policy[0], net.policy[1])[0])
    assert C.same_bits(v[3], R.M.linear(z, net.value[0], net.value[1])[0, 0])
    assert np.isnan(p[5]).all() and np.isfinite(np.delete(p, 5, axis=0)).all()  # tower 1 reads the NaN: its row alone
    # the rows differ: no two towers gave the same result
    assert len({p[b].tobytes() for b in range(5)}) == 5


def torch_reference(x, net, m, d, e, dtype):
    """a torch transcription of hironaka/jax/net.py:84-103 on the rule's parameters"""
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(dtype)  # noqa: E731
    x = t(x)
    x = x.reshape((*x.shape[:-1], -1, d))
    count = torch.sum(x[..., :m, 0] >= 0, dim=-1)
    available = (count.unsqueeze(-1) == torch.arange(m)).to(dtype)  # jax.nn.one_hot(count, m): all zero at count == m
    extra = x[..., m:, :].reshape((*x.shape[:-2], -1))
    outs = []
    n = C.n_last(net)
    for i in range(m):
        out = torch.cat([x[..., : i + 1, :].reshape((*x.shape[:-2], -1)), extra], dim=-1)
        # (the trunk as test_pvnet_rules.py transcribes it, read off behind an identity head)
        identity = R.Net(net.towers[i], (np.eye(n, dtype=np.float64), None), (np.zeros((1, n)), None))
        outs.append(torch.from_numpy(torch_trunk_forward(out.numpy(), identity, dtype)[0]))
    out = torch.sum(torch.stack(outs, dim=-1) * available[..., None, :], dim=-1)
    features = torch.cat([out, extra], dim=-1)
    lin = lambda head: torch.nn.functional.linear(features, t(head[0]), t(head[1]))  # noqa: E731
    return lin(net.policy).numpy(), torch.tanh(lin(net.value))[:, 0].numpy()


# (name, m, d, e, block widths, kind, actions): the reference's test config under both roles, its training config's
# dense towers, and 20 points with a block that changes its width
NETS = [
    ("test_host", 5, 3, 0, [32, 32], "residue", 4),
    ("test_agent", 5, 3, 3, [32, 32], "residue", 3),
    ("dense_agent", 5, 3, 3, [128, 128], "dense", 3),
    ("twenty_agent", 20, 3, 3, [64, 32], "residue", 3),
]
ROWS = 48


@pytest.mark.parametrize("case", NETS, ids=[c[0] for c in NETS])
def test_rule_lies_within_torchs_own_distance_of_the_references_formula(case):
    """forward64 IS the reference's formula (a float64 torch transcription of net.py:84-103 agrees to rtol 1e-9), and
    E_rule <= 2 * E_torch against it, both in units of max |y64| * 2^-24 (mlp_rules.units), the larger of the policy's and
    the value's, on 48 rows whose counts cover every value 0..m; E_torch is the float32 transcription's -- all towers,
    mask, sum.  Measured here (E_torch / E_rule):
        test_host 1230 / 1.58     test_agent 410 / 1.12     dense_agent 3.66 / 5.2     twenty_agent 564 / 1.9
    (at a normed width of 32 a group is one column: the rule gives the bias exactly and torch's fused group norm keeps
    its rounding, as test_pvnet_rules.py explains)."""
    name, m, d, e, arch, kind, actions = case
    rng = np.random.default_rng(sum(map(ord, name)))
    net = C.random_net(rng, m, d, e, arch, actions, kind)
    cs = np.arange(ROWS) % (m + 1)
    x = C.rows_with_counts(rng, cs, m, d, e)
    assert sorted(set(C.counts(x, m, d))) == list(range(m + 1))
    p, v = C.forward(x, net, m, d, e)
    v = np.tanh(v.astype(np.float64)).astype(F32)
    p64, v64 = C.forward64(x, net, m, d, e)
    t64 = torch_reference(x, net, m, d, e, torch.float64)
    assert np.allclose(t64[0], p64, rtol=1e-9, atol=1e-11) and np.allclose(t64[1], v64, rtol=1e-9, atol=1e-11)
    pt, vt = torch_reference(x, net, m, d, e, torch.float32)
    e_torch = max(C.units(pt, p64), C.units(vt, v64))
    e_rule = max(C.units(p, p64), C.units(v, v64))
    print(f"{name}: E_torch {e_torch:.3g} E_rule {e_rule:.3g}")
    assert e_rule <= 2 * e_torch


# ---- hironaka_amd.net.CustomNet on the CPU ----------------------------------------------------------------------------

def to_numpy(t):
    return None if t is None else t.detach().cpu().numpy()


def randomised(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.add_(torch.rand(p.shape, generator=g) - 0.5)
    return net


@pytest.mark.parametrize("role,block", [("host", "DenseResidueBlock"), ("agent", "DenseBlock")])
def test_the_module_is_the_references_formula(role, block):
    from hironaka_amd import net as N
    m, d = 4, 3
    e = d if role == "agent" else 0
    module = randomised(N.CustomNet(2 ** d - d - 1 if role == "host" else d, [64, 32], (m, d), block_cls=getattr(N, block),
                                    role=role, seed=3), 4).double()
    assert not isinstance(module, N.DenseResNet) and module.extra_dim == e and module.input_dim == m * d + e
    # flax's compact auto-names: tower t's block l is <block>_{t L + l}; the heads Dense_0 (n_last + e inputs), Dense_1
    names = [name for name, _ in module.named_children()]
    assert names == [f"{block}_{i}" for i in range(m * 2)] + ["Dense_0", "Dense_1"]
    for t, tower in enumerate(module.towers):
        assert [type(b).__name__ for b in tower] == [block] * 2 and tower[0] is getattr(module, f"{block}_{2 * t}")
        assert tower[0].Dense_0.in_features == (t + 1) * d + e and tower[1].Dense_0.in_features == 64
    assert module.Dense_0.in_features == module.Dense_1.in_features == 32 + e and module.Dense_1.out_features == 1
    rng = np.random.default_rng(5)
    x = C.rows_with_counts(rng, np.arange(30) % (m + 1), m, d, e)
    want = torch_reference(x, C.module_net(module, to_numpy), m, d, e, torch.float64)
    p, v = module.plain_forward(torch.from_numpy(x).double())
    assert p.requires_grad and v.shape == (30, 1)
    # (the transcription carries eps as the float the rule carries, 1e-6 rounded to float32, the module as a double: a
    # relative 3e-9 of eps, half of that in 1 / sqrt(var + eps) where the variance is zero)
    assert np.allclose(p.detach().numpy(), want[0], rtol=1e-7, atol=1e-9)
    assert np.allclose(v.detach().numpy()[:, 0], want[1], rtol=1e-7, atol=1e-9)
    got = module(torch.from_numpy(x).double().view(30, -1, d))  # forward on the CPU is plain_forward, and says why
    assert torch.equal(got[0], p) and module.fused_last_reason is not None


def test_parameters_seeds_and_flax_trees():
    from hironaka_amd import net as N
    make = lambda seed: N.CustomNet(3, [32, 32], (5, 3), role="agent", seed=seed)  # noqa: E731
    a, b, c = make(1), make(1), make(2)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert not torch.equal(a.Dense_0.weight, c.Dense_0.weight)
    assert all(not bool(p.any()) for name, p in a.named_parameters() if name.endswith("Dense_0.bias"))  # zero biases
    randomised(a, 6)
    tree = a.flax_params()
    assert set(tree["params"]) == {f"DenseResidueBlock_{i}" for i in range(10)} | {"Dense_0", "Dense_1"}
    assert tree["params"]["DenseResidueBlock_2"]["Dense_0"]["kernel"].shape == (2 * 3 + 3, 32)  # tower 1: two points
    assert set(tree["params"]["DenseResidueBlock_0"]) == {"Dense_0", "GroupNorm_0", "Dense_1", "GroupNorm_1", "res_proj", "norm_proj"}
    assert tree["params"]["Dense_0"]["kernel"].shape == (32 + 3, 3)
    c.load_flax_params(tree)
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), c.parameters()))
    with pytest.raises(KeyError):
        c.load_flax_params({k: v for k, v in tree["params"].items() if k != "DenseResidueBlock_9"})
    with pytest.raises(ValueError):
        N.CustomNet(3, [32], (5, 3))  # neither extra_dim nor role
    assert N.CustomNet(3, [32], (5, 3), extra_dim=7).input_dim == 22


def test_build_net_builds_it_behind_the_flag():
    from hironaka_amd import net as N
    custom = N.build_net("custom", "host", 4, [32, 32], (5, 3), seed=1, custom_net=True)
    dense = N.build_net("custom_dense", "agent", 3, [40, 24], (5, 3), seed=1, custom_net=True)
    assert type(custom) is N.CustomNet and all(type(b) is N.DenseResidueBlock for b in custom.blocks)
    assert type(dense) is N.CustomNet and all(type(b) is N.DenseBlock for b in dense.blocks)
    assert (custom.extra_dim, dense.extra_dim, len(custom.blocks), dense.net_arch) == (0, 3, 10, [40, 24])
    assert type(N.build_net("dense", "host", 4, [32], (5, 3), custom_net=True)).__name__ == "DenseResNet"
    for net_type in ("custom", "custom_dense"):
        with pytest.raises(ValueError, match="CustomNet"):
            N.build_net(net_type, "host", 4, [32], (5, 3), custom_net=False)


def test_shapes_beyond_the_limits_give_a_reason():
    from hironaka_amd import net as N
    with torch.no_grad():
        assert N.CustomNet(3, [32, 32], (5, 3), role="agent").fused_reason is None
        assert "width" in N.CustomNet(3, [512], (5, 3), role="agent", block_cls=N.DenseBlock).fused_reason
        assert "width" in N.CustomNet(3, [32], (64, 5), role="host").fused_reason                  # m d + e > 256
        assert "width" in N.CustomNet(3, [256], (5, 3), role="agent").fused_reason                 # n_last + e > 256
        assert "normed" in N.CustomNet(3, [96], (5, 3), role="agent").fused_reason
        assert "points" in N.CustomNet(3, [32], (65, 2), role="host").fused_reason
        assert "coordinates" in N.CustomNet(3, [32], (5, 1), role="host").fused_reason
        assert "blocks" in N.CustomNet(3, [8] * 33, (2, 2), role="host", block_cls=N.DenseBlock).fused_reason
        off = N.CustomNet(3, [32], (5, 3), role="host")
        off.fused_enabled = False
        assert off.fused_reason == "fused_enabled is False"
    net = N.CustomNet(3, [32], (5, 3), role="host")
    net.fused_training = True  # HipTrainer sets it; it changes nothing
    assert net.fused_reason == "gradients are on"
    x = torch.from_numpy(C.rows_with_counts(np.random.default_rng(7), [0, 2, 5], 5, 3, 0))
    p, v = net(x)
    (p.sum() + v.sum()).backward()
    assert net.fused_last_reason == "gradients are on"
    grads = [any(q.grad is not None and bool(q.grad.abs().sum() > 0) for q in b.parameters()) for b in net.blocks]
    assert grads == [True, False, True, False, False]  # the towers that had rows: counts 0 and 2; 5 == m has none
    assert bool(net.Dense_0.weight.grad.abs().sum() > 0) and bool(net.Dense_1.weight.grad.abs().sum() > 0)
