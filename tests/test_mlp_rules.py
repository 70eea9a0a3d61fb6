"""CPU-side checks of the rule of hk_mlp_forward (tests/mlp_rules.py): its vectorised fma is dqn_rules.fma_exact to the
bit, hironaka_amd.nets.create_mlp builds what the reference's does (tests/golden/mlp_nets.npz), and the rule lies within
a measured distance of torch."""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

import dqn_rules as D
import mlp_rules as R
from conftest import GOLDEN
from hironaka_amd import nets

F32 = np.float32
KEYS = [f"{name}_{head}" for name in R.NET_ARCHS for head in R.HEADS]


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "mlp_nets.npz"))


def _tie_cases(rng, n):
    """a * b + c within 2^-50 relative of a float32 midpoint, on either side of it.  a = 1 + i 2^-23 and b = 1 - i 2^-23
    multiply to 1 - i^2 2^-46 exactly; C is an even integer of [2^24, 2^25), where float32 holds the even integers and
    C +- 1 are midpoints.  c = +C puts the sum i^2 2^-46 below the midpoint C + 1, c = -C puts its magnitude as much
    above the midpoint C - 1: i^2 2^-70 relative, i <= 1024.  Below i = 362 the distance is under half an ulp of the
    double sum, which then IS the midpoint and ties to even -- wrongly for one parity of C / 2.  Everything is scaled
    by powers of two."""
    i = rng.integers(1, 1025, n)
    i[:64] = np.arange(1, 65)
    a = (1 + i * 2.0 ** -23).astype(F32)
    b = (1 - i * 2.0 ** -23).astype(F32)
    c = (2.0 ** 24 + 2 * rng.integers(1, 2 ** 23 - 1, n)) * rng.choice([-1.0, 1.0], n)
    sa, sb = 2.0 ** rng.integers(-20, 20, n), 2.0 ** rng.integers(-20, 20, n)
    a, b, c = (a * sa).astype(F32), (b * sb).astype(F32), (c * sa * sb).astype(F32)
    exact = a.astype(np.float64) * b.astype(np.float64)  # 48 bits: exact
    assert (np.abs(exact / (sa * sb) - 1) == (i * 2.0 ** -23) ** 2).all() and (c.astype(np.float64) % (2 * sa * sb) == 0).all()
    return a, b, c


def test_fma32_is_fma_exact():
    rng = np.random.default_rng(1)
    n = 4000
    e = lambda: (rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)).astype(F32)  # noqa: E731
    a, b, c = e(), e(), e()
    # sums that cancel, zeros, infinities and NaNs
    c[:400] = -(a[:400].astype(np.float64) * b[:400]).astype(F32)
    a[400:420], c[420:440] = 0, 0
    a[440:445], c[445:450], b[450:455] = np.inf, -np.inf, np.nan
    ta, tb, tc = _tie_cases(rng, 2000)
    a, b, c = np.concatenate([a, ta]), np.concatenate([b, tb]), np.concatenate([c, tc])
    want = np.array([D.fma_exact(x, y, z, F32) for x, y, z in zip(a, b, c)], dtype=F32)
    assert R.same_bits(R.fma32(a, b, c), want)
    twice = R.fma32_twice(a, b, c)
    wrong = (twice.view(np.uint32) != want.view(np.uint32)) & ~np.isnan(want)
    assert wrong[n:].sum() > 100, "the constructed ties do not tell the double-rounding form from an fma"
    # scalars and broadcasting
    assert R.fma32(F32(3), F32(5), F32(-15)).tobytes() == F32(0).tobytes()
    assert R.fma32(a[:6, None], b[None, :5], c[:5]).shape == (6, 5)


def _ours(fixture, key):
    name, head = key.rsplit("_", 1)
    input_dim, output_dim = R.HEADS[head]
    extractor = nets.HostFeatureExtractor if head == "host" else nets.AgentFeatureExtractor
    net = nets.create_mlp(extractor(input_dim), json.loads(str(fixture[f"{key}_arch"])), input_dim, output_dim)
    shapes = json.loads(str(fixture[f"{key}_shapes"]))
    return net, shapes, R.seeded_state(shapes, int(fixture[f"{key}_seed"]))


def _input(fixture, key, dtype=torch.float32):
    points = torch.from_numpy(fixture[f"{key}_points"]).to(dtype)
    if key.endswith("_host"):
        return points
    return {"points": points, "coords": torch.from_numpy(fixture[f"{key}_coords"]).to(dtype)}


@pytest.mark.parametrize("key", KEYS)
def test_create_mlp_builds_the_references_net(fixture, key):
    net, shapes, state = _ours(fixture, key)
    assert isinstance(net, nets.FusedSequential) and isinstance(net, nn.Sequential)
    assert [type(m).__name__ for m in net.children()] == json.loads(str(fixture[f"{key}_children"]))
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == shapes
    assert nets.expand_net_list(R.NET_ARCHS[key.rsplit("_", 1)[0]]) == nets.expand_net_list(
        json.loads(str(fixture[f"{key}_arch"])))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    net.eval()
    with torch.no_grad():
        assert (net.fused_reason is None) == (key.rsplit("_", 1)[0] not in R.RESIDUAL), net.fused_reason
        # on the CPU the forward is nn.Sequential's: the reference's recorded outputs to the bit
        y32 = net(_input(fixture, key)).numpy()
        y64 = net.double()(_input(fixture, key, torch.float64)).numpy()
    assert y32.tobytes() == fixture[f"{key}_y32"].tobytes() and y64.tobytes() == fixture[f"{key}_y64"].tobytes()
    fused = nets.fuse(nn.Sequential(*net.children()))
    assert list(fused.children()) == list(net.children()) and list(fused.state_dict()) == list(net.state_dict())


def test_fused_reason_names_what_is_in_the_way():
    head = nets.HostFeatureExtractor(60)
    net = nets.create_mlp(head, [16, "b", 16], 60, 4)
    assert net.fused_reason == "a BatchNorm1d in training mode"
    net.eval()
    assert net.fused_reason == "gradients are on"
    with torch.no_grad():
        assert net.fused_reason is None
        assert nets.create_mlp(head, [16], 60, 4).train().fused_reason is None  # no batch norm: the mode is no matter
        assert "float32" in net.double().fused_reason
        assert "Tanh" in nets.create_mlp(head, [16], 60, 4, activation_fn=nn.Tanh).fused_reason
        assert "wider" in nets.create_mlp(head, [257], 60, 4).fused_reason
        assert "more than 32" in nets.create_mlp(head, [8] * 32, 60, 4).fused_reason
        assert nets.create_mlp(head, [8] * 31, 60, 4).fused_reason is None
        bn = nets.create_mlp(head, [16, "b"], 60, 4).eval()
        bn[3].track_running_stats, bn[3].running_mean, bn[3].running_var = False, None, None
        assert "running statistics" in bn.fused_reason
    frozen = nets.create_mlp(head, [16], 60, 4).requires_grad_(False)
    assert frozen.fused_reason is None  # gradients are on, but no parameter wants one


@pytest.mark.parametrize("key", [k for k in KEYS if k.rsplit("_", 1)[0] not in R.RESIDUAL])
def test_rule_lies_within_the_measured_distance_of_torch(fixture, key):
    """E_rule <= 8 * max(E_torch, 1) in units of max |y64| * 2^-24: the rule is one sequential chain over up to 256
    terms where torch's CPU GEMM adds blocked partial sums; a chain's rounding error grows with the square root of its
    length, so a few times torch's is expected.  Recorded: E_torch / E_rule 13.2 / 10.1 and 23.1 / 14.4 on 8 x 256,
    31.8 / 49.0 and 35.3 / 32.3 on the example config, 3.1 / 2.6 and 3.5 / 2.9 on the test config."""
    net, _, state = _ours(fixture, key)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    layers, input_relu, input_bn = R.spec_layers(nets.mlp_spec(net), lambda t: None if t is None else t.detach().numpy())
    x = fixture[f"{key}_points"].reshape(R.ROWS, -1)
    if key.endswith("_agent"):
        x = np.concatenate([x, fixture[f"{key}_coords"]], axis=1)
    y = R.forward(x, layers, input_relu, input_bn)
    y64 = fixture[f"{key}_y64"]
    e_torch, e_rule = R.units(fixture[f"{key}_y32"], y64), R.units(y, y64)
    print(f"{key}: E_torch {e_torch:.2f} E_rule {e_rule:.2f}")
    assert e_torch == float(fixture[f"{key}_e_torch"]) and e_rule == float(fixture[f"{key}_e_rule"])
    assert e_rule <= 8 * max(e_torch, 1)
    assert (y.argmax(1) == y64.argmax(1)).all()


def test_a_module_used_twice_keeps_both_places():
    """one activation instance in several slots: nn.Sequential.forward runs every slot, so the spec reads every slot and
    fuse keeps every slot"""
    torch.manual_seed(3)
    act = nn.ReLU()
    plain = nn.Sequential(nn.Linear(6, 5), act, nn.Linear(5, 4), act, nn.Linear(4, 3))
    x = torch.randn(7, 6)
    with torch.no_grad():
        for net in (nets.fuse(plain), nets.FusedSequential(*plain)):
            assert len(net) == len(plain) == 5 and list(net.state_dict()) == list(plain.state_dict())
            assert [id(m) for m in net] == [id(m) for m in plain]
            assert torch.equal(net(x), plain(x))
            assert net.fused_reason is None
            spec = nets.mlp_spec(net)
            assert [relu for _, _, relu in spec.blocks] == [True, True, False] and not spec.input_relu
        # the rule on that spec is the stack's forward within float32 rounding
        layers, input_relu, input_bn = R.spec_layers(spec, lambda t: None if t is None else t.detach().numpy())
        assert np.allclose(R.forward(x.numpy(), layers, input_relu, input_bn), plain(x).numpy(), rtol=1e-5, atol=1e-6)
        # a Linear used twice is two layers on one weight
        lin = nn.Linear(4, 4)
        twice = nets.FusedSequential(nn.Linear(6, 4), act, lin, act, lin)
        assert len(nets.mlp_spec(twice).blocks) == 3 and len(nets.fuse(twice)) == 5


def test_the_last_calls_reason():
    net = nets.create_mlp(nets.HostFeatureExtractor(60), [16], 60, 4).eval()
    assert net.fused_last_reason is None
    with torch.no_grad():
        net(torch.zeros(2, 20, 3))
        assert net.fused_reason is None and "not on a HIP device" in net.fused_last_reason
    net(torch.zeros(2, 20, 3))
    assert net.fused_last_reason == "gradients are on"


def test_expand_net_list():
    assert nets.expand_net_list([]) == []
    assert nets.expand_net_list([1, "b", {"repeat": 2, "net_arch": [2, {"repeat": 2, "net_arch": ["b"]}]}, 3]) == [
        1, "b", 2, "b", "b", 2, "b", "b", 3]
    assert nets.expand_net_list([{"repeat": 0, "net_arch": [5]}]) == []
    for bad in ([{"repeat": 2}], [{"net_arch": [1]}], [{"repeat": 2, "net_arch": 5}]):
        with pytest.raises(AssertionError):
            nets.expand_net_list(bad)
    with pytest.raises(AssertionError):
        nets.create_mlp(nn.Flatten(), ["x"], 4, 2)
    with pytest.raises(AssertionError):
        nets.create_mlp(nn.Flatten(), ["r0"], 4, 2)
