"""CPU-side checks of the rule of hk_train_mlp_forward / hk_train_mlp_backward (tests/mlp_train_rules.py): its two sums
are the header's orders, it lies within the project's bound of torch's own training forward and backward
(tests/golden/mlp_train.npz), and nets.FusedSequential.fused_training names what is in its way -- and changes nothing
while it is off."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import mlp_rules as R
import mlp_train_rules as T
from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import nets

F32 = np.float32


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "mlp_train.npz"))


def test_rowsum_and_chain_are_the_headers_orders():
    rng = np.random.default_rng(1)
    for rows in (1, 2, 15, 16, 17, 40, 257):
        v = (rng.standard_normal(rows) * 2.0 ** rng.integers(-20, 20, rows)).astype(F32)
        p = [F32(0)] * 16
        for b in range(rows):
            p[b % 16] = F32(p[b % 16] + v[b])
        q = [F32(p[i] + p[i + 8]) for i in range(8)]
        r = [F32(q[i] + q[i + 4]) for i in range(4)]
        s = [F32(r[i] + r[i + 2]) for i in range(2)]
        assert T.rowsum(v[:, None])[0].tobytes() == F32(s[0] + s[1]).tobytes()
    # a chain that ends in -0 stays -0 at a multiple of 16 terms and becomes +0 otherwise
    for k, sign in ((16, True), (32, True), (15, False), (17, False), (1, False)):
        z = T.linear(np.full((2, k), -0.0, F32), np.ones((3, k), F32), np.full(3, -0.0, F32))
        assert np.signbit(z).all() == sign and not z.any()
    # the running statistics move by momentum, the variance unbiased
    layers = T.random_layers(rng, (4, 3), momentum=0.25)
    x = rng.standard_normal((5, 4)).astype(F32)
    _, saved, stats = T.forward(x, layers)
    z = saved[0]["z"].astype(np.float64)
    assert np.allclose(stats[0][0], 0.75 * layers[0].bn_mean + 0.25 * z.mean(0), rtol=1e-6)
    assert np.allclose(stats[0][1], 0.75 * layers[0].bn_var + 0.25 * z.var(0, ddof=1), rtol=1e-6)
    assert np.allclose(saved[0]["inv"], 1 / np.sqrt(z.var(0) + 1e-5), rtol=1e-6)


@pytest.mark.parametrize("key", list(T.CASES))
def test_rule_lies_within_the_bound_of_torch(fixture, key):
    """E_rule <= 8 * max(E_torch, 1) for the output, every gradient and every running statistic, E in units of
    max |v64| * 2^-24 against torch's float64 run (the bias gradient of a Linear in front of a batch norm, zero in exact
    arithmetic, in the units of that Linear's weight gradient).  Recorded, largest E_torch / largest E_rule / worst
    E_rule : max(E_torch, 1) over the tensors: test at 256 rows 11.8 / 19.3 / 1.96, example at 256 rows
    716 953 / 1 021 158 / 3.19 (22 batch norms deep, the gradients of these seeded weights are ill-conditioned in torch
    itself: its float32 run is 4 % off its float64 run), deep at 64 rows 16.2 / 17.5 / 1.20, plain at 17 rows
    5.30 / 5.47 / 1.59."""
    seed = int(fixture[f"{key}_seed"])
    net = T.seeded_net(T.CASES[key][0], "host", seed)
    points, grad = T.case_inputs(key, seed + 1)
    r64 = T.torch_run(net, points, grad, torch.float64)
    r32 = T.torch_run(net, points, grad, torch.float32)
    assert [k for k, _ in r64] == list(fixture[f"{key}_names"])
    if key == "test_256":
        for (k, v32), (_, v64) in zip(r32, r64):
            assert v32.tobytes() == fixture[f"{key}_32_{k}"].tobytes(), k
            assert v64.tobytes() == fixture[f"{key}_64_{k}"].tobytes(), k
    rule = T.rule_run(net, points, grad)
    assert [k for k, _ in rule] == [k for k, _ in r64]
    e_torch, e_rule = T.case_units(r32, r64), T.case_units(rule, r64)
    worst = max(r / max(t, 1) for r, t in zip(e_rule, e_torch))
    print(f"{key}: max E_torch {max(e_torch):.2f} max E_rule {max(e_rule):.2f} worst ratio {worst:.2f}")
    assert e_torch == list(fixture[f"{key}_e_torch"]) and e_rule == list(fixture[f"{key}_e_rule"])
    for (k, _), t, r in zip(r64, e_torch, e_rule):
        assert r <= 8 * max(t, 1), (k, r, t)


def test_reasons_with_the_switch_on():
    head = nets.HostFeatureExtractor(60)
    make = lambda arch, **kw: nets.create_mlp(head, arch, 60, 4, fused_training=True, **kw)  # noqa: E731
    net = make([16, "b", 16])
    assert net.fused_training and not nets.create_mlp(head, [16], 60, 4).fused_training
    assert nets.fuse(nn.Sequential(*net.children()), training=True).fused_training
    assert not nets.fuse(nn.Sequential(*net.children())).fused_training and not nets.FusedSequential.fused_training
    assert net.fused_reason is None  # training mode, gradients on: the training kernels'
    with torch.no_grad():
        assert net.fused_reason is None  # a target net left in training mode
    net.eval()
    assert net.fused_reason == "gradients are on"  # running statistics and a backward: torch's
    with torch.no_grad():
        assert net.fused_reason is None
    assert make([16]).fused_reason is None and make([16]).eval().fused_reason is None  # no batch norm: either mode
    assert make(["b", 16]).fused_reason == "a BatchNorm1d on the input in training mode"
    with torch.no_grad():
        assert make(["b", 16]).eval().fused_reason is None
    none = make([16, "b"])
    none[3].momentum = None
    assert none.fused_reason == "a BatchNorm1d with momentum=None in training mode"
    bn = make([16, "b"])
    bn[3].track_running_stats, bn[3].running_mean, bn[3].running_var = False, None, None
    assert "running statistics" in bn.fused_reason
    assert "ResidualBlock" in make([16, "r16"]).fused_reason
    assert "float32" in make([16, "b"]).double().fused_reason
    assert "Tanh" in make([16], activation_fn=nn.Tanh).fused_reason
    assert "wider" in make([257]).fused_reason and "more than 32" in make([8] * 32).fused_reason
    lin = nn.Linear(4, 4)
    twice = nets.fuse(nn.Sequential(nn.Linear(6, 4), nn.ReLU(), lin, nn.ReLU(), lin), training=True)
    assert twice.fused_reason == "a parameter is used twice and gradients are on"
    with torch.no_grad():
        assert twice.fused_reason is None
    off = make([16, "b"])
    off.fused_enabled = False
    assert off.fused_reason == "fused_enabled is False"
    # on the CPU the call is nn.Sequential's, and says so
    x = torch.zeros(3, 20, 3)
    y = net.train()(x)
    assert "not on a HIP device" in net.fused_last_reason and y.requires_grad
    plain = nn.Sequential(*net.children())
    assert torch.equal(net(x), plain(x))
    # deepcopy and pickling keep the switch and drop the tables
    import copy
    import pickle
    assert copy.deepcopy(net).fused_training and pickle.loads(pickle.dumps(net)).fused_training


def test_switch_off_is_todays_reasons():
    head = nets.HostFeatureExtractor(60)
    net = nets.create_mlp(head, [16, "b", 16], 60, 4)
    assert not net.fused_training
    assert net.fused_reason == "a BatchNorm1d in training mode"
    net(torch.zeros(2, 20, 3))
    assert net.fused_last_reason == "a BatchNorm1d in training mode"
    net.eval()
    assert net.fused_reason == "gradients are on"
    net(torch.zeros(2, 20, 3))
    assert net.fused_last_reason == "gradients are on"
    with torch.no_grad():
        assert net.fused_reason is None
        net(torch.zeros(2, 20, 3))
        assert "not on a HIP device" in net.fused_last_reason
        assert nets.create_mlp(head, [16], 60, 4).train().fused_reason is None
    assert nets.create_mlp(head, [16], 60, 4).fused_reason == "gradients are on"
    assert A.HK_MLP_TRAIN_MAX_BATCH >= 256
