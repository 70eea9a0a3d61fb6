"""tests/pvgrad_rules.py, the rule of hk_pvgrad_forward / hk_pvgrad_backward in numpy: its forward is pvnet_rules', the group
norm's backward pinned by hand, a width of one column per group gives exact zeros, and the whole rule pinned to torch on the
CPU within torch's own distance of a float64 run."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pvgrad_rules as G
import pvnet_rules as R
from mlp_rules import UNIT

F32 = np.float32


def _case(seed, k0, arch, actions, rows, kind="residue", **kw):
    rng = np.random.default_rng(seed)
    net = R.random_net(rng, k0, arch, actions, kind, **kw)
    x = rng.uniform(-1, 1, (rows, k0)).astype(F32)
    gp = (rng.standard_normal((rows, actions)) / rows).astype(F32)
    gv = (rng.standard_normal(rows) / rows).astype(F32)
    return net, x, gp, gv


def test_forward_has_the_bits_of_pvnet_rules():
    for seed, (k0, arch, kind) in enumerate([(18, [64, 128], "residue"), (60, [128, 128, 32], "residue"),
                                             (7, [17, 64, 40], ["dense", "residue", "dense"])]):
        net, x, _, _ = _case(seed, k0, arch, 5, 9, kind)
        p, v, saved = G.forward_saved(x, net)
        p0, v0 = R.forward(x, net)
        assert R.same_bits(p, p0) and R.same_bits(v, v0)
        assert len(saved) == len(arch) and all(s["h"].shape == (9, n) for s, n in zip(saved, arch))
        assert R.same_bits(saved[-1]["h"], R.trunk(x, net.blocks))


def test_group_norm_backward_by_hand():
    """one row of width 128 (groups of four columns), eps = 0, every number exact in float32: z = (2, -2, 2, -2) has mean 0,
    variance 4, inv = 1/2, xhat = (1, -1, 1, -1); with e = (1, 2, 3, 6) and scale 2: u = (2, 4, 6, 12), m1 = 6,
    u * xhat = (2, -4, 6, -12), m2 = -2, dz = ((u - 6) + 2 xhat) / 2 = (-1, -2, 1, 2)"""
    z, e = np.zeros((1, 128), F32), np.zeros((1, 128), F32)
    z[0, 8:12], e[0, 8:12] = (2, -2, 2, -2), (1, 2, 3, 6)
    z[0, 124:], e[0, 124:] = (5, 1, 5, 1), (1, 2, 3, 6)  # another mean, the same d
    dense = R.Dense(np.zeros((128, 1), F32), None, np.full(128, 2, F32), np.zeros(128, F32))
    dz, d_scale, d_bias = G.gnb(e, z, dense, 0.0)
    for at in (8, 124):
        assert R.same_bits(dz[0, at:at + 4], np.array([-1, -2, 1, 2], F32))
        assert R.same_bits(d_scale[at:at + 4], np.array([1, -2, 3, -6], F32))  # e * xhat, one row
        assert R.same_bits(d_bias[at:at + 4], np.array([1, 2, 3, 6], F32))
    # a group whose columns are equal: d = 0, var = 0, inv = 1 / sqrt(eps): xhat = 0, dz = inv * (u - m1)
    z[:], e[:] = 0, 0
    z[0, :4], e[0, :4] = 3, (1, 2, 3, 6)
    dz, d_scale, _ = G.gnb(e, z, dense._replace(gn_scale=None), 0.25)
    assert R.same_bits(dz[0, :4], np.array([-4, -2, 0, 6], F32)) and not d_scale.any()


@pytest.mark.parametrize("arch", [[32], [32, 32]])
def test_one_column_per_group_gives_exact_zeros(arch):
    """width 32: g = 1, d = 0, xhat = 0 and u - m1 = 0 for every finite z, so dz and with it d_weight and d_bias of every
    normed Dense are exactly zero, and so is d_gn_scale = ROWSUM(e * 0); d_gn_bias = ROWSUM(e) is not"""
    net, x, gp, gv = _case(3, 18, arch, 4, 21)
    p, v, saved = G.forward_saved(x, net)
    blocks, policy, value = G.backward(saved, net, gp, gv)
    assert np.abs(policy["d_weight"]).max() > 0 and np.abs(value["d_bias"]).max() > 0
    for l, b in enumerate(blocks):
        for which in ("dense1", "dense2", "proj"):
            if b[which] is None:
                assert which == "proj" and l > 0
                continue
            assert not b[which]["d_weight"].any() and not b[which]["d_bias"].any() and not b[which]["d_gn_scale"].any()
            assert not np.signbit(b[which]["d_weight"]).any()
            # (dense1's e is da = relu'(a) * (dz2 . W2) = 0 here: dz2 is zero)
            assert (np.abs(b[which]["d_gn_bias"]).max() > 0) == (which != "dense1")


def torch_grads(x, net, gp, gv, dtype):
    """the parameter gradients, in pvgrad_rules.param_grads' order, of sum(gp * policy) + sum(gv * tanh value) by torch's
    autograd on the plain composition in `dtype`"""
    params = []

    def t(a):
        if a is None:
            return None
        p = torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True)
        params.append(p)
        return p

    def dn(d, norm):
        return [t(d[0]), t(d[1])] + ([t(d.gn_scale), t(d.gn_bias)] if norm else [None, None])

    blocks = []
    for b in net.blocks:
        res = b.kind == "residue"
        n, k = b.dense1.weight.shape
        blocks.append((b, dn(b.dense1, res), dn(b.dense2, True) if res else None, dn(b.proj, True) if res and k != n else None))
    policy, value = dn(net.policy, False), dn(net.value, False)
    lin = lambda h, d: F.linear(h, d[0], d[1])  # noqa: E731
    gn = lambda z, d, eps: F.group_norm(z, R.GROUPS, d[2], d[3], eps=float(F32(eps)))  # noqa: E731
    h = torch.from_numpy(x).to(dtype)
    for b, d1, d2, dp in blocks:
        if d2 is None:
            h = torch.relu(lin(h, d1))
            continue
        y = gn(lin(torch.relu(gn(lin(h, d1), d1, b.eps)), d2), d2, b.eps)
        h = torch.relu((h if dp is None else gn(lin(h, dp), dp, b.eps)) + y)
    p, v = lin(h, policy), torch.tanh(lin(h, value))[:, 0]
    ((p * torch.from_numpy(gp).to(dtype)).sum() + (v * torch.from_numpy(gv).to(dtype)).sum()).backward()
    return [q.grad.numpy() for q in params]


def units(g, g64, largest):
    """test_gpu_pv_loss._units: max |g - g64| in units of max |g64| * 2^-24, of the network's largest gradient where this
    tensor's own is zero in exact arithmetic"""
    own = np.abs(g64).max()
    scale = (own if own > largest * UNIT else largest) * UNIT
    err = np.abs(np.asarray(g, np.float64) - g64).max()
    return 0.0 if err == 0 else err / scale


NETS = [("same_width", 18, [128, 128]), ("projection", 60, [256, 128])]


@pytest.mark.parametrize("name,k0,arch", NETS, ids=[n[0] for n in NETS])
def test_rule_lies_within_torchs_own_distance_of_float64(name, k0, arch):
    """E_rule <= 2 * max(E_torch32, 1): E the largest over the parameter gradients of max |g - g64| in units of
    max |g64| * 2^-24, g64 from torch's autograd on a float64 copy of the plain composition; 21 rows, 4 actions, normed widths
    128 and 256 (at 32 and 64 the gradient in front of a norm is zero or pure rounding noise on both sides).
    Measured here (E_torch / E_rule): same_width 44.4 / 72.2, projection 85.7 / 58.1."""
    net, x, gp, gv = _case(sum(map(ord, name)), k0, arch, 4, 21)
    p, v, saved = G.forward_saved(x, net)
    tanh_v = np.tanh(v.astype(np.float64)).astype(F32)
    rule = [g for _, g in G.param_grads(G.backward(saved, net, gp, G.tanh_grad(gv, tanh_v)))]
    g64 = torch_grads(x, net, gp, gv, torch.float64)
    g32 = torch_grads(x, net, gp, gv, torch.float32)
    assert len(rule) == len(g64) == len(g32) and all(a.shape == b.shape for a, b in zip(rule, g64))
    largest = max(np.abs(r).max() for r in g64)
    e_torch = max(units(g, r, largest) for g, r in zip(g32, g64))
    e_rule = max(units(g, r, largest) for g, r in zip(rule, g64))
    print(f"{name}: E_torch {e_torch:.3g} E_rule {e_rule:.3g}")
    assert e_rule <= 2 * max(e_torch, 1)
