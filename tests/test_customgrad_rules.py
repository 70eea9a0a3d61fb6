"""tests/customgrad_rules.py, the rule of hk_customgrad_forward / hk_customgrad_backward in numpy: its forward is
customnet_rules', a tower without rows gets exact +0, a tower's gradients are pvgrad_rules' on its group's rows alone, and the
whole rule is pinned to torch on the CPU -- autograd through the reference's formula (all towers, the mask, the sum) --
within torch's own distance of a float64 run."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import customgrad_rules as CG
import customnet_rules as C
import pvgrad_rules as G
import pvnet_rules as R
from test_pvgrad_rules import units

F32 = np.float32


def _case(seed, spec, arch, actions, cs, kind="residue", **kw):
    rng = np.random.default_rng(seed)
    net = C.random_net(rng, *spec, arch, actions, kind, **kw)
    cs = np.asarray(cs)
    x = C.rows_with_counts(rng, cs, *spec)
    gp = (rng.standard_normal((len(cs), actions)) / len(cs)).astype(F32)
    gv = (rng.standard_normal(len(cs)) / len(cs)).astype(F32)
    return net, x, gp, gv


def test_forward_has_the_bits_of_customnet_rules():
    for seed, (spec, arch, kind) in enumerate([((5, 3, 3), [64, 32], "residue"), ((3, 2, 0), [17, 64], ["dense", "residue"]),
                                               ((1, 2, 2), [32], "residue")]):
        m = spec[0]
        cs = np.arange(23) % (m + 1)
        net, x, _, _ = _case(seed, spec, arch, 4, cs, kind)
        p, v, saved = CG.forward_saved(x, net, *spec)
        p0, v0 = C.forward(x, net, *spec)
        assert C.same_bits(p, p0) and C.same_bits(v, v0)
        assert np.array_equal(saved["c"], cs) and np.array_equal(saved["c"][saved["order"]], np.sort(cs))
        for t in range(m + 1):  # ascending row index inside a group
            assert np.all(np.diff(saved["order"][np.sort(cs) == t]) > 0)
        assert not saved["z"][cs == m, : arch[-1]].any()


def _all_plus_zero(pairs, prefix):
    got = [w for label, w in pairs if label.startswith(prefix)]
    return bool(got) and all(not w.any() and not np.signbit(w).any() for w in got)


def test_a_tower_without_rows_gets_exact_plus_zero():
    spec = (5, 3, 3)
    net, x, gp, gv = _case(3, spec, [64, 32], 3, [0, 1, 3, 4, 5] * 4)
    _, _, saved = CG.forward_saved(x, net, *spec)
    pairs = CG.param_grads(CG.backward(saved, net, gp, gv))
    assert _all_plus_zero(pairs, "tower2.")
    for t in (0, 1, 3, 4):
        assert dict(pairs)[f"tower{t}.block1.dense2.d_gn_bias"].any()  # (at 32 columns dz in front of a norm is zero)
    # rows without a tower alone: every tower at +0, the heads not
    net, x, gp, gv = _case(4, spec, [64, 32], 3, [5] * 9)
    _, _, saved = CG.forward_saved(x, net, *spec)
    pairs = CG.param_grads(CG.backward(saved, net, gp, gv))
    assert all(_all_plus_zero(pairs, f"tower{t}.") for t in range(5))
    heads = dict(pairs)
    assert heads["policy.d_weight"][:, 32:].any() and not heads["policy.d_weight"][:, :32].any()
    assert heads["policy.d_bias"].any() and heads["value.d_weight"].any() and heads["value.d_bias"].any()


def test_a_group_is_pvgrad_rules_on_its_rows_alone():
    """17 rows of one count in front of another group (e = 0, so that the heads are a pvnet's): tower t's gradients are
    pvgrad_rules.backward on that group's rows as a batch of their own, bit for bit"""
    spec = (5, 3, 0)
    cs = [4] * 2 + [1] * 9 + [3] * 4 + [1] * 8 + [4] * 3 + [5] * 2
    net, x, gp, gv = _case(5, spec, [64, 32], 4, cs)
    cs = np.asarray(cs)
    _, _, saved = CG.forward_saved(x, net, *spec)
    towers, policy, value = CG.backward(saved, net, gp, gv)
    assert (cs == 1).sum() == 17
    for t in (1, 3, 4):
        rows = np.nonzero(cs == t)[0]
        pv = R.Net(net.towers[t], net.policy, net.value)
        _, _, psaved = G.forward_saved(x[rows, : (t + 1) * 3], pv)
        want = G.param_grads(G.backward(psaved, pv, gp[rows], gv[rows]))
        got = CG.param_grads(([towers[t]], policy, value))
        trunk = [(label, w) for label, w in want if label.startswith("block")]
        assert len(trunk) == len(got) - 4
        for (label, w), (_, g) in zip(trunk, got):
            assert C.same_bits(g, w), (t, label)


def torch_grads(x, net, spec, gp, gv, dtype):
    """the parameter gradients, in customgrad_rules.param_grads' order, of sum(gp * policy) + sum(gv * tanh value) by torch's
    autograd on the reference's formula in `dtype`: every tower on every row, the one-hot of the count, the sum"""
    m, d, e = spec
    params = []

    def t(a):
        if a is None:
            return None
        p = torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True)
        params.append(p)
        return p

    def dn(dense, norm):
        return [t(dense[0]), t(dense[1])] + ([t(dense.gn_scale), t(dense.gn_bias)] if norm else [None, None])

    lin = lambda h, p: F.linear(h, p[0], p[1])  # noqa: E731
    gn = lambda z, p, eps: F.group_norm(z, R.GROUPS, p[2], p[3], eps=float(F32(eps)))  # noqa: E731
    xt = torch.from_numpy(x).to(dtype)
    extra = xt[:, m * d:]
    available = torch.from_numpy((C.counts(x, m, d)[:, None] == np.arange(m)[None, :])).to(dtype)
    outs = []
    for tower_index, tower in enumerate(net.towers):
        h = torch.cat([xt[:, : (tower_index + 1) * d], extra], dim=-1)
        for b in tower:
            res = b.kind == "residue"
            n, k = b.dense1.weight.shape
            d1 = dn(b.dense1, res)
            if not res:
                h = torch.relu(lin(h, d1))
                continue
            d2 = dn(b.dense2, True)
            dp = dn(b.proj, True) if k != n else None
            y = gn(lin(torch.relu(gn(lin(h, d1), d1, b.eps)), d2), d2, b.eps)
            h = torch.relu((h if dp is None else gn(lin(h, dp), dp, b.eps)) + y)
        outs.append(h)
    out = (torch.stack(outs, dim=-1) * available.unsqueeze(1)).sum(-1)
    z = torch.cat([out, extra], dim=-1)
    policy, value = dn(net.policy, False), dn(net.value, False)
    p, v = lin(z, policy), torch.tanh(lin(z, value))[:, 0]
    ((p * torch.from_numpy(gp).to(dtype)).sum() + (v * torch.from_numpy(gv).to(dtype)).sum()).backward()
    return [q.grad.numpy() for q in params]


NETS = [("same_width", [128, 128]), ("projection", [256, 128])]


@pytest.mark.parametrize("name,arch", NETS, ids=[n[0] for n in NETS])
def test_rule_lies_within_torchs_own_distance_of_float64(name, arch):
    """E_rule <= 2 * max(E_torch32, 1): E the largest over the parameter gradients of max |g - g64| in units of
    max |g64| * 2^-24 (test_pvgrad_rules.units), g64 from torch's autograd on a float64 copy of the reference's formula, E_torch
    the same formula in float32; the (3, 3) agent, 28 rows over every count, 3 actions, normed widths 128 and 256.
    Measured here (E_torch / E_rule): same_width 891 / 107, projection 29.9 / 39.2."""
    spec = (3, 3, 3)
    net, x, gp, gv = _case(sum(map(ord, name)), spec, arch, 3, np.arange(28) % 4)
    p, v, saved = CG.forward_saved(x, net, *spec)
    tanh_v = np.tanh(v.astype(np.float64)).astype(F32)
    rule = [g for _, g in CG.param_grads(CG.backward(saved, net, gp, CG.tanh_grad(gv, tanh_v)))]
    g64 = torch_grads(x, net, spec, gp, gv, torch.float64)
    g32 = torch_grads(x, net, spec, gp, gv, torch.float32)
    assert len(rule) == len(g64) == len(g32) and all(a.shape == b.shape for a, b in zip(rule, g64))
    largest = max(np.abs(r).max() for r in g64)
    e_torch = max(units(g, r, largest) for g, r in zip(g32, g64))
    e_rule = max(units(g, r, largest) for g, r in zip(rule, g64))
    print(f"{name}: E_torch {e_torch:.3g} E_rule {e_rule:.3g}")
    assert e_rule <= 2 * max(e_torch, 1)
