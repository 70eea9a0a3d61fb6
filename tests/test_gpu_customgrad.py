"""hk_customgrad_forward / hk_customgrad_backward on the device against tests/customgrad_rules.py (which
test_customgrad_rules.py pins to pvgrad_rules on a group's rows alone and, within torch's own distance of float64, to the
reference's formula): policy, raw value and EVERY gradient bit for bit, a tower without rows at exact +0.  Finite inputs
only.  Every case asserts that its inputs hold the point counts it claims to cover.  The shapes are the smallest that reach
every path: both block kinds, a projection and none in the first block (a tower whose input is as wide as the block),
groups on both sides of the 16-row chain step in front of another group, more towers than rows, more than one row tile."""
import ctypes

import numpy as np
import pytest
import torch

import customgrad_rules as CG
import customnet_rules as C
from hironaka_amd import _abi as A
from test_gpu_customnet import device_plan
from test_gpu_mlp import SENTINEL, Guarded, dev

pytestmark = pytest.mark.gpu
same_bits = C.same_bits
F32 = np.float32


def _ops():
    from hironaka_amd import ops
    return ops


def grads_in(rng, batch, actions):
    """gradients at the outputs of the size a mean over the batch gives, with a few zeros"""
    gp = (rng.standard_normal((batch, actions)) / batch).astype(F32)
    gp[rng.random((batch, actions)) < 0.05] = 0
    return gp, (rng.standard_normal(batch) / batch).astype(F32)


def rule(x, net, spec, gp, gv):
    """(policy, raw value, [(label, gradient)]) by the rule, gv being the gradient at the raw value"""
    p, v, saved = CG.forward_saved(x, net, *spec)
    return p, v, CG.param_grads(CG.backward(saved, net, gp, gv))


def compare(got, want, where):
    p, v, grads = got
    assert same_bits(p.cpu().numpy(), want[0]), (where, "policy")
    assert same_bits(v.cpu().numpy(), want[1]), (where, "value")
    assert len(grads) == len(want[2])
    for g, (label, w) in zip(grads, want[2]):
        assert tuple(g.shape) == w.shape and same_bits(g.cpu().numpy(), w), (where, label)


def check(cs, spec, arch, kind, actions, seed, holes=False, where=None):
    """rows of the point counts `cs` through a random net of the shape: the kernels against the rule"""
    ops = _ops()
    m, d, e = spec
    rng = np.random.default_rng(seed)
    net = C.random_net(rng, m, d, e, arch, actions, kind)
    cs = np.asarray(cs)
    x = C.rows_with_counts(rng, cs, m, d, e, holes=holes)
    assert np.array_equal(C.counts(x, m, d), cs), where
    gp, gv = grads_in(rng, len(cs), actions)
    plan = device_plan(net, m, d, e)
    p, v, saved = ops.customnet_train_forward(dev(x), plan, raw_value=True)
    grads = ops.customnet_backward(saved, dev(gp), dev(gv))
    want = rule(x, net, spec, gp, gv)
    compare((p, v, grads), want, where)
    return want


# (name, (m, d, e), block widths, kind, actions)
SHAPES = [
    ("host", (5, 3, 0), [32, 32], "residue", 4),
    ("agent", (5, 3, 3), [32, 32], "residue", 3),
    ("three_two", (3, 2, 2), [64, 32], "residue", 2),
    ("one_point", (1, 2, 0), [32], "residue", 1),
]


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_kernels_match_the_rule(shape):
    name, spec, arch, kind, actions = shape
    m = spec[0]
    cs = np.concatenate([np.arange(m + 1), np.random.default_rng(len(name)).integers(0, m + 1, 30)])
    check(cs, spec, arch, kind, actions, sum(map(ord, name)), where=name)


def test_sixty_four_towers_and_seventy_rows():
    """more towers than rows: most towers get +0, the grid does not depend on it"""
    rng = np.random.default_rng(64)
    cs = np.concatenate([[64, 63, 0], rng.integers(0, 65, 67)])
    want = check(cs, (64, 2, 0), [32], "dense", 3, 64, where="m = 64")
    empty = sorted(set(range(64)) - set(int(c) for c in cs))
    assert empty
    for label, w in want[2]:
        if label.startswith(f"tower{empty[0]}."):
            assert not w.any() and not np.signbit(w).any()


@pytest.mark.parametrize("trunk", [([64, 128], "residue"), ([128, 128], "residue"), ([33, 64], "dense"),
                                   ([64, 33, 128], ["residue", "dense", "residue"]), ([17, 32, 32], ["dense", "residue", "residue"])],
                         ids=["projection", "wide", "dense", "mixed", "dense_first"])
def test_trunks(trunk):
    arch, kind = trunk
    cs = np.concatenate([np.arange(4), np.random.default_rng(7).integers(0, 4, 34)])
    check(cs, (3, 2, 2), arch, kind, 3, 70 + len(arch) + arch[0], where=trunk)


def test_a_tower_whose_input_is_as_wide_as_its_first_block():
    """tower 15 of (16, 2) takes 32 inputs into a residue block of 32: no projection there, one in every other tower"""
    cs = np.concatenate([[15] * 5, np.arange(17), [14, 15, 16, 0]])
    want = check(cs, (16, 2, 0), [32, 32], "residue", 3, 16, where="k == n")
    labels = [label for label, _ in want[2]]
    assert "tower14.block0.proj.d_weight" in labels and "tower15.block0.proj.d_weight" not in labels


@pytest.mark.parametrize("batch", [1, 15, 16, 17, 67, 130])
def test_batches(batch):
    rng = np.random.default_rng(batch)
    check(rng.integers(0, 6, batch), (5, 3, 3), [32], "residue", 3, 100 + batch, where=batch)


MIXES = {
    "one group": [3] * 37,
    "every count": list(np.arange(40) % 6),
    "a tower with no rows": [0, 1, 3, 4, 5] * 7,
    "sixteen, then another group": [1] * 16 + [4] * 5,
    "seventeen, then another group": [4] * 3 + [1] * 17 + [4] * 2,
    "only rows without a tower": [5] * 19,
}


@pytest.mark.parametrize("mix", list(MIXES), ids=[k.replace(" ", "_").replace(",", "") for k in MIXES])
def test_count_mixes(mix):
    cs = np.asarray(MIXES[mix])
    want = check(cs, (5, 3, 3), [32, 32], "residue", 3, len(mix), where=mix)
    grads = dict(want[2])
    for t in range(5):
        assert grads[f"tower{t}.block1.dense2.d_gn_bias"].any() == (cs == t).any(), (mix, t)
        if not (cs == t).any():
            assert all(not w.any() and not np.signbit(w).any() for label, w in want[2] if label.startswith(f"tower{t}."))
    assert grads["policy.d_weight"].any()


def test_rows_with_holes():
    rng = np.random.default_rng(5)
    cs = np.concatenate([np.arange(1, 6), rng.integers(1, 5, 20)])
    check(cs, (5, 3, 3), [32, 32], "residue", 3, 55, holes=True, where="holes")


@pytest.fixture(scope="module")
def agent():
    """the (5, 3) agent with its rule results on 45 rows of every count, interleaved"""
    spec = (5, 3, 3)
    rng = np.random.default_rng(50)
    net = C.random_net(rng, *spec, [64, 32], 3, value_gain=3.0)
    x = C.rows_with_counts(rng, (np.arange(45) * 5) % 6, *spec)
    gp, gv = grads_in(rng, 45, 3)
    return spec, net, x, gp, gv, rule(x, net, spec, gp, gv)


def test_forward_is_customnet_forward_to_the_bit(agent):
    ops = _ops()
    spec, net, x, gp, gv, want = agent
    plan = device_plan(net, *spec)
    for raw in (False, True):
        p, v, _ = ops.customnet_train_forward(dev(x), plan, raw_value=raw)
        p0, v0 = ops.customnet_forward(dev(x), plan, raw_value=raw)
        assert same_bits(p.cpu().numpy(), p0.cpu().numpy()) and same_bits(v.cpu().numpy(), v0.cpu().numpy())


def test_the_tanh_path(agent):
    """without raw_value the stored value is the tanh's and dzh[:, A] = t * (1 - v * v) from the STORED v"""
    ops = _ops()
    spec, net, x, gp, gv, _ = agent
    plan = device_plan(net, *spec)
    p, v, saved = ops.customnet_train_forward(dev(x), plan)
    assert float(v.abs().max()) <= 1
    grads = ops.customnet_backward(saved, dev(gp), dev(gv).unsqueeze(1))
    rp, rv, rsaved = CG.forward_saved(x, net, *spec)
    want = CG.param_grads(CG.backward(rsaved, net, gp, CG.tanh_grad(gv, v.cpu().numpy())))
    compare((p, dev(rv), grads), (rp, rv, want), "tanh")


def test_strided_columns_of_a_record(agent):
    """x, grad_policy and grad_value as columns of wider records"""
    ops = _ops()
    spec, net, x, gp, gv, want = agent
    batch, actions = len(x), 3
    gx = Guarded(batch, x.shape[1], 3, x.shape[1] + 5, x)
    record = Guarded(batch, actions + 1, 1, actions + 4, np.concatenate([gp, gv[:, None]], axis=1))
    p, v, saved = ops.customnet_train_forward(gx.view, device_plan(net, *spec), raw_value=True)
    grads = ops.customnet_backward(saved, record.view[:, :actions], record.view[:, actions])
    compare((p, v, grads), want, "record")
    assert gx.holds() and record.holds()


def test_same_bits_twice_from_a_larger_workspace_and_nothing_else_written(agent):
    """two calls give the same bits (the grouped order is the same on every launch), a larger workspace changes none, and
    nothing outside the gradient buffer's and the workspace's own bytes changes"""
    ops = _ops()
    from hironaka_amd._lib import lib
    spec, net, x, gp, gv, want = agent
    plan = device_plan(net, *spec)
    xd = dev(x)
    p, v, saved = ops.customnet_train_forward(xd, plan, raw_value=True)
    first = ops.customnet_backward(saved, dev(gp), dev(gv))
    compare((p, v, first), want, "first")
    first = [g.clone() for g in first]
    for _ in range(3):
        p1, v1, saved1 = ops.customnet_train_forward(xd, plan, raw_value=True)
        again = ops.customnet_backward(saved1, dev(gp), dev(gv))
        assert torch.equal(p1, p) and torch.equal(v1, v) and all(torch.equal(a, b) for a, b in zip(again, first))
    # the forward into a workspace with 40 floats before and 1000 behind what it needs
    need = saved.workspace.numel()
    store = torch.full((40 + need + 1000,), SENTINEL, dtype=torch.float32, device="cuda")
    p2, v2 = torch.empty_like(p), torch.empty_like(v)
    g = ops._customgrad_desc(plan, xd, p2, v2, store[40:], True)
    assert lib().hk_customgrad_workspace_bytes(ctypes.byref(g)) == 4 * need
    assert lib().hk_customgrad_forward(ctypes.byref(g), None) == A.HK_OK
    torch.cuda.synchronize()
    assert torch.equal(p2, p) and torch.equal(v2, v)
    assert bool((store[:40] == SENTINEL).all()) and bool((store[40 + need:] == SENTINEL).all())
    # the backward from it, into a guarded buffer
    out = torch.full((7 + plan.grad_floats + 9,), SENTINEL, dtype=torch.float32, device="cuda")
    saved2 = ops.CustomnetSaved(plan, xd, p2, v2, store[40:], True)
    second = ops.customnet_backward(saved2, dev(gp), dev(gv), out=out[7:7 + plan.grad_floats])
    compare((p2, v2, second), want, "second")
    assert all(g.data_ptr() == out.data_ptr() + 4 * (7 + s) for g, s in zip(second, plan.grad_starts))
    assert bool((out[:7] == SENTINEL).all()) and bool((out[7 + plan.grad_floats:] == SENTINEL).all())
    inside = torch.ones(plan.grad_floats, dtype=torch.bool, device="cuda")
    for s, t in zip(plan.grad_starts, plan.params):
        inside[s:s + t.numel()] = False
    assert bool((out[7:7 + plan.grad_floats][inside] == SENTINEL).all())  # the floats between two gradients
    assert bool((store[:40] == SENTINEL).all()) and bool((store[40 + need:] == SENTINEL).all())


def test_python_boundary_refusals(agent):
    ops = _ops()
    spec, net, x, gp, gv, _ = agent
    plan = device_plan(net, *spec)
    k = x.shape[1]
    with pytest.raises(TypeError):
        ops.customnet_train_forward(dev(x), object())
    with pytest.raises(ValueError):
        ops.customnet_train_forward(torch.zeros(A.HK_PVGRAD_MAX_BATCH + 1, k, device="cuda"), plan)
    with pytest.raises(ValueError):
        ops.customnet_train_forward(torch.zeros(3, k - 1, device="cuda"), plan)
    with pytest.raises(TypeError):
        ops.customnet_train_forward(torch.zeros(3, k, device="cuda", dtype=torch.float64), plan)
    with pytest.raises(TypeError):
        ops.customnet_train_forward(torch.zeros(3, k), plan)
    p, v, saved = ops.customnet_train_forward(dev(x[:3]), plan)
    with pytest.raises(TypeError):
        ops.customnet_backward(saved, torch.zeros(3, 4, device="cuda"), torch.zeros(3, device="cuda"))
    with pytest.raises(TypeError):
        ops.customnet_backward(saved, torch.zeros(3, 3, device="cuda"), torch.zeros(4, device="cuda"))
    with pytest.raises(TypeError):
        ops.customnet_backward(saved, torch.zeros(3, 3, device="cuda", dtype=torch.float64), torch.zeros(3, device="cuda"))
    with pytest.raises(ValueError):
        ops.customnet_backward(saved, torch.zeros(3, 3, device="cuda"), torch.zeros(3, device="cuda"),
                               out=torch.zeros(plan.grad_floats + 1, device="cuda"))
    with pytest.raises(TypeError):
        ops.customnet_backward(saved, torch.zeros(3, 3, device="cuda"), torch.zeros(3, device="cuda"),
                               out=torch.zeros(plan.grad_floats, device="cuda", dtype=torch.float64))
    # params: tower after tower, block after block, then the heads
    per_tower = (3 + 3) * 4  # both blocks change the width: dense1, dense2 and proj, four parameters each
    assert len(plan.params) == 5 * per_tower + 4
    assert [tuple(t.shape) for t in plan.params[:4]] == [(64, 6), (64,), (64,), (64,)]
    assert tuple(plan.params[per_tower].shape) == (64, 9) and tuple(plan.params[-4].shape) == (3, 35)
    # an empty batch: empty results, zero gradients, no launch
    p, v, saved = ops.customnet_train_forward(torch.zeros(0, k, device="cuda"), plan)
    grads = ops.customnet_backward(saved, torch.zeros(0, 3, device="cuda"), torch.zeros(0, device="cuda"))
    assert p.shape == (0, 3) and v.shape == (0,) and all(not bool(t.any()) for t in grads)
