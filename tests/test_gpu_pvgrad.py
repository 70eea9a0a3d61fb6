"""hk_pvgrad_forward / hk_pvgrad_backward on the device against tests/pvgrad_rules.py (which test_pvgrad_rules.py pins by
hand and, within torch's own distance of float64, to torch): policy, raw value and EVERY gradient bit for bit.  Finite inputs
only (a NaN row reaches every weight gradient).  The shapes are the smallest that reach every path: normed widths 32 / 64 /
128 / 256 behind input widths on both sides of the MFMA's 16, blocks with and without a projection, dense blocks, batches
that cover ROWSUM's sixteen residues and more than one row tile, 32 blocks (the parameter table split over launches)."""
import ctypes

import numpy as np
import pytest
import torch

import pvgrad_rules as G
import pvnet_rules as R
from hironaka_amd import _abi as A
from test_gpu_mlp import SENTINEL, Guarded, Packed, dev, inputs
from test_gpu_pvnet import device_plan

pytestmark = pytest.mark.gpu
same_bits = R.same_bits
F32 = np.float32


def _ops():
    from hironaka_amd import ops
    return ops


def grads_in(rng, batch, actions):
    """gradients at the outputs of the size a mean over the batch gives, with a few zeros"""
    gp = (rng.standard_normal((batch, actions)) / batch).astype(F32)
    gp[rng.random((batch, actions)) < 0.05] = 0
    return gp, (rng.standard_normal(batch) / batch).astype(F32)


def rule(x, net, gp, gv):
    """(policy, raw value, [(label, gradient)]) by the rule, gv being the gradient at the raw value"""
    p, v, saved = G.forward_saved(x, net)
    return p, v, G.param_grads(G.backward(saved, net, gp, gv))


def compare(got, want, where):
    p, v, grads = got
    assert same_bits(p.cpu().numpy(), want[0]), (where, "policy")
    assert same_bits(v.cpu().numpy(), want[1]), (where, "value")
    assert len(grads) == len(want[2])
    for g, (label, w) in zip(grads, want[2]):
        assert tuple(g.shape) == w.shape and same_bits(g.cpu().numpy(), w), (where, label)


def check(x, net, gp, gv, where=None, want=None):
    ops = _ops()
    plan = device_plan(net)
    p, v, saved = ops.pvnet_train_forward(dev(x), plan, raw_value=True)
    grads = ops.pvnet_backward(saved, dev(gp), dev(gv))
    want = rule(x, net, gp, gv) if want is None else want
    compare((p, v, grads), want, where)
    return want


@pytest.mark.parametrize("n", [32, 64, 128, 256])
def test_cross_of_normed_and_input_widths(n):
    rng = np.random.default_rng(n)
    for k0 in (1, 15, 18, 63, 256):
        net = R.random_net(rng, k0, [n], 4)
        check(inputs(rng, 19, k0), net, *grads_in(rng, 19, 4), where=(k0, n))


def test_trunks_with_and_without_projection():
    rng = np.random.default_rng(30)
    for k0, arch in ((60, [64, 128, 128, 32]), (64, [64, 64])):
        net = R.random_net(rng, k0, arch, 4)
        check(inputs(rng, 21, k0), net, *grads_in(rng, 21, 4), where=(k0, arch))


def test_dense_blocks_alone_and_mixed():
    rng = np.random.default_rng(31)
    check(inputs(rng, 21, 63), R.random_net(rng, 63, [17, 33, 1, 64], 3, "dense"), *grads_in(rng, 21, 3), where="dense")
    for k0, arch, kinds in ((18, [64, 33, 128], ["residue", "dense", "residue"]), (60, [17, 32, 1], ["dense", "residue", "dense"])):
        check(inputs(rng, 21, k0), R.random_net(rng, k0, arch, 3, kinds), *grads_in(rng, 21, 3), where=(k0, arch, kinds))


@pytest.mark.parametrize("actions", [1, 3, 15, 16, 255])
def test_policy_widths(actions):
    rng = np.random.default_rng(actions)
    for k0, arch, kind in ((18, [64], "residue"), (33, [17], "dense")):
        check(inputs(rng, 18, k0), R.random_net(rng, k0, arch, actions, kind), *grads_in(rng, 18, actions), where=(actions, kind))


@pytest.mark.parametrize("batch", [1, 3, 15, 16, 17, 33, 67, 130])
def test_batches(batch):
    """ROWSUM's residues, chains on both sides of a multiple of 4 and of 16, more than one row tile"""
    rng = np.random.default_rng(batch)
    net = R.random_net(rng, 18, [64, 128], 4)
    check(inputs(rng, batch, 18), net, *grads_in(rng, batch, 4), where=batch)


def test_without_biases_and_affine_parameters():
    rng = np.random.default_rng(32)
    for bias, affine in ((False, True), (True, False), (False, False)):
        net = R.random_net(rng, 18, [64, 128, 128], 4, bias=bias, affine=affine)
        want = check(inputs(rng, 19, 18), net, *grads_in(rng, 19, 4), where=(bias, affine))
        assert len(want[2]) == (3 + 3 + 2) * (1 + bias + 2 * affine) + 2 * (1 + bias)


def test_the_tanh_path():
    """without raw_value the stored value is the tanh's and dzh[:, A] = t * (1 - v * v) from the STORED v"""
    ops = _ops()
    rng = np.random.default_rng(33)
    net = R.random_net(rng, 18, [128, 64], 4, value_gain=3.0)
    x = inputs(rng, 21, 18)
    gp, gv = grads_in(rng, 21, 4)
    plan = device_plan(net)
    p, v, saved = ops.pvnet_train_forward(dev(x), plan)
    p0, v0 = ops.pvnet_forward(dev(x), plan)
    assert torch.equal(p, p0) and torch.equal(v, v0) and float(v.abs().max()) <= 1
    grads = ops.pvnet_backward(saved, dev(gp), dev(gv).unsqueeze(1))
    rp, rv, rsaved = G.forward_saved(x, net)
    want = G.param_grads(G.backward(rsaved, net, gp, G.tanh_grad(gv, v.cpu().numpy())))
    compare((p, dev(rv), grads), (rp, rv, want), "tanh")


def test_forward_is_pvnet_forward_to_the_bit():
    ops = _ops()
    rng = np.random.default_rng(34)
    for k0, arch, kinds, batch in ((60, [64, 128, 128, 32], "residue", 35), (63, [17, 33, 64], ["dense", "dense", "residue"], 16)):
        plan = device_plan(R.random_net(rng, k0, arch, 5, kinds))
        x = dev(inputs(rng, batch, k0))
        for raw in (False, True):
            p, v, _ = ops.pvnet_train_forward(x, plan, raw_value=raw)
            p0, v0 = ops.pvnet_forward(x, plan, raw_value=raw)
            assert same_bits(p.cpu().numpy(), p0.cpu().numpy()) and same_bits(v.cpu().numpy(), v0.cpu().numpy())


def test_strided_columns_of_a_record():
    """x, grad_policy and grad_value as columns of wider records"""
    ops = _ops()
    rng = np.random.default_rng(35)
    batch, k0, actions = 19, 18, 4
    net = R.random_net(rng, k0, [64, 128], actions)
    x = inputs(rng, batch, k0)
    gp, gv = grads_in(rng, batch, actions)
    gx = Guarded(batch, k0, 3, k0 + 5, x)
    record = Guarded(batch, actions + 1, 1, actions + 4, np.concatenate([gp, gv[:, None]], axis=1))
    p, v, saved = ops.pvnet_train_forward(gx.view, device_plan(net), raw_value=True)
    grads = ops.pvnet_backward(saved, record.view[:, :actions], record.view[:, actions])
    compare((p, v, grads), rule(x, net, gp, gv), "record")
    assert gx.holds() and record.holds()


def test_thirty_two_blocks_split_the_parameter_table():
    rng = np.random.default_rng(36)
    arch = [32, 64] * 16
    net = R.random_net(rng, 18, arch, 3)
    assert sum(1 + (b.dense2 is not None) + (b.proj is not None) for b in net.blocks) + 2 == 98 > 2 * A.HK_PVGRAD_TABLE
    check(inputs(rng, 5, 18), net, *grads_in(rng, 5, 3), where="32 blocks")


def test_same_bits_twice_from_a_larger_workspace_and_nothing_else_written():
    """the gradients written into sentinel-guarded tensors, the workspace inside a larger guarded buffer: two launches give
    the same bits, a larger workspace changes none, and nothing outside the gradients and the workspace's own bytes changes"""
    ops = _ops()
    from hironaka_amd._lib import lib
    rng = np.random.default_rng(37)
    batch, k0, actions = 21, 60, 4
    net = R.random_net(rng, k0, [64, 128, 128], actions)
    x = inputs(rng, batch, k0)
    gp, gv = grads_in(rng, batch, actions)
    want = rule(x, net, gp, gv)
    plan = device_plan(net)
    xd = dev(x)
    p, v, saved = ops.pvnet_train_forward(xd, plan, raw_value=True)
    first = ops.pvnet_backward(saved, dev(gp), dev(gv))
    compare((p, v, first), want, "first")
    # the forward into a workspace with 40 floats before and 1000 behind what it needs
    need = saved.workspace.numel()
    store = torch.full((40 + need + 1000,), SENTINEL, dtype=torch.float32, device="cuda")
    p2, v2 = torch.empty_like(p), torch.empty_like(v)
    g = ops._pvgrad_desc(plan, xd, p2, v2, store[40:], True)
    assert lib().hk_pvgrad_workspace_bytes(ctypes.byref(g)) == 4 * need
    assert lib().hk_pvgrad_forward(ctypes.byref(g), None) == A.HK_OK
    torch.cuda.synchronize()
    assert torch.equal(p2, p) and torch.equal(v2, v)
    assert bool((store[:40] == SENTINEL).all()) and bool((store[40 + need:] == SENTINEL).all())
    # the backward from it, into guarded gradients
    packed = Packed([np.zeros(w.shape, F32) for _, w in want[2]], 5, gap=3)
    saved2 = ops.PvnetSaved(plan, xd, p2, v2, store[40:], True)
    second = ops.pvnet_backward(saved2, dev(gp), dev(gv), grads=packed.views)
    compare((p2, v2, second), want, "second")
    for i, (_, w) in enumerate(want[2]):
        packed.put(i, w)
    assert packed.holds()
    assert bool((store[:40] == SENTINEL).all()) and bool((store[40 + need:] == SENTINEL).all())
    assert not bool((store[40:40 + need] == SENTINEL).any())  # every element of the workspace has a writer


def test_python_boundary_refusals():
    ops = _ops()
    rng = np.random.default_rng(38)
    net = R.random_net(rng, 18, [64], 4)
    plan = device_plan(net)
    with pytest.raises(ValueError):
        ops.pvnet_train_forward(torch.zeros(A.HK_PVGRAD_MAX_BATCH + 1, 18, device="cuda"), plan)
    with pytest.raises(ValueError):
        ops.pvnet_train_forward(torch.zeros(3, 17, device="cuda"), plan)
    with pytest.raises(TypeError):
        ops.pvnet_train_forward(torch.zeros(3, 18, device="cuda", dtype=torch.float64), plan)
    p, v, saved = ops.pvnet_train_forward(dev(inputs(rng, 3, 18)), plan)
    with pytest.raises(TypeError):
        ops.pvnet_backward(saved, torch.zeros(3, 5, device="cuda"), torch.zeros(3, device="cuda"))
    with pytest.raises(TypeError):
        ops.pvnet_backward(saved, torch.zeros(3, 4, device="cuda"), torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError):
        ops.pvnet_backward(saved, torch.zeros(3, 4, device="cuda"), torch.zeros(3, device="cuda"), grads=[])
    assert len(plan.params) == 3 * 4 + 4 and [tuple(t.shape) for t in plan.params[:4]] == [(64, 18), (64,), (64,), (64,)]
    # an empty batch: empty results, zero gradients
    p, v, saved = ops.pvnet_train_forward(torch.zeros(0, 18, device="cuda"), plan)
    grads = ops.pvnet_backward(saved, torch.zeros(0, 4, device="cuda"), torch.zeros(0, device="cuda"))
    assert p.shape == (0, 4) and v.shape == (0,) and all(not bool(t.any()) for t in grads)
