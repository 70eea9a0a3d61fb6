"""hironaka_amd.net.DenseResNet / DenseNet with fused_training = True on the device: the .grads are ops.pvnet_backward's, they
lie within torch's own distance of a float64 run, frozen parameters get None, everything that is not served falls back with
its reason, and with fused_training = False the module is what it was."""
import copy
import pickle

import numpy as np
import pytest
import torch

from hironaka_amd import _abi as A
from test_pvgrad_rules import units

pytestmark = pytest.mark.gpu


def _net():
    from hironaka_amd import net
    return net


def make(cls, arch, in_dim=60, actions=4, seed=5, fused=True):
    module = getattr(_net(), cls)(actions, arch, input_dim=in_dim, seed=seed).cuda()
    rng = np.random.default_rng(seed)
    with torch.no_grad():  # off the initial zeros and ones, so that every gradient is a sum of unlike terms
        for p in module.parameters():
            p.add_(0.1 * torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)).cuda())
    module.fused_training = fused
    return module


def data(batch, in_dim, actions, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(batch, in_dim, generator=g) * 2 - 1
    gp, gv = torch.randn(batch, actions, generator=g) / batch, torch.randn(batch, 1, generator=g) / batch
    return tuple(t.to("cuda", dtype) for t in (x, gp, gv))


def backward(module, x, gp, gv):
    module.zero_grad()
    p, v = module(x)
    ((p * gp).sum() + (v * gv).sum()).backward()
    return p.detach(), v.detach(), [None if q.grad is None else q.grad.detach().clone() for q in module.parameters()]


@pytest.mark.parametrize("cls,arch", [("DenseResNet", [64, 128, 128]), ("DenseNet", [33, 64])])
def test_grads_are_pvnet_backwards(cls, arch):
    from hironaka_amd import ops
    module = make(cls, arch)
    assert module.fused_reason is None
    x, gp, gv = data(21, 60, 4)
    p, v, grads = backward(module, x, gp, gv)
    assert module.fused_last_reason is None and v.shape == (21, 1)
    plan = module._cached_plan()
    assert [id(t) for t in plan.params] == [id(t) for t in module.parameters()]  # module order
    p2, v2, saved = ops.pvnet_train_forward(x, plan)
    want = ops.pvnet_backward(saved, gp, gv)
    assert torch.equal(p, p2) and torch.equal(v[:, 0], v2)
    assert all(torch.equal(g, w) for g, w in zip(grads, want)) and all(float(g.abs().max()) > 0 for g in grads)
    with torch.no_grad():  # under no_grad the module takes hk_pvnet_forward as before, with the same bits
        p3, v3 = module(x)
    assert module.fused_last_reason is None and torch.equal(p3, p) and torch.equal(v3, v)
    # gradients accumulate as autograd's do
    p, v = module(x)
    ((p * gp).sum() + (v * gv).sum()).backward()
    assert all(torch.equal(q.grad, 2 * w) for q, w in zip(module.parameters(), want))


NETS = [("same_width", [128, 128]), ("projection", [256, 128])]


@pytest.mark.parametrize("name,arch", NETS, ids=[n[0] for n in NETS])
def test_fused_backward_lies_within_torchs_distance_of_float64(name, arch):
    """E_fused <= 2 * max(E_torch, 1): E the largest over the parameters' gradients of max |g - g64| in units of
    max |g64| * 2^-24 (test_pvgrad_rules.units) against a float64 run of a copy of the module, torch's float32 autograd on the
    same module as the yardstick; 32 rows.
    Recorded on an MI355X (E_torch / E_fused): same_width 52.4 / 33.1, projection 40.6 / 48.7."""
    module = make("DenseResNet", arch)
    x, gp, gv = data(32, 60, 4, seed=3)
    _, _, g_fused = backward(module, x, gp, gv)
    assert module.fused_last_reason is None
    module.fused_training = False
    _, _, g_torch = backward(module, x, gp, gv)
    assert module.fused_last_reason == "gradients are on"
    _, _, g64 = backward(copy.deepcopy(module).double(), x.double(), gp.double(), gv.double())
    g64 = [g.cpu().numpy() for g in g64]
    largest = max(np.abs(r).max() for r in g64)
    e_torch = max(units(g.cpu().numpy(), r, largest) for g, r in zip(g_torch, g64))
    e_fused = max(units(g.cpu().numpy(), r, largest) for g, r in zip(g_fused, g64))
    print(f"{name}: E_torch {e_torch:.3g} E_fused {e_fused:.3g}")
    assert e_fused <= 2 * max(e_torch, 1)


def test_frozen_parameters_get_none():
    module = make("DenseResNet", [64, 64])
    x, gp, gv = data(9, 60, 4)
    _, _, full = backward(module, x, gp, gv)
    frozen = [module.DenseResidueBlock_0.Dense_0.weight, module.DenseResidueBlock_1.GroupNorm_1.bias, module.Dense_1.bias]
    for q in frozen:
        q.requires_grad_(False)
    _, _, grads = backward(module, x, gp, gv)
    assert module.fused_last_reason is None
    for q, g, w in zip(module.parameters(), grads, full):
        assert (g is None) if any(q is f for f in frozen) else torch.equal(g, w)
    for q in module.parameters():
        q.requires_grad_(False)
    module(x)  # nothing requires a gradient: hk_pvnet_forward, as before
    assert module.fused_last_reason is None


def test_fall_back_reasons():
    module = make("DenseResNet", [64, 64])
    x, gp, gv = data(5, 60, 4)
    _, _, want = backward(module, x, gp, gv)
    xg = x.clone().requires_grad_(True)
    p, v = module(xg)
    assert module.fused_last_reason == "the input is not float32 on cuda:0 with a batch dimension, or requires a gradient"
    ((p * gp).sum() + (v * gv).sum()).backward()
    assert xg.grad is not None
    many = torch.zeros(A.HK_PVGRAD_MAX_BATCH + 1, 60, device="cuda")
    module(many)
    assert module.fused_last_reason == f"more than {A.HK_PVGRAD_MAX_BATCH} rows with gradients on"
    module(many[:-1])
    assert module.fused_last_reason is None
    with pytest.raises(RuntimeError):  # torch's own refusal of a float64 input to float32 weights: the plain path
        module(x.double())
    assert "not float32" in module.fused_last_reason
    double = copy.deepcopy(module).double()
    assert double.fused_training and double.fused_reason == "parameters are not float32"
    odd = make("DenseResNet", [96, 64])
    assert odd.fused_reason == f"a normed width that is none of {A.PVNET_NORMED_WIDTHS}"
    _, _, g = backward(odd, x, gp, gv)
    assert odd.fused_last_reason == odd.fused_reason and all(t is not None for t in g)
    shared = make("DenseResNet", [64, 64, 64])
    shared.DenseResidueBlock_2.Dense_1 = shared.DenseResidueBlock_1.Dense_1
    shared(x)
    assert shared.fused_last_reason == "a parameter is used twice and gradients are on"
    module.fused_enabled = False
    module(x)
    assert module.fused_last_reason == "fused_enabled is False"


def test_without_fused_training_the_module_is_what_it_was():
    module = make("DenseResNet", [64, 64], fused=False)
    assert _net().DenseResNet.fused_training is False and module.fused_reason == "gradients are on"
    x, gp, gv = data(9, 60, 4)
    p, v, grads = backward(module, x, gp, gv)
    assert module.fused_last_reason == "gradients are on"
    module.zero_grad()
    pp, vv = module.plain_forward(x)
    ((pp * gp).sum() + (vv * gv).sum()).backward()
    assert torch.equal(p, pp) and torch.equal(v, vv)
    assert all(torch.equal(g, q.grad) for g, q in zip(grads, module.parameters()))


def test_double_backward_raises():
    module = make("DenseResNet", [64])
    x, gp, gv = data(5, 60, 4)
    p, v = module(x)
    # (a gradient at the outputs that itself has a graph, so that the backward's results would have one)
    (g,) = torch.autograd.grad((p * gp).sum() ** 2 + (v * gv).sum() ** 2, [module.Dense_0.weight], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_deepcopy_and_pickle_carry_the_flag_and_not_the_plan():
    module = make("DenseResNet", [64, 64])
    x, gp, gv = data(5, 60, 4)
    _, _, want = backward(module, x, gp, gv)
    assert "_fused_plan" in module.__dict__
    for clone in (copy.deepcopy(module), pickle.loads(pickle.dumps(module))):
        assert clone.fused_training is True and "_fused_plan" not in clone.__dict__
        _, _, got = backward(clone, x, gp, gv)
        assert clone.fused_last_reason is None and all(torch.equal(g, w) for g, w in zip(got, want))
        assert clone._cached_plan() is not module._cached_plan()
