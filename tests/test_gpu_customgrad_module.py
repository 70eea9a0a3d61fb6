"""hironaka_amd.net.CustomNet with fused_tower_training = True and HipTrainer(custom_net=True, fused_tower_training=True) on
the device: the .grads are ops.customnet_backward's, they lie within torch's own distance of a float64 run of the reference's
formula, frozen parameters get None, everything that is not served falls back with its reason, with the flag off the module
is what it was, train is the public pieces and nothing else, and one step replays from a graph."""
import copy
import pickle

import numpy as np
import pytest
import torch

import customnet_rules as C
from hironaka_amd import _abi as A
from test_gpu_customnet import trainer_config
from test_gpu_trainer_train import _flat
from test_pvgrad_rules import units

pytestmark = pytest.mark.gpu
SPEC = (5, 3)


def _net():
    from hironaka_amd import net
    return net


def make(arch, block="DenseResidueBlock", role="agent", seed=5, fused=True, spec=SPEC):
    N = _net()
    module = N.CustomNet(3 if role == "agent" else 4, arch, spec, block_cls=getattr(N, block), role=role, seed=seed).cuda()
    rng = np.random.default_rng(seed)
    with torch.no_grad():  # off the initial zeros and ones, so that every gradient is a sum of unlike terms
        for p in module.parameters():
            p.add_(0.1 * torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32)).cuda())
    module.fused_tower_training = fused
    return module


def data(module, cs, seed=0, dtype=torch.float32):
    m, d = module.spec
    rng = np.random.default_rng(seed)
    x = C.rows_with_counts(rng, np.asarray(cs), m, d, module.extra_dim)
    g = torch.Generator().manual_seed(seed)
    gp, gv = torch.randn(len(cs), module.output_size, generator=g) / len(cs), torch.randn(len(cs), 1, generator=g) / len(cs)
    return tuple(t.to("cuda", dtype) for t in (torch.from_numpy(x), gp, gv))


def backward(module, x, gp, gv):
    module.zero_grad()
    p, v = module(x)
    ((p * gp).sum() + (v * gv).sum()).backward()
    return p.detach(), v.detach(), [None if q.grad is None else q.grad.detach().clone() for q in module.parameters()]


@pytest.mark.parametrize("block,arch", [("DenseResidueBlock", [64, 128]), ("DenseBlock", [33, 64])])
def test_grads_are_customnet_backwards(block, arch):
    from hironaka_amd import ops
    module = make(arch, block)
    assert module.fused_reason is None and _net().CustomNet.fused_tower_training is False
    x, gp, gv = data(module, np.arange(41) % 6)
    p, v, grads = backward(module, x, gp, gv)
    assert module.fused_last_reason is None and v.shape == (41, 1)
    plan = module._cached_plan()
    assert [id(t) for t in plan.params] == [id(t) for t in module.parameters()]  # module order
    p2, v2, saved = ops.customnet_train_forward(x, plan)
    want = ops.customnet_backward(saved, gp, gv)
    assert torch.equal(p, p2) and torch.equal(v[:, 0], v2)
    assert all(torch.equal(g, w) for g, w in zip(grads, want)) and all(float(g.abs().max()) > 0 for g in grads)
    with torch.no_grad():  # under no_grad the module takes hk_customnet_forward as before, with the same bits
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
    max |g64| * 2^-24 (test_pvgrad_rules.units) against a float64 run of a copy of the module through plain_forward (the
    reference's formula), the flag-off module in float32 -- autograd through the same formula -- as the yardstick; the (3, 3)
    agent, 32 rows over every count.
    Recorded on an MI355X (E_torch / E_fused): same_width 94.5 / 123, projection 66.8 / 36.4."""
    module = make(arch, spec=(3, 3))
    x, gp, gv = data(module, np.arange(32) % 4, seed=3)
    _, _, g_fused = backward(module, x, gp, gv)
    assert module.fused_last_reason is None
    module.fused_tower_training = False
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
    module = make([64, 64])
    x, gp, gv = data(module, np.arange(19) % 6)
    _, _, full = backward(module, x, gp, gv)
    frozen = [module.DenseResidueBlock_0.Dense_0.weight, module.DenseResidueBlock_7.GroupNorm_1.bias, module.Dense_1.bias]
    for q in frozen:
        q.requires_grad_(False)
    _, _, grads = backward(module, x, gp, gv)
    assert module.fused_last_reason is None
    for q, g, w in zip(module.parameters(), grads, full):
        assert (g is None) if any(q is f for f in frozen) else torch.equal(g, w)
    for q in module.parameters():
        q.requires_grad_(False)
    module(x)  # nothing requires a gradient: hk_customnet_forward, as before
    assert module.fused_last_reason is None


def test_fall_back_reasons():
    module = make([64, 64])
    x, gp, gv = data(module, np.arange(7) % 6)
    backward(module, x, gp, gv)
    assert module.fused_last_reason is None
    xg = x.clone().requires_grad_(True)
    p, v = module(xg)
    assert module.fused_last_reason == "the input is not float32 on cuda:0 with a batch dimension, or requires a gradient"
    ((p * gp).sum() + (v * gv).sum()).backward()
    assert xg.grad is not None
    many = torch.zeros(A.HK_PVGRAD_MAX_BATCH + 1, 18, device="cuda")
    module(many)
    assert module.fused_last_reason == f"more than {A.HK_PVGRAD_MAX_BATCH} rows with gradients on"
    module(many[:-1])
    assert module.fused_last_reason is None
    with pytest.raises(RuntimeError):  # torch's own refusal of a float64 input to float32 weights: the plain path
        module(x.double())
    assert "not float32" in module.fused_last_reason
    with pytest.raises(RuntimeError):  # the plain path's own refusal of a row of another width
        module(x[:, :-1])
    assert module.fused_last_reason == "the input is not 18 wide"
    double = copy.deepcopy(module).double()
    assert double.fused_tower_training and double.fused_reason == "parameters are not float32"
    odd = make([96, 64])
    assert odd.fused_reason == f"a normed width that is none of {A.PVNET_NORMED_WIDTHS}"
    _, _, g = backward(odd, x, gp, gv)
    assert odd.fused_last_reason == odd.fused_reason and all(t is not None for t in g)
    flat = make([64], spec=(5, 1), role="host")
    assert flat.fused_reason == f"not 1 to {A.HK_CUSTOMNET_MAX_POINTS} points of at least 2 coordinates"
    shared = make([64, 64, 64])
    shared.DenseResidueBlock_2.Dense_1 = shared.DenseResidueBlock_1.Dense_1
    shared(x)
    assert shared.fused_last_reason == "a parameter is used twice and gradients are on"
    module.fused_enabled = False
    module(x)
    assert module.fused_last_reason == "fused_enabled is False"


def test_with_the_flag_off_the_module_is_what_it_was():
    module = make([64, 64], fused=False)
    module.fused_training = True  # has no effect on a CustomNet
    assert module.fused_reason == "gradients are on"
    x, gp, gv = data(module, np.arange(13) % 6)
    p, v, grads = backward(module, x, gp, gv)
    assert module.fused_last_reason == "gradients are on"
    module.zero_grad()
    pp, vv = module.plain_forward(x)
    ((pp * gp).sum() + (vv * gv).sum()).backward()
    assert torch.equal(p, pp) and torch.equal(v, vv)
    assert all(torch.equal(g, q.grad) for g, q in zip(grads, module.parameters()))


def test_double_backward_raises():
    module = make([64])
    x, gp, gv = data(module, np.arange(5))
    p, v = module(x)
    # (a gradient at the outputs that itself has a graph, so that the backward's results would have one)
    (g,) = torch.autograd.grad((p * gp).sum() ** 2 + (v * gv).sum() ** 2, [module.Dense_0.weight], create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_a_backward_after_an_in_place_change_is_refused():
    module = make([64])
    x, gp, gv = data(module, np.arange(5))
    p, v = module(x)
    with torch.no_grad():
        module.DenseResidueBlock_3.Dense_0.weight.mul_(2)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        ((p * gp).sum() + (v * gv).sum()).backward()


def test_deepcopy_and_pickle_carry_the_flag_and_not_the_plan():
    module = make([64, 64])
    x, gp, gv = data(module, np.arange(11) % 6)
    _, _, want = backward(module, x, gp, gv)
    assert "_fused_plan" in module.__dict__
    for clone in (copy.deepcopy(module), pickle.loads(pickle.dumps(module))):
        assert clone.fused_tower_training is True and "_fused_plan" not in clone.__dict__
        _, _, got = backward(clone, x, gp, gv)
        assert clone.fused_last_reason is None and all(torch.equal(g, w) for g, w in zip(got, want))
        assert clone._cached_plan() is not module._cached_plan()


def test_an_adam_step_with_a_tower_that_saw_no_row_leaves_a_finite_state():
    from hironaka_amd import optim
    module = make([32, 32])
    optimizer = optim.Adam(module.parameters(), lr=1e-2)
    x, gp, gv = data(module, [0, 1, 3, 4, 5] * 3)
    before = [q.detach().clone() for q in module.parameters()]
    for _ in range(2):
        optimizer.zero_grad()
        p, v = module(x)
        ((p * gp).sum() + (v * gv).sum()).backward()
        optimizer.step()
    assert module.fused_last_reason is None
    assert all(bool(torch.isfinite(q).all()) for q in module.parameters())
    assert all(bool(torch.isfinite(s).all()) for state in optimizer.state.values() for s in state.values() if torch.is_tensor(s))
    tower2 = [q for b in module.towers[2] for q in b.parameters()]
    for q, b in zip(module.parameters(), before):  # zero gradients, no weight decay: the tower that saw no row stays
        if any(q is t for t in tower2):
            assert torch.equal(q, b)
    assert not torch.equal(module.Dense_0.weight, before[-4])


# ---- through HipTrainer -----------------------------------------------------------------------------------------------

def make_trainer(net_type, fused=True):
    from hironaka_amd.trainer_api import HipTrainer
    return HipTrainer(42, trainer_config(net_type), custom_net=True, fused_tower_training=fused)


@pytest.fixture(scope="module")
def rollouts():
    """simulate's output per net type and role, once (the trainers below start from the same seed)"""
    out = {}
    for net_type in ("custom", "custom_dense"):
        t = make_trainer(net_type)
        out[net_type] = {role: tuple(x.clone() for x in t.simulate(7, role)) for role in ("host", "agent")}
    return out


def _by_hand(t, start, role, samples, batches):
    from hironaka_amd import loss as hkloss
    from hironaka_amd import optim
    from hironaka_amd.functional import get_feature_fn
    from hironaka_amd.trainer_api import get_apply_fn, optim_from_config
    module = copy.deepcopy(start)
    assert module.fused_tower_training is True
    name, kwargs = optim_from_config(t.config[role]["optim"])
    optimizer = getattr(optim, name)(module.parameters(), **kwargs)
    apply_fn = get_apply_fn(role, module, t.spec, feature_fn=get_feature_fn(role, t.spec,
                                                                          scale_observation=t.scale_observation))
    obs, target_policy, target_value = samples
    losses = []
    for rows in batches:
        loss = hkloss.compute_loss(None, apply_fn, (obs[rows], target_policy[rows], target_value[rows]),
                                   hkloss.policy_value_loss)
        assert module.fused_last_reason is None  # the library's forward, with gradients on
        optimizer.zero_grad()
        loss.backward()
        optim.safe_clip_grads_(list(module.parameters()), t.max_grad_norm)
        optimizer.step()
        losses.append(loss.item())
    return _flat(module.parameters()), losses


@pytest.mark.parametrize("net_type,role", [("custom", "agent"), ("custom_dense", "host")])
def test_train_is_the_public_pieces(rollouts, net_type, role):
    t = make_trainer(net_type)
    assert all(m.fused_tower_training is True for m in t.built_nets.values())
    assert all(m.fused_tower_training is False for m in make_trainer(net_type, fused=False).built_nets.values())
    samples = rollouts[net_type][role]
    N, batch = samples[0].shape[0], t.config[role]["batch_size"]
    arange = torch.arange(batch, device="cuda")
    batches = [(i * batch + arange) % N for i in range(3)]
    start = copy.deepcopy(t.built_nets[role])
    before = _flat(start.parameters())
    want_bits, want_losses = _by_hand(t, start, role, samples, batches)
    losses = t.train(5, role, 3, samples)
    assert t.built_nets[role].fused_last_reason is None
    assert losses.tolist() == want_losses and all(x == x for x in want_losses)
    got = _flat(t.built_nets[role].parameters())
    assert got == want_bits and got != before
    # with the flag off the step goes through autograd, as before
    off = make_trainer(net_type, fused=False)
    off.train(5, role, 1, samples)
    assert off.built_nets[role].fused_last_reason == "gradients are on"


@pytest.mark.parametrize("net_type", ["custom", "custom_dense"])
def test_one_gradient_step_replays_from_a_graph(rollouts, net_type):
    from hironaka_amd import ops
    samples = rollouts[net_type]["agent"]
    rows = torch.arange(8, 16, device="cuda")
    eager = make_trainer(net_type)
    eager_loss = eager.train_step("agent", samples, rows).item()
    want = _flat(eager.built_nets["agent"].parameters())

    t = make_trainer(net_type)
    module, opt = t.built_nets["agent"], t.optimizers["agent"]
    start = [p.detach().clone() for p in module.parameters()]
    assert _flat(start) != want

    def undo():
        with torch.no_grad():
            for p, s in zip(module.parameters(), start):
                p.copy_(s)
                opt.state[p]["exp_avg"].zero_()
                opt.state[p]["exp_avg_sq"].zero_()
            opt._blocks[0].copy_(ops.optim_state("cuda"))
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):  # one step on the side stream builds state, tables and descriptors
        t.train_step("agent", samples, rows)
    torch.cuda.current_stream().wait_stream(warm)
    torch.cuda.synchronize()
    undo()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=warm):
        loss = t.train_step("agent", samples, rows)
    assert module.fused_last_reason is None
    undo()
    graph.replay()
    torch.cuda.synchronize()
    assert loss.item() == eager_loss
    assert _flat(module.parameters()) == want
