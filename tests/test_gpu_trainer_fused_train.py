"""HipTrainer(..., fused_training=True) on the device: the gradient step's forward and backward through the network are
hk_pvgrad_forward / hk_pvgrad_backward, train is still the public pieces and nothing else, one step replays from a graph, the
trained networks still take hk_pvnet_forward inside simulate, and the first step's loss is the unfused trainer's within the
last bits of the two forwards."""
import copy

import pytest
import torch

from hironaka_amd import loss as hkloss
from hironaka_amd import optim
from hironaka_amd.functional import get_feature_fn
from hironaka_amd.trainer_api import HipTrainer, get_apply_fn, optim_from_config
from test_gpu_trainer import CONFIG
from test_gpu_trainer_train import BATCH, OPTIMS, _flat

pytestmark = pytest.mark.gpu
ARCHS = {"test": [32, 32], "wide": [128, 128]}


def make_trainer(arch, fused=True, optim_name="adam"):
    section = {"net_arch": ARCHS[arch], "batch_size": BATCH, "optim": OPTIMS[optim_name]}
    return HipTrainer(42, dict(CONFIG, host=dict(section), agent=dict(section)), fused_training=fused)


@pytest.fixture(scope="module")
def rollouts():
    """simulate's output per architecture and role, once (the trainers below start from the same seed)"""
    out = {}
    for arch in ARCHS:
        t = make_trainer(arch)
        out[arch] = {role: tuple(x[:96].clone() for x in t.simulate(7, role)) for role in ("host", "agent")}
    return out


def _by_hand(t, start, role, samples, batches):
    module = copy.deepcopy(start)
    assert module.fused_training is True
    name, kwargs = optim_from_config(OPTIMS["adam"])
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


@pytest.mark.parametrize("arch,role", [("test", "host"), ("wide", "agent")])
def test_train_is_the_public_pieces(rollouts, arch, role):
    t = make_trainer(arch)
    assert all(m.fused_training is True for m in t.built_nets.values())
    assert all(m.fused_training is False for m in make_trainer(arch, fused=False).built_nets.values())
    N = 70
    samples = tuple(x[:N] for x in rollouts[arch][role])
    arange = torch.arange(BATCH, device="cuda")
    batches = [(i * BATCH + arange) % N for i in range(3)]
    start = copy.deepcopy(t.built_nets[role])
    before = _flat(start.parameters())
    want_bits, want_losses = _by_hand(t, start, role, samples, batches)
    losses = t.train(5, role, 3, samples)
    assert t.built_nets[role].fused_last_reason is None
    assert losses.tolist() == want_losses and all(x == x for x in want_losses)
    got = _flat(t.built_nets[role].parameters())
    assert got == want_bits and got != before


@pytest.mark.parametrize("arch", list(ARCHS))
def test_one_gradient_step_replays_from_a_graph(rollouts, arch):
    from hironaka_amd import ops
    samples = rollouts[arch]["agent"]
    rows = torch.arange(40, 40 + BATCH, device="cuda")
    eager = make_trainer(arch)
    eager_loss = eager.train_step("agent", samples, rows).item()
    want = _flat(eager.built_nets["agent"].parameters())

    t = make_trainer(arch)
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
    with torch.cuda.stream(warm):  # one step on the side stream builds state, descriptors and workspaces
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


def test_simulate_after_train_takes_the_forward_kernel_with_new_parameters(rollouts):
    t = make_trainer("test")
    t.train(0, "host", 3, rollouts["test"]["host"])
    t.train(0, "agent", 3, rollouts["test"]["agent"])
    obs, policy, value = t.simulate(7, "host")
    for role in ("host", "agent"):
        assert t.built_nets[role].fused_last_reason is None, role
    assert not torch.equal(policy[:96], rollouts["test"]["host"][1]) and torch.isfinite(value).all()


@pytest.mark.parametrize("arch", list(ARCHS))
def test_first_step_loss_is_the_unfused_trainers(rollouts, arch):
    """two trainers from one key, one fused and one not: the forwards differ in the last bits only"""
    samples = rollouts[arch]["host"]
    rows = torch.arange(BATCH, device="cuda")
    fused = make_trainer(arch).train_step("host", samples, rows).item()
    plain_trainer = make_trainer(arch, fused=False)
    plain = plain_trainer.train_step("host", samples, rows).item()
    assert plain_trainer.built_nets["host"].fused_last_reason == "gradients are on"
    print(f"{arch}: fused {fused!r} unfused {plain!r}")
    assert abs(fused - plain) <= 32 * 2.0 ** -24 * abs(plain)
