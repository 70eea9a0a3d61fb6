"""HipTrainer.train / set_optim (hironaka_amd/trainer_api.py; jax_trainer.py:322-375, 727-733) on the device: the loop is
the public pieces and nothing else -- the same batches through compute_loss, backward, safe_clip_grads_ and step on a
deep copy give the same bits --, the draws of random_sampling come from the documented generator, the trained networks
still take the fused forward inside simulate, one step replays from a graph, and what is not served is refused."""
import copy

import pytest
import torch

from hironaka_amd import loss as hkloss
from hironaka_amd import optim, trainer_api
from hironaka_amd.functional import get_feature_fn
from hironaka_amd.trainer_api import HipTrainer, get_apply_fn, optim_from_config, standin_mlp
from test_gpu_trainer import CONFIG

pytestmark = pytest.mark.gpu

BATCH = 32
OPTIMS = {
    "adam": {"name": "adam", "args": {"learning_rate": 1e-2}},
    "adamw": {"name": "adamw", "args": {"learning_rate": 1e-2, "weight_decay": 1e-2}},
    "sgd": {"name": "sgd", "args": {"learning_rate": 1e-2, "momentum": 0.9, "nesterov": True}},
}


def make_trainer(optim_name="adam", **kw):
    section = {"net_arch": [32, 32], "batch_size": BATCH}
    if optim_name is not None:
        section["optim"] = OPTIMS[optim_name]
    return HipTrainer(42, dict(CONFIG, host=dict(section), agent=dict(section)), **kw)


@pytest.fixture(scope="module")
def rollouts():
    """simulate's output for both roles, once: the trainers below start from the same seed, hence the same networks"""
    t = make_trainer()
    return {role: tuple(x.clone() for x in t.simulate(7, role)) for role in ("host", "agent")}


def _flat(params):
    return torch.cat([p.detach().reshape(-1) for p in params]).cpu().numpy().tobytes()


def _by_hand(t, start, role, optim_name, samples, batches):
    """the public pieces on a deep copy of `start`, the network before any step: (parameter bits, losses)"""
    module = copy.deepcopy(start)
    name, kwargs = optim_from_config(OPTIMS[optim_name])
    optimizer = getattr(optim, name)(module.parameters(), **kwargs)
    apply_fn = get_apply_fn(role, module, t.spec, feature_fn=get_feature_fn(role, t.spec,
                                                                          scale_observation=t.scale_observation))
    obs, target_policy, target_value = samples
    losses = []
    for rows in batches:
        loss = hkloss.compute_loss(None, apply_fn, (obs[rows], target_policy[rows], target_value[rows]),
                                   hkloss.policy_value_loss)
        optimizer.zero_grad()
        loss.backward()
        optim.safe_clip_grads_(list(module.parameters()), t.max_grad_norm)
        optimizer.step()
        losses.append(loss.item())
    return _flat(module.parameters()), losses


@pytest.mark.parametrize("optim_name,role", [("adam", "host"), ("adamw", "agent"), ("sgd", "agent"), ("sgd", "host")])
def test_train_is_the_public_pieces(rollouts, optim_name, role):
    t = make_trainer(optim_name)
    assert type(t.optimizers[role]).__name__ == optim_from_config(OPTIMS[optim_name])[0]
    assert getattr(t, f"{role}_optim") is t.optimizers[role] and t.loss_fn is hkloss.policy_value_loss
    N = 70  # no multiple of the batch: the third batch wraps around
    samples = tuple(x[:N] for x in rollouts[role])
    arange = torch.arange(BATCH, device="cuda")
    batches = [(i * BATCH + arange) % N for i in range(3)]
    assert batches[2].tolist() == list(range(64, 70)) + list(range(26))
    start = copy.deepcopy(t.built_nets[role])
    before = _flat(start.parameters())
    want_bits, want_losses = _by_hand(t, start, role, optim_name, samples, batches)
    losses = t.train(5, role, 3, samples)
    assert losses.shape == (3,) and losses.is_cuda and losses.dtype == torch.float32
    assert losses.tolist() == want_losses and all(x == x for x in want_losses)
    got = _flat(t.built_nets[role].parameters())
    assert got == want_bits and got != before
    # a second call starts at row 0 again: its first batch is the by-hand fourth step on rows 0 .. 31
    want_bits4, want_losses4 = _by_hand(t, start, role, optim_name, samples, batches + [arange])
    assert want_losses4[:3] == want_losses
    again = t.train(6, role, 1, samples, save_best=False)
    assert again.tolist() == want_losses4[3:] and _flat(t.built_nets[role].parameters()) == want_bits4


def test_random_sampling_draws_from_the_mask_with_the_documented_generator(rollouts, monkeypatch):
    t = make_trainer("adam")
    samples = rollouts["host"]
    N = samples[0].shape[0]
    allowed = [3, 17, 500, N - 2, N - 1]
    mask = torch.zeros(N, dtype=torch.bool, device="cuda")
    mask[allowed] = True
    drawn = []
    step = t.train_step
    monkeypatch.setattr(t, "train_step", lambda role, rollouts, rows: drawn.append(rows.clone()) or step(role, rollouts, rows))
    t.train(1234, "host", 4, samples, mask=mask, random_sampling=True)
    generator = torch.Generator(device="cuda").manual_seed(1234)
    for rows in drawn:
        want = torch.multinomial(mask.float(), BATCH, replacement=True, generator=generator)
        assert torch.equal(rows, want) and rows.dtype == torch.int64 and rows.shape == (BATCH,)
        assert set(rows.tolist()) <= set(allowed)
    assert len(drawn) == 4 and len({tuple(r.tolist()) for r in drawn}) == 4
    drawn.clear()
    t.train(1234, "host", 1, samples, random_sampling=True)  # no mask: every row may be drawn
    assert len(set(drawn[0].tolist()) - set(allowed)) > 0


def test_simulate_after_train_takes_the_fused_forward_with_new_parameters(rollouts, capsys):
    t = make_trainer("adam")
    losses = t.train(0, "host", 3, rollouts["host"], verbose=1)
    printed = capsys.readouterr().out
    assert printed.count("loss") == 3 and repr(losses[0].item())[:6] in printed
    t.train(0, "agent", 3, rollouts["agent"])
    obs, policy, value = t.simulate(7, "host")
    for role in ("host", "agent"):
        assert t.built_nets[role].fused_last_reason is None, role
    assert policy.shape == rollouts["host"][1].shape and not torch.equal(policy, rollouts["host"][1])
    assert torch.isfinite(value).all()


def test_one_gradient_step_replays_from_a_graph(rollouts):
    samples = tuple(x[:96] for x in rollouts["agent"])
    rows = torch.arange(40, 40 + BATCH, device="cuda")
    eager = make_trainer("adam")
    eager_loss = eager.train_step("agent", samples, rows).item()
    want = _flat(eager.built_nets["agent"].parameters())

    t = make_trainer("adam")
    module, opt = t.built_nets["agent"], t.optimizers["agent"]
    start = [p.detach().clone() for p in module.parameters()]
    assert _flat(start) != want
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):  # one step on the side stream builds state, descriptors and workspaces
        t.train_step("agent", samples, rows)
    torch.cuda.current_stream().wait_stream(warm)
    torch.cuda.synchronize()
    from hironaka_amd import ops
    with torch.no_grad():  # and is undone: parameters, Adam's state and the count
        for p, s in zip(module.parameters(), start):
            p.copy_(s)
            opt.state[p]["exp_avg"].zero_()
            opt.state[p]["exp_avg_sq"].zero_()
        opt._blocks[0].copy_(ops.optim_state("cuda"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=warm):
        loss = t.train_step("agent", samples, rows)
    with torch.no_grad():  # whatever the capture did to them
        for p, s in zip(module.parameters(), start):
            p.copy_(s)
            opt.state[p]["exp_avg"].zero_()
            opt.state[p]["exp_avg_sq"].zero_()
        opt._blocks[0].copy_(ops.optim_state("cuda"))
    graph.replay()
    torch.cuda.synchronize()
    assert loss.item() == eager_loss
    assert _flat(module.parameters()) == want


def test_refusals(rollouts, monkeypatch):
    t = make_trainer(None)  # a config without `optim` builds as before
    assert t.optimizers == {} and set(t.built_nets) == {"host", "agent"}
    with pytest.raises(ValueError, match="optim"):
        t.train(0, "host", 1, rollouts["host"])
    with pytest.raises(ValueError, match="role"):
        t.train(0, "referee", 1, rollouts["host"])
    with pytest.raises(ValueError, match="eps_root"):
        t.set_optim("host", {"name": "adam", "args": {"learning_rate": 1e-3, "eps_root": 1e-8}})
    with pytest.raises(ValueError, match="lion"):
        t.set_optim("host", {"name": "lion", "args": {"learning_rate": 1e-3}})
    assert t.optimizers == {}
    assert isinstance(t.set_optim("host", OPTIMS["sgd"]), optim.SGD) and t.host_optim is t.optimizers["host"]
    monkeypatch.setattr(trainer_api.hkdist, "world", lambda: 2)
    with pytest.raises(NotImplementedError, match="rank"):
        t.train(0, "host", 1, rollouts["host"])
    monkeypatch.undo()
    # the host network given as a callable: nothing to differentiate, whatever the config says
    m, d = CONFIG["max_num_points"], CONFIG["dimension"]
    host_net, host_params = standin_mlp(m * d, 2 ** d - d - 1, 3, width=64)
    given = make_trainer("adam", host_net=host_net, host_params=host_params)
    assert set(given.built_nets) == {"agent"} and set(given.optimizers) == {"agent"}
    with pytest.raises(ValueError, match="callable"):
        given.train(0, "host", 1, rollouts["host"])
    with pytest.raises(ValueError, match="callable"):
        given.set_optim("host", OPTIMS["adam"])
    with pytest.raises(ValueError, match="callable"):
        given.get_apply_fn("host")
    assert given.train(0, "agent", 1, rollouts["agent"]).shape == (1,)
