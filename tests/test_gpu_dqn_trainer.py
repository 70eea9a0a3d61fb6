"""Trainer / DQNTrainer on the GPU: the cases of the reference's test/testTrainer.py restated on the device (its test
config with use_cuda: true, use_tensorboard: false and the replay buffer on the device), then training, evaluation,
action counts, save / load and the learning-rate schedule."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

ROLE = dict(batch_size=2, initial_rollout_size=2, steps_before_rollout=2, steps_before_update_target=2, rollout_size=2,
            max_rollout_step=10, gradient_steps_per_loop=10,
            optim=dict(name="adam", args=dict(lr=1e-8), lr_schedule=dict(mode="exponential", initial_lr=1e-3, rate=0.996)),
            er=0.2, er_schedule=dict(mode="exponential", initial_er=0.5, rate=0.996),
            net_arch=[16, "b", {"repeat": 2, "net_arch": [32, "b"]}, 16, "b"], gamma=0.99, tau=0.9)


def config(roles=("host", "agent"), **over):
    cfg = dict(use_tensorboard=False, layerwise_logging=True, log_time=True, use_cuda=True, scale_observation=True,
               version_string="vanilla_v0", dimension=3, max_num_points=20, max_value=20, max_grad_norm=10,
               replay_buffer=dict(type="base", buffer_size=100, use_cuda=True))
    for role in roles:
        cfg[role] = copy.deepcopy(ROLE)
    cfg.update(over)
    return cfg


@pytest.fixture(scope="module")
def trainer():
    from hironaka_amd import DQNTrainer
    torch.manual_seed(0)
    return DQNTrainer(config())


def params_of(net):
    return [p.detach().clone() for p in net.parameters()]


def test_dummy_module_init(trainer):
    from hironaka_amd import DQNTrainer
    from hironaka_amd.player_modules import RandomAgentModule
    with pytest.raises(AssertionError):
        DQNTrainer(config(("host",)))  # the agent is not in the config and no net is given
    t = DQNTrainer(config(("host",)), agent_net=RandomAgentModule(3, 20, device=torch.device("cuda")))
    assert t.trained_roles == ["host"] and t.get_net_target("agent") is None and t.get_optim("agent") is None
    t = DQNTrainer(config(("host",)), agent_net=trainer.agent_net)
    assert t.trained_roles == ["host"]


def test_replace_nets_and_set_trainable(trainer):
    from hironaka_amd import DQNTrainer
    from hironaka_amd.player_modules import RandomAgentModule
    dummy = lambda: RandomAgentModule(3, 20, device=torch.device("cuda"))  # noqa: E731
    t = DQNTrainer(config(("host",)), agent_net=dummy())
    t.replace_nets(agent_net=trainer.agent_net)
    assert "agent" not in t.trained_roles and t.fused_game.agent_net is trainer.agent_net

    t = DQNTrainer(config(), agent_net=dummy())
    assert "agent" not in t.trained_roles
    with pytest.raises(AssertionError):
        t.set_trainable(["agent"])
    t.replace_nets(agent_net=trainer.agent_net)
    t.set_trainable(["agent"])
    assert "agent" in t.trained_roles and t.get_net_target("agent") is not None


def test_refusals():
    from hironaka_amd import DQNTrainer
    with pytest.raises(TypeError, match="no CPU path"):
        DQNTrainer(config(use_cuda=False))
    with pytest.raises(NotImplementedError):
        DQNTrainer(config(), use_cuda_ids=[0, 1])
    try:
        import tensorboard  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="use_tensorboard"):
            DQNTrainer(config(use_tensorboard=True))


def test_train_moves_parameters_and_fills_the_buffers(trainer):
    from hironaka_amd import _abi as A
    from hironaka_amd import optim
    from hironaka_amd.nets import FusedSequential
    assert trainer.trained_roles == ["host", "agent"]
    for role in ("host", "agent"):
        assert isinstance(trainer.get_net(role), FusedSequential) and isinstance(trainer.get_optim(role), optim.Adam)
        assert trainer.get_replay_buffer(role).device.type == "cuda"
        assert int(trainer.get_replay_buffer(role).cursor[A.HK_REPLAY_TOTAL_PUSHED]) > 0  # the initial roll-out
    before = {role: params_of(trainer.get_net(role)) for role in ("host", "agent")}
    pushed = {role: int(trainer.get_replay_buffer(role).cursor[A.HK_REPLAY_TOTAL_PUSHED]) for role in before}
    steps = trainer.total_num_steps
    trainer.train(3)
    assert trainer.total_num_steps == steps + 3 and len(trainer.losses) == 6
    assert all(torch.isfinite(loss) for loss in trainer.losses)
    for role in before:
        after = params_of(trainer.get_net(role))
        assert any(not torch.equal(a, b) for a, b in zip(after, before[role])), role
        assert all(torch.isfinite(a).all() for a in after), role
        assert int(trainer.get_replay_buffer(role).cursor[A.HK_REPLAY_TOTAL_PUSHED]) > pushed[role], role
        assert not trainer.get_net(role).training and trainer.get_net_target(role) is not None
    assert "train_total" in trainer.time_log


def test_evaluate_rho_and_count_actions(trainer):
    trainer.set_training(False)
    rhos = trainer.evaluate_rho(num_samples=100, max_steps=20)
    assert len(rhos) == 5
    for rho in rhos:
        assert isinstance(rho, torch.Tensor) and rho.dim() == 0 and bool(torch.isfinite(rho)) and float(rho) > 0
    assert trainer.last_evaluation.fused
    for role, width in (("host", 4), ("agent", 3)):
        counts = trainer.count_actions(role, 100, 20, er=0.0)
        assert counts.shape == (width,) and counts.dtype == torch.int64 and trainer.last_evaluation.fused
        assert int(counts.sum()) == int(trainer.last_evaluation.lengths.sum()) > 0
        explored = trainer.count_actions(role, 100, 20, er=0.5)
        assert explored.shape == (width,) and int(explored.sum()) > 0
    trainer.set_training(True)
    assert trainer.evaluate_rho() == [] and trainer.count_actions("host", 10, 5, er=0.0) is None
    trainer.set_training(False)


def test_save_and_load(trainer, tmp_path):
    from hironaka_amd import DQNTrainer
    path = str(tmp_path / "trainer.pt")
    trainer.save(path)
    loaded = DQNTrainer.load(path)
    assert loaded.trained_roles == trainer.trained_roles and loaded.config == trainer.config
    for role in ("host", "agent"):
        for get in ("get_net", "get_net_target"):
            a, b = getattr(trainer, get)(role), getattr(loaded, get)(role)
            assert a is not b
            for (name, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
                assert torch.equal(x, y), (role, get, name)
    clone = trainer.copy()
    assert clone.host_net is not trainer.host_net
    assert all(torch.equal(x, y) for x, y in zip(clone.host_net.parameters(), trainer.host_net.parameters()))


def test_learning_rate_follows_the_scheduler(trainer):
    from hironaka_amd.scheduler import ExponentialLRScheduler
    trainer.set_learning_rate()
    for role in ("host", "agent"):
        scheduler = trainer.get_lr_scheduler(role)
        assert isinstance(scheduler, ExponentialLRScheduler)
        want = 1e-3 * 0.996 ** trainer.total_num_steps + 1e-8 * (1 - 0.996 ** trainer.total_num_steps)
        assert scheduler(trainer.total_num_steps) == want
        assert [g["lr"] for g in trainer.get_optim(role).param_groups] == [want]
    steps = trainer.total_num_steps
    trainer.train(2)
    # as in the reference, the schedule is read at total_num_steps, which a call of train() advances at its end
    want = trainer.get_lr_scheduler("host")(steps)
    assert want != trainer.get_lr_scheduler("host")(steps + 2)
    assert [g["lr"] for g in trainer.get_optim("host").param_groups] == [want]
    assert trainer.get_er("host") == 0.5 * 0.996 ** (steps + 2) + 0.2 * (1 - 0.996 ** (steps + 2))
