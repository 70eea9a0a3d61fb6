"""What of the MCTS trainer's learning side needs no device: hironaka_amd.loss on CPU tensors against
tests/pv_loss_rules.py, optim.safe_clip_grads_ against the reference's formula in float64, optim.AdamW's construction and
state exchange, and trainer_api.optim_from_config, the mapping behind HipTrainer.set_optim."""
import numpy as np
import pytest
import torch

import hironaka_amd
import pv_loss_rules as R
from hironaka_amd import loss as hkloss
from hironaka_amd import optim
from hironaka_amd.trainer_api import optim_from_config

EPS64 = np.finfo(np.float64).eps


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("weight,index,column", [(False, False, False), (True, True, True), (True, False, True),
                                                 (False, True, False)])
def test_policy_value_loss_on_cpu_tensors_is_the_rule(dtype, weight, index, column):
    rng = np.random.default_rng(21)
    for B, A in [(1, 1), (6, 3), (33, 26)]:
        logits, value, tp, tv, w, idx = R.case(rng, B, A, weight=weight, index=index)
        want = R.pv_loss(logits, value, tp, tv, w, idx)
        t = lambda a: None if a is None else torch.from_numpy(a).to(dtype)  # noqa: E731
        x, v = t(logits).requires_grad_(), (t(value).reshape(B, 1) if column else t(value)).requires_grad_()
        got = hkloss.policy_value_loss(x, v, t(tp), t(tv), t(w), index=None if idx is None else torch.from_numpy(idx),
                                       params=None)
        assert got.shape == () and got.dtype == dtype
        got.backward()
        assert v.grad.shape == v.shape
        tol = 64 * (EPS64 if dtype == torch.float64 else np.finfo(np.float32).eps)
        scale = max(1.0, float(np.abs(want.row_loss).max()))
        assert abs(got.item() - want.loss) <= tol * scale, (B, A)
        assert np.abs(x.grad.numpy() - want.dlogits).max() <= tol, (B, A)
        assert np.abs(v.grad.numpy().reshape(B) - want.dvalue).max() <= tol, (B, A)


def test_compute_loss_and_clip_log():
    seen = {}

    def apply_fn(obs, params):
        seen["apply"] = (obs, params)
        return obs[:, :3] * params, obs[:, 3]

    def loss_fn(policy_logits, value, target_policy, target_value, weight=None, **kwargs):
        seen["loss"] = (weight, kwargs)
        return hkloss.policy_value_loss(policy_logits, value, target_policy, target_value, weight, **kwargs)

    g = torch.Generator().manual_seed(3)
    obs, tp, tv = torch.randn(5, 4, generator=g), torch.randn(5, 3, generator=g), torch.randn(5, generator=g)
    params = torch.tensor(2.0, requires_grad=True)
    got = hkloss.compute_loss(params, apply_fn, (obs, tp, tv), loss_fn)
    assert seen["apply"][0] is obs and seen["apply"][1] is params and seen["loss"][0] is None
    assert seen["loss"][1] == {"params": params}
    want = hkloss.torch_policy_value_loss(obs[:, :3] * 2.0, obs[:, 3], tp, tv)
    assert torch.equal(got.detach(), want)
    got.backward()
    assert params.grad is not None and torch.isfinite(params.grad)
    w = torch.rand(5, generator=g)
    assert torch.equal(hkloss.compute_loss(params, apply_fn, (obs, tp, tv), loss_fn, weight=w).detach(),
                       hkloss.torch_policy_value_loss(obs[:, :3] * 2.0, obs[:, 3], tp, tv, w))
    x = torch.tensor([0.0, 1e-9, 1e-8, 0.5, 2.0])
    assert torch.equal(hkloss.clip_log(x), torch.log(torch.tensor([1e-8, 1e-8, 1e-8, 0.5, 2.0])))
    assert torch.equal(hkloss.clip_log(x, a_min=1.0), torch.log(torch.tensor([1.0, 1.0, 1.0, 1.0, 2.0])))
    for name in ("policy_value_loss", "compute_loss", "clip_log"):
        assert getattr(hironaka_amd, name) is getattr(hkloss, name) and name in hironaka_amd.__all__
    for name in ("AdamW", "safe_clip_grads_"):
        assert getattr(hironaka_amd, name) is getattr(optim, name) and name in hironaka_amd.__all__


def _params_with_grads(scale, dtype):
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.zeros(shape, dtype=dtype)) for shape in [(3, 4), (5,), (2, 2, 2)]]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g, dtype=torch.float64).to(dtype)
    norm = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ps)))
    for p in ps:
        p.grad.mul_(scale / norm)
    return ps + [torch.nn.Parameter(torch.zeros(3, dtype=dtype))]  # the last one has no gradient


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_safe_clip_grads_below_at_and_above_max_norm(dtype):
    """jax/util.py:426-430: g where norm < max_norm, else g * max_norm / (norm + 1e-9)"""
    eps = EPS64 if dtype == torch.float64 else np.finfo(np.float32).eps
    for scale, max_norm in [(0.5, 1.0), (0.999, 1.0), (3.0, 1.0), (40.0, 0.5), (2.0, 2.0), (0.0, 1.0)]:
        ps = _params_with_grads(scale, dtype) if scale else _params_with_grads(1.0, dtype)
        if not scale:
            for p in ps[:-1]:
                p.grad.zero_()
        before = [p.grad.double().clone() for p in ps[:-1]]
        norm = float(torch.sqrt(sum((g ** 2).sum() for g in before)))
        got = optim.safe_clip_grads_(ps, max_norm)
        assert got.shape == () and got.dtype == dtype and abs(float(got) - norm) <= 8 * eps * max(norm, 1.0)
        assert ps[-1].grad is None
        for p, g in zip(ps[:-1], before):
            if norm < max_norm:
                assert torch.equal(p.grad.double(), g), (scale, max_norm)  # untouched, to the bit
            else:
                want = g * max_norm / (norm + 1e-9)
                assert (p.grad.double() - want).abs().max() <= 4 * eps * want.abs().max(), (scale, max_norm)
    # norm == max_norm exactly (3-4-5): not `<`, so the gradients shrink by the hair the 1e-9 makes
    p = torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))
    p.grad = torch.tensor([3.0, 4.0], dtype=torch.float64)
    assert float(optim.safe_clip_grads_(p, 5.0)) == 5.0
    assert torch.equal(p.grad, torch.tensor([3.0, 4.0], dtype=torch.float64) * (5.0 / (5.0 + 1e-9)))
    assert bool((p.grad < torch.tensor([3.0, 4.0], dtype=torch.float64)).all())
    # torch's rule differs there and just above: min(1, max_norm / (norm + 1e-6))
    assert float(optim.safe_clip_grads_([torch.nn.Parameter(torch.zeros(2))], 1.0)) == 0.0  # no gradient at all


def test_adamw_construction_and_state_exchange():
    ps = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]
    ours = optim.AdamW(ps, lr=0.1, betas=(0.8, 0.9), eps=1e-6)
    assert isinstance(ours, optim.Adam) and ours.defaults["weight_decay"] == 1e-2
    theirs = torch.optim.AdamW(ps, lr=0.1, betas=(0.8, 0.9), eps=1e-6)
    assert ours.defaults == theirs.defaults  # decoupled_weight_decay included
    assert ours.state_dict()["param_groups"] == theirs.state_dict()["param_groups"]
    assert ours._apply_args(ours.param_groups[0])["weight_decay"] == 0.0  # the kernel's coupled decay is off
    for p in ps:
        p.grad = torch.full_like(p, 0.5)
    theirs.step()
    ours.load_state_dict(theirs.state_dict())
    assert all(torch.equal(ours.state[p]["exp_avg"], theirs.state[p]["exp_avg"]) for p in ps)
    assert ours._block_start(ours.param_groups[0], False) == (1, 0.8, 0.9)
    back = torch.optim.AdamW(ps, lr=1.0)
    back.load_state_dict(ours.state_dict())
    assert back.param_groups[0]["lr"] == 0.1 and back.param_groups[0]["decoupled_weight_decay"] is True
    with pytest.raises(ValueError):
        optim.AdamW(ps, lr=-1.0)
    with pytest.raises(ValueError):
        optim.AdamW(ps, weight_decay=-1.0)
    for name in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError):
            optim.AdamW(ps, **{name: True})
    with pytest.raises(NotImplementedError, match="float"):
        optim.AdamW(ps, lr=torch.tensor(0.1))
    ours.param_groups[0]["lr"] = torch.tensor(0.1)
    with pytest.raises(NotImplementedError, match="float"):
        ours.step()
    # a state of torch's AdamW does not load into the coupled Adam, nor the other way round silently
    with pytest.raises(NotImplementedError):
        optim.Adam(ps, lr=0.1).load_state_dict(theirs.state_dict())


def test_optim_from_config_names_arguments_and_refusals():
    assert optim_from_config({"name": "adam", "args": {"learning_rate": 1e-3}}) == \
        ("Adam", {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8})
    assert optim_from_config({"name": "adam", "args": {"learning_rate": 3e-4, "b1": 0.5, "b2": 0.75, "eps": 1e-5,
                                                       "eps_root": 0.0, "mu_dtype": None}}) == \
        ("Adam", {"lr": 3e-4, "betas": (0.5, 0.75), "eps": 1e-5})
    assert optim_from_config({"name": "adamw", "args": {"learning_rate": 1e-3}}) == \
        ("AdamW", {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 1e-4})  # optax's default
    assert optim_from_config({"name": "adamw", "args": {"learning_rate": 1, "weight_decay": 0.5, "mask": None}}) == \
        ("AdamW", {"lr": 1.0, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0.5})
    assert optim_from_config({"name": "sgd", "args": {"learning_rate": 0.1}}) == \
        ("SGD", {"lr": 0.1, "momentum": 0.0, "nesterov": False})
    assert optim_from_config({"name": "sgd", "args": {"learning_rate": 0.1, "momentum": None}})[1]["momentum"] == 0.0
    assert optim_from_config({"name": "sgd", "args": {"learning_rate": 0.1, "momentum": 0.9, "nesterov": True,
                                                      "accumulator_dtype": None}}) == \
        ("SGD", {"lr": 0.1, "momentum": 0.9, "nesterov": True})
    ps = [torch.nn.Parameter(torch.ones(3))]
    for config in ({"name": "adam", "args": {"learning_rate": 1e-3}}, {"name": "adamw", "args": {"learning_rate": 1e-3}},
                   {"name": "sgd", "args": {"learning_rate": 0.1, "momentum": 0.9, "nesterov": True}}):
        name, kwargs = optim_from_config(config)
        built = getattr(optim, name)(ps, **kwargs)
        assert type(built).__name__ == name and built.param_groups[0]["lr"] == kwargs["lr"]
    with pytest.raises(ValueError, match="rmsprop"):
        optim_from_config({"name": "rmsprop", "args": {"learning_rate": 1e-3}})
    with pytest.raises(KeyError):
        optim_from_config({"args": {"learning_rate": 1e-3}})
    for name, key, value in [("adam", "eps_root", 1e-8), ("adam", "mu_dtype", "bfloat16"), ("adam", "weight_decay", 0.1),
                             ("adam", "nesterov", True), ("adamw", "mask", [True]), ("sgd", "b1", 0.9),
                             ("sgd", "accumulator_dtype", "float16"), ("adamw", "momentum", 0.9), ("sgd", "lr", 0.1)]:
        with pytest.raises(ValueError, match=key):
            optim_from_config({"name": name, "args": {"learning_rate": 1e-3, key: value}})
    for name in ("adam", "adamw", "sgd"):
        with pytest.raises(ValueError, match="learning_rate"):
            optim_from_config({"name": name, "args": {}})
        with pytest.raises(ValueError, match="learning_rate"):
            optim_from_config({"name": name, "args": {"learning_rate": lambda step: 1e-3}})
