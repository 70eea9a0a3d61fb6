"""The learning half of the DQN trainers' loop -- ``DQNTrainer._fit_network`` and ``_update_target_net``
(``hironaka/trainer/dqn_trainer/dqn_trainer.py:45-125, 192-204``) with ``polyak_update`` / ``zip_equal``
(``hironaka/src/_borrowed_fn.py:17-49``) -- under the reference's names, without its timers and tensorboard calls.

Between ``ReplayBuffer.sample`` and ``loss.backward()`` the reference launches a row max, a reshape, ``~dones``, two
multiplies, an add, a gather, ``smooth_l1_loss`` and its mean, and in the backward pass the Huber backward, a zero fill
and a scatter; here that is ONE launch of ``hk_dqn_td`` (include/hironaka_hip_dqn.h), whose outputs are the loss and its
gradient with respect to Q.  ``polyak_update`` is ONE launch of ``hk_polyak_update`` per 64 tensors instead of two per
tensor.  Nothing here synchronises (``td_loss(check=True)`` apart), so a fit step can be captured into a graph.

Deviations: the gradient entry is ``clamp(x, -1, 1) / B`` (torch multiplies by a rounded ``1 / B``: the last bit may
differ); an action outside ``[0, A)`` gives a zero row and a status bit instead of a device-side assertion; the loss is
the mean of the rows summed in double, the same bits on every launch.
"""
from itertools import zip_longest
from typing import Iterable

import torch
from torch import nn

from . import _abi as A
from . import ops


def zip_equal(*iterables):
    """zip that raises ValueError where the iterables have different lengths"""
    sentinel = object()
    for combo in zip_longest(*iterables, fillvalue=sentinel):
        if sentinel in combo:
            raise ValueError("Iterables have different lengths")
        yield combo


def polyak_update(params: Iterable[torch.Tensor], target_params: Iterable[torch.Tensor], tau: float) -> None:
    """``target = tau * param + (1 - tau) * target`` for every pair, in place and under ``no_grad``: tau = 1 copies the
    parameters, tau = 0 changes nothing.  One launch per 64 pairs."""
    with torch.no_grad():
        pairs = list(zip_equal(params, target_params))
        ops.polyak_update([p.data for p, _ in pairs], [t.data for _, t in pairs], tau)


def update_target_net(q_net: nn.Module, q_net_target: nn.Module, tau: float) -> None:
    """the parameters, then the batch-norm running means and variances (dqn_trainer.py:192-204)"""
    polyak_update(q_net.parameters(), q_net_target.parameters(), tau)
    modules, modules_target = [], []
    for module, module_target in zip(q_net.modules(), q_net_target.modules()):
        for key in ["running_mean", "running_var"]:
            if hasattr(module, key):
                modules.append(getattr(module, key))
                modules_target.append(getattr(module_target, key))
    polyak_update(modules, modules_target, tau)


class _TdLoss(torch.autograd.Function):
    """forward: the one hk_dqn_td launch; backward: grad_output * dq"""

    @staticmethod
    def forward(ctx, current_q, next_q, actions, rewards, dones, gamma, check):
        res = ops.dqn_td(current_q.detach(), next_q, actions, rewards, dones, gamma, want=())
        if check and int(res.status.item()) & A.HK_DQN_BAD_ACTION:
            raise IndexError(f"an action lies outside [0, {current_q.shape[1]})")
        ctx.save_for_backward(res.dq)
        return res.loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        (dq,) = ctx.saved_tensors
        return grad_output * dq, None, None, None, None, None, None


def td_loss(current_q: torch.Tensor, next_q: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor,
            dones: torch.Tensor, gamma: float, check: bool = False) -> torch.Tensor:
    """``smooth_l1_loss(gather(current_q, 1, actions), rewards + (~dones) * gamma * next_q.max(1))`` as a scalar that
    ``backward()`` can be called on: the gradient reaches ``current_q`` alone (double backward is not supported).
    ``actions``, ``rewards`` and ``dones`` are [B, 1] or [B], as ``ReplayBuffer.sample`` returns them.  ``next_q`` must
    not require grad (the target net runs under ``no_grad``).  ``check=True`` reads the status word back, which
    synchronises, and raises IndexError for an action outside [0, A)."""
    if next_q.requires_grad:
        raise ValueError("next_q must not require grad: run the target network under torch.no_grad()")
    return _TdLoss.apply(current_q, next_q, actions, rewards, dones, gamma, check)


def td_target(next_q: torch.Tensor, rewards: torch.Tensor, dones: torch.Tensor, gamma: float) -> torch.Tensor:
    """``rewards + (~dones) * gamma * next_q.max(1)`` as [B] (dqn_trainer.py:70-76), from the same launch as td_loss"""
    next_q = next_q.detach()
    zeros = torch.zeros(next_q.shape[0], dtype=torch.int32, device=next_q.device)
    return ops.dqn_td(next_q, next_q, zeros, rewards, dones, gamma, want=("target",)).target


def fit_network(q_net: nn.Module, q_net_target: nn.Module, optimizer: torch.optim.Optimizer, replay_buffer,
                batch_size: int, gamma: float, max_grad_norm: float) -> torch.Tensor:
    """One step of ``DQNTrainer._fit_network``: sample, target net under ``no_grad``, TD loss, ``zero_grad``,
    ``backward``, ``clip_grad_norm_``, ``step`` (the last two in two launches where the optimizer is one of
    ``hironaka_amd.optim``, whose parameters are then taken to be ``q_net``'s).  Returns the loss tensor without reading
    it."""
    observations, actions, rewards, dones, next_observations = replay_buffer.sample(batch_size)
    with torch.no_grad():
        next_q_values = q_net_target(next_observations)
    current_q_values = q_net(observations)
    loss = td_loss(current_q_values, next_q_values, actions, rewards, dones, gamma)
    optimizer.zero_grad()
    loss.backward()
    if hasattr(optimizer, "clip_and_step"):  # hironaka_amd.optim.Adam / SGD: the two lines below in two launches
        optimizer.clip_and_step(max_grad_norm)
    else:
        nn.utils.clip_grad_norm_(q_net.parameters(), max_grad_norm)
        optimizer.step()
    return loss
