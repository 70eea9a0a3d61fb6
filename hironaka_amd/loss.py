"""The loss of the MCTS trainer's gradient step -- ``hironaka/jax/loss.py`` under the reference's names and argument
order: ``policy_value_loss``, ``compute_loss``, ``clip_log``.

Between the network's forward and ``loss.backward()`` the torch composition launches two softmaxes, a product, two means,
a subtraction, an abs, an add and a multiply, and as many again in the backward pass -- plus three gathers where the
batch is a sample of a rollout; for float32 tensors on a HIP device that is ONE launch of ``hk_pv_loss``
(include/hironaka_hip_pvloss.h states the rule), whose outputs are the loss and its gradient with respect to the logits
and the value: ``policy_value_loss`` is a ``torch.autograd.Function`` whose backward scales them by the incoming
gradient.  Anything else (float64, CPU tensors) runs ``torch_policy_value_loss``, the plain composition of the same
formula.  Nothing here synchronises, so a gradient step can be captured into a graph.

Deviations from the reference: every row is evaluated in double and rounded to float32 once (jax evaluates in float32);
a product ``q * logp`` with ``q == 0`` is skipped (jax's ``-0 * -inf`` is NaN where a masked target meets a logit of
``-inf``); the loss is the mean of the rows summed in double in a fixed order, the same bits on every launch; ``index``
is an addition: the rows of the targets and the weight a batch row takes, gathered inside the launch; an index outside
the samples gives a zero row (and a status bit at ``ops.pv_loss``) instead of jax's clamped gather.
"""
from typing import Callable, Optional

import torch
import torch.nn.functional as F

from . import ops


def torch_policy_value_loss(policy_logit: torch.Tensor, value: torch.Tensor, target_policy: torch.Tensor,
                            target_value: torch.Tensor, weight: Optional[torch.Tensor] = None, *,
                            index: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the formula of ``policy_value_loss`` as a composition of torch operators, in the dtype of its arguments, on any
    device; autograd differentiates it"""
    if index is not None:
        target_policy, target_value = target_policy[index], target_value.reshape(-1)[index]
        weight = weight.reshape(-1)[index] if weight is not None else None
    value = value.reshape(value.shape[0])
    q = F.softmax(target_policy, dim=-1)
    logp = F.log_softmax(policy_logit, dim=-1)
    product = torch.where(q == 0, torch.zeros_like(q), q * logp)  # no 0 * inf
    row = -product.sum(dim=-1) / policy_logit.shape[-1] + (value - target_value.reshape(-1)).abs()
    if weight is not None:
        row = row * weight.reshape(-1)
    return row.mean()


class _PvLoss(torch.autograd.Function):
    """forward: the one hk_pv_loss launch; backward: grad_output * dlogits, grad_output * dvalue"""

    @staticmethod
    def forward(ctx, policy_logit, value, target_policy, target_value, weight, index):
        res = ops.pv_loss(policy_logit.detach(), value.detach(), target_policy, target_value, weight, index, want=())
        ctx.save_for_backward(res.dlogits, res.dvalue)
        return res.loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        dlogits, dvalue = ctx.saved_tensors
        return grad_output * dlogits, grad_output * dvalue, None, None, None, None


def _takes_kernel(*tensors) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors if t is not None)


def policy_value_loss(policy_logit: torch.Tensor, value: torch.Tensor, target_policy: torch.Tensor,
                      target_value: torch.Tensor, weight: Optional[torch.Tensor] = None, *,
                      index: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
    """``mean((mean_a(-softmax(target_policy) * log_softmax(policy_logit)) + |value - target_value|) * weight)`` as a
    scalar that ``backward()`` can be called on (hironaka/jax/loss.py:12-24).

    policy_logit [B, A], value [B] or [B, 1]: the network's outputs.  target_policy [N, A], target_value [N], weight [N]
    or None; index [B] int64 or None (then N == B): the sample each batch row takes.  float32 tensors on a HIP device
    take the kernel: the gradient reaches ``policy_logit`` and ``value`` alone, so the targets and the weight must not
    require one, and double backward is not supported.  ``**kwargs`` (the reference passes ``params=``) is ignored."""
    if not _takes_kernel(policy_logit, value, target_policy, target_value, weight):
        return torch_policy_value_loss(policy_logit, value, target_policy, target_value, weight, index=index)
    if index is not None and not (isinstance(index, torch.Tensor) and index.dtype == torch.int64
                                  and index.device == policy_logit.device):
        raise TypeError(f"index must be an int64 tensor on {policy_logit.device}, where the other tensors live. Got "
                        f"{getattr(index, 'dtype', type(index))} on {getattr(index, 'device', 'the host')}.")
    for name, t in (("target_policy", target_policy), ("target_value", target_value), ("weight", weight)):
        if t is not None and t.requires_grad:
            raise ValueError(f"{name} must not require grad: the fused loss differentiates with respect to "
                             "policy_logit and value alone (torch_policy_value_loss differentiates everything).")
    return _PvLoss.apply(policy_logit, value, target_policy, target_value, weight, index)


def compute_loss(params, apply_fn: Callable, sample, loss_fn: Callable, weight=None) -> torch.Tensor:
    """hironaka/jax/loss.py:5-9: ``loss_fn`` of ``apply_fn(obs, params)`` and the sample's targets.  A ``weight`` of None
    goes to ``loss_fn`` as None, which is a weight of ones."""
    obs, target_policy_logits, target_value = sample
    policy_logits, value = apply_fn(obs, params)
    return loss_fn(policy_logits, value, target_policy_logits, target_value, weight=weight, params=params)


def clip_log(x: torch.Tensor, a_min: float = 1e-8) -> torch.Tensor:
    """hironaka/jax/loss.py:27-28"""
    return torch.log(torch.clamp(x, min=a_min))
