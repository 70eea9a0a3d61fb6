"""The optimiser step of the DQN trainers' loop -- ``nn.utils.clip_grad_norm_(q_net.parameters(), max_grad_norm)`` and
``optimizer.step()`` (``hironaka/trainer/dqn_trainer/dqn_trainer.py:95-98``; ``torch.optim.Adam`` or ``torch.optim.SGD``,
``trainer.py:63``) -- in TWO launches per 64 parameter tensors instead of dozens of foreach passes:
``hk_optim_prepare`` reads the gradients once and leaves the total norm, the clipping coefficient, the step count and
the bias corrections in a 64-byte block on the device, ``hk_optim_apply`` clips the gradients and updates parameters and
state (include/hironaka_hip_optim.h has the rules).  Nothing here synchronises (``state_dict()`` apart, which reads the
step count back), so a whole fit step can be captured into a graph, with a learning-rate schedule when
``param_group["lr"]`` is a one-element tensor on the device.

``Adam`` and ``SGD`` are ``torch.optim.Optimizer`` subclasses whose per-parameter state carries torch's keys, so
``state_dict()`` / ``load_state_dict()`` exchange with ``torch.optim.Adam`` / ``SGD`` in both directions.

``AdamW`` is ``Adam`` behind torch's decoupled decay (one ``torch._foreach_mul_`` per group, then the two launches with
``weight_decay = 0``); its ``state_dict`` exchanges with ``torch.optim.AdamW``.  ``safe_clip_grads_`` is the MCTS trainer's
clipping rule (``hironaka/jax/util.py:426-430``), which is not torch's: the norm from ``hk_optim_prepare``'s pass, the
coefficient on the device, one ``torch._foreach_mul_``.  Followed by ``step()`` that is a second pass over the gradients
(``clip_and_step`` reads them once): the rule differs from the one the kernels have, whose flag and kind spaces are
pinned.

Deviations from torch: a parameter group has ONE step count and one pair of running powers ``beta ** step`` on the
device (torch counts per parameter and evaluates the power in Python: at most ``step * 2**-53`` relative apart; a
parameter whose ``.grad`` is None is skipped as in torch, but does not fall behind in count); Adam's last line is
``p + (-step_size * m) / (sqrt(v) / bias2_sqrt + eps)`` rounded operation by operation, within a unit in the last
place of torch's ``addcdiv_``; SGD's momentum buffer is taken to be fresh (``buf = g``) on the group's first step;
``step()`` alone runs the same two launches with the coefficient fixed at 1.
"""
import copy
from typing import Iterable, Union

import torch

from . import ops

_REFUSED = ("amsgrad", "maximize", "capturable", "differentiable")
_CLIP_STATES = {}  # (device, stream) -> the state block of clip_grad_norm_ calls
_CLIP_CHAINS = {}  # (device, stream, sizes, dtype) -> OptimChain; the chains hold no gradients (set_grads per call)


def _addresses(tensors):
    return tuple(t.data_ptr() for t in tensors)


def clip_grad_norm_(parameters: Union[torch.Tensor, Iterable[torch.Tensor]], max_norm: float) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` for the 2-norm in two launches: the gradients are
    multiplied in place by ``min(1, max_norm / (total_norm + 1e-6))``; returns the total norm as a tensor on the device
    (of no gradient: a zero, as torch does)."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    dev = grads[0].device
    ops._require_device(grads[0], "grad")
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    block = _CLIP_STATES.get(key)
    if block is None:
        block = _CLIP_STATES[key] = ops.optim_state(dev)
    ckey = (key, tuple(g.numel() for g in grads), grads[0].dtype)
    chain = _CLIP_CHAINS.get(ckey)
    if chain is None:
        if len(_CLIP_CHAINS) > 64:
            _CLIP_CHAINS.clear()
        chain = _CLIP_CHAINS[ckey] = ops.OptimChain("scale", grads, state=block, hold_grads=False)
    else:
        chain.set_grads(grads)
    ops.optim_prepare(chain, max_norm=max_norm)
    ops.optim_apply(chain)
    return block[3].to(grads[0].dtype, copy=True)


def safe_clip_grads_(parameters: Union[torch.Tensor, Iterable[torch.Tensor]], max_norm: float) -> torch.Tensor:
    """The MCTS trainer's clipping rule, ``safe_clip_grads`` (hironaka/jax/util.py:426-430), in place: with ``norm`` the
    2-norm of all gradients, they stay as they are where ``norm < max_norm`` and are multiplied by
    ``max_norm / (norm + 1e-9)`` otherwise (so at ``norm == max_norm`` they shrink by a hair).  Not torch's rule, which
    is ``min(1, max_norm / (norm + 1e-6))``.  On a HIP device the norm is ``hk_optim_prepare``'s one pass over the
    gradients, the coefficient a one-element expression on the device (in float64, rounded to the gradients' dtype) and
    the scaling one ``torch._foreach_mul_``; elsewhere it is torch's operators.  Returns the norm as a tensor on the
    gradients' device (of no gradient: a zero).  Nothing here synchronises.

    The reference multiplies by ``max_norm`` and then divides; here the quotient is taken first: the last bit of a
    clipped gradient may differ."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    dev = grads[0].device
    if dev.type == "cuda":
        key = (dev, torch.cuda.current_stream(dev).cuda_stream)
        block = _CLIP_STATES.get(key)
        if block is None:
            block = _CLIP_STATES[key] = ops.optim_state(dev)
        ckey = (key, tuple(g.numel() for g in grads), grads[0].dtype)
        chain = _CLIP_CHAINS.get(ckey)
        if chain is None:
            if len(_CLIP_CHAINS) > 64:
                _CLIP_CHAINS.clear()
            chain = _CLIP_CHAINS[ckey] = ops.OptimChain("scale", grads, state=block, hold_grads=False)
        else:
            chain.set_grads(grads)
        ops.optim_prepare(chain, clip=False)  # the norm alone: the block's coefficient is 1 and is not used
        norm = block[3].clone()
    else:
        norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g.double()) for g in grads]))
    coef = torch.where(norm < max_norm, torch.ones_like(norm), max_norm / (norm + 1e-9))
    torch._foreach_mul_(grads, coef.to(grads[0].dtype))
    return norm.to(grads[0].dtype)


class _TwoLaunch(torch.optim.Optimizer):
    """what Adam and SGD share: a state block and a chain of descriptors per parameter group"""
    _kind = None

    def __init__(self, params, defaults):
        for name in _REFUSED:
            if defaults.get(name):
                raise NotImplementedError(f"{name}=True is not supported by hironaka_amd.optim.{type(self).__name__}.")
        super().__init__(params, defaults)
        self._blocks = {}  # group index -> state block
        self._chains = {}  # group index -> (addresses, OptimChain)

    # -- per kind
    def _init_state(self, p, group):
        raise NotImplementedError

    def _columns(self, ps, group):
        raise NotImplementedError

    def _block_start(self, group, fresh):
        """(step, beta1_pow, beta2_pow) of a group's block, from the per-parameter state"""
        raise NotImplementedError

    def _prepare_args(self, group):
        raise NotImplementedError

    def _apply_args(self, group):
        raise NotImplementedError

    # -- shared
    def _check_group(self, group):
        for name in _REFUSED + ("decoupled_weight_decay",):
            if group.get(name):
                raise NotImplementedError(f"{name}=True is not supported by hironaka_amd.optim.{type(self).__name__}.")

    def _chain(self, k, group):
        ps = [p for p in group["params"] if p.grad is not None]
        if not ps:
            return None
        for p in ps:
            if p.grad.is_sparse:
                raise TypeError(f"hironaka_amd.optim.{type(self).__name__} does not support sparse gradients.")
        if len({p.dtype for p in ps} | {p.grad.dtype for p in ps}) != 1:
            raise TypeError("the parameters and gradients of a group must have one dtype (float32 or float64). Got "
                            f"{sorted({str(p.dtype) for p in ps} | {str(p.grad.dtype) for p in ps})}.")
        fresh = False  # a parameter's state is made here: the group has seen no step
        for p in ps:
            if not self.state[p]:
                self._init_state(p, group)
                fresh = True
        grads = [p.grad for p in ps]
        columns = self._columns(ps, group)
        # the descriptors hold addresses: they serve while parameters and state lie where they lay; the gradients, which
        # backward allocates anew after zero_grad(), are brought on every call and not held
        addresses = _addresses(ps) + tuple(a for col in columns if col for a in _addresses(col))
        cached = self._chains.get(k)
        if cached is not None and cached[0] == addresses:
            cached[1].set_grads(grads)
            return cached[1]
        block = self._blocks.get(k)
        if block is None:
            block = self._blocks[k] = ops.optim_state(ps[0].device, *self._block_start(group, fresh))
        chain = ops.OptimChain(self._kind, grads, [p.data for p in ps], *columns, state=block, hold_grads=False)
        self._chains[k] = (addresses, chain)
        return chain

    def clip_and_step(self, max_grad_norm: float, keep_grads: bool = False):
        """``clip_grad_norm_(params, max_grad_norm)`` and ``step()`` in two launches per group of up to 64 tensors.  Each
        parameter group is clipped by its own norm (the trainers have one group).  The clipped gradients are left in
        ``.grad`` unless ``keep_grads``.  It is a call of ``step``: the step hooks fire and a learning-rate scheduler
        sees that the optimizer has stepped."""
        return self.step(max_grad_norm=max_grad_norm, keep_grads=keep_grads)

    def step(self, closure=None, *, max_grad_norm=None, keep_grads: bool = True):
        """``step()`` alone: the same two launches without clipping (the coefficient is 1 whatever the norm is, so a
        non-finite gradient spoils its own element alone, as in torch; ``total_norm()`` still has the norm)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = max_grad_norm is not None
        with torch.no_grad():
            for k, group in enumerate(self.param_groups):
                self._check_group(group)
                chain = self._chain(k, group)
                if chain is None:
                    continue
                ops.optim_prepare(chain, max_norm=max_grad_norm if clip else float("inf"), clip=clip, lr=group["lr"],
                                  advance=True, **self._prepare_args(group))
                ops.optim_apply(chain, keep_grads=keep_grads, **self._apply_args(group))
        return loss

    def total_norm(self, group: int = 0) -> torch.Tensor:
        """the gradient norm the group's last step saw, as a float64 scalar on the device"""
        return self._blocks[group][3].clone()

    def _sync_counts(self):
        """the device's step counts into the per-parameter state (reads them back: synchronises)"""

    def state_dict(self):
        self._sync_counts()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._blocks.clear()
        self._chains.clear()
        for group in self.param_groups:
            self._check_group(group)


class Adam(_TwoLaunch):
    """``torch.optim.Adam`` (amsgrad off, coupled L2 weight decay) in two launches per step; see the module's text."""
    _kind = "adam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *, amsgrad=False, maximize=False,
                 capturable=False, differentiable=False):
        if not isinstance(lr, torch.Tensor) and lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid eps / weight_decay / betas: {eps}, {weight_decay}, {betas}")
        # torch.optim.Adam's keys with its defaults, so that a state_dict loads into either class
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=None, capturable=capturable, differentiable=differentiable, fused=None,
                        decoupled_weight_decay=False)
        super().__init__(params, defaults)

    def _init_state(self, p, group):
        state = self.state[p]
        state["step"] = torch.tensor(0.0)
        state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _columns(self, ps, group):
        return [self.state[p]["exp_avg"] for p in ps], [self.state[p]["exp_avg_sq"] for p in ps]

    def _block_start(self, group, fresh):
        steps = {int(float(self.state[p]["step"])) for p in group["params"] if self.state.get(p)}
        if len(steps) > 1:
            raise ValueError(f"the parameters of a group must share one step count. Got {sorted(steps)}.")
        step = steps.pop() if steps else 0
        beta1, beta2 = group["betas"]
        return step, float(beta1) ** step, float(beta2) ** step

    def _prepare_args(self, group):
        return dict(beta1=group["betas"][0], beta2=group["betas"][1])

    def _apply_args(self, group):
        return dict(beta1=group["betas"][0], beta2=group["betas"][1], eps=group["eps"],
                    weight_decay=group["weight_decay"])

    def _sync_counts(self):
        for k, group in enumerate(self.param_groups):
            block = self._blocks.get(k)
            if block is None:
                continue
            step = ops.optim_state_read(block)["step"]
            for p in group["params"]:
                if self.state.get(p):
                    self.state[p]["step"] = torch.tensor(float(step))


class AdamW(Adam):
    """``torch.optim.AdamW``: the decoupled decay ``p *= 1 - lr * weight_decay`` of every parameter that has a gradient
    (one ``torch._foreach_mul_`` per group), then ``Adam``'s two launches with ``weight_decay = 0`` -- torch's order and
    torch's factor.  (optax's adamw, which the reference's configs name, subtracts ``lr * (update + weight_decay * p)``
    in one line: the same rule, rounded differently.)  The factor is computed on the host, so a learning rate that lives
    on the device is refused."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, amsgrad=False,
                 maximize=False, capturable=False, differentiable=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                         maximize=maximize, capturable=capturable, differentiable=differentiable)
        # torch.optim.AdamW's own mark, in the defaults and in every group, so that a state_dict loads into either class
        self.defaults["decoupled_weight_decay"] = True
        for group in self.param_groups:
            group["decoupled_weight_decay"] = True
            self._check_group(group)

    def _check_group(self, group):
        for name in _REFUSED:
            if group.get(name):
                raise NotImplementedError(f"{name}=True is not supported by hironaka_amd.optim.AdamW.")
        if isinstance(group["lr"], torch.Tensor):
            raise NotImplementedError("hironaka_amd.optim.AdamW takes the learning rate as a float: the decay factor "
                                      "1 - lr * weight_decay is computed on the host.  (optim.Adam accepts a "
                                      "one-element tensor on the device.)")

    def _apply_args(self, group):
        return dict(super()._apply_args(group), weight_decay=0.0)  # the decay is step()'s first line

    def step(self, closure=None, *, max_grad_norm=None, keep_grads: bool = True):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        with torch.no_grad():
            for group in self.param_groups:
                self._check_group(group)
                ps = [p for p in group["params"] if p.grad is not None]
                if ps and group["weight_decay"] != 0:
                    torch._foreach_mul_(ps, 1 - group["lr"] * group["weight_decay"])
        super().step(max_grad_norm=max_grad_norm, keep_grads=keep_grads)
        return loss


class SGD(_TwoLaunch):
    """``torch.optim.SGD`` in two launches per step; see the module's text."""
    _kind = "sgd"

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 differentiable=False):
        if not isinstance(lr, torch.Tensor) and lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0 or weight_decay < 0.0:
            raise ValueError(f"Invalid momentum / weight_decay: {momentum}, {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=None, differentiable=differentiable, fused=None)
        super().__init__(params, defaults)

    def _init_state(self, p, group):
        if group["momentum"] != 0:
            self.state[p]["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        else:
            self.state[p]["momentum_buffer"] = None

    def _columns(self, ps, group):
        if group["momentum"] == 0:
            return None, None
        for p in ps:
            if self.state[p].get("momentum_buffer") is None:
                self._init_state(p, group)
        return [self.state[p]["momentum_buffer"] for p in ps], None

    def _block_start(self, group, fresh):
        # state that a state_dict brought has seen a step: the group's first step (buf = g) is over
        return (0 if fresh else 1), 1.0, 1.0

    def _prepare_args(self, group):
        return {}

    def _apply_args(self, group):
        return dict(weight_decay=group["weight_decay"], momentum=group["momentum"], dampening=group["dampening"],
                    nesterov=bool(group["nesterov"]))


def from_torch(optimizer: torch.optim.Optimizer):
    """an ``Adam`` / ``SGD`` of this module over the parameters of a ``torch.optim.Adam`` / ``torch.optim.SGD``, with its
    hyper-parameters and state (the state tensors are copies).  A ``torch.optim.AdamW`` is refused here: build an
    ``AdamW`` over its parameters and ``load_state_dict`` its ``state_dict()``."""
    if type(optimizer) is torch.optim.Adam:
        cls, names = Adam, ("lr", "betas", "eps", "weight_decay")
    elif type(optimizer) is torch.optim.SGD:
        cls, names = SGD, ("lr", "momentum", "dampening", "weight_decay", "nesterov")
    else:
        raise NotImplementedError(f"from_torch serves torch.optim.Adam and torch.optim.SGD. Got {type(optimizer)}.")
    groups = []
    for group in optimizer.param_groups:
        for name in _REFUSED + ("decoupled_weight_decay",):
            if group.get(name):
                raise NotImplementedError(f"{name}=True is not supported by hironaka_amd.optim.{cls.__name__}.")
        groups.append({"params": group["params"], **{name: group[name] for name in names}})
    new = cls(groups, **{name: optimizer.defaults[name] for name in names})
    new.load_state_dict(copy.deepcopy(optimizer.state_dict()))  # load_state_dict alone would share the tensors
    return new
