"""The policy-value networks of the MCTS trainer -- the reference's hironaka/jax/net.py (DenseResNet, DenseNet and their
blocks) as torch modules under the reference's names, whose gradient-free float32 forward on a HIP device is ONE
hk_pvnet_forward launch (include/hironaka_hip_pvnet.h states the rule).

    net = DenseResNet(output_size, net_arch, spec=(max_num_points, dimension), role="host")
    policy_logits, value = net(features)            # [B, output_size], [B, 1]

What differs from flax, and why:
  * torch cannot infer the input width at the first call: `input_dim` is required, or follows from `spec` and `role`
    (host: max_num_points * dimension, agent: that plus dimension);
  * the module holds its parameters, so `forward(x, params=None, train=True)` accepts and ignores `params` -- which makes
    an instance a valid `host_net` / `agent_net` of HipTrainer;
  * a normed width that is no multiple of 32 raises at construction (flax raises at the first call);
  * the initial values are flax's default DISTRIBUTIONS (lecun_normal kernels, zero biases, unit scales) drawn from a
    seeded torch.Generator: jax's own draws cannot be reproduced here.

CustomNet (hironaka/jax/net.py:73-103; net_type custom / custom_dense) has one tower per point count.  The reference runs
every tower on every row and multiplies all but one result by a one-hot of the row's count; the kernel path
(hk_customnet_forward, include/hironaka_hip_customnet.h: two launches) groups the rows by their count and runs ONE tower per
row.  A row whose points are ALL there (count == max_num_points) gets no tower at all -- the reference's one_hot(m, m) is
all zero -- and its heads see zeros and the extra features: followed here, in both paths.  build_net and HipTrainer build
it only with `custom_net=True`; without the flag both net types raise as before.  Its gradient step is torch autograd
through the reference's formula unless `CustomNet.fused_tower_training` is set (off by default): then the forward and backward
are hk_customgrad_forward / hk_customgrad_backward (include/hironaka_hip_customgrad.h), one tower per row both ways."""
import copy
import math
from functools import partial
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import _abi as A
from .trainer_api import get_apply_fn  # noqa: F401  (hironaka/jax/net.py:110-133)

NUM_GROUPS = 32
EPS = 1e-6  # flax's GroupNorm default
NORMED_WIDTHS = A.PVNET_NORMED_WIDTHS


def lecun_normal_(weight: torch.Tensor, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """flax's default kernel initialiser on a [out, in] weight: a normal of variance 1 / fan_in truncated at two
    standard deviations (the 0.8796... restores the variance the truncation takes)"""
    std = math.sqrt(1.0 / weight.shape[1]) / 0.87962566103423978
    return nn.init.trunc_normal_(weight, mean=0.0, std=std, a=-2 * std, b=2 * std, generator=generator)


def _dense(k: int, n: int, generator) -> nn.Linear:
    lin = nn.Linear(k, n)
    with torch.no_grad():
        lecun_normal_(lin.weight, generator)
        lin.bias.zero_()
    return lin


def _norm(n: int) -> nn.GroupNorm:
    return nn.GroupNorm(NUM_GROUPS, n, eps=EPS)  # (ValueError where n is no multiple of 32; scale 1, bias 0)


class DenseResidueBlock(nn.Module):
    """relu(o + GN(Dense(relu(GN(Dense(x)))))) with o = x, or GN(Dense(x)) (res_proj / norm_proj) where the block changes
    the width (hironaka/jax/net.py:14-33); children under flax's names"""

    def __init__(self, in_features: int, features: int, generator: Optional[torch.Generator] = None):
        super().__init__()
        self.in_features, self.features = in_features, features
        self.Dense_0, self.GroupNorm_0 = _dense(in_features, features, generator), _norm(features)
        self.Dense_1, self.GroupNorm_1 = _dense(features, features, generator), _norm(features)
        if in_features != features:
            self.res_proj, self.norm_proj = _dense(in_features, features, generator), _norm(features)
        else:
            self.res_proj = self.norm_proj = None

    def forward(self, x):
        y = self.GroupNorm_1(self.Dense_1(torch.relu(self.GroupNorm_0(self.Dense_0(x)))))
        if self.res_proj is not None:
            x = self.norm_proj(self.res_proj(x))
        return torch.relu(x + y)


class DenseBlock(nn.Module):
    """relu(Dense(x)) (hironaka/jax/net.py:36-45)"""

    def __init__(self, in_features: int, features: int, generator: Optional[torch.Generator] = None):
        super().__init__()
        self.in_features, self.features = in_features, features
        self.Dense_0 = _dense(in_features, features, generator)

    def forward(self, x):
        return torch.relu(self.Dense_0(x))


def input_dim_of(spec: Sequence[int], role: str) -> int:
    if role not in ("host", "agent"):
        raise ValueError(f"role must be either host or agent. Got {role}.")
    m, d = spec
    return m * d + (d if role == "agent" else 0)


class _PolicyValueNet(nn.Module):
    """What DenseResNet and CustomNet share: the attributes of the kernel's path, the copies that drop the cached plan,
    and the flax parameter trees.  A subclass has `_block_names` (its blocks in flax's order), the heads `Dense_0` /
    `Dense_1` and `_reason()`."""

    fused_enabled = True
    fused_training = False
    fused_tower_training = False
    fused_last_reason = None

    @property
    def blocks(self) -> List[nn.Module]:
        return [getattr(self, name) for name in self._block_names]

    @property
    def fused_reason(self) -> Optional[str]:
        return self._reason()

    def _tensors(self):
        return [t for m in self.modules() for t in list(m._parameters.values()) + list(m._buffers.values())
                if t is not None and t.is_floating_point()]

    def _records_graph(self) -> bool:
        """whether a call now would record a graph over the parameters"""
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def _blocks_reason(self, blocks, input_widths) -> Optional[str]:
        """why the kernels do not serve these blocks behind inputs of `input_widths`, None: they do"""
        if any(type(b) not in (DenseResidueBlock, DenseBlock) for b in blocks):
            return "a block that is neither a DenseResidueBlock nor a DenseBlock"
        widths = list(input_widths) + [b.Dense_0.out_features for b in blocks]
        if max(widths) > A.HK_PVNET_MAX_WIDTH or min(widths) < 1:
            return f"a width outside 1..{A.HK_PVNET_MAX_WIDTH}"
        if any(type(b) is DenseResidueBlock and b.Dense_0.out_features not in NORMED_WIDTHS for b in blocks):
            return f"a normed width that is none of {NORMED_WIDTHS}"
        if any(gn.num_groups != NUM_GROUPS or not gn.affine
               for b in blocks for gn in b.children() if isinstance(gn, nn.GroupNorm)):
            return f"a group norm that is not GroupNorm({NUM_GROUPS}) with scale and bias"
        if not 1 <= self.Dense_0.out_features <= A.HK_PVNET_MAX_WIDTH - 1 or self.Dense_1.out_features != 1:
            return f"a policy head outside 1..{A.HK_PVNET_MAX_WIDTH - 1} logits, or a value head of more than one"
        tensors = self._tensors()
        if any(t.dtype != torch.float32 for t in tensors):
            return "parameters are not float32"
        if len({t.device for t in tensors}) > 1:
            return "parameters live on more than one device"
        return None

    @staticmethod
    def _block_records(blocks):
        """ops.PvnetBlock's fields for every block"""
        def dn(lin, gn=None):
            return (lin.weight, lin.bias) + ((gn.weight, gn.bias) if gn is not None else (None, None))
        records = []
        for b in blocks:
            if type(b) is DenseBlock:
                records.append(("dense", dn(b.Dense_0), None, None, EPS))
            else:
                records.append(("residue", dn(b.Dense_0, b.GroupNorm_0), dn(b.Dense_1, b.GroupNorm_1),
                                dn(b.res_proj, b.norm_proj) if b.res_proj is not None else None, b.GroupNorm_0.eps))
        return records

    def _records(self):
        return (self._block_records(self.blocks), (self.Dense_0.weight, self.Dense_0.bias),
                (self.Dense_1.weight, self.Dense_1.bias))

    def _plan_key(self):
        """what a cached plan was built from: one data_ptr() and shape per tensor the modules hold now, and the eps"""
        records, policy, value = self._records()
        flat = [x for r in records for part in r for x in (part if isinstance(part, tuple) else (part,))] + list(policy + value)
        return tuple((x.data_ptr(), tuple(x.shape)) if isinstance(x, torch.Tensor) else x for x in flat)

    def _input_reason(self, x, dev) -> Optional[str]:
        if dev.type != "cuda":
            return f"parameters live on {dev}, not on a HIP device"
        if not (isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.device == dev and x.dim() >= 2
                and not (torch.is_grad_enabled() and x.requires_grad)):
            return f"the input is not float32 on {dev} with a batch dimension, or requires a gradient"
        if math.prod(x.shape[1:]) != self.input_dim:
            return f"the input is not {self.input_dim} wide"
        return None

    def __deepcopy__(self, memo):
        # the copy builds its own table (this one's points at this module's tensors)
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k not in ("_fused_plan", "_fused_check"):
                new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_fused_plan", None)
        state.pop("_fused_check", None)
        return state

    # ---- flax parameter trees -----------------------------------------------------------------------------------
    def _flax_leaves(self):
        """(scope path, kind, tensor): kind "kernel" ([in, out]: the weight transposed), "bias" or "scale" """
        for name, block in zip(self._block_names, self.blocks):
            for child, module in block.named_children():
                if isinstance(module, nn.Linear):
                    yield (name, child), "kernel", module.weight
                    yield (name, child), "bias", module.bias
                elif isinstance(module, nn.GroupNorm):
                    yield (name, child), "scale", module.weight
                    yield (name, child), "bias", module.bias
        for child in ("Dense_0", "Dense_1"):
            yield (child,), "kernel", getattr(self, child).weight
            yield (child,), "bias", getattr(self, child).bias

    def flax_params(self) -> Dict[str, Any]:
        """The parameters as a flax parameter dict of numpy arrays, `{"params": {...}}`: block scopes
        `DenseResidueBlock_i` / `DenseBlock_i` holding `Dense_0`, `GroupNorm_0`, `Dense_1`, `GroupNorm_1`, `res_proj`,
        `norm_proj`; the heads `Dense_0` (policy) and `Dense_1` (value); every `kernel` is [in, out], the transpose of
        the nn.Linear weight.  These scope names are flax's compact auto-naming as I know it.  flax is not on this
        machine, so nobody here has checked them against a real checkpoint."""
        tree: Dict[str, Any] = {}
        for path, kind, t in self._flax_leaves():
            node = tree
            for scope in path:
                node = node.setdefault(scope, {})
            a = t.detach().cpu().numpy()
            node[kind] = np.ascontiguousarray(a.T) if kind == "kernel" else a.copy()
        return {"params": tree}

    def load_flax_params(self, tree: Dict[str, Any]) -> "_PolicyValueNet":
        """Copy a flax parameter dict (flax_params' layout, with or without the outer "params") into the module, in
        place; a missing scope, a leaf of another shape or a scope the module has no use for raises.  The same caveat
        about the scope names as flax_params: not checked against a real checkpoint."""
        tree = tree.get("params", tree)
        seen = set()
        with torch.no_grad():
            for path, kind, t in self._flax_leaves():
                node = tree
                for scope in path:
                    if scope not in node:
                        raise KeyError(f"the tree has no scope {'/'.join(path)}")
                    node = node[scope]
                if kind not in node:
                    raise KeyError(f"the tree has no {'/'.join(path)}/{kind}")
                a = np.asarray(node[kind])
                a = a.T if kind == "kernel" else a
                if tuple(a.shape) != tuple(t.shape):
                    raise ValueError(f"{'/'.join(path)}/{kind}: expected {tuple(t.shape)}"
                                     f"{' (transposed)' if kind == 'kernel' else ''}, got {tuple(a.shape)}")
                t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(t.dtype))
                seen.add(path)

        def scopes(node, path=()):
            for key, sub in node.items():
                if isinstance(sub, dict):
                    yield from scopes(sub, path + (key,))
            if node and not any(isinstance(sub, dict) for sub in node.values()):
                yield path
        extra = [p for p in scopes(tree) if p not in seen]
        if extra:
            raise KeyError(f"the tree has scopes this module has none for: {['/'.join(p) for p in extra]}")
        return self


class DenseResNet(_PolicyValueNet):
    """A trunk of `block_cls` blocks of the widths `net_arch`, a policy head `Dense_0` of `output_size` logits and a
    value head `Dense_1` behind a tanh (hironaka/jax/net.py:48-67).  Children: `DenseResidueBlock_i` / `DenseBlock_i`,
    `Dense_0`, `Dense_1`.

    `forward(x, params=None, train=True) -> (p [B, output_size], v [B, 1])` takes the kernel's path when gradients are
    off or no parameter requires one, parameters and input are float32 on one HIP device, and the shapes are within the
    kernel's limits (input and widths up to 256, normed widths 32 / 64 / 128 / 256, up to 32 blocks, up to 255
    logits); otherwise it IS the plain composition of the children.  `fused_reason` says why the MODULE is not served
    (None: it is), `fused_last_reason` why the last CALL was not (None: it was); `fused_enabled = False` pins torch's
    path.  The two paths differ in the last bits.  The block table is built once and rebuilt when a parameter's
    `data_ptr()` changed (assigned anew, `.to()`); in-place updates need nothing.  Nothing here synchronises.

    With `fused_training = True` (off by default) a call with gradients on is served too: the forward and backward are a
    once-differentiable autograd.Function over ops.pvnet_train_forward / ops.pvnet_backward (include/hironaka_hip_pvgrad.h
    states the rule) where the module is servable apart from "gradients are on" and the input is float32 on the device,
    requires no gradient and has at most HK_PVGRAD_MAX_BATCH rows; parameters that require no gradient get None.  Anything
    else is torch's path, with `fused_last_reason` saying why."""

    def __init__(self, output_size: int, net_arch: List[int], spec: Optional[Tuple[int, int]] = None,
                 input_dim: Optional[int] = None, block_cls=DenseResidueBlock, role: Optional[str] = None, seed: int = 0):
        super().__init__()
        if input_dim is None:
            if spec is None or role is None:
                raise ValueError("DenseResNet needs input_dim, or spec and role to take it from (torch cannot infer the "
                                 "input width at the first call as flax does).")
            input_dim = input_dim_of(spec, role)
        self.output_size, self.net_arch, self.spec, self.input_dim = int(output_size), [int(n) for n in net_arch], spec, int(input_dim)
        generator = torch.Generator().manual_seed(int(seed) % (1 << 63))
        self._block_names = []
        k = self.input_dim
        for i, n in enumerate(self.net_arch):
            name = f"{block_cls.__name__}_{i}"
            self.add_module(name, block_cls(k, n, generator))
            self._block_names.append(name)
            k = n
        self.Dense_0 = _dense(k, self.output_size, generator)
        self.Dense_1 = _dense(k, 1, generator)

    # ---- torch's path: the plain composition of the children -----------------------------------------------------
    def plain_forward(self, x):
        x = x.flatten(1)
        for block in self.blocks:
            x = block(x)
        return self.Dense_0(x), torch.tanh(self.Dense_1(x))

    # ---- the kernel's path --------------------------------------------------------------------------------------
    def _reason(self) -> Optional[str]:
        if not self.fused_enabled:
            return "fused_enabled is False"
        blocks = self.blocks
        if not 1 <= len(blocks) <= A.HK_PVNET_MAX_BLOCKS:
            return f"not 1 to {A.HK_PVNET_MAX_BLOCKS} blocks"
        reason = self._blocks_reason(blocks, [self.input_dim])
        if reason is None and not self.fused_training and self._records_graph():
            return "gradients are on"
        return reason

    def _cached_plan(self):
        """the block table, rebuilt when the module no longer is what the table was built from: a tensor the modules hold
        NOW lies elsewhere (one data_ptr() per tensor per call), or a shape or an eps changed.  In-place updates change
        no address and need nothing."""
        from . import ops
        key = self._plan_key()
        plan = self.__dict__.get("_fused_plan")
        if plan is None or plan.key != key:
            records, policy, value = self._records()
            plan = ops.PvnetPlan([ops.PvnetBlock(*r) for r in records], policy, value)
            plan.key = key
            self.__dict__["_fused_plan"] = plan
        return plan

    def forward(self, x, params: Any = None, train: bool = True):
        reason = self._reason()
        if reason is None:
            reason = self._input_reason(x, self.Dense_0.weight.device)
        grads = reason is None and self._records_graph()  # (only with fused_training: _reason)
        if grads:
            records, policy, value = self._records()
            params = [t for r in records for part in r[1:4] if part is not None for t in part if t is not None]
            params += list(policy + value)
            if x.shape[0] > A.HK_PVGRAD_MAX_BATCH:
                reason = f"more than {A.HK_PVGRAD_MAX_BATCH} rows with gradients on"
            elif len({id(p) for p in params}) < len(params):
                reason = "a parameter is used twice and gradients are on"
        self.__dict__["fused_last_reason"] = reason
        if reason is not None:
            return self.plain_forward(x)
        from . import ops
        plan = self._cached_plan()
        if grads:
            p, v = _PvnetTrainFunction.apply(plan, x, *plan.params)
        else:
            p, v = ops.pvnet_forward(x, plan)
        return p, v.unsqueeze(1)


class CustomNet(_PolicyValueNet):
    """One tower of `block_cls` blocks of the widths `net_arch` per point count, and a policy head `Dense_0` and a value
    head `Dense_1` (behind a tanh) over the chosen tower's result and the extra features (hironaka/jax/net.py:73-103).
    A row is `m * d` point coordinates (m, d = spec) and `extra_dim` more features (0 for the host, d for the agent: it
    follows from `role` where it is not given).  With c = #{i < m : x[i * d] >= 0}, a row of c < m runs tower c on its
    first c + 1 points ++ extra; A ROW OF c == m RUNS NO TOWER: the reference's one_hot(m, m) is all zero, so its heads
    see zeros ++ extra.  That is the reference's behaviour and is followed, in both paths.

    Children under flax's compact auto-names: tower t's block l is `DenseResidueBlock_{t * L + l}` /
    `DenseBlock_{t * L + l}` with L = len(net_arch); the heads are `Dense_0` (n_last + extra_dim inputs) and `Dense_1`.
    `flax_params()` / `load_flax_params()` as DenseResNet's, with the same caveat about the names.

    `forward(x, params=None, train=True) -> (p [B, output_size], v [B, 1])` takes the kernels' path
    (ops.customnet_forward: two launches, one tower per row) under DenseResNet's conditions: gradients off or no
    parameter requires one, float32 on one HIP device, and 1 <= m <= 64, d >= 2, m * d + extra_dim and n_last + extra_dim
    up to 256, widths and normed widths as DenseResNet's.  Otherwise it is `plain_forward`, the reference's formula: all
    towers, the mask, the sum -- differentiable, and the path HipTrainer.train takes through autograd.  `fused_enabled`,
    `fused_reason` and `fused_last_reason` are DenseResNet's; `fused_training` exists because HipTrainer sets it and has
    no effect: with gradients on `fused_last_reason` says "gradients are on".  The two paths differ in the last bits, and
    where a row holds a NaN: the mask multiplies the other towers' NaN by zero, which is NaN.  Nothing here synchronises.

    With `fused_tower_training = True` (a class attribute, off by default; HipTrainer(..., fused_tower_training=True) sets
    it) a call with gradients on is served too: the forward and backward are a once-differentiable autograd.Function over
    ops.customnet_train_forward / ops.customnet_backward (include/hironaka_hip_customgrad.h states the rule: every row runs
    ONE tower both ways, a tower's gradients sum over its own rows, a tower without rows gets zeros) where the module is
    servable apart from "gradients are on", the input is float32 on the device, requires no gradient and has at most
    HK_PVGRAD_MAX_BATCH rows, and no parameter is used twice; parameters that require no gradient get None.  Anything else
    is `plain_forward`, with `fused_last_reason` saying why.  deepcopy and pickle carry the flag and not the plan."""

    def __init__(self, output_size: int, net_arch: List[int], spec: Tuple[int, int], block_cls=DenseResidueBlock,
                 role: Optional[str] = None, extra_dim: Optional[int] = None, seed: int = 0):
        super().__init__()
        m, d = (int(v) for v in spec)
        if extra_dim is None:
            if role is None:
                raise ValueError("CustomNet needs extra_dim, or role to take it from (host: 0, agent: dimension).")
            extra_dim = input_dim_of((m, d), role) - m * d
        if m < 1 or d < 1 or extra_dim < 0 or not len(net_arch):
            raise ValueError(f"CustomNet needs at least one point, one coordinate and one block. Got spec {spec}, "
                             f"extra_dim {extra_dim}, net_arch {net_arch}.")
        self.output_size, self.net_arch, self.spec = int(output_size), [int(n) for n in net_arch], (m, d)
        self.extra_dim, self.input_dim = int(extra_dim), m * d + int(extra_dim)
        generator = torch.Generator().manual_seed(int(seed) % (1 << 63))
        self._block_names = []
        for t in range(m):
            k = (t + 1) * d + self.extra_dim
            for n in self.net_arch:
                name = f"{block_cls.__name__}_{len(self._block_names)}"
                self.add_module(name, block_cls(k, n, generator))
                self._block_names.append(name)
                k = n
        self.Dense_0 = _dense(k + self.extra_dim, self.output_size, generator)
        self.Dense_1 = _dense(k + self.extra_dim, 1, generator)

    @property
    def towers(self) -> List[List[nn.Module]]:
        blocks, L = self.blocks, len(self.net_arch)
        return [blocks[t * L: (t + 1) * L] for t in range(self.spec[0])]

    # ---- torch's path: the reference's formula ------------------------------------------------------------------
    def plain_forward(self, x):
        m, d = self.spec
        x = x.flatten(1)
        count = (x[:, : m * d: d] >= 0).sum(-1)
        # (not F.one_hot: the count m is out of its range; that row's mask is all zero)
        available = (count.unsqueeze(-1) == torch.arange(m, device=x.device)).to(x.dtype)
        extra = x[:, m * d:]
        outs = []
        for t, tower in enumerate(self.towers):
            out = torch.cat([x[:, : (t + 1) * d], extra], dim=-1)
            for block in tower:
                out = block(out)
            outs.append(out)
        out = (torch.stack(outs, dim=-1) * available.unsqueeze(1)).sum(-1)
        features = torch.cat([out, extra], dim=-1)
        return self.Dense_0(features), torch.tanh(self.Dense_1(features))

    # ---- the kernels' path --------------------------------------------------------------------------------------
    def _check_key(self):
        """what the last check of the module and the cached plan were made from: per tensor the children hold NOW its
        address and shape (a tensor of another dtype or device lies elsewhere), per child its eps -- ONE flat walk per
        call over the m x L blocks, which is all a call pays where nothing changed (in-place updates change nothing)"""
        key = []
        mods = self._modules
        for name in self._block_names:
            for child in mods[name]._modules.values():
                if child is not None:
                    key.append(getattr(child, "eps", None))
                    for t in child._parameters.values():
                        key.append(None if t is None else (t.data_ptr(), t.shape))
        for child in (mods["Dense_0"], mods["Dense_1"]):
            for t in child._parameters.values():
                key.append(None if t is None else (t.data_ptr(), t.shape))
        return tuple(key)

    def _checked(self):
        """(key, why the module as it is now is not served apart from fused_enabled and the gradients; None: it is)"""
        key = self._check_key()
        last = self.__dict__.get("_fused_check")
        if last is None or last[0] != key:
            (m, d), e, L = self.spec, self.extra_dim, len(self.net_arch)
            if not 1 <= L <= A.HK_PVNET_MAX_BLOCKS:
                reason = f"not 1 to {A.HK_PVNET_MAX_BLOCKS} blocks per tower"
            elif not 1 <= m <= A.HK_CUSTOMNET_MAX_POINTS or d < 2:
                reason = f"not 1 to {A.HK_CUSTOMNET_MAX_POINTS} points of at least 2 coordinates"
            else:
                reason = self._blocks_reason(self.blocks, [m * d + e, self.net_arch[-1] + e])
            last = self.__dict__["_fused_check"] = (key, reason)
        return last

    def _reason(self) -> Optional[str]:
        if not self.fused_enabled:
            return "fused_enabled is False"
        reason = self._checked()[1]
        if reason is None and not self.fused_tower_training and self._records_graph():
            return "gradients are on"
        return reason

    def _cached_plan(self, key=None):
        """the tower table in device memory and the workspace, rebuilt under DenseResNet._cached_plan's conditions
        (key: what _checked() just returned, to spare the second walk)"""
        from . import ops
        key = self._checked()[0] if key is None else key
        plan = self.__dict__.get("_fused_plan")
        if plan is None or plan.key != key:
            heads = (self.Dense_0.weight, self.Dense_0.bias), (self.Dense_1.weight, self.Dense_1.bias)
            plan = ops.CustomnetPlan([[ops.PvnetBlock(*r) for r in self._block_records(tower)] for tower in self.towers],
                                     *heads, spec=self.spec, extra_dim=self.extra_dim)
            plan.key = key
            self.__dict__["_fused_plan"] = plan
        return plan

    def forward(self, x, params: Any = None, train: bool = True):
        key = None
        if not self.fused_enabled:
            reason = "fused_enabled is False"
        else:
            key, reason = self._checked()
            if reason is None and not self.fused_tower_training and self._records_graph():
                reason = "gradients are on"
        if reason is None:
            reason = self._input_reason(x, self.Dense_0.weight.device)
        grads = reason is None and self._records_graph()  # (only with fused_tower_training)
        if grads:
            params = [t for b in self.blocks for child in b.children() for t in child.parameters(recurse=False)]
            params += list(self.Dense_0.parameters()) + list(self.Dense_1.parameters())
            if x.shape[0] > A.HK_PVGRAD_MAX_BATCH:
                reason = f"more than {A.HK_PVGRAD_MAX_BATCH} rows with gradients on"
            elif len({id(p) for p in params}) < len(params):
                reason = "a parameter is used twice and gradients are on"
        self.__dict__["fused_last_reason"] = reason
        if reason is not None:
            return self.plain_forward(x)
        from . import ops
        plan = self._cached_plan(key)
        if grads:
            p, v = _CustomnetTrainFunction.apply(plan, x, *plan.params)
        else:
            p, v = ops.customnet_forward(x, plan)
        return p, v.unsqueeze(1)


class _PvnetTrainFunction(torch.autograd.Function):
    """forward: ops.pvnet_train_forward; backward: ops.pvnet_backward.  The parameters are saved so that torch's version
    check refuses a backward after one of them was changed in place; the input gets no gradient, a parameter that requires
    none gets None."""

    @staticmethod
    def forward(ctx, plan, x, *params):
        from . import ops
        policy, value, saved = ops.pvnet_train_forward(x, plan)
        ctx.hk_saved = saved
        ctx.save_for_backward(*params)
        return policy, value

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_policy, grad_value):
        ctx.saved_tensors  # the version check, before anything is launched
        from . import ops
        grads = ops.pvnet_backward(ctx.hk_saved, grad_policy, grad_value)
        return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


class _CustomnetTrainFunction(torch.autograd.Function):
    """forward: ops.customnet_train_forward; backward: ops.customnet_backward; otherwise _PvnetTrainFunction's"""

    @staticmethod
    def forward(ctx, plan, x, *params):
        from . import ops
        policy, value, saved = ops.customnet_train_forward(x, plan)
        ctx.hk_saved = saved
        ctx.save_for_backward(*params)
        return policy, value

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_policy, grad_value):
        ctx.saved_tensors  # the version check, before anything is launched
        from . import ops
        grads = ops.customnet_backward(ctx.hk_saved, grad_policy, grad_value)
        return (None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[2:]))


DenseNet = partial(DenseResNet, block_cls=DenseBlock)
DResNetMini = partial(DenseResNet, net_arch=[32] * 2)
DResNet18 = partial(DenseResNet, net_arch=[256] * 18)

NET_TYPES = {"dense_resnet": DenseResNet, "dense": DenseNet}


def build_net(net_type: str, role: str, output_size: int, net_arch: List[int], spec: Tuple[int, int], seed: int = 0,
              custom_net: bool = False):
    """the network JAXTrainer builds for `net_type` (jax_trainer.py:126-129, 216-218): dense_resnet -> DenseResNet,
    dense -> DenseNet; with `custom_net=True`, custom -> CustomNet and custom_dense -> CustomNet of DenseBlock.  Without
    the flag custom / custom_dense raise, as they did before CustomNet was built: turning the default is a later one-line
    change, together with the two tests that pin the refusal (tests/test_net.py, tests/test_gpu_pvnet.py)."""
    if net_type in ("custom", "custom_dense"):
        if custom_net:
            return CustomNet(output_size, net_arch, spec, block_cls=DenseResidueBlock if net_type == "custom" else DenseBlock,
                             role=role, seed=seed)
        raise ValueError(f"net_type {net_type!r} is CustomNet (one sub-network per point count, chosen per row), which is "
                         "not built unless custom_net=True is given: give HipTrainer host_net / agent_net, or use net_type "
                         "dense / dense_resnet.")
    if net_type not in NET_TYPES:
        raise ValueError(f"net_type must be one of {sorted(NET_TYPES)}. Got {net_type!r}.")
    return NET_TYPES[net_type](output_size, net_arch, spec=spec, role=role, seed=seed)
