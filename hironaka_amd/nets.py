"""The Q-networks of the DQN trainers (the reference's ``hironaka/trainer/nets.py``): ``create_mlp`` and the two feature
extractors under the reference's names, with the eval-mode forward of the stack in ONE launch.

``create_mlp`` returns a ``FusedSequential``: an ``nn.Sequential`` with exactly the children the reference's function
produces (``state_dict`` keys, ``deepcopy``, ``.to()``, ``parameters()``, checkpoints: all ``nn.Sequential``'s), whose
``forward`` hands the whole stack to ``ops.mlp_forward`` (``hk_mlp_forward``, include/hironaka_hip_mlp.h) where that
serves it and runs ``nn.Sequential.forward`` unchanged where it does not.  Training-mode forward and backward are
torch's unless ``fused_training`` is set: then they are ``ops.mlp_train_forward`` / ``ops.mlp_backward``
(include/hironaka_hip_mlp_train.h), one launch per layer each way."""
import abc
from typing import Any, Dict, List, NamedTuple, Optional, Tuple, Type, Union

import torch
from torch import nn

from . import _abi as A

TensorDict = Dict[Union[str, int], torch.Tensor]


def expand_net_list(net_arch: List[Any]) -> List[Any]:
    """`net_arch` flattened: every {"repeat": n, "net_arch": [...]} entry is replaced by n copies of its own flattened
    list, to any depth; every other entry stays where it is"""
    flat: List[Any] = []
    for entry in net_arch:
        if not isinstance(entry, dict):
            flat.append(entry)
            continue
        missing = {"repeat", "net_arch"} - set(entry)
        assert not missing, f"a repeated part of net_arch needs 'repeat' and 'net_arch'; {sorted(missing)} missing in {entry}"
        assert isinstance(entry["net_arch"], list), f"a repeated part's 'net_arch' is a list, not {type(entry['net_arch'])}"
        flat.extend(expand_net_list(entry["net_arch"]) * entry["repeat"])
    return flat


class ResidualBlock(nn.Module):
    """lin1 -> bn1 -> relu -> lin2 -> bn2, plus the input (through `down_sample` where the widths differ).  Plain torch:
    a stack with one of these takes torch's path."""

    def __init__(self, in_channels: int, out_channels: int, down_sample: Optional[nn.Module] = None):
        super().__init__()
        self.lin1 = nn.Linear(in_channels, out_channels)
        self.bn1 = nn.BatchNorm1d(out_channels)
        self.relu = nn.ReLU(inplace=True)
        self.lin2 = nn.Linear(out_channels, out_channels)
        self.bn2 = nn.BatchNorm1d(out_channels)
        self.down_sample = down_sample

    def forward(self, x):
        out = self.bn2(self.lin2(self.relu(self.bn1(self.lin1(x)))))
        out += self.down_sample(x) if self.down_sample else x
        return out


def make_residual(in_channels: int, out_channels: int) -> ResidualBlock:
    if in_channels == out_channels:
        return ResidualBlock(in_channels, out_channels)
    return ResidualBlock(in_channels, out_channels,
                         nn.Sequential(nn.Linear(in_channels, out_channels), nn.BatchNorm1d(out_channels)))


class BaseFeaturesExtractor(nn.Module, abc.ABC):
    """A head of `create_mlp`: `forward(observations)` gives [batch, feature_dim] rows."""

    def __init__(self, input_dim: int):
        super().__init__()
        self.input_dim = input_dim

    @property
    def feature_dim(self) -> int:
        return self.input_dim

    @abc.abstractmethod
    def forward(self, observations) -> torch.Tensor:
        pass


class AgentFeatureExtractor(BaseFeaturesExtractor):
    """{"points": [B, ...], "coords": [B, ...]} -> the two flattened, side by side"""

    def __init__(self, input_dim: int):
        super().__init__(input_dim)
        self.extractors = {"points": nn.Flatten(), "coords": nn.Flatten()}

    def forward(self, observations: TensorDict) -> torch.Tensor:
        return torch.cat([extractor(observations[key]) for key, extractor in self.extractors.items()], dim=1)


class HostFeatureExtractor(BaseFeaturesExtractor):
    def __init__(self, input_dim: int):
        super().__init__(input_dim)
        self.flatten = nn.Flatten()

    def forward(self, observations: torch.Tensor) -> torch.Tensor:
        return self.flatten(observations)


class MlpSpec(NamedTuple):
    """how a stack reads as hk_mlp_forward's input: the head (an extractor, an nn.Flatten or None), the batch norm and
    the ReLU on the input, and the (Linear, BatchNorm1d or None, whether a ReLU follows) blocks"""
    head: Optional[nn.Module]
    input_bn: Optional[nn.BatchNorm1d]
    input_relu: bool
    blocks: List[Tuple[nn.Linear, Optional[nn.BatchNorm1d], bool]]


def _bn_ok(bn: nn.BatchNorm1d, width: int) -> bool:
    return bn.track_running_stats and bn.running_mean is not None and bn.num_features == width


def mlp_spec(sequential: nn.Sequential) -> Union[MlpSpec, str]:
    """the MlpSpec of a stack in create_mlp's order -- [head] [BatchNorm1d] [ReLU] (Linear [BatchNorm1d] [ReLU])+ --
    or, as a string, why it is not one"""
    mods = list(sequential._modules.values())  # every slot: children() would drop a module that is used twice
    head = None
    if mods and isinstance(mods[0], (HostFeatureExtractor, AgentFeatureExtractor, nn.Flatten)):
        head = mods.pop(0)
        if isinstance(head, nn.Flatten) and (head.start_dim, head.end_dim) != (1, -1):
            return "the head flattens other dimensions than 1..-1"
    first = next((m for m in mods if isinstance(m, nn.Linear)), None)
    if first is None:
        return "the stack has no Linear"
    input_bn, input_relu, at = None, False, 0
    if isinstance(mods[at], nn.BatchNorm1d):
        input_bn, at = mods[at], at + 1
        if not _bn_ok(input_bn, first.in_features):
            return "a BatchNorm1d without running statistics, or of another width than its input"
    if isinstance(mods[at], nn.ReLU):
        input_relu, at = True, at + 1
    blocks = []
    width = first.in_features
    while at < len(mods):
        lin = mods[at]
        if not isinstance(lin, nn.Linear):
            return f"a {type(lin).__name__} where create_mlp puts a Linear"
        if lin.in_features != width:
            return "consecutive widths do not match"
        width, at, bn, relu = lin.out_features, at + 1, None, False
        if at < len(mods) and isinstance(mods[at], nn.BatchNorm1d):
            bn, at = mods[at], at + 1
            if not _bn_ok(bn, width):
                return "a BatchNorm1d without running statistics, or of another width than its input"
        if at < len(mods) and isinstance(mods[at], nn.ReLU):
            relu, at = True, at + 1
        blocks.append((lin, bn, relu))
    if len(blocks) > A.HK_MLP_MAX_LAYERS:
        return f"more than {A.HK_MLP_MAX_LAYERS} Linear"
    if max(max(lin.in_features, lin.out_features) for lin, _, _ in blocks) > A.HK_MLP_MAX_WIDTH:
        return f"a layer wider than {A.HK_MLP_MAX_WIDTH}"
    if min(min(lin.in_features, lin.out_features) for lin, _, _ in blocks) < 1:
        return "a layer of width 0"
    return MlpSpec(head, input_bn, input_relu, blocks)


class FusedSequential(nn.Sequential):
    """An nn.Sequential whose eval-mode, gradient-free float32 forward on a HIP device is one hk_mlp_forward launch
    and, with `fused_training`, whose training-mode forward and backward are one launch per layer each way.

    `forward` takes the kernel's path when the stack is create_mlp's shape (mlp_spec), it is in eval mode or has no
    BatchNorm1d, gradients are off or no parameter requires one, and parameters and input are float32 on one HIP
    device; otherwise it IS nn.Sequential.forward.  `fused_reason` says why the MODULE is not served (None: it is);
    `fused_last_reason` says why the last CALL was not (None: it was), which adds what only a call shows: parameters
    that are not on a HIP device, an input of another dtype, device or shape.  The two paths differ in the
    last bits (one fma chain per output against torch's GEMM), so there is no automatic crossover between them:
    `fused_enabled = False` pins torch's.  With `fused_training = True` (off by default) a stack in training mode, or
    one without a BatchNorm1d with gradients on, is served by ops.mlp_train_forward / ops.mlp_backward through an
    autograd.Function: up to HK_MLP_TRAIN_MAX_BATCH rows, at least 2 with a batch norm, every batch norm with a float
    momentum and none on the input, an input that requires no gradient.  A stack with a batch norm in eval mode keeps
    the rule above (running statistics have no backward here).  Nothing here synchronises."""

    fused_enabled = True
    # opt-in: the training-mode forward (batch statistics, running statistics updated) and the backward through
    # ops.mlp_train_forward / ops.mlp_backward.  False: exactly the paths and reasons described above.
    fused_training = False
    fused_last_reason = None

    def _tensors(self):
        return [t for m in self.modules() for t in list(m._parameters.values()) + list(m._buffers.values())
                if t is not None and t.is_floating_point()]

    @property
    def fused_reason(self) -> Optional[str]:
        return self._reason_and_spec()[0]

    def _reason_and_spec(self):
        return self._resolve()[:2]

    def _resolve(self):
        """(why the module is not served or None, its MlpSpec, "eval" or "train": which kernels serve it)"""
        if not self.fused_enabled:
            return "fused_enabled is False", None, None
        spec = mlp_spec(self)
        if isinstance(spec, str):
            return spec, None, None
        reason, mode = self._state_reason(spec)
        return reason, spec, mode

    def _bn_and_grads(self):
        """whether the stack has a BatchNorm1d, and whether a call now would record a graph over its parameters"""
        return (any(isinstance(m, nn.BatchNorm1d) for m in self.children()),
                torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()))

    def _state_reason(self, spec: MlpSpec):
        tensors = self._tensors()
        if any(t.dtype != torch.float32 for t in tensors):
            return "parameters are not float32", None
        if len({t.device for t in tensors}) > 1:
            return "parameters live on more than one device", None
        has_bn, grads = self._bn_and_grads()
        if not self.fused_training:
            if self.training and has_bn:
                return "a BatchNorm1d in training mode", None
            return ("gradients are on", None) if grads else (None, "eval")
        if has_bn and not self.training:  # running statistics: hk_mlp_forward's, which has no backward
            return ("gradients are on", None) if grads else (None, "eval")
        if not has_bn and not grads:
            return None, "eval"
        if spec.input_bn is not None:
            return "a BatchNorm1d on the input in training mode", None
        if any(bn is not None and not isinstance(bn.momentum, float) for _, bn, _ in spec.blocks):
            return "a BatchNorm1d with momentum=None in training mode", None
        params = [p for lin, bn, _ in spec.blocks for p in (lin.weight, lin.bias) + ((bn.weight, bn.bias) if bn else ())
                  if p is not None]
        if grads and len({id(p) for p in params}) < len(params):
            return "a parameter is used twice and gradients are on", None
        return None, "train"

    def _cached_plan(self, slot: str, spec: MlpSpec, records, build):
        """the layer table kept in `slot`, rebuilt (build()) when the stack no longer is what the table was built from:
        the tensors of `records` that the modules hold NOW lie elsewhere (one data_ptr() per tensor per call: a parameter
        or buffer that was assigned anew, a state loaded with assign=True, .to()), or a batch norm, a ReLU or another
        scalar of `records` came, went or changed.  In-place updates -- optimizer.step, Polyak, load_state_dict --
        change no address and need nothing."""
        key = (spec.input_relu,) + tuple(lin.weight.shape for lin, _, _ in spec.blocks) + tuple(
            x.data_ptr() if isinstance(x, torch.Tensor) else x for r in records for x in r)
        plan = self.__dict__.get(slot)
        if plan is None or plan.key != key:
            plan = build()
            plan.key = key
            self.__dict__[slot] = plan
        return plan

    def _plan(self, spec: MlpSpec):
        """hk_mlp_forward's layer table"""
        from . import ops
        records = [(lin.weight, lin.bias) + (_bn_fields(bn) if bn is not None else (None,) * 4)
                   + (bn.eps if bn is not None else 0.0, relu) for lin, bn, relu in spec.blocks]
        in_bn = spec.input_bn
        in_record = None if in_bn is None else (None, None) + _bn_fields(in_bn) + (in_bn.eps,)
        return self._cached_plan(
            "_fused_plan", spec, records + [in_record or ()],
            lambda: ops.MlpPlan([ops.MlpLayer(*r) for r in records], spec.input_relu,
                                None if in_record is None else ops.MlpLayer(*in_record)))

    def _train_plan(self, spec: MlpSpec):
        """the training kernels' layer table: the batch norms' momenta and counters count too"""
        from . import ops
        records = [(lin.weight, lin.bias) + (_bn_fields(bn) + (bn.eps, relu, bn.momentum, bn.num_batches_tracked)
                                             if bn is not None else (None,) * 4 + (0.0, relu, 0.0, None))
                   for lin, bn, relu in spec.blocks]
        return self._cached_plan("_fused_train_plan", spec, records,
                                 lambda: ops.MlpTrainPlan([ops.MlpTrainLayer(*r) for r in records], spec.input_relu))

    def _forward_train(self, spec: MlpSpec, x0, x1):
        """the training kernels' forward, or None with fused_last_reason set where this CALL is torch's"""
        from . import ops
        batch = x0.shape[0]
        has_bn, grads = self._bn_and_grads()  # (no batch norm on the input here: _state_reason)
        reason = None
        if batch > A.HK_MLP_TRAIN_MAX_BATCH:
            reason = f"more than {A.HK_MLP_TRAIN_MAX_BATCH} rows in training mode"
        elif batch == 0:
            reason = "an empty batch in training mode"
        elif batch == 1 and has_bn:
            reason = "a batch of 1 with a BatchNorm1d in training mode"
        elif torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (x0, x1)):
            reason = "the input requires a gradient"
        if reason is not None:
            self.__dict__["fused_last_reason"] = reason
            return None
        plan = self._train_plan(spec)
        if not grads:
            return ops.mlp_train_forward(x0, plan, x1=x1)[0]
        return _MlpTrainFunction.apply(plan, x0, x1, *plan.params)

    def forward(self, input):
        reason, spec, mode = self._resolve()
        self.__dict__["fused_last_reason"] = reason
        if reason is None:
            x1 = None
            if isinstance(spec.head, AgentFeatureExtractor):
                x0, x1 = (input[key] for key in spec.head.extractors)
            else:
                x0 = input
            dev = spec.blocks[0][0].weight.device
            # (a head flattens whatever follows the batch dimension; without one the rows come as they are)
            if dev.type == "cuda" and all(
                    isinstance(x, torch.Tensor) and x.dtype == torch.float32 and x.device == dev
                    and (x.dim() >= 2 if spec.head is not None else x.dim() == 2)
                    for x in ((x0,) if x1 is None else (x0, x1))):
                from . import ops
                if mode == "eval":
                    return ops.mlp_forward(x0, self._plan(spec), x1=x1)
                out = self._forward_train(spec, x0, x1)
                return out if out is not None else super().forward(input)
            self.__dict__["fused_last_reason"] = (
                f"parameters live on {dev}, not on a HIP device" if dev.type != "cuda" else
                f"the input is not float32 on {dev} with a batch dimension" + ("" if spec.head is not None else " and one more"))
        return super().forward(input)

    def __deepcopy__(self, memo):
        # the copy builds its own table (this one's points at this module's tensors)
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        import copy
        for k, v in self.__dict__.items():
            if k not in ("_fused_plan", "_fused_train_plan"):
                new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_fused_plan", None)
        state.pop("_fused_train_plan", None)
        return state


class _MlpTrainFunction(torch.autograd.Function):
    """forward: ops.mlp_train_forward; backward: ops.mlp_backward.  The parameters are saved so that torch's version
    check refuses a backward after one of them was changed in place; the input gets no gradient."""

    @staticmethod
    def forward(ctx, plan, x0, x1, *params):
        from . import ops
        out, saved = ops.mlp_train_forward(x0, plan, x1=x1)
        ctx.hk_saved = saved
        ctx.save_for_backward(*params)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        ctx.saved_tensors  # the version check, before anything is launched
        from . import ops
        return (None, None, None) + tuple(ops.mlp_backward(ctx.hk_saved, grad_out))


def _bn_fields(bn: nn.BatchNorm1d):
    return bn.running_mean, bn.running_var, bn.weight, bn.bias


def fuse(sequential: nn.Sequential, training: bool = False) -> FusedSequential:
    """a FusedSequential over the SAME modules, under the same names (nothing is copied); training: its
    fused_training"""
    fused = FusedSequential()
    if training:
        fused.fused_training = True
    for name, module in sequential._modules.items():  # every slot: named_children() drops a module's second use
        fused.add_module(name, module)
    fused.train(sequential.training)
    return fused


def create_mlp(head: nn.Module, net_arch: List[Any], input_dim: int, output_dim: int,
               activation_fn: Type[nn.Module] = nn.ReLU, fused_training: bool = False) -> nn.Module:
    """`head`, then the layers `net_arch` describes, then a Linear to `output_dim`, as a FusedSequential.
    `head` gives [batch, input_dim] rows.  In `net_arch` (its own input and output widths are not listed)
        an int is a Linear of that width followed by an activation,
        'b' puts a BatchNorm1d between the layer before it and that layer's activation (a second 'b' in a row is
            dropped; at the very front it normalises the head's output),
        'r<width>' is a residual block of that width followed by an activation,
        {"repeat": n, "net_arch": [...]} repeats a part, recursively.
    The activation after the last item is dropped.  fused_training: the FusedSequential's attribute of that name."""
    nets = [head, activation_fn()]
    last_dim, last_type = input_dim, None
    for item in expand_net_list(net_arch):
        if isinstance(item, int):
            nets += [nn.Linear(last_dim, item), activation_fn()]
            last_dim, last_type = item, "l"
        elif isinstance(item, str):
            assert item[:1] in ("b", "r"), f"a string in net_arch is 'b' or 'r<width>', not {item!r}"
            if item[0] == "b":
                if last_type == "b":
                    continue
                nets.pop()  # the activation moves behind the batch norm
                nets += [nn.BatchNorm1d(last_dim), activation_fn()]
                last_type = "b"
            else:
                width = int(item[1:])
                assert width > 0, f"a residual block is written 'r<width>' with a positive width, not {item!r}"
                nets += [make_residual(last_dim, width), activation_fn()]
                last_dim, last_type = width, "r"
    nets.pop()  # no activation in front of the output layer
    nets.append(nn.Linear(last_dim, output_dim))
    net = FusedSequential(*nets)
    if fused_training:
        net.fused_training = True
    return net
