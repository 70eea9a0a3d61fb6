"""The rule of hk_mlp_forward (include/hironaka_hip_mlp.h) in numpy: float32, every operation rounded once, the Linear
as ONE fma chain per output in ascending k.  test_mlp_rules.py pins `fma32` to dqn_rules.fma_exact and the rule to
torch within a measured tolerance; test_gpu_mlp.py holds the kernel to the rule bit for bit."""
import collections

import numpy as np

from dqn_rules import same_bits  # noqa: F401  (the comparison every user of the rule wants)

F32 = np.float32
# the fields of ops.MlpLayer, as numpy arrays
Layer = collections.namedtuple("Layer", "weight bias bn_mean bn_var bn_weight bn_bias eps relu",
                               defaults=(None, None, None, None, None, 1e-5, False))


def fma32_twice(a, b, c):
    """float32(double(a) * b + c): the product is exact but the sum is rounded to double and then to float32 -- WRONG
    where the double lands on a float32 midpoint that the exact sum only lies next to (test_mlp_rules.py shows one)"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
                + np.asarray(c, F32).astype(np.float64)).astype(F32)


def fma32(a, b, c):
    """round(a * b + c) with ONE rounding to float32, elementwise with broadcasting.  The product of two float32 is
    exact in double.  The sum is rounded to double, its error comes from TwoSum; where the error is not zero and the
    double's last bit is even the double steps to its neighbour on the error's side (rounding to odd: the sticky bit
    survives in the last place), and the odd double rounds to float32 as the exact sum would (53 >= 24 + 2 bits)."""
    a, b, c = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)
        even = (s.view(np.int64) & 1) == 0 if s.ndim else (np.float64(s).view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def relu(x):
    return np.where(x < 0, F32(0), x).astype(F32)


def batch_norm(z, mean, var, weight, bias, eps):
    with np.errstate(all="ignore"):
        inv = F32(1) / np.sqrt(var.astype(F32) + F32(eps))
        alpha = weight.astype(F32) * inv if weight is not None else inv
        beta = bias.astype(F32) if bias is not None else np.zeros_like(inv)
        return fma32(z - mean.astype(F32), alpha, beta)


def linear(h, weight, bias):
    n, k = weight.shape
    acc = np.broadcast_to(bias.astype(F32) if bias is not None else np.zeros(n, F32), (h.shape[0], n))
    for i in range(k):
        acc = fma32(h[:, i:i + 1], weight[None, :, i], acc)
    return np.ascontiguousarray(acc)


def forward(x, layers, input_relu=False, input_bn=None):
    """x [B, K] float32 (the two segments already side by side) through `layers` (Layer records); input_bn: a Layer
    whose batch-norm fields alone count"""
    h = np.asarray(x, F32)
    if input_bn is not None:
        h = batch_norm(h, *input_bn[2:7])
    if input_relu:
        h = relu(h)
    for l in layers:
        h = linear(h, np.asarray(l.weight, F32), l.bias)
        if l.bn_mean is not None:
            h = batch_norm(h, *l[2:7])
        if l.relu:
            h = relu(h)
    return h


def random_layers(rng, widths, bias=True, bn=False, affine=True, last_relu=False, scale=None):
    """Layer records for widths[0] -> widths[1] -> ...: ReLU behind every layer but the last (behind it too with
    last_relu), weights of the size nn.Linear draws"""
    layers = []
    for i, (k, n) in enumerate(zip(widths[:-1], widths[1:])):
        bound = scale if scale is not None else 1.0 / np.sqrt(k)
        vec = lambda lo, hi: rng.uniform(lo, hi, n).astype(F32)  # noqa: E731
        layers.append(Layer(
            rng.uniform(-bound, bound, (n, k)).astype(F32), vec(-bound, bound) if bias else None,
            vec(-0.5, 0.5) if bn else None, vec(0.5, 2.0) if bn else None,
            vec(0.5, 1.5) if bn and affine else None, vec(-0.5, 0.5) if bn and affine else None,
            1e-5, last_relu or i + 2 < len(widths)))
    return layers


def spec_layers(spec, to_numpy):
    """(layers, input_relu, input_bn) of a hironaka_amd.nets.MlpSpec; to_numpy turns a tensor (or None) into an array"""
    def bn_fields(bn):
        return tuple(to_numpy(t) for t in (bn.running_mean, bn.running_var, bn.weight, bn.bias)) + (bn.eps,)
    layers = [Layer(to_numpy(lin.weight), to_numpy(lin.bias), *(bn_fields(bn) if bn is not None else (None,) * 4 + (0.0,)),
                    relu) for lin, bn, relu in spec.blocks]
    input_bn = None if spec.input_bn is None else Layer(None, None, *bn_fields(spec.input_bn))
    return layers, spec.input_relu, input_bn


# ---- the nets of tests/golden/mlp_nets.npz ----------------------------------------------------------------------------

MAX_POINTS, DIM = 20, 3
HEADS = {"host": (MAX_POINTS * DIM, 2 ** DIM - DIM - 1), "agent": (MAX_POINTS * DIM + DIM, DIM)}  # input_dim, output_dim
NET_ARCHS = {
    "plain": [32, 32],
    "deep": [256] * 8,
    "example": [128, "b", {"repeat": 20, "net_arch": [256, "b"]}, 128, "b"],
    "test": [16, "b", {"repeat": 2, "net_arch": [32, "b"]}, 16, "b"],
    "empty": [],
    "doubled_bn": ["b", "b", 16],
    "residual": [32, "r32", 16],
}
RESIDUAL = ("residual",)
ROWS = 96
UNIT = 2.0 ** -24


def seeded_state(shapes, seed):
    """a state_dict's arrays from numpy's PCG64 (the same on every machine and torch version), in the order of
    `shapes` = [(key, shape), ...]: Linear weights uniform in +-sqrt(6 / k), running_var in [0.5, 2], running_mean and
    every bias in [-0.5, 0.5], batch-norm weights in [0.5, 1.5], counters 0"""
    rng = np.random.default_rng(seed)
    state = {}
    for key, shape in shapes:
        shape = tuple(shape)
        if key.endswith("num_batches_tracked"):
            state[key] = np.zeros(shape, np.int64)
        elif len(shape) == 2:
            bound = np.sqrt(6.0 / shape[1])
            state[key] = rng.uniform(-bound, bound, shape).astype(F32)
        elif key.endswith("running_var"):
            state[key] = rng.uniform(0.5, 2.0, shape).astype(F32)
        elif key.endswith("weight"):
            state[key] = rng.uniform(0.5, 1.5, shape).astype(F32)
        else:
            state[key] = rng.uniform(-0.5, 0.5, shape).astype(F32)
    return state


def seeded_inputs(seed):
    """ROWS feature rows with entries in [-0.2, 1] (negative ones stand for padding values) and 0/1 coordinate rows with
    at least two ones each"""
    rng = np.random.default_rng(seed)
    points = rng.uniform(-0.2, 1.0, (ROWS, MAX_POINTS, DIM)).astype(F32)
    coords = np.zeros((ROWS, DIM), F32)
    for row in coords:
        row[rng.choice(DIM, size=rng.integers(2, DIM + 1), replace=False)] = 1
    return points, coords


def units(y, y64):
    """max |y - y64| in units of max |y64| * 2^-24"""
    y64 = np.asarray(y64, np.float64)
    return float(np.abs(np.asarray(y, np.float64) - y64).max() / (np.abs(y64).max() * UNIT))
