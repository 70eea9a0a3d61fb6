"""The rule of hk_train_mlp_forward / hk_train_mlp_backward (include/hironaka_hip_mlp_train.h) in numpy: float32, every
operation rounded once, CHAIN and ROWSUM in the header's orders.  test_mlp_train_rules.py holds the rule to torch within
the project's bound; test_gpu_mlp_train.py holds the kernels to the rule bit for bit."""
import collections

import numpy as np

import mlp_rules as R
from mlp_rules import F32, fma32, relu, same_bits  # noqa: F401

# ops.MlpTrainLayer's fields as numpy arrays; bn_mean / bn_var are the running statistics (None: no batch norm)
Layer = collections.namedtuple("Layer", "weight bias bn_mean bn_var bn_weight bn_bias eps relu momentum",
                               defaults=(None, None, None, None, None, 1e-5, False, 0.1))
ZERO = F32(0)


def _pad(acc, terms):
    """the chain runs on to the next multiple of 16 with zero terms: -0 becomes +0"""
    return acc + ZERO if terms % 16 else acc


def rowsum(v):
    """ROWSUM over axis 0 of v [B, ...]"""
    v = np.asarray(v, F32)
    p = np.zeros((16,) + v.shape[1:], F32)
    with np.errstate(all="ignore"):
        for at in range(0, v.shape[0], 16):
            rows = v[at:at + 16]
            p[:len(rows)] = p[:len(rows)] + rows
        for half in (8, 4, 2, 1):
            p = p[:half] + p[half:]
    return p[0]


def linear(h, weight, bias):
    with np.errstate(all="ignore"):
        return _pad(R.linear(h, weight, bias), weight.shape[1])


def forward(x, layers, input_relu=False):
    """x [B, K] float32 through `layers` in training mode.  Returns (out, saved, stats): saved per layer a dict with
    a_in, z, act, mean, inv (None without a batch norm), stats per layer (running_mean, running_var) after the update"""
    h = np.asarray(x, F32)
    if input_relu:
        h = relu(h)
    fb = F32(h.shape[0])
    saved, stats = [], []
    with np.errstate(all="ignore"):
        for l in layers:
            s = dict(a_in=h, z=None, mean=None, inv=None)
            h = linear(h, np.asarray(l.weight, F32), l.bias)
            if l.bn_mean is not None:
                n = h.shape[1]
                mean = rowsum(h) / fb
                e = h - mean
                var = rowsum(e * e) / fb
                inv = F32(1) / np.sqrt(var + F32(l.eps))
                gamma = l.bn_weight if l.bn_weight is not None else np.ones(n, F32)
                beta = l.bn_bias if l.bn_bias is not None else np.zeros(n, F32)
                s.update(z=h, mean=mean, inv=inv)
                h = fma32((h - mean) * inv, gamma, beta)
                m = F32(l.momentum)
                keep = F32(1) - m
                stats.append((fma32(m, mean, keep * l.bn_mean), fma32(m, var * (fb / (fb - F32(1))), keep * l.bn_var)))
            else:
                stats.append((None, None))
            if l.relu:
                h = relu(h)
            s["act"] = h
            saved.append(s)
    return h, saved, stats


def backward(layers, saved, grad_out):
    """per layer a dict with d_weight, d_bias, d_bn_weight, d_bn_bias (None where the parameter is) and dz"""
    fb = F32(grad_out.shape[0])
    grads = [None] * len(layers)
    dz_next = None
    with np.errstate(all="ignore"):
        for i in reversed(range(len(layers))):
            l, s = layers[i], saved[i]
            n, k = l.weight.shape
            if dz_next is None:
                d = np.asarray(grad_out, F32)
            else:
                wn = np.asarray(layers[i + 1].weight, F32)
                d = np.zeros((dz_next.shape[0], n), F32)
                for j in range(wn.shape[0]):
                    d = fma32(dz_next[:, j:j + 1], wn[j][None, :], d)
                d = _pad(d, wn.shape[0])
            if l.relu:
                d = np.where(s["act"] > 0, d, ZERO).astype(F32)
            g = dict(d_weight=None, d_bias=None, d_bn_weight=None, d_bn_bias=None)
            if l.bn_mean is not None:
                xhat = (s["z"] - s["mean"]) * s["inv"]
                dbeta = rowsum(d)
                dgamma = rowsum(d * xhat)
                scale = l.bn_weight * s["inv"] if l.bn_weight is not None else s["inv"]
                dz = scale * ((d - dbeta / fb) - xhat * (dgamma / fb))
                if l.bn_weight is not None:
                    g["d_bn_weight"] = dgamma
                if l.bn_bias is not None:
                    g["d_bn_bias"] = dbeta
            else:
                dz = d
            dz = np.ascontiguousarray(dz, F32)
            if l.bias is not None:
                g["d_bias"] = rowsum(dz)
            dw = np.zeros((n, k), F32)
            a = s["a_in"]
            for b in range(dz.shape[0]):
                dw = fma32(dz[b][:, None], a[b][None, :], dw)
            g["d_weight"] = _pad(dw, dz.shape[0])
            g["dz"] = dz
            grads[i] = g
            dz_next = dz
    return grads


def param_grads(layers, grads):
    """the gradients in parameter order: per layer weight, bias, bn_weight, bn_bias, those that exist"""
    return [g[name] for g in grads for name in ("d_weight", "d_bias", "d_bn_weight", "d_bn_bias") if g[name] is not None]


def random_layers(rng, widths, bias=True, bn=True, affine=True, last_relu=False, momentum=0.1):
    return [Layer(*l[:8], momentum) for l in R.random_layers(rng, widths, bias, bn, affine, last_relu)]


def spec_layers(spec, to_numpy):
    """(layers, input_relu) of a hironaka_amd.nets.MlpSpec without a batch norm on the input"""
    layers, input_relu, input_bn = R.spec_layers(spec, to_numpy)
    assert input_bn is None
    return [Layer(*l[:8], bn.momentum if bn is not None else 0.0) for l, (_, bn, _) in zip(layers, spec.blocks)], input_relu


def sparse_grad(rng, batch, n):
    """dL/dQ as hk_dqn_td emits it: one action per row, scaled by 1 / B"""
    g = np.zeros((batch, n), F32)
    g[np.arange(batch), rng.integers(0, n, batch)] = (rng.uniform(-1, 1, batch) / batch).astype(F32)
    return g


def seeded_net(name, head, seed, fused_training=False):
    """hironaka_amd.nets.create_mlp of R.NET_ARCHS[name] behind the host's or the agent's extractor, in training mode,
    with mlp_rules.seeded_state(seed) loaded"""
    import torch
    from hironaka_amd import nets
    input_dim, output_dim = R.HEADS[head]
    extractor = nets.HostFeatureExtractor if head == "host" else nets.AgentFeatureExtractor
    net = nets.create_mlp(extractor(input_dim), R.NET_ARCHS[name], input_dim, output_dim, fused_training=fused_training)
    state = R.seeded_state([(k, v.shape) for k, v in net.state_dict().items()], seed)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return net.train()


def seeded_rows(seed, rows):
    """`rows` feature rows as mlp_rules.seeded_inputs draws them (flattened points, 0/1 coordinates)"""
    rng = np.random.default_rng(seed)
    points = rng.uniform(-0.2, 1.0, (rows, R.MAX_POINTS, R.DIM)).astype(F32)
    coords = np.zeros((rows, R.DIM), F32)
    for row in coords:
        row[rng.choice(R.DIM, size=rng.integers(2, R.DIM + 1), replace=False)] = 1
    return points, coords


# ---- the cases of tests/golden/mlp_train.npz: (net, rows), behind the host's extractor ---------------------------------
CASES = {"test_256": ("test", 256), "example_256": ("example", 256), "deep_64": ("deep", 64), "plain_17": ("plain", 17)}


def case_inputs(key, seed):
    name, rows = CASES[key]
    points, _ = seeded_rows(seed, rows)
    return points, sparse_grad(np.random.default_rng(seed + 1), rows, R.HEADS["host"][1])


def torch_run(net, points, grad, dtype):
    """one training forward and backward of a copy of `net` in `dtype` on the CPU, torch's own: the named results --
    out, every parameter's gradient, every batch norm's running statistics afterwards"""
    import copy
    import torch
    net = copy.deepcopy(net).to(dtype).train()
    net.fused_enabled = False
    q = net(torch.from_numpy(points).to(dtype))
    q.backward(torch.from_numpy(grad).to(dtype))
    got = [("out", q.detach().numpy())]
    got += [(f"grad.{k}", p.grad.numpy()) for k, p in net.named_parameters()]
    got += [(k, b.numpy()) for k, b in net.named_buffers() if b.is_floating_point()]
    return got


def rule_run(net, points, grad):
    """the same results by the rule, under the same names"""
    from hironaka_amd import nets
    spec = nets.mlp_spec(net)
    layers, input_relu = spec_layers(spec, lambda t: None if t is None else t.detach().numpy().copy())
    out, saved, stats = forward(points.reshape(len(points), -1), layers, input_relu)
    grads = param_grads(layers, backward(layers, saved, grad))
    names = [k for k, _ in net.named_parameters()]
    got = [("out", out)] + [(f"grad.{k}", g) for k, g in zip(names, grads)]
    flat = [s for st in stats if st[0] is not None for s in st]
    return got + list(zip([k for k, b in net.named_buffers() if b.is_floating_point()], flat))


def case_units(results, reference):
    """E of every named result against the float64 run, in units of max |v64| * 2^-24 -- but the bias gradient of a
    Linear that feeds a batch norm, which is zero in exact arithmetic, in the units of that Linear's weight gradient"""
    ref = dict(reference)
    names = [k for k, _ in reference]
    units = []
    for k, v in results:
        scale = ref[k]
        if k.startswith("grad.") and k.endswith(".bias"):
            at = names.index(k)
            feeds_bn = at + 1 < len(names) and names[at + 1].startswith("grad.") and names[at + 1].endswith(".weight") \
                and ref[names[at + 1]].ndim == 1
            if feeds_bn:
                scale = ref[k[:-len("bias")] + "weight"]
        units.append(float(np.abs(np.asarray(v, np.float64) - ref[k]).max() / (np.abs(scale).max() * R.UNIT)))
    return units
