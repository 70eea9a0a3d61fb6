"""The rule of hk_pvnet_forward (include/hironaka_hip_pvnet.h) in numpy, built on mlp_rules.fma32 / linear: float32, every
operation rounded once, the Dense as ONE fma chain per output in ascending k, the group norm's two sums balanced and
pairwise.  test_pvnet_rules.py pins the group norm by hand and the rule to torch within torch's own distance of a float64
evaluation; test_gpu_pvnet.py holds the kernel to the rule bit for bit."""
import collections

import numpy as np

import mlp_rules as M
from mlp_rules import same_bits, units  # noqa: F401  (what every user of the rule wants)

F32 = np.float32
GROUPS = 32
EPS = 1e-6
# the fields of ops.PvnetDense / ops.PvnetBlock, as numpy arrays
Dense = collections.namedtuple("Dense", "weight bias gn_scale gn_bias", defaults=(None, None, None))
Block = collections.namedtuple("Block", "kind dense1 dense2 proj eps", defaults=(None, None, EPS))
Net = collections.namedtuple("Net", "blocks policy value")  # policy / value: (weight, bias or None)


def group_sum(v, g):
    """[B, n] -> [B, n / g]: the balanced pairwise sum of every g adjacent columns (g a power of two)"""
    v = np.asarray(v, F32).reshape(v.shape[0], -1, g)
    with np.errstate(all="ignore"):
        while v.shape[-1] > 1:
            v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def group_norm(z, scale, bias, eps=EPS):
    z = np.asarray(z, F32)
    n = z.shape[1]
    assert n % GROUPS == 0 and n // GROUPS in (1, 2, 4, 8)
    g = n // GROUPS
    with np.errstate(all="ignore"):
        mean = group_sum(z, g) / F32(g)
        d = z - np.repeat(mean, g, axis=1)
        var = group_sum(d * d, g) / F32(g)
        inv = np.repeat(F32(1) / np.sqrt(var + F32(eps)), g, axis=1)
        alpha = np.asarray(scale, F32) * inv if scale is not None else inv
        beta = np.asarray(bias, F32) if bias is not None else np.zeros(n, F32)
        return M.fma32(d, alpha, beta)


def dense(h, d, norm, eps):
    z = M.linear(h, np.asarray(d.weight, F32), d.bias)
    return group_norm(z, d.gn_scale, d.gn_bias, eps) if norm else z


def trunk(x, blocks):
    h = np.asarray(x, F32)
    for b in blocks:
        if b.kind == "dense":
            h = M.relu(dense(h, b.dense1, False, b.eps))
            continue
        y = dense(M.relu(dense(h, b.dense1, True, b.eps)), b.dense2, True, b.eps)
        n, k = b.dense1.weight.shape
        o = h if k == n else dense(h, b.proj, True, b.eps)
        with np.errstate(all="ignore"):
            h = M.relu(o + y)
    return h


def forward(x, net):
    """(policy [B, A], the value head BEFORE its tanh [B]) of x [B, k0]: what the kernel stores with HK_PVNET_RAW_VALUE"""
    h = trunk(x, net.blocks)
    return M.linear(h, np.asarray(net.policy[0], F32), net.policy[1]), M.linear(h, np.asarray(net.value[0], F32), net.value[1])[:, 0]


def forward64(x, net):
    """the same net in float64, plain sums: (policy, tanh value)"""
    f = lambda a: None if a is None else np.asarray(a, np.float64)  # noqa: E731

    def lin(h, d):
        z = h @ f(d[0]).T
        return z if d[1] is None else z + f(d[1])

    def gn(z, d, eps):
        zz = z.reshape(z.shape[0], GROUPS, -1)
        y = ((zz - zz.mean(-1, keepdims=True)) / np.sqrt(zz.var(-1, keepdims=True) + float(F32(eps)))).reshape(z.shape)
        if d.gn_scale is not None:
            y = y * f(d.gn_scale)
        return y if d.gn_bias is None else y + f(d.gn_bias)

    h = np.asarray(x, np.float64)
    for b in net.blocks:
        if b.kind == "dense":
            h = np.maximum(lin(h, b.dense1), 0)
            continue
        y = gn(lin(np.maximum(gn(lin(h, b.dense1), b.dense1, b.eps), 0), b.dense2), b.dense2, b.eps)
        n, k = b.dense1.weight.shape
        h = np.maximum((h if k == n else gn(lin(h, b.proj), b.proj, b.eps)) + y, 0)
    return lin(h, net.policy), np.tanh(lin(h, net.value)[:, 0])


def random_dense(rng, k, n, bias=True, affine=True, gain=1.0, norm=True):
    bound = gain / np.sqrt(k)
    vec = lambda lo, hi: rng.uniform(lo, hi, n).astype(F32)  # noqa: E731
    return Dense(rng.uniform(-bound, bound, (n, k)).astype(F32), vec(-bound, bound) if bias else None,
                 vec(0.5, 1.5) if norm and affine else None, vec(-0.5, 0.5) if norm and affine else None)


def random_net(rng, k0, arch, actions, kind="residue", bias=True, affine=True, value_gain=1.0):
    """a net of the given input width and block widths: `kind` for every block, or a sequence of kinds; dense blocks
    get weights of the size that keeps a ReLU stack's activations (uniform in +-sqrt(6 / k))"""
    kinds = [kind] * len(arch) if isinstance(kind, str) else list(kind)
    blocks, k = [], k0
    for n, kd in zip(arch, kinds):
        if kd == "dense":
            blocks.append(Block("dense", random_dense(rng, k, n, bias, gain=np.sqrt(6.0), norm=False)))
        else:
            blocks.append(Block("residue", random_dense(rng, k, n, bias, affine), random_dense(rng, n, n, bias, affine),
                                random_dense(rng, k, n, bias, affine) if k != n else None))
        k = n
    head = lambda n, gain: tuple(random_dense(rng, k, n, bias, gain=gain, norm=False)[:2])  # noqa: E731
    return Net(blocks, head(actions, 1.0), head(1, value_gain))


def module_net(module, to_numpy):
    """the Net of a hironaka_amd.net.DenseResNet; to_numpy turns a tensor (or None) into an array"""
    def dn(lin, gn=None):
        return Dense(to_numpy(lin.weight), to_numpy(lin.bias), *((to_numpy(gn.weight), to_numpy(gn.bias)) if gn is not None
                                                                 else (None, None)))
    blocks = []
    for b in module.blocks:
        if type(b).__name__ == "DenseBlock":
            blocks.append(Block("dense", dn(b.Dense_0)))
        else:
            blocks.append(Block("residue", dn(b.Dense_0, b.GroupNorm_0), dn(b.Dense_1, b.GroupNorm_1),
                                dn(b.res_proj, b.norm_proj) if b.res_proj is not None else None, b.GroupNorm_0.eps))
    return Net(blocks, tuple(dn(module.Dense_0)[:2]), tuple(dn(module.Dense_1)[:2]))
