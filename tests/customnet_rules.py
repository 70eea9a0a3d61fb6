"""The rule of hk_customnet_forward (include/hironaka_hip_customnet.h) in numpy, on top of pvnet_rules / mlp_rules: a row's
point count c picks ONE tower, whose trunk is pvnet_rules.trunk on the first c + 1 points ++ extra; a row of c == m gets
no tower (h = +0); the heads are the rule's Dense over h ++ extra.  forward64 is the reference's own formula
(hironaka/jax/net.py:84-103) in float64: all towers, the one-hot, the product, the sum.  test_customnet_rules.py pins the
choice of tower by hand and the rule to the reference's formula; test_gpu_customnet.py holds the kernels to the rule bit
for bit."""
import collections
import types

import numpy as np

import mlp_rules as M
import pvnet_rules as R
from mlp_rules import same_bits, units  # noqa: F401  (what every user of the rule wants)

F32 = np.float32
# towers: m lists of pvnet_rules.Block, tower t for the rows with t points; policy / value: (weight, bias or None)
Net = collections.namedtuple("Net", "towers policy value")


def counts(x, m, d):
    """c per row: the points whose coordinate 0 is >= 0 (a NaN does not count)"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(x)[:, : m * d: d] >= 0).sum(axis=1)


def n_last(net):
    return net.towers[0][-1].dense1.weight.shape[0]


def forward(x, net, m, d, e):
    """(policy [B, A], the value head BEFORE its tanh [B]) of x [B, m d + e]: what the kernels store with
    HK_CUSTOMNET_RAW_VALUE"""
    x = np.asarray(x, F32)
    assert x.shape[1] == m * d + e and len(net.towers) == m
    c = counts(x, m, d)
    extra = x[:, m * d:]
    h = np.zeros((len(x), n_last(net)), F32)
    for t in range(m):
        rows = np.nonzero(c == t)[0]
        if len(rows):
            h[rows] = R.trunk(np.concatenate([x[rows, : (t + 1) * d], extra[rows]], axis=1), net.towers[t])
    z = np.concatenate([h, extra], axis=1)
    return M.linear(z, np.asarray(net.policy[0], F32), net.policy[1]), M.linear(z, np.asarray(net.value[0], F32), net.value[1])[:, 0]


def forward64(x, net, m, d, e):
    """the reference's formula in float64: every tower on every row, times the one-hot of the count, summed:
    (policy, tanh value)"""
    x = np.asarray(x, np.float64)
    n = n_last(net)
    available = (counts(x, m, d)[:, None] == np.arange(m)[None, :]).astype(np.float64)  # one_hot(c, m): all zero at c == m
    extra = x[:, m * d:]
    outs = []
    for t in range(m):
        u = np.concatenate([x[:, : (t + 1) * d], extra], axis=1)
        # (pvnet_rules.forward64 with the identity as its policy head: h itself, exactly)
        outs.append(R.forward64(u, R.Net(net.towers[t], (np.eye(n), None), (np.zeros((1, n)), None)))[0])
    out = (np.stack(outs, axis=-1) * available[:, None, :]).sum(axis=-1)
    z = np.concatenate([out, extra], axis=1)
    f = lambda a: None if a is None else np.asarray(a, np.float64)  # noqa: E731
    lin = lambda head: z @ f(head[0]).T + (0 if head[1] is None else f(head[1]))  # noqa: E731
    return lin(net.policy), np.tanh(lin(net.value)[:, 0])


def random_net(rng, m, d, e, arch, actions, kind="residue", bias=True, affine=True, value_gain=1.0):
    """m towers of the block widths `arch` (pvnet_rules.random_net's blocks) and heads over n_last + e inputs"""
    towers = [R.random_net(rng, (t + 1) * d + e, arch, 1, kind, bias, affine).blocks for t in range(m)]
    k = arch[-1] + e
    head = lambda n, gain: tuple(R.random_dense(rng, k, n, bias, gain=gain, norm=False)[:2])  # noqa: E731
    return Net(towers, head(actions, 1.0), head(1, value_gain))


def module_net(module, to_numpy):
    """the Net of a hironaka_amd.net.CustomNet; to_numpy turns a tensor (or None) into an array"""
    nets = [R.module_net(types.SimpleNamespace(blocks=tower, Dense_0=module.Dense_0, Dense_1=module.Dense_1), to_numpy)
            for tower in module.towers]
    return Net([n.blocks for n in nets], nets[0].policy, nets[0].value)


def rows_with_counts(rng, cs, m, d, e, holes=False):
    """one row per entry of `cs` with that many points (coordinates in [0, 1], high to low by coordinate 0, -1 rows behind
    them, as the feature function leaves them) and e extra features in [-1, 1]; holes: the points lie at random places
    among the -1 rows instead"""
    x = np.full((len(cs), m * d + e), -1, F32)
    for b, c in enumerate(cs):
        pts = rng.uniform(0, 1, (c, d)).astype(F32)
        pts = pts[np.argsort(-pts[:, 0], kind="stable")]
        where = np.sort(rng.choice(m, c, replace=False)) if holes else np.arange(c)
        x[b, : m * d].reshape(m, d)[where] = pts
    x[:, m * d:] = rng.uniform(-1, 1, (len(cs), e)).astype(F32)
    return x
