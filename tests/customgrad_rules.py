"""The rule of hk_customgrad_forward / hk_customgrad_backward (include/hironaka_hip_customgrad.h) in numpy, on top of
pvgrad_rules (the blocks' forward with what is saved, GNB, CHAIN, ROWSUM, a Dense's gradients) and customnet_rules (the
point count, the choice of tower): every row runs ONE tower both ways, a tower's parameter gradients sum over its own rows
in ascending row index, the heads' over all rows in the GROUPED ORDER (the rows sorted by (count, index)), a tower without
rows gets +0.  test_customgrad_rules.py pins the rule to pvgrad_rules on a group's rows alone and to torch within torch's
own distance of float64; test_gpu_customgrad.py holds the kernels to the rule bit for bit."""
import numpy as np

import customnet_rules as CR
import pvgrad_rules as G
import pvnet_rules as P
from mlp_rules import F32, same_bits, units  # noqa: F401

ZERO = F32(0)
tanh_grad = G.tanh_grad


def grouped_order(c):
    """s -> b(s): the rows sorted by (c(b), b), both ascending"""
    c = np.asarray(c)
    return np.lexsort((np.arange(len(c)), c))


def _trunk_net(blocks):
    """a pvnet_rules.Net of a tower's blocks alone (heads nobody looks at)"""
    n = blocks[-1].dense1.weight.shape[0]
    return P.Net(blocks, (np.zeros((1, n), F32), None), (np.zeros((1, n), F32), None))


def forward_saved(x, net, m, d, e):
    """(policy [B, A], the value head BEFORE its tanh [B], saved): customnet_rules.forward's results and what the backward
    needs -- c per row, the grouped order, per tower its rows G_t (ascending) and pvgrad_rules.forward_saved's list for them
    (None without rows), and z = h ++ extra per row (by the row's own index)"""
    x = np.asarray(x, F32)
    assert x.shape[1] == m * d + e and len(net.towers) == m
    c = CR.counts(x, m, d)
    extra = x[:, m * d:]
    h = np.zeros((len(x), CR.n_last(net)), F32)
    groups, towers = [], []
    for t in range(m):
        rows = np.nonzero(c == t)[0]
        groups.append(rows)
        towers.append(None)
        if len(rows):
            u = np.concatenate([x[rows, : (t + 1) * d], extra[rows]], axis=1)
            towers[t] = G.forward_saved(u, _trunk_net(net.towers[t]))[2]
            h[rows] = towers[t][-1]["h"]
    z = np.concatenate([h, extra], axis=1)
    policy = CR.M.linear(z, np.asarray(net.policy[0], F32), net.policy[1])
    value = CR.M.linear(z, np.asarray(net.value[0], F32), net.value[1])[:, 0]
    return policy, value, dict(c=c, order=grouped_order(c), groups=groups, towers=towers, z=z)


def tower_backward(saved, blocks, D):
    """pvgrad_rules.backward's block loop from the gradient D at the trunk's result: per block a dict {dense1, dense2,
    proj} of pvgrad_rules.dense_grads"""
    out = [None] * len(blocks)
    with np.errstate(all="ignore"):
        for l in reversed(range(len(blocks))):
            b, s = blocks[l], saved[l]
            e = np.where(s["h"] > 0, D, ZERO).astype(F32)
            w1 = np.asarray(b.dense1.weight, F32)
            if b.kind == "dense":
                out[l] = dict(dense1=G.dense_grads(e, s["a_in"], b.dense1[:2]), dense2=None, proj=None)
                D = G.chain_t(e, w1) if l else None
                continue
            dz2, gs2, gb2 = G.gnb(e, s["z2"], b.dense2, b.eps)
            da = G.chain_t(dz2, b.dense2.weight)
            da = np.where(s["a"] > 0, da, ZERO).astype(F32)
            dz1, gs1, gb1 = G.gnb(da, s["z1"], b.dense1, b.eps)
            got = dict(dense1=G.dense_grads(dz1, s["a_in"], b.dense1, gs1, gb1),
                       dense2=G.dense_grads(dz2, s["a"], b.dense2, gs2, gb2), proj=None)
            dzp = None
            if s["zp"] is not None:
                dzp, gsp, gbp = G.gnb(e, s["zp"], b.proj, b.eps)
                got["proj"] = G.dense_grads(dzp, s["a_in"], b.proj, gsp, gbp)
            out[l] = got
            if l:
                d1 = G.chain_t(dz1, w1)
                D = d1 + e if dzp is None else d1 + G.chain_t(dzp, b.proj.weight)
    return out


def _zero_dense(dense, normed):
    """a Dense's gradients where no row reached it: +0 in every parameter that exists"""
    z = lambda a: None if a is None else np.zeros(np.shape(a), F32)  # noqa: E731
    return dict(d_weight=z(dense[0]), d_bias=z(dense[1]), d_gn_scale=z(dense[2]) if normed else None,
                d_gn_bias=z(dense[3]) if normed else None)


def zero_tower(blocks):
    out = []
    for b in blocks:
        if b.kind == "dense":
            out.append(dict(dense1=_zero_dense(b.dense1, False), dense2=None, proj=None))
        else:
            out.append(dict(dense1=_zero_dense(b.dense1, True), dense2=_zero_dense(b.dense2, True),
                            proj=_zero_dense(b.proj, True) if b.proj is not None else None))
    return out


def backward(saved, net, grad_policy, grad_value_raw):
    """(towers, policy, value): per tower pvgrad_rules.backward's list of blocks (zero_tower where it has no rows), then the
    heads' pvgrad_rules.dense_grads.  grad_policy [B, A] and grad_value_raw [B] (the gradient at the value head BEFORE its
    tanh) are indexed by the rows' own indices."""
    Gp = np.asarray(grad_policy, F32)
    dzh = np.concatenate([Gp, np.asarray(grad_value_raw, F32)[:, None]], axis=1)
    actions = Gp.shape[1]
    n = CR.n_last(net)
    order = saved["order"]
    # the heads: every row, in grouped order, over all n_last + e inputs
    policy = G.dense_grads(dzh[order][:, :actions], saved["z"][order], net.policy)
    value = G.dense_grads(dzh[order][:, actions:], saved["z"][order], net.value)
    wh = np.concatenate([np.asarray(net.policy[0], F32), np.asarray(net.value[0], F32)], axis=0)
    D = G.chain_t(dzh, wh[:, :n])  # the columns of h alone: extra belongs to the input
    towers = []
    for t, blocks in enumerate(net.towers):
        rows = saved["groups"][t]
        towers.append(tower_backward(saved["towers"][t], blocks, D[rows]) if len(rows) else zero_tower(blocks))
    return towers, policy, value


def param_grads(grads):
    """the gradients in ops.CustomnetPlan.params' order: tower after tower, block after block (pvgrad_rules.param_grads'
    order inside a tower), then the policy head's and the value head's.  Pairs (label, array)."""
    towers, policy, value = grads
    out = []
    for t, blocks in enumerate(towers):
        for l, b in enumerate(blocks):
            for which in ("dense1", "dense2", "proj"):
                if b[which] is not None:
                    out += [(f"tower{t}.block{l}.{which}.{n}", b[which][n]) for n in G.NAMES if b[which][n] is not None]
    for label, g in (("policy", policy), ("value", value)):
        out += [(f"{label}.{n}", g[n]) for n in G.NAMES[:2] if g[n] is not None]
    return out
