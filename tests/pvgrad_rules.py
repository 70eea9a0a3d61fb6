"""The rule of hk_pvgrad_forward / hk_pvgrad_backward (include/hironaka_hip_pvgrad.h) in numpy, built on pvnet_rules (the
forward, the group norm's balanced sums), mlp_rules.fma32 and mlp_train_rules' CHAIN padding and ROWSUM: float32, every
operation rounded once.  test_pvgrad_rules.py pins the group norm's backward by hand and the rule to torch within torch's own
distance of a float64 run; test_gpu_pvgrad.py holds the kernels to the rule bit for bit."""
import numpy as np

import mlp_rules as M
import mlp_train_rules as T
import pvnet_rules as P
from mlp_rules import F32, fma32, same_bits  # noqa: F401

ZERO = F32(0)


def _gn_parts(z, eps):
    """(d, inv, g) of the forward's group norm on z [B, n], inv repeated over the group's columns"""
    g = z.shape[1] // P.GROUPS
    with np.errstate(all="ignore"):
        mean = P.group_sum(z, g) / F32(g)
        d = z - np.repeat(mean, g, axis=1)
        var = P.group_sum(d * d, g) / F32(g)
        inv = np.repeat(F32(1) / np.sqrt(var + F32(eps)), g, axis=1)
    return d, inv, g


def forward_saved(x, net):
    """(policy, raw value, saved): pvnet_rules.forward's results, and per block a dict of what the backward needs -- a_in,
    h (the block's output) and, for a residue block, z1, a, z2, zp (None without a projection)"""
    h = np.asarray(x, F32)
    saved = []
    for b in net.blocks:
        s = dict(a_in=h)
        if b.kind == "dense":
            h = M.relu(P.dense(h, b.dense1, False, b.eps))
        else:
            s["z1"] = P.dense(h, b.dense1, False, b.eps)
            s["a"] = M.relu(P.group_norm(s["z1"], b.dense1.gn_scale, b.dense1.gn_bias, b.eps))
            s["z2"] = P.dense(s["a"], b.dense2, False, b.eps)
            y = P.group_norm(s["z2"], b.dense2.gn_scale, b.dense2.gn_bias, b.eps)
            n, k = b.dense1.weight.shape
            s["zp"] = None if k == n else P.dense(h, b.proj, False, b.eps)
            o = h if k == n else P.group_norm(s["zp"], b.proj.gn_scale, b.proj.gn_bias, b.eps)
            with np.errstate(all="ignore"):
                h = M.relu(o + y)
        s["h"] = h
        saved.append(s)
    policy = M.linear(h, np.asarray(net.policy[0], F32), net.policy[1])
    value = M.linear(h, np.asarray(net.value[0], F32), net.value[1])[:, 0]
    return policy, value, saved


def chain_t(dz, weight):
    """D[b, j] = CHAIN(+0; dz[b, i] * weight[i, j], i ascending)"""
    dz, weight = np.asarray(dz, F32), np.asarray(weight, F32)
    acc = np.zeros((dz.shape[0], weight.shape[1]), F32)
    for i in range(weight.shape[0]):
        acc = fma32(dz[:, i:i + 1], weight[i][None, :], acc)
    with np.errstate(all="ignore"):
        return T._pad(acc, weight.shape[0])


def gnb(e, z, dense, eps):
    """(dz, d_gn_scale, d_gn_bias) of the group norm behind a Dense whose result was z, for the gradient e at its output"""
    e = np.asarray(e, F32)
    d, inv, g = _gn_parts(np.asarray(z, F32), eps)
    with np.errstate(all="ignore"):
        xhat = d * inv
        u = e * np.asarray(dense.gn_scale, F32) if dense.gn_scale is not None else e
        m1 = np.repeat(P.group_sum(u, g) / F32(g), g, axis=1)
        m2 = np.repeat(P.group_sum(u * xhat, g) / F32(g), g, axis=1)
        dz = inv * ((u - m1) - xhat * m2)
        return np.ascontiguousarray(dz, F32), T.rowsum(e * xhat), T.rowsum(e)


def dense_grads(dz, a_in, dense, d_gn_scale=None, d_gn_bias=None):
    """dict(d_weight, d_bias, d_gn_scale, d_gn_bias, dz) of one Dense: None where the parameter is"""
    dz, a_in = np.ascontiguousarray(dz, F32), np.asarray(a_in, F32)
    dw = np.zeros((dz.shape[1], a_in.shape[1]), F32)
    for b in range(dz.shape[0]):
        dw = fma32(dz[b][:, None], a_in[b][None, :], dw)
    with np.errstate(all="ignore"):
        dw = T._pad(dw, dz.shape[0])
    return dict(d_weight=dw, d_bias=T.rowsum(dz) if dense[1] is not None else None,
                d_gn_scale=d_gn_scale if len(dense) > 2 and dense.gn_scale is not None else None,
                d_gn_bias=d_gn_bias if len(dense) > 2 and dense.gn_bias is not None else None, dz=dz)


def backward(saved, net, grad_policy, grad_value_raw):
    """per block a dict {dense1, dense2, proj} of dense_grads (None where the block has none), then "policy" and "value":
    (blocks, policy, value).  grad_value_raw [B]: the gradient at the value head BEFORE its tanh (dzh[:, A] of the header:
    t * (1 - v * v) with the stored tanh value, or t itself with HK_PVNET_RAW_VALUE)."""
    G = np.asarray(grad_policy, F32)
    dzh = np.concatenate([G, np.asarray(grad_value_raw, F32)[:, None]], axis=1)
    actions = G.shape[1]
    wh = np.concatenate([np.asarray(net.policy[0], F32), np.asarray(net.value[0], F32)], axis=0)
    h_last = saved[-1]["h"]
    policy = dense_grads(dzh[:, :actions], h_last, net.policy)
    value = dense_grads(dzh[:, actions:], h_last, net.value)
    D = chain_t(dzh, wh)
    blocks = [None] * len(net.blocks)
    with np.errstate(all="ignore"):
        for l in reversed(range(len(net.blocks))):
            b, s = net.blocks[l], saved[l]
            e = np.where(s["h"] > 0, D, ZERO).astype(F32)
            w1 = np.asarray(b.dense1.weight, F32)
            if b.kind == "dense":
                blocks[l] = dict(dense1=dense_grads(e, s["a_in"], b.dense1[:2]), dense2=None, proj=None)
                D = chain_t(e, w1) if l else None
                continue
            dz2, gs2, gb2 = gnb(e, s["z2"], b.dense2, b.eps)
            da = chain_t(dz2, b.dense2.weight)
            da = np.where(s["a"] > 0, da, ZERO).astype(F32)
            dz1, gs1, gb1 = gnb(da, s["z1"], b.dense1, b.eps)
            got = dict(dense1=dense_grads(dz1, s["a_in"], b.dense1, gs1, gb1),
                       dense2=dense_grads(dz2, s["a"], b.dense2, gs2, gb2), proj=None)
            dzp = None
            if s["zp"] is not None:
                dzp, gsp, gbp = gnb(e, s["zp"], b.proj, b.eps)
                got["proj"] = dense_grads(dzp, s["a_in"], b.proj, gsp, gbp)
            blocks[l] = got
            if l:
                d1 = chain_t(dz1, w1)
                D = d1 + e if dzp is None else d1 + chain_t(dzp, b.proj.weight)
    return blocks, policy, value


NAMES = ("d_weight", "d_bias", "d_gn_scale", "d_gn_bias")


def param_grads(grads):
    """the gradients in ops.PvnetPlan.params' order: per block dense1, dense2, proj (those it has), per Dense weight, bias,
    gn_scale, gn_bias (those that exist); then the policy head's and the value head's.  Pairs (label, array)."""
    blocks, policy, value = grads
    out = []
    for l, b in enumerate(blocks):
        for which in ("dense1", "dense2", "proj"):
            if b[which] is not None:
                out += [(f"block{l}.{which}.{n}", b[which][n]) for n in NAMES if b[which][n] is not None]
    for label, g in (("policy", policy), ("value", value)):
        out += [(f"{label}.{n}", g[n]) for n in NAMES[:2] if g[n] is not None]
    return out


def tanh_grad(grad_value, value_tanh):
    """dzh[:, A] of the header from t = grad_value and the stored tanh value v: t * (1 - v * v), each operation rounded"""
    v = np.asarray(value_tanh, F32)
    with np.errstate(all="ignore"):
        return (np.asarray(grad_value, F32) * (F32(1) - v * v)).astype(F32)
