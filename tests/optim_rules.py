"""The rules of hk_optim_prepare / hk_optim_apply (include/hironaka_hip_optim.h) restated in plain numpy: what
test_optim_rules.py pins to torch's own clip_grad_norm_, Adam and SGD (tests/golden/optim_step.npz) and test_gpu_optim.py
holds the kernels to.  T is np.float32 or np.float64; every operation below rounds once, to T, unless it is an fma."""
import math

import numpy as np

from dqn_rules import fma_exact, same_bits  # noqa: F401  (same_bits: for the tests that import the rules)

MAX_TENSORS, CHUNK_BYTES, THREADS, WAVE = 64, 16384, 256, 64
SCALE, SGD, ADAM = 0, 1, 2


def _fma(a, b, c):
    """fma element by element; a, b, c arrays (or scalars) of one dtype T"""
    c = np.asarray(c)
    dtype = c.dtype
    a, b = np.broadcast_to(np.asarray(a, dtype=dtype), c.shape), np.broadcast_to(np.asarray(b, dtype=dtype), c.shape)
    out = np.empty(c.shape, dtype=dtype)
    fa, fb, fc, fo = a.reshape(-1), b.reshape(-1), c.reshape(-1), out.reshape(-1)
    for i in range(fc.size):
        fo[i] = fma_exact(fa[i], fb[i], fc[i], dtype)
    return out


# ---- hk_optim_prepare -----------------------------------------------------------------------------------------------

def workgroups(numels, dtype):
    esz = np.dtype(dtype).itemsize
    return sum((int(n) * esz + CHUNK_BYTES - 1) // CHUNK_BYTES for n in numels)


def slots(grads):
    """the workspace slots of a chain over `grads` (arrays of one dtype T), in index order: a workgroup owns CHUNK_BYTES
    of one gradient; lane l adds the squares (in double) of the chunk's elements l, l + 256, ... in that order, a wave's
    64 lanes are added as a halving tree, the 4 waves in order"""
    out = []
    with np.errstate(all="ignore"):
        for g in grads:
            g = np.asarray(g).reshape(-1)
            per = CHUNK_BYTES // g.dtype.itemsize
            for begin in range(0, g.size, per):
                x = np.zeros(per, dtype=np.float64)
                part = g[begin:begin + per].astype(np.float64)
                x[:part.size] = part
                x = x.reshape(per // THREADS, THREADS)
                acc = np.zeros(THREADS, dtype=np.float64)
                for k in range(x.shape[0]):
                    acc = acc + x[k] * x[k]
                w = acc.reshape(THREADS // WAVE, WAVE)
                s = WAVE // 2
                while s > 0:
                    w = w[:, :s] + w[:, s:2 * s]
                    s //= 2
                total = w[0, 0]
                for k in range(1, w.shape[0]):
                    total = total + w[k, 0]
                out.append(float(total))
    return out


def sum_squares(grads):
    """the slots added in index order, in double"""
    total = 0.0
    with np.errstate(all="ignore"):
        for v in slots(grads):
            total = float(np.float64(total) + np.float64(v))
    return total


def total_norm(grads, dtype):
    """(T)sqrt(sum), the square root in double"""
    with np.errstate(all="ignore"):
        return np.dtype(dtype).type(np.sqrt(np.float64(sum_squares(grads))))


def clip_coef(norm, max_norm, dtype):
    """c > 1 ? 1 : c with c = ((T)1 / (norm + (T)1e-6)) * (T)max_norm: torch's `max_norm / (total_norm + 1e-6)`, which
    Tensor.__rtruediv__ evaluates as reciprocal() * max_norm, then clamp(max=1), through which a NaN passes"""
    T = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        c = (T(1) / (T(norm) + T(1e-6))) * T(max_norm)
    return T(1) if c > T(1) else T(c)


def new_state():
    return dict(step=0, beta1_pow=1.0, beta2_pow=1.0, total_norm=0.0, clip_coef=0.0, neg_step_size=0.0, bias2_sqrt=0.0,
                lr=0.0)


def prepare(state, grads, dtype, max_norm=math.inf, lr=0.0, beta1=0.0, beta2=0.0, advance=False, clip=True):
    """the state block after hk_optim_prepare (a new dict); clip=False: HK_OPTIM_NO_CLIP, the coefficient is 1"""
    st = dict(state)
    norm = total_norm(grads, dtype)
    st["total_norm"] = float(norm)
    st["clip_coef"] = float(clip_coef(norm, max_norm, dtype)) if clip else 1.0
    st["lr"] = float(lr)
    if advance:
        st["step"] = state["step"] + 1
        st["beta1_pow"] = state["beta1_pow"] * float(beta1)
        st["beta2_pow"] = state["beta2_pow"] * float(beta2)
        with np.errstate(all="ignore"):
            st["neg_step_size"] = float(-(np.float64(lr) / np.float64(1.0 - st["beta1_pow"])))
            st["bias2_sqrt"] = float(np.sqrt(np.float64(1.0 - st["beta2_pow"])))
    return st


# ---- hk_optim_apply -------------------------------------------------------------------------------------------------

def scale(grad, coef):
    with np.errstate(all="ignore"):
        return (grad * grad.dtype.type(coef)).astype(grad.dtype)


def sgd(p, grad, buf, state, weight_decay=0.0, momentum=0.0, dampening=0.0, nesterov=False):
    """(p, clipped grad, buf) after HK_OPTIM_SGD; buf is None without momentum"""
    dtype = p.dtype
    T = dtype.type
    with np.errstate(all="ignore"):
        g = scale(grad, state["clip_coef"])
        d = g
        if weight_decay != 0:
            d = _fma(T(weight_decay), p, d)
        if momentum != 0:
            if state["step"] == 1:
                buf = d.copy()
            else:
                scaled = (buf * T(momentum)).astype(dtype)
                buf = (scaled + d).astype(dtype) if dampening == 0 else _fma(T(1.0 - float(dampening)), d, scaled)
            d = _fma(T(momentum), buf, d) if nesterov else buf
        return _fma(T(-state["lr"]), d, p), g, buf


def adam(p, grad, m, v, state, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """(p, clipped grad, m, v) after HK_OPTIM_ADAM"""
    dtype = p.dtype
    T = dtype.type
    with np.errstate(all="ignore"):
        g = scale(grad, state["clip_coef"])
        d = g
        if weight_decay != 0:
            d = _fma(T(weight_decay), p, d)
        w1 = T(1.0 - float(beta1))
        diff = (d - m).astype(dtype)
        m = _fma(w1, diff, m) if w1 < T(0.5) else _fma(-diff, T(1) - w1, d)
        gw = (T(1.0 - float(beta2)) * d).astype(dtype)
        v = _fma(gw, d, (v * T(beta2)).astype(dtype))
        denom = (np.sqrt(v) / T(state["bias2_sqrt"]) + T(eps)).astype(dtype)
        p = (p + (T(state["neg_step_size"]) * m).astype(dtype) / denom).astype(dtype)
        return p, g, m, v


# ---- the cases of tests/golden/optim_step.npz (make_optim_golden.py writes them) -------------------------------------

STEPS, BATCH, NUM_ACTIONS, LR = 3, 5, 3, 0.05
CASES = (  # name, kind, hyper-parameters
    ("adam", ADAM, dict(betas=(0.9, 0.999))),
    ("adam_wd", ADAM, dict(betas=(0.9, 0.999), weight_decay=0.01)),
    ("adam_low_betas", ADAM, dict(betas=(0.4, 0.9))),
    ("adam_low_betas_wd", ADAM, dict(betas=(0.4, 0.9), weight_decay=0.01)),
    ("sgd", SGD, dict()),
    ("sgd_wd", SGD, dict(weight_decay=0.01)),
    ("sgd_momentum", SGD, dict(momentum=0.9)),
    ("sgd_momentum_dampening", SGD, dict(momentum=0.9, dampening=0.25, weight_decay=0.01)),
    ("sgd_nesterov", SGD, dict(momentum=0.9, nesterov=True)),
)
DTYPES = (np.float32, np.float64)


def case_keys():
    """(key, case name, kind, hyper-parameters, dtype, net kind) of every case of the fixture"""
    from dqn_rules import NET_KINDS
    out = []
    for name, kind, hyper in CASES:
        for dtype in DTYPES:
            for net in NET_KINDS:
                out.append((f"{name}_{np.dtype(dtype).name}_{net}", name, kind, hyper, dtype, net))
    return out


def split(flat, shapes):
    """a flat vector as the list of arrays of `shapes`"""
    out, at = [], 0
    for shape in shapes:
        n = int(np.prod(shape))
        out.append(flat[at:at + n].reshape(shape))
        at += n
    assert at == flat.size
    return out


def ulp(x, dtype):
    """the unit in the last place of |x| in dtype"""
    return np.spacing(np.abs(np.asarray(x)).astype(dtype)).astype(np.longdouble)


def adam_reference(p, clipped, m, v, state, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """Adam's parameters after the step whose scalars `state` holds, evaluated element by element in np.longdouble from
    parameters, state and clipped gradient of type T: the "float64 result" that the tolerance of Adam's last line is
    measured from (for float32 it differs from a float64 evaluation by 2^-29 float32 units; for float64 it is the higher
    precision there is).  The step's two scalars -lr / (1 - beta1^step) and sqrt(1 - beta2^step) are the doubles of the
    state block, as they are doubles in torch: 1 - beta2^step cancels nine bits at beta2 = 0.999, which no evaluation of
    the elements in a wider format should be held against."""
    L = np.longdouble
    p, g, m, v = (np.asarray(x).astype(L) for x in (p, clipped, m, v))
    b1, b2 = L(betas[0]), L(betas[1])
    if weight_decay != 0:
        g = g + L(weight_decay) * p
    m = m + (L(1) - b1) * (g - m)
    v = v * b2 + (L(1) - b2) * g * g
    denom = np.sqrt(v) / L(state["bias2_sqrt"]) + L(eps)
    return p + L(state["neg_step_size"]) * m / denom


def adam_distance(got, want, before, dtype):
    """the largest |got - want| in units of max(ulp(want), ulp(want - before)) of dtype"""
    want, before = np.asarray(want).astype(np.longdouble), np.asarray(before).astype(np.longdouble)
    unit = np.maximum(ulp(want, dtype), ulp(want - before, dtype))
    return float((np.abs(np.asarray(got).astype(np.longdouble) - want) / unit).max())
