"""Randomised parity of the five network kernels -- hk_mlp_forward ("mlp"), hk_train_mlp_forward / hk_train_mlp_backward
("train"), hk_pvnet_forward ("pvnet"), hk_pvgrad_forward / hk_pvgrad_backward ("pvgrad") and hk_customnet_forward
("customnet") -- against their numpy rules, bit for bit, on cases whose axes are drawn JOINTLY: batch, forced tile, widths,
depth, options, input segments, the layout of inputs and outputs, the layout of the parameters (fresh allocations, or every
tensor of the net back to back in one sentinel-padded flat buffer at any 4-byte boundary) and a stray NaN or Inf.

    python tests/fuzz_nets.py --minutes 3 [--seed 0] [--family mlp]      # by hand, on the GPU

Four separable parts, so that everything but the launch runs without a GPU (tests/test_fuzz_nets.py):
    draw(rng, family) -> case     a plain description: numpy arrays and layout numbers, no torch
    rule(case) -> want            the family's rule, and the expected image of every storage and flat buffer
    device(case) -> got           the same names from the operators of hironaka_amd.ops
    compare(case, got, want)      same_bits on every name; raises Mismatch and dumps the arrays under DUMP
tests/test_gpu_fuzz_nets.py runs a fixed, seeded slice (`run_cases`) as a `-m gpu` test.  Case i of a seed has a generator
of its own (`case_rng`), so a failing case is rebuilt from (family, seed, index) alone (`case_at`).

"pvgrad" draws FINITE inputs only (case["nonfinite"] is None): every weight gradient is a chain over all rows of the batch,
so one NaN row reaches every element of every gradient and the case compares NaN masks instead of bits (test_gpu_pvgrad.py
says the same).  Both new families run with raw_value: the tanh path is not pinned to the bit.  "customnet" keeps the
broadcast layout of x: the operator takes a row stride of zero (every row is then the first: one group)."""
import argparse
import collections
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import customnet_rules as C  # noqa: E402
import mlp_rules as M  # noqa: E402
import mlp_train_rules as T  # noqa: E402
import pvgrad_rules as G  # noqa: E402
import pvnet_rules as P  # noqa: E402
from hironaka_amd import _abi as A  # noqa: E402  (constants alone: neither torch nor the library)
from mlp_rules import F32, same_bits  # noqa: E402

# (case_rng seeds by a family's index here: new families go behind the others, whose cases then stay what they were)
FAMILIES = ("mlp", "train", "pvnet", "pvgrad", "customnet")
SENTINEL = -77.25  # test_gpu_mlp.SENTINEL: what Guarded fills its storage with
WIDTHS = (1, 3, 15, 16, 17, 18, 33, 60, 63, 64, 100, 255, 256)
HIDDEN = tuple(w for w in WIDTHS if w >= 8)  # behind a ReLU: a narrower layer leaves rows that are all zero
NORMED = (32, 64, 128, 256)
ACTIONS = (1, 3, 4, 15, 16, 17, 255)
TILES = (None, 16, 64)
TRAIN_BATCHES = (2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024)
TRAIN_CAP = 1024
DEEP = 32
# the rule costs about one fma32 over [batch, n] per k: a case whose batch * sum(k * n) lies above this is drawn again
# (mlp, pvnet: a 256-wide pair of layers at 193 rows; train, whose backward costs twice the forward: a 64-wide net at 1 024)
# (pvgrad: train's, three times the forward -- two narrow dense blocks at 4 096 rows, a 32-wide residue block at 1 024, a
# 256-wide one at 17; customnet: a row runs one tower, the rule besides costs a pass per tower)
WORK_CAP = {"mlp": 30e6, "pvnet": 30e6, "train": 12e6, "pvgrad": 12e6, "customnet": 20e6}
INPUT_KINDS = ("dense", "offset", "stride", "broadcast")
OUTPUT_KINDS = ("dense", "offset", "stride")
# pvgrad: ROWSUM's residues, both sides of the 16-row tile, several tiles, the operator's cap (the nets with the table's
# boundary counts of Denses and the deep ones take the small batches alone: the work cap)
PVGRAD_BATCHES = (1, 2, 3, 15, 16, 17, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096)
PVGRAD_CAP = A.HK_PVGRAD_MAX_BATCH
PVGRAD_TABLE = A.HK_PVGRAD_TABLE  # Denses per launch of the parameter gradients, the two heads among them
# customnet: points, coordinates, features behind the points; the large m cost the rule a pass per tower: drawn less often
POINTS = (1, 2, 5, 20, 63, 64)
DIMS = (2, 3, 4)
EXTRAS = (0, 1, 3, 16)
ODD_WIDTHS = (15, 17, 24, 33)
LARGE_ROWS = (1023, 1024, 1025, 2049)  # the group launch takes 1 024 rows per workgroup
STRUCTURES = ("uniform", "one group", "no tower", "no point", "tile", "extremes")
# what a case may plant at coordinate 0 of a point slot, and whether the rule's `>= 0` counts it a point
EDGES = {"-0": (-0.0, True), "+subnormal": (2.0 ** -149, True), "-subnormal": (-2.0 ** -149, False),
         "nan": (np.nan, False), "+inf": (np.inf, True), "-inf": (-np.inf, False)}

Layout = collections.namedtuple("Layout", "kind offset stride")
Layout.__doc__ = """where a [batch, width] tensor lies in its storage: `offset` elements in, rows `stride` elements apart.
kind: dense, offset (no 16-byte alignment), stride, broadcast (one row, stride 0) or record (a run of columns of the
case's one record; offset is then the column)."""


# where compare leaves the arrays of a mismatch: HK_FUZZ_DUMP, or fuzz_out/ in the repository (kept out of git)
DUMP = os.environ.get("HK_FUZZ_DUMP") or os.path.join(ROOT, "fuzz_out")


class Mismatch(AssertionError):
    pass


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _coin(rng, p=0.5):
    return bool(rng.random() < p)


def inputs(rng, batch, k):
    """entries in [-1, 1], a few zeros and negative zeros (test_gpu_mlp.inputs)"""
    x = rng.uniform(-1, 1, (batch, k)).astype(F32)
    x[rng.random((batch, k)) < 0.05] = 0
    x[rng.random((batch, k)) < 0.02] = -0.0
    return x


# ---- layouts: the numpy image of test_gpu_mlp.Guarded -----------------------------------------------------------------

def _draw_layout(rng, width, kinds):
    kind = _pick(rng, kinds)
    if kind == "dense":
        return Layout(kind, 0, width)
    if kind == "offset":
        return Layout(kind, int(rng.integers(1, 4)), width)
    if kind == "stride":
        return Layout(kind, int(rng.integers(0, 4)), width + int(rng.integers(1, 8)))
    return Layout(kind, int(rng.integers(0, 4)), 0)


def storage_rows(batch, width, lay):
    """(rows, stride) of the Guarded that holds a tensor of this layout"""
    return (1, width) if lay.kind == "broadcast" else (batch, lay.stride)


def image(batch, width, lay, values=None):
    """the storage Guarded(rows, width, lay.offset, stride, values) holds: sentinels, and `values` where the tensor lies"""
    rows, stride = storage_rows(batch, width, lay)
    a = np.full(lay.offset + rows * stride + 8, SENTINEL, F32)
    if values is not None:
        at = lay.offset + np.arange(rows)[:, None] * stride + np.arange(width)[None, :]
        a[at] = np.asarray(values, F32).reshape(batch, width)[:rows]
    return a


def _draw_io(rng, case, ins, outs, together=None):
    """layouts of the tensors `ins` / `outs` ({name: width}): each its own storage, or (one case in five) those of
    `together` (default: all) runs of columns of one record, in a drawn order, with spare columns between and behind them"""
    lay = {}
    for name, width in ins.items():
        lay[name] = _draw_layout(rng, width, INPUT_KINDS)
    for name, width in outs.items():
        lay[name] = _draw_layout(rng, width, OUTPUT_KINDS)
    case["record"] = None
    if _coin(rng, 0.2):
        names = list(ins) + list(outs) if together is None else list(together)
        order = [names[i] for i in rng.permutation(len(names))]
        at = 0
        for name in order:
            at += int(rng.integers(0, 3))
            lay[name] = (at, dict(ins, **outs)[name])
            at += lay[name][1]
        stride = at + int(rng.integers(0, 3))
        for name in names:
            lay[name] = Layout("record", lay[name][0], stride)
        case["record"] = Layout("record", int(rng.integers(0, 4)), stride)
    case["layout"], case["io_widths"] = lay, dict(ins, **outs)
    case["inputs"], case["outputs"] = tuple(ins), tuple(outs)


def _flatten_broadcast(case, x, segments):
    """a broadcast segment holds one row: every row of x becomes the first there"""
    at = 0
    for name, width in segments:
        if case["layout"][name].kind == "broadcast":
            x[:, at:at + width] = x[:1, at:at + width]
        at += width
    return x


def _draw_nonfinite(rng, case, x, segments):
    """one NaN or Inf in one row of x (not in a broadcast segment, which is every row), in one case in sixteen"""
    case["nonfinite"] = None
    if not _coin(rng, 1 / 16):
        return
    cols, at = [], 0
    for name, width in segments:
        if case["layout"][name].kind != "broadcast":
            cols += range(at, at + width)
        at += width
    if cols:
        row, col, value = int(rng.integers(len(x))), int(_pick(rng, cols)), float(_pick(rng, (np.nan, np.nan, np.inf)))
        x[row, col] = value
        case["nonfinite"] = (row, col, "nan" if np.isnan(value) else "inf")


# ---- the parameters: fresh allocations, or back to back in a flat buffer ---------------------------------------------------

def _walk(obj, fn, name=None):
    """obj with fn(field name, array) in place of every numpy array of a nest of namedtuples, tuples and lists"""
    if isinstance(obj, np.ndarray):
        return fn(name, obj)
    if isinstance(obj, tuple) and hasattr(obj, "_fields"):
        return type(obj)(*(_walk(v, fn, f) for f, v in zip(obj._fields, obj)))
    if isinstance(obj, (list, tuple)):
        return type(obj)(_walk(v, fn, name) for v in obj)
    return obj


def _written(case, name):
    return case["family"] == "train" and name in ("bn_mean", "bn_var")


def leaves(case, written=False):
    """the parameter arrays in table order: those the launch only reads, or (train) the running statistics it updates"""
    out = []
    _walk(case["net"], lambda name, a: out.append(a) if _written(case, name) == written else None)
    return out


def grad_shapes(case):
    """the shapes of train's (pvgrad's) gradients in parameter order"""
    if case["family"] == "pvgrad":  # every parameter, in the walk's order: ops.PvnetPlan.params'
        return [a.shape for a in leaves(case)]
    return [a.shape for l in case["net"] for a in (l.weight, l.bias, l.bn_weight, l.bn_bias) if a is not None]


def grads_flat(case):
    """whether the gradients are views of the second flat buffer: train's with flat parameters, pvgrad's by a draw of
    its own"""
    return case["params"] == "flat" if case["family"] == "train" else case.get("grads") == "flat"


def positions(sizes, start, gaps):
    at, pos = [], start
    for size, gap in zip(sizes, gaps):
        at.append(pos)
        pos += size + gap
    return at, pos + 8


def pack(arrays, start, gaps):
    """(flat, at): the arrays back to back (`gaps` sentinels behind each) from element `start` of a sentinel-filled
    buffer with 8 more sentinels at its end; None leaves the sentinels where an array would lie"""
    at, total = positions([a.size for a in arrays], start, gaps)
    flat = np.full(total, SENTINEL, F32)
    for a, p in zip(arrays, at):
        flat[p:p + a.size] = a.ravel()
    return flat, at


def _draw_params(rng, case):
    """fresh allocations or flat buffers: the read-only parameters in one, what train writes (running statistics, then
    the gradients) in a second; each at a start offset 0..3 with 0 or 1 sentinels between neighbours, so that every
    tensor lands on an arbitrary 4-byte boundary"""
    case["params"] = "flat" if _coin(rng) else "fresh"
    read, stats = leaves(case), leaves(case, True)
    extra = len(grad_shapes(case)) if case["family"] in ("train", "pvgrad") else 0
    case["start"], case["gaps"] = int(rng.integers(0, 4)), [int(g) for g in rng.integers(0, 2, len(read))]
    case["start2"], case["gaps2"] = int(rng.integers(0, 4)), [int(g) for g in rng.integers(0, 2, len(stats) + extra)]
    at = positions([a.size for a in read], case["start"], case["gaps"])[0] if case["params"] == "flat" else [0] * len(read)
    # (k, the weight's address modulo 16 bytes in floats): the kernels' 16-byte loads need k % 4 == 0 and the second 0
    case["weights"] = [(a.shape[1], p % 4) for a, p in zip(read, at) if a.ndim == 2]


# ---- draw ---------------------------------------------------------------------------------------------------------------

def _draw_batch(rng, tile):
    t = tile or 16
    return int(_pick(rng, (1, 2, 15, 16, 17, 63, 64, 65, 3 * t - 1, 3 * t, 3 * t + 1)))


def _mlp_widths(rng, nl, deep, opts, widths=WIDTHS, hidden=HIDDEN):
    k = int(_pick(rng, widths))
    if deep:
        return [k] + [int(_pick(rng, (15, 16, 17, 33, 64))) for _ in range(nl - 1)] + [int(_pick(rng, widths))]
    mid = [int(_pick(rng, hidden)) for _ in range(nl - 1)]
    # a narrow first layer that is not between two ReLUs, where a bias keeps the rows behind it apart
    if nl >= 3 and not opts["input_relu"] and opts["bias"] and _coin(rng, 0.25):
        mid[0] = int(_pick(rng, (1, 3)))
    return [k] + mid + [int(_pick(rng, widths))]


def _segments(rng, k):
    """(k0, k1): one segment, or two"""
    if k >= 2 and _coin(rng):
        k1 = int(_pick(rng, [w for w in (1, 3, 4, k // 2, k - 1) if 1 <= w < k]))
        return k - k1, k1
    return k, 0


def _dead_input(k, opts):
    """a narrow input behind a ReLU, with neither a bias nor a batch norm behind it: rows that are zero to the end"""
    return k < 8 and opts["input_relu"] and not (opts["bias"] or opts["bn"])


def _work(batch, widths):
    return batch * sum(k * n for k, n in zip(widths[:-1], widths[1:]))


def _draw_mlp(rng):
    case = dict(family="mlp")
    while True:
        tile = _pick(rng, TILES)
        deep = _coin(rng, 0.04)
        batch = _draw_batch(rng, tile)
        nl = DEEP if deep else int(rng.integers(1, 7))
        opts = {k: _coin(rng) for k in ("bias", "bn", "affine", "input_relu", "last_relu", "input_bn", "input_affine")}
        widths = _mlp_widths(rng, nl, deep, opts)
        if _work(batch, widths) <= WORK_CAP["mlp"] and not _dead_input(widths[0], opts):
            break
    layers = [l._replace(weight=(l.weight * np.sqrt(6.0)).astype(F32))
              for l in M.random_layers(rng, widths, opts["bias"], opts["bn"], opts["affine"], opts["last_relu"])]
    k = widths[0]
    input_bn = None
    if opts["input_bn"]:
        vec = lambda lo, hi: rng.uniform(lo, hi, k).astype(F32)  # noqa: E731
        input_bn = M.Layer(None, None, vec(-0.5, 0.5), vec(0.5, 2.0), *((vec(0.5, 1.5), vec(-0.5, 0.5)) if opts["input_affine"]
                                                                       else (None, None)), 1e-5, False)
    k0, k1 = _segments(rng, k)
    case.update(batch=batch, tile=tile, widths=widths, k0=k0, k1=k1, options=opts, net=(input_bn, layers))
    segments = [("x0", k0)] + ([("x1", k1)] if k1 else [])
    _draw_io(rng, case, dict(segments), {"out": widths[-1]})
    case["x"] = _flatten_broadcast(case, inputs(rng, batch, k), segments)
    _draw_nonfinite(rng, case, case["x"], segments)
    _draw_params(rng, case)
    return case


def _draw_train(rng):
    case = dict(family="train")
    while True:
        opts = {k: _coin(rng) for k in ("bias", "bn", "affine", "input_relu", "last_relu")}
        batch = int(_pick(rng, TRAIN_BATCHES + (() if opts["bn"] else (1, 1))))
        deep = _coin(rng, 0.04)
        nl = DEEP if deep else int(rng.integers(1, 7))
        small = tuple(w for w in WIDTHS if w <= 64)  # large batches: the rule's time
        widths = _mlp_widths(rng, nl, deep, opts, *((small, tuple(w for w in small if w >= 8)) if batch > 65 else ()))
        if 3 * _work(batch, widths) <= WORK_CAP["train"] and not _dead_input(widths[0], opts):
            break
    momentum = float(_pick(rng, (0.1, 0.5, 0.01)))
    layers = [l._replace(weight=(l.weight * np.sqrt(6.0)).astype(F32)) for l in
              T.random_layers(rng, widths, opts["bias"], opts["bn"], opts["affine"], opts["last_relu"], momentum)]
    k0, k1 = _segments(rng, widths[0])
    case.update(batch=batch, tile=None, widths=widths, k0=k0, k1=k1, options=dict(opts, momentum=momentum), net=layers)
    segments = [("x0", k0)] + ([("x1", k1)] if k1 else [])
    # (the operator allocates what it writes: the gradient it reads is the third tensor with a layout)
    _draw_io(rng, case, dict(segments, grad_out=widths[-1]), {})
    case["layout"]["grad_out"] = case["layout"]["grad_out"] if case["layout"]["grad_out"].kind != "broadcast" \
        else Layout("dense", 0, widths[-1])
    case["x"] = _flatten_broadcast(case, rng.standard_normal((batch, widths[0])).astype(F32), segments)
    case["grad"] = T.sparse_grad(rng, batch, widths[-1]) if _coin(rng) else rng.standard_normal((batch, widths[-1])).astype(F32)
    _draw_nonfinite(rng, case, case["x"], segments)
    _draw_params(rng, case)
    return case


def _draw_pvnet(rng):
    case = dict(family="pvnet")
    while True:
        tile = _pick(rng, TILES)
        deep = _coin(rng, 0.04)
        batch = _draw_batch(rng, tile)
        nb = DEEP if deep else int(rng.integers(1, 7))
        bias = _coin(rng)
        k0 = int(_pick(rng, WIDTHS))
        arch, kinds, k = [], [], k0
        for i in range(nb):
            if _coin(rng, 0.6):
                # one time in three the width of the block before, where that is a normed one: no projection
                n = k if k in NORMED and _coin(rng, 1 / 3) else int(_pick(rng, (32, 64) if deep else NORMED))
                kinds.append("residue")
            else:
                # a dense block narrower than 8 leaves rows that are all zero: seldom, and rarely as the last block
                narrow = bias and _coin(rng, 0.15) and (i + 1 < nb or _coin(rng, 0.1))
                n = int(_pick(rng, (1, 3) if narrow else (15, 16, 33, 64) if deep else HIDDEN))
                kinds.append("dense")
            arch.append(n)
            k = n
        actions = int(_pick(rng, ACTIONS))
        if _work(batch, [k0] + arch) + batch * sum(2 * n * n for n, kd in zip(arch, kinds) if kd == "residue") <= WORK_CAP["pvnet"]:
            break
    net = P.random_net(rng, k0, arch, actions, kinds, bias, True, float(_pick(rng, (1.0, 4.0))))
    eps = float(_pick(rng, (P.EPS, P.EPS, 1e-5)))
    drops = []

    def strip(d):  # the scale and the shift of each group norm, separately
        if d is None or d.gn_scale is None:
            return d
        # (a group of one column -- width 32 -- normalises to zero: without its shift the block's output is zero)
        keep = (_coin(rng, 0.7), _coin(rng, 0.7) or d.weight.shape[0] == 32)
        drops.append(keep)
        return d._replace(gn_scale=d.gn_scale if keep[0] else None, gn_bias=d.gn_bias if keep[1] else None)
    net = net._replace(blocks=[b._replace(dense1=strip(b.dense1), dense2=strip(b.dense2), proj=strip(b.proj), eps=eps)
                               for b in net.blocks])
    opts = dict(bias=bias, scale_on=any(s for s, _ in drops), scale_off=any(not s for s, _ in drops),
                shift_on=any(s for _, s in drops), shift_off=any(not s for _, s in drops))
    case.update(batch=batch, tile=tile, widths=[k0] + arch, kinds=kinds, actions=actions, k0=k0, k1=0, options=opts, net=net,
                eps=eps)
    # (the library takes policy and value as columns of one record, but no input next to an output)
    _draw_io(rng, case, {"x0": k0}, {"policy": actions, "value": 1}, together=("policy", "value"))
    case["x"] = _flatten_broadcast(case, inputs(rng, batch, k0), [("x0", k0)])
    _draw_nonfinite(rng, case, case["x"], [("x0", k0)])
    _draw_params(rng, case)
    return case


def _strip_norms(rng, blocks, eps, drops):
    """the blocks with `eps` and with the scale and the shift of each group norm stripped separately (`drops` collects
    what was kept, per normed Dense)"""
    def strip(d):
        if d is None or d.gn_scale is None:
            return d
        # (a group of one column -- width 32 -- normalises to zero: without its shift the block's output is zero)
        keep = (_coin(rng, 0.7), _coin(rng, 0.7) or d.weight.shape[0] == 32)
        drops.append(keep)
        return d._replace(gn_scale=d.gn_scale if keep[0] else None, gn_bias=d.gn_bias if keep[1] else None)
    return [b._replace(dense1=strip(b.dense1), dense2=strip(b.dense2), proj=strip(b.proj), eps=eps) for b in blocks]


def _norm_options(bias, drops):
    return dict(bias=bias, scale_on=any(s for s, _ in drops), scale_off=any(not s for s, _ in drops),
                shift_on=any(s for _, s in drops), shift_off=any(not s for _, s in drops),
                scale_alone=any(s and not t for s, t in drops), shift_alone=any(t and not s for s, t in drops))


def _seldom_broadcast(rng, case, name, p=0.6):
    """a broadcast x makes every row the first: most of the time another layout is drawn in its place"""
    if case["layout"][name].kind == "broadcast" and _coin(rng, p):
        case["layout"][name] = _draw_layout(rng, case["io_widths"][name], OUTPUT_KINDS)


def _pvgrad_menus(batch):
    """(k0, normed widths besides 32, dense widths, the most blocks) that the work cap leaves a batch of this size"""
    if batch <= 65:
        return WIDTHS, (64, 128, 256), HIDDEN + (32,), 6
    if batch <= 257:
        return tuple(w for w in WIDTHS if w <= 100), (64, 128), tuple(w for w in HIDDEN if w <= 64) + (32,), 4
    if batch <= 1025:  # (no normed width but 32 fits: behind a 32-wide dense block)
        return tuple(w for w in WIDTHS if w <= 64), (), (15, 16, 17, 18, 32, 32, 33), 3
    return tuple(w for w in WIDTHS if w <= 33), (), (15, 16, 17, 18, 33), 2  # dense blocks alone


def _pvgrad_trunk(rng, k0, nb, target, normed, dense, narrow, seldom):
    """(block widths, kinds) of nb blocks behind k0 inputs, or None where the draw got stuck.  target: the number of Denses
    the trunk must have exactly (a dense block has one, a residue block two, three with a projection), or None.
    A 32-wide residue block has dz == 0 exactly (a group of one column), so that nothing in front of one WITH a
    projection gets a gradient: width 32 is drawn behind a 32-wide block, where the block needs no projection and the
    gradient passes, and with a projection with the probability `seldom` alone"""
    arch, kinds, k, left = [], [], k0, target
    for i in range(nb):
        if target is None:
            residue = _coin(rng, 0.6)
            same = residue and k in NORMED and _coin(rng, 0.5 if k == 32 else 1 / 3)
        else:
            rest = nb - i - 1
            counts = [c for c in (1, 2, 3) if rest <= left - c <= 3 * rest and (c != 2 or k in NORMED)]
            if not counts:
                return None
            c = int(_pick(rng, counts))
            left -= c
            residue, same = c > 1, c == 2
        if residue and same:
            n = k
        elif residue:
            menu = [w for w in normed if w != k or target is None]
            if k != 32 and seldom and _coin(rng, seldom):
                n = 32
            elif menu:
                n = int(_pick(rng, menu))
            elif target is None and k == 32:
                n = k  # (no other normed width fits the batch: no projection)
            elif target is None:
                residue = False
            else:
                return None
        if not residue:
            # a dense block narrower than 8 leaves rows that are all zero: seldom, and rarely as the last block
            thin = narrow and _coin(rng, 0.15) and (i + 1 < nb or _coin(rng, 0.1))
            n = int(_pick(rng, (1, 3) if thin else dense))
        arch.append(n)
        kinds.append("residue" if residue else "dense")
        k = n
    return arch, kinds


def dense_count(case):
    """the Denses of a pvgrad case as hk_pvgrad_backward's table counts them: those of every block, and the two heads"""
    return sum(1 + (b.dense2 is not None) + (b.proj is not None) for b in case["net"].blocks) + 2


def _draw_pvgrad(rng):
    case = dict(family="pvgrad")
    # what the net is drawn for: the table's boundary (exactly HK_PVGRAD_TABLE Denses, one more), the depth, or freely
    # ("launches": the depth again, with so many residue blocks that the parameter table takes more than two launches,
    # which the work cap leaves the batches up to 3)
    mode = _pick(rng, ("table",) * 2 + ("table + 1",) * 2 + ("deep",) + ("launches",) * 2 + ("free",) * 17)
    # (the rule's weight gradients are chains over the rows, one step of numpy per row and Dense whatever the widths: the
    # batches above 1 000 rows are drawn half as often as the others)
    small = tuple(b for b in PVGRAD_BATCHES if b <= 65)
    often = tuple(b for b in PVGRAD_BATCHES if b <= 257)
    batch = int(_pick(rng, {"free": PVGRAD_BATCHES + often, "deep": small[:6], "launches": small[:3]}.get(mode, small)))
    k0s, normed, dense, most = _pvgrad_menus(batch)
    # (decided once, not per attempt: the nets the work cap turns away are the wide ones, and a 32-wide block is cheap)
    seldom = 0.3 if _coin(rng, 0.03) else 0.0
    while True:
        bias = _coin(rng)
        k0 = int(_pick(rng, k0s))
        # (inputs() draws zeros: without a bias a row of zeros stays one to the end, and a narrow x has such rows)
        if not bias and ((k0 == 1 and batch >= 15) or (k0 == 3 and batch > 257)):
            continue
        if mode == "free":
            trunk = _pvgrad_trunk(rng, k0, int(rng.integers(1, most + 1)), None, normed, dense, bias and batch <= 65, seldom)
        elif mode in ("deep", "launches"):
            # (the deep nets of the larger batches get 64-wide blocks, most without a projection)
            many = mode == "launches"
            trunk = _pvgrad_trunk(rng, k0, DEEP, int(rng.integers(2 * PVGRAD_TABLE, 3 * DEEP - 3)) if many else None,
                                  (64, 128) if many else (64,), (15, 16, 33, 64), False, seldom)
        else:
            target = PVGRAD_TABLE - 2 + (mode == "table + 1")
            trunk = _pvgrad_trunk(rng, k0, int(rng.integers((target + 2) // 3, A.HK_PVNET_MAX_BLOCKS + 1)), target,
                                  (64, 128), (15, 16, 17, 18, 32, 33), False, seldom)
        if trunk is None:
            continue
        arch, kinds = trunk
        actions = int(_pick(rng, ACTIONS if batch <= 257 else tuple(a for a in ACTIONS if a <= 17)))
        widths = [k0] + arch
        work = _work(batch, widths) + batch * sum(n * n + (k != n) * k * n
                                                  for k, n, kd in zip(widths[:-1], arch, kinds) if kd == "residue")
        if 3 * (work + batch * arch[-1] * (actions + 1)) <= WORK_CAP["pvgrad"]:
            break
    net = P.random_net(rng, k0, arch, actions, kinds, bias, True)
    eps = float(_pick(rng, (P.EPS, 1e-5)))
    drops = []
    net = net._replace(blocks=_strip_norms(rng, net.blocks, eps, drops))
    case.update(batch=batch, tile=None, widths=widths, kinds=kinds, actions=actions, k0=k0, k1=0, mode=mode,
                options=_norm_options(bias, drops), net=net, eps=eps)
    case["denses"] = dense_count(case)
    # everything with a layout is read: x and the two gradients at the outputs may be columns of one record
    _draw_io(rng, case, {"x0": k0, "grad_policy": actions, "grad_value": 1}, {})
    for name in ("grad_policy", "grad_value"):  # (the operator copies a gradient whose rows overlap: not a layout of its own)
        if case["layout"][name].kind == "broadcast":
            case["layout"][name] = Layout("dense", 0, case["io_widths"][name])
    _seldom_broadcast(rng, case, "x0")
    case["x"] = _flatten_broadcast(case, inputs(rng, batch, k0), [("x0", k0)])
    case["grad_kind"] = "sparse" if _coin(rng, 0.3) else "mean"
    if case["grad_kind"] == "sparse":  # one non-zero row
        row = int(rng.integers(batch))
        gp, gv = np.zeros((batch, actions), F32), np.zeros(batch, F32)
        gp[row], gv[row] = rng.standard_normal(actions).astype(F32), F32(rng.standard_normal())
    else:  # test_gpu_pvgrad.grads_in: of the size a mean over the batch gives, with a few zeros
        gp = (rng.standard_normal((batch, actions)) / batch).astype(F32)
        gp[rng.random((batch, actions)) < 0.05] = 0
        gv = (rng.standard_normal(batch) / batch).astype(F32)
    case["grad_policy"], case["grad_value"] = gp, gv
    case["nonfinite"] = None  # finite only: a NaN row reaches every weight gradient
    _draw_params(rng, case)
    case["grads"] = "flat" if _coin(rng) else "own"
    return case


def _customnet_counts(rng, structure, batch, m, tile):
    """(the point count of every row, the batch) of a structure; "tile" may ask for more rows"""
    t = tile or 16
    if structure == "uniform":
        return rng.integers(0, m + 1, batch), batch
    if structure == "one group":
        return np.full(batch, int(rng.integers(0, m))), batch
    if structure == "no tower":
        return np.full(batch, m), batch
    if structure == "no point":
        return np.zeros(batch, np.int64), batch
    if structure == "extremes":
        return np.where(rng.random(batch) < 0.5, 0, m), batch
    # one group of exactly the tile's rows, one more or one fewer, among rows of the other counts
    size = t + int(_pick(rng, (-1, 0, 1)))
    if batch < size + 2:
        batch = int(_pick(rng, (3 * t - 1, 3 * t, 3 * t + 1)))
    c = int(rng.integers(0, m + 1))
    others = np.array([v for v in range(m + 1) if v != c])
    cs = np.concatenate([np.full(size, c), others[rng.integers(0, len(others), batch - size)]])
    return cs[rng.permutation(batch)], batch


def _draw_customnet(rng):
    case = dict(family="customnet")
    while True:
        tile = _pick(rng, TILES)
        large = _coin(rng, 0.08)  # more than one workgroup of the group launch, with a small net
        m = int(_pick(rng, (1, 2, 5) if large else POINTS[:4] * 3 + POINTS[4:]))
        d, e = int(_pick(rng, DIMS)), int(_pick(rng, EXTRAS))
        batch = int(_pick(rng, LARGE_ROWS)) if large else _draw_batch(rng, tile)
        nb = 1 if large else int(rng.integers(1, 4))
        kinds = ["residue" if _coin(rng) else "dense" for _ in range(nb)]
        normed = (32, 64) if large or m >= 20 else (32, 64, 128)
        arch = [int(_pick(rng, normed if kd == "residue" else ODD_WIDTHS + (16, 64))) for kd in kinds]
        actions = int(_pick(rng, ACTIONS))
        if m * d + e > A.HK_PVNET_MAX_WIDTH or arch[-1] + e > A.HK_PVNET_MAX_WIDTH:
            continue
        widest = [m * d + e] + arch  # the last tower's widths
        work = _work(batch, widest) + batch * sum(2 * n * n for n, kd in zip(arch, kinds) if kd == "residue")
        # (a pass of the rule over one tower costs what some 400 elements per term of its chains cost)
        if work + 400 * m * (sum(widest) + 2 * sum(n for n, kd in zip(arch, kinds) if kd == "residue")) <= WORK_CAP["customnet"]:
            break
    bias = _coin(rng)
    eps = float(_pick(rng, (P.EPS, 1e-5)))
    net = C.random_net(rng, m, d, e, arch, actions, kinds, bias, True, float(_pick(rng, (1.0, 4.0))))
    drops = []
    net = net._replace(towers=[_strip_norms(rng, tower, eps, drops) for tower in net.towers])
    structure = "no tower" if _coin(rng, 0.03) else _pick(rng, ("uniform", "uniform", "one group", "no point", "tile", "tile",
                                                                  "extremes"))
    cs, batch = _customnet_counts(rng, structure, batch, m, tile)
    holes = _coin(rng, 0.3)
    k = m * d + e
    case.update(batch=batch, tile=tile, m=m, d=d, e=e, widths=[k] + arch, kinds=kinds, actions=actions, k0=k, k1=0,
                options=_norm_options(bias, drops), net=net, eps=eps, structure=structure, holes=holes)
    _draw_io(rng, case, {"x0": k}, {"policy": actions, "value": 1}, together=("policy", "value"))
    _seldom_broadcast(rng, case, "x0")
    x = C.rows_with_counts(rng, cs, m, d, e, holes)
    # an edge value at coordinate 0 of one point slot, which decides the tower of its row; one time in five a NaN or an Inf
    # in another column as well.  (the finite ones are drawn twice as often: the non-finite cases have a cap)
    case["nonfinite"] = None
    if _coin(rng, 0.18):
        lone = case["layout"]["x0"].kind == "broadcast"  # (every row is the first)
        row, slot = 0 if lone else int(rng.integers(batch)), int(rng.integers(m))
        kind = _pick(rng, ("-0", "+subnormal", "-subnormal") * 2 + ("nan", "+inf", "-inf"))
        x[row, slot * d] = F32(EDGES[kind][0])
        planted = [(row, slot * d, kind)]
        if _coin(rng, 0.2):
            row2, col = 0 if lone else int(rng.integers(batch)), int(_pick(rng, [c for c in range(k) if c != slot * d]))
            other = _pick(rng, ("nan", "nan", "+inf"))
            x[row2, col] = F32(EDGES[other][0])
            planted.append((row2, col, other))
        case["nonfinite"] = tuple(planted)
    case["x"] = _flatten_broadcast(case, x, [("x0", k)])
    _draw_params(rng, case)
    return case


_DRAW = {"mlp": _draw_mlp, "train": _draw_train, "pvnet": _draw_pvnet, "pvgrad": _draw_pvgrad, "customnet": _draw_customnet}


def draw(rng, family):
    case = _DRAW[family](rng)
    case.setdefault("index", None)
    case.setdefault("seed", None)
    return case


def case_rng(family, seed, index):
    return np.random.default_rng([int(seed), FAMILIES.index(family), int(index)])


def case_at(family, seed, index):
    """case `index` of the slice of `seed`: what run_cases(family, count > index, seed) runs there"""
    case = draw(case_rng(family, seed, index), family)
    case["index"], case["seed"] = index, seed
    return case


def scalars(case):
    """the case without its arrays"""
    keep = ("family", "index", "seed", "batch", "tile", "widths", "kinds", "actions", "k0", "k1", "options", "eps", "layout",
            "record", "params", "start", "gaps", "start2", "gaps2", "nonfinite", "mode", "denses", "grad_kind", "grads",
            "m", "d", "e", "structure", "holes")
    return {k: case[k] for k in keep if k in case}


# ---- rule ---------------------------------------------------------------------------------------------------------------

def _io_images(case, values):
    """the expected storages of the tensors with a layout: {name + ".store": image} or {"record.store": image}"""
    batch, lay, widths = case["batch"], case["layout"], case["io_widths"]
    out = {name + ".store": image(batch, widths[name], lay[name], values.get(name)) for name in lay if lay[name].kind != "record"}
    if case["record"] is not None:
        out["record.store"] = image(batch, case["record"].stride, case["record"], _record(case, values))
    return out


def _record(case, values):
    """the case's record as [batch, stride]: sentinels, and the tensors that are columns of it"""
    lay, widths = case["layout"], case["io_widths"]
    rec = np.full((case["batch"], case["record"].stride), SENTINEL, F32)
    for name in lay:
        if lay[name].kind == "record" and values.get(name) is not None:
            rec[:, lay[name].offset:lay[name].offset + widths[name]] = np.asarray(values[name], F32).reshape(case["batch"], -1)
    return rec


def _param_images(case, stats_after=None, grads=None):
    """"params": the read-only parameters as the launch must leave them -- the flat buffer, or the arrays one behind the
    other; "written" (where grads_flat): the second buffer with train's updated statistics and the gradients"""
    read = leaves(case)
    out = {"params": np.concatenate([a.ravel() for a in read]) if case["params"] == "fresh"
           else pack(read, case["start"], case["gaps"])[0]}
    if grads_flat(case):
        out["written"] = pack(list(stats_after or ()) + list(grads), case["start2"], case["gaps2"])[0]
    return out


def _segments_of(case):
    k0 = case["k0"]
    x = case["x"]
    return {"x0": x[:, :k0], **({"x1": x[:, k0:]} if case["k1"] else {})}


def rule(case):
    family, x = case["family"], case["x"]
    want = {}
    values = _segments_of(case)
    if family == "mlp":
        input_bn, layers = case["net"]
        out = M.forward(x, layers, case["options"]["input_relu"], input_bn)
        want["out"] = out
        values["out"] = out
        want.update(_param_images(case))
    elif family == "pvnet":
        policy, value = P.forward(x, case["net"])
        want["policy"], want["value"] = policy, value
        values.update(policy=policy, value=value)
        want.update(_param_images(case))
    elif family == "pvgrad":
        policy, value, saved = G.forward_saved(x, case["net"])
        grads = G.param_grads(G.backward(saved, case["net"], case["grad_policy"], case["grad_value"]))
        want["policy"], want["value"] = policy, value
        for j, (_, g) in enumerate(grads):
            want[f"grad{j}"] = np.ascontiguousarray(g, F32)
        values.update(grad_policy=case["grad_policy"], grad_value=case["grad_value"])
        want.update(_param_images(case, None, [g for _, g in grads]))
    elif family == "customnet":
        policy, value = C.forward(x, case["net"], case["m"], case["d"], case["e"])
        want["policy"], want["value"] = policy, value
        values.update(policy=policy, value=value)
        want.update(_param_images(case))
        want["workspace"] = np.zeros(1 + A.HK_CUSTOMNET_MAX_POINTS + 1, np.int32)  # the ticket and the histogram: zero again
    else:
        layers = case["net"]
        out, saved, stats = T.forward(x, layers, case["options"]["input_relu"])
        grads = T.param_grads(layers, T.backward(layers, saved, case["grad"]))
        want["out"] = out
        for i, (l, s, st) in enumerate(zip(layers, saved, stats)):
            want[f"act{i}"] = s["act"]
            if l.bn_mean is not None:
                want.update({f"z{i}": s["z"], f"mean{i}": s["mean"], f"inv{i}": s["inv"], f"running_mean{i}": st[0],
                             f"running_var{i}": st[1]})
        want["num_batches_tracked"] = np.ones(sum(l.bn_mean is not None for l in layers), np.int64)
        for j, g in enumerate(grads):
            want[f"grad{j}"] = np.ascontiguousarray(g, F32)
        values["grad_out"] = case["grad"]
        want.update(_param_images(case, [a for st in stats if st[0] is not None for a in st], grads))
    want.update(_io_images(case, values))
    return want


def last_hidden(case):
    """the activations the last Linear (pvnet: the heads) reads, by the rule; None for a net of one layer"""
    family, x = case["family"], case["x"]
    if family in ("pvnet", "pvgrad"):
        return P.trunk(x, case["net"].blocks)
    if family == "customnet":  # the chosen tower's result, of the rows that have a tower
        m, d = case["m"], case["d"]
        c = C.counts(x, m, d)
        rows = [P.trunk(np.concatenate([x[c == t, : (t + 1) * d], x[c == t, m * d:]], axis=1), case["net"].towers[t])
                for t in range(m) if (c == t).any()]
        return np.concatenate(rows) if rows else None
    if len(case["widths"]) < 3:
        return None
    if family == "mlp":
        input_bn, layers = case["net"]
        return M.forward(x, layers[:-1], case["options"]["input_relu"], input_bn)
    return T.forward(x, case["net"][:-1], case["options"]["input_relu"])[0]


def degenerate(case, want=None):
    """some row's last hidden activations are all zero: nothing behind that point is tested on it (customnet: of the rows
    with a tower; those without are zero by design).  pvgrad as well: the gradient of the first block's weight is all
    zero by the rule (`want`: rule(case), where the caller has it)."""
    h = last_hidden(case)
    if h is not None and bool((h == 0).all(axis=1).any()):
        return True
    if case["family"] == "pvgrad":
        return not (rule(case) if want is None else want)["grad0"].any()
    return False


# ---- device -------------------------------------------------------------------------------------------------------------

def _device_io(case, values):
    """({name: tensor view}, {store name: Guarded}) for the tensors with a layout, filled with `values` where given"""
    from test_gpu_mlp import SENTINEL as theirs
    from test_gpu_mlp import Guarded
    assert theirs == SENTINEL
    batch, lay, widths = case["batch"], case["layout"], case["io_widths"]
    views, stores = {}, {}
    if case["record"] is not None:
        rec = stores["record.store"] = Guarded(batch, case["record"].stride, case["record"].offset, case["record"].stride,
                                               _record(case, values))
    for name in lay:
        if lay[name].kind == "record":
            views[name] = rec.view[:, lay[name].offset:lay[name].offset + widths[name]]
            continue
        rows, stride = storage_rows(batch, widths[name], lay[name])
        v = values.get(name)
        g = stores[name + ".store"] = Guarded(rows, widths[name], lay[name].offset, stride,
                                              None if v is None else np.ascontiguousarray(v.reshape(batch, -1)[:rows]))
        views[name] = g.view.expand(batch, widths[name]) if lay[name].kind == "broadcast" else g.view
    return views, stores


def _device_net(case):
    """(the net with device tensors in place of its arrays, read, written): read / written are the flat buffers (or,
    fresh, `read` is the list of tensors); train's gradient tensors come behind the statistics in `written`"""
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    if case["params"] == "fresh":
        made = []

        def fresh(name, a):
            t = dev(a)
            if not _written(case, name):
                made.append(t)
            return t
        return _walk(case["net"], fresh), made, None, None
    read, stats = leaves(case), leaves(case, True)
    flat, at = pack(read, case["start"], case["gaps"])
    flat, at = dev(flat), iter(at)
    flat2, at2, grads = None, iter(()), None
    if case["family"] == "train":
        shapes = grad_shapes(case)
        flat2, where = pack(stats + [np.full(s, SENTINEL, F32) for s in shapes], case["start2"], case["gaps2"])
        flat2 = dev(flat2)
        at2 = iter(where)
        grads = [flat2[p:p + int(np.prod(s))].view(*s) for p, s in zip(where[len(stats):], shapes)]

    def view(name, a):
        buf, p = (flat2, next(at2)) if _written(case, name) else (flat, next(at))
        return buf[p:p + a.size].view(*a.shape)
    return _walk(case["net"], view), flat, flat2, grads


def _np(t):
    return t.detach().cpu().numpy()


def device(case):
    import torch
    from hironaka_amd import ops
    family = case["family"]
    values = _segments_of(case)
    if family == "train":
        values["grad_out"] = case["grad"]
    if family == "pvgrad":
        values.update(grad_policy=case["grad_policy"], grad_value=case["grad_value"])
    views, stores = _device_io(case, values)
    net, read, written, grads = _device_net(case)
    got = {}
    blocks = lambda bs: [ops.PvnetBlock(b.kind, *(None if d is None else ops.PvnetDense(*d)  # noqa: E731
                                                  for d in (b.dense1, b.dense2, b.proj)), b.eps) for b in bs]
    if family == "pvgrad":
        if case["grads"] == "flat":  # the gradients as views of a second sentinel-padded flat buffer
            shapes = grad_shapes(case)
            flat2, where = pack([np.full(s, SENTINEL, F32) for s in shapes], case["start2"], case["gaps2"])
            written = torch.from_numpy(flat2).cuda()
            grads = [written[p:p + int(np.prod(s))].view(*s) for p, s in zip(where, shapes)]
        plan = ops.PvnetPlan(blocks(net.blocks), net.policy, net.value)
        p, v, saved = ops.pvnet_train_forward(views["x0"], plan, raw_value=True)
        gs = ops.pvnet_backward(saved, views["grad_policy"], views["grad_value"][:, 0], grads=grads)
        assert grads is None or all(g is t for g, t in zip(gs, grads))
        got["policy"], got["value"] = _np(p), _np(v)
        for j, g in enumerate(gs):
            got[f"grad{j}"] = _np(g)
        if written is not None:
            got["written"] = _np(written)
    elif family == "customnet":
        plan = ops.CustomnetPlan([blocks(tower) for tower in net.towers], net.policy, net.value, (case["m"], case["d"]), case["e"])
        p, v = ops.customnet_forward(views["x0"], plan, tile=case["tile"], raw_value=True,
                                     out=(views["policy"], views["value"][:, 0]))
        got["policy"], got["value"] = _np(p), _np(v)
        # the ticket and the histogram at the head of the plan's workspace (words 1 and 4 .. 68)
        head = _np(plan.workspace.view(torch.int32).reshape(-1)[:72])
        got["workspace"] = head[[1] + list(range(4, 5 + A.HK_CUSTOMNET_MAX_POINTS))]
    elif family == "mlp":
        input_bn, layers = net
        out = ops.mlp_forward(views["x0"], [ops.MlpLayer(*l) for l in layers], x1=views.get("x1"),
                              input_relu=case["options"]["input_relu"], out=views["out"], tile=case["tile"],
                              input_bn=None if input_bn is None else ops.MlpLayer(*input_bn))
        assert out is views["out"]
        got["out"] = _np(out)
    elif family == "pvnet":
        dn = lambda d: None if d is None else ops.PvnetDense(*d)  # noqa: E731
        plan = ops.PvnetPlan([ops.PvnetBlock(b.kind, dn(b.dense1), dn(b.dense2), dn(b.proj), b.eps) for b in net.blocks],
                             net.policy, net.value)
        p, v = ops.pvnet_forward(views["x0"], plan, tile=case["tile"], raw_value=True, policy=views["policy"],
                                 value=views["value"][:, 0])
        got["policy"], got["value"] = _np(p), _np(v)
    else:
        counters = [torch.zeros((), dtype=torch.int64, device="cuda") if l.bn_mean is not None else None for l in net]
        dl = [ops.MlpTrainLayer(*l[:8], float(l.momentum), c) for l, c in zip(net, counters)]
        out, sv = ops.mlp_train_forward(views["x0"], ops.MlpTrainPlan(dl, case["options"]["input_relu"]), x1=views.get("x1"))
        gs = ops.mlp_backward(sv, views["grad_out"], grads=grads)
        got["out"] = _np(out)
        for i, l in enumerate(net):
            act, z, mean, inv = sv.layer(i)
            got[f"act{i}"] = _np(act)
            if l.bn_mean is not None:
                got.update({f"z{i}": _np(z), f"mean{i}": _np(mean), f"inv{i}": _np(inv), f"running_mean{i}": _np(l.bn_mean),
                            f"running_var{i}": _np(l.bn_var)})
        got["num_batches_tracked"] = np.array([int(c) for c in counters if c is not None], np.int64)
        for j, g in enumerate(gs):
            got[f"grad{j}"] = _np(g)
        if written is not None:
            got["written"] = _np(written)
    got["params"] = _np(read) if case["params"] == "flat" else np.concatenate([_np(t).ravel() for t in read])
    for name, g in stores.items():
        got[name] = _np(g.store)
    return got


# ---- compare ------------------------------------------------------------------------------------------------------------

def compare(case, got, want):
    """every array of `want` against `got`, bit for bit (NaNs in the same places)"""
    names = [k for k in want if k not in got] + [k for k in got if k not in want]
    bad = names or [k for k in want if not same_bits(np.asarray(got[k]), np.asarray(want[k]))]
    if not bad:
        return
    dump = DUMP
    os.makedirs(dump, exist_ok=True)
    arrays = {f"got.{k}": np.asarray(v) for k, v in got.items() if k in bad}
    arrays.update({f"want.{k}": np.asarray(v) for k, v in want.items() if k in bad})
    np.savez(os.path.join(dump, f"fuzz_nets_mismatch_{case['family']}.npz"), cfg=np.array(repr(scalars(case))), **arrays)
    raise Mismatch(f"{case['family'].upper()} MISMATCH in {bad} at case {case['index']} of seed {case['seed']}: {scalars(case)}")


def run_cases(family: str, count: int, seed: int) -> int:
    """`count` seeded cases of one family (the slice the -m gpu test runs)"""
    for index in range(count):
        case = case_at(family, seed, index)
        compare(case, device(case), rule(case))
    return count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--family", choices=FAMILIES, default=None)
    args = ap.parse_args()
    families = [args.family] if args.family else list(FAMILIES)
    t_end = time.time() + 60 * args.minutes
    n = 0
    while time.time() < t_end:
        family = families[n % len(families)]
        case = case_at(family, args.seed, n // len(families))
        try:
            compare(case, device(case), rule(case))
        except Mismatch as e:
            print(e, flush=True)
            sys.exit(1)
        n += 1
        if n % 100 == 0:
            print(f"{n} cases ok", flush=True)
    print(f"fuzz ok: {n} cases", flush=True)


if __name__ == "__main__":
    main()
