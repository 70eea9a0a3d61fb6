"""The lane body of hk_dqn_agent_move and the host's pick of hk_dqn_host_move run on the CPU: tests/dqn_move_lane.hip
builds hk_dqn_move_kernel.h's dqn_agent_lane and dqn_first_argmax for the host under AddressSanitizer +
UndefinedBehaviorSanitizer (a stand-alone program with its own main: nothing is loaded into Python under a sanitizer).
Every game runs in two memory layouts and under four fills of whatever is not an input; the program itself fails on a
fill-dependent result or a touched canary, the sanitizers on an overrun.  Here its results are compared with
tests/dqn_move_rules.py as bit patterns, without tolerances.  No GPU is involved: what this cannot show is the device
compiler's code for the same source."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import dqn_move_rules as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hironaka_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "dqn_move_lane.hip")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-host-only", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
         "-I", CSRC, "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
SHAPES = ((1, 2), (2, 2), (5, 2), (20, 3), (8, 4), (12, 5), (6, 6), (6, 7), (64, 3), (64, 7))
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/dqn_move_lane.hip, compiled once; returns run(blocks) -> the results per block, where a block is
    (m, d, masked, rescale, points [count, m, d], q [count, d], class_id [count], host_q [count, classes]) and the
    dtypes of points and q select the instantiation"""
    where = tmp_path_factory.mktemp("dqn_move_lane")
    exe = str(where / "dqn_move_lane")
    done = subprocess.run([HIPCC] + FLAGS + [SOURCE, "-o", exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    serial = itertools.count()

    def run(blocks):
        stem = str(where / ("cases%d" % next(serial)))
        with open(stem + ".in", "wb") as f:
            f.write(b"HKDM" + struct.pack("<2i", 1, len(blocks)))
            for m, d, masked, rescale, points, q, cls, host_q in blocks:
                f.write(struct.pack("<7i", m, d, DTYPES.index(points.dtype.type), DTYPES.index(q.dtype.type),
                                    int(masked), int(rescale), len(points)))
                f.write(np.ascontiguousarray(points).tobytes() + np.ascontiguousarray(q).tobytes()
                        + np.ascontiguousarray(cls, np.int32).tobytes() + np.ascontiguousarray(host_q).tobytes())
        done = subprocess.run([exe, stem + ".in", stem + ".out"], capture_output=True, text=True, timeout=600)
        if done.returncode != 0:
            print(done.stderr[-8000:])
        assert done.returncode == 0, "exit status %d\n%s" % (done.returncode, done.stderr[-4000:])
        assert not any(word in done.stderr for word in ("Sanitizer", "runtime error", "FAILED")), done.stderr[-4000:]
        raw, at, res = open(stem + ".out", "rb").read(), 0, []
        for m, d, _, _, points, _, _, _ in blocks:
            count, got = len(points), {}
            for name, kind, shape in (("points", points.dtype, (count, m, d)), ("features", points.dtype, (count, m, d)),
                                      ("axis", np.int32, (count,)), ("done", np.int32, (count,)),
                                      ("prev_done", np.int32, (count,)), ("host_class", np.int32, (count,))):
                size = int(np.prod(shape)) * np.dtype(kind).itemsize
                got[name] = np.frombuffer(raw[at: at + size], dtype=kind).reshape(shape)
                at += size
            res.append(got)
        assert at == len(raw)
        return res

    return run


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    a = np.where(np.isnan(a), np.array(np.nan, a.dtype), a)  # one NaN is as good as another
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def odd_values(q, rng, sub=None):
    """ties, infinities, NaNs, -0.0 and the lowest finite value sprinkled over the rows of q (in place); where `sub`
    (the subsets as 0/1 rows) is given, rows 0..3 get them outside and rows 4..7 inside the subset"""
    dt = q.dtype.type
    count, width = q.shape
    q[:] = np.round(q, 1)  # ties
    odd = [dt(np.nan), dt(np.inf), dt(-np.inf), dt(-0.0), np.finfo(q.dtype).min, dt(0.0)]
    for g in range(8, count):
        if g % 3 == 0:
            q[g, rng.integers(0, width, 2)] = [odd[g % len(odd)], odd[(g // 3) % len(odd)]]
    if sub is not None:
        for g in range(min(8, count)):
            inside = np.flatnonzero(sub[g] == (g >= 4))
            if len(inside):
                q[g, inside[0]] = odd[g % 3]  # NaN, +inf, -inf
    if count >= 2:
        q[count - 1] = dt(np.nan)
        q[count - 2] = dt(-0.0)
        q[count - 2, width - 1] = dt(0.0)
    return q


def games(rng, m, d, dtype, count=48):
    """states over small integers with holes, a third of them rescaled; games 0..3 finished (0, 1: one point; 2, 3:
    none), 4..7 with duplicate rows, 8..11 with equal first coordinates"""
    p = rng.integers(0, 6, (count, m, d)).astype(dtype)
    p[rng.random((count, m)) < 0.3] = -1
    p[:4, 1:] = -1
    p[:2, 0] = [1] + [0] * (d - 1)
    p[2:4, 0] = -1
    if m > 1:
        p[4:8, 1] = p[4:8, 0]
        p[8:12, :, 0] = np.where(p[8:12, :, 0] >= 0, dtype(2), dtype(-1))
    third = slice(12, count, 3)
    mx = np.maximum(p[third].max(axis=(1, 2), keepdims=True), dtype(1))
    p[third] = np.where(p[third] >= 0, p[third] / mx, dtype(-1))
    return p


def block(rng, m, d, dtype, qdtype, masked, rescale):
    points = games(rng, m, d, dtype)
    count, classes = len(points), R.num_classes(d)
    cls = rng.integers(-1, classes + 1, count)
    sub = R.O.decode_class(R.clamp_class(cls, d), d)
    q = odd_values(rng.normal(size=(count, d)).astype(qdtype), rng, sub)
    host_q = odd_values(rng.normal(size=(count, classes)).astype(qdtype), rng)
    return (m, d, masked, rescale, points, q, cls, host_q)


def assert_block(got, blk, what):
    m, d, masked, rescale, points, q, cls, host_q = blk
    new, axis, feats, done, prev_done = R.agent_move(points, q, cls, masked=masked, rescale=rescale)
    want = dict(points=new, features=feats, axis=axis, done=done.astype(np.int32), prev_done=prev_done.astype(np.int32),
                host_class=R.host_pick(host_q, d)[0])
    for name, w in want.items():
        bad = np.argwhere(bits(got[name]) != bits(w))
        assert len(bad) == 0, "%s %s: %d differ, the first at %s: got %r, want %r" % (
            what, name, len(bad), bad[0].tolist(), got[name][tuple(bad[0])], w[tuple(bad[0])])
    return want


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_lane_body_matches_the_rules(program, dtype):
    """every shape x both Q dtypes x masked on / off x rescale on / off, with finished and one-point games, duplicate
    rows, equal first coordinates, class ids beyond both ends, and NaN / inf / -0.0 / lowest Q-values inside and
    outside the subset; unmasked, the axis falls outside the subset in some games and the shift is skipped"""
    rng = np.random.default_rng(11)
    blocks, what = [], []
    for (m, d), qdtype, masked, rescale in itertools.product(SHAPES, DTYPES, (True, False), (True, False)):
        blocks.append(block(rng, m, d, dtype, qdtype, masked, rescale))
        what.append("(%d,%d) q=%s masked=%d rescale=%d" % (m, d, np.dtype(qdtype).name, masked, rescale))
    outside = moved = ended = 0
    for got, blk, name in zip(program(blocks), blocks, what):
        want = assert_block(got, blk, name)
        m, d, masked, _, points, _, cls, _ = blk
        sub = R.O.decode_class(R.clamp_class(cls, d), d)
        legal = sub[np.arange(len(cls)), want["axis"]] == 1
        assert legal.all() or not masked or np.isnan(blk[5]).any() or np.isinf(blk[5]).any(), name
        outside += int((~legal & (want["prev_done"] == 0)).sum())
        moved += int((bits(want["points"]) != bits(points)).any((1, 2)).sum())
        ended += int(((want["done"] == 1) & (want["prev_done"] == 0)).sum())
    assert outside > 50 and moved > 500 and ended > 20, (outside, moved, ended)
