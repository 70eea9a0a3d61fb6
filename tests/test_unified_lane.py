"""The lane body of hk_unified_expand run on the CPU: tests/unified_lane.hip builds hk_unified_kernel.h's unified_lane
and unified_host_state for the host under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program with its
own main: nothing is loaded into Python under a sanitizer).  Every game runs in two memory layouts and under four fills
of whatever is not an input; the program itself fails on a fill-dependent result or a touched canary, the sanitizers on
an overrun.  Here its results are compared with tests/unified_rules.py as bit patterns, without tolerances.  No GPU is
involved: what this cannot show is the device compiler's code for the same source."""
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

import unified_rules as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hironaka_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "unified_lane.hip")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-host-only", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
         "-I", CSRC, "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
F = np.float32


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/unified_lane.hip, compiled once; returns run(blocks) -> the results per block, where a block is
    (m, d, kind, reposition, scale, states [count, m*d + d], actions [count])"""
    where = tmp_path_factory.mktemp("unified_lane")
    exe = str(where / "unified_lane")
    done = subprocess.run([HIPCC] + FLAGS + [SOURCE, "-o", exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    serial = itertools.count()

    def run(blocks):
        stem = str(where / ("cases%d" % next(serial)))
        with open(stem + ".in", "wb") as f:
            f.write(b"HKUL" + struct.pack("<2i", 1, len(blocks)))
            for m, d, kind, repos, scale, states, actions in blocks:
                f.write(struct.pack("<6i", m, d, kind, int(repos), int(scale), len(states)))
                f.write(np.ascontiguousarray(states, F).tobytes() + np.ascontiguousarray(actions, np.int32).tobytes())
        done = subprocess.run([exe, stem + ".in", stem + ".out"], capture_output=True, text=True, timeout=600)
        if done.returncode != 0:
            print(done.stderr[-8000:])
        assert done.returncode == 0, "exit status %d\n%s" % (done.returncode, done.stderr[-4000:])
        assert not any(word in done.stderr for word in ("Sanitizer", "runtime error", "FAILED")), done.stderr[-4000:]
        raw, at, res = open(stem + ".out", "rb").read(), 0, []
        for m, d, _, _, _, states, _ in blocks:
            count, width, got = len(states), m * d + d, {}
            for name, kind, cols in (("next_state", F, width), ("net_in", F, width), ("subset", np.int32, 1),
                                     ("reward", F, 1), ("host_state", np.int32, 1)):
                size = count * cols * 4
                got[name] = np.frombuffer(raw[at: at + size], dtype=kind).reshape((count, cols) if cols > 1 else (count,))
                at += size
            res.append(got)
        assert at == len(raw)
        return res

    return run


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    return np.where(np.isnan(a), np.array(np.nan, a.dtype), a).view(np.uint32)  # one NaN is as good as another


def assert_block(got, states, actions, m, d, repos, scale, what):
    want = U.expand(states, actions, m, d, reposition_points=repos, scale_observation=scale)
    for name in ("next_state", "net_in", "subset", "reward"):
        bad = np.argwhere(bits(got[name]) != bits(want[name]))
        assert len(bad) == 0, "%s %s: %d differ, the first at %s: got %r, want %r" % (
            what, name, len(bad), bad[0].tolist(), got[name][tuple(bad[0])], want[name][tuple(bad[0])])
    assert (got["host_state"].astype(bool) == U.is_host_state(np.asarray(states, F), d)).all(), what
    return want


def small_states(d):
    rows = np.array([[-1] * d] + list(itertools.product(range(3), repeat=d)), F)
    return rows[np.array(list(itertools.product(range(len(rows)), repeat=3)))]


def with_tail(points, tail):
    return np.concatenate([points.reshape(len(points), -1), np.asarray(tail, F)], 1)


@pytest.mark.parametrize("d", (2, 3))
def test_lane_body_on_the_small_states_of_the_rules(program, d):
    """the 3-row states over {hole, 0..2}^d (all of them at d = 2, every 7th at d = 3) with every subset as the tail and
    every axis, -1 and d + 1 included, as an agent-kind batch; with every class id, out-of-range ones included, as a
    host-kind batch"""
    states = small_states(d)[:: 1 if d == 2 else 7]
    masks, ncls, m = U.masks_of(d), U.num_actions(d), 3
    s, c, a = np.meshgrid(np.arange(len(states)), np.arange(len(masks)), np.arange(-1, d + 2), indexing="ij")
    agent = (with_tail(states[s.ravel()], U.bits_of(masks[c.ravel()], d)), a.ravel())
    s, c = np.meshgrid(np.arange(len(states)), np.arange(-2, ncls + 2), indexing="ij")
    host = (with_tail(states[s.ravel()], np.zeros((s.size, d), F)), c.ravel())
    assert U.batch_kind(agent[0], d) == 0 and U.batch_kind(host[0], d) == 1
    blocks, what = [], []
    for repos, scale in itertools.product((False, True), repeat=2):
        blocks += [(m, d, 0, repos, scale) + agent, (m, d, 1, repos, scale) + host]
        what += ["agent kind repos=%d scale=%d" % (repos, scale), "host kind repos=%d scale=%d" % (repos, scale)]
    ended = 0
    for got, blk, name in zip(program(blocks), blocks, what):
        want = assert_block(got, blk[5], blk[6], m, d, blk[3], blk[4], "d=%d %s" % (d, name))
        ended += int((want["reward"] == -1).sum())
    assert ended > 100  # games that end on the move were among them


def test_lane_body_on_wider_games_odd_tails_and_mixed_batches(program):
    """specs up to (20, 4) and (7, 5); tails at exactly 1e-8 and 2e-8, -0.0 and NaN; a host state among agent states
    makes the batch a host batch for every game; ended games"""
    rng = np.random.default_rng(3)
    eps = F(1e-8)
    blocks, what = [], []
    for m, d in ((5, 2), (10, 3), (20, 4), (7, 5)):
        count = 96
        p = rng.integers(0, 6, (count, m, d)).astype(F)
        p[rng.random((count, m)) < 0.3] = -1
        p[:4, 1:] = -1  # ended games: at most one point
        p[:2, 0] = 1
        masks = U.masks_of(d)
        tail = U.bits_of(masks[rng.integers(0, len(masks), count)], d)
        action = rng.integers(-2, U.num_actions(d) + 2, count)
        odd = tail.copy()
        odd[0::4, 0], odd[1::4, 0], odd[2::4, 1], odd[3::8, 1] = 2 * eps, -2 * eps, F(1), np.nan
        for name, t in (("agent", tail), ("odd tails", odd)):
            states = with_tail(p, t)
            assert U.batch_kind(states, d) == 0, name
            blocks.append((m, d, 0, True, True, states, action))
            what.append("(%d,%d) %s" % (m, d, name))
        for name, row in (("eps", [eps, -eps] + [0] * (d - 2)), ("minus zero", [-0.0] * d), ("zero", [0.0] * d)):
            t = tail.copy()
            t[count // 2] = row
            states = with_tail(p, t)
            assert U.batch_kind(states, d) == 1 and U.is_host_state(states, d).sum() == 1, name
            blocks.append((m, d, 1, False, True, states, action))
            what.append("(%d,%d) one host state: %s" % (m, d, name))
    for got, blk, name in zip(program(blocks), blocks, what):
        assert_block(got, blk[5], blk[6], blk[0], blk[1], blk[3], blk[4], name)
