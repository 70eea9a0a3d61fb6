"""hk_unified_expand and hk_unified_prior (include/hironaka_hip_unified.h) against tests/unified_rules.py, bit for bit:
every spec the lane frame meets a different way, batches around a wave, all-host, all-agent and mixed batches with the
single host state in the first lane, in the last lane of a full wave and in the partial last wave, tails at the edge of
isclose, actions out of range, ended games, parents and nodes at both ends of the table, and a sentinel-filled table that
shows that only row node[b] is written.  The statuses are checked on the host, before any launch, in the manner of
tests/test_pvnet_abi.py (those tests need no GPU and carry no mark)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_cases
import unified_rules as U
from conftest import ROOT
from hironaka_amd import _abi as A
from hironaka_amd import _lib

F = np.float32
SPECS = [(5, 2), (10, 3), (20, 3), (20, 4), (7, 5)]
BATCHES = [1, 63, 64, 65, 130]
NODES = 5
SENTINEL = F(-12345.5)
EPS = F(1e-8)


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    return np.where(np.isnan(a), np.array(np.nan, a.dtype), a).view(np.uint32)  # one NaN is as good as another


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, "%s: %d differ, the first at %s: got %r, want %r" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def games(rng, b, m, d):
    """games with holes, duplicate rows and, in the first lanes, ended games (one point, none)"""
    p = rng.integers(0, 6, (b, m, d)).astype(F)
    p[rng.random((b, m)) < 0.3] = -1
    p[: min(b, 3), 1:] = -1
    p[:1, 0] = 2
    if b > 4:
        p[4, 1] = p[4, 0]
    return p


def batch_of(kind, b, m, d, seed):
    """(parent states [b, m*d + d], actions [b]) of one named kind of batch"""
    rng = np.random.default_rng(seed)
    p = games(rng, b, m, d)
    masks, ncls = U.masks_of(d), U.num_actions(d)
    tail = U.bits_of(masks[rng.integers(0, len(masks), b)], d)
    action = rng.integers(0, ncls, b)
    if kind == "all-host":
        tail[:] = 0
        tail[0::3, 0], tail[1::3, d - 1], tail[2::5, 0] = EPS, -EPS, -0.0  # still close to zero
        action[0::7], action[3::7] = -1 - (np.arange(len(action[0::7])) % 2), ncls + (np.arange(len(action[3::7])) % 3)
    elif kind == "all-agent":
        action = rng.integers(0, d, b)
        action[0::7], action[3::7] = -1, d + (np.arange(len(action[3::7])) % 2)  # axes that match nothing
        outside = np.array([int(np.argmin(t)) for t in tail])  # an axis outside the subset, where the subset is not all
        action[5::7] = outside[5::7]
    elif kind == "odd-tails":  # no host state: 2e-8 is not close, neither is NaN, and 1e-8 next to a 1 is no zero tail
        action = rng.integers(-1, d + 1, b)
        tail[0::4, 0], tail[1::4, 0], tail[3::8, 1] = 2 * EPS, EPS, np.nan
        tail[2::4, d - 1] = F(1)
        tail[1::4, 1] = F(1)
    else:  # one host state among agent states
        at = {"first-lane": 0, "last-lane-of-a-full-wave": 63, "partial-last-wave": b - 1}[kind]
        tail[at] = [EPS, -0.0] + [0] * (d - 2)
        action = rng.integers(-1, ncls + 1, b)
    return np.concatenate([p.reshape(b, -1), tail], 1), action


def kinds_for(b):
    return ["all-host", "all-agent", "odd-tails", "first-lane"] + (["last-lane-of-a-full-wave"] if b >= 64 else []) + (
        ["partial-last-wave"] if b % 64 != 0 and b > 1 else [])


def table_of(parents, parent, w):
    """a sentinel-filled [b, NODES, w] table with the parent states at their nodes"""
    b = len(parents)
    table = np.full((b, NODES, w), SENTINEL, F)
    table[np.arange(b), parent] = parents
    return table


@pytest.mark.gpu
@pytest.mark.parametrize("spec", SPECS, ids=lambda s: "%dx%d" % s)
def test_expand_and_prior_against_the_rules(spec):
    from hironaka_amd import ops
    m, d = spec
    w, a = m * d + d, U.num_actions(d)
    dev = torch.device("cuda")
    seen = set()
    for b in BATCHES:
        for k, kind in enumerate(kinds_for(b)):
            for repos, scale in ((False, True), (True, True), (True, False))[k % 3: k % 3 + 1] if b != 65 else (
                    (False, True), (True, True), (True, False)):
                rng = np.random.default_rng(1000 * b + k)
                parents, action = batch_of(kind, b, m, d, seed=b * 31 + k)
                parent = rng.integers(0, NODES, b)
                node = (parent + rng.integers(1, NODES, b)) % NODES  # another node of the game
                parent[: min(b, 2)], node[: min(b, 2)] = (0, NODES - 1)[: min(b, 2)], (NODES - 1, 0)[: min(b, 2)]
                table = table_of(parents, parent, w)
                want = U.expand(parents, action, m, d, reposition_points=repos, scale_observation=scale, discount=0.97)
                assert want["kind"] == (0 if kind in ("all-agent", "odd-tails") else 1), kind
                seen.add((kind, want["kind"], bool(U.is_host_state(parents, d).all())))
                emb = torch.from_numpy(table).to(dev)
                kind_word = torch.zeros(3, dtype=torch.int32, device=dev)
                i32 = lambda x: torch.from_numpy(np.asarray(x, np.int32)).to(dev)  # noqa: E731
                got = ops.unified_expand(emb, i32(parent), i32(action), i32(node), kind_word[1:2], spec=spec,
                                         discount=0.97, scale_observation=scale, reposition=repos)
                what = "%s b=%d repos=%d scale=%d" % (kind, b, repos, scale)
                assert kind_word.tolist() == [0, want["kind"], 0], what
                after = table.copy()
                after[np.arange(b), node] = want["next_state"]
                assert_bits(emb.cpu().numpy(), after, what + ": the table (only row node[b] is written)")
                assert_bits(got["net_in"].cpu().numpy(), want["net_in"], what + ": net_in")
                assert_bits(got["subset"].cpu().numpy(), want["subset"], what + ": subset")
                assert_bits(got["reward"].cpu().numpy(), want["reward"], what + ": reward")
                assert_bits(got["discount"].cpu().numpy(), want["discount"], what + ": discount")
                # the prior of the node: sentinel-filled outputs, every element written once, either side selected
                al, av = rng.standard_normal((b, d)).astype(F), rng.standard_normal(b).astype(F)
                hl, hv = rng.standard_normal((b, a)).astype(F), rng.standard_normal(b).astype(F)
                t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
                prior = torch.full((b, a), float(SENTINEL), device=dev)
                value = torch.full((b,), float(SENTINEL), device=dev)
                ops.unified_prior(kind_word[1:2], t(al), t(av), t(hl), t(hv), got["subset"], dim=d, prior=prior, value=value)
                want_prior, want_value = U.prior(want["kind"], al, av, hl, hv, want["subset"], d)
                assert_bits(prior.cpu().numpy(), want_prior, what + ": prior")
                assert_bits(value.cpu().numpy(), want_value, what + ": value")
    # reached, by the rules alone: host batches of host states only, agent batches, host batches with agent states in them
    assert {(k, h) for _, k, h in seen} == {(1, True), (0, False), (1, False)}, seen


def test_games_that_end_and_ended_games_are_among_the_cases():
    """from the rules alone, on the batches the test above runs: a move that ends a game (reward -1), an ended parent
    (reward -0.0), an axis outside the subset that still shifts (JAX semantics do not test it)"""
    ended = moved_off = already = 0
    for m, d in SPECS:
        parents, action = batch_of("all-agent", 130, m, d, seed=130 * 31 + 1)
        want = U.expand(parents, action, m, d, reposition_points=True)
        ended += int((want["reward"] == -1).sum())
        already += int(want["prev_done"].sum())
        tail = parents[:, m * d:]
        off = (action >= 0) & (action < d) & (tail[np.arange(130), np.clip(action, 0, d - 1)] == 0)
        moved_off += int((bits(want["next_state"][off, : m * d]) != bits(parents[off, : m * d])).any(1).sum())
    assert ended > 0 and already >= 2 * len(SPECS) and moved_off > 0, (ended, already, moved_off)


# ---- the boundary: exports, constants, layouts, statuses (no GPU) ---------------------------------------------------

def test_library_exports_the_unified_entry_points():
    _lib.build()
    declared = abi_cases.declared("hironaka_hip_unified.h")
    assert declared == set(A.UNIFIED_PROTOTYPES) == {"hk_unified_expand", "hk_unified_prior", "hk_unified_pvnet_forward"}
    exported = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(re.findall(r"\bT (hk_unified_\w+)", exported)) == declared
    text = abi_cases.header()
    assert text.index('#include "hironaka_hip_pvgrad.h"') < text.index('#include "hironaka_hip_unified.h"')
    assert not re.search(r"#define\s+HK_UNIFIED_", text)  # the feature's defines live in its own header
    for name in declared:
        assert getattr(_lib.lib(), name).argtypes == A.UNIFIED_PROTOTYPES[name][1], name  # bound by default
    with open(os.path.join(ROOT, "hironaka_amd", "csrc", "Makefile")) as f:
        assert re.search(r"^SINGLES :=.*\bunified\b", f.read(), flags=re.M)
    defines = re.findall(r"#define\s+(HK_\w+)\s+(\d+)u?\s", abi_cases.header("hironaka_hip_unified.h"))
    assert len(defines) == 2
    for name, value in defines:
        assert getattr(A, name) == int(value), name


def test_unified_descriptor_layout_matches_c(tmp_path):
    abi_cases.assert_layouts_match_c({"hk_unified_expand_desc": A.hk_unified_expand_desc}, tmp_path)


_PTRS = ("embeddings", "parent", "action", "node", "kind", "net_in", "subset", "reward", "discount_out")


def _desc(batch=4, nodes=3, m=5, d=3, **change):
    """every array a region of its own of one host block (the pointers are the host's: every call returns before a
    launch); ("shift", bytes) moves a pointer, ("at", field, bytes) points it at another field's region"""
    region = 64 * 1024
    buf = (ctypes.c_char * (region * (len(_PTRS) + 1)))()
    at = (ctypes.addressof(buf) + 63) // 64 * 64
    q = A.hk_unified_expand_desc()
    for j, name in enumerate(_PTRS):
        setattr(q, name, at + j * region)
    q.batch, q.num_nodes, q.max_points, q.dim, q.dtype, q.discount = batch, nodes, m, d, A.HK_F32, 0.99
    for name, v in change.items():
        if isinstance(v, tuple) and v[0] == "shift":
            v = getattr(q, name) + v[1]
        elif isinstance(v, tuple) and v[0] == "at":
            v = getattr(q, v[1]) + v[2]
        setattr(q, name, v)
    q._keep = buf
    return q


def test_unified_expand_validation_without_gpu():
    L = _lib.lib()
    run = lambda **kw: L.hk_unified_expand(ctypes.byref(_desc(**kw)), None)  # noqa: E731
    # what is accepted is asked with batch=0 (HK_OK comes after the checks of the sizes): a batch > 0 that passes launches
    ok = lambda **kw: L.hk_unified_expand(ctypes.byref(_desc(batch=0, **kw)), None)  # noqa: E731
    assert L.hk_unified_expand(None, None) == A.HK_ERR_NULL
    assert ok() == A.HK_OK and all(ok(d=d) == A.HK_OK for d in (2, 3, 4, 5))
    assert ok(flags=A.HK_UNIFIED_REPOSITION | A.HK_UNIFIED_SCALE_OBSERVATION) == A.HK_OK
    assert run(batch=-1) == A.HK_ERR_SHAPE and run(nodes=0) == A.HK_ERR_SHAPE and run(m=0) == A.HK_ERR_SHAPE
    assert run(d=1) == A.HK_ERR_SHAPE
    assert run(d=6) == A.HK_ERR_UNSUPPORTED and ok(d=6) == A.HK_ERR_UNSUPPORTED and run(d=7) == A.HK_ERR_UNSUPPORTED
    assert run(dtype=A.HK_F64) == A.HK_ERR_UNSUPPORTED and run(flags=4) == A.HK_ERR_UNSUPPORTED
    # the slice of the lane frame: 2 m d + 2 d floats, odd, within 64 KiB
    assert ok(m=2046, d=4) == A.HK_OK and ok(m=2047, d=4) == A.HK_ERR_UNSUPPORTED
    for name in _PTRS:
        assert run(**{name: None}) == A.HK_ERR_NULL, name
        assert run(**{name: ("shift", 2)}) == A.HK_ERR_ALIGN, name
    # no written range shares a byte with another range: 4 games x 3 nodes x 18 floats = 864 bytes, a [4] array 16
    for name in ("net_in", "subset", "reward", "discount_out", "kind", "parent", "action", "node"):
        assert run(**{name: ("at", "embeddings", 860)}) == A.HK_ERR_SHAPE, name
    assert run(subset=("at", "reward", 12)) == A.HK_ERR_SHAPE and run(node=("at", "net_in", 4 * 18 * 4 - 4)) == A.HK_ERR_SHAPE
    assert run(kind=("at", "discount_out", 0)) == A.HK_ERR_SHAPE


def test_unified_prior_and_gated_forward_validation_without_gpu():
    L = _lib.lib()
    region = 4096
    buf = (ctypes.c_char * (region * 9))()
    at = (ctypes.addressof(buf) + 63) // 64 * 64
    ptrs = [at + j * region for j in range(8)]

    def run(batch=4, dim=3, **change):
        p = list(ptrs)
        for j, v in change.items():
            p[int(j[1:])] = v
        return L.hk_unified_prior(*p, batch, dim, None)
    assert run(batch=0) == A.HK_OK and run(batch=-1) == A.HK_ERR_SHAPE and run(dim=1) == A.HK_ERR_SHAPE
    assert run(dim=6) == A.HK_ERR_UNSUPPORTED
    for j in range(8):
        assert run(**{"p%d" % j: None}) == A.HK_ERR_NULL, j
        assert run(**{"p%d" % j: ptrs[j] + 2}) == A.HK_ERR_ALIGN, j
    for j in range(6):  # an output on an input
        assert run(**{"p%d" % j: ptrs[6]}) == A.HK_ERR_SHAPE and run(**{"p%d" % j: ptrs[7] + 12}) == A.HK_ERR_SHAPE, j
    assert run(p7=ptrs[6] + 4 * 4 * 4 - 4) == A.HK_ERR_SHAPE
    # the gated forward: hk_pvnet_forward's own checks first, then the gate
    import test_pvnet_abi as P
    gate = at + 8 * region
    fwd = lambda g=gate, **kw: L.hk_unified_pvnet_forward(ctypes.byref(P._desc(**kw)), g, 1, None)  # noqa: E731
    assert L.hk_unified_pvnet_forward(None, gate, 1, None) == A.HK_ERR_NULL
    assert fwd(batch=0) == A.HK_OK and fwd(batch=-1) == A.HK_ERR_SHAPE and fwd(policy=None) == A.HK_ERR_NULL
    assert fwd(widths=(18, 96)) == A.HK_ERR_UNSUPPORTED and fwd(x=("shift", 2)) == A.HK_ERR_ALIGN
    assert fwd(g=None) == A.HK_ERR_NULL and fwd(g=None, batch=0) == A.HK_ERR_NULL and fwd(g=gate + 2) == A.HK_ERR_ALIGN
