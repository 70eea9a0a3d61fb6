"""spivakovsky_game and random_spivakovsky_game (hk_spivakovsky.h) run on the CPU: tests/spivakovsky_routines.hip is a
stand-alone program over the header, built once at -O3 and once under AddressSanitizer + UndefinedBehaviorSanitizer.
Every game runs in allocations of exactly m * d elements, so the sanitized build reports any access outside the game.
The masks of both builds must equal those of tests/spivakovsky_rules.py bit for bit, in both dtypes; for float32 the
rules run on the rounded values.  No GPU is involved: what this cannot show is the device compiler's code for the same
source.

The 3-row states are those whose rows are a hole or a point of {0, 1, 2}^d: every input stays inside the operator's
contract (finite, non-negative points)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from spivakovsky_rules import (random_spivakovsky_candidates, random_words, rule_spivakovsky, three_row_states)
from test_lane_routines import COMMON, HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "spivakovsky_routines.hip")
BUILDS = {"sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
          "optimised": ["-O3"]}
DTYPES = (np.float32, np.float64)
SHAPES = [(m, d) for m in (1, 2, 5, 20, 33, 64) for d in range(2, 7)]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """both builds, compiled once; returns run(blocks) -> per block (spivakovsky masks, random masks)"""
    where = tmp_path_factory.mktemp("spivakovsky_routines")
    exes = {name: str(where / name) for name in BUILDS}
    jobs = [subprocess.Popen([HIPCC] + COMMON + flags + [SOURCE, "-o", exes[name]], stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True) for name, flags in BUILDS.items()]
    for job in jobs:
        log = job.communicate()[0]
        assert job.returncode == 0, log

    def run(blocks):
        """blocks: (games [count, m, d] of a dtype, seed, game_offset, step)"""
        stem = str(where / "cases")
        with open(stem + ".in", "wb") as f:
            f.write(b"HKSP" + struct.pack("<2i", 1, len(blocks)))
            for games, seed, game_offset, step in blocks:
                count, m, d = games.shape
                f.write(struct.pack("<4i2Q2I", DTYPES.index(games.dtype.type), m, d, count, seed, game_offset, step, 0))
                f.write(np.ascontiguousarray(games).tobytes())
        results = {}
        for name, exe in exes.items():
            done = subprocess.run([exe, stem + ".in", stem + "." + name], capture_output=True, text=True, timeout=600)
            assert done.returncode == 0, "%s build: exit status %d\n%s" % (name, done.returncode, done.stderr[-4000:])
            assert not any(word in done.stderr for word in ("Sanitizer", "runtime error", "FAILED")), done.stderr[-4000:]
            raw = np.fromfile(stem + "." + name, dtype=np.int32)
            assert len(raw) == 2 * sum(len(b[0]) for b in blocks)
            got, at = [], 0
            for games, _, _, _ in blocks:
                got.append((raw[at: at + len(games)], raw[at + len(games): at + 2 * len(games)]))
                at += 2 * len(games)
            results[name] = got
        return results

    return run


def expected(games, seed, game_offset, step):
    """the rules' masks for one block, on the values the block holds"""
    words = random_words(seed, game_offset, len(games), step)
    spiv, rnd = [], []
    for st, word in zip(games.astype(np.float64), words):
        spiv.append(rule_spivakovsky(st))
        cands = random_spivakovsky_candidates(st)
        rnd.append(cands[(int(word) * len(cands)) >> 32] if cands else 0)
    return np.array(spiv, np.int32), np.array(rnd, np.int32)


def check(program, blocks, wants=None):
    results = program(blocks)
    for b, block in enumerate(blocks):
        want = expected(*block) if wants is None else wants[b]
        for name in BUILDS:
            for which, got, exp in zip(("spivakovsky", "random_spivakovsky"), results[name][b], want):
                bad = np.flatnonzero(got != exp)
                assert len(bad) == 0, "%s, %s build, block %d %s %s: %d differ, the first game %d: got %d, want %d\n%s" % (
                    which, name, b, block[0].shape, block[0].dtype, len(bad), bad[0], got[bad[0]], exp[bad[0]],
                    block[0][bad[0]])


def test_every_three_row_state(program):
    """0, 1, 2 and 3 points; zero rows, equal rows, holes in every place"""
    blocks, wants = [], []
    for d in (2, 3):
        states = three_row_states(d)
        assert len(states) == (3 ** d + 1) ** 3
        want = expected(states, 11, 5, 2)  # 0, 1 and 2 are exact in float32: one run of the rules serves both dtypes
        assert {0, 1, 2} <= {bin(v).count("1") for v in want[0].tolist()} and (want[1] == 0).any()
        for dt in DTYPES:
            blocks.append((states.astype(dt), 11, 5, 2))
            wants.append(want)
    check(program, blocks, wants)


def test_seeded_random_games(program):
    """every (m, d) of m in (1, 2, 5, 20, 33, 64) and d in 2..6: small values (ties, zeros) and large ones, holes
    anywhere, a nonzero game_offset beyond 32 bits and a nonzero step"""
    rng = np.random.default_rng(20261021)
    blocks = []
    for m, d in SHAPES:
        games = np.where(rng.random((24, 1, 1)) < 0.5, rng.integers(0, 4, (24, m, d)), rng.integers(0, 21, (24, m, d)))
        games = games.astype(np.float64)
        games[rng.random((24, m)) < 0.25] = -1.0
        for dt in DTYPES:
            blocks.append((games.astype(dt), 0x1234567890ABCDEF, (1 << 32) + 7, 3))
    check(program, blocks)


def test_rescaled_fixture_states(program):
    """doubles in [0, 1] that float32 rounds: the float32 run is held against the rules on the rounded values"""
    fx = np.load(os.path.join(GOLDEN, "spivakovsky.npz"))
    blocks = []
    for d in range(2, 7):
        states = fx[f"sel{d}_states"][fx[f"sel{d}_kind"] == 2]
        assert len(states) >= 50 and (states.astype(np.float32) != states).any()
        for dt in DTYPES:
            blocks.append((states.astype(dt), 3, 0, 0))
    check(program, blocks)
    # the float64 run is the reference's own answer
    results = program([b for b in blocks if b[0].dtype == np.float64])
    for d, (got, _) in zip(range(2, 7), results["optimised"]):
        masks = fx[f"sel{d}_spivakovsky"][fx[f"sel{d}_kind"] == 2]
        assert got.tolist() == [sum(1 << k for k in np.nonzero(mk)[0].tolist()) for mk in masks], d
