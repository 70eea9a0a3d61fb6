"""
Generate tests/golden/replay_buffer.npz by RUNNING the reference's own ReplayBuffer (hironaka/trainer/replay_buffer.py,
which imports only torch and is loaded as a file, as make_golden.py loads the rest).  Runs only where the reference
checkout exists; the resulting .npz is what travels, and it holds data only.

Two buffers of buffer_size 10 on the CPU, dtype float32: the tuple shape (4, 3) and the dict shape
{"points": (4, 3), "coords": (3,)}.  Each is fed the add sequence 4, 0, 6, 7, 3, 9, 5 and then 10 rows.  `pos` after
the adds: 4, 4 (an empty add), 0 (an exact fill to the end: `full` turns True), 7, 0 (exactly to the end again), 9
(buffer_size - 1 rows at once), 4 (a wrap in the middle of an add); the add of 10 rows trips the reference's
assertion, which is recorded as `asserts`, and leaves the buffer as it was.  The inputs come in other types than the
buffer's (float64 observations and rewards, int64 actions, uint8 dones), so the forced types are part of what is
recorded; the values are quarters of small integers, exact in every float type.

Layout, per tag in ("tuple", "dict"), add number a and column c in COLUMNS[tag] (tests/replay_rules.py names them):
    {tag}_lengths        [A] int64   the rows of every add, the refused one last
    {tag}_asserts        [A] uint8   1 where the reference's add raised AssertionError
    {tag}_a{a}_in_{c}    the add's input, as given
    {tag}_a{a}_buf_{c}   the buffer's storage after the add, as the reference holds it (dtype included)
    {tag}_pos, {tag}_full [A] int64 / uint8 after every add

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_replay_golden.py
"""
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from make_golden import OUT, REF, _load  # noqa: E402
from replay_rules import COLUMNS, SHAPES  # noqa: E402

BUFFER_SIZE = 10
LENGTHS = [4, 0, 6, 7, 3, 9, 5, 10]


def _storage(buf, tag):
    """the reference's storage as {column: tensor}"""
    out = {}
    for side, value in (("obs", buf.observations), ("next", buf.next_observations)):
        if isinstance(value, dict):
            for key, t in value.items():
                out[f"{side}_{key}"] = t
        else:
            out[side] = value
    out["action"], out["reward"], out["done"] = buf.actions, buf.rewards, buf.dones
    assert sorted(out) == sorted(COLUMNS[tag])
    return out


def _inputs(rng, tag, n):
    shape = SHAPES[tag]
    quarter = lambda *s: rng.integers(0, 50, s).astype(np.float64) / 4  # noqa: E731
    rec = {}
    for side in ("obs", "next"):
        if isinstance(shape, dict):
            for key, s in shape.items():
                rec[f"{side}_{key}"] = quarter(n, *s)
        else:
            rec[side] = quarter(n, *shape)
    rec["action"] = rng.integers(0, 3, (n, 1)).astype(np.int64)
    rec["reward"] = quarter(n, 1) - 3.0
    rec["done"] = rng.integers(0, 2, (n, 1)).astype(np.uint8)
    return rec


def _as_args(rec, tag):
    t = {c: torch.from_numpy(v.copy()) for c, v in rec.items()}
    if isinstance(SHAPES[tag], dict):
        obs = {key: t[f"obs_{key}"] for key in SHAPES[tag]}
        nxt = {key: t[f"next_{key}"] for key in SHAPES[tag]}
    else:
        obs, nxt = t["obs"], t["next"]
    return obs, t["action"], t["reward"], t["done"], nxt


def main():
    if not os.path.isdir(REF):
        raise SystemExit(f"{REF} not present: fixtures can only be regenerated next to the reference")
    ref = _load("hironaka_ref_replay_buffer", "hironaka/trainer/replay_buffer.py")
    rng = np.random.default_rng(20260)
    rec = {}
    for tag in ("tuple", "dict"):
        buf = ref.ReplayBuffer(SHAPES[tag], 3, BUFFER_SIZE, torch.device("cpu"), dtype=torch.float32)
        pos, full, asserts = [], [], []
        for a, n in enumerate(LENGTHS):
            given = _inputs(rng, tag, n)
            for c, v in given.items():
                rec[f"{tag}_a{a}_in_{c}"] = v
            try:
                buf.add(*_as_args(given, tag))
                asserts.append(0)
            except AssertionError:
                asserts.append(1)
            for c, t in _storage(buf, tag).items():
                rec[f"{tag}_a{a}_buf_{c}"] = t.numpy().copy()
            pos.append(int(buf.pos))
            full.append(int(buf.full))
        rec[f"{tag}_lengths"] = np.array(LENGTHS, dtype=np.int64)
        rec[f"{tag}_asserts"] = np.array(asserts, dtype=np.uint8)
        rec[f"{tag}_pos"] = np.array(pos, dtype=np.int64)
        rec[f"{tag}_full"] = np.array(full, dtype=np.uint8)
        # the sequence passes through what it is meant to
        assert pos == [4, 4, 0, 7, 0, 9, 4, 4] and full == [0, 0, 1, 1, 1, 1, 1, 1], (pos, full)
        assert asserts == [0] * 7 + [1]
    path = os.path.join(OUT, "replay_buffer.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {len(rec)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
