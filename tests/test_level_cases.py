"""The inputs of tests/test_gpu_levels.py reach every level of every staircase -- shown on the C oracle alone.

For every (family, shape, configuration) the GPU file runs, the oracle plays its cases with the observations recorded;
`level_cases.level_path` maps the live rows of every wave and step to the ladder, and the union over the cases must hold
every level as a stepped level and as a publish level, every adjacent re-deal, and a re-deal that skips a level.  There
is no list of exemptions: whatever is not reached is named in the failure."""
import numpy as np
import pytest

import level_cases as LC
from test_gpu_step_loops import CONFIGS

CASES = [(f, s) for f in ("four", "two", "one") for s in LC.ROLLOUT_SHAPES[f]]


def test_ladders():
    assert LC.ladder("four", 50) == [1, 2, 3, 4, 5, 6, 8, 10, 13]
    assert LC.ladder("four", 20) == [1, 2, 3, 4, 5] and LC.ladder("four", 10) == [1, 2, 3]
    assert LC.ladder("two", 20) == [1, 2, 3, 4, 5, 6, 8, 10] and LC.ladder("two", 16) == [1, 2, 3, 4, 5, 6, 8]
    assert LC.ladder("two", 5) == [1, 2, 3] and LC.ladder("two", 8) == [1, 2, 3, 4]
    assert LC.ladder("one", 20) == [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20]
    assert LC.ladder("one", 4) == [1, 2, 3, 4] and LC.ladder("one", 10) == [1, 2, 3, 4, 5, 6, 7, 8, 10]
    assert [LC.level_of("four", 50, n) for n in (0, 1, 4, 5, 24, 25, 32, 33, 40, 41, 50)] == \
        [1, 1, 1, 2, 6, 8, 8, 10, 10, 13, 13]
    assert [LC.level_of("two", 20, n) for n in (0, 2, 3, 12, 13, 16, 17, 20)] == [1, 1, 2, 6, 8, 8, 10, 10]
    assert [LC.level_of("one", 20, n) for n in (0, 1, 8, 9, 10, 19, 20)] == [1, 1, 8, 10, 10, 20, 20]


def test_level_path_on_hand_written_widths():
    """three width sequences by hand: (widest of the wave's 16 games) per state, four lanes at (50,4)"""
    def widths(seq):  # one wave: game 0 carries the width, the others one row
        n = np.ones((len(seq), 16), dtype=np.int32)
        n[:, 0] = seq
        return n
    # 50 rows, 38 after step 0, 37 after step 1 (10 slots both: no re-deal), 20 after step 2; the drop to 3 rows after the
    # last step is never re-dealt, and the image is built on the last step's level
    (p,) = LC.level_path(widths([50, 38, 37, 20, 3]), "four", 50, 4)
    assert p == dict(entered=13, steps=[13, 10, 10, 5], redeals=[(13, 10), (10, 5)], publish=5)
    # 48 rows to 45: 12 slots on the 13-slot level, a re-deal inside the bucket; T = 1: no re-deal at all
    (p,) = LC.level_path(widths([50, 45, 45]), "four", 50, 2)
    assert p == dict(entered=13, steps=[13, 13], redeals=[(13, 13)], publish=13)
    (p,) = LC.level_path(widths([36, 2]), "four", 50, 1)
    assert p == dict(entered=10, steps=[10], redeals=[], publish=10)
    # the one-slot level: no re-deal; with `still`, the wave leaves once every game is at its fixed point; T = 0
    n = widths([5, 4, 1, 1, 1, 1])
    still = np.zeros(n.shape, dtype=bool)
    still[3:] = True
    (p,) = LC.level_path(n, "four", 50, 5)
    assert p == dict(entered=2, steps=[2, 1, 1, 1, 1], redeals=[(2, 1)], publish=1)
    (p,) = LC.level_path(n, "four", 50, 5, still)
    assert p == dict(entered=2, steps=[2, 1, 1], redeals=[(2, 1)], publish=1)
    (p,) = LC.level_path(widths([50]), "four", 50, 0)
    assert p == dict(entered=None, steps=[], redeals=[], publish=None)
    # two waves of the one-lane family (64 games each), two lanes on the same counts (32 games: four waves)
    n = np.zeros((3, 128), dtype=np.int32)
    n[:, 5], n[:, 100] = [20, 18, 9], [9, 9, 2]
    a, b = LC.level_path(n, "one", 20, 2)
    assert a == dict(entered=20, steps=[20, 18], redeals=[(20, 18)], publish=18)
    assert b == dict(entered=10, steps=[10, 10], redeals=[], publish=10)
    assert [p["steps"] for p in LC.level_path(n, "two", 20, 2)] == [[10, 10], [1, 1], [1, 1], [5, 5]]


def test_placed_width_states():
    for family, (m, d), S in (("four", (50, 4), 40), ("four", (50, 4), 500), ("two", (20, 3), 12), ("one", (5, 3), 12)):
        games = LC.FAMILIES[family][1]
        p = LC.batch(m, d, family, S, 5)
        assert p.shape == ((2 * m + 4) * games, m, d) and p.dtype == np.float32
        widest = LC.widest_per_wave(p, family)
        assert widest[:m] == list(range(m, 0, -1)) and widest[m:2 * m] == list(range(m, 0, -1)) and widest[2 * m:] == [2] * 4
        live = (p >= 0).all(axis=-1)
        assert ((p == -1.0).all(axis=-1) | live).all()
        assert (p.sum(axis=-1)[live] == S).all()  # on the hyperplane: an antichain
        for g in p[::7]:
            rows = g[(g >= 0).all(axis=-1)]
            assert len({tuple(r) for r in rows}) == len(rows)
        # every bucket of the ladder is some wave's entry level
        assert {LC.level_of(family, m, n) for n in widest} == set(LC.ladder(family, m))


@pytest.mark.parametrize("cfg", LC.CONFIG_NAMES)
@pytest.mark.parametrize("family,shape", CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_rollout_cases_walk_every_level(family, shape, cfg):
    paths, by_sum = LC.family_paths(family, shape, cfg, CONFIGS[cfg])
    miss = LC.missing(LC.coverage(paths), family, shape[0])
    if family == "four" and shape == (50, 4):
        miss += LC.missing_at_50_4(paths, by_sum)
    assert not miss, f"{family} lanes {shape} {cfg}: not reached: {', '.join(miss)}"
