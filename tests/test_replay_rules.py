"""tests/replay_rules.py against the fixture made by running the reference's own ReplayBuffer
(tests/golden/replay_buffer.npz): every add of the sequence move for move, and a push with `keep` against compacting
first and adding then."""
import os

import numpy as np
import pytest

import replay_rules as RR
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "replay_buffer.npz"))


@pytest.mark.parametrize("tag", ["tuple", "dict"])
def test_push_follows_the_reference_add_for_add(fixture, tag):
    lengths = fixture[f"{tag}_lengths"]
    assert list(lengths) == [4, 0, 6, 7, 3, 9, 5, 10]
    assert list(fixture[f"{tag}_pos"]) == [4, 4, 0, 7, 0, 9, 4, 4]  # an exact fill, a wrap inside an add
    rings, cursor = RR.new_rings(tag, 10), RR.new_cursor()
    total = 0
    for a, n in enumerate(lengths):
        rows = [fixture[f"{tag}_a{a}_in_{c}"] for c in RR.COLUMNS[tag]]
        assert rows[0].shape[0] == n
        if fixture[f"{tag}_asserts"][a]:
            with pytest.raises(AssertionError):
                RR.push(rings, rows, cursor)
        else:
            RR.push(rings, rows, cursor)
            total += n
            if n:
                assert cursor[RR.LAST_COUNT] == n
        for c, ring in zip(RR.COLUMNS[tag], rings):
            want = fixture[f"{tag}_a{a}_buf_{c}"]
            assert ring.dtype == want.dtype and ring.shape == want.shape, (a, c)
            assert ring.tobytes() == want.tobytes(), (a, c)
        assert cursor[RR.POS] == fixture[f"{tag}_pos"][a] and cursor[RR.FULL] == fixture[f"{tag}_full"][a], a
        assert cursor[RR.TOTAL_PUSHED] == total
    assert fixture[f"{tag}_asserts"].sum() == 1


@pytest.mark.parametrize("pattern", ["all", "none", "one", "alternating", "random"])
def test_push_with_keep_is_compact_then_add(pattern):
    rng = np.random.default_rng(5)
    cap, batch = 23, 9
    rings_a, cur_a = RR.new_rings("dict", cap), RR.new_cursor()
    rings_b, cur_b = RR.new_rings("dict", cap), RR.new_cursor()
    for move in range(6):
        rows = [rng.integers(0, 2 if r.dtype == np.bool_ else 9, (batch, *r.shape[1:])).astype(r.dtype)
                for r in rings_a]
        keep = {"all": np.ones(batch), "none": np.zeros(batch), "one": np.arange(batch) == move,
                "alternating": np.arange(batch) % 2, "random": rng.integers(0, 2, batch)}[pattern].astype(np.uint8)
        RR.push(rings_a, rows, cur_a, keep=keep * 255 if move % 2 else keep)  # any nonzero byte keeps
        n = RR.add(rings_b, [r[keep != 0] for r in rows], cur_b)
        assert cur_a[RR.LAST_COUNT] == n == keep.sum()
        for x, y in zip(rings_a, rings_b):
            assert x.tobytes() == y.tobytes()
        assert cur_a[RR.POS] == cur_b[RR.POS] and cur_a[RR.FULL] == cur_b[RR.FULL]


def test_sample_indices():
    cur = RR.new_cursor()
    assert (RR.sample_indices(cur, 50, 7, seed=3) == -1).all() and cur[RR.SAMPLES_DRAWN] == 1
    cur[RR.POS] = 13
    a = RR.sample_indices(cur, 50, 4096, seed=3)
    b = RR.sample_indices(cur, 50, 4096, seed=3)
    assert a.min() == 0 and a.max() == 12 and cur[RR.SAMPLES_DRAWN] == 3 and (a != b).any()
    cur2 = RR.new_cursor()
    cur2[RR.POS], cur2[RR.SAMPLES_DRAWN] = 13, 1
    assert (RR.sample_indices(cur2, 50, 4096, seed=3) == a).all()  # keyed by the draw number, not by history
    assert (RR.sample_indices(cur2, 50, 100, seed=3) == b[:100]).all()  # index j does not depend on batch_size
    cur[RR.FULL] = 1
    c = RR.sample_indices(cur, 50, 4096, seed=4)
    assert c.max() == 49 and np.bincount(c, minlength=50).min() > 40  # uniform over the whole ring: 82 expected
