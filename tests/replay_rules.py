"""The replay buffer restated in plain numpy: hironaka/trainer/replay_buffer.py:89-127 (add) followed line by line,
with the two rules that are include/hironaka_hip_replay.h's own -- a push with a `keep` mask, which is compacting first
and adding then, and the sample's indices, Philox words keyed by the seed and the number of samples drawn.  Nothing here
comes from hironaka_amd: test_replay_rules.py pins `push` to the fixture made by running the reference's own
ReplayBuffer (tests/golden/make_replay_golden.py), and the GPU tests compare hk_replay_push / hk_replay_sample,
ReplayBuffer and FusedGame.collect with it.

A buffer is a list of columns, each an array [capacity, ...], and a cursor of 8 int64 words (POS .. TICKET below)."""
import numpy as np

POS, FULL, LAST_COUNT, TOTAL_PUSHED, SAMPLES_DRAWN, TICKET = 0, 1, 2, 3, 4, 5
CURSOR_WORDS = 8
STREAM_REPLAY = 4

# the fixture's two buffers, and their columns in the experience's order
SHAPES = {"tuple": (4, 3), "dict": {"points": (4, 3), "coords": (3,)}}
COLUMNS = {"tuple": ["obs", "action", "reward", "done", "next"],
           "dict": ["obs_points", "obs_coords", "action", "reward", "done", "next_points", "next_coords"]}
DTYPES = {"action": np.int32, "reward": np.float32, "done": np.bool_}


def new_cursor():
    return np.zeros(CURSOR_WORDS, dtype=np.int64)


def new_rings(tag, capacity, dtype=np.float32):
    """the storage of ReplayBuffer(SHAPES[tag], ., capacity, ., dtype): zeros, the forced types"""
    shape = SHAPES[tag]
    rings = []
    for c in COLUMNS[tag]:
        if c in DTYPES:
            rings.append(np.zeros((capacity, 1), dtype=DTYPES[c]))
        else:
            rows = shape[c.split("_", 1)[1]] if isinstance(shape, dict) else shape
            rings.append(np.zeros((capacity, *rows), dtype=dtype))
    return rings


def add(rings, rows, cursor):
    """replay_buffer.py:89-127 on columns: `rows[c]` [length, ...] enters ring c at pos, rolling over at the end"""
    capacity = rings[0].shape[0]
    length = rows[0].shape[0]
    assert capacity > length, f"{length} samples are more than the buffer size."
    pos = int(cursor[POS])
    for target, source in zip(rings, rows):
        source = np.asarray(source).astype(target.dtype)  # _make_types
        assert source.shape[0] == length and source.shape[1:] == target.shape[1:]
        if pos + length < capacity:
            target[pos:pos + length] = source
        else:
            target[pos:capacity] = source[:capacity - pos]
            target[:length + pos - capacity] = source[capacity - pos:]
    cursor[FULL] = int(bool(cursor[FULL]) or (length + pos) >= capacity)
    cursor[POS] = (length + pos) % capacity
    return length


def push(rings, rows, cursor, keep=None):
    """hk_replay_push: the rows with keep != 0 (None: all), compacted in batch order, then added; the batch itself must
    be smaller than the buffer.  A batch of no rows leaves the cursor as it is, last_count included."""
    batch = rows[0].shape[0]
    assert rings[0].shape[0] > batch
    if batch == 0:
        return
    if keep is not None:
        kept = np.asarray(keep).reshape(-1) != 0
        assert kept.shape == (batch,)
        rows = [np.asarray(r)[kept] for r in rows]
    n = add(rings, rows, cursor)
    cursor[LAST_COUNT] = n
    cursor[TOTAL_PUSHED] += n


def sample_indices(cursor, capacity, batch_size, seed):
    """hk_replay_sample's indices [batch_size] int64 (-1 throughout for an empty buffer); samples_drawn moves on"""
    from oracle import np_oracle as NO
    if batch_size == 0:
        return np.zeros(0, dtype=np.int64)
    size = capacity if cursor[FULL] else int(cursor[POS])
    drawn = int(cursor[SAMPLES_DRAWN])
    cursor[SAMPLES_DRAWN] = drawn + 1
    if size == 0:
        return np.full(batch_size, -1, dtype=np.int64)
    j = np.arange(batch_size, dtype=np.uint64)
    words = NO.philox4x32(j >> np.uint64(2), drawn & 0xFFFFFFFF, (drawn >> 32) & 0xFFFFFFFF, STREAM_REPLAY, seed)
    word = np.choose((j & np.uint64(3)).astype(np.int64), [np.asarray(w, dtype=np.uint64) for w in words])
    return ((word * np.uint64(size)) >> np.uint64(32)).astype(np.int64)
