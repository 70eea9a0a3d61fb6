"""The per-game routines of the one-game-per-lane operators, run on the CPU: tests/lane_routines.hip builds
hk_game_generic.h, hk_hosts.h, hk_search_wave.h, hk_lane_games.h and the lane bodies of hk_game_play and hk_env_step for
the host, once under AddressSanitizer + UndefinedBehaviorSanitizer and once with the library's own host-relevant flags.
Every game runs in two memory layouts (every part its own allocation of the documented length; three adjacent slices
with canaries) and under four fills of whatever is not an input; the program itself fails on a fill-dependent result or
a touched canary, the sanitizers on an overrun of a part.  Here the results of both builds are compared with each other
and with the references -- oracle.c_oracle, tests/search_rules.py, morin_rules.py, play_rules.py, env_rules.py,
oracle.np_oracle -- as bit patterns, without tolerances.  (One NaN is as good as another: the sign and payload of the
NaN that inf - inf or inf * 0 gives are the compiler's choice of operand order, so all NaNs compare as one pattern;
-0.0 and +0.0 stay apart.)

Every test asserts from the reference's results alone, before it runs the program, that its inputs reach what it claims
to test.  No GPU is involved: what this cannot show is the device compiler's code for the same source."""
import itertools
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import env_rules as E
import morin_rules as M
import play_rules as P
import search_rules as S
from hironaka_amd import _abi as A
from oracle import c_oracle as CO
from oracle import np_oracle as NO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hironaka_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "lane_routines.hip")
HIPCC = "/opt/rocm/bin/hipcc"
COMMON = ["--offload-host-only", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
          "-I", CSRC]
BUILDS = {"sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
          "optimised": ["-O3"]}

(NUM_POINTS, STAGES, RESCALE, ZEILLINGER, FEATURE_SORT, LIST_PAIR, HOST_CLASS, SHIFT_CHILD, NOTE_INEXACT, REDUCE_CHILD,
 EXPAND_CHILD, EXPAND_MORIN, FIND_ROW, ROW_CONTAINED, EXCEEDS, NTH_BIT, RANDOM_AXIS, SUBSET_COEFFS, FORCED_OR_HOST,
 RECORD_MOVE, FINISH_GAME, PLAY_LANE, ENV_MOVE, EXTENT, ENV_FRESH, ENV_HOST_STEP, ENV_AGENT_STEP) = range(1, 28)

DTYPES = (np.float32, np.float64)
HOST_CODES = {"all_coord": A.HK_HOST_ALL_COORD, "zeillinger": A.HK_HOST_ZEILLINGER,
              "zeillinger_lex": A.HK_HOST_ZEILLINGER_LEX, "weak_spivakovsky": A.HK_HOST_WEAK_SPIVAKOVSKY,
              "weak_spivakovsky_min_hitting": A.HK_HOST_MIN_HITTING}
EXACT_LIMIT = {np.float32: 2 ** 24, np.float64: 2 ** 53}
TAKE = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON
LIST_SORTED = A.HK_SEM_LIST | A.HK_FLAG_COMPACT_SORTED  # kListFlags


# ---- the program ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """both builds of tests/lane_routines.hip, compiled once; returns run(cases) -> the results per block"""
    where = tmp_path_factory.mktemp("lane_routines")
    exes = {name: str(where / name) for name in BUILDS}
    jobs = [subprocess.Popen([HIPCC] + COMMON + flags + [SOURCE, "-o", exes[name]], stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True) for name, flags in BUILDS.items()]
    for job in jobs:
        log = job.communicate()[0]
        assert job.returncode == 0, log
    serial = itertools.count()

    def run(cases):
        stem = str(where / ("cases%d" % next(serial)))
        cases.write(stem + ".in")
        results = {}
        for name, exe in exes.items():
            done = subprocess.run([exe, stem + ".in", stem + "." + name], capture_output=True, text=True, timeout=600)
            if done.returncode != 0:
                print(done.stderr[-8000:])  # the sanitizer's report, or the program's own FAILED lines
            assert done.returncode == 0, "%s build: exit status %d\n%s" % (name, done.returncode, done.stderr[-4000:])
            assert not any(word in done.stderr for word in ("Sanitizer", "runtime error", "FAILED")), done.stderr[-4000:]
            results[name] = cases.read(stem + "." + name)
        for blk, (a, b) in enumerate(zip(results["sanitized"], results["optimised"])):
            for x, y in zip(a, b):
                assert_bits(x, y, "block %d: the two builds" % blk)
        return results["sanitized"]

    return run


class Cases:
    """the blocks of one case file"""

    def __init__(self):
        self.blocks = []

    def add(self, routine, dtype, m, d, T=None, I=None, D=None, out=(0, 0, 0), flags=0, ipar=(), dpar=()):
        given = [np.asarray(x) for x in (T, I, D) if x is not None]
        count = len(given[0])
        assert all(len(x) == count for x in given)
        T = np.zeros((count, 0), dtype) if T is None else np.ascontiguousarray(T, dtype=dtype).reshape(count, -1)
        I = np.zeros((count, 0), np.int32) if I is None else np.ascontiguousarray(I, dtype=np.int32).reshape(count, -1)
        D = np.zeros((count, 0), np.float64) if D is None else np.ascontiguousarray(D, dtype=np.float64).reshape(count, -1)
        ipar = list(ipar) + [0] * (8 - len(ipar))
        dpar = list(dpar) + [0.0] * (4 - len(dpar))
        head = struct.pack("<4iI7i8i4d", routine, DTYPES.index(dtype), m, d, flags, count, T.shape[1], I.shape[1],
                           D.shape[1], *out, *ipar, *dpar)
        self.blocks.append((head, T, I, D, dtype, count, out))
        return len(self.blocks) - 1

    def write(self, path):
        with open(path, "wb") as f:
            f.write(b"HKLR" + struct.pack("<2i", 1, len(self.blocks)))
            for head, T, I, D, _, _, _ in self.blocks:
                f.write(head + T.tobytes() + I.tobytes() + D.tobytes())

    def read(self, path):
        raw, at, res = open(path, "rb").read(), 0, []
        for _, _, _, _, dtype, count, out in self.blocks:
            got = []
            for kind, width in zip((dtype, np.int32, np.float64), out):
                size = count * width * np.dtype(kind).itemsize
                got.append(np.frombuffer(raw[at: at + size], dtype=kind).reshape(count, width))
                at += size
            res.append(tuple(got))
        assert at == len(raw)
        return res


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    a = np.where(np.isnan(a), np.array(np.nan, a.dtype), a)  # one NaN for all (the module's docstring)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, "%s: %d differ, the first at %s: got %r, want %r" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- inputs -----------------------------------------------------------------------------------------------------------

def masks_of(d):
    """the subsets of >= 2 coordinates as bit masks, in class order"""
    return [v for v in range(1 << d) if bin(v).count("1") >= 2]


def coords_of(classes, d, dtype):
    masks = np.array(masks_of(d))[np.asarray(classes)]
    return ((masks[:, None] >> np.arange(d)) & 1).astype(dtype)


def axis_index(axis, d):
    """hk_common.h axis_index: what the generic kernel hands stages_game for a caller's axis"""
    axis = np.asarray(axis)
    return np.where((axis >= 0) & (axis < d), axis, -1).astype(np.int32)


def small_states(d):
    """every state of 3 rows, each a hole or coordinates in 0..2: (1 + 3^d)^3 of them, [count, 3, d] int64"""
    rows = np.array([[-1] * d] + list(itertools.product(range(3), repeat=d)), dtype=np.int64)
    idx = np.array(list(itertools.product(range(len(rows)), repeat=3)))
    return rows[idx]


def random_games(rng, count, m, d, dtype, maxv=9, holes=0.3, integer=True):
    """seeded games with holes anywhere, duplicate rows, zero rows and supports that cover fewer than 2 coordinates"""
    p = rng.integers(0, maxv + 1, (count, m, d)).astype(np.float64)
    if not integer:
        p = p + rng.integers(0, 4, p.shape) / 4.0
    kind = rng.integers(0, 8, count)
    for g in range(count):
        if kind[g] == 1 and m > 1:  # duplicate rows
            src, dst = rng.integers(0, m, 2)
            p[g, dst] = p[g, src]
        if kind[g] == 2:  # a zero row
            p[g, rng.integers(0, m)] = 0
        if kind[g] == 3:  # one coordinate carries every support
            k = rng.integers(0, d)
            keep = p[g, :, k].copy()
            p[g] = 0
            p[g, :, k] = keep
        if kind[g] == 4:  # sparse supports
            p[g] *= rng.integers(0, 2, (m, d))
    p[rng.random((count, m)) < holes] = -1
    return p.astype(dtype)


SHAPES = [(m, d) for m in (1, 2, 5, 20, 33, 64) for d in range(2, 8)]


# ---- hk_game_generic.h against the C oracle ---------------------------------------------------------------------------

SEM_FLAGS = {"jax": [0], "torch": [0, A.HK_FLAG_AXIS_NOOP_IF_INVALID, A.HK_FLAG_IGNORE_ENDED,
                                   A.HK_FLAG_AXIS_NOOP_IF_INVALID | A.HK_FLAG_IGNORE_ENDED],
             "list": [0, A.HK_FLAG_AXIS_NOOP_IF_INVALID]}


def add_stages(cases, p, coords, axis, stages, flags, pad=-1.0):
    """a stages_game block as the generic kernel calls it, and the oracle's result for the same request"""
    count, m, d = p.shape
    shift = bool(stages & A.HK_STAGE_SHIFT)
    T = np.concatenate([p.reshape(count, -1), coords], 1) if shift else p.reshape(count, -1)
    want = CO.step(p, coords if shift else None, np.asarray(axis, np.int32) if shift else None, stages=stages,
                   flags=flags, padding_value=pad)["points"]
    blk = cases.add(STAGES, p.dtype.type, m, d, T=T, I=axis_index(axis, d), out=(m * d, 0, 0), flags=flags,
                    ipar=(stages,), dpar=(pad,))
    return blk, want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sem", ("jax", "torch", "list"))
@pytest.mark.parametrize("d", (2, 3))
def test_stages_on_every_small_state_class_and_axis(program, d, sem, dtype):
    """every state of 3 rows over {hole, 0..2}^d, every class, every axis (-1 and the axes outside the subset
    included), through shift + reposition + Newton"""
    states = small_states(d)
    assert len(states) == {2: 1000, 3: 21952}[d]
    ncls = len(masks_of(d))
    axes = np.arange(-1, d + (d == 2))  # d itself too where that is cheap: it matches nothing, as -1 does
    s, c, a = np.meshgrid(np.arange(len(states)), np.arange(ncls), axes, indexing="ij")
    p = states[s.ravel()].astype(dtype)
    coords, axis = coords_of(c.ravel(), d, dtype), a.ravel()
    flags = A.SEMANTICS[sem] | (A.HK_FLAG_AXIS_NOOP_IF_INVALID if sem != "jax" else 0)
    cases = Cases()
    blk, want = add_stages(cases, p, coords, axis, TAKE, flags)
    # reached, by the oracle alone: games that end, games that do not, rows that Newton removes, illegal axes
    live_in, live_out = (p[:, :, 0] >= 0).sum(1), (want[:, :, 0] >= 0).sum(1)
    assert (live_out < 2).any() and (live_out == 3).any() and (live_out < live_in).any()
    illegal = (axis_index(axis, d) < 0) | (coords[np.arange(len(axis)), np.clip(axis, 0, d - 1)] == 0)
    assert illegal.any() and (~illegal).any()
    if sem == "list":  # sort_compact_game moves rows: the list result is not the rows-in-place result
        in_place = CO.step(p, coords, axis.astype(np.int32), stages=TAKE,
                           flags=A.HK_SEM_TORCH | A.HK_FLAG_AXIS_NOOP_IF_INVALID)["points"]
        assert (want != in_place).any(axis=(1, 2)).sum() > len(p) // 10
    got = program(cases)[blk][0]
    assert_bits(got.reshape(want.shape), want, "stages_game %s d=%d" % (sem, d))


def stage_requests():
    """(stages, flags) for every stage mask hk_step accepts, under every semantics and flag the routines read"""
    out = []
    for stages in range(1, 16):
        for sem, extras in SEM_FLAGS.items():
            for extra in extras:
                for compact in ((0, A.HK_FLAG_COMPACT_SORTED) if sem != "list" else (0,)):
                    out.append((stages, A.SEMANTICS[sem] | extra | compact))
    return out


def per_shape(m):
    return 24 if m <= 5 else 8 if m <= 20 else 3


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", range(2, 8))
def test_stages_on_random_games_under_every_mask_semantics_and_flag(program, d, dtype):
    rng = np.random.default_rng(100 + d)
    cases, wants, moved, ended = Cases(), [], 0, 0
    for m in (1, 2, 5, 20, 33, 64):
        for k, (stages, flags) in enumerate(stage_requests()):
            count = per_shape(m)
            p = random_games(rng, count, m, d, dtype, integer=bool(k % 2))
            coords = coords_of(rng.integers(0, len(masks_of(d)), count), d, dtype)
            axis = rng.integers(-1, d + 1, count)
            blk, want = add_stages(cases, p, coords, axis, stages, flags, pad=(-1.0, -1e-8)[(k // 2) % 2])
            wants.append((blk, want, (m, stages, flags)))
            if (stages & A.HK_STAGE_NEWTON) and (flags & (A.HK_SEM_LIST | A.HK_FLAG_COMPACT_SORTED)):
                plain = CO.step(p, coords, axis.astype(np.int32), stages=stages & ~A.HK_STAGE_RESCALE,
                                flags=(flags & ~(A.HK_FLAG_COMPACT_SORTED | A.HK_SEM_MASK)) | A.HK_SEM_TORCH)["points"]
                moved += int(((want[:, :, 0] >= 0) != (plain[:, :, 0] >= 0)).any())
            ended += int(((want[:, :, 0] >= 0).sum(1) < 2).any())
    assert moved > 20 and ended > 20  # sort_compact_game moved rows; games ended
    got = program(cases)
    for blk, want, what in wants:
        assert_bits(got[blk][0].reshape(want.shape), want, "stages_game m=%d stages=%d flags=%d" % what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rescale_num_points_zeillinger_and_features_against_the_oracle(program, dtype):
    rng = np.random.default_rng(7)
    cases, wants, zero_max, positive_max, ties = Cases(), [], 0, 0, 0
    for m, d in SHAPES:
        count = 3 * per_shape(m)
        p = random_games(rng, count, m, d, dtype, maxv=3, integer=False)
        p[0][p[0] > 0] = 0  # the maximum of game 0 is zero
        n = m * d
        top = np.where(p[:, :, :1] >= 0, p, -np.inf).reshape(count, -1).max(1)
        zero_max += int((top == 0).sum())
        positive_max += int((top > 0).sum())
        ties += int(sum(len(np.unique(g[:, -1])) < m for g in p))
        for sem in ("jax", "torch", "list"):
            for pad in (-1.0, -1e-8):
                blk = cases.add(RESCALE, dtype, m, d, T=p, out=(n, 0, 0), flags=A.SEMANTICS[sem], dpar=(pad,))
                wants.append((blk, 0, CO.rescale(p, padding_value=pad, sem=sem).reshape(count, n), "rescale " + sem))
        blk = cases.add(NUM_POINTS, dtype, m, d, T=p, out=(0, 1, 0))
        wants.append((blk, 1, CO.get_num_points(p)[:, None], "num_points"))
        for listed, sem in enumerate(("jax", "list")):
            blk = cases.add(ZEILLINGER, dtype, m, d, T=p, out=(0, 1, 0), ipar=(listed,))
            wants.append((blk, 1, CO.zeillinger(p, sem=sem)[:, None], "zeillinger " + sem))
        for scale in (False, True):  # hk_get_features: [rescale,] the sort on the last coordinate
            stages = (A.HK_STAGE_RESCALE if scale else 0) | 256
            blk = cases.add(STAGES, dtype, m, d, T=p, I=np.full(count, -1), out=(n, 0, 0), flags=A.HK_SEM_JAX,
                            ipar=(stages,), dpar=(-1.0,))
            wants.append((blk, 0, CO.get_features(p, scale_observation=scale), "get_features scale=%d" % scale))
        blk = cases.add(STAGES, dtype, m, d, T=p, I=np.full(count, -1), out=(n, 0, 0), flags=A.HK_SEM_TORCH,
                        ipar=(512,), dpar=(-1.0,))
        wants.append((blk, 0, CO.get_features_torch(p).reshape(count, n), "get_features_torch"))
        for coord0, want in ((0, CO.get_features(p, scale_observation=False)), (1, CO.get_features_torch(p))):
            blk = cases.add(FEATURE_SORT, dtype, m, d, T=p, out=(n, 0, 0), ipar=(coord0,))
            wants.append((blk, 0, want.reshape(count, n), "feature_sort_game coord0=%d" % coord0))
    assert zero_max >= len(SHAPES) and positive_max > 100 and ties > 100
    got = program(cases)
    for blk, which, want, what in wants:
        assert_bits(got[blk][which], want, what)


def nonfinite_games(rng, count, m, d, dtype):
    p = random_games(rng, count, m, d, dtype)
    for g in range(count):
        r, k = rng.integers(0, m), rng.integers(0, d)
        if g % 5 == 4:
            p[g, r] = p[g, r] * (-1) ** rng.integers(0, 2, d)  # a row of mixed signs
            continue
        if p[g, r, 0] < 0:
            p[g, r] = 1
        p[g, r, k] = (np.inf, np.nan, -0.0, -np.inf)[g % 5]
        if g % 10 == 7:
            p[g, (r + 1) % m] = p[g, r]  # a duplicate of a non-finite row
    return p


@pytest.mark.parametrize("dtype", DTYPES)
def test_stages_on_non_finite_input(program, dtype):
    """inf, NaN, -0.0 and mixed-sign rows under the jax and torch semantics (list semantics stay finite-only), and the
    game of tests/golden/nonfinite_regression.json"""
    rng = np.random.default_rng(4)
    cases, wants, nans = Cases(), [], 0
    for m, d in ((1, 2), (2, 3), (5, 3), (6, 3), (20, 4), (7, 5), (33, 6), (9, 7)):
        count = 40
        p = nonfinite_games(rng, count, m, d, dtype)
        coords = coords_of(rng.integers(0, len(masks_of(d)), count), d, dtype)
        axis = rng.integers(0, d, count)
        for sem in ("jax", "torch"):
            flags = A.SEMANTICS[sem] | (A.HK_FLAG_AXIS_NOOP_IF_INVALID if sem == "torch" else 0)
            for stages in (1, 2, 4, 8, 3, 7, 15):
                blk, want = add_stages(cases, p, coords, axis, stages, flags)
                wants.append((blk, want, (m, d, sem, stages)))
                nans += int((np.isnan(want) & ~np.isnan(p)).sum())
    with open(os.path.join(ROOT, "tests", "golden", "nonfinite_regression.json")) as f:
        fx = json.load(f)
    conv = lambda rows: np.array([[float(v) for v in r] for r in rows], dtype=dtype)[None]  # noqa: E731
    pin, pexp = conv(fx["points_in"]), conv(fx["points_out"])
    blk, want = add_stages(cases, pin, coords_of([fx["host_class"]], fx["dim"], dtype), np.array([fx["axis"]]),
                           fx["stages"], A.HK_SEM_JAX)
    assert np.array_equal(want, pexp, equal_nan=True)
    wants.append((blk, pexp, "nonfinite_regression.json"))
    assert nans > 50  # inf * 0 and inf - inf were reached: NaN where the input had none
    got = program(cases)
    for blk, want, what in wants:
        assert_bits(got[blk][0].reshape(want.shape), want, "stages_game %r" % (what,))


# ---- hk_hosts.h against tests/search_rules.py -------------------------------------------------------------------------

def rule_class(host, state):
    """the class id host_class_game is to return for one game: -1 where the rules have no list.  AllCoord is the one
    routine without a -1: host_class_game<ALL_COORD> names the full subset whatever the state (its callers test the
    number of points themselves)"""
    d = state.shape[1]
    if host == "all_coord":
        return S.class_id(range(d), d)
    got = S.host_list(host, state)
    return -1 if got is None else S.class_id(got, d)


def rule_pair(state, lex):
    pair = S.zeillinger_pair(state, lex)
    return -1 if pair is None else pair[0] * 8 + pair[1]


def add_hosts(cases, p, dtype, widths, rules=None, which=None):
    """blocks of host_class_game (every host, the given bitmap widths) and zeillinger_list_pair on the games p, and what
    the rules say: [(block, want, what)].  rules: a dict that keeps the rules' answers for another dtype of the same p;
    which: one host's name, or "pair", to add that routine's blocks alone"""
    count, m, d = p.shape
    ints = p.astype(np.int64)
    rules = {} if rules is None else rules
    out = []
    for host, code in HOST_CODES.items():
        if which not in (None, host):
            continue
        if host not in rules:
            rules[host] = np.array([rule_class(host, g) for g in ints], np.int32)[:, None]
        want = rules[host]
        for wide in widths:
            blk = cases.add(HOST_CLASS, dtype, m, d, T=p, out=(0, 1, 0), ipar=(code, wide))
            out.append((blk, want, "host_class_game %s %s m=%d d=%d" % (host, ("uint64_t", "Bits128")[wide], m, d)))
    for lex in (0, 1) if which in (None, "pair") else ():
        if lex not in rules:
            rules[lex] = np.array([rule_pair(g, bool(lex)) for g in ints], np.int32)[:, None]
        want = rules[lex]
        blk = cases.add(LIST_PAIR, dtype, m, d, T=p, out=(0, 1, 0), ipar=(lex,))
        out.append((blk, want, "zeillinger_list_pair lex=%d m=%d d=%d" % (lex, m, d)))
    return out


def assert_hosts_reached(wants, sizes, which=None):
    """from the rules alone: every host but AllCoord says -1 somewhere, and so does zeillinger_list_pair; the hitting-set
    hosts pick every size in `sizes`; both bitmap widths occur"""
    for host in HOST_CODES:
        mine = [w for _, w, what in wants if what.startswith("host_class_game %s " % host)]
        assert host == "all_coord" or which not in (None, host) or any((w == -1).any() for w in mine), host
    if which in (None, "pair"):
        assert any((w == -1).any() for _, w, what in wants if what.startswith("zeillinger_list_pair"))
    if which != "pair":
        assert {what.split()[2] for _, _, what in wants if what.startswith("host_class")} == {"uint64_t", "Bits128"}
    for host in ("weak_spivakovsky", "weak_spivakovsky_min_hitting"):
        if which not in (None, host):
            continue
        seen = set()
        for _, w, what in wants:
            if what.startswith("host_class_game %s " % host):
                d = int(what.rsplit("d=", 1)[1])
                seen |= {(d, bin(masks_of(d)[c]).count("1")) for c in set(w.ravel().tolist()) if c >= 0}
        assert sizes <= seen, (host, sorted(sizes - seen))


@pytest.mark.parametrize("which", list(HOST_CODES) + ["pair"])
@pytest.mark.parametrize("d", (2, 3))
def test_hosts_on_every_small_state(program, d, which):
    states = small_states(d)
    cases, wants, rules = Cases(), [], {}
    for dtype in DTYPES:
        wants += add_hosts(cases, states.astype(dtype), dtype, (0, 1), rules, which)
    assert_hosts_reached(wants, {(d, k) for k in range(2, d + 1)}, which)
    got = program(cases)
    for blk, want, what in wants:
        assert_bits(got[blk][1], want, what)


def unit_rows(rng, m, d, k):
    """a game whose supports are the singletons of the first k coordinates: every hitting set has all k"""
    p = np.full((m, d), -1, np.int64)
    for i in range(min(k, m)):
        p[i] = 0
        p[i, i] = rng.integers(1, 9)
    return p


@pytest.mark.parametrize("dtype", DTYPES)
def test_hosts_on_random_games(program, dtype):
    rng = np.random.default_rng(11)
    cases, wants = Cases(), []
    for m, d in SHAPES:
        count = 24 if m <= 5 else 8
        p = random_games(rng, count, m, d, np.int64, maxv=4)
        named = [unit_rows(rng, m, d, k) for k in range(2, d + 1) if k <= m]
        p = np.concatenate([p] + [g[None] for g in named]).astype(dtype)
        wants += add_hosts(cases, p, dtype, (0, 1) if d <= 6 else (1,))
    assert_hosts_reached(wants, {(d, k) for d in range(2, 8) for k in range(2, d + 1)})
    got = program(cases)
    for blk, want, what in wants:
        assert_bits(got[blk][1], want, what)


# ---- hk_search_wave.h and hk_lane_games.h: the pieces of a move -------------------------------------------------------

def padded(pts, m, dtype):
    out = np.full((m, pts.shape[1]), -1, dtype)
    out[: len(pts)] = pts
    return out


def exact_limit_games(m, d, dtype):
    """rows with a coordinate at the last exact integer and at the first inexact one, so that a shift lands below, on
    and (by one addend) on the limit again: every sum stays representable, so the integer rules still give the state"""
    L = EXACT_LIMIT[dtype]
    games = []
    for big, other in ((L - 1, 0), (L - 1, 1), (L, 0), (L - 2, 1), (L - 2, 2)):
        p = np.full((m, d), -1, np.int64)
        p[0] = 0
        p[0, 0], p[0, 1] = big, other
        if m > 1:
            p[m - 1] = 0
            p[m - 1, 1] = 3
        games.append(p)
    return np.array(games)


@pytest.mark.parametrize("dtype", DTYPES)
def test_children_against_the_rules(program, dtype):
    """shift_child, note_inexact, reduce_child, expand_child, expand_morin_child, find_row, row_contained"""
    rng = np.random.default_rng(13)
    L = EXACT_LIMIT[dtype]
    cases, wants = Cases(), []
    seen = dict(inexact=0, exact_at_limit=0, kept=0, lost=0, twin=0, moved=0)
    for m, d in SHAPES:
        n = m * d
        p = random_games(rng, 12 if m <= 20 else 4, m, d, np.int64, maxv=5)
        p = np.concatenate([p, exact_limit_games(m, d, dtype)])
        p[(p[:, :, 0] >= 0).sum(1) == 0, 0] = 1  # no game without a point: the Morin child needs a row to follow
        count = len(p)
        cls = rng.integers(0, len(masks_of(d)), count)
        cls[-5:] = 0  # the limit games: coordinates 0 and 1
        coords = coords_of(cls, d, dtype)
        subsets = [[k for k in range(d) if c[k]] for c in coords]
        ax = np.array([s[rng.integers(0, len(s))] for s in subsets])
        ax[-5:] = 0
        pd = np.array([rng.choice(np.nonzero(g[:, 0] >= 0)[0]) for g in p])
        T = np.concatenate([p.reshape(count, n), coords], 1)
        shifted, child, np_child, inexact = [], [], [], []
        morin, morin_np, morin_dist, contained, found, reduced_np = [], [], [], [], [], []
        for g, sub, a, at in zip(p, subsets, ax.tolist(), pd.tolist()):
            live = S.live(g)
            sh = g.copy()
            sh[g[:, 0] >= 0] = S.shift(live, sub, a)
            shifted.append(sh)
            kid = S.child(live, sub, a)
            child.append(padded(kid, m, np.int64))
            np_child.append(len(kid))
            inexact.append(int((live[:, sub].sum(1) >= L).any()))
            seen["moved"] += int(not np.array_equal(kid, S.shift(live, sub, a)[: len(kid)]))
            rank = int((g[:at, 0] >= 0).sum())
            kept, nd, twin = S.morin_child(live, sub, a, rank)
            morin.append(padded(kept, m, np.int64))
            morin_np.append(len(kept))
            morin_dist.append(-1 if nd is None else nd)
            seen["kept" if nd is not None else "lost"] += 1
            seen["twin"] += int(twin)
            red, where = M.tracked_newton(g, at)
            contained.append(int(where < 0))
            reduced_np.append(len(red))
            found.append(where)
        seen["inexact"] += sum(inexact)
        seen["exact_at_limit"] += int(sum(1 for g, sub, flag in zip(p, subsets, inexact)
                                          if not flag and (S.live(g)[:, sub].sum(1) == L - 1).any()))
        as_T = lambda rows: np.array(rows).astype(dtype).reshape(count, -1)  # noqa: E731
        col = lambda *cols: np.array(cols, np.int32).T  # noqa: E731
        add = lambda routine, which, want, what, **kw: wants.append(  # noqa: E731
            (cases.add(routine, dtype, m, d, **kw), which, want, "%s m=%d d=%d" % (what, m, d)))
        add(SHIFT_CHILD, 0, np.concatenate([as_T(shifted), as_T(p)], 1), "shift_child", T=T, I=ax, out=(2 * n, 0, 0))
        for entry in (0, 1):
            add(NOTE_INEXACT, 1, col(np.array(inexact) | entry), "note_inexact", T=as_T(shifted),
                I=col(ax, np.full(count, entry)), out=(0, 1, 0))
        add(REDUCE_CHILD, 0, as_T(child), "reduce_child", T=as_T(shifted), out=(n, 1, 0))
        add(REDUCE_CHILD, 1, col(np_child), "reduce_child's count", T=as_T(shifted), out=(n, 1, 0))
        add(EXPAND_CHILD, 0, as_T(child), "expand_child", T=T, I=ax, out=(n, 2, 0))
        add(EXPAND_CHILD, 1, col(np_child, inexact), "expand_child's count and inexact", T=T, I=ax, out=(n, 2, 0))
        add(EXPAND_MORIN, 0, as_T(morin), "expand_morin_child", T=T, I=col(ax, pd), out=(n, 3, 0))
        add(EXPAND_MORIN, 1, col(morin_np, inexact, morin_dist), "expand_morin_child's count, inexact and dist", T=T,
            I=col(ax, pd), out=(n, 3, 0))
        rows = np.array([g[at] for g, at in zip(p, pd)])
        add(ROW_CONTAINED, 1, col(contained), "row_contained", T=np.concatenate([as_T(p), as_T(rows)], 1), I=pd,
            out=(0, 1, 0))
        reduced = np.array([padded(M.tracked_newton(g, -1)[0], m, np.int64) for g in p])
        last = [max([i for i in range(k) if (r[i] == row).all()], default=-1)
                for r, row, k in zip(reduced, rows, reduced_np)]
        assert all(f == w for f, w in zip(last, found) if w >= 0)  # where the row survives, the rules name its place
        add(FIND_ROW, 1, col(last), "find_row", T=np.concatenate([as_T(reduced), as_T(rows)], 1), I=reduced_np,
            out=(0, 1, 0))
    assert seen["inexact"] >= 2 * len(SHAPES) and seen["exact_at_limit"] >= len(SHAPES), seen
    assert seen["kept"] > 100 and seen["lost"] > 100 and seen["twin"] > 5 and seen["moved"] > 100, seen
    got = program(cases)
    for blk, which, want, what in wants:
        assert_bits(got[blk][which], want, what)


def u64(v):
    """a 64-bit value as the two int32 the case file carries"""
    v = int(v) % (1 << 64)
    return [np.uint32(v & 0xFFFFFFFF).astype(np.int32), np.uint32(v >> 32).astype(np.int32)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_exceeds_game_at_and_next_to_a_coordinate(program, dtype):
    rng = np.random.default_rng(17)
    cases, wants, over, under = Cases(), [], 0, 0
    for m, d in SHAPES:
        p = random_games(rng, 6, m, d, dtype, maxv=50, integer=False)
        p[0, :, 0] = -1
        p[0, :, 1:] = 99  # holes whose other coordinates are large: not points, so nothing exceeds
        p[1, 0] = np.arange(d) + 1  # at least one point
        top = np.array([P.points_of(g).max(initial=0) for g in p], np.float64)
        for nudge in (-1, 0, 1):
            thr = top if nudge == 0 else np.nextafter(top, nudge * np.inf)
            want = np.array([[int(P.exceeds(g, t))] for g, t in zip(p, thr)], np.int32)
            over, under = over + int(want.sum()), under + int((1 - want).sum())
            assert nudge >= 0 or want[1:][top[1:] > 0].all()  # one ulp (of a double) below the maximum: exceeded
            assert nudge < 0 or not want.any()
            blk = cases.add(EXCEEDS, dtype, m, d, T=p, D=thr, out=(0, 1, 0))
            wants.append((blk, want, "exceeds_game m=%d d=%d nudge=%d" % (m, d, nudge)))
    assert over > 100 and under > 100
    got = program(cases)
    for blk, want, what in wants:
        assert_bits(got[blk][1], want, what)


def test_bits_draws_and_coefficients(program):
    """nth_bit, random_legal_axis (against env_rules.philox_axis and np_oracle.philox4x32) and subset_coeffs"""
    rng = np.random.default_rng(19)
    cases, wants = Cases(), []
    pairs = [(sub, k) for sub in list(range(1, 128)) + [0x80000000, 0xFFFFFFFF, 0x40000001]
             for k in range(bin(sub).count("1"))]
    want = [[b for b in range(32) if (sub >> b) & 1][k] for sub, k in pairs]
    blk = cases.add(NTH_BIT, np.float32, 1, 2, I=np.array(pairs, np.uint32).astype(np.int32), out=(0, 1, 0))
    wants.append((blk, 1, np.array(want, np.int32)[:, None], "nth_bit"))
    rows, want = [], []
    for k in range(600):
        d = int(rng.integers(2, 8))
        sub = int(rng.integers(1, 1 << d))
        game = int(rng.integers(0, 1 << 63)) if k % 3 else int(rng.integers(0, 5)) + (0xFFFFFFFF if k % 2 else 0)
        counter, seed = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 63)) * 2 + 1
        stream = 3 if k % 4 else int(rng.integers(0, 6))
        rows.append([np.uint32(sub).astype(np.int32)] + u64(game) + [np.uint32(counter).astype(np.int32),
                                                                     stream] + u64(seed))
        word = int(NO.philox4x32(game & 0xFFFFFFFF, game >> 32, counter, stream, seed)[0])
        axis = E.mask_coords(sub, d)[(word * bin(sub).count("1")) >> 32]
        if stream == E.STREAM_PLAY_AGENT:
            assert axis == E.philox_axis(seed, game, counter, sub, d)
        want.append(axis)
    assert len(set(want)) == 7  # every coordinate is drawn
    blk = cases.add(RANDOM_AXIS, np.float32, 1, 2, I=np.array(rows, np.int32), out=(0, 1, 0))
    wants.append((blk, 1, np.array(want, np.int32)[:, None], "random_legal_axis"))
    for dtype in DTYPES:
        for d in range(2, 8):
            subs = np.arange(1 << d)
            blk = cases.add(SUBSET_COEFFS, dtype, 1, d, I=subs, out=(d, 0, 0))
            wants.append((blk, 0, ((subs[:, None] >> np.arange(d)) & 1).astype(dtype), "subset_coeffs d=%d" % d))
    got = program(cases)
    for blk, which, want, what in wants:
        assert_bits(got[blk][which], want, what)


def test_moves_given_and_left(program):
    """forced_or_host_move, record_move and finish_game against their contract in hk_lane_games.h, the host's choice
    from the rules"""
    rng = np.random.default_rng(23)
    cases, wants, seen = Cases(), [], dict(forced=0, host=0, none=0, outside=0, beyond=0)
    dtype = np.float64
    for m, d, steps in ((1, 2, 1), (5, 3, 4), (20, 4, 7), (33, 6, 3), (9, 7, 5)):
        ncls, n = len(masks_of(d)), m * d
        for host in [None] + list(HOST_CODES):
            for bits in (0, 1, 2, 3):
                count = 24
                p = random_games(rng, count, m, d, np.int64, maxv=3)
                t = rng.integers(0, steps, count)
                cin = rng.integers(-2, ncls + 2, (count, steps))
                ain = rng.integers(-2, d + 1, (count, steps))
                want = []
                for g in range(count):
                    cls = int(cin[g, t[g]]) if bits & 1 else -1
                    seen["forced"] += cls >= 0
                    if cls < 0 and host is not None:
                        cls = rule_class(host, p[g]) if host != "all_coord" else S.class_id(range(d), d)
                        seen["host"] += 1
                    if cls < 0 or cls >= ncls:
                        want.append([0, cls, -9, -9])
                        seen["none" if cls < 0 else "beyond"] += 1
                        continue
                    sub = masks_of(d)[cls]
                    ax = int(ain[g, t[g]]) if bits & 2 else -1
                    ok = ax < 0 or (ax < d and (sub >> ax) & 1)
                    seen["outside"] += not ok
                    want.append([int(ok), cls, sub, ax])
                blk = cases.add(FORCED_OR_HOST, dtype, m, d, T=p, I=np.concatenate([t[:, None], cin, ain], 1),
                                out=(0, 4, 0), ipar=(-1 if host is None else HOST_CODES[host], steps, bits))
                wants.append((blk, 1, np.array(want, np.int32), "forced_or_host_move %s bits=%d m=%d d=%d" % (host, bits, m, d)))
        for bits in (0, 4, 8, 12):
            count = 3 * steps
            t, cls, ax = np.arange(count) % steps, rng.integers(0, ncls, count), rng.integers(0, d, count)
            want = np.full((count, 2, steps), -7, np.int32)
            want[np.arange(count), 0, t], want[np.arange(count), 1, t] = cls, ax
            want[:, 0] *= bool(bits & 4)
            want[:, 1] *= bool(bits & 8)
            blk = cases.add(RECORD_MOVE, dtype, m, d, I=np.stack([t, cls, ax], 1), out=(0, 2 * steps, 0),
                            ipar=(0, steps, bits))
            wants.append((blk, 1, want.reshape(count, -1), "record_move bits=%d" % bits))
            for kind in DTYPES:
                lens = np.arange(2 * (steps + 1)) // 2
                swapped = np.arange(len(lens)) % 2
                state = random_games(rng, len(lens), m, d, kind)
                want = np.full((len(lens), 2, steps), -1, np.int32)
                for g, ln in enumerate(lens):
                    want[g, :, :ln] = 7
                want[:, 0] *= bool(bits & 4)
                want[:, 1] *= bool(bits & 8)
                blk = cases.add(FINISH_GAME, kind, m, d, T=state, I=np.stack([lens, swapped], 1),
                                out=(n, 2 * steps, 0), ipar=(0, steps, bits))
                wants.append((blk, 0, state.reshape(len(lens), n), "finish_game's state bits=%d" % bits))
                wants.append((blk, 1, want.reshape(len(lens), -1), "finish_game's records bits=%d" % bits))
    assert all(v > 20 for v in seen.values()), seen
    got = program(cases)
    for blk, which, want, what in wants:
        assert_bits(got[blk][which], want, what)


# ---- the lane bodies --------------------------------------------------------------------------------------------------

AGENT_CODES = {"choose_first": A.HK_AGENT_CHOOSE_FIRST, "choose_last": A.HK_AGENT_CHOOSE_LAST,
               "random": A.HK_AGENT_RANDOM_LEGAL}
OUTCOMES = {P.RUNNING: "step limit", P.ENDED: "ended", P.NO_MOVE: "no move", P.INEXACT: "inexact",
            P.VALUE_LIMIT: "value limit"}


def play_block(cases, rng, dtype, m, d, host, agent, flags, roots, steps, forced, thresholds):
    """one play_lane block and what play_rules.play says of every game: (block, the final states, [length, outcome,
    classes, axes] per game)"""
    count, ncls = len(roots), len(masks_of(d))
    bits = 12 | (3 if forced else 0) | (1 if host is None else 0)
    cin = np.full((count, steps), -1, np.int64)
    ain = np.full((count, steps), -1, np.int64)
    if forced:
        cin = np.where(rng.random(cin.shape) < 0.7, rng.integers(0, ncls, cin.shape), -1)
        ain = np.where(rng.random(ain.shape) < 0.15, rng.integers(0, d, ain.shape), -1)
        cin[rng.random(count) < 0.05, 0] = ncls  # a class the dimension does not have
    if host is None:
        cin = np.where(cin < 0, rng.integers(0, ncls, cin.shape), cin)
    offsets = rng.integers(0, 1 << 62, count)
    seeds = rng.integers(0, 1 << 62, count)
    step0 = rng.integers(0, 1 << 31, count)
    ints = np.array([list(cin[g]) + list(ain[g]) + u64(offsets[g]) + u64(seeds[g]) + [step0[g]] for g in range(count)])
    states, results = [], []
    for g in range(count):
        if agent == "random":
            pick = lambda coords, t, g=g: E.philox_axis(int(seeds[g]), int(offsets[g]), int(step0[g]) + t,  # noqa: E731
                                                        E.coords_mask(coords), d)
        else:
            pick = agent
        got = P.play(roots[g], host, pick, steps, classes=cin[g] if forced or host is None else None,
                     axes=ain[g] if forced else None, reposition=bool(flags & 1), rescaled=bool(flags & 2),
                     reduce_root=bool(flags & 4), rescale_root=bool(flags & 8),
                     value_threshold=thresholds[g] if thresholds[g] > 0 else None, dtype=dtype)
        states.append(np.asarray(got.state, dtype).reshape(-1))
        pad = [-1] * (steps - got.length)
        results.append([got.length, got.outcome] + got.classes + pad + got.axes + pad)
    blk = cases.add(PLAY_LANE, dtype, m, d, T=np.asarray(roots, dtype), I=ints, D=thresholds, out=(m * d, 2 + 2 * steps, 0),
                    ipar=(-1 if host is None else HOST_CODES[host], steps, bits, AGENT_CODES[agent], flags))
    return blk, np.array(states), np.array(results, np.int32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("host", [None] + list(HOST_CODES))
def test_play_lane_against_the_rules(program, host, dtype):
    """whole games: every fixed host and the forced launch, the three agents, all sixteen combinations of reposition,
    rescale, reduce_root and rescale_root, forced classes and axes, a value threshold, roots at the exactness limit"""
    rng = np.random.default_rng(29 + len(host or ""))
    L = EXACT_LIMIT[dtype]
    cases, wants, seen = Cases(), [], {name: 0 for name in OUTCOMES.values()}
    for k, (m, d) in enumerate(SHAPES):
        for flags in range(16):
            agent = ("choose_first", "random", "choose_last")[(flags + k) % 3]
            count = 4 if m <= 5 else 1
            roots = random_games(rng, count, m, d, np.int64, maxv=12, holes=0.2)
            limit = exact_limit_games(m, d, dtype)[:3]
            roots = np.concatenate([roots, limit])
            steps = int(rng.integers(1, 9))
            thresholds = np.where(rng.random(len(roots)) < 0.3, rng.integers(8, 40, len(roots)), 0).astype(np.float64)
            if flags & 10:  # rescaled states lie in [0, 1]
                thresholds = np.where(thresholds > 0, 0.5, 0.0)
            blk, state, ints = play_block(cases, rng, dtype, m, d, host, agent, flags, roots, steps,
                                          forced=bool((flags + k) % 2), thresholds=thresholds)
            wants.append((blk, state, ints, "play_lane %s %s flags=%d m=%d d=%d" % (host, agent, flags, m, d)))
            for code in ints[:, 1]:
                seen[OUTCOMES[int(code)]] += 1
    assert all(count > 0 for count in seen.values()), seen
    got = program(cases)
    for blk, state, ints, what in wants:
        assert_bits(got[blk][1], ints, what + ": length, outcome, classes, axes")
        assert_bits(got[blk][0], state, what + ": the final state")


def env_roots(rng, count, m, d):
    roots = random_games(rng, count, m, d, np.int64, maxv=9, holes=0.2)
    roots[(roots[:, :, 0] >= 0).sum(1) == 0, 0] = 1  # reset is handed at least one point
    return roots


@pytest.mark.parametrize("dtype", DTYPES)
def test_env_move_extent_and_fresh(program, dtype):
    rng = np.random.default_rng(31)
    cases, wants, seen = Cases(), [], dict(no_axis=0, moved=0, short=0, long=0, second_newton=0)
    for m, d in SHAPES:
        n, count = m * d, 10 if m <= 5 else 4
        p = env_roots(rng, count, m, d).astype(dtype)
        blk = cases.add(EXTENT, dtype, m, d, T=p, out=(0, 1, 0))
        want = [max([i + 1 for i in range(m) if g[i, 0] >= 0], default=0) for g in p]
        wants.append((blk, 1, np.array(want, np.int32)[:, None], "extent_game"))
        for reposition in (0, 1):
            subs = rng.integers(0, 1 << d, count)
            ax, want = [], []
            for g, sub in zip(p, subs):
                coords = E.mask_coords(sub, d)
                if len(coords) >= 2 and rng.random() < 0.8:
                    ax.append(int(rng.choice(coords)))
                    want.append(P.move(g, coords, ax[-1], bool(reposition))[0])
                    seen["moved"] += 1
                else:  # Agent.move without an axis: the stages behind the shift run all the same
                    ax.append(-1)
                    pts = P.points_of(g)
                    want.append(P.reduce(P.padded(pts - pts.min(0) if reposition else pts, m)))
                    seen["no_axis"] += 1
            blk = cases.add(ENV_MOVE, dtype, m, d, T=p, I=np.stack([subs, ax], 1), out=(n, 0, 0), ipar=(reposition,))
            wants.append((blk, 0, np.array(want, dtype).reshape(count, n), "env_move reposition=%d" % reposition))
        for flags in (0, A.HK_ENV_SCALE_OBSERVATION, A.HK_ENV_IMPROVE_EFFICIENCY,
                      A.HK_ENV_SCALE_OBSERVATION | A.HK_ENV_IMPROVE_EFFICIENCY):
            max_value = int(rng.choice([3, 20, 64, 65, 1000]))
            seen["short" if max_value <= 64 else "long"] += 1
            games, seeds = rng.integers(0, 1 << 63, count), rng.integers(0, 1 << 63, count)
            states, nps = [], []
            for gg, seed in zip(games.tolist(), seeds.tolist()):
                env = E.AgentEnv("choose_first", m, d, dtype=dtype, scale_observation=bool(flags & 1),
                                 improve_efficiency=bool(flags & 16))
                env.reset(E.generator_root(m, d, max_value, seed, gg))
                states.append(env.state.reshape(-1))
                nps.append(E.num_points(env.state))
                if flags == A.HK_ENV_SCALE_OBSERVATION | A.HK_ENV_IMPROVE_EFFICIENCY:
                    seen["second_newton"] += int(E.unreduced(env.state))
            blk = cases.add(ENV_FRESH, dtype, m, d, I=[u64(g) + u64(s) for g, s in zip(games, seeds)], out=(n, 1, 0),
                            ipar=(max_value, flags))
            wants.append((blk, 0, np.array(states, dtype), "env_fresh's state flags=%d max_value=%d" % (flags, max_value)))
            wants.append((blk, 1, np.array(nps, np.int32)[:, None], "env_fresh's count flags=%d" % flags))
    assert seen["no_axis"] > 50 and seen["moved"] > 50 and seen["short"] > 10 and seen["long"] > 10, seen
    got = program(cases)
    for blk, which, want, what in wants:
        assert_bits(got[blk][which], want, what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("host", list(HOST_CODES))
def test_env_host_step_against_the_rules(program, host, dtype):
    rng = np.random.default_rng(37)
    cases, wants = Cases(), []
    seen = dict(legal=0, illegal=0, ended=0, value=0, invalid=0, after_stop=0, running=0)
    for k, (m, d) in enumerate([(1, 2), (2, 2), (5, 2), (5, 3), (20, 3), (5, 4), (33, 4), (20, 5), (64, 6), (5, 7), (20, 7)]):
        for flags in (0, 1, 2, 3):
            thr = (None, 30.0, 0.75, 0.75)[flags] if (k + flags) % 2 else None
            rows = []
            for root in env_roots(rng, 8 if m <= 5 else 3, m, d):
                env = E.HostEnv(host, m, d, dtype=dtype, value_threshold=thr, invalid_move_penalty=-0.125,
                                stop_after_invalid_move=bool(flags & 2), scale_observation=bool(flags & 1))
                env.raise_no_move = False
                env.reset(root)
                was_stopped = False
                for _ in range(5):
                    state, cls = env.state.copy(), env.pending_class
                    act = int(rng.choice(env.coords)) if env.coords and rng.random() < 0.75 else int(rng.integers(-1, d + 1))
                    legal = act in env.coords
                    _, reward, stopped = env.step(act)
                    rows.append((state.reshape(-1), [act, cls], env.state.reshape(-1),
                                 [env.pending_class, int(stopped), int(env.exceed_threshold)], [reward]))
                    seen["legal" if legal else "illegal"] += 1
                    seen["after_stop"] += was_stopped
                    if stopped:
                        seen["ended" if env.ended else "value" if env.exceed_threshold else "invalid"] += 1
                    else:
                        seen["running"] += 1
                    was_stopped |= stopped
            blk = cases.add(ENV_HOST_STEP, dtype, m, d, T=[r[0] for r in rows], I=[r[1] for r in rows],
                            D=[[thr or 0.0, -0.125]] * len(rows), out=(m * d, 3, 1), ipar=(HOST_CODES[host], flags))
            what = "env_host_step %s flags=%d m=%d d=%d" % (host, flags, m, d)
            wants.append((blk, 0, np.array([r[2] for r in rows], dtype), what + ": the state"))
            wants.append((blk, 1, np.array([r[3] for r in rows], np.int32), what + ": class, stopped, exceed"))
            wants.append((blk, 2, np.array([r[4] for r in rows], np.float64), what + ": the reward"))
    assert all(v > 10 for v in seen.values()), seen  # (a host without a list: test_hosts_*, no reduced state has one)
    got = program(cases)
    for blk, which, want, what in wants:
        assert_bits(got[blk][which], want, what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_env_agent_step_against_the_rules(program, dtype):
    rng = np.random.default_rng(41)
    cases, wants = Cases(), []
    seen = dict(no_axis=0, axis=0, ended=0, steps=0, value=0, running=0, reduction=0)
    for k, (m, d) in enumerate([(1, 2), (2, 2), (5, 2), (5, 3), (20, 3), (5, 4), (33, 4), (20, 5), (64, 6), (5, 7), (20, 7)]):
        for flags in (0, 1, 4, 5, 8, 13, 32, 37, 45):
            agent = ("choose_first", "random")[(k + flags) % 2]
            thr = (None, 0.75 if flags & 1 else 30.0)[(k + flags // 4) % 2]
            fixed = (None, -7.0)[k % 2]
            step_threshold = 3
            rows = []
            for root in env_roots(rng, 6 if m <= 5 else 2, m, d):
                seed, gg = int(rng.integers(0, 1 << 63)), int(rng.integers(0, 1 << 63))
                pick = "choose_first" if agent == "choose_first" else (
                    lambda coords, env, seed=seed, gg=gg: E.philox_axis(seed, gg, env.current_step - 1,
                                                                        E.coords_mask(coords), d))
                env = E.AgentEnv(pick, m, d, reposition=bool(flags & 32), dtype=dtype, value_threshold=thr,
                                 step_threshold=step_threshold, fixed_penalty_crossing_threshold=fixed,
                                 stop_at_threshold=bool(flags & 4), scale_observation=bool(flags & 1),
                                 reward_based_on_point_reduction=bool(flags & 8))
                env.reset(root)
                for _ in range(4):
                    state, before = env.state.copy(), E.num_points(env.state)
                    mask = int(rng.integers(0, 1 << d)) | (int(rng.integers(0, 2)) << (d + 1))  # a bit beyond d: ignored
                    _, reward, stopped = env.step(mask)
                    axis = -1 if env.last_action_taken is None else env.last_action_taken
                    rows.append((state.reshape(-1), [mask] + u64(gg) + [env.current_step] + u64(seed),
                                 env.state.reshape(-1), [axis, int(stopped), int(env.exceed_threshold)], [reward]))
                    seen["axis" if axis >= 0 else "no_axis"] += 1
                    seen["reduction"] += before != E.num_points(env.state)
                    if env.ended:
                        seen["ended"] += 1
                    elif stopped:
                        seen["value" if env.exceed_threshold else "steps"] += 1
                    else:
                        seen["running"] += 1
            penalty = float(-step_threshold if fixed is None else fixed)
            blk = cases.add(ENV_AGENT_STEP, dtype, m, d, T=[r[0] for r in rows], I=[r[1] for r in rows],
                            D=[[thr or 0.0, penalty]] * len(rows), out=(m * d, 3, 1),
                            ipar=(AGENT_CODES[agent], flags, step_threshold))
            what = "env_agent_step %s flags=%d m=%d d=%d" % (agent, flags, m, d)
            wants.append((blk, 0, np.array([r[2] for r in rows], dtype), what + ": the state"))
            wants.append((blk, 1, np.array([r[3] for r in rows], np.int32), what + ": axis, stopped, exceed"))
            wants.append((blk, 2, np.array([r[4] for r in rows], np.float64), what + ": the reward"))
    assert all(v > 10 for v in seen.values()), seen
    got = program(cases)
    for blk, which, want, what in wants:
        assert_bits(got[blk][which], want, what)
