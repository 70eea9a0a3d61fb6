"""Which level of a staircase a wave is on, and batches that walk every level.

The register-resident kernels have one straight-line body per bucket of slots per lane (a LEVEL).  A wave enters on the
level of its widest game, steps there, re-deals its rows down when the widest game fits fewer slots, and publishes on
the level its last step ran on.  This module restates the three ladders and that rule in plain Python, so that a test
can say from the ORACLE's row counts alone which levels its inputs reach -- nothing here is read back from the kernels.
No GPU, no torch."""
import functools

import numpy as np

# family -> (lanes per game, games per wave of 64 lanes)
FAMILIES = {"four": (4, 16), "two": (2, 32), "one": (1, 64)}

# the shapes each rollout family is specialised for
ROLLOUT_SHAPES = {
    "four": [(10, 3), (20, 3), (20, 4), (50, 4)],                          # hk_quad_kernel.h: HK_QUAD_SPECS
    "two": [(20, 3), (10, 3), (5, 3), (16, 3), (8, 4), (20, 4)],          # test_forced_rollout_families_match_oracle
    "one": [(4, 3), (5, 3), (10, 3), (16, 3), (20, 3), (8, 4), (20, 4)],  # hk_fast_kernel.h: HK_FAST_SPECS
}
STEPS = (0, 1, 2, 3, 5)
# the configurations of test_gpu_step_loops.CONFIGS that the level tests run
CONFIG_NAMES = ("jax7", "jax15", "torch7", "list", "list_compact", "zeillinger")


def next_bucket(family, nb):
    if family == "four":  # hk_quad_kernel.h:59, QuadGeom::next_bucket
        return nb + 1 if nb < 6 else (nb + 2 if nb < 10 else nb + 3)
    if family == "two":   # hk_duo_kernel.h:233, DuoLadder::next_bucket
        return nb + 1 if nb < 6 else nb + 2
    if family == "one":   # hk_fast_rows.h:422, RowLadder::next_bucket
        return nb + 1 if nb < 8 else nb + 2
    raise ValueError(family)


def top_level(family, m):
    """slots per lane of the widest body: QuadGeom::R = ceil(M / 4) (hk_quad_kernel.h:42), DuoGeom::CH = (C + 1) / 2
    (hk_duo_kernel.h:66), FastGeom::C = min(M, 32) (hk_fast_kernel.h:55)"""
    lanes = FAMILIES[family][0]
    rows = m if family == "four" else min(m, 32)
    return -(-rows // lanes)


def ladder(family, m):
    """the levels from 1 up: the buckets below the top, then the top itself (hk_fast_rows.h:441-456, Levels: from the
    top NB down to the largest bucket below it)"""
    top, out, nb = top_level(family, m), [], 1
    while nb < top:
        out.append(nb)
        nb = next_bucket(family, nb)
    return out + [top]


def slots(family, n):
    """slots per lane that n live rows take (a wave of empty games still runs the one-slot body)"""
    lanes = FAMILIES[family][0]
    return max(1, -(-int(n) // lanes))


def level_of(family, m, n):
    s = slots(family, n)
    for nb in ladder(family, m):
        if s <= nb:
            return nb
    raise ValueError(f"{n} rows do not fit {family} lanes at m={m}")


def live_rows(states):
    """[..., m, d] -> [...]: rows without a negative coordinate (canonical states: the padding value is negative)"""
    return (np.asarray(states) >= 0).all(axis=-1).sum(axis=-1).astype(np.int32)


def at_fixed_point(states):
    """[..., m, d] -> [...] bool: the game is down to one point at the origin, or to none"""
    s = np.asarray(states)
    live = (s >= 0).all(axis=-1)
    return (live.sum(axis=-1) <= 1) & ~(live & (s != 0).any(axis=-1)).any(axis=-1)


def level_path(num_points, family, m, T, still=None):
    """num_points [T + 1, B]: the live rows of every game before step 0, ..., before step T - 1 and at the end.
    still [T + 1, B] (optional): at_fixed_point of the same states -- with it the path ends where the one-slot loop
    leaves at the wave's fixed point; without it that loop is taken to run all its steps (on the same level either way).
    Returns one dict per wave: entered (level or None), steps (the level of every step played), redeals ((from, to)
    per re-deal, in order; from == to where the slots shrink inside one bucket), publish (level or None).
    The rule (hk_quadroll_kernel.h:721-792, hk_duo_kernel.h:1101-1212, hk_fast_kernel.h:605-647): the slots per lane
    follow the widest game and never grow; after step t the rows are re-dealt only if t + 1 < T; the image is built on
    the level of the last step; T = 0 publishes without entering a level; on one slot there is no re-deal, only the
    exit once every game of the wave sits at its fixed point (tested while t + 1 < T)."""
    num_points = np.asarray(num_points)
    assert num_points.shape[0] == T + 1
    games = FAMILIES[family][1]
    out = []
    for g0 in range(0, num_points.shape[1], games):
        n = num_points[:, g0:g0 + games]
        if T == 0:
            out.append(dict(entered=None, steps=[], redeals=[], publish=None))
            continue
        s = slots(family, n[0].max())
        entered = level_of(family, m, n[0].max())
        steps, redeals = [], []
        for t in range(T):
            lvl = [nb for nb in ladder(family, m) if s <= nb][0]
            steps.append(lvl)
            if t + 1 >= T:
                break
            if lvl == 1:
                if still is not None and still[t + 1, g0:g0 + games].all() and (n[t + 1] < 2).all():
                    break
            else:
                s_new = slots(family, n[t + 1].max())
                if s_new < s:
                    redeals.append((lvl, level_of(family, m, n[t + 1].max())))
                    s = s_new
        out.append(dict(entered=entered, steps=steps, redeals=redeals, publish=steps[-1]))
    return out


def coverage(paths):
    """the union over waves (and cases: concatenate the lists): stepped, published, entered, redeals"""
    cov = dict(stepped=set(), published=set(), entered=set(), redeals=set())
    for p in paths:
        cov["stepped"].update(p["steps"])
        cov["redeals"].update(p["redeals"])
        if p["publish"] is not None:
            cov["published"].add(p["publish"])
        if p["entered"] is not None:
            cov["entered"].add(p["entered"])
    return cov


def missing(cov, family, m):
    """what a coverage set lacks of: every level stepped on and published on, every adjacent re-deal, and a re-deal
    that skips a level where the ladder has three or more; a list of names, empty when nothing is missing"""
    lad = ladder(family, m)
    miss = [f"step on {nb}" for nb in lad if nb not in cov["stepped"]]
    miss += [f"publish on {nb}" for nb in lad if nb not in cov["published"]]
    miss += [f"re-deal {hi}->{lo}" for lo, hi in zip(lad, lad[1:]) if (hi, lo) not in cov["redeals"]]
    if len(lad) >= 3 and not any(lad.index(hi) - lad.index(lo) >= 2 for hi, lo in cov["redeals"]):
        miss.append("a re-deal that skips a level")
    return miss


# ---- batches --------------------------------------------------------------------------------------------------------
def compositions(rng, n, total, d):
    """n distinct rows of d non-negative integers summing to `total` (stars and bars): an antichain"""
    seen = set()
    while len(seen) < n:
        cuts = np.sort(rng.choice(total + d - 1, size=d - 1, replace=False))
        parts = np.diff(np.concatenate(([-1], cuts, [total + d - 1]))) - 1
        seen.add(tuple(int(x) for x in parts))
    rows = np.array(sorted(seen), dtype=np.float32).reshape(n, d)
    return rows[rng.permutation(n)]


def place(rng, game, n, total):
    """n antichain rows at scattered row indices of one game [m, d] (the rest keeps the padding value)"""
    m, d = game.shape
    if n > 0:
        game[np.sort(rng.choice(m, size=n, replace=False))] = compositions(rng, n, total, d)


@functools.lru_cache(maxsize=None)
def batch(m, d, family, S, seed):
    """placed_width_states, built once per process and read-only"""
    p = placed_width_states(m, d, family, S, seed)
    p.setflags(write=False)
    return p


PAIR_WAVES = (1, 1, 2, 4)  # games that hold the easy pair in each of the last waves


def placed_width_states(m, d, family, S, seed, pad=-1.0):
    """[(2 * m + 4) * G, m, d] float32, G the family's games per wave; live rows are distinct compositions of S into d
    parts.
    Waves 0 .. m - 1, the crowd: the widest game of wave w (somewhere in the wave) has exactly m - w live rows, the
    others a random number up to that.
    Waves m .. 2 m - 1, the solo waves, hand-built for the narrow transitions a crowd of G games seldom makes (its
    widest game shrinks slowly): one game of m - (w - m) rows, the others at most one row -- the wave comes down as that
    one game does.
    Waves 2 m .. 2 m + 3, the pair waves: 1, 1, 2 and 4 games hold the two rows (S, 0, ..) and (S - 1, 1, 0, ..), which any
    subset with coordinates 0 and 1 and either of them as the axis reduces to one row; the other games are empty -- the
    wave drops from two rows to one within a few steps whatever the dimension."""
    games = FAMILIES[family][1]
    rng = np.random.default_rng(seed)
    p = np.full(((2 * m + len(PAIR_WAVES)) * games, m, d), pad, dtype=np.float32)
    for k, holders in enumerate(PAIR_WAVES):
        if m < 2:
            break
        for i in rng.choice(games, size=holders, replace=False):
            rows = np.sort(rng.choice(m, size=2, replace=False))
            game = p[(2 * m + k) * games + int(i)]
            game[rows] = 0.0
            game[rows[0], 0], game[rows[1], 0], game[rows[1], 1] = S, S - 1, 1
    for w in range(2 * m):
        solo = w >= m
        widest = m - (w % m)
        lead = int(rng.integers(0, games))
        for i in range(games):
            if i == lead:
                n = widest
            elif solo:
                n = int(rng.integers(0, 2)) if widest > 3 else 0
            else:
                n = int(rng.integers(0, widest + 1))
            place(rng, p[w * games + i], n, S)
    return p


def widest_per_wave(states, family):
    games = FAMILIES[family][1]
    n = live_rows(states)
    return [int(n[g:g + games].max()) for g in range(0, len(n), games)]


def sums_for(m):
    """S = 12: duplicates after shifts, short games; S = 40: shifted coordinates stay <= 126 (the packed test's range);
    S = 500, where a game can hold more than 32 rows: the float two-level test"""
    return (12, 40, 500) if m > 32 else (12, 40)


# (family, shape) -> salt of the seeds, where salt 0 left a transition out under some configuration: chosen with the oracle
# on the CPU (tests/test_level_cases.py fails by name if a changed seed drops a level)
SEED_SALT = {("two", (5, 3)): 1, ("one", (20, 3)): 1, ("one", (8, 4)): 2, ("one", (20, 4)): 3}


def rollout_cases(family, shape, salt=None):
    """(S, T, seed of the batch, seed of the policies) for every rollout case of a (family, shape): one batch per S"""
    m, _ = shape
    salt = SEED_SALT.get((family, tuple(shape)), 0) if salt is None else salt
    return [(S, T, 100 + S + 10000 * salt, 1000 + 7 * T + S + 10000 * salt) for S in sums_for(m) for T in STEPS]


_traces = {}


def trace(family, shape, cfg_name, cfg, case):
    """One rollout case on the C oracle, recorded: (initial states, final states, records, level path per wave).
    cfg: (flags, host policy, agent policy, stages, padding value), an entry of test_gpu_step_loops.CONFIGS.
    Computed once per process and shared."""
    key = (family, tuple(shape), cfg_name, case)
    if key not in _traces:
        from oracle import c_oracle as CO
        (m, d), (S, T, batch_seed, policy_seed) = shape, case
        flags, host_policy, agent, stages, pad = cfg
        p0 = batch(m, d, family, S, batch_seed)
        final, rec = CO.rollout(p0, T, policy_seed, game_offset=3, host_policy=host_policy, agent_policy=agent,
                                stages=stages, flags=flags, padding_value=pad, record=True)
        states = np.concatenate([rec["obs"], final[None]], axis=0)
        paths = level_path(live_rows(states), family, m, T, at_fixed_point(states))
        _traces[key] = (p0, final, rec, paths)
    return _traces[key]


def family_paths(family, shape, cfg_name, cfg):
    """the level paths of every rollout case of a (family, shape, configuration), and those of each S alone"""
    paths, by_sum = [], {}
    for case in rollout_cases(family, shape):
        p = trace(family, shape, cfg_name, cfg, case)[3]
        paths += p
        by_sum.setdefault(case[0], []).extend(p)
    return paths, by_sum


def missing_at_50_4(paths, by_sum):
    """the four-lane kernel at (50,4): what the issue of the untested 10-slot level names, beyond `missing`"""
    cov = coverage(paths)
    miss = [] if 10 in cov["entered"] else ["entry on 10"]
    miss += [f"re-deal {hi}->{lo}" for hi, lo in ((13, 10), (10, 8)) if (hi, lo) not in cov["redeals"]]
    miss += [f"step on 10 with S = {S}" for S in (40, 500) if 10 not in coverage(by_sum.get(S, []))["stepped"]]
    return miss


def describe(paths, wave):
    p = paths[wave]
    return f"wave {wave}: entered {p['entered']}, steps {p['steps']}, re-deals {p['redeals']}, publish {p['publish']}"


def first_wave_of_width(states, family, lo, hi):
    """index of the first wave whose widest game has lo .. hi live rows"""
    for w, n in enumerate(widest_per_wave(states, family)):
        if lo <= n <= hi:
            return w
    raise ValueError(f"no wave of width {lo}..{hi}")
