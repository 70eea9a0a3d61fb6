"""Spivakovsky's host (hironaka/host.py:130-290) and RandomSpivakovsky (host.py:293-354) restated in plain Python on
one padded state [m, d] in list semantics: a row is a point when its coordinate 0 is >= 0, rows are read in row order,
holes may sit anywhere.  Both answer with bit masks (bit k <-> coordinate k), as hk_spivakovsky_select does.  Values
are Python floats (doubles), sums run left to right from 0 (CPython 3.10's sum; the compensated sum of 3.12 is not
followed).  tests/test_spivakovsky_rules.py holds these rules against the fixture made by running the reference's own
classes (tests/golden/make_spivakovsky_golden.py)."""
import itertools
import math

import numpy as np

from oracle.np_oracle import philox4x32

ONE = 0.999  # the reference's "reaches 1" (host.py:215, 258)
INF = float("inf")


def _div(a, b):
    """a / b as IEEE has it, where Python raises"""
    if b == 0.0 and b == b:
        if a != a or a == 0.0:
            return float("nan")
        neg = (a < 0) != (math.copysign(1.0, b) < 0)
        return -INF if neg else INF
    return a / b


def live_rows(state):
    return [[float(x) for x in row] for row in state if row[0] >= 0]


def rule_spivakovsky(state, trace=None):
    """the mask of Spivakovsky._select_coord on one game; 0 for fewer than 2 points.  `trace`, a dict, receives
    levels (the levels completed), last ("none": not run, "set": it returned a subset, "empty": it found none) and
    emptied (alive ran empty)"""
    v = live_rows(state)
    d = len(state[0])
    if trace is None:
        trace = {}
    trace.update(levels=0, last="none", emptied=False)
    if len(v) < 2:
        return 0
    alive, act, res = list(range(len(v))), list(range(d)), 0
    for _ in range(d):
        if not alive:
            break
        mn = {}
        for k in range(d):
            for n, i in enumerate(alive):
                if n == 0 or v[i][k] < mn[k]:
                    mn[k] = v[i][k]
        mv = {i: {k: v[i][k] - mn[k] for k in act} for i in alive}
        if any(all(mv[i][k] == 0 for k in act) for i in alive):
            break
        md, S = INF, set()
        for i in alive:
            s = 0.0
            for k in act:
                s += mv[i][k]
            if s < md:
                md, S = s, set()
            if s == md:
                S |= {k for k in act if mv[i][k] > 0}
        res |= sum(1 << k for k in S)
        I = [k for k in act if k not in S]
        stay = []
        for i in alive:
            q = {k: _div(mv[i][k], md) for k in act}
            t = 0.0
            for k in sorted(S):
                t += q[k]
            if t < ONE:
                stay.append(i)
                for k in I:
                    v[i][k] = _div(q[k], 1.0 - t)
        alive = stay
        if I:
            act = I
        trace["levels"] += 1
    trace["emptied"] = not alive
    if not alive:
        return res
    trace["last"] = "empty"
    for r in range(1, len(act)):
        for comb in itertools.combinations(act, r):
            permissible = True
            for i in alive:
                s = 0.0
                for k in comb:
                    s += v[i][k]
                if s < ONE:
                    permissible = False
            if permissible:
                trace["last"] = "set"
                return res | sum(1 << k for k in comb)
    return res


def random_spivakovsky_candidates(state):
    """RandomSpivakovsky's candidates on one game, the reference built with dim = d: the masks of >= 2 coordinates that
    meet every support (x != 0), of the smallest such size, ascending.  [] for fewer than 2 points or when nothing meets
    every support (a zero row)."""
    rows = live_rows(state)
    d = len(state[0])
    if len(rows) < 2:
        return []
    supports = {sum(1 << k for k in range(d) if row[k] != 0) for row in rows}
    hits = [c for c in range(3, 1 << d) if bin(c).count("1") >= 2 and all(c & s for s in supports)]
    if not hits:
        return []
    size = min(bin(c).count("1") for c in hits)
    return [c for c in hits if bin(c).count("1") == size]


def rule_random_spivakovsky(state, word):
    """the mask hk_spivakovsky_select gives for the Philox word `word`: candidate number (word * n) >> 32, 0 without
    candidates"""
    cands = random_spivakovsky_candidates(state)
    return cands[(int(word) * len(cands)) >> 32] if cands else 0


def mask_bits(mask, d):
    return [(int(mask) >> k) & 1 for k in range(d)]


STREAM = 5  # kStreamRandomSpivakovsky (hk_common.h)


def random_words(seed, game_offset, count, step):
    """the Philox word of RandomSpivakovsky's draw for the games game_offset .. game_offset + count"""
    game = np.arange(count, dtype=np.uint64) + np.uint64(game_offset)
    return philox4x32(game & np.uint64(0xFFFFFFFF), game >> np.uint64(32), step, STREAM, seed)[0]


def three_row_states(d, every=1):
    """the 3-row states whose rows are a hole (all -1) or a point of {0, 1, 2}^d, every `every`-th, as one array"""
    rows = [(-1.0,) * d] + list(itertools.product((0.0, 1.0, 2.0), repeat=d))
    return np.array(list(itertools.islice(itertools.product(rows, repeat=3), 0, None, every)))
