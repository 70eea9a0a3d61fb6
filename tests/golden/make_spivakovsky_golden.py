"""
Generate tests/golden/spivakovsky.npz by RUNNING the reference's own Spivakovsky (hironaka/host.py:130-290) and
RandomSpivakovsky (host.py:293-354) through their `select_coord` on ListPoints, and GameHironaka (game.py:84-119)
under Spivakovsky.  Runs only where the reference checkout exists; the .npz is what travels.  Spivakovsky prints while
it selects: its stdout is swallowed.

Selection groups, one per dimension d = 2..6 (states padded with -1 rows at the end, the reference's row order kept):
    sel{d}_states             [N, 20, d]  per value range 0-3 and 0-20: Newton-reduced states (ListPoints after
                                          get_newton_polytope, >= 2 points), raw distinct rows without a zero row, and
                                          Newton-reduced states after ListPoints.rescale() (doubles in [0, 1])
    sel{d}_kind               [N] int8    0 reduced, 1 raw, 2 rescaled reduced
    sel{d}_spivakovsky        [N, d] int8 Spivakovsky().select_coord as a mask (0, 1 or more coordinates)
    sel{d}_random_candidates  [N, C] int32  every subset RandomSpivakovsky(dim=d) can answer with, as bit masks in the
                                          order of its list `answers`, padded with -1: answer k is what select_coord
                                          returns with random.randint of the reference's host module replaced by
                                          "return k", until that raises IndexError
Game group (GameHironaka(Spivakovsky(), ChooseFirstAgent(), scale_observation=False), dim 3, 10 points, values < 20,
16 games): game_start [16, 10, 3]; game_states [T+1, 16, 10, 3]; game_masks [T, 16, 3], the host's subsets, zeros for a
game with fewer than 2 points (the reference's class still answers for a lone point; hironaka_amd's select_coord
empties such games, and nothing moves either way).  T = GAME_STEPS: a game whose host offers one coordinate never moves
again, so the batch never ends; the cap also keeps every coordinate below 2^53 (asserted).  The seed is chosen so that a
game meets a one-coordinate subset, and the maker asserts that the reference leaves the state of such a game unchanged
by that move.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_spivakovsky_golden.py
"""
import contextlib
import io
import os
import sys
import time

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, load_reference, pad_lists  # noqa: E402

SEL_M = 20
PER_KIND = 28  # states per (dim, value range, kind): N = 168
GAME_STEPS = 24
GAME_SEED = 20261021
REDUCED, RAW, RESCALED = 0, 1, 2


def host_points(rows):
    return REF.ListPoints([[list(map(float, r)) for r in rows]], value_threshold=1e8)


def quiet(fn, *args):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args)


def to_mask(coords, d):
    mk = np.zeros(d, np.int8)
    assert all(0 <= int(c) < d for c in coords), coords
    mk[[int(c) for c in coords]] = 1
    return mk


def selection_states(rng, d):
    states, kinds = [], []
    for hi in (3, 20):
        for kind in (REDUCED, RESCALED):
            got = 0
            while got < PER_KIND:
                rows = rng.integers(0, hi + 1, (int(rng.integers(2, 41)), d)).tolist()
                lp = host_points(rows)
                lp.get_newton_polytope()
                if not 2 <= len(lp.points[0]) <= SEL_M:
                    continue
                if kind == RESCALED:
                    lp.rescale()
                states.append([list(r) for r in lp.points[0]])
                kinds.append(kind)
                got += 1
        got = 0
        while got < PER_KIND:  # raw distinct rows, no zero row, in a random order
            rows = np.unique(rng.integers(0, hi + 1, (int(rng.integers(2, SEL_M + 1)), d)), axis=0)
            rows = rows[rows.any(axis=1)]
            if len(rows) < 2:
                continue
            states.append(rows[rng.permutation(len(rows))].tolist())
            kinds.append(RAW)
            got += 1
    return states, kinds


def random_candidates(host, host_module, rows):
    """every answer RandomSpivakovsky can give on one game, in the order of its list"""
    out, keep = [], host_module.random.randint
    try:
        for k in range(1 << 16):
            host_module.random.randint = lambda a, b, k=k: k
            try:
                coords = host.select_coord(host_points(rows))[0]
            except IndexError:
                break
            out.append(sum(1 << int(c) for c in coords))
    finally:
        host_module.random.randint = keep
    return out


def game(ref, seed, b=16, m=10, d=3):
    rng = np.random.default_rng(seed)
    start = rng.integers(0, 20, (b, m, d)).astype(np.float64)
    g = ref.game.GameHironaka(ref.ListPoints(start.tolist(), value_threshold=1e8), ref.host.Spivakovsky(),
                              ref.agent.ChooseFirstAgent(), scale_observation=False)
    states, masks, singles = [pad_lists(g.state.points, m, d)], [], 0
    for _ in range(GAME_STEPS):
        live = [len(p) >= 2 for p in g.state.points]
        quiet(g.step)
        mk = np.stack([to_mask(c, d) if a else np.zeros(d, np.int8) for c, a in zip(g.coord_history[-1], live)])
        masks.append(mk)
        states.append(pad_lists(g.state.points, m, d))
        for i in range(b):
            if live[i] and mk[i].sum() < 2:
                singles += 1
                assert g.move_history[-1][i] is None
                assert np.array_equal(states[-1][i], states[-2][i]), "the reference moved on a one-coordinate subset"
    states = np.stack(states)
    assert states.max() < 2.0 ** 53, "GAME_STEPS lets a coordinate leave the exact integers"
    return start, states, np.stack(masks), singles


def main():
    global REF
    t0 = time.time()
    REF = ref = load_reference()
    rng = np.random.default_rng(20261021)
    rec = {}
    for d in range(2, 7):
        states, kinds = selection_states(rng, d)
        spiv, rand = ref.host.Spivakovsky(), ref.host.RandomSpivakovsky(dim=d)
        rec[f"sel{d}_states"] = pad_lists(states, SEL_M, d)
        rec[f"sel{d}_kind"] = np.asarray(kinds, np.int8)
        masks = np.stack([to_mask(quiet(spiv.select_coord, host_points(s))[0], d) for s in states])
        rec[f"sel{d}_spivakovsky"] = masks
        cands = [random_candidates(rand, ref.host, s) for s in states]
        width = max(len(c) for c in cands)
        assert min(len(c) for c in cands) >= 1
        rec[f"sel{d}_random_candidates"] = np.array([c + [-1] * (width - len(c)) for c in cands], np.int32)
        sizes = np.bincount(masks.sum(1), minlength=d + 1).tolist()
        print(f"sel{d}: {len(states)} states, subset sizes {sizes}, up to {width} candidates ({time.time() - t0:.1f} s)")
    seed = GAME_SEED
    while True:
        start, states, masks, singles = game(ref, seed)
        if singles:
            break
        seed += 1
    rec["game_start"], rec["game_states"], rec["game_masks"] = start, states, masks
    rec["game_seed"] = np.asarray(seed)
    print(f"game: seed {seed}, {len(masks)} steps, {singles} one-coordinate moves, "
          f"{int((states[-1][:, 1, 0] >= 0).sum())} games alive at the end, max {states.max():.0f}")
    np.savez_compressed(os.path.join(OUT, "spivakovsky.npz"), **rec)
    print(f"wrote spivakovsky.npz in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
