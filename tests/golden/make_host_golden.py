"""
Generate tests/golden/hosts.npz by RUNNING the reference's own hosts (hironaka/host.py): ZeillingerLex (116-127),
WeakSpivakovsky (357-378), WeakSpivakovskyMinHitting (381-427), and Zeillinger (54-95) as a control, through their
`select_coord` on ListPoints, their GameHironaka (game.py:84-119) and util/search.py:9-32 `search_depth`.  Runs only
where the reference checkout exists; the .npz is what travels.

Selection groups, one per dimension d = 2..6 (states padded with -1 rows at the end, the reference's row order kept):
    sel{d}_states     [N, 20, d]   Newton-reduced states (ListPoints after get_newton_polytope, >= 2 points) and raw
                                   distinct rows without a zero row (ZeillingerLex depends on the row order), values
                                   0-3 (many zeros, many tied supports) and 0-20; sel3 starts with test/testGame.py:45-52
    sel{d}_{host}     [N, d] int8  select_coord as a mask; all -1 where the reference returned no subset for the game
    sel{d}_reduced    [N] bool     the state is Newton-reduced
Game groups (GameHironaka vs ChooseFirstAgent, scale_observation=False, dim 3, 10 points, values < 20, 16 games):
    game_{host}_start [16, 10, 3]; _states [T+1, 16, 10, 3]; _masks [T, 16, 3] (the host's subsets); a step cap of
    GAME_STEPS, since a weak host's game may not end
Depth groups (seeded raw roots, dims 3 and 4; trees over NODE_CAP nodes are dropped, and the count of roots tried is
kept): depth_{host}{d}_roots [N, m, d], _depth [N], _nodes [N] (host.select_coord calls), _tried (scalar)

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_host_golden.py
"""
import os
import sys
import time

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _load, load_reference, pad_lists  # noqa: E402
from make_search_depth_golden import _TooLarge, counting, pad  # noqa: E402

HOSTS = {"zeillinger_lex": "ZeillingerLex", "weak_spivakovsky": "WeakSpivakovsky",
         "weak_spivakovsky_min_hitting": "WeakSpivakovskyMinHitting", "zeillinger": "Zeillinger"}
SEL_M = 20
PER_KIND = 40  # states per (dim, value range, reduced / raw)
GAME_STEPS = 40
NODE_CAP = 5000
DEPTH_TRIES = {"zeillinger_lex": 60, "weak_spivakovsky": 40, "weak_spivakovsky_min_hitting": 40}


def select_mask(host, rows, d):
    """the reference's subset for one game as a mask, all -1 when it returns none for the game"""
    try:
        out = host.select_coord(host_points(rows))
    except (AssertionError, IndexError):
        out = []
    mk = np.full(d, -1, np.int8)
    if len(out) == 1 and len(out[0]) > 0 and all(0 <= int(c) < d for c in out[0]):
        mk[:] = 0
        mk[[int(c) for c in out[0]]] = 1
    return mk


def host_points(rows):
    return REF.ListPoints([[list(map(float, r)) for r in rows]], value_threshold=1e8)


def selection_states(rng, d):
    states, reduced = [], []
    if d == 3:
        states.append([[0, 1, 2], [2, 1, 0]])  # test/testGame.py:45-52
        reduced.append(False)
    for hi in (3, 20):
        got = 0
        while got < PER_KIND:  # Newton-reduced
            rows = rng.integers(0, hi + 1, (int(rng.integers(2, 41)), d)).tolist()
            lp = host_points(rows)
            lp.get_newton_polytope()
            red = lp.points[0]
            if 2 <= len(red) <= SEL_M:
                states.append([list(r) for r in red])
                reduced.append(True)
                got += 1
        got = 0
        while got < PER_KIND:  # raw distinct rows, no zero row, in a random order
            rows = np.unique(rng.integers(0, hi + 1, (int(rng.integers(2, SEL_M + 1)), d)), axis=0)
            rows = rows[rows.any(axis=1)]
            if len(rows) < 2:
                continue
            states.append(rows[rng.permutation(len(rows))].tolist())
            reduced.append(False)
            got += 1
    return states, reduced


def games(ref, rng, host_cls, b=16, m=10, d=3):
    start = rng.integers(0, 20, (b, m, d)).astype(np.float64)
    game = ref.game.GameHironaka(ref.ListPoints(start.tolist(), value_threshold=1e8), host_cls(), ref.agent.ChooseFirstAgent(),
                                 scale_observation=False)
    states, masks = [pad_lists(game.state.points, m, d)], []
    alive = not game.stopped
    while alive and len(masks) < GAME_STEPS:
        alive = game.step()
        mk = np.zeros((b, d), np.int8)
        for g, c in enumerate(game.coord_history[-1]):
            mk[g, c] = 1
        masks.append(mk)
        states.append(pad_lists(game.state.points, m, d))
    return start, np.stack(states), np.stack(masks)


def depth_roots(search_depth, host_cls, rng, tries, m_hi, d):
    roots, depth, nodes = [], [], []
    for _ in range(tries):
        rows = rng.integers(0, 21, (int(rng.integers(2, m_hi + 1)), d)).tolist()
        host = counting(host_cls, NODE_CAP)()
        try:
            r = search_depth(host_points(rows), host)
        except _TooLarge:
            continue
        except (AssertionError, IndexError):  # a root the reference's host returns nothing for
            continue
        roots.append(rows)
        depth.append(r)
        nodes.append(host.calls)
    return pad(roots, m_hi, d), np.asarray(depth, np.int64), np.asarray(nodes, np.int64)


def main():
    global REF
    t0 = time.time()
    REF = ref = load_reference()
    search = _load("hironaka.util.search", "hironaka/util/search.py")
    hosts = {k: getattr(ref.host, v)() for k, v in HOSTS.items()}
    rng = np.random.default_rng(20261016)
    rec = {}
    for d in range(2, 7):
        states, reduced = selection_states(rng, d)
        rec[f"sel{d}_states"] = pad_lists(states, SEL_M, d)
        rec[f"sel{d}_reduced"] = np.asarray(reduced)
        for k, h in hosts.items():
            rec[f"sel{d}_{k}"] = np.stack([select_mask(h, s, d) for s in states])
        print(f"sel{d}: {len(states)} states, no subset: "
              f"{ {k: int((rec[f'sel{d}_{k}'][:, 0] < 0).sum()) for k in hosts} } ({time.time() - t0:.1f} s)")
    for k in ("zeillinger_lex", "weak_spivakovsky"):
        start, states, masks = games(ref, rng, getattr(ref.host, HOSTS[k]))
        rec[f"game_{k}_start"], rec[f"game_{k}_states"], rec[f"game_{k}_masks"] = start, states, masks
        print(f"game {k}: {len(masks)} steps, {int((states[-1][:, 1, 0] >= 0).sum())} games alive at the end")
    for k, tries in DEPTH_TRIES.items():
        for d, m_hi in ((3, 10), (4, 8)):
            roots, depth, nodes = depth_roots(search.search_depth, getattr(ref.host, HOSTS[k]), rng, tries, m_hi, d)
            g = f"depth_{k}{d}"
            rec[f"{g}_roots"], rec[f"{g}_depth"], rec[f"{g}_nodes"] = roots, depth, nodes
            rec[f"{g}_tried"] = np.asarray(tries)
            print(f"{g}: {len(depth)} of {tries} roots within {NODE_CAP} nodes; depth max "
                  f"{depth.max() if len(depth) else '-'} ({time.time() - t0:.1f} s)")
    np.savez_compressed(os.path.join(OUT, "hosts.npz"), **rec)
    print(f"wrote hosts.npz in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
