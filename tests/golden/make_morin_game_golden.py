"""
Generate tests/golden/morin_game.npz by RUNNING the reference's own `GameMorin` (hironaka/game.py:122-154) with its own
`AgentMorin`, ListPoints and hosts, `scale_observation=False`, `np.random` seeded per game.  Runs only where the
reference checkout exists; the resulting .npz is what travels, and it holds data only.

The files are loaded one by one as make_golden.py does (the package __init__ files import jax).

Layout (G games, S moves in all; tests/morin_rules.py load_games unpacks it):
    names        [G] str
    hosts        [5] str      the host keys, indexed by meta's host column
    meta         [G, 10] int64 m, d, the distinguished row of the root, np.random's seed, host, raised (1: the reference
                              raised at the move after the recorded ones), rows after Game.__init__, the distinguished
                              row after Game.__init__ (-1: lost there; the game is then not stepped), moves recorded,
                              stopped (0: still running when the recording ended, 1: state.ended, 2: no contribution)
    roots        flat         the roots as given, m*d each
    root_states  flat         the states after Game.__init__'s get_newton_polytope
    lists        [S, 7]       the host's list at every move in the reference's order, padded with -1
    axes         [S]          the agent's axis
    weights      [S, 7]       the weights after the move, padded with -1
    dists        [S]          the distinguished row after the move, -1 for None
    counts       [S]          the rows after the move
    states       flat         the states after every move
    de_*                      the reference's ListPoints run of test/testPoints.py:152-172 test_distinguished_elements:
                              the root, the shifts (subset mask and axis) and, after each of the three
                              get_newton_polytope calls, the state and the index

Roots: thom_points_homogeneous(3) and (4) and test/testThom.py:94-114's root, distinguished point last; seeded roots of
dim 2..7 with 2..9 points; roots with a twin of the distinguished row.  Every root is played under each of the five
deterministic hosts and under SEEDS.  A game is recorded until it stops, MAX_MOVES moves, or a coordinate reaches
VALUE_CAP; a move at which the reference raises (a host without a move) ends the recording with `raised` set, the
moves before it kept.  At most 5 % of the games may raise.

The plain restatement (tests/morin_rules.py play, here with the reference's own hosts and the recorded axes at ties)
follows every game move for move before anything is written.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_morin_game_golden.py
"""
import os
import sys
import time

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from make_golden import OUT, _load, load_reference  # noqa: E402
from morin_rules import ENDED, NO_CONTRIBUTION, RUNNING, morin_axis, play, tracked_newton  # noqa: E402
from search_rules import rows_of  # noqa: E402

HOSTS = {"zeillinger": "Zeillinger", "all_coord": "AllCoordHost", "zeillinger_lex": "ZeillingerLex",
         "weak_spivakovsky": "WeakSpivakovsky", "weak_spivakovsky_min_hitting": "WeakSpivakovskyMinHitting"}
SEEDS = (0, 1, 2)
MAX_MOVES = 100
VALUE_CAP = 2 ** 22
TWINS = ([[1, 2], [1, 2], [3, 0]], [[2, 1, 0], [0, 0, 3], [2, 1, 0]], [[1, 1, 2, 0], [0, 3, 0, 1], [1, 1, 2, 0], [2, 0, 0, 2]])


def run(ref, host_name, rows, dist, seed):
    """one reference game: (root state, root dist, moves [(list, axis, state, weights, dist)], raised, stopped)"""
    np.random.seed(seed)
    host = getattr(ref.host, HOSTS[host_name])()
    pts = ref.ListPoints([[list(r) for r in rows]], distinguished_points=[dist])
    game = ref.game.GameMorin(pts, host, ref.agent.AgentMorin(), scale_observation=False)
    root_state = rows_of(game.state.points[0])
    root_dist = game.state.distinguished_points[0]
    moves, raised = [], 0
    if root_dist is None:
        return root_state, -1, moves, raised, 2
    while not game.stopped and len(moves) < MAX_MOVES and max(map(max, game.state.points[0])) < VALUE_CAP:
        try:
            game.step()
        except Exception:  # noqa: BLE001 -- the reference's own failures: a host without a move
            raised = 1
            break
        nd = game.state.distinguished_points[0]
        moves.append(([int(c) for c in game.coord_history[-1][0]], int(game.move_history[-1][0]),
                      rows_of(game.state.points[0]), [int(v) for v in game.weights[0]], -1 if nd is None else int(nd)))
    stopped = 0
    if game.stopped and not raised:
        stopped = 2 if game.state.distinguished_points[0] is None else 1
    return root_state, int(root_dist), moves, raised, stopped


def follow(ref, host_name, rows, dist, got):
    """the restatement, with the reference's own host and the recorded axes at ties, must give the same game"""
    root_state, root_dist, moves, raised, stopped = got
    host = getattr(ref.host, HOSTS[host_name])()
    st, nd = tracked_newton(np.asarray(rows), dist)
    assert rows_of(st) == root_state and nd == root_dist, (host_name, rows, dist)
    w, axes = [1] * len(rows[0]), []
    for coords, a, _, w2, _ in moves:
        rule = morin_axis(coords, w, "random")  # None at a tie: the recorded axis is fed in
        assert a in coords and rule in (None, a), (host_name, rows, dist)
        axes.append(a if rule is None else -1)
        w = w2
    mine = play(rows, [1] * len(rows[0]), dist, lambda s: host.select_coord(ref.ListPoints([rows_of(s)]))[0],
                len(moves), axes=axes, tie="random", reduce_root=True)
    assert mine.length == len(moves), (host_name, rows, dist, mine.length, len(moves))
    for (coords, a, state, w2, d2), (s3, w3, d3), a3 in zip(moves, mine.history, mine.axes):
        assert rows_of(s3) == state and w3 == w2 and d3 == d2 and a3 == a, (host_name, rows, dist)
    want = {0: RUNNING, 1: ENDED, 2: NO_CONTRIBUTION}[stopped]
    assert mine.outcome == want, (host_name, rows, dist, mine.outcome, want)


def main():
    t0 = time.time()
    ref = load_reference()
    thom = _load("hironaka.src._thom_fn", "hironaka/src/_thom_fn.py")
    host_keys = list(HOSTS)
    names, meta = [], []
    flat = {k: [] for k in ("roots", "root_states", "lists", "axes", "weights", "dists", "counts", "states")}
    seen = {"ended": 0, "lost": 0, "running": 0, "lost_at_root": 0}

    def add(name, rows, dist):
        for host_name in HOSTS:
            for seed in SEEDS:
                got = run(ref, host_name, rows, dist, seed)
                follow(ref, host_name, rows, dist, got)
                root_state, root_dist, moves, raised, stopped = got
                names.append(f"{name}_{host_name}_s{seed}")
                meta.append([len(rows), len(rows[0]), dist, seed, host_keys.index(host_name), raised, len(root_state),
                             root_dist, len(moves), stopped])
                flat["roots"] += [v for r in rows for v in r]
                flat["root_states"] += [v for r in root_state for v in r]
                for coords, a, state, w, nd in moves:
                    flat["lists"].append(coords + [-1] * (7 - len(coords)))
                    flat["axes"].append(a)
                    flat["weights"].append(w + [-1] * (7 - len(w)))
                    flat["dists"].append(nd)
                    flat["counts"].append(len(state))
                    flat["states"] += [v for r in state for v in r]
                seen["ended"] += stopped == 1
                seen["lost"] += stopped == 2 and root_dist >= 0
                seen["running"] += stopped == 0 and not raised
                seen["lost_at_root"] += root_dist < 0

    for order in (3, 4):
        rows = [[int(v) for v in r] for r in thom.thom_points_homogeneous(order)]
        add(f"thom{order}", rows, len(rows) - 1)
    tp = [[int(v) for v in r] for r in thom.thom_points(4)]
    original = [[r[0] + sum(r[1:]) - 4] + r[1:] for r in tp]  # test/testThom.py:95-101
    add("thom_original", original, len(original) - 1)
    for j, rows in enumerate(TWINS):
        add(f"twin{j}", rows, 0)
    rng = np.random.default_rng(20261017)
    for d in (2, 3, 4, 5, 6, 7):
        for j in range(3):
            rows = rng.integers(0, 8, (int(rng.integers(2, 10)), d)).tolist()
            add(f"d{d}_{j}", rows, int(rng.integers(0, len(rows))))
        rows = rng.integers(0, 5, (int(rng.integers(3, 8)), d)).tolist()
        rows.append(list(rows[1]))  # a twin of the distinguished row
        add(f"d{d}_twin", rows, 1)

    meta = np.asarray(meta, np.int64)
    raised = int(meta[:, 5].sum())
    assert raised * 20 <= len(names), (raised, len(names))
    assert seen["ended"] and seen["lost"] and seen["lost_at_root"], seen
    assert set(meta[:, 1]) == {2, 3, 4, 5, 6, 7} and meta[:, 8].max() > 3

    # test/testPoints.py:152-172
    de_root = [[7, 5, 3, 8], [8, 1, 8, 18], [8, 3, 17, 8], [11, 11, 1, 19], [11, 12, 18, 6], [16, 11, 5, 6]]
    de_shifts = [[[0, 1], 0], [[0, 2], 0], [[2, 3], 2], [[0, 1], 1]]
    pts = ref.ListPoints([[list(r) for r in de_root]], distinguished_points=[2])
    de_states, de_counts, de_dists = [], [], []

    def snap():
        pts.get_newton_polytope()
        nd = pts.distinguished_points[0]
        de_states.extend(v for r in pts.points[0] for v in r)
        de_counts.append(len(pts.points[0]))
        de_dists.append(-1 if nd is None else nd)

    snap()
    pts.shift([de_shifts[0][0]], [de_shifts[0][1]])
    snap()
    for coords, a in de_shifts[1:]:
        pts.shift([coords], [a])
    snap()
    assert de_dists[2] == -1 and de_dists[0] >= 0 and de_dists[1] >= 0

    rec = {k: np.asarray(v, np.int32) for k, v in flat.items()}
    rec.update(names=np.asarray(names), hosts=np.asarray(host_keys), meta=meta,
               de_root=np.asarray(de_root, np.int32), de_states=np.asarray(de_states, np.int32),
               de_shifts=np.asarray([[int(k in c) for k in range(4)] + [a] for c, a in de_shifts], np.int32),
               de_counts=np.asarray(de_counts, np.int32), de_dists=np.asarray(de_dists, np.int32))
    path = os.path.join(OUT, "morin_game.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(OUT, "search_morin.npz"))
    print(f"wrote morin_game.npz: {len(names)} games, {len(flat['axes'])} moves, {raised} raised, {seen}, "
          f"{os.path.getsize(path)} bytes in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
