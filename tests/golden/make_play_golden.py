"""
Generate tests/golden/play_game.npz by RUNNING the reference's own `GameHironaka` (hironaka/game.py:84-119) with its own
hosts, `ChooseFirstAgent` / `RandomAgent` and ListPoints, and its own `HironakaValidator.playoff`
(hironaka/validator/hironaka_validator.py:30-48).  Runs only where the reference checkout exists; the resulting .npz is
what travels, and it holds data only.

The files are loaded one by one as make_golden.py does (the package __init__ files import jax).

Layout (G games, S moves in all; tests/play_rules.py load_games / load_playoffs unpack it):
    names        [G] str
    hosts        [5] str      the host keys, indexed by the host columns
    agents       [2] str      "choose_first", "random"
    meta         [G, 10] int64 m, d, host, agent, scale_observation, the seed of `random`, rows after Game.__init__,
                              moves recorded, stopped (1: state.ended, 0: the recording ended first), raised (1: the
                              reference raised at the move after the recorded ones)
    roots        flat int32   the roots as given, m*d each
    lists        [S, 7]       the host's list at every move in the reference's order, padded with -1
    axes         [S]          the agent's axis
    counts       [S]          the rows after the move
    int_states   flat int64   of the games without scale_observation: the state after Game.__init__, then after every move
    float_states flat float64 the same of the games with scale_observation
    po_names     [P] str      the playoffs
    po_meta      [P, 10]      host, agent, scale_observation, step_threshold, num_steps, m, d, reset states recorded,
                              entries of len_history, steps recorded
    po_thresholds [P] float64 value_threshold, 0 for None
    po_states    flat int32   the states `reset` handed out, in order (raw, before its rescale), the one of the
                              constructor first and the one of playoff's closing reset last
    po_history   flat         len_history
    po_axes      flat         move_history: the agent's axis of every step

Games: seeded roots of dim 2..7 with 2..11 points and a few 20-point roots of dim 3, each under the five deterministic
hosts x the two agents (`random` seeded per game) x scale_observation on and off, value_threshold None.  A game is
recorded until it stops, MAX_MOVES moves, or a coordinate passes 2^22 (without scale_observation; with it no coordinate
passes 1).  At most 2 % of the games may raise.

Playoffs: playoff(300) with np.random and random seeded, step_threshold 25, scale_observation both ways: Zeillinger,
ZeillingerLex and AllCoordHost against both agents, the two weak hosts against ChooseFirstAgent, and one with
value_threshold 1e3.

The plain restatement (tests/play_rules.py) follows every game move for move, and every playoff, before anything is
written.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_play_golden.py
"""
import os
import random
import sys
import time

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from make_golden import OUT, _load, load_reference  # noqa: E402
import play_rules as R  # noqa: E402

HOSTS = {"zeillinger": "Zeillinger", "all_coord": "AllCoordHost", "zeillinger_lex": "ZeillingerLex",
         "weak_spivakovsky": "WeakSpivakovsky", "weak_spivakovsky_min_hitting": "WeakSpivakovskyMinHitting"}
AGENTS = {"choose_first": "ChooseFirstAgent", "random": "RandomAgent"}
MAX_MOVES = 40
VALUE_CAP = 2 ** 22


def run(ref, host_name, agent_name, scale, rows, seed):
    random.seed(seed)
    host = getattr(ref.host, HOSTS[host_name])()
    agent = getattr(ref.agent, AGENTS[agent_name])()
    game = ref.game.GameHironaka(ref.ListPoints([[list(r) for r in rows]], value_threshold=None), host, agent,
                                 scale_observation=scale)
    root_state = [list(r) for r in game.state.points[0]]
    moves, raised = [], 0
    while not game.stopped and len(moves) < MAX_MOVES and max(map(max, game.state.points[0])) < VALUE_CAP:
        try:
            game.step()
        except Exception:  # noqa: BLE001 -- the reference's own failures: a host without a move
            raised = 1
            break
        moves.append(([int(c) for c in game.coord_history[-1][0]], int(game.move_history[-1][0]),
                      [list(r) for r in game.state.points[0]]))
    return root_state, moves, raised, int(game.stopped and not raised)


def follow(host_name, agent_name, scale, rows, got):
    """the restatement, with the recorded axes of a random agent fed in, must give the same game bit for bit"""
    root_state, moves, raised, stopped = got
    dtype = np.float64 if scale else np.int64
    axes = [a for _, a, _ in moves] if agent_name == "random" else None
    mine = R.play(rows, host_name, "choose_first", len(moves), axes=axes, rescaled=scale, reduce_root=True,
                  rescale_root=scale, dtype=dtype)
    assert mine.length == len(moves), (host_name, agent_name, scale, rows, mine.length, len(moves))
    same = lambda st, want: np.array_equal(R.points_of(st), np.asarray(want, dtype).reshape(-1, len(rows[0])))  # noqa: E731
    first = R.play(rows, host_name, "choose_first", 0, reduce_root=True, rescale_root=scale, dtype=dtype)
    assert same(first.state, root_state), (host_name, rows)
    for (coords, a, state), c3, a3, s3 in zip(moves, mine.lists, mine.axes, mine.history):
        assert c3 == coords and a3 == a and same(s3, state), (host_name, agent_name, scale, rows)
    if not raised:
        assert (mine.outcome == R.ENDED) == bool(stopped), (host_name, agent_name, scale, rows, mine.outcome)


def run_playoff(ref, val, host_name, agent_name, scale, thr, seed, num_steps=300, step_threshold=25):
    np.random.seed(seed)
    random.seed(seed)
    handed = []
    draw = ref.fn.generate_batch_points

    def recording(**kwargs):
        pts = draw(**kwargs)
        handed.append(np.asarray(pts[0], np.int32))
        return pts

    val.generate_batch_points = recording
    try:
        v = val.HironakaValidator(getattr(ref.host, HOSTS[host_name])(), getattr(ref.agent, AGENTS[agent_name])(),
                                  value_threshold=thr, step_threshold=step_threshold, scale_observation=scale)
        history = v.playoff(num_steps)
    finally:
        val.generate_batch_points = draw
    axes = [-1 if a[0] is None else int(a[0]) for a in v.move_history]
    assert len(axes) == num_steps
    return np.stack(handed), [int(x) for x in history], axes


def main():
    t0 = time.time()
    ref = load_reference()
    val = _load("hironaka.validator.hironaka_validator", "hironaka/validator/hironaka_validator.py")
    host_keys, agent_keys = list(HOSTS), list(AGENTS)
    names, meta = [], []
    flat = {k: [] for k in ("roots", "lists", "axes", "counts", "int_states", "float_states")}
    seen = {"ended": 0, "running": 0, "raised": 0}

    def add(name, rows, seed):
        for host_name in HOSTS:
            for agent_name in AGENTS:
                for scale in (False, True):
                    got = run(ref, host_name, agent_name, scale, rows, seed)
                    follow(host_name, agent_name, scale, rows, got)
                    root_state, moves, raised, stopped = got
                    names.append(f"{name}_{host_name}_{agent_name}_{'scaled' if scale else 'plain'}")
                    meta.append([len(rows), len(rows[0]), host_keys.index(host_name), agent_keys.index(agent_name),
                                 int(scale), seed, len(root_state), len(moves), stopped, raised])
                    key = "float_states" if scale else "int_states"
                    flat["roots"] += [v for r in rows for v in r]
                    flat[key] += [v for r in root_state for v in r]
                    for coords, a, state in moves:
                        flat["lists"].append(coords + [-1] * (7 - len(coords)))
                        flat["axes"].append(a)
                        flat["counts"].append(len(state))
                        flat[key] += [v for r in state for v in r]
                    seen["ended"] += stopped
                    seen["running"] += not stopped and not raised
                    seen["raised"] += raised

    rng = np.random.default_rng(20261018)
    seed = 0
    for d in (2, 3, 4, 5, 6, 7):
        for j in range(2):
            rows = rng.integers(0, 10, (int(rng.integers(2, 12)), d)).tolist()
            add(f"d{d}_{j}", rows, seed)
            seed += 1
    for j in range(2):
        add(f"d3_twenty_{j}", rng.integers(0, 30, (20, 3)).tolist(), seed)
        seed += 1

    meta = np.asarray(meta, np.int64)
    assert seen["raised"] * 50 <= len(names), seen
    assert seen["ended"] and seen["running"] and set(meta[:, 1]) == {2, 3, 4, 5, 6, 7} and meta[:, 7].max() > 3

    po_names, po_meta, po_thr = [], [], []
    po = {k: [] for k in ("po_states", "po_history", "po_axes")}
    cases = [(h, a, s, None) for h in ("zeillinger", "zeillinger_lex", "all_coord") for a in AGENTS for s in (True, False)]
    cases += [(h, "choose_first", s, None) for h in ("weak_spivakovsky", "weak_spivakovsky_min_hitting")
              for s in (True, False)]
    cases += [("weak_spivakovsky", "choose_first", False, 1e3), ("zeillinger", "choose_first", False, 1e3)]
    for j, (host_name, agent_name, scale, thr) in enumerate(cases):
        states, history, axes = run_playoff(ref, val, host_name, agent_name, scale, thr, 100 + j)
        mine, used = R.playoff(states, 300, host_name, "choose_first", 25, scale, thr,
                               axes=axes if agent_name == "random" else None)
        assert mine == history and used == len(states), (host_name, agent_name, scale, thr, mine, history)
        po_names.append(f"{host_name}_{agent_name}_{'scaled' if scale else 'plain'}_{'thr' if thr else 'nothr'}")
        po_meta.append([host_keys.index(host_name), agent_keys.index(agent_name), int(scale), 25, 300, states.shape[1],
                        states.shape[2], len(states), len(history), len(axes)])
        po_thr.append(thr or 0.0)
        po["po_states"] += states.reshape(-1).tolist()
        po["po_history"] += history
        po["po_axes"] += axes

    rec = {k: np.asarray(v, np.int32) for k, v in flat.items() if k not in ("int_states", "float_states")}
    rec.update({k: np.asarray(v, np.int32) for k, v in po.items()})
    rec.update(names=np.asarray(names), hosts=np.asarray(host_keys), agents=np.asarray(agent_keys), meta=meta,
               int_states=np.asarray(flat["int_states"], np.int64), float_states=np.asarray(flat["float_states"], np.float64),
               po_names=np.asarray(po_names), po_meta=np.asarray(po_meta, np.int64),
               po_thresholds=np.asarray(po_thr, np.float64))
    path = os.path.join(OUT, "play_game.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) <= 512 * 1024
    print(f"wrote play_game.npz: {len(names)} games, {len(flat['axes'])} moves, {seen}, {len(po_names)} playoffs, "
          f"{os.path.getsize(path)} bytes in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
