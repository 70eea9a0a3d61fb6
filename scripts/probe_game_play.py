"""Probe of hk_game_play (hironaka_amd.game.GameHironaka.play): writes profiles/game_play_probe.json (or the path given as
the first argument) and prints the same JSON line.  No threshold is attached to any figure.

65 536 games at (20,3) and at (8,5), each shape on its own device-generated batch (ops.generate_points, values below 20),
played to the end (at most MAX_MOVES moves) in float32 without scale_observation:

  zeillinger    Zeillinger against the random agent: GameHironaka.play (one launch) and the step() loop over the same
                games (host, fused move and the end test per move: the path before hk_game_play)
  min_hitting   WeakSpivakovskyMinHitting against a random agent with USE_REPOSITION: the agent's play() (one launch;
                GameHironaka.play takes the two plain agents only) and the step() loop
  rollout       at (20,3) under Zeillinger only: hk_rollout with its specialised Zeillinger kernel and the random-legal
                agent for MAX_MOVES steps, the ceiling of a kernel written for one shape and one host

Events around the whole run, construction excluded, median of 5 after a warm-up.  The two ways draw their random axes
from different generators, so they play different games from the same roots: each is divided by its own move count
(us_per_move = microseconds per game-move).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from hironaka_amd import _abi as A
from hironaka_amd import ops
from hironaka_amd.agent import RandomAgent
from hironaka_amd.core import HipPoints
from hironaka_amd.game import GameHironaka
from hironaka_amd.host import WeakSpivakovskyMinHitting, Zeillinger

MAX_MOVES = 200
GAMES = 65536


class RepositioningRandomAgent(RandomAgent):
    USE_REPOSITION = True


def event_seconds(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3


def timed(make, run, moves_of, reps=5):
    run(make())  # warm-up
    runs, last = [], None
    for _ in range(reps):
        subject = make()
        torch.cuda.synchronize()
        runs.append(event_seconds(lambda: run(subject)))
        last = subject
    moves = int(moves_of(last))
    s = float(np.median(runs))
    return {"s": s, "runs_s": runs, "moves": moves, "us_per_move": 1e6 * s / max(moves, 1)}


def step_loop(game):
    for _ in range(MAX_MOVES):
        if not game.step():
            break


def history_moves(game):
    return sum(int((a >= 0).sum()) for a in game.move_history)


def probe_shape(m, d):
    roots = ops.generate_points(GAMES, m, d, 20, seed=m * 100 + d)
    out = {"shape": [m, d], "games": GAMES}

    def game(host, agent):
        return GameHironaka(HipPoints(roots.clone(), semantics="list"), host, agent, scale_observation=False)

    zeil = lambda: game(Zeillinger(), RandomAgent(1))  # noqa: E731
    out["zeillinger"] = {"fused": timed(zeil, lambda g: g.play(MAX_MOVES), lambda g: g.length.sum()),
                         "step_loop": timed(zeil, step_loop, history_moves)}
    # the reposition case: play() of the agent on the reduced roots, and the step loop with the same agent class
    reduced = game(WeakSpivakovskyMinHitting(), RepositioningRandomAgent(1)).state.points
    results = []
    fused = timed(lambda: reduced.clone(),
                  lambda pts: results.append(RepositioningRandomAgent(1).play(pts, host="weak_spivakovsky_min_hitting",
                                                                              max_steps=MAX_MOVES, out=pts)),
                  lambda pts: results[-1].length.sum())
    fused["outcomes"] = {ops.PLAY_OUTCOMES[int(k)]: int(v) for k, v in
                         zip(*torch.unique(results[-1].outcome, return_counts=True))}
    out["min_hitting"] = {"fused": fused,
                          "step_loop": timed(lambda: game(WeakSpivakovskyMinHitting(), RepositioningRandomAgent(1)),
                                             step_loop, history_moves)}
    if (m, d) == (20, 3):
        lengths = []

        def rollout(pts):
            res = ops.rollout(pts, MAX_MOVES, 1, host_policy=A.HK_HOST_ZEILLINGER, agent_policy=A.HK_AGENT_RANDOM_LEGAL,
                              stages=A.HK_STAGE_SHIFT | A.HK_STAGE_NEWTON, record=("game_length",))
            lengths.append(res["game_length"])

        start = ops.generate_points(GAMES, m, d, 20, seed=m * 100 + d, reposition=False)
        out["rollout"] = timed(lambda: start.clone(), rollout, lambda pts: lengths[-1].sum())
    for case in ("zeillinger", "min_hitting"):
        out[case]["step_loop_over_fused_per_move"] = (out[case]["step_loop"]["us_per_move"]
                                                      / out[case]["fused"]["us_per_move"])
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "game_play_probe.json")
    res = {"shapes": [probe_shape(20, 3), probe_shape(8, 5)], "max_moves": MAX_MOVES, "dtype": "float32",
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
