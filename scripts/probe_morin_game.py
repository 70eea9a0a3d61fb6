"""Probe of hk_search_morin_play (hironaka_amd.game.GameMorin): writes profiles/morin_game_probe.json (or the path given
as the first argument) and prints the same JSON line.  No threshold is attached to any figure.

  thom4        the thom_points_homogeneous(4) game (19 points, dim 7, the last row distinguished) under WeakSpivakovsky
               with AgentMorin(tie="lowest"), played to the end: once as GameMorin.play (one launch) and once as the
               step() loop (one launch and one synchronisation per move); events around the whole game, construction
               excluded, median of 5 after a warm-up
  batch        65 536 seeded (8,5) games (values below 21, the lightest row distinguished) under Zeillinger's host,
               tie "random" with a fixed seed, the same two ways; moves = the moves played over the whole batch
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from hironaka_amd.agent import AgentMorin
from hironaka_amd.core import HipPoints
from hironaka_amd.game import GameMorin
from hironaka_amd.host import WeakSpivakovsky, Zeillinger

MAX_MOVES = 100  # test/testThom.py:68


def event_seconds(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / 1e3


def fused(game):
    game.play(MAX_MOVES)


def stepped(game):
    for _ in range(MAX_MOVES):
        if not game.step():
            break


def measure(make, reps=5):
    """per way of playing: the median seconds of a whole game batch, the runs, the moves played and the launches"""
    out = {}
    for name, run in (("fused", fused), ("step_loop", stepped)):
        run(make())  # warm-up
        runs, game = [], None
        for _ in range(reps):
            game = make()
            torch.cuda.synchronize()
            runs.append(event_seconds(lambda: run(game)))
        assert game.stopped, name
        moves = int(sum(int((a >= 0).sum()) for a in game.move_history))
        out[name] = {"s": float(np.median(runs)), "runs_s": runs, "moves": moves,
                     "launches": 1 if name == "fused" else len(game.move_history),
                     "moves_per_s": moves / float(np.median(runs))}
    assert out["fused"]["moves"] == out["step_loop"]["moves"]
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "morin_game_probe.json")
    golden = np.load(os.path.join(ROOT, "tests", "golden", "morin_game.npz"))
    m, d = (int(v) for v in golden["meta"][list(golden["names"]).index("thom4_weak_spivakovsky_s0")][:2])
    at = sum(int(r[0] * r[1]) for r in golden["meta"][: list(golden["names"]).index("thom4_weak_spivakovsky_s0")])
    thom_root = golden["roots"][at: at + m * d].reshape(1, m, d).astype(np.float32)

    def thom():
        state = HipPoints(thom_root.copy(), distinguished_points=[m - 1], semantics="list")
        return GameMorin(state, WeakSpivakovsky(), AgentMorin(tie="lowest"), scale_observation=False)

    rng = np.random.default_rng(65536)
    b, bm, bd = 65536, 8, 5
    roots = rng.integers(0, 21, (b, bm, bd)).astype(np.float32)
    count = rng.integers(2, bm + 1, b)
    for i in range(b):
        roots[i, count[i]:] = -1.0
    light = np.where(roots[:, :, 0] >= 0, roots.sum(2), np.inf).argmin(1).astype(np.int32)
    roots_dev, light_dev = torch.as_tensor(roots, device="cuda"), torch.as_tensor(light, device="cuda")

    def batch():
        state = HipPoints(roots_dev.clone(), distinguished_points=light_dev.clone(), semantics="list")
        return GameMorin(state, Zeillinger(), AgentMorin(tie="random", seed=1), scale_observation=False)

    res = {"thom4": dict(measure(thom), shape=[m, d], host="weak_spivakovsky", tie="lowest"),
           "batch": dict(measure(batch), games=b, shape=[bm, bd], host="zeillinger", tie="random"),
           "max_moves": MAX_MOVES, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
