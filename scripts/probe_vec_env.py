"""Time one step of the vectorised environments (vec_env: one hk_env_step launch, with auto reset and, like the parent,
without) against one step of gym_env's HironakaHostEnv / HironakaAgentEnv on the same batch of the same box, in
alternating rounds.

    python scripts/probe_vec_env.py [--games 65536] [--rounds 7] [--steps 10] [--out profiles/vec_env_probe.json]

A round resets the environment, then times `steps` steps between two device synchronisations with the host's clock, so
that the figure is what a learner's loop pays per step: launches and the Python around them.  Actions are drawn once
and live on the device.  Reported: the median over the rounds, in microseconds per step."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hironaka_amd.agent import ChooseFirstAgent  # noqa: E402
from hironaka_amd.gym_env import HironakaAgentEnv, HironakaHostEnv  # noqa: E402
from hironaka_amd.host import Zeillinger  # noqa: E402
from hironaka_amd.vec_env import HironakaAgentVecEnv, HironakaHostVecEnv  # noqa: E402

SHAPES = ((20, 3), (10, 3))


def one_round(env, actions, steps):
    env.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        env.step(actions[k])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def probe(mode, m, d, games, rounds, steps):
    cfg = dict(dimension=d, max_num_points=m, max_value=20, seed=1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    if mode == "host":
        fused = HironakaHostVecEnv(Zeillinger(), games, **cfg)
        plain = HironakaHostVecEnv(Zeillinger(), games, auto_reset=False, **cfg)
        parent = HironakaHostEnv(Zeillinger(), num_envs=games, **cfg)
        actions = torch.randint(0, d, (steps, games), device="cuda", generator=gen, dtype=torch.int32)
    else:
        fused = HironakaAgentVecEnv(ChooseFirstAgent(), games, **cfg)
        plain = HironakaAgentVecEnv(ChooseFirstAgent(), games, auto_reset=False, **cfg)
        parent = HironakaAgentEnv(ChooseFirstAgent(), num_envs=games, **cfg)
        actions = (torch.rand((steps, games, d), device="cuda", generator=gen) < 0.7).to(torch.int32)
    times = {"fused": [], "fused_no_reset": [], "parent": []}
    for r in range(rounds + 1):  # round 0 warms all up
        for name, env in (("fused", fused), ("fused_no_reset", plain), ("parent", parent)):
            t = one_round(env, actions, steps)
            if r:
                times[name].append(t)
    f, p = statistics.median(times["fused"]), statistics.median(times["parent"])
    return {"mode": mode, "max_points": m, "dim": d, "games": games, "rounds": rounds, "steps_per_round": steps,
            "fused_step_us": round(f, 1), "parent_step_us": round(p, 1), "parent_over_fused": round(p / f, 2),
            "fused_no_reset_step_us": round(statistics.median(times["fused_no_reset"]), 1),
            "fused_rounds_us": [round(t, 1) for t in times["fused"]],
            "parent_rounds_us": [round(t, 1) for t in times["parent"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    results = [probe(mode, m, d, a.games, a.rounds, a.steps) for mode in ("host", "agent") for m, d in SHAPES]
    for r in results:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
