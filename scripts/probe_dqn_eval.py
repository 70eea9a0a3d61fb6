"""Dev probe: the DQN trainers' evaluation -- Trainer.get_rho_for_pair, and a whole evaluate_rho + count_actions of both
roles, as DQNTrainer._train runs them every evaluation_interval steps -- three ways on the same build:

  kernels   FusedGame.evaluate on hk_dqn_host_move / hk_dqn_agent_move, launched eagerly (four launches per move)
  graph     the same with use_graph=True: one move captured per call and replayed (the capture is inside the time)
  torch     the loop over FusedGame.host_move / agent_move with exploration_rate=0.0 and the accounting on the device
            (evaluate(force_torch=True)): those two methods are the parent commit's unchanged, and the loop is the
            fairest one that could be written on it -- the reference's own adds B device reads per sum()

on the reference's test config (dim 3, 20 points, 100 games, 100 moves, net_arch of widths 16 / 32) and on
dqn_config_example.yml's shapes (the same game, net_arch 128, 20 x 256, 128) at 100 and 4096 games.  A host clock around
calls that end in a device synchronise, every way warmed up, the ways taking turns, the median of 7 runs with their
minimum and maximum.  Fresh games are drawn inside every call, as the trainer draws them.

Usage:  python scripts/probe_dqn_eval.py [--out profiles/dqn_eval_probe.json]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from hironaka_amd import DQNTrainer
from hironaka_amd.fused_game import FusedGame
from hironaka_amd.player_modules import (AllCoordHostModule, ChooseFirstAgentModule, RandomAgentModule,
                                         RandomHostModule)

WAYS = {"kernels": dict(), "graph": dict(use_graph=True), "torch": dict(force_torch=True)}
ARCHS = {"test_config": [16, "b", {"repeat": 2, "net_arch": [32, "b"]}, 16, "b"],
         "example_config": [128, "b", {"repeat": 20, "net_arch": [256, "b"]}, 128, "b"]}
REPS, MAX_STEPS = 7, 100


def config(net_arch):
    role = dict(batch_size=256, initial_rollout_size=100, steps_before_rollout=10, steps_before_update_target=100,
                rollout_size=20, max_rollout_step=10, optim=dict(name="adam", args=dict(lr=1e-8)), er=0.2,
                net_arch=net_arch, gamma=0.99, tau=0.9)
    return dict(use_tensorboard=False, layerwise_logging=False, log_time=False, use_cuda=True, scale_observation=True,
                version_string="probe", dimension=3, max_num_points=20, max_value=20, max_grad_norm=10,
                host=copy.deepcopy(role), agent=copy.deepcopy(role),
                replay_buffer=dict(type="base", buffer_size=10000, use_cuda=True))


def rho_for_pair(t, host, agent, games, way, count_for=None):
    """Trainer.get_rho_for_pair / count_actions(er=0.0) with the way of playing chosen"""
    with torch.inference_mode():
        points = t._generate_random_points(games, t.device)
        game = FusedGame(host, agent, device=t.device, log_time=False, reward_func=t.reward_func, dtype=t.dtype)
        return game.evaluate(points, MAX_STEPS, scale_observation=t.scale_observation, count_for=count_for, **WAYS[way])


def whole_evaluation(t, games, way):
    """the five pairs of evaluate_rho, then count_actions of both roles"""
    p = (t.dimension, t.max_num_points, t.device)
    hosts = [t.host_net] * 3 + [RandomHostModule(*p), AllCoordHostModule(*p)]
    agents = [t.agent_net, RandomAgentModule(*p), ChooseFirstAgentModule(*p)] + [t.agent_net] * 2
    out = [rho_for_pair(t, h, a, games, way).rho for h, a in zip(hosts, agents)]
    return out + [rho_for_pair(t, t.host_net, t.agent_net, games, way, count_for=role).counts for role in ("host", "agent")]


def clocked(fn):
    torch.cuda.synchronize()
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3


def take_turns(fns):
    """ms per call of each of `fns` (a dict): the median of REPS runs, the ways alternating, and (min, max)"""
    for fn in fns.values():
        fn()
        fn()
    times = {name: [] for name in fns}
    for _ in range(REPS):
        for name, fn in fns.items():
            times[name].append(clocked(fn))
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_eval_probe.json"))
    args = ap.parse_args()
    torch.manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "max_steps": MAX_STEPS,
              "unit": f"ms per call by a host clock around a synchronised call, median of {REPS} runs after two warm-up "
                      "calls, the ways alternating; min / max are the spread of those runs"}
    for name, games in (("test_config", 100), ("example_config", 100), ("example_config", 4096)):
        t = DQNTrainer(config(ARCHS[name]))
        t.set_training(False)
        key = f"{name}_games{games}"
        pair = take_turns({way: (lambda way=way: rho_for_pair(t, t.host_net, t.agent_net, games, way)) for way in WAYS})
        whole = take_turns({way: (lambda way=way: whole_evaluation(t, games, way)) for way in WAYS})
        result[key] = {"get_rho_for_pair": pair, "evaluate_rho_and_count_actions": whole}
        for what, r in (("get_rho_for_pair", pair), ("evaluate_rho + count_actions", whole)):
            print(f"{key} {what}: " + ", ".join(
                f"{way} {v['median_ms']:.2f} ms ({v['min_ms']:.2f}..{v['max_ms']:.2f})" for way, v in r.items())
                + f"; torch / kernels = {r['torch']['median_ms'] / r['kernels']['median_ms']:.2f}, torch / graph = "
                  f"{r['torch']['median_ms'] / r['graph']['median_ms']:.2f}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
