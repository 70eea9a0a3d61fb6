"""Dev probe: HipTrainer.simulate(key, "host", use_unified_tree=True) -- the rollouts of the reference's main training
script, one tree for both players -- with fused_expand=True (recurrent_fn.UnifiedExpander: the kind of every batch decided
on the device, gated network launches, graph replay) against the SAME build with fused_expand=False, which is the parent
commit's path unchanged (the generic recurrent function: one host synchronisation per simulation, not capturable).

A host clock around whole simulate calls that end in a device synchronise; every way is warmed up first (captures
included), then the ways take turns, and the median of the runs is reported with their minimum and maximum.  Three
ways per shape: the generic path, the expander eagerly, the expander with use_graph=True.  The rollouts of the three are
compared bit for bit before anything is timed.

Shapes: the test config (tests/test_gpu_trainer.py: 64 games, (20, 3), 10 simulations, 20 moves), jax_mcts.yml's
(512 games, (5, 3), 100 simulations, 40 moves, 10 considered actions, [128] x 8 networks) and BASELINE configs[4]
(8192 games, (20, 3), 32 simulations, 20 moves); each with dense_resnet networks the trainer builds (the gated path)
and with trainer_api.standin_mlp callables (both networks run on every expansion).

Usage:  python scripts/probe_unified.py [--out profiles/unified_probe.json] [--shapes test,jax_mcts,baseline5] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from hironaka_amd.trainer_api import HipTrainer, standin_mlp

COMMON = {"max_value": 20, "max_grad_norm": 1.0, "gumbel_scale": 0.3, "use_cuda": True, "version_string": "probe",
          "net_type": "dense_resnet", "eval_on_cpu": False}
SHAPES = {
    "test": dict(eval_batch_size=64, max_num_points=20, dimension=3, max_length_game=20, scale_observation=True,
                 reposition=True, num_evaluations=10, num_evaluations_as_opponent=4, max_num_considered_actions=10,
                 discount=0.99, net_arch=[32, 32]),
    "jax_mcts": dict(eval_batch_size=512, max_num_points=5, dimension=3, max_length_game=40, scale_observation=False,
                     reposition=False, num_evaluations=100, num_evaluations_as_opponent=100, max_num_considered_actions=10,
                     discount=0.98, net_arch=[128] * 8),
    "baseline5": dict(eval_batch_size=8192, max_num_points=20, dimension=3, max_length_game=20, scale_observation=True,
                      reposition=True, num_evaluations=32, num_evaluations_as_opponent=4, max_num_considered_actions=10,
                      discount=0.99, net_arch=[128] * 8),
}


def trainer(shape, built, **kw):
    cfg = dict(COMMON, **{k: v for k, v in shape.items() if k != "net_arch"})
    m, d = cfg["max_num_points"], cfg["dimension"]
    if built:
        section = {"net_arch": shape["net_arch"]}
        return HipTrainer(42, dict(cfg, host=dict(section), agent=dict(section)), **kw)
    host_net, host_params = standin_mlp(m * d, 2 ** d - d - 1, 3)
    agent_net, agent_params = standin_mlp(m * d + d, d, 4)
    return HipTrainer(42, cfg, host_net=host_net, agent_net=agent_net, host_params=host_params,
                      agent_params=agent_params, **kw)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def same(a, b):
    return all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unified_probe.json"))
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float32",
              "unit": f"ms per simulate(key, 'host', use_unified_tree=True), host clock around a call that ends in a device "
                      f"synchronise, median of {args.reps} runs after a warm-up call of every way, the ways alternating; "
                      "generic: fused_expand=False (the parent commit's path)"}
    for name in args.shapes.split(","):
        shape = SHAPES[name]
        for built in (True, False):
            ways = {"generic": trainer(shape, built, fused_expand=False),
                    "expander_eager": trainer(shape, built, fused_expand=True),
                    "expander_graph": trainer(shape, built, fused_expand=True, use_graph=True)}
            run = {k: (lambda t=t: t.simulate(9, "host", use_unified_tree=True)) for k, t in ways.items()}
            outs = {k: [x.clone() for x in fn()] for k, fn in run.items()}  # warm-up (and capture), and the results
            agree = all(same(outs["generic"], outs[k]) for k in ("expander_eager", "expander_graph"))
            times = {k: [] for k in run}
            for _ in range(args.reps):
                for k, fn in run.items():
                    times[k].append(timed(fn))
            med = {k: statistics.median(v) for k, v in times.items()}
            key = f"{name}_{'dense_resnet' if built else 'standin_mlp'}"
            result[key] = {"shape": shape, "same_bits_as_generic": agree,
                           **{k: round(v, 3) for k, v in med.items()},
                           "min_max": {k: (round(min(v), 3), round(max(v), 3)) for k, v in times.items()},
                           "generic_over_expander_eager": round(med["generic"] / med["expander_eager"], 3),
                           "generic_over_expander_graph": round(med["generic"] / med["expander_graph"], 3)}
            print(key, json.dumps(result[key]), flush=True)
            del ways, run, outs
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
