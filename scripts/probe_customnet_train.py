"""Dev probe: the MCTS trainer's gradient step on a CustomNet with CustomNet.fused_tower_training -- the network's forward and
backward through hk_customgrad_forward / hk_customgrad_backward, one tower per row both ways -- against the SAME build with the
flag off, which is the parent commit's path unchanged to the bit (torch autograd through plain_forward: every tower on every
row) measured in the same process.  The method is probe_pvnet_train.py's: HIP events around warmed-up eager calls, the median
of 7 runs of 20 calls, the ways alternating; every way also captured 20 times into one graph and replayed, which leaves the
device's time without the host's share of an eager call.

  (a) the network's forward and backward alone: module(features), then backward from given gradients at policy and value
  (b) one whole HipTrainer.train_step of the agent network: gather, features, forward, hk_pv_loss, backward,
      optim.safe_clip_grads_, the optimiser

The rows are an agent `simulate`'s, so that the point counts are the workload's (the histogram is recorded).  Shapes: the test
config ((5, 3), custom, [32] x 2, 32 rows), the reference's training config ((5, 3), custom_dense, [128] x 8, 128 rows), the
same as custom (residue blocks), and (20, 3), custom_dense, [128] x 8 at 256 rows.

Usage:  python scripts/probe_customnet_train.py [--out profiles/customnet_train_probe.json]
        python scripts/probe_customnet_train.py --kernel-only   (200 forward + backward per shape and nothing else: for a
                                                                  kernel trace)"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from hironaka_amd.functional import get_feature_fn
from hironaka_amd.trainer_api import HipTrainer
from probe_replay import alternate
from probe_stages import timeit

# (name, net_type, max_num_points, block widths, rows per step)
SHAPES = [("test_custom_5pt_2x32", "custom", 5, [32] * 2, 32),
          ("jax_mcts_custom_dense_5pt_8x128", "custom_dense", 5, [128] * 8, 128),
          ("custom_5pt_8x128", "custom", 5, [128] * 8, 128),
          ("custom_dense_20pt_8x128", "custom_dense", 20, [128] * 8, 256)]
ROLE = "agent"


def trainer_of(net_type, m, arch, rows, fused):
    section = {"batch_size": rows, "net_arch": arch, "optim": {"name": "adamw", "args": {"learning_rate": 1e-3}}}
    config = {"use_cuda": True, "scale_observation": True, "reposition": True, "gumbel_scale": 0.3, "version_string": "mcts",
              "net_type": net_type, "dimension": 3, "max_num_points": m, "max_length_game": 8, "max_value": 20,
              "max_grad_norm": 1, "eval_batch_size": 64, "num_evaluations": 4, "num_evaluations_as_opponent": 2,
              "eval_on_cpu": False, "max_num_considered_actions": 10, "discount": 0.99,
              "host": dict(section), "agent": dict(section)}
    return HipTrainer(42, config, custom_net=True, fused_tower_training=fused)


def forward_backward(module, x, grad_policy, grad_value):
    policy, value = module(x)
    return torch.autograd.grad((policy, value), list(module.parameters()), (grad_policy, grad_value))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "customnet_train_probe.json"))
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "role": ROLE,
              "unit": "us per eager call, median of 7 runs of 20 calls, the ways alternating; graph_*: us per call of 20 "
                      "calls captured into one graph and replayed 10 times; unfused: the same build with "
                      "fused_tower_training = False (the parent commit's path: autograd through plain_forward)"}
    for name, net_type, m, arch, rows in SHAPES:
        fused, plain = (trainer_of(net_type, m, arch, rows, flag) for flag in (True, False))
        rollouts = tuple(t.clone() for t in fused.simulate(7, ROLE))
        index = torch.arange(rows, device="cuda") % rollouts[0].shape[0]
        feature_fn = get_feature_fn(ROLE, fused.spec, scale_observation=fused.scale_observation)
        with torch.no_grad():
            x = feature_fn(rollouts[0][index]).flatten(1).clone()
        actions = rollouts[1].shape[1]
        gp, gv = torch.randn(rows, actions, device="cuda") / rows, torch.randn(rows, 1, device="cuda") / rows
        nets = [copy.deepcopy(t.built_nets[ROLE]) for t in (fused, plain)]
        if args.kernel_only:
            for _ in range(200):
                forward_backward(nets[0], x, gp, gv)
            assert nets[0].fused_last_reason is None
            torch.cuda.synchronize()
            continue
        counts = torch.bincount((x[:, : 3 * m: 3] >= 0).sum(-1), minlength=m + 1).tolist()
        ways = [lambda n=n: forward_backward(n, x, gp, gv) for n in nets]
        (t_hk, t_torch), spread = alternate(ways, iters=20)
        assert nets[0].fused_last_reason is None and nets[1].fused_last_reason == "gradients are on"
        g_hk, g_torch = (timeit(fn, iters=20, reps=10) for fn in ways)
        result[f"network_{name}"] = {"rows": rows, "rows_per_point_count": counts, "a_fused_forward_backward": t_hk,
                                     "a_unfused_forward_backward": t_torch, "unfused_over_fused": t_torch / t_hk,
                                     "min_max": spread, "graph_fused": g_hk, "graph_unfused": g_torch,
                                     "graph_unfused_over_fused": g_torch / g_hk}
        print(f"(a) {name}: fused {t_hk:.1f} us, unfused {t_torch:.1f} us; from a graph {g_hk:.1f} / {g_torch:.1f} us; "
              f"rows per count {counts}", flush=True)

        steps = [lambda t=t: t.train_step(ROLE, rollouts, index) for t in (fused, plain)]
        (t_hk, t_torch), spread = alternate(steps, iters=20)
        assert fused.built_nets[ROLE].fused_last_reason is None
        assert plain.built_nets[ROLE].fused_last_reason == "gradients are on"
        g_hk, g_torch = (timeit(fn, iters=20, reps=10) for fn in steps)
        result[f"step_{name}"] = {"rows": rows, "b_fused_step": t_hk, "b_unfused_step": t_torch,
                                  "unfused_over_fused": t_torch / t_hk, "min_max": spread, "graph_fused": g_hk,
                                  "graph_unfused": g_torch, "graph_unfused_over_fused": g_torch / g_hk}
        print(f"(b) {name}: fused step {t_hk:.1f} us, unfused step {t_torch:.1f} us; from a graph {g_hk:.1f} / {g_torch:.1f} us",
              flush=True)
    if args.kernel_only:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
