"""Dev probe: the MCTS trainer's gradient step with DenseResNet.fused_training -- the network's forward and backward through
hk_pvgrad_forward / hk_pvgrad_backward -- against the SAME build with fused_training = False, which is the parent commit's
path unchanged to the bit (torch autograd through the module's children) measured in the same process.  HIP events around
warmed-up eager calls, the median of 7 runs of 20 calls, the ways alternating; every way also captured 20 times into one
graph and replayed, which leaves the device's time without the host's share of an eager call.

  (a) the network's forward and backward alone: module(x), then backward from given gradients at policy and value
  (b) one whole gradient step of a host network (spec (20, 3): 60 inputs, 4 actions): gather, forward, hk_pv_loss,
      backward, optim.safe_clip_grads_, optim.Adam -- HipTrainer.train_step's pieces

Shapes: pv_loss_probe.json's -- [32] x 2 at 32 rows, [128] x 8 at 128 and 256 rows -- and [256] x 18 at 256 rows; 4096 samples.

Usage:  python scripts/probe_pvnet_train.py [--out profiles/pvnet_train_probe.json]
        python scripts/probe_pvnet_train.py --kernel-only      (200 forward + backward per shape and nothing else: for a
                                                                 kernel trace)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from hironaka_amd import loss as hkloss
from hironaka_amd import net as hknet
from hironaka_amd import optim
from probe_pv_loss import ACTIONS, IN_DIM, data
from probe_replay import alternate
from probe_stages import timeit

SHAPES = [([32] * 2, 32), ([128] * 8, 128), ([128] * 8, 256), ([256] * 18, 256)]


def module_of(arch, fused):
    module = hknet.DenseResNet(ACTIONS, arch, input_dim=IN_DIM, seed=1).cuda()
    module.fused_training = fused
    return module


def forward_backward(module, x, grad_policy, grad_value):
    policy, value = module(x)
    return torch.autograd.grad((policy, value), list(module.parameters()), (grad_policy, grad_value))


def step(module, optimizer, obs, target_policy, target_value, index):
    logits, value = module(obs[index])
    loss = hkloss.policy_value_loss(logits, value, target_policy, target_value, index=index)
    optimizer.zero_grad()
    loss.backward()
    optim.safe_clip_grads_(list(module.parameters()), 1.0)
    optimizer.step()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pvnet_train_probe.json"))
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if args.kernel_only:
        for arch, rows in SHAPES:
            module = module_of(arch, True)
            x = torch.rand(rows, IN_DIM, device="cuda")
            gp, gv = torch.randn(rows, ACTIONS, device="cuda") / rows, torch.randn(rows, 1, device="cuda") / rows
            for _ in range(200):
                forward_backward(module, x, gp, gv)
            assert module.fused_last_reason is None
        torch.cuda.synchronize()
        return
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "in_dim": IN_DIM, "actions": ACTIONS,
              "unit": "us per eager call, median of 7 runs of 20 calls, the ways alternating; graph_*: us per call of 20 "
                      "calls captured into one graph and replayed 10 times; unfused: the same build with "
                      "fused_training = False (the parent commit's path)"}
    for arch, rows in SHAPES:
        obs, target_policy, target_value, index = data(rows)
        x = obs[index].clone()
        gp, gv = torch.randn(rows, ACTIONS, device="cuda") / rows, torch.randn(rows, 1, device="cuda") / rows
        key = f"{len(arch)}x{arch[0]}_rows{rows}"
        nets = [module_of(arch, True), module_of(arch, False)]
        ways = [lambda m=m: forward_backward(m, x, gp, gv) for m in nets]
        (t_hk, t_torch), spread = alternate(ways, iters=20)
        assert nets[0].fused_last_reason is None and nets[1].fused_last_reason == "gradients are on"
        g_hk, g_torch = (timeit(fn, iters=20, reps=10) for fn in ways)
        result[f"network_{key}"] = {"a_fused_forward_backward": t_hk, "a_unfused_forward_backward": t_torch,
                                    "unfused_over_fused": t_torch / t_hk, "min_max": spread, "graph_fused": g_hk,
                                    "graph_unfused": g_torch, "graph_unfused_over_fused": g_torch / g_hk}
        print(f"(a) {key}: fused {t_hk:.1f} us, unfused {t_torch:.1f} us; from a graph {g_hk:.1f} / {g_torch:.1f} us", flush=True)

        def pair():
            mods = [module_of(arch, True), module_of(arch, False)]
            opts = [optim.Adam(m.parameters(), lr=1e-3) for m in mods]
            return [lambda m=m, o=o: step(m, o, obs, target_policy, target_value, index) for m, o in zip(mods, opts)]

        (t_hk, t_torch), spread = alternate(pair(), iters=20)
        g_hk, g_torch = (timeit(fn, iters=20, reps=10) for fn in pair())
        result[f"step_{key}"] = {"b_fused_step": t_hk, "b_unfused_step": t_torch, "unfused_over_fused": t_torch / t_hk,
                                 "min_max": spread, "graph_fused": g_hk, "graph_unfused": g_torch,
                                 "graph_unfused_over_fused": g_torch / g_hk}
        print(f"(b) {key}: fused step {t_hk:.1f} us, unfused step {t_torch:.1f} us; from a graph {g_hk:.1f} / {g_torch:.1f} us",
              flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
