"""Dev probe: the MCTS trainer's gradient step -- hk_pv_loss through hironaka_amd.loss, and one whole step of
HipTrainer.train_step's pieces -- against the same step written with torch's own operators on the same device (the
parent commit has none of this, so torch is the yardstick, not the code under test).  HIP events around warmed-up eager
calls, the median of 7 runs of 20 calls, the ways alternating; every way also captured 20 times into one graph and
replayed, which leaves the device's time without the host's share of an eager call.

  (a) loss and its backward alone: loss.policy_value_loss(..., index=rows) + backward down to logits and value, against
      the three gathers + loss.torch_policy_value_loss + backward
  (b) one whole gradient step of a host network (spec (20, 3): 60 inputs, 4 actions): gather, forward, loss, backward,
      clipping, optimiser -- policy_value_loss + optim.safe_clip_grads_ + optim.Adam against torch_policy_value_loss +
      torch.nn.utils.clip_grad_norm_ + torch.optim.Adam (capturable where captured)

Shapes: the test config's [32] x 2 DenseResNet at 32 rows, [128] x 8 at 128 and 256 rows; 4096 samples.

Usage:  python scripts/probe_pv_loss.py [--out profiles/pv_loss_probe.json]
        python scripts/probe_pv_loss.py --kernel-only      (500 launches per shape and nothing else: for a kernel trace)"""
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
from probe_replay import alternate
from probe_stages import timeit

SAMPLES, IN_DIM, ACTIONS = 4096, 60, 4
SHAPES = [([32] * 2, 32), ([128] * 8, 128), ([128] * 8, 256)]


def data(rows):
    g = torch.Generator(device="cuda").manual_seed(rows)
    obs = torch.rand(SAMPLES, IN_DIM, device="cuda", generator=g)
    target_policy = 3 * torch.randn(SAMPLES, ACTIONS, device="cuda", generator=g)
    target_policy[torch.rand(SAMPLES, ACTIONS, device="cuda", generator=g) < 0.2] = -float("inf")
    target_policy[:, 0] = 0.0  # never a row of -inf alone
    target_value = torch.rand(SAMPLES, device="cuda", generator=g) * 2 - 1
    index = torch.randint(0, SAMPLES, (rows,), device="cuda", generator=g)
    return obs, target_policy, target_value, index


def loss_fused(logits, value, target_policy, target_value, index):
    x, v = logits.detach().requires_grad_(), value.detach().requires_grad_()
    loss = hkloss.policy_value_loss(x, v, target_policy, target_value, index=index)
    return (loss,) + torch.autograd.grad(loss, (x, v))


def loss_torch(logits, value, target_policy, target_value, index):
    x, v = logits.detach().requires_grad_(), value.detach().requires_grad_()
    loss = hkloss.torch_policy_value_loss(x, v, target_policy[index], target_value[index])
    return (loss,) + torch.autograd.grad(loss, (x, v))


def step_fused(module, optimizer, obs, target_policy, target_value, index):
    logits, value = module(obs[index])
    loss = hkloss.policy_value_loss(logits, value, target_policy, target_value, index=index)
    optimizer.zero_grad()
    loss.backward()
    optim.safe_clip_grads_(list(module.parameters()), 1.0)
    optimizer.step()
    return loss


def step_torch(module, optimizer, obs, target_policy, target_value, index):
    logits, value = module(obs[index])
    loss = hkloss.torch_policy_value_loss(logits, value, target_policy[index], target_value[index])
    optimizer.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(module.parameters(), 1.0)
    optimizer.step()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pv_loss_probe.json"))
    ap.add_argument("--kernel-only", action="store_true")
    args = ap.parse_args()
    if args.kernel_only:
        for _, rows in SHAPES:
            obs, target_policy, target_value, index = data(rows)
            logits, value = torch.randn(rows, ACTIONS, device="cuda"), torch.randn(rows, 1, device="cuda")
            for _ in range(500):
                hkloss.policy_value_loss(logits, value, target_policy, target_value, index=index)
        torch.cuda.synchronize()
        return
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "samples": SAMPLES, "actions": ACTIONS,
              "unit": "us per eager call, median of 7 runs of 20 calls, the ways alternating; graph_*: us per call of 20 "
                      "calls captured into one graph and replayed 10 times"}
    for arch, rows in SHAPES:
        obs, target_policy, target_value, index = data(rows)
        logits, value = torch.randn(rows, ACTIONS, device="cuda"), torch.randn(rows, 1, device="cuda")
        ways = [lambda: loss_fused(logits, value, target_policy, target_value, index),
                lambda: loss_torch(logits, value, target_policy, target_value, index)]
        (t_hk, t_torch), spread = alternate(ways, iters=20)
        g_hk, g_torch = (timeit(fn, iters=20, reps=10) for fn in ways)
        key = f"{len(arch)}x{arch[0]}_rows{rows}"
        result[f"loss_{key}"] = {"a_fused_loss_and_backward": t_hk, "a_torch_loss_and_backward": t_torch,
                                 "torch_over_fused": t_torch / t_hk, "min_max": spread, "graph_fused": g_hk,
                                 "graph_torch": g_torch, "graph_torch_over_fused": g_torch / g_hk}
        print(f"(a) {key}: fused {t_hk:.1f} us, torch {t_torch:.1f} us; from a graph {g_hk:.1f} / {g_torch:.1f} us",
              flush=True)

        def pair(capturable):
            fused = hknet.DenseResNet(ACTIONS, arch, input_dim=IN_DIM, seed=1).cuda()
            plain = hknet.DenseResNet(ACTIONS, arch, input_dim=IN_DIM, seed=1).cuda()
            o_fused = optim.Adam(fused.parameters(), lr=1e-3)
            o_plain = torch.optim.Adam(plain.parameters(), lr=1e-3, capturable=capturable)
            return [lambda: step_fused(fused, o_fused, obs, target_policy, target_value, index),
                    lambda: step_torch(plain, o_plain, obs, target_policy, target_value, index)]

        (t_hk, t_torch), spread = alternate(pair(False), iters=20)
        g_hk, g_torch = (timeit(fn, iters=20, reps=10) for fn in pair(True))
        result[f"step_{key}"] = {"b_fused_loss_step": t_hk, "b_all_torch_step": t_torch, "torch_over_fused": t_torch / t_hk,
                                 "min_max": spread, "graph_fused": g_hk, "graph_torch": g_torch,
                                 "graph_torch_over_fused": g_torch / g_hk}
        print(f"(b) {key}: fused-loss step {t_hk:.1f} us, all-torch step {t_torch:.1f} us; from a graph {g_hk:.1f} / "
              f"{g_torch:.1f} us", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
