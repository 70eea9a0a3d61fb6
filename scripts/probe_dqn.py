"""Dev probe: the DQN fit step's glue -- hk_dqn_td and hk_polyak_update -- against the reference's own formulation in
torch on the same device (the parent commit has none of this, so torch is the yardstick, not the code under test).  HIP
events around warmed-up eager calls, the median of 7 runs, the ways alternating; (a) and (b) also replayed from a
captured graph, which leaves the device's time without the host's share of an eager call.

  (a) ops.dqn_td against dqn_trainer.py:68-88 in torch plus its autograd backward down to dL/dQ, float32,
      B in {256, 4096, 65536} x A in {3, 26}
  (b) ops.polyak_update against the reference's loop (two launches per tensor) and against torch._foreach_mul_ /
      _foreach_add_: the parameters of an 8 x 256-wide MLP, and 130 small tensors
  (c) one fit_network step against the same step with the torch formulation (an MLP 63 -> 256 -> 256 -> 3, batch 4096)
  (d) the fixture end to end: how far the parameters after one step lie from tests/golden/dqn_fit.npz, for the torch
      formulation on this device and for fit_network (test_gpu_dqn.py allows the latter twice the former)

Usage:  python scripts/probe_dqn.py [--out profiles/dqn_probe.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from hironaka_amd import dqn, ops
from probe_replay import alternate
from probe_stages import timeit

GAMMA, TAU = 0.99, 0.005


def torch_td(q, next_q, actions, rewards, dones):
    """the reference's lines and their backward down to q"""
    leaf = q.detach().requires_grad_(True)
    with torch.no_grad():
        mx, _ = next_q.max(dim=1)
        target = rewards + (~dones) * GAMMA * mx.reshape(-1, 1)
    loss = torch.nn.functional.smooth_l1_loss(torch.gather(leaf, dim=1, index=actions.long()), target)
    (grad,) = torch.autograd.grad(loss, leaf)
    return loss, grad


def torch_fit(q_net, q_net_target, optimizer, batch, max_grad_norm):
    observations, actions, rewards, dones, next_observations = batch
    with torch.no_grad():
        mx, _ = q_net_target(next_observations).max(dim=1)
        target = rewards + (~dones) * GAMMA * mx.reshape(-1, 1)
    current = torch.gather(q_net(observations), dim=1, index=actions.long())
    loss = torch.nn.functional.smooth_l1_loss(current, target)
    optimizer.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(q_net.parameters(), max_grad_norm)
    optimizer.step()
    return loss


def reference_polyak(srcs, dsts, tau):
    with torch.no_grad():
        for s, d in zip(srcs, dsts):
            d.mul_(1 - tau)
            torch.add(d, s, alpha=tau, out=d)


def foreach_polyak(srcs, dsts, tau):
    with torch.no_grad():
        torch._foreach_mul_(dsts, 1 - tau)
        torch._foreach_add_(dsts, srcs, alpha=tau)


class Fixed:
    def __init__(self, batch):
        self.batch = batch

    def sample(self, batch_size, device=None, clone=True):
        return self.batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_probe.json"))
    args = ap.parse_args()
    torch.manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float32",
              "unit": "us per eager call, median of 7 runs of 20 calls, the ways alternating; graph_*: us per call of 20 "
                      "calls captured into one graph and replayed 10 times"}
    for B in (256, 4096, 65536):
        for A_ in (3, 26):
            q, next_q = torch.randn(B, A_, device="cuda") * 2, torch.randn(B, A_, device="cuda") * 2
            actions = torch.randint(0, A_, (B, 1), device="cuda", dtype=torch.int32)
            rewards = torch.randint(-1, 2, (B, 1), device="cuda").float()
            dones = torch.rand(B, 1, device="cuda") < 0.3
            (t_hk, t_torch), spread = alternate([lambda: ops.dqn_td(q, next_q, actions, rewards, dones, GAMMA, want=()),
                                                 lambda: torch_td(q, next_q, actions, rewards, dones)], iters=20)
            # the same calls replayed from a captured graph: the device's time, without the host's share
            g_hk = timeit(lambda: ops.dqn_td(q, next_q, actions, rewards, dones, GAMMA, want=()), iters=20, reps=10)
            g_torch = timeit(lambda: torch_td(q, next_q, actions, rewards, dones), iters=20, reps=10)
            result[f"td_B{B}_A{A_}"] = {"a_hk_dqn_td": t_hk, "a_torch_lines_and_backward": t_torch,
                                       "torch_over_hk": t_torch / t_hk, "min_max": spread,
                                       "graph_hk_dqn_td": g_hk, "graph_torch": g_torch, "graph_torch_over_hk": g_torch / g_hk}
            print(f"    from a graph: hk_dqn_td {g_hk:.1f} us, torch {g_torch:.1f} us", flush=True)
            print(f"(a) B {B} A {A_}: hk_dqn_td {t_hk:.1f} us, torch {t_torch:.1f} us: torch / hk = {t_torch / t_hk:.2f}",
                  flush=True)
    lists = {"mlp_8x256": [n for _ in range(8) for n in (256 * 256, 256)], "small_130": [64 + k for k in range(130)]}
    for name, sizes in lists.items():
        srcs = [torch.randn(n, device="cuda") for n in sizes]
        dsts = [torch.randn(n, device="cuda") for n in sizes]
        (t_hk, t_ref, t_each), spread = alternate([lambda: ops.polyak_update(srcs, dsts, TAU),
                                                   lambda: reference_polyak(srcs, dsts, TAU),
                                                   lambda: foreach_polyak(srcs, dsts, TAU)], iters=20)
        graph = [timeit(fn, iters=20, reps=10) for fn in (lambda: ops.polyak_update(srcs, dsts, TAU),
                                                          lambda: reference_polyak(srcs, dsts, TAU),
                                                          lambda: foreach_polyak(srcs, dsts, TAU))]
        print(f"    from a graph: hk {graph[0]:.1f} us, reference loop {graph[1]:.1f} us, foreach {graph[2]:.1f} us",
              flush=True)
        result[f"polyak_{name}"] = {"graph_hk_polyak_update": graph[0], "graph_reference_loop": graph[1],
                                    "graph_torch_foreach": graph[2], "tensors": len(sizes), "elements": sum(sizes), "b_hk_polyak_update": t_hk,
                                    "b_reference_loop": t_ref, "b_torch_foreach": t_each, "loop_over_hk": t_ref / t_hk,
                                    "foreach_over_hk": t_each / t_hk, "min_max": spread}
        print(f"(b) {name}: hk_polyak_update {t_hk:.1f} us, reference loop {t_ref:.1f} us, foreach {t_each:.1f} us",
              flush=True)
    B, obs_dim, A_ = 4096, 63, 3
    make = lambda: torch.nn.Sequential(torch.nn.Linear(obs_dim, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256),  # noqa: E731
                                       torch.nn.ReLU(), torch.nn.Linear(256, A_)).cuda()
    batch = (torch.randn(B, obs_dim, device="cuda"), torch.randint(0, A_, (B, 1), device="cuda", dtype=torch.int32),
             torch.randint(-1, 2, (B, 1), device="cuda").float(), torch.rand(B, 1, device="cuda") < 0.3,
             torch.randn(B, obs_dim, device="cuda"))
    nets = [(make(), make()) for _ in range(2)]
    optims = [torch.optim.SGD(q.parameters(), lr=1e-3) for q, _ in nets]
    (t_hk, t_torch), spread = alternate(
        [lambda: dqn.fit_network(nets[0][0], nets[0][1], optims[0], Fixed(batch), B, GAMMA, 1.0),
         lambda: torch_fit(nets[1][0], nets[1][1], optims[1], batch, 1.0)], iters=20)
    result["fit_step_B4096"] = {"c_fit_network": t_hk, "c_torch_formulation": t_torch, "torch_over_hk": t_torch / t_hk,
                                "min_max": spread}
    print(f"(c) fit step: fit_network {t_hk:.1f} us, torch formulation {t_torch:.1f} us", flush=True)
    from test_gpu_dqn import fit_distances
    distances = fit_distances(np.load(os.path.join(ROOT, "tests", "golden", "dqn_fit.npz")))
    result["fixture_end_to_end"] = {"unit": "largest |parameter - recorded| / largest |recorded| of its tensor, in eps_T",
                                    "d_torch_on_device_max": max(t for t, _ in distances),
                                    "d_fit_network_max": max(o for _, o in distances),
                                    "per_case_torch_then_fit_network": distances}
    print(f"(d) fixture: torch on device {result['fixture_end_to_end']['d_torch_on_device_max']:.3f} eps, "
          f"fit_network {result['fixture_end_to_end']['d_fit_network_max']:.3f} eps", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
