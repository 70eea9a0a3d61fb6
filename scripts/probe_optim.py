"""Dev probe: the optimiser step -- optim.Adam.clip_and_step (hk_optim_prepare + hk_optim_apply) -- against the two lines
it replaces, nn.utils.clip_grad_norm_ + torch.optim.Adam.step() with foreach=True and with fused=True, on the same
device (the parent commit has none of this, so torch is the yardstick, not the code under test).  HIP events around
warmed-up eager calls, the median of 7 runs of 20 calls, the ways alternating; and the same calls replayed from a
captured graph (torch's Adam with capturable=True there: it refuses a capture otherwise), which leaves the device's time
without the host's share of an eager call.

  (a) two parameter lists, float32: the 8 x 256-wide MLP of the Polyak probe (16 tensors), and the architecture of the
      reference's example config, net_arch [128, 'b', {repeat 20: [256, 'b']}, 128, 'b'] (90 tensors: two launches of
      each kernel)
  (b) the prepare / apply kernel times from a `rocprofv3 --kernel-trace` run of its own (a fresh child process
      that does nothing but steps), for the two lists and for one tensor of 2^25 elements, where apply's bytes (4 loads
      and 4 stores of 4 bytes per element) over its time is set against the HBM rate
  (c) one whole fit_network step with optim.Adam against the parent's path (torch.optim.Adam, same net, same batch),
      alternating, three rounds each: accepted where the new median is at or below the parent's median plus the parent's
      own spread

Usage:  python scripts/probe_optim.py [--out profiles/optim_probe.json] [--no-trace]"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch
from hironaka_amd import dqn, optim
from probe_replay import alternate
from probe_stages import timeit

HBM_BYTES_PER_S = 8.0e12  # MI355X, peak
MAX_NORM, LR = 1.0, 1e-3
OBS_DIM, NUM_ACTIONS = 63, 3


def example_config_sizes():
    widths = [128] + [256] * 20 + [128]
    sizes, fan_in = [], OBS_DIM
    for w in widths:
        sizes += [fan_in * w, w, w, w]  # Linear weight and bias, BatchNorm1d weight and bias
        fan_in = w
    return sizes + [fan_in * NUM_ACTIONS, NUM_ACTIONS]


LISTS = {"mlp_8x256": [n for _ in range(8) for n in (256 * 256, 256)], "example_config": example_config_sizes()}


def make_params(sizes):
    params = [torch.nn.Parameter(torch.randn(n, device="cuda")) for n in sizes]
    for p in params:
        p.grad = torch.randn_like(p)
    return params


def torch_step(params, opt):
    torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
    opt.step()


def child():
    """what the kernel trace sees: 20 steps per list"""
    for sizes in list(LISTS.values()) + [[1 << 25]]:
        params = make_params(sizes)
        opt = optim.Adam(params, lr=LR)
        for _ in range(20):
            opt.clip_and_step(MAX_NORM)
        torch.cuda.synchronize()


def kernel_trace():
    """{"prepare" / "apply": the durations in ns of the optimiser kernels in launch order} from a rocprofv3 kernel trace
    of a child of its own"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child"]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        if done.returncode != 0:
            return {"unmeasured": f"rocprofv3 ended with {done.returncode}: {done.stdout.decode()[-300:]}"}
        rows = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    name = row.get("Kernel_Name", "")
                    for short in ("prepare", "apply"):
                        if f"optim_{short}_kernel" in name:
                            start = int(row["Start_Timestamp"])
                            rows.setdefault(short, []).append((start, int(row["End_Timestamp"]) - start))
        if sorted(rows) != ["apply", "prepare"]:
            return {"unmeasured": "no optimiser kernel in the trace"}
        return {short: [d for _, d in sorted(v)] for short, v in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_probe.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    if args.child:
        return child()
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float32",
              "unit": "us per eager call, median of 7 runs of 20 calls, the ways alternating; graph_*: us per call of 20 "
                      "calls captured into one graph and replayed 10 times"}
    for name, sizes in LISTS.items():
        sets = [make_params(sizes) for _ in range(3)]
        ours = optim.Adam(sets[0], lr=LR)
        each = torch.optim.Adam(sets[1], lr=LR, foreach=True)
        fused = torch.optim.Adam(sets[2], lr=LR, fused=True)
        fns = [lambda: ours.clip_and_step(MAX_NORM), lambda: torch_step(sets[1], each), lambda: torch_step(sets[2], fused)]
        (t_hk, t_each, t_fused), spread = alternate(fns, iters=20)
        entry = {"tensors": len(sizes), "elements": sum(sizes), "a_clip_and_step": t_hk, "a_torch_foreach": t_each,
                 "a_torch_fused": t_fused, "foreach_over_hk": t_each / t_hk, "fused_over_hk": t_fused / t_hk,
                 "min_max": spread}
        graph_sets = [make_params(sizes) for _ in range(3)]
        g_ours = optim.Adam(graph_sets[0], lr=LR)
        g_each = torch.optim.Adam(graph_sets[1], lr=LR, foreach=True, capturable=True)
        g_fused = torch.optim.Adam(graph_sets[2], lr=LR, fused=True, capturable=True)
        for key, fn in (("graph_clip_and_step", lambda: g_ours.clip_and_step(MAX_NORM)),
                        ("graph_torch_foreach", lambda: torch_step(graph_sets[1], g_each)),
                        ("graph_torch_fused", lambda: torch_step(graph_sets[2], g_fused))):
            try:
                entry[key] = timeit(fn, iters=20, reps=10)
            except Exception as e:  # noqa: BLE001  (a capture that torch refuses is a finding, not a failure)
                entry[key] = f"unmeasured: {type(e).__name__}: {str(e)[:200]}"
        result[f"step_{name}"] = entry
        print(f"(a) {name}: {entry}", flush=True)
    if args.no_trace:
        result["kernel_trace"] = {"unmeasured": "--no-trace"}
    else:
        trace = kernel_trace()
        if "unmeasured" in trace:
            result["kernel_trace"] = trace
        else:
            # the child's launches in order: 20 steps per list, one launch of each kernel per 64 tensors
            out, at = {"unit": "ns per step (the launches of a chain added), median of the last 10 of 20 steps"}, 0
            for name, sizes in list(LISTS.items()) + [("one_tensor_2^25", [1 << 25])]:
                launches = (len(sizes) + 63) // 64
                entry = {"launches_per_kernel": launches}
                for short in ("prepare", "apply"):
                    mine = trace[short][at:at + 20 * launches]
                    steps = [sum(mine[k * launches:(k + 1) * launches]) for k in range(20)]
                    entry[short] = statistics.median(steps[10:])
                at += 20 * launches
                nbytes = sum(sizes) * 4 * 8  # Adam with the clipped gradient written back: 4 loads and 4 stores
                entry["apply_bytes"] = nbytes
                entry["apply_fraction_of_hbm_peak"] = nbytes / (entry["apply"] * 1e-9) / HBM_BYTES_PER_S
                out[name] = entry
            assert at == len(trace["prepare"]) == len(trace["apply"]), (at, len(trace["prepare"]), len(trace["apply"]))
            result["kernel_trace"] = out
        print(f"(b) {result['kernel_trace']}", flush=True)
    B = 4096
    make = lambda: torch.nn.Sequential(torch.nn.Linear(OBS_DIM, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256),  # noqa: E731
                                       torch.nn.ReLU(), torch.nn.Linear(256, NUM_ACTIONS)).cuda()
    batch = (torch.randn(B, OBS_DIM, device="cuda"), torch.randint(0, NUM_ACTIONS, (B, 1), device="cuda", dtype=torch.int32),
             torch.randint(-1, 2, (B, 1), device="cuda").float(), torch.rand(B, 1, device="cuda") < 0.3,
             torch.randn(B, OBS_DIM, device="cuda"))

    class Fixed:
        def sample(self, batch_size, device=None, clone=True):
            return batch

    nets = [(make(), make()) for _ in range(2)]
    new = optim.Adam(nets[0][0].parameters(), lr=LR)
    parent = torch.optim.Adam(nets[1][0].parameters(), lr=LR)
    (t_new, t_parent), spread = alternate(
        [lambda: dqn.fit_network(nets[0][0], nets[0][1], new, Fixed(), B, 0.99, MAX_NORM),
         lambda: dqn.fit_network(nets[1][0], nets[1][1], parent, Fixed(), B, 0.99, MAX_NORM)], reps=3, iters=20)
    parent_spread = spread[1][1] - spread[1][0]
    result["fit_step_B4096"] = {"c_fit_network_optim_adam": t_new, "c_fit_network_torch_adam": t_parent,
                                "parent_over_new": t_parent / t_new, "min_max": spread, "parent_spread": parent_spread,
                                "accepted": bool(t_new <= t_parent + parent_spread)}
    print(f"(c) fit step: {result['fit_step_B4096']}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
