"""Dev probe: the gradient-free forward of the MCTS trainer's policy-value networks in one launch (hk_pvnet_forward through
hironaka_amd.net.DenseResNet) against the SAME module with `fused_enabled = False` (the plain composition of its
children), float32.  HIP events around warmed-up work, the median of repeated runs, the two ways alternating.

  (a) one forward of: the reference's test config (5 points: inputs 15 / 18, [32, 32], 100 rows); train/jax_mcts.yml
      ([128] x 8, 512 rows); BASELINE configs[4] (inputs 60 / 63, [128] x 8 and [256] x 8, 8 192 rows: the 64-row tile);
      DResNet18 at 256 and 4 096 rows -- eagerly, and 10 calls captured into one graph and replayed
  (b) the kernel's own time from a `rocprofv3 --kernel-trace` run of its own (a fresh child process), with the achieved
      fraction of the 157.3 TF f32 matrix peak
  (c) one whole HipTrainer.simulate at configs[4] (8 192 games, 32 simulations per move, 20 moves) with the [128] x 8 nets
      the trainer builds from its config, fused on and off
  (d) the largest deviation of the kernel's tanh from float64's over the inputs of tests/test_gpu_pvnet.py::test_the_tanh,
      in units of 2^-24 (the test's bound is twice this figure)

Usage:  python scripts/probe_pvnet.py [--out profiles/pvnet_probe.json] [--no-trace] [--no-simulate]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from torch import nn
from hironaka_amd import net as N
from hironaka_amd import ops
from probe_replay import alternate
from probe_stages import timeit

# (name, constructor, input width, rows)
CASES = [
    ("test_host_2x32", lambda: N.DenseResNet(4, [32, 32], input_dim=15), 15, 100),
    ("test_agent_2x32", lambda: N.DenseResNet(3, [32, 32], input_dim=18), 18, 100),
    ("mcts_host_8x128", lambda: N.DenseResNet(4, [128] * 8, input_dim=60), 60, 512),
    ("mcts_agent_8x128", lambda: N.DenseResNet(3, [128] * 8, input_dim=63), 63, 512),
    ("configs4_host_8x128", lambda: N.DenseResNet(4, [128] * 8, input_dim=60), 60, 8192),
    ("configs4_agent_8x128", lambda: N.DenseResNet(3, [128] * 8, input_dim=63), 63, 8192),
    ("configs4_host_8x256", lambda: N.DenseResNet(4, [256] * 8, input_dim=60), 60, 8192),
    ("configs4_agent_8x256", lambda: N.DenseResNet(3, [256] * 8, input_dim=63), 63, 8192),
    ("dresnet18", lambda: N.DResNet18(3, input_dim=63), 63, 256),
    ("dresnet18", lambda: N.DResNet18(3, input_dim=63), 63, 4096),
]
F32_MATRIX_PEAK = 157.3e12
TRACE_CALLS = 20
CONFIGS4 = {"eval_batch_size": 8192, "max_num_points": 20, "dimension": 3, "max_length_game": 20, "max_value": 20,
            "scale_observation": True, "reposition": True, "gumbel_scale": 0.3, "net_type": "dense_resnet",
            "num_evaluations": 32, "num_evaluations_as_opponent": 4, "max_num_considered_actions": 10, "discount": 0.99,
            "host": {"net_arch": [128] * 8}, "agent": {"net_arch": [128] * 8}}


def flops(net, batch):
    return 2 * batch * sum(m.in_features * m.out_features for m in net.modules() if isinstance(m, nn.Linear))


def child():
    """what the kernel trace sees: TRACE_CALLS forwards per case"""
    with torch.no_grad():
        for _, make, k, rows in CASES:
            net = make().cuda()
            x = torch.rand(rows, k, device="cuda")
            for _ in range(TRACE_CALLS):
                net(x)
            torch.cuda.synchronize()


def kernel_trace():
    """the durations in ns of the pvnet kernel in launch order, from a rocprofv3 kernel trace of a child of its own"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child"]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        if done.returncode != 0:
            return {"unmeasured": f"rocprofv3 ended with {done.returncode}: {done.stdout.decode()[-300:]}"}
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if "pvnet_kernel" in row.get("Kernel_Name", ""):
                        start = int(row["Start_Timestamp"])
                        rows.append((start, int(row["End_Timestamp"]) - start))
        if not rows:
            return {"unmeasured": "no pvnet kernel in the trace"}
        return {"durations": [d for _, d in sorted(rows)]}


def tanh_deviation():
    """(d): the net and the inputs of tests/test_gpu_pvnet.py::test_the_tanh"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pvnet_rules as R
    rng = np.random.default_rng(27)
    net = R.random_net(rng, 60, [128, 128], 4, value_gain=4.0)
    x = rng.uniform(-1, 1, (257, 60)).astype(np.float32)  # test_gpu_mlp.inputs
    x[rng.random((257, 60)) < 0.05] = 0
    x[rng.random((257, 60)) < 0.02] = -0.0
    raw = R.forward(x, net)[1]
    dev = lambda t: None if t is None else torch.from_numpy(np.ascontiguousarray(t)).cuda()  # noqa: E731
    dn = lambda d: None if d is None else ops.PvnetDense(*(dev(t) for t in d))  # noqa: E731
    plan = ops.PvnetPlan([ops.PvnetBlock(b.kind, dn(b.dense1), dn(b.dense2), dn(b.proj), b.eps) for b in net.blocks],
                         tuple(dev(t) for t in net.policy), tuple(dev(t) for t in net.value))
    worst = 0.0
    for tile in (None, 16, 64):
        v = ops.pvnet_forward(dev(x), plan, tile=tile)[1].cpu().numpy().astype(np.float64)
        worst = max(worst, float(np.abs(v - np.tanh(raw.astype(np.float64))).max() / 2.0 ** -24))
    return {"tanh_max_units": worst, "unit": "2^-24", "rows": 257, "pre_activation_min_max": [float(raw.min()), float(raw.max())]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pvnet_probe.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-simulate", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    if args.child:
        return child()
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float32",
              "unit": "us per eager call, median of 7 runs of 10 calls, the ways alternating; graph_*: us per call of 10 "
                      "calls captured into one graph and replayed 10 times"}
    result["tanh"] = tanh_deviation()
    print(f"(d) {result['tanh']}", flush=True)
    with torch.no_grad():
        for name, make, k, rows in CASES:
            net, torch_net = make().cuda(), make().cuda()
            torch_net.load_state_dict(net.state_dict())
            torch_net.fused_enabled = False
            x = torch.rand(rows, k, device="cuda")
            net(x), torch_net(x)
            assert net.fused_last_reason is None and torch_net.fused_last_reason == "fused_enabled is False"
            (t_hk, t_torch), spread = alternate([lambda: net(x), lambda: torch_net(x)], iters=10)
            entry = {"row_tile": ops.lib().hk_mlp_row_tile(rows), "a_fused": t_hk, "a_torch": t_torch,
                     "torch_over_fused": t_torch / t_hk, "min_max": spread}
            for key, fn in (("graph_fused", lambda: net(x)), ("graph_torch", lambda: torch_net(x))):
                try:
                    entry[key] = timeit(fn, iters=10, reps=10)
                except Exception as e:  # noqa: BLE001  (a capture that torch refuses is a finding, not a failure)
                    entry[key] = f"unmeasured: {type(e).__name__}: {str(e)[:200]}"
            result[f"forward_{name}_B{rows}"] = entry
            print(f"(a) {name} x {rows}: {entry}", flush=True)
    if args.no_trace:
        result["kernel_trace"] = {"unmeasured": "--no-trace"}
    else:
        trace = kernel_trace()
        if "unmeasured" not in trace:
            durations, at = trace["durations"], 0
            out = {"unit": f"ns per launch, median of the last {TRACE_CALLS // 2} of {TRACE_CALLS} calls"}
            for name, make, k, rows in CASES:
                net = make()
                ns = statistics.median(durations[at + TRACE_CALLS // 2:at + TRACE_CALLS])
                at += TRACE_CALLS
                out[f"{name}_B{rows}"] = {"kernel_ns": ns, "flop": flops(net, rows),
                                          "fraction_of_f32_matrix_peak": flops(net, rows) / (ns * 1e-9) / F32_MATRIX_PEAK}
            assert at == len(durations), (at, len(durations))
            trace = out
        result["kernel_trace"] = trace
        print(f"(b) {result['kernel_trace']}", flush=True)
    if args.no_simulate:
        result["simulate_configs4"] = {"unmeasured": "--no-simulate"}
    else:
        from hironaka_amd.trainer_api import HipTrainer
        trainer = HipTrainer(42, CONFIGS4)
        entry = {"unit": "ms per simulate(role), median of 3 after one warm-up"}
        for role in ("host", "agent"):
            for way, enabled in (("fused", True), ("torch", False)):
                for net in trainer.built_nets.values():
                    net.fused_enabled = enabled
                times = []
                for rep in range(4):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    trainer.simulate(7 + rep, role)
                    e1.record()
                    torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1))
                entry[f"{role}_{way}"] = statistics.median(times[1:])
                print(f"(c) simulate {role} {way}: {times}", flush=True)
            entry[f"{role}_torch_over_fused"] = entry[f"{role}_torch"] / entry[f"{role}_fused"]
        result["simulate_configs4"] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
