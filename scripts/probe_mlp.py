"""Dev probe: the eval-mode forward of create_mlp's Q-networks in one launch (hk_mlp_forward through
hironaka_amd.nets.FusedSequential) against the SAME modules as a plain nn.Sequential, float32.  HIP events around
warmed-up work, the median of repeated runs, the two ways alternating.

  (a) one forward of the 2 x 32, 8 x 256 and example-config nets (host head, (20,3) features) at batch 256, 4 096, 4 097 (either
      side of the row tile's crossover), 16 384 and 65 536: eagerly, and 10 calls captured into one graph and replayed
  (b) the kernel's own time from a `rocprofv3 --kernel-trace` run of its own (a fresh child process), with the achieved
      fraction of the 157.3 TF f32 matrix peak
  (c) FusedGame.collect per step at (20,3) x 65 536 for both roles with the example-config nets: fused nets against the
      same modules as plain nn.Sequential (the parent's path)

Usage:  python scripts/probe_mlp.py [--out profiles/mlp_probe.json] [--no-trace]"""
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
import torch
from torch import nn
from hironaka_amd import nets, ops
from hironaka_amd.core import HipPoints
from hironaka_amd.fused_game import FusedGame
from hironaka_amd.replay_buffer import ReplayBuffer
from probe_replay import alternate
from probe_stages import timeit

M, D = 20, 3
ARCHS = {"2x32": [32, 32], "8x256": [256] * 8,
         "example": [128, "b", {"repeat": 20, "net_arch": [256, "b"]}, 128, "b"]}
BATCHES = (256, 4096, 4097, 16384, 65536)  # 4 096 / 4 097: the last batch on 16-row tiles, the first on 64-row ones
F32_MATRIX_PEAK = 157.3e12
TRACE_CALLS = 20


def make(arch, role="host"):
    if role == "host":
        net = nets.create_mlp(nets.HostFeatureExtractor(M * D), arch, M * D, 2 ** D - D - 1)
    else:
        net = nets.create_mlp(nets.AgentFeatureExtractor(M * D + D), arch, M * D + D, D)
    return net.eval().cuda()


def plain(net):
    return nn.Sequential(*net.children()).eval()


def flops(net, batch):
    return 2 * batch * sum(m.in_features * m.out_features for m in net if isinstance(m, nn.Linear))


def child():
    """what the kernel trace sees: TRACE_CALLS forwards per net and batch"""
    with torch.inference_mode():
        for arch in ARCHS.values():
            net = make(arch)
            for batch in BATCHES:
                x = torch.rand(batch, M, D, device="cuda")
                for _ in range(TRACE_CALLS):
                    net(x)
                torch.cuda.synchronize()


def kernel_trace():
    """the durations in ns of the mlp kernel in launch order, from a rocprofv3 kernel trace of a child of its own"""
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
                    if "mlp_kernel" in row.get("Kernel_Name", ""):
                        start = int(row["Start_Timestamp"])
                        rows.append((start, int(row["End_Timestamp"]) - start))
        if not rows:
            return {"unmeasured": "no mlp kernel in the trace"}
        return {"durations": [d for _, d in sorted(rows)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_probe.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    if args.child:
        return child()
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "spec": [M, D],
              "unit": "us per eager call, median of 7 runs of 10 calls, the ways alternating; graph_*: us per call of 10 "
                      "calls captured into one graph and replayed 10 times"}
    with torch.inference_mode():
        for name, arch in ARCHS.items():
            net = make(arch)
            torch_net = plain(net)
            assert net.fused_reason is None
            for batch in BATCHES:
                x = torch.rand(batch, M, D, device="cuda")
                (t_hk, t_torch), spread = alternate([lambda: net(x), lambda: torch_net(x)], iters=10)
                entry = {"row_tile": ops.lib().hk_mlp_row_tile(batch), "a_fused": t_hk, "a_torch": t_torch,
                         "torch_over_fused": t_torch / t_hk, "min_max": spread}
                for key, fn in (("graph_fused", lambda: net(x)), ("graph_torch", lambda: torch_net(x))):
                    try:
                        entry[key] = timeit(fn, iters=10, reps=10)
                    except Exception as e:  # noqa: BLE001  (a capture that torch refuses is a finding, not a failure)
                        entry[key] = f"unmeasured: {type(e).__name__}: {str(e)[:200]}"
                result[f"forward_{name}_B{batch}"] = entry
                print(f"(a) {name} x {batch}: {entry}", flush=True)
    if args.no_trace:
        result["kernel_trace"] = {"unmeasured": "--no-trace"}
    else:
        trace = kernel_trace()
        if "unmeasured" not in trace:
            durations, at = trace["durations"], 0
            out = {"unit": f"ns per launch, median of the last {TRACE_CALLS // 2} of {TRACE_CALLS} calls"}
            for name, arch in ARCHS.items():
                net = make(arch)
                for batch in BATCHES:
                    ns = statistics.median(durations[at + TRACE_CALLS // 2:at + TRACE_CALLS])
                    at += TRACE_CALLS
                    out[f"{name}_B{batch}"] = {"kernel_ns": ns, "flop": flops(net, batch),
                                               "fraction_of_f32_matrix_peak": flops(net, batch) / (ns * 1e-9) / F32_MATRIX_PEAK}
            assert at == len(durations), (at, len(durations))
            trace = out
        result["kernel_trace"] = trace
        print(f"(b) {result['kernel_trace']}", flush=True)
    # (c) two moves in, as probe_replay.py: some games have finished
    B = BATCHES[-1]
    host, agent = make(ARCHS["example"], "host"), make(ARCHS["example"], "agent")
    games = {"fused": FusedGame(host, agent, log_time=False), "torch": FusedGame(plain(host), plain(agent), log_time=False)}
    pts = HipPoints(ops.generate_points(B, M, D, 20, seed=42))
    pts.get_newton_polytope()
    for _ in range(2):
        games["torch"].step(pts, "host", exploration_rate=0.2)
    P = pts.points.clone()
    for role in ("host", "agent"):
        shape = (M, D) if role == "host" else {"points": (M, D), "coords": (D,)}
        bufs = {k: ReplayBuffer(shape, D if role == "agent" else 2 ** D - D - 1, 1 << 20, "cuda") for k in games}

        def collect(k):
            pts.points.copy_(P)
            games[k].collect(pts, role, bufs[k], exploration_rate=0.2)
        (t_fused, t_torch), spread = alternate([lambda: collect("fused"), lambda: collect("torch")], iters=10)
        result[f"collect_{role}_B{B}"] = {"c_fused_nets": t_fused, "c_plain_sequential": t_torch,
                                          "torch_over_fused": t_torch / t_fused, "min_max": spread}
        print(f"(c) collect {role}: {result[f'collect_{role}_B{B}']}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
