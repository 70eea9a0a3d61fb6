"""Dev probe: nets.FusedSequential.fused_training -- the training-mode forward and the backward of a create_mlp stack as
one hk_train_mlp_forward / hk_train_mlp_backward launch per layer -- against the same module with the switch off, which
is the parent commit's path (torch's forward and backward).  HIP events around warmed-up eager calls, the median of 7
runs of 10 calls, the ways alternating; and the same calls replayed from a captured graph, which leaves the device's time
without the host's share of an eager call.

  (a) forward + backward alone: q = net(x); q.backward(g) with a sparse g as hk_dqn_td emits it
  (b) one whole fit step: both nets, TD, backward, optim.Adam.clip_and_step, Polyak
  on the reference's example config at 256 and 1 024 rows, its test config at 256, and 8 x 256 without batch norm at 256
  (c) the kernels' durations from a `rocprofv3 --kernel-trace` run of its own (a fresh child process that does nothing
      but forward + backward of the example config at 256 rows)
Accepted (probe_optim.py's condition) where, on the example config at 256 rows, the new median is at or below the off
path's median plus the off path's own spread, eagerly and from a graph.

Usage:  python scripts/probe_mlp_train.py [--out profiles/mlp_train_probe.json] [--no-trace]"""
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
from hironaka_amd import dqn, nets, optim
from probe_replay import alternate
from probe_stages import timeit

OBS_DIM, NUM_ACTIONS = 60, 4
ARCHS = {"example": [128, "b", {"repeat": 20, "net_arch": [256, "b"]}, 128, "b"],
         "test": [16, "b", {"repeat": 2, "net_arch": [32, "b"]}, 16, "b"],
         "mlp_8x256": [256] * 8}
CASES = [("example", 256), ("example", 1024), ("test", 256), ("mlp_8x256", 256)]


def make(arch, training):
    torch.manual_seed(0)
    net = nets.create_mlp(nets.HostFeatureExtractor(OBS_DIM), ARCHS[arch], OBS_DIM, NUM_ACTIONS,
                          fused_training=training).cuda().train()
    for p in net.parameters():  # static gradients, as a captured step needs them
        p.grad = torch.zeros_like(p)
    return net


def batch_of(rows):
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda *shape: torch.rand(*shape, device="cuda", generator=g)  # noqa: E731
    actions = (rand(rows, 1) * NUM_ACTIONS).to(torch.int32).clamp_(0, NUM_ACTIONS - 1)
    grad = torch.zeros(rows, NUM_ACTIONS, device="cuda").scatter_(1, actions.long(), (rand(rows, 1) - 0.5) / rows)
    return (rand(rows, 20, 3), actions, (rand(rows, 1) * 3).floor() - 1, rand(rows, 1) < 0.3, rand(rows, 20, 3)), grad


def forward_backward(net, x, grad):
    def fn():
        net(x).backward(grad)
    return fn


def fit_step(q_net, target, opt, batch):
    observations, actions, rewards, dones, next_observations = batch

    def fn():
        with torch.no_grad():
            next_q = target(next_observations)
        loss = dqn.td_loss(q_net(observations), next_q, actions, rewards, dones, 0.99)
        opt.zero_grad(set_to_none=False)
        loss.backward()
        opt.clip_and_step(1.0)
        dqn.update_target_net(q_net, target, 0.01)
    return fn


def compare(fn_on, fn_off):
    (t_on, t_off), spread = alternate([fn_on, fn_off], iters=10)
    entry = {"eager_on": t_on, "eager_off": t_off, "eager_off_over_on": t_off / t_on, "eager_min_max": spread,
             "eager_off_spread": spread[1][1] - spread[1][0]}
    entry["eager_accepted"] = bool(t_on <= t_off + entry["eager_off_spread"])
    graphs = {"on": [], "off": []}
    for _ in range(3):
        for key, fn in (("on", fn_on), ("off", fn_off)):
            graphs[key].append(timeit(fn, iters=4, reps=10))
    g_on, g_off = statistics.median(graphs["on"]), statistics.median(graphs["off"])
    entry.update(graph_on=g_on, graph_off=g_off, graph_off_over_on=g_off / g_on,
                 graph_min_max=[(min(v), max(v)) for v in (graphs["on"], graphs["off"])],
                 graph_off_spread=max(graphs["off"]) - min(graphs["off"]))
    entry["graph_accepted"] = bool(g_on <= g_off + entry["graph_off_spread"])
    return entry


def child():
    """what the kernel trace sees: 20 forward + backward passes of the example config at 256 rows"""
    net = make("example", True)
    batch, grad = batch_of(256)
    for _ in range(20):
        net(batch[0]).backward(grad)
    torch.cuda.synchronize()


def kernel_trace():
    """{"forward" / "backward": the kernels' durations in ns in launch order} from a rocprofv3 kernel trace of a child of
    its own"""
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
                    for short in ("forward", "backward"):
                        if f"mlp_train_{short}_kernel" in name:
                            start = int(row["Start_Timestamp"])
                            rows.setdefault(short, []).append((start, int(row["End_Timestamp"]) - start))
        if sorted(rows) != ["backward", "forward"]:
            return {"unmeasured": "no training kernel in the trace"}
        out = {"unit": "ns; per pass: the 23 launches of one pass added, median of the last 10 of 20 passes"}
        for short, v in rows.items():
            d = [x for _, x in sorted(v)]
            layers = len(d) // 20
            passes = [sum(d[k * layers:(k + 1) * layers]) for k in range(20)]
            last = d[-layers:]
            out[short] = {"launches_per_pass": layers, "per_pass": statistics.median(passes[10:]),
                          "per_launch_min_median_max": [min(last), statistics.median(last), max(last)]}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_train_probe.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child()
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float32",
              "unit": "us per call; eager_*: median of 7 runs of 10 calls, on and off alternating; graph_*: 4 calls "
                      "captured into one graph and replayed 10 times, median of 3 such graphs each, alternating; on: "
                      "fused_training, off: torch's forward and backward (the parent's path)"}
    for arch, rows in CASES:
        batch, grad = batch_of(rows)
        on, off = make(arch, True), make(arch, False)
        entry = {"forward_backward": compare(forward_backward(on, batch[0], grad), forward_backward(off, batch[0], grad))}
        assert on.fused_last_reason is None and off.fused_last_reason is not None
        steps = []
        for training in (True, False):
            q_net, target = make(arch, training), make(arch, training)
            steps.append(fit_step(q_net, target, optim.Adam(q_net.parameters(), lr=1e-3), batch))
        entry["fit_step"] = compare(*steps)
        result[f"{arch}_{rows}"] = entry
        print(f"{arch}_{rows}: {entry}", flush=True)
    flagship = result["example_256"]
    result["accepted"] = all(flagship[part][f"{way}_accepted"] for part in ("forward_backward", "fit_step")
                             for way in ("eager", "graph"))
    result["kernel_trace"] = {"unmeasured": "--no-trace"} if args.no_trace else kernel_trace()
    print(f"kernel trace: {result['kernel_trace']}", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
