"""Dev probe: the gradient-free forward of CustomNet in two launches (hk_customnet_forward through
hironaka_amd.net.CustomNet: one tower per row) against the SAME module with `fused_enabled = False` (the reference's
formulation: every tower on every row, the mask, the sum), float32.  HIP events around warmed-up work, the median of
repeated runs, the ways alternating in one process.

  (a) one forward at: the reference's test config (5 points in dimension 3, [32, 32] residue towers, 100 rows);
      train/jax_mcts.yml (5 points, [128] x 8 dense towers, 512 rows); 20 points, [128] x 8 dense towers, 8 192 rows --
      both roles, eagerly, and 10 calls captured into one graph and replayed.  The rows are observations a `simulate` at
      that shape produces (seeded; their point counts are recorded).  Beside each: hk_pvnet_forward on ONE DenseResNet /
      DenseNet of the same net_arch and rows -- the gap to it is the cost of grouping and of partial tiles
  (b) the kernels' own times from a `rocprofv3 --kernel-trace` run of its own (a fresh child process)
  (c) one whole HipTrainer.simulate at train/jax_mcts.yml's shapes (512 games, 100 simulations per move, 40 moves), fused
      on and off

Usage:  python scripts/probe_customnet.py [--out profiles/customnet_probe.json] [--no-trace] [--no-simulate]"""
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
from hironaka_amd import net as N
from hironaka_amd import ops
from hironaka_amd.trainer_api import HipTrainer
from probe_replay import alternate
from probe_stages import timeit

# (name, (m, d), net_arch, net_type, rows)
CASES = [
    ("test_2x32", (5, 3), [32, 32], "custom", 100),
    ("mcts_8x128", (5, 3), [128] * 8, "custom_dense", 512),
    ("twenty_8x128", (20, 3), [128] * 8, "custom_dense", 8192),
]
ROLES = ("host", "agent")
TRACE_CALLS = 20
SEED = 20261021
MCTS = {"eval_batch_size": 512, "max_num_points": 5, "dimension": 3, "max_length_game": 40, "max_value": 20,
        "max_grad_norm": 0.5, "scale_observation": False, "reposition": False, "gumbel_scale": 0.3, "net_type": "custom_dense",
        "num_evaluations": 100, "num_evaluations_as_opponent": 100, "max_num_considered_actions": 10, "discount": 0.98,
        "host": {"batch_size": 128, "net_arch": [128] * 8, "optim": {"name": "adam", "args": {"learning_rate": 0.001}}},
        "agent": {"batch_size": 128, "net_arch": [128] * 8, "optim": {"name": "adam", "args": {"learning_rate": 0.001}}}}


def trainer_for(spec, arch, net_type, games=512, moves=20):
    cfg = dict(MCTS, max_num_points=spec[0], dimension=spec[1], net_type=net_type, eval_batch_size=games,
               max_length_game=moves, num_evaluations=4, num_evaluations_as_opponent=2, scale_observation=True, reposition=True,
               host={"net_arch": list(arch)}, agent={"net_arch": list(arch)})
    return HipTrainer(SEED, cfg, custom_net=True)


def rows_of(trainer, role, rows):
    """`rows` observations of simulate(SEED, role), drawn with a seeded generator, and their point counts"""
    obs = trainer.simulate(SEED, role)[0]
    pick = torch.randint(0, obs.shape[0], (rows,), generator=torch.Generator().manual_seed(SEED)).to(obs.device)
    x = obs[pick].contiguous()
    m, d = trainer.spec
    counts = torch.bincount((x[:, : m * d: d] >= 0).sum(1), minlength=m + 1).tolist()
    return x, counts


def one_tower(net, role):
    """a DenseResNet / DenseNet of the same net_arch and input width"""
    block = type(net.blocks[0])
    return N.DenseResNet(net.output_size, net.net_arch, spec=net.spec, role=role, block_cls=block).cuda()


def child():
    """what the kernel trace sees: every case's rows first (their simulate calls the networks too), then TRACE_CALLS
    forwards per case and role -- the trace's LAST launches, in the order of CASES x ROLES"""
    work = []
    with torch.no_grad():
        for _, spec, arch, net_type, rows in CASES:
            trainer = trainer_for(spec, arch, net_type)
            for role in ROLES:
                work.append((trainer.built_nets[role], rows_of(trainer, role, rows)[0]))
        torch.cuda.synchronize()
        for net, x in work:
            for _ in range(TRACE_CALLS):
                net(x)
        torch.cuda.synchronize()


def kernel_trace():
    """the durations in ns of the two kernels in launch order, from a rocprofv3 kernel trace of a child of its own"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child"]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        if done.returncode != 0:
            return {"unmeasured": f"rocprofv3 ended with {done.returncode}: {done.stdout.decode()[-300:]}"}
        found = {"group": [], "forward": []}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    name = row.get("Kernel_Name", "")
                    key = "group" if "customnet_group_kernel" in name else "forward" if "customnet_kernel" in name else None
                    if key:
                        start = int(row["Start_Timestamp"])
                        found[key].append((start, int(row["End_Timestamp"]) - start))
        if not found["forward"]:
            return {"unmeasured": "no customnet kernel in the trace"}
        return {k: [d for _, d in sorted(v)] for k, v in found.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "customnet_probe.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--no-simulate", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    if args.child:
        return child()
    result = {"device": torch.cuda.get_device_name(0), "dtype": "float32", "seed": SEED,
              "unit": "us per eager call, median of 7 runs of 10 calls, the ways alternating; graph_*: us per call of 10 "
                      "calls captured into one graph and replayed 10 times; one_tower: hk_pvnet_forward on one DenseResNet "
                      "/ DenseNet of the same net_arch and rows"}
    marks = []  # (case, role, rows): the order of the child's launches
    with torch.no_grad():
        for name, spec, arch, net_type, rows in CASES:
            trainer = trainer_for(spec, arch, net_type)
            for role in ROLES:
                x, counts = rows_of(trainer, role, rows)
                net = trainer.built_nets[role]
                tower = one_tower(net, role)
                net.fused_enabled = True
                fused = lambda: net(x)  # noqa: E731

                def plain():
                    net.fused_enabled = False
                    try:
                        return net(x)
                    finally:
                        net.fused_enabled = True
                single = lambda: tower(x)  # noqa: E731
                fused(), plain(), single()
                net(x)
                assert net.fused_last_reason is None and tower.fused_last_reason is None
                (t_hk, t_torch, t_one), spread = alternate([fused, plain, single], iters=10)
                entry = {"rows": rows, "point_counts": counts, "row_tile": ops.lib().hk_mlp_row_tile(rows),
                         "a_fused": t_hk, "a_torch": t_torch, "a_one_tower": t_one, "torch_over_fused": t_torch / t_hk,
                         "fused_over_one_tower": t_hk / t_one, "min_max": spread}
                for key, fn in (("graph_fused", fused), ("graph_torch", plain), ("graph_one_tower", single)):
                    try:
                        entry[key] = timeit(fn, iters=10, reps=10)
                    except Exception as e:  # noqa: BLE001  (a capture that torch refuses is a finding, not a failure)
                        entry[key] = f"unmeasured: {type(e).__name__}: {str(e)[:200]}"
                if all(isinstance(entry[k], float) for k in ("graph_fused", "graph_torch", "graph_one_tower")):
                    entry["graph_torch_over_fused"] = entry["graph_torch"] / entry["graph_fused"]
                    entry["graph_fused_over_one_tower"] = entry["graph_fused"] / entry["graph_one_tower"]
                result[f"forward_{name}_{role}_B{rows}"] = entry
                marks.append(f"{name}_{role}_B{rows}")
                print(f"(a) {name} {role} x {rows}: {entry}", flush=True)
    if args.no_trace:
        result["kernel_trace"] = {"unmeasured": "--no-trace"}
    else:
        trace = kernel_trace()
        if "unmeasured" not in trace:
            # the child's timed forwards are the trace's last len(marks) * TRACE_CALLS launches of either kernel
            out = {"unit": f"ns per launch, median of the last {TRACE_CALLS // 2} of {TRACE_CALLS} calls"}
            for i, mark in enumerate(marks):
                entry = {}
                for key in ("group", "forward"):
                    mine = trace[key][len(trace[key]) - (len(marks) - i) * TRACE_CALLS:][:TRACE_CALLS]
                    entry[f"{key}_kernel_ns"] = statistics.median(mine[TRACE_CALLS // 2:])
                out[mark] = entry
            trace = out
        result["kernel_trace"] = trace
        print(f"(b) {result['kernel_trace']}", flush=True)
    if args.no_simulate:
        result["simulate_mcts"] = {"unmeasured": "--no-simulate"}
    else:
        trainer = HipTrainer(42, MCTS, custom_net=True)
        entry = {"unit": "ms per simulate(role), median of 2 after one warm-up"}
        for role in ROLES:
            for way, enabled in (("fused", True), ("torch", False)):
                for net in trainer.built_nets.values():
                    net.fused_enabled = enabled
                times = []
                for rep in range(3):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    trainer.simulate(7 + rep, role)
                    e1.record()
                    torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1))
                entry[f"{role}_{way}"] = statistics.median(times[1:])
                print(f"(c) simulate {role} {way}: {times}", flush=True)
            entry[f"{role}_torch_over_fused"] = entry[f"{role}_torch"] / entry[f"{role}_fused"]
        result["simulate_mcts"] = entry
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
