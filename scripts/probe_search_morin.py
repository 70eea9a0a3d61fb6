"""Probe of hk_search_morin_tree (hironaka_amd.util.search_trees_morin): writes profiles/search_morin_probe.json (or the
path given as the first argument) and prints the same JSON line.

  thom4                    per finite host: the nodes of the whole thom_points_homogeneous(4) tree (19 points, dim 7,
                           weights all 1, the last row distinguished), the time of search_trees_morin on that root
                           (events around the whole call, median of 5 after a warm-up) and the reference's CPU seconds
                           for the same tree, which tests/golden/search_morin.npz carries as data
  batch_nodes_per_s        tree nodes / s over 2 048 seeded (8,5) roots with weights in 1..3 and a random distinguished
                           row, max_nodes = 2^13, states not kept; roots over the cap stop at NODE_LIMIT and their
                           recorded nodes count
  tree_batch_nodes_per_s   search_trees on the same roots in the same session, for orientation only: its trees are
                           other trees (no pruning, no lost points, no reposition)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from hironaka_amd import _abi as A
from hironaka_amd.host import WeakSpivakovsky, WeakSpivakovskyMinHitting, Zeillinger, ZeillingerLex
from hironaka_amd.util import search_trees, search_trees_morin

HOSTS = {"zeillinger": Zeillinger, "zeillinger_lex": ZeillingerLex, "weak_spivakovsky": WeakSpivakovsky,
         "weak_spivakovsky_min_hitting": WeakSpivakovskyMinHitting}


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / 1e3)
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "search_morin_probe.json")
    golden = np.load(os.path.join(ROOT, "tests", "golden", "search_morin.npz"))
    cases = [str(c) for c in golden["cases"]]
    ref_s = dict(zip((str(h) for h in golden["thom4_hosts"]), golden["thom4_ref_seconds"].tolist()))
    thom = {}
    for name, cls in HOSTS.items():
        i = cases.index(f"thom4_{name}_full")
        root = torch.as_tensor(golden[f"c{i}_root"], dtype=torch.float32, device="cuda").unsqueeze(0)
        wts = torch.as_tensor(golden[f"c{i}_weights"], device="cuda").unsqueeze(0)
        dst = torch.as_tensor(golden[f"c{i}_meta"][3:4], device="cuda")
        kw = dict(max_nodes=1 << 12, stack_nodes=1 << 10)
        r = search_trees_morin(root, wts, dst, cls(), **kw)  # warm-up
        assert int(r.status[0]) == 0 and int(r.count[0]) == len(golden[f"c{i}_ident"]) + 1
        t = timed(lambda: search_trees_morin(root, wts, dst, cls(), **kw), 5)
        thom[name] = {"nodes": int(r.count[0]), "gpu_s": float(np.median(t)), "gpu_runs_s": t,
                      "reference_cpu_s": ref_s[name]}

    rng = np.random.default_rng(2048)
    b, m, d = 2048, 8, 5
    roots = rng.integers(0, 21, (b, m, d)).astype(np.float32)
    count = rng.integers(2, m + 1, b)
    for i in range(b):
        roots[i, count[i]:] = -1.0
    dist = torch.as_tensor(rng.integers(0, count), device="cuda")
    wts = torch.as_tensor(rng.integers(1, 4, (b, d)), device="cuda")
    roots = torch.as_tensor(roots, device="cuda")
    host = Zeillinger()
    bk = dict(max_nodes=1 << 13, stack_nodes=1 << 12, states=False)
    rm = search_trees_morin(roots, wts, dist, host, **bk)  # warm-up
    tm = timed(lambda: search_trees_morin(roots, wts, dist, host, **bk), 5)
    rt = search_trees(roots, host, **bk)  # warm-up
    tt = timed(lambda: search_trees(roots, host, **bk), 5)
    sm, st = rm.status.cpu().numpy(), rt.status.cpu().numpy()
    res = {"thom4": thom, "batch_roots": b, "batch_shape": [m, d], "batch_max_nodes": 1 << 13, "batch_host": "zeillinger",
           "batch_nodes": int(rm.count.sum()), "batch_s": float(np.median(tm)),
           "batch_nodes_per_s": int(rm.count.sum()) / float(np.median(tm)),
           "batch_exact_roots": int((sm == 0).sum()),
           "batch_node_limit_roots": int(((sm & A.HK_SEARCH_NODE_LIMIT) != 0).sum()),
           "tree_batch_nodes": int(rt.count.sum()), "tree_batch_s": float(np.median(tt)),
           "tree_batch_nodes_per_s": int(rt.count.sum()) / float(np.median(tt)),
           "tree_batch_node_limit_roots": int(((st & A.HK_SEARCH_NODE_LIMIT) != 0).sum()),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
