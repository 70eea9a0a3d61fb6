"""Probe of hk_search_depth (hironaka_amd.util.search_depth): prints one JSON line.

  root_5552_s      wall time of search_depth on test/testSearch.py:13-24's root (depth 5552, 564 448 nodes),
                   median of 5 after a warm-up, device-synchronised (the reference takes 35.7 s on a CPU)
  batch_nodes_per_s  visited nodes / s over 2 048 seeded (10,4) roots, values <= 20, max_nodes = 2^18
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hironaka_amd import _abi as A
from hironaka_amd.host import Zeillinger
from hironaka_amd.util import search_depth, search_depths

ROOT_5552 = [[7, 5, 3, 8], [8, 1, 8, 18], [8, 3, 17, 8], [11, 11, 1, 19], [11, 12, 18, 6], [16, 11, 5, 6]]


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def main():
    host = Zeillinger()
    root = torch.tensor(ROOT_5552, dtype=torch.float32, device="cuda")
    assert search_depth(root, host) == 5552  # warm-up
    t5552 = wall(lambda: search_depth(root, host), 5)

    rng = np.random.default_rng(2048)
    b, m, d = 2048, 10, 4
    roots = rng.integers(0, 21, (b, m, d)).astype(np.float32)
    count = rng.integers(2, m + 1, b)
    for i in range(b):
        roots[i, count[i]:] = -1.0
    roots = torch.as_tensor(roots, device="cuda")
    kw = dict(max_nodes=1 << 18, stack_nodes=1 << 12)
    r = search_depths(roots, host, **kw)  # warm-up
    tb = wall(lambda: search_depths(roots, host, **kw), 3)
    nodes = int(r.nodes.sum())
    st = r.status.cpu().numpy()
    print(json.dumps({
        "root_5552_s": float(np.median(t5552)), "root_5552_runs_s": t5552,
        "batch_roots": b, "batch_shape": [m, d], "batch_max_nodes": 1 << 18, "batch_nodes": nodes,
        "batch_s": float(np.median(tb)), "batch_nodes_per_s": nodes / float(np.median(tb)),
        "batch_exact_roots": int((st == 0).sum()),
        "batch_node_limit_roots": int(((st & A.HK_SEARCH_NODE_LIMIT) != 0).sum()),
        "batch_stack_limit_roots": int(((st & A.HK_SEARCH_STACK_LIMIT) != 0).sum()),
        "batch_inexact_roots": int(((st & A.HK_SEARCH_INEXACT) != 0).sum()),
        "batch_nodes_max": int(r.nodes.max()), "batch_depth_max": int(r.depth.max()),
        "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
