"""Probe of hk_search_game_tree (hironaka_amd.util.search_trees): prints one JSON line.

  root_5552_tree_s         wall time of the whole tree of test/testSearch.py:13-24's root (1 128 897 nodes, 564 448
                           expanded), states kept, median of 3 after a warm-up, device-synchronised
  root_5552_tree_nostates_s  the same without the states output
  root_5552_depth_s        search_depth on the same root, same session (traversal alone, no records)
  batch_nodes_per_s        tree nodes / s over the 2 048 seeded (10,4) roots of probe_search_depth.py, max_nodes = 2^15,
                           states not kept; roots over the cap stop at NODE_LIMIT and their recorded nodes count
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
from hironaka_amd.util import search_depth, search_depths, search_trees

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
    root = torch.tensor([ROOT_5552], dtype=torch.float32, device="cuda")
    kw = dict(max_nodes=1 << 21, stack_nodes=1 << 16)
    r = search_trees(root, host, **kw)  # warm-up
    assert int(r.status[0]) == 0 and int(r.count[0]) == 1128897
    t_tree = wall(lambda: search_trees(root, host, **kw), 3)
    t_nost = wall(lambda: search_trees(root, host, states=False, **kw), 3)
    assert search_depth(root, host) == 5552
    t_depth = wall(lambda: search_depth(root, host), 3)

    rng = np.random.default_rng(2048)
    b, m, d = 2048, 10, 4
    roots = rng.integers(0, 21, (b, m, d)).astype(np.float32)
    count = rng.integers(2, m + 1, b)
    for i in range(b):
        roots[i, count[i]:] = -1.0
    roots = torch.as_tensor(roots, device="cuda")
    bk = dict(max_nodes=1 << 15, stack_nodes=1 << 12, states=False)
    rb = search_trees(roots, host, **bk)  # warm-up
    tb = wall(lambda: search_trees(roots, host, **bk), 3)
    nodes = int(rb.count.sum())
    st = rb.status.cpu().numpy()
    print(json.dumps({
        "root_5552_tree_s": float(np.median(t_tree)), "root_5552_tree_runs_s": t_tree,
        "root_5552_tree_nostates_s": float(np.median(t_nost)),
        "root_5552_depth_s": float(np.median(t_depth)),
        "batch_roots": b, "batch_shape": [m, d], "batch_max_nodes": 1 << 15, "batch_nodes": nodes,
        "batch_s": float(np.median(tb)), "batch_nodes_per_s": nodes / float(np.median(tb)),
        "batch_exact_roots": int((st == 0).sum()),
        "batch_node_limit_roots": int(((st & A.HK_SEARCH_NODE_LIMIT) != 0).sum()),
        "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
