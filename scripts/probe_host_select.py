"""Probe of hk_host_select and of hk_search_depth with ZeillingerLex: prints one JSON line.

  select[shape][host]_us   hk_host_select per call, float32: median over 5 windows of a host clock around N calls
                           that ends in a device synchronise, divided by N (each window >= ~0.1 s)
  select[shape][copy]_us   a device copy of the same state (read + write of B*m*d floats), the bandwidth yardstick
  select[shape][zeillinger_list]_us  hk_zeillinger(HK_SEM_LIST) on the same batch
  search_nodes_per_s       search_depths nodes / s on probe_search_depth.py's batch (2 048 seeded (10,4) roots,
                           values <= 20, max_nodes = 2^18), for Zeillinger and ZeillingerLex in the same process
Shapes: (20,3) x 65 536 and (50,4) x 262 144 games, seeded values < 20 with 25 % padding rows.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hironaka_amd import _abi as A
from hironaka_amd import ops
from hironaka_amd._lib import check, lib
from hironaka_amd.host import Zeillinger, ZeillingerLex
from hironaka_amd.util import search_depths


def per_call_us(fn, n, windows=5):
    fn()  # warm-up
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / n * 1e6)
    return float(np.median(out)), out


def select_probe(b, m, d, n):
    rng = np.random.default_rng(b + m + d)
    p = rng.integers(0, 20, (b, m, d)).astype(np.float32)
    p[rng.random((b, m)) < 0.25] = -1.0
    pts = torch.as_tensor(p, device="cuda")
    dst = torch.empty_like(pts)
    out = torch.empty(b, dtype=torch.int32, device="cuda")
    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    res = {"games": b, "shape": [m, d], "state_bytes": b * m * d * 4}

    def sel(code):
        return lambda: check(L.hk_host_select(pts.data_ptr(), m * d, out.data_ptr(), b, m, d, A.HK_F32, code, stream))

    for name, code in ops.HOSTS.items():
        res[f"{name}_us"], res[f"{name}_runs_us"] = per_call_us(sel(code), n)
    res["copy_us"], res["copy_runs_us"] = per_call_us(lambda: dst.copy_(pts), n)
    res["zeillinger_list_us"], res["zeillinger_list_runs_us"] = per_call_us(
        lambda: check(L.hk_zeillinger(pts.data_ptr(), m * d, out.data_ptr(), b, m, d, A.HK_F32, A.HK_SEM_LIST,
                                      stream)), n)
    for name in ("weak_spivakovsky", "weak_spivakovsky_min_hitting"):
        res[f"{name}_over_copy"] = res[f"{name}_us"] / res["copy_us"]
    res["zeillinger_lex_over_zeillinger_list"] = res["zeillinger_lex_us"] / res["zeillinger_list_us"]
    return res


def search_probe():
    rng = np.random.default_rng(2048)  # probe_search_depth.py's batch
    b, m, d = 2048, 10, 4
    roots = rng.integers(0, 21, (b, m, d)).astype(np.float32)
    count = rng.integers(2, m + 1, b)
    for i in range(b):
        roots[i, count[i]:] = -1.0
    roots = torch.as_tensor(roots, device="cuda")
    kw = dict(max_nodes=1 << 18, stack_nodes=1 << 12)
    res = {}
    for name, host in (("zeillinger", Zeillinger()), ("zeillinger_lex", ZeillingerLex())):
        r = search_depths(roots, host, **kw)  # warm-up
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            search_depths(roots, host, **kw)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        nodes = int(r.nodes.sum())
        res[name] = {"nodes": nodes, "s": float(np.median(times)), "runs_s": times,
                     "nodes_per_s": nodes / float(np.median(times)),
                     "exact_roots": int((r.status == 0).sum()), "depth_max": int(r.depth.max())}
    return res


def main():
    out = {"select": {"20x3": select_probe(65536, 20, 3, 400), "50x4": select_probe(262144, 50, 4, 60)},
           "search_nodes_per_s": search_probe(), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
