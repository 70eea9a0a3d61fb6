"""Probe of hk_spivakovsky_select: writes profiles/spivakovsky_probe.json (or --out) and prints the same JSON line.

  [shape][host]_us               hk_spivakovsky_select per launch, float32: median over 5 windows of a host clock
                                 around N launches that ends in a device synchronise, divided by N
  [shape][weak_spivakovsky]_us   ops.host_select(..., "weak_spivakovsky")'s launch on the same tensors
  [shape][copy]_us               a device copy of the same state (read + write of B*m*d floats), the bandwidth yardstick
Shapes: (20,3) x 65 536, (50,4) x 262 144 and (64,6) x 4 096 games, seeded values < 20 with 25 % padding rows.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from hironaka_amd import _abi as A
from hironaka_amd import ops
from hironaka_amd._lib import check, lib


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


def probe(b, m, d, n):
    rng = np.random.default_rng(b + m + d)
    p = rng.integers(0, 20, (b, m, d)).astype(np.float32)
    p[rng.random((b, m)) < 0.25] = -1.0
    pts = torch.as_tensor(p, device="cuda")
    dst = torch.empty_like(pts)
    out = torch.empty(b, dtype=torch.int32, device="cuda")
    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    res = {"games": b, "shape": [m, d], "state_bytes": b * m * d * 4, "launches_per_window": n}
    for name, code in ops.SPIVAKOVSKY_HOSTS.items():
        res[f"{name}_us"], res[f"{name}_runs_us"] = per_call_us(
            lambda: check(L.hk_spivakovsky_select(pts.data_ptr(), m * d, out.data_ptr(), b, m, d, A.HK_F32, code, 1, 0,
                                                  0, stream)), n)
    res["weak_spivakovsky_us"], res["weak_spivakovsky_runs_us"] = per_call_us(
        lambda: check(L.hk_host_select(pts.data_ptr(), m * d, out.data_ptr(), b, m, d, A.HK_F32,
                                       A.HK_HOST_WEAK_SPIVAKOVSKY, stream)), n)
    res["copy_us"], res["copy_runs_us"] = per_call_us(lambda: dst.copy_(pts), n)
    for name in ops.SPIVAKOVSKY_HOSTS:
        res[f"{name}_over_copy"] = res[f"{name}_us"] / res["copy_us"]
        res[f"{name}_over_weak_spivakovsky"] = res[f"{name}_us"] / res["weak_spivakovsky_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spivakovsky_probe.json"))
    args = ap.parse_args()
    out = {"20x3": probe(65536, 20, 3, 200), "50x4": probe(262144, 50, 4, 20), "64x6": probe(4096, 64, 6, 100),
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
