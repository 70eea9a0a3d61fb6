"""
Generate tests/golden/search_depth.npz by RUNNING the reference's own `search_depth`
(hironaka/util/search.py:9-32) with its own ListPoints, Zeillinger and AllCoordHost.  Runs only
where the reference checkout exists; the resulting .npz (roots, depth, nodes per group) is what
travels.

The files are loaded one by one as make_golden.py does (the package __init__ files import jax).
Nodes are counted as calls of `host.select_coord`, with a subclass of the reference host that also
enforces a node cap: a seeded root whose tree is larger than the cap is dropped, not truncated.

Groups (name -> host, roots [N, m, d] float64 padded with -1 at the end, depth [N], nodes [N]):
    lit4   Zeillinger   test/testSearch.py:13-24 (the disabled 5552 case) and :27-33 (== 6)
    lit3   Zeillinger   test/testSearch.py:35-40
    z3     Zeillinger   seeded dim-3 roots, 2-20 points, values <= 20
    z4     Zeillinger   seeded dim-4 roots, 2-10 points, values <= 20
    a2     AllCoordHost seeded dim-2 roots, 2-10 points, values <= 20

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_search_depth_golden.py
"""
import os
import sys
import time

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _load, load_reference  # noqa: E402

NODE_CAP = 30000

LITERALS = {
    "lit4": [[(7, 5, 3, 8), (8, 1, 8, 18), (8, 3, 17, 8), (11, 11, 1, 19), (11, 12, 18, 6), (16, 11, 5, 6)],
             [(0, 1, 0, 1), (0, 2, 0, 0), (1, 0, 0, 1), (1, 0, 1, 0), (1, 1, 0, 0), (2, 0, 0, 0)]],
    "lit3": [[[3, 5, 8], [5, 2, 6], [1, 3, 6], [3, 5, 3], [7, 3, 3], [1, 6, 3], [1, 0, 6], [5, 1, 6], [7, 3, 0],
              [6, 7, 7]]],
}


class _TooLarge(Exception):
    pass


def counting(host_cls, cap):
    class Counting(host_cls):
        def __init__(self):
            super().__init__()
            self.calls = 0

        def select_coord(self, points, debug=False):
            self.calls += 1
            if cap is not None and self.calls > cap:
                raise _TooLarge()
            return super().select_coord(points, debug=debug)

    return Counting


def run(ref, search_depth, host_cls, rows, cap):
    host = counting(host_cls, cap)()
    pts = ref.ListPoints([[list(map(float, r)) for r in rows]])
    return search_depth(pts, host), host.calls


def pad(rows_list, m, d):
    out = np.full((len(rows_list), m, d), -1.0)
    for i, rows in enumerate(rows_list):
        out[i, :len(rows)] = np.asarray(rows, dtype=np.float64)
    return out


def seeded(ref, search_depth, host_cls, rng, want, m_lo, m_hi, d, max_value, cap):
    roots, depth, nodes = [], [], []
    tried = 0
    while len(roots) < want:
        tried += 1
        n = int(rng.integers(m_lo, m_hi + 1))
        rows = rng.integers(0, max_value + 1, (n, d)).tolist()
        try:
            r, c = run(ref, search_depth, host_cls, rows, cap)
        except _TooLarge:
            continue
        roots.append(rows)
        depth.append(r)
        nodes.append(c)
    return pad(roots, m_hi, d), np.asarray(depth, np.int64), np.asarray(nodes, np.int64), tried


def main():
    t0 = time.time()
    ref = load_reference()
    search = _load("hironaka.util.search", "hironaka/util/search.py")
    Z, ALL = ref.host.Zeillinger, ref.host.AllCoordHost
    rec = {}
    for name, roots in LITERALS.items():
        d = len(roots[0][0])
        m = max(len(r) for r in roots)
        res = [run(ref, search.search_depth, Z, r, None) for r in roots]
        rec[f"{name}_roots"] = pad(roots, m, d)
        rec[f"{name}_depth"] = np.asarray([r for r, _ in res], np.int64)
        rec[f"{name}_nodes"] = np.asarray([c for _, c in res], np.int64)
        rec[f"{name}_host"] = np.asarray("zeillinger")
        print(f"{name}: depth {rec[f'{name}_depth'].tolist()} nodes {rec[f'{name}_nodes'].tolist()} "
              f"({time.time() - t0:.1f} s)")
    rng = np.random.default_rng(20261015)
    for name, host_cls, host_name, want, m_lo, m_hi, d in (("z3", Z, "zeillinger", 120, 2, 20, 3),
                                                           ("z4", Z, "zeillinger", 80, 2, 10, 4),
                                                           ("a2", ALL, "all_coord", 40, 2, 10, 2)):
        roots, depth, nodes, tried = seeded(ref, search.search_depth, host_cls, rng, want, m_lo, m_hi, d, 20,
                                            NODE_CAP)
        rec[f"{name}_roots"], rec[f"{name}_depth"], rec[f"{name}_nodes"] = roots, depth, nodes
        rec[f"{name}_host"] = np.asarray(host_name)
        print(f"{name}: {want} of {tried} roots within {NODE_CAP} nodes; depth max {depth.max()}, "
              f"nodes max {nodes.max()} sum {nodes.sum()} ({time.time() - t0:.1f} s)")
    rec["groups"] = np.asarray(list(LITERALS) + ["z3", "z4", "a2"])
    np.savez_compressed(os.path.join(OUT, "search_depth.npz"), **rec)
    print(f"wrote search_depth.npz in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
