"""
Generate tests/golden/search_tree.npz by RUNNING the reference's own `search_tree` (hironaka/util/search.py:35-50)
with its own ListPoints and hosts, into a stub tree that records every `create_node` call.  Runs only where the
reference checkout exists; the resulting .npz is what travels.

The files are loaded one by one as make_golden.py does (the package __init__ files import jax).  The recursion of
`search_tree` is one Python frame per tree level, so the recursion limit is raised.

Cases (index i; `cases` lists the names):
    c{i}_root    [m, d] float64       the root, the reference's row order kept (no padding)
    c{i}_meta    [3] int64            max_size (-1: the whole tree, run with a max_size above any tree here), the
                                      tree size s0 before the call, curr_node
    c{i}_host    str                  a key of hironaka_amd.ops.SEARCH_HOSTS
    c{i}_ident   [n] int64            identifiers of the created nodes in creation order (empty: the call returned None)
    c{i}_parent  [n] int64            their parents' identifiers
    c{i}_states  [n, m, d] int32      their states (ListPoints.points[0]), padded with -1 rows at the end
    lit_str      [107] str            str(data) of the test/testSearch.py:42-50 literal's nodes at max_size=100

Cases: the test/testSearch.py:42-50 literal at max_size=100 and in full (Zeillinger); the ROOT_6 root of
test/testSearch.py:27-33 in full; seeded dim-2..5 roots under all five deterministic hosts at max_size in
{0, 1, 7, 100, full}; the literal at max_size=100 below node 3 of a tree that already holds 5 nodes.  Roots whose
full tree exceeds NODE_CAP nodes, or where the reference raises, are skipped.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_search_tree_golden.py
"""
import os
import sys
import time

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, _load, load_reference  # noqa: E402

HOSTS = {"zeillinger": "Zeillinger", "all_coord": "AllCoordHost", "zeillinger_lex": "ZeillingerLex",
         "weak_spivakovsky": "WeakSpivakovsky", "weak_spivakovsky_min_hitting": "WeakSpivakovskyMinHitting"}
LITERAL = [[0, 0, 4], [5, 0, 1], [1, 5, 1], [0, 25, 0]]
ROOT_6 = [[0, 1, 0, 1], [0, 2, 0, 0], [1, 0, 0, 1], [1, 0, 1, 0], [1, 1, 0, 0], [2, 0, 0, 0]]
SIZES = (0, 1, 7, 100, None)
NODE_CAP = 3000
FULL = 10 ** 9  # max_size of a "full" run


class StubTree:
    """size() and create_node(tag, identifier, parent=, data=), as treelib's Tree; records the calls"""

    def __init__(self, n0=1):
        self.calls = [(i, i - 1 if i else None, None) for i in range(n0)]

    def size(self):
        return len(self.calls)

    def create_node(self, tag, identifier, parent=None, data=None):
        assert tag == identifier == len(self.calls)
        self.calls.append((identifier, parent, data))


def run(ref, search_tree, host_name, rows, max_size, n0=1, curr=0):
    tree = StubTree(n0)
    pts = ref.ListPoints([[list(r) for r in rows]])
    out = search_tree(pts, tree, curr, getattr(ref.host, HOSTS[host_name])(), max_size=FULL if max_size is None
                      else max_size)
    new = tree.calls[n0:]
    assert (out is None) == (len(new) == 0)
    return new


def record(rec, i, rows, host_name, max_size, n0, curr, new):
    m, d = len(rows), len(rows[0])
    rec[f"c{i}_root"] = np.asarray(rows, np.float64)
    rec[f"c{i}_meta"] = np.asarray([-1 if max_size is None else max_size, n0, curr], np.int64)
    rec[f"c{i}_host"] = np.asarray(host_name)
    rec[f"c{i}_ident"] = np.asarray([c[0] for c in new], np.int64)
    rec[f"c{i}_parent"] = np.asarray([c[1] for c in new], np.int64)
    st = np.full((len(new), m, d), -1, np.int32)
    for j, c in enumerate(new):
        p = c[2].points[0]
        st[j, :len(p)] = np.asarray(p, np.int32).reshape(len(p), d)
    rec[f"c{i}_states"] = st


def main():
    t0 = time.time()
    sys.setrecursionlimit(100000)
    ref = load_reference()
    search = _load("hironaka.util.search", "hironaka/util/search.py")
    rec, names = {}, []

    def add(name, rows, host_name, max_size, n0=1, curr=0):
        new = run(ref, search.search_tree, host_name, rows, max_size, n0, curr)
        record(rec, len(names), rows, host_name, max_size, n0, curr, new)
        names.append(name)
        return new

    new = add("literal_100", LITERAL, "zeillinger", 100)
    rec["lit_str"] = np.asarray([str(c[2]) for c in new])
    add("literal_full", LITERAL, "zeillinger", None)
    add("root6_full", ROOT_6, "zeillinger", None)
    add("literal_100_s0_5_curr_3", LITERAL, "zeillinger", 100, n0=5, curr=3)
    rng = np.random.default_rng(20261016)
    skipped = 0
    for host_name in HOSTS:
        for d in (2, 3, 4, 5):
            got = 0
            while got < 2:
                rows = rng.integers(0, 8, (int(rng.integers(2, 7)), d)).tolist()
                try:
                    full = run(ref, search.search_tree, host_name, rows, NODE_CAP)
                except Exception:  # noqa: BLE001 -- the reference's own failures: a zero row, |U| < 2
                    skipped += 1
                    continue
                if len(full) > NODE_CAP:  # truncated: too large for the fixture
                    skipped += 1
                    continue
                for ms in SIZES:
                    add(f"{host_name}_d{d}_{got}_{'full' if ms is None else ms}", rows, host_name, ms)
                got += 1
        print(f"{host_name}: {len(names)} cases, {skipped} roots skipped ({time.time() - t0:.1f} s)")
    rec["cases"] = np.asarray(names)
    np.savez_compressed(os.path.join(OUT, "search_tree.npz"), **rec)
    n = sum(len(rec[f"c{i}_ident"]) for i in range(len(names)))
    print(f"wrote search_tree.npz: {len(names)} cases, {n} nodes in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
