"""
Generate tests/golden/search_morin.npz by RUNNING the reference's own `search_tree_morin`
(hironaka/util/search.py:53-93) with its own ListPoints and hosts, into a stub tree that records every `create_node`
call.  Runs only where the reference checkout exists; the resulting .npz is what travels, and it holds data only.

The files are loaded one by one as make_golden.py does (the package __init__ files import jax).

Cases (index i; `cases` lists the names):
    c{i}_root     [m, d] int64         the root, the reference's row order kept (no padding)
    c{i}_weights  [d] int64            the weights at the call
    c{i}_meta     [4] int64            max_size (-1: the whole tree, run with a max_size above any tree here), the
                                       tree size s0 before the call, curr_node, the distinguished row
    c{i}_host     str                  a key of hironaka_amd.ops.SEARCH_HOSTS
    c{i}_ident    [n] int64            identifiers of the created nodes in creation order
    c{i}_parent   [n] int64            their parents' identifiers
    c{i}_data     [n] str              their data strings (Node.points)
    stats         [4] int64            over all cases: nodes lost to an identical row, nodes lost to a strictly smaller
                                       row, pruned actions, "...more..." nodes below an ended node
    thom4_hosts / thom4_ref_seconds    the reference's CPU seconds for the whole Thom N = 4 tree per finite host

Cases: the thom_points_homogeneous(3) and (4) roots (weights all 1, distinguished = the last row) under all five hosts
at max_size in {0, 1, 7, 100, full}; test/testThom.py:94-114's root with weights [1, 1, 2, 3, 2, 3, 3] under
WeakSpivakovsky; seeded roots of dim 2..7 with 2..8 points, weights in 1..3 and a random distinguished row under every
host at the same sizes; hand-made roots with a duplicate of the distinguished row; one call below a non-zero
curr_node of a tree that already holds several nodes.  A root whose full tree exceeds NODE_CAP nodes is run at the
finite sizes only under AllCoordHost (whose Thom trees do not end) and skipped under the other hosts; roots where the
reference raises are skipped.

The plain restatement of the rules (morin_tree of tests/search_rules.py, here with the reference's own hosts) follows
every reference run node for node; it is what counts the events of `stats`, and the coverage assertions at the end
keep a weak fixture from being written.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_search_morin_golden.py
"""
import os
import sys
import time

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from make_golden import OUT, _load, load_reference  # noqa: E402
from search_rules import created, morin_data, morin_tree, rows_of  # noqa: E402

HOSTS = {"zeillinger": "Zeillinger", "all_coord": "AllCoordHost", "zeillinger_lex": "ZeillingerLex",
         "weak_spivakovsky": "WeakSpivakovsky", "weak_spivakovsky_min_hitting": "WeakSpivakovskyMinHitting"}
SIZES = (0, 1, 7, 100, None)
NODE_CAP = 3000
FULL = 10 ** 9  # max_size of a "full" run
THOM_ORIGINAL_WEIGHTS = [1, 1, 2, 3, 2, 3, 3]
DUPLICATES = ([[1, 2], [1, 2], [3, 0]], [[2, 1, 0], [0, 0, 3], [2, 1, 0]])  # the distinguished row 0 has a twin


class StubTree:
    """size() and create_node(tag, identifier, parent=, data=), as treelib's Tree; records the calls"""

    def __init__(self, n0=1):
        self.calls = [(i, i - 1 if i else None, None) for i in range(n0)]

    def size(self):
        return len(self.calls)

    def create_node(self, tag, identifier, parent=None, data=None):
        assert tag == identifier == len(self.calls)
        self.calls.append((identifier, parent, data))


def run(ref, morin, host_name, rows, weights, dist, max_size, n0=1, curr=0, stats=None):
    """the reference's run; with `stats`, the restatement must follow it node for node"""
    ms = FULL if max_size is None else max_size
    tree = StubTree(n0)
    host = getattr(ref.host, HOSTS[host_name])()
    pts = ref.ListPoints([[list(r) for r in rows]], distinguished_points=[dist])
    out = morin(pts, tree, curr, list(weights), host, max_size=ms)
    assert out is tree
    new = [(c[0], c[1], c[2].points) for c in tree.calls[n0:]]
    if stats is not None:
        local = [0, 0, 0, 0]
        mine = morin_tree(rows, weights, dist, lambda st: host.select_coord(ref.ListPoints([rows_of(st)]))[0], ms, s0=n0,
                          stats=local)
        calls = [c + (morin_data(mine, j + 1),) for j, c in enumerate(created(mine, n0, curr))]
        assert calls == new, (host_name, rows, weights, dist, max_size)
        for i in range(4):
            stats[i] += local[i]
    return new


def depth_of(new, curr):
    dep = {curr: 0}
    for ident, parent, _ in new:
        dep[ident] = dep[parent] + 1
    return max(dep.values())


def main():
    t0 = time.time()
    sys.setrecursionlimit(100000)
    ref = load_reference()
    morin = _load("hironaka.util.search", "hironaka/util/search.py").search_tree_morin
    thom = _load("hironaka.src._thom_fn", "hironaka/src/_thom_fn.py")
    rec, names, stats = {}, [], [0, 0, 0, 0]
    dim7_depth = {h: 0 for h in HOSTS}

    def add(name, rows, host_name, weights, dist, max_size, n0=1, curr=0):
        new = run(ref, morin, host_name, rows, weights, dist, max_size, n0, curr, stats)
        i = len(names)
        rec[f"c{i}_root"] = np.asarray(rows, np.int64)
        rec[f"c{i}_weights"] = np.asarray(weights, np.int64)
        rec[f"c{i}_meta"] = np.asarray([-1 if max_size is None else max_size, n0, curr, dist], np.int64)
        rec[f"c{i}_host"] = np.asarray(host_name)
        rec[f"c{i}_ident"] = np.asarray([c[0] for c in new], np.int64)
        rec[f"c{i}_parent"] = np.asarray([c[1] for c in new], np.int64)
        rec[f"c{i}_data"] = np.asarray([c[2] for c in new], dtype=str)
        names.append(name)
        if len(rows[0]) == 7 and new:
            dim7_depth[host_name] = max(dim7_depth[host_name], depth_of(new, curr))
        return new

    def add_sizes(name, rows, host_name, weights, dist):
        """every size of SIZES; False when the root is skipped"""
        try:
            full = run(ref, morin, host_name, rows, weights, dist, NODE_CAP)
        except Exception:  # noqa: BLE001 -- the reference's own failures: a zero row, |U| < 2
            return False
        ends = len(full) <= NODE_CAP
        if not ends and host_name != "all_coord":
            return False
        for ms in SIZES:
            if ms is not None or ends:
                add(f"{name}_{'full' if ms is None else ms}", rows, host_name, weights, dist, ms)
        return True

    thom_rows = {}
    for order in (3, 4):
        rows = [[int(v) for v in r] for r in thom.thom_points_homogeneous(order)]
        thom_rows[order] = rows
        for host_name in HOSTS:
            assert add_sizes(f"thom{order}_{host_name}", rows, host_name, [1] * len(rows[0]), len(rows) - 1)
    finite = [h for h in HOSTS if h != "all_coord"]
    seconds = []
    for host_name in finite:
        t1 = time.perf_counter()
        run(ref, morin, host_name, thom_rows[4], [1] * 7, len(thom_rows[4]) - 1, None)
        seconds.append(time.perf_counter() - t1)
    rec["thom4_hosts"] = np.asarray(finite)
    rec["thom4_ref_seconds"] = np.asarray(seconds, np.float64)

    tp = [[int(v) for v in r] for r in thom.thom_points(4)]
    original = [[r[0] + sum(r[1:]) - 4] + r[1:] for r in tp]  # test/testThom.py:95-101
    new = add("thom_original", original, "weak_spivakovsky", THOM_ORIGINAL_WEIGHTS, len(original) - 1, 10000)
    assert len(new) + 1 == 37, len(new)
    add("thom4_weak_spivakovsky_100_s0_6_curr_4", thom_rows[4], "weak_spivakovsky", [1] * 7, len(thom_rows[4]) - 1, 100,
        n0=6, curr=4)
    for j, rows in enumerate(DUPLICATES):
        for host_name in HOSTS:
            add_sizes(f"duplicate{j}_{host_name}", rows, host_name, [1, 2, 1][:len(rows[0])], 0)

    rng = np.random.default_rng(20261017)
    skipped = 0
    for host_name in HOSTS:
        for d in (2, 3, 4, 5, 6, 7):
            got = 0
            while got < 2:
                rows = rng.integers(0, 8, (int(rng.integers(2, 9)), d)).tolist()
                weights = rng.integers(1, 4, d).tolist()
                dist = int(rng.integers(0, len(rows)))
                if add_sizes(f"{host_name}_d{d}_{got}", rows, host_name, weights, dist):
                    got += 1
                else:
                    skipped += 1
        print(f"{host_name}: {len(names)} cases, {skipped} roots skipped ({time.time() - t0:.1f} s)")

    n = sum(len(rec[f"c{i}_ident"]) for i in range(len(names)))
    assert all(v >= 3 for v in dim7_depth.values()), dim7_depth
    assert stats[0] >= 1 and stats[1] >= 1 and stats[2] >= 1 and stats[3] >= 1, stats
    assert n <= 40000, n
    rec["stats"] = np.asarray(stats, np.int64)
    rec["cases"] = np.asarray(names)
    path = os.path.join(OUT, "search_morin.npz")
    np.savez_compressed(path, **rec)
    assert os.path.getsize(path) < 1000000
    print(f"wrote search_morin.npz: {len(names)} cases, {n} nodes, stats {stats}, {os.path.getsize(path)} bytes in "
          f"{time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
