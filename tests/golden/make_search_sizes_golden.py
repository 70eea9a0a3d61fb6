"""
Generate tests/golden/search_sizes.npz by RUNNING the reference's own `search_tree` and `search_tree_morin`
(hironaka/util/search.py:35-93) at the largest roots the fixed-host search operators accept, with its own ListPoints
and hosts, into a stub tree that records every `create_node` call.  Runs only where the reference checkout exists; the
resulting .npz is what travels, and it holds data only.

Roots have every row live and the rows pairwise incomparable, so that neither the reference's Newton step nor a kernel
would change them: for dim >= 3 distinct rows of one coordinate sum, for dim 2 a staircase (x strictly ascending, y
strictly descending, unequal sums; equal-sum roots end after one step there), convex so that its tree is wide.

Per shape (m, d):
    root_{m}x{d}         [m, d] int64   the root of the cases below
    root_{m}x{d}_sparse  [m, d] int64   its first m // 2 rows at the odd rows, padding (-1) between them
    root_{m}x{d}_tail    [m, d] int64   its last 3 rows at the end, padding before them: a short game
    morin_{m}x{d}_weights [d], morin_{m}x{d}_dist   the weights and the distinguished row of the Morin cases (morin_call)
    morin_{m}x{d}_weights_sparse, _dist_sparse, _weights_tail, _dist_tail   the same for the sparse and tail roots
The sparse and tail roots are not run through the reference, which keeps no padding rows.

Cases (index i; `cases` lists the names {op}_{m}x{d}_{host}), one per operator, shape and host:
    c{i}_op        "tree" or "morin"
    c{i}_root      [m, d] int64
    c{i}_host      str                 a key of hironaka_amd.ops.SEARCH_HOSTS
    c{i}_max_size  int64               finite, so that AllCoordHost's endless trees stay bounded
    c{i}_ident     [n] int64           identifiers of the created nodes in creation order (the root is node 0 of a
                                       tree of size 1)
    c{i}_parent    [n] int64           their parents' identifiers
    c{i}_states    [n, m, d] int16     tree: their states (ListPoints.points[0]), padded with -1 rows at the end
    c{i}_weights, c{i}_dist, c{i}_data [n] str    morin: the call's weights and distinguished row, the data strings

search_tree runs at (64,2), (64,3), (33,4), (48,5), (64,6); search_tree_morin at (33,4), (64,6), (24,7), (64,7).  The
reference's search_depth has no cap and cannot run at these shapes.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_search_sizes_golden.py
"""
import os
import sys
import time
from math import gcd

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from make_golden import OUT, _load, load_reference  # noqa: E402
from make_search_tree_golden import HOSTS, StubTree  # noqa: E402
import search_rules as R  # noqa: E402

TREE_SHAPES = ((64, 2), (64, 3), (33, 4), (48, 5), (64, 6))
MORIN_SHAPES = ((33, 4), (64, 6), (24, 7), (64, 7))
TREE_MAX_SIZE = 24
MORIN_MAX_SIZE = 40


def antichain(rng, m, d):
    if d == 2:
        # a convex staircase: the m - 1 steps (a, -b) run through coprime pairs by falling slope b / a.  A move keeps
        # the points on one side of the slope it tests, so both children of a node go on and the tree is wide; under a
        # random staircase one child of every node ends at once.
        steps = sorted({(a, b) for a in range(1, 31) for b in range(1, 31) if gcd(a, b) == 1}, key=lambda v: -v[1] / v[0])
        pick = np.linspace(0, len(steps) - 1, m - 1).round().astype(int)
        assert len(set(pick.tolist())) == m - 1
        x = np.concatenate(([0], np.cumsum([steps[i][0] for i in pick])))
        y = np.concatenate(([0], np.cumsum([steps[i][1] for i in pick])))
        rows = np.stack([x, y[-1] - y], 1)
        assert len(set(rows.sum(1).tolist())) > 1
    else:
        total = int(rng.integers(20, 31))
        seen = set()
        while len(seen) < m:  # a composition of `total` into d parts: cuts of a line of total + d - 1 cells
            cuts = np.sort(rng.choice(total + d - 1, d - 1, replace=False))
            seen.add(tuple(np.diff(np.concatenate(([-1], cuts, [total + d - 1]))) - 1))
        rows = np.asarray(sorted(seen))
        rows = rows[rng.permutation(m)]
        assert (rows.sum(1) == total).all()
    le = (rows[:, None, :] <= rows[None, :, :]).all(2)
    assert le.sum() == m and rows.min() >= 0  # pairwise incomparable
    return rows.astype(np.int64)


def morin_call(root):
    """Weights and a distinguished row under which every host's tree is large.  Most rows are lost within a move or
    two: the restated rules (tests/search_rules.py) try every row, with all weights 1 (as the Thom roots have them)
    and with the last one 2, and the pair with the largest smallest tree over the hosts is taken.  The reference then
    runs that call like any other."""
    d = root.shape[1]
    best = None
    for weights in ([1] * d, [1] * (d - 1) + [2]):
        for dist in np.nonzero(root[:, 0] >= 0)[0].tolist():
            sizes = [len(R.morin_tree(root, weights, dist, h, max_size=MORIN_MAX_SIZE).parent) for h in HOSTS]
            score = (min(sizes), sum(sizes))
            if best is None or score > best[0]:
                best = (score, weights, dist)
    return best[1], best[2]


def main():
    t0 = time.time()
    sys.setrecursionlimit(100000)
    ref = load_reference()
    search = _load("hironaka.util.search", "hironaka/util/search.py")
    rng = np.random.default_rng(20261018)
    rec, names = {}, []
    for m, d in sorted(set(TREE_SHAPES) | set(MORIN_SHAPES)):
        root = antichain(rng, m, d)
        rec[f"root_{m}x{d}"] = root
        sparse = np.full((m, d), -1, np.int64)
        sparse[1::2] = root[:m // 2]
        tail = np.full((m, d), -1, np.int64)
        tail[m - 3:] = root[m - 3:]
        rec[f"root_{m}x{d}_sparse"], rec[f"root_{m}x{d}_tail"] = sparse, tail
        if (m, d) in MORIN_SHAPES:
            for kind, r in (("", root), ("_sparse", sparse), ("_tail", tail)):
                weights, dist = morin_call(r)
                rec[f"morin_{m}x{d}_weights{kind}"] = np.asarray(weights, np.int64)
                rec[f"morin_{m}x{d}_dist{kind}"] = np.asarray(dist, np.int64)

    def add(op, m, d, host_name, new):
        i = len(names)
        rec[f"c{i}_op"] = np.asarray(op)
        rec[f"c{i}_root"] = rec[f"root_{m}x{d}"]
        rec[f"c{i}_host"] = np.asarray(host_name)
        rec[f"c{i}_ident"] = np.asarray([c[0] for c in new], np.int64)
        rec[f"c{i}_parent"] = np.asarray([c[1] for c in new], np.int64)
        names.append(f"{op}_{m}x{d}_{host_name}")
        return i

    for m, d in TREE_SHAPES:
        rows = rec[f"root_{m}x{d}"].tolist()
        for host_name in HOSTS:
            tree = StubTree(1)
            out = search.search_tree(ref.ListPoints([[list(r) for r in rows]]), tree, 0,
                                     getattr(ref.host, HOSTS[host_name])(), max_size=TREE_MAX_SIZE)
            assert out is tree
            new = tree.calls[1:]
            i = add("tree", m, d, host_name, new)
            rec[f"c{i}_max_size"] = np.asarray(TREE_MAX_SIZE, np.int64)
            st = np.full((len(new), m, d), -1, np.int16)
            for j, c in enumerate(new):
                p = np.asarray(c[2].points[0], np.int64).reshape(-1, d)
                assert p.max() < 2 ** 15
                st[j, :len(p)] = p
            rec[f"c{i}_states"] = st
        print(f"tree {m}x{d}: {time.time() - t0:.1f} s")
    for m, d in MORIN_SHAPES:
        rows = rec[f"root_{m}x{d}"].tolist()
        weights, dist = rec[f"morin_{m}x{d}_weights"].tolist(), int(rec[f"morin_{m}x{d}_dist"])
        for host_name in HOSTS:
            tree = StubTree(1)
            pts = ref.ListPoints([[list(r) for r in rows]], distinguished_points=[dist])
            out = search.search_tree_morin(pts, tree, 0, list(weights), getattr(ref.host, HOSTS[host_name])(),
                                           max_size=MORIN_MAX_SIZE)
            assert out is tree
            new = tree.calls[1:]
            i = add("morin", m, d, host_name, new)
            rec[f"c{i}_max_size"] = np.asarray(MORIN_MAX_SIZE, np.int64)
            rec[f"c{i}_weights"] = np.asarray(weights, np.int64)
            rec[f"c{i}_dist"] = np.asarray(dist, np.int64)
            rec[f"c{i}_data"] = np.asarray([c[2].points for c in new], dtype=str)
        print(f"morin {m}x{d}: {time.time() - t0:.1f} s")
    rec["cases"] = np.asarray(names)
    path = os.path.join(OUT, "search_sizes.npz")
    np.savez_compressed(path, **rec)
    n = sum(len(rec[f"c{i}_ident"]) for i in range(len(names)))
    assert os.path.getsize(path) < 1000000
    print(f"wrote search_sizes.npz: {len(names)} cases, {n} nodes, {os.path.getsize(path)} bytes in "
          f"{time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
