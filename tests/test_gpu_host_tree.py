"""hk_tree_expand / ops.tree_expand and hironaka_amd.host_tree on the GPU, bit for bit against tests/host_tree_rules.py
(the plain recursion that test_host_tree_rules.py pins to the reference's recorded trees): single levels at every
shape class, capacity and layouts, whole trees under callable hosts, the reference's own trees, and the reference-named
search_tree_fix_host.  All values are small integers, exact in float32."""
import functools
import os

import numpy as np
import pytest
import torch

import host_tree_rules as H
import layout_cases as LC
import search_rules as R
from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import host_tree, ops, players
from hironaka_amd.host import AllCoordHost
from hironaka_amd.util import search as US
from oracle import np_oracle as NO

pytestmark = pytest.mark.gpu

BIG = 1364  # the largest max_points at dim 6 whose parent and child fit 64 KiB in float32 (681 in float64)
SHAPES = ((2, 2), (5, 4), (20, 3), (19, 7), ("big", 6))
SENTINEL = 777.0


def _m(m, dtype):
    return (BIG if dtype == torch.float32 else 681) if m == "big" else m


def _per_block(m, d, dtype):
    es = 4 if dtype == torch.float32 else 8
    return min(64, 65536 // (((2 * m * d + 2 * d) | 1) * es))


@functools.lru_cache(maxsize=None)
def _level(m, d, n, sem, reposition, per_block):
    """(states [n, m, d] float64, classes [n], the expected children in slot order as (parent, axis, state))"""
    rng = np.random.default_rng(m * 100 + d * 10 + n)
    ncls = 2 ** d - d - 1
    st = rng.integers(0, 7, (n, m, d)).astype(np.float64)
    st[rng.random((n, m)) < 0.35] = -1.0  # holes between live rows
    st[1::7, 1:] = -1.0  # parents that are already done (one point, or none)
    cls = ((np.arange(n) + 1) % (ncls + 1) - 1).astype(np.int32)  # every class id of the dimension, and -1
    for edge in range(per_block, n, per_block) if per_block > 1 else ():  # zero-child parents at the block edges
        cls[edge - 1] = cls[edge] = -1
    if m > 64:  # the restatement costs m^2 * d per child (0.2 s): at the largest shape one parent in 64 is expanded
        cls[np.arange(n) % 64 != 0] = -1
    want = [(i, a, new) for i in range(n) for a, new in H.expand(st[i], int(cls[i]), sem, reposition)]
    return st, cls, want


def _check_level(res, want, m, d, dtype, sem, upto=None):
    k = len(want) if upto is None else upto
    np_dt = np.float32 if dtype == torch.float32 else np.float64
    width = int(np.prod(res.children.shape[1:]))  # m*d, or m*d + d for records (k may be 0)
    got = res.children[:k].cpu().numpy().reshape(k, width)[:, :m * d].reshape(k, m, d)
    assert np.array_equal(got, np.asarray([w[2] for w in want[:k]], np_dt).reshape(k, m, d))
    assert res.child_parent[:k].tolist() == [w[0] for w in want[:k]]
    assert res.child_axis[:k].tolist() == [w[1] for w in want[:k]]
    assert res.child_num_points[:k].tolist() == [H.num_points(w[2]) for w in want[:k]]
    assert res.child_done[:k].tolist() == [H.is_done(w[2], sem, d) for w in want[:k]]


@pytest.mark.parametrize("reposition", (False, True), ids=("plain", "repos"))
@pytest.mark.parametrize("sem", ("jax", "list"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("f32", "f64"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_level_matches_the_recursion(shape, dtype, sem, reposition):
    d = shape[1]
    m = _m(shape[0], dtype)
    per_block = _per_block(m, d, dtype)
    for n in (1, 63, 64, 65, 3 * per_block + 1):
        st, cls, want = _level(m, d, n, sem, reposition, per_block)
        parents = torch.as_tensor(st, dtype=dtype, device="cuda")
        out = torch.full((n * d + 3, m, d), SENTINEL, dtype=dtype, device="cuda")
        res = ops.tree_expand(parents, torch.as_tensor(cls, device="cuda"), spec=(m, d), sem=sem,
                              reposition=reposition, out=out, capacity=n * d)
        assert int(res.total) == len(want) and int(res.status) == 0, n
        _check_level(res, want, m, d, dtype, sem)
        assert bool((out[len(want):] == SENTINEL).all()), n  # slots from total on are untouched


@pytest.mark.parametrize("sem", ("jax", "list"))
def test_capacity_bounds_what_is_written(sem):
    m, d, n, dtype = 20, 3, 65, torch.float32
    st, cls, want = _level(m, d, n, sem, True, 64)
    parents = torch.as_tensor(st, dtype=dtype, device="cuda")
    klass = torch.as_tensor(cls, device="cuda")
    middle = next(k for k in range(5, len(want)) if want[k][0] == want[k - 1][0])  # inside a parent's children
    for capacity in (middle, len(want) - 1, 1):
        out = torch.full((len(want) + 8, m * d + d), SENTINEL, dtype=dtype, device="cuda")
        res = ops.tree_expand(parents, klass, spec=(m, d), sem=sem, out=out, capacity=capacity, zero_tail=True)
        assert int(res.total) == len(want) and int(res.status) == A.HK_TREE_OVERFLOW
        assert res.child_parent.shape[0] == capacity
        _check_level(res, want, m, d, dtype, sem, upto=capacity)
        assert bool((out[:capacity, m * d:] == 0).all())
        assert bool((out[capacity:] == SENTINEL).all())  # the guard behind the capacity
    out = torch.full((len(want), m * d + d), SENTINEL, dtype=dtype, device="cuda")
    assert int(ops.tree_expand(parents, klass, spec=(m, d), sem=sem, out=out, zero_tail=True).status) == 0


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("f32", "f64"))
def test_layouts(dtype):
    m, d, n = 5, 4, 65
    st, cls, want = _level(m, d, n, "jax", True, 64)
    klass = torch.as_tensor(cls, device="cuda")
    k = len(want)
    np_dt = np.float32 if dtype == torch.float32 else np.float64
    rec = torch.as_tensor(LC.records(st.astype(np_dt), np.full((n, d), 9.0)), device="cuda")  # records with a tail
    wide = torch.full((n, 2 * (m * d + d) + 3), 5.0, dtype=dtype, device="cuda")
    wide[:, 3:3 + m * d] = rec[:, :m * d]
    views = {"records": rec, "flat": rec[:, :m * d].contiguous(), "points": rec[:, :m * d].reshape(n, m, d),
             "strided": wide[:, 3:3 + m * d + d], "offset": wide[:, 3:3 + m * d],
             "transposed": rec[:, :m * d].reshape(n, m, d).transpose(1, 2).contiguous().transpose(1, 2)}
    for name, view in views.items():
        if name in ("strided", "offset"):
            assert view.data_ptr() != wide.data_ptr() and not view.is_contiguous()
        res = ops.tree_expand(view, klass, spec=(m, d))
        assert int(res.total) == k and tuple(res.children.shape) == (n * d, m, d), name
        _check_level(res, want, m, d, dtype, "jax")
    # the tail: written only with zero_tail; children as strided records
    for zero_tail in (False, True):
        buf = torch.full((k + 2, m * d + d + 5), SENTINEL, dtype=dtype, device="cuda")
        out = buf[:, 2:2 + m * d + d]
        res = ops.tree_expand(rec, klass, spec=(m, d), out=out, zero_tail=zero_tail)
        assert res.children is out and int(res.status) == 0
        _check_level(res, want, m, d, dtype, "jax")
        assert bool((out[:k, m * d:] == (0.0 if zero_tail else SENTINEL)).all())
        assert bool((buf[:, :2] == SENTINEL).all() and (buf[:, 2 + m * d + d:] == SENTINEL).all())
        assert bool((buf[k:] == SENTINEL).all())
    with pytest.raises(ValueError):
        ops.tree_expand(rec, klass, spec=(m, d), out=buf[:, 2:2 + m * d], zero_tail=True)
    with pytest.raises(ValueError):
        ops.tree_expand(rec, klass[:-1], spec=(m, d))


# ---- whole trees -------------------------------------------------------------------------------------------------

def _roots(m, d, b, seed):
    rng = np.random.default_rng(seed)
    st = rng.integers(0, 6, (b, m, d)).astype(np.float32)
    st[rng.random((b, m)) < 0.3] = -1.0
    st[0, 1:] = -1.0  # a one-point root
    st[0, 0] = 2.0
    st[1] = -1.0  # an ended root
    return st


def _table_np(state):
    d = state.shape[1]
    return int(np.clip(state, 0, None).sum()) % (2 ** d - d) - 1


def _table_torch(points, key=None, **kwargs):
    d = points.shape[-1]
    return (points.clamp(min=0).sum((1, 2)).long() % (2 ** d - d) - 1).to(torch.int32)


def _compare_trees(res, roots, host_np, sem, reposition, max_depth, replay=False):
    start = 0
    counts = res.count.tolist()
    cols = [c.cpu().numpy() for c in (res.parent, res.axis, res.depth, res.num_points, res.done, res.host_class,
                                      res.states, res.root)]
    assert sum(counts) == len(cols[0])
    for b, root in enumerate(roots):
        sl = slice(start, start + counts[b])
        if replay:  # the host's draws, in the order the recursion asks for them
            asked = iter([int(c) for c, dn, dep in zip(cols[5][sl], cols[4][sl], cols[2][sl])
                          if not dn and dep <= max_depth])
            t = H.tree(root, lambda s: next(asked), sem, reposition, max_depth)
        else:
            t = H.tree(root, host_np, sem, reposition, max_depth)
        assert counts[b] == len(t.parent), b
        for got, want in zip(cols[:6], (t.parent, t.axis, t.depth, t.num_points, t.done, t.host_class)):
            assert got[sl].tolist() == list(want), b
        assert np.array_equal(cols[6][sl], np.asarray(t.states, np.float32)), b
        assert (cols[7][sl] == b).all()
        start += counts[b]


@pytest.mark.parametrize("max_depth", (0, 1, 3))
@pytest.mark.parametrize("host_input", ("obs", "points"))
def test_whole_trees_match_the_recursion(host_input, max_depth):
    m, d, b = 6, 3, 9
    roots = _roots(m, d, b, 11)
    dev = torch.as_tensor(roots, device="cuda")
    ncls = 2 ** d - d - 1
    hosts = {"zeillinger": (players.zeillinger_fn, lambda s: int(NO.zeillinger_class(s[None])[0])),
             "all_coord": (players.all_coord_host_fn, lambda s: ncls - 1),
             "table": (_table_torch, _table_np),
             "random": (players.random_host_fn, None)}
    for name, (fn, fn_np) in hosts.items():
        if host_input == "obs":
            call = players.get_host_with_flattened_obs((m, d), fn, truncate_input=True)
            given = torch.cat([dev.reshape(b, -1), torch.zeros(b, d, device="cuda")], 1)
        else:
            call, given = fn, dev
        for sem, reposition in (("jax", True), ("list", False)):
            res = host_tree.search_trees_fix_host(given, (m, d), call, key=5, max_depth=max_depth, sem=sem,
                                                  reposition=reposition, host_input=host_input)
            _compare_trees(res, roots, fn_np, sem, reposition, max_depth, replay=fn_np is None)
            cut = [bool(((res.root == r) & ~res.done & (res.depth == max_depth + 1)).any()) for r in range(b)]
            assert res.status.tolist() == [host_tree.DEPTH_LIMIT if c else 0 for c in cut], name
    # max_nodes too small: the status names the limit and nothing beyond the bound is made
    full = host_tree.search_trees_fix_host(dev, (m, d), players.all_coord_host_fn, max_depth=max_depth,
                                           host_input="points")
    small = host_tree.search_trees_fix_host(dev, (m, d), players.all_coord_host_fn, max_depth=max_depth,
                                            host_input="points", max_nodes=b + 4)
    assert int(full.count.sum()) > b + 4 and int(small.count.sum()) == b + 4
    assert bool((small.status & host_tree.NODE_LIMIT).any()) and not bool((full.status & host_tree.NODE_LIMIT).any())


def test_reference_trees_on_the_gpu():
    """list semantics without reposition under the ascending-list hosts, passed through ops.host_select: the
    reference's recorded search_tree cases, and util.search_trees under AllCoordHost"""
    g = np.load(os.path.join(GOLDEN, "search_tree.npz"))
    seen = 0
    for i, name in enumerate(g["cases"]):
        max_size, n0, curr = (int(v) for v in g[f"c{i}_meta"])
        host = str(g[f"c{i}_host"])
        if max_size >= 0 or host not in ("all_coord", "weak_spivakovsky", "weak_spivakovsky_min_hitting"):
            continue
        root = np.asarray(g[f"c{i}_root"], np.float32)
        m, d = root.shape
        dev = torch.as_tensor(root[None], device="cuda")
        res = host_tree.search_trees_fix_host(dev, (m, d), lambda pts, key=None: ops.host_select(pts, host),
                                              sem="list", reposition=False, host_input="points")
        assert res.status.tolist() == [0], name
        parent = res.parent.tolist()
        ident = [curr] + [n0 + j - 1 for j in range(1, len(parent))]
        assert ident[1:] == g[f"c{i}_ident"].tolist(), name
        assert [ident[p] for p in parent[1:]] == g[f"c{i}_parent"].tolist(), name
        states = res.states.cpu().numpy()
        for j, st in enumerate(g[f"c{i}_states"]):
            assert R.rows_of(R.live(states[j + 1])) == [r for r in np.asarray(st).tolist() if r[0] >= 0], (name, j)
        if host == "all_coord":
            ref = US.search_trees(dev, AllCoordHost(), max_nodes=len(parent) + 1)
            k = int(ref.count[0])
            assert k == len(parent) and int(ref.status[0]) == 0
            for mine, theirs in ((res.parent, ref.parent), (res.axis, ref.axis), (res.depth, ref.depth),
                                 (res.num_points, ref.num_points)):
                assert torch.equal(mine, theirs[0, :k]), name
            assert torch.equal(res.states[1:], ref.states[0, 1:k]), name  # (a root is kept as given)
        seen += 1
    assert seen >= 3


@pytest.mark.parametrize("depth", (0, 2))
def test_search_tree_fix_host_builds_the_reference_recursion(depth):
    m, d = 6, 3
    root = _roots(m, d, 4, 3)[3]
    data = torch.cat([torch.as_tensor(root).reshape(1, -1), torch.zeros(1, d)], 1).cuda()
    host = players.get_host_with_flattened_obs((m, d), players.zeillinger_fn, truncate_input=True)
    node = host_tree.TreeNode(data=data)
    got = host_tree.search_tree_fix_host(node, (m, d), host, depth, 7, scale_observation=True, max_depth=4)
    assert got is node
    t = H.tree(root, lambda s: int(NO.zeillinger_class(s[None])[0]), "jax", True, max_depth=4, depth=depth)
    assert len(t.parent) > 1 and max(t.depth) <= 5 - depth
    made = [node]

    def walk(n):
        for c in n.children:
            assert c.parent is n
            made.append(c)
            walk(c)

    walk(node)
    assert len(made) == len(t.parent)
    for j in range(1, len(made)):
        assert made[j].parent is made[t.parent[j]] and made[j].action_from_parent == t.axis[j]
        assert tuple(made[j].data.shape) == (1, (m + 1) * d) and made[j].children is not None
        want = np.concatenate([np.asarray(t.states[j], np.float32).reshape(-1), np.zeros(d, np.float32)])
        assert np.array_equal(made[j].data.cpu().numpy()[0], want), j
    assert "--" in node.to_dot(label_fn=lambda n: host_tree.default_label_fn(n, (m, d)))
