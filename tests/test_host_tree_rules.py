"""CPU-side checks of hk_tree_expand / hironaka_amd.host_tree: tests/host_tree_rules.py, the plain recursion the GPU
tests compare the kernel and the level loop with, pinned to the reference's recorded trees (search_tree.npz); the C
boundary; and TreeNode's DOT text."""
import ctypes
import os
import re

import numpy as np
import pytest

import abi_cases
import host_tree_rules as H
import search_rules as R
from conftest import GOLDEN
from hironaka_amd import _abi as A
from hironaka_amd import _lib
from oracle import np_oracle as NO

ASCENDING_HOSTS = ("all_coord", "weak_spivakovsky", "weak_spivakovsky_min_hitting")


def test_recursion_reproduces_the_reference_trees():
    """list semantics without reposition under the ascending-list hosts is the reference's search_tree: ident, parent
    and states of every full-tree case of those hosts, in the reference's creation order"""
    g = np.load(os.path.join(GOLDEN, "search_tree.npz"))
    seen = {h: 0 for h in ASCENDING_HOSTS}
    for i, name in enumerate(g["cases"]):
        max_size, n0, curr = (int(v) for v in g[f"c{i}_meta"])
        host = str(g[f"c{i}_host"])
        if max_size >= 0 or host not in ASCENDING_HOSTS:
            continue
        t = H.tree(g[f"c{i}_root"], H.list_host(host), sem="list", reposition=False)
        calls = R.created(t, n0, curr)
        assert [c[0] for c in calls] == g[f"c{i}_ident"].tolist(), name
        assert [c[1] for c in calls] == g[f"c{i}_parent"].tolist(), name
        want = g[f"c{i}_states"]
        assert len(want) == len(t.parent) - 1, name
        for j, st in enumerate(want):
            assert R.rows_of(R.live(t.states[j + 1])) == [r for r in np.asarray(st).tolist() if r[0] >= 0], (name, j)
        seen[host] += 1
    assert all(seen.values()), seen


def test_jax_expansion_is_the_oracle_step_per_axis():
    rng = np.random.default_rng(5)
    m, d = 6, 4
    table = NO.decode_table(d)
    for trial in range(20):
        state = rng.integers(0, 7, (m, d)).astype(np.float32)
        state[rng.random(m) < 0.3] = -1.0
        cls = int(rng.integers(0, len(table)))
        for reposition in (False, True):
            got = H.expand(state, cls, "jax", reposition)
            axes = [k for k in range(d) if table[cls][k]]
            assert [a for a, _ in got] == axes
            for a, new in got:
                want = NO.step(state[None], table[cls][None].astype(np.float32), np.asarray([a]), sem="jax",
                               do_reposition=reposition)[0]
                assert np.array_equal(new, want), (trial, a)
    assert H.expand(state, -1, "jax", True) == [] and H.expand(state, len(table), "jax", True) == []


def test_leaves_sit_one_level_below_max_depth():
    """search.py:90 tests depth > max_depth at the node: the nodes AT max_depth are still expanded"""
    root = np.array([[4, 0, 1], [0, 5, 2], [1, 1, 6], [3, 3, 0]], np.float32)
    # the all-coordinates class of dimension 3; with reposition that game need not end, so every tree here is capped
    full = H.tree(root, lambda s: 3, max_depth=3)
    assert max(full.depth) == 4
    for cap in (0, 1, 2):
        t = H.tree(root, lambda s: 3, max_depth=cap)
        assert max(t.depth) == cap + 1
        assert len(t.parent) == sum(dep <= cap + 1 for dep in full.depth)
        assert all(c == -1 for c, dep in zip(t.host_class, t.depth) if dep == cap + 1)
        assert all(c == 3 for c, dep, dn in zip(t.host_class, t.depth, t.done) if dep <= cap and not dn)
    # `depth` offsets the test
    t = H.tree(root, lambda s: 3, max_depth=3, depth=2)
    assert max(t.depth) == 2 and len(t.parent) == sum(dep <= 2 for dep in full.depth)
    assert len(H.tree(root, lambda s: 3, max_depth=1, depth=2).parent) == 1


def test_symbol_constants_and_descriptor_are_bound(tmp_path):
    handle = ctypes.CDLL(_lib.build())
    assert hasattr(handle, "hk_tree_expand") and set(A.TREE_PROTOTYPES) == {"hk_tree_expand"}
    assert _lib.lib().hk_tree_expand.argtypes == A.TREE_PROTOTYPES["hk_tree_expand"][1]
    text = abi_cases.header("hironaka_hip_tree.h")
    assert re.search(r"^int hk_tree_expand\(const hk_tree_expand_desc\* desc, void\* stream\);", text, flags=re.M)
    assert '#include "hironaka_hip_tree.h"' in abi_cases.header()
    found = re.findall(r"#define\s+(HK_TREE_\w+)\s+\(?(-?\d+)u?\)?\s", text)
    assert len(found) == 3
    for name, value in found:
        assert getattr(A, name) == int(value), name
    assert A.HK_ABI_VERSION == 6 and _lib.lib().hk_abi_version() == 6
    abi_cases.assert_layouts_match_c({"hk_tree_expand_desc": A.hk_tree_expand_desc}, tmp_path)


def _desc(buf, out, ints, **kw):
    q = A.hk_tree_expand_desc()
    q.parents_in, q.children_out = ctypes.addressof(buf), ctypes.addressof(out)
    q.class_id = q.child_offset = q.child_parent = q.child_axis = q.child_num_points = ctypes.addressof(ints)
    q.child_done = q.status = ctypes.addressof(ints)
    q.n_parents, q.capacity, q.max_points, q.dim, q.dtype, q.sem = 4, 8, 5, 3, A.HK_F32, A.HK_SEM_JAX
    q.in_stride, q.out_stride = 15, 18
    q.flags = A.HK_TREE_REPOSITION | A.HK_TREE_ZERO_TAIL
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def test_argument_validation_without_gpu():
    """every refusal is decided on the host, before any launch"""
    L = _lib.lib()
    buf, out, ints = (ctypes.c_double * 512)(), (ctypes.c_double * 512)(), (ctypes.c_int64 * 64)()
    call = lambda **kw: L.hk_tree_expand(ctypes.byref(_desc(buf, out, ints, **kw)), None)  # noqa: E731
    assert L.hk_tree_expand(None, None) == A.HK_ERR_NULL
    assert call(n_parents=0) == A.HK_OK  # nothing to do
    assert call(n_parents=0, parents_in=None, class_id=None) == A.HK_OK
    # the largest max_points whose parent and child fit 64 KiB: (2*m*d + 2*d) | 1 elements
    assert call(n_parents=0, dim=6, max_points=1364) == A.HK_OK
    assert call(n_parents=0, dim=6, max_points=681, dtype=A.HK_F64) == A.HK_OK
    for bad in (dict(dtype=A.HK_I32), dict(dim=8), dict(sem=A.HK_SEM_TORCH), dict(flags=4),
                dict(dim=6, max_points=1365), dict(dim=6, max_points=682, dtype=A.HK_F64)):
        assert call(**bad) == A.HK_ERR_UNSUPPORTED, bad
    for bad in (dict(n_parents=-1), dict(capacity=-1), dict(max_points=0), dict(dim=1), dict(in_stride=14),
                dict(out_stride=17), dict(out_stride=14, flags=0)):
        assert call(**bad) == A.HK_ERR_SHAPE, bad
    for bad in (dict(parents_in=None), dict(children_out=None), dict(class_id=None), dict(child_offset=None),
                dict(child_parent=None), dict(child_axis=None), dict(child_num_points=None), dict(child_done=None),
                dict(status=None)):
        assert call(**bad) == A.HK_ERR_NULL, bad
    base = ctypes.addressof(buf)
    assert call(children_out=base) == A.HK_ERR_SHAPE  # children over the parents
    assert call(children_out=base + 4 * 20) == A.HK_ERR_SHAPE  # the children start inside the parents' span
    assert call(parents_in=ctypes.addressof(out) + 4 * 20) == A.HK_ERR_SHAPE  # the parents inside the children's span
    assert call(children_out=base + 4 * 20, in_stride=40, out_stride=40) == A.HK_ERR_SHAPE  # interleaved records
    assert call(children_out=base, out_stride=20) == A.HK_ERR_SHAPE  # the same pointer, different strides
    assert call(in_stride=14, flags=0, out_stride=15) == A.HK_ERR_SHAPE
    assert call(out_stride=17, children_out=base + 4 * 2048) == A.HK_ERR_SHAPE  # a stride below m*d + d with the zero tail
    # records that span more than 2^63 bytes (the byte count would wrap): refused, behind the null checks
    for bad in (dict(in_stride=1 << 62), dict(out_stride=1 << 62), dict(in_stride=1 << 62, out_stride=1 << 62),
                dict(n_parents=5, in_stride=1 << 60),  # 4 rows x 2^60 elements x 4 bytes: exactly 2^64
                dict(in_stride=1 << 62, capacity=0),  # the parents' span counts where no child is written
                dict(children_out=base, in_stride=1 << 62, out_stride=1 << 62)):  # children over the parents
        assert call(**bad) == A.HK_ERR_SHAPE, bad
    for name in ("parents_in", "children_out", "status"):
        assert call(in_stride=1 << 62, out_stride=1 << 62, **{name: None}) == A.HK_ERR_NULL, name
    iaddr = ctypes.addressof(ints)
    for bad in (dict(parents_in=base + 2), dict(children_out=ctypes.addressof(out) + 2), dict(class_id=iaddr + 2),
                dict(child_offset=iaddr + 4), dict(child_axis=iaddr + 1), dict(status=iaddr + 3),
                dict(dtype=A.HK_F64, parents_in=base + 4), dict(dtype=A.HK_F64, children_out=ctypes.addressof(out) + 4)):
        assert call(**bad) == A.HK_ERR_ALIGN, bad


def test_wrappers_refuse_what_cannot_run():
    import torch
    from hironaka_amd import host_tree, ops
    with pytest.raises(TypeError):
        ops.tree_expand(torch.zeros(2, 4, 3), torch.zeros(2, dtype=torch.int32), spec=(4, 3))  # CPU tensors
    with pytest.raises(ValueError):
        ops.tree_expand(torch.zeros(2, 4, 3), torch.zeros(2, dtype=torch.int32), spec=(4, 3), sem="torch")
    with pytest.raises(ValueError):
        host_tree.search_trees_fix_host(torch.zeros(2, 4, 3), (4, 3), None, host_input="features")
    assert host_tree.level_key(7, 3) == 10 and host_tree.level_key(None, 3) is None
    gen = torch.Generator()
    assert host_tree.level_key(gen, 3) is gen
    one_hot = torch.tensor([[0., 1., 1., 0.], [0., 0., 0., 0.]])
    assert host_tree.host_classes(one_hot, 2, 3, "cpu").tolist() == [1, 0]  # the first maximum
    assert host_tree.host_classes(torch.tensor([3, -1]), 2, 3, "cpu").tolist() == [3, -1]
    with pytest.raises(ValueError):
        host_tree.host_classes(torch.zeros(2, 5), 2, 3, "cpu")


def test_tree_nodes_to_dot():
    from hironaka_amd.host_tree import TreeNode, default_label_fn
    root = TreeNode(children=[], data=np.array([[2, 0, 0, 3, -1, -1, 0, 0]]))
    kids = [TreeNode(children=[], parent=root, action_from_parent=a, data=np.array([[a, 1, -1, -1, -1, -1, 0, 0]]))
            for a in (0, 1)]
    root.children.extend(kids)
    deep = TreeNode(children=None, parent=kids[0], action_from_parent=1, data=np.array([[5, 5, -1, -1, -1, -1, 0, 0]]))
    kids[0].children.append(deep)
    assert root.to_dot() == ('strict graph {\n  0 [label="0"];\n  1 [label="1"];\n  0 -- 1 [label="0"];\n'
                             '  2 [label="2"];\n  0 -- 2 [label="1"];\n  3 [label="3"];\n  1 -- 3 [label="1"];\n}\n')
    assert root.to_dot(max_depth=1) == ('strict graph {\n  0 [label="0"];\n  1 [label="1"];\n  0 -- 1 [label="0"];\n'
                                        '  2 [label="2"];\n  0 -- 2 [label="1"];\n}\n')
    assert root.to_dot(max_depth=0) == 'strict graph {\n  0 [label="0"];\n}\n'
    label = lambda node: default_label_fn(node, (3, 2))  # noqa: E731
    assert default_label_fn(root, (3, 2)) == "[[2 0]\n [0 3]]"
    assert root.to_dot(0, label) == 'strict graph {\n  0 [label="[[2 0]\\n [0 3]]"];\n}\n'
    assert kids[1].to_dot(label_fn=lambda node: 'a"b\\') == 'strict graph {\n  0 [label="a\\"b\\\\"];\n}\n'
    try:
        import pygraphviz  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="pygraphviz"):
            root.to_graphviz()
