"""The search tree kernels one by one against their counterparts in oracle/search_oracle.py: hk_search_select against
SO.simulate, hk_search_backup against SO.expand + SO.backward, hk_search_policy against SO.final_policy.  Trees are
the oracle's own after some simulations of a toy search (test_search.grow_tree), with statistics overwritten game by
game to reach the edges of the decision arithmetic; the structure (parents, children_index, visit counts) is never
touched.  Every action count at both ends of the kernels' buckets (AMAX 4 / 8 / 16 / 32), batch tails of every launch
grid.  Exact: integers equal, floats equal as raw bits (a NaN as a NaN)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from hironaka_amd import _abi as A
from hironaka_amd._lib import check, lib
from hironaka_amd.recurrent_fn import RecurrentFnOutput
from hironaka_amd.search import CapturedSearch, RootFnOutput, gumbel_muzero_policy
from oracle import search_oracle as SO
from test_search import SUM_ORDER_ACTIONS, _toy_recurrent_fn, butterfly_flips, grow_tree, sum_order_roots

pytestmark = pytest.mark.gpu

ACTIONS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 26, 32)
BATCHES = (1, 7, 8, 9, 63, 64, 65, 257)
NUM_SIMULATIONS, GROWN = 16, 11  # trees of 17 nodes, 11 of them expanded: the next free node is 12
STATS = ("node_visits", "raw_values", "node_values", "parents", "action_from_parent", "children_index",
         "children_prior_logits", "children_visits", "children_rewards", "children_discounts", "children_values")
F32_MAX = np.float32(np.finfo(np.float32).max)
# what game g of a case is made of: KINDS[g % len(KINDS)]
KINDS = ("plain", "one_valid", "none_valid", "equal_q", "near_equal_q", "wide_logits", "ties", "neg_max", "nan",
         "pos_inf", "neg_inf", "gumbel_nan")


def host(t):
    return t.detach().cpu().numpy()


def dev(x):
    return torch.from_numpy(np.array(x)).cuda()


def same(got, want, what=""):
    """equal as raw bits; NaN matches NaN whatever its payload"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), what
        got, want = np.where(nan, 0, got), np.where(nan, 0, want)
        got, want = got.view(np.int32), want.view(np.int32)
    bad = np.argwhere(got != want)
    if bad.size:
        at = tuple(bad[0])
        raise AssertionError(f"{what}: first difference at {list(at)}: {got[at]} != {want[at]} ({len(bad)} in all)")


def tree_on_device(tree, b):
    """the first b games of an oracle tree as device tensors + the descriptor the C entry points take"""
    t = {name: dev(getattr(tree, name)[:b]) for name in STATS}
    d = A.hk_search_tree()
    for name in STATS:
        setattr(d, name, t[name].data_ptr())
    d.batch, d.num_nodes, d.num_actions = b, tree.node_visits.shape[1], tree.children_index.shape[2]
    return t, d


def copy_tree(tree):
    return SO.Tree(*(x.copy() for x in tree))


def _ptr(x):
    return None if x is None else x.data_ptr()


def _edges(tree, gumbel, seed):
    """overwrite the statistics of game g to reach edge KINDS[g % len(KINDS)] -> the invalid-action pattern"""
    rng = np.random.default_rng(seed)
    b, n, a = tree.children_index.shape
    invalid = np.zeros((b, a), np.uint8)
    ulp = np.float32(2.0 ** -25)  # of 0.25
    for g in range(b):
        kind = KINDS[g % len(KINDS)]
        live = np.flatnonzero(tree.node_visits[g] > 0)  # the nodes that exist
        if kind == "plain":
            invalid[g] = rng.random(a) < 0.3
        elif kind == "one_valid":
            invalid[g] = 1
            invalid[g, rng.integers(a)] = 0
        elif kind == "none_valid":
            invalid[g] = 1
        elif kind in ("equal_q", "near_equal_q", "ties"):
            # every Q-value and the raw values 0 (the 1e-8 span floor; 0, so that the mixed value is exactly 0 too and
            # the floor does not amplify the last bits of an exp()), or spread over less than 1e-6 around 0.25
            tree.children_rewards[g] = 0.0
            tree.children_discounts[g] = 1.0
            if kind == "near_equal_q":
                tree.children_values[g] = np.float32(0.25) + ulp * rng.integers(0, 17, (n, a))
                tree.raw_values[g] = np.float32(0.25) + ulp * rng.integers(0, 17, n)
            else:
                tree.children_values[g] = 0.0
                tree.raw_values[g] = 0.0
            tree.node_values[g] = tree.raw_values[g]
            if kind == "ties":  # equal logits, no noise: every considered action scores the same
                tree.children_prior_logits[g] = 0.0
                gumbel[g] = 0.0
        elif kind == "wide_logits":
            # exp() underflows to 0 in double for all but one logit per node (the FLT_MIN probability floor); the
            # survivor sits on an unvisited action where there is one
            tree.children_prior_logits[g] = rng.uniform(-1000.0, -750.0, (n, a)).astype(np.float32)
            for x in range(n):
                free = np.flatnonzero(tree.children_visits[g, x] == 0)
                top = rng.choice(free) if free.size else rng.integers(a)
                tree.children_prior_logits[g, x, top] = rng.uniform(-1.0, 1.0)
        elif kind == "neg_max":
            for arr in (tree.children_values[g], tree.children_prior_logits[g], tree.raw_values[g]):
                arr[rng.random(arr.shape) < 0.3] = -F32_MAX
            gumbel[g, rng.random(a) < 0.3] = -F32_MAX
        elif kind in ("nan", "pos_inf", "neg_inf"):
            v = {"nan": np.nan, "pos_inf": np.inf, "neg_inf": -np.inf}[kind]
            which = rng.integers(4)
            for _ in range(rng.integers(1, 3)):
                x = rng.choice(live)
                if which == 0:
                    tree.children_values[g, x, rng.integers(a)] = v
                elif which == 1:
                    tree.raw_values[g, x] = v
                    tree.node_values[g, x] = v
                elif which == 2:
                    tree.children_rewards[g, x, rng.integers(a)] = v
                else:  # logits of a node below the root
                    x = rng.choice(live[1:]) if live.size > 1 else rng.integers(1, n)
                    tree.children_prior_logits[g, x, rng.integers(a)] = v
        elif kind == "gumbel_nan":
            gumbel[g, rng.integers(a)] = np.nan
    return invalid


@functools.lru_cache(maxsize=None)
def _case(num_actions, max_considered):
    """(tree, gumbel, invalid pattern, table) of 257 games, edges applied; read-only for the tests"""
    seed = 100 * num_actions + max_considered
    tree, gumbel, table = grow_tree(max(BATCHES), num_actions, NUM_SIMULATIONS, GROWN, max_considered, seed)
    invalid = _edges(tree, gumbel, seed)
    for x in (*tree, gumbel, invalid, table):
        x.setflags(write=False)
    return tree, gumbel, invalid, table


def _considered(num_actions):
    return (1, num_actions, num_actions + 3)


def _select(tree, gumbel, invalid, table, max_considered, max_depth, next_free, b):
    t, d = tree_on_device(tree, b)
    g, inv, tab = dev(gumbel[:b]), None if invalid is None else dev(invalid[:b]), dev(table)
    out = [torch.full((b,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    check(lib().hk_search_select(C.byref(d), g.data_ptr(), _ptr(inv), tab.data_ptr(), max_considered,
                                 table.shape[1], max_depth, next_free, *(o.data_ptr() for o in out), None),
          "hk_search_select")
    torch.cuda.synchronize()
    for name in STATS:  # select writes nothing but its outputs
        same(host(t[name]), getattr(tree, name)[:b], name + " (select writes only its outputs)")
    return [host(o) for o in out]


@pytest.mark.parametrize("num_actions", ACTIONS)
def test_select_matches_oracle(num_actions):
    for max_considered in _considered(num_actions):
        tree, gumbel, invalid, table = _case(num_actions, max_considered)
        for max_depth in (1, 2, NUM_SIMULATIONS):
            for inv in (None, invalid):
                with np.errstate(all="ignore"):
                    want = SO.simulate(tree, gumbel, inv, table, max_considered, max_depth, GROWN + 1)
                for b in BATCHES:
                    got = _select(tree, gumbel, inv, table, max_considered, max_depth, GROWN + 1, b)
                    for name, x, y in zip(("parent", "action", "node"), got, want):
                        same(x, y[:b].astype(np.int32), f"{name} A={num_actions} m={max_considered} "
                                                        f"depth={max_depth} invalid={inv is not None} b={b}")


@pytest.mark.parametrize("num_actions", SUM_ORDER_ACTIONS)
def test_select_sums_in_action_order(num_actions):
    """the sums inside the lane-parallel completed Q-values (grp_seq_sum) add in action order 0 .. A-1, as the oracle:
    roots whose two best scores tie exactly in that order (test_search.sum_order_roots), so the first of the two must
    be chosen; another order of the same sums picks the other one in the games listed by butterfly_flips"""
    tree, gumbel, table, m, tied = sum_order_roots(max(BATCHES), num_actions, num_actions)
    assert tied.all()
    flips = butterfly_flips(tree, gumbel, table, m)
    assert flips.size >= 1  # the fixture tells the orders apart
    want = SO.simulate(tree, gumbel, None, table, m, 1, 7)
    for b in BATCHES:
        got = _select(tree, gumbel, None, table, m, 1, 7, b)
        for name, x, y in zip(("parent", "action", "node"), got, want):
            same(x, y[:b].astype(np.int32), f"{name} A={num_actions} b={b} (order-sensitive games: {flips.tolist()})")


def _step_outputs(b, a, seed):
    """what a recurrent function hands the backup, with non-finite entries in some games"""
    rng = np.random.default_rng(seed)
    logits = rng.normal(size=(b, a)).astype(np.float32)
    value = rng.normal(size=b).astype(np.float32)
    reward = rng.normal(size=b).astype(np.float32)
    discount = rng.choice(np.array([0.0, 0.99, 1.0], np.float32), b)
    for g in range(0, b, 5):
        v = (np.nan, np.inf, -np.inf, -F32_MAX)[(g // 5) % 4]
        target = (g // 20) % 3
        if target == 0:
            logits[g, rng.integers(a)] = v
        elif target == 1:
            value[g] = v
        else:
            reward[g] = v
    return logits, value, reward, discount


def _backup_and_compare(tree, parent, action, node, outs, what):
    logits, value, reward, discount = outs
    with np.errstate(all="ignore"):
        want = copy_tree(tree)
        SO.expand(want, parent, action, node, logits, value, reward, discount)
        SO.backward(want, node)
    for b in BATCHES:
        if b > tree.node_visits.shape[0]:
            continue
        t, d = tree_on_device(tree, b)
        ins = [dev(np.asarray(x[:b], dt)) for x, dt in zip((parent, action, node, logits, value, reward, discount),
                                                           (np.int32,) * 3 + (np.float32,) * 4)]
        check(lib().hk_search_backup(C.byref(d), *(x.data_ptr() for x in ins), None), "hk_search_backup")
        for name in STATS:
            same(host(t[name]), getattr(want, name)[:b], f"{name} {what} b={b}")


@pytest.mark.parametrize("num_actions", ACTIONS)
def test_backup_matches_oracle(num_actions):
    """expansion + backward pass after the oracle's own descent: a new node, or the existing child at the depth cut"""
    for max_considered in _considered(num_actions):
        tree, gumbel, invalid, table = _case(num_actions, max_considered)
        for max_depth in (1, NUM_SIMULATIONS):
            with np.errstate(all="ignore"):
                parent, action, node = SO.simulate(tree, gumbel, invalid, table, max_considered, max_depth, GROWN + 1)
            outs = _step_outputs(len(parent), num_actions, num_actions + max_depth)
            what = f"A={num_actions} m={max_considered} depth={max_depth}"
            _backup_and_compare(tree, parent, action, node, outs, what)


@pytest.mark.parametrize("discount", [0.0, 1.0])
def test_backup_long_chain(discount):
    """a path of 64 nodes below the root (every node the only child of the one above): the backward pass walks 65
    edges; discounts of 0 (the leaf value stops at the first edge) and 1 (it adds up all the way)"""
    b, a, depth = 65, 5, 64
    n = depth + 2
    rng = np.random.default_rng(int(discount) + 7)
    tree = SO.new_tree(b, n, a, 1)
    acts = rng.integers(0, a, (b, depth + 1))
    for g in range(b):
        for x in range(1, depth + 1):
            tree.parents[g, x], tree.action_from_parent[g, x] = x - 1, acts[g, x]
            tree.children_index[g, x - 1, acts[g, x]] = x
        tree.node_visits[g, :depth + 1] = np.arange(depth + 1, 0, -1)
        for x in range(1, depth + 1):
            tree.children_visits[g, x - 1, acts[g, x]] = tree.node_visits[g, x]
    tree.children_prior_logits[:] = rng.normal(size=(b, n, a))
    tree.node_values[:, :depth + 1] = rng.normal(size=(b, depth + 1))
    tree.raw_values[:] = tree.node_values
    tree.children_rewards[:] = rng.normal(size=(b, n, a))
    tree.children_discounts[:] = discount
    for g in range(b):
        for x in range(1, depth + 1):
            tree.children_values[g, x - 1, acts[g, x]] = tree.node_values[g, x]
    parent = np.full(b, depth, np.int64)
    action = acts[:, 0]
    node = np.full(b, depth + 1, np.int64)
    logits, value, reward, _ = _step_outputs(b, a, 11)
    discount_in = np.full(b, discount, np.float32)
    _backup_and_compare(tree, parent, action, node, (logits, value, reward, discount_in), f"chain discount={discount}")


@pytest.mark.parametrize("num_actions", ACTIONS)
def test_policy_matches_oracle(num_actions):
    for max_considered in _considered(num_actions):
        tree, gumbel, invalid, _ = _case(num_actions, max_considered)
        for inv in (None, invalid):
            with np.errstate(all="ignore"):
                want_action, want_weights = SO.final_policy(tree, gumbel, inv)
            for b in BATCHES:
                t, d = tree_on_device(tree, b)
                g, i = dev(gumbel[:b]), None if inv is None else dev(inv[:b])
                action = torch.full((b,), -7, dtype=torch.int32, device="cuda")
                weights = torch.full((b, num_actions), -7.0, dtype=torch.float32, device="cuda")
                check(lib().hk_search_policy(C.byref(d), g.data_ptr(), _ptr(i), action.data_ptr(), weights.data_ptr(),
                                             None), "hk_search_policy")
                what = f"A={num_actions} m={max_considered} invalid={inv is not None} b={b}"
                same(host(action), want_action[:b], "action " + what)
                same(host(weights), want_weights[:b], "weights " + what)


def _torch_recurrent(fn, poison=False):
    """a numpy recurrent function for the HIP search; poison: non-finite outputs for some games (the same for both
    searches: drawn from the per-simulation key)"""
    def numpy_fn(params, key, action, embedding):
        (reward, discount, logits, value), nxt = fn(params, key, action, embedding)
        if poison:
            rng = np.random.default_rng(key % (1 << 32))
            reward, logits, value = reward.copy(), logits.copy(), value.copy()
            for g in np.flatnonzero(rng.random(len(action)) < 0.15):
                v = (np.nan, np.inf, -np.inf)[rng.integers(3)]
                target = rng.integers(3)
                if target == 0:
                    reward[g] = v
                elif target == 1:
                    value[g] = v
                else:
                    logits[g, rng.integers(logits.shape[1])] = v
        return (reward, discount, logits, value), nxt

    def torch_fn(params, key, action, embedding):
        (reward, discount, logits, value), nxt = numpy_fn(params, key, host(action), host(embedding))
        return RecurrentFnOutput(dev(reward), dev(discount), dev(logits), dev(value)), dev(nxt)

    return numpy_fn, torch_fn


@pytest.mark.parametrize("num_actions", ACTIONS)
def test_whole_search_matches_oracle(num_actions):
    """search.gumbel_muzero_policy against SO.gumbel_muzero_policy on the toy environment; the second round with
    non-finite network outputs and a NaN in the root noise"""
    b, n = 65, 10
    rng = np.random.default_rng(num_actions)
    logits = (2.0 * rng.normal(size=(b, num_actions))).astype(np.float32)
    value = rng.normal(size=b).astype(np.float32)
    emb = rng.integers(0, 7, size=(b, 1)).astype(np.float32)
    gumbel = (0.3 * rng.gumbel(size=(b, num_actions))).astype(np.float32)
    invalid = np.zeros((b, num_actions), np.uint8)
    invalid[::3, -1] = 1
    for poison in (False, True):
        if poison:
            gumbel[::7, rng.integers(num_actions)] = np.nan
        numpy_fn, torch_fn = _torch_recurrent(_toy_recurrent_fn(num_actions, 9), poison)
        for inv in (None, invalid):
            for max_considered in (4, num_actions):
                out = gumbel_muzero_policy((), 77, RootFnOutput(dev(logits), dev(value), dev(emb)), torch_fn, n,
                                           invalid_actions=None if inv is None else dev(inv),
                                           max_num_considered_actions=max_considered, gumbel=dev(gumbel))
                with np.errstate(all="ignore"):
                    want = SO.gumbel_muzero_policy((), logits, value, emb, numpy_fn, n, gumbel, invalid_actions=inv,
                                                   max_num_considered_actions=max_considered, rng_key=77)
                what = f"A={num_actions} poison={poison} invalid={inv is not None} m={max_considered}"
                for name in STATS + ("embeddings",):
                    same(host(getattr(out.search_tree, name)), getattr(want.search_tree, name), f"{name} {what}")
                same(host(out.action).astype(np.int32), want.action, "action " + what)
                same(host(out.action_weights), want.action_weights, "weights " + what)


def test_captured_search_equals_eager_at_32_actions():
    """CapturedSearch replays the AMAX 32 kernels from a hipGraph with the eager result"""
    b, a, n = 40, 32, 8

    def graph_safe(params, key, action, embedding):  # the toy environment in tensor operations (no host copies)
        nxt = torch.remainder(embedding * 3 + action[:, None].to(embedding.dtype) + 1, 7)
        logits = W.index_select(0, nxt[:, 0].long())
        return RecurrentFnOutput((nxt[:, 0] == 0).to(torch.float32), torch.full((len(action),), 0.99, device="cuda"),
                                 logits, torch.tanh(logits[:, 0])), nxt

    W = torch.randn(7, a, generator=torch.Generator().manual_seed(5)).cuda()
    rng = np.random.default_rng(1)
    cap = None
    for seed in (1, 2):
        root = RootFnOutput(dev((2.0 * rng.normal(size=(b, a))).astype(np.float32)),
                            dev(rng.normal(size=b).astype(np.float32)),
                            dev(rng.integers(0, 7, size=(b, 1)).astype(np.float32)))
        if cap is None:
            cap = CapturedSearch((), 5, root, graph_safe, n, max_num_considered_actions=16, gumbel_scale=0.5)
        got = cap(10 + seed, root)
        want = gumbel_muzero_policy((), 10 + seed, root, graph_safe, n, max_num_considered_actions=16,
                                    gumbel_scale=0.5)
        assert torch.equal(got.action, want.action)
        assert torch.equal(got.action_weights, want.action_weights)
        for name in STATS + ("embeddings",):
            assert torch.equal(getattr(got.search_tree, name), getattr(want.search_tree, name)), name


@pytest.mark.parametrize("d", [2, 5, 6])
def test_expand_operators_at_more_dims(d):
    """the expansion glue at dim 2, 5 and 6, with logit rows that are all NaN, all -inf or tied; the agent's action
    mask written in place (out == logits)"""
    L = lib()
    rng = np.random.default_rng(d)
    b, n, m = 70, 6, 7
    e, ncls = m * d, 2 ** d - d - 1
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)
    emb, feat, o2, f2 = f32(b, n, e), f32(b, n, e), f32(b, e), f32(b, e)
    parent = rng.integers(0, n, b).astype(np.int32)
    node = rng.integers(0, n, b).astype(np.int32)
    action = rng.integers(-1, ncls + 1, b).astype(np.int32)
    logits, hl = f32(b, d), f32(b, ncls)
    for x in (logits, hl):
        x[0::4] = np.nan
        x[1::4] = -np.inf
        x[2::4] = 0.5
        x[3::8, -1] = np.nan
    g_emb, g_feat, g_par, g_act, g_node = dev(emb), dev(feat), dev(parent), dev(action), dev(node)
    obs = torch.empty((b, e), dtype=torch.float32, device="cuda")
    af = torch.empty((b, e + d), dtype=torch.float32, device="cuda")
    check(L.hk_search_expand_gather(g_emb.data_ptr(), g_feat.data_ptr(), g_par.data_ptr(), g_act.data_ptr(),
                                    obs.data_ptr(), af.data_ptr(), b, n, m, d, 0, None), "gather")
    want_obs, want_af = SO.expand_gather(emb, feat, parent, action, d)
    same(host(obs), want_obs, "obs")
    same(host(af), want_af, "agent features")
    g_log = dev(logits)
    axis = torch.empty(b, dtype=torch.int32, device="cuda")
    check(L.hk_search_masked_argmax(g_log.data_ptr(), g_act.data_ptr(), axis.data_ptr(), b, d, None), "argmax")
    same(host(axis), SO.masked_argmax(logits, action, d), "masked argmax")
    g_o2, g_f2, g_hl = dev(o2), dev(f2), dev(hl)
    check(L.hk_search_expand_scatter(g_o2.data_ptr(), g_f2.data_ptr(), g_node.data_ptr(), g_emb.data_ptr(),
                                     g_feat.data_ptr(), b, n, m, d, None), "scatter")
    want_emb, want_feat = SO.expand_scatter(o2, f2, node, emb, feat)
    same(host(g_emb), want_emb, "embeddings")
    same(host(g_feat), want_feat, "features")
    embA, featA = f32(b, n, e + d), f32(b, n, e)
    g_embA, g_featA = dev(embA), dev(featA)
    pts = torch.empty((b, e), dtype=torch.float32, device="cuda")
    crd = torch.empty((b, d), dtype=torch.float32, device="cuda")
    check(L.hk_search_expand_gather_agent(g_embA.data_ptr(), g_par.data_ptr(), pts.data_ptr(), crd.data_ptr(), b, n,
                                          m, d, None), "gather_agent")
    want_pts, want_crd = SO.expand_gather_agent(embA, parent, d)
    same(host(pts), want_pts, "points")
    same(host(crd), want_crd, "coords")
    afeat = torch.empty((b, e + d), dtype=torch.float32, device="cuda")
    cls = torch.empty(b, dtype=torch.int32, device="cuda")
    check(L.hk_search_expand_scatter_agent(g_o2.data_ptr(), g_f2.data_ptr(), g_hl.data_ptr(), g_node.data_ptr(),
                                           g_embA.data_ptr(), g_featA.data_ptr(), afeat.data_ptr(), cls.data_ptr(),
                                           b, n, m, d, ncls, None), "scatter_agent")
    want_embA, want_featA, want_afeat, want_cls = SO.expand_scatter_agent(o2, f2, hl, node, embA, featA, d)
    same(host(cls), want_cls, "host class")
    same(host(afeat), want_afeat, "agent features (agent tree)")
    same(host(g_embA), want_embA, "embeddings (agent tree)")
    same(host(g_featA), want_featA, "features (agent tree)")
    check(L.hk_search_mask_logits(g_log.data_ptr(), cls.data_ptr(), g_log.data_ptr(), b, d, None), "mask_logits")
    same(host(g_log), SO.mask_logits(logits, want_cls, d), "mask_logits in place")


def test_search_entry_point_bounds():
    """the shape checks of the three C entry points and of the driver"""
    L = lib()
    tree, gumbel, invalid, table = _case(4, 4)
    t, d = tree_on_device(tree, 8)
    g, tab = dev(gumbel[:8]), dev(table)
    out = [torch.zeros(8, dtype=torch.int32, device="cuda") for _ in range(3)]
    w = torch.zeros((8, 4), dtype=torch.float32, device="cuda")
    select = lambda m, sims, depth, nf: L.hk_search_select(C.byref(d), g.data_ptr(), None, tab.data_ptr(), m, sims,
                                                           depth, nf, *(o.data_ptr() for o in out), None)
    assert select(4, NUM_SIMULATIONS, NUM_SIMULATIONS, GROWN + 1) == A.HK_OK
    assert select(4, NUM_SIMULATIONS, NUM_SIMULATIONS, NUM_SIMULATIONS) == A.HK_OK  # the last node
    assert select(4, NUM_SIMULATIONS, NUM_SIMULATIONS, NUM_SIMULATIONS + 1) == A.HK_ERR_SHAPE  # next_free == nodes
    assert select(4, NUM_SIMULATIONS, NUM_SIMULATIONS, 0) == A.HK_ERR_SHAPE  # the root is never free
    assert select(4, NUM_SIMULATIONS, 0, GROWN + 1) == A.HK_ERR_SHAPE  # max_depth
    assert select(0, NUM_SIMULATIONS, NUM_SIMULATIONS, GROWN + 1) == A.HK_ERR_SHAPE  # max_num_considered_actions
    assert select(4, NUM_SIMULATIONS + 1, NUM_SIMULATIONS, GROWN + 1) == A.HK_ERR_SHAPE  # num_simulations + 1 > nodes
    assert select(4, 0, NUM_SIMULATIONS, GROWN + 1) == A.HK_ERR_SHAPE
    torch.cuda.synchronize()
    d.num_actions = 0
    assert L.hk_search_policy(C.byref(d), g.data_ptr(), None, out[0].data_ptr(), w.data_ptr(), None) == A.HK_ERR_SHAPE
    # 33 actions, past the largest bucket, on buffers sized for 33 (a regressed check returns HK_OK, nothing overruns)
    wide = SO.new_tree(8, NUM_SIMULATIONS + 1, 33, 1)
    wide.node_visits[:, 0] = 1
    t33, d33 = tree_on_device(wide, 8)
    g33 = torch.zeros((8, 33), dtype=torch.float32, device="cuda")
    w33 = torch.zeros((8, 33), dtype=torch.float32, device="cuda")
    tab33 = dev(SO.get_table_of_considered_visits(4, NUM_SIMULATIONS))
    edge = [torch.tensor(v, dtype=torch.int32, device="cuda").repeat(8) for v in (0, 0, 1)]  # parent, action, node
    one = torch.zeros(8, dtype=torch.float32, device="cuda")
    assert L.hk_search_select(C.byref(d33), g33.data_ptr(), None, tab33.data_ptr(), 4, NUM_SIMULATIONS,
                              NUM_SIMULATIONS, 1, *(o.data_ptr() for o in out), None) == A.HK_ERR_SHAPE
    assert L.hk_search_backup(C.byref(d33), *(x.data_ptr() for x in edge), w33.data_ptr(), one.data_ptr(),
                              one.data_ptr(), one.data_ptr(), None) == A.HK_ERR_SHAPE
    assert L.hk_search_policy(C.byref(d33), g33.data_ptr(), None, out[0].data_ptr(), w33.data_ptr(),
                              None) == A.HK_ERR_SHAPE
    root = RootFnOutput(torch.zeros((2, 33), device="cuda"), torch.zeros(2, device="cuda"),
                        torch.zeros((2, 1), device="cuda"))
    with pytest.raises(ValueError, match="32 actions"):
        gumbel_muzero_policy((), 0, root, lambda *a: None, 4)
