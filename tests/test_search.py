"""Gumbel-MuZero search.  The reference takes it from the third-party package mctx,
which is not available: PARITY UNPINNED.  CPU tests: the sequential-halving schedule and invariants of
the restatement in oracle/search_oracle.py.  GPU tests: the HIP tree kernels + driver against that
restatement, on the real environment."""
import numpy as np
import pytest

from oracle import search_oracle as SO


def test_sequential_halving_schedule():
    # worked by hand from the definition: 4 considered actions, 16 simulations -> two rounds over 4 actions,
    # then 4 rounds over the best 2
    assert SO.get_sequence_of_considered_visits(4, 16) == (0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5)
    assert SO.get_sequence_of_considered_visits(1, 5) == (0, 1, 2, 3, 4)
    assert SO.get_sequence_of_considered_visits(0, 3) == (0, 1, 2)
    for m in (2, 3, 4, 11, 16):
        for n in (1, 7, 32, 50):
            seq = SO.get_sequence_of_considered_visits(m, n)
            assert len(seq) == n and seq[0] == 0
            assert all(b - a in (0, 1) or b < a for a, b in zip(seq, seq[1:]))
    table = SO.get_table_of_considered_visits(4, 32)
    assert table.shape == (5, 32) and table.dtype == np.int32


def _toy_recurrent_fn(num_actions, seed):
    """a deterministic synthetic environment + evaluator on integer embeddings"""
    rng = np.random.default_rng(seed)
    w = rng.normal(size=(7, num_actions)).astype(np.float32)

    def recurrent_fn(params, key, action, embedding):
        nxt = (embedding * 3 + action[:, None] + 1) % 7
        feat = np.eye(7, dtype=np.float32)[nxt[:, 0].astype(np.int64)]
        logits = feat @ w
        value = np.tanh(feat @ w[:, 0]).astype(np.float32)
        reward = ((nxt[:, 0] == 0) * 1.0).astype(np.float32)
        discount = np.full(len(action), 0.99, np.float32)
        return (reward, discount, logits, value), nxt.astype(embedding.dtype)

    return recurrent_fn


@pytest.mark.parametrize("num_actions,num_simulations,max_considered", [(4, 32, 16), (3, 8, 2), (11, 20, 4), (4, 5, 16)])
def test_oracle_search_invariants(num_actions, num_simulations, max_considered):
    rng = np.random.default_rng(5)
    b = 64
    logits = rng.normal(size=(b, num_actions)).astype(np.float32)
    value = rng.normal(size=b).astype(np.float32)
    emb = rng.integers(0, 7, size=(b, 1)).astype(np.float32)
    gumbel = (0.3 * rng.gumbel(size=(b, num_actions))).astype(np.float32)
    out = SO.gumbel_muzero_policy((), logits, value, emb, _toy_recurrent_fn(num_actions, 1), num_simulations, gumbel,
                                  max_num_considered_actions=max_considered)
    t = out.search_tree
    assert np.all(t.children_visits[:, 0].sum(-1) == num_simulations)
    assert np.all(t.node_visits[:, 0] == num_simulations + 1)
    assert np.allclose(out.action_weights.sum(-1), 1.0, atol=1e-6) and np.all(out.action_weights >= 0)
    rows = np.arange(b)
    assert np.all(t.children_visits[rows, 0, out.action] == t.children_visits[:, 0].max(-1))
    assert np.all(t.children_index[rows, 0, out.action] >= 1)
    # every expanded node hangs under the edge that points to it
    for g in range(b):
        for n in range(1, num_simulations + 1):
            p, a = t.parents[g, n], t.action_from_parent[g, n]
            if p >= 0:
                assert t.children_index[g, p, a] == n
    # the number of root actions ever tried is bounded by the Gumbel-top-k size
    assert np.all((t.children_visits[:, 0] > 0).sum(-1) <= min(max_considered, num_actions))
    # with an invalid-action mask the masked actions are never visited nor chosen
    invalid = np.zeros((b, num_actions), np.uint8)
    invalid[:, 0] = 1
    out2 = SO.gumbel_muzero_policy((), logits, value, emb, _toy_recurrent_fn(num_actions, 1), num_simulations, gumbel,
                                   invalid_actions=invalid, max_num_considered_actions=max_considered)
    assert np.all(out2.search_tree.children_visits[:, 0, 0] == 0) and np.all(out2.action != 0)
    assert np.all(out2.action_weights[:, 0] < 1e-12)


def test_oracle_search_depth_limit():
    rng = np.random.default_rng(6)
    b, a, n = 32, 4, 24
    logits = rng.normal(size=(b, a)).astype(np.float32)
    out = SO.gumbel_muzero_policy((), logits, np.zeros(b, np.float32), np.zeros((b, 1), np.float32),
                                  _toy_recurrent_fn(a, 2), n, np.zeros((b, a), np.float32), max_depth=2,
                                  max_num_considered_actions=2)
    t = out.search_tree
    # depth of every node <= 2
    for g in range(b):
        for node in range(1, n + 1):
            if t.parents[g, node] >= 0:
                d, x = 0, node
                while x != 0:
                    x = t.parents[g, x]
                    d += 1
                assert d <= 2
    assert np.all(t.node_visits[:, 0] == n + 1)


def test_expansion_glue_restatement():
    """oracle/search_oracle.py's expansion glue: the argmax rule equals the tensor library's (first maximum, NaN wins),
    decode clamps, gather / scatter are inverse on the touched rows"""
    import torch
    rng = np.random.default_rng(0)
    x = rng.standard_normal((200, 4)).astype(np.float32)
    x[rng.random(x.shape) < 0.15] = np.nan
    x[rng.random(x.shape) < 0.15] = 0.5
    assert np.array_equal(SO._first_argmax_nan_wins(x), torch.argmax(torch.tensor(x), dim=1).numpy())
    b, n, m, d = 50, 6, 5, 3
    e = m * d
    emb = rng.standard_normal((b, n, e)).astype(np.float32)
    feat = rng.standard_normal((b, n, e)).astype(np.float32)
    parent = rng.integers(0, n, b)
    action = rng.integers(-2, 7, b)
    obs, af = SO.expand_gather(emb, feat, parent, action, d)
    assert obs.shape == (b, e) and af.shape == (b, e + d)
    assert set(np.unique(af[:, e:])) <= {0.0, 1.0} and (af[:, e:].sum(axis=1) >= 2).all()
    emb2, feat2 = SO.expand_scatter(obs, af[:, :e], parent, emb, feat)
    assert np.array_equal(emb2, emb) and np.array_equal(feat2, feat)
    ax = SO.masked_argmax(x[:b, :d], action, d)
    assert (af[np.arange(b), e + ax] == 1.0).all()
    ml = SO.mask_logits(x[:b, :d], np.clip(action, 0, 3), d)
    assert np.isneginf(ml[af[:, e:] == 0.0]).all()


def grow_tree(batch, num_actions, num_simulations, k, max_considered, seed, max_depth=None):
    """the oracle's tree after k < num_simulations simulations of a search over _toy_recurrent_fn (the snapshot the
    kernel tests start from) -> (tree, root gumbel [B, A], table of considered visits)"""
    rng = np.random.default_rng(seed)
    logits = (2.0 * rng.normal(size=(batch, num_actions))).astype(np.float32)
    value = rng.normal(size=batch).astype(np.float32)
    emb = rng.integers(0, 7, size=(batch, 1)).astype(np.float32)
    gumbel = (0.3 * rng.gumbel(size=(batch, num_actions))).astype(np.float32)
    fn = _toy_recurrent_fn(num_actions, seed)
    tree = SO.instantiate_tree_from_root(logits, value, emb, num_simulations)
    table = SO.get_table_of_considered_visits(max_considered, num_simulations)
    max_depth = num_simulations if max_depth is None else max_depth
    bi = np.arange(batch)
    for sim in range(k):
        node, action, new_node = SO.simulate(tree, gumbel, None, table, max_considered, max_depth, sim + 1)
        (reward, discount, prior, val), nxt = fn((), None, action, tree.embeddings[bi, node])
        tree.embeddings[bi, new_node] = nxt
        SO.expand(tree, node, action, new_node, prior, val, reward, discount)
        SO.backward(tree, new_node)
    return tree, gumbel, table


def test_oracle_steps_compose_to_the_search():
    """grow_tree's loop of simulate / expand / backward run to the end + final_policy is gumbel_muzero_policy"""
    b, a, n, m = 24, 5, 9, 4
    tree, gumbel, _ = grow_tree(b, a, n, n, m, 3)
    rng = np.random.default_rng(3)
    logits = (2.0 * rng.normal(size=(b, a))).astype(np.float32)
    value = rng.normal(size=b).astype(np.float32)
    emb = rng.integers(0, 7, size=(b, 1)).astype(np.float32)
    want = SO.gumbel_muzero_policy((), logits, value, emb, _toy_recurrent_fn(a, 3), n, gumbel,
                                   max_num_considered_actions=m)
    for name in SO.Tree._fields:
        assert np.array_equal(getattr(tree, name), getattr(want.search_tree, name)), name
    action, weights = SO.final_policy(tree, gumbel, None)
    assert np.array_equal(action, want.action) and np.array_equal(weights, want.action_weights)


@pytest.mark.parametrize("num_actions", [1, 2, 17, 32])
def test_oracle_search_at_every_bucket_end(num_actions):
    """invariants of the restatement at the action counts the other tests skip: 1, 2 and past 16"""
    b, n = 16, 12
    tree, gumbel, _ = grow_tree(b, num_actions, n, n, 16, 4)
    assert np.all(tree.node_visits[:, 0] == n + 1) and np.all(tree.children_visits[:, 0].sum(-1) == n)
    assert np.all((tree.children_visits[:, 0] > 0).sum(-1) <= min(16, num_actions))
    action, weights = SO.final_policy(tree, gumbel, None)
    rows = np.arange(b)
    assert np.all(tree.children_visits[rows, 0, action] == tree.children_visits[:, 0].max(-1))
    assert np.allclose(weights.sum(-1), 1.0, atol=1e-6)
    # every action invalid: nothing is considered (row 0 of the table), the first action is taken
    invalid = np.ones((b, num_actions), np.uint8)
    table = SO.get_table_of_considered_visits(16, n)
    fresh, _, _ = grow_tree(b, num_actions, n, 3, 16, 4)
    node, act, _ = SO.simulate(fresh, gumbel, invalid, table, 16, 1, 4)  # (max_depth 1: the root's choice)
    assert np.all(node == 0) and np.all(act == 0)
    action, _ = SO.final_policy(fresh, gumbel, invalid)
    assert np.all(action == 0)


def test_oracle_depth_cut_and_nan_rule():
    """simulate stops at the depth limit on an EXISTING child; a NaN statistic wins the argmax (numpy / JAX rule)"""
    b, a, n = 8, 4, 10
    tree, gumbel, table = grow_tree(b, a, n, 6, 1, 5)  # one considered action: one deep path
    node, action, new_node = SO.simulate(tree, gumbel, None, table, 1, 1, 7)
    assert np.all(node == 0)
    assert np.array_equal(new_node, tree.children_index[np.arange(b), 0, action])
    assert np.all(new_node >= 1)
    node, action, new_node = SO.simulate(tree, gumbel, None, table, 1, n, 7)
    assert np.all(new_node == 7)
    g2 = gumbel.copy()
    g2[:, 2] = np.nan
    with np.errstate(invalid="ignore"):
        node, action, _ = SO.simulate(tree, g2, None, table, 1, 1, 7)
        assert np.all(action == 2)  # NaN + the -inf penalty is still NaN
        act, _ = SO.final_policy(tree, g2, None)
    assert np.all(act == 2)


def butterfly_sum(x: np.ndarray) -> np.ndarray:
    """the sum over the last axis in the order of an xor-butterfly over a power-of-two group of lanes (lanes past the
    end hold 0): NOT the kernels' order -- a stand-in for a reduction someone might swap in"""
    a = x.shape[-1]
    width = 4
    while width < a:
        width *= 2
    v = np.zeros(x.shape[:-1] + (width,), x.dtype)
    v[..., :a] = x
    off = width // 2
    while off:
        v = v + v[..., np.arange(width) ^ off]
        off //= 2
    return v[..., 0]


def sum_order_roots(batch, num_actions, seed):
    """roots on which the root choice depends on the order of the sums inside the completed Q-values.

    Every prior logit is 0 (every exp() is exp(0) = 1, exact on any machine).  k >= 3 of the root actions (not all) were
    visited once; their Q-values lie within 1e-8 of each other and above the mixed value, so the span is the 1e-8 floor and every
    completed Q moves by ~1e-11 with the last bit of the mixed value -- of the sums over the visited actions.  Two of
    them, x and y, differ in Q by 2^-60 only (q_y = (1 + 2^-23) * (2^-14 - 2^-37) in double, q_x = 2^-14); y's Gumbel
    entry (~4e-10, its float32 steps far below a float64 step of the score) is tuned until the two scores tie EXACTLY
    in the oracle's order, and the first of the two wins.  Another order of the same sums breaks the tie at random.
    -> (tree, gumbel, table, max_considered, tied [B] bool: the games whose tie could be made exact)"""
    assert num_actions >= 4
    rng = np.random.default_rng(seed)
    n = 17
    k = min(num_actions - 1, 10)  # visited actions: at least one unvisited action carries the mixed value
    tree = SO.new_tree(batch, n, num_actions, 1)
    gumbel = np.full((batch, num_actions), -1.0, np.float32)
    x_q, u = np.float32(2.0 ** -14), np.float32(2.0 ** -37)
    tied = np.zeros(batch, bool)
    for g in range(batch):
        acts = rng.choice(num_actions, k, replace=False)
        for i, act in enumerate(acts):
            tree.parents[g, i + 1], tree.action_from_parent[g, i + 1] = 0, act
            tree.children_index[g, 0, act] = i + 1
            tree.node_visits[g, i + 1] = 1
            tree.children_visits[g, 0, act] = 1
        tree.node_visits[g, 0] = k + 1
        tree.children_discounts[g, 0] = 1.0
        vals = x_q + u * rng.integers(1, 60, k).astype(np.float32)
        x, y = rng.choice(acts, 2, replace=False)
        vals[list(acts).index(x)] = x_q
        vals[list(acts).index(y)] = x_q - u
        tree.children_discounts[g, 0, y] = np.float32(1.0 + 2.0 ** -23)
        tree.children_values[g, 0, acts] = vals
        tree.node_values[g, 1:k + 1] = vals
        tree.raw_values[g, 0] = x_q - u * np.float32(rng.integers(2000, 4000))
        tree.node_values[g, 0] = tree.raw_values[g, 0]
        gumbel[g, x] = 0.0
        cq = SO.completed_qvalues(SO.Tree(*(f[g:g + 1] for f in tree)), np.zeros(1, np.int64))[0]
        want = np.float64(0.0) + 0.0 + cq[x]
        z = np.float32(cq[x] - cq[y])
        for _ in range(64):  # walk float32 steps towards the exact tie
            s = np.float64(z) + 0.0 + cq[y]
            if s == want:
                tied[g] = True
                break
            z = np.nextafter(z, np.float32(np.inf if s < want else -np.inf))
        gumbel[g, y] = z
    table = SO.get_table_of_considered_visits(k, n - 1)  # k considered: the k visited actions at the next simulation
    return tree, gumbel, table, k, tied


SUM_ORDER_ACTIONS = (8, 9, 16, 17, 26, 32)  # (with 3-4 visited actions, at 4 or 5 actions, no order mattered)


def butterfly_flips(tree, gumbel, table, max_considered):
    """games of a sum_order_roots fixture whose root choice changes when the oracle adds in butterfly order"""
    _, want, _ = SO.simulate(tree, gumbel, None, table, max_considered, 1, 7)
    sums = SO._seq_sum
    try:
        SO._seq_sum = butterfly_sum
        _, other, _ = SO.simulate(tree, gumbel, None, table, max_considered, 1, 7)
    finally:
        SO._seq_sum = sums
    return np.flatnonzero(want != other)


def test_sum_order_roots_discriminate():
    """the fixture of the kernels' summation-order test: exact ties in the oracle's order, and a butterfly order of the
    same sums changes the root choice in some games at every action count the GPU test uses"""
    for a in SUM_ORDER_ACTIONS:
        tree, gumbel, table, m, tied = sum_order_roots(257, a, a)
        assert tied.all(), a
        assert butterfly_flips(tree, gumbel, table, m).size >= 1, a
