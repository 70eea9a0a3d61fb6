"""The Morin game played forward, restated in plain Python on exact integers: what hk_search_morin_play /
hironaka_amd.ops.morin_play define as their outputs (hironaka/game.py:122-154 GameMorin, hironaka/agent.py:114-136
AgentMorin, core/list_points.py:86-116 the tracked get_newton_polytope).  The hosts, the child and the class codec are
tests/search_rules.py's.  Nothing here comes from hironaka_amd: test_morin_rules.py pins this module to the fixture made
by running the reference (tests/golden/make_morin_game_golden.py), and the GPU tests compare the kernel with it.

A root is an [m, d] array whose rows with coordinate 0 >= 0 are the points, holes anywhere; `dist` is a row index of
that array or -1.  Every state made here is an int64 array of live rows only."""
from collections import namedtuple

import numpy as np

from search_rules import class_id, host_list, live, morin_child, newton

RUNNING, ENDED, NO_CONTRIBUTION, NO_MOVE, INEXACT = 0, 1, 2, 3, 4  # HK_MORIN_*
LIMITS = {np.dtype(np.float32): 2 ** 24, np.dtype(np.float64): 2 ** 53}

Played = namedtuple("Played", "state weights dist length outcome classes axes history untouched")
# state: the final live rows; dist: the distinguished row or -1; classes / axes: the moves played; history: (state,
# weights, dist) after every move; untouched: the root left the call as it came (holes and all)


def subset_of_class(cls, d):
    """the coordinates of class id `cls`, None when the dimension has no such class"""
    masks = [v for v in range(1 << d) if bin(v).count("1") >= 2]
    if not 0 <= cls < len(masks):
        return None
    return [k for k in range(d) if (masks[cls] >> k) & 1]


def tracked_newton(state, dist):
    """ListPoints._get_newton_polytope with row `dist` marked: (state, the row's new index or -1 when it is lost).  The
    marked row sorts before an identical one and is removed as contained, so a twin loses it too."""
    state = np.asarray(state)
    pts = live(state)
    kept = newton(pts)
    if dist < 0:
        return kept, -1
    p = pts[int((state[:dist, 0] >= 0).sum())]
    others = np.delete(pts, int((state[:dist, 0] >= 0).sum()), axis=0)
    if len(others) and (others <= p).all(1).any():
        return kept, -1
    return kept, int(np.nonzero((kept == p).all(1))[0][0])


def morin_axis(coords, w, tie):
    """AgentMorin._get_actions on the two lowest coordinates of the subset; None where a random tie has to be fed in"""
    c0, c1 = sorted(coords)[:2]
    if w[c0] != w[c1]:
        return c0 if w[c0] < w[c1] else c1
    return {"lowest": c0, "highest": max(coords)}.get(tie)


def next_weights(coords, w, a, rule):
    if rule == "agent":
        return [0 if i in coords and i != a else w[i] for i in range(len(w))]
    return [w[i] - w[a] if i in coords and i != a else w[i] for i in range(len(w))]


def play(root, weights, dist, host, max_steps, classes=None, axes=None, tie="lowest", weight_rule="agent",
         reduce_root=False, limit=2 ** 53):
    """host: a name of search_rules.HOSTS, select(state) -> the host's list, or None (every class forced).  classes /
    axes: per move, an entry < 0 (or a missing one) leaves the move to the host / the agent's rule."""
    select = host if callable(host) else (lambda st: host_list(host, st) if host is not None else None)
    root = np.asarray(root)
    d = root.shape[1]
    w = [int(v) for v in weights]
    dist = int(dist)
    if not (0 <= dist < len(root) and root[dist, 0] >= 0):
        dist = -1
    track = True
    if reduce_root:
        track = dist >= 0
        pts, dist = tracked_newton(root, dist)
    else:
        pts = live(root)
        dist = int((root[:dist, 0] >= 0).sum()) if dist >= 0 else -1
    outcome = NO_CONTRIBUTION if track and dist < 0 else (ENDED if len(pts) < 2 else RUNNING)
    out_c, out_a, history = [], [], []
    for t in range(max_steps):
        if outcome != RUNNING:
            break
        forced = classes[t] if classes is not None and t < len(classes) else -1
        coords = subset_of_class(int(forced), d) if forced >= 0 else select(pts)
        if coords is None:
            outcome = NO_MOVE
            break
        coords = sorted(int(c) for c in coords)
        a = int(axes[t]) if axes is not None and t < len(axes) else -1
        if a >= 0:
            if a not in coords:
                outcome = NO_MOVE
                break
        else:
            a = morin_axis(coords, w, tie)
            if a is None:
                raise ValueError("a random tie needs its axis fed in")
        w = next_weights(coords, w, a, weight_rule)
        shifted_max = int(pts[:, coords].sum(1).max())
        pts, nd, _ = morin_child(pts, coords, a, dist if track else 0)
        out_c.append(class_id(coords, d)), out_a.append(a)
        if track:
            dist = -1 if nd is None else nd
        history.append((pts, list(w), dist))
        if track and nd is None:
            outcome = NO_CONTRIBUTION
        elif len(pts) < 2:
            outcome = ENDED
        if shifted_max >= limit:
            outcome = INEXACT
    untouched = not reduce_root and not out_c
    return Played(pts, w, dist if track else -1, len(out_c), outcome, out_c, out_a, history, untouched)


def padded(state, m, dtype=np.int64):
    """live rows -> [m, d] with padding -1"""
    state = np.asarray(state)
    out = np.full((m, state.shape[1]), -1, dtype=dtype)
    out[: len(state)] = state
    return out


def final_state(root, played, dtype=np.int64):
    """the [m, d] array the operator leaves for a root: the root itself where the game was copied through"""
    root = np.asarray(root)
    return root.astype(dtype) if played.untouched else padded(played.state, len(root), dtype)


# ---- the fixture tests/golden/morin_game.npz (make_morin_game_golden.py) ---------------------------------------------

Recorded = namedtuple("Recorded", "name host seed root dist root_state root_dist lists axes states weights dists "
                                  "raised stopped")
# one reference game: lists / axes / states / weights / dists per move; stopped: 0 still running when the recording
# ended, 1 state.ended, 2 no contribution (at the root when there are no moves and root_dist is -1)


def load_games(npz):
    """the games of the fixture as Recorded tuples of numpy arrays"""
    hosts = [str(h) for h in npz["hosts"]]
    flat = {k: npz[k].astype(np.int64) for k in ("roots", "root_states", "states")}
    at = {k: 0 for k in flat}

    def take(key, rows, d):
        out = flat[key][at[key]: at[key] + rows * d].reshape(rows, d)
        at[key] += rows * d
        return out

    games, s = [], 0
    for name, row in zip(npz["names"], npz["meta"].tolist()):
        m, d, dist, seed, host, raised, root_n, root_dist, moves, stopped = row
        root, root_state = take("roots", m, d), take("root_states", root_n, d)
        counts = npz["counts"][s: s + moves].tolist()
        games.append(Recorded(str(name), hosts[host], seed, root, dist, root_state, root_dist,
                              [[c for c in r if c >= 0] for r in npz["lists"][s: s + moves].tolist()],
                              npz["axes"][s: s + moves].tolist(), [take("states", c, d) for c in counts],
                              [r[:d] for r in npz["weights"][s: s + moves].tolist()],
                              npz["dists"][s: s + moves].tolist(), raised, stopped))
        s += moves
    assert s == len(npz["axes"]) and all(at[k] == len(flat[k]) for k in flat)
    return games


def forced_moves(game):
    """(classes, axes) that replay a recorded game: every class forced, the axis only where the weights tie"""
    d = game.root.shape[1]
    w, classes, axes = [1] * d, [], []
    for coords, a, w2 in zip(game.lists, game.axes, game.weights):
        classes.append(class_id(coords, d))
        axes.append(a if morin_axis(coords, w, "random") is None else -1)
        w = w2
    return classes, axes
