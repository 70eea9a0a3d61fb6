"""The plain Hironaka game played forward, restated in plain numpy: what hk_game_play / hironaka_amd.ops.game_play define
as their outputs (hironaka/game.py:84-119 GameHironaka, hironaka/agent.py:85-98 RandomAgent / ChooseFirstAgent), and the
bookkeeping of hironaka/validator/hironaka_validator.py:30-48 playoff as a literal loop over a list of reset states.
The hosts are tests/search_rules.py's.  Nothing here comes from hironaka_amd: test_play_rules.py pins this module to the
fixture made by running the reference (tests/golden/make_play_golden.py), and the GPU tests compare the kernel with it.

Everything runs in the dtype it is given: int64 (exact; no rescale), float32 or float64 (every sum in ascending
coordinate order, the rescale a division by the maximum).  A state is an [m, d] array in that dtype whose rows with
coordinate 0 >= 0 are the points, padding -1: a root as given, holes anywhere; after a reduction or a move, the points
sorted descending and packed to the front."""
from collections import namedtuple

import numpy as np

from search_rules import class_id, host_list, newton

RUNNING, ENDED, NO_MOVE, INEXACT, VALUE_LIMIT = 0, 1, 3, 4, 5  # HK_PLAY_*
LIMITS = {np.dtype(np.float32): 2 ** 24, np.dtype(np.float64): 2 ** 53, np.dtype(np.int64): 2 ** 53}

Played = namedtuple("Played", "state length outcome classes axes lists history")
# state: the final [m, d] state; classes / axes / lists: the moves played (lists: the host's list in its own order);
# history: the [m, d] state after every move


def points_of(state):
    state = np.asarray(state)
    return state[state[:, 0] >= 0]


def padded(pts, m):
    out = np.full((m, pts.shape[1]), -1, dtype=pts.dtype)
    out[: len(pts)] = pts
    return out


def reduce(state):
    """Newton, sorted and packed (get_newton_polytope on ListPoints)"""
    pts = points_of(state)
    return padded(newton(pts) if len(pts) else pts, len(state))


def rescale(state):
    """scale_points (src/_fn.py:133-153): x / max over the points, skipped when max is 0; rows stay where they are"""
    state = np.array(state)
    if state.dtype.kind != "f":
        raise TypeError("the rescale needs a float dtype")
    on = state[:, 0] >= 0
    if on.any() and state[on].max() != 0:
        state[on] = state[on] / state[on].max()
    return state


def exceeds(state, threshold):
    """ListPoints.exceed_threshold (core/list_points.py:60-70)"""
    return bool((points_of(state).astype(np.float64) > threshold).any())


def subset_of_class(cls, d):
    masks = [v for v in range(1 << d) if bin(v).count("1") >= 2]
    return [k for k in range(d) if (masks[cls] >> k) & 1] if 0 <= cls < len(masks) else None


AGENTS = {"choose_first": lambda coords, t: min(coords), "choose_last": lambda coords, t: max(coords)}


def random_agent(rng):
    """RandomAgent with draws from a numpy Generator (the kernel's come from Philox: its axes are fed in instead)"""
    return lambda coords, t: sorted(coords)[int(rng.integers(len(coords)))]


def move(state, coords, a, reposition=False, rescaled=False):
    """(the state after the agent's axis `a` on the host's `coords`, whether a shifted coordinate left the exact
    integers): shift, [reposition], Newton sorted and packed, [rescale]"""
    pts = points_of(state).copy()
    total = pts[:, min(coords)].copy()
    for k in sorted(coords)[1:]:
        total = total + pts[:, k]
    pts[:, a] = total
    inexact = bool((total >= LIMITS[pts.dtype]).any())
    if reposition:
        pts = pts - pts.min(0)
    new = padded(newton(pts), len(state))
    return (rescale(new) if rescaled else new), inexact


def play(root, host, agent, max_steps, classes=None, axes=None, reposition=False, rescaled=False, reduce_root=False,
         rescale_root=False, value_threshold=None, dtype=np.int64):
    """host: a name of search_rules.HOSTS, select(state) -> the host's list, or None (every class forced).  agent: a
    key of AGENTS or pick(coords, t) -> axis.  classes / axes: per move, an entry < 0 (or a missing one) leaves the move
    to the host / the agent."""
    select = host if callable(host) else (lambda st: host_list(host, st) if host is not None else None)
    pick = agent if callable(agent) else AGENTS[agent]
    state = np.asarray(root).astype(dtype)
    d = state.shape[1]
    if reduce_root:
        state = reduce(state)
    if rescale_root:
        state = rescale(state)
    outcome = ENDED if len(points_of(state)) < 2 else RUNNING
    out_c, out_a, lists, history = [], [], [], []
    for t in range(max_steps):
        if outcome != RUNNING:
            break
        forced = classes[t] if classes is not None and t < len(classes) else -1
        coords = subset_of_class(int(forced), d) if forced >= 0 else select(state)
        if coords is None:
            outcome = NO_MOVE
            break
        coords = [int(c) for c in coords]
        a = int(axes[t]) if axes is not None and t < len(axes) else -1
        if a >= 0:
            if a not in coords:
                outcome = NO_MOVE
                break
        else:
            a = int(pick(coords, t))
        state, inexact = move(state, coords, a, reposition, rescaled)
        out_c.append(class_id(coords, d)), out_a.append(a), lists.append(coords), history.append(state)
        if len(points_of(state)) < 2:
            outcome = ENDED
        elif value_threshold is not None and value_threshold > 0 and exceeds(state, value_threshold):
            outcome = VALUE_LIMIT
        if inexact and not rescaled:
            outcome = INEXACT
    return Played(state, len(out_c), outcome, out_c, out_a, lists, history)


def playoff(reset_states, num_steps, host, agent, step_threshold, scale_observation=True, value_threshold=None,
            axes=None, dtype=np.float64):
    """HironakaValidator.playoff (hironaka_validator.py:30-48) as the loop it is, with `reset` handing out reset_states
    in order (raw states, rescaled here when scale_observation is set).  axes: the agent's axes of every step in order,
    fed in instead of `agent` (a recorded RandomAgent).  Returns (len_history, the reset states used, the last
    one being that of the closing reset)."""
    pick = agent if callable(agent) else AGENTS[agent]
    feed = None if axes is None else iter(axes)
    handed = 0

    def reset():
        nonlocal handed
        st = np.asarray(reset_states[handed]).astype(dtype)
        handed += 1
        return rescale(st) if scale_observation else st

    state, counter, history = reset(), 0, []
    for _ in range(num_steps):
        exceed = value_threshold is not None and exceeds(state, value_threshold)
        coords = host_list(host, state)
        fed = None if feed is None else next(feed)
        going = False
        if coords is not None:
            a = int(pick(coords, counter)) if fed is None else int(fed)
            assert a in coords
            state, _ = move(state, coords, a, False, scale_observation)
            going = len(points_of(state)) >= 2
        if going and counter < step_threshold and not exceed:
            counter += 1
        else:
            history.append(counter)
            counter = 0
            state = reset()
    history.append(counter)
    return history, handed + 1


# ---- the fixture tests/golden/play_game.npz (make_play_golden.py) ----------------------------------------------------

Recorded = namedtuple("Recorded", "name host agent scale seed root root_state lists axes states stopped raised")
# one reference game: root as given (ints), root_state after Game.__init__ (Newton, then the rescale when scale is
# set), then per move the host's list, the agent's axis and the state; stopped: 1 when state.ended, 0 when the recording
# ended first; raised: the reference raised at the move after the recorded ones

Playoff = namedtuple("Playoff", "name host agent scale value_threshold step_threshold num_steps states len_history axes")


def load_games(npz):
    hosts, agents = [str(h) for h in npz["hosts"]], [str(a) for a in npz["agents"]]
    flat = {"roots": npz["roots"], "int_states": npz["int_states"], "float_states": npz["float_states"]}
    at = {k: 0 for k in flat}

    def take(key, rows, d):
        out = flat[key][at[key]: at[key] + rows * d].reshape(rows, d)
        at[key] += rows * d
        return out

    games, s = [], 0
    for name, row in zip(npz["names"], npz["meta"].tolist()):
        m, d, host, agent, scale, seed, root_n, moves, stopped, raised = row
        key = "float_states" if scale else "int_states"
        root = take("roots", m, d).astype(np.int64)
        root_state = take(key, root_n, d)
        counts = npz["counts"][s: s + moves].tolist()
        games.append(Recorded(str(name), hosts[host], agents[agent], bool(scale), seed, root, root_state,
                              [[c for c in r if c >= 0] for r in npz["lists"][s: s + moves].tolist()],
                              npz["axes"][s: s + moves].tolist(), [take(key, c, d) for c in counts], stopped, raised))
        s += moves
    assert s == len(npz["axes"]) and all(at[k] == len(flat[k]) for k in flat)
    return games


def load_playoffs(npz):
    hosts, agents = [str(h) for h in npz["hosts"]], [str(a) for a in npz["agents"]]
    out, s, h, x = [], 0, 0, 0
    for name, row, thr in zip(npz["po_names"], npz["po_meta"].tolist(), npz["po_thresholds"].tolist()):
        host, agent, scale, step_threshold, num_steps, m, d, nstates, nhist, naxes = row
        out.append(Playoff(str(name), hosts[host], agents[agent], bool(scale), None if thr <= 0 else thr, step_threshold,
                           num_steps, npz["po_states"][s: s + nstates * m * d].reshape(nstates, m, d).astype(np.int64),
                           npz["po_history"][h: h + nhist].tolist(), npz["po_axes"][x: x + naxes].tolist()))
        s, h, x = s + nstates * m * d, h + nhist, x + naxes
    return out
