"""The rules of one greedy move of the DQN evaluation (include/hironaka_hip_dqn_move.h; the reference's
trainer/fused_game.py:104-163 with exploration off and trainer/trainer.py:302-325), restated in numpy on top of
oracle.np_oracle in torch semantics.  tests/test_dqn_move_rules.py pins the argmax rules to torch on the CPU and the
whole of `evaluate` to a recording of the reference's Trainer; the GPU kernels and the CPU build of the lane body are
compared with `host_pick`, `agent_move` and `evaluate` bit for bit."""
import numpy as np

from oracle import np_oracle as O
from oracle.search_oracle import _first_argmax_nan_wins


def num_classes(d):
    return 2 ** d - d - 1


def host_pick(q, d, dtype=np.float32):
    """the host's class (the first maximum of the row; the first NaN wins) and its subset as 0/1 values of `dtype`"""
    cls = _first_argmax_nan_wins(np.asarray(q)[:, : num_classes(d)])
    return cls, O.decode_class(cls, d).astype(dtype)


def clamp_class(cls, d):
    return np.clip(np.asarray(cls, np.int64), 0, num_classes(d) - 1)


def agent_axis(q, coords, masked=True):
    """fused_game.py:143-146 in q's dtype, every operation an array operation of that type: the argmax of
    q * mask + (1 - mask) * finfo.min when `masked`, of q itself otherwise"""
    q = np.asarray(q)
    if masked:
        dt = q.dtype.type
        mask = np.asarray(coords).astype(q.dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            q = q * mask + (dt(1) - mask) * np.finfo(q.dtype).min
    return _first_argmax_nan_wins(q)


def features(points):
    """TensorPoints.get_features: the rows by coordinate 0, descending, ties in row order"""
    order = np.argsort(-points[:, :, 0], axis=1, kind="stable")
    return np.take_along_axis(points, order[:, :, None], axis=1)


def agent_move(points, q, cls, *, masked=True, rescale=True, padding_value=-1.0):
    """hk_dqn_agent_move on a batch: points [B, m, d], q [B, d], cls [B].  Returns the new points, axis (int32), the
    features of the new points, done, prev_done"""
    points = np.asarray(points)
    b, m, d = points.shape
    coords = O.decode_class(clamp_class(cls, d), d)
    axis = agent_axis(q, coords, masked)
    prev_done = O.get_dones(points)
    new = O.step(points, coords, axis, padding_value=padding_value, sem="torch", do_reposition=False,
                 do_rescale=rescale, noop_if_invalid=True, ignore_ended=True)
    return new, axis.astype(np.int32), features(new), O.get_dones(new), prev_done


def evaluate(points, host_q, agent_q, max_steps, *, masked=True, scale_observation=True, count_for=None,
             padding_value=-1.0):
    """FusedGame.evaluate: host_q(features [B, m, d]) -> [B, classes], agent_q(features, coords [B, d]) -> [B, d].
    Returns lengths int32 [B], initial_done bool [B], counts int32 or None, rho (float, NaN for 0 / 0), the final
    points"""
    points = np.array(points)
    b, m, d = points.shape
    lengths = np.zeros(b, np.int32)
    initial_done = O.get_dones(points)
    counts = None
    if count_for is not None:
        counts = np.zeros(num_classes(d) if count_for == "host" else d, np.int32)
    feats = features(points)
    for _ in range(max_steps):
        cls, coords = host_pick(host_q(feats), d, points.dtype)
        points, axis, feats, _, prev_done = agent_move(points, agent_q(feats, coords), cls, masked=masked,
                                                       rescale=scale_observation, padding_value=padding_value)
        lengths += ~prev_done
        if count_for is not None:
            np.add.at(counts, (cls if count_for == "host" else axis)[~prev_done], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.float32(b - initial_done.sum()) / np.float32(lengths.sum())
    return lengths, initial_done, counts, rho, points
