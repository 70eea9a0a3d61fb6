"""
Generate tests/golden/dqn_fit.npz by RUNNING the reference's own DQN fit step on torch CPU: `polyak_update`
(hironaka/src/_borrowed_fn.py) and `DQNTrainer._fit_network` / `_update_target_net`
(hironaka/trainer/dqn_trainer/dqn_trainer.py), called unbound on a stub `self`.  The files are loaded one by one as
make_golden.py loads the rest; `hironaka.trainer.trainer`, whose imports (yaml, tensorboard, the jax-side packages) are
not installed and whose `Trainer` only serves as a base class that neither method touches, is a stub module with an
empty `Trainer`.  Runs only where the reference checkout exists; the .npz is what travels, and it holds data only.

One case per (B, A) in {1, 5, 259} x {1, 3, 11, 120}, float32 and float64 alternating so that either dtype meets every B
and every A; the nets (tests/dqn_rules.py build_net: two and three nn.Linear layers, and one with a BatchNorm1d, the
latter for B > 1 only: it trains on batch statistics) cycle with the cases, as do the dones (all false, all true, mixed),
gamma and max_grad_norm; rewards are drawn from {-1, 0, 1}; plain SGD.  The last layer of both nets is scaled so that the
TD errors x lie on both sides of 1 and one is well above it (a case with B > 1 is redrawn, nets and batch, from the next
seed until they do; the B = 1 cases lie on either side between them, which main() asserts).

What is recorded is what the reference computed, caught where it passes through torch: forward hooks on the two nets
(next_q, current_q and, by a tensor hook, dL/dcurrent_q), tensor hooks on the parameters (their gradients as backward
produced them, before clip_grad_norm_), and the arguments of nn.functional.smooth_l1_loss (the gathered Q-values and the
target).  Layout, for case k (the case_* arrays describe the cases; names are those of named_parameters / named_buffers):
    c{k}_obs, _actions, _rewards, _dones, _next_obs          the batch the stub buffer served
    c{k}_q0_{name}, c{k}_t0_{name}                           both nets before the step
    c{k}_next_q, _current_q, _target, _loss, _dq             of the step
    c{k}_grad_{name}                                         parameter gradients before clipping
    c{k}_q1_{name}, c{k}_t1_{name}                           both nets after the step (the target net's BatchNorm
                                                             statistics moved in its forward pass)
    c{k}_tau{j}_{name}                                       the target net after _update_target_net(q1, t1, TAUS[j])

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dqn_golden.py
"""
import copy
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dqn_rules as R  # noqa: E402
from make_golden import OUT, REF, _load, _pkg  # noqa: E402

BATCHES, ACTIONS = (1, 5, 259), (1, 3, 11, 120)
DONES = ("none", "all", "mixed")
GAMMAS, GRAD_NORMS, LR = (0.99, 0.9), (0.5, 10.0), 0.05


def load_reference():
    _pkg("hironaka")
    src = _pkg("hironaka.src")
    trainer = _pkg("hironaka.trainer")
    borrowed = _load("hironaka.src._borrowed_fn", "hironaka/src/_borrowed_fn.py")
    src.polyak_update = borrowed.polyak_update
    _load("hironaka.trainer.replay_buffer", "hironaka/trainer/replay_buffer.py")
    _load("hironaka.trainer.timer", "hironaka/trainer/timer.py")
    base = types.ModuleType("hironaka.trainer.trainer")
    base.Trainer = type("Trainer", (), {})
    sys.modules["hironaka.trainer.trainer"] = base
    trainer.trainer = base
    _pkg("hironaka.trainer.dqn_trainer")
    dqn = _load("hironaka.trainer.dqn_trainer.dqn_trainer", "hironaka/trainer/dqn_trainer/dqn_trainer.py")
    return dqn.DQNTrainer, borrowed.polyak_update


class StubBuffer:
    def __init__(self, batch):
        self.batch = batch

    def sample(self, batch_size, device=None, clone=True):
        assert batch_size == self.batch[1].shape[0]
        return self.batch


def numpy_state(net):
    return {k: v.detach().numpy().copy() for k, v in R.net_state(net).items()}


def run_case(DQNTrainer, rng, seed, k, B, A, dtype, kind, dones_mode, gamma, max_grad_norm, rec):
    torch.manual_seed(seed)
    q_net, q_net_target = R.build_net(kind, A, dtype), R.build_net(kind, A, dtype)
    with torch.no_grad():  # spread the Q-values: TD errors on both sides of 1, one well above
        for net, scale in ((q_net, 6.0), (q_net_target, 3.0)):
            net[-1].weight.mul_(scale)
            net[-1].bias.mul_(scale)
    ndt = np.float32 if dtype == torch.float32 else np.float64
    obs, next_obs = (rng.standard_normal((B, R.OBS_DIM)).astype(ndt) for _ in range(2))
    actions = rng.integers(0, A, (B, 1)).astype(np.int32)
    actions[0, 0], actions[-1, 0] = 0, A - 1
    rewards = rng.integers(-1, 2, (B, 1)).astype(np.float32)
    dones = {"none": np.zeros((B, 1), bool), "all": np.ones((B, 1), bool),
             "mixed": rng.integers(0, 2, (B, 1)).astype(bool)}[dones_mode]
    batch = tuple(torch.from_numpy(x.copy()) for x in (obs, actions, rewards, dones, next_obs))
    for name, x in zip(("obs", "actions", "rewards", "dones", "next_obs"), (obs, actions, rewards, dones, next_obs)):
        rec[f"c{k}_{name}"] = x
    for tag, net in (("q0", q_net), ("t0", q_net_target)):
        for name, v in numpy_state(net).items():
            rec[f"c{k}_{tag}_{name}"] = v
    caught = {}

    def on_target(module, args, output):
        caught["next_q"] = output.detach().numpy().copy()

    def on_q(module, args, output):
        caught["current_q"] = output.detach().numpy().copy()
        output.register_hook(lambda g: caught.__setitem__("dq", g.numpy().copy()))

    handles = [q_net_target.register_forward_hook(on_target), q_net.register_forward_hook(on_q)]
    for name, p in q_net.named_parameters():
        handles.append(p.register_hook(lambda g, name=name: caught.__setitem__("grad_" + name, g.numpy().copy())))
    huber = nn.functional.smooth_l1_loss

    def recording_huber(current, target, *args, **kw):
        caught["picked"], caught["target"] = current.detach().numpy().copy(), target.detach().numpy().copy()
        return huber(current, target, *args, **kw)

    stub = types.SimpleNamespace(time_log={}, log_time=False, use_cuda=False, device=torch.device("cpu"),
                                 max_grad_norm=max_grad_norm, use_tensorboard=False, total_num_steps=0,
                                 layerwise_logging=False)
    optimizer = torch.optim.SGD(q_net.parameters(), lr=LR)
    nn.functional.smooth_l1_loss = recording_huber
    try:
        loss = DQNTrainer._fit_network(stub, q_net, q_net_target, optimizer, StubBuffer(batch), B, gamma)
    finally:
        nn.functional.smooth_l1_loss = huber
        for h in handles:
            h.remove()
    assert caught["target"].shape == (B, 1) and caught["target"].dtype == ndt and caught["dq"].shape == (B, A)
    x = (caught["picked"] - caught["target"]).reshape(-1)
    for name in ("next_q", "current_q", "dq"):
        rec[f"c{k}_{name}"] = caught[name]
    rec[f"c{k}_target"] = caught["target"].reshape(-1)
    rec[f"c{k}_loss"] = loss.detach().numpy().copy()
    for name, _ in q_net.named_parameters():
        rec[f"c{k}_grad_{name}"] = caught["grad_" + name]
    for tag, net in (("q1", q_net), ("t1", q_net_target)):
        for name, v in numpy_state(net).items():
            rec[f"c{k}_{tag}_{name}"] = v
    for j, tau in enumerate(R.TAUS):
        target = copy.deepcopy(q_net_target)
        DQNTrainer._update_target_net(q_net, target, tau)
        for name, v in numpy_state(target).items():
            rec[f"c{k}_tau{j}_{name}"] = v
    return np.abs(x)


def main():
    if not os.path.isdir(REF):
        raise SystemExit(f"{REF} not present: fixtures can only be regenerated next to the reference")
    DQNTrainer, _ = load_reference()
    rec, meta, single = {}, {n: [] for n in ("B", "A", "f64", "net", "dones", "gamma", "max_grad_norm")}, []
    k = 0
    for bi, B in enumerate(BATCHES):
        for ai, A in enumerate(ACTIONS):
            f64 = (bi + ai + 1) % 2  # the largest case, (259, 120), in float32: the fixture's size
            kind = R.NET_KINDS[k % 3] if B > 1 else R.NET_KINDS[k % 2]
            dones_mode, gamma, norm = DONES[(k + bi) % 3], GAMMAS[k % 2], GRAD_NORMS[(k // 2) % 2]
            # redraw a case (nets and batch) until its TD errors lie where they are wanted
            for attempt in range(200):
                mine = {}
                ax = run_case(DQNTrainer, np.random.default_rng([20261, k, attempt]), 1000 * attempt + k, k, B, A,
                              torch.float64 if f64 else torch.float32, kind, dones_mode, gamma, norm, mine)
                if B == 1 or (ax.min() < 0.9 and ax.max() > 3.0 and (ax > 1.1).sum() >= 2):
                    break
            else:
                raise AssertionError((k, B, A))
            rec.update(mine)
            if B == 1:
                single.append(float(ax[0]))
            for n, v in zip(meta, (B, A, f64, R.NET_KINDS.index(kind), DONES.index(dones_mode), gamma, norm)):
                meta[n].append(v)
            k += 1
    assert min(single) < 1.0 < max(single), single
    for n, v in meta.items():
        rec[f"case_{n}"] = np.array(v, dtype=np.float64 if n in ("gamma", "max_grad_norm") else np.int64)
    rec["lr"] = np.array(LR)
    for f64 in (0, 1):  # either dtype meets every B, every A, every net and every kind of dones
        mine = [i for i in range(k) if meta["f64"][i] == f64]
        for n, full in (("B", BATCHES), ("A", ACTIONS), ("net", range(3)), ("dones", range(3))):
            assert {meta[n][i] for i in mine} == set(full), (f64, n)
    path = os.path.join(OUT, "dqn_fit.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {k} cases, {len(rec)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
