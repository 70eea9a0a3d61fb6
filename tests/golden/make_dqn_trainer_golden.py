"""
Generate tests/golden/dqn_trainer.npz by RUNNING the reference's own `Trainer.get_rho_for_pair`, `Trainer.count_actions`
(hironaka/trainer/trainer.py:302-347), schedulers (trainer/scheduler.py) and dummy player modules
(trainer/player_modules/modules.py) on torch CPU.  The files are loaded one by one as make_golden.py loads the rest;
`torch.utils.tensorboard`, which is not installed, is a stub module that the run never touches (use_tensorboard: false).
Runs only where the reference checkout exists; the .npz is what travels, and it holds data only.

The players are make_golden.py's row-permutation-invariant SetNet with integer weights in [-4, 4] and distinct dyadic
biases; scale_observation is off, max_value <= 5, max_steps <= 10.  So every coordinate stays an integer and every sum a
network forms is exact in float32 whatever the order of the rows -- the reference's unstable argsort cannot matter --
which `main` asserts on every state the games visit (the largest sum needs fewer than 24 bits, the biases' 6 fractional
bits included).  The start states are recorded as `_generate_random_points` hands them to the play (after the Newton
polytope) and served again to `count_actions`, so rho, the lengths and the counts belong to the same games.

Layout, per shape tag t = m{m}_d{d}:
    {t}/start [B, m, d]; {t}/host_w, host_b, agent_w, agent_v, agent_b; {t}/max_steps
    {t}/rho (float32), {t}/lengths int32 [B] (the move at which each game ended: 0 at the start, max_steps never),
    {t}/initial_done, {t}/host_counts, {t}/agent_counts (int64)
sched/{name}_{steps}: the scheduler values at SCHED_STEPS (float64); sched/params the constructor arguments
dummy/...: the modules' outputs on the recorded observations

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dqn_trainer_golden.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference tree

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, SetNet, _load, _pkg, load_reference  # noqa: E402

SHAPES = ((5, 2, 5, 3), (20, 3, 5, 10), (8, 4, 4, 8))  # m, d, max_value, max_steps
GAMES = 64
SCHED_STEPS = (0, 1, 10, 1000)
SCHED_PARAMS = dict(value=1e-8, initial=1e-3, rate=0.996, inverse_rate=0.5)


def load_trainer():
    ref = load_reference()
    sys.modules["hironaka.src"].HostActionEncoder = ref.fn.HostActionEncoder
    try:
        import torch.utils.tensorboard  # noqa: F401
    except ImportError:
        stub = types.ModuleType("torch.utils.tensorboard")
        stub.SummaryWriter = type("SummaryWriter", (), {})
        sys.modules["torch.utils.tensorboard"] = stub
    _pkg("hironaka.trainer")
    for name in ("timer", "fused_game", "nets", "replay_buffer", "scheduler"):
        _load(f"hironaka.trainer.{name}", f"hironaka/trainer/{name}.py")
    _pkg("hironaka.trainer.player_modules")
    modules = _load("hironaka.trainer.player_modules.modules", "hironaka/trainer/player_modules/modules.py")
    for k in dir(modules):
        if k.endswith("Module"):
            setattr(sys.modules["hironaka.trainer.player_modules"], k, getattr(modules, k))
    trainer = _load("hironaka.trainer.trainer", "hironaka/trainer/trainer.py")
    return ref, trainer, sys.modules["hironaka.trainer.scheduler"], modules, sys.modules["hironaka.trainer.fused_game"]


def config(m, d, max_value):
    role = dict(batch_size=2, initial_rollout_size=2, max_rollout_step=2, er=0.0, net_arch=[4],
                optim=dict(name="adam", args=dict(lr=1e-3)))
    return dict(use_tensorboard=False, layerwise_logging=False, log_time=False, use_cuda=False, scale_observation=False,
                version_string="golden", dimension=d, max_num_points=m, max_value=max_value,
                host=dict(role), agent=dict(role), replay_buffer=dict(type="base", buffer_size=10, use_cuda=False,
                                                                     deactivate=True))


def main():
    if not os.path.isdir(REF):
        sys.exit(f"{REF} not found: the fixture is generated where the reference checkout exists")
    ref, trainer_mod, sched, modules, fg = load_trainer()
    Concrete = type("Concrete", (trainer_mod.Trainer,), {"_train": lambda self, *a, **k: None})
    rng = np.random.default_rng(20260321)
    rec = {}
    for m, d, max_value, max_steps in SHAPES:
        tag = f"m{m}_d{d}"
        n_cls = 2 ** d - d - 1
        hw = rng.integers(-4, 5, (d, n_cls)).astype(np.float32)
        hb = (rng.permutation(n_cls) / 64.0).astype(np.float32)
        aw = rng.integers(-4, 5, (d, d)).astype(np.float32)
        av = rng.integers(-4, 5, (d, d)).astype(np.float32)
        ab = (rng.permutation(d) / 64.0).astype(np.float32)
        t = Concrete(config(m, d, max_value), host_net=SetNet(hw, hb), agent_net=SetNet(aw, ab, av))
        t.set_training(False)
        torch.manual_seed(20260321 + m)
        start = t._generate_random_points(GAMES, t.device).points.clone()
        start[0, 1:] = -1.0  # a game that is over at the start
        t._generate_random_points = lambda samples, device: ref.TensorPoints(start.clone(), device=device)

        seen = {"ended": [], "largest": float(start.abs().max())}
        agent_move = fg.FusedGame.agent_move

        def recording(self, points, *args, **kwargs):
            out = agent_move(self, points, *args, **kwargs)
            seen["ended"].append(points.ended_batch_in_tensor.clone().numpy())
            seen["largest"] = max(seen["largest"], float(points.points.abs().max()))
            return out

        fg.FusedGame.agent_move = recording
        try:
            rho = t.get_rho_for_pair(t.host_net, t.agent_net, GAMES, max_steps)
        finally:
            fg.FusedGame.agent_move = agent_move
        ended = np.stack(seen["ended"])  # [max_steps, B]
        initial_done = (start[:, :, 0] >= 0).sum(1).numpy() < 2
        lengths = np.where(ended.any(0), ended.argmax(0) + 1, max_steps).astype(np.int32)
        lengths[initial_done] = 0
        assert np.float32(GAMES - initial_done.sum()) / np.float32(lengths.sum()) == rho.numpy()
        host_counts = t.count_actions("host", GAMES, max_steps, er=0.0).numpy()
        agent_counts = t.count_actions("agent", GAMES, max_steps, er=0.0).numpy()
        assert host_counts.sum() == agent_counts.sum() == lengths.sum()
        # the exactness bound: the largest sum a network forms, in units of the biases' 1/64
        bound = (seen["largest"] * m * d * 4 + d * 4 + 1) * 64
        print(tag, "rho", float(rho), "largest", seen["largest"], "bits", np.log2(bound), "lengths", np.bincount(lengths))
        assert bound < 2 ** 24, (tag, bound)
        assert 0 < initial_done.sum() < GAMES and (lengths == max_steps).any() and (0 < lengths).any()
        rec.update({f"{tag}/start": start.numpy(), f"{tag}/host_w": hw, f"{tag}/host_b": hb, f"{tag}/agent_w": aw,
                    f"{tag}/agent_v": av, f"{tag}/agent_b": ab, f"{tag}/max_steps": np.int32(max_steps),
                    f"{tag}/rho": rho.numpy(), f"{tag}/lengths": lengths, f"{tag}/initial_done": initial_done,
                    f"{tag}/host_counts": host_counts, f"{tag}/agent_counts": agent_counts})

    p = SCHED_PARAMS
    schedulers = {
        "constant": sched.ConstantScheduler(p["value"]),
        "exponential_lr": sched.ExponentialLRScheduler(p["value"], mode="exponential", initial_lr=p["initial"], rate=p["rate"]),
        "inverse_lr": sched.InverseLRScheduler(p["value"], mode="inverse", initial_lr=p["initial"], rate=p["inverse_rate"]),
        "exponential_er": sched.ExponentialERScheduler(0.2, mode="exponential", initial_er=0.5, rate=p["rate"]),
    }
    rec["sched/params"] = np.array([p["value"], p["initial"], p["rate"], p["inverse_rate"], 0.2, 0.5], np.float64)
    rec["sched/steps"] = np.array(SCHED_STEPS, np.int64)
    for name, s in schedulers.items():
        rec[f"sched/{name}"] = np.array([s(step) for step in SCHED_STEPS], np.float64)

    d, m, b = 3, 20, 16
    coords = torch.tensor(np.array([[(v >> j) & 1 for j in range(d)] for v in (3, 5, 6, 7)] * 4, np.float32))
    feats = torch.tensor(rng.integers(0, 5, (b, m, d)).astype(np.float32))
    rec["dummy/coords"], rec["dummy/points"] = coords.numpy(), feats.numpy()
    dev = torch.device("cpu")
    obs = {"points": feats, "coords": coords}
    rec["dummy/choose_first"] = modules.ChooseFirstAgentModule(d, m, dev)(obs).numpy()
    rec["dummy/choose_last"] = modules.ChooseLastAgentModule(d, m, dev)(obs).numpy()
    rec["dummy/all_coord"] = modules.AllCoordHostModule(d, m, dev)(feats).numpy()
    np.savez_compressed(os.path.join(OUT, "dqn_trainer.npz"), **rec)
    print(f"wrote dqn_trainer.npz ({len(rec)} arrays)")


if __name__ == "__main__":
    main()
