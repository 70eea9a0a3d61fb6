"""Dev probe: the glue around the DQN trainers' roll-out move -- getting a step's experiences into the replay buffer and
a training batch out of it -- the parent's way against ReplayBuffer / FusedGame.collect, at (20,3) x 65 536 games,
float32, capacity 2^20.  HIP events around warmed-up work, the median of repeated runs, the two ways alternating.

  (a) FusedGame.step, then its outputs assigned slice by slice into preallocated ring tensors, the position kept on
      the host: the reference's ReplayBuffer.add restated with torch
  (b) FusedGame.collect into hironaka_amd.ReplayBuffer
  (c) hk_replay_push alone against one torch device-to-device copy of the same number of bytes
  (d) hk_replay_sample of 4 096 rows against the same gathers through torch indexing

Usage:  python scripts/probe_replay.py [--out profiles/replay_probe.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from hironaka_amd import ops
from hironaka_amd.core import HipPoints
from hironaka_amd.fused_game import FusedGame
from hironaka_amd.replay_buffer import ReplayBuffer
from probe_stages import timeit

B, M, D, CAPACITY, SAMPLE = 65536, 20, 3, 1 << 20, 4096


def eager(fn, iters=10):
    """us per call, no graph: (a) synchronises on every step by itself"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def alternate(fns, reps=7, **kw):
    """the median us per call of each fn, the fns taking turns"""
    for fn in fns:
        fn()  # warm-up
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            times[k].append(eager(fn, **kw))
    return [statistics.median(t) for t in times], [(min(t), max(t)) for t in times]


class TorchRing:
    """the reference's add on preallocated tensors: pos and full on the host, a slice copy per column (two at the wrap)"""

    def __init__(self, like: ReplayBuffer):
        self.cols = [torch.zeros_like(r) for r in like._rings()]
        self.split = like._split
        self.pos, self.full, self.size = 0, False, like.buffer_size

    def add(self, obs, action, reward, done, next_obs):
        rows = self.split(obs, "obs") + [action, reward, done] + self.split(next_obs, "next_obs")
        length = action.shape[0]
        for target, source in zip(self.cols, rows):
            if self.pos + length < self.size:
                target[self.pos:self.pos + length] = source
            else:
                target[self.pos:self.size] = source[:self.size - self.pos]
                target[:length + self.pos - self.size] = source[self.size - self.pos:]
        self.full = self.full or (length + self.pos) >= self.size
        self.pos = (length + self.pos) % self.size


def nets():
    flat = torch.nn.Flatten()

    class AgentNet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.body = torch.nn.Sequential(torch.nn.Linear(M * D + D, 256), torch.nn.ReLU(), torch.nn.Linear(256, D))

        def forward(self, x):
            return self.body(torch.cat([flat(x["points"]), x["coords"]], dim=1))

    host = torch.nn.Sequential(flat, torch.nn.Linear(M * D, 256), torch.nn.ReLU(), torch.nn.Linear(256, 2 ** D - D - 1))
    return host, AgentNet()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "replay_probe.json"))
    args = ap.parse_args()
    torch.manual_seed(0)
    result = {"games": B, "spec": [M, D], "dtype": "float32", "capacity": CAPACITY, "sample_rows": SAMPLE,
              "device": torch.cuda.get_device_name(0), "unit": "us per call, median of 7 runs"}
    # two moves in: some games have finished, so keep = ~done drops rows
    P = ops.generate_points(B, M, D, 20, seed=42)
    game = FusedGame(*nets(), log_time=False)
    pts = HipPoints(P.clone())
    pts.get_newton_polytope()
    for _ in range(2):
        game.step(pts, "host", exploration_rate=0.2)
    P = pts.points.clone()
    done = pts.ended_batch_in_tensor
    result["games_running"] = int((~done).sum())
    for role in ("host", "agent"):
        shape = (M, D) if role == "host" else {"points": (M, D), "coords": (D,)}
        buf = ReplayBuffer(shape, D, CAPACITY, "cuda")
        ring = TorchRing(buf)

        def parent():
            pts.points.copy_(P)
            ring.add(*game.step(pts, role, exploration_rate=0.2))

        def collect():
            pts.points.copy_(P)
            game.collect(pts, role, buf, exploration_rate=0.2)

        def step_only():
            pts.points.copy_(P)
            game.step(pts, role, exploration_rate=0.2)

        (ta, tb, ts), spread = alternate([parent, collect, step_only])
        result[f"collect_{role}"] = {"a_step_then_slice_add": ta, "b_collect": tb, "step_alone": ts,
                                     "a_over_b": ta / tb, "min_max": spread}
        print(f"{role}: (a) step + slice add {ta:.1f} us, (b) collect {tb:.1f} us, step alone {ts:.1f} us: "
              f"a / b = {ta / tb:.2f}", flush=True)
        # (c) the push alone, every row and keep = ~done, against one copy of the bytes of every row
        rings = buf._rings()
        rows = [torch.rand((B,) + tuple(r.shape[1:]), device="cuda").to(r.dtype) for r in rings]
        nbytes = sum(r[0].numel() * r.element_size() for r in rings) * B
        src = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        keep = ~done
        t_all = timeit(lambda: ops.replay_push(rings, rows, buf.cursor), iters=20, reps=10)
        t_keep = timeit(lambda: ops.replay_push(rings, rows, buf.cursor, keep=keep), iters=20, reps=10)
        t_copy = timeit(lambda: dst.copy_(src), iters=20, reps=10)
        result[f"push_{role}"] = {"bytes": nbytes, "c_push_all_rows": t_all, "c_push_keep": t_keep,
                                  "c_torch_copy_same_bytes": t_copy, "push_over_copy": t_all / t_copy,
                                  "push_GBps_read_plus_write": 2 * nbytes / t_all / 1e3}
        print(f"{role}: (c) push of {nbytes / 1e6:.1f} MB {t_all:.1f} us ({2 * nbytes / t_all / 1e3:.0f} GB/s r+w), "
              f"with keep {t_keep:.1f} us, torch copy {t_copy:.1f} us: push / copy = {t_all / t_copy:.2f}", flush=True)
        # (d) the sample against torch's index draw and gathers on the device
        out = [torch.zeros((SAMPLE,) + tuple(r.shape[1:]), dtype=r.dtype, device="cuda") for r in rings]

        def torch_sample():
            idx = torch.randint(CAPACITY, (SAMPLE,), device="cuda")
            return [r[idx] for r in rings]

        buf.cursor[1] = 1  # full: both draw from the whole ring
        t_hk = timeit(lambda: ops.replay_sample(rings, buf.cursor, SAMPLE, 3, out=out), iters=20, reps=10)
        t_torch = timeit(torch_sample, iters=20, reps=10)
        result[f"sample_{role}"] = {"d_hk_replay_sample": t_hk, "d_torch_randint_and_gathers": t_torch,
                                    "torch_over_hk": t_torch / t_hk}
        print(f"{role}: (d) sample of {SAMPLE} rows {t_hk:.1f} us, torch randint + {len(rings)} gathers "
              f"{t_torch:.1f} us", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
