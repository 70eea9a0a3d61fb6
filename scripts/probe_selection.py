"""Which kernels a table of requests launches: the launchable rows of tests/kernel_selection.hip through the C ABI.

    python scripts/probe_selection.py [--lib PATH]        one line per row: its label and the status it returned
    python scripts/probe_selection.py --names TRACE.csv   the hk:: kernels of a rocprofv3 kernel trace in dispatch order,
                                                          one line each: the name (template arguments included), the
                                                          grid and the workgroup size

Run the first form under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/probe_selection.py`
(a run of its own, no counters) once per library and compare the two --names lists and the two status lists: a
change of the host-side selection that keeps every launch shows an empty diff (profiles/selection_trace.txt is the
list of the committed code).  Batch 97 under the testing flags walks the ladders of every family; the crossover
batches of `pick` run at the default flags with short rollouts.
"""
import argparse
import csv
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_names(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        if "hk::" in r["Kernel_Name"]:
            print(f'{r["Kernel_Name"]} grid={r["Grid_Size_X"]} block={r["Workgroup_Size_X"]}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="another build of libhironaka_hip.so (default: the package's)")
    ap.add_argument("--names", metavar="TRACE.csv")
    args = ap.parse_args()
    if args.names:
        return kernel_names(args.names)

    import torch
    from hironaka_amd import _abi as A
    from hironaka_amd import _lib
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    L = _lib.lib()
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    TAKE = A.HK_STAGE_SHIFT | A.HK_STAGE_REPOSITION | A.HK_STAGE_NEWTON
    TORCH = A.HK_SEM_TORCH | A.HK_FLAG_AXIS_NOOP_IF_INVALID | A.HK_FLAG_IGNORE_ENDED
    ONE, TWO, FOUR = A.HK_FLAG_FORCE_ONE_LANE, A.HK_FLAG_FORCE_TWO_LANES, A.HK_FLAG_FORCE_FOUR_LANES
    TEAM, GENERIC = A.HK_FLAG_FORCE_TEAM, A.HK_FLAG_FORCE_GENERIC
    keep = []  # every buffer lives to the final synchronise

    def states(b, m, d, dtype=torch.float32, extra=0):
        g = torch.Generator().manual_seed(b * 1000 + m * 10 + d)
        p = torch.randint(0, 20, (b, m, d), generator=g).to(dtype)
        p[torch.rand((b, m), generator=g) < 0.25] = -1.0
        p[:, :2] = p[:, :2].clamp(min=0)  # at least two live rows
        rec = torch.full((b, m * d + extra), 0.0, dtype=dtype)
        rec[:, :m * d] = p.reshape(b, -1)
        keep.append(rec.to(dev))
        return keep[-1]

    def zeros(*shape, dtype=torch.float32):
        keep.append(torch.zeros(*shape, dtype=dtype, device=dev))
        return keep[-1]

    def report(label, status):
        print(f"{label} -> {status}", flush=True)

    # ---- hk_step / hk_step_features ------------------------------------------------------------------------------------
    ACTS = {"mask-f32/axis-i32": (A.HK_F32, A.HK_I32), "mask-f32/axis-i64": (A.HK_F32, A.HK_I64),
            "mask-f32/axis-f32": (A.HK_F32, A.HK_F32), "class-i32/axis-i32": (A.HK_COORDS_CLASS_I32, A.HK_I32),
            "class-i32/logits": (A.HK_COORDS_CLASS_I32, A.HK_AXIS_MASKED_LOGITS), "mask-u8/axis-i32": (A.HK_U8, A.HK_I32)}
    AXIS = {A.HK_I32: torch.int32, A.HK_I64: torch.int64, A.HK_F32: torch.float32}

    def step(label, m, d, stages, flags, act="mask-f32/axis-i32", b=97, feat=False, dtype=A.HK_F32, stride_extra=0,
             offset=0, feat_offset=0):
        tdt = torch.float32 if dtype == A.HK_F32 else torch.float64
        src = states(b + 1, m, d, tdt, stride_extra)
        dst = zeros(b + 1, m * d + stride_extra, dtype=tdt)
        s = A.hk_step_desc()
        s.points_in, s.points_out = src.data_ptr() + offset, dst.data_ptr() + offset
        s.in_stride = s.out_stride = m * d + stride_extra
        s.padding_value, s.reward_sign = -1.0, 1.0
        s.batch, s.max_points, s.dim, s.dtype, s.stages, s.flags = b, m, d, dtype, stages, flags
        s.coords_kind = A.HK_COORDS_NONE
        if stages & A.HK_STAGE_SHIFT:
            kind, axis = ACTS[act]
            s.coords_kind, s.axis_dtype, s.coords_stride = kind, axis, d
            if kind == A.HK_COORDS_CLASS_I32:
                s.coords = zeros(b, dtype=torch.int32).data_ptr()  # class 0: the first two coordinates
            else:
                keep.append(torch.ones(b, d, dtype=torch.uint8 if kind == A.HK_U8 else torch.float32, device=dev))
                s.coords = keep[-1].data_ptr()
            if axis == A.HK_AXIS_MASKED_LOGITS:
                s.axis = zeros(b, d).data_ptr()
            else:
                s.axis = zeros(b, dtype=AXIS[axis]).data_ptr()
        if feat:
            out = zeros(b + 1, m * d)
            report(label, L.hk_step_features(C.byref(s), out.data_ptr() + feat_offset, 0, stream))
        else:
            report(label, L.hk_step(C.byref(s), stream))

    for act in ACTS:
        step(f"step (20,3) jax take_actions {act}", 20, 3, TAKE, A.HK_SEM_JAX, act)
        step(f"step (20,3) torch {act}", 20, 3, TAKE, A.HK_SEM_TORCH, act)
        step(f"step+features (20,3) jax take_actions {act}", 20, 3, TAKE, A.HK_SEM_JAX, act, feat=True)
        step(f"step+features (20,3) torch {act}", 20, 3, TAKE, A.HK_SEM_TORCH, act, feat=True)
    step("step (50,4) jax take_actions class-i32/logits", 50, 4, TAKE, A.HK_SEM_JAX, "class-i32/logits")
    step("step (50,4) torch class-i32/logits", 50, 4, TAKE, A.HK_SEM_TORCH, "class-i32/logits")
    step("step (50,4) jax take_actions mask-f32/axis-i32", 50, 4, TAKE, A.HK_SEM_JAX)
    step("step+features (50,4) jax take_actions class-i32/axis-i32", 50, 4, TAKE, A.HK_SEM_JAX, "class-i32/axis-i32", feat=True)
    step("step+features (20,3) list class-i32/axis-i32", 20, 3, TAKE, A.HK_SEM_LIST, "class-i32/axis-i32", feat=True)
    step("step+features (20,3) jax compact-sorted class-i32/axis-i32", 20, 3, TAKE,
         A.HK_SEM_JAX | A.HK_FLAG_COMPACT_SORTED, "class-i32/axis-i32", feat=True)
    step("step+features (20,3) jax take_actions mask-f32/axis-i32 FOUR_LANES", 20, 3, TAKE, A.HK_SEM_JAX | FOUR, feat=True)
    step("step+features (20,3) jax take_actions class-i32/axis-i32 ONE_LANE", 20, 3, TAKE, A.HK_SEM_JAX | ONE,
         "class-i32/axis-i32", feat=True)
    step("step+features (20,3) jax take_actions class-i32/axis-i32 misaligned features", 20, 3, TAKE, A.HK_SEM_JAX,
         "class-i32/axis-i32", feat=True, feat_offset=4)
    step("step (16,3) jax take_actions mask-f32/axis-i32", 16, 3, TAKE, A.HK_SEM_JAX)
    step("step (16,3) jax take_actions class-i32/logits", 16, 3, TAKE, A.HK_SEM_JAX, "class-i32/logits")
    step("step (20,3) jax newton only", 20, 3, A.HK_STAGE_NEWTON, A.HK_SEM_JAX)
    step("step (20,3) list: sorted output, m*d = 60", 20, 3, TAKE, A.HK_SEM_LIST)
    step("step (20,4) list: sorted output, m*d = 80", 20, 4, TAKE, A.HK_SEM_LIST)
    step("step (50,4) list: sorted output, m*d = 200", 50, 4, TAKE, A.HK_SEM_LIST)
    step("step (20,3) jax compact-sorted", 20, 3, TAKE, A.HK_SEM_JAX | A.HK_FLAG_COMPACT_SORTED)
    step("step (20,3) list TWO_LANES", 20, 3, TAKE, A.HK_SEM_LIST | TWO)
    step("step (20,3) misaligned", 20, 3, TAKE, A.HK_SEM_JAX, offset=4)
    step("step (20,3) strided", 20, 3, TAKE, A.HK_SEM_JAX, stride_extra=4)
    step("step (20,3) strided TWO_LANES", 20, 3, TAKE, A.HK_SEM_JAX | TWO, stride_extra=4)
    step("step (20,3) misaligned ONE_LANE", 20, 3, TAKE, A.HK_SEM_JAX | ONE, offset=4)
    step("step (50,4) strided", 50, 4, TAKE, A.HK_SEM_JAX, stride_extra=4)
    step("step (7,3) strided", 7, 3, TAKE, A.HK_SEM_JAX, stride_extra=4)
    FORCES = {"GENERIC": GENERIC, "TEAM": TEAM, "ONE_LANE": ONE, "TWO_LANES": TWO, "FOUR_LANES": FOUR,
              "ONE_LANE|TWO_LANES": ONE | TWO, "FOUR_LANES|ONE_LANE": FOUR | ONE, "FOUR_LANES|TWO_LANES": FOUR | TWO,
              "TEAM|FOUR_LANES": TEAM | FOUR, "GENERIC|TEAM": GENERIC | TEAM}
    for name, f in FORCES.items():
        step(f"step (20,3) jax take_actions {name}", 20, 3, TAKE, A.HK_SEM_JAX | f)
    step("step (20,3) jax take_actions TWO_LANES x 98368", 20, 3, TAKE, A.HK_SEM_JAX | TWO, b=98368)
    step("step (7,3) jax take_actions", 7, 3, TAKE, A.HK_SEM_JAX)
    step("step (7,3) list", 7, 3, TAKE, A.HK_SEM_LIST)
    step("step (9,7) jax take_actions", 9, 7, TAKE, A.HK_SEM_JAX)
    step("step (70,3) jax take_actions", 70, 3, TAKE, A.HK_SEM_JAX)
    step("step (20,3) f64", 20, 3, TAKE, A.HK_SEM_JAX, dtype=A.HK_F64)

    # ---- the sorted observation features ---------------------------------------------------------------------------------
    def feats(label, m, d, torch_sem=False, scale=0, b=97):
        src, dst = states(b, m, d), zeros(b, m * d)
        if torch_sem:
            st = L.hk_get_features_torch(src.data_ptr(), m * d, dst.data_ptr(), m * d, b, m, d, A.HK_F32, -1.0, stream)
        else:
            st = L.hk_get_features(src.data_ptr(), m * d, dst.data_ptr(), m * d, b, m, d, A.HK_F32, scale, -1.0, stream)
        report(label, st)

    feats("features sort (50,4)", 50, 4)
    feats("features sort (50,4) rescaled", 50, 4, scale=1)
    feats("features sort (20,3)", 20, 3)
    feats("features sort (20,3) torch", 20, 3, torch_sem=True)
    feats("features sort (7,3)", 7, 3)

    # ---- hk_rollout --------------------------------------------------------------------------------------------------------
    def rollout(label, m, d, b, steps=20, flags=A.HK_SEM_JAX, stages=TAKE, host=A.HK_HOST_RANDOM, recs=False, obs=False,
                gen=False, episodes=1, dtype=A.HK_F32, stride_ok=True, offset=0):
        tdt = torch.float32 if dtype == A.HK_F32 else torch.float64
        r = A.hk_rollout_desc()
        buf = zeros(b + 1, m * d, dtype=tdt)
        r.points = buf.data_ptr() + offset
        if not gen:
            r.points_in = states(b + 1, m, d, tdt).data_ptr() + offset
        r.seed, r.padding_value, r.reward_sign = 7, -1.0, 1.0
        r.batch, r.max_points, r.dim, r.dtype, r.steps = b, m, d, dtype, steps
        r.host_policy = host
        r.agent_policy = A.HK_AGENT_RANDOM_LEGAL if (flags & ~(ONE | TWO | FOUR | TEAM | GENERIC)) == TORCH else A.HK_AGENT_RANDOM
        r.stages, r.flags, r.episodes = stages, flags, episodes
        if gen:
            r.gen_max_value, r.gen_seed = 20, 11
        if recs:
            r.axis_out = zeros(steps, b, dtype=torch.int32).data_ptr()
        if obs:
            r.obs_out = zeros(steps, b, m * d).data_ptr()
        nbytes = L.hk_rollout_workspace_bytes(C.byref(r))
        if nbytes:
            r.workspace, r.workspace_bytes = zeros(nbytes // 4, dtype=torch.int32).data_ptr(), nbytes
            r.done_count = zeros(steps + 1, dtype=torch.int64).data_ptr()
        report(f"{label} [workspace {nbytes}]", L.hk_rollout(C.byref(r), stream))

    ZEIL = A.HK_HOST_ZEILLINGER
    for name, f in FORCES.items():
        rollout(f"rollout (20,3) jax x 97 {name}", 20, 3, 97, flags=A.HK_SEM_JAX | f)
        rollout(f"rollout (20,3) jax x 97 3 episodes {name}", 20, 3, 97, flags=A.HK_SEM_JAX | f, episodes=3)
        rollout(f"rollout (50,4) jax x 97 3 episodes {name}", 50, 4, 97, flags=A.HK_SEM_JAX | f, episodes=3)
    for f, fname in ((0, ""), (TWO, " TWO_LANES"), (ONE, " ONE_LANE")):
        rollout(f"rollout (20,3) jax{fname} x 97", 20, 3, 97, flags=A.HK_SEM_JAX | f)
        rollout(f"rollout (20,3) torch{fname} x 97", 20, 3, 97, flags=TORCH | f)
        rollout(f"rollout (20,3) list{fname} x 97", 20, 3, 97, flags=A.HK_SEM_LIST | f)
        rollout(f"rollout (20,3) jax rescaled{fname} x 97", 20, 3, 97, flags=A.HK_SEM_JAX | f, stages=TAKE | A.HK_STAGE_RESCALE)
        rollout(f"rollout (20,3) jax Zeillinger's host{fname} x 97", 20, 3, 97, flags=A.HK_SEM_JAX | f, host=ZEIL)
        rollout(f"rollout (20,3) jax small records{fname} x 97", 20, 3, 97, flags=A.HK_SEM_JAX | f, recs=True)
        rollout(f"rollout (20,3) torch small records{fname} x 97", 20, 3, 97, flags=TORCH | f, recs=True)
        rollout(f"rollout (20,3) jax observations{fname} x 97", 20, 3, 97, flags=A.HK_SEM_JAX | f, obs=True)
        rollout(f"rollout (20,3) torch observations{fname} x 97", 20, 3, 97, flags=TORCH | f, obs=True)
        rollout(f"rollout (20,3) jax Zeillinger's host small records{fname} x 97", 20, 3, 97, flags=A.HK_SEM_JAX | f,
                host=ZEIL, recs=True)
    rollout("rollout (50,4) jax x 97", 50, 4, 97)
    rollout("rollout (50,4) jax Zeillinger's host x 97", 50, 4, 97, host=ZEIL)
    rollout("rollout (50,4) list x 97", 50, 4, 97, flags=A.HK_SEM_LIST)
    rollout("rollout (50,4) jax observations x 97", 50, 4, 97, obs=True)
    rollout("rollout (50,4) jax Zeillinger's host observations x 97", 50, 4, 97, host=ZEIL, obs=True)
    rollout("rollout (50,4) jax TWO_LANES x 97", 50, 4, 97, flags=A.HK_SEM_JAX | TWO)
    rollout("rollout (16,3) jax x 97", 16, 3, 97)
    rollout("rollout (7,3) jax x 97", 7, 3, 97)
    rollout("rollout (7,3) jax Zeillinger's host x 97", 7, 3, 97, host=ZEIL)
    rollout("rollout (9,7) jax x 97", 9, 7, 97)
    rollout("rollout (20,3) f64 x 97", 20, 3, 97, dtype=A.HK_F64)
    rollout("rollout (20,3) jax misaligned x 97", 20, 3, 97, offset=4)
    # the crossovers of pick, at the default flags, short rollouts
    rollout("rollout (20,3) jax 7 steps x 32768", 20, 3, 32768, steps=7)
    rollout("rollout (20,3) jax 7 steps x 32784", 20, 3, 32784, steps=7)
    rollout("rollout (20,3) jax 6 steps x 65536", 20, 3, 65536, steps=6)
    rollout("rollout (20,3) jax 7 steps x 65536", 20, 3, 65536, steps=7)
    rollout("rollout (20,3) jax 6 steps x 65552", 20, 3, 65552, steps=6)
    rollout("rollout (20,3) jax 7 steps x 98304", 20, 3, 98304, steps=7)
    rollout("rollout (20,3) jax 7 steps x 98368", 20, 3, 98368, steps=7)
    rollout("rollout (20,4) jax 7 steps x 98368", 20, 4, 98368, steps=7)
    rollout("rollout (16,3) jax 7 steps x 98368", 16, 3, 98368, steps=7)
    rollout("rollout (20,3) jax small records 2 steps x 65536", 20, 3, 65536, steps=2, recs=True)
    rollout("rollout (20,3) jax small records 2 steps x 98368", 20, 3, 98368, steps=2, recs=True)
    rollout("rollout (20,3) jax observations 2 steps x 65536", 20, 3, 65536, steps=2, obs=True)
    rollout("rollout (20,3) jax 7 steps FOUR_LANES x 98368", 20, 3, 98368, steps=7, flags=A.HK_SEM_JAX | FOUR)
    # generated initial states, episodes back to back
    for b, steps in ((97, 20), (65552, 3)):
        rollout(f"rollout (20,3) jax generated x {b}", 20, 3, b, steps, gen=True)
        rollout(f"rollout (20,3) torch generated x {b}", 20, 3, b, steps, flags=TORCH, gen=True)
        rollout(f"rollout (20,3) jax rescaled generated x {b}", 20, 3, b, steps, stages=TAKE | A.HK_STAGE_RESCALE, gen=True)
        rollout(f"rollout (20,3) jax Zeillinger's host generated x {b}", 20, 3, b, steps, host=ZEIL, gen=True)
        rollout(f"rollout (20,3) jax generated 3 episodes x {b}", 20, 3, b, steps, gen=True, episodes=3)
        rollout(f"rollout (20,3) jax 3 episodes x {b}", 20, 3, b, steps, episodes=3)
        rollout(f"rollout (20,3) torch 3 episodes x {b}", 20, 3, b, steps, flags=TORCH, episodes=3)
        rollout(f"rollout (20,3) list 3 episodes x {b}", 20, 3, b, steps, flags=A.HK_SEM_LIST, episodes=3)
        rollout(f"rollout (20,3) jax Zeillinger's host 3 episodes x {b}", 20, 3, b, steps, host=ZEIL, episodes=3)
    rollout("rollout (20,3) jax 3 episodes 3 steps x 65536", 20, 3, 65536, 3, episodes=3)
    rollout("rollout (50,4) jax generated x 97", 50, 4, 97, gen=True)
    rollout("rollout (50,4) jax Zeillinger's host generated x 97", 50, 4, 97, host=ZEIL, gen=True)
    rollout("rollout (50,4) jax 3 episodes x 97", 50, 4, 97, episodes=3)
    rollout("rollout (50,4) jax Zeillinger's host 3 episodes x 97", 50, 4, 97, host=ZEIL, episodes=3)
    rollout("rollout (20,3) jax generated misaligned", 20, 3, 97, gen=True, offset=4)
    rollout("rollout (16,3) jax generated x 97", 16, 3, 97, gen=True)
    rollout("rollout (7,3) jax generated x 97", 7, 3, 97, gen=True)

    # ---- the generator, the binning entries, hk_zeillinger -----------------------------------------------------------------
    def generate(label, m, d, stages=0, flags=A.HK_SEM_JAX, pad=-1.0, dtype=A.HK_F32, offset=0, b=97):
        out = zeros(b + 1, m * d, dtype=torch.float32 if dtype == A.HK_F32 else torch.float64)
        report(label, L.hk_generate_points(out.data_ptr() + offset, b, m, d, dtype, 20, 5, 0, stages, pad, flags, stream))

    for name, f in FORCES.items():
        generate(f"generate (20,3) {name}", 20, 3, flags=A.HK_SEM_JAX | f)
    generate("generate (20,3)", 20, 3)
    generate("generate (50,4) newton", 50, 4, A.HK_STAGE_NEWTON)
    generate("generate (20,3) list newton", 20, 3, A.HK_STAGE_NEWTON, A.HK_SEM_LIST)
    generate("generate (20,3) list", 20, 3, 0, A.HK_SEM_LIST)
    generate("generate (20,3) padding 0", 20, 3, pad=0.0)
    generate("generate (20,3) misaligned", 20, 3, offset=4)
    generate("generate (16,3)", 16, 3)
    generate("generate (7,3)", 7, 3)
    generate("generate (20,3) f64", 20, 3, dtype=A.HK_F64)

    def binned(label, m, d, flags=A.HK_SEM_JAX, b=1000, from_memory=False):
        out, ids, nps = zeros(b, m * d), zeros(b, dtype=torch.int32), zeros(b, dtype=torch.int32)
        if from_memory:
            st = L.hk_bin_by_live_rows(states(b, m, d).data_ptr(), out.data_ptr(), ids.data_ptr(), nps.data_ptr(), b, m, d,
                                       A.HK_F32, stream)
        else:
            st = L.hk_generate_points_binned(out.data_ptr(), ids.data_ptr(), nps.data_ptr(), b, m, d, A.HK_F32, 20, 5, 0, 0,
                                             -1.0, flags, stream)
        report(label, st)

    for m, d in ((10, 3), (20, 3), (20, 4), (50, 4), (16, 3)):
        binned(f"generate binned ({m},{d}) x 1000", m, d)
        binned(f"bin by live rows ({m},{d}) x 1000", m, d, from_memory=True)
    binned("generate binned (20,3) x 1000 ONE_LANE", 20, 3, flags=A.HK_SEM_JAX | ONE)

    def zeillinger(label, m, d, flags=A.HK_SEM_JAX, dtype=A.HK_F32, offset=0, stride_extra=0, b=97):
        src = states(b + 1, m, d, torch.float32 if dtype == A.HK_F32 else torch.float64, stride_extra)
        out = zeros(b, dtype=torch.int32)
        report(label, L.hk_zeillinger(src.data_ptr() + offset, m * d + stride_extra, out.data_ptr(), b, m, d, dtype, flags,
                                      stream))

    for name, f in FORCES.items():
        zeillinger(f"zeillinger (20,3) {name}", 20, 3, A.HK_SEM_JAX | f)
    zeillinger("zeillinger (20,3) jax", 20, 3)
    zeillinger("zeillinger (50,4) jax", 50, 4)
    zeillinger("zeillinger (20,3) list", 20, 3, A.HK_SEM_LIST)
    zeillinger("zeillinger (50,4) list", 50, 4, A.HK_SEM_LIST)
    zeillinger("zeillinger (20,3) jax misaligned", 20, 3, offset=4)
    zeillinger("zeillinger (20,3) jax strided", 20, 3, stride_extra=4)
    zeillinger("zeillinger (16,3) jax", 16, 3)
    zeillinger("zeillinger (7,3) jax", 7, 3)
    zeillinger("zeillinger (9,7) jax", 9, 7)
    zeillinger("zeillinger (20,3) f64", 20, 3, dtype=A.HK_F64)
    torch.cuda.synchronize()
    print("done", flush=True)


if __name__ == "__main__":
    main()
