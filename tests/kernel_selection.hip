// Which kernel serves a request: a stand-alone host program over the selection headers of hironaka_amd/csrc (no
// library, no device).  For a fixed table of requests -- one row per branch of the selection and of every family's
// choice of instantiation -- it prints
//     label -> family / the family's variant / grid / count_slots
// (tests/test_kernel_selection.py compares the output with tests/golden/kernel_selection.txt) and checks for every row:
//   * the family `pick` names has an instantiation for the request (its variant is not none; the generic kernel, the
//     last resort, has one instantiation per dtype and declines by its geometry alone);
//   * planned_grid is that family's own grid function;
//   * count_slots of the row's geometry is at least the grid under every combination of the testing flags: a kernel
//     adds its finished-game counts at [step][workgroup] of a workspace of that row length.
// Without a device device_simds() is 1024, the MI355X's own number: the crossovers below are that machine's.
#include <cstdio>
#include <string>
#include <vector>

#include "hk_select.h"

using namespace hk;

namespace {

constexpr unsigned kTake = HK_STAGE_SHIFT | HK_STAGE_REPOSITION | HK_STAGE_NEWTON;  // the trainers' take_actions
constexpr unsigned kTorch = kHotTorchFlags;
void* const kIn = reinterpret_cast<void*>(0x100000);
void* const kOut = reinterpret_cast<void*>(0x200000);
void* const kAux = reinterpret_cast<void*>(0x300000);  // coords, axis, records, features: any aligned pointer

struct Row {
  std::string label;
  Params prm;
  int dtype = HK_F32;
};
std::vector<Row> rows;
int failures = 0;

Params base(int mode, int m, int d, int batch, unsigned stages, unsigned flags) {
  Params p{};
  p.in = kIn;
  p.out = kOut;
  p.in_stride = p.out_stride = (int64_t)m * d;
  p.coords_kind = HK_COORDS_NONE;
  p.pad = -1.0;
  p.reward_sign = 1.0f;
  p.batch = batch;
  p.m = m;
  p.d = d;
  p.stages = stages;
  p.flags = flags;
  p.mode = mode;
  p.episodes = 1;
  return p;
}
// hk_step with a caller's action: the subset as `coords_kind`, the axis as `axis_dtype`
Params step(int m, int d, unsigned stages, unsigned flags, int coords_kind = HK_F32, int axis_dtype = HK_I32, int batch = 97) {
  Params p = base(kModeStep, m, d, batch, stages, flags);
  if (stages & HK_STAGE_SHIFT) {
    p.coords = kAux;
    p.coords_stride = d;
    p.coords_kind = coords_kind;
    p.axis = kAux;
    p.axis_dtype = axis_dtype;
  }
  return p;
}
Params features(Params p) {
  p.feat_out = (float*)kAux;
  return p;
}
Params rollout(int m, int d, int batch, int steps = 20, unsigned flags = HK_SEM_JAX, unsigned stages = kTake) {
  Params p = base(kModeRollout, m, d, batch, stages, flags);
  p.steps = steps;
  p.host_policy = HK_HOST_RANDOM;
  p.agent_policy = flags == kTorch ? HK_AGENT_RANDOM_LEGAL : HK_AGENT_RANDOM;
  return p;
}
Params zeil_host(Params p) {
  p.host_policy = HK_HOST_ZEILLINGER;
  return p;
}
Params small_recs(Params p) {
  p.r_axis_out = (int32_t*)kAux;
  return p;
}
Params observations(Params p) {
  p.obs_out = kAux;
  return p;
}
Params generated(Params p, int episodes = 1) {  // hk_rollout_desc.gen_max_value
  p.in = nullptr;
  p.max_value = 20;
  p.episodes = episodes;
  return p;
}
Params episodes(Params p, int n) {
  p.episodes = n;
  return p;
}
Params generate(int m, int d, unsigned stages = 0, unsigned flags = HK_SEM_JAX, int batch = 97) {
  Params p = base(kModeGenerate, m, d, batch, stages, flags);
  p.in = nullptr;
  p.max_value = 20;
  return p;
}
Params zeillinger(int m, int d, unsigned flags = HK_SEM_JAX, int batch = 97) {
  Params p = base(kModeZeillinger, m, d, batch, 0, flags);
  p.out = nullptr;
  p.class_out = (int32_t*)kAux;
  return p;
}
Params with_flags(Params p, unsigned f) {
  p.flags |= f;
  return p;
}
Params misaligned(Params p) {  // element-aligned, not vector-aligned
  if (p.in) p.in = (const char*)p.in + 4;
  p.out = p.out ? (char*)p.out + 4 : p.out;
  return p;
}
Params strided(Params p) {
  p.in_stride += 4;
  p.out_stride += 4;
  return p;
}
void add(const std::string& label, const Params& p, int dtype = HK_F32) { rows.push_back({label, p, dtype}); }

const char* name(Kernel k) {
  switch (k) {
    case Kernel::None: return "none";
    case Kernel::Quad: return "quad";
    case Kernel::QuadRoll: return "quadroll";
    case Kernel::QuadRollFused: return "quadroll-fused";
    case Kernel::QuadGen: return "quadgen";
    case Kernel::QuadZeil: return "quadzeil";
    case Kernel::Duo: return "duo";
    case Kernel::Fast: return "fast";
    case Kernel::Team: return "team";
    case Kernel::Generic: return "generic";
  }
  return "?";
}
const char* mode_name(int mode) {
  switch (mode) {
    case kModeStep: return "step";
    case kModeRollout: return "rollout";
    case kModeGenerate: return "generate";
    case kModeRolloutRec: return "rollout-rec";
    case kModeStepAux: return "step-aux";
  }
  return "none";
}
const char* hot_name(int hot) {
  switch (hot) {
    case kHotNone: return "runtime";
    case kHotJax: return "jax";
    case kHotTorch: return "torch";
    case kHotSort: return "sort";
    case kHotList: return "list";
  }
  return "none";
}
const char* act_name(int act) {
  static const char* const names[] = {"any", "mask-f32/axis-i32", "mask-f32/axis-i64", "mask-f32/axis-f32",
                                      "class-i32/axis-i32", "class-i32/logits"};
  return names[act];
}

// the family's own grid function: planned_grid must agree
int64_t family_grid(Kernel k, const Params& p, int dtype) {
  switch (k) {
    case Kernel::Quad:
    case Kernel::QuadGen: return quad_grid(p);
    case Kernel::QuadRoll:
    case Kernel::QuadRollFused:
    case Kernel::QuadZeil: return quadroll_grid(p);
    case Kernel::Duo: return duo_grid(p);
    case Kernel::Fast: return fast_grid(p);
    case Kernel::Team: return team_grid(p);
    case Kernel::Generic: return generic_grid(p, dtype);
    case Kernel::None: break;
  }
  return 0;
}

// the variant of the family for the request as its launcher sees it; *none: the family has no instantiation for it
std::string variant(Kernel k, const Params& request, int dtype, bool* none) {
  Params p = as_launched(request);
  if (p.mode == kModeZeillinger && (k == Kernel::Fast || k == Kernel::Team)) p = zeillinger_step(p);
  if (p.mode == kModeRollout && k != Kernel::QuadRollFused) p = plain_rollout(p);
  char buf[160];
  switch (k) {
    case Kernel::Quad: {
      const QuadVariant v = quad_variant(p, quad_shape(p.m, p.d));
      *none = v.none();
      snprintf(buf, sizeof buf, "hot=%s act=%s feat=%d", hot_name(v.hot), act_name(v.act), (int)v.feat);
      break;
    }
    case Kernel::QuadZeil: p = quadzeil_rollout(p);  // fall through
    case Kernel::QuadRoll:
    case Kernel::QuadRollFused: {
      const QuadRollVariant v = quadroll_variant(p);
      *none = v.none();
      snprintf(buf, sizeof buf, "hot=%s rec=%d zeil=%d gen=%d epi=%d", hot_name(v.hot), (int)v.rec, (int)v.zeil, (int)v.gen,
               (int)v.epi);
      break;
    }
    case Kernel::QuadGen:
      *none = !quad_shape(p.m, p.d).known;
      snprintf(buf, sizeof buf, "wpb=%d", quad_shape(p.m, p.d).wpb);
      break;
    case Kernel::Duo: {
      const DuoVariant v = duo_variant(p);
      *none = v.none();
      snprintf(buf, sizeof buf, "mode=%s hot=%s acts=%d zeil=%d", mode_name(v.mode), hot_name(v.hot), (int)v.acts, (int)v.zeil);
      break;
    }
    case Kernel::Fast: {
      const FastVariant v = fast_variant(p);
      *none = v.none();
      snprintf(buf, sizeof buf, "mode=%s hot=%s", mode_name(v.mode), hot_name(v.hot));
      break;
    }
    case Kernel::Team: {
      const TeamVariant v = team_variant(p);
      *none = v.none();
      snprintf(buf, sizeof buf, "mode=%s zeil=%d lds_stride=%d", mode_name(v.mode), (int)v.zeil, team_lds_stride(p.m, p.d));
      break;
    }
    case Kernel::Generic: {
      // (the one family whose launcher may still decline: plan_generic finds no geometry for a game that large, and
      // launch_generic returns HK_ERR_UNSUPPORTED -- there is no kernel after the generic one to fall back to)
      *none = false;
      if (plan_generic(p, dtype) == HK_OK) snprintf(buf, sizeof buf, "games_per_block=%d lds_stride=%d", p.games_per_block, p.lds_stride);
      else snprintf(buf, sizeof buf, "no geometry");
      break;
    }
    case Kernel::None:
      *none = false;
      snprintf(buf, sizeof buf, "-");
      break;
  }
  return buf;
}

void fail(const Row& r, const char* what) {
  printf("FAILED %s: %s\n", r.label.c_str(), what);
  ++failures;
}

// the geometry hk_rollout sizes the workspace for
Params geometry(const Params& p, int dtype) {
  return p.mode == kModeRollout && pick(p, dtype) != Kernel::QuadRollFused ? plain_rollout(p) : p;
}

void report(const Row& r) {
  const Kernel k = pick(r.prm, r.dtype);
  bool none = false;
  const std::string v = variant(k, r.prm, r.dtype, &none);
  const Params geo = geometry(r.prm, r.dtype);
  const int64_t grid = planned_grid(geo, r.dtype), slots = count_slots(geo, r.dtype);
  printf("%s -> %s / %s / grid=%lld / count_slots=%lld\n", r.label.c_str(), name(k), v.c_str(), (long long)grid,
         (long long)slots);
  if (none) fail(r, "the family pick names has no instantiation for the request");
  if (grid != family_grid(pick(geo, r.dtype), geo, r.dtype)) fail(r, "planned_grid is not the family's grid");
  for (unsigned combo = 0; combo < 32; ++combo) {  // every combination of the five testing flags
    Params q = r.prm;
    q.flags &= ~kForceFlags;
    if (combo & 1) q.flags |= HK_FLAG_FORCE_GENERIC;
    if (combo & 2) q.flags |= HK_FLAG_FORCE_TEAM;
    if (combo & 4) q.flags |= HK_FLAG_FORCE_ONE_LANE;
    if (combo & 8) q.flags |= HK_FLAG_FORCE_TWO_LANES;
    if (combo & 16) q.flags |= HK_FLAG_FORCE_FOUR_LANES;
    if (planned_grid(geometry(q, r.dtype), r.dtype) > slots) fail(r, "a forced family's grid exceeds count_slots");
  }
}

void table() {
  // ---- hk_step: every action layout, in the JAX trainer's configuration (hot) and not -------------------------------
  const struct {
    const char* name;
    int coords, axis;
  } acts[] = {{"mask-f32/axis-i32", HK_F32, HK_I32},           {"mask-f32/axis-i64", HK_F32, HK_I64},
              {"mask-f32/axis-f32", HK_F32, HK_F32},           {"class-i32/axis-i32", HK_COORDS_CLASS_I32, HK_I32},
              {"class-i32/logits", HK_COORDS_CLASS_I32, HK_AXIS_MASKED_LOGITS}, {"mask-u8/axis-i32", HK_U8, HK_I32}};
  for (const auto& a : acts) {
    add(std::string("step (20,3) jax take_actions ") + a.name, step(20, 3, kTake, HK_SEM_JAX, a.coords, a.axis));
    add(std::string("step (20,3) torch ") + a.name, step(20, 3, kTake, HK_SEM_TORCH, a.coords, a.axis));
    // feat_out: each accepted and each refused action layout
    add(std::string("step+features (20,3) jax take_actions ") + a.name, features(step(20, 3, kTake, HK_SEM_JAX, a.coords, a.axis)));
    add(std::string("step+features (20,3) torch ") + a.name, features(step(20, 3, kTake, HK_SEM_TORCH, a.coords, a.axis)));
  }
  add("step (50,4) jax take_actions class-i32/logits", step(50, 4, kTake, HK_SEM_JAX, HK_COORDS_CLASS_I32, HK_AXIS_MASKED_LOGITS));
  add("step (50,4) torch class-i32/logits", step(50, 4, kTake, HK_SEM_TORCH, HK_COORDS_CLASS_I32, HK_AXIS_MASKED_LOGITS));
  add("step (50,4) jax take_actions mask-f32/axis-i32", step(50, 4, kTake, HK_SEM_JAX));
  add("step+features (50,4) jax take_actions class-i32/axis-i32", features(step(50, 4, kTake, HK_SEM_JAX, HK_COORDS_CLASS_I32, HK_I32)));
  add("step+features (20,3) list class-i32/axis-i32", features(step(20, 3, kTake, HK_SEM_LIST, HK_COORDS_CLASS_I32, HK_I32)));
  add("step+features (20,3) jax compact-sorted class-i32/axis-i32",
      features(step(20, 3, kTake, HK_SEM_JAX | HK_FLAG_COMPACT_SORTED, HK_COORDS_CLASS_I32, HK_I32)));
  add("step+features (20,3) jax take_actions mask-f32/axis-i32 FOUR_LANES",
      with_flags(features(step(20, 3, kTake, HK_SEM_JAX)), HK_FLAG_FORCE_FOUR_LANES));
  add("step+features (20,3) jax take_actions class-i32/axis-i32 ONE_LANE",
      with_flags(features(step(20, 3, kTake, HK_SEM_JAX, HK_COORDS_CLASS_I32, HK_I32)), HK_FLAG_FORCE_ONE_LANE));
  add("step+features (20,3) jax take_actions class-i32/axis-i32 misaligned features", [] {
    Params p = features(step(20, 3, kTake, HK_SEM_JAX, HK_COORDS_CLASS_I32, HK_I32));
    p.feat_out += 1;
    return p;
  }());
  add("step (16,3) jax take_actions mask-f32/axis-i32", step(16, 3, kTake, HK_SEM_JAX));
  add("step (16,3) jax take_actions class-i32/logits", step(16, 3, kTake, HK_SEM_JAX, HK_COORDS_CLASS_I32, HK_AXIS_MASKED_LOGITS));
  add("step (20,3) jax newton only", step(20, 3, HK_STAGE_NEWTON, HK_SEM_JAX));
  add("step (20,3) jax take_actions coords in record", [] {
    Params p = step(20, 3, kTake, HK_SEM_JAX, HK_COORDS_IN_RECORD, HK_I32);
    p.in_stride += 3;
    return p;
  }());
  // the sorted observation features, the class output, sorted + compacted output
  add("features sort (50,4)", step(50, 4, kStageFeatureSort, HK_SEM_JAX));
  add("features sort (50,4) rescaled", step(50, 4, HK_STAGE_RESCALE | kStageFeatureSort, HK_SEM_JAX));
  add("features sort (20,3)", step(20, 3, kStageFeatureSort, HK_SEM_JAX));
  add("features sort (20,3) torch", step(20, 3, kStageFeatureSort0, HK_SEM_TORCH));
  add("features sort (20,3) ONE_LANE", with_flags(step(20, 3, kStageFeatureSort, HK_SEM_JAX), HK_FLAG_FORCE_ONE_LANE));
  add("features sort (20,3) TWO_LANES", with_flags(step(20, 3, kStageFeatureSort, HK_SEM_JAX), HK_FLAG_FORCE_TWO_LANES));
  add("features sort (7,3)", step(7, 3, kStageFeatureSort, HK_SEM_JAX));
  add("step (20,3) class_out", [] {
    Params p = step(20, 3, 0, HK_SEM_JAX);
    p.class_out = (int32_t*)kAux;
    return p;
  }());
  add("step (20,3) list: sorted output, m*d = 60", step(20, 3, kTake, HK_SEM_LIST));
  add("step (20,4) list: sorted output, m*d = 80", step(20, 4, kTake, HK_SEM_LIST));
  add("step (50,4) list: sorted output, m*d = 200", step(50, 4, kTake, HK_SEM_LIST));
  add("step (20,3) jax compact-sorted", step(20, 3, kTake, HK_SEM_JAX | HK_FLAG_COMPACT_SORTED));
  add("step (20,3) list TWO_LANES", with_flags(step(20, 3, kTake, HK_SEM_LIST), HK_FLAG_FORCE_TWO_LANES));
  // layouts, per family
  add("step (20,3) misaligned", misaligned(step(20, 3, kTake, HK_SEM_JAX)));
  add("step (20,3) strided", strided(step(20, 3, kTake, HK_SEM_JAX)));
  add("step (20,3) strided TWO_LANES", with_flags(strided(step(20, 3, kTake, HK_SEM_JAX)), HK_FLAG_FORCE_TWO_LANES));
  add("step (20,3) misaligned ONE_LANE", with_flags(misaligned(step(20, 3, kTake, HK_SEM_JAX)), HK_FLAG_FORCE_ONE_LANE));
  add("step (50,4) strided", strided(step(50, 4, kTake, HK_SEM_JAX)));
  add("step (7,3) strided", strided(step(7, 3, kTake, HK_SEM_JAX)));
  // the testing flags on steps
  const struct {
    const char* name;
    unsigned flags;
  } forces[] = {{"GENERIC", HK_FLAG_FORCE_GENERIC},
                {"TEAM", HK_FLAG_FORCE_TEAM},
                {"ONE_LANE", HK_FLAG_FORCE_ONE_LANE},
                {"TWO_LANES", HK_FLAG_FORCE_TWO_LANES},
                {"FOUR_LANES", HK_FLAG_FORCE_FOUR_LANES},
                {"ONE_LANE|TWO_LANES", HK_FLAG_FORCE_ONE_LANE | HK_FLAG_FORCE_TWO_LANES},
                {"FOUR_LANES|ONE_LANE", HK_FLAG_FORCE_FOUR_LANES | HK_FLAG_FORCE_ONE_LANE},
                {"FOUR_LANES|TWO_LANES", HK_FLAG_FORCE_FOUR_LANES | HK_FLAG_FORCE_TWO_LANES},
                {"TEAM|FOUR_LANES", HK_FLAG_FORCE_TEAM | HK_FLAG_FORCE_FOUR_LANES},
                {"GENERIC|TEAM", HK_FLAG_FORCE_GENERIC | HK_FLAG_FORCE_TEAM}};
  for (const auto& f : forces) {
    add(std::string("step (20,3) jax take_actions ") + f.name, with_flags(step(20, 3, kTake, HK_SEM_JAX), f.flags));
    add(std::string("rollout (20,3) jax x 97 ") + f.name, with_flags(rollout(20, 3, 97), f.flags));
    add(std::string("rollout (20,3) jax x 97 3 episodes ") + f.name, with_flags(episodes(rollout(20, 3, 97), 3), f.flags));
    add(std::string("rollout (50,4) jax x 97 3 episodes ") + f.name, with_flags(episodes(rollout(50, 4, 97), 3), f.flags));
    add(std::string("generate (20,3) ") + f.name, with_flags(generate(20, 3), f.flags));
    add(std::string("zeillinger (20,3) ") + f.name, with_flags(zeillinger(20, 3), f.flags));
  }
  add("step (20,3) jax take_actions TWO_LANES x 98368", with_flags(step(20, 3, kTake, HK_SEM_JAX, HK_F32, HK_I32, 98368), HK_FLAG_FORCE_TWO_LANES));
  add("step (20,3) torch ONE_LANE|TWO_LANES x 98368",
      with_flags(step(20, 3, kTake, HK_SEM_TORCH, HK_F32, HK_I32, 98368), HK_FLAG_FORCE_ONE_LANE | HK_FLAG_FORCE_TWO_LANES));
  // shapes without a specialisation, f64
  add("step (7,3) jax take_actions", step(7, 3, kTake, HK_SEM_JAX));
  add("step (7,3) list", step(7, 3, kTake, HK_SEM_LIST));
  add("step (9,7) jax take_actions", step(9, 7, kTake, HK_SEM_JAX));
  add("step (70,3) jax take_actions", step(70, 3, kTake, HK_SEM_JAX));
  add("step (20,3) f64", step(20, 3, kTake, HK_SEM_JAX), HK_F64);
  add("step (2000,30) f64: no kernel holds a game", step(2000, 30, kTake, HK_SEM_JAX), HK_F64);

  // ---- rollouts: the compiled configurations -----------------------------------------------------------------------
  for (const int b : {97, 98368}) {  // (four lanes per game, then -- past every crossover -- one)
    const std::string at = " x " + std::to_string(b);
    add("rollout (20,3) jax" + at, rollout(20, 3, b));
    add("rollout (20,3) torch" + at, rollout(20, 3, b, 20, kTorch));
    add("rollout (20,3) list" + at, rollout(20, 3, b, 20, HK_SEM_LIST));
    add("rollout (20,3) jax rescaled: run-time configured" + at, rollout(20, 3, b, 20, HK_SEM_JAX, kTake | HK_STAGE_RESCALE));
    add("rollout (20,3) jax Zeillinger's host" + at, zeil_host(rollout(20, 3, b)));
    add("rollout (20,3) jax small records" + at, small_recs(rollout(20, 3, b)));
    add("rollout (20,3) torch small records" + at, small_recs(rollout(20, 3, b, 20, kTorch)));
    add("rollout (20,3) jax observations" + at, observations(rollout(20, 3, b)));
    add("rollout (20,3) torch observations" + at, observations(rollout(20, 3, b, 20, kTorch)));
    add("rollout (20,3) jax Zeillinger's host small records" + at, small_recs(zeil_host(rollout(20, 3, b))));
  }
  for (const int b : {97, 65536}) {  // (two lanes per game at 65 536)
    const std::string at = " TWO_LANES x " + std::to_string(b);
    add("rollout (20,3) jax" + at, with_flags(rollout(20, 3, b), HK_FLAG_FORCE_TWO_LANES));
    add("rollout (20,3) torch" + at, with_flags(rollout(20, 3, b, 20, kTorch), HK_FLAG_FORCE_TWO_LANES));
    add("rollout (20,3) list" + at, with_flags(rollout(20, 3, b, 20, HK_SEM_LIST), HK_FLAG_FORCE_TWO_LANES));
    add("rollout (20,3) jax Zeillinger's host" + at, with_flags(zeil_host(rollout(20, 3, b)), HK_FLAG_FORCE_TWO_LANES));
    add("rollout (20,3) jax small records" + at, with_flags(small_recs(rollout(20, 3, b)), HK_FLAG_FORCE_TWO_LANES));
    add("rollout (20,3) torch small records" + at, with_flags(small_recs(rollout(20, 3, b, 20, kTorch)), HK_FLAG_FORCE_TWO_LANES));
    add("rollout (20,3) jax observations" + at, with_flags(observations(rollout(20, 3, b)), HK_FLAG_FORCE_TWO_LANES));
  }
  add("rollout (20,3) jax small records x 65536: the two-lane kernel takes them", small_recs(rollout(20, 3, 65536)));
  add("rollout (20,3) jax observations x 65536", observations(rollout(20, 3, 65536)));
  add("rollout (50,4) jax x 97", rollout(50, 4, 97));
  add("rollout (50,4) jax x 262144", rollout(50, 4, 262144));
  add("rollout (50,4) jax Zeillinger's host x 97", zeil_host(rollout(50, 4, 97)));
  add("rollout (50,4) list x 97", rollout(50, 4, 97, 20, HK_SEM_LIST));
  add("rollout (50,4) jax observations x 97", observations(rollout(50, 4, 97)));
  add("rollout (50,4) jax Zeillinger's host observations x 97", observations(zeil_host(rollout(50, 4, 97))));
  add("rollout (50,4) jax TWO_LANES x 97", with_flags(rollout(50, 4, 97), HK_FLAG_FORCE_TWO_LANES));
  add("rollout (16,3) jax x 97", rollout(16, 3, 97));
  add("rollout (16,3) jax x 98368", rollout(16, 3, 98368));
  add("rollout (20,4) jax x 98368: m*d > 64 keeps two lanes", rollout(20, 4, 98368));
  add("rollout (7,3) jax x 97", rollout(7, 3, 97));
  add("rollout (7,3) jax Zeillinger's host x 97", zeil_host(rollout(7, 3, 97)));
  add("rollout (9,7) jax x 97", rollout(9, 7, 97));
  add("rollout (20,3) f64 x 97", rollout(20, 3, 97), HK_F64);
  add("rollout (20,3) jax misaligned x 97", misaligned(rollout(20, 3, 97)));
  add("rollout (20,3) jax strided x 97", strided(rollout(20, 3, 97)));
  add("rollout (50,4) jax strided x 97", strided(rollout(50, 4, 97)));
  add("rollout (20,3) jax misaligned observations x 97", [] {
    Params p = observations(rollout(20, 3, 97));
    p.obs_out = (char*)p.obs_out + 4;
    return p;
  }());
  // the crossovers of pick (1024 SIMDs)
  add("rollout (20,3) jax x 32768: two four-lane waves per SIMD", rollout(20, 3, 32768));
  add("rollout (20,3) jax x 32784", rollout(20, 3, 32784));
  add("rollout (20,3) jax 6 steps x 65536: four waves per SIMD", rollout(20, 3, 65536, 6));
  add("rollout (20,3) jax 7 steps x 65536", rollout(20, 3, 65536, 7));
  add("rollout (20,3) jax 6 steps x 65552", rollout(20, 3, 65552, 6));
  add("rollout (20,3) jax x 98304: one and a half one-lane waves per SIMD", rollout(20, 3, 98304));
  add("rollout (20,3) jax x 98368", rollout(20, 3, 98368));
  add("rollout (20,3) jax small records x 98304", small_recs(rollout(20, 3, 98304)));
  add("rollout (20,3) jax FOUR_LANES x 98368", with_flags(rollout(20, 3, 98368), HK_FLAG_FORCE_FOUR_LANES));
  // generated initial states (GEN) and episodes back to back (EPI)
  for (const int b : {97, 65552}) {
    const std::string at = " x " + std::to_string(b);
    add("rollout (20,3) jax generated" + at, generated(rollout(20, 3, b)));
    add("rollout (20,3) torch generated" + at, generated(rollout(20, 3, b, 20, kTorch)));
    add("rollout (20,3) jax rescaled generated" + at, generated(rollout(20, 3, b, 20, HK_SEM_JAX, kTake | HK_STAGE_RESCALE)));
    add("rollout (20,3) jax Zeillinger's host generated" + at, generated(zeil_host(rollout(20, 3, b))));
    add("rollout (20,3) jax generated 3 episodes" + at, generated(rollout(20, 3, b), 3));
    add("rollout (20,3) jax 3 episodes" + at, episodes(rollout(20, 3, b), 3));
    add("rollout (20,3) torch 3 episodes" + at, episodes(rollout(20, 3, b, 20, kTorch), 3));
    add("rollout (20,3) list 3 episodes" + at, episodes(rollout(20, 3, b, 20, HK_SEM_LIST), 3));
    add("rollout (20,3) jax rescaled 3 episodes" + at, episodes(rollout(20, 3, b, 20, HK_SEM_JAX, kTake | HK_STAGE_RESCALE), 3));
    add("rollout (20,3) jax Zeillinger's host 3 episodes" + at, episodes(zeil_host(rollout(20, 3, b)), 3));
    add("rollout (50,4) jax generated" + at, generated(rollout(50, 4, b)));
    add("rollout (50,4) jax Zeillinger's host generated" + at, generated(zeil_host(rollout(50, 4, b))));
    add("rollout (50,4) jax 3 episodes" + at, episodes(rollout(50, 4, b), 3));
    add("rollout (50,4) jax Zeillinger's host 3 episodes" + at, episodes(zeil_host(rollout(50, 4, b)), 3));
  }
  add("rollout (20,3) jax 3 episodes x 65536: four waves per SIMD resident", episodes(rollout(20, 3, 65536), 3));
  add("rollout (20,3) jax generated padding 0", [] {
    Params p = generated(rollout(20, 3, 97));
    p.pad = 0.0;
    return p;
  }());
  add("rollout (20,3) jax generated misaligned", misaligned(generated(rollout(20, 3, 97))));
  add("rollout (16,3) jax generated x 97", generated(rollout(16, 3, 97)));
  add("rollout (7,3) jax generated x 97", generated(rollout(7, 3, 97)));

  // ---- the generator and the two binning entries ----------------------------------------------------------------------
  add("generate (20,3)", generate(20, 3));
  add("generate (50,4) newton", generate(50, 4, HK_STAGE_NEWTON));
  add("generate (20,3) list newton", generate(20, 3, HK_STAGE_NEWTON, HK_SEM_LIST));
  add("generate (20,3) list", generate(20, 3, 0, HK_SEM_LIST));
  add("generate (20,3) padding 0", [] {
    Params p = generate(20, 3);
    p.pad = 0.0;
    return p;
  }());
  add("generate (20,3) misaligned", misaligned(generate(20, 3)));
  add("generate (16,3)", generate(16, 3));
  add("generate (7,3)", generate(7, 3));
  add("generate (20,3) f64", generate(20, 3), HK_F64);

  // ---- hk_zeillinger ------------------------------------------------------------------------------------------------------
  add("zeillinger (20,3) jax", zeillinger(20, 3));
  add("zeillinger (50,4) jax", zeillinger(50, 4));
  add("zeillinger (20,3) list", zeillinger(20, 3, HK_SEM_LIST));
  add("zeillinger (50,4) list", zeillinger(50, 4, HK_SEM_LIST));
  add("zeillinger (20,3) jax misaligned", misaligned(zeillinger(20, 3)));
  add("zeillinger (20,3) jax strided", strided(zeillinger(20, 3)));
  add("zeillinger (16,3) jax", zeillinger(16, 3));
  add("zeillinger (7,3) jax", zeillinger(7, 3));
  add("zeillinger (9,7) jax", zeillinger(9, 7));
  add("zeillinger (20,3) f64", zeillinger(20, 3), HK_F64);
}

// hk_generate_points_binned / hk_bin_by_live_rows: the generator's selection decides, the binning kernel has its own grid
void binning() {
  for (const auto& s : {std::pair<int, int>{10, 3}, {20, 3}, {20, 4}, {50, 4}, {16, 3}}) {
    const int group = quadbin_group_games(s.first, s.second, HK_F32);
    const Params p = generate(s.first, s.second, 0, HK_SEM_JAX, 1000);
    printf("binned (%d,%d) x 1000 -> group_games=%d / generate_points_binned: %s / grid=%lld\n", s.first, s.second, group,
           pick(p, HK_F32) == Kernel::QuadGen ? "quadbin gen=1" : "unsupported", (long long)(group ? workgroups(1000, group) : 0));
  }
  printf("binned (20,3) f64 -> group_games=%d\n", quadbin_group_games(20, 3, HK_F64));
  printf("binned (20,3) x 1000 ONE_LANE -> generate_points_binned: %s\n",
         pick(with_flags(generate(20, 3, 0, HK_SEM_JAX, 1000), HK_FLAG_FORCE_ONE_LANE), HK_F32) == Kernel::QuadGen ? "quadbin gen=1"
                                                                                                                     : "unsupported");
}

}  // namespace

int main() {
  table();
  for (const Row& r : rows) report(r);
  binning();
  printf("%d rows, %d failures\n", (int)rows.size(), failures);
  return failures ? 1 : 0;
}
