// Kernel selection (host only): which kernel family serves a request, and the grid of that launch.
//
// `pick` alone decides the family (DESIGN.md §5 has the table).  The *_supported predicates of the family headers say
// what a kernel CAN serve (shapes, alignment, semantics, mode, records, and that its *_variant names an instantiation);
// pick adds the testing flags and the measured crossovers, and everything that launches or sizes a launch asks it.
// Which instantiation of the family runs is the family's *_variant, on which grid its *_grid: the predicate, the launcher
// and planned_grid / count_slots below read the same two functions.
#pragma once

#include <algorithm>

#include "hk_fast_kernel.h"
#include "hk_duo_kernel.h"
#include "hk_quad_kernel.h"
#include "hk_quadroll_kernel.h"
#include "hk_quadgen_kernel.h"
#include "hk_quadbin_kernel.h"
#include "hk_team_kernel.h"
#include "hk_generic_kernel.h"

namespace hk {

// LDS geometry of the generic kernel: odd per-game stride, as many games per wave as fit
inline int plan_generic(Params& prm, int dtype) {
  const int n = prm.m * prm.d;
  int stride = n + prm.d;
  stride |= 1;
  const int64_t per_game = (int64_t)stride * (int64_t)elem_size(dtype);
  int gpb = kWave;
  while (gpb > 1 && per_game * gpb > kMaxLdsBytes) gpb >>= 1;
  if (per_game * gpb > kMaxLdsBytes) return HK_ERR_UNSUPPORTED;
  prm.lds_stride = stride;
  prm.games_per_block = gpb;
  return HK_OK;
}
// (0: the generic kernel cannot hold a game of this shape)
inline int64_t generic_grid(Params prm, int dtype) {
  return plan_generic(prm, dtype) == HK_OK ? workgroups(prm.batch, prm.games_per_block) : 0;
}

enum class Kernel { None, Quad, QuadRoll, QuadRollFused, QuadGen, QuadZeil, Duo, Fast, Team, Generic };

constexpr unsigned kForceFlags = HK_FLAG_FORCE_GENERIC | HK_FLAG_FORCE_TEAM | HK_FLAG_FORCE_ONE_LANE |
                                 HK_FLAG_FORCE_TWO_LANES | HK_FLAG_FORCE_FOUR_LANES;
// read by pick only: cleared before a launcher, or a predicate, sees the request (the compiled configurations compare
// flags)
constexpr unsigned kHostSideFlags = HK_FLAG_FORCE_ONE_LANE | HK_FLAG_FORCE_TWO_LANES | HK_FLAG_FORCE_FOUR_LANES;
inline Params as_launched(Params prm) {
  prm.flags &= ~kHostSideFlags;
  return prm;
}

// a generated / multi-episode rollout the fused kernel declines runs as hk_generate_points into `out` + one plain
// rollout per episode from there
inline Params plain_rollout(Params prm) {
  prm.max_value = 0;
  prm.episodes = 1;
  if (!prm.in) prm.in = prm.out;
  return prm;
}

// hk_zeillinger on the register-resident / team kernels: a step launch without stages and without a state output, whose
// only product is class_out (both variants: the semantics code travels in the flags)
inline Params zeillinger_step(Params prm) {
  prm.mode = kModeStep;
  prm.pad = -1.0;
  return prm;
}

// The testing flags (HK_FLAG_FORCE_*) choose among the kernels that can serve a request, never change its result.
// Precedence:
//   GENERIC   the generic kernel, for every request;
//   TEAM      the team kernel where it applies, else the generic kernel;
//   then, on requests a kernel with a per-shape specialisation can serve:
//   steps     FOUR_LANES: the four-lane kernel wherever it applies (over ONE_LANE / TWO_LANES); else ONE_LANE or TWO_LANES
//             keep it out; then ONE_LANE: one lane per game (over TWO_LANES), TWO_LANES: two lanes wherever they apply;
//   rollouts  ONE_LANE or TWO_LANES keep every four-lane kernel out (over FOUR_LANES), then as steps; FOUR_LANES: the
//             four-lane kernel wherever it applies, the fused one without its residency rule;
//   generator ONE_LANE or TWO_LANES keep the four-lane kernel out; FOUR_LANES changes nothing;
//   hk_zeillinger: TEAM, ONE_LANE or TWO_LANES keep the four-lane kernel out; FOUR_LANES changes nothing.
// Kernel::None: no kernel serves the request.
inline Kernel pick(const Params& prm, int dtype) {
  const unsigned f = prm.flags;
  const bool generic = f & HK_FLAG_FORCE_GENERIC;
  const bool shaped = !(f & (HK_FLAG_FORCE_GENERIC | HK_FLAG_FORCE_TEAM));  // the kernels with per-shape specialisations
  const bool lanes = f & (HK_FLAG_FORCE_ONE_LANE | HK_FLAG_FORCE_TWO_LANES);
  const bool four = f & HK_FLAG_FORCE_FOUR_LANES;
  const Params req = as_launched(prm);  // what the predicates judge: the request as its launcher will see it
  const int64_t quad_waves = workgroups(prm.batch, kQuadGames);
  // measured (scripts/probe_duo.py): two lanes per game are ahead while the one-lane kernel (64 games per wave) leaves
  // SIMDs short of a second wave -- up to 1.5 waves per SIMD, 98 304 games on the 1024 SIMDs of an MI355X -- and at any
  // size for the shapes whose one-lane kernel runs one wave per SIMD
  const auto duo_preferred = [&] {
    return (int64_t)prm.batch * 2 <= (int64_t)3 * kWave * device_simds() || prm.m * prm.d > 64;
  };

  if (prm.mode == kModeZeillinger) {
    if (generic) return Kernel::Generic;
    // four lanes per game (the rollout kernel's prologue + its balanced pair loop) wherever that kernel exists: the JAX
    // variant over contiguous 16-B aligned records ((20,3) x 65 536: 21.4 us on one lane per game, (20,4): 37.4)
    if (shaped && !lanes && quadzeil_supported(req, dtype)) return Kernel::QuadZeil;
    const Params step = zeillinger_step(req);
    if (shaped && fast_supported(step, dtype)) return Kernel::Fast;
    return team_supported(step, dtype) ? Kernel::Team : Kernel::Generic;
  }

  if (prm.mode == kModeRollout && (prm.max_value > 0 || prm.episodes > 1)) {
    // generated initial states and / or several episodes as ONE launch (hk_quadroll_kernel.h: GEN, EPI)
    if (shaped && !lanes) {
      if (prm.max_value > 0) {
        if (quadroll_gen_supported(req, dtype)) return Kernel::QuadRollFused;
      } else if (quadroll_episodes_supported(req, dtype)) {
        // episodes from the states in memory: where the waves of the launch are resident all at once (four per SIMD), a
        // wave that starts its next episode early fills what the launch boundary left idle -- (20,3) x 65 536: 16.5 -
        // 17.0 us per episode against 20.8 one launch each; beyond (131 072 games: 37 against 30 us; (50,4) x 262 144:
        // 205 against 172 us, scripts/probe_persistent.py) the per-episode launches of the default kernels stay ahead
        if (four || (prm.m <= 32 && quad_waves <= (int64_t)4 * device_simds())) return Kernel::QuadRollFused;
      }
    }
    return pick(plain_rollout(prm), dtype);
  }

  // hk_step on four lanes per game: everywhere it applies (scripts/probe_crossover.py: ahead of the one-lane kernel
  // from 32 768 to 524 288 games on (10,3), (20,3), (20,4) -- e.g. (20,3): 6.0 vs 11.3 us at 32 768, 44.9 vs 52.7 us at
  // 524 288 -- and of the team kernel on (50,4): 94 vs 113 us at 262 144)
  if (shaped && (four || !lanes) && quad_supported(req, dtype)) return Kernel::Quad;
  // hk_generate_points on four lanes per game: everywhere it applies
  if (shaped && !lanes && quadgen_supported(req, dtype)) return Kernel::QuadGen;
  if (shaped && !lanes && quadroll_supported(req, dtype)) {
    // plain rollouts on four lanes per game: the shapes without a two-lane kernel ((50,4): hk::team_kernel's rollouts
    // before) ... and, on the small shapes, batches of up to two of its waves per SIMD (32 768 games on an MI355X):
    // measured (scripts/probe_rollout_families.py, (20,3)): 14.0 / 15.0 / 17.4 us per 20-step episode at 4 096 / 16 384 /
    // 32 768 games against 16.9 / 18.3 / 18.8 on two lanes per game, 24.5 against 22.2 at 65 536
    if (four || prm.m > 32) return Kernel::QuadRoll;
    // Zeillinger's host: the two-lane kernel is ahead at every size it serves (scripts/probe_zeillinger.py, (20,3):
    // 40.9 against 44.3 us at 32 768 games, 37.4 against 38.5 at 8 192, 44.2 against 57.0 at 65 536)
    if (prm.host_policy != HK_HOST_ZEILLINGER) {
      // Recording rollouts: at every size (scripts/probe_records.py, (20,3), per 20-step episode incl. the counter
      // reduce: 39.8 against 48.6 us with the small records and 69.5 against 82.1 us with the observations at 65 536
      // games, 90.6 / 240 against 114 / 279 us at 262 144) -- except that the small records without observations ride
      // on the two-lane plain rollout too (hk_duo_kernel.h: flush_records): where that is the faster plain kernel it
      // takes them (28.8 -> ~23 us at (20,3) x 65 536)
      if (prm.obs_out) return Kernel::QuadRoll;
      if (small_records(prm) && !(duo_supported(req, dtype) && duo_preferred())) return Kernel::QuadRoll;
      // short rollouts (measured at (20,3) x 65 536, scripts/probe_short_rollouts.py: 1 / 2 / 4 / 6 steps 8.2 / 10.0 /
      // 12.3 / 14.4 us against the two-lane kernel's 9.6 / 11.5 / 13.6 / 15.0; level at 8 steps): the wave's shorter
      // chain counts while the wide first steps are most of the launch
      const int64_t simds = device_simds();
      if (prm.steps <= 6 && quad_waves <= 4 * simds) return Kernel::QuadRoll;
      if (quad_waves <= 2 * simds) return Kernel::QuadRoll;
    }
  }
  // (the step's observation features, and the agent's move as an argmax of its logits, come from the four-lane kernel only)
  if (prm.feat_out || ((prm.stages & HK_STAGE_SHIFT) && prm.axis_dtype == HK_AXIS_MASKED_LOGITS)) return Kernel::None;
  if (shaped && fast_supported(req, dtype)) {
    const bool two = !(f & HK_FLAG_FORCE_ONE_LANE) && duo_supported(req, dtype) &&
                     ((f & HK_FLAG_FORCE_TWO_LANES) || duo_preferred());
    return two ? Kernel::Duo : Kernel::Fast;
  }
  // the team kernel: f32, dim 2..6, <= 64 rows; the generic kernel: anything else (f64, dim > 6, > 64 rows, and the few
  // mode / semantics combinations fast_supported / team_supported decline)
  return !generic && team_supported(req, dtype) ? Kernel::Team : Kernel::Generic;
}

// workgroups of the launch of family `k` for a request (0: not launchable)
inline int64_t grid_of(Kernel k, const Params& prm, int dtype) {
  switch (k) {
    case Kernel::Quad:
    case Kernel::QuadGen: return quad_grid(prm);
    case Kernel::QuadRoll:
    case Kernel::QuadRollFused:
    case Kernel::QuadZeil: return quadroll_grid(prm);
    case Kernel::Duo: return duo_grid(prm);
    case Kernel::Fast: return fast_grid(prm);
    case Kernel::Team: return team_grid(prm);
    case Kernel::Generic: return generic_grid(prm, dtype);
    case Kernel::None: break;
  }
  return 0;
}

// workgroups of the launch that serves this request (0: not launchable)
inline int64_t planned_grid(const Params& prm, int dtype) {
  return prm.batch == 0 ? 0 : grid_of(pick(prm, dtype), prm, dtype);
}

// row length of the finished-game workspace for a geometry: an upper bound of the grids of all the kernel
// variants that may serve it (records, policies and semantics choose among them per launch)
inline int64_t count_slots(const Params& prm, int dtype) {
  if (prm.batch == 0) return 0;
  int64_t slots = planned_grid(prm, dtype);
  if (dtype == HK_F32 && prm.d >= 2 && prm.d <= 6 && prm.m <= kTeam * kTeamSlots) slots = std::max(slots, team_grid(prm));
  if (has_fast_path(prm.m, prm.d, dtype)) slots = std::max(slots, duo_grid(prm));
  return std::max(slots, generic_grid(prm, dtype));
}

}  // namespace hk
