// hk_env_step: one move of every game of a vectorised gym environment (hironaka_amd/gym_env.py HironakaHostEnv.step /
// HironakaAgentEnv.step read per row), and the next episode of a game that stopped (HironakaBase.reset) drawn inside the
// same launch, one game per lane.
//
// The frame is hk_lane_games.h's, with slices of its own (env_lds_stride).  Every stage works in place: the move has no
// use for the state before it, so a slice holds one state, not hk_game_play's two.  The terminal observations of the
// games that stopped leave with a coalesced store of the wave before those lanes draw their next episode into the same
// slices.  HBM traffic: one read and one write of the state, one write of the float32 observation, one of the terminal
// observation for the games that stopped, and the per-game scalars.  Every loop is bounded by m, d or m * d.
#pragma once

#include "hk_lane_games.h"

namespace hk {

struct EnvStepArgs {
  const void* points;
  void* points_out;
  int32_t* class_io;
  int32_t* step_count;
  int32_t* episode;
  const int32_t* action;
  double* reward;
  uint8_t* stopped;
  uint8_t* exceed;
  float* obs_points;
  double* obs_coords;
  float* final_points;
  double* final_coords;
  int32_t* agent_axis;
  uint64_t seed, agent_seed, game_offset, world_games;
  double value_threshold, invalid_move_penalty, threshold_penalty;
  int batch, m, d, agent, max_value, step_threshold, lds_stride, games_per_block;
  uint32_t flags;
};

// LDS elements per lane: the game, the shift coefficients c and sort_compact's row scratch; odd, so that the lanes'
// slices start in different banks.  Half of search_lds_stride's: twice the waves per CU.
inline int env_lds_stride(int m, int d) { return (m * d + 2 * d) | 1; }

template <typename T>
struct EnvSlice {
  T *par, *c, *row;
  __device__ EnvSlice(T* lds, int lane, int stride, int n, int d)
      : par(lds + (size_t)lane * stride), c(par + n), row(c + d) {}
};

// shift along ax by the subset sub (ax < 0: no axis, no shift), [reposition], Newton sorted + compacted, in place.  Agent
// mode comes here without an axis too (a subset of fewer than 2 coordinates): Agent.move runs the stages behind the shift
// all the same.  On a reduced state they change nothing, unless its rescale has merged coordinates that were an ulp
// apart.  Host mode does not come here without a legal axis: HironakaHostEnv.step leaves such a game untouched.
template <typename T>
__device__ inline void env_move(const EnvSlice<T>& s, int m, int d, uint32_t sub, int ax, bool reposition) {
  if (ax >= 0) {
    subset_coeffs(s.c, sub, d);
    shift_game(s.par, m, d, s.c, ax, (T)-1, kListFlags);
  }
  if (reposition) reposition_game(s.par, m, d, (T)-1, kListFlags);
  newton_game(s.par, m, d, (T)-1, kListFlags);
  sort_compact_game(s.par, m, d, (T)-1, s.row);
}

// the rows of p up to its last point: every stage behind this looks at no row beyond (they hold padding, and each
// stage would leave padding there)
template <typename T>
__device__ inline int extent_game(const T* p, int m, int d) {
  int ext = 0;
  for (int i = 0; i < m; ++i) ext = (p[i * d] >= (T)0) ? i + 1 : ext;
  return ext;
}

// HironakaBase.reset on the game gg of the generator's stream (hk_generic_kernel.h kModeGenerate without stages), then
// Newton -> [rescale] -> [Newton, unless HK_ENV_IMPROVE_EFFICIENCY] in both modes: host mode's step(None) is a step
// without a legal axis, which runs no stage.  Returns the number of points: the state is compacted.
template <typename T>
__device__ inline int env_fresh(const EnvStepArgs& a, const EnvSlice<T>& s, uint64_t gg) {
  const int m = a.m, d = a.d, n = m * d;
  const bool sh = gen_short((uint32_t)a.max_value);
  const int per = sh ? 8 : 4;
  for (int e = 0; e < n; e += per) {
    const U4 r = philox4x32((uint32_t)gg, (uint32_t)(gg >> 32), (uint32_t)(e / per), kStreamGenerate, a.seed);
    uint32_t v[8];
    gen_block_values(r, (uint32_t)a.max_value, sh, v);
    for (int q = 0; q < per && e + q < n; ++q) s.par[e + q] = (T)v[q];
  }
  newton_game(s.par, m, d, (T)-1, kListFlags);
  sort_compact_game(s.par, m, d, (T)-1, s.row);
  int np = num_points(s.par, m, d);
  if (a.flags & HK_ENV_SCALE_OBSERVATION) rescale_game(s.par, np, d, (T)-1, kListFlags);
  if (!(a.flags & HK_ENV_IMPROVE_EFFICIENCY)) {
    newton_game(s.par, np, d, (T)-1, kListFlags);
    sort_compact_game(s.par, np, d, (T)-1, s.row);
    np = num_points(s.par, np, d);
  }
  return np;
}

struct EnvOutcome {
  double reward;
  bool stopped, exceed;
};

// HironakaHostEnv.step on one game of m rows (its extent): act is the agent's axis, cls the pending class on entry and
// the new one on return.  Without a legal axis the state is looked at as it is: no shift and no Newton.
template <typename T, int HOST>
__device__ inline EnvOutcome env_host_step(const EnvStepArgs& a, const EnvSlice<T>& s, int m, int act, int& cls) {
  const int d = a.d;
  const int ncls = (1 << d) - d - 1;
  const uint32_t sub = (cls >= 0 && cls < ncls) ? decode_class(cls, d) : 0u;
  const bool legal = act >= 0 && act < d && ((sub >> act) & 1u);
  if (legal) env_move(s, m, d, sub, act, false);
  const bool ended = num_points(s.par, m, d) < 2;
  EnvOutcome o;
  o.reward = legal ? (ended ? 0.0 : 1.0) : a.invalid_move_penalty;
  o.exceed = a.value_threshold > 0.0 && exceeds_game(s.par, m, d, a.value_threshold);
  o.stopped = ended || o.exceed || (!legal && (a.flags & HK_ENV_STOP_AFTER_INVALID));
  cls = -1;
  if (!o.stopped) cls = host_class_any<T, HOST>(s.par, m, d);
  if (cls >= ncls) cls = -1;
  if (a.flags & HK_ENV_SCALE_OBSERVATION) rescale_game(s.par, m, d, (T)-1, kListFlags);
  return o;
}

// HironakaAgentEnv.step on one game of m rows (its extent): mask is the host's subset, gg the game's index in the
// random agent's counter, sc the step counter after its increment; ax returns the agent's axis
template <typename T>
__device__ inline EnvOutcome env_agent_step(const EnvStepArgs& a, const EnvSlice<T>& s, int m, uint32_t mask,
                                            uint64_t gg, int sc, int& ax) {
  const int d = a.d;
  const uint32_t sub = mask & ((1u << d) - 1u);
  const int before = num_points(s.par, m, d);
  ax = -1;
  if (__popc(sub) >= 2) {
    ax = a.agent == HK_AGENT_CHOOSE_FIRST ? __ffs((int)sub) - 1
                                          : random_legal_axis(sub, gg, (uint32_t)(sc - 1), kStreamPlayAgent, a.agent_seed);
  }
  env_move(s, m, d, sub, ax, (a.flags & HK_ENV_AGENT_REPOSITION) != 0);
  const bool ended = num_points(s.par, m, d) < 2;
  EnvOutcome o;
  o.stopped = ended;
  o.reward = 0.0;
  o.exceed = a.value_threshold > 0.0 && exceeds_game(s.par, m, d, a.value_threshold);
  if (a.flags & HK_ENV_STOP_AT_THRESHOLD) {
    const bool trip = o.exceed || sc >= a.step_threshold;
    o.stopped = o.stopped || trip;
    o.reward = o.reward + (trip ? 1.0 : 0.0) * a.threshold_penalty;
  }
  if (a.flags & HK_ENV_SCALE_OBSERVATION) rescale_game(s.par, m, d, (T)-1, kListFlags);
  if (a.flags & HK_ENV_POINT_REDUCTION_REWARD) o.reward = o.reward + (double)(before - num_points(s.par, m, d));
  o.reward = o.reward + (ended ? 1.0 : 0.0);
  return o;
}

// the wave writes the games whose bit is set in `which` as float32: element e of game g from lds[g * S + e]
template <typename T>
__device__ inline void store_obs(const T* lds, float* out, int n, int S, int64_t g0, int ngames, int lane,
                                 unsigned long long which) {
  for (int i = lane; i < ngames * n; i += kWave) {
    const int g = i / n, e = i - g * n;
    if ((which >> g) & 1ull) out[(g0 + g) * n + e] = (float)lds[g * S + e];
  }
}

// HOST: a fixed host's code (host mode), or 0 (agent mode)
template <typename T, int HOST>
__global__ void __launch_bounds__(kWave) env_step_kernel(EnvStepArgs a) {
  extern __shared__ unsigned char hk_env_lds[];
  T* lds = reinterpret_cast<T*>(hk_env_lds);
  const int lane = threadIdx.x;
  const int m = a.m, d = a.d, n = m * d;
  const LaneBlock blk = lane_block(a.batch, a.games_per_block);
  const int64_t g0 = blk.g0;
  const int ngames = blk.ngames;
  const bool reset_all = (a.flags & HK_ENV_RESET_ALL) != 0;
  if (!reset_all) stage_games(lds, a.points, (int64_t)n, n, a.lds_stride, blk, lane);
  __syncthreads();
  const bool active = lane < ngames;
  const int64_t g = g0 + lane;
  const EnvSlice<T> s(lds, lane, a.lds_stride, n, d);
  int sc = 0, ep = 0, cls = -1, ax = -1;
  EnvOutcome o{0.0, false, false};
  if (active) {
    sc = a.step_count[g];
    ep = a.episode[g];
    if (!reset_all) {
      sc += 1;
      const int ext = extent_game(s.par, m, d);
      if constexpr (HOST != 0) {
        cls = a.class_io[g];
        o = env_host_step<T, HOST>(a, s, ext, a.action[g], cls);
      } else {
        const uint64_t gg = a.game_offset + (uint64_t)(int64_t)ep * a.world_games + (uint64_t)g;
        o = env_agent_step<T>(a, s, ext, (uint32_t)a.action[g], gg, sc, ax);
      }
    }
  }
  // the terminal observations leave before the resets overwrite them
  const bool fin = active && !reset_all && o.stopped && (a.flags & HK_ENV_AUTO_RESET);
  const unsigned long long finmask = __ballot(fin);
  if (finmask) {
    __syncthreads();
    if (a.final_points) store_obs(lds, a.final_points, n, a.lds_stride, g0, ngames, lane, finmask);
    __syncthreads();
  }
  if (active) {
    if (fin || reset_all) {
      if (HOST != 0 && fin && a.final_coords)  // a stopped game has no pending subset
        for (int j = 0; j < d; ++j) a.final_coords[g * d + j] = 0.0;
      ep += 1;
      const uint64_t gg = a.game_offset + (uint64_t)(int64_t)ep * a.world_games + (uint64_t)g;
      const int np = env_fresh<T>(a, s, gg);
      sc = 0;
      if constexpr (HOST != 0) {  // _post_reset_update: step(None)
        sc = 1;
        cls = -1;
        (void)env_host_step<T, HOST>(a, s, np, -1, cls);
      }
    }
    a.step_count[g] = sc;
    a.episode[g] = ep;
    a.reward[g] = o.reward;
    a.stopped[g] = o.stopped ? 1 : 0;
    if (a.exceed) a.exceed[g] = o.exceed ? 1 : 0;
    if constexpr (HOST != 0) {
      a.class_io[g] = cls;
      const uint32_t sub = cls >= 0 ? decode_class(cls, d) : 0u;
      for (int j = 0; j < d; ++j) a.obs_coords[g * d + j] = ((sub >> j) & 1u) ? 1.0 : 0.0;
    } else if (a.agent_axis) {
      a.agent_axis[g] = ax;
    }
  }
  __syncthreads();
  unstage_games(lds, a.points_out, (int64_t)n, n, a.lds_stride, blk, lane);
  store_obs(lds, a.obs_points, n, a.lds_stride, g0, ngames, lane, ~0ull);
}

}  // namespace hk
