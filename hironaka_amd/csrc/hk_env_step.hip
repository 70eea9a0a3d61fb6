// C ABI of hk_env_step (include/hironaka_hip_env.h, an addition within ABI 6): argument validation and launch of
// hk::env_step_kernel.  No allocation, no synchronisation; every status is decided before the launch.
#include "hk_env_step_kernel.h"

using namespace hk;

extern "C" {

int hk_env_step(const hk_env_step_desc* q, void* stream) {
  if (!q) return HK_ERR_NULL;
  if (q->dtype != HK_F32 && q->dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (q->mode != HK_ENV_MODE_HOST && q->mode != HK_ENV_MODE_AGENT) return HK_ERR_UNSUPPORTED;
  if (q->batch < 0 || q->max_points < 1 || q->dim < 2) return HK_ERR_SHAPE;
  if (q->max_points > kFixedHostMaxPoints || q->dim > kLaneGameMaxDim) return HK_ERR_UNSUPPORTED;
  const bool host_mode = q->mode == HK_ENV_MODE_HOST;
  if (host_mode && !fixed_host(q->host)) return HK_ERR_UNSUPPORTED;
  if (!host_mode && q->agent != HK_AGENT_RANDOM_LEGAL && q->agent != HK_AGENT_CHOOSE_FIRST) return HK_ERR_UNSUPPORTED;
  const uint32_t known = HK_ENV_SCALE_OBSERVATION | HK_ENV_STOP_AFTER_INVALID | HK_ENV_STOP_AT_THRESHOLD |
                         HK_ENV_POINT_REDUCTION_REWARD | HK_ENV_IMPROVE_EFFICIENCY | HK_ENV_AGENT_REPOSITION |
                         HK_ENV_AUTO_RESET | HK_ENV_RESET_ALL;
  if (q->flags & ~known) return HK_ERR_UNSUPPORTED;
  if (q->value_threshold != q->value_threshold || q->invalid_move_penalty != q->invalid_move_penalty ||
      q->threshold_penalty != q->threshold_penalty)
    return HK_ERR_UNSUPPORTED;
  const bool reset_all = (q->flags & HK_ENV_RESET_ALL) != 0;
  if ((q->flags & (HK_ENV_AUTO_RESET | HK_ENV_RESET_ALL)) && q->max_value < 1) return HK_ERR_SHAPE;
  if (q->batch == 0) return HK_OK;
  if (!q->points_out || !q->step_count || !q->episode || !q->reward || !q->stopped || !q->obs_points) return HK_ERR_NULL;
  if (!reset_all && (!q->points_in || !q->action)) return HK_ERR_NULL;
  if (host_mode && (!q->class_io || !q->obs_coords)) return HK_ERR_NULL;
  const size_t es = elem_size(q->dtype);
  const int64_t n = (int64_t)q->max_points * q->dim;
  // a workgroup's write-back must not meet another's staging read: other than in place, the two spans do not overlap
  const uint64_t bytes = span_bytes(q->batch, n, n, es);  // dense records of the sizes accepted above: never too large
  if (!reset_all && q->points_in != q->points_out && overlap(q->points_in, bytes, q->points_out, bytes)) return HK_ERR_SHAPE;
  if (!all_aligned({q->class_io, q->step_count, q->episode, q->action, q->obs_points, q->final_points, q->agent_axis}, 4) ||
      !all_aligned({q->reward, q->obs_coords, q->final_coords}, 8) || !all_aligned({q->points_in, q->points_out}, es))
    return HK_ERR_ALIGN;
  EnvStepArgs a{};
  a.points = q->points_in;
  a.points_out = q->points_out;
  a.class_io = q->class_io;
  a.step_count = q->step_count;
  a.episode = q->episode;
  a.action = q->action;
  a.reward = q->reward;
  a.stopped = q->stopped;
  a.exceed = q->exceed;
  a.obs_points = q->obs_points;
  a.obs_coords = q->obs_coords;
  a.final_points = q->final_points;
  a.final_coords = q->final_coords;
  a.agent_axis = q->agent_axis;
  a.seed = q->seed;
  a.agent_seed = q->agent_seed;
  a.game_offset = q->game_offset;
  a.world_games = q->world_games;
  a.value_threshold = q->value_threshold;
  a.invalid_move_penalty = q->invalid_move_penalty;
  a.threshold_penalty = q->threshold_penalty;
  a.batch = q->batch;
  a.m = q->max_points;
  a.d = q->dim;
  a.agent = q->agent;
  a.max_value = q->max_value;
  a.step_threshold = q->step_threshold;
  a.flags = q->flags;
  a.lds_stride = env_lds_stride(a.m, a.d);
  const LaneGeometry geo = lane_geometry(a.lds_stride, es, a.batch);
  a.games_per_block = geo.per_block;
  // agent mode: no host, the kernel's HOST is 0
  return with_fixed_host_or(q->dtype, host_mode ? q->host : 0, std::integral_constant<int, 0>(), [&](auto t, auto h) {
    return launch_kernel(env_step_kernel<decltype(t), h>, dim3(geo.grid), dim3(kWave), geo.lds, (hipStream_t)stream, a);
  });
}

}  // extern "C"
