// C ABI of hk_game_play (include/hironaka_hip.h, an addition within ABI 6): argument validation and launch of
// hk::game_play_kernel.  No allocation, no synchronisation; every status is decided before the launch.
#include "hk_game_play_kernel.h"

using namespace hk;

extern "C" {

int hk_game_play(const hk_game_play_desc* q, void* stream) {
  if (!q) return HK_ERR_NULL;
  if (q->dtype != HK_F32 && q->dtype != HK_F64) return HK_ERR_UNSUPPORTED;
  if (q->batch < 0 || q->max_points < 1 || q->dim < 2 || q->max_steps < 0) return HK_ERR_SHAPE;
  if (q->max_points > kFixedHostMaxPoints || q->dim > kLaneGameMaxDim) return HK_ERR_UNSUPPORTED;
  if (!fixed_host(q->host) && q->host != HK_PLAY_HOST_FORCED) return HK_ERR_UNSUPPORTED;
  if (q->agent != HK_AGENT_RANDOM_LEGAL && q->agent != HK_AGENT_CHOOSE_FIRST && q->agent != HK_AGENT_CHOOSE_LAST)
    return HK_ERR_UNSUPPORTED;
  const uint32_t known = HK_PLAY_REPOSITION | HK_PLAY_RESCALE | HK_PLAY_REDUCE_ROOT | HK_PLAY_RESCALE_ROOT;
  if (q->flags & ~known) return HK_ERR_UNSUPPORTED;
  if (q->value_threshold != q->value_threshold) return HK_ERR_UNSUPPORTED;
  if (q->batch == 0) return HK_OK;
  if (!q->points_in || !q->points_out || !q->length_out || !q->outcome_out) return HK_ERR_NULL;
  if (q->host == HK_PLAY_HOST_FORCED && q->max_steps > 0 && !q->class_in) return HK_ERR_NULL;
  const int64_t n = (int64_t)q->max_points * q->dim;
  if (q->in_stride < n || q->out_stride < n) return HK_ERR_SHAPE;
  if (q->points_in == q->points_out && q->in_stride != q->out_stride) return HK_ERR_SHAPE;
  const size_t es = elem_size(q->dtype);
  // a workgroup's write-back must not meet another's staging read: other than in place, the two spans do not overlap
  const uint64_t in_bytes = span_bytes(q->batch, q->in_stride, n, es), out_bytes = span_bytes(q->batch, q->out_stride, n, es);
  if (!in_bytes || !out_bytes) return HK_ERR_SHAPE;  // a span beyond 2^63 bytes
  if (q->points_in != q->points_out && overlap(q->points_in, in_bytes, q->points_out, out_bytes)) return HK_ERR_SHAPE;
  if (!all_aligned({q->class_in, q->axis_in, q->class_out, q->axis_out, q->length_out, q->outcome_out}, 4) ||
      !all_aligned({q->points_in, q->points_out}, es))
    return HK_ERR_ALIGN;
  GamePlayArgs a{};
  a.points = q->points_in;
  a.points_out = q->points_out;
  a.class_in = q->class_in;
  a.axis_in = q->axis_in;
  a.class_out = q->class_out;
  a.axis_out = q->axis_out;
  a.length_out = q->length_out;
  a.outcome_out = q->outcome_out;
  a.in_stride = q->in_stride;
  a.out_stride = q->out_stride;
  a.seed = q->seed;
  a.game_offset = q->game_offset;
  a.value_threshold = q->value_threshold;
  a.step_offset = q->step_offset;
  a.batch = q->batch;
  a.m = q->max_points;
  a.d = q->dim;
  a.max_steps = q->max_steps;
  a.agent = q->agent;
  a.reposition = (q->flags & HK_PLAY_REPOSITION) ? 1 : 0;
  a.rescale = (q->flags & HK_PLAY_RESCALE) ? 1 : 0;
  a.reduce_root = (q->flags & HK_PLAY_REDUCE_ROOT) ? 1 : 0;
  a.rescale_root = (q->flags & HK_PLAY_RESCALE_ROOT) ? 1 : 0;
  a.lds_stride = search_lds_stride(a.m, a.d);
  const LaneGeometry geo = lane_geometry(a.lds_stride, es, a.batch);
  a.games_per_block = geo.per_block;
  return with_fixed_host_or(q->dtype, q->host, std::integral_constant<int, HK_PLAY_HOST_FORCED>(), [&](auto t, auto h) {
    return launch_kernel(game_play_kernel<decltype(t), h>, dim3(geo.grid), dim3(kWave), geo.lds, (hipStream_t)stream, a);
  });
}

}  // extern "C"
