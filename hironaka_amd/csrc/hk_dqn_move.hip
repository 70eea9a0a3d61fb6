// C ABI of hk_dqn_host_move and hk_dqn_agent_move (include/hironaka_hip_dqn_move.h, additions within ABI 6): argument
// validation and launch of hk::dqn_host_move_kernel and hk::dqn_agent_move_kernel.  No allocation, no synchronisation;
// every status is decided before the launch.
#include "hk_dqn_move_kernel.h"

using namespace hk;

namespace {
bool real_dtype(int dtype) { return dtype == HK_F32 || dtype == HK_F64; }
}  // namespace

extern "C" {

int hk_dqn_host_move(const hk_dqn_host_move_desc* q, void* stream) {
  if (!q) return HK_ERR_NULL;
  if (!real_dtype(q->q_dtype) || !real_dtype(q->coords_dtype)) return HK_ERR_UNSUPPORTED;
  if (q->batch < 0 || q->dim < 2) return HK_ERR_SHAPE;
  if (q->dim > kDqnMoveMaxDim) return HK_ERR_UNSUPPORTED;
  const int classes = (1 << q->dim) - q->dim - 1;
  if (q->q_stride < classes) return HK_ERR_SHAPE;
  if (q->batch == 0) return HK_OK;
  if (!q->q || !q->class_out || !q->coords_out) return HK_ERR_NULL;
  const size_t qs = elem_size(q->q_dtype), cs = elem_size(q->coords_dtype);
  if (!all_aligned({q->class_out, q->counts}, 4) || !aligned(q->q, qs) || !aligned(q->coords_out, cs)) return HK_ERR_ALIGN;
  const uint64_t q_bytes = span_bytes(q->batch, q->q_stride, classes, qs);
  if (!q_bytes) return HK_ERR_SHAPE;
  // what is written while other workgroups still read: no written range shares a byte with another range
  const uint64_t games = (uint64_t)q->batch;
  const void* written[3] = {q->class_out, q->coords_out, q->counts};
  const uint64_t written_bytes[3] = {games * 4u, games * (uint64_t)q->dim * cs, (uint64_t)classes * 4u};
  for (int i = 0; i < 3; ++i) {
    for (int j = i + 1; j < 3; ++j)
      if (overlap(written[i], written_bytes[i], written[j], written_bytes[j])) return HK_ERR_SHAPE;
    if (overlap(written[i], written_bytes[i], q->q, q_bytes) || overlap(written[i], written_bytes[i], q->prev_done, games))
      return HK_ERR_SHAPE;
  }
  DqnHostMoveArgs a{q->q, q->q_stride, q->class_out, q->coords_out, q->prev_done, q->counts, q->batch, q->dim, classes};
  return with_dqn_move_types(q->q_dtype, q->coords_dtype, [&](auto qt, auto ct) {
    return launch_kernel(dqn_host_move_kernel<decltype(qt), decltype(ct)>, dim3((unsigned)workgroups(a.batch, kDqnHostBlock)),
                         dim3(kDqnHostBlock), 0, (hipStream_t)stream, a);
  });
}

int hk_dqn_agent_move(const hk_dqn_agent_move_desc* q, void* stream) {
  if (!q) return HK_ERR_NULL;
  if (!real_dtype(q->dtype) || !real_dtype(q->q_dtype)) return HK_ERR_UNSUPPORTED;
  if (q->batch < 0 || q->max_points < 1 || q->dim < 2) return HK_ERR_SHAPE;
  if (q->max_points > kFixedHostMaxPoints || q->dim > kDqnMoveMaxDim) return HK_ERR_UNSUPPORTED;
  if (q->flags & ~(HK_DQN_MOVE_MASKED | HK_DQN_MOVE_RESCALE)) return HK_ERR_UNSUPPORTED;
  if (!(q->padding_value < 0.0)) return HK_ERR_UNSUPPORTED;  // a NaN included
  if (q->q_stride < q->dim) return HK_ERR_SHAPE;
  if (q->batch == 0) return HK_OK;
  if (!q->points || !q->q || !q->class_id || !q->axis_out || !q->features_out || !q->done_out || !q->lengths)
    return HK_ERR_NULL;
  const size_t es = elem_size(q->dtype), qs = elem_size(q->q_dtype);
  if (!all_aligned({q->class_id, q->axis_out, q->lengths, q->counts}, 4) || !all_aligned({q->points, q->features_out}, es) ||
      !aligned(q->q, qs))
    return HK_ERR_ALIGN;
  const int64_t n = (int64_t)q->max_points * q->dim;
  const uint64_t q_bytes = span_bytes(q->batch, q->q_stride, q->dim, qs);
  if (!q_bytes) return HK_ERR_SHAPE;
  // what is written while other workgroups still read: no written range shares a byte with another range
  const uint64_t games = (uint64_t)q->batch;
  const uint64_t state = span_bytes(q->batch, n, n, es);  // dense records of the sizes accepted above: never too large
  const void* written[6] = {q->points, q->features_out, q->axis_out, q->done_out, q->lengths, q->counts};
  const uint64_t written_bytes[6] = {state, state, games * 4u, games, games * 4u, (uint64_t)q->dim * 4u};
  for (int i = 0; i < 6; ++i) {
    for (int j = i + 1; j < 6; ++j)
      if (overlap(written[i], written_bytes[i], written[j], written_bytes[j])) return HK_ERR_SHAPE;
    if (overlap(written[i], written_bytes[i], q->q, q_bytes) || overlap(written[i], written_bytes[i], q->class_id, games * 4u))
      return HK_ERR_SHAPE;
  }
  DqnAgentMoveArgs a{};
  a.points = q->points;
  a.q = q->q;
  a.q_stride = q->q_stride;
  a.class_id = q->class_id;
  a.axis_out = q->axis_out;
  a.features_out = q->features_out;
  a.done_out = q->done_out;
  a.lengths = q->lengths;
  a.counts = q->counts;
  a.pad = q->padding_value;
  a.batch = q->batch;
  a.m = q->max_points;
  a.d = q->dim;
  a.masked = (q->flags & HK_DQN_MOVE_MASKED) ? 1 : 0;
  a.rescale = (q->flags & HK_DQN_MOVE_RESCALE) ? 1 : 0;
  a.lds_stride = search_lds_stride(a.m, a.d);
  const LaneGeometry geo = lane_geometry(a.lds_stride, es, a.batch);
  a.games_per_block = geo.per_block;
  return with_dqn_move_types(q->dtype, q->q_dtype, [&](auto t, auto qt) {
    return launch_kernel(dqn_agent_move_kernel<decltype(t), decltype(qt)>, dim3(geo.grid), dim3(kWave), geo.lds,
                         (hipStream_t)stream, a);
  });
}

}  // extern "C"
