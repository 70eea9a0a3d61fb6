/*
 * hironaka_hip_dqn_move.h -- one greedy move of the DQN trainers' evaluation (FusedGame.host_move / agent_move with
 * exploration off) as two launches around the two network launches: hk_dqn_host_move and hk_dqn_agent_move, additions
 * within ABI 6 that a consumer detects by their symbols.  Part of the C ABI of hironaka_hip.h, which includes this file;
 * HK_F32 / HK_F64 and the status codes are defined there.  The entry points have no counterpart in the CPU oracle: the
 * Python binding lists them in hironaka_amd/_abi.py DQN_MOVE_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 */
#ifndef HIRONAKA_HIP_DQN_MOVE_H
#define HIRONAKA_HIP_DQN_MOVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the argmax rule of both kernels ----
 * The index of a row's maximum is the first index that holds it; a NaN beats every number and the first NaN wins
 * (torch.argmax).  -0.0 and 0.0 are equal.
 *
 * ---- hk_dqn_host_move: the host's class from its Q-values, and the subset as a 0/1 vector ----
 * Per game b: class_out[b] = argmax of q[b * q_stride + 0 .. classes), classes = 2^dim - dim - 1; coords_out[b] is the
 * subset of that class as dim values 0 / 1 of coords_dtype (bit j of the (class)-th integer >= 3 that is no power of
 * two <-> coordinate j: hk_decode_host_class).  With prev_done and counts both given: counts[class_out[b]] += 1 for
 * every game with prev_done[b] == 0 (integer atomics: the result does not depend on the order).  With either NULL
 * nothing is counted.
 * dim 2..7, q_dtype and coords_dtype HK_F32 / HK_F64, q_stride >= classes, batch >= 0. */
typedef struct hk_dqn_host_move_desc {
  const void* q;            /* [batch] rows of `classes` values, q_stride elements apart                            */
  int64_t q_stride;
  int32_t* class_out;       /* [batch]                                                                              */
  void* coords_out;         /* [batch, dim] of coords_dtype                                                         */
  const uint8_t* prev_done; /* [batch] or NULL: games that take no part in counts                                   */
  int32_t* counts;          /* [classes] or NULL, added to                                                          */
  int32_t batch;
  int32_t dim;
  int32_t q_dtype;
  int32_t coords_dtype;
} hk_dqn_host_move_desc;
int hk_dqn_host_move(const hk_dqn_host_move_desc* desc, void* stream);

/* ---- hk_dqn_agent_move: the agent's axis from its Q-values, the move, and the next observation ----
 * One game per lane.  Per game b, with sub the subset of class_id[b] (clamped into [0, classes) as hk_step clamps):
 *   axis: HK_DQN_MOVE_MASKED: argmax over k of q[k] * mask[k] + (1 - mask[k]) * lowest, mask[k] = 1 on sub and 0
 *   elsewhere, lowest = the most negative finite value of q_dtype, every operation rounded on its own in q_dtype (so an
 *   infinite q outside sub gives NaN, which wins).  Otherwise the plain argmax of q[0 .. dim).
 *   The move, in torch semantics with HK_FLAG_AXIS_NOOP_IF_INVALID | HK_FLAG_IGNORE_ENDED: shift along axis by sub (no
 *   shift when the axis lies outside sub or the game has fewer than 2 points), Newton polytope, rescale with
 *   HK_DQN_MOVE_RESCALE -- the state hk_step leaves for these stages and flags.  points is updated in place.
 *   axis_out[b] = axis; done_out[b] = the new state has fewer than 2 points; features_out[b] = the new state's rows by
 *   coordinate 0, descending, ties in row order (hk_get_features_torch); for a game that had at least 2 points before
 *   the move: lengths[b] += 1 and, where counts is given, counts[axis] += 1 (integer atomics).
 * dim 2..7, max_points 1..64, dtype and q_dtype HK_F32 / HK_F64, q_stride >= dim, padding_value negative (a state's
 * unavailable entries, as in hk_step), batch >= 0.  features_out must not share memory with points. */
#define HK_DQN_MOVE_MASKED 1u  /* hk_dqn_agent_move_desc.flags */
#define HK_DQN_MOVE_RESCALE 2u
typedef struct hk_dqn_agent_move_desc {
  void* points;            /* [batch, max_points, dim] of dtype, in and out                                         */
  const void* q;           /* [batch] rows of dim values of q_dtype, q_stride elements apart                        */
  int64_t q_stride;
  const int32_t* class_id; /* [batch]                                                                               */
  int32_t* axis_out;       /* [batch]                                                                               */
  void* features_out;      /* [batch, max_points, dim] of dtype                                                     */
  uint8_t* done_out;       /* [batch]                                                                               */
  int32_t* lengths;        /* [batch] in and out                                                                    */
  int32_t* counts;         /* [dim] or NULL, added to                                                               */
  double padding_value;
  int32_t batch;
  int32_t max_points;
  int32_t dim;
  int32_t dtype;
  int32_t q_dtype;
  uint32_t flags;
} hk_dqn_agent_move_desc;
int hk_dqn_agent_move(const hk_dqn_agent_move_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_DQN_MOVE_H */
