/*
 * hironaka_hip_play.h -- whole games of the plain Hironaka game (hk_game_play, an addition within ABI 6 that a consumer
 * detects by its symbol), part of the C ABI of hironaka_hip.h, which includes this file; the HK_HOST_* and HK_AGENT_*
 * codes, HK_F32 / HK_F64 and the status codes are defined there.  Like hk_host_select (hironaka_hip_hosts.h) the entry
 * point has no counterpart in the CPU oracle (oracle/), which restates the entry points of hironaka_hip.h itself: the
 * Python binding lists it in hironaka_amd/_abi.py PLAY_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 */
#ifndef HIRONAKA_HIP_PLAY_H
#define HIRONAKA_HIP_PLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the plain Hironaka game played forward (an addition within ABI 6; hironaka/game.py:84-119 GameHironaka with
 * hironaka/agent.py:85-98 RandomAgent / ChooseFirstAgent: what hironaka/validator/hironaka_validator.py:30-48 playoff
 * loops over) ----
 * One game per lane, in list semantics (padding -1, rows with coordinate 0 >= 0 are the points).  The state is read once
 * and written once; points_out may equal points_in (with equal strides), otherwise the byte ranges the records of
 * points_in and of points_out span must not overlap (HK_ERR_SHAPE): workgroups write back while others still read.
 * Records that span more than 2^63 bytes are HK_ERR_SHAPE too, in place or not.
 *
 * Root: HK_PLAY_REDUCE_ROOT runs Newton sorted + compacted before any move (Game.__init__); HK_PLAY_RESCALE_ROOT then
 * applies the list rescale (x / max over the points, skipped when max is 0).  With max_steps 0 the call is just these.
 * A root that is not reduced is played as given: rows in row order, holes anywhere (HironakaValidator.reset).
 *
 * Move t < max_steps of a game that has at least 2 points:
 *   host    class_in[b, t] when class_in is given and the entry is >= 0, else the fixed host `host` (hk_host_select's
 *           codes 1..5; HK_PLAY_HOST_FORCED: none).  No class (-1, or an id beyond the dim's classes): the game stops
 *           with HK_PLAY_NO_MOVE, untouched.
 *   agent   axis_in[b, t] when given and >= 0; an axis outside the subset stops the game with HK_PLAY_NO_MOVE,
 *           untouched.  Else HK_AGENT_CHOOSE_FIRST (the subset's lowest coordinate), HK_AGENT_CHOOSE_LAST (its highest)
 *           or HK_AGENT_RANDOM_LEGAL (uniform over the subset: word 0 of Philox4x32-10 with key `seed` and counter
 *           (game_offset + b, step_offset + t, stream 3), so that shards and launches that continue a game reproduce
 *           the one launch; the j-th coordinate of the subset in ascending order for j = (word * |subset|) >> 32).
 *   state   shift (the sum in ascending coordinate order), reposition if HK_PLAY_REPOSITION (Agent.USE_REPOSITION),
 *           Newton sorted + compacted, the list rescale if HK_PLAY_RESCALE (IEEE division; scale_observation).
 *   stops   fewer than 2 points: HK_PLAY_ENDED.  Else a coordinate > value_threshold (when that is > 0):
 *           HK_PLAY_VALUE_LIMIT.  Without HK_PLAY_RESCALE, a shifted coordinate that reached 2^24 (float32) / 2^53
 *           (float64) stops the game with HK_PLAY_INEXACT after that move, whatever else it did: its values are not to
 *           be trusted.
 * Outputs: the final points; length_out [batch] the moves played; outcome_out [batch] one of the codes below, which
 * keep the numbers of the HK_MORIN_* codes they share; class_out / axis_out [batch, max_steps] (each may be NULL) the
 * moves played, -1 from length on.  A game with fewer than 2 points on entry (after the root stages) is copied through
 * with length 0 and HK_PLAY_ENDED.
 * dim 2..7, max_points 1..64, HK_F32 / HK_F64, strides >= max_points*dim, max_steps >= 0; anything else is
 * HK_ERR_UNSUPPORTED / HK_ERR_SHAPE before any launch (HK_HOST_RANDOM and HK_AGENT_RANDOM included: in list semantics
 * an axis outside the subset is a no-op).  A consumer of ABI 6 detects this entry point by its symbol. */
#define HK_PLAY_RUNNING 0       /* stopped by max_steps only                                           */
#define HK_PLAY_ENDED 1         /* fewer than 2 points                                                 */
#define HK_PLAY_NO_MOVE 3       /* no class from the host, or a forced axis outside the subset         */
#define HK_PLAY_INEXACT 4       /* a coordinate left the exact integers                                */
#define HK_PLAY_VALUE_LIMIT 5   /* a coordinate passed value_threshold                                 */
#define HK_PLAY_REPOSITION 1u   /* hk_game_play_desc.flags                                             */
#define HK_PLAY_RESCALE 2u
#define HK_PLAY_REDUCE_ROOT 4u
#define HK_PLAY_RESCALE_ROOT 8u
#define HK_PLAY_HOST_FORCED (-1) /* hk_game_play_desc.host: every class comes from class_in            */
typedef struct hk_game_play_desc {
  const void* points_in;   /* [batch] records of in_stride elements                                    */
  void* points_out;        /* [batch] records of out_stride elements; the first max_points*dim are written */
  int64_t in_stride;
  int64_t out_stride;
  const int32_t* class_in; /* [batch, max_steps] or NULL                                               */
  const int32_t* axis_in;  /* [batch, max_steps] or NULL                                               */
  int32_t* class_out;      /* [batch, max_steps] or NULL                                               */
  int32_t* axis_out;       /* [batch, max_steps] or NULL                                               */
  int32_t* length_out;     /* [batch]                                                                  */
  int32_t* outcome_out;    /* [batch]                                                                  */
  uint64_t seed;
  uint64_t game_offset;
  double value_threshold;  /* <= 0: none                                                               */
  int32_t batch;
  int32_t max_points;
  int32_t dim;
  int32_t dtype;
  int32_t host;
  int32_t agent;
  int32_t max_steps;
  uint32_t flags;
  uint32_t step_offset;    /* the number of the launch's first move in the random agent's counter      */
  uint32_t reserved_;
} hk_game_play_desc;
int hk_game_play(const hk_game_play_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_PLAY_H */
