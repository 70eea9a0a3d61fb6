/*
 * hironaka_hip_env.h -- one move of every game of a vectorised gym environment, with the reset of a stopped game inside
 * the launch (hk_env_step, an addition within ABI 6 that a consumer detects by its symbol), part of the C ABI of
 * hironaka_hip.h, which includes this file; the HK_HOST_* and HK_AGENT_* codes, HK_F32 / HK_F64 and the status codes are
 * defined there.  Like hk_game_play (hironaka_hip_play.h) the entry point has no counterpart in the CPU oracle: the
 * Python binding lists it in hironaka_amd/_abi.py ENV_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 */
#ifndef HIRONAKA_HIP_ENV_H
#define HIRONAKA_HIP_ENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the step of hironaka_amd/gym_env.py's HironakaHostEnv / HironakaAgentEnv, per game, in one launch ----
 * One game per lane, in list semantics (padding -1, sorted descending-lexicographically and compacted).  The state
 * [batch, max_points, dim] is read once and written once; points_out may equal points_in, otherwise the two must not
 * overlap (HK_ERR_SHAPE).  Every game carries its own step counter and episode number, so games stop and start again
 * independently of each other.
 *
 * HK_ENV_MODE_HOST (the environment fixes a host, the learner is the agent), per game:
 *   step_count += 1.  legal = 0 <= action < dim and the action is a coordinate of the pending subset class_io (a class
 *   id, -1: none; an action outside [0, dim) indexes nothing).  A legal move is shift + Newton, sorted and compacted; an
 *   illegal one leaves the state untouched (see "no move" below).  ended = fewer than 2 points.  reward = invalid_move_penalty if not
 *   legal, else 1 if not ended, else 0.  exceed = value_threshold > 0 and a coordinate of the state > value_threshold, tested
 *   before this step's rescale.  stopped = ended | exceed | (not legal and HK_ENV_STOP_AFTER_INVALID).  The new pending
 *   subset is the host's class on the state before the rescale, -1 if stopped or the host has none.  The list rescale
 *   follows if HK_ENV_SCALE_OBSERVATION.  Observation: the points as float32 and the pending subset as a 0/1 vector
 *   (zero when there is none).
 * HK_ENV_MODE_AGENT (the environment fixes an agent, the learner is the host), per game:
 *   step_count += 1.  The action is the host's subset as a bit mask over the dim coordinates; a mask with fewer than 2
 *   bits is no move (agent_axis -1).  Otherwise the agent's axis is the subset's lowest coordinate
 *   (HK_AGENT_CHOOSE_FIRST) or uniform over it (HK_AGENT_RANDOM_LEGAL: word 0 of Philox4x32-10 with key
 *   agent_seed and counter (game_offset + episode * world_games + b, step_count - 1, stream 3); the j-th coordinate of
 *   the subset in ascending order for j = (word * |subset|) >> 32 -- hk_game_play's rule with the game index extended
 *   by the episode), and the move is shift, reposition if HK_ENV_AGENT_REPOSITION, Newton sorted and compacted.
 *   ended = fewer than 2 points; stopped = ended; reward = 0.  With HK_ENV_STOP_AT_THRESHOLD: trip = exceed (as above) |
 *   step_count >= step_threshold; stopped |= trip; reward += trip * threshold_penalty.  The list rescale follows if
 *   HK_ENV_SCALE_OBSERVATION; reward += points before - points after if HK_ENV_POINT_REDUCTION_REWARD; reward += 1 if
 *   ended.  Observation: the points as float32.
 * No move.  Host mode, an illegal axis: no stage runs (hironaka_host_env.py:46-52 touches the points only where the
 *   action is in the pending list); ended, exceed and the host look at the state as it is, and the rescale follows.
 *   Agent mode, a mask with fewer than 2 bits: the shift is skipped and the stages behind it run, as Agent.move runs
 *   them.  They leave a state that is reduced already as it is, except where its rescale has merged coordinates that
 *   were an ulp apart: Newton then drops the row that has become dominated.
 * HK_ENV_AUTO_RESET, for a game with stopped set: its terminal observation goes to final_points / final_coords (where
 *   given; untouched for every other game), episode += 1, and max_points * dim integers in [0, max_value) are drawn by
 *   the generator's element rule for the global game index game_offset + episode * world_games + b with key seed -- row
 *   b of hk_generate_points(batch = world_games, game_offset = episode * world_games, no stages) -- followed by Newton
 *   sorted and compacted, the list rescale if HK_ENV_SCALE_OBSERVATION, and Newton again unless
 *   HK_ENV_IMPROVE_EFFICIENCY.  Host mode then does what the environment's first step(None) does, a step without a
 *   move, which leaves the fresh state as it is: step_count = 1 and
 *   the pending subset is the host's class on the fresh state, -1 if that state has fewer than 2 points, exceeds
 *   value_threshold, or HK_ENV_STOP_AFTER_INVALID is set (the environment counts step(None) as an invalid move).  Agent
 *   mode: step_count = 0.  The observation, the state and the counters returned are the fresh episode's; reward,
 *   stopped and exceed remain the finished step's.  A fresh state with fewer than 2 points is delivered as it is.
 *   Without HK_ENV_AUTO_RESET a stopped game is left as the step left it and final_* are not written.
 * HK_ENV_RESET_ALL: no move is played and points_in, action and final_* are not looked at; every game is given a fresh
 *   episode as above (episode += 1: episode -1 on entry starts episode 0) with reward 0, stopped 0 and exceed 0.
 *
 * dim 2..7, max_points 1..64, HK_F32 / HK_F64, batch >= 0, host one of hk_host_select's codes 1..5, agent
 * HK_AGENT_CHOOSE_FIRST or HK_AGENT_RANDOM_LEGAL, max_value >= 1 when a reset can happen; anything else, a NULL pointer
 * where one is required and an unknown flag are HK_ERR_UNSUPPORTED / HK_ERR_SHAPE / HK_ERR_NULL before any launch. */
#define HK_ENV_MODE_HOST 0
#define HK_ENV_MODE_AGENT 1
#define HK_ENV_SCALE_OBSERVATION 1u      /* hk_env_step_desc.flags                                            */
#define HK_ENV_STOP_AFTER_INVALID 2u     /* host mode                                                         */
#define HK_ENV_STOP_AT_THRESHOLD 4u      /* agent mode                                                        */
#define HK_ENV_POINT_REDUCTION_REWARD 8u /* agent mode                                                        */
#define HK_ENV_IMPROVE_EFFICIENCY 16u
#define HK_ENV_AGENT_REPOSITION 32u      /* agent mode                                                        */
#define HK_ENV_AUTO_RESET 64u
#define HK_ENV_RESET_ALL 128u
typedef struct hk_env_step_desc {
  const void* points_in;   /* [batch, max_points, dim]; may be NULL with HK_ENV_RESET_ALL                     */
  void* points_out;        /* [batch, max_points, dim]                                                        */
  int32_t* class_io;       /* [batch] in and out, host mode: the pending subset as a class id, -1 for none    */
  int32_t* step_count;     /* [batch] in and out                                                              */
  int32_t* episode;        /* [batch] in and out                                                              */
  const int32_t* action;   /* [batch] host mode: an axis; agent mode: the subset as a bit mask                */
  double* reward;          /* [batch]                                                                         */
  uint8_t* stopped;        /* [batch]                                                                         */
  uint8_t* exceed;         /* [batch] or NULL: whether value_threshold was passed                             */
  float* obs_points;       /* [batch, max_points, dim]                                                        */
  double* obs_coords;      /* [batch, dim], host mode                                                         */
  float* final_points;     /* [batch, max_points, dim] or NULL                                                */
  double* final_coords;    /* [batch, dim] or NULL, host mode                                                 */
  int32_t* agent_axis;     /* [batch] or NULL, agent mode: the axis the agent chose, -1 for no move           */
  uint64_t seed;           /* the generator's key                                                             */
  uint64_t agent_seed;     /* the random agent's key                                                          */
  uint64_t game_offset;
  uint64_t world_games;    /* the games of one episode over all shards                                        */
  double value_threshold;  /* <= 0: none                                                                      */
  double invalid_move_penalty;
  double threshold_penalty;
  int32_t batch;
  int32_t max_points;
  int32_t dim;
  int32_t dtype;
  int32_t mode;
  int32_t host;
  int32_t agent;
  int32_t max_value;
  int32_t step_threshold;
  uint32_t flags;
} hk_env_step_desc;
int hk_env_step(const hk_env_step_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_ENV_H */
