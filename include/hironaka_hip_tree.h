/*
 * hironaka_hip_tree.h -- one level of a game tree under any host (hk_tree_expand, an addition within ABI 6 that a
 * consumer detects by its symbol), part of the C ABI of hironaka_hip.h, which includes this file; the HK_SEM_* codes,
 * HK_F32 / HK_F64 and the status codes are defined there.  Like hk_host_select (hironaka_hip_hosts.h) and hk_game_play
 * (hironaka_hip_play.h) the entry point has no counterpart in the CPU oracle (oracle/), which restates the entry points
 * of hironaka_hip.h itself: the Python binding lists it in hironaka_amd/_abi.py TREE_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 */
#ifndef HIRONAKA_HIP_TREE_H
#define HIRONAKA_HIP_TREE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one level of hironaka/jax/search.py:73-113 search_tree_fix_host over a whole frontier (an addition within ABI 6)
 * The host ran outside: class_id[n] is its subset at parent n as a class id (hk_step's coords codec); an id < 0, or one
 * beyond the dim's classes, means "do not expand this node".  Parent n with the subset S has one child per coordinate a
 * of S in ascending a (search.py:102); child number r goes to slot child_offset[n] + r, where child_offset is the
 * exclusive prefix sum of the parents' |S| that the caller computed.  A slot outside [0, capacity) is never written:
 * the other children of that parent still are, and HK_TREE_OVERFLOW is OR-ed into *status (an atomic; the caller zeroes
 * the word).  The return value is still HK_OK.
 *
 * A child's state is the step of the parent's with that subset and axis:
 *   HK_SEM_JAX   shift, reposition if HK_TREE_REPOSITION, Newton polytope; rows keep their places and holes stay
 *                (jax/util.py:83-125 get_take_actions("host", spec, rescale_points=False, reposition=...))
 *   HK_SEM_LIST  shift, reposition if HK_TREE_REPOSITION, Newton sorted + compacted (what hk_search_game_tree and
 *                hk_game_play compute per move)
 * Per slot: the state into the first max_points*dim elements of a record of out_stride elements, followed by dim zeros
 * if HK_TREE_ZERO_TAIL (search.py:107; otherwise nothing else of the record is touched); child_parent = n; child_axis =
 * a; child_num_points = the rows with coordinate 0 >= 0; child_done = 1 when, under HK_SEM_JAX, at most dim of the
 * max_points*dim entries are >= 0 (jax/util.py:38-39 get_done_from_flatten) or, under HK_SEM_LIST, fewer than 2 points
 * remain, else 0.
 *
 * dim 2..7, HK_F32 / HK_F64, any max_points whose parent and child fit one workgroup's 64 KiB of LDS together
 * ((2*max_points*dim + 2*dim) | 1 elements), HK_SEM_JAX / HK_SEM_LIST; in_stride >= max_points*dim, out_stride >=
 * max_points*dim (+ dim with HK_TREE_ZERO_TAIL); the byte ranges that the records of parents_in and of children_out
 * span must not overlap, and neither is more than 2^63 bytes.  Anything else is HK_ERR_UNSUPPORTED / HK_ERR_SHAPE /
 * HK_ERR_NULL / HK_ERR_ALIGN before any launch.  n_parents 0 is HK_OK with nothing done. */
#define HK_TREE_REPOSITION 1u /* hk_tree_expand_desc.flags                                          */
#define HK_TREE_ZERO_TAIL 2u
#define HK_TREE_OVERFLOW 1u   /* *status: a child's slot lay outside [0, capacity)                  */
typedef struct hk_tree_expand_desc {
  const void* parents_in;      /* [n_parents] records of in_stride elements; the state is the first max_points*dim */
  void* children_out;          /* [capacity] records of out_stride elements                        */
  int64_t in_stride;
  int64_t out_stride;
  const int32_t* class_id;     /* [n_parents]                                                      */
  const int64_t* child_offset; /* [n_parents]                                                      */
  int32_t* child_parent;       /* [capacity]                                                       */
  int32_t* child_axis;         /* [capacity]                                                       */
  int32_t* child_num_points;   /* [capacity]                                                       */
  uint8_t* child_done;         /* [capacity]                                                       */
  uint32_t* status;            /* one word                                                         */
  int32_t n_parents;
  int32_t capacity;
  int32_t max_points;
  int32_t dim;
  int32_t dtype;
  int32_t sem;                 /* HK_SEM_JAX or HK_SEM_LIST                                        */
  uint32_t flags;
  uint32_t reserved_;
} hk_tree_expand_desc;
int hk_tree_expand(const hk_tree_expand_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_TREE_H */
