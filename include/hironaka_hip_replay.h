/*
 * hironaka_hip_replay.h -- the DQN trainers' replay buffer as a ring on the device: a masked, order-keeping push of a
 * batch of experiences and a uniform sample, one launch each (hk_replay_push / hk_replay_sample, additions within ABI 6
 * that a consumer detects by their symbols), part of the C ABI of hironaka_hip.h, which includes this file; the status
 * codes are defined there.  Like hk_env_step (hironaka_hip_env.h) the entry points have no counterpart in the CPU
 * oracle: the Python binding lists them in hironaka_amd/_abi.py REPLAY_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 */
#ifndef HIRONAKA_HIP_REPLAY_H
#define HIRONAKA_HIP_REPLAY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the ring of hironaka/trainer/replay_buffer.py, its cursor kept on the device ----
 * A buffer is 1..8 columns (observations, actions, rewards, dones, next observations; a dict observation is one column
 * per key).  Column c is a ring of `capacity` rows of row_bytes[c] bytes each, packed; the rows are opaque bytes.  The
 * batch side of a column (`rows`: the source of a push, the destination of a sample) has its rows rows_stride_bytes
 * apart, so a column may be a slice of wider records.
 *
 * The cursor: 8 int64 words on the device, 8-byte aligned.  A zeroed block is an empty buffer.
 *   word 0  pos            the ring slot the next pushed row goes to, 0 <= pos < capacity
 *   word 1  full           0 / 1: every slot has been written at least once
 *   word 2  last_count     the rows the last push kept
 *   word 3  total_pushed   the rows kept by all pushes
 *   word 4  samples_drawn  the hk_replay_sample calls so far: the draw number of the next one
 *   word 5  ticket         the workgroups of the running launch that have read the cursor; 0 between launches
 *   word 6, 7              reserved, left as they are
 * Both entry points read the cursor and rewrite it inside their launch, so calls that share a cursor belong on one
 * stream (or are ordered by the caller).
 *
 * hk_replay_push: with n the number of rows j of the batch with keep[j] != 0 (keep NULL: every row), the kept rows,
 * in batch order k = 0..n-1, go to ring slot (pos + k) mod capacity of every column.  Then full |= (pos + n >=
 * capacity), pos = (pos + n) mod capacity, last_count = n, total_pushed += n: replay_buffer.py:116-127 with length n,
 * where n is decided on the device.  Slots that are not written keep their bytes.  batch >= capacity is HK_ERR_SHAPE
 * (the reference asserts buffer_size > length).  batch == 0 is HK_OK without a launch: the cursor stays as it is,
 * last_count included.
 *
 * hk_replay_sample: size = full ? capacity : pos.  For j = 0..batch_size-1, with s = samples_drawn on entry:
 *   block = Philox4x32-10 with key seed at counter (j >> 2, s low 32 bits, s high 32 bits, stream 4)
 *   index_j = (word (j & 3) of block * size) >> 32
 * Row index_j of every column's ring goes to row j of its `rows`, and index_out[j] = index_j (index_out may be NULL).
 * Then samples_drawn += 1.  If size == 0 every index is -1 and no row is written.  desc.batch and desc.keep are not
 * looked at; batch_size == 0 is HK_OK without a launch and does not count as a draw.
 *
 * Before any launch: a NULL descriptor, cursor, ring or rows is HK_ERR_NULL; ncols outside 1..8, row_bytes < 1,
 * rows_stride_bytes < row_bytes, batch or batch_size < 0, capacity < 1 and batch >= capacity are HK_ERR_SHAPE;
 * row_bytes above 2^20 is HK_ERR_UNSUPPORTED; a cursor that is not 8-byte aligned is HK_ERR_ALIGN.  Rings and rows of
 * any alignment are served: 16-byte and 4-byte accesses where the pointers, the row size and the stride are multiples
 * of that, bytes otherwise.  The rings and the batch side must not overlap. */
#define HK_REPLAY_MAX_COLS 8
#define HK_REPLAY_CURSOR_WORDS 8
#define HK_REPLAY_POS 0
#define HK_REPLAY_FULL 1
#define HK_REPLAY_LAST_COUNT 2
#define HK_REPLAY_TOTAL_PUSHED 3
#define HK_REPLAY_SAMPLES_DRAWN 4
#define HK_REPLAY_TICKET 5
#define HK_REPLAY_STREAM 4 /* the Philox stream id of the sample indices */
#define HK_REPLAY_TILE_ROWS 128 /* the batch rows one workgroup of either kernel owns */
typedef struct hk_replay_col {
  void* ring;                /* [capacity] rows of row_bytes                                                    */
  void* rows;                /* the batch side: [batch] rows read by a push, [batch_size] rows written by a sample */
  int64_t row_bytes;         /* 1 .. 2^20                                                                       */
  int64_t rows_stride_bytes; /* >= row_bytes                                                                    */
} hk_replay_col;
typedef struct hk_replay_desc {
  hk_replay_col col[HK_REPLAY_MAX_COLS];
  const uint8_t* keep; /* [batch] or NULL (every row); push only                                                */
  int64_t* cursor;     /* [HK_REPLAY_CURSOR_WORDS]                                                              */
  int32_t ncols;       /* 1 .. HK_REPLAY_MAX_COLS                                                               */
  int32_t batch;       /* the rows offered to a push, < capacity                                                */
  int32_t capacity;    /* the rows of every ring                                                                */
  int32_t reserved_;
} hk_replay_desc;
int hk_replay_push(const hk_replay_desc* desc, void* stream);
int hk_replay_sample(const hk_replay_desc* desc, int batch_size, uint64_t seed, int64_t* index_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_REPLAY_H */
