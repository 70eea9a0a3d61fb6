/*
 * hironaka_hip_dqn.h -- the learning half of the DQN trainers' loop between ReplayBuffer.sample and loss.backward():
 * the 1-step TD target, the Huber loss and its gradient with respect to Q in one launch (hk_dqn_td), and the Polyak
 * update of a whole parameter list in one launch (hk_polyak_update); additions within ABI 6 that a consumer detects by
 * their symbols, part of the C ABI of hironaka_hip.h, which includes this file; HK_F32 / HK_F64 and the status codes
 * are defined there.  Like hk_replay_push (hironaka_hip_replay.h) the entry points have no counterpart in the CPU
 * oracle: the Python binding lists them in hironaka_amd/_abi.py DQN_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 */
#ifndef HIRONAKA_HIP_DQN_H
#define HIRONAKA_HIP_DQN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- hk_dqn_td: hironaka/trainer/dqn_trainer/dqn_trainer.py:68-88 and the backward pass of its loss down to Q ----
 * T is float (HK_F32) or double (HK_F64); B = batch, A = num_actions.  Row b of q, next_q and dq starts q_stride /
 * next_q_stride / dq_stride ELEMENTS after row b - 1.  With g = (T)(float)gamma (the reference's `(~dones) * gamma` is
 * a float32 tensor whatever T is), for every row b:
 *   mx       = the largest of next_q[b, 0..A); NaN if any of them is NaN (torch.max)
 *   target   = (T)rewards[b] + (dones[b] ? 0 : g) * mx      a rounded multiply, then a rounded add; the multiply is
 *                                                            never skipped: 0 * inf is NaN, as in the reference
 *   x        = q[b, actions[b]] - target
 *   row_loss = |x| < 1 ? 0.5 * x * x : |x| - 0.5             smooth_l1_loss, beta 1; NaN stays NaN
 *   dq[b, actions[b]] = (x < -1 ? -1 : x > 1 ? 1 : x) / (T)B    an IEEE divide; every other dq[b, c] = 0
 * and loss = (T)(the sum of the row_loss in double / B).  Every element of the B rows of dq is written; the elements
 * between the rows (dq_stride > A) are not touched.  target and row_loss may be NULL.
 *
 * An action outside [0, A) reads and writes nothing out of bounds: the row's target is as above, its row_loss and its
 * whole dq row are 0, HK_DQN_BAD_ACTION is OR-ed into *status (an atomic; the caller zeroes the word) and the return
 * value is still HK_OK.  (The reference's torch.gather fails with a device-side assertion there.)
 *
 * loss is the same bits on every launch with the same inputs: a workgroup owns HK_DQN_TILE_ROWS consecutive rows, adds
 * their row_loss in double in a fixed tree and leaves the sum in the workspace slot with its own index; the workgroup
 * that draws the last ticket adds the slots in index order, writes loss and zeroes the ticket.  No float atomics, and
 * nobody waits for anybody.  The workspace: hk_dqn_td_workspace_bytes(batch) bytes, 8-byte aligned, zeroed ONCE by the
 * caller before its first use (word 0 is the ticket, 0 between launches; the slots follow 16 bytes in); a larger one
 * serves a smaller batch.  Launches that share a workspace belong on one stream.
 *
 * B >= 0 (0: HK_OK, nothing is launched and nothing written), 1 <= A <= HK_DQN_MAX_ACTIONS.  Before any launch: a NULL
 * descriptor, q, next_q, actions, rewards, dones, dq, loss, workspace or status is HK_ERR_NULL; B < 0, A out of range, a
 * stride below A (or rows that span more than 2^63 bytes) HK_ERR_SHAPE; a dtype other than HK_F32 / HK_F64, or dq
 * overlapping q or next_q, HK_ERR_UNSUPPORTED; a pointer that is not aligned to its element (the workspace: 8 bytes)
 * HK_ERR_ALIGN. */
#define HK_DQN_TILE_ROWS 256    /* the batch rows one workgroup owns                               */
#define HK_DQN_MAX_ACTIONS 65536
#define HK_DQN_BAD_ACTION 1u    /* *status: an action lay outside [0, num_actions)                 */
typedef struct hk_dqn_td_desc {
  const void* q;          /* [B] rows of q_stride T, the first A of each are the row             */
  const void* next_q;     /* [B] rows of next_q_stride T                                         */
  const int32_t* actions; /* [B]                                                                  */
  const float* rewards;   /* [B] float32 whatever T is                                           */
  const uint8_t* dones;   /* [B] nonzero: the episode ended with this experience                 */
  void* target;           /* [B] T, or NULL                                                       */
  void* row_loss;         /* [B] T, or NULL                                                       */
  void* dq;               /* [B] rows of dq_stride T                                              */
  void* loss;             /* one T                                                                */
  void* workspace;        /* hk_dqn_td_workspace_bytes(batch) bytes                               */
  uint32_t* status;       /* one word                                                             */
  int64_t q_stride;
  int64_t next_q_stride;
  int64_t dq_stride;
  double gamma;
  int32_t batch;
  int32_t num_actions;
  int32_t dtype;          /* HK_F32 or HK_F64                                                     */
  int32_t reserved_;
} hk_dqn_td_desc;
uint64_t hk_dqn_td_workspace_bytes(int batch);
int hk_dqn_td(const hk_dqn_td_desc* desc, void* stream);

/* ---- hk_polyak_update: hironaka/src/_borrowed_fn.py:25-49 polyak_update over a whole parameter list ----
 * For every entry t < ntensors and element i < numel:
 *   dst[i] = fma((T)tau, src[i], round(dst[i] * (T)(1 - tau)))      1 - tau computed in double
 * which is what the reference's two lines compute (`mul_`, then `torch.add(..., alpha=tau, out=...)`: a rounded
 * multiply, then a fused multiply-add).  tau = 1 therefore copies src bit for bit where dst was finite, and tau = 0
 * leaves dst as it was where src is finite.  The descriptor is read on the host and travels to the kernel as its
 * argument: there is no table on the device.  A workgroup owns HK_POLYAK_CHUNK_BYTES of one tensor; where src and dst of
 * an entry sit at the same offset from a 16-byte boundary the elements move 16 bytes at a time, with single elements in
 * front of the first boundary and behind the last, otherwise element by element.
 *
 * ntensors == 0 and entries with numel == 0 are HK_OK with nothing done for them.  Before any launch: a NULL descriptor,
 * or a NULL src or dst with numel > 0, is HK_ERR_NULL; ntensors outside 0..HK_POLYAK_MAX_TENSORS or numel < 0
 * HK_ERR_SHAPE; a dtype other than HK_F32 / HK_F64, or a dst range that overlaps its own src (src == dst included), the
 * src of another entry or the dst of another entry, HK_ERR_UNSUPPORTED; a pointer that is not aligned to its element
 * HK_ERR_ALIGN. */
#define HK_POLYAK_MAX_TENSORS 64
#define HK_POLYAK_CHUNK_BYTES 16384 /* of one tensor, per workgroup: 256 lanes x 4 transfers of 16 bytes */
typedef struct hk_polyak_tensor {
  const void* src;
  void* dst;
  int64_t numel;
} hk_polyak_tensor;
typedef struct hk_polyak_desc {
  hk_polyak_tensor tensor[HK_POLYAK_MAX_TENSORS];
  double tau;
  int32_t ntensors; /* 0 .. HK_POLYAK_MAX_TENSORS */
  int32_t dtype;    /* HK_F32 or HK_F64, of every tensor */
} hk_polyak_desc;
int hk_polyak_update(const hk_polyak_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_DQN_H */
