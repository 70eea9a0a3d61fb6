/*
 * hironaka_hip_pvloss.h -- the loss of the MCTS trainer's gradient step between the network's forward and
 * loss.backward(): policy_value_loss (hironaka/jax/loss.py:12-24) and its gradient with respect to the policy logits and
 * the value in one launch (hk_pv_loss); an addition within ABI 6 that a consumer detects by its symbols, part of the C ABI
 * of hironaka_hip.h, which includes this file; HK_F32 and the status codes are defined there.  Like hk_dqn_td
 * (hironaka_hip_dqn.h) the entry points have no counterpart in the CPU oracle: the Python binding lists them in
 * hironaka_amd/_abi.py PVLOSS_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 */
#ifndef HIRONAKA_HIP_PVLOSS_H
#define HIRONAKA_HIP_PVLOSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- hk_pv_loss: hironaka/jax/loss.py:12-24 policy_value_loss and the backward pass down to logits and value ----
 * float32 in and out; B = batch, A = actions, N = num_samples.  Row b of logits, target_policy and dlogits starts
 * logits_stride / target_policy_stride / dlogits_stride ELEMENTS after row b - 1; element b of value and dvalue lies
 * value_stride / dvalue_stride elements after element b - 1.  logits and value are the network's outputs for the B rows
 * of the batch and are not indexed; target_policy, target_value and weight have N rows, of which batch row b takes row
 *   r = index ? index[b] : b
 * (the gather of the sampled rows out of the rollout happens inside the launch).  For every row b:
 *   q_a     = softmax(target_policy[r, :])_a          exp(t_a - max t) / the sum of them
 *   logp_a  = log_softmax(logits[b, :])_a             (x_a - max x) - log(the sum of exp(x_a - max x))
 *   p_a     = exp(logp_a)
 *   w       = weight ? weight[r] : 1
 *   row_b   = ( -(sum_a q_a * logp_a) / A  +  |value[b] - target_value[r]| ) * w
 *   loss    = (sum_b row_b) / B
 *   dlogits[b, a] = w * (p_a * (sum_a q_a) - q_a) / (A * B)
 *   dvalue[b]     = w * sign(value[b] - target_value[r]) / B        sign(0) = 0
 * Every row is evaluated in double with the device library's double exp / log, the operations in the order written
 * (A * B is one double product); row_loss[b] (may be NULL), dlogits, dvalue and loss are each rounded to float32 once,
 * from that double.  A product q_a * logp_a with q_a == 0 is skipped, so a target of -inf (what the agent's masked
 * policy produces) contributes 0 where logp_a is -inf too, and its dlogits is w * p_a * (sum q) / (A * B).  A NaN, a row
 * of targets that are all -inf and a logit of +inf give the NaN the formula gives, in that row and in loss.  Every
 * element of the B rows of dlogits and the B elements of dvalue is written; the elements between them are not touched.
 *
 * An index[b] outside [0, N) reads nothing out of bounds: the row's row_loss, its dlogits row and its dvalue are 0,
 * HK_PVLOSS_BAD_INDEX is OR-ed into *status (an atomic; the caller zeroes the word) and the return value is still HK_OK.
 *
 * loss is the same bits on every launch with the same inputs: a workgroup owns HK_PVLOSS_TILE_ROWS consecutive rows,
 * adds their row_b (the doubles) in a fixed tree and leaves the sum in the workspace slot with its own index; the
 * workgroup that draws the last ticket adds the slots in index order, writes loss and zeroes the ticket.  No float
 * atomics, and nobody waits for anybody.  The workspace: hk_pv_loss_workspace_bytes(batch) bytes, 8-byte aligned,
 * zeroed ONCE by the caller before its first use (word 0 is the ticket, 0 between launches; the slots follow 16 bytes
 * in); a larger one serves a smaller batch.  Launches that share a workspace belong on one stream.
 *
 * B >= 0 (0: HK_OK, nothing is launched and nothing written), 1 <= A <= HK_PVLOSS_MAX_ACTIONS (the policy head's range,
 * hironaka_hip_pvnet.h), N >= 1 where B > 0, and N >= B where index is NULL.  Before any launch: a NULL descriptor, logits, value,
 * target_policy, target_value, dlogits, dvalue, loss, workspace or status is HK_ERR_NULL; B < 0, A or N out of range, a
 * row stride below A, an element stride below 1 (or rows that span more than 2^63 bytes) HK_ERR_SHAPE; a dtype other
 * than HK_F32, a flag (none is defined), or dlogits, dvalue, row_loss or loss overlapping logits, value, target_policy,
 * target_value, weight or index HK_ERR_UNSUPPORTED; a pointer that is not aligned to its element (index and the
 * workspace: 8 bytes) HK_ERR_ALIGN. */
#define HK_PVLOSS_TILE_ROWS 16    /* the batch rows one workgroup owns                               */
#define HK_PVLOSS_MAX_ACTIONS 255
#define HK_PVLOSS_BAD_INDEX 1u    /* *status: an index lay outside [0, num_samples)                  */
typedef struct hk_pv_loss_desc {
  const float* logits;        /* [B] rows of logits_stride floats, the first A of each are the row   */
  const float* value;         /* [B] elements value_stride floats apart                              */
  const float* target_policy; /* [N] rows of target_policy_stride floats                             */
  const float* target_value;  /* [N]                                                                  */
  const float* weight;        /* [N], or NULL: 1                                                      */
  const int64_t* index;       /* [B], or NULL: row b takes sample b                                   */
  float* dlogits;             /* [B] rows of dlogits_stride floats                                    */
  float* dvalue;              /* [B] elements dvalue_stride floats apart                              */
  float* row_loss;            /* [B], or NULL                                                         */
  float* loss;                /* one float                                                            */
  void* workspace;            /* hk_pv_loss_workspace_bytes(batch) bytes                              */
  uint32_t* status;           /* one word                                                             */
  int64_t logits_stride;
  int64_t value_stride;
  int64_t target_policy_stride;
  int64_t dlogits_stride;
  int64_t dvalue_stride;
  int64_t num_samples;
  int32_t batch;
  int32_t actions;
  int32_t dtype;              /* HK_F32                                                               */
  int32_t flags;              /* 0                                                                    */
} hk_pv_loss_desc;
uint64_t hk_pv_loss_workspace_bytes(int batch);
int hk_pv_loss(const hk_pv_loss_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_PVLOSS_H */
