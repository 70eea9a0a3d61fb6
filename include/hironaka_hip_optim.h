/*
 * hironaka_hip_optim.h -- the optimiser step of the DQN trainers' loop (hironaka/trainer/dqn_trainer/dqn_trainer.py:95-98:
 * nn.utils.clip_grad_norm_ and optimizer.step() with torch.optim.Adam or torch.optim.SGD, trainer.py:63) in TWO launches
 * per HK_OPTIM_MAX_TENSORS tensors: hk_optim_prepare reads the gradients once and leaves the total norm, the clipping
 * coefficient and the step's scalars in a 64-byte block on the device, hk_optim_apply clips and updates.  Additions
 * within ABI 6 that a consumer detects by their symbols, part of the C ABI of hironaka_hip.h, which includes this file;
 * HK_F32 / HK_F64 and the status codes are defined there.  The entry points have no counterpart in the CPU oracle: the
 * Python binding lists them in hironaka_amd/_abi.py OPTIM_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 *
 * T is float (HK_F32) or double (HK_F64), one per descriptor.  Every operation below is rounded once in T unless it is
 * written fma (one rounding for the multiply and the add together).
 *
 * ---- the state block: hk_optim_state, HK_OPTIM_STATE_BYTES bytes on the device, 8-byte aligned ----
 * The caller initialises it ONCE to step = 0, beta1_pow = beta2_pow = 1.0 (the rest: anything).  The count lives on the
 * device so that a captured graph advances it.  hk_optim_prepare writes it, hk_optim_apply reads it.
 *
 * ---- hk_optim_prepare: one pass over the gradients ----
 * A workgroup owns HK_OPTIM_CHUNK_BYTES of one gradient (tensor t has ceil(numel * sizeof(T) / HK_OPTIM_CHUNK_BYTES)
 * workgroups, wherever it lies in memory; the sum of these over the table is the launch's workgroup count).  Lane l of
 * its 256 adds (double)g * (double)g of the chunk's elements l, l + 256, l + 512, ... in that order, the 64 lanes of a
 * wave are added as a halving tree (lane i += lane i + 32, then 16, ... 1), the 4 waves in order, and the sum goes to the
 * workspace slot slot_base + the workgroup's index.  With HK_OPTIM_LAST the workgroup that draws the last ticket adds
 * the slots [0, slot_base + the launch's workgroups) in index order -- the same bits on every launch; no float atomics,
 * nobody waits, the ticket is zero again afterwards -- and writes into the state block
 *   total_norm = (T)sqrt(sum)                                          the square root in double
 *   clip_coef  = c > 1 ? 1 : c  with  c = ((T)1 / (total_norm + (T)1e-6)) * (T)max_norm
 *                (torch's clip_grad_norm_ to the bit: its `max_norm / (total_norm + 1e-6)` is a reciprocal and a
 *                multiply, two roundings; max_norm = +inf gives 1; a non-finite norm goes through the same arithmetic,
 *                as torch with error_if_nonfinite=False)
 *                With HK_OPTIM_NO_CLIP the coefficient is 1 whatever the norm is, so that a step without clipping
 *                meets a non-finite gradient as torch's step() does: in that element alone.
 *   lr         = *lr_dev where lr_dev is not NULL (a learning-rate schedule under graph replay), else desc.lr
 * and with HK_OPTIM_ADVANCE, all in double,
 *   step += 1;  beta1_pow *= beta1;  beta2_pow *= beta2
 *   neg_step_size = -(lr / (1 - beta1_pow));  bias2_sqrt = sqrt(1 - beta2_pow)
 * (torch evaluates beta ** step in Python: the running product differs from that by at most step * 2^-53 relative).
 * A list longer than one table is a chain of launches on ONE stream with one workspace: launch k has slot_base = the
 * workgroups of the launches before it, only the last carries HK_OPTIM_LAST.  Only the gradients are read: param,
 * state1 and state2 may be NULL.  Workspace: hk_optim_workspace_bytes(the chain's workgroups) bytes, 8-byte aligned,
 * zeroed ONCE by the caller (word 0 is the ticket; the slots follow 16 bytes in); a larger one serves a smaller chain.
 *
 * ---- hk_optim_apply: per element, coef = (T)clip_coef and the scalars from the state block ----
 * HK_OPTIM_SCALE (clipping alone)   grad = grad * coef
 * HK_OPTIM_SGD    (torch.optim.SGD; mu = momentum, state1 = the momentum buffer, needed where mu != 0)
 *   g = grad * coef
 *   if weight_decay != 0:  g = fma((T)wd, p, g)
 *   if mu != 0:            buf = g where the block's step is 1 (the first step), else
 *                          buf = dampening == 0 ? buf * mu + g : fma((T)(1 - dampening), g, buf * mu)
 *                          g = HK_OPTIM_NESTEROV ? fma(mu, buf, g) : buf
 *   p = fma((T)(-lr), g, p)
 * HK_OPTIM_ADAM   (torch.optim.Adam, amsgrad off, coupled L2 weight decay; state1 = exp_avg m, state2 = exp_avg_sq v)
 *   g = grad * coef
 *   if weight_decay != 0:  g = fma((T)wd, p, g)
 *   m = w1 < 0.5 ? fma(w1, g - m, m) : fma(-(g - m), (T)1 - w1, g)    w1 = (T)(1 - beta1)   (torch's lerp_)
 *   v = fma((T)(1 - beta2) * g, g, v * (T)beta2)
 *   denom = sqrt(v) / (T)bias2_sqrt + (T)eps
 *   p = p + ((T)neg_step_size * m) / denom
 * The last line is this library's own: torch's vectorised addcdiv_ differs from every scalar form in the last bit of a
 * few elements in ten thousand.  1 - beta1, 1 - beta2, 1 - dampening and -lr are computed in double.
 * The clipped gradient grad * coef (before the weight decay) is written back to grad, as clip_grad_norm_ changes .grad
 * in place; HK_OPTIM_KEEP_GRADS skips that store.  Where all pointers that the kind uses of an entry sit at the same
 * offset from a 16-byte boundary the elements move 16 bytes at a time, with single elements in front of the first
 * boundary and behind the last; otherwise element by element.
 *
 * ---- status, both entry points, before any launch ----
 * ntensors == 0 and entries with numel == 0 are HK_OK with nothing done for them (a prepare with HK_OPTIM_LAST and
 * slot_base > 0 still launches one workgroup that adds the earlier launches' slots).  A NULL descriptor, state,
 * workspace (prepare) or a NULL pointer that the kind uses with numel > 0 is HK_ERR_NULL; ntensors outside
 * 0..HK_OPTIM_MAX_TENSORS, numel < 0, slot_base < 0 or more than 2^31 - 1 workgroups HK_ERR_SHAPE; an unknown kind,
 * dtype or flag, HK_OPTIM_SCALE with HK_OPTIM_KEEP_GRADS (nothing to do), or (apply, which writes them) two of the used
 * param / grad / state ranges of any entries that share a byte, HK_ERR_UNSUPPORTED; a pointer that is not aligned to its
 * element (state, workspace, lr_dev: 8 bytes) HK_ERR_ALIGN. */
#ifndef HIRONAKA_HIP_OPTIM_H
#define HIRONAKA_HIP_OPTIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HK_OPTIM_MAX_TENSORS 64
#define HK_OPTIM_CHUNK_BYTES 16384 /* of one tensor, per workgroup: 256 lanes x 4 transfers of 16 bytes */
#define HK_OPTIM_STATE_BYTES 64
/* kind */
#define HK_OPTIM_SCALE 0
#define HK_OPTIM_SGD 1
#define HK_OPTIM_ADAM 2
/* flags */
#define HK_OPTIM_LAST 1u       /* prepare: the last launch of its chain: reduce and write the state block */
#define HK_OPTIM_ADVANCE 2u    /* prepare: count the step and move the running powers on                  */
#define HK_OPTIM_KEEP_GRADS 4u /* apply: do not write the clipped gradient back                           */
#define HK_OPTIM_NESTEROV 8u   /* apply, HK_OPTIM_SGD                                                     */
#define HK_OPTIM_NO_CLIP 16u   /* prepare: clip_coef = 1 whatever the norm is (a step without clipping)   */

typedef struct hk_optim_tensor {
  void* param;
  void* grad;
  void* state1; /* Adam: exp_avg;    SGD: the momentum buffer */
  void* state2; /* Adam: exp_avg_sq; SGD: unused              */
  int64_t numel;
} hk_optim_tensor;

typedef struct hk_optim_state {
  int64_t step;
  double beta1_pow;
  double beta2_pow;
  double total_norm;    /* a value of T */
  double clip_coef;     /* a value of T */
  double neg_step_size;
  double bias2_sqrt;
  double lr;
} hk_optim_state;

typedef struct hk_optim_desc {
  hk_optim_tensor tensor[HK_OPTIM_MAX_TENSORS];
  void* state;          /* hk_optim_state on the device                                  */
  void* workspace;      /* prepare: hk_optim_workspace_bytes(...) bytes                   */
  const double* lr_dev; /* prepare: NULL, or the learning rate on the device             */
  double lr;
  double beta1;
  double beta2;
  double eps;
  double weight_decay;
  double momentum;
  double dampening;
  double max_norm;
  int32_t ntensors;     /* 0 .. HK_OPTIM_MAX_TENSORS                                      */
  int32_t dtype;        /* HK_F32 or HK_F64, of every tensor                              */
  int32_t kind;         /* HK_OPTIM_SCALE / _SGD / _ADAM                                  */
  int32_t slot_base;    /* prepare: the workgroups of the chain's earlier launches       */
  uint32_t flags;
  int32_t reserved_;
} hk_optim_desc;

uint64_t hk_optim_workspace_bytes(int64_t total_workgroups);
int hk_optim_prepare(const hk_optim_desc* desc, void* stream);
int hk_optim_apply(const hk_optim_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_OPTIM_H */
