/*
 * hironaka_hip_unified.h -- one expansion of the role-agnostic ("unified") search tree of the MCTS trainer (the
 * reference's hironaka/jax/recurrent_fn.py:126-199 get_unified_recurrent_fn and jax/util.py:240-257) without a decision
 * on the host: the kind of the batch is found on the device, the expansion reads it, the two policy-value networks are
 * launched behind a gate on it, and a last kernel selects the prior.  An addition within ABI 6 that a consumer detects
 * by its symbols, part of the C ABI of hironaka_hip.h, which includes this file (after hironaka_hip_pvnet.h, whose
 * descriptor the gated network launch takes); HK_F32 and the status codes are defined there.  The entry points have no
 * counterpart in the CPU oracle: the Python binding lists them in hironaka_amd/_abi.py UNIFIED_PROTOTYPES.
 * Same conventions as hironaka_hip.h: device pointers, no allocation, no synchronisation, an int status.
 *
 * ---- the rule (the reference's, quirks included) ----
 * A state is max_points * dim points followed by a tail of dim floats.  A game's parent embeddings[b, parent[b]] is a
 * HOST state when every tail entry x has |x| <= 1e-8 in float (isclose to 0; a NaN is not close).  The decision is made
 * ONCE PER BATCH: if any game's parent is a host state, every game of the batch is expanded as one (kind 1); only a
 * batch without a host state is expanded as agent states (kind 0).  An agent state in a kind-1 batch is treated as the
 * rule says, not "repaired".
 *   kind 1  next points = the parent's, bit for bit; next tail = the 0 / 1 subset of the class id action[b], clamped
 *           into [0, 2^dim - dim - 1) as hk_decode_host_class clamps; the next node is an agent node
 *   kind 0  next points = hk_step on the parent's points in JAX semantics (shift, [reposition], Newton, no rescale) with
 *           the parent's tail as the float mask and action[b] as the axis (outside [0, dim) it matches nothing);
 *           next tail = zeros; the next node is a host node
 *   reward[b] = -1 * (float)(done and not done before), done = fewer than 2 points, as hk_step's reward output with
 *   reward_sign -1;  discount_out[b] = -discount.
 *
 * ---- hk_unified_expand: two launches ----
 * (a) ORs 1 into *kind when a game's parent is a host state.  The caller zeroes the word before (one word per
 *     expansion, so nothing is ever reset); nothing spins or waits on it.
 * (b) reads *kind and writes, per game b:
 *       embeddings[b, node[b]]   the next state (every game)
 *       net_in[b]                [max_points * dim + dim]: hk_get_features of the next points (rescaled first with
 *                                HK_UNIFIED_SCALE_OBSERVATION), then the next tail: the agent network's input, whose
 *                                first max_points * dim columns are the host network's
 *       subset[b]                the bit mask of the next tail (bit j <-> coordinate j; 0 in kind 0)
 *       reward[b], discount_out[b]
 * embeddings is a contiguous [batch, num_nodes, max_points * dim + dim] float table.  parent[b] and node[b] are node
 * indices in [0, num_nodes), as hk_search_select gives them; the kernels read node 0 for a parent outside and write no
 * state for a node outside.  Served: float, dim 2 .. 5 (the search takes at most 32 actions), any max_points whose slice
 * of 2 * max_points * dim + 2 * dim floats fits 64 KiB of LDS.
 *
 * ---- hk_unified_prior ----
 * prior_out [batch, A], A = 2^dim - dim - 1, and value_out [batch], every element written once:
 *   *kind != 0  prior_out[b, j] = agent_logits[b, j] where j < dim and bit j of subset[b] is set, -inf elsewhere;
 *               value_out[b] = agent_value[b]                 (host_logits / host_value are not read; at dim 2, A = 1:
 *               the agent's second logit is dropped, as the reference's pad by A - dim = -1 crops it)
 *   *kind == 0  prior_out[b, :] = host_logits[b, :]; value_out[b] = host_value[b]     (the agent's are not read)
 * agent_logits is [batch, dim], host_logits [batch, A], the values [batch], all contiguous floats.
 *
 * ---- hk_unified_pvnet_forward ----
 * hk_pvnet_forward behind a gate: the same descriptor, the same validation and status, the same launch shape and the
 * same bits, but every workgroup returns before it touches memory unless *gate == want; the outputs of a launch whose
 * gate is closed are left as they were.  gate NULL is HK_ERR_NULL, not aligned to 4 bytes HK_ERR_ALIGN (after the
 * descriptor's own checks).  One expansion is hk_unified_expand, the agent network gated on kind 1, the host network
 * gated on kind 0, hk_unified_prior: one network's work, not two, and no word of it decided on the host.
 *
 * ---- status, before any launch ----
 * batch == 0 is HK_OK with nothing launched (after the checks of the sizes).  A NULL descriptor or pointer is
 * HK_ERR_NULL; batch < 0, num_nodes < 1, max_points < 1, dim < 2, a table beyond 2^63 bytes, or a written range that
 * shares a byte with another range of the call HK_ERR_SHAPE; another dtype, dim > 5, an unknown flag or a slice beyond
 * the LDS HK_ERR_UNSUPPORTED; a pointer that is not aligned to 4 bytes HK_ERR_ALIGN. */
#ifndef HIRONAKA_HIP_UNIFIED_H
#define HIRONAKA_HIP_UNIFIED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* descriptor flags */
#define HK_UNIFIED_REPOSITION 1u
#define HK_UNIFIED_SCALE_OBSERVATION 2u

typedef struct hk_unified_expand_desc {
  void* embeddings;      /* [batch, num_nodes, max_points * dim + dim], read at parent, written at node */
  const int32_t* parent; /* [batch] */
  const int32_t* action; /* [batch] */
  const int32_t* node;   /* [batch] */
  int32_t* kind;         /* one word, zero on entry */
  void* net_in;          /* [batch, max_points * dim + dim] */
  int32_t* subset;       /* [batch] */
  void* reward;          /* [batch] */
  void* discount_out;    /* [batch] */
  float discount;
  int32_t batch;
  int32_t num_nodes;
  int32_t max_points;
  int32_t dim;
  int32_t dtype; /* HK_F32 */
  uint32_t flags;
} hk_unified_expand_desc;

int hk_unified_expand(const hk_unified_expand_desc* desc, void* stream);

int hk_unified_prior(const int32_t* kind, const void* agent_logits, const void* agent_value, const void* host_logits,
                     const void* host_value, const int32_t* subset, void* prior_out, void* value_out, int batch, int dim,
                     void* stream);

int hk_unified_pvnet_forward(const hk_pvnet_desc* desc, const int32_t* gate, int32_t want, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIRONAKA_HIP_UNIFIED_H */
