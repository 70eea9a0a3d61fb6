// hk_optim_prepare / hk_optim_apply: gradient clipping and the Adam / SGD step of a whole parameter list in two launches
// (hironaka/trainer/dqn_trainer/dqn_trainer.py:95-98; include/hironaka_hip_optim.h has the rules).
//
// Both kernels deal their workgroups to (tensor, chunk) pairs as polyak_kernel does (hk_table.h): the table is the
// kernel's argument, a workgroup finds its tensor by bisection over the tensors' first workgroups.
//
// optim_prepare_kernel.  A chunk is kOptimChunkBytes of one gradient counted from its first element, wherever that
// lies: which elements a lane adds, and in which order, must not depend on the alignment, or the norm's last bit would.
// Lane l loads elements l, l + 256, ... of the chunk (all loads in flight together, consecutive lanes on consecutive
// elements), adds their squares in double in that order; wave: a halving tree; workgroup: the 4 waves in order; then
// the slot and, in the chain's last launch, the ticket (hk_ticket.h).  The workgroup with the last ticket adds the
// slots in index order and its lane 0 writes the state block, which the next launch on the stream reads.
//
// optim_apply_kernel.  polyak_kernel's chunking: 16 bytes per lane and transfer where the entry allows it (chunk 0 also
// serves the elements in front of the first 16-byte boundary and behind the last), single elements otherwise.  All
// loads of a lane's 4 transfers are issued before the arithmetic.  At worst 4 loads and 4 stores per element (Adam with
// the clipped gradient written back): the kernel is bound by memory.
#pragma once

#include "hk_table.h"
#include "hk_ticket.h"

namespace hk {

constexpr int kOptimThreads = 256;
constexpr int kOptimWaves = kOptimThreads / kWave;
constexpr int kOptimUnroll = 4;  // transfers per lane
constexpr int kOptimChunkBytes = HK_OPTIM_CHUNK_BYTES;

static_assert(kOptimChunkBytes == kOptimThreads * kOptimUnroll * 16, "a chunk is 4 transfers of 16 bytes per lane");

struct OptimArgs {
  hk_optim_tensor t[HK_OPTIM_MAX_TENSORS];
  uint32_t first[HK_OPTIM_MAX_TENSORS + 1];  // the first workgroup of every tensor; first[ntensors] = blocks
  int8_t head[HK_OPTIM_MAX_TENSORS];  // apply: elements in front of the first 16-byte boundary; -1: element by element
  hk_optim_state* state;
  unsigned long long* ws;
  const double* lr_dev;
  double lr, beta1, beta2, eps, weight_decay, momentum, dampening, max_norm;
  int32_t ntensors;
  int32_t slot_base;
  uint32_t blocks;  // workgroups that own a chunk (prepare's last launch of a chain has one even without any)
  uint32_t flags;
};
static_assert(sizeof(OptimArgs) <= 4096, "the table travels as the kernel's argument");

template <typename T>
__device__ __forceinline__ T hk_sqrt(T x);
template <>
__device__ __forceinline__ float hk_sqrt<float>(float x) {
  return sqrtf(x);
}
template <>
__device__ __forceinline__ double hk_sqrt<double>(double x) {
  return sqrt(x);
}

template <typename T>
__global__ void __launch_bounds__(kOptimThreads) optim_prepare_kernel(OptimArgs a) {
  constexpr int kPer = kOptimChunkBytes / (int)sizeof(T);  // elements of a chunk
  constexpr int kLoads = kPer / kOptimThreads;
  __shared__ double s_wave[kOptimWaves];
  __shared__ double s_slot[kOptimThreads];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const bool owns = blockIdx.x < a.blocks;  // the same for the whole workgroup
  double acc = 0.0;
  if (owns) {
    const int lo = table_find(a.first, a.ntensors, blockIdx.x);
    const int64_t numel = a.t[lo].numel;
    const T* g = static_cast<const T*>(a.t[lo].grad);
    const int64_t begin = (int64_t)(blockIdx.x - a.first[lo]) * kPer;
    T v[kLoads];
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
      const int64_t i = begin + k * kOptimThreads + tid;
      v[k] = i < numel ? g[i] : (T)0;
    }
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
      const double sq = (double)v[k] * (double)v[k];
      acc += sq;
    }
  }
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) acc += __shfl_down(acc, s, kWave);
  if (lane == 0) s_wave[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    if (owns) {
      double part = s_wave[0];
#pragma unroll
      for (int w = 1; w < kOptimWaves; ++w) part += s_wave[w];
      slot_store(a.ws + kTicketSlotOffset + (uint32_t)a.slot_base + blockIdx.x, part);
    }
    s_last = (a.flags & HK_OPTIM_LAST) ? (int)ticket_draw(a.ws, gridDim.x) : 0;
  }
  __syncthreads();
  if (!s_last) return;  // the same for the whole workgroup
  const double total = ticket_sum<kOptimThreads>(a.ws, (uint32_t)a.slot_base + a.blocks, s_slot, tid);
  if (tid != 0) return;
  hk_optim_state* st = a.state;
  const T norm = (T)sqrt(total);
  const T inv = (T)1 / (norm + (T)1e-6);  // torch: max_norm / tensor is tensor.reciprocal() * max_norm
  const T c = inv * (T)a.max_norm;
  const T coef = (a.flags & HK_OPTIM_NO_CLIP) ? (T)1 : (c > (T)1 ? (T)1 : c);  // a NaN stays, as in torch.clamp
  const double lr = a.lr_dev ? *a.lr_dev : a.lr;
  st->total_norm = (double)norm;
  st->clip_coef = (double)coef;
  st->lr = lr;
  if (a.flags & HK_OPTIM_ADVANCE) {
    const double b1 = st->beta1_pow * a.beta1, b2 = st->beta2_pow * a.beta2;
    st->step = st->step + 1;
    st->beta1_pow = b1;
    st->beta2_pow = b2;
    st->neg_step_size = -(lr / (1.0 - b1));
    st->bias2_sqrt = sqrt(1.0 - b2);
  }
  ticket_reset(a.ws);
}

// the step's constants in T
template <typename T>
struct OptimConst {
  T coef, wd, mu, rest_damp, neg_lr;               // SGD: 1 - dampening, -lr
  T w1, rest_w1, rest_b2, beta2, bias2_sqrt, eps, neg_step_size;  // Adam: 1 - beta1, 1 - w1, 1 - beta2
  bool has_wd, has_mu, first, plain_damp, nesterov, low_weight;
};

template <typename T>
__device__ __forceinline__ OptimConst<T> optim_const(const OptimArgs& a) {
  const hk_optim_state* st = a.state;
  OptimConst<T> c;
  c.coef = (T)st->clip_coef;
  c.wd = (T)a.weight_decay;
  c.mu = (T)a.momentum;
  c.rest_damp = (T)(1.0 - a.dampening);
  c.neg_lr = (T)(-st->lr);
  c.w1 = (T)(1.0 - a.beta1);
  c.rest_w1 = (T)1 - c.w1;
  c.rest_b2 = (T)(1.0 - a.beta2);
  c.beta2 = (T)a.beta2;
  c.bias2_sqrt = (T)st->bias2_sqrt;
  c.eps = (T)a.eps;
  c.neg_step_size = (T)st->neg_step_size;
  c.has_wd = a.weight_decay != 0.0;
  c.has_mu = a.momentum != 0.0;
  c.first = st->step == 1;
  c.plain_damp = a.dampening == 0.0;
  c.nesterov = (a.flags & HK_OPTIM_NESTEROV) != 0;
  c.low_weight = c.w1 < (T)0.5;
  return c;
}

// one element: g becomes the clipped gradient, p / m / v the updated parameter and state (-ffp-contract=off: every
// product below is rounded before it is added unless it is written hk_fma)
template <typename T, int KIND>
__device__ __forceinline__ void optim_one(const OptimConst<T>& c, T& p, T& g, T& m, T& v) {
  g = g * c.coef;
  if (KIND == HK_OPTIM_SCALE) return;
  T d = g;
  if (c.has_wd) d = hk_fma<T>(c.wd, p, d);
  if (KIND == HK_OPTIM_SGD) {
    if (c.has_mu) {
      if (c.first) {
        m = d;
      } else {
        const T scaled = m * c.mu;
        m = c.plain_damp ? scaled + d : hk_fma<T>(c.rest_damp, d, scaled);
      }
      d = c.nesterov ? hk_fma<T>(c.mu, m, d) : m;
    }
    p = hk_fma<T>(c.neg_lr, d, p);
  } else {
    const T diff = d - m;
    m = c.low_weight ? hk_fma<T>(c.w1, diff, m) : hk_fma<T>(-diff, c.rest_w1, d);
    const T gw = c.rest_b2 * d;
    const T scaled = v * c.beta2;
    v = hk_fma<T>(gw, d, scaled);
    const T root = hk_sqrt<T>(v);
    const T scaled_root = root / c.bias2_sqrt;
    const T denom = scaled_root + c.eps;
    const T num = c.neg_step_size * m;
    const T upd = num / denom;
    p = p + upd;
  }
}

template <typename T, int KIND>
__device__ __forceinline__ void optim_scalar(const OptimConst<T>& c, const hk_optim_tensor& t, int64_t i, bool keep) {
  T* P = static_cast<T*>(t.param);
  T* G = static_cast<T*>(t.grad);
  T* M = static_cast<T*>(t.state1);
  T* V = static_cast<T*>(t.state2);
  const bool use_m = KIND == HK_OPTIM_ADAM || (KIND == HK_OPTIM_SGD && c.has_mu);
  T p = (T)0, m = (T)0, v = (T)0;
  T g = G[i];
  if (KIND != HK_OPTIM_SCALE) p = P[i];
  if (use_m) m = M[i];
  if (KIND == HK_OPTIM_ADAM) v = V[i];
  optim_one<T, KIND>(c, p, g, m, v);
  if (!keep) G[i] = g;
  if (KIND != HK_OPTIM_SCALE) P[i] = p;
  if (use_m) M[i] = m;
  if (KIND == HK_OPTIM_ADAM) V[i] = v;
}

template <typename T, int KIND>
__global__ void __launch_bounds__(kOptimThreads) optim_apply_kernel(OptimArgs a) {
  constexpr int VE = 16 / (int)sizeof(T);  // elements per transfer
  typedef T Vec __attribute__((ext_vector_type(VE)));
  const int tid = threadIdx.x;
  const int lo = table_find(a.first, a.ntensors, blockIdx.x);
  const hk_optim_tensor t = a.t[lo];
  const int64_t chunk = (int64_t)(blockIdx.x - a.first[lo]);
  const OptimConst<T> c = optim_const<T>(a);
  const bool keep = (a.flags & HK_OPTIM_KEEP_GRADS) != 0;
  const bool use_m = KIND == HK_OPTIM_ADAM || (KIND == HK_OPTIM_SGD && c.has_mu);
  const int head8 = a.head[lo];
  if (head8 < 0) {
    constexpr int64_t per = kOptimChunkBytes / (int64_t)sizeof(T);
    const int64_t begin = chunk * per;
    const int64_t end = begin + per < t.numel ? begin + per : t.numel;
    for (int64_t i = begin + tid; i < end; i += kOptimThreads) optim_scalar<T, KIND>(c, t, i, keep);
    return;
  }
  const int64_t head = head8;  // < VE, and the host clipped it to numel
  const int64_t nvec = (t.numel - head) / VE;
  const int64_t tail0 = head + nvec * VE;
  if (chunk == 0) {
    if (tid < head) optim_scalar<T, KIND>(c, t, tid, keep);
    const int64_t i = tail0 + tid;
    if (i < t.numel) optim_scalar<T, KIND>(c, t, i, keep);
  }
  Vec* vp = reinterpret_cast<Vec*>(static_cast<T*>(t.param) + head);
  Vec* vg = reinterpret_cast<Vec*>(static_cast<T*>(t.grad) + head);
  Vec* vm = reinterpret_cast<Vec*>(static_cast<T*>(t.state1) + head);
  Vec* vv = reinterpret_cast<Vec*>(static_cast<T*>(t.state2) + head);
  const int64_t v0 = chunk * (kOptimThreads * kOptimUnroll);
  Vec p[kOptimUnroll], g[kOptimUnroll], m[kOptimUnroll], v[kOptimUnroll];
#pragma unroll
  for (int k = 0; k < kOptimUnroll; ++k) {
    const int64_t x = v0 + k * kOptimThreads + tid;
    p[k] = g[k] = m[k] = v[k] = (Vec)(T)0;
    if (x < nvec) {
      g[k] = vg[x];
      if (KIND != HK_OPTIM_SCALE) p[k] = vp[x];
      if (use_m) m[k] = vm[x];
      if (KIND == HK_OPTIM_ADAM) v[k] = vv[x];
    }
  }
#pragma unroll
  for (int k = 0; k < kOptimUnroll; ++k) {
    const int64_t x = v0 + k * kOptimThreads + tid;
    if (x < nvec) {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        T pe = p[k][e], ge = g[k][e], me = m[k][e], ve = v[k][e];
        optim_one<T, KIND>(c, pe, ge, me, ve);
        p[k][e] = pe;
        g[k][e] = ge;
        m[k][e] = me;
        v[k][e] = ve;
      }
      if (!keep) vg[x] = g[k];
      if (KIND != HK_OPTIM_SCALE) vp[x] = p[k];
      if (use_m) vm[x] = m[k];
      if (KIND == HK_OPTIM_ADAM) vv[x] = v[k];
    }
  }
}

}  // namespace hk
