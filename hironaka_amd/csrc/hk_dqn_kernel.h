// hk_dqn_td / hk_polyak_update: the arithmetic between ReplayBuffer.sample and loss.backward() of the DQN trainers
// (hironaka/trainer/dqn_trainer/dqn_trainer.py:68-88, :192-204; include/hironaka_hip_dqn.h has the rules).
//
// dqn_td_kernel.  A workgroup of kDqnThreads threads owns kDqnTile consecutive rows, a wave 16 of them.  Lane i of a wave
// first fetches what row i needs besides its maximum: action, reward, done and the one element q[b, a] (two dependent
// loads for the whole wave).  A row's maximum is taken by L = the power of two >= A (at most 64) neighbouring lanes,
// 64 / L rows per pass, so that the lanes of a wave sit on consecutive elements of next_q; the loads of different
// passes do not depend on each other (the index of a row past the wave's last is clamped, nothing is branched around),
// so several passes are in flight together -- as a chain of load, butterfly, dependent load, store per pass the kernel
// took as many memory latencies as a wave had passes.  The butterfly's result goes back to lane i, which computes the
// row's target, x, loss and gradient once and writes target and row_loss; the dq rows are then written pass by pass
// with consecutive lanes on consecutive elements, the row's action and gradient fetched from lane i.  A > 64: a row per
// pass, every lane on columns lane, lane + 64, ...
//
// The loss crosses workgroups: a workgroup's rows are added in double (a fixed tree: lane, wave, workgroup) and ONE lane
// leaves the sum in the workspace slot of the workgroup and draws a ticket; the workgroup whose ticket is the last adds
// the slots in index order (hk_ticket.h, which hk_optim_kernel.h shares: the stores, the loads and why none of them is
// a plain one).  Nobody waits on anybody; the last workgroup zeroes the ticket for the next launch.
//
// polyak_kernel.  The host dealt the workgroups to (tensor, chunk) pairs; the table is the kernel's argument.  A
// workgroup finds its tensor by bisection over the tensors' first workgroups and updates its chunk: 16 bytes per lane
// and transfer where the entry allows it (chunk 0 also serves the elements in front of the first 16-byte boundary and
// behind the last), single elements otherwise.
#pragma once

#include "hk_common.h"
#include "hk_table.h"
#include "hk_ticket.h"

namespace hk {

constexpr int kDqnThreads = 1024;
constexpr int kDqnTile = HK_DQN_TILE_ROWS;
constexpr int kDqnWaves = kDqnThreads / kWave;
constexpr int kDqnWaveRows = kDqnTile / kDqnWaves;  // rows per wave
constexpr int kDqnFlight = 4;     // independent loads of next_q a lane has in flight
constexpr int kDqnSlotOffset = kTicketSlotOffset;

static_assert(kDqnTile % kDqnWaves == 0 && kDqnWaveRows <= kWave, "a lane per row of the wave's share");

struct DqnArgs {
  const void* q;
  const void* next_q;
  const int32_t* actions;
  const float* rewards;
  const uint8_t* dones;
  void* target;
  void* row_loss;
  void* dq;
  void* loss;
  unsigned long long* ws;
  uint32_t* status;
  int64_t q_stride, next_q_stride, dq_stride;
  float gamma;  // (float)desc.gamma
  int32_t batch, num_actions;
  int32_t lanes_log2;  // log2 L
};

// torch.max's order: the larger of the two, NaN if either is
template <typename T>
__device__ __forceinline__ T nan_max(T a, T b) {
  return (b > a || b != b) ? b : a;
}

template <typename T>
__global__ void __launch_bounds__(kDqnThreads) dqn_td_kernel(DqnArgs a) {
  __shared__ double s_wave[kDqnWaves];
  __shared__ double s_slot[kDqnThreads];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int lg = a.lanes_log2, L = 1 << lg, sub = lane & (L - 1), rows_per_pass = kWave >> lg;
  const int A = a.num_actions;
  const int64_t wave0 = (int64_t)blockIdx.x * kDqnTile + (int64_t)wave * kDqnWaveRows;
  const int64_t left = (int64_t)a.batch - wave0;
  const int rows = left < 0 ? 0 : (left < kDqnWaveRows ? (int)left : kDqnWaveRows);  // of this wave
  const int npass = (rows + rows_per_pass - 1) / rows_per_pass;                      // A <= 64
  const T* q = static_cast<const T*>(a.q);
  const T* next_q = static_cast<const T*>(a.next_q);
  T* dq = static_cast<T*>(a.dq);
  const T g = (T)a.gamma;
  const T fB = (T)a.batch;
  // lane i and row i of the wave: everything but the maximum
  const bool mine = lane < rows;
  const int64_t b1 = wave0 + lane;
  int act = -1;
  T rew = (T)0, coef = (T)0, qa = (T)0;
  if (mine) {
    act = a.actions[b1];
    rew = (T)a.rewards[b1];
    coef = a.dones[b1] ? (T)0 : g;
    if (act < 0 || act >= A) act = -1;  // matches no column
    if (act >= 0) qa = q[b1 * a.q_stride + act];
  }
  T mx = -(T)INFINITY;
  if (rows > 0) {  // the same for the whole wave, as are npass and rows: every lane takes part in the exchanges
    const int64_t last = wave0 + rows - 1;
    if (A <= kWave) {
      // kDqnFlight passes at a time: their loads first, all of them in flight together, then the exchanges (a pass past
      // the last loads the wave's last row again and hands it to lanes that own no row)
      for (int p0 = 0; p0 < npass; p0 += kDqnFlight) {
        T m[kDqnFlight];
#pragma unroll
        for (int k = 0; k < kDqnFlight; ++k) {
          int64_t b = wave0 + (p0 + k) * rows_per_pass + (lane >> lg);
          if (b > last) b = last;  // no branch between the loads
          m[k] = sub < A ? next_q[b * a.next_q_stride + sub] : -(T)INFINITY;
        }
#pragma unroll
        for (int k = 0; k < kDqnFlight; ++k) {
          const int first = (p0 + k) * rows_per_pass;  // the pass's first row
          // every step is taken and the wide ones dropped: no loop of L's own length
#pragma unroll
          for (int s = kWave / 2; s > 0; s >>= 1) {
            const T other = __shfl_xor(m[k], s, kWave);
            if (s < L) m[k] = nan_max(m[k], other);
          }
          // row first + j sits in lanes j * L ..: lane i takes its row's from the first of them (one value per row,
          // whatever order the butterfly met a +0 and a -0 in)
          const T v = __shfl(m[k], ((lane - first) << lg) & (kWave - 1), kWave);
          if (lane >= first && lane < first + rows_per_pass) mx = v;
        }
      }
    } else {
      for (int r = 0; r < rows; ++r) {
        const T* row = next_q + (wave0 + r) * a.next_q_stride;
        T m = -(T)INFINITY;
        for (int c0 = lane; c0 < A; c0 += kWave * kDqnFlight) {
          T v[kDqnFlight];
#pragma unroll
          for (int k = 0; k < kDqnFlight; ++k) {
            const int c = c0 + k * kWave;
            v[k] = row[c < A ? c : A - 1];  // the last column again rather than a branch: the maximum does not mind
          }
#pragma unroll
          for (int k = 0; k < kDqnFlight; ++k) m = nan_max(m, v[k]);
        }
#pragma unroll
        for (int s = kWave / 2; s > 0; s >>= 1) m = nan_max(m, __shfl_xor(m, s, kWave));
        m = __shfl(m, 0, kWave);
        if (lane == r) mx = m;
      }
    }
  }
  const bool ok = act >= 0;
  const T tgt = rew + coef * mx;
  const T x = qa - tgt;
  const T ax = x < (T)0 ? -x : x;
  const T rl = ok ? (ax < (T)1 ? (T)0.5 * x * x : ax - (T)0.5) : (T)0;
  const T gr = ok ? (x < (T)-1 ? (T)-1 : (x > (T)1 ? (T)1 : x)) / fB : (T)0;
  double acc = 0.0;
  bool bad = false;
  if (mine) {
    if (a.target) static_cast<T*>(a.target)[b1] = tgt;
    if (a.row_loss) static_cast<T*>(a.row_loss)[b1] = rl;
    acc = (double)rl;
    bad = !ok;
  }
  if (rows > 0) {
    if (A <= kWave) {
      for (int p = 0; p < npass; ++p) {
        const int r = p * rows_per_pass + (lane >> lg);
        const int ar = __shfl(act, r & (kWave - 1), kWave);
        const T gv = __shfl(gr, r & (kWave - 1), kWave);
        if (r < rows && sub < A) dq[(wave0 + r) * a.dq_stride + sub] = sub == ar ? gv : (T)0;
      }
    } else {
      for (int r = 0; r < rows; ++r) {
        const int ar = __shfl(act, r, kWave);
        const T gv = __shfl(gr, r, kWave);
        T* out = dq + (wave0 + r) * a.dq_stride;
        for (int c = lane; c < A; c += kWave) out[c] = c == ar ? gv : (T)0;
      }
    }
  }
  if (bad) __hip_atomic_fetch_or(a.status, (uint32_t)HK_DQN_BAD_ACTION, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) acc += __shfl_down(acc, s, kWave);
  if (lane == 0) s_wave[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    double part = s_wave[0];
#pragma unroll
    for (int w = 1; w < kDqnWaves; ++w) part += s_wave[w];
    slot_store(a.ws + kDqnSlotOffset + blockIdx.x, part);
    s_last = ticket_draw(a.ws, gridDim.x);
  }
  __syncthreads();
  if (!s_last) return;  // the same for the whole workgroup
  const double total = ticket_sum<kDqnThreads>(a.ws, gridDim.x, s_slot, tid);
  if (tid == 0) {
    *static_cast<T*>(a.loss) = (T)(total / (double)a.batch);
    ticket_reset(a.ws);
  }
}

// ---- hk_polyak_update -------------------------------------------------------------------------------------------------

constexpr int kPolyakThreads = 256;
constexpr int kPolyakUnroll = 4;  // transfers per lane
constexpr int kPolyakChunkBytes = HK_POLYAK_CHUNK_BYTES;

static_assert(kPolyakChunkBytes == kPolyakThreads * kPolyakUnroll * 16, "a chunk is 4 transfers of 16 bytes per lane");

struct PolyakTensor {
  const void* src;
  void* dst;
  int64_t numel;
  int32_t head;  // elements in front of the first 16-byte boundary; -1: src and dst disagree, element by element
  int32_t pad_;
};

struct PolyakArgs {
  PolyakTensor t[HK_POLYAK_MAX_TENSORS];
  uint32_t first[HK_POLYAK_MAX_TENSORS + 1];  // the first workgroup of every tensor; first[ntensors] = the grid
  double tau, rest;                           // tau, 1 - tau
  int32_t ntensors;
};

template <typename T>
__device__ __forceinline__ T polyak_one(T tau, T rest, T s, T d) {
  const T scaled = d * rest;  // rounded: -ffp-contract=off keeps it out of the fma
  return hk_fma<T>(tau, s, scaled);
}

template <typename T>
__global__ void __launch_bounds__(kPolyakThreads) polyak_kernel(PolyakArgs a) {
  constexpr int VE = 16 / (int)sizeof(T);  // elements per transfer
  typedef T Vec __attribute__((ext_vector_type(VE)));
  const int tid = threadIdx.x;
  const int lo = table_find(a.first, a.ntensors, blockIdx.x);
  const PolyakTensor t = a.t[lo];
  const int64_t chunk = (int64_t)(blockIdx.x - a.first[lo]);
  const T tau = (T)a.tau, rest = (T)a.rest;
  const T* src = static_cast<const T*>(t.src);
  T* dst = static_cast<T*>(t.dst);
  if (t.head < 0) {
    constexpr int64_t per = kPolyakChunkBytes / (int64_t)sizeof(T);
    const int64_t begin = chunk * per;
    const int64_t end = begin + per < t.numel ? begin + per : t.numel;
    for (int64_t i = begin + tid; i < end; i += kPolyakThreads) dst[i] = polyak_one<T>(tau, rest, src[i], dst[i]);
    return;
  }
  const int64_t head = t.head;  // < VE <= numel's share in front of the boundary (the host clipped it to numel)
  const int64_t nvec = (t.numel - head) / VE;
  const int64_t tail0 = head + nvec * VE;
  if (chunk == 0) {
    if (tid < head) dst[tid] = polyak_one<T>(tau, rest, src[tid], dst[tid]);
    const int64_t i = tail0 + tid;
    if (i < t.numel) dst[i] = polyak_one<T>(tau, rest, src[i], dst[i]);
  }
  const Vec* vs = reinterpret_cast<const Vec*>(src + head);
  Vec* vd = reinterpret_cast<Vec*>(dst + head);
  const int64_t v0 = chunk * (kPolyakThreads * kPolyakUnroll);
  Vec s[kPolyakUnroll], d[kPolyakUnroll];
#pragma unroll
  for (int k = 0; k < kPolyakUnroll; ++k) {
    const int64_t v = v0 + k * kPolyakThreads + tid;
    if (v < nvec) {
      s[k] = vs[v];
      d[k] = vd[v];
    }
  }
#pragma unroll
  for (int k = 0; k < kPolyakUnroll; ++k) {
    const int64_t v = v0 + k * kPolyakThreads + tid;
    if (v < nvec) {
      Vec r;
#pragma unroll
      for (int e = 0; e < VE; ++e) r[e] = polyak_one<T>(tau, rest, s[k][e], d[k][e]);
      vd[v] = r;
    }
  }
}

}  // namespace hk
