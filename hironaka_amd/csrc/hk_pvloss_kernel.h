// hk_pv_loss: policy_value_loss (hironaka/jax/loss.py:12-24) and its gradient with respect to logits and value, the
// sampled rows of the targets gathered on the way (include/hironaka_hip_pvloss.h has the rule).
//
// pv_loss_kernel.  The launch is a few thousand elements and latency-bound, so every row is evaluated in double and the
// layout serves the chain of dependent loads, not the arithmetic.  A workgroup of kPvLossThreads threads owns kPvLossTile
// consecutive rows, a wave kPvLossWaveRows of them.  A row belongs to L = the power of two >= A (at most 64)
// neighbouring lanes, 64 / L rows per pass, every lane on the columns sub, sub + L, ... (at most kPvLossCols of them: one
// where A <= 64), so that the lanes of a wave sit on consecutive elements of logits, target_policy and dlogits.  With the
// test config's A = 3 or 4 a wave plays its four rows in one pass, with A = 255 in four.  A pass is: the row's index,
// then its logits, targets, value, target value and weight (independent loads, in flight together), the two maxima, the
// two sums of exponentials, the sum of q and of q * logp -- five butterflies over the row's lanes, which leave every
// lane with the row's figure -- and the stores.  A lane group past the wave's last row repeats that row and stores
// nothing: nothing is branched around the exchanges.
//
// The loss crosses workgroups as hk_dqn_td's does: a workgroup's rows are added in double (a fixed tree: lane, wave,
// workgroup) and ONE lane leaves the sum in the workspace slot of the workgroup and draws a ticket; the workgroup whose
// ticket is the last adds the slots in index order (hk_ticket.h).  Nobody waits on anybody; the last workgroup zeroes the
// ticket for the next launch.
#pragma once

#include "hk_common.h"
#include "hk_ticket.h"

namespace hk {

constexpr int kPvLossThreads = 256;
constexpr int kPvLossTile = HK_PVLOSS_TILE_ROWS;
constexpr int kPvLossWaves = kPvLossThreads / kWave;
constexpr int kPvLossWaveRows = kPvLossTile / kPvLossWaves;  // rows per wave
constexpr int kPvLossCols = (HK_PVLOSS_MAX_ACTIONS + kWave - 1) / kWave;  // columns a lane holds at most
constexpr int kPvLossSlotOffset = kTicketSlotOffset;

static_assert(kPvLossTile % kPvLossWaves == 0 && kPvLossWaveRows <= kWave, "a lane group per row of the wave's share");

struct PvLossArgs {
  const float* logits;
  const float* value;
  const float* target_policy;
  const float* target_value;
  const float* weight;
  const int64_t* index;
  float* dlogits;
  float* dvalue;
  float* row_loss;
  float* loss;
  unsigned long long* ws;
  uint32_t* status;
  int64_t logits_stride, value_stride, target_policy_stride, dlogits_stride, dvalue_stride;
  int64_t num_samples;
  int32_t batch, actions;
  int32_t lanes_log2;  // log2 L
};

// the larger of the two, NaN if either is: both lanes of an exchange end with the same value
__device__ __forceinline__ double pv_max(double a, double b) { return (b > a || b != b) ? b : a; }

// over the L lanes of a row: every step of the butterfly is taken and the wide ones dropped (no loop of L's own length);
// a + b is b + a, so every lane of the row ends with the same bits
__device__ __forceinline__ double row_max(double v, int L) {
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) {
    const double other = __shfl_xor(v, s, kWave);
    if (s < L) v = pv_max(v, other);
  }
  return v;
}
__device__ __forceinline__ double row_sum(double v, int L) {
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) {
    const double other = __shfl_xor(v, s, kWave);
    if (s < L) v += other;
  }
  return v;
}

__global__ void __launch_bounds__(kPvLossThreads) pv_loss_kernel(PvLossArgs a) {
  __shared__ double s_wave[kPvLossWaves];
  __shared__ double s_slot[kPvLossThreads];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int lg = a.lanes_log2, L = 1 << lg, sub = lane & (L - 1), rows_per_pass = kWave >> lg;
  const int A = a.actions;
  const int64_t wave0 = (int64_t)blockIdx.x * kPvLossTile + (int64_t)wave * kPvLossWaveRows;
  const int64_t left = (int64_t)a.batch - wave0;
  const int rows = left < 0 ? 0 : (left < kPvLossWaveRows ? (int)left : kPvLossWaveRows);  // of this wave
  const int npass = (rows + rows_per_pass - 1) / rows_per_pass;  // the same for the whole wave
  const double dA = (double)A, dB = (double)a.batch, dAB = dA * dB;
  double acc = 0.0;
  bool bad = false;
  for (int p = 0; p < npass; ++p) {
    const int r = p * rows_per_pass + (lane >> lg);
    const bool live = r < rows;
    const int64_t b = wave0 + (live ? r : rows - 1);
    int64_t s = a.index ? a.index[b] : b;
    const bool ok = s >= 0 && s < a.num_samples;
    if (!ok) s = 0;  // read in bounds; nothing of it is kept
    const float* xrow = a.logits + b * a.logits_stride;
    const float* trow = a.target_policy + s * a.target_policy_stride;
    float x[kPvLossCols], t[kPvLossCols];
#pragma unroll
    for (int k = 0; k < kPvLossCols; ++k) {
      const int c = sub + k * L;
      x[k] = c < A ? xrow[c] : -INFINITY;
      t[k] = c < A ? trow[c] : -INFINITY;
    }
    const double v = (double)a.value[b * a.value_stride], tv = (double)a.target_value[s];
    const double w = a.weight ? (double)a.weight[s] : 1.0;
    double xm = (double)x[0], tm = (double)t[0];
#pragma unroll
    for (int k = 1; k < kPvLossCols; ++k) {
      xm = pv_max(xm, (double)x[k]);
      tm = pv_max(tm, (double)t[k]);
    }
    xm = row_max(xm, L);
    tm = row_max(tm, L);
    double dx[kPvLossCols], et[kPvLossCols], sx = 0.0, st = 0.0;
#pragma unroll
    for (int k = 0; k < kPvLossCols; ++k) {
      dx[k] = et[k] = 0.0;
      if (sub + k * L < A) {
        dx[k] = (double)x[k] - xm;
        et[k] = exp((double)t[k] - tm);
        sx += exp(dx[k]);
        st += et[k];
      }
    }
    sx = row_sum(sx, L);
    st = row_sum(st, L);
    const double lse = log(sx);
    double q[kPvLossCols], pr[kPvLossCols], sq = 0.0, cross = 0.0;
#pragma unroll
    for (int k = 0; k < kPvLossCols; ++k) {
      q[k] = pr[k] = 0.0;
      if (sub + k * L < A) {
        q[k] = et[k] / st;
        const double lp = dx[k] - lse;
        pr[k] = exp(lp);
        sq += q[k];
        if (q[k] != 0.0) cross += q[k] * lp;  // a NaN is not 0: it stays
      }
    }
    sq = row_sum(sq, L);
    cross = row_sum(cross, L);
    if (live) {
      float* out = a.dlogits + b * a.dlogits_stride;
#pragma unroll
      for (int k = 0; k < kPvLossCols; ++k) {
        const int c = sub + k * L;
        if (c < A) out[c] = ok ? (float)(w * (pr[k] * sq - q[k]) / dAB) : 0.0f;
      }
      if (sub == 0) {
        const double d = v - tv;
        const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : d);  // 0 stays 0, NaN stays NaN
        const double row = ok ? (-cross / dA + fabs(d)) * w : 0.0;
        a.dvalue[b * a.dvalue_stride] = ok ? (float)(w * sg / dB) : 0.0f;
        if (a.row_loss) a.row_loss[b] = (float)row;
        acc += row;
        bad = bad || !ok;
      }
    }
  }
  if (bad) __hip_atomic_fetch_or(a.status, (uint32_t)HK_PVLOSS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) acc += __shfl_down(acc, s, kWave);
  if (lane == 0) s_wave[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    double part = s_wave[0];
#pragma unroll
    for (int w = 1; w < kPvLossWaves; ++w) part += s_wave[w];
    slot_store(a.ws + kPvLossSlotOffset + blockIdx.x, part);
    s_last = ticket_draw(a.ws, gridDim.x);
  }
  __syncthreads();
  if (!s_last) return;  // the same for the whole workgroup
  const double total = ticket_sum<kPvLossThreads>(a.ws, gridDim.x, s_slot, tid);
  if (tid == 0) {
    *a.loss = (float)(total / dB);
    ticket_reset(a.ws);
  }
}

}  // namespace hk
