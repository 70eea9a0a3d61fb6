// hk_spivakovsky_select: the subset Spivakovsky's host or RandomSpivakovsky picks, as a bit mask, one game per lane
// (hk_spivakovsky.h).
//
// The frame is hk_lane_games.h's, with the launch shape of hk_host_select: slices of one state (m * d elements, made
// odd), the games per block halved from a wave until the slices fit kHostSelectLdsBytes.  Spivakovsky's host computes
// in doubles and overwrites its copy, so its slices hold doubles whatever the dtype (a float32 state is widened while
// it is staged): 16 games per block at (64, 6).  RandomSpivakovsky reads supports only and stages the state as it is.
// HBM traffic: one read of the state, 4 B written per game.
#pragma once

#include "hk_host_select_kernel.h"
#include "hk_spivakovsky.h"

namespace hk {

struct SpivakovskyArgs {
  const void* points;  // [batch] records of `stride` elements; the game is the first m*d
  int32_t* mask_out;
  int64_t stride;
  uint64_t seed, game_offset;
  uint32_t step;
  int batch, m, d, lds_stride, games_per_block;
};

// stage_games into slices of another element type: the wave copies the first n elements of the block's records
// (stride elements apart), kLaneGameBatch loads per lane in flight as copy_slab has them, and converts on the way
template <typename W, typename T>
__device__ inline void stage_games_as(W* lds, const T* src, int64_t stride, int n, int lds_stride, const LaneBlock& b,
                                      int lane) {
  int g = lane / n, e = lane % n;
  const int dg = kWave / n, de = kWave % n;
  const int total = b.ngames * n;
  for (int c0 = lane; c0 < total; c0 += kWave * kLaneGameBatch) {
    T v[kLaneGameBatch];
    int lo[kLaneGameBatch];
    int64_t go[kLaneGameBatch];
#pragma unroll
    for (int u = 0; u < kLaneGameBatch; ++u) {
      lo[u] = g * lds_stride + e;
      go[u] = (b.g0 + g) * stride + e;
      g += dg;
      e += de;
      if (e >= n) {
        e -= n;
        ++g;
      }
    }
    // requests past the end repeat the batch's first (valid) one: every load is unconditional (copy_slab)
#pragma unroll
    for (int u = 1; u < kLaneGameBatch; ++u)
      if (c0 + u * kWave >= total) {
        lo[u] = lo[0];
        go[u] = go[0];
      }
#pragma unroll
    for (int u = 0; u < kLaneGameBatch; ++u) v[u] = src[go[u]];
#pragma unroll
    for (int u = 0; u < kLaneGameBatch; ++u) asm volatile("" : "+v"(v[u]));
#pragma unroll
    for (int u = 0; u < kLaneGameBatch; ++u)
      if (c0 + u * kWave < total) lds[lo[u]] = (W)v[u];
  }
}

// the element type of the slices: doubles for Spivakovsky's host, the state's own for RandomSpivakovsky
template <typename T, int HOST>
using SpivakovskySlice = std::conditional_t<HOST == HK_HOST_SPIVAKOVSKY, double, T>;

template <typename T, int HOST>
__global__ void __launch_bounds__(kWave) spivakovsky_select_kernel(SpivakovskyArgs a) {
  using W = SpivakovskySlice<T, HOST>;
  extern __shared__ unsigned char hk_sp_lds[];
  W* lds = reinterpret_cast<W*>(hk_sp_lds);
  const int lane = threadIdx.x;
  const LaneBlock blk = lane_block(a.batch, a.games_per_block);
  if constexpr (std::is_same<W, T>::value) stage_games(lds, a.points, a.stride, a.m * a.d, a.lds_stride, blk, lane);
  else stage_games_as(lds, static_cast<const T*>(a.points), a.stride, a.m * a.d, a.lds_stride, blk, lane);
  __syncthreads();
  if (lane >= blk.ngames) return;
  W* game = lds + (size_t)lane * a.lds_stride;
  uint32_t mask;
  if constexpr (HOST == HK_HOST_SPIVAKOVSKY) mask = spivakovsky_game(game, a.m, a.d);
  else mask = random_spivakovsky_game<W>(game, a.m, a.d, a.game_offset + (uint64_t)(blk.g0 + lane), a.step, a.seed);
  a.mask_out[blk.g0 + lane] = (int32_t)mask;
}

}  // namespace hk
