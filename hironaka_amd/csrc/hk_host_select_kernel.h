// hk_host_select: the class id a deterministic host of hironaka/host.py picks, one game per lane (hk_hosts.h).
//
// The frame is hk_lane_games.h's, with slices of one state (m * d elements, made odd) and a launch shape of its own: the
// games per block halve from a wave until their slices fit kHostSelectLdsBytes.  HBM traffic: one read of the state,
// 4 B written per game.  HK_HOST_ALL_COORD reads nothing.
#pragma once

#include "hk_lane_games.h"

namespace hk {

constexpr int kHostSelectLdsBytes = 64 * 1024;  // per workgroup

struct HostSelectArgs {
  const void* points;  // [batch] records of `stride` elements; the game is the first m*d
  int32_t* class_out;
  int64_t stride;
  int batch, m, d, lds_stride, games_per_block;
};

template <typename T, int HOST>
__global__ void __launch_bounds__(kWave) host_select_kernel(HostSelectArgs a) {
  extern __shared__ unsigned char hk_hs_lds[];
  T* lds = reinterpret_cast<T*>(hk_hs_lds);
  const int lane = threadIdx.x;
  const LaneBlock blk = lane_block(a.batch, a.games_per_block);
  const int64_t g0 = blk.g0;
  const int ngames = blk.ngames;
  if (HOST == HK_HOST_ALL_COORD) {
    if (lane < ngames) a.class_out[g0 + lane] = encode_mask((1u << a.d) - 1u);
    return;
  }
  stage_games(lds, a.points, a.stride, a.m * a.d, a.lds_stride, blk, lane);
  __syncthreads();
  if (lane < ngames) a.class_out[g0 + lane] = host_class_game<T, HOST>(lds + (size_t)lane * a.lds_stride, a.m, a.d);
}

}  // namespace hk
