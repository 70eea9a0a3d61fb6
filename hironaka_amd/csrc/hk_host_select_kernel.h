// hk_host_select: the class id a deterministic host of hironaka/host.py picks, one game per lane (hk_hosts.h).
//
// A workgroup is one wave that owns `games_per_block` consecutive games.  It stages their rows into LDS with the
// coalesced slab copy of the generic kernel (odd per-game stride: lane g walks its own game conflict-free), with
// kHostSelectBatch loads per lane in flight, then lane g decides game g alone.  HBM traffic: one read of the state,
// 4 B written per game.  HK_HOST_ALL_COORD reads nothing.
#pragma once

#include "hk_generic_kernel.h"
#include "hk_hosts.h"

namespace hk {

constexpr int kHostSelectLdsBytes = 64 * 1024;  // per workgroup
constexpr int kHostSelectBatch = 16;            // loads per lane in flight while staging

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
  const int64_t g0 = (int64_t)blockIdx.x * a.games_per_block;
  const int64_t left = (int64_t)a.batch - g0;
  const int ngames = left < a.games_per_block ? (int)left : a.games_per_block;
  if (HOST == HK_HOST_ALL_COORD) {
    if (lane < ngames) a.class_out[g0 + lane] = encode_mask((1u << a.d) - 1u);
    return;
  }
  copy_slab<T, true, kHostSelectBatch>(lds, const_cast<T*>(static_cast<const T*>(a.points)), a.stride, a.m * a.d,
                                       a.lds_stride, g0, ngames, lane);
  __syncthreads();
  if (lane < ngames) a.class_out[g0 + lane] = host_class_game<T, HOST>(lds + (size_t)lane * a.lds_stride, a.m, a.d);
}

}  // namespace hk
