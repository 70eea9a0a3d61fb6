// hk_replay_push / hk_replay_sample: the DQN trainers' replay buffer (hironaka/trainer/replay_buffer.py) as a ring
// whose cursor lives on the device (include/hironaka_hip_replay.h).
//
// Push is a stable compaction into the ring.  A workgroup of kReplayThreads threads owns kReplayTile consecutive rows
// of the batch.  It counts the kept rows in front of its tile itself, from the keep bytes (at most `batch` bytes, 16
// per lane and load, served by L2), so where its rows go depends on the keep array and the cursor alone: no slot is
// reserved with an atomic, and no workgroup waits for another.  The kept rows of the tile are listed in LDS in batch
// order, and every column is copied unit by unit (16 bytes, 4 bytes or 1 byte, whatever the column's pointers and
// sizes allow) with consecutive lanes on consecutive units of the destination, which is one run of the ring, or two at
// the wrap.
//
// The cursor is read by every workgroup and rewritten once all of them have read it: each workgroup draws a ticket from
// cursor word 5 AFTER its cursor words have arrived (lane 0 has parked them in LDS and the workgroup has passed a
// barrier), and the workgroup that draws the last ticket writes the new cursor and zeroes the ticket.  Nothing a
// workgroup computes passes to another: the last one counts the kept rows behind its tile itself to know the push's
// total.  Cursor and ticket are touched with agent-scope atomics only, which are served where every XCD sees them.
// Sample uses the same ticket to advance samples_drawn.  Every loop is bounded by the batch, a tile or a row.
// Tickets on one address are served one after the other, about 12 ns each: 64-row tiles (1024 workgroups at 65 536
// rows) made the push 6 us slower than 128-row tiles (profiles/replay_probe.json has the latter).
#pragma once

#include "hk_common.h"

namespace hk {

constexpr int kReplayThreads = 256;
constexpr int kReplayTile = HK_REPLAY_TILE_ROWS;
constexpr int kReplayUnroll = 4;                 // units per lane in flight
constexpr int64_t kReplayMaxRowBytes = 1 << 20;  // a tile's units are counted in 32 bits

static_assert(kReplayTile % kWave == 0 && kReplayTile <= kReplayThreads, "a lane per row of the tile");

struct ReplayCol {
  char* ring;
  char* rows;
  int64_t stride;     // of `rows`, bytes
  int32_t row_bytes;
  int32_t vec;        // bytes per access: 16, 4 or 1
};

struct ReplayArgs {
  ReplayCol col[HK_REPLAY_MAX_COLS];
  const uint8_t* keep;
  unsigned long long* cursor;
  int64_t* index_out;
  uint64_t seed;
  int32_t ncols, batch, capacity, batch_size;
};

__device__ __forceinline__ unsigned long long cursor_load(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void cursor_store(unsigned long long* p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// whether this workgroup is the last of the launch to have read the cursor
__device__ __forceinline__ bool draw_ticket(unsigned long long* cursor) {
  const unsigned long long old =
      __hip_atomic_fetch_add(cursor + HK_REPLAY_TICKET, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return old == (unsigned long long)gridDim.x - 1ull;
}

__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x) {
  return (uint32_t)__popc((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u);
}
// the bytes lo <= b < hi of a dword as a mask
__device__ __forceinline__ uint32_t byte_range_mask(int64_t lo, int64_t hi) {
  const uint32_t below_hi = hi >= 4 ? 0xFFFFFFFFu : (hi <= 0 ? 0u : (1u << (8 * (int)hi)) - 1u);
  const uint32_t below_lo = lo >= 4 ? 0xFFFFFFFFu : (lo <= 0 ? 0u : (1u << (8 * (int)lo)) - 1u);
  return below_hi & ~below_lo;
}

// this lane's share of the nonzero bytes of keep[begin, end): the aligned 16-byte pieces that hold the range, the
// bytes of the first and last piece outside it masked off
__device__ inline uint32_t count_kept(const uint8_t* keep, int64_t begin, int64_t end, int tid) {
  if (end <= begin) return 0u;
  const uint8_t* p = keep + begin;
  const int64_t len = end - begin;
  const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(p) & 15u);
  const uint4* base = reinterpret_cast<const uint4*>(p - mis);
  const int64_t chunks = (mis + len + 15) >> 4;
  uint32_t c = 0;
  for (int64_t i = tid; i < chunks; i += kReplayThreads) {
    const uint4 v = base[i];
    const int64_t at = i * 16 - mis;  // the piece's first byte, counted from `begin`
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) c += nonzero_bytes(w[k] & byte_range_mask(-(at + 4 * k), len - (at + 4 * k)));
  }
  return c;
}

// the workgroup's lanes add their shares into *acc (LDS)
__device__ inline void add_shares(uint32_t* acc, uint32_t mine) {
#pragma unroll
  for (int s = kWave / 2; s > 0; s >>= 1) mine += __shfl_down(mine, s, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && mine) atomicAdd(acc, mine);
}

// rows src_row[0..cnt) of src (src_pitch bytes apart) go to rows dst_first, dst_first + 1, .. of dst (dst_pitch apart),
// starting over at row 0 where dst_wrap is reached.  Unit u of the copy is unit u % upr of row u / upr; lanes take
// consecutive units, kReplayUnroll loads in flight each; (k, w) walk on without a division per unit.  cnt >= 1.
template <typename V>
__device__ inline void copy_rows(char* dst, int64_t dst_pitch, int64_t dst_first, int64_t dst_wrap, const char* src,
                                 int64_t src_pitch, const int32_t* src_row, int cnt, int row_bytes, int tid) {
  const int upr = row_bytes / (int)sizeof(V);
  const int total = cnt * upr;
  const int qs = kReplayThreads / upr, rs = kReplayThreads % upr;
  int k = tid / upr, w = tid % upr;
  for (int u = tid; u < total; u += kReplayThreads * kReplayUnroll) {
    V v[kReplayUnroll];
    int kk[kReplayUnroll], ww[kReplayUnroll];
#pragma unroll
    for (int i = 0; i < kReplayUnroll; ++i) {
      // a lane past the end loads unit 0 again (total > 0) and drops it: no branch between the loads
      const bool in = u + i * kReplayThreads < total;
      kk[i] = in ? k : 0;
      ww[i] = in ? w : 0;
      v[i] = *reinterpret_cast<const V*>(src + (int64_t)src_row[kk[i]] * src_pitch +
                                         (int64_t)ww[i] * (int64_t)sizeof(V));
      k += qs;
      w += rs;
      if (w >= upr) {
        w -= upr;
        ++k;
      }
    }
#pragma unroll
    for (int i = 0; i < kReplayUnroll; ++i) {
      if (u + i * kReplayThreads < total) {
        int64_t r = dst_first + kk[i];
        if (r >= dst_wrap) r -= dst_wrap;
        *reinterpret_cast<V*>(dst + r * dst_pitch + (int64_t)ww[i] * (int64_t)sizeof(V)) = v[i];
      }
    }
  }
}

typedef uint32_t ReplayV16 __attribute__((ext_vector_type(4)));  // a native vector: stays in registers

template <typename... A>
__device__ inline void copy_rows_vec(int vec, A... args) {
  if (vec == 16)
    copy_rows<ReplayV16>(args...);
  else if (vec == 4)
    copy_rows<uint32_t>(args...);
  else
    copy_rows<uint8_t>(args...);
}

__global__ void __launch_bounds__(kReplayThreads) replay_push_kernel(ReplayArgs a) {
  __shared__ int32_t s_src[kReplayTile];           // the tile's kept rows, in batch order
  __shared__ uint32_t s_wave[kReplayTile / kWave]; // kept rows per wave of the tile
  __shared__ uint32_t s_count[2];                  // kept rows in front of the tile; behind it (last ticket only)
  __shared__ unsigned long long s_cur[3];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t tile0 = (int64_t)blockIdx.x * kReplayTile;
  const int64_t left = (int64_t)a.batch - tile0;
  const int rows_here = left < kReplayTile ? (int)left : kReplayTile;
  if (tid == 0) {
    s_cur[0] = cursor_load(a.cursor + HK_REPLAY_POS);
    s_cur[1] = cursor_load(a.cursor + HK_REPLAY_FULL);
    s_cur[2] = cursor_load(a.cursor + HK_REPLAY_TOTAL_PUSHED);
    s_count[0] = 0u;
    s_count[1] = 0u;
  }
  const bool kept = tid < rows_here && (a.keep ? a.keep[tile0 + tid] != 0 : true);
  const unsigned long long votes = __ballot(kept);
  if (tid < kReplayTile && lane == 0) s_wave[wave] = (uint32_t)__popcll(votes);
  __syncthreads();
  // the cursor words are in LDS, so their loads have returned: now the ticket
  if (tid == 0) s_last = draw_ticket(a.cursor) ? 1 : 0;
  if (a.keep) add_shares(&s_count[0], count_kept(a.keep, 0, tile0, tid));
  if (kept) {
    int at = __popcll(votes & ((1ull << lane) - 1ull));
    for (int v = 0; v < wave; ++v) at += (int)s_wave[v];
    s_src[at] = (int32_t)(tile0 + tid);
  }
  __syncthreads();
  int cnt = 0;
#pragma unroll
  for (int v = 0; v < kReplayTile / kWave; ++v) cnt += (int)s_wave[v];
  const int64_t cap = a.capacity;
  const int64_t before = a.keep ? (int64_t)s_count[0] : tile0;
  int64_t pos = (int64_t)s_cur[0];
  if (pos < 0 || pos >= cap) pos = 0;  // a cursor nobody should have written: stay inside the ring
  int64_t first = pos + before;        // before < batch < cap
  if (first >= cap) first -= cap;
  if (cnt > 0) {
    for (int c = 0; c < a.ncols; ++c) {
      const ReplayCol col = a.col[c];
      copy_rows_vec(col.vec, col.ring, (int64_t)col.row_bytes, first, cap, (const char*)col.rows, col.stride,
                    (const int32_t*)s_src, cnt, (int)col.row_bytes, tid);
    }
  }
  if (s_last) {  // the same for the whole workgroup; every workgroup has read the cursor
    const int64_t tile1 = tile0 + rows_here;
    if (a.keep) add_shares(&s_count[1], count_kept(a.keep, tile1, (int64_t)a.batch, tid));
    __syncthreads();
    if (tid == 0) {
      const int64_t n = before + cnt + (a.keep ? (int64_t)s_count[1] : (int64_t)a.batch - tile1);
      const int64_t end = pos + n;  // n <= batch < cap
      cursor_store(a.cursor + HK_REPLAY_POS, (unsigned long long)(end >= cap ? end - cap : end));
      cursor_store(a.cursor + HK_REPLAY_FULL, (s_cur[1] != 0ull || end >= cap) ? 1ull : 0ull);
      cursor_store(a.cursor + HK_REPLAY_LAST_COUNT, (unsigned long long)n);
      cursor_store(a.cursor + HK_REPLAY_TOTAL_PUSHED, s_cur[2] + (unsigned long long)n);
      cursor_store(a.cursor + HK_REPLAY_TICKET, 0ull);
    }
  }
}

__global__ void __launch_bounds__(kReplayThreads) replay_sample_kernel(ReplayArgs a) {
  __shared__ int32_t s_idx[kReplayTile];
  __shared__ unsigned long long s_cur[3];
  __shared__ int s_last;
  const int tid = threadIdx.x;
  const int64_t tile0 = (int64_t)blockIdx.x * kReplayTile;
  const int64_t left = (int64_t)a.batch_size - tile0;
  const int rows_here = left < kReplayTile ? (int)left : kReplayTile;
  if (tid == 0) {
    s_cur[0] = cursor_load(a.cursor + HK_REPLAY_POS);
    s_cur[1] = cursor_load(a.cursor + HK_REPLAY_FULL);
    s_cur[2] = cursor_load(a.cursor + HK_REPLAY_SAMPLES_DRAWN);
  }
  __syncthreads();
  if (tid == 0) s_last = draw_ticket(a.cursor) ? 1 : 0;
  const int64_t cap = a.capacity;
  int64_t pos = (int64_t)s_cur[0];
  if (pos < 0 || pos >= cap) pos = 0;
  const uint32_t size = (uint32_t)(s_cur[1] != 0ull ? cap : pos);
  const unsigned long long drawn = s_cur[2];
  if (tid < rows_here) {
    const int64_t j = tile0 + tid;
    int32_t idx = -1;
    if (size > 0u) {
      const U4 r = philox4x32((uint32_t)(j >> 2), (uint32_t)drawn, (uint32_t)(drawn >> 32), kStreamReplay, a.seed);
      idx = (int32_t)mulhi32(u4_word(r, (uint32_t)j & 3u), size);
    }
    s_idx[tid] = idx;
    if (a.index_out) a.index_out[j] = (int64_t)idx;
  }
  __syncthreads();
  if (size > 0u) {
    for (int c = 0; c < a.ncols; ++c) {
      const ReplayCol col = a.col[c];
      copy_rows_vec(col.vec, col.rows, col.stride, tile0, (int64_t)INT64_MAX, (const char*)col.ring,
                    (int64_t)col.row_bytes, (const int32_t*)s_idx, rows_here, (int)col.row_bytes, tid);
    }
  }
  if (s_last && tid == 0) {
    cursor_store(a.cursor + HK_REPLAY_SAMPLES_DRAWN, drawn + 1ull);
    cursor_store(a.cursor + HK_REPLAY_TICKET, 0ull);
  }
}

}  // namespace hk
