// hk::customnet_group_kernel and hk::customnet_kernel -- the gradient-free forward of CustomNet in two launches
// (include/hironaka_hip_customnet.h states the rule).  The reference runs all m towers on every row and keeps one; here
// the first launch groups the rows by their point count c, and the second is hk::pvnet_kernel (hk_pvnet_kernel.h: the tile,
// the LDS image, the Dense, the group norm, the block loop pvnet_trunk) on row tiles that each hold rows of ONE group,
// reached through a permutation: a row costs one tower.
//
// ---- the workspace (int32 words; hk_customnet_workspace_bytes) ----
//   [0]                   the number of row tiles; [1] the ticket of the group launch's workgroups; [2..3] unused
//   [4 .. 68]             the histogram of c over the batch; [69 .. 71] unused
//   [72 ..]               customnet_max_tiles(batch, m) records {tower c, first slot, rows, 0}
//   behind them           perm[batch]: the rows grouped by c, group c at the slots first[c] ..; then count[batch]: c of a row
// The ticket and the histogram are ZERO between calls: the caller zeroes them once, the group launch's last workgroup
// leaves them zero.  Everything else the group launch writes before the forward reads it.
//
// ---- the group launch: a workgroup of 1024 threads per 1024 rows ----
// A thread counts c of its row (m loads, one per point, eight in flight), keeps it in count[], and adds to its
// workgroup's histogram in LDS -- one atomic per wave and value of c, the lanes of a wave that share a c are ranked by a
// ballot; the workgroup adds its histogram to the one in memory and draws a ticket.  The workgroup that draws the LAST
// ticket (every other one has published its counts: fence, then ticket) finishes alone: it takes the histogram and zeroes
// it and the ticket, thread 0 turns it into the groups' first slots and first tiles (at most 65 values), all threads write
// the tile records, and a pass over count[] hands every row its slot: first[c] + its rank among the arrivals at
// cursor[c].  Nobody waits for anybody: no spinning.  A batch of one workgroup (up to 1024 rows) skips the hand-over.  The order inside a group is whichever the atomics give; a row's
// result does not depend on it.
//
// ---- the forward launch: batch / TR + m + 1 workgroups, the worst case ----
// A workgroup at or beyond the stored tile count returns before its first barrier.  A live one loads
// u = x[b, :(c + 1) d] ++ x[b, m d : m d + e] of its rows b = perm[first + r] (zeros behind the tile's rows), runs the
// blocks of tower c from the table in device memory, writes the extra behind h in the same panel (thread j owns column
// j; the barrier before it lets the other waves' zeros of pvnet_store's padding land first), and runs the heads over
// n_last + e inputs, storing to the rows' own indices.  A tile of c == m skips the trunk: h = +0.
#pragma once
#include "hk_pvnet_kernel.h"

namespace hk {

static_assert(HK_CUSTOMNET_FORCE_TILE_SMALL == HK_MLP_FORCE_TILE_SMALL && HK_CUSTOMNET_FORCE_TILE_LARGE == HK_MLP_FORCE_TILE_LARGE &&
                  HK_CUSTOMNET_RAW_VALUE == HK_PVNET_RAW_VALUE, "the flags are hk_pvnet_forward's");

constexpr int kCustomnetGroupThreads = 1024;
constexpr int kCustomnetHeader = 72;  // words in front of the tile records
constexpr int kCustomnetTicket = 1, kCustomnetHist = 4;

// the most row tiles a batch can have: every group but its last tile is full, and the tile is at least the small one
__host__ __device__ inline int64_t customnet_max_tiles(int64_t batch, int m) {
  return (batch + HK_MLP_TILE_SMALL - 1) / HK_MLP_TILE_SMALL + m + 1;
}

// this lane's rank among the lanes of the workgroup that came to counter[c] (every lane of the wave is here; `valid`
// says whether it has a row): one atomic per wave and value of c
__device__ __forceinline__ int customnet_arrive(int* counter, int c, bool valid, int lane) {
  int mine = 0;
  unsigned long long todo = __ballot(valid);
  while (todo) {  // (uniform over the wave)
    const int leader = __ffsll(todo) - 1;
    const int cc = __shfl(c, leader);
    const bool in = valid && c == cc;
    const unsigned long long same = __ballot(in);
    int start = 0;
    if (lane == leader) start = atomicAdd(&counter[cc], __popcll(same));
    start = __shfl(start, leader);
    if (in) mine = start + __popcll(same & ((1ull << lane) - 1ull));
    todo &= ~same;
  }
  return mine;
}

__global__ __launch_bounds__(kCustomnetGroupThreads) void customnet_group_kernel(const hk_customnet_desc q, int tr) {
  if (q.gate && *q.gate != q.want) return;
  __shared__ int hist[HK_CUSTOMNET_MAX_POINTS + 1], cursor[HK_CUSTOMNET_MAX_POINTS + 1];
  __shared__ int first[HK_CUSTOMNET_MAX_POINTS + 1], tile0[HK_CUSTOMNET_MAX_POINTS + 1];
  __shared__ int last;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int m = q.m, d = q.d;
  const int64_t batch = q.batch;
  int32_t* const ws = static_cast<int32_t*>(q.workspace);
  int32_t* const tiles = ws + kCustomnetHeader;
  int32_t* const perm = tiles + 4 * customnet_max_tiles(batch, m);
  int32_t* const count = perm + batch;
  const float* const x = static_cast<const float*>(q.x);
  if (tid <= m) hist[tid] = 0, cursor[tid] = 0;
  __syncthreads();

  {  // this workgroup's rows: c, the histogram
    const int64_t b = (int64_t)blockIdx.x * kCustomnetGroupThreads + tid;
    const bool valid = b < batch;
    int c = 0;
    if (valid) {
      const float* row = x + b * q.x_stride;
      for (int i0 = 0; i0 < m; i0 += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = i0 + j < m ? row[(i0 + j) * d] : -1.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) c += v[j] >= 0.0f ? 1 : 0;  // (a NaN compares false)
      }
      count[b] = c;
    }
    customnet_arrive(hist, c, valid, lane);
  }
  __syncthreads();
  if (gridDim.x > 1) {  // (one workgroup has the whole histogram in its own LDS, and nobody to wait for)
    if (tid <= m && hist[tid]) atomicAdd(&ws[kCustomnetHist + tid], hist[tid]);
    __threadfence();  // this thread's count and share of the histogram are out before the workgroup's ticket is drawn
    __syncthreads();
    if (tid == 0) last = atomicAdd(&ws[kCustomnetTicket], 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!last) return;
    // the last workgroup: every other one has published its counts
    __threadfence();
    if (tid <= m) hist[tid] = atomicExch(&ws[kCustomnetHist + tid], 0);  // taken, and zero for the next call
    if (tid == 0) ws[kCustomnetTicket] = 0;
    __syncthreads();
  }
  if (tid == 0) {
    int slot = 0, t = 0;
    for (int c = 0; c <= m; ++c) {
      first[c] = slot, tile0[c] = t;
      slot += hist[c], t += (hist[c] + tr - 1) / tr;
    }
    ws[0] = t;
  }
  __syncthreads();
  for (int c = 0; c <= m; ++c) {
    const int n = hist[c], nt = (n + tr - 1) / tr;
    for (int t = tid; t < nt; t += kCustomnetGroupThreads) {
      int32_t* rec = tiles + 4 * (tile0[c] + t);
      rec[0] = c, rec[1] = first[c] + t * tr, rec[2] = n - t * tr < tr ? n - t * tr : tr, rec[3] = 0;
    }
  }
  for (int64_t base = 0; base < batch; base += kCustomnetGroupThreads) {
    const int64_t b = base + tid;
    const bool valid = b < batch;
    // (another workgroup's store: read at the device's scope, past this CU's cache)
    const int c = valid ? __hip_atomic_load(&count[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    const int rank = customnet_arrive(cursor, c, valid, lane);
    if (valid) perm[first[c] + rank] = (int32_t)b;
  }
}

template <int TR>
__global__ __launch_bounds__(kWave * mlp_waves(TR)) void customnet_kernel(const hk_customnet_desc q) {
  typedef MlpTile<TR> T;
  if (q.gate && *q.gate != q.want) return;
  const int32_t* const ws = static_cast<const int32_t*>(q.workspace);
  if ((int)blockIdx.x >= ws[0]) return;  // the grid is the worst case
  const int32_t* const rec = ws + kCustomnetHeader + 4 * (int64_t)blockIdx.x;
  const int tower = __builtin_amdgcn_readfirstlane(rec[0]), first = __builtin_amdgcn_readfirstlane(rec[1]);
  const int rows = __builtin_amdgcn_readfirstlane(rec[2]);
  const int32_t* const perm = ws + kCustomnetHeader + 4 * customnet_max_tiles(q.batch, q.m) + first;

  extern __shared__ __align__(16) float hk_customnet_lds[];
  float* cur = hk_customnet_lds;
  float* nxt = cur + TR * kMlpLda;
  float* const wst = nxt + TR * kMlpLda;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int lm = lane & 15, lg = lane >> 4;
  auto f = [](const void* p) { return static_cast<const float*>(p); };
  const float* const x = f(q.x);
  const int m = q.m, d = q.d, e = q.e, N = q.n_last;

  typename T::Acc acc;
  if (tower < m) {
    // u = the first tower + 1 points ++ the extra: thread k of a row, zeros behind the width and behind the tile's rows
    const int k0 = (tower + 1) * d, K = k0 + e, Kp = (K + 15) & ~15;
    if (tid < Kp) {
      const int p = mlp_pos(tid), col = tid < k0 ? tid : m * d + (tid - k0);
#pragma unroll 4
      for (int r = 0; r < TR; ++r) {
        float v = 0.0f;
        if (r < rows && tid < K) v = x[(int64_t)perm[r] * q.x_stride + col];
        cur[r * kMlpLda + p] = v;
      }
    }
    pvnet_trunk<TR>(q.towers + (int64_t)tower * q.nblocks, q.nblocks, cur, nxt, wst, acc, tid);
    __syncthreads();  // every wave's store of h, and of the zeros behind it, has landed
  } else if (tid < ((N + 15) & ~15)) {  // all points are there: no tower, h = +0
#pragma unroll 4
    for (int r = 0; r < TR; ++r) cur[r * kMlpLda + mlp_pos(tid)] = 0.0f;
  }
  // z = h ++ extra: the columns N .. N + e - 1 and the zeros up to the next multiple of 16, thread j of a row
  const int Kh = N + e, Khp = (Kh + 15) & ~15;
  if (tid >= N && tid < Khp) {
    const int p = mlp_pos(tid), col = m * d + (tid - N);
#pragma unroll 4
    for (int r = 0; r < TR; ++r) {
      float v = 0.0f;
      if (r < rows && tid < Kh) v = x[(int64_t)perm[r] * q.x_stride + col];
      cur[r * kMlpLda + p] = v;
    }
  }

  // the heads, as pvnet_tile's, to the rows' own indices
  const int A = q.actions, NT = (A + 16) >> 4;
  mlp_dense<TR, true>(acc, cur, wst, f(q.policy_weight), f(q.policy_bias), f(q.value_weight), f(q.value_bias), Kh, A + 1, tid);
  float* policy = static_cast<float*>(q.policy);
  float* value = static_cast<float*>(q.value);
  const bool raw = q.flags & HK_CUSTOMNET_RAW_VALUE;
#pragma unroll
  for (int i = 0; i < T::TPW; ++i) {
    const int nt = wave + T::W * i;
    if (nt < NT) {
      const int j = nt * 16 + lm;
#pragma unroll
      for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = mt * 16 + 4 * lg + r;
          const float v = acc[mt][i][r];
          if (row < rows) {
            const int64_t b = perm[row];
            if (j < A) policy[b * q.policy_stride + j] = v;
            if (j == A) value[b * q.value_stride] = raw ? v : tanhf(v);
          }
        }
    }
  }
}

}  // namespace hk
