// hk::customgrad_group_kernel / customgrad_forward_kernel / customgrad_rows_kernel / customgrad_params_kernel -- the
// training-mode forward of CustomNet and its backward, one tower per row both ways (include/hironaka_hip_customgrad.h states
// the rule, the grouped order and the workspace).  The row tile, the panels and every per-block body are hk_pvgrad_kernel.h's
// (pvgrad_forward_block, pvgrad_backward_block, pvgrad_param_tile); the tile records, the permutation and the tower table in
// device memory are hk_customnet_kernel.h's idea.  What is this file's own:
//
// ---- a stable grouping, in one workgroup ----
// At most 4 096 rows: 1 024 threads make up to four passes, thread t of pass p holds row 1024 p + t, so (pass, wave) in
// ascending order IS ascending b.  A wave ranks its lanes that share a c by ballot (the rank among the lower lanes) and
// its leader lane of that c writes the count into cnt[pass 16 + wave][c] in LDS -- no atomic, every cell has one writer.
// Thread c then scans its column over the 64 (pass, wave) cells in order, thread 0 turns the totals into first slots and
// first tiles, and every row's slot is first[c] + the cell's start + the rank: the rows sorted by (c, b), the same on every
// launch.  No ticket, no counter in memory, nothing to zero between calls.  LDS: 64 x 65 + 3 x 65 ints = 17 420 bytes.
//
// ---- the row kernels ----
// hk::customnet_kernel's frame (tile record, rows through the permutation) around hk_pvgrad_kernel.h's bodies: a tile's
// rows are the slots first .. first + rows - 1, which play the part of the rows row0 .. below `batch` there; the saved
// arrays are addressed by slot, so every store and load of the bodies is the dense one they have in hk_pvgrad_*.
//
// ---- the parameter gradients ----
// One wave per (tower, Dense, 16 x 16 tile) on a grid that gives every tower the same number of tiles (its first block
// counted at the full input width); the heads' tiles lie behind the towers'.  A wave finds its tower by a division, its
// Dense by a walk over the blocks' widths (kernel arguments), reads the group's first slot and size from the workspace and
// runs pvgrad_param_tile over that run of slots.  A tile its tower does not have (a narrower first input, no projection)
// returns.
#pragma once
#define HK_PVGRAD_BODIES_ONLY  // the bodies of hk_pvgrad_kernel.h; its three kernels are hk_pvgrad.hip's
#include "hk_pvgrad_kernel.h"

namespace hk {

// the most row tiles a batch can have (hk_customnet_kernel.h's customnet_max_tiles at the 16-row tile): every group but
// its last tile is full
__host__ __device__ inline int64_t customgrad_max_tiles(int64_t batch, int m) {
  return (batch + kPvgradTile - 1) / kPvgradTile + m + 1;
}

constexpr int kCustomgradGroupThreads = 1024;
constexpr int kCustomgradPasses = HK_PVGRAD_MAX_BATCH / kCustomgradGroupThreads;
constexpr int kCustomgradCells = kCustomgradPasses * (kCustomgradGroupThreads / kWave);
static_assert(kCustomgradPasses * kCustomgradGroupThreads == HK_PVGRAD_MAX_BATCH, "one workgroup holds every row");
static_assert(HK_CUSTOMGRAD_FIRST + HK_CUSTOMNET_MAX_POINTS + 1 <= HK_CUSTOMGRAD_SIZE &&
                  HK_CUSTOMGRAD_SIZE + HK_CUSTOMNET_MAX_POINTS + 1 <= HK_CUSTOMGRAD_HEADER && HK_CUSTOMGRAD_HEADER % 4 == 0,
              "the header's words");

// the sizes every launch and the host compute the workspace's layout from
struct CustomgradShape {
  int32_t batch, m, d, e, nblocks, actions;
  int32_t n[HK_PVNET_MAX_BLOCKS], kind[HK_PVNET_MAX_BLOCKS];
};

__host__ __device__ inline int customgrad_kin(const CustomgradShape& S) { return S.m * S.d + S.e; }
// the saved arrays of block l: hk_pvgrad_kernel.h's, with a projection's wherever a tower can have one
__host__ __device__ inline bool customgrad_proj(const CustomgradShape& S, int l) { return l == 0 || S.n[l - 1] != S.n[l]; }
__host__ __device__ inline int customgrad_slots(const CustomgradShape& S, int l) {
  return S.kind[l] == HK_PVNET_DENSE ? 2 : (customgrad_proj(S, l) ? 13 : 10);
}
// the words in front of the float arrays
__host__ __device__ inline int64_t customgrad_int_words(const CustomgradShape& S) {
  return HK_CUSTOMGRAD_HEADER + 4 * customgrad_max_tiles(S.batch, S.m) + (((int64_t)S.batch + 3) & ~(int64_t)3);
}
__host__ __device__ inline int64_t customgrad_float_words(const CustomgradShape& S) {
  int64_t floats = (int64_t)S.batch * customgrad_kin(S);
  for (int l = 0; l < S.nblocks; ++l) floats += (int64_t)customgrad_slots(S, l) * S.batch * S.n[l];
  return floats + (int64_t)S.batch * (S.n[S.nblocks - 1] + S.e) + (int64_t)S.batch * (S.actions + 1);
}
// the tiles of the parameter launch that every tower gets, and the heads'
__host__ __device__ inline int customgrad_tower_tiles(const CustomgradShape& S) {
  int tiles = 0;
  for (int l = 0; l < S.nblocks; ++l) {
    const int NT = (S.n[l] + 15) >> 4, KT = ((l ? S.n[l - 1] : customgrad_kin(S)) + 15) >> 4;
    tiles += NT * KT;
    if (S.kind[l] != HK_PVNET_DENSE) tiles += NT * NT + (customgrad_proj(S, l) ? NT * KT : 0);
  }
  return tiles;
}
__host__ __device__ inline int customgrad_head_tiles(const CustomgradShape& S) {
  return (((S.actions + 15) >> 4) + 1) * ((S.n[S.nblocks - 1] + S.e + 15) >> 4);
}

struct CustomgradGroupArgs {
  const float* x;
  int32_t* ws;
  int64_t x_stride;
  int32_t batch, m, d;
};
struct CustomgradRowsArgs {
  hk_customnet_desc q;
  CustomgradShape S;
  const float* grad_policy;
  const float* grad_value;
  int64_t grad_policy_stride, grad_value_stride;
};
struct CustomgradParamsArgs {
  CustomgradShape S;
  const hk_pvnet_block* towers;
  const hk_customgrad_block* table;
  const int32_t* ws;
  float* grads;
  hk_customgrad_dense policy, value;
  int32_t tower_tiles;
};
static_assert(sizeof(CustomgradRowsArgs) <= 4096 - 64 && sizeof(CustomgradParamsArgs) <= 4096 - 64,
              "every launch's share travels as the kernel's argument");

__global__ __launch_bounds__(kCustomgradGroupThreads) void customgrad_group_kernel(const CustomgradGroupArgs args) {
  __shared__ int cnt[kCustomgradCells][HK_CUSTOMNET_MAX_POINTS + 1];
  __shared__ int first[HK_CUSTOMNET_MAX_POINTS + 1], size[HK_CUSTOMNET_MAX_POINTS + 1], tile0[HK_CUSTOMNET_MAX_POINTS + 1];
  constexpr int TR = kPvgradTile;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int m = args.m, d = args.d, batch = args.batch;
  int32_t* const ws = args.ws;
  int32_t* const tiles = ws + HK_CUSTOMGRAD_HEADER;
  int32_t* const perm = tiles + 4 * customgrad_max_tiles(batch, m);
  for (int i = tid; i < kCustomgradCells * (HK_CUSTOMNET_MAX_POINTS + 1); i += kCustomgradGroupThreads) (&cnt[0][0])[i] = 0;
  __syncthreads();

  int c[kCustomgradPasses], rank[kCustomgradPasses];
#pragma unroll
  for (int p = 0; p < kCustomgradPasses; ++p) {
    c[p] = 0, rank[p] = 0;
    if (p * kCustomgradGroupThreads >= batch) continue;  // (uniform over the workgroup)
    const int b = p * kCustomgradGroupThreads + tid;
    const bool valid = b < batch;
    if (valid) {
      const float* row = args.x + (int64_t)b * args.x_stride;
      int n = 0;
      for (int i0 = 0; i0 < m; i0 += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = i0 + j < m ? row[(i0 + j) * d] : -1.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) n += v[j] >= 0.0f ? 1 : 0;  // (a NaN compares false)
      }
      c[p] = n;
    }
    unsigned long long todo = __ballot(valid);
    while (todo) {  // (uniform over the wave)
      const int leader = __ffsll(todo) - 1;
      const int cc = __shfl(c[p], leader);
      const bool in = valid && c[p] == cc;
      const unsigned long long same = __ballot(in);
      if (in) rank[p] = __popcll(same & ((1ull << lane) - 1ull));
      if (lane == leader) cnt[p * (kCustomgradGroupThreads / kWave) + wave][cc] = __popcll(same);
      todo &= ~same;
    }
  }
  __syncthreads();
  if (tid <= m) {  // the scan of column c over the cells in (pass, wave) order
    int run = 0;
    for (int w = 0; w < kCustomgradCells; ++w) {
      const int v = cnt[w][tid];
      cnt[w][tid] = run;
      run += v;
    }
    size[tid] = run;
  }
  __syncthreads();
  if (tid == 0) {
    int slot = 0, t = 0;
    for (int cc = 0; cc <= m; ++cc) {
      first[cc] = slot, tile0[cc] = t;
      slot += size[cc], t += (size[cc] + TR - 1) / TR;
    }
    ws[0] = t;
  }
  __syncthreads();
  if (tid <= m) ws[HK_CUSTOMGRAD_FIRST + tid] = first[tid], ws[HK_CUSTOMGRAD_SIZE + tid] = size[tid];
  for (int cc = 0; cc <= m; ++cc) {
    const int n = size[cc], nt = (n + TR - 1) / TR;
    for (int t = tid; t < nt; t += kCustomgradGroupThreads) {
      int32_t* rec = tiles + 4 * (tile0[cc] + t);
      rec[0] = cc, rec[1] = first[cc] + t * TR, rec[2] = n - t * TR < TR ? n - t * TR : TR, rec[3] = 0;
    }
  }
#pragma unroll
  for (int p = 0; p < kCustomgradPasses; ++p) {
    const int b = p * kCustomgradGroupThreads + tid;
    if (b < batch) perm[first[c[p]] + cnt[p * (kCustomgradGroupThreads / kWave) + wave][c[p]] + rank[p]] = b;
  }
}

// a tile's record; false: no such tile (the grid is the worst case)
struct CustomgradTileRec {
  int tower, first, rows;
  const int32_t* perm;
};
__device__ __forceinline__ bool customgrad_tile(const void* workspace, int batch, int m, CustomgradTileRec& t) {
  const int32_t* const ws = static_cast<const int32_t*>(workspace);
  if ((int)blockIdx.x >= ws[0]) return false;
  const int32_t* const rec = ws + HK_CUSTOMGRAD_HEADER + 4 * (int64_t)blockIdx.x;
  t.tower = __builtin_amdgcn_readfirstlane(rec[0]), t.first = __builtin_amdgcn_readfirstlane(rec[1]);
  t.rows = __builtin_amdgcn_readfirstlane(rec[2]);
  t.perm = ws + HK_CUSTOMGRAD_HEADER + 4 * customgrad_max_tiles(batch, m) + t.first;
  return true;
}

__global__ __launch_bounds__(kWave * mlp_waves(kPvgradTile)) void customgrad_forward_kernel(const hk_customnet_desc q,
                                                                                            const CustomgradShape S) {
  constexpr int TR = kPvgradTile;
  typedef PvgradTile T;
  CustomgradTileRec tile;
  if (!customgrad_tile(q.workspace, q.batch, q.m, tile)) return;
  const int tower = tile.tower, first = tile.first, rows = tile.rows;
  const int32_t* const perm = tile.perm;

  extern __shared__ __align__(16) float hk_customgrad_lds[];
  float* cur = hk_customgrad_lds;
  float* nxt = cur + TR * kMlpLda;
  float* const wst = nxt + TR * kMlpLda;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int lm = lane & 15, lg = lane >> 4;
  auto f = [](const void* p) { return static_cast<const float*>(p); };
  const float* const x = f(q.x);
  const int m = q.m, d = q.d, e = q.e, N = q.n_last, batch = q.batch;
  const int Kin = customgrad_kin(S), Kh = N + e, Khp = (Kh + 15) & ~15;
  float* const u = static_cast<float*>(q.workspace) + customgrad_int_words(S);
  float* base = u + (int64_t)batch * Kin;

  PvgradAcc acc;
  if (tower < m) {
    // u = the first tower + 1 points ++ the extra: thread k of a row, zeros behind the width and behind the tile's rows
    const int k0 = (tower + 1) * d, K = k0 + e, Kp = (K + 15) & ~15;
    if (tid < Kp) {
      const int p = mlp_pos(tid), col = tid < k0 ? tid : m * d + (tid - k0);
#pragma unroll 4
      for (int r = 0; r < TR; ++r) {
        float v = 0.0f;
        if (r < rows && tid < K) {
          v = x[(int64_t)perm[r] * q.x_stride + col];
          u[(int64_t)(first + r) * Kin + tid] = v;
        }
        cur[r * kMlpLda + p] = v;
      }
    }
    const hk_pvnet_block* const blocks = q.towers + (int64_t)tower * q.nblocks;
    for (int l = 0; l < q.nblocks; ++l) {
      const int64_t sz = (int64_t)batch * S.n[l];
      pvgrad_forward_block(blocks[l], base, sz, cur, nxt, wst, acc, first, first + rows, tid);
      base += customgrad_slots(S, l) * sz;
    }
    __syncthreads();  // every wave's store of h, and of the zeros behind it, has landed
  } else {
    for (int l = 0; l < q.nblocks; ++l) base += (int64_t)customgrad_slots(S, l) * batch * S.n[l];
    if (tid < ((N + 15) & ~15)) {  // all points are there: no tower, h = +0
#pragma unroll 4
      for (int r = 0; r < TR; ++r) cur[r * kMlpLda + mlp_pos(tid)] = 0.0f;
    }
  }
  // z = h ++ extra: the columns N .. N + e - 1 and the zeros up to the next multiple of 16, thread j of a row; saved by slot
  float* const z = base;
  if (tid < N) {
    const int p = mlp_pos(tid);
    for (int r = 0; r < rows; ++r) z[(int64_t)(first + r) * Kh + tid] = cur[r * kMlpLda + p];
  } else if (tid < Khp) {
    const int p = mlp_pos(tid), col = m * d + (tid - N);
#pragma unroll 4
    for (int r = 0; r < TR; ++r) {
      float v = 0.0f;
      if (r < rows && tid < Kh) {
        v = x[(int64_t)perm[r] * q.x_stride + col];
        z[(int64_t)(first + r) * Kh + tid] = v;
      }
      cur[r * kMlpLda + p] = v;
    }
  }

  // the heads, as hk::customnet_kernel's, to the rows' own indices
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
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * lg + r;
        const float v = acc[0][i][r];
        if (row < rows) {
          const int64_t b = perm[row];
          if (j < A) policy[b * q.policy_stride + j] = v;
          if (j == A) value[b * q.value_stride] = raw ? v : tanhf(v);
        }
      }
    }
  }
}

__global__ __launch_bounds__(kWave * mlp_waves(kPvgradTile)) void customgrad_rows_kernel(const CustomgradRowsArgs args) {
  constexpr int TR = kPvgradTile;
  typedef PvgradTile T;
  const hk_customnet_desc& q = args.q;
  const CustomgradShape& S = args.S;
  CustomgradTileRec tile;
  if (!customgrad_tile(q.workspace, q.batch, q.m, tile)) return;
  const int tower = tile.tower, first = tile.first, rows = tile.rows;
  const int32_t* const perm = tile.perm;

  extern __shared__ __align__(16) float hk_customgrad_lds[];
  float* const pa = hk_customgrad_lds;
  float* const pb = pa + TR * kMlpLda;
  float* const wst = pb + TR * kMlpLda;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int lm = lane & 15, lg = lane >> 4;
  const int batch = q.batch, A = q.actions, N = q.n_last, Kh = N + q.e;
  auto f = [](const void* p) { return static_cast<const float*>(p); };

  float* base = static_cast<float*>(q.workspace) + customgrad_int_words(S) + (int64_t)batch * customgrad_kin(S);
  for (int l = 0; l < q.nblocks; ++l) base += (int64_t)customgrad_slots(S, l) * batch * S.n[l];

  // the heads: dzh by slot from the gradients at the rows' own indices, and D = dzh . Wh over the n_last columns of h
  PvgradAcc D;
  {
    float* const dzh = base + (int64_t)batch * Kh;
    const float* value = f(q.value);
    const bool raw = q.flags & HK_CUSTOMNET_RAW_VALUE;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * lg + r;
      const bool live = row < rows;
      const int64_t bq = perm[live ? row : rows - 1];
#pragma unroll
      for (int i = 0; i < T::TPW; ++i) {
        const int j = (wave + T::W * i) * 16 + lm;
        float v = 0.0f;
        if (j < A) {
          v = args.grad_policy[bq * args.grad_policy_stride + j];
        } else if (j == A) {
          const float t = args.grad_value[bq * args.grad_value_stride];
          if (raw) {
            v = t;
          } else {
            const float tv = value[bq * q.value_stride];
            const float sq = tv * tv;
            v = t * (1.0f - sq);
          }
        }
        D[0][i][r] = v;
        if (live && j <= A) dzh[(int64_t)(first + row) * (A + 1) + j] = v;
      }
    }
    if (tower >= q.m) return;  // no tower: the heads' gradients are all this row gives (uniform over the workgroup)
    const float* Wp = f(q.policy_weight);
    const float* Wv = f(q.value_weight);
    pvgrad_to_panel(D, pa, A + 1, tid);
    pvgrad_dense_t(D, pa, wst, [&](int c) { return c < A ? Wp + (int64_t)c * Kh : Wv; }, A + 1, N, tid);
  }

  const hk_pvnet_block* const blocks = q.towers + (int64_t)tower * q.nblocks;
  for (int l = q.nblocks - 1; l >= 0; --l) {
    const int64_t sz = (int64_t)batch * S.n[l];
    base -= customgrad_slots(S, l) * sz;
    pvgrad_backward_block(blocks[l], l == 0, base, sz, D, pa, pb, wst, first, first + rows, tid);
  }
}

__global__ __launch_bounds__(kPvgradParamThreads) void customgrad_params_kernel(const CustomgradParamsArgs args) {
  const CustomgradShape& S = args.S;
  const int lane = threadIdx.x;
  const int batch = S.batch, Kin = customgrad_kin(S), L = S.nblocks;
  const float* const u = reinterpret_cast<const float*>(args.ws) + customgrad_int_words(S);
  auto G = [&](int64_t off) { return off < 0 ? nullptr : args.grads + off; };
  PvgradParam P = {};
  int local = (int)blockIdx.x - S.m * args.tower_tiles;
  if (local >= 0) {  // the heads: every row, in grouped order
    const float* base = u + (int64_t)batch * Kin;
    for (int l = 0; l < L; ++l) base += (int64_t)customgrad_slots(S, l) * batch * S.n[l];
    const int A = S.actions, Kh = S.n[L - 1] + S.e, KT = (Kh + 15) >> 4;
    const int policy_tiles = ((A + 15) >> 4) * KT;
    const bool value = local >= policy_tiles;
    if (value) local -= policy_tiles;
    const hk_customgrad_dense& H = value ? args.value : args.policy;
    P.a_in = base, P.a_stride = Kh;
    P.dz = base + (int64_t)batch * Kh + (value ? A : 0), P.dz_stride = A + 1;
    P.n = value ? 1 : A, P.k = Kh;
    P.d_weight = G(H.d_weight), P.d_bias = G(H.d_bias);
    const int jt = local / KT;
    pvgrad_param_tile(P, batch, jt, local - jt * KT, lane);
    return;
  }
  const int tower = (int)blockIdx.x / args.tower_tiles;
  local = (int)blockIdx.x - tower * args.tower_tiles;
  const int first = args.ws[HK_CUSTOMGRAD_FIRST + tower], R = args.ws[HK_CUSTOMGRAD_SIZE + tower];
  const float* base = u + (int64_t)batch * Kin;
  const float* a_in = u + (int64_t)first * Kin;
  int a_stride = Kin;
  for (int l = 0; l < L; ++l) {
    const int n = S.n[l], NT = (n + 15) >> 4, KT = (a_stride + 15) >> 4;  // (a_stride: the widest input of block l)
    const bool dense = S.kind[l] == HK_PVNET_DENSE, proj = customgrad_proj(S, l);
    const int64_t sz = (int64_t)batch * n;
    const int t1 = NT * KT, t2 = dense ? 0 : NT * NT, tp = !dense && proj ? NT * KT : 0;
    if (local < t1 + t2 + tp) {
      const hk_pvnet_block& B = args.towers[(int64_t)tower * L + l];
      const hk_customgrad_block& T = args.table[(int64_t)tower * L + l];
      auto at = [&](int slot) { return base + slot * sz + (int64_t)first * n; };
      const int which = local < t1 ? 0 : (local < t1 + t2 ? 1 : 2);
      if (which == 1) local -= t1;
      if (which == 2) local -= t1 + t2;
      const int KTw = which == 1 ? NT : KT;
      const int jt = local / KTw, kt = local - jt * KTw;
      const int k = which == 1 ? n : B.k;
      if (kt * 16 >= k || (which == 2 && B.k == n)) return;  // a tile this tower does not have
      const hk_customgrad_dense& D = which == 0 ? T.dense1 : (which == 1 ? T.dense2 : T.proj);
      P.n = n, P.k = k, P.dz_stride = n;
      if (dense) {
        P.dz = at(kPgDenseDz1), P.a_in = a_in, P.a_stride = a_stride;
      } else if (which == 0) {
        P.dz = at(kPgDz1), P.a_in = a_in, P.a_stride = a_stride, P.ge = at(kPgDa), P.gx = at(kPgGx1);
      } else if (which == 1) {
        P.dz = at(kPgDz2), P.a_in = at(kPgA), P.a_stride = n, P.ge = at(kPgE), P.gx = at(kPgGx2);
      } else {
        P.dz = at(kPgDzp), P.a_in = a_in, P.a_stride = a_stride, P.ge = at(kPgE), P.gx = at(kPgGxp);
      }
      P.d_weight = G(D.d_weight), P.d_bias = G(D.d_bias);
      if (!dense) P.d_gn_scale = G(D.d_gn_scale), P.d_gn_bias = G(D.d_gn_bias);
      pvgrad_param_tile(P, R, jt, kt, lane);
      return;
    }
    local -= t1 + t2 + tp;
    a_in = base + (dense ? kPgDenseH : kPgH) * sz + (int64_t)first * n;
    a_stride = n;
    base += customgrad_slots(S, l) * sz;
  }
}

}  // namespace hk
