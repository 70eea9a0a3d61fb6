// hk::pvgrad_forward_kernel / hk::pvgrad_rows_kernel / hk::pvgrad_params_kernel -- the training-mode forward of a
// DenseResNet / DenseNet policy-value network and its backward (include/hironaka_hip_pvgrad.h states the rule and the
// workspace).  The tile, the panels, the weight stage and every forward Dense are hk::pvnet_kernel's (hk_pvnet_kernel.h,
// hk_mlp_kernel.h: MlpTile<16>, mlp_dense, pvnet_group_norm, pvnet_store); 4 waves carry 16 rows.
//
// ---- forward ----
// hk::pvnet_kernel's loop with stores: a Dense's result leaves for the workspace from the registers of the MFMA's result
// (column j on lane & 15: 16 adjacent floats per row), what pvnet_store wrote into a panel is read back by the thread that
// wrote it.  Nothing else differs, so policy and value have hk_pvnet_forward's bits.
//
// ---- backward, the row chain ----
// The gradient D at a block's output stays in the 16 registers of C/D from one block to the next: the ReLU's mask, the
// group norm's backward and the residual's add are all elementwise in that layout, and the group sums are the forward's
// DPP exchanges (pvnet_group_sum).  Only a product dz . W needs LDS: dz goes into a panel in mlp_pos order (the A operand,
// as the activations of the forward), W through the stage TRANSPOSED -- the contraction runs over W's rows, so thread j
// loads W[c .. c+15][j] (a wave reads 256 adjacent bytes of each row) and writes row j of the stage as four
// ds_write_b128; the ds_read_b128 and the MFMA chain are mlp_dense's.  Two panels alternate between consecutive products.
// LDS: 2 x 16 x 260 + 256 x 20 floats = 53 760 bytes, as the forward.  Banks: the reads are hk_mlp_kernel.h's; the
// stage's ds_write_b128 of 16 lanes go to rows 20 floats apart, 4 (5 j + g) mod 64: the sixteen j of a group of lanes
// cover the 16 quads of banks once.
//
// ---- backward, the parameter gradients ----
// One wave per (Dense, 16 output columns, 16 input columns) tile: dW = dz^T a_in as ONE chain over the batch rows in
// ascending order, 4 MFMAs per 16 rows.  Both operands come straight from memory in the MFMA's own layout: A[i][k] =
// dz[16 T + k][j0 + i] and B[k][j] = a_in[16 T + k][k0 + j] are 16 adjacent floats per row and lane group, so the
// transposition of dz is the choice of which lane loads what and needs no LDS.  The waves of the first input tile add
// ROWSUM's sixteen partial sums from the same registers (part 4 t + lane group in register t) and finish the tree with
// two register adds and two lane exchanges.  No atomics, no workgroup waits for another.
#pragma once
#include "hk_pvnet_kernel.h"

namespace hk {

constexpr int kPvgradTile = HK_MLP_TILE_SMALL;
typedef MlpTile<kPvgradTile> PvgradTile;
typedef PvgradTile::Acc PvgradAcc;
static_assert(PvgradTile::MT == 1 && PvgradTile::W == 4 && PvgradTile::TPW == 4, "16 rows, 4 waves of 4 column tiles");
static_assert(HK_PVGRAD_MAX_BATCH == HK_MLP_TILE_CROSSOVER, "the 16-row tile's range");

// the workspace's [batch, n] arrays of a block, in order (the header's list)
enum { kPgZ1, kPgA, kPgZ2, kPgH, kPgE, kPgDa, kPgDz1, kPgDz2, kPgGx1, kPgGx2, kPgZp, kPgDzp, kPgGxp };
enum { kPgDenseH, kPgDenseDz1 };
__host__ __device__ inline int pvgrad_slots(const hk_pvnet_block& B) {
  return B.kind == HK_PVNET_DENSE ? 2 : (B.k == B.n ? 10 : 13);
}

struct PvgradForwardArgs {
  hk_pvnet_desc q;
  float* ws;
};
struct PvgradRowsArgs {
  hk_pvnet_desc q;
  float* ws;
  const float* grad_policy;
  const float* grad_value;
  int64_t grad_policy_stride, grad_value_stride;
};
// one Dense of the parameter gradients: dz [batch, n] dz_stride apart, its input a_in [batch, k] a_stride apart, the
// group norm's e and e * xhat ([batch, n] dense; NULL: no norm), the gradients (NULL: not written), its first tile
struct PvgradParam {
  const float *dz, *a_in, *ge, *gx;
  float *d_weight, *d_bias, *d_gn_scale, *d_gn_bias;
  int64_t a_stride;
  int32_t dz_stride, n, k, tile0;
};
struct PvgradParamsArgs {
  PvgradParam t[HK_PVGRAD_TABLE];
  int32_t count, batch;
};
static_assert(sizeof(PvgradForwardArgs) <= 4096 - 64 && sizeof(PvgradRowsArgs) <= 4096 - 64 &&
                  sizeof(PvgradParamsArgs) <= 4096 - 64, "every launch's share travels as the kernel's argument");

// out[b, j] = acc (row 4 lg + r, column j) for the rows of the batch and the columns below N
__device__ __forceinline__ void pvgrad_save(const PvgradAcc& acc, float* out, int N, int64_t row0, int batch, int tid) {
  const int lane = tid & (kWave - 1), wave = tid >> 6, lm = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int i = 0; i < PvgradTile::TPW; ++i) {
    const int j = (wave + PvgradTile::W * i) * 16 + lm;
    if (j < N)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t b = row0 + 4 * lg + r;
        if (b < batch) out[b * N + j] = acc[0][i][r];
      }
  }
}
// the same of a panel's elements: each thread reads back what it wrote itself (pvnet_store)
__device__ __forceinline__ void pvgrad_save_panel(const float* panel, float* out, int N, int64_t row0, int batch, int tid) {
  const int lane = tid & (kWave - 1), wave = tid >> 6, lm = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int i = 0; i < PvgradTile::TPW; ++i) {
    const int j = (wave + PvgradTile::W * i) * 16 + lm;
    if (j < N)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t b = row0 + 4 * lg + r;
        if (b < batch) out[b * N + j] = panel[(4 * lg + r) * kMlpLda + mlp_pos(j)];
      }
  }
}

// one block of the training forward on a row tile: the rows row0 .. below `batch` (where the tile ends), the block's saved
// [., N] arrays `sz` floats apart from `base`.  The block's input is in `cur` and so is its result (a dense block swaps the
// panels).  The one copy of the body: pvgrad_forward_kernel's and hk::customgrad_forward_kernel's (hk_customgrad_kernel.h)
__device__ __forceinline__ void pvgrad_forward_block(const hk_pvnet_block& B, float* base, int64_t sz, float*& cur, float*& nxt,
                                                     float* const wst, PvgradAcc& acc, int64_t row0, int batch, int tid) {
  constexpr int TR = kPvgradTile;
  typedef PvgradTile T;
  auto f = [](const void* p) { return static_cast<const float*>(p); };
  const int K = B.k, N = B.n;
  if (B.kind == HK_PVNET_DENSE) {
    mlp_dense<TR, false>(acc, cur, wst, f(B.dense1.weight), f(B.dense1.bias), nullptr, nullptr, K, N, tid);
    pvnet_store<TR, false>(acc, nxt, N, tid, acc, false);
    pvgrad_save_panel(nxt, base + kPgDenseH * sz, N, row0, batch, tid);
    float* const swap = cur;
    cur = nxt;
    nxt = swap;
    return;
  }
  const bool proj = K != N;
  PvgradAcc o;
  if (proj) {
    mlp_dense<TR, false>(o, cur, wst, f(B.proj.weight), f(B.proj.bias), nullptr, nullptr, K, N, tid);
    pvgrad_save(o, base + kPgZp * sz, N, row0, batch, tid);
    pvnet_group_norm<TR>(o, B.proj, B.eps, N, tid);
  } else {
#pragma unroll
    for (int i = 0; i < T::TPW; ++i) o[0][i] = mlp_f4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  mlp_dense<TR, false>(acc, cur, wst, f(B.dense1.weight), f(B.dense1.bias), nullptr, nullptr, K, N, tid);
  pvgrad_save(acc, base + kPgZ1 * sz, N, row0, batch, tid);
  pvnet_group_norm<TR>(acc, B.dense1, B.eps, N, tid);
  pvnet_store<TR, false>(acc, nxt, N, tid, acc, false);
  pvgrad_save_panel(nxt, base + kPgA * sz, N, row0, batch, tid);
  mlp_dense<TR, false>(acc, nxt, wst, f(B.dense2.weight), f(B.dense2.bias), nullptr, nullptr, N, N, tid);
  pvgrad_save(acc, base + kPgZ2 * sz, N, row0, batch, tid);
  pvnet_group_norm<TR>(acc, B.dense2, B.eps, N, tid);
  pvnet_store<TR, true>(acc, cur, N, tid, o, proj);
  pvgrad_save_panel(cur, base + kPgH * sz, N, row0, batch, tid);
}

// (HK_PVGRAD_BODIES_ONLY: a second translation unit that builds its own kernels from the bodies -- hk_customgrad.hip -- leaves
// the three kernels to hk_pvgrad.hip)
#ifndef HK_PVGRAD_BODIES_ONLY
__global__ __launch_bounds__(kWave * mlp_waves(kPvgradTile)) void pvgrad_forward_kernel(const PvgradForwardArgs args) {
  constexpr int TR = kPvgradTile;
  typedef PvgradTile T;
  const hk_pvnet_desc& q = args.q;
  extern __shared__ __align__(16) float hk_pvgrad_lds[];
  float* cur = hk_pvgrad_lds;
  float* nxt = cur + TR * kMlpLda;
  float* const wst = nxt + TR * kMlpLda;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int lm = lane & 15, lg = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * TR;
  const int batch = q.batch;

  auto f = [](const void* p) { return static_cast<const float*>(p); };
  mlp_load_rows<TR, false>(cur, MlpInput{f(q.x), nullptr, q.x_stride, 0, q.k0}, row0, batch, tid);

  PvgradAcc acc;
  float* base = args.ws;
  for (int l = 0; l < q.nblocks; ++l) {
    const hk_pvnet_block& B = q.block[l];
    const int64_t sz = (int64_t)batch * B.n;
    pvgrad_forward_block(B, base, sz, cur, nxt, wst, acc, row0, batch, tid);
    base += pvgrad_slots(B) * sz;
  }

  // the heads, as hk::pvnet_kernel's
  const int K = q.block[q.nblocks - 1].n, A = q.actions, NT = (A + 16) >> 4;
  mlp_dense<TR, true>(acc, cur, wst, f(q.policy_weight), f(q.policy_bias), f(q.value_weight), f(q.value_bias), K, A + 1, tid);
  float* policy = static_cast<float*>(q.policy);
  float* value = static_cast<float*>(q.value);
  const bool raw = q.flags & HK_PVNET_RAW_VALUE;
#pragma unroll
  for (int i = 0; i < T::TPW; ++i) {
    const int nt = wave + T::W * i;
    if (nt < NT) {
      const int j = nt * 16 + lm;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t b = row0 + 4 * lg + r;
        const float v = acc[0][i][r];
        if (b < batch) {
          if (j < A) policy[b * q.policy_stride + j] = v;
          if (j == A) value[b * q.value_stride] = raw ? v : tanhf(v);
        }
      }
    }
  }
}

#endif

// ---- the row chain ----------------------------------------------------------------------------------------------------

// panel[row][pos(j)] = acc for the columns below N, +0 behind them up to the next multiple of 16 (the product's padding)
__device__ __forceinline__ void pvgrad_to_panel(const PvgradAcc& acc, float* panel, int N, int tid) {
  const int lane = tid & (kWave - 1), wave = tid >> 6, lm = lane & 15, lg = lane >> 4;
  const int NT = (N + 15) >> 4;
#pragma unroll
  for (int i = 0; i < PvgradTile::TPW; ++i) {
    const int nt = wave + PvgradTile::W * i;
    if (nt < NT) {
      const int j = nt * 16 + lm, pj = mlp_pos(j);
#pragma unroll
      for (int r = 0; r < 4; ++r) panel[(4 * lg + r) * kMlpLda + pj] = j < N ? acc[0][i][r] : 0.0f;
    }
  }
}

// acc (row, column j < J) = CHAIN(+0; src[row][c] * rowp(c)[j], c < C): the product with the TRANSPOSE of the weight whose
// row c (J floats) rowp(c) points at.  The barriers are mlp_dense's: the first of a pass says the stage is free (and, at
// c == 0, that `src` is complete); nothing waits behind the last pass.
template <class RowPtr>
__device__ __forceinline__ void pvgrad_dense_t(PvgradAcc& acc, const float* src, float* wst, RowPtr rowp, int C, int J, int tid) {
  const int lane = tid & (kWave - 1), wave = tid >> 6, lm = lane & 15, lg = lane >> 4;
  const int Cp = (C + 15) & ~15, JT = (J + 15) >> 4;
#pragma unroll
  for (int i = 0; i < PvgradTile::TPW; ++i) acc[0][i] = mlp_f4{0.0f, 0.0f, 0.0f, 0.0f};
  float w[kMlpKc];
  // every address is clamped into the weight and the value masked afterwards (hk_mlp_train_kernel.h: no load waits in a
  // branch of its own)
  const int jq = tid < J ? tid : 0;
  auto load = [&](int cc) {
#pragma unroll
    for (int ii = 0; ii < kMlpKc; ++ii) {
      const bool in = cc + ii < C && tid < J;
      const float v = rowp(in ? cc + ii : 0)[jq];
      w[ii] = in ? v : 0.0f;
    }
  };
  load(0);
  for (int cc = 0; cc < Cp; cc += kMlpKc) {
    __syncthreads();
    if (tid < JT * 16) {
#pragma unroll
      for (int g = 0; g < 4; ++g)  // position 4 g + t holds c = cc + 4 t + g (mlp_pos)
        *reinterpret_cast<mlp_f4*>(wst + tid * kMlpLdw + 4 * g) = mlp_f4{w[g], w[4 + g], w[8 + g], w[12 + g]};
    }
    __syncthreads();
    if (cc + kMlpKc < Cp) load(cc + kMlpKc);
    const mlp_f4 a = *reinterpret_cast<const mlp_f4*>(src + lm * kMlpLda + cc + 4 * lg);
#pragma unroll
    for (int i = 0; i < PvgradTile::TPW; ++i) {
      const int nt = wave + PvgradTile::W * i;
      if (nt < JT) {
        const mlp_f4 b = *reinterpret_cast<const mlp_f4*>(wst + (nt * 16 + lm) * kMlpLdw + 4 * lg);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[0][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[t], acc[0][i], 0, 0, 0);
      }
    }
  }
}

// d = act[b, j] > 0 ? d : +0 over the columns below N (act: a saved [batch, N] array), stored to `out` where given
__device__ __forceinline__ void pvgrad_mask(PvgradAcc& d, const float* act, float* out, int N, int64_t row0, int batch, int tid) {
  const int lane = tid & (kWave - 1), wave = tid >> 6, lm = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int i = 0; i < PvgradTile::TPW; ++i) {
    const int j = (wave + PvgradTile::W * i) * 16 + lm;
    const int jq = j < N ? j : 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t b = row0 + 4 * lg + r;
      const bool live = b < batch && j < N;
      const float h = act[(b < batch ? b : batch - 1) * N + jq];
      const float v = live && h > 0.0f ? d[0][i][r] : 0.0f;
      d[0][i][r] = v;
      if (out && live) out[b * N + j] = v;
    }
  }
}

// dz = GNB(e; z, D) over the N columns of a normed width (the header's rule); e * xhat goes to gx, dz to dzo
__device__ __forceinline__ void pvgrad_gnb(PvgradAcc& dz, const PvgradAcc& e, const float* z, const hk_pvnet_dense& D, float eps,
                                           float* gx, float* dzo, int N, int64_t row0, int batch, int tid) {
  const int lane = tid & (kWave - 1), wave = tid >> 6, lm = lane & 15, lg = lane >> 4;
  const int g = N >> 5;
  const float rg = 1.0f / (float)g;
  const float* scale = static_cast<const float*>(D.gn_scale);
#pragma unroll
  for (int i = 0; i < PvgradTile::TPW; ++i) {
    const int nt = wave + PvgradTile::W * i;
    if (nt * 16 < N) {  // (uniform in the wave: every lane takes part in the exchanges)
      const int j = nt * 16 + lm;
      const float gamma = scale ? scale[j] : 1.0f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t b = row0 + 4 * lg + r;
        const bool live = b < batch;
        const float zv = z[(live ? b : batch - 1) * N + j];
        const float d = zv - pvnet_group_sum(zv, g) * rg;
        const float inv = 1.0f / sqrtf(pvnet_group_sum(d * d, g) * rg + eps);
        const float xhat = d * inv;
        const float ev = e[0][i][r];
        const float u = scale ? ev * gamma : ev;
        const float m1 = pvnet_group_sum(u, g) * rg;
        const float m2 = pvnet_group_sum(u * xhat, g) * rg;
        const float v = inv * ((u - m1) - xhat * m2);
        dz[0][i][r] = v;
        if (live) {
          gx[b * N + j] = ev * xhat;
          dzo[b * N + j] = v;
        }
      }
    } else {
      dz[0][i] = mlp_f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
  }
}

// one block of the row chain, backward: D is the gradient at the block's output when it is called and at its input when it
// returns -- but for the net's `first` block, whose input gets none.  The rows, `base` and `sz` as pvgrad_forward_block's;
// pa and pb are the two panels.  The one copy of the body: pvgrad_rows_kernel's and hk::customgrad_rows_kernel's
__device__ __forceinline__ void pvgrad_backward_block(const hk_pvnet_block& B, bool first, float* base, int64_t sz, PvgradAcc& D,
                                                      float* const pa, float* const pb, float* const wst, int64_t row0, int batch,
                                                      int tid) {
  typedef PvgradTile T;
  auto f = [](const void* p) { return static_cast<const float*>(p); };
  const int K = B.k, N = B.n;
  const float* W1 = f(B.dense1.weight);
  if (B.kind == HK_PVNET_DENSE) {
    pvgrad_mask(D, base + kPgDenseH * sz, base + kPgDenseDz1 * sz, N, row0, batch, tid);
    if (first) return;
    __syncthreads();
    pvgrad_to_panel(D, pa, N, tid);
    pvgrad_dense_t(D, pa, wst, [&](int c) { return W1 + (int64_t)c * K; }, N, K, tid);
    return;
  }
  const bool proj = K != N;
  const float* W2 = f(B.dense2.weight);
  PvgradAcc t;
  pvgrad_mask(D, base + kPgH * sz, base + kPgE * sz, N, row0, batch, tid);  // D is e from here
  pvgrad_gnb(t, D, base + kPgZ2 * sz, B.dense2, B.eps, base + kPgGx2 * sz, base + kPgDz2 * sz, N, row0, batch, tid);
  __syncthreads();
  pvgrad_to_panel(t, pa, N, tid);
  pvgrad_dense_t(t, pa, wst, [&](int c) { return W2 + (int64_t)c * N; }, N, N, tid);
  pvgrad_mask(t, base + kPgA * sz, base + kPgDa * sz, N, row0, batch, tid);
  pvgrad_gnb(t, t, base + kPgZ1 * sz, B.dense1, B.eps, base + kPgGx1 * sz, base + kPgDz1 * sz, N, row0, batch, tid);
  if (first) {
    if (proj) pvgrad_gnb(t, D, base + kPgZp * sz, B.proj, B.eps, base + kPgGxp * sz, base + kPgDzp * sz, N, row0, batch, tid);
    return;
  }
  PvgradAcc d1;
  __syncthreads();
  pvgrad_to_panel(t, pb, N, tid);
  pvgrad_dense_t(d1, pb, wst, [&](int c) { return W1 + (int64_t)c * K; }, N, K, tid);
  if (proj) {
    const float* Wq = f(B.proj.weight);
    pvgrad_gnb(t, D, base + kPgZp * sz, B.proj, B.eps, base + kPgGxp * sz, base + kPgDzp * sz, N, row0, batch, tid);
    __syncthreads();
    pvgrad_to_panel(t, pa, N, tid);
    pvgrad_dense_t(D, pa, wst, [&](int c) { return Wq + (int64_t)c * K; }, N, K, tid);
  }
#pragma unroll
  for (int i = 0; i < T::TPW; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) D[0][i][r] = d1[0][i][r] + D[0][i][r];  // d1 + e, or d1 + the projection's product
}

#ifndef HK_PVGRAD_BODIES_ONLY
__global__ __launch_bounds__(kWave * mlp_waves(kPvgradTile)) void pvgrad_rows_kernel(const PvgradRowsArgs args) {
  constexpr int TR = kPvgradTile;
  typedef PvgradTile T;
  const hk_pvnet_desc& q = args.q;
  extern __shared__ __align__(16) float hk_pvgrad_lds[];
  float* const pa = hk_pvgrad_lds;
  float* const pb = pa + TR * kMlpLda;
  float* const wst = pb + TR * kMlpLda;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int lm = lane & 15, lg = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * TR;
  const int batch = q.batch, A = q.actions;
  auto f = [](const void* p) { return static_cast<const float*>(p); };

  float* base = args.ws;
  for (int l = 0; l < q.nblocks; ++l) base += (int64_t)pvgrad_slots(q.block[l]) * batch * q.block[l].n;

  // the heads: dzh, and D = dzh . Wh
  PvgradAcc D;
  {
    float* const dzh = base;
    const float* value = f(q.value);
    const bool raw = q.flags & HK_PVNET_RAW_VALUE;
#pragma unroll
    for (int i = 0; i < T::TPW; ++i) {
      const int j = (wave + T::W * i) * 16 + lm;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t b = row0 + 4 * lg + r;
        const bool live = b < batch;
        const int64_t bq = live ? b : batch - 1;
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
        if (live && j <= A) dzh[b * (A + 1) + j] = v;
      }
    }
    const int K = q.block[q.nblocks - 1].n;
    const float* Wp = f(q.policy_weight);
    const float* Wv = f(q.value_weight);
    pvgrad_to_panel(D, pa, A + 1, tid);
    pvgrad_dense_t(D, pa, wst, [&](int c) { return c < A ? Wp + (int64_t)c * K : Wv; }, A + 1, K, tid);
  }

  for (int l = q.nblocks - 1; l >= 0; --l) {
    const hk_pvnet_block& B = q.block[l];
    const int64_t sz = (int64_t)batch * B.n;
    base -= pvgrad_slots(B) * sz;
    pvgrad_backward_block(B, l == 0, base, sz, D, pa, pb, wst, row0, batch, tid);
  }
}

#endif

// ---- the parameter gradients ----------------------------------------------------------------------------------------------
constexpr int kPvgradParamThreads = kWave;

// one wave's 16 x 16 tile (jt, kt) of a Dense's parameter gradients over the B rows its pointers begin at, in ascending
// order; B == 0 writes +0.  The one copy of the chain: pvgrad_params_kernel's and hk::customgrad_params_kernel's, which
// hands it a group's run of slots
__device__ __forceinline__ void pvgrad_param_tile(const PvgradParam& P, int B, int jt, int kt, int lane) {
  const int lm = lane & 15, lg = lane >> 4;
  const int n = P.n, k = P.k;
  const int j = jt * 16 + lm, kcol = kt * 16 + lm;
  const bool jin = j < n, kin = kcol < k, sums = kt == 0, normed = P.ge != nullptr;
  const float* dzp = P.dz + (jin ? j : n - 1);
  const float* ap = P.a_in + (kin ? kcol : k - 1);
  const float* gep = normed ? P.ge + (jin ? j : n - 1) : dzp;
  const float* gxp = normed ? P.gx + (jin ? j : n - 1) : dzp;
  const int64_t dzs = P.dz_stride, as = P.a_stride;

  mlp_f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  float sb[4] = {0.0f, 0.0f, 0.0f, 0.0f}, se[4] = {0.0f, 0.0f, 0.0f, 0.0f}, sx[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  const int tiles = (B + 15) >> 4;
  for (int T = 0; T < tiles; ++T) {
    float a[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int row = 16 * T + 4 * t + lg;
      const bool live = row < B;
      const int64_t rq = live ? row : B - 1;
      const float av = dzp[rq * dzs], bv = ap[rq * as];
      a[t] = live && jin ? av : 0.0f;
      b[t] = live && kin ? bv : 0.0f;
      if (sums) {  // (uniform in the wave)
        sb[t] = live ? sb[t] + av : sb[t];
        if (normed) {
          const float ev = gep[rq * n], xv = gxp[rq * n];
          se[t] = live ? se[t] + ev : se[t];
          sx[t] = live ? sx[t] + xv : sx[t];
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b[t], acc, 0, 0, 0);
  }
  if (kin) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int jj = jt * 16 + 4 * lg + r;
      if (jj < n) P.d_weight[(int64_t)jj * k + kcol] = acc[r];
    }
  }
  if (sums) {
    // ROWSUM's tree: part i = 4 t + lg; i + 8 is register t + 2, i + 4 register t + 1, i + 2 the lane group lg ^ 2
    auto tree = [](const float (&s)[4]) {
      float v = (s[0] + s[2]) + (s[1] + s[3]);
      v = v + __shfl_xor(v, 32);
      return v + __shfl_xor(v, 16);
    };
    const float vb = tree(sb), ve = tree(se), vx = tree(sx);
    if (lg == 0 && jin) {
      if (P.d_bias) P.d_bias[j] = vb;
      if (normed && P.d_gn_bias) P.d_gn_bias[j] = ve;
      if (normed && P.d_gn_scale) P.d_gn_scale[j] = vx;
    }
  }
}

#ifndef HK_PVGRAD_BODIES_ONLY
__global__ __launch_bounds__(kPvgradParamThreads) void pvgrad_params_kernel(const PvgradParamsArgs args) {
  int at = 0;
  for (int i = 1; i < args.count; ++i)
    if (args.t[i].tile0 <= (int)blockIdx.x) at = i;
  const PvgradParam& P = args.t[at];
  const int KT = (P.k + 15) >> 4;
  const int local = (int)blockIdx.x - P.tile0, jt = local / KT;
  pvgrad_param_tile(P, args.batch, jt, local - jt * KT, threadIdx.x);
}

#endif

}  // namespace hk
