// hk::mlp_train_forward_kernel / hk::mlp_train_backward_kernel -- one layer of a create_mlp stack in training mode, one
// launch per layer each way (include/hironaka_hip_mlp_train.h states the rule).  A workgroup of 4 waves owns 16 columns
// of the layer for ALL batch rows, so a batch norm's statistics never leave it; the layers follow each other by launch
// order on the stream alone.
//
// ---- who computes what ----
// The rows are RT x 4 tiles of 16; wave w owns the row tiles w, w + 4, ...: RT accumulators of 4 registers, each ONE
// chain over the whole k axis in ascending order on v_mfma_f32_16x16x4_f32 (hk_mlp_kernel.h: bit for bit a k-ordered
// fmaf chain).  The forward's k axis is the layer's input; the backward's first product d = dz_{l+1} W_{l+1}[:, cols]
// has the next layer's outputs there, its second dW = dz^T a_in the batch rows: there the A operand is dz transposed
// through LDS, the B operand the rows of a_in straight from memory (16 adjacent floats per row and lane group: each
// wave reads its own column tiles of a_in once, there is nothing for LDS to share), and wave w owns the column tiles
// w, w + 4, ... of the layer's input.
//
// ---- the LDS image ----
//   stage  [RT * 64 rows][kTrainLd = 20]: a 16-k chunk of the A operand, k-transposed as in hk_mlp_kernel.h (mlp_pos)
//   wstage [16 columns][20]: the same chunk of the 16 weight rows (forward) or columns (backward)
//   panel  [16 columns][ldz = roundup(B, 64) + 16]: a column of the tile per row, over the stage (which is dead by
//          then); the rows k-transposed per 16 so that the second product's ds_read_b128 gives four MFMAs' operands
//   stat   [2][16]: per-column scalars from the sixteen threads that reduce a column to the threads that own it
// ---- banks ----
// Stage and wstage are hk_mlp_kernel.h's: a row stride of 20 floats, one 2-way conflict per ds_read_b128 group.  The
// panel's writes of register r go to ldz * lm + pos(row): lm runs over 16 strides of 16 banks mod 64 -- a 4-way
// conflict on a write that happens three times per element at most; its reads in ROWSUM come from thread (column c =
// tid >> 4, part i = tid & 15) at ldz * c + 16 t + pos(i): a wave's 4 columns x 16 parts cover the 64 banks once.
// The second product reads ds_read_b128 at ldz * lm + 16 T + 4 g: 16 banks apart per lm, 4-way; at one read per 16
// MFMAs of a wave that is not where the time goes.
#pragma once
#include "hk_mlp_kernel.h"

namespace hk {

constexpr int kTrainWaves = 4;
constexpr int kTrainThreads = kTrainWaves * kWave;
constexpr int kTrainLd = kMlpKc + 4;
constexpr int kTrainCols = 16;

// rows an instantiation holds: RT row tiles of 16 per wave
constexpr int train_rows(int rt) { return rt * kTrainWaves * 16; }
constexpr int kTrainRtSmall = HK_MLP_TRAIN_ROWS_SMALL / (kTrainWaves * 16);
constexpr int kTrainRtLarge = HK_MLP_TRAIN_MAX_BATCH / (kTrainWaves * 16);
static_assert(train_rows(kTrainRtSmall) == HK_MLP_TRAIN_ROWS_SMALL && train_rows(kTrainRtLarge) == HK_MLP_TRAIN_MAX_BATCH,
              "the header's row counts");

// THE place the instantiation is picked: the small one keeps 16 accumulator registers per wave and 21 KiB of LDS, the
// large one 64 and 82 KiB
inline int train_rt(int64_t batch) { return batch <= HK_MLP_TRAIN_ROWS_SMALL ? kTrainRtSmall : kTrainRtLarge; }

__host__ __device__ constexpr int train_ldz(int batch) { return ((batch + 63) & ~63) + 16; }
constexpr size_t train_lds_bytes(int rt) {
  const size_t stage = (size_t)train_rows(rt) * kTrainLd, panel = (size_t)kTrainCols * train_ldz(train_rows(rt));
  return ((stage > panel ? stage : panel) + kTrainCols * kTrainLd + 2 * kTrainCols) * sizeof(float);
}
static_assert(train_lds_bytes(kTrainRtLarge) <= (size_t)kMaxLdsBytes, "stage, weight stage and scalars fit the CU's LDS");

// what one layer's launch needs (the kernel's argument)
struct TrainArgs {
  hk_mlp_train_layer L;
  const float* a_in;  // [batch, k] dense: the block before's act; NULL: the stack's input (x0 | x1)
  const float* x0;
  const float* x1;
  int64_t x0_stride, x1_stride;
  int32_t k0, input_relu;
  int32_t batch;
  // backward
  int32_t n_next;        // 0: the last layer, d comes from grad
  const float* w_next;   // [n_next, n]
  const float* dz_next;  // [batch, n_next] dense
  const float* grad;     // [batch, n] grad_stride apart
  int64_t grad_stride;
  float* dz_out;  // [batch, n] dense or NULL (the first layer)
};

// column k of a row-major operand: element (b, k) is p[b * stride], through the ReLU where `relu`
struct TrainCol {
  const float* p;
  int64_t stride;
  bool relu;
  __device__ float at(int b) const {
    const float v = p[b * stride];
    return relu ? mlp_relu(v) : v;
  }
};

// column k of the layer's input a_l
__device__ inline TrainCol train_input(const TrainArgs& q, int k) {
  if (q.a_in) return TrainCol{q.a_in + k, q.L.k, false};
  if (k < q.k0) return TrainCol{q.x0 + k, q.x0_stride, q.input_relu != 0};
  return TrainCol{q.x1 + (k - q.k0), q.x1_stride, q.input_relu != 0};
}

// ROWSUM: thread `part` of the sixteen of a column adds the rows part, part + 16, ...; the tree runs over the sixteen
// adjacent lanes.  Lane part == 0 holds the rule's value.
template <class F>
__device__ inline float train_rowsum(F v, int batch, int part) {
  float s = 0.0f;
  for (int row = part; row < batch; row += 16) s = s + v(row);
  s = s + __shfl_xor(s, 8);
  s = s + __shfl_xor(s, 4);
  s = s + __shfl_xor(s, 2);
  s = s + __shfl_xor(s, 1);
  return s;
}

// acc[rt][r] (row (wave + 4 rt) * 16 + 4 lg + r, column lm) = CHAIN(acc; a(k).at(row) * w(lm, k), k < K) for the row tiles
// below `tiles`: a 16-k chunk of both operands goes through LDS, the next one waits in registers meanwhile
template <int RT, class FA, class FW>
__device__ inline void train_gemm(mlp_f4 (&acc)[RT], FA a, FW w, int K, int batch, float* stage, float* wstage, int tid) {
  const int lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6), lm = lane & 15, lg = lane >> 4;
  const int Kp = (K + 15) & ~15, tiles = (batch + 15) >> 4, kk = tid & 15, r0 = tid >> 4, pk = mlp_pos(kk);
  float ar[RT * 4], wr;
  auto load = [&](int kc) {
    // every address is clamped into the operand and the value masked afterwards, with no branch at all: a load inside
    // a branch of its own (a uniform one too) is waited for on the spot, sixteen in a row cost sixteen round trips
    const bool kin = kc + kk < K;
    const int kq = kin ? kc + kk : K - 1;
    const TrainCol col = a(kq);
#pragma unroll
    for (int i = 0; i < RT * 4; ++i) {
      const int row = r0 + 16 * i;
      const float v = col.at(row < batch ? row : batch - 1);
      ar[i] = row < batch && kin ? v : 0.0f;
    }
    const float wv = w(r0, kq);
    wr = kin ? wv : 0.0f;
  };
  load(0);
  for (int kc = 0; kc < Kp; kc += kMlpKc) {
    __syncthreads();  // the stage is free
#pragma unroll
    for (int i = 0; i < RT * 4; ++i)
      if (i < tiles) stage[(r0 + 16 * i) * kTrainLd + pk] = ar[i];
    wstage[r0 * kTrainLd + pk] = wr;
    __syncthreads();
    if (kc + kMlpKc < Kp) load(kc + kMlpKc);
    const mlp_f4 b = *reinterpret_cast<const mlp_f4*>(wstage + lm * kTrainLd + 4 * lg);
    mlp_f4 av[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
      if (wave + kTrainWaves * rt < tiles)
        av[rt] = *reinterpret_cast<const mlp_f4*>(stage + ((wave + kTrainWaves * rt) * 16 + lm) * kTrainLd + 4 * lg);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
        if (wave + kTrainWaves * rt < tiles)
          acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt][t], b[t], acc[rt], 0, 0, 0);
  }
  __syncthreads();  // the stage may become the panel
}

template <int RT>
__global__ __launch_bounds__(kTrainThreads) void mlp_train_forward_kernel(const TrainArgs q) {
  extern __shared__ __align__(16) float hk_train_lds[];
  constexpr size_t kStage = (size_t)train_rows(RT) * kTrainLd, kPanel = (size_t)kTrainCols * train_ldz(train_rows(RT));
  float* const stage = hk_train_lds;
  float* const panel = hk_train_lds;
  float* const wstage = hk_train_lds + (kStage > kPanel ? kStage : kPanel);
  float* const stat = wstage + kTrainCols * kTrainLd;
  const hk_mlp_train_layer& L = q.L;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6), lm = lane & 15, lg = lane >> 4;
  const int K = L.k, N = L.n, B = q.batch, c0 = blockIdx.x * kTrainCols, ldz = train_ldz(B), tiles = (B + 15) >> 4;
  const float* W = static_cast<const float*>(L.weight);
  const float* bias = static_cast<const float*>(L.bias);
  const int col = c0 + lm;
  const bool cvalid = col < N;

  mlp_f4 acc[RT];
  {
    const float b0 = bias && cvalid ? bias[col] : 0.0f;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt] = mlp_f4{b0, b0, b0, b0};
  }
  train_gemm<RT>(
      acc, [&](int k) { return train_input(q, k); },
      [&](int c, int k) {
        const float v = W[(int64_t)(c0 + c < N ? c0 + c : N - 1) * K + k];
        return c0 + c < N ? v : 0.0f;
      },
      K, B, stage, wstage, tid);

  const bool bn = L.flags & HK_MLP_TRAIN_BN;
  float mean = 0.0f, inv = 1.0f;
  if (bn) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
      if (wave + kTrainWaves * rt < tiles)
#pragma unroll
        for (int r = 0; r < 4; ++r) panel[lm * ldz + (wave + kTrainWaves * rt) * 16 + mlp_pos(4 * lg + r)] = acc[rt][r];
    __syncthreads();
    const int c = tid >> 4, part = tid & 15, pp = mlp_pos(part), cc = c0 + c;
    const float* pc = panel + c * ldz + pp;  // row 16 t + part sits at 16 t + pos(part)
    const float fb = (float)B;
    const float m = train_rowsum([&](int row) { return pc[row - part]; }, B, part) / fb;
    const float var = train_rowsum(
                          [&](int row) {
                            const float e = pc[row - part] - m;
                            return e * e;
                          },
                          B, part) / fb;
    const float iv = 1.0f / sqrtf(var + L.eps);
    if (part == 0) {
      stat[c] = m, stat[kTrainCols + c] = iv;
      if (cc < N) {
        static_cast<float*>(L.mean)[cc] = m;
        static_cast<float*>(L.inv)[cc] = iv;
        float* rm = static_cast<float*>(L.running_mean);
        float* rv = static_cast<float*>(L.running_var);
        const float keep = 1.0f - L.momentum;
        rm[cc] = fmaf(L.momentum, m, keep * rm[cc]);
        rv[cc] = fmaf(L.momentum, var * (fb / (fb - 1.0f)), keep * rv[cc]);
      }
    }
    if (tid == 0 && blockIdx.x == 0 && L.num_batches_tracked) {
      long long* nbt = static_cast<long long*>(L.num_batches_tracked);
      *nbt = *nbt + 1;
    }
    __syncthreads();
    mean = stat[lm], inv = stat[kTrainCols + lm];
  }
  const float gamma = bn && L.bn_weight && cvalid ? static_cast<const float*>(L.bn_weight)[col] : 1.0f;
  const float beta = bn && L.bn_bias && cvalid ? static_cast<const float*>(L.bn_bias)[col] : 0.0f;
  const bool relu = L.flags & HK_MLP_RELU;
  float* zo = static_cast<float*>(L.z);
  float* ao = static_cast<float*>(L.act);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
    if (wave + kTrainWaves * rt < tiles)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = (wave + kTrainWaves * rt) * 16 + 4 * lg + r;
        float v = acc[rt][r];
        if (cvalid && row < B) {
          const int64_t at = (int64_t)row * N + col;
          if (bn) {
            zo[at] = v;
            v = fmaf((v - mean) * inv, gamma, beta);
          }
          ao[at] = relu ? mlp_relu(v) : v;
        }
      }
}

template <int RT>
__global__ __launch_bounds__(kTrainThreads) void mlp_train_backward_kernel(const TrainArgs q) {
  extern __shared__ __align__(16) float hk_train_lds[];
  constexpr size_t kStage = (size_t)train_rows(RT) * kTrainLd, kPanel = (size_t)kTrainCols * train_ldz(train_rows(RT));
  float* const stage = hk_train_lds;
  float* const panel = hk_train_lds;
  float* const wstage = hk_train_lds + (kStage > kPanel ? kStage : kPanel);
  float* const stat = wstage + kTrainCols * kTrainLd;
  const hk_mlp_train_layer& L = q.L;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6), lm = lane & 15, lg = lane >> 4;
  const int K = L.k, N = L.n, B = q.batch, c0 = blockIdx.x * kTrainCols, ldz = train_ldz(B), tiles = (B + 15) >> 4;
  const int col = c0 + lm;
  const bool cvalid = col < N;
  const bool bn = L.flags & HK_MLP_TRAIN_BN, relu = L.flags & HK_MLP_RELU;
  const float* act = static_cast<const float*>(L.act);
  const float* zs = static_cast<const float*>(L.z);

  // d, masked by the ReLU
  mlp_f4 d[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) d[rt] = mlp_f4{0.0f, 0.0f, 0.0f, 0.0f};
  if (q.n_next > 0) {
    const float* Wn = q.w_next;
    const float* dzn = q.dz_next;
    const int Nn = q.n_next;
    train_gemm<RT>(
        d, [&](int j) { return TrainCol{dzn + j, Nn, false}; },
        [&](int c, int j) {
          const float v = Wn[(int64_t)j * N + (c0 + c < N ? c0 + c : N - 1)];
          return c0 + c < N ? v : 0.0f;
        },
        Nn, B, stage, wstage, tid);
  }
  mlp_f4 xhat[RT];
  float mean = 0.0f, inv = 1.0f;
  if (bn && cvalid) mean = static_cast<const float*>(L.mean)[col], inv = static_cast<const float*>(L.inv)[col];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (wave + kTrainWaves * rt) * 16 + 4 * lg + r;
      // (the addresses clamped, the values masked: see train_gemm)
      const int rq = row < B ? row : B - 1, cq = cvalid ? col : N - 1;
      const int64_t at = (int64_t)rq * N + cq;
      float v = d[rt][r], xh = 0.0f;
      if (q.n_next == 0) v = q.grad[rq * q.grad_stride + cq];
      if (relu) v = act[at] > 0.0f ? v : 0.0f;
      if (bn) xh = (zs[at] - mean) * inv;
      if (!(cvalid && row < B)) v = 0.0f, xh = 0.0f;
      d[rt][r] = v, xhat[rt][r] = xh;
    }

  const int c = tid >> 4, part = tid & 15, pp = mlp_pos(part), cc = c0 + c;
  const float* pc = panel + c * ldz + pp;
  auto to_panel = [&](auto value) {  // value(rt, r) of every owned element into the panel, then the barrier
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
      if (wave + kTrainWaves * rt < tiles)
#pragma unroll
        for (int r = 0; r < 4; ++r) panel[lm * ldz + (wave + kTrainWaves * rt) * 16 + mlp_pos(4 * lg + r)] = value(rt, r);
    __syncthreads();
  };
  auto column_sum = [&]() { return train_rowsum([&](int row) { return pc[row - part]; }, B, part); };

  if (bn) {
    const float fb = (float)B;
    to_panel([&](int rt, int r) { return d[rt][r]; });
    const float dbeta = column_sum();
    __syncthreads();
    to_panel([&](int rt, int r) { return d[rt][r] * xhat[rt][r]; });
    const float dgamma = column_sum();
    if (part == 0) {
      stat[c] = dbeta / fb, stat[kTrainCols + c] = dgamma / fb;
      if (cc < N) {
        if (L.d_bn_bias) static_cast<float*>(L.d_bn_bias)[cc] = dbeta;
        if (L.d_bn_weight) static_cast<float*>(L.d_bn_weight)[cc] = dgamma;
      }
    }
    __syncthreads();
    const float c1 = stat[lm], c2 = stat[kTrainCols + lm];
    const float g = L.bn_weight && cvalid ? static_cast<const float*>(L.bn_weight)[col] * inv : inv;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = (wave + kTrainWaves * rt) * 16 + 4 * lg + r;
        const float v = g * ((d[rt][r] - c1) - xhat[rt][r] * c2);
        d[rt][r] = cvalid && row < B ? v : 0.0f;
      }
  }
  // dz: to the panel for the two sums below, to memory for the layer before
  to_panel([&](int rt, int r) { return d[rt][r]; });
  if (q.dz_out && cvalid) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = (wave + kTrainWaves * rt) * 16 + 4 * lg + r;
        if (wave + kTrainWaves * rt < tiles && row < B) q.dz_out[(int64_t)row * N + col] = d[rt][r];
      }
  }
  {
    const float dbias = column_sum();
    if (part == 0 && cc < N && L.d_bias) static_cast<float*>(L.d_bias)[cc] = dbias;
  }

  // dW[c0 + i, k] = CHAIN over the rows: A = dz^T from the panel, B = a_in[rows, k] from memory
  constexpr int KT = kMlpColumnTiles / kTrainWaves;
  const int KTn = (K + 15) >> 4;
  mlp_f4 dw[KT];
#pragma unroll
  for (int i = 0; i < KT; ++i) dw[i] = mlp_f4{0.0f, 0.0f, 0.0f, 0.0f};
  TrainCol incol[KT];
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    const int k = (wave + kTrainWaves * i) * 16 + lm;
    incol[i] = train_input(q, k < K ? k : K - 1);
  }
  for (int T = 0; T < tiles; ++T) {
    const mlp_f4 a = *reinterpret_cast<const mlp_f4*>(panel + lm * ldz + 16 * T + 4 * lg);
    float bv[KT][4];
#pragma unroll
    for (int i = 0; i < KT; ++i) {
      const int k = (wave + kTrainWaves * i) * 16 + lm;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int row = 16 * T + 4 * t + lg;
        const float v = incol[i].at(row < B ? row : B - 1);
        bv[i][t] = k < K && row < B ? v : 0.0f;
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < KT; ++i)
        if (wave + kTrainWaves * i < KTn) dw[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], bv[i][t], dw[i], 0, 0, 0);
  }
  float* dW = static_cast<float*>(L.d_weight);
#pragma unroll
  for (int i = 0; i < KT; ++i) {
    const int k = (wave + kTrainWaves * i) * 16 + lm;
    if (wave + kTrainWaves * i < KTn && k < K)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = c0 + 4 * lg + r;
        if (j < N) dW[(int64_t)j * K + k] = dw[i][r];
      }
  }
}

}  // namespace hk
