// hk::mlp_kernel -- the eval-mode forward of a create_mlp stack in one launch (include/hironaka_hip_mlp.h states the
// rule).  One workgroup of 4 waves (16 rows) or 16 waves (64 rows) carries TR batch rows through every layer; the
// activations ping-pong between two LDS panels, the weights pass through a 16-k stage of LDS, the products run on
// v_mfma_f32_16x16x4_f32, which is bit for bit a k-ordered fmaf chain.  The tile (MlpTile), the input load
// (mlp_load_rows) and the Dense k-loop (mlp_dense) are hk::pvnet_kernel's too (hk_pvnet_kernel.h): its one copy is here.
//
// ---- who computes what ----
// A layer's output is MT = TR / 16 row tiles x NT = ceil(n / 16) column tiles of 16 x 16.  Wave w of W owns the column
// tiles w, w + W, ... (those below NT) of EVERY row tile: up to 16 / W x MT accumulators of 4 registers, each ONE chain
// over the whole K in ascending k -- K is never split, the independent accumulators that hide the MFMA's 40-cycle
// dependent latency are different output tiles.  The A operand (activations) is shared by a wave's column tiles, the B
// operand (weights) by its row tiles.
//
// ---- the LDS image ----
// The MFMA takes A[i = lane & 15][k = lane >> 4] and B[k = lane >> 4][j = lane & 15]: instruction t of a chain must hold
// the real k's 4t .. 4t+3 on the lane groups g = 0 .. 3, so a lane needs k = g, 4 + g, 8 + g, 12 + g of every 16.  Both
// images therefore keep each run of 16 k's TRANSPOSED 4 x 4: real k = 16T + 4t + g sits at position 16T + 4g + t
// (mlp_pos), and one 16-byte ds_read_b128 at 16T + 4g gives a lane its operands of four consecutive MFMAs.
//   activations  [TR rows][kMlpLda = 260 floats], two panels (2 x 64 x 260 x 4 = 130 KiB at TR = 64)
//   weight stage [256 rows j][kMlpLdw = 20 floats]: W[j][kc .. kc+15], 20 KiB, refilled per 16 k's
// The weights come from memory as 16-byte loads along k (4 lanes cover 64 contiguous bytes of one row of W; rows whose
// base or length is no multiple of 16 bytes go float by float), wait in registers while the chunk before them is
// multiplied, and are written into the stage as 4 ds_write_b32 per load: the transposition happens in that write.
// Widths that are no multiple of 16 are padded with zeros in both images, behind the real k's; a layer's epilogue
// writes the zeros of the next layer's padding itself.
//
// ---- banks (64 banks of 4 bytes) ----
// Row strides of 260 and 20 floats are 4 and 20 banks.  ds_read_b128 serves 16 lanes per LDS cycle.  A lane reads the
// banks 4m + 4g + c (activations) or 20j + 4g + c (stage), c = 0..3, m / j = lane & 15: for one g the 16 rows cover the
// 64 banks exactly once (4m and 20j mod 64 run through the 16 multiples of 4).  The hardware's groups of 16 are not one
// g each but {0-3, 12-15, 20-27} and their like: 8 rows of one g and 8 of the next, whose shifted quads meet in ONE
// quad of banks -- one 2-way conflict per group, 5 LDS cycles instead of 4 per read.  At 5 to 8 reads per 16 to
// 64 MFMAs of 32 cycles of a wave that is not where the time goes; no stride of the form 256 + 4 * odd removes it.
// The stage's ds_write_b32 of a wave go to 20 * row + 4c + q for 16 rows x 4 q: 64 different banks.  The epilogue's
// ds_write_b32 of register r go to 4 * (4g + r) + pos(j): 16 positions of one run of 16 on the lanes of a group, the
// groups 16 banks apart -- 64 different banks again.
#pragma once
#include "hk_common.h"

namespace hk {

// waves of a workgroup: 4 carry 16 rows; 64 rows take 16, four per SIMD with one column tile of the widest layer each,
// so that one wave's LDS reads, barriers and weight loads hide behind the others' MFMAs (the LDS allows one such
// workgroup per CU either way; measured at 65 536 rows of the example config: 4 waves 3.45 ms, 8 waves 2.28, 16 1.88)
constexpr int mlp_waves(int tile_rows) { return tile_rows > 16 ? 16 : 4; }
constexpr int kMlpLda = HK_MLP_MAX_WIDTH + 4;
constexpr int kMlpKc = 16;
constexpr int kMlpLdw = kMlpKc + 4;
constexpr int kMlpColumnTiles = HK_MLP_MAX_WIDTH / 16;
// the compute units the row tile is chosen for (gfx950: 256)
constexpr int kMlpCus = 256;

static_assert(sizeof(hk_mlp_desc) <= 4096 - 64, "the layer table travels as the kernel's argument");
static_assert(HK_MLP_TILE_CROSSOVER == HK_MLP_TILE_SMALL * kMlpCus, "the header's crossover");
static_assert(kMlpColumnTiles % mlp_waves(HK_MLP_TILE_SMALL) == 0 && kMlpColumnTiles % mlp_waves(HK_MLP_TILE_LARGE) == 0 &&
                  HK_MLP_MAX_WIDTH <= kWave * mlp_waves(HK_MLP_TILE_SMALL), "tiling: a thread per input column");

// THE place the row tile is picked: 16 rows while every 16-row workgroup has a compute unit to itself (64-row tiles
// would leave three in four idle), 64 beyond.  Measured on the example config: 16-row tiles take 0.55 ms from 256 to
// 4 096 rows and 1.15 ms at 16 320 (four workgroups per CU), 64-row tiles 0.47 ms per round of 256 workgroups.
inline int mlp_row_tile(int64_t batch, uint32_t flags = 0) {
  if (flags & HK_MLP_FORCE_TILE_SMALL) return HK_MLP_TILE_SMALL;
  if (flags & HK_MLP_FORCE_TILE_LARGE) return HK_MLP_TILE_LARGE;
  return batch <= HK_MLP_TILE_CROSSOVER ? HK_MLP_TILE_SMALL : HK_MLP_TILE_LARGE;
}

constexpr size_t mlp_lds_bytes(int tile_rows) {
  return ((size_t)2 * tile_rows * kMlpLda + (size_t)HK_MLP_MAX_WIDTH * kMlpLdw) * sizeof(float);
}
static_assert(mlp_lds_bytes(HK_MLP_TILE_LARGE) <= (size_t)kMaxLdsBytes, "two panels and the stage fit the CU's LDS");

// ---- what every entry point that takes a layer table asks of it (Desc: hk_mlp_desc, hk_mlp_train_desc) ----------------
// The checks come in the order of the headers' status rules; an entry puts its own between them.
// The descriptor itself: there, float, no flag outside `known`.
template <typename Desc>
int mlp_check_desc(const Desc* q, uint32_t known) {
  if (!q) return HK_ERR_NULL;
  if (q->dtype != HK_F32) return HK_ERR_UNSUPPORTED;
  return (q->flags & ~known) ? HK_ERR_UNSUPPORTED : HK_OK;
}
// The sizes: nlayers, the batch, the input's widths and strides, every layer's flags (within `layer_flags`) and the chain
// of widths, whose end -- the last layer's n -- `width` receives.
template <typename Desc>
int mlp_check_sizes(const Desc* q, uint32_t layer_flags, int64_t& width) {
  if (q->nlayers < 1 || q->nlayers > HK_MLP_MAX_LAYERS) return HK_ERR_SHAPE;
  if (q->batch < 0 || q->k0 < 1 || q->k1 < 0 || q->x0_stride < 0 || q->x1_stride < 0) return HK_ERR_SHAPE;
  width = (int64_t)q->k0 + q->k1;
  for (int l = 0; l < q->nlayers; ++l) {
    const auto& L = q->layer[l];
    if (L.flags & ~layer_flags) return HK_ERR_UNSUPPORTED;
    if (L.k < 1 || L.k > HK_MLP_MAX_WIDTH || L.n < 1 || L.n > HK_MLP_MAX_WIDTH || L.k != width) return HK_ERR_SHAPE;
    width = L.n;
  }
  return HK_OK;
}
template <typename Desc>
bool mlp_input_missing(const Desc* q) {
  return !q->x0 || (q->k1 > 0 && !q->x1);
}
// The bytes the rows of x0 and of x1 span (1 for an absent x1); false: rows, and a span beyond 2^63 bytes.
template <typename Desc>
bool mlp_input_spans(const Desc* q, uint64_t& x0_bytes, uint64_t& x1_bytes) {
  x0_bytes = span_bytes(q->batch, q->x0_stride, q->k0, sizeof(float));
  x1_bytes = q->k1 > 0 ? span_bytes(q->batch, q->x1_stride, q->k1, sizeof(float)) : 1;
  return q->batch == 0 || (x0_bytes && x1_bytes);
}

// where real k sits in a row of either image
__host__ __device__ constexpr int mlp_pos(int k) { return (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3); }

typedef float mlp_f4 __attribute__((ext_vector_type(4)));

__device__ inline float mlp_relu(float x) { return x < 0.0f ? 0.0f : x; }

// this thread's share of W[:, kc .. kc+15]: rows (tid >> 2) + PER i of the PER = threads / 4 rows a pass covers, the
// floats kc + 4 (tid & 3) .. + 3; zeros outside W
template <int PASSES>
__device__ inline void mlp_load_w(mlp_f4 (&w)[PASSES], const float* W, int K, int N, int rows, int kc, bool vec, int tid) {
  constexpr int PER = HK_MLP_MAX_WIDTH / PASSES;
  const int k = kc + 4 * (tid & 3);
#pragma unroll
  for (int i = 0; i < PASSES; ++i) {
    const int row = (tid >> 2) + PER * i;
    mlp_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (PER * i < rows && row < N) {
      const float* p = W + row * K + k;
      if (vec) {
        if (k < K) v = *reinterpret_cast<const mlp_f4*>(p);  // K is a multiple of 4 here: all four or none
      } else {
        if (k + 0 < K) v.x = p[0];
        if (k + 1 < K) v.y = p[1];
        if (k + 2 < K) v.z = p[2];
        if (k + 3 < K) v.w = p[3];
      }
    }
    w[i] = v;
  }
}

// the tile of a workgroup that carries TR rows: MT row tiles, W waves of TPW column tiles each (the accumulators Acc), and
// the PASSES of PER rows in which its threads cover the weight stage (mlp_load_w)
template <int TR>
struct MlpTile {
  static constexpr int MT = TR / 16, W = mlp_waves(TR), TPW = kMlpColumnTiles / W;
  static constexpr int PASSES = HK_MLP_MAX_WIDTH / (W * kWave / 4), PER = HK_MLP_MAX_WIDTH / PASSES;
  typedef mlp_f4 Acc[MT][TPW];
};

// the rows a workgroup starts from: x0 | x1 per row, x1_stride apart; the batch norm (bn_mean: there is one) and the
// ReLU come before the first layer.  Only the x0 fields count where mlp_load_rows is told so.
struct MlpInput {
  const float *x0, *x1;
  int64_t x0_stride, x1_stride;
  int k0, k1;
  const float *bn_mean, *bn_var, *bn_weight, *bn_bias;
  float eps;
  bool relu;
};

// the input rows row0 .. row0 + TR - 1 into the panel `dst`: thread k of a row, zeros behind the width and below the
// batch.  EXTRAS: the second segment, the batch norm and the ReLU of `in` (false: x0 alone, as it is)
template <int TR, bool EXTRAS>
__device__ __forceinline__ void mlp_load_rows(float* dst, const MlpInput& in, int64_t row0, int64_t batch, int tid) {
  const int K = EXTRAS ? in.k0 + in.k1 : in.k0, Kp = (K + 15) & ~15;
  if (tid < Kp) {
    const int p = mlp_pos(tid);
    const bool bn = EXTRAS && in.bn_mean && tid < K;
    float mu = 0.0f, alpha = 1.0f, beta = 0.0f;
    if (bn) {
      mu = in.bn_mean[tid];
      const float inv = 1.0f / sqrtf(in.bn_var[tid] + in.eps);
      alpha = in.bn_weight ? in.bn_weight[tid] * inv : inv;
      beta = in.bn_bias ? in.bn_bias[tid] : 0.0f;
    }
#pragma unroll 4
    for (int r = 0; r < TR; ++r) {
      const int64_t b = row0 + r;
      float v = 0.0f;
      if (b < batch && tid < K) {
        v = !EXTRAS || tid < in.k0 ? in.x0[b * in.x0_stride + tid] : in.x1[b * in.x1_stride + (tid - in.k0)];
        if (bn) v = fmaf(v - mu, alpha, beta);
        if (EXTRAS && in.relu) v = mlp_relu(v);
      }
      dst[r * kMlpLda + p] = v;
    }
  }
}

// acc = Dense(src): N outputs over K inputs, every chain started from its bias (NULL: 0).  HEADS: the last of the N rows
// of the weight comes from Wv (its bias from bv, NULL: 0) and the N - 1 before it from W -- hk::pvnet_kernel's two
// heads as one layer; without HEADS all N come from W, and Wv and bv are not looked at.
// The chunk of 16 k's a pass multiplies waits in the stage `wst`, the one behind it in the registers w: the first
// barrier of a pass says that every wave has read the stage (and, at kc == 0, that whoever wrote the panel `src` is
// done), the second that the stage is written.  Nothing waits behind the last pass: a caller may write the OTHER panel
// right after the call (every wave left its last read of it before this call's barriers), but other waves may still be
// reading `src` and the stage until the next call's first barrier.  Stage writes and ds_read_b128 reads: the bank
// notes at the head of this file.
template <int TR, bool HEADS>
__device__ __forceinline__ void mlp_dense(typename MlpTile<TR>::Acc& acc, const float* src, float* wst, const float* W,
                                          const float* bias, const float* Wv, const float* bv, int K, int N, int tid) {
  typedef MlpTile<TR> T;
  const int lane = tid & (kWave - 1), wave = tid >> 6, lm = lane & 15, lg = lane >> 4;
  const int Kp = (K + 15) & ~15, NT = (N + 15) >> 4, rows = NT * 16;
  const int NW = HEADS ? N - 1 : N;  // the rows W holds
  const bool vec = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15u) == 0;
#pragma unroll
  for (int i = 0; i < T::TPW; ++i) {
    const int j = (wave + T::W * i) * 16 + lm;
    float b0 = bias && j < NW ? bias[j] : 0.0f;
    if (HEADS && bv && j == NW) b0 = bv[0];
#pragma unroll
    for (int mt = 0; mt < T::MT; ++mt) acc[mt][i] = mlp_f4{b0, b0, b0, b0};
  }
  mlp_f4 w[T::PASSES];
  auto load = [&](int kc) {
    mlp_load_w<T::PASSES>(w, W, K, NW, rows, kc, vec, tid);
    if (HEADS) {  // the value row, float by float: one row of the chunk
      const int k = kc + 4 * (tid & 3);
#pragma unroll
      for (int i = 0; i < T::PASSES; ++i)
        if ((tid >> 2) + T::PER * i == NW) {
          if (k + 0 < K) w[i].x = Wv[k + 0];
          if (k + 1 < K) w[i].y = Wv[k + 1];
          if (k + 2 < K) w[i].z = Wv[k + 2];
          if (k + 3 < K) w[i].w = Wv[k + 3];
        }
    }
  };
  load(0);
  for (int kc = 0; kc < Kp; kc += kMlpKc) {
    __syncthreads();  // the stage is free (and, at kc == 0, the panel `src` is complete)
#pragma unroll
    for (int i = 0; i < T::PASSES; ++i)
      if (T::PER * i < rows) {
        float* s = wst + ((tid >> 2) + T::PER * i) * kMlpLdw + (tid & 3);
        s[0] = w[i].x, s[4] = w[i].y, s[8] = w[i].z, s[12] = w[i].w;
      }
    __syncthreads();
    if (kc + kMlpKc < Kp) load(kc + kMlpKc);
    mlp_f4 a[T::MT];
#pragma unroll
    for (int mt = 0; mt < T::MT; ++mt)
      a[mt] = *reinterpret_cast<const mlp_f4*>(src + (mt * 16 + lm) * kMlpLda + kc + 4 * lg);
#pragma unroll
    for (int i = 0; i < T::TPW; ++i) {
      const int nt = wave + T::W * i;
      if (nt < NT) {
        const mlp_f4 b = *reinterpret_cast<const mlp_f4*>(wst + (nt * 16 + lm) * kMlpLdw + 4 * lg);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int mt = 0; mt < T::MT; ++mt)
            acc[mt][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt][t], b[t], acc[mt][i], 0, 0, 0);
      }
    }
  }
}

template <int TR>
__global__ __launch_bounds__(kWave * mlp_waves(TR)) void mlp_kernel(const hk_mlp_desc q) {
  typedef MlpTile<TR> T;
  extern __shared__ __align__(16) float hk_mlp_lds[];
  float* cur = hk_mlp_lds;
  float* nxt = cur + TR * kMlpLda;
  float* const wst = nxt + TR * kMlpLda;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int lm = lane & 15, lg = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * TR;
  auto f = [](const void* p) { return static_cast<const float*>(p); };

  mlp_load_rows<TR, true>(cur,
                          MlpInput{f(q.x0), f(q.x1), q.x0_stride, q.x1_stride, q.k0, q.k1, f(q.in_bn_mean), f(q.in_bn_var),
                                   f(q.in_bn_weight), f(q.in_bn_bias), q.in_eps, (q.flags & HK_MLP_INPUT_RELU) != 0},
                          row0, q.batch, tid);

  for (int l = 0; l < q.nlayers; ++l) {
    const hk_mlp_layer& L = q.layer[l];
    const int N = L.n, NT = (N + 15) >> 4;
    const bool last = l + 1 == q.nlayers;
    typename T::Acc acc;
    mlp_dense<TR, false>(acc, cur, wst, f(L.weight), f(L.bias), nullptr, nullptr, L.k, N, tid);

    // epilogue: C/D has its column j on lane & 15 and its rows 4 (lane >> 4) + r in the registers
    const float* mean = f(L.bn_mean);
    const float* var = f(L.bn_var);
    const float* gamma = f(L.bn_weight);
    const float* beta_p = f(L.bn_bias);
    const bool relu = L.flags & HK_MLP_RELU;
    float* out = static_cast<float*>(q.out);
#pragma unroll
    for (int i = 0; i < T::TPW; ++i) {
      const int nt = wave + T::W * i;
      if (nt < NT) {
        const int j = nt * 16 + lm;
        const bool valid = j < N;
        float mu = 0.0f, alpha = 1.0f, beta = 0.0f;
        if (mean && valid) {
          mu = mean[j];
          const float inv = 1.0f / sqrtf(var[j] + L.eps);
          alpha = gamma ? gamma[j] * inv : inv;
          beta = beta_p ? beta_p[j] : 0.0f;
        }
        const int pj = mlp_pos(j);
#pragma unroll
        for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = mt * 16 + 4 * lg + r;
            float v = acc[mt][i][r];
            if (mean) v = fmaf(v - mu, alpha, beta);
            if (relu) v = mlp_relu(v);
            if (last) {
              if (valid && row0 + row < q.batch) out[(row0 + row) * q.out_stride + j] = v;
            } else {
              nxt[row * kMlpLda + pj] = valid ? v : 0.0f;
            }
          }
      }
    }
    float* const swap = cur;
    cur = nxt;
    nxt = swap;
  }
}

// ---- the host's side of a kernel on this tile (hk_mlp.hip, hk_pvnet.hip) -------------------------------------------------
// a descriptor may force one row tile, not both
inline bool mlp_forces_both_tiles(uint32_t flags) {
  return (flags & HK_MLP_FORCE_TILE_SMALL) && (flags & HK_MLP_FORCE_TILE_LARGE);
}
// the launch over q.batch rows of the instantiation mlp_row_tile picks: `small` is the kernel's <HK_MLP_TILE_SMALL>,
// `large` its <HK_MLP_TILE_LARGE>
template <typename Desc>
int mlp_launch(void (*small)(const Desc), void (*large)(const Desc), const Desc& q, hipStream_t stream) {
  const int tr = mlp_row_tile(q.batch, q.flags);
  return launch_kernel_lds(tr == HK_MLP_TILE_LARGE ? large : small, 48 * 1024, dim3((unsigned)workgroups(q.batch, tr)),
                           dim3(kWave * mlp_waves(tr)), mlp_lds_bytes(tr), stream, q);
}

}  // namespace hk
