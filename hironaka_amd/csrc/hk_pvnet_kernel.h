// hk::pvnet_kernel -- the gradient-free forward of a DenseResNet / DenseNet policy-value network in one launch
// (include/hironaka_hip_pvnet.h states the rule).  The scheme is hk::mlp_kernel's (hk_mlp_kernel.h: who computes what, the
// LDS image, mlp_pos, the banks) and so is the code: MlpTile, the input load mlp_load_rows and every Dense, mlp_dense.
// A workgroup of 4 waves carries 16 rows, one of 16 waves 64 rows, through every block and both heads; the rows live in
// two LDS panels, the weights pass through the 16-k stage, every Dense is one k-ordered chain per output on
// v_mfma_f32_16x16x4_f32.  What is this kernel's own:
//
// ---- the group norm, in the registers of the MFMA's result ----
// C/D has column j on lane & 15 and the rows 4 (lane >> 4) + r in its four registers.  A group is g = n / 32 in
// {1, 2, 4, 8} ADJACENT columns and 16 is a multiple of each: a group is g adjacent lanes of one 16-lane row and never
// leaves a column tile.  The two balanced sums of the rule are therefore lane exchanges inside a DPP row: xor 1 and
// xor 2 as quad permutes, xor 4 as row_half_mirror (lane i <- lane 7 - i of its half row: the OTHER quad, whose four
// lanes all hold the same sum after the first two levels).  A float add is commutative, so both lanes of a pair, and in
// the end all lanes of a group, hold the same bits -- the rule's.  No LDS round trip, no barrier.
//
// ---- the residual, without a third panel ----
// The block's input h sits in panel `cur`.  Dense1 writes relu(GN1(.)) into `nxt`; Dense2 reads `nxt`, and its epilogue
// reads h at the same (row, position) of `cur`, adds, and writes relu(o + y) back over it: every element is read and
// written by the one thread that owns (row, j) in C/D.  Every wave left its last read of `cur` (Dense1's k-loop) before
// the barriers of Dense2's k-loop, which every wave passes before its epilogue.  Where the block changes the width the
// projection runs first, over `cur`, and its normed result waits in 16 accumulator registers (at either tile) for
// Dense2's epilogue: Densep and Dense2 have the same (row, j) on the same thread.
//
// ---- the heads ----
// One last layer of actions + 1 columns: rows j < actions of the stage come from the policy weight, row `actions` from
// the value weight (float by float: one row of the 16-k chunk), the chains start from the two biases; the epilogue
// stores columns j < actions to policy and tanhf (or, HK_PVNET_RAW_VALUE, the value itself) of column `actions` to value.
#pragma once
#include "hk_mlp_kernel.h"

namespace hk {

static_assert(sizeof(hk_pvnet_desc) <= 4096 - 64, "the block table travels as the kernel's argument");
static_assert(sizeof(hk_pvnet_block) == 112, "three (weight, bias, scale, bias) quadruples, eps, k, n, kind");
static_assert(HK_PVNET_MAX_WIDTH == HK_MLP_MAX_WIDTH && HK_PVNET_FORCE_TILE_SMALL == HK_MLP_FORCE_TILE_SMALL &&
                  HK_PVNET_FORCE_TILE_LARGE == HK_MLP_FORCE_TILE_LARGE, "the panels, the stage and the tiles are hk_mlp_forward's");

// the widths a normed layer may have: g = n / 32 columns per group, a power of two that divides the MFMA's 16
inline bool pvnet_normed_width(int n) { return n == 32 || n == 64 || n == 128 || n == 256; }

template <int CTRL>
__device__ __forceinline__ float pvnet_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// the balanced sum over the g adjacent lanes of a group (every lane of the wave is active here); see the header comment
__device__ __forceinline__ float pvnet_group_sum(float v, int g) {
  if (g >= 2) v = v + pvnet_dpp<0xB1>(v);   // quad_perm [1, 0, 3, 2]: lane ^ 1
  if (g >= 4) v = v + pvnet_dpp<0x4E>(v);   // quad_perm [2, 3, 0, 1]: lane ^ 2
  if (g >= 8) v = v + pvnet_dpp<0x141>(v);  // row_half_mirror: a lane of the quad lane ^ 4 lies in
  return v;
}

// acc = GN(acc) over the N columns (a normed width: every column of a tile below N / 16 is real)
template <int TR>
__device__ __forceinline__ void pvnet_group_norm(typename MlpTile<TR>::Acc& acc, const hk_pvnet_dense& D, float eps, int N,
                                                 int tid) {
  typedef MlpTile<TR> T;
  const int wave = tid >> 6, lm = tid & 15;
  const int g = N >> 5;
  const float rg = 1.0f / (float)g;  // a power of two: the product with it is the rule's quotient, to the bit
  const float* scale = static_cast<const float*>(D.gn_scale);
  const float* shift = static_cast<const float*>(D.gn_bias);
#pragma unroll
  for (int i = 0; i < T::TPW; ++i) {
    const int nt = wave + T::W * i;
    if (nt * 16 < N) {
      const int j = nt * 16 + lm;
      const float gamma = scale ? scale[j] : 1.0f, beta = shift ? shift[j] : 0.0f;
#pragma unroll
      for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float z = acc[mt][i][r];
          const float d = z - pvnet_group_sum(z, g) * rg;
          const float inv = 1.0f / sqrtf(pvnet_group_sum(d * d, g) * rg + eps);
          acc[mt][i][r] = fmaf(d, scale ? gamma * inv : inv, beta);
        }
    }
  }
}

// dst[row][pos(j)] = relu(acc) for the columns below N, +0 behind them up to the next multiple of 16 (the next layer's
// padding); RESIDUAL: relu(o + acc) with o from `other` (a projection's result: `projected`) or from dst itself
template <int TR, bool RESIDUAL>
__device__ __forceinline__ void pvnet_store(const typename MlpTile<TR>::Acc& acc, float* dst, int N, int tid,
                                            const typename MlpTile<TR>::Acc& other, bool projected) {
  typedef MlpTile<TR> T;
  const int lane = tid & (kWave - 1), wave = tid >> 6, lm = lane & 15, lg = lane >> 4;
  const int NT = (N + 15) >> 4;
#pragma unroll
  for (int i = 0; i < T::TPW; ++i) {
    const int nt = wave + T::W * i;
    if (nt < NT) {
      const int j = nt * 16 + lm, pj = mlp_pos(j);
      const bool valid = j < N;
#pragma unroll
      for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* at = dst + (mt * 16 + 4 * lg + r) * kMlpLda + pj;
          float v = acc[mt][i][r];
          if (RESIDUAL) v = (projected ? other[mt][i][r] : *at) + v;
          *at = valid ? mlp_relu(v) : 0.0f;
        }
    }
  }
}

// the trunk on a workgroup's row tile: the `nblocks` blocks of `blocks` (a kernel argument's table or one in device
// memory) on the rows in `cur`; the result is in `cur` when it returns (a dense block swaps the panels).  The one copy of
// the block loop: pvnet_tile's and hk::customnet_kernel's (hk_customnet_kernel.h)
template <int TR>
__device__ __forceinline__ void pvnet_trunk(const hk_pvnet_block* blocks, int nblocks, float*& cur, float*& nxt,
                                            float* const wst, typename MlpTile<TR>::Acc& acc, int tid) {
  typedef MlpTile<TR> T;
  auto f = [](const void* p) { return static_cast<const float*>(p); };
  for (int l = 0; l < nblocks; ++l) {
    const hk_pvnet_block& B = blocks[l];
    const int K = B.k, N = B.n;
    if (B.kind == HK_PVNET_DENSE) {
      mlp_dense<TR, false>(acc, cur, wst, f(B.dense1.weight), f(B.dense1.bias), nullptr, nullptr, K, N, tid);
      pvnet_store<TR, false>(acc, nxt, N, tid, acc, false);
      float* const swap = cur;
      cur = nxt;
      nxt = swap;
      continue;
    }
    const bool proj = K != N;
    typename T::Acc o;
    if (proj) {
      mlp_dense<TR, false>(o, cur, wst, f(B.proj.weight), f(B.proj.bias), nullptr, nullptr, K, N, tid);
      pvnet_group_norm<TR>(o, B.proj, B.eps, N, tid);
    } else {
#pragma unroll
      for (int i = 0; i < T::TPW; ++i)
#pragma unroll
        for (int mt = 0; mt < T::MT; ++mt) o[mt][i] = mlp_f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    mlp_dense<TR, false>(acc, cur, wst, f(B.dense1.weight), f(B.dense1.bias), nullptr, nullptr, K, N, tid);
    pvnet_group_norm<TR>(acc, B.dense1, B.eps, N, tid);
    pvnet_store<TR, false>(acc, nxt, N, tid, acc, false);
    mlp_dense<TR, false>(acc, nxt, wst, f(B.dense2.weight), f(B.dense2.bias), nullptr, nullptr, N, N, tid);
    pvnet_group_norm<TR>(acc, B.dense2, B.eps, N, tid);
    pvnet_store<TR, true>(acc, cur, N, tid, o, proj);
  }
}

// the whole forward of a workgroup's row tile: the body of pvnet_kernel and of pvnet_gated_kernel
template <int TR>
__device__ __forceinline__ void pvnet_tile(const hk_pvnet_desc& q) {
  typedef MlpTile<TR> T;
  extern __shared__ __align__(16) float hk_pvnet_lds[];
  float* cur = hk_pvnet_lds;
  float* nxt = cur + TR * kMlpLda;
  float* const wst = nxt + TR * kMlpLda;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int lm = lane & 15, lg = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * TR;

  auto f = [](const void* p) { return static_cast<const float*>(p); };
  mlp_load_rows<TR, false>(cur, MlpInput{f(q.x), nullptr, q.x_stride, 0, q.k0}, row0, q.batch, tid);

  typename T::Acc acc;
  pvnet_trunk<TR>(q.block, q.nblocks, cur, nxt, wst, acc, tid);

  // the heads: columns 0 .. actions - 1 the policy, column `actions` the value
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
      for (int mt = 0; mt < T::MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t b = row0 + mt * 16 + 4 * lg + r;
          const float v = acc[mt][i][r];
          if (b < q.batch) {
            if (j < A) policy[b * q.policy_stride + j] = v;
            if (j == A) value[b * q.value_stride] = raw ? v : tanhf(v);
          }
        }
    }
  }
}

template <int TR>
__global__ __launch_bounds__(kWave * mlp_waves(TR)) void pvnet_kernel(const hk_pvnet_desc q) {
  pvnet_tile<TR>(q);
}

// hk_unified_pvnet_forward (include/hironaka_hip_unified.h): the same forward where *gate == want; otherwise every
// workgroup returns before it touches anything but the gate, and the outputs stay as they were.  The gate is uniform
// over the launch, so a workgroup either runs whole or not at all: no barrier is ever left half attended.
template <int TR>
__global__ __launch_bounds__(kWave * mlp_waves(TR)) void pvnet_gated_kernel(const hk_pvnet_desc q, const int32_t* gate,
                                                                            int32_t want) {
  if (*gate != want) return;
  pvnet_tile<TR>(q);
}

}  // namespace hk
