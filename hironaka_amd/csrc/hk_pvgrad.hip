// C ABI of hk_pvgrad_forward / hk_pvgrad_backward (include/hironaka_hip_pvgrad.h, an addition within ABI 6): argument
// validation, the workspace's layout and the launches of hk::pvgrad_forward_kernel, hk::pvgrad_rows_kernel and
// hk::pvgrad_params_kernel.  No allocation on the device, no synchronisation; every status is decided before the first
// launch.  The descriptor is read here, on the host: each launch gets its own argument.
#include <utility>
#include <vector>

#include "hk_pvgrad_kernel.h"

using namespace hk;

namespace {

using Ranges = std::vector<std::pair<const void*, uint64_t>>;

// the Denses a block of its kind uses, with their gradients
int denses(const hk_pvnet_block& B, const hk_pvgrad_block& G, const hk_pvnet_dense* (&d)[3], const hk_pvgrad_dense* (&g)[3]) {
  d[0] = &B.dense1, g[0] = &G.dense1;
  if (B.kind == HK_PVNET_DENSE) return 1;
  d[1] = &B.dense2, g[1] = &G.dense2;
  if (B.k == B.n) return 2;
  d[2] = &B.proj, g[2] = &G.proj;
  return 3;
}

// the sizes alone: what the layout needs to be meaningful
bool sizes_ok(const hk_pvnet_desc& q) {
  if (q.nblocks < 1 || q.nblocks > HK_PVNET_MAX_BLOCKS || q.batch <= 0 || q.actions < 1 || q.actions > HK_PVNET_MAX_WIDTH - 1)
    return false;
  for (int l = 0; l < q.nblocks; ++l)
    if (q.block[l].n < 1 || q.block[l].n > HK_PVNET_MAX_WIDTH) return false;
  return true;
}

uint64_t workspace_floats(const hk_pvnet_desc& q) {
  uint64_t floats = 0;
  for (int l = 0; l < q.nblocks; ++l) floats += (uint64_t)pvgrad_slots(q.block[l]) * (uint64_t)q.batch * (uint64_t)q.block[l].n;
  return floats + (uint64_t)q.batch * (uint64_t)(q.actions + 1);
}

int validate(const hk_pvgrad_desc* g, bool backward) {
  if (!g) return HK_ERR_NULL;
  const hk_pvnet_desc& q = g->net;
  {
    // everything hk_pvnet_forward refuses, by asking it: without rows it launches nothing
    hk_pvnet_desc probe = q;
    if (probe.batch > 0) probe.batch = 0;
    if (const int bad = hk_pvnet_forward(&probe, nullptr)) return bad;
  }
  if (q.flags & (HK_PVNET_FORCE_TILE_SMALL | HK_PVNET_FORCE_TILE_LARGE)) return HK_ERR_UNSUPPORTED;
  if (q.batch > HK_PVGRAD_MAX_BATCH) return HK_ERR_SHAPE;
  if (backward && (g->grad_policy_stride < q.actions || g->grad_value_stride < 1)) return HK_ERR_SHAPE;
  const uint64_t ws_bytes = q.batch > 0 ? workspace_floats(q) * sizeof(float) : 0;
  if (g->workspace_bytes < ws_bytes) return HK_ERR_SHAPE;
  if (!g->workspace) return HK_ERR_NULL;
  const hk_pvnet_dense* d[3];
  const hk_pvgrad_dense* dg[3];
  if (backward) {
    if (!g->grad_policy || !g->grad_value || !g->policy.d_weight || !g->value.d_weight) return HK_ERR_NULL;
    for (int l = 0; l < q.nblocks; ++l)
      for (int i = 0, n = denses(q.block[l], g->block[l], d, dg); i < n; ++i)
        if (!dg[i]->d_weight) return HK_ERR_NULL;
  }
  if (!aligned(g->workspace, 4)) return HK_ERR_ALIGN;
  if (backward) {
    if (!all_aligned({g->grad_policy, g->grad_value, g->policy.d_weight, g->policy.d_bias, g->value.d_weight, g->value.d_bias}, 4))
      return HK_ERR_ALIGN;
    for (int l = 0; l < q.nblocks; ++l)
      for (int i = 0, n = denses(q.block[l], g->block[l], d, dg); i < n; ++i)
        if (!all_aligned({dg[i]->d_weight, dg[i]->d_bias, dg[i]->d_gn_scale, dg[i]->d_gn_bias}, 4)) return HK_ERR_ALIGN;
  }
  if (q.batch == 0) return HK_OK;

  // what is read and what is written
  Ranges rd, wr;
  const uint64_t x_bytes = span_bytes(q.batch, q.x_stride, q.k0, sizeof(float));
  const uint64_t policy_bytes = span_bytes(q.batch, q.policy_stride, q.actions, sizeof(float));
  const uint64_t value_bytes = span_bytes(q.batch, q.value_stride, 1, sizeof(float));
  const uint64_t gp_bytes = backward ? span_bytes(q.batch, g->grad_policy_stride, q.actions, sizeof(float)) : 1;
  const uint64_t gv_bytes = backward ? span_bytes(q.batch, g->grad_value_stride, 1, sizeof(float)) : 1;
  if (!x_bytes || !policy_bytes || !value_bytes || !gp_bytes || !gv_bytes) return HK_ERR_SHAPE;  // beyond 2^63 bytes
  const uint64_t last = (uint64_t)q.block[q.nblocks - 1].n * sizeof(float);
  rd.emplace_back(q.x, x_bytes);
  rd.emplace_back(q.policy_weight, last * (uint64_t)q.actions);
  rd.emplace_back(q.value_weight, last);
  rd.emplace_back(q.policy_bias, (uint64_t)q.actions * sizeof(float));
  rd.emplace_back(q.value_bias, sizeof(float));
  wr.emplace_back(g->workspace, ws_bytes);
  if (backward) {
    rd.emplace_back(q.value, value_bytes);
    rd.emplace_back(g->grad_policy, gp_bytes);
    rd.emplace_back(g->grad_value, gv_bytes);
    wr.emplace_back(g->policy.d_weight, last * (uint64_t)q.actions);
    wr.emplace_back(g->policy.d_bias, (uint64_t)q.actions * sizeof(float));
    wr.emplace_back(g->value.d_weight, last);
    wr.emplace_back(g->value.d_bias, sizeof(float));
  } else {
    wr.emplace_back(q.policy, policy_bytes);
    wr.emplace_back(q.value, value_bytes);
  }
  for (int l = 0; l < q.nblocks; ++l) {
    const hk_pvnet_block& B = q.block[l];
    const uint64_t vec = (uint64_t)B.n * sizeof(float);
    for (int i = 0, n = denses(B, g->block[l], d, dg); i < n; ++i) {
      const uint64_t mat = vec * (uint64_t)(i == 1 ? B.n : B.k);  // dense2 is [n, n]
      const bool normed = B.kind == HK_PVNET_RESIDUE;
      rd.emplace_back(d[i]->weight, mat);
      rd.emplace_back(d[i]->bias, vec);
      if (normed) rd.emplace_back(d[i]->gn_scale, vec), rd.emplace_back(d[i]->gn_bias, vec);
      if (backward) {
        wr.emplace_back(dg[i]->d_weight, mat);
        wr.emplace_back(dg[i]->d_bias, vec);
        if (normed) wr.emplace_back(dg[i]->d_gn_scale, vec), wr.emplace_back(dg[i]->d_gn_bias, vec);
      }
    }
  }
  for (size_t i = 0; i < wr.size(); ++i) {
    for (const auto& r : rd)
      if (overlap(wr[i].first, wr[i].second, r.first, r.second)) return HK_ERR_UNSUPPORTED;
    for (size_t j = i + 1; j < wr.size(); ++j)
      if (overlap(wr[i].first, wr[i].second, wr[j].first, wr[j].second)) return HK_ERR_UNSUPPORTED;
  }
  return HK_OK;
}

const dim3 kRowBlock(kWave * mlp_waves(kPvgradTile));

int forward(const hk_pvgrad_desc* g, hipStream_t stream) {
  const int bad = validate(g, false);
  if (bad != HK_OK) return bad;
  if (g->net.batch == 0) return HK_OK;
  PvgradForwardArgs a;
  a.q = g->net;
  a.ws = static_cast<float*>(g->workspace);
  return launch_kernel_lds(pvgrad_forward_kernel, 48 * 1024, dim3((unsigned)workgroups(a.q.batch, kPvgradTile)), kRowBlock,
                           mlp_lds_bytes(kPvgradTile), stream, a);
}

int backward(const hk_pvgrad_desc* g, hipStream_t stream) {
  const int bad = validate(g, true);
  if (bad != HK_OK) return bad;
  const hk_pvnet_desc& q = g->net;
  if (q.batch == 0) return HK_OK;
  float* const ws = static_cast<float*>(g->workspace);
  {
    PvgradRowsArgs a;
    a.q = q;
    a.ws = ws;
    a.grad_policy = static_cast<const float*>(g->grad_policy), a.grad_value = static_cast<const float*>(g->grad_value);
    a.grad_policy_stride = g->grad_policy_stride, a.grad_value_stride = g->grad_value_stride;
    const int status = launch_kernel_lds(pvgrad_rows_kernel, 48 * 1024, dim3((unsigned)workgroups(q.batch, kPvgradTile)),
                                         kRowBlock, mlp_lds_bytes(kPvgradTile), stream, a);
    if (status != HK_OK) return status;
  }
  // the table of every Dense in use, then a launch per HK_PVGRAD_TABLE of them
  std::vector<PvgradParam> table;
  const int64_t batch = q.batch;
  auto F = [](void* p) { return static_cast<float*>(p); };
  auto add = [&](const float* dz, int dz_stride, const float* a_in, int64_t a_stride, const float* ge, const float* gx,
                 const hk_pvgrad_dense& G, bool normed, int n, int k) {
    PvgradParam p = {};
    p.dz = dz, p.a_in = a_in, p.ge = ge, p.gx = gx;
    p.d_weight = F(G.d_weight), p.d_bias = F(G.d_bias);
    p.d_gn_scale = normed ? F(G.d_gn_scale) : nullptr, p.d_gn_bias = normed ? F(G.d_gn_bias) : nullptr;
    p.a_stride = a_stride, p.dz_stride = dz_stride, p.n = n, p.k = k;
    table.push_back(p);
  };
  const float* h = static_cast<const float*>(q.x);  // the block's input and its row stride
  int64_t h_stride = q.x_stride;
  float* base = ws;
  for (int l = 0; l < q.nblocks; ++l) {
    const hk_pvnet_block& B = q.block[l];
    const hk_pvgrad_block& G = g->block[l];
    const int64_t sz = batch * B.n;
    auto at = [&](int slot) { return base + slot * sz; };
    if (B.kind == HK_PVNET_DENSE) {
      add(at(kPgDenseDz1), B.n, h, h_stride, nullptr, nullptr, G.dense1, false, B.n, B.k);
      h = at(kPgDenseH);
    } else {
      add(at(kPgDz1), B.n, h, h_stride, at(kPgDa), at(kPgGx1), G.dense1, true, B.n, B.k);
      add(at(kPgDz2), B.n, at(kPgA), B.n, at(kPgE), at(kPgGx2), G.dense2, true, B.n, B.n);
      if (B.k != B.n) add(at(kPgDzp), B.n, h, h_stride, at(kPgE), at(kPgGxp), G.proj, true, B.n, B.k);
      h = at(kPgH);
    }
    h_stride = B.n;
    base += pvgrad_slots(B) * sz;
  }
  const int A = q.actions, last = q.block[q.nblocks - 1].n;
  add(base, A + 1, h, h_stride, nullptr, nullptr, g->policy, false, A, last);
  add(base + A, A + 1, h, h_stride, nullptr, nullptr, g->value, false, 1, last);
  for (size_t first = 0; first < table.size(); first += HK_PVGRAD_TABLE) {
    PvgradParamsArgs a = {};
    a.batch = q.batch;
    int tiles = 0;
    for (size_t i = first; i < table.size() && i < first + HK_PVGRAD_TABLE; ++i) {
      PvgradParam& p = a.t[a.count++] = table[i];
      p.tile0 = tiles;
      tiles += ((p.n + 15) >> 4) * ((p.k + 15) >> 4);
    }
    const int status = launch_kernel(pvgrad_params_kernel, dim3((unsigned)tiles), dim3(kPvgradParamThreads), 0, stream, a);
    if (status != HK_OK) return status;
  }
  return HK_OK;
}

}  // namespace

extern "C" {

uint64_t hk_pvgrad_workspace_bytes(const hk_pvgrad_desc* g) {
  return g && sizes_ok(g->net) ? workspace_floats(g->net) * sizeof(float) : 0;
}

int hk_pvgrad_forward(const hk_pvgrad_desc* g, void* stream) { return forward(g, (hipStream_t)stream); }

int hk_pvgrad_backward(const hk_pvgrad_desc* g, void* stream) { return backward(g, (hipStream_t)stream); }

}  // extern "C"
