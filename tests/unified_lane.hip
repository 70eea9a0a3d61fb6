// The lane body of hk_unified_expand (hk_unified_kernel.h: unified_lane and unified_host_state), built for the host: a
// stand-alone program in the manner of tests/lane_routines.hip (no library, no device).  tests/test_unified_lane.py
// compiles it with AddressSanitizer and UndefinedBehaviorSanitizer and compares what it computes with
// tests/unified_rules.py, bit for bit.  For this translation unit alone `__device__` means host and device, and the
// intrinsics the routines use have host stand-ins below.
//
// Every game runs 2 x 4 times:
//   * two memory layouts.  "exact": par, chd, c and row are heap allocations of exactly m*d, m*d, d and d floats, so
//     that an overrun by one element lands in a redzone.  "production": three adjacent slices of search_lds_stride
//     floats built by LaneSlice, the game in the middle one; the neighbours and the stride's spare element hold a canary
//     that is checked after the routine returns;
//   * four fills of everything that is not an input: a quiet NaN, a large finite value, the pad -1 and 0.
// The results of all eight runs must be identical bit for bit; those of the first are written out.  A fill-dependent
// result or a touched canary is reported on stderr and makes the exit status 1; a sanitizer report aborts.
//
// usage: unified_lane CASES RESULTS
// CASES (binary, little-endian): char[4] "HKUL", int32 version (1), int32 blocks, then per block
//   int32 m, d, kind, reposition, scale, count;  float state[count][m*d + d];  int32 action[count]
// RESULTS: per block float next_state[count][m*d + d], float net_in[count][m*d + d], int32 subset[count],
//   float reward[count], int32 host_state[count] (unified_host_state of the parent's tail).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))

namespace host_standins {
inline int popc(unsigned x) { return __builtin_popcount(x); }
inline unsigned brev(unsigned x) { return __builtin_bitreverse32(x); }
inline int ffs(int x) { return __builtin_ffs(x); }
inline int clz(int x) { return x == 0 ? 32 : __builtin_clz((unsigned)x); }
inline unsigned umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
}  // namespace host_standins
#define __popc host_standins::popc
#define __brev host_standins::brev
#define __ffs host_standins::ffs
#define __clz host_standins::clz
#define __umulhi host_standins::umulhi

#include "hk_unified_kernel.h"

using namespace hk;

namespace {

int failures = 0;
void fail(int block, int game, int layout, int fill, const char* what) {
  if (++failures <= 20)
    fprintf(stderr, "FAILED block %d game %d layout %s fill %d: %s\n", block, game, layout ? "production" : "exact", fill, what);
}

float fill_value(int fill) {
  switch (fill) {
    case 0: return std::numeric_limits<float>::quiet_NaN();
    case 1: return 1e30f;
    case 2: return -1.0f;
  }
  return 0.0f;
}
constexpr float kCanary = -7654321.0f;

struct Frame {
  bool prod;
  int m, d, n, stride, used;
  std::vector<void*> owned;
  float *lds = nullptr, *par, *chd, *c, *row;

  float* take(size_t count) {
    void* p = malloc(count * sizeof(float) ? count * sizeof(float) : 1);
    owned.push_back(p);
    return static_cast<float*>(p);
  }
  Frame(int m_, int d_, bool production) : prod(production), m(m_), d(d_), n(m_ * d_) {
    stride = search_lds_stride(m, d);
    used = 2 * n + 2 * d;
    if (prod) {
      lds = take((size_t)3 * stride);
      const LaneSlice<float> s(lds, 1, stride, m, d);
      par = s.par, chd = s.chd, c = s.c, row = s.row;
    } else {
      par = take(n), chd = take(n), c = take(d), row = take(d);
    }
  }
  ~Frame() {
    for (void* p : owned) free(p);
  }
  Frame(const Frame&) = delete;
  LaneSlice<float> slice() const {
    LaneSlice<float> s(par, 0, stride, 0, 0);
    s.par = par, s.chd = chd, s.c = c, s.row = row;
    return s;
  }
  void reset(int fill) {
    const float fv = fill_value(fill);
    if (prod) {
      for (int e = 0; e < 3 * stride; ++e) lds[e] = kCanary;
      for (int e = 0; e < used; ++e) par[e] = fv;
    } else {
      for (int e = 0; e < n; ++e) par[e] = chd[e] = fv;
      for (int e = 0; e < d; ++e) c[e] = row[e] = fv;
    }
  }
  bool canaries_intact() const {
    if (!prod) return true;
    bool ok = true;
    for (int e = 0; e < 3 * stride; ++e)
      if (e < stride || e >= stride + used) ok &= memcmp(&lds[e], &kCanary, sizeof(float)) == 0;
    return ok;
  }
};

template <typename U>
std::vector<U> read_vec(FILE* fp, size_t count) {
  std::vector<U> v(count);
  if (count && fread(v.data(), sizeof(U), count, fp) != count) {
    fprintf(stderr, "short case file\n");
    exit(2);
  }
  return v;
}
template <typename U>
void write_vec(FILE* fp, const std::vector<U>& v) {
  if (!v.empty() && fwrite(v.data(), sizeof(U), v.size(), fp) != v.size()) {
    fprintf(stderr, "short write\n");
    exit(2);
  }
}

void run_block(int block, const int32_t* head, FILE* in, FILE* out) {
  const int m = head[0], d = head[1], kind = head[2], repos = head[3], scale = head[4], count = head[5];
  const int n = m * d, len = n + d;
  const std::vector<float> states = read_vec<float>(in, (size_t)count * len);
  const std::vector<int32_t> actions = read_vec<int32_t>(in, count);
  std::vector<float> next((size_t)count * len), net((size_t)count * len), reward(count), next2(len), net2(len);
  std::vector<int32_t> subset(count), host(count);
  Frame exact(m, d, false), production(m, d, true);
  for (int g = 0; g < count; ++g) {
    const float* st = states.data() + (size_t)g * len;
    for (int run = 0; run < 8; ++run) {
      const int layout = run >> 2, fill = run & 3;
      Frame& f = layout ? production : exact;
      f.reset(fill);
      for (int e = 0; e < n; ++e) f.chd[e] = st[e];
      for (int e = 0; e < d; ++e) f.c[e] = st[n + e];
      const bool is_host = unified_host_state(f.c, d);
      const UnifiedOutcome o = unified_lane(f.slice(), m, d, kind, actions[g], repos != 0, scale != 0);
      float* nx = run ? next2.data() : next.data() + (size_t)g * len;
      float* ni = run ? net2.data() : net.data() + (size_t)g * len;
      for (int e = 0; e < n; ++e) nx[e] = f.chd[e], ni[e] = f.par[e];
      for (int e = 0; e < d; ++e) nx[n + e] = ni[n + e] = f.c[e];
      if (!f.canaries_intact()) fail(block, g, layout, fill, "a canary outside the game's slice changed");
      if (!run) {
        subset[g] = (int32_t)o.subset, reward[g] = o.reward, host[g] = is_host;
      } else if (memcmp(nx, next.data() + (size_t)g * len, sizeof(float) * len) != 0 ||
                 memcmp(ni, net.data() + (size_t)g * len, sizeof(float) * len) != 0 || subset[g] != (int32_t)o.subset ||
                 memcmp(&reward[g], &o.reward, sizeof(float)) != 0 || host[g] != (int32_t)is_host) {
        fail(block, g, layout, fill, "the result differs from that of the exact layout under the NaN fill");
      }
    }
  }
  write_vec(out, next);
  write_vec(out, net);
  write_vec(out, subset);
  write_vec(out, reward);
  write_vec(out, host);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s CASES RESULTS\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) {
    fprintf(stderr, "cannot open the files\n");
    return 2;
  }
  char magic[4];
  int32_t head[2];
  if (fread(magic, 1, 4, in) != 4 || memcmp(magic, "HKUL", 4) != 0 || fread(head, 4, 2, in) != 2 || head[0] != 1) {
    fprintf(stderr, "not a case file of version 1\n");
    return 2;
  }
  for (int b = 0; b < head[1]; ++b) {
    int32_t h[6];
    if (fread(h, 4, 6, in) != 6) {
      fprintf(stderr, "short case file\n");
      return 2;
    }
    if (h[0] < 1 || h[0] > 1024 || h[1] < 2 || h[1] > kUnifiedMaxDim || h[5] < 0 || (h[2] | h[3] | h[4]) & ~1) {
      fprintf(stderr, "block %d: not a header\n", b);
      return 2;
    }
    run_block(b, h, in, out);
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  if (failures) fprintf(stderr, "%d failures\n", failures);
  return failures ? 1 : 0;
}
