// The lane body of hk_dqn_agent_move (hk_dqn_move_kernel.h: dqn_agent_lane) and the host's pick of hk_dqn_host_move
// (dqn_first_argmax), built for the host: a stand-alone program in the manner of tests/unified_lane.hip (no library, no
// device).  tests/test_dqn_move_lane.py compiles it with AddressSanitizer and UndefinedBehaviorSanitizer and compares
// what it computes with tests/dqn_move_rules.py, bit for bit.  For this translation unit alone `__device__` means host
// and device, and the intrinsics the routines use have host stand-ins below.
//
// Every game runs 2 x 4 times:
//   * two memory layouts.  "exact": par, chd, c, row and the game's Q-values are heap allocations of exactly m*d, m*d,
//     d, d and d elements, so that an overrun by one element lands in a redzone.  "production": three adjacent slices of
//     search_lds_stride elements built by LaneSlice, the game in the middle one; the neighbours and the stride's spare
//     element hold a canary that is checked after the routine returns;
//   * four fills of everything that is not an input: a quiet NaN, a large finite value, the pad -1 and 0.
// The results of all eight runs must be identical bit for bit; those of the first are written out.  A fill-dependent
// result or a touched canary is reported on stderr and makes the exit status 1; a sanitizer report aborts.
//
// usage: dqn_move_lane CASES RESULTS
// CASES (binary, little-endian): char[4] "HKDM", int32 version (1), int32 blocks, then per block
//   int32 m, d, dtype, q_dtype (0: float, 1: double), masked, rescale, count;  T points[count][m*d];  Q q[count][d];
//   int32 class_id[count];  Q host_q[count][2^d - d - 1]
// RESULTS: per block T next[count][m*d], T features[count][m*d], int32 axis[count], int32 done[count],
//   int32 prev_done[count], int32 host_class[count].
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

#include "hk_dqn_move_kernel.h"

using namespace hk;

namespace {

int failures = 0;
void fail(int block, int game, int layout, int fill, const char* what) {
  if (++failures <= 20)
    fprintf(stderr, "FAILED block %d game %d layout %s fill %d: %s\n", block, game, layout ? "production" : "exact", fill, what);
}

template <typename T>
T fill_value(int fill) {
  switch (fill) {
    case 0: return std::numeric_limits<T>::quiet_NaN();
    case 1: return (T)1e30;
    case 2: return (T)-1;
  }
  return (T)0;
}

template <typename T>
struct Frame {
  static constexpr T kCanary = (T)-7654321;
  bool prod;
  int m, d, n, stride, used;
  std::vector<void*> owned;
  T *lds = nullptr, *par, *chd, *c, *row;

  T* take(size_t count) {
    void* p = malloc(count * sizeof(T) ? count * sizeof(T) : 1);
    owned.push_back(p);
    return static_cast<T*>(p);
  }
  Frame(int m_, int d_, bool production) : prod(production), m(m_), d(d_), n(m_ * d_) {
    stride = search_lds_stride(m, d);
    used = 2 * n + 2 * d;
    if (prod) {
      lds = take((size_t)3 * stride);
      const LaneSlice<T> s(lds, 1, stride, m, d);
      par = s.par, chd = s.chd, c = s.c, row = s.row;
    } else {
      par = take(n), chd = take(n), c = take(d), row = take(d);
    }
  }
  ~Frame() {
    for (void* p : owned) free(p);
  }
  Frame(const Frame&) = delete;
  LaneSlice<T> slice() const {
    LaneSlice<T> s(par, 0, stride, 0, 0);
    s.par = par, s.chd = chd, s.c = c, s.row = row;
    return s;
  }
  void reset(int fill) {
    const T fv = fill_value<T>(fill);
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
    const T canary = kCanary;
    bool ok = true;
    for (int e = 0; e < 3 * stride; ++e)
      if (e < stride || e >= stride + used) ok &= memcmp(&lds[e], &canary, sizeof(T)) == 0;
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

template <typename T, typename Q>
void run_block(int block, const int32_t* head, FILE* in, FILE* out) {
  const int m = head[0], d = head[1], masked = head[4], rescale = head[5], count = head[6];
  const int n = m * d, classes = (1 << d) - d - 1;
  const std::vector<T> points = read_vec<T>(in, (size_t)count * n);
  const std::vector<Q> qs = read_vec<Q>(in, (size_t)count * d);
  const std::vector<int32_t> cls = read_vec<int32_t>(in, count);
  const std::vector<Q> host_q = read_vec<Q>(in, (size_t)count * classes);
  std::vector<T> next((size_t)count * n), feat((size_t)count * n), next2(n), feat2(n);
  std::vector<int32_t> axis(count), done(count), prev(count), host_cls(count);
  Frame<T> exact(m, d, false), production(m, d, true);
  for (int g = 0; g < count; ++g) {
    // the Q-values in allocations of their exact sizes: a read past either lands in a redzone
    Q* q = static_cast<Q*>(malloc(sizeof(Q) * d));
    Q* hq = static_cast<Q*>(malloc(sizeof(Q) * classes));
    memcpy(q, qs.data() + (size_t)g * d, sizeof(Q) * d);
    memcpy(hq, host_q.data() + (size_t)g * classes, sizeof(Q) * classes);
    host_cls[g] = dqn_first_argmax(hq, classes);
    for (int run = 0; run < 8; ++run) {
      const int layout = run >> 2, fill = run & 3;
      Frame<T>& f = layout ? production : exact;
      f.reset(fill);
      for (int e = 0; e < n; ++e) f.par[e] = points[(size_t)g * n + e];
      const DqnMoveOutcome o = dqn_agent_lane<T, Q>(f.slice(), q, m, d, cls[g], masked != 0, rescale != 0, (T)-1);
      T* nx = run ? next2.data() : next.data() + (size_t)g * n;
      T* ft = run ? feat2.data() : feat.data() + (size_t)g * n;
      for (int e = 0; e < n; ++e) nx[e] = f.par[e], ft[e] = f.chd[e];
      if (!f.canaries_intact()) fail(block, g, layout, fill, "a canary outside the game's slice changed");
      if (!run) {
        axis[g] = o.axis, done[g] = o.done, prev[g] = o.prev_done;
      } else if (memcmp(nx, next.data() + (size_t)g * n, sizeof(T) * n) != 0 ||
                 memcmp(ft, feat.data() + (size_t)g * n, sizeof(T) * n) != 0 || axis[g] != o.axis ||
                 done[g] != (int32_t)o.done || prev[g] != (int32_t)o.prev_done) {
        fail(block, g, layout, fill, "the result differs from that of the exact layout under the NaN fill");
      }
    }
    free(q);
    free(hq);
  }
  write_vec(out, next);
  write_vec(out, feat);
  write_vec(out, axis);
  write_vec(out, done);
  write_vec(out, prev);
  write_vec(out, host_cls);
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
  if (fread(magic, 1, 4, in) != 4 || memcmp(magic, "HKDM", 4) != 0 || fread(head, 4, 2, in) != 2 || head[0] != 1) {
    fprintf(stderr, "not a case file of version 1\n");
    return 2;
  }
  for (int b = 0; b < head[1]; ++b) {
    int32_t h[7];
    if (fread(h, 4, 7, in) != 7) {
      fprintf(stderr, "short case file\n");
      return 2;
    }
    if (h[0] < 1 || h[0] > 64 || h[1] < 2 || h[1] > kDqnMoveMaxDim || h[6] < 0 || (h[2] | h[3] | h[4] | h[5]) & ~1) {
      fprintf(stderr, "block %d: not a header\n", b);
      return 2;
    }
    if (h[2] == 0 && h[3] == 0) run_block<float, float>(b, h, in, out);
    else if (h[2] == 0) run_block<float, double>(b, h, in, out);
    else if (h[3] == 0) run_block<double, float>(b, h, in, out);
    else run_block<double, double>(b, h, in, out);
  }
  fclose(in);
  if (fclose(out) != 0) return 2;
  if (failures) fprintf(stderr, "%d failures\n", failures);
  return failures ? 1 : 0;
}
