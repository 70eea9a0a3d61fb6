// spivakovsky_game and random_spivakovsky_game (hk_spivakovsky.h) built for the host: a stand-alone program, no
// library and no device.  tests/test_spivakovsky_routines.py compiles it twice -- at -O3, and with AddressSanitizer and
// UndefinedBehaviorSanitizer -- and compares the masks with the plain-Python rules, bit for bit.  For this translation
// unit alone `__device__` means host and device, and the intrinsics the routines and hk_hosts.h use have host
// stand-ins below (tests/lane_routines.hip has the same five).
//
// Every game runs in allocations of its own: exactly m * d doubles for spivakovsky_game (the game widened, as the
// kernel stages it), exactly m * d elements of the dtype for random_spivakovsky_game.  An access past either end lands
// in a redzone of the sanitized build.
//
// usage: spivakovsky_routines CASES RESULTS
//
// CASES (binary, little-endian, no padding):
//   char[4] "HKSP", int32 version (1), int32 blocks, then per block
//     int32  dtype (0 float, 1 double), m, d, count
//     uint64 seed, game_offset;  uint32 step, 0    RandomSpivakovsky's draw: game g of the block is game_offset + g
//     T[count * m * d]                             the games
// RESULTS: per block int32[count] spivakovsky_game's masks, then int32[count] random_spivakovsky_game's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))

namespace host_standins {
inline int popc(unsigned x) { return __builtin_popcount(x); }
inline unsigned brev(unsigned x) { return __builtin_bitreverse32(x); }
inline int ffs(int x) { return __builtin_ffs(x); }
inline int clz(int x) { return x == 0 ? 32 : __builtin_clz((unsigned)x); }  // the hardware's value at 0
inline unsigned umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
}  // namespace host_standins
#define __popc host_standins::popc
#define __brev host_standins::brev
#define __ffs host_standins::ffs
#define __clz host_standins::clz
#define __umulhi host_standins::umulhi

#include "hk_spivakovsky.h"

using namespace hk;

namespace {

struct Header {
  int32_t dtype, m, d, count;
  uint64_t seed, game_offset;
  uint32_t step, zero;
};
static_assert(sizeof(Header) == 4 * 4 + 2 * 8 + 2 * 4, "the header is packed");

bool read_all(FILE* f, void* dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, f) == bytes; }

template <typename T>
bool run_block(const Header& h, FILE* in, FILE* out) {
  const size_t n = (size_t)h.m * h.d;
  std::vector<T> games(n * h.count);
  if (!read_all(in, games.data(), games.size() * sizeof(T))) return false;
  std::vector<int32_t> spiv(h.count), rnd(h.count);
  for (int g = 0; g < h.count; ++g) {
    const T* src = games.data() + n * g;
    double* w = static_cast<double*>(malloc(n * sizeof(double)));
    T* p = static_cast<T*>(malloc(n * sizeof(T)));
    if (!w || !p) return false;
    for (size_t e = 0; e < n; ++e) {
      w[e] = (double)src[e];
      p[e] = src[e];
    }
    spiv[g] = (int32_t)spivakovsky_game(w, h.m, h.d);
    rnd[g] = (int32_t)random_spivakovsky_game<T>(p, h.m, h.d, h.game_offset + (uint64_t)g, h.step, h.seed);
    free(w);
    free(p);
  }
  return fwrite(spiv.data(), 4, spiv.size(), out) == spiv.size() && fwrite(rnd.data(), 4, rnd.size(), out) == rnd.size();
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
    fprintf(stderr, "FAILED to open %s or %s\n", argv[1], argv[2]);
    return 2;
  }
  char magic[4];
  int32_t head[2];
  if (!read_all(in, magic, 4) || memcmp(magic, "HKSP", 4) != 0 || !read_all(in, head, 8) || head[0] != 1) {
    fprintf(stderr, "FAILED: not a case file of version 1\n");
    return 2;
  }
  for (int b = 0; b < head[1]; ++b) {
    Header h;
    if (!read_all(in, &h, sizeof(h)) || h.m < 1 || h.m > kFixedHostMaxPoints || h.d < 2 || h.d > kFixedHostMaxDim ||
        h.count < 0 || (h.dtype != 0 && h.dtype != 1)) {
      fprintf(stderr, "FAILED: block %d has a bad header\n", b);
      return 2;
    }
    if (!(h.dtype == 0 ? run_block<float>(h, in, out) : run_block<double>(h, in, out))) {
      fprintf(stderr, "FAILED: block %d is truncated or could not be written\n", b);
      return 2;
    }
  }
  fclose(in);
  return fclose(out) == 0 ? 0 : 2;
}
