// Host model of the Box-Muller arithmetic of the proposal draw
// (nautilus_amd/csrc/nb_draw.h, the very header the kernels include) against
// long double: prints, for draw_log, the sine and the cosine of draw_sincos
// and the pair of draw_normal_pair, the largest error and the word it occurs
// at, and the number of results that are not finite or out of range.  The
// words: the corner words of tests/draw_words.py (written out again here) and
// argv[1] random ones.  Run by tests/test_draw_words.py.
//
// A model: the three AMD builtins have stand-ins (the reciprocal estimate is a
// float-rounded 1 / b, not the hardware's table), and the host compiler
// contracts nothing.  The verdict on the device is tests/test_draw_words_gpu.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#define NB_DRAW_HOST_MODEL
#define __device__
#define __forceinline__ inline
static inline double model_rcp(double b) { return (double)(float)(1.0 / b); }
static inline double model_frexp_mant(double x) { int e; return std::frexp(x, &e); }
static inline int model_frexp_exp(double x) { int e; std::frexp(x, &e); return e; }
#define __builtin_amdgcn_rcp model_rcp
#define __builtin_amdgcn_frexp_mant model_frexp_mant
#define __builtin_amdgcn_frexp_exp model_frexp_exp
static inline double nb_unit32(uint32_t w) {      // nb_common.h
  return ((double)w + 0.5) * (1.0 / 4294967296.0);
}
#include "nb_draw.h"

namespace {

struct Worst {
  double err = 0.0;
  uint32_t w0 = 0, w1 = 0;
  long bad = 0;
  void take(double e, uint32_t a, uint32_t b) {
    if (!(e <= err)) err = e, w0 = a, w1 = b;
  }
};

double ulps(double got, long double t) {
  const double ulp = std::ldexp(1.0, std::ilogb((double)t) - 52);
  return std::fabs((double)(((long double)got - t) / ulp));
}

const long double HALF_PI = 1.57079632679489661923132169163975144L;

// sin(2 pi u), cos(2 pi u) with the exact remainder of 4 u
void exact_sincos(double u, long double& sn, long double& cs) {
  const double a = 4.0 * u, q = std::nearbyint(a);
  const long double y = (long double)(a - q) * HALF_PI;
  const long double s = sinl(y), c = cosl(y);
  switch ((int)q & 3) {
    case 0: sn = s, cs = c; break;
    case 1: sn = c, cs = -s; break;
    case 2: sn = -s, cs = -c; break;
    default: sn = -c, cs = s; break;
  }
}

}  // namespace

int main(int argc, char** argv) {
  const long count = argc > 1 ? std::atol(argv[1]) : 2000000;
  std::vector<uint32_t> words;
  auto add = [&](long long w) {
    if (w >= 0 && w <= 0xffffffffLL) words.push_back((uint32_t)w);
  };
  for (long long k = 0; k < 4096; ++k) {
    add(k), add(0xffffffffLL - k);
    for (long long q = 1; q <= 7; ++q)
      add((q << 29) + k), add((q << 29) - 1 - k);
  }
  for (int k = 0; k < 32; ++k) {
    add(1LL << k), add((1LL << k) - 1);
    const long long c = (long long)std::floor(std::ldexp(std::sqrt(0.5), 32 - k));
    for (long long j = -63; j <= 64; ++j) add(c + j);
  }
  add(0x75c646d6LL), add(0xca33c991LL);
  std::sort(words.begin(), words.end());
  words.erase(std::unique(words.begin(), words.end()), words.end());
  const size_t corners = words.size();

  Worst lg, sn, cs, zz;
  auto test = [&](uint32_t w0, uint32_t w1) {
    const double u0 = nb_unit32(w0), u1 = nb_unit32(w1);
    const long double tl = logl((long double)u0);
    const double l = draw_log(u0);
    if (!(std::isfinite(l) && l < 0.0)) ++lg.bad;
    lg.take(ulps(l, tl), w0, w1);
    long double ts, tc;
    exact_sincos(u1, ts, tc);
    double s, c;
    draw_sincos(u1, s, c);
    if (!(std::fabs(s) <= 1.0)) ++sn.bad;
    if (!(std::fabs(c) <= 1.0)) ++cs.bad;
    sn.take(ulps(s, ts), w1, w0);
    cs.take(ulps(c, tc), w1, w0);
    double z0, z1;
    draw_normal_pair(w0, w1, z0, z1);
    const long double r = sqrtl(-2.0L * tl);
    if (!(std::isfinite(z0) && std::isfinite(z1))) ++zz.bad;
    // relative error in units of 2^-53
    zz.take(std::fabs((double)(((long double)z0 - r * tc) / (r * tc))) *
                9007199254740992.0, w0, w1);
    zz.take(std::fabs((double)(((long double)z1 - r * ts) / (r * ts))) *
                9007199254740992.0, w0, w1);
  };
  // every corner word in both places, paired with a corner word far from it
  for (size_t i = 0; i < corners; ++i)
    test(words[i], words[(i + corners / 2 + 1) % corners]);
  std::mt19937_64 g(1);
  for (long i = 0; i < count; ++i) {
    const uint64_t r = g();
    test((uint32_t)r, (uint32_t)(r >> 32));
  }
  std::printf("log %.6f 0x%08x %ld\n", lg.err, lg.w0, lg.bad);
  std::printf("sin %.6f 0x%08x %ld\n", sn.err, sn.w0, sn.bad);
  std::printf("cos %.6f 0x%08x %ld\n", cs.err, cs.w0, cs.bad);
  std::printf("pair %.6f 0x%08x,0x%08x %ld\n", zz.err, zz.w0, zz.w1, zz.bad);
  std::printf("corners %zu\n", corners);
  return 0;
}
