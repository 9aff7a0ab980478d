// The float64 log of nb_poisson.hip, in a header of its own so that a host
// compiler can build the very same arithmetic (tests/test_poisson_log.py
// compiles it with -ffp-contract=off and compares it with long double).  On
// the host the mantissa / exponent split is std::frexp and the reciprocal
// estimate is a float division, as crude as v_rcp_f64; everything after them
// is shared.
#pragma once
#include <cmath>

#if defined(__HIP_DEVICE_COMPILE__)
#define NB_PO_INLINE __device__ __forceinline__
NB_PO_INLINE double po_frexp(double x, int* e) {
  *e = __builtin_amdgcn_frexp_exp(x);
  return __builtin_amdgcn_frexp_mant(x);
}
NB_PO_INLINE double po_rcp(double x) { return __builtin_amdgcn_rcp(x); }
#elif defined(__HIPCC__)
#define NB_PO_INLINE __device__ __forceinline__
NB_PO_INLINE double po_frexp(double x, int* e) { return frexp(x, e); }
NB_PO_INLINE double po_rcp(double x) { return 1.0 / x; }
#else
#define NB_PO_INLINE static inline
NB_PO_INLINE double po_frexp(double x, int* e) { return std::frexp(x, e); }
NB_PO_INLINE double po_rcp(double x) { return (double)(1.0f / (float)x); }
#endif

// log x for a positive finite x (subnormals included), 0.85 ulp measured
// against long double on the host (tests/test_poisson_log.py): x = 2^e m with
// m in [sqrt(1/2), sqrt(2)), f = m - 1, s = f / (2 + f), and with R = sum_i 2 / (2 i + 1) s^(2 i), i = 1
// .. 11 (the series of log((1 + s) / (1 - s)) - 2 s over s; the next term is
// below 2e-20 of the result),
//     log x = e ln2_hi - ((f^2 / 2 - (s (f^2 / 2 + R) + e ln2_lo)) - f);
// ln2_hi is log 2 cut to 32 bits, so e ln2_hi is exact.  A third of the
// instructions of the library's log, which also serves zero, negative and
// infinite arguments that po_term never passes on.
NB_PO_INLINE double po_log(double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  int e;
  double m = po_frexp(x, &e);                    // in [1/2, 1)
  const bool low = m < 0.70710678118654752;
  m = low ? m + m : m;
  e = low ? e - 1 : e;
  const double f = m - 1.0;                      // exact
  const double den = 2.0 + f;
  double r = po_rcp(den);
  r = fma(fma(-den, r, 1.0), r, r);
  r = fma(fma(-den, r, 1.0), r, r);
  double s = f * r;
  s = fma(fma(-den, s, f), r, s);
  const double z = s * s;
  double p = 2.0 / 23.0;
  p = fma(p, z, 2.0 / 21.0);
  p = fma(p, z, 2.0 / 19.0);
  p = fma(p, z, 2.0 / 17.0);
  p = fma(p, z, 2.0 / 15.0);
  p = fma(p, z, 2.0 / 13.0);
  p = fma(p, z, 2.0 / 11.0);
  p = fma(p, z, 2.0 / 9.0);
  p = fma(p, z, 2.0 / 7.0);
  p = fma(p, z, 2.0 / 5.0);
  p = fma(p, z, 2.0 / 3.0);
  const double big_r = p * z;
  const double hfsq = 0.5 * f * f;
  const double de = (double)e;
  const double ln2_hi = 0x1.62e42fee00000p-1, ln2_lo = 0x1.a39ef35793c76p-33;
  return fma(de, ln2_hi,
             -((hfsq - fma(s, hfsq + big_r, de * ln2_lo)) - f));
}
