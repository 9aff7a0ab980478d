// One term of the Poisson deviance, shared by the streaming kernel
// (nb_poisson.hip) and the folding one (nb_fold.hip): device code only -- the
// log it calls, nb_poisson_log.h, is the part a host compiler builds too.
#pragma once
#include "nb_poisson_log.h"

namespace {

constexpr unsigned PO_NAN = 1u, PO_NEG_INF = 2u;

// D(mu, k) of one element; *flag collects PO_NAN / PO_NEG_INF
__device__ __forceinline__ double po_term(double m, double k, double ik,
                                          double e, double b, unsigned* flag) {
#pragma clang fp contract(off)
  const double mu = e * m + b;
  const bool fin = mu >= 0.0 && mu < __builtin_inf();   // false for NaN
  const bool pos = k > 0.0;
  const bool zero = mu == 0.0;
  *flag |= (fin ? 0u : PO_NAN) | (zero && pos ? PO_NEG_INF : 0u);
  // k = 0 has 1 / k = 0 in the table, so t = 0 and d = 0 there; what a
  // flagged element computes is never looked at (the flag overrides the row)
  const double t = (mu - k) * ik;
  const bool small = fabs(t) < 0.5;
  const double hi = 1.0 + t;
  const double arg = small ? hi : mu * ik;
  double r = __builtin_amdgcn_rcp(hi);
  r = fma(fma(-hi, r, 1.0), r, r);
  const double corr = small ? (t - (hi - 1.0)) * r : 0.0;
  const double lg = po_log(arg) + corr;
  const double d = k * (t - lg);
  return pos ? d : mu;
}

}  // namespace
