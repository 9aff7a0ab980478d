// Gaussian likelihood of P measurements with outliers (the user-side
// likelihood callable of reference sampler.py:863-873 for a model prediction
// m(theta) compared with data d where every measurement is either good or
// bad: the two-component mixture of Hogg, Bovy & Lang 2010), as a term of the
// streaming kernel of nb_rowprod.h:
//     log L = log_norm + sum_j log[ (1 - p) v_j^-1/2 exp(e1_j)
//                                   +    p  u_j^-1/2 exp(e2_j) ],
//     v_j = c sigma_j^2 + a + f m_j^2,   e1_j = -(m_j - d_j)^2 / (2 v_j),
//     u_j = sigma_j^2 + s,               e2_j = -(d_j - b)^2 / (2 u_j),
// (c, a, f, p, b, s) per point.  Per element no log and one exp, of an
// argument that is never positive: with A1 = (1 - p) v^-1/2, A2 = p u^-1/2,
// "hi" the component with the larger exponent among those whose A is not zero
// and "lo" the other,
//     log q = e_hi + log B,   B = A_hi + A_lo exp(-(e_hi - e_lo)),
// all terms >= 0 and B >= A_hi > 0: nothing underflows however far out a
// measurement lies, and p = 0 or p = 1 give the one-component value whatever
// the exponent of the absent component is.  e_hi joins the kernel's sum and B
// its product.  v^-1/2 and u^-1/2 are v_rsq_f64 with two Newton steps each;
// their squares serve as 1 / v and 1 / u.
// A row with an m or a b that is not finite, a v or a u outside (0, +inf) or
// a p outside [0, 1] is NaN.
#include "../../include/nautilus_hip.h"          // NB_OUTLIER_WIDTH
#include "nb_rowprod.h"

namespace {

// x^-1/2 for x in (0, +inf): the estimate of v_rsq_f64 and two Newton steps
// y <- y + y (1/2 - (y / 2) (x y)), each of which squares the relative error
// (times 3/2); what is left after the second is the rounding of the last fma
// and the eps / 4 that the rounding of x y leaves in the correction
__device__ __forceinline__ double ol_rsqrt(double x) {
#pragma clang fp contract(off)
  double y = __builtin_amdgcn_rsq(x);
  y = fma(y, fma(-(0.5 * y), x * y, 0.5), y);
  y = fma(y, fma(-(0.5 * y), x * y, 0.5), y);
  return y;
}

// mix: n rows of the 6 doubles (c, a, f, p, b, s)
struct ol_term {
  static constexpr bool PER_ELEMENT = false;

  // the coefficients of a row; w1 = 1 - p
  struct row {
    double c, a, f, w1, p, b, s;
  };

  __device__ __forceinline__ static unsigned load(const double* w, row* k) {
    k->c = w[0];
    k->a = w[1];
    k->f = w[2];
    k->p = w[3];
    k->b = w[4];
    k->s = w[5];
    k->w1 = 1.0 - k->p;
    // false for NaN
    return !(k->p >= 0.0 && k->p <= 1.0) || !(fabs(k->b) < __builtin_inf())
               ? 1u
               : 0u;
  }

  // one element: e_hi; the mantissa and exponent of B; *bad is set where the
  // element makes its row NaN
  __device__ __forceinline__ static double term(double m, double, double d,
                                                double s2, const row& k,
                                                double* mant, int* expo,
                                                bool* bad) {
#pragma clang fp contract(off)
    const double r1 = m - d;
    const double r2 = d - k.b;
    const double v = fma(k.f, m * m, fma(k.c, s2, k.a));
    const double u = s2 + k.s;
    // false for NaN on either side
    *bad = !(fabs(m) < __builtin_inf()) || !(v > 0.0 && v < __builtin_inf()) ||
           !(u > 0.0 && u < __builtin_inf());
    const double yv = ol_rsqrt(v);
    const double yu = ol_rsqrt(u);
    const double e1 = -0.5 * ((r1 * r1) * (yv * yv));
    const double e2 = -0.5 * ((r2 * r2) * (yu * yu));
    const double a1 = k.w1 * yv;
    const double a2 = k.p * yu;
    // a component whose A is zero is absent, whatever its exponent (| and &:
    // three compares and no branch)
    const bool one = (a2 == 0.0) | ((a1 != 0.0) & (e1 >= e2));
    const double e_hi = one ? e1 : e2;
    const double e_lo = one ? e2 : e1;
    const double a_hi = one ? a1 : a2;
    const double a_lo = one ? a2 : a1;
    // e_lo > e_hi only beside a_lo = 0: the minimum keeps 0 * exp finite
    const double t = exp(fmin(e_lo - e_hi, 0.0));
    const double big_b = fma(a_lo, t, a_hi);
    *mant = __builtin_amdgcn_frexp_mant(big_b);
    *expo = __builtin_amdgcn_frexp_exp(big_b);
    return e_hi;
  }

  __device__ __forceinline__ static double result(double log_norm, double v) {
    return log_norm + v;
  }
};

}  // namespace

int nb_launch_outlier(const double* tab, int n_data, const double* model,
                      long long ld, const double* mix, long long ld_mix,
                      long long n, double log_norm, double* out,
                      hipStream_t stream) {
  if (n <= 0) return NB_OK;
  return nb_rowprod_launch<ol_term>(tab, n_data, model, ld, mix, ld_mix, n,
                                    log_norm, out, stream);
}
