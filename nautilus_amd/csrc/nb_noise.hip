// Gaussian likelihood of P measurements whose VARIANCE depends on the point
// (the user-side likelihood callable of reference sampler.py:863-873 for a
// model prediction m(theta) compared with data d under error bars that carry
// free parameters), as a term of the streaming kernel of nb_rowprod.h:
//     log L = log_norm - 1/2 sum_j [ (m_j - d_j)^2 / v_j + log v_j ],
//     NB_NOISE_ROW   v_j = c sigma_j^2 + a + f m_j^2,  (c, a, f) per point,
//     NB_NOISE_FULL  v_j = sigma_j^2 + w_j,            w per element.
// The log v term depends on the point and stays; but no log is taken per
// element: the chi^2 term joins the kernel's sum and v its product, 46
// instructions per element in row mode and 49 in full mode where
// nb_poisson.hip spends about 100.
// A row with an m that is not finite or a v outside (0, +inf) is NaN.
#include "../../include/nautilus_hip.h"          // NB_NOISE_ROW, NB_NOISE_FULL
#include "nb_rowprod.h"

namespace {

// noise: row mode n rows of 3 doubles (c, a, f), full mode n rows of n_data
// doubles
template <int MODE>
struct no_term {
  static constexpr bool PER_ELEMENT = MODE == NB_NOISE_FULL;

  struct row {
    double c, a, f;
  };

  __device__ __forceinline__ static unsigned load(const double* w, row* k) {
    if constexpr (PER_ELEMENT) {
      k->c = k->a = k->f = 0.0;
    } else {
      k->c = w[0];
      k->a = w[1];
      k->f = w[2];
    }
    return 0u;
  }

  // one element: the chi^2 term; the mantissa and exponent of v; *bad is set
  // where the element makes its row NaN
  __device__ __forceinline__ static double term(double m, double w, double d,
                                                double s2, const row& k,
                                                double* mant, int* expo,
                                                bool* bad) {
#pragma clang fp contract(off)
    const double r = m - d;
    double v;
    if constexpr (MODE == NB_NOISE_ROW)
      v = fma(k.f, m * m, fma(k.c, s2, k.a));
    else
      v = s2 + w;
    // false for NaN on either side
    *bad = !(fabs(m) < __builtin_inf()) || !(v > 0.0 && v < __builtin_inf());
    *mant = __builtin_amdgcn_frexp_mant(v);
    *expo = __builtin_amdgcn_frexp_exp(v);
    double iv = __builtin_amdgcn_rcp(v);
    iv = fma(fma(-v, iv, 1.0), iv, iv);
    iv = fma(fma(-v, iv, 1.0), iv, iv);
    return (r * r) * iv;
  }

  __device__ __forceinline__ static double result(double log_norm, double v) {
    return log_norm - 0.5 * v;
  }
};

}  // namespace

int nb_launch_noise(const double* tab, int n_data, int mode,
                    const double* model, long long ld, const double* noise,
                    long long ld_noise, long long n, double log_norm,
                    double* out, hipStream_t stream) {
  if (n <= 0) return NB_OK;
  if (mode == NB_NOISE_FULL)
    return nb_rowprod_launch<no_term<NB_NOISE_FULL>>(
        tab, n_data, model, ld, noise, ld_noise, n, log_norm, out, stream);
  return nb_rowprod_launch<no_term<NB_NOISE_ROW>>(
      tab, n_data, model, ld, noise, ld_noise, n, log_norm, out, stream);
}
