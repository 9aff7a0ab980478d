// Gaussian likelihood of P measurements with outliers (the user-side
// likelihood callable of reference sampler.py:863-873 for a model prediction
// m(theta) compared with data d where every measurement is either good or
// bad: the two-component mixture of Hogg, Bovy & Lang 2010), in one streaming
// kernel:
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
// the exponent of the absent component is.  sum_j e_hi joins a running sum;
// sum_j log B_j = log prod_j B_j as in nb_noise.hip: a lane multiplies the
// mantissas of its B into a running product and adds their exponents to an
// integer, every NB_OUTLIER_RENORM steps the product's own exponent moves to
// the integer as well, and at the end of a row a lane takes one log (po_log,
// nb_poisson_log.h) per product and adds exponent * ln 2.  v^-1/2 and u^-1/2
// are v_rsq_f64 with two Newton steps each; their squares serve as 1 / v and
// 1 / u.
//
// Layout, loads and the order of the sums are those of nb_noise_kernel, on
// the same table (d, sigma^2):
//  * L lanes share a row, a lane group walks R rows at once and U column
//    blocks of L per step, (L, R, U) a function of P alone; the values of the
//    next step are requested before the arithmetic of the current one;
//  * a lane group loads its rows' six coefficients once;
//  * row and column indices past the end are clamped to the last one and the
//    element masked: every load is in bounds without a branch;
//  * per lane R U partial sums and products; a row's U partials are added in
//    a fixed tree, then over its L lanes by shuffles.  No atomics, no row
//    split across workgroups: the bits of a row depend on neither n, the
//    row's place in the batch, ld, ld_mix, the stream nor the grid.
// A row with an m or a b that is not finite, a v or a u outside (0, +inf) or
// a p outside [0, 1] is NaN: a flag, OR-ed over the row, that overrides the
// sum; nothing relies on what inf - inf happens to be.
#include "../../include/nautilus_hip.h"          // NB_OUTLIER_WIDTH
#include "nb_common.h"
#include "nb_launch.h"
#include "nb_poisson_log.h"

namespace {

constexpr int NB_OUTLIER_RENORM = 256;           // steps between two frexp

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

// the coefficients of a row; w1 = 1 - p
struct ol_row {
  double c, a, f, w1, p, b, s;
};

// one element: e_hi; the mantissa and exponent of B; *bad is set where the
// element makes its row NaN
__device__ __forceinline__ double ol_term(double m, double d, double s2,
                                          const ol_row& k, double* mant,
                                          int* expo, bool* bad) {
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

// tab: d [P], sigma^2 [P].  model: n rows of n_data doubles, ld doubles
// apart.  mix: n rows of the 6 doubles (c, a, f, p, b, s), ld_mix doubles
// apart.
template <int L, int R, int U>
__global__ void __launch_bounds__(256)
nb_outlier_kernel(const double* __restrict__ tab, int n_data,
                  const double* __restrict__ model, long long ld,
                  const double* __restrict__ mix, long long ld_mix,
                  long long n, double log_norm, double* __restrict__ out) {
  static_assert(U == 1 || U == 2 || U == 4, "fixed tree over the partials");
  constexpr int G = 256 / L;                     // lane groups of a workgroup
  const int sub = threadIdx.x & (L - 1);
  const double* td = tab;
  const double* ts = tab + n_data;
  const long long stride = (long long)gridDim.x * G * R;
  for (long long p0 = ((long long)blockIdx.x * G + threadIdx.x / L) * R;
       p0 < n; p0 += stride) {
    // a row past the end of the batch is the last row again, never stored
    const double* row[R];
    ol_row k[R];
    unsigned flag[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long i = p0 + r < n ? p0 + r : n - 1;
      row[r] = model + i * ld;
      const double* w = mix + i * ld_mix;
      k[r].c = w[0];
      k[r].a = w[1];
      k[r].f = w[2];
      k[r].p = w[3];
      k[r].b = w[4];
      k[r].s = w[5];
      k[r].w1 = 1.0 - k[r].p;
      // false for NaN
      flag[r] = !(k[r].p >= 0.0 && k[r].p <= 1.0) ||
                        !(fabs(k[r].b) < __builtin_inf())
                    ? 1u
                    : 0u;
    }
    double acc[R][U], prod[R][U], next[R][U];
    int esum[R][U];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        acc[r][u] = 0.0;
        prod[r][u] = 1.0;
        esum[r][u] = 0;
        const int j = sub + L * u;               // a column past the end is
        const int jc = j < n_data ? j : n_data - 1;      // the last again
        next[r][u] = row[r][jc];
      }
    }
    int step = 0;
    for (int c = sub; c < n_data; c += L * U) {
      double m[R][U], d[U], s2[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = c + L * u;
        const int jc = j < n_data ? j : n_data - 1;
        d[u] = td[jc];
        s2[u] = ts[jc];
#pragma unroll
        for (int r = 0; r < R; ++r) m[r][u] = next[r][u];
      }
      if (c + L * U < n_data) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int j = c + L * U + L * u;
          const int jc = j < n_data ? j : n_data - 1;
#pragma unroll
          for (int r = 0; r < R; ++r) next[r][u] = row[r][jc];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool in = c + L * u < n_data;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          double mant;
          int expo;
          bool bad;
          const double e =
              ol_term(m[r][u], d[u], s2[u], k[r], &mant, &expo, &bad);
          acc[r][u] += in ? e : 0.0;
          prod[r][u] *= in ? mant : 1.0;
          esum[r][u] += in ? expo : 0;
          flag[r] |= in && bad ? 1u : 0u;
        }
      }
      // the same for every lane of the wavefront: c advances in step
      if (++step == NB_OUTLIER_RENORM) {
        step = 0;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int u = 0; u < U; ++u) {
            esum[r][u] += __builtin_amdgcn_frexp_exp(prod[r][u]);
            prod[r][u] = __builtin_amdgcn_frexp_mant(prod[r][u]);
          }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      // of a flagged row the products may be anything (0, NaN, inf): their
      // log is never looked at
      double t[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma clang fp contract(off)
        const double lg = fma((double)esum[r][u], 0x1.62e42fefa39efp-1,
                              po_log(prod[r][u]));
        t[u] = acc[r][u] + lg;
      }
      double v = t[0];
      if constexpr (U == 2) v = t[0] + t[1];
      if constexpr (U == 4) v = (t[0] + t[1]) + (t[2] + t[3]);
      unsigned f = flag[r];
#pragma unroll
      for (int s = 1; s < L; s <<= 1) {
        v += __shfl_xor(v, s);
        f |= (unsigned)__shfl_xor((int)f, s);
      }
      double res = log_norm + v;
      if (f) res = __builtin_nan("");
      if (sub == 0 && p0 + r < n) out[p0 + r] = res;
    }
  }
}

template <int L, int R, int U>
int launch(const double* tab, int n_data, const double* model, long long ld,
           const double* mix, long long ld_mix, long long n, double log_norm,
           double* out, hipStream_t stream) {
  constexpr long long rows = (256 / L) * R;      // of a workgroup per step
  long long b = (n + rows - 1) / rows;
  if (b > 8192) b = 8192;
  (void)hipGetLastError();
  hipLaunchKernelGGL((nb_outlier_kernel<L, R, U>), dim3((unsigned)b),
                     dim3(256), 0, stream, tab, n_data, model, ld, mix,
                     ld_mix, n, log_norm, out);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}

}  // namespace

// the shape is a function of P alone (a row's bits depend on it):
// device.outlier_launch_shape repeats it
int nb_launch_outlier(const double* tab, int n_data, const double* model,
                      long long ld, const double* mix, long long ld_mix,
                      long long n, double log_norm, double* out,
                      hipStream_t stream) {
  if (n <= 0) return NB_OK;
  if (n_data <= 32)
    return launch<16, 4, 1>(tab, n_data, model, ld, mix, ld_mix, n, log_norm,
                            out, stream);
  if (n_data <= 512)
    return launch<16, 2, 2>(tab, n_data, model, ld, mix, ld_mix, n, log_norm,
                            out, stream);
  return launch<64, 1, 4>(tab, n_data, model, ld, mix, ld_mix, n, log_norm,
                          out, stream);
}
