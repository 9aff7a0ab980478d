// Gaussian likelihood of P measurements whose VARIANCE depends on the point
// (the user-side likelihood callable of reference sampler.py:863-873 for a
// model prediction m(theta) compared with data d under error bars that carry
// free parameters), in one streaming kernel:
//     log L = log_norm - 1/2 sum_j [ (m_j - d_j)^2 / v_j + log v_j ],
//     NB_NOISE_ROW   v_j = c sigma_j^2 + a + f m_j^2,  (c, a, f) per point,
//     NB_NOISE_FULL  v_j = sigma_j^2 + w_j,            w per element.
// The log v term depends on the point and stays; but no log is taken per
// element, because sum_j log v_j = log prod_j v_j: a lane multiplies the
// mantissas of its v (v_frexp_mant, in [1/2, 1)) into a running product and
// adds their exponents to an integer.  Every NB_NOISE_RENORM steps the
// product's own exponent moves to the integer as well (two more frexp, no
// log), so that it stays in (2^-(NB_NOISE_RENORM + 1), 1] for any row length
// and any finite positive v, subnormal ones included.  At the end of a row a
// lane takes one log (po_log, nb_poisson_log.h) per product and adds
// exponent * ln 2: 46 instructions per element in row mode and 49 in full
// mode where nb_poisson.hip spends about 100.
//
// Layout, loads and the order of the sums are those of nb_poisson_kernel:
//  * L lanes share a row, a lane group walks R rows at once and U column
//    blocks of L per step, (L, R, U) a function of P alone; the values of the
//    next step are requested before the arithmetic of the current one;
//  * the table (d, sigma^2: device memory, L2 resident) read once serves R
//    rows; in row mode a lane group loads its rows' (c, a, f) once;
//  * row and column indices past the end are clamped to the last one and the
//    element masked: every load is in bounds without a branch;
//  * per lane R U partial sums and products; a row's U partials are added in
//    a fixed tree, then over its L lanes by shuffles.  No atomics, no row
//    split across workgroups: the bits of a row depend on neither n, the
//    row's place in the batch, ld, ld_noise, the stream nor the grid.
// A row with an m that is not finite or a v outside (0, +inf) is NaN: a flag,
// OR-ed over the row, that overrides the sum; nothing relies on what inf -
// inf happens to be.
#include "../../include/nautilus_hip.h"          // NB_NOISE_ROW, NB_NOISE_FULL
#include "nb_common.h"
#include "nb_launch.h"
#include "nb_poisson_log.h"

namespace {

constexpr int NB_NOISE_RENORM = 256;             // steps between two frexp

// one element: the chi^2 term; the mantissa and exponent of v; *bad is set
// where the element makes its row NaN
template <int MODE>
__device__ __forceinline__ double no_term(double m, double w, double d,
                                          double s2, double c, double a,
                                          double f, double* mant, int* expo,
                                          bool* bad) {
#pragma clang fp contract(off)
  const double r = m - d;
  double v;
  if constexpr (MODE == NB_NOISE_ROW)
    v = fma(f, m * m, fma(c, s2, a));
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

// tab: d [P], sigma^2 [P].  model: n rows of n_data doubles, ld doubles
// apart.  noise: row mode n rows of 3 doubles (c, a, f), full mode n rows of
// n_data doubles, ld_noise doubles apart.
template <int MODE, int L, int R, int U>
__global__ void __launch_bounds__(256)
nb_noise_kernel(const double* __restrict__ tab, int n_data,
                const double* __restrict__ model, long long ld,
                const double* __restrict__ noise, long long ld_noise,
                long long n, double log_norm, double* __restrict__ out) {
  static_assert(U == 1 || U == 2 || U == 4, "fixed tree over the partials");
  constexpr bool FULL = MODE == NB_NOISE_FULL;
  constexpr int G = 256 / L;                     // lane groups of a workgroup
  const int sub = threadIdx.x & (L - 1);
  const double* td = tab;
  const double* ts = tab + n_data;
  const long long stride = (long long)gridDim.x * G * R;
  for (long long p0 = ((long long)blockIdx.x * G + threadIdx.x / L) * R;
       p0 < n; p0 += stride) {
    // a row past the end of the batch is the last row again, never stored
    const double* row[R];
    const double* wrow[R];
    double cc[R], ca[R], cf[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long i = p0 + r < n ? p0 + r : n - 1;
      row[r] = model + i * ld;
      wrow[r] = noise + i * ld_noise;
      cc[r] = ca[r] = cf[r] = 0.0;
      if constexpr (!FULL) {
        cc[r] = wrow[r][0];
        ca[r] = wrow[r][1];
        cf[r] = wrow[r][2];
      }
    }
    double acc[R][U], prod[R][U], next[R][U], wnext[R][U];
    int esum[R][U];
    unsigned flag[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      flag[r] = 0u;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        acc[r][u] = 0.0;
        prod[r][u] = 1.0;
        esum[r][u] = 0;
        const int j = sub + L * u;               // a column past the end is
        const int jc = j < n_data ? j : n_data - 1;      // the last again
        next[r][u] = row[r][jc];
        wnext[r][u] = 0.0;
        if constexpr (FULL) wnext[r][u] = wrow[r][jc];
      }
    }
    int step = 0;
    for (int c = sub; c < n_data; c += L * U) {
      double m[R][U], w[R][U], d[U], s2[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = c + L * u;
        const int jc = j < n_data ? j : n_data - 1;
        d[u] = td[jc];
        s2[u] = ts[jc];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          m[r][u] = next[r][u];
          w[r][u] = wnext[r][u];
        }
      }
      if (c + L * U < n_data) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int j = c + L * U + L * u;
          const int jc = j < n_data ? j : n_data - 1;
#pragma unroll
          for (int r = 0; r < R; ++r) {
            next[r][u] = row[r][jc];
            if constexpr (FULL) wnext[r][u] = wrow[r][jc];
          }
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
          const double q = no_term<MODE>(m[r][u], w[r][u], d[u], s2[u], cc[r],
                                         ca[r], cf[r], &mant, &expo, &bad);
          acc[r][u] += in ? q : 0.0;
          prod[r][u] *= in ? mant : 1.0;
          esum[r][u] += in ? expo : 0;
          flag[r] |= in && bad ? 1u : 0u;
        }
      }
      // the same for every lane of the wavefront: c advances in step
      if (++step == NB_NOISE_RENORM) {
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
      double res = log_norm - 0.5 * v;
      if (f) res = __builtin_nan("");
      if (sub == 0 && p0 + r < n) out[p0 + r] = res;
    }
  }
}

template <int MODE, int L, int R, int U>
int launch(const double* tab, int n_data, const double* model, long long ld,
           const double* noise, long long ld_noise, long long n,
           double log_norm, double* out, hipStream_t stream) {
  constexpr long long rows = (256 / L) * R;      // of a workgroup per step
  long long b = (n + rows - 1) / rows;
  if (b > 8192) b = 8192;
  (void)hipGetLastError();
  hipLaunchKernelGGL((nb_noise_kernel<MODE, L, R, U>), dim3((unsigned)b),
                     dim3(256), 0, stream, tab, n_data, model, ld, noise,
                     ld_noise, n, log_norm, out);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}

// the shape is a function of P alone (a row's bits depend on it), the one of
// nb_launch_poisson: short rows put their independent work into several rows
// per lane, long rows into column blocks of a whole wavefront
template <int MODE>
int launch_mode(const double* tab, int n_data, const double* model,
                long long ld, const double* noise, long long ld_noise,
                long long n, double log_norm, double* out,
                hipStream_t stream) {
  if (n_data <= 32)
    return launch<MODE, 16, 4, 1>(tab, n_data, model, ld, noise, ld_noise, n,
                                  log_norm, out, stream);
  if (n_data <= 512)
    return launch<MODE, 16, 2, 2>(tab, n_data, model, ld, noise, ld_noise, n,
                                  log_norm, out, stream);
  return launch<MODE, 64, 1, 4>(tab, n_data, model, ld, noise, ld_noise, n,
                                log_norm, out, stream);
}

}  // namespace

int nb_launch_noise(const double* tab, int n_data, int mode,
                    const double* model, long long ld, const double* noise,
                    long long ld_noise, long long n, double log_norm,
                    double* out, hipStream_t stream) {
  if (n <= 0) return NB_OK;
  if (mode == NB_NOISE_FULL)
    return launch_mode<NB_NOISE_FULL>(tab, n_data, model, ld, noise, ld_noise,
                                      n, log_norm, out, stream);
  return launch_mode<NB_NOISE_ROW>(tab, n_data, model, ld, noise, ld_noise, n,
                                   log_norm, out, stream);
}
