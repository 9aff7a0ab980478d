// The streaming kernel of the likelihoods that add, per row, a running sum
// and the log of a running product over the table (d, sigma^2): nb_noise.hip
// and nb_outlier.hip supply the arithmetic as a term type T,
//     T::row                         the coefficients of a row,
//     T::load(w, &k)                 reads them from the row's auxiliary
//                                    input; a result that is not zero makes
//                                    the row NaN,
//     T::PER_ELEMENT                 the auxiliary input also holds a value w
//                                    per element, laid out like the model,
//     T::term(m, w, d, s2, k, &mant, &expo, &bad)
//                                    one element: what joins the sum; the
//                                    mantissa and exponent of what joins the
//                                    product; *bad where the element makes its
//                                    row NaN,
//     T::result(log_norm, v)         of v = sum + log product.
// No log is taken per element, because sum_j log x_j = log prod_j x_j: a lane
// multiplies the mantissas (v_frexp_mant, in [1/2, 1)) into a running product
// and adds the exponents to an integer.  Every NB_ROWPROD_RENORM steps the
// product's own exponent moves to the integer as well (two more frexp, no
// log), so that it stays in (2^-(NB_ROWPROD_RENORM + 1), 1] for any row
// length and any finite positive factor, subnormal ones included.  At the end
// of a row a lane takes one log (po_log, nb_poisson_log.h) per product and
// adds exponent * ln 2.
//
// Layout, loads and the order of the sums are those of nb_poisson_kernel:
//  * L lanes share a row, a lane group walks R rows at once and U column
//    blocks of L per step, (L, R, U) a function of P alone
//    (nb_stream_dispatch, nb_launch.h); the values of the next step are
//    requested before the arithmetic of the current one;
//  * the table (d, sigma^2: device memory, L2 resident) read once serves R
//    rows; a lane group loads its rows' coefficients once;
//  * row and column indices past the end are clamped to the last one and the
//    element masked: every load is in bounds without a branch;
//  * per lane R U partial sums and products; a row's U partials are added in
//    a fixed tree, then over its L lanes by shuffles.  No atomics, no row
//    split across workgroups: the bits of a row depend on neither n, the
//    row's place in the batch, ld, ld_aux, the stream nor the grid.
// A flag, OR-ed over the row, overrides the sum with NaN; nothing relies on
// what inf - inf happens to be.
#pragma once

#include "nb_common.h"
#include "nb_launch.h"
#include "nb_poisson_log.h"

constexpr int NB_ROWPROD_RENORM = 256;           // steps between two frexp

// tab: d [P], sigma^2 [P].  model: n rows of n_data doubles, ld doubles
// apart.  aux: n rows of what T::load and, with PER_ELEMENT, T::term read,
// ld_aux doubles apart.
template <class T, int L, int R, int U>
__global__ void __launch_bounds__(256)
nb_rowprod_kernel(const double* __restrict__ tab, int n_data,
                  const double* __restrict__ model, long long ld,
                  const double* __restrict__ aux, long long ld_aux,
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
    const double* wrow[R];
    typename T::row k[R];
    double acc[R][U], prod[R][U], next[R][U], wnext[R][U];
    int esum[R][U];
    unsigned flag[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long i = p0 + r < n ? p0 + r : n - 1;
      row[r] = model + i * ld;
      wrow[r] = aux + i * ld_aux;
      flag[r] = T::load(wrow[r], &k[r]);
    }
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
        wnext[r][u] = 0.0;
        if constexpr (T::PER_ELEMENT) wnext[r][u] = wrow[r][jc];
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
            if constexpr (T::PER_ELEMENT) wnext[r][u] = wrow[r][jc];
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
          const double q = T::term(m[r][u], w[r][u], d[u], s2[u], k[r], &mant,
                                   &expo, &bad);
          acc[r][u] += in ? q : 0.0;
          prod[r][u] *= in ? mant : 1.0;
          esum[r][u] += in ? expo : 0;
          flag[r] |= in && bad ? 1u : 0u;
        }
      }
      // the same for every lane of the wavefront: c advances in step
      if (++step == NB_ROWPROD_RENORM) {
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
      double res = T::result(log_norm, v);
      if (f) res = __builtin_nan("");
      if (sub == 0 && p0 + r < n) out[p0 + r] = res;
    }
  }
}

template <class T>
int nb_rowprod_launch(const double* tab, int n_data, const double* model,
                      long long ld, const double* aux, long long ld_aux,
                      long long n, double log_norm, double* out,
                      hipStream_t stream) {
  return nb_stream_dispatch(n_data, [&](auto s) {
    using S = decltype(s);
    (void)hipGetLastError();
    hipLaunchKernelGGL((nb_rowprod_kernel<T, S::L, S::R, S::U>),
                       dim3(S::grid(n)), dim3(256), 0, stream, tab, n_data,
                       model, ld, aux, ld_aux, n, log_norm, out);
    NB_HIP_CHECK(hipGetLastError());
    return NB_OK;
  });
}
