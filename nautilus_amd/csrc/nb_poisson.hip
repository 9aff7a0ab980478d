// Poisson likelihood of BINNED COUNTS in one streaming kernel (the user-side
// likelihood callable of reference sampler.py:863-873 for a model prediction
// m(theta) of the rates in P bins with observed counts k):
//     mu_j = e_j m_j + b_j,      log L = C - sum_j D(mu_j, k_j),
//     D(mu, 0) = mu,
//     D(mu, k) = k (t - lg),  t = (mu - k) (1 / k),
//                lg = log1p(t) if |t| < 1/2 else log(mu (1 / k)),
// the deviance form: every term is >= 0, so the sum does not cancel the way
// k log mu - mu does for large counts.  C (0, or sum_j k log k - k - lgamma(k
// + 1)) comes from the host.
//
// 8 P bytes read + 8 written per point, and per element about 100
// instructions, ~35 of them the float64 log (po_log, nb_poisson_log.h): VALU
// issue, not HBM, sets the time.  Layout after nb_chi2_diag_kernel:
//  * L lanes share a row (16 up to P = 512, a whole wavefront beyond: L
//    depends on P only); a load instruction of a wavefront covers 64 / L rows
//    x 128 L / 16 contiguous bytes;
//  * a lane group walks R rows at once and U column blocks of L per step, so
//    R U independent loads, logs and partial sums are in flight per lane and
//    a table entry (k, 1 / k, e, b: device memory, L2 resident) read once
//    serves R rows; the model values of the next step are requested before
//    the logs of the current one start;
//  * one log per element: for |t| < 1/2 the argument is hi = fl(1 + t) and the
//    rounding error lo = t - (hi - 1) (exact) comes back as lo / hi, so that
//    log1p(t) = log(hi) + lo / hi to O(eps^2); otherwise the argument is
//    mu (1 / k) and the correction is switched off;
//  * a row's U partials are added in a fixed tree, then over its L lanes by
//    shuffles.  The order depends on P alone: no atomics, and the bits of a
//    row depend on neither n, the row's place in the batch, ld, the stream nor
//    the grid (R only says which rows travel together).
// mu = 0 with k > 0 gives -inf; a negative, NaN or infinite mu gives NaN and
// wins over -inf.  Both are flags, OR-ed over the row, and a flagged row's sum
// is discarded: nothing relies on what inf - inf happens to be.
#include "nb_common.h"
#include "nb_launch.h"
#include "nb_poisson_term.h"

namespace {

// tab: k [P], 1 / k [P] (0 where k = 0), e [P], b [P].  model: n rows of
// n_data doubles, ld doubles apart.
template <int L, int R, int U>
__global__ void __launch_bounds__(256)
nb_poisson_kernel(const double* __restrict__ tab, int n_data,
                  const double* __restrict__ model, long long ld, long long n,
                  double log_const, double* __restrict__ out) {
  static_assert(U == 1 || U == 2 || U == 4, "fixed tree over the partials");
  constexpr int G = 256 / L;                     // lane groups of a workgroup
  const int sub = threadIdx.x & (L - 1);
  const double* tk = tab;
  const double* tik = tab + n_data;
  const double* te = tab + 2 * (size_t)n_data;
  const double* tb = tab + 3 * (size_t)n_data;
  const long long stride = (long long)gridDim.x * G * R;
  for (long long p0 = ((long long)blockIdx.x * G + threadIdx.x / L) * R;
       p0 < n; p0 += stride) {
    // a row past the end of the batch is the last row again, never stored
    const double* row[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
      row[r] = model + (p0 + r < n ? p0 + r : n - 1) * ld;
    double a[R][U], next[R][U];
    unsigned flag[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      flag[r] = 0u;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        a[r][u] = 0.0;
        const int j = sub + L * u;               // a column past the end is
        next[r][u] = row[r][j < n_data ? j : n_data - 1];   // the last again
      }
    }
    for (int c = sub; c < n_data; c += L * U) {
      double m[R][U], k[U], ik[U], e[U], b[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = c + L * u;
        const int jc = j < n_data ? j : n_data - 1;
        k[u] = tk[jc];
        ik[u] = tik[jc];
        e[u] = te[jc];
        b[u] = tb[jc];
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
          unsigned f = 0u;
          const double d = po_term(m[r][u], k[u], ik[u], e[u], b[u], &f);
          a[r][u] += in ? d : 0.0;
          flag[r] |= in ? f : 0u;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double v = a[r][0];
      if constexpr (U == 2) v = a[r][0] + a[r][1];
      if constexpr (U == 4) v = (a[r][0] + a[r][1]) + (a[r][2] + a[r][3]);
      unsigned f = flag[r];
#pragma unroll
      for (int s = 1; s < L; s <<= 1) {
        v += __shfl_xor(v, s);
        f |= (unsigned)__shfl_xor((int)f, s);
      }
      double res = log_const - v;
      if (f & PO_NEG_INF) res = -__builtin_inf();
      if (f & PO_NAN) res = __builtin_nan("");
      if (sub == 0 && p0 + r < n) out[p0 + r] = res;
    }
  }
}

}  // namespace

int nb_launch_poisson(const double* tab, int n_data, const double* model,
                      long long ld, long long n, double log_const,
                      double* out, hipStream_t stream) {
  if (n <= 0) return NB_OK;
  return nb_stream_dispatch(n_data, [&](auto s) {
    using S = decltype(s);
    (void)hipGetLastError();
    hipLaunchKernelGGL((nb_poisson_kernel<S::L, S::R, S::U>),
                       dim3(S::grid(n)), dim3(256), 0, stream, tab, n_data,
                       model, ld, n, log_const, out);
    NB_HIP_CHECK(hipGetLastError());
    return NB_OK;
  });
}
