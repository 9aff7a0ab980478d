// Gaussian-process likelihood of a long ORDERED series (the user-side
// likelihood callable of reference sampler.py:863-873 for a model prediction
// m(theta) of a time series under correlated noise with free kernel
// hyper-parameters):
//     log L = log_norm - 1/2 [ r^T K^-1 r + log det K ],   r = m - d,
//     K[j,k] = a rho(|t_j - t_k| / l) + delta_jk (sigma_j^2 + s),
// for the kernels whose process is a linear stochastic differential equation
// with R states: exp (R = 1), Matern-3/2 (2), Matern-5/2 (3) and the
// underdamped oscillator sho (2).  No matrix is built: a row is one sequential
// pass over the series in the scaled state (f, f' / lambda, f'' / lambda^2),
// lambda = c / l with c = 1, sqrt 3, sqrt 5, 1.  With x = lambda dt and the
// transition Phi(x) (gps_phi below), p the first column of the stationary
// covariance over a ([1], [1, 0], [1, 0, -1/3], [1, 0]), G = 0 (R x R,
// symmetric) and g = 0 (R), step n is
//     G <- Phi G Phi^T,  g <- Phi g                (dt_0 = 0: Phi = 1)
//     d = (a - G00) + (sigma_n^2 + s)
//     v = (m_n - d_n) - g0
//     u = a p - G[:,0],  k = u / d
//     g <- g + k v,  G <- G + u k^T        (G00 as a - (sigma_n^2 + s) k0)
//     Q += v^2 / d (a compensated sum),  L += log d
// and the result log_norm - (Q + L) / 2.  G is the deficit of the predictive
// covariance below the stationary one; nothing cancels but the a - G00 of the
// problem itself.
//
// Mapping: lane = row, a workgroup is ONE wavefront and owns 64 rows; the pass
// over P is sequential.  m is (n, P) row-major, so the lanes' reads would be
// ld doubles apart: a block of 64 rows x NB_GPS_BLOCK columns is staged
// through LDS (nb_gps_stage.h, shared with the kernel for sums of terms,
// nb_gps_terms.hip, as is the transition gps_phi) with 16-byte loads that run along the rows (pairs of doubles at
// 8-byte-aligned addresses, nb_d2u) and an odd row stride in doubles, so that
// the column-wise reads of the recursion fall on distinct banks.  The next
// block's loads are issued into registers before the recursion over the
// current block starts and are written to LDS after it: they are in flight
// for NB_GPS_BLOCK steps.  dt, d and sigma^2 are wave-uniform and come through
// scalar loads of the table's four doubles per step.
//
// log d is not taken per step: the mantissas of the d are multiplied and their
// exponents added, with the renormalisation of nb_noise.hip, and one po_log
// per row ends it.  1 / d is a reciprocal estimate with two Newton steps.
//
// A row's bits depend on P, the kernel and the row's own inputs only: every
// lane runs the same sequence for its own row, no sum crosses lanes, and the
// grid only decides which wavefront takes a row.  A row with an m that is not
// finite, a bad hyper-parameter or a pivot d outside (0, +inf) is NaN: a flag
// that overrides the sum.
#include "../../include/nautilus_hip.h"
#include "nb_common.h"
#include "nb_gps_stage.h"
#include "nb_launch.h"
#include "nb_layout.h"
#include "nb_poisson_log.h"

namespace {

#ifndef NB_GPS_UNROLL
#define NB_GPS_UNROLL 4
#endif
constexpr int GPS_UNROLL = NB_GPS_UNROLL;        // steps of a whole block

// The running state of one row.
template <int KERNEL>
struct gps_state {
  static constexpr int R = gps_states(KERNEL);
  double G[R][R], g[R];
  double Q, Qc, prod;
  int esum;
  bool bad;

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      g[i] = 0.0;
#pragma unroll
      for (int j = 0; j < R; ++j) G[i][j] = 0.0;
    }
    Q = Qc = 0.0;
    prod = 1.0;
    esum = 0;
    bad = false;
  }

  __device__ __forceinline__ void step(const gps_row& h, double dt, double dat,
                                       double s2, double m) {
#pragma clang fp contract(off)
    double phi[R][R];
    gps_phi<KERNEL, R>(h, dt, phi);
    // T = Phi G, then the lower triangle of T Phi^T, sums in index order
    double T[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) {
        double t = phi[i][0] * G[0][j];
#pragma unroll
        for (int k = 1; k < R; ++k) t = t + phi[i][k] * G[k][j];
        T[i][j] = t;
      }
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double t = T[i][0] * phi[j][0];
#pragma unroll
        for (int k = 1; k < R; ++k) t = t + T[i][k] * phi[j][k];
        G[i][j] = t;
        G[j][i] = t;
      }
    double gn[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      double t = phi[i][0] * g[0];
#pragma unroll
      for (int k = 1; k < R; ++k) t = t + phi[i][k] * g[k];
      gn[i] = t;
    }
    const double noise = s2 + h.s;
    const double d = (h.a - G[0][0]) + noise;
    const double v = (m - dat) - gn[0];
    // false for NaN on either side
    bad = bad || !(fabs(m) < __builtin_inf()) ||
          !(d > 0.0 && d < __builtin_inf());
    double id = __builtin_amdgcn_rcp(d);
    id = fma(fma(-d, id, 1.0), id, id);
    id = fma(fma(-d, id, 1.0), id, id);
    double u[R], k[R];
    u[0] = h.a - G[0][0];
    if constexpr (R > 1) u[1] = -G[1][0];
    if constexpr (R > 2) u[2] = h.a * -0x1.5555555555555p-2 - G[2][0];
#pragma unroll
    for (int i = 0; i < R; ++i) k[i] = u[i] * id;
#pragma unroll
    for (int i = 0; i < R; ++i) g[i] = gn[i] + k[i] * v;
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        const double t = G[i][j] + u[i] * k[j];
        G[i][j] = t;
        G[j][i] = t;
      }
    // the same number as G00 + u0 k0, in the form that leaves a - G00 = 0
    // exactly behind a measurement without noise
    G[0][0] = h.a - noise * k[0];
    // compensated: a plain chain of 2^20 additions would lose ten bits
    const double y = (v * v) * id - Qc;
    const double qs = Q + y;
    Qc = (qs - Q) - y;
    Q = qs;
    prod = prod * __builtin_amdgcn_frexp_mant(d);
    esum += __builtin_amdgcn_frexp_exp(d);
  }

  __device__ __forceinline__ void renorm() {
    esum += __builtin_amdgcn_frexp_exp(prod);
    prod = __builtin_amdgcn_frexp_mant(prod);
  }
};

// tab: (dt, d, sigma^2, 0) per datum (nb_layout.h).  model: n rows of n_data
// doubles, ld apart.  hyper: n rows of (a, l, s[, q]), ld_hyper apart.
template <int KERNEL>
__global__ void __launch_bounds__(64)
nb_gps_kernel(const double* __restrict__ tab, int n_data,
              const double* __restrict__ model, long long ld,
              const double* __restrict__ hyper, long long ld_hyper,
              long long n, double log_norm, double* __restrict__ out) {
  __shared__ double lds[64 * GPS_LS];
  const int lane = threadIdx.x;
  for (long long row0 = (long long)blockIdx.x * 64; row0 < n;
       row0 += (long long)gridDim.x * 64) {
    const long long i = row0 + lane < n ? row0 + lane : n - 1;
    gps_row h;
    bool bad_row;
    {
#pragma clang fp contract(off)
      const double* hp = hyper + i * ld_hyper;
      const double l = hp[1];
      h.a = hp[0];
      h.s = hp[2];
      // false for NaN
      bad_row = !(h.a >= 0.0 && h.a < __builtin_inf()) ||
                !(l > 0.0 && l < __builtin_inf()) ||
                !(h.s >= 0.0 && h.s < __builtin_inf());
      // 0 times this stays 0 for a subnormal l as well
      h.inv_l = fmin(1.0 / l, 0x1.fffffffffffffp+1023);
      h.w = h.eta = h.inv_eta = 0.0;
      if constexpr (KERNEL == NB_GPS_SHO) {
        const double q = hp[3];
        bad_row = bad_row || !(q > 0.5 && q < __builtin_inf());
        h.w = 1.0 / (2.0 * q);
        h.eta = sqrt(1.0 - h.w * h.w);
        h.inv_eta = 1.0 / h.eta;
      }
    }
    gps_state<KERNEL> st;
    st.init();
    st.bad = bad_row;
    nb_d2u next[GPS_LOADS];
    __syncthreads();                             // the last pass's reads
    gps_first_block(model, ld, row0, n, n_data, lane, lds, next);
    __syncthreads();
    int since = 0;
    for (int c0 = 0; c0 < n_data; c0 += GPS_C) {
      const int c1 = c0 + GPS_C;
      gps_next_block(model, ld, row0, n, c0, n_data, lane, next);
      const int width = n_data - c0 < GPS_C ? n_data - c0 : GPS_C;
      const double* mine = lds + lane * GPS_LS;
      const double* e = tab + (size_t)NB_GPS_STRIDE * (size_t)c0;
      if (width == GPS_C) {
        // a whole block: unrolled, so that the transition of a later step,
        // which does not depend on the state, fills the gaps of the chain
#pragma unroll GPS_UNROLL
        for (int c = 0; c < GPS_C; ++c)
          st.step(h, e[NB_GPS_STRIDE * c + NB_GPS_DT],
                  e[NB_GPS_STRIDE * c + NB_GPS_DATA],
                  e[NB_GPS_STRIDE * c + NB_GPS_SIGMA2], mine[c]);
      } else {
#pragma unroll 1
        for (int c = 0; c < width; ++c)
          st.step(h, e[NB_GPS_STRIDE * c + NB_GPS_DT],
                  e[NB_GPS_STRIDE * c + NB_GPS_DATA],
                  e[NB_GPS_STRIDE * c + NB_GPS_SIGMA2], mine[c]);
      }
      // the same for every lane: the columns advance in step
      since += width;
      if (since >= GPS_RENORM) {
        since = 0;
        st.renorm();
      }
      __syncthreads();
      if (c1 < n_data) gps_stage(lds, lane, next);
      __syncthreads();
    }
    double res;
    {
#pragma clang fp contract(off)
      // of a flagged row the product may be anything: its log is not used
      const double lg = fma((double)st.esum, 0x1.62e42fefa39efp-1,
                            po_log(st.prod));
      res = log_norm - 0.5 * (st.Q + lg);
    }
    if (st.bad) res = __builtin_nan("");
    if (row0 + lane < n) out[row0 + lane] = res;
  }
}

template <int KERNEL>
int launch(const double* tab, int n_data, const double* model, long long ld,
           const double* hyper, long long ld_hyper, long long n,
           double log_norm, double* out, hipStream_t stream) {
  long long b = (n + 63) / 64;
  if (b > (1 << 20)) b = 1 << 20;
  (void)hipGetLastError();
  hipLaunchKernelGGL((nb_gps_kernel<KERNEL>), dim3((unsigned)b), dim3(64), 0,
                     stream, tab, n_data, model, ld, hyper, ld_hyper, n,
                     log_norm, out);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}

}  // namespace

int nb_launch_gps(const double* tab, int n_data, int kernel,
                  const double* model, long long ld, const double* hyper,
                  long long ld_hyper, long long n, double log_norm,
                  double* out, hipStream_t stream) {
  if (n <= 0) return NB_OK;
  switch (kernel) {
    case NB_GPS_EXP:
      return launch<NB_GPS_EXP>(tab, n_data, model, ld, hyper, ld_hyper, n,
                                log_norm, out, stream);
    case NB_GPS_MATERN32:
      return launch<NB_GPS_MATERN32>(tab, n_data, model, ld, hyper, ld_hyper,
                                     n, log_norm, out, stream);
    case NB_GPS_MATERN52:
      return launch<NB_GPS_MATERN52>(tab, n_data, model, ld, hyper, ld_hyper,
                                     n, log_norm, out, stream);
    default:
      return launch<NB_GPS_SHO>(tab, n_data, model, ld, hyper, ld_hyper, n,
                                log_norm, out, stream);
  }
}
