// The filter of the Gaussian-process likelihood of a long ORDERED series (the
// user-side likelihood callable of reference sampler.py:863-873 for a model
// prediction m(theta) of a time series under correlated noise with free kernel
// hyper-parameters):
//     log L = log_norm - 1/2 [ r^T K^-1 r + log det K ],   r = m - d,
//     K[j,k] = sum_I a_I rho_I(|t_j - t_k| / l_I) + delta_jk (sigma_j^2 + s),
// a sum of one to three terms, every rho_I one of the kernels whose process is
// a linear stochastic differential equation with R states: exp (R = 1),
// Matern-3/2 (2), Matern-5/2 (3) and the underdamped oscillator sho (2).  No
// matrix is built: a row is one sequential pass over the series.  A term lives
// in the scaled state (f, f' / lambda, f'' / lambda^2), lambda = c / l with c =
// 1, sqrt 3, sqrt 5, 1.  A sum of state-space kernels is a state-space kernel:
// the state is the concatenation of the terms' states, the transition is block
// diagonal and the observation reads the first component of every block.  The
// terms are held in SLOTS, sorted by kernel code (equal codes in the caller's
// order); slot I has R_I states from index o_I on, S = sum R_I <=
// NB_GPS_MAX_STATES, the transition Phi_I = gps_phi of its kernel at r_I =
// min(dt / l_I, 1e4) and the first column p_I of its stationary covariance
// over a_I ([1], [1, 0], [1, 0, -1/3], [1, 0]).  With A = sum_I a_I (added in
// slot order), G = 0 (S x S, symmetric) and g = 0 (S), step n is
//   1. G_IJ <- Phi_I G_IJ Phi_J^T for the blocks I >= J (T = Phi_I G_IJ first,
//      every sum in index order; of a diagonal block the lower triangle), the
//      upper blocks by symmetry;  g_I <- Phi_I g_I          (dt_0 = 0: Phi = 1)
//   2. Gh[i] = sum_J G[i][o_J],  c = sum_I Gh[o_I],  noise = sigma_n^2 + s,
//      d = (A - c) + noise
//   3. v = (m_n - d_n) - sum_I g[o_I]
//   4. u[i] = a_I p_I[i - o_I] - Gh[i]  (-Gh[i] where p is 0),  k = u (1 / d)
//   5. g <- g + k v,  G <- G + u k^T on the lower triangle, mirrored; of ONE
//      term, G00 as a - noise k0
//   6. Q += v^2 / d (a compensated sum),  L += log d
// and the result log_norm - (Q + L) / 2.  The sums over slots run in slot
// order; with one slot they are that slot's element and no addition.  G is the
// deficit of the predictive covariance of the state below the stationary one;
// nothing cancels but the A - c of the problem itself.  One term's a - noise
// k0 is the same number as G00 + u0 k0, in the form that leaves a - G00 = 0
// exactly behind a measurement without noise: a repeated time with sigma_n^2 +
// s = 0 then has the pivot 0 and the row is NaN.  The form has no analogue for
// a sum: there such a pivot is 0 only up to rounding, and the row is NaN or
// finite (nothing else, and no other row is touched).
//
// Mapping: lane = row, a workgroup is ONE wavefront and owns 64 rows; the pass
// over P is sequential.  m is (n, P) row-major, so the lanes' reads would be
// ld doubles apart: a block of 64 rows x NB_GPS_BLOCK columns is staged
// through LDS with 16-byte loads that run along the rows (pairs of doubles at
// 8-byte-aligned addresses, nb_d2u) and an odd row stride in doubles, so that
// the column-wise reads of the recursion fall on distinct banks.  The next
// block's loads are issued into registers (gps_request) before the recursion
// over the current block starts and are written to LDS (gps_stage) after it:
// they are in flight for NB_GPS_BLOCK steps.  dt, d and sigma^2 are
// wave-uniform and come through scalar loads of the table's four doubles per
// step.  G and g live in registers: every index is a constant after unrolling.
// One instantiation per multiset of kernels (4 + 23, nb_gps.hip): Phi is
// straight-line code without a switch, and the 1 to 3 exp / sincos of a step,
// which do not depend on the state, fill the gaps of the dependent chain of
// the step before.
//
// log d is not taken per step: the mantissas of the d are multiplied and their
// exponents added, with the renormalisation of nb_noise.hip, and one po_log
// per row ends it.  1 / d is a reciprocal estimate with two Newton steps.
//
// A row's bits depend on P, the multiset of kernels and the row's own inputs
// in slot order only: every lane runs the same sequence for its own row, no
// sum crosses lanes, and the grid only decides which wavefront takes a row.  A
// row with an m that is not finite, a bad hyper-parameter of any term or a
// pivot d outside (0, +inf) is NaN: a flag that overrides the sum.
#pragma once
#include "../../include/nautilus_hip.h"
#include "nb_common.h"
#include "nb_layout.h"
#include "nb_poisson_log.h"

namespace {

// steps of a whole block that are unrolled, of one term and of a sum
#ifndef NB_GPS_UNROLL
#define NB_GPS_UNROLL 4
#endif
#ifndef NB_GPS_TERMS_UNROLL
#define NB_GPS_TERMS_UNROLL 4
#endif

constexpr int GPS_C = NB_GPS_BLOCK;              // columns of a staged block
constexpr int GPS_LS = GPS_C + 1;                // LDS row stride, odd
constexpr int GPS_LOADS = GPS_C / 2;             // 16-byte loads per lane
constexpr int GPS_RENORM = 256;                  // steps between two frexp
static_assert(GPS_C % 2 == 0 && 64 % GPS_LOADS == 0, "whole rows per load");

constexpr int gps_states(int kernel) {
  return kernel < 0 ? 0
         : kernel == NB_GPS_EXP ? 1 : kernel == NB_GPS_MATERN52 ? 3 : 2;
}

// what a row keeps of the hyper-parameters of a term
struct gps_row {
  double a, inv_l;
  double w, eta, inv_eta;                        // sho: 1 / (2 q), eta, 1 / eta
};

// The hyper-parameters of one term from hp = (a, l) and, for sho, q = *qp;
// true when the row is to be NaN.
template <int KERNEL>
__device__ __forceinline__ bool gps_load(const double* hp, const double* qp,
                                         gps_row& h) {
#pragma clang fp contract(off)
  const double l = hp[1];
  h.a = hp[0];
  // false for NaN
  bool bad = !(h.a >= 0.0 && h.a < __builtin_inf()) ||
             !(l > 0.0 && l < __builtin_inf());
  // 0 times this stays 0 for a subnormal l as well
  h.inv_l = fmin(1.0 / l, 0x1.fffffffffffffp+1023);
  h.w = h.eta = h.inv_eta = 0.0;
  if constexpr (KERNEL == NB_GPS_SHO) {
    const double q = *qp;
    bad = bad || !(q > 0.5 && q < __builtin_inf());
    h.w = 1.0 / (2.0 * q);
    h.eta = sqrt(1.0 - h.w * h.w);
    h.inv_eta = 1.0 / h.eta;
  }
  return bad;
}

// Phi(x) at r = dt / l into the rows O.. of phi, capped as gp_rho caps it
// (beyond 1e4 every exponential here is 0 in float64, and the cap keeps an
// infinite r from meeting that 0; it also bounds the argument of the sine)
template <int KERNEL, int O, int S>
__device__ __forceinline__ void gps_phi(const gps_row& h, double dt,
                                        double (&phi)[S][3]) {
#pragma clang fp contract(off)
  const double r = fmin(dt * h.inv_l, 1e4);
  if constexpr (KERNEL == NB_GPS_EXP) {
    phi[O][0] = exp(-r);
  } else if constexpr (KERNEL == NB_GPS_MATERN32) {
    const double x = 0x1.bb67ae8584caap+0 * r;              // sqrt(3) r
    const double e = exp(-x);
    const double ex = e * x;
    phi[O][0] = e * (1.0 + x);
    phi[O][1] = ex;
    phi[O + 1][0] = -ex;
    phi[O + 1][1] = e * (1.0 - x);
  } else if constexpr (KERNEL == NB_GPS_MATERN52) {
    const double x = 0x1.1e3779b97f4a8p+1 * r;              // sqrt(5) r
    const double e = exp(-x);
    const double x2 = x * x;
    const double hx = 0.5 * x2;
    phi[O][0] = e * ((1.0 + x) + hx);
    phi[O][1] = e * (x + x2);
    phi[O][2] = e * hx;
    phi[O + 1][0] = -(e * hx);
    phi[O + 1][1] = e * ((1.0 + x) - x2);
    phi[O + 1][2] = e * (x - hx);
    phi[O + 2][0] = e * (hx - x);
    phi[O + 2][1] = e * (x2 - 3.0 * x);
    phi[O + 2][2] = e * ((1.0 - 2.0 * x) + hx);
  } else {
    const double e = exp(-(r * h.w));
    const double arg = h.eta * r;                // in [0, 1e4]
    double sn, c;
    sincos(arg, &sn, &c);
    const double sg = sn * h.inv_eta;
    const double sw = sg * h.w;
    const double es = e * sg;
    phi[O][0] = e * (c + sw);
    phi[O][1] = es;
    phi[O + 1][0] = -es;
    phi[O + 1][1] = e * (c - sw);
  }
}

// G_IJ <- Phi_I G_IJ Phi_J^T of the block at rows OI.., columns OJ.., OI >=
// OJ, mirrored into the upper triangle
template <int OI, int RI, int OJ, int RJ, int S>
__device__ __forceinline__ void gps_block(double (&G)[S][S],
                                          const double (&phi)[S][3]) {
#pragma clang fp contract(off)
  double T[RI][RJ];
#pragma unroll
  for (int i = 0; i < RI; ++i)
#pragma unroll
    for (int j = 0; j < RJ; ++j) {
      double t = phi[OI + i][0] * G[OI][OJ + j];
#pragma unroll
      for (int k = 1; k < RI; ++k) t = t + phi[OI + i][k] * G[OI + k][OJ + j];
      T[i][j] = t;
    }
#pragma unroll
  for (int i = 0; i < RI; ++i)
#pragma unroll
    for (int j = 0; j < (OI == OJ ? i + 1 : RJ); ++j) {
      double t = T[i][0] * phi[OJ + j][0];
#pragma unroll
      for (int k = 1; k < RJ; ++k) t = t + T[i][k] * phi[OJ + j][k];
      G[OI + i][OJ + j] = t;
      G[OJ + j][OI + i] = t;
    }
}

// gn_I = Phi_I g_I
template <int OI, int RI, int S>
__device__ __forceinline__ void gps_vec(const double (&g)[S], double (&gn)[S],
                                        const double (&phi)[S][3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    double t = phi[OI + i][0] * g[OI];
#pragma unroll
    for (int k = 1; k < RI; ++k) t = t + phi[OI + i][k] * g[OI + k];
    gn[OI + i] = t;
  }
}

// u_I = a_I p_I - Gh_I
template <int KERNEL, int OI, int S>
__device__ __forceinline__ void gps_gain(double a, const double (&Gh)[S],
                                         double (&u)[S]) {
#pragma clang fp contract(off)
  constexpr int R = gps_states(KERNEL);
  u[OI] = a - Gh[OI];
  if constexpr (R > 1) u[OI + 1] = -Gh[OI + 1];
  if constexpr (R > 2) u[OI + 2] = a * -0x1.5555555555555p-2 - Gh[OI + 2];
}

// The running state of one row under the terms <K0, K1, K2> in slot order;
// K1 < 0: one term, K2 < 0: at most two.
template <int K0, int K1, int K2>
struct gps_state {
  static constexpr int J = K1 < 0 ? 1 : K2 < 0 ? 2 : 3;
  static constexpr int R0 = gps_states(K0), R1 = gps_states(K1);
  static constexpr int R2 = gps_states(K2);
  static constexpr int O0 = 0, O1 = R0, O2 = R0 + R1;
  static constexpr int S = R0 + R1 + R2;
  static constexpr int UNROLL = J == 1 ? NB_GPS_UNROLL : NB_GPS_TERMS_UNROLL;
  static_assert(K0 >= 0 && (K1 >= 0 || K2 < 0), "the slots fill in order");
  static_assert((K1 < 0 || K0 <= K1) && (K2 < 0 || K1 <= K2),
                "the slots are sorted");
  static_assert(S <= NB_GPS_MAX_STATES, "too many states");

  gps_row h[J];                                  // the slots' hyper-parameters
  double total, s;                               // A and the jitter variance
  double G[S][S], g[S];
  double Q, Qc, prod;
  int esum;
  bool bad;

  // hp: the row of the hyper input (plan: nb_layout.h)
  __device__ __forceinline__ void init(const double* hp,
                                       const nb_gps_plan& plan) {
#pragma clang fp contract(off)
    s = hp[plan.col_s];
    // false for NaN
    bad = !(s >= 0.0 && s < __builtin_inf());
    bad = gps_load<K0>(hp + plan.col[0], hp + plan.col_q[0], h[0]) || bad;
    total = h[0].a;
    if constexpr (J > 1) {
      bad = gps_load<K1>(hp + plan.col[1], hp + plan.col_q[1], h[1]) || bad;
      total = total + h[1].a;
    }
    if constexpr (J > 2) {
      bad = gps_load<K2>(hp + plan.col[2], hp + plan.col_q[2], h[2]) || bad;
      total = total + h[2].a;
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
      g[i] = 0.0;
#pragma unroll
      for (int j = 0; j < S; ++j) G[i][j] = 0.0;
    }
    Q = Qc = 0.0;
    prod = 1.0;
    esum = 0;
  }

  __device__ __forceinline__ void step(double dt, double dat, double s2,
                                       double m) {
#pragma clang fp contract(off)
    double phi[S][3];
    gps_phi<K0, O0>(h[0], dt, phi);
    if constexpr (J > 1) gps_phi<K1, O1>(h[1], dt, phi);
    if constexpr (J > 2) gps_phi<K2, O2>(h[2], dt, phi);
    // 1. the lower blocks, then g
    double gn[S];
    gps_block<O0, R0, O0, R0>(G, phi);
    if constexpr (J > 1) {
      gps_block<O1, R1, O0, R0>(G, phi);
      gps_block<O1, R1, O1, R1>(G, phi);
    }
    if constexpr (J > 2) {
      gps_block<O2, R2, O0, R0>(G, phi);
      gps_block<O2, R2, O1, R1>(G, phi);
      gps_block<O2, R2, O2, R2>(G, phi);
    }
    gps_vec<O0, R0>(g, gn, phi);
    if constexpr (J > 1) gps_vec<O1, R1>(g, gn, phi);
    if constexpr (J > 2) gps_vec<O2, R2>(g, gn, phi);
    // 2. what the observation sees of G, and the pivot
    double Gh[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      double t = G[i][O0];
      if constexpr (J > 1) t = t + G[i][O1];
      if constexpr (J > 2) t = t + G[i][O2];
      Gh[i] = t;
    }
    double c = Gh[O0], gs = gn[O0];
    if constexpr (J > 1) {
      c = c + Gh[O1];
      gs = gs + gn[O1];
    }
    if constexpr (J > 2) {
      c = c + Gh[O2];
      gs = gs + gn[O2];
    }
    const double noise = s2 + s;
    const double d = (total - c) + noise;
    // 3.
    const double v = (m - dat) - gs;
    // false for NaN on either side
    bad = bad || !(fabs(m) < __builtin_inf()) ||
          !(d > 0.0 && d < __builtin_inf());
    double id = __builtin_amdgcn_rcp(d);
    id = fma(fma(-d, id, 1.0), id, id);
    id = fma(fma(-d, id, 1.0), id, id);
    // 4.
    double u[S], k[S];
    gps_gain<K0, O0>(h[0].a, Gh, u);
    if constexpr (J > 1) gps_gain<K1, O1>(h[1].a, Gh, u);
    if constexpr (J > 2) gps_gain<K2, O2>(h[2].a, Gh, u);
#pragma unroll
    for (int i = 0; i < S; ++i) k[i] = u[i] * id;
    // 5.
#pragma unroll
    for (int i = 0; i < S; ++i) g[i] = gn[i] + k[i] * v;
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        const double t = G[i][j] + u[i] * k[j];
        G[i][j] = t;
        G[j][i] = t;
      }
    // the same number as G00 + u0 k0, in the form that leaves a - G00 = 0
    // exactly behind a measurement without noise
    if constexpr (J == 1) G[0][0] = h[0].a - noise * k[0];
    // 6. compensated: a plain chain of 2^20 additions would lose ten bits
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

// Requests the block of 64 rows x GPS_C columns from column c0 on: load j of
// a lane is the pair of columns 2 q, 2 q + 1 of row 64 / GPS_LOADS * j + lane
// / GPS_LOADS, q = lane % GPS_LOADS, so that GPS_LOADS neighbouring lanes read
// 16 GPS_LOADS contiguous bytes.  A pair that straddles the end of the row is
// one double, a pair beyond it is not read.
template <bool WHOLE>
__device__ __forceinline__ void gps_request(const double* __restrict__ model,
                                            long long ld, long long row0,
                                            long long n, int c0, int n_data,
                                            int lane, nb_d2u (&v)[GPS_LOADS]) {
  constexpr int RPL = 64 / GPS_LOADS;            // rows of one load
  const int q = lane % GPS_LOADS;
  const int col = c0 + 2 * q;
#pragma unroll
  for (int j = 0; j < GPS_LOADS; ++j) {
    long long i = row0 + RPL * j + lane / GPS_LOADS;
    i = i < n ? i : n - 1;                       // the last row again
    const double* src = model + i * ld + col;
    if (WHOLE || col + 1 < n_data) {
      v[j] = *(const nb_d2u*)src;
    } else {
      v[j].x = col < n_data ? src[0] : 0.0;
      v[j].y = 0.0;
    }
  }
}

__device__ __forceinline__ void gps_stage(double* lds, int lane,
                                          const nb_d2u (&v)[GPS_LOADS]) {
  constexpr int RPL = 64 / GPS_LOADS;
  const int q = lane % GPS_LOADS;
#pragma unroll
  for (int j = 0; j < GPS_LOADS; ++j) {
    double* dst = lds + (RPL * j + lane / GPS_LOADS) * GPS_LS + 2 * q;
    dst[0] = v[j].x;
    dst[1] = v[j].y;
  }
}

// Requests and stages the first block of a pass.
__device__ __forceinline__ void gps_first_block(
    const double* __restrict__ model, long long ld, long long row0,
    long long n, int n_data, int lane, double* lds,
    nb_d2u (&next)[GPS_LOADS]) {
  if (GPS_C <= n_data)
    gps_request<true>(model, ld, row0, n, 0, n_data, lane, next);
  else
    gps_request<false>(model, ld, row0, n, 0, n_data, lane, next);
  gps_stage(lds, lane, next);
}

// Requests the block after the one from column c0 on, if there is one.
__device__ __forceinline__ void gps_next_block(
    const double* __restrict__ model, long long ld, long long row0,
    long long n, int c0, int n_data, int lane, nb_d2u (&next)[GPS_LOADS]) {
  const int c1 = c0 + GPS_C;
  if (c1 + GPS_C <= n_data)
    gps_request<true>(model, ld, row0, n, c1, n_data, lane, next);
  else if (c1 < n_data)
    gps_request<false>(model, ld, row0, n, c1, n_data, lane, next);
}

// The rows of one wavefront, 64 at a time.  tab: (dt, d, sigma^2, 0) per datum
// (nb_layout.h).  model: n rows of n_data doubles, ld apart.  hyper: n rows,
// ld_hyper apart, read as plan says.  lds: 64 * GPS_LS doubles.
template <class State>
__device__ __forceinline__ void gps_rows(
    const double* __restrict__ tab, int n_data,
    const double* __restrict__ model, long long ld,
    const double* __restrict__ hyper, long long ld_hyper,
    const nb_gps_plan& plan, long long n, double log_norm,
    double* __restrict__ out, double* lds) {
  const int lane = threadIdx.x;
  for (long long row0 = (long long)blockIdx.x * 64; row0 < n;
       row0 += (long long)gridDim.x * 64) {
    const long long i = row0 + lane < n ? row0 + lane : n - 1;
    State st;
    st.init(hyper + i * ld_hyper, plan);
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
        // a whole block: unrolled, so that the transitions of a later step,
        // which do not depend on the state, fill the gaps of the chain
#pragma unroll State::UNROLL
        for (int c = 0; c < GPS_C; ++c)
          st.step(e[NB_GPS_STRIDE * c + NB_GPS_DT],
                  e[NB_GPS_STRIDE * c + NB_GPS_DATA],
                  e[NB_GPS_STRIDE * c + NB_GPS_SIGMA2], mine[c]);
      } else {
#pragma unroll 1
        for (int c = 0; c < width; ++c)
          st.step(e[NB_GPS_STRIDE * c + NB_GPS_DT],
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

}  // namespace
