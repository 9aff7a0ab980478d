// Gaussian-process likelihood of a long ORDERED series whose covariance is a
// SUM of two or three kernel terms (the user-side likelihood callable of
// reference sampler.py:863-873 for a model prediction m(theta) of a time
// series under correlated noise with free kernel hyper-parameters):
//     log L = log_norm - 1/2 [ r^T K^-1 r + log det K ],   r = m - d,
//     K[j,k] = sum_I a_I rho_I(|t_j - t_k| / l_I) + delta_jk (sigma_j^2 + s),
// every rho_I one of the kernels of nb_gps.hip.  A sum of state-space kernels
// is a state-space kernel: the state is the concatenation of the terms'
// states, the transition is block diagonal and the observation reads the first
// component of every block.  The terms are held in SLOTS, sorted by kernel
// code (equal codes in the caller's order); slot I has R_I states from index
// o_I on, S = sum R_I <= NB_GPS_MAX_STATES, the transition Phi_I = gps_phi of
// its kernel at r_I = min(dt / l_I, 1e4) and the first column p_I of its
// stationary covariance over a_I ([1], [1, 0], [1, 0, -1/3], [1, 0]).  With
// A = sum_I a_I (added in slot order), G = 0 (S x S, symmetric) and g = 0 (S),
// step n is
//   1. G_IJ <- Phi_I G_IJ Phi_J^T for the blocks I >= J (T = Phi_I G_IJ first,
//      every sum in index order; of a diagonal block the lower triangle), the
//      upper blocks by symmetry;  g_I <- Phi_I g_I
//   2. Gh[i] = sum_J G[i][o_J],  c = sum_I Gh[o_I],  noise = sigma_n^2 + s,
//      d = (A - c) + noise
//   3. v = (m_n - d_n) - sum_I g[o_I]
//   4. u[i] = a_I p_I[i - o_I] - Gh[i]  (-Gh[i] where p is 0),  k = u (1 / d)
//   5. g <- g + k v,  G <- G + u k^T on the lower triangle, mirrored
//   6. Q += v^2 / d (a compensated sum),  L += log d
// and the result log_norm - (Q + L) / 2.  The sums over slots run in slot
// order.  G is the deficit of the predictive covariance of the state below the
// stationary one, as in nb_gps.hip, but its G00 = a - noise k0 form has no
// analogue for a sum: a repeated time with sigma_n^2 + s = 0 leaves a pivot
// that is 0 only up to rounding, and such a row is NaN or finite (nothing
// else, and no other row is touched).
//
// Mapping, staging of m (nb_gps_stage.h), scalar reads of the table, the log
// of the product of the pivots' mantissas and the reciprocal are those of
// nb_gps.hip.  G and g live in registers: every index below is a constant
// after unrolling.  One instantiation per multiset of kernels (23): Phi is
// straight-line code without a switch, and the 1 to 3 exp / sincos of a step,
// which do not depend on the state, fill the gaps of the dependent chain of
// the step before.
//
// A row's bits depend on P, the multiset of kernels and the row's own inputs
// in slot order only.  A row with an m that is not finite, a bad
// hyper-parameter of any term or a pivot d outside (0, +inf) is NaN.
#include "../../include/nautilus_hip.h"
#include "nb_common.h"
#include "nb_gps_stage.h"
#include "nb_launch.h"
#include "nb_layout.h"
#include "nb_poisson_log.h"

namespace {

#ifndef NB_GPS_TERMS_UNROLL
#define NB_GPS_TERMS_UNROLL 4
#endif
constexpr int GPT_UNROLL = NB_GPS_TERMS_UNROLL;  // steps of a whole block

// slot I of <K0, K1, K2>; K2 < 0: two terms
template <int K0, int K1, int K2>
struct gpt_shape {
  static constexpr int J = K2 < 0 ? 2 : 3;
  static constexpr int R0 = gps_states(K0), R1 = gps_states(K1);
  static constexpr int R2 = K2 < 0 ? 0 : gps_states(K2);
  static constexpr int A2 = R2 > 0 ? R2 : 1;     // no array of no elements
  static constexpr int O0 = 0, O1 = R0, O2 = R0 + R1;
  static constexpr int S = R0 + R1 + R2;
  static_assert(K0 <= K1 && (K2 < 0 || K1 <= K2), "slots are sorted");
  static_assert(S <= NB_GPS_MAX_STATES, "too many states");
};

// G_IJ <- Phi_I G_IJ Phi_J^T of the block at rows OI.., columns OJ.., OI >=
// OJ, mirrored into the upper triangle
template <int OI, int OJ, int S, int RI, int RJ>
__device__ __forceinline__ void gpt_block(double (&G)[S][S],
                                          const double (&pi)[RI][RI],
                                          const double (&pj)[RJ][RJ]) {
#pragma clang fp contract(off)
  double T[RI][RJ];
#pragma unroll
  for (int i = 0; i < RI; ++i)
#pragma unroll
    for (int j = 0; j < RJ; ++j) {
      double t = pi[i][0] * G[OI][OJ + j];
#pragma unroll
      for (int k = 1; k < RI; ++k) t = t + pi[i][k] * G[OI + k][OJ + j];
      T[i][j] = t;
    }
#pragma unroll
  for (int i = 0; i < RI; ++i)
#pragma unroll
    for (int j = 0; j < (OI == OJ ? i + 1 : RJ); ++j) {
      double t = T[i][0] * pj[j][0];
#pragma unroll
      for (int k = 1; k < RJ; ++k) t = t + T[i][k] * pj[j][k];
      G[OI + i][OJ + j] = t;
      G[OJ + j][OI + i] = t;
    }
}

// gn_I = Phi_I g_I
template <int OI, int S, int RI>
__device__ __forceinline__ void gpt_vec(const double (&g)[S], double (&gn)[S],
                                        const double (&pi)[RI][RI]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < RI; ++i) {
    double t = pi[i][0] * g[OI];
#pragma unroll
    for (int k = 1; k < RI; ++k) t = t + pi[i][k] * g[OI + k];
    gn[OI + i] = t;
  }
}

// u_I = a_I p_I - Gh_I
template <int KERNEL, int OI, int S>
__device__ __forceinline__ void gpt_gain(double a, const double (&Gh)[S],
                                         double (&u)[S]) {
#pragma clang fp contract(off)
  constexpr int R = gps_states(KERNEL);
  u[OI] = a - Gh[OI];
  if constexpr (R > 1) u[OI + 1] = -Gh[OI + 1];
  if constexpr (R > 2) u[OI + 2] = a * -0x1.5555555555555p-2 - Gh[OI + 2];
}

// The running state of one row.
template <int K0, int K1, int K2>
struct gpt_state {
  using sh = gpt_shape<K0, K1, K2>;
  static constexpr int S = sh::S;
  double G[S][S], g[S];
  double Q, Qc, prod;
  int esum;
  bool bad;

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int i = 0; i < S; ++i) {
      g[i] = 0.0;
#pragma unroll
      for (int j = 0; j < S; ++j) G[i][j] = 0.0;
    }
    Q = Qc = 0.0;
    prod = 1.0;
    esum = 0;
    bad = false;
  }

  // h: the slots' hyper-parameters, total: A, s: the jitter variance
  __device__ __forceinline__ void step(const gps_row (&h)[3], double total,
                                       double s, double dt, double dat,
                                       double s2, double m) {
#pragma clang fp contract(off)
    double p0[sh::R0][sh::R0], p1[sh::R1][sh::R1], p2[sh::A2][sh::A2];
    gps_phi<K0, sh::R0>(h[0], dt, p0);
    gps_phi<K1, sh::R1>(h[1], dt, p1);
    if constexpr (sh::J > 2) gps_phi<K2, sh::R2>(h[2], dt, p2);
    // 1. the lower blocks, then g
    gpt_block<sh::O0, sh::O0>(G, p0, p0);
    gpt_block<sh::O1, sh::O0>(G, p1, p0);
    gpt_block<sh::O1, sh::O1>(G, p1, p1);
    if constexpr (sh::J > 2) {
      gpt_block<sh::O2, sh::O0>(G, p2, p0);
      gpt_block<sh::O2, sh::O1>(G, p2, p1);
      gpt_block<sh::O2, sh::O2>(G, p2, p2);
    }
    double gn[S];
    gpt_vec<sh::O0>(g, gn, p0);
    gpt_vec<sh::O1>(g, gn, p1);
    if constexpr (sh::J > 2) gpt_vec<sh::O2>(g, gn, p2);
    // 2. what the observation sees of G, and the pivot
    double Gh[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      double t = G[i][sh::O0] + G[i][sh::O1];
      if constexpr (sh::J > 2) t = t + G[i][sh::O2];
      Gh[i] = t;
    }
    double c = Gh[sh::O0] + Gh[sh::O1];
    double gs = gn[sh::O0] + gn[sh::O1];
    if constexpr (sh::J > 2) {
      c = c + Gh[sh::O2];
      gs = gs + gn[sh::O2];
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
    gpt_gain<K0, sh::O0>(h[0].a, Gh, u);
    gpt_gain<K1, sh::O1>(h[1].a, Gh, u);
    if constexpr (sh::J > 2) gpt_gain<K2, sh::O2>(h[2].a, Gh, u);
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

// where a row of the hyper input holds (a, l[, q]) of every slot, and s
struct gpt_cols {
  int term[3];
  int s;
};

// The hyper-parameters of one slot from hp = (a, l[, q]); true when the row
// is to be NaN.
template <int KERNEL>
__device__ __forceinline__ bool gpt_load(const double* hp, gps_row& h) {
#pragma clang fp contract(off)
  const double l = hp[1];
  h.a = hp[0];
  h.s = 0.0;
  // false for NaN
  bool bad = !(h.a >= 0.0 && h.a < __builtin_inf()) ||
             !(l > 0.0 && l < __builtin_inf());
  // 0 times this stays 0 for a subnormal l as well
  h.inv_l = fmin(1.0 / l, 0x1.fffffffffffffp+1023);
  h.w = h.eta = h.inv_eta = 0.0;
  if constexpr (KERNEL == NB_GPS_SHO) {
    const double q = hp[2];
    bad = bad || !(q > 0.5 && q < __builtin_inf());
    h.w = 1.0 / (2.0 * q);
    h.eta = sqrt(1.0 - h.w * h.w);
    h.inv_eta = 1.0 / h.eta;
  }
  return bad;
}

// tab: (dt, d, sigma^2, 0) per datum (nb_layout.h).  model: n rows of n_data
// doubles, ld apart.  hyper: n rows, ld_hyper apart, with (a, l[, q]) of slot
// I from column cols.term[I] on and s in column cols.s.
template <int K0, int K1, int K2>
__global__ void __launch_bounds__(64)
nb_gps_terms_kernel(const double* __restrict__ tab, int n_data,
                    const double* __restrict__ model, long long ld,
                    const double* __restrict__ hyper, long long ld_hyper,
                    gpt_cols cols, long long n, double log_norm,
                    double* __restrict__ out) {
  __shared__ double lds[64 * GPS_LS];
  const int lane = threadIdx.x;
  for (long long row0 = (long long)blockIdx.x * 64; row0 < n;
       row0 += (long long)gridDim.x * 64) {
    const long long i = row0 + lane < n ? row0 + lane : n - 1;
    gps_row h[3];
    double total, s;
    bool bad_row;
    {
#pragma clang fp contract(off)
      const double* hp = hyper + i * ld_hyper;
      s = hp[cols.s];
      bad_row = !(s >= 0.0 && s < __builtin_inf());
      bad_row = gpt_load<K0>(hp + cols.term[0], h[0]) || bad_row;
      bad_row = gpt_load<K1>(hp + cols.term[1], h[1]) || bad_row;
      total = h[0].a + h[1].a;
      if constexpr (K2 >= 0) {
        bad_row = gpt_load<K2>(hp + cols.term[2], h[2]) || bad_row;
        total = total + h[2].a;
      } else {
        h[2] = h[1];                             // never read
      }
    }
    gpt_state<K0, K1, K2> st;
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
        // a whole block: unrolled, so that the transitions of a later step,
        // which do not depend on the state, fill the gaps of the chain
#pragma unroll GPT_UNROLL
        for (int c = 0; c < GPS_C; ++c)
          st.step(h, total, s, e[NB_GPS_STRIDE * c + NB_GPS_DT],
                  e[NB_GPS_STRIDE * c + NB_GPS_DATA],
                  e[NB_GPS_STRIDE * c + NB_GPS_SIGMA2], mine[c]);
      } else {
#pragma unroll 1
        for (int c = 0; c < width; ++c)
          st.step(h, total, s, e[NB_GPS_STRIDE * c + NB_GPS_DT],
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

template <int K0, int K1, int K2>
int launch(const double* tab, int n_data, const double* model, long long ld,
           const double* hyper, long long ld_hyper, const gpt_cols& cols,
           long long n, double log_norm, double* out, hipStream_t stream) {
  long long b = (n + 63) / 64;
  if (b > (1 << 20)) b = 1 << 20;
  (void)hipGetLastError();
  hipLaunchKernelGGL((nb_gps_terms_kernel<K0, K1, K2>), dim3((unsigned)b),
                     dim3(64), 0, stream, tab, n_data, model, ld, hyper,
                     ld_hyper, cols, n, log_norm, out);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}

// -1 for "no third term" is digit 0
constexpr int gpt_key(int k0, int k1, int k2) {
  return k0 + 4 * k1 + 16 * (k2 + 1);
}

}  // namespace

int nb_launch_gps_terms(const double* tab, int n_data, int n_terms,
                        const int* kinds, const int* cols, int col_s,
                        const double* model, long long ld,
                        const double* hyper, long long ld_hyper, long long n,
                        double log_norm, double* out, hipStream_t stream) {
  if (n <= 0) return NB_OK;
  gpt_cols cc;
  cc.term[0] = cols[0];
  cc.term[1] = cols[1];
  cc.term[2] = n_terms > 2 ? cols[2] : cols[1];
  cc.s = col_s;
#define GPT_CASE(K0, K1, K2)                                                 \
  case gpt_key(K0, K1, K2):                                                  \
    return launch<K0, K1, K2>(tab, n_data, model, ld, hyper, ld_hyper, cc,   \
                              n, log_norm, out, stream);
  switch (gpt_key(kinds[0], kinds[1], n_terms > 2 ? kinds[2] : -1)) {
    // the 10 pairs
    GPT_CASE(0, 0, -1) GPT_CASE(0, 1, -1) GPT_CASE(0, 2, -1)
    GPT_CASE(0, 3, -1) GPT_CASE(1, 1, -1) GPT_CASE(1, 2, -1)
    GPT_CASE(1, 3, -1) GPT_CASE(2, 2, -1) GPT_CASE(2, 3, -1)
    GPT_CASE(3, 3, -1)
    // the 13 triples of at most NB_GPS_MAX_STATES states
    GPT_CASE(0, 0, 0) GPT_CASE(0, 0, 1) GPT_CASE(0, 0, 2) GPT_CASE(0, 0, 3)
    GPT_CASE(0, 1, 1) GPT_CASE(0, 1, 2) GPT_CASE(0, 1, 3) GPT_CASE(0, 2, 3)
    GPT_CASE(0, 3, 3) GPT_CASE(1, 1, 1) GPT_CASE(1, 1, 3) GPT_CASE(1, 3, 3)
    GPT_CASE(3, 3, 3)
  }
#undef GPT_CASE
  nb_set_error("no Gaussian-process series likelihood kernel for these terms "
               "(sorted kernel codes, at most %d states)", NB_GPS_MAX_STATES);
  return NB_ERR_ARG;
}
