// What nb_gps.hip (one kernel term) and nb_gps_terms.hip (a sum of two or
// three) share: the transition Phi of a term and the staging of the model
// output m through LDS.
//
// m is (n, P) row-major and a lane owns a row, so the lanes' reads would be ld
// doubles apart: a block of 64 rows x NB_GPS_BLOCK columns is staged through
// LDS with 16-byte loads that run along the rows (pairs of doubles at
// 8-byte-aligned addresses, nb_d2u) and an odd row stride in doubles, so that
// the column-wise reads of the recursion fall on distinct banks.  The next
// block's loads are issued into registers (gps_request) before the recursion
// over the current block starts and are written to LDS (gps_stage) after it:
// they are in flight for NB_GPS_BLOCK steps.
#pragma once
#include "nb_common.h"
#include "nb_layout.h"

namespace {

constexpr int GPS_C = NB_GPS_BLOCK;              // columns of a staged block
constexpr int GPS_LS = GPS_C + 1;                // LDS row stride, odd
constexpr int GPS_LOADS = GPS_C / 2;             // 16-byte loads per lane
constexpr int GPS_RENORM = 256;                  // steps between two frexp
static_assert(GPS_C % 2 == 0 && 64 % GPS_LOADS == 0, "whole rows per load");

constexpr int gps_states(int kernel) {
  return kernel == NB_GPS_EXP ? 1 : kernel == NB_GPS_MATERN52 ? 3 : 2;
}

// what a row keeps of the hyper-parameters of a term
struct gps_row {
  double a, s, inv_l;
  double w, eta, inv_eta;                        // sho: 1 / (2 q), eta, 1 / eta
};

// Phi(x) at r = dt / l, capped as gp_rho caps it (beyond 1e4 every exponential
// here is 0 in float64, and the cap keeps an infinite r from meeting that 0;
// it also bounds the argument of the sine)
template <int KERNEL, int R>
__device__ __forceinline__ void gps_phi(const gps_row& h, double dt,
                                        double (&phi)[R][R]) {
#pragma clang fp contract(off)
  const double r = fmin(dt * h.inv_l, 1e4);
  if constexpr (KERNEL == NB_GPS_EXP) {
    phi[0][0] = exp(-r);
  } else if constexpr (KERNEL == NB_GPS_MATERN32) {
    const double x = 0x1.bb67ae8584caap+0 * r;              // sqrt(3) r
    const double e = exp(-x);
    const double ex = e * x;
    phi[0][0] = e * (1.0 + x);
    phi[0][1] = ex;
    phi[1][0] = -ex;
    phi[1][1] = e * (1.0 - x);
  } else if constexpr (KERNEL == NB_GPS_MATERN52) {
    const double x = 0x1.1e3779b97f4a8p+1 * r;              // sqrt(5) r
    const double e = exp(-x);
    const double x2 = x * x;
    const double hx = 0.5 * x2;
    phi[0][0] = e * ((1.0 + x) + hx);
    phi[0][1] = e * (x + x2);
    phi[0][2] = e * hx;
    phi[1][0] = -(e * hx);
    phi[1][1] = e * ((1.0 + x) - x2);
    phi[1][2] = e * (x - hx);
    phi[2][0] = e * (hx - x);
    phi[2][1] = e * (x2 - 3.0 * x);
    phi[2][2] = e * ((1.0 - 2.0 * x) + hx);
  } else {
    const double e = exp(-(r * h.w));
    const double arg = h.eta * r;                // in [0, 1e4]
    double sn, c;
    sincos(arg, &sn, &c);
    const double sg = sn * h.inv_eta;
    const double sw = sg * h.w;
    const double es = e * sg;
    phi[0][0] = e * (c + sw);
    phi[0][1] = es;
    phi[1][0] = -es;
    phi[1][1] = e * (c - sw);
  }
}

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

}  // namespace
