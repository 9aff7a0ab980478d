// |B_inv (x - c)|^2 of 16-point tiles against a lower-triangular matrix held
// in LDS as K-permuted 16x16 operand tiles: the matrix-core contraction
// shared by the streaming ellipsoid test (nb_stream.hip, whose header
// describes the layout) and the Gaussian-mixture likelihood (nb_mixture.hip).
#pragma once
#include "nb_common.h"

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

namespace {

// |B_inv (x - c)|^2 contributions of one group of TPW tiles: d holds the
// centred inputs in the permuted K order.  Work is trimmed to the real
// dimension: k-steps beyond ceil(n_dim / 4) hold only zero padding and are
// skipped, and a last row tile with at most 4 real rows (n_dim mod 16 in
// 1..4, e.g. D = 50 or 20) runs on v_mfma_f64_4x4x4_4b_f64 -- 16 instead of 64
// cycles per k-step (A lane i + 4b + 16k, B lane p + 16k, D lane p + 16i; the
// A operand is gathered from the same tile storage).  At D = 50 that removes
// a third of the matrix cycles of a kernel that sits at the ridge between
// the HBM and the fp64 MFMA roof.
#define MFMA4(a, b, c) __builtin_amdgcn_mfma_f64_4x4x4f64((a), (b), (c), 0, 0, 0)

// KL = number of k-steps that hold real features (the K permutation pairs
// k-steps: 2j, 2j+1 cover features 8j .. 8j+7, so KL = 2 ceil(n_dim / 8));
// SMALL = the last row tile has at most 4 real rows.  Both are compile-time
// so that the MFMA sequences stay branch free.
template <int DT, int TPW, int KL, bool SMALL>
__device__ __forceinline__ void stream_quadform(const double* wl, int n_dim,
                                                int lane,
                                                const double (&d)[TPW][4 * DT],
                                                double (&part)[TPW]) {
#pragma unroll
  for (int t = 0; t < TPW; ++t) part[t] = 0.0;
#pragma unroll
  for (int ht = 0; ht < DT; ++ht) {
    const int ks_n = (4 * (ht + 1) < KL) ? 4 * (ht + 1) : KL;   // lower-tri
    // (always true; the run-time test keeps the row tiles in separate basic
    // blocks -- merged, the scheduler hoists every operand read and the kernel
    // spills 220 registers)
    if (16 * ht >= n_dim) continue;
    if (SMALL && ht == DT - 1) {
      double r[TPW];
#pragma unroll
      for (int t = 0; t < TPW; ++t) r[t] = 0.0;
      const int roff = (lane >> 4) * 16 + (lane & 3);
#pragma unroll
      for (int ks = 0; ks < 4 * DT; ++ks) {
        if (ks < ks_n) {
          const int kt = ks >> 2, s = ks & 3;
          const double a =
              wl[((ht * (ht + 1)) / 2 + kt) * NB_TILE + s * 64 + roff];
#pragma unroll
          for (int t = 0; t < TPW; ++t) r[t] = MFMA4(a, d[t][ks], r[t]);
        }
      }
#pragma unroll
      for (int t = 0; t < TPW; ++t) part[t] = fma(r[t], r[t], part[t]);
    } else {
      nb_d4 acc[TPW];
#pragma unroll
      for (int t = 0; t < TPW; ++t) acc[t] = nb_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < 4 * DT; ++ks) {
        if (ks < ks_n) {
          const int kt = ks >> 2, s = ks & 3;
          const double a =
              wl[((ht * (ht + 1)) / 2 + kt) * NB_TILE + s * 64 + lane];
#pragma unroll
          for (int t = 0; t < TPW; ++t) acc[t] = MFMA(a, d[t][ks], acc[t]);
        }
      }
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          part[t] = fma(acc[t][r], acc[t][r], part[t]);
    }
  }
}

// The same with the A operands read AHEAD of their MFMAs: left to the
// scheduler every LDS read sits directly in front of its first MFMA, and with
// one or two tiles per wavefront (n_dim > 64) an operand feeds 64-128 cycles
// of matrix work behind ~120 cycles of exposed LDS latency.  The k-steps go
// in chunks of four; the reads of a chunk are issued in front of the MFMAs of
// the chunk before it (256-512 cycles of cover, eight more registers) and
// pinned there by scheduling barriers.
template <int DT, int TPW, int KL, bool SMALL>
__device__ __forceinline__ void stream_quadform_ahead(
    const double* wl, int lane, const double (&d)[TPW][4 * DT],
    double (&part)[TPW]) {
  double a[DT][4 * DT];
  auto read_chunk = [&](int ht, int c) __attribute__((always_inline)) {
    const int ks_n = (4 * (ht + 1) < KL) ? 4 * (ht + 1) : KL;
    // (a last row tile of at most 4 rows: the A operand of the 4x4x4 tile)
    const int off = (SMALL && ht == DT - 1)
                        ? (lane >> 4) * 16 + (lane & 3) : lane;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (4 * c + s < ks_n)
        a[ht][4 * c + s] =
            wl[((ht * (ht + 1)) / 2 + c) * NB_TILE + s * 64 + off];
  };
#pragma unroll
  for (int t = 0; t < TPW; ++t) part[t] = 0.0;
  read_chunk(0, 0);
#pragma unroll
  for (int ht = 0; ht < DT; ++ht) {
    const int ks_n = (4 * (ht + 1) < KL) ? 4 * (ht + 1) : KL;
    const int n_c = (ks_n + 3) / 4;
    if (SMALL && ht == DT - 1) {
      // 4x4x4 tiles (16 instead of 64 cycles per k-step); even and odd
      // k-steps in accumulators of their own: with one or two tiles per
      // wavefront a single chain waits for its own results
      double r[TPW][2];
#pragma unroll
      for (int t = 0; t < TPW; ++t) r[t][0] = r[t][1] = 0.0;
#pragma unroll
      for (int c = 0; c < DT; ++c) {
        if (c < n_c) {
          if (c + 1 < n_c) read_chunk(ht, c + 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int s = 0; s < 4; ++s)
            if (4 * c + s < ks_n) {
#pragma unroll
              for (int t = 0; t < TPW; ++t)
                r[t][s & 1] = MFMA4(a[ht][4 * c + s], d[t][4 * c + s],
                                    r[t][s & 1]);
            }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        const double y = r[t][0] + r[t][1];
        part[t] = fma(y, y, part[t]);
      }
    } else {
      nb_d4 acc[TPW];
#pragma unroll
      for (int t = 0; t < TPW; ++t) acc[t] = nb_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int c = 0; c < DT; ++c) {
        if (c < n_c) {
          if (c + 1 < n_c) read_chunk(ht, c + 1);
          else if (ht + 1 < DT) read_chunk(ht + 1, 0);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int s = 0; s < 4; ++s)
            if (4 * c + s < ks_n) {
#pragma unroll
              for (int t = 0; t < TPW; ++t)
                acc[t] = MFMA(a[ht][4 * c + s], d[t][4 * c + s], acc[t]);
            }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          part[t] = fma(acc[t][r], acc[t][r], part[t]);
    }
  }
}

}  // namespace
