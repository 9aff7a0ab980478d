// Poisson likelihood of BINNED COUNTS behind a RESPONSE MATRIX in one kernel
// (the user-side likelihood callable of reference sampler.py:863-873 for a
// model prediction s(theta) of K source-space quantities that an instrument
// response or a set of templates R maps onto P bins with observed counts k):
//     mu_ij = e_j sum_k R_jk s_ik + b_j,     log L_i = C - sum_j D(mu_ij, k_j),
// D, the two flags and the one-log trick those of nb_poisson_term.h.  A GEMM
// fused with the deviance: the n x P matrix of the mu is never stored (at
// n = 65 536 and P = 4096 it would be 2 GiB written and read back).
//
// Work per point 2 P K flop on the matrix cores and about 100 P vector
// instructions (the log), traffic 8 K bytes read + 8 written.  The blocking
// is the panel driver's (nb_panel.h) with A = R, zero padded in both
// directions, and x = the source values s.  Its own:
//  * every (panel, k-tile) pair is dense; the slice of s is read again for
//    every panel (from L2: a block's source rows are 8 K TPW 16 bytes);
//  * when a panel's k range ends, po_term turns an accumulator into D(e_j acc
//    + b_j, k_j) with k, 1 / k, e, b of the lane's bins from the device table
//    (requested before the chunk's matrix work starts); a bin past P adds
//    neither a term nor a flag.  The terms go into the per-lane partial and
//    the flags into the per-lane word of each point.
// A NON-FINITE source value s_ik makes row i NaN and changes no other row:
// every bin j < P multiplies it by the finite R_jk, which gives NaN (R_jk = 0,
// or a NaN to begin with) or an infinity; the sum over k is then NaN or
// infinite, so is mu_ij (e_j > 0 is finite), and both set PO_NAN in po_term
// (mu >= 0 && mu < inf is false).  There is at least one bin (P >= 1) and the
// padding rows of R meet masked bins only, so no separate poison term is
// needed, unlike in nb_chi2_kernel, where the zeros above the diagonal are
// skipped.  A finite sum that overflows is NaN by the same rule, as in the
// numpy twin.
#include "nb_common.h"
#include "nb_launch.h"
#include "nb_panel.h"
#include "nb_poisson_term.h"

namespace {

struct fold_policy {
  static constexpr bool FLAGS = true;
  // k, 1 / k, e, b of the lane's bins: [row tile][register]
  struct table { double k[2][4], ik[2][4], e[2][4], b[2][4]; };
  const nb_gd *tk, *tik, *te, *tb;               // 16 dt doubles each
  int n_data, nkt;
  double log_const;

  __device__ __forceinline__ int k_tiles(int, int) const { return nkt; }
  __device__ __forceinline__ bool takes_part(int, int) const { return true; }
  __device__ __forceinline__ void request(int, int) const {}
  __device__ __forceinline__ double staged(int, double s, bool inside) const {
    // a padding column is an exact zero, never a repeated load: it meets
    // zeros of R only
    return inside ? s : 0.0;
  }
  // the table is padded to whole tiles
  __device__ __forceinline__ table prefetch(const int (&row0)[2],
                                            const bool (&in)[2]) const {
    table t;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int bin = in[j] ? row0[j] + 4 * r : 0;
        t.k[j][r] = tk[bin];
        t.ik[j][r] = tik[bin];
        t.e[j][r] = te[bin];
        t.b[j][r] = tb[bin];
      }
    return t;
  }
  template <int TPW>
  __device__ __forceinline__ void fold(const nb_d4 (&acc)[2][TPW],
                                       double (&part)[TPW],
                                       unsigned (&flag)[TPW], const table& t,
                                       const int (&row0)[2],
                                       const bool (&in)[2]) const {
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (in[j]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool live = row0[j] + 4 * r < n_data;
#pragma unroll
          for (int p = 0; p < TPW; ++p) {
            unsigned f = 0u;
            const double d = po_term(acc[j][p][r], t.k[j][r], t.ik[j][r],
                                     t.e[j][r], t.b[j][r], &f);
            part[p] += live ? d : 0.0;
            flag[p] |= live ? f : 0u;
          }
        }
      }
  }
  __device__ __forceinline__ void publish(int, int) const {}
  __device__ __forceinline__ double result(double v, unsigned f, int) const {
    double res = log_const - v;
    if (f & PO_NEG_INF) res = -__builtin_inf();
    if (f & PO_NAN) res = __builtin_nan("");
    return res;
  }
};

// blob: k, 1 / k, e, b, each padded to 16 DT doubles (nb_fold_r_offset), then
// the operand tiles of R, every k-tile of every panel (nb_layout.h).  src: n
// rows of n_src doubles, ld doubles apart.
template <int TPW>
__global__ void __launch_bounds__(64 * NB_PANEL_WAVES)
nb_fold_poisson_kernel(const double* __restrict__ blob, int n_data, int n_src,
                       const double* __restrict__ src, long long ld,
                       long long n, double log_const,
                       double* __restrict__ out) {
  const int dt = (n_data + 15) >> 4;
  const nb_gd* tab = (const nb_gd*)blob;
  const fold_policy pol{tab, tab + 16 * (size_t)dt, tab + 32 * (size_t)dt,
                        tab + 48 * (size_t)dt, n_data, (n_src + 15) >> 4,
                        log_const};
  nb_panel_rows<TPW>(pol, tab + nb_fold_r_offset(dt), dt, (const nb_gd*)src,
                     n_src, ld, n, out);
}

}  // namespace

int nb_launch_fold_poisson(const double* blob, int n_data, int n_src,
                           const double* src, long long ld, long long n,
                           double log_const, double* out, hipStream_t stream) {
  if (n <= 0) return NB_OK;
  // the larger block of points once it still gives each of the 256 CUs a
  // workgroup (a slice of R staged in LDS then serves twice the points); the
  // bits of a row are the same in both
  if (n >= 256 * 64)
    return nb_panel_launch<4>(nb_fold_poisson_kernel<4>, n, stream, blob,
                              n_data, n_src, src, ld, n, log_const, out);
  return nb_panel_launch<2>(nb_fold_poisson_kernel<2>, n, stream, blob, n_data,
                            n_src, src, ld, n, log_const, out);
}
