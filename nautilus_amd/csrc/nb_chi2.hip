// Gaussian likelihood of a DATA VECTOR in one kernel (the user-side likelihood
// callable of reference sampler.py:863-873 for a model prediction m(theta) of
// P data points d with covariance C = L L^T):
//     log L = log_norm - 1/2 |W (m - d)|^2,   W = L^-1 lower triangular,
// P up to NB_CHI2_MAX_DATA = 4096 -- far beyond the register-resident tiles of
// nb_quadform.h (n_dim <= 128).  A triangular GEMM fused with a row norm: the
// n x P product is never stored.
//
// Algorithmic work n P (P + 16) flop, traffic 8 P bytes read + 8 written per
// point.  The blocking is the panel driver's (nb_panel.h) with A = W and x =
// the residuals r = m - d, formed on the fly from the model rows.  Its own:
//  * k-tiles above the diagonal are neither stored, staged nor multiplied: a
//    panel's k range ends at its last row tile, and inside the panel a
//    wavefront skips the chunks above its own row tile;
//  * when a panel's k range ends, the squares of its accumulators are folded
//    into the per-lane partial of each point.
// A non-finite residual poisons its point explicitly (r * 0 added to the
// sum): +inf against the exact zeros of the diagonal tiles alone would give
// NaN or inf depending on the column it sits in.
//
// The diagonal case (sigma) is a separate memory-bound kernel below.
#include "nb_common.h"
#include "nb_launch.h"
#include "nb_panel.h"

namespace {

struct chi2_policy {
  static constexpr bool FLAGS = false;
  struct table {};
  const nb_gd* d;                                // zero padded to whole tiles
  double* bad;                                   // LDS: a point's 0 or NaN
  double log_norm;
  double poison = 0.0, dv[4];

  __device__ __forceinline__ int k_tiles(int panel, int nrt) const {
    return NB_PANEL_TILES * panel + nrt;
  }
  __device__ __forceinline__ bool takes_part(int rt, int kt) const {
    return kt <= rt;
  }
  __device__ __forceinline__ void request(int e, int col) { dv[e] = d[col]; }
  __device__ __forceinline__ double staged(int e, double m, bool inside) {
    // a padding column is an exact zero: it meets zeros of W only
    const double r = inside ? m - dv[e] : 0.0;
    poison = fma(r, 0.0, poison);
    return r;
  }
  __device__ __forceinline__ table prefetch(const int (&)[2],
                                            const bool (&)[2]) const {
    return {};
  }
  template <int TPW>
  __device__ __forceinline__ void fold(const nb_d4 (&acc)[2][TPW],
                                       double (&part)[TPW], unsigned (&)[TPW],
                                       const table&, const int (&)[2],
                                       const bool (&)[2]) const {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          part[t] = fma(acc[j][t][r], acc[j][t][r], part[t]);
  }
  __device__ __forceinline__ void publish(int sp, int sq) {
    poison += __shfl_xor(poison, 1);
    poison += __shfl_xor(poison, 2);
    if (sq == 0) bad[sp] = poison;
  }
  __device__ __forceinline__ double result(double chi2, unsigned,
                                           int p) const {
    return fma(-0.5, chi2 + bad[p], log_norm);
  }
};

// blob: d zero padded to 16 DT doubles (nb_chi2_w_offset), then the operand
// tiles of W, k-tiles 0 .. the panel's last row tile (nb_layout.h).  model: n
// rows of n_data doubles, ld doubles apart.
template <int TPW>
__global__ void __launch_bounds__(64 * NB_PANEL_WAVES)
nb_chi2_kernel(const double* __restrict__ blob, int n_data,
               const double* __restrict__ model, long long ld, long long n,
               double log_norm, double* __restrict__ out) {
  __shared__ double bad[16 * TPW];
  const int dt = (n_data + 15) >> 4;
  const nb_gd* dpad = (const nb_gd*)blob;
  chi2_policy pol{dpad, bad, log_norm};
  nb_panel_rows<TPW>(pol, dpad + nb_chi2_w_offset(dt), dt,
                     (const nb_gd*)model, n_data, ld, n, out);
}

// Diagonal covariance: log L = log_norm - 1/2 sum_k ((m_k - d_k) / sigma_k)^2.
// Memory bound (8 P bytes per point, read once): 16 lanes share a row, every
// load instruction of a wavefront covers 4 rows x 128 contiguous bytes, four
// loads in flight per lane with a partial sum each; the partials are added
// as (0 + 1) + (2 + 3), then over the 16 lanes by shuffles -- a fixed order
// per row.  blob: d [P], then 1 / sigma [P].
__global__ void __launch_bounds__(256)
nb_chi2_diag_kernel(const double* __restrict__ blob, int n_data,
                    const double* __restrict__ model, long long ld,
                    long long n, double log_norm, double* __restrict__ out) {
  const int sub = threadIdx.x & 15;
  const double* d = blob;
  const double* is = blob + n_data;
  const long long stride = (long long)gridDim.x * (blockDim.x >> 4);
  for (long long p = (long long)blockIdx.x * (blockDim.x >> 4) +
                     (threadIdx.x >> 4);
       p < n; p += stride) {
    const double* row = model + p * ld;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    double poison = 0.0;
    for (int i = sub; i < n_data; i += 64) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = i + 16 * u;
        if (k < n_data) {
          const double t = (row[k] - d[k]) * is[k];
          a[u] = fma(t, t, a[u]);
          poison = fma(t, 0.0, poison);          // non-finite -> NaN
        }
      }
    }
    double v = ((a[0] + a[1]) + (a[2] + a[3])) + poison;
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    if (sub == 0) out[p] = fma(-0.5, v, log_norm);
  }
}

}  // namespace

int nb_launch_chi2(const double* blob, int n_data, const double* model,
                   long long ld, long long n, double log_norm, double* out,
                   hipStream_t stream) {
  if (n <= 0) return NB_OK;
  // the largest block of points that gives each of the 256 CUs a workgroup
  // (a slice of W staged in LDS then serves the most points); the bits of a
  // row are the same in all three
  if (n >= 256 * 128)
    return nb_panel_launch<8>(nb_chi2_kernel<8>, n, stream, blob, n_data,
                              model, ld, n, log_norm, out);
  if (n >= 256 * 64)
    return nb_panel_launch<4>(nb_chi2_kernel<4>, n, stream, blob, n_data,
                              model, ld, n, log_norm, out);
  return nb_panel_launch<2>(nb_chi2_kernel<2>, n, stream, blob, n_data, model,
                            ld, n, log_norm, out);
}

int nb_launch_chi2_diag(const double* blob, int n_data, const double* model,
                        long long ld, long long n, double log_norm,
                        double* out, hipStream_t stream) {
  if (n <= 0) return NB_OK;
  long long b = (n + 15) / 16;
  if (b > 8192) b = 8192;
  (void)hipGetLastError();
  hipLaunchKernelGGL(nb_chi2_diag_kernel, dim3((unsigned)b), dim3(256), 0,
                     stream, blob, n_data, model, ld, n, log_norm, out);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}
