// Gaussian-process likelihood of P <= 128 measurements whose full covariance
// depends on the point (the user-side likelihood callable of reference
// sampler.py:863-873 for a model prediction m(theta) under correlated noise
// with free kernel hyper-parameters):
//     log L = log_norm - 1/2 [ r^T K^-1 r + log det K ],   r = m - d,
//     NB_GP_HYPER  K[j,k] = a rho(dist[j,k] / l) + delta_jk (sigma_j^2 + s),
//     NB_GP_FULL   K = C + diag(sigma^2), the lower triangle of C from memory.
// One workgroup per point, templated on the tile count T = ceil(P / 16), with
// nb_gp_waves(T) wavefronts.  K lives in LDS as the T (T + 1) / 2 tiles of its
// lower triangle (nb_layout.h: tile (ti, tj) column-major, so that a k-step of
// an fp64 MFMA operand and the 16 rows of a column are both 64 resp. 16
// contiguous doubles, free of bank conflicts) and is never stored anywhere
// else.  Rows and columns from P on are a unit diagonal: they factorise to
// themselves, add log 1 = 0 and carry a zero residual.
//
// Blocked Cholesky with 16-wide panels, left-looking for the matrix and
// right-looking for the residual.  For panel k:
//  A. the tiles (ti, k), ti >= k, one per wavefront in turn, subtract
//     sum_{m < k} L(ti, m) L(k, m)^T on v_mfma_f64_16x16x4 -- 4 k instructions
//     into one accumulator, m and the k-steps ascending; the operands are
//     swapped (A = -L(k, m), B = L(ti, m)) so that the accumulator's lane map
//     is the tile's own storage order: a tile is read and written once per
//     panel, not once per earlier panel as a right-looking update would;
//  B. wavefront 0 factorises the diagonal tile, a row per lane in registers,
//     the column of the pivot passed round by v_readlane; a pivot is tested
//     for (0, +inf) before its square root;
//  C. a thread per row below, and one more for the residual's segment, solves
//     x L(k, k)^T = a by substitution (the extra row of the factor of
//     [[K, r], [r^T, .]] is y^T = (L^-1 r)^T); then every row thread takes
//     its row's product with the panel's y off the residual below.
// At the end wavefront 0 adds y_j^2 + log pivot_j over the rows, a fixed
// tree.  Nothing is split across workgroups and there are no atomics: the
// bits of a row depend on P, the kernel, the mode and its own inputs only.
// A bad input or pivot sets a flag that overrides the result with NaN; the
// workgroup runs to the end regardless.
#include "../../include/nautilus_hip.h"          // NB_GP_*
#include "nb_common.h"
#include "nb_launch.h"

#define GP_MFMA(a, b, c) \
  __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

namespace {

// the value lane l holds (l the same for every lane)
__device__ __forceinline__ double gp_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ bool gp_finite(double v) {
  return fabs(v) < __builtin_inf();              // false for NaN
}

// rho(x), x = dist / l >= 0; beyond 1e4 every kernel is 0 in float64, and the
// clamp keeps an infinite x from meeting the 0 of its own exponential
__device__ __forceinline__ double gp_rho(int kernel, double x) {
#pragma clang fp contract(off)
  x = fmin(x, 1e4);
  switch (kernel) {
    case NB_GP_SQEXP:
      return exp(-0.5 * (x * x));
    case NB_GP_EXP:
      return exp(-x);
    case NB_GP_MATERN32: {
      const double u = 0x1.bb67ae8584caap+0 * x;            // sqrt(3) x
      return (1.0 + u) * exp(-u);
    }
    default: {
      const double u = 0x1.1e3779b97f4a8p+1 * x;            // sqrt(5) x
      return ((1.0 + u) + (u * u) * 0x1.5555555555555p-2) * exp(-u);
    }
  }
}

// tile row of tile number t of the lower triangle (nb_gp_tile)
__device__ __forceinline__ int gp_tile_row(int t) {
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  return ti;
}

// tab: d [16 T], sigma^2 [16 T], distance tiles.  model: n rows of n_data
// doubles, ld doubles apart.  cov: hyper mode n rows of 3 doubles (a, l, s),
// full mode n rows of n_data * n_data doubles, ld_cov doubles apart.
template <int T, int MODE>
__global__ void __launch_bounds__(64 * nb_gp_waves(T))
nb_gp_kernel(const double* __restrict__ tab, int n_data, int kernel,
             const double* __restrict__ model, long long ld,
             const double* __restrict__ cov, long long ld_cov, long long n,
             double log_norm, double* __restrict__ out) {
  constexpr int W = nb_gp_waves(T);
  constexpr int NT = 64 * W;
  constexpr int PP = 16 * T;
  constexpr int NTILES = nb_gp_tiles(T);
  extern __shared__ double gp_lds[];
  double* kt = gp_lds;                           // the tiles of K, then of L
  double* res = kt + NTILES * NB_TILE;           // r, then y      [PP]
  double* piv = res + PP;                        // the pivots     [PP]
  double* yk = piv + PP;                         // y of a panel   [16]
  double* rinv = yk + 16;                        // 1 / l_jj of a panel [16]
  int* flag = (int*)(rinv + 16);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const double* sig2 = tab + PP;
  const double* dist = tab + nb_gp_dist_offset(T);

  for (long long i = blockIdx.x; i < n; i += gridDim.x) {
    __syncthreads();                             // the last point is read out
    if (tid == 0) *flag = 0;
    __syncthreads();

    // ---- fill ------------------------------------------------------------
    bool bad = false;
    for (int j = tid; j < PP; j += NT) {
      double r = 0.0;
      if (j < n_data) {
        const double m = model[i * ld + j];
        bad |= !gp_finite(m);
        r = m - tab[j];
      }
      res[j] = r;
    }
    if constexpr (MODE == NB_GP_HYPER) {
#pragma clang fp contract(off)
      const double* h = cov + i * ld_cov;
      const double a = h[0], l = h[1], s = h[2];
      bad |= !(a >= 0.0 && a < __builtin_inf()) ||
             !(l > 0.0 && l < __builtin_inf()) ||
             !(s >= 0.0 && s < __builtin_inf());
      const double inv_l = 1.0 / l;
      for (int e = tid; e < NTILES * NB_TILE; e += NT) {
        const int t = e >> 8;
        const int ti = gp_tile_row(t);
        const int tj = t - ti * (ti + 1) / 2;
        const int row = 16 * ti + (e & 15);
        const int col = 16 * tj + ((e >> 4) & 15);
        double v;
        if (col > row)
          v = 0.0;
        else if (row >= n_data)
          v = row == col ? 1.0 : 0.0;
        else if (row == col)
          v = a + (sig2[row] + s);
        else
          v = a * gp_rho(kernel, dist[e] * inv_l);
        kt[e] = v;
      }
    } else {
      const double* c = cov + i * ld_cov;
      // pairs of doubles where every pair of a row is 16-byte aligned
      const bool wide = (n_data & 1) == 0 && (ld_cov & 1) == 0 &&
                        ((unsigned long long)cov & 15ull) == 0ull;
      for (int e = tid; e < NTILES * 64; e += NT) {
        const int t = e >> 6;
        const int ti = gp_tile_row(t);
        const int tj = t - ti * (ti + 1) / 2;
        const int r = e & 15;
        const int c0 = 4 * ((e >> 4) & 3);
        const int row = 16 * ti + r;
        const int col0 = 16 * tj + c0;
        double x[4] = {0.0, 0.0, 0.0, 0.0};
        if (row < n_data && col0 <= row) {
          const double* src = c + (long long)row * n_data + col0;
          if (wide) {
            const double2 p0 = *(const double2*)src;         // col0 + 1 < P
            x[0] = p0.x;
            x[1] = p0.y;
            if (col0 + 2 <= row) {
              const double2 p1 = *(const double2*)(src + 2);
              x[2] = p1.x;
              x[3] = p1.y;
            }
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (col0 + q <= row) x[q] = src[q];
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int col = col0 + q;
          const bool in = row < n_data && col <= row;
          bad |= in && !gp_finite(x[q]);
          double v;
          if (in)
            v = row == col ? x[q] + sig2[row] : x[q];
          else
            v = row == col ? 1.0 : 0.0;
          kt[t * NB_TILE + nb_gp_index(r, c0 + q)] = v;
        }
      }
    }
    if (bad) *flag = 1;
    __syncthreads();

    // ---- factorisation -----------------------------------------------------
#pragma unroll 1
    for (int k = 0; k < T; ++k) {
      // A: tile (ti, k) -= sum_{m < k} L(ti, m) L(k, m)^T
      if (k > 0) {
        for (int ti = k + wave; ti < T; ti += W) {
          double* tile = kt + nb_gp_tile(ti, k) * NB_TILE;
          nb_d4 acc;
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] = tile[64 * r + lane];
          for (int m = 0; m < k; ++m) {
            const double* pa = kt + nb_gp_tile(k, m) * NB_TILE;
            const double* pb = kt + nb_gp_tile(ti, m) * NB_TILE;
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
              acc = GP_MFMA(-pa[64 * s4 + lane], pb[64 * s4 + lane], acc);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) tile[64 * r + lane] = acc[r];
        }
        __syncthreads();
      }

      // B: the diagonal tile, a row per lane of wavefront 0
      if (wave == 0) {
        double* tile = kt + nb_gp_tile(k, k) * NB_TILE;
        const int row = lane & 15;
        double a[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) a[c] = tile[nb_gp_index(row, c)];
        bool badp = false;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const double d = gp_readlane(a[j], j);
          badp |= !(d > 0.0 && d < __builtin_inf());
          const double ljj = sqrt(d);
          const double ri = 1.0 / ljj;
          a[j] = row == j ? ljj : a[j] * ri;
          if (lane == 0) {
            piv[16 * k + j] = d;
            rinv[j] = ri;
          }
#pragma unroll
          for (int c = j + 1; c < 16; ++c)
            a[c] = fma(-a[j], gp_readlane(a[j], c), a[c]);
        }
        if (lane < 16) {
#pragma unroll
          for (int c = 0; c < 16; ++c)
            tile[nb_gp_index(row, c)] = c <= row ? a[c] : 0.0;
        }
        if (badp && lane == 0) *flag = 1;
      }
      __syncthreads();

      // C: the rows below and the residual's segment against L(k, k)
      const int n_rows = 16 * (T - 1 - k);
      double x[16];
      double* dst = nullptr;                     // row of a tile, stride 16
      if (tid < n_rows)
        dst = kt + nb_gp_tile(k + 1 + (tid >> 4), k) * NB_TILE + (tid & 15);
      if (tid <= n_rows) {
        const double* lkk = kt + nb_gp_tile(k, k) * NB_TILE;
#pragma unroll
        for (int c = 0; c < 16; ++c)
          x[c] = dst != nullptr ? dst[16 * c] : res[16 * k + c];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          double sum = x[j];
#pragma unroll
          for (int m = 0; m < j; ++m)
            sum = fma(-x[m], lkk[nb_gp_index(j, m)], sum);
          x[j] = sum * rinv[j];
        }
        if (dst != nullptr) {
#pragma unroll
          for (int c = 0; c < 16; ++c) dst[16 * c] = x[c];
        } else {
#pragma unroll
          for (int c = 0; c < 16; ++c) {
            yk[c] = x[c];
            res[16 * k + c] = x[c];
          }
        }
      }
      __syncthreads();
      if (tid < n_rows) {
        double v = res[16 * (k + 1) + tid];
#pragma unroll
        for (int c = 0; c < 16; ++c) v = fma(-x[c], yk[c], v);
        res[16 * (k + 1) + tid] = v;
      }
    }
    __syncthreads();

    // ---- |y|^2 + log det K -------------------------------------------------
    if (wave == 0) {
#pragma clang fp contract(off)
      double v = 0.0;
      if (lane < PP) v = res[lane] * res[lane] + log(piv[lane]);
      if constexpr (PP > 64) {
        double v1 = 0.0;
        if (lane + 64 < PP)
          v1 = res[lane + 64] * res[lane + 64] + log(piv[lane + 64]);
        v = v + v1;
      }
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
      double result = log_norm - 0.5 * v;
      if (*flag != 0) result = __builtin_nan("");
      if (lane == 0) out[i] = result;
    }
  }
}

template <int T, int MODE>
int launch(const double* tab, int n_data, int kernel, const double* model,
           long long ld, const double* cov, long long ld_cov, long long n,
           double log_norm, double* out, hipStream_t stream) {
  const size_t lds = nb_gp_lds_doubles(T) * sizeof(double);
  if (const int rc = nb_allow_lds<nb_gp_kernel<T, MODE>>(lds)) return rc;
  const long long b = n < (1ll << 20) ? n : (1ll << 20);
  (void)hipGetLastError();
  hipLaunchKernelGGL((nb_gp_kernel<T, MODE>), dim3((unsigned)b),
                     dim3(64 * nb_gp_waves(T)), lds, stream, tab, n_data,
                     kernel, model, ld, cov, ld_cov, n, log_norm, out);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}

template <int MODE>
int launch_mode(const double* tab, int n_data, int kernel,
                const double* model, long long ld, const double* cov,
                long long ld_cov, long long n, double log_norm, double* out,
                hipStream_t stream) {
  if (n_data < 1 || n_data > NB_GP_MAX_DATA) {
    nb_set_error("Gaussian-process likelihood: n_data %d outside 1..%d", n_data,
                 NB_GP_MAX_DATA);
    return NB_ERR_ARG;
  }
  return nb_tile_dispatch((n_data + 15) / 16, [&](auto t) {
    return launch<t(), MODE>(tab, n_data, kernel, model, ld, cov, ld_cov, n,
                             log_norm, out, stream);
  });
}

}  // namespace

int nb_launch_gp(const double* tab, int n_data, int kernel, int mode,
                 const double* model, long long ld, const double* cov,
                 long long ld_cov, long long n, double log_norm, double* out,
                 hipStream_t stream) {
  if (n <= 0) return NB_OK;
  if (mode == NB_GP_FULL)
    return launch_mode<NB_GP_FULL>(tab, n_data, kernel, model, ld, cov, ld_cov,
                                   n, log_norm, out, stream);
  return launch_mode<NB_GP_HYPER>(tab, n_data, kernel, model, ld, cov, ld_cov,
                                  n, log_norm, out, stream);
}
