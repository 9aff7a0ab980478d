// Ellipsoid-frame coordinates and input standardisation for the emulator's
// training set (reference nautilus/bounds/basic.py:340 Ellipsoid.transform,
// nautilus/neural.py:74-77 mean / scale / (x - mean) / scale).  The transform
// runs through the same matrix-core tile code as contains() and the emulator
// evaluation (nb_tile.h), so the network is trained on exactly the inputs it
// later sees inside nb_eval_fast_kernel.
#include "nb_tile.h"
#include "nb_launch.h"
#include "../../include/nautilus_hip.h"

namespace {

template <int DT>
__global__ void __launch_bounds__(256)
nb_transform_kernel(const double* __restrict__ blk, int n_dim,
                    const double* __restrict__ x, long long n,
                    double* __restrict__ y_out) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lg = lane >> 4;
  const long long n_tiles = (n + 15) / 16;
  for (long long tile = (long long)blockIdx.x * 4 + wave; tile < n_tiles;
       tile += (long long)gridDim.x * 4) {
    long long pt[1] = {tile * 16 + (lane & 15)};
    bool valid[1] = {pt[0] < n};
    double xin[1][4 * DT], y[1][4 * DT], r2[1];
    bool box_bad[1];
    load_points<DT, 1>((const nb_gd*)x, pt, valid, n_dim, n, lane, xin);
    ell_eval<DT, 1>(blk, n_dim, xin, lane, y, box_bad, r2);
    if (valid[0]) {
#pragma unroll
      for (int j = 0; j < 4 * DT; ++j) {
        const int unit = 4 * j + lg;          // C/D layout of the MFMA
        if (unit < n_dim) y_out[pt[0] * n_dim + unit] = y[0][j];
      }
    }
  }
}

// per-column mean and population standard deviation (two passes, fixed
// reduction order), one workgroup per column.  The first pass gives the mean
// to the rounding of a sum of n terms, a few ulp OF THE MEAN.  In a column
// that lies far from zero (mean 1e6, spread 1) that is 1e-10 of the spread,
// and nb_standardize_kernel puts it into every coordinate of the column.  So
// the second pass also sums the residuals x - centre, which are small and
// exact, and where their mean exceeds NB_MEAN_SHIFT standard deviations the
// mean is centre plus that shift: correctly rounded but for ties.  Below the
// threshold the standardised points move by less than their own rounding and
// the first-pass mean stands, so columns centred near zero (the unit cube,
// ellipsoid-frame coordinates) keep the values they always had.  The
// deviation is the one about `centre` in either case: the two differ by the
// square of the shift, below its rounding.
constexpr double NB_MEAN_SHIFT = 1e-12;

__global__ void __launch_bounds__(256)
nb_colstats_kernel(const double* __restrict__ x, long long n, int d,
                   double* __restrict__ mean, double* __restrict__ scale) {
  __shared__ double red[2][4];
  const int col = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double result[2];
  double centre = 0.0, shift = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    double s = 0.0, r = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) {
      const double v = x[i * d + col] - centre;
      s += pass == 0 ? v : v * v;
      r += v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s += __shfl_xor(s, o);
      r += __shfl_xor(r, o);
    }
    __syncthreads();
    if (lane == 0) {
      red[0][wave] = s;
      red[1][wave] = r;
    }
    __syncthreads();
    result[pass] = (red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (double)n;
    if (pass == 0) centre = result[0];
    else shift = (red[1][0] + red[1][1] + red[1][2] + red[1][3]) / (double)n;
  }
  if (threadIdx.x == 0) {
    const double sd = sqrt(result[1]);
    mean[col] = fabs(shift) > NB_MEAN_SHIFT * sd ? centre + shift : centre;
    scale[col] = sd;
  }
}

__global__ void __launch_bounds__(256)
nb_standardize_kernel(const double* __restrict__ x, long long total, int d,
                      const double* __restrict__ mean,
                      const double* __restrict__ scale,
                      double* __restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       e < total; e += stride) {
    const int col = (int)(e % d);
    out[e] = (x[e] - mean[col]) / scale[col];
  }
}

// Prior.unit_to_physical (reference nautilus/prior.py:85-120: x_j =
// dist_j.isf(1 - u_j)) for the two distribution families that cover flat and
// Gaussian priors, evaluated with scipy's formulas:
//   uniform(loc, scale).isf(q) = (1 - q) * scale + loc
//   norm(loc, scale).isf(q)    = -ndtri(q) * scale + loc
struct PriorArgs {
  double p0[16 * NB_MAX_DT], p1[16 * NB_MAX_DT];
  unsigned char kind[16 * NB_MAX_DT];     // 0 uniform, 1 normal
};

__global__ void __launch_bounds__(256)
nb_prior_kernel(const double* __restrict__ u, long long total, int d,
                PriorArgs a, double* __restrict__ out) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       e < total; e += stride) {
    const int col = (int)(e % d);
    const double q = 1.0 - u[e];
    const double z = a.kind[col] ? -normcdfinv(q) : 1.0 - q;
    out[e] = z * a.p1[col] + a.p0[col];
  }
}


// Table-driven prior transform: the same x_j = dist_j.isf(1 - u_j) for
// seventeen families, with the per-column table in device memory (uploaded
// once per prior by nb_prior_table_create, nb_api.hip) instead of a by-value
// argument.
//   kind  scipy name             z(q), then x = z * scale + loc
//   0     uniform                1 - q
//   1     norm                   -ndtri(q)
//   2     loguniform/reciprocal  exp(log a + (1 - q) (log b - log a))
//   3     lognorm                exp(-s ndtri(q))
//   4     halfnorm               -ndtri(q / 2)
//   5     truncnorm              see pt_value (and pt_truncnorm_log)
//   7-17  the closed-form tier   see pt_closed_form
// Products and sums are rounded one by one (no contraction), as numpy does,
// so that kind 0 equals scipy bit for bit whatever loc and scale are.
//
// A workgroup stages PT_ROWS rows in LDS with 16-byte reads that run along
// the rows; then every wavefront takes whole columns (lane = row), so a
// wavefront executes ONE kind and the ndtri families do not pay for each
// other.  The LDS row stride is odd in doubles: the row-wise fill writes
// consecutive doubles, the column-wise pass reads addresses 2 * LS dwords
// apart, which fall on 32 distinct even banks per half wavefront.  From the
// staged block either layout is written: row-major (n, d), or column-major
// (n_keys, n) with one contiguous row per key of the prior -- a free
// parameter's column, a fixed parameter's constant, a tied parameter's root
// column written a second time.
constexpr int PT_ROWS = 64;
constexpr int PT_THREADS = 256;
// rows of the parameter table (column-contiguous: par[row * d + column])
enum { PT_LOC = 0, PT_SCALE, PT_P0, PT_P1, PT_P2, PT_P3, PT_P4, PT_P5, PT_NPAR };
static_assert(PT_NPAR == NB_PRIOR_NPAR, "table rows");

// Standard normal truncated to [a, b] (kind 5): with p = 1 - q (exact for
// every q that is 1 - u rounded once),
//   Phi(x) = Phi(a) + p M      1 - Phi(x) = (1 - Phi(b)) + q M
// where M = Phi(b) - Phi(a) is the mass of the interval.  Both are sums of
// positive terms, so neither cancels; the one that is at most 1/2 is inverted
// (the tail side of x: there ndtri turns a relative error delta of its
// argument into at most 1.26 delta in x, while on the far side it amplifies
// by 1 / pdf).  The three constants come from the host in extended precision
// (each from the tail it lives in), one fma rounds a function that is
// monotone in u once, and the choice of side is monotone as well, so the
// result is non-decreasing in u; the clamp keeps it inside [a, b].
//
// Kind 6 (internal; nb_prior_table_create turns a truncnorm into it when the
// interval starts more than NB_PRIOR_LOG_SPACE standard deviations out, where
// the masses above underflow): the same equation in log space.  With the
// interval mirrored to the right tail, [a, b] with a > 0, and S = 1 - Phi,
//   S(x) / S(a) = r = R0 + qq R1,   R0 = S(b) / S(a),  R1 = 1 - R0
// (qq = q, or p for a mirrored interval), and with S(x) = erfcx(x / sqrt 2)
// exp(-x^2 / 2) / 2 the equation log S(x) - log S(a) - log r = 0 reads
//   log erfcx(x / sqrt 2) - log erfcx(a / sqrt 2) - (x - a)(x + a) / 2 - log r
// in which no term is large.  Newton steps from the asymptotic solution
// x^2 = a^2 - 2 log r; the derivative is minus the hazard rate
// sqrt(2 / pi) / erfcx(x / sqrt 2).  (An "ndtri of a logarithm" without
// forming the logarithm of the tiny mass at all.)
__device__ __forceinline__ double pt_truncnorm_log(double qq, double a,
                                                   double b, double log_ea,
                                                   double r0, double r1) {
  const double r = fma(qq, r1, r0);
  const double lr = log(r);
  double x = sqrt(fma(a, a, -2.0 * lr));
#pragma unroll 1
  for (int it = 0; it < 4; ++it) {
    const double e = erfcx(x * 0.70710678118654752440);
    const double f = (log(e) - log_ea) - 0.5 * (x - a) * (x + a) - lr;
    x = fma(f * e, 1.2533141373155002512, x);         // sqrt(pi / 2)
  }
  x = r > 0.0 ? x : b;                    // all of the mass is below: x = b
  return fmin(fmax(x, a), b);
}

// The closed-form tier (kinds 7 to 17): quantile functions that are a few
// log / exp / sqrt / sinpi operations, z = dist.isf(q).
//   kind  scipy name (shape)   z(q)                       rows PT_P0..
//   7     cauchy               cot(pi q)
//   8     halfcauchy           cot(pi q / 2)
//   9     laplace              -log(2 q), q < 1/2; log(2 p) otherwise
//   10    logistic             log(p / q)
//   11    gumbel_r             -log(-log p)
//   12    gumbel_l             log(-log q)
//   13    weibull_min (c)      (-log q)^(1 / c)           1 / c
//   14    rayleigh             sqrt(-2 log q)
//   15    pareto (b)           q^(-1 / b)                 1 / b
//   16    powerlaw (a)         p^(1 / a)                  1 / a
//   17    triang (c)           sqrt(c p), p < c;          c, 1 - c
//                              1 - sqrt((1 - c) q) otherwise
// q is the given number and p = 1 - q is exact for q >= 1/2, so m, whichever
// of the two is at most 1/2, is always exact, and the symmetric families
// (7, 9, 10) are evaluated in the tail that m measures, with the sign of the
// side: cot(pi q) = -cot(pi p), log(p / q) = log1p((1 - 2 m) / m) on the left
// of the median and minus that on the right, where 1 - 2 m loses nothing.  The
// argument of sincospi never leaves [0, 1/2], so no general-argument tan with
// its reduction of large arguments is needed, and sinpi(0) = +0 gives the
// infinite end its sign.
// log p is formed as log1p(-q) where it matters (kind 11: -log p is the
// ARGUMENT of a logarithm; kind 16 multiplies it by 1 / a and is content with
// log of the rounded p).  Powers are exp(log(.) / shape) with the reciprocal
// shape rounded once on the host, as scipy forms it.  The kind is the
// wavefront's, so each case is a scalar branch and runs alone; inside a case
// the two sides of the median share every library call.  The clamps of kinds
// 15 and 16 cost one instruction and keep a likelihood that takes a logarithm
// of x - loc - scale or of loc + scale - x safe whatever exp rounds to.
__device__ __forceinline__ double pt_closed_form(int kind, double q, double p,
                                                 const double* __restrict__ par,
                                                 int d) {
#pragma clang fp contract(off)
  const bool low = q < 0.5;
  const double m = low ? q : p;
  double z, t;
  switch (kind) {
    case 7:
    case 8: {
      double s, c;
      sincospi(kind == 7 ? m : 0.5 * q, &s, &c);
      z = c / s;
      if (kind == 7 && !low) z = -z;
      break;
    }
    case 9:
      t = log(2.0 * m);
      z = low ? -t : t;
      break;
    case 10:
      t = 2.0 * m;
      t = 1.0 - t;
      t = log1p(t / m);
      z = low ? t : -t;
      break;
    case 11:
      z = -log(fabs(log1p(-q)));
      break;
    case 12:
      z = log(fabs(log(q)));
      break;
    case 13:
      t = log(fabs(log(q)));
      z = exp(t * par[PT_P0 * d]);
      break;
    case 14:
      t = 2.0 * fabs(log(q));
      z = sqrt(t);
      break;
    case 15:
      t = fabs(log(q)) * par[PT_P0 * d];
      z = fmax(exp(t), 1.0);
      break;
    case 16:
      t = log(p) * par[PT_P0 * d];
      z = fmin(exp(t), 1.0);
      break;
    default: {                                        // 17
      const double c = par[PT_P0 * d];
      const bool left = p < c;
      t = left ? c * p : par[PT_P1 * d] * q;
      t = sqrt(t);
      z = left ? t : 1.0 - t;
      break;
    }
  }
  return z;
}

// pt_value has ONE call site of normcdfinv and one of exp for the kinds below
// 7 (they differ in the argument and in what is done with the result).  The
// library's inverse normal distribution function alone takes more than 400
// vector registers, which leaves one wavefront per SIMD.  So the kernel comes
// in three base levels, chosen per table: 0 for kinds 0 and 2 only (44
// registers: flat and log-uniform priors stream at full occupancy), 1 with
// the normal families, 2 with the log-space truncnorm as well (its erfcx /
// log loop costs the others a few per cent when it is compiled in).  A table
// with a closed-form kind runs level base + 3, the same code with
// pt_closed_form compiled in; a table without one runs what it always ran.
template <int LEVEL>
__device__ __forceinline__ double pt_value(int kind, double u,
                                           const double* __restrict__ par,
                                           int d) {
#pragma clang fp contract(off)
  constexpr int BASE = LEVEL % 3;
  const double q = 1.0 - u;
  const double p = 1.0 - q;
  double z = p;                                       // kind 0
  bool upper = false;
  if (BASE >= 1 && (kind == 1 || (kind >= 3 && kind <= 5))) {
    double arg = q;                                   // kinds 1, 3
    if (kind == 4) arg = q * 0.5;
    if (kind == 5) {
      arg = fma(p, par[PT_P4 * d], par[PT_P2 * d]);   // Phi(x)
      upper = arg > 0.5;
      if (upper) arg = fma(q, par[PT_P4 * d], par[PT_P3 * d]);
    }
    z = normcdfinv(arg);
    if (kind == 5) {
      z = upper ? fmax(-z, 0.0) : z;
      z = fmin(fmax(z, par[PT_P0 * d]), par[PT_P1 * d]);
    } else if (kind != 3) {
      z = -z;
    }
  }
  if (kind == 2 || kind == 3) {
    double t;
    if (kind == 2) {
      t = p * par[PT_P1 * d];
      t = par[PT_P0 * d] + t;
    } else {
      t = par[PT_P0 * d] * z;
      t = -t;
    }
    z = exp(t);
  }
  if (BASE >= 2 && kind == 6) {
    const double sign = par[PT_P5 * d];
    z = sign * pt_truncnorm_log(sign < 0.0 ? p : q, par[PT_P0 * d],
                                par[PT_P1 * d], par[PT_P2 * d], par[PT_P3 * d],
                                par[PT_P4 * d]);
  }
  if (LEVEL >= 3 && kind >= 7) z = pt_closed_form(kind, q, p, par, d);
  const double zs = z * par[PT_SCALE * d];
  return zs + par[PT_LOC * d];
}

// copies `total` doubles between a contiguous global span and the staged
// block (row stride ls), two per lane and step; TO_LDS selects the direction
template <bool TO_LDS>
__device__ inline void pt_copy_block(double* __restrict__ g, double* lds,
                                     int total, int d, int ls) {
  const int pairs = total >> 1;
  const int step_r = (2 * PT_THREADS) / d, step_c = (2 * PT_THREADS) % d;
  int e = 2 * (int)threadIdx.x;
  int r = e / d, c = e - r * d;
  for (int i = threadIdx.x; i < pairs; i += PT_THREADS) {
    const int r1 = c + 1 == d ? r + 1 : r;
    const int c1 = c + 1 == d ? 0 : c + 1;
    if (TO_LDS) {
      const nb_d2u v = ((const nb_d2u*)g)[i];
      lds[r * ls + c] = v.x;
      lds[r1 * ls + c1] = v.y;
    } else {
      nb_d2u v;
      v.x = lds[r * ls + c];
      v.y = lds[r1 * ls + c1];
      ((nb_d2u*)g)[i] = v;
    }
    r += step_r;
    c += step_c;
    if (c >= d) { c -= d; ++r; }
  }
  if ((total & 1) && threadIdx.x == 0) {    // last element of an odd block
    const int rl = (total - 1) / d, cl = (total - 1) - rl * d;
    if (TO_LDS) lds[rl * ls + cl] = g[total - 1];
    else g[total - 1] = lds[rl * ls + cl];
  }
}

template <bool COLUMN_MAJOR, int LEVEL>
__global__ void __launch_bounds__(PT_THREADS)
nb_prior_table_kernel(const double* __restrict__ u, long long n, int d, int ls,
                      const double* __restrict__ par,
                      const unsigned char* __restrict__ kind,
                      int n_keys, const int* __restrict__ key_column,
                      const double* __restrict__ key_value,
                      double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double pt_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long n_blocks = (n + PT_ROWS - 1) / PT_ROWS;
  for (long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const long long row0 = blk * PT_ROWS;
    const int rows = n - row0 < PT_ROWS ? (int)(n - row0) : PT_ROWS;
    pt_copy_block<true>(const_cast<double*>(u) + row0 * d, pt_lds, rows * d, d,
                        ls);
    __syncthreads();
    if (lane < rows) {
      for (int col = wave; col < d; col += PT_THREADS / 64) {
        double* at = pt_lds + lane * ls + col;
        // the column, hence its kind, is the wavefront's: a scalar branch
        const int kd = __builtin_amdgcn_readfirstlane((int)kind[col]);
        *at = pt_value<LEVEL>(kd, *at, par + col, d);
      }
    }
    __syncthreads();
    if (COLUMN_MAJOR) {
      for (int k = wave; k < n_keys; k += PT_THREADS / 64) {
        const int col = key_column[k];
        if (lane < rows)
          out[(long long)k * n + row0 + lane] =
              col >= 0 ? pt_lds[lane * ls + col] : key_value[k];
      }
    } else {
      pt_copy_block<false>(out + row0 * d, pt_lds, rows * d, d, ls);
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int nb_prior_transform(const double* u, int64_t n, int32_t d,
                                  const uint8_t* kind, const double* loc,
                                  const double* scale, double* out,
                                  void* stream_v) {
  hipStream_t stream = (hipStream_t)stream_v;
  if (d < 1 || d > 16 * NB_MAX_DT || kind == nullptr || loc == nullptr ||
      scale == nullptr || (n > 0 && (!u || !out))) {
    nb_set_error("bad prior transform arguments");
    return NB_ERR_ARG;
  }
  for (int j = 0; j < d; ++j)
    if (kind[j] > 1) {
      nb_set_error("prior kind %d of parameter %d is not supported", kind[j], j);
      return NB_ERR_UNSUPPORTED;
    }
  if (n <= 0) return NB_OK;
  PriorArgs a;
  for (int j = 0; j < 16 * NB_MAX_DT; ++j) {
    a.kind[j] = j < d ? kind[j] : 0;
    a.p0[j] = j < d ? loc[j] : 0.0;
    a.p1[j] = j < d ? scale[j] : 1.0;
  }
  const long long total = (long long)n * d;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(nb_prior_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     stream, u, total, d, a, out);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}

int nb_launch_prior_table(const double* u, long long n, int d,
                          const double* par, const unsigned char* kind,
                          int n_keys, const int* key_column,
                          const double* key_value, int column_major,
                          int level, double* out, hipStream_t stream) {
  if (n <= 0) return NB_OK;
  const int ls = d | 1;
  const size_t lds = (size_t)PT_ROWS * ls * sizeof(double);
  if (level < 0 || level > 5) {
    nb_set_error("bad prior table level %d", level);
    return NB_ERR_ARG;
  }
  long long blocks = (n + PT_ROWS - 1) / PT_ROWS;
  if (blocks > 2048) blocks = 2048;
  auto launch = [&](auto cm) {
    // the six levels, counted from one
    return nb_tile_dispatch<6>(level + 1, [&](auto level1) {
      constexpr auto kernel =
          nb_prior_table_kernel<decltype(cm)::value, level1() - 1>;
      if (const int rc = nb_allow_lds<kernel>(lds)) return rc;
      (void)hipGetLastError();
      hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(PT_THREADS), lds,
                         stream, u, n, d, ls, par, kind, n_keys, key_column,
                         key_value, out);
      NB_HIP_CHECK(hipGetLastError());
      return NB_OK;
    });
  };
  return !column_major ? launch(std::false_type()) : launch(std::true_type());
}

int nb_launch_transform(const double* ell_block, int dt, int n_dim,
                        const double* x, long long n, double* y,
                        hipStream_t stream) {
  if (n <= 0) return NB_OK;
  long long blocks = ((n + 15) / 16 + 3) / 4;
  if (blocks > 2048) blocks = 2048;
  const int rc = nb_tile_dispatch(dt, [&](auto t) {
    hipLaunchKernelGGL(nb_transform_kernel<t()>, dim3((unsigned)blocks),
                       dim3(256), 0, stream, ell_block, n_dim, x, n, y);
    return NB_OK;
  });
  if (rc != NB_OK) return rc;
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}

int nb_launch_standardize(const double* x, long long n, int d, double* mean,
                          double* scale, double* out, hipStream_t stream) {
  if (n <= 0 || d <= 0) return NB_OK;
  hipLaunchKernelGGL(nb_colstats_kernel, dim3(d), dim3(256), 0, stream, x, n,
                     d, mean, scale);
  if (out != nullptr) {
    const long long total = n * d;
    long long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(nb_standardize_kernel, dim3((unsigned)blocks),
                       dim3(256), 0, stream, x, total, d, mean, scale, out);
  }
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}

extern "C" int nb_standardize(const double* x, int64_t n, int32_t n_dim,
                              double* mean, double* scale, double* out,
                              void* stream) {
  if (x == nullptr || mean == nullptr || scale == nullptr) {
    nb_set_error("null argument");
    return NB_ERR_ARG;
  }
  return nb_launch_standardize(x, n, n_dim, mean, scale, out,
                               (hipStream_t)stream);
}
