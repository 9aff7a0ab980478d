// Gaussian likelihood of a DATA VECTOR in one kernel (the user-side likelihood
// callable of reference sampler.py:863-873 for a model prediction m(theta) of
// P data points d with covariance C = L L^T):
//     log L = log_norm - 1/2 |W (m - d)|^2,   W = L^-1 lower triangular,
// P up to NB_CHI2_MAX_DATA = 4096 -- far beyond the register-resident tiles of
// nb_quadform.h (n_dim <= 128).  A triangular GEMM fused with a row norm: the
// n x P product is never stored.
//
// Algorithmic work n P (P + 16) flop, traffic 8 P bytes read + 8 written per
// point.  Two-level blocking on v_mfma_f64_16x16x4_f64:
//  * a workgroup of 8 wavefronts owns a block of TPW tiles of 16 points; the
//    points are the FREE index of the B operand (lane & 15), so a NaN in a
//    point's residual stays in that point's column of every product;
//  * the rows of W go in PANELS of 16 row tiles (256 rows).  Wavefront w holds
//    the accumulators of row tiles w and 8 + w of the panel for all TPW point
//    tiles in registers (16 TPW VGPRs) -- row tiles interleaved, so that a
//    short W (P <= 128) still occupies all wavefronts and the triangle is
//    balanced;
//  * k runs in CHUNKS of one k-tile (16 columns of W).  Per chunk the panel's
//    slice of W (packed on the host as operand tiles, nb_chi2_create) arrives
//    in LDS by global_load_lds, and the residuals r = m - d of the block's
//    points, formed on the fly from the model rows, are written there once
//    for all wavefronts.  Both are double buffered: the chunk after the
//    current one is on its way while the matrix cores work (one barrier per
//    chunk).  An operand of W read from LDS feeds TPW MFMAs, a residual two;
//  * k-tiles above the diagonal are neither stored, staged nor multiplied: a
//    panel's k range ends at its last row tile, and inside the panel a
//    wavefront skips the chunks above its own row tile;
//  * when a panel's k range ends, the squares of its accumulators are folded
//    into a per-lane partial of each point -- registers 0..3, row tiles in
//    order, panels in order -- and at the end the four lanes of a point, then
//    the eight wavefronts (through LDS, in order) are added.  The order is
//    fixed per row: no atomics, and the bits of a row depend on neither n,
//    the row's place in the batch, ld, nor TPW (the launcher picks the
//    largest block of points that still gives every CU a workgroup).
// A non-finite residual poisons its point explicitly (r * 0 added to the
// sum): +inf against the exact zeros of the diagonal tiles alone would give
// NaN or inf depending on the column it sits in.
//
// The diagonal case (sigma) is a separate memory-bound kernel below.
#include "nb_common.h"
#include "nb_launch.h"
#include "nb_lds_copy.h"

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

namespace {

constexpr int CH_WAVES = 8;                     // wavefronts of a workgroup
constexpr int CH_RT = NB_CHI2_PANEL / CH_WAVES; // row tiles per wavefront
static_assert(CH_RT == 2, "row tiles w and 8 + w");

// blob: d zero padded to 16 DT doubles (nb_chi2_w_offset), then for every
// panel p and k-tile kt <= last row tile of p the panel's row tiles as 16x16
// operand tiles: element (row, k = 4 lg + s) of a tile at s * 64 + lg * 16 +
// row.  model: n rows of n_data doubles, ld doubles apart.
template <int TPW>
__global__ void __launch_bounds__(64 * CH_WAVES)
nb_chi2_kernel(const double* __restrict__ blob, int n_data,
               const double* __restrict__ model, long long ld, long long n,
               double log_norm, double* __restrict__ out) {
  constexpr int PB = 16 * TPW;                   // points of a workgroup
  __shared__ __attribute__((aligned(16))) double w_a[NB_CHI2_PANEL * NB_TILE];
  __shared__ __attribute__((aligned(16))) double w_b[NB_CHI2_PANEL * NB_TILE];
  __shared__ __attribute__((aligned(16))) double r_a[PB * 16];
  __shared__ __attribute__((aligned(16))) double r_b[PB * 16];
  __shared__ double red[CH_WAVES * PB];
  __shared__ double bad[PB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dt = (n_data + 15) >> 4;
  const int n_panels = (dt + NB_CHI2_PANEL - 1) / NB_CHI2_PANEL;
  const nb_gd* dpad = (const nb_gd*)blob;
  const nb_gd* wg = dpad + nb_chi2_w_offset(dt);

  // staging role: thread 4 p + q brings columns 4 q .. 4 q + 3 of every chunk
  // of point p of the block (a wavefront covers one tile of 16 points, 128
  // contiguous bytes of each); a point past the end of the batch is the last
  // row again and stores nothing
  const bool stager = tid < 4 * PB;              // whole wavefronts
  const int sp = tid >> 2, sq = tid & 3;
  const long long row0 = (long long)blockIdx.x * PB;
  const long long srow = row0 + sp < n ? row0 + sp : n - 1;
  const nb_gd* mrow = (const nb_gd*)model + srow * ld;
  const int r_at = ((sp >> 4) * 16 + sq) * 16 + (sp & 15);   // + e * 64
  double poison = 0.0;

  double mv[4], dv[4];
  auto load_r = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = 16 * kt + 4 * sq + e;      // < 16 dt
      mv[e] = mrow[col < n_data ? col : n_data - 1];
      dv[e] = dpad[col];
    }
  };
  auto write_r = [&](double* r_dst, int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = 16 * kt + 4 * sq + e;
      // a padding column is an exact zero: it meets zeros of W only
      const double r = col < n_data ? mv[e] - dv[e] : 0.0;
      poison = fma(r, 0.0, poison);
      r_dst[r_at + e * 64] = r;
    }
  };

  nb_d4 acc[CH_RT][TPW];
  double part[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    part[t] = 0.0;
#pragma unroll
    for (int j = 0; j < CH_RT; ++j) acc[j][t] = nb_d4{0.0, 0.0, 0.0, 0.0};
  }

  // state of the walk over (panel, k-tile)
  int panel = 0, kt = 0;
  int nrt = dt < NB_CHI2_PANEL ? dt : NB_CHI2_PANEL;   // row tiles of the panel
  const nb_gd* wsrc = wg;                              // chunk (panel, kt)

  // one chunk: w_cur / r_cur hold (panel, kt); the chunk after it goes to
  // w_nxt / r_nxt.  Returns false after the last chunk.
  auto step = [&](const double* w_cur, const double* r_cur, double* w_nxt,
                  double* r_nxt) __attribute__((always_inline)) -> bool {
    nb_wait_copies();
    __syncthreads();
    const int nkt = NB_CHI2_PANEL * panel + nrt;       // k-tiles of the panel
    const bool last_of_panel = kt + 1 == nkt;
    const bool more = !(last_of_panel && panel + 1 == n_panels);
    const int kt_n = last_of_panel ? 0 : kt + 1;
    const int panel_n = last_of_panel ? panel + 1 : panel;
    const int left = dt - NB_CHI2_PANEL * panel_n;
    const int nrt_n = left < NB_CHI2_PANEL ? left : NB_CHI2_PANEL;
    const nb_gd* wsrc_n = wsrc + (size_t)nrt * NB_TILE;
    if (more) {
      nb_copy_tiles<CH_WAVES>(wsrc_n, w_nxt, nrt_n, wave, lane);
      if (stager) load_r(kt_n);
    }

    const int tile0 = wave, tile1 = CH_WAVES + wave;   // of the panel
    const int rt0 = NB_CHI2_PANEL * panel + tile0;
    const bool on0 = tile0 < nrt && kt <= rt0;
    const bool on1 = tile1 < nrt && kt <= rt0 + CH_WAVES;
    if (on0 || on1) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        double b[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t) b[t] = r_cur[(t * 4 + s) * 64 + lane];
        if (on0) {
          const double a = w_cur[tile0 * NB_TILE + s * 64 + lane];
#pragma unroll
          for (int t = 0; t < TPW; ++t) acc[0][t] = MFMA(a, b[t], acc[0][t]);
        }
        if (on1) {
          const double a = w_cur[tile1 * NB_TILE + s * 64 + lane];
#pragma unroll
          for (int t = 0; t < TPW; ++t) acc[1][t] = MFMA(a, b[t], acc[1][t]);
        }
      }
    }
    if (last_of_panel) {
      // the panel's rows are complete: fold their squares, fixed order
#pragma unroll
      for (int j = 0; j < CH_RT; ++j)
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            part[t] = fma(acc[j][t][r], acc[j][t][r], part[t]);
          acc[j][t] = nb_d4{0.0, 0.0, 0.0, 0.0};
        }
    }
    if (more && stager) write_r(r_nxt, kt_n);
    wsrc = wsrc_n;
    kt = kt_n;
    panel = panel_n;
    nrt = nrt_n;
    return more;
  };

  // chunk (0, 0) into the a buffers
  nb_copy_tiles<CH_WAVES>(wsrc, w_a, nrt, wave, lane);
  if (stager) {
    load_r(0);
    write_r(r_a, 0);
  }
  for (;;) {
    if (!step(w_a, r_a, w_b, r_b)) break;
    if (!step(w_b, r_b, w_a, r_a)) break;
  }

  // the four lanes of a point, then the wavefronts in order
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    double v = part[t];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (lane < 16) red[wave * PB + 16 * t + lane] = v;
  }
  if (stager) {
    poison += __shfl_xor(poison, 1);
    poison += __shfl_xor(poison, 2);
    if (sq == 0) bad[sp] = poison;               // 0 or NaN
  }
  __syncthreads();
  if (tid < PB && row0 + tid < n) {
    double chi2 = red[tid];
#pragma unroll
    for (int w = 1; w < CH_WAVES; ++w) chi2 += red[w * PB + tid];
    chi2 += bad[tid];
    out[row0 + tid] = fma(-0.5, chi2, log_norm);
  }
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

template <int TPW>
int launch_full(const double* blob, int n_data, const double* model,
                long long ld, long long n, double log_norm, double* out,
                hipStream_t stream) {
  const long long blocks = (n + 16 * TPW - 1) / (16 * TPW);
  if (blocks > 0x7fffffffll) {
    nb_set_error("n = %lld is too large for one launch", n);
    return NB_ERR_UNSUPPORTED;
  }
  (void)hipGetLastError();
  hipLaunchKernelGGL(nb_chi2_kernel<TPW>, dim3((unsigned)blocks),
                     dim3(64 * CH_WAVES), 0, stream, blob, n_data, model, ld,
                     n, log_norm, out);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
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
    return launch_full<8>(blob, n_data, model, ld, n, log_norm, out, stream);
  if (n >= 256 * 64)
    return launch_full<4>(blob, n_data, model, ld, n, log_norm, out, stream);
  return launch_full<2>(blob, n_data, model, ld, n, log_norm, out, stream);
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
