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
// is that of nb_chi2_kernel on v_mfma_f64_16x16x4_f64:
//  * a workgroup of 8 wavefronts owns a block of TPW tiles of 16 points; the
//    points are the FREE index of the B operand (lane & 15), so whatever a
//    point's source values hold stays in that point's column of every product;
//  * the bins go in PANELS of 16 row tiles (256 bins).  Wavefront w holds the
//    accumulators of row tiles w and 8 + w of the panel for all TPW point tiles
//    in registers (16 TPW VGPRs);
//  * k runs in CHUNKS of one k-tile (16 source columns).  Per chunk the panel's
//    slice of R (packed on the host as operand tiles, zero padded in both
//    directions, nb_fold_poisson_create) arrives in LDS by global_load_lds,
//    and the block's slice of s is written there once for all wavefronts; a
//    padding column of s (k >= K) is an exact zero, never a repeated load.
//    Both are double buffered: the chunk after the current one is on its way
//    while the matrix cores work (one barrier per chunk).  Every (panel,
//    k-tile) pair is dense; the slice of s is read again for every panel (from
//    L2: a block's source rows are 8 K TPW 16 bytes);
//  * when a panel's k range ends, accumulator register r of row tile t of
//    lane l holds sum_k R_jk s_ik for bin j = 16 t + (l >> 4) + 4 r and point
//    i = l & 15.  po_term turns it into D(e_j acc + b_j, k_j) with k, 1 / k,
//    e, b of the lane's bins from the device table (requested before the
//    chunk's matrix work starts); a bin past P adds neither a term nor a flag.
//    The terms go into a per-lane partial and the flags into a per-lane word
//    of each point -- registers 0..3, row tiles in order, panels in order --
//    and at the end the four lanes of a point (^16, then ^32), then the eight
//    wavefronts (through LDS, in order) are added.  No atomics: the bits of a
//    row depend on P and K only, not on n, the row's place in the batch, ld,
//    the stream, the grid or TPW (the launcher picks the block of points by
//    n alone, and a point's accumulators never see its neighbours).
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
#include "nb_lds_copy.h"
#include "nb_poisson_term.h"

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

namespace {

constexpr int FO_WAVES = 8;                     // wavefronts of a workgroup
constexpr int FO_RT = NB_FOLD_PANEL / FO_WAVES; // row tiles per wavefront
static_assert(FO_RT == 2, "row tiles w and 8 + w");

// blob: k, 1 / k, e, b, each padded to 16 DT doubles (nb_fold_r_offset), then
// for every panel p and k-tile kt the panel's row tiles as 16x16 operand
// tiles: element (row, k = 4 lg + s) of a tile at s * 64 + lg * 16 + row.
// src: n rows of n_src doubles, ld doubles apart.
template <int TPW>
__global__ void __launch_bounds__(64 * FO_WAVES)
nb_fold_poisson_kernel(const double* __restrict__ blob, int n_data, int n_src,
                       const double* __restrict__ src, long long ld,
                       long long n, double log_const,
                       double* __restrict__ out) {
  constexpr int PB = 16 * TPW;                   // points of a workgroup
  __shared__ __attribute__((aligned(16))) double w_a[NB_FOLD_PANEL * NB_TILE];
  __shared__ __attribute__((aligned(16))) double w_b[NB_FOLD_PANEL * NB_TILE];
  __shared__ __attribute__((aligned(16))) double s_a[PB * 16];
  __shared__ __attribute__((aligned(16))) double s_b[PB * 16];
  __shared__ double red[FO_WAVES * PB];
  __shared__ unsigned redf[FO_WAVES * PB];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int dt = (n_data + 15) >> 4;
  const int nkt = (n_src + 15) >> 4;             // k-tiles of every panel
  const int n_panels = (dt + NB_FOLD_PANEL - 1) / NB_FOLD_PANEL;
  const nb_gd* tk = (const nb_gd*)blob;
  const nb_gd* tik = tk + 16 * (size_t)dt;
  const nb_gd* te = tk + 32 * (size_t)dt;
  const nb_gd* tb = tk + 48 * (size_t)dt;
  const nb_gd* wg = tk + nb_fold_r_offset(dt);

  // staging role: thread 4 p + q brings columns 4 q .. 4 q + 3 of every chunk
  // of point p of the block (a wavefront covers one tile of 16 points, 128
  // contiguous bytes of each); a point past the end of the batch is the last
  // row again and stores nothing
  const bool stager = tid < 4 * PB;              // whole wavefronts
  const int sp = tid >> 2, sq = tid & 3;
  const long long row0 = (long long)blockIdx.x * PB;
  const long long srow = row0 + sp < n ? row0 + sp : n - 1;
  const nb_gd* mrow = (const nb_gd*)src + srow * ld;
  const int s_at = ((sp >> 4) * 16 + sq) * 16 + (sp & 15);   // + e * 64

  double mv[4];
  auto load_s = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = 16 * kt + 4 * sq + e;      // < 16 nkt
      mv[e] = mrow[col < n_src ? col : n_src - 1];
    }
  };
  auto write_s = [&](double* s_dst, int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = 16 * kt + 4 * sq + e;
      // a padding column is an exact zero: it meets zeros of R only
      s_dst[s_at + e * 64] = col < n_src ? mv[e] : 0.0;
    }
  };

  nb_d4 acc[FO_RT][TPW];
  double part[TPW];
  unsigned flag[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    part[t] = 0.0;
    flag[t] = 0u;
#pragma unroll
    for (int j = 0; j < FO_RT; ++j) acc[j][t] = nb_d4{0.0, 0.0, 0.0, 0.0};
  }

  // state of the walk over (panel, k-tile)
  int panel = 0, kt = 0;
  int nrt = dt < NB_FOLD_PANEL ? dt : NB_FOLD_PANEL;   // row tiles of the panel
  const nb_gd* wsrc = wg;                              // chunk (panel, kt)

  // one chunk: w_cur / s_cur hold (panel, kt); the chunk after it goes to
  // w_nxt / s_nxt.  Returns false after the last chunk.
  auto step = [&](const double* w_cur, const double* s_cur, double* w_nxt,
                  double* s_nxt) __attribute__((always_inline)) -> bool {
    nb_wait_copies();
    __syncthreads();
    const bool last_of_panel = kt + 1 == nkt;
    const bool more = !(last_of_panel && panel + 1 == n_panels);
    const int kt_n = last_of_panel ? 0 : kt + 1;
    const int panel_n = last_of_panel ? panel + 1 : panel;
    const int left = dt - NB_FOLD_PANEL * panel_n;
    const int nrt_n = left < NB_FOLD_PANEL ? left : NB_FOLD_PANEL;
    const nb_gd* wsrc_n = wsrc + (size_t)nrt * NB_TILE;
    if (more) {
      nb_copy_tiles<FO_WAVES>(wsrc_n, w_nxt, nrt_n, wave, lane);
      if (stager) load_s(kt_n);
    }

    const int tile[FO_RT] = {wave, FO_WAVES + wave};   // of the panel
    const bool on[FO_RT] = {tile[0] < nrt, tile[1] < nrt};
    // the table entries of the lane's bins, on their way during the matrix
    // work of the panel's last chunk (the table is padded to whole tiles)
    double bk[FO_RT][4], bik[FO_RT][4], be[FO_RT][4], bb[FO_RT][4];
    if (last_of_panel) {
#pragma unroll
      for (int j = 0; j < FO_RT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int bin = on[j] ? 16 * (NB_FOLD_PANEL * panel + tile[j]) +
                                      (lane >> 4) + 4 * r
                                : 0;
          bk[j][r] = tk[bin];
          bik[j][r] = tik[bin];
          be[j][r] = te[bin];
          bb[j][r] = tb[bin];
        }
    }

    if (on[0]) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        double b[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t) b[t] = s_cur[(t * 4 + s) * 64 + lane];
        {
          const double a = w_cur[tile[0] * NB_TILE + s * 64 + lane];
#pragma unroll
          for (int t = 0; t < TPW; ++t) acc[0][t] = MFMA(a, b[t], acc[0][t]);
        }
        if (on[1]) {
          const double a = w_cur[tile[1] * NB_TILE + s * 64 + lane];
#pragma unroll
          for (int t = 0; t < TPW; ++t) acc[1][t] = MFMA(a, b[t], acc[1][t]);
        }
      }
    }
    if (last_of_panel) {
      // the panel's bins are complete: their terms and flags, fixed order
#pragma unroll
      for (int j = 0; j < FO_RT; ++j) {
        if (on[j]) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int bin = 16 * (NB_FOLD_PANEL * panel + tile[j]) +
                            (lane >> 4) + 4 * r;
            const bool in = bin < n_data;
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
              unsigned f = 0u;
              const double d = po_term(acc[j][t][r], bk[j][r], bik[j][r],
                                       be[j][r], bb[j][r], &f);
              part[t] += in ? d : 0.0;
              flag[t] |= in ? f : 0u;
            }
          }
        }
#pragma unroll
        for (int t = 0; t < TPW; ++t) acc[j][t] = nb_d4{0.0, 0.0, 0.0, 0.0};
      }
    }
    if (more && stager) write_s(s_nxt, kt_n);
    wsrc = wsrc_n;
    kt = kt_n;
    panel = panel_n;
    nrt = nrt_n;
    return more;
  };

  // chunk (0, 0) into the a buffers
  nb_copy_tiles<FO_WAVES>(wsrc, w_a, nrt, wave, lane);
  if (stager) {
    load_s(0);
    write_s(s_a, 0);
  }
  for (;;) {
    if (!step(w_a, s_a, w_b, s_b)) break;
    if (!step(w_b, s_b, w_a, s_a)) break;
  }

  // the four lanes of a point, then the wavefronts in order
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    double v = part[t];
    unsigned f = flag[t];
    v += __shfl_xor(v, 16);
    f |= (unsigned)__shfl_xor((int)f, 16);
    v += __shfl_xor(v, 32);
    f |= (unsigned)__shfl_xor((int)f, 32);
    if (lane < 16) {
      red[wave * PB + 16 * t + lane] = v;
      redf[wave * PB + 16 * t + lane] = f;
    }
  }
  __syncthreads();
  if (tid < PB && row0 + tid < n) {
    double v = red[tid];
    unsigned f = redf[tid];
#pragma unroll
    for (int w = 1; w < FO_WAVES; ++w) {
      v += red[w * PB + tid];
      f |= redf[w * PB + tid];
    }
    double res = log_const - v;
    if (f & PO_NEG_INF) res = -__builtin_inf();
    if (f & PO_NAN) res = __builtin_nan("");
    out[row0 + tid] = res;
  }
}

template <int TPW>
int launch(const double* blob, int n_data, int n_src, const double* src,
           long long ld, long long n, double log_const, double* out,
           hipStream_t stream) {
  const long long blocks = (n + 16 * TPW - 1) / (16 * TPW);
  if (blocks > 0x7fffffffll) {
    nb_set_error("n = %lld is too large for one launch", n);
    return NB_ERR_UNSUPPORTED;
  }
  (void)hipGetLastError();
  hipLaunchKernelGGL(nb_fold_poisson_kernel<TPW>, dim3((unsigned)blocks),
                     dim3(64 * FO_WAVES), 0, stream, blob, n_data, n_src, src,
                     ld, n, log_const, out);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
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
    return launch<4>(blob, n_data, n_src, src, ld, n, log_const, out, stream);
  return launch<2>(blob, n_data, n_src, src, ld, n, log_const, out, stream);
}
