// The PANEL DRIVER of the likelihoods that multiply a packed matrix A (P x K)
// with the rows x_i of a batch and reduce every column of the product to one
// number per row i: out_i = result(sum_j f_j((A x_i)_j)).  nb_chi2.hip (A = W
// lower triangular, x = m - d, f = square) and nb_fold.hip (A = R dense, x =
// s, f = the Poisson deviance) are its two users; the n x P product is never
// stored.  Device code only.
//
// Two-level blocking on v_mfma_f64_16x16x4_f64:
//  * a workgroup of 8 wavefronts owns a block of TPW tiles of 16 points; the
//    points are the FREE index of the B operand (lane & 15), so whatever a
//    point's row holds (a NaN, say) stays in that point's column of every
//    product;
//  * the rows of A go in PANELS of NB_PANEL_TILES row tiles (256 rows).
//    Wavefront w holds the accumulators of row tiles w and 8 + w of the panel
//    for all TPW point tiles in registers (16 TPW VGPRs) -- row tiles
//    interleaved, so that a short A (P <= 128) still occupies all wavefronts
//    and a triangle is balanced;
//  * k runs in CHUNKS of one k-tile (16 columns of A).  Per chunk the panel's
//    slice of A (packed on the host as operand tiles in the order of the walk,
//    put_panel_tiles of nb_pack.h) arrives in LDS by global_load_lds, and the
//    block's slice of x, formed on the fly from the batch's rows, is written
//    there once for all wavefronts.  Both are double buffered: the chunk after
//    the current one is on its way while the matrix cores work (one barrier
//    per chunk).  An operand of A read from LDS feeds TPW MFMAs, one of x two;
//  * when a panel's k range ends, accumulator register r of row tile t of lane
//    l holds (A x_i)_j for j = 16 t + (l >> 4) + 4 r and point i = l & 15.
//    The policy folds them into a per-lane partial (and, if it has one, a
//    per-lane flag word) of each point -- registers 0..3, row tiles in order,
//    panels in order -- and at the end the four lanes of a point (^16, then
//    ^32), then the eight wavefronts (through LDS, in order) are added.  The
//    order is fixed per row: no atomics, and the bits of a row depend on
//    neither n, the row's place in the batch, ld, the grid nor TPW (a
//    launcher picks the block of points by n alone).
//
// What the two kernels do not share is the POLICY, a struct of
// __forceinline__ members resolved at compile time:
//   FLAGS                  whether a flag word travels with the partial sum
//   k_tiles(panel, nrt)    k-tiles of a panel of nrt row tiles
//   takes_part(rt, kt)     whether row tile rt multiplies chunk kt
//   request(e, col)        what else staging column col needs, asked for with
//                          the row's own value (slot e of 4)
//   staged(e, v, inside)   the staged value of that column from the row's
//                          value v; inside = not a padding column
//   table, prefetch(row0, in)  what the fold needs from memory, requested
//                          before the matrix work of a panel's last chunk;
//                          row0 = the row of A in accumulator register 0 of
//                          the wavefront's two row tiles in this lane, in =
//                          whether the panel has the row tile
//   fold(acc, part, flag, table, row0, in)  the panel's accumulators into
//                          part (and flag)
//   publish(sp, sq)        what a staging thread leaves for result()
//   result(v, f, p)        the row's result from the summed value and flags,
//                          p = the point's index in the block
#pragma once
#include "nb_common.h"

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

namespace {

constexpr int NB_PANEL_WAVES = 8;               // wavefronts of a workgroup
static_assert(NB_PANEL_TILES == 2 * NB_PANEL_WAVES, "row tiles w and 8 + w");

typedef const void __attribute__((address_space(1))) * nb_gptr;
typedef void __attribute__((address_space(3))) * nb_lptr;

// s_waitcnt vmcnt(0) (expcnt and lgkmcnt left at their maxima)
__device__ __forceinline__ void nb_wait_copies() {
  __builtin_amdgcn_s_waitcnt(0x0F70);
}

// n_tiles operand tiles, global -> LDS without passing registers, by the
// whole workgroup in 1 KB pieces (destination = uniform base + lane * 16)
__device__ __forceinline__ void nb_copy_tiles(const nb_gd* __restrict__ src,
                                              double* dst, int n_tiles,
                                              int wave, int lane) {
  for (int c = wave; c < 2 * n_tiles; c += NB_PANEL_WAVES)
    __builtin_amdgcn_global_load_lds((nb_gptr)(src + c * 128 + 2 * lane),
                                     (nb_lptr)(dst + c * 128), 16, 0, 0);
}

// The block of 16 TPW rows of a workgroup of 64 NB_PANEL_WAVES threads.
// tiles: for every panel and every k-tile of it the panel's row tiles as
// 16x16 operand tiles (nb_operand_index), dt row tiles in all.  rows: n rows
// of n_cols doubles, ld doubles apart.
template <int TPW, class Policy>
__device__ __forceinline__ void nb_panel_rows(Policy& pol, const nb_gd* tiles,
                                              int dt, const nb_gd* rows,
                                              int n_cols, long long ld,
                                              long long n,
                                              double* __restrict__ out) {
  constexpr int PB = 16 * TPW;                   // points of a workgroup
  constexpr bool FLAGS = Policy::FLAGS;
  __shared__ __attribute__((aligned(16))) double w_a[NB_PANEL_TILES * NB_TILE];
  __shared__ __attribute__((aligned(16))) double w_b[NB_PANEL_TILES * NB_TILE];
  __shared__ __attribute__((aligned(16))) double x_a[PB * 16];
  __shared__ __attribute__((aligned(16))) double x_b[PB * 16];
  __shared__ double red[NB_PANEL_WAVES * PB];
  __shared__ unsigned redf[FLAGS ? NB_PANEL_WAVES * PB : 1];   // FLAGS only

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n_panels = (dt + NB_PANEL_TILES - 1) / NB_PANEL_TILES;

  // staging role: thread 4 p + q brings columns 4 q .. 4 q + 3 of every chunk
  // of point p of the block (a wavefront covers one tile of 16 points, 128
  // contiguous bytes of each); a point past the end of the batch is the last
  // row again and stores nothing
  const bool stager = tid < 4 * PB;              // whole wavefronts
  const int sp = tid >> 2, sq = tid & 3;
  const long long row0 = (long long)blockIdx.x * PB;
  const long long srow = row0 + sp < n ? row0 + sp : n - 1;
  const nb_gd* mrow = rows + srow * ld;
  const int x_at = ((sp >> 4) * 16 + sq) * 16 + (sp & 15);   // + e * 64

  double mv[4];
  auto load_x = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = 16 * kt + 4 * sq + e;      // < 16 k-tiles of the panel
      mv[e] = mrow[col < n_cols ? col : n_cols - 1];
      pol.request(e, col);
    }
  };
  auto write_x = [&](double* x_dst, int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = 16 * kt + 4 * sq + e;
      x_dst[x_at + e * 64] = pol.staged(e, mv[e], col < n_cols);
    }
  };

  nb_d4 acc[2][TPW];
  double part[TPW];
  unsigned flag[TPW];                            // unused without FLAGS
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    part[t] = 0.0;
    flag[t] = 0u;
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[j][t] = nb_d4{0.0, 0.0, 0.0, 0.0};
  }

  // the row, within a panel, that accumulator register 0 of the wavefront's
  // two row tiles holds in this lane (register r: 4 r further)
  const int lrow[2] = {16 * wave + (lane >> 4),
                       16 * (NB_PANEL_WAVES + wave) + (lane >> 4)};

  // state of the walk over (panel, k-tile)
  int panel = 0, kt = 0;
  int nrt = dt < NB_PANEL_TILES ? dt : NB_PANEL_TILES;  // row tiles of the panel
  const nb_gd* wsrc = tiles;                             // chunk (panel, kt)

  // one chunk: w_cur / x_cur hold (panel, kt); the chunk after it goes to
  // w_nxt / x_nxt.  Returns false after the last chunk.
  auto step = [&](const double* w_cur, const double* x_cur, double* w_nxt,
                  double* x_nxt) __attribute__((always_inline)) -> bool {
    nb_wait_copies();
    __syncthreads();
    const bool last_of_panel = kt + 1 == pol.k_tiles(panel, nrt);
    const bool more = !(last_of_panel && panel + 1 == n_panels);
    const int kt_n = last_of_panel ? 0 : kt + 1;
    const int panel_n = last_of_panel ? panel + 1 : panel;
    const int left = dt - NB_PANEL_TILES * panel_n;
    const int nrt_n = left < NB_PANEL_TILES ? left : NB_PANEL_TILES;
    const nb_gd* wsrc_n = wsrc + (size_t)nrt * NB_TILE;
    if (more) {
      nb_copy_tiles(wsrc_n, w_nxt, nrt_n, wave, lane);
      if (stager) load_x(kt_n);
    }

    const int tile[2] = {wave, NB_PANEL_WAVES + wave};   // of the panel
    const int rt[2] = {NB_PANEL_TILES * panel + tile[0],
                       NB_PANEL_TILES * panel + tile[1]};
    const bool in[2] = {tile[0] < nrt, tile[1] < nrt};
    const bool on[2] = {in[0] && pol.takes_part(rt[0], kt),
                        in[1] && pol.takes_part(rt[1], kt)};
    const int row0[2] = {16 * NB_PANEL_TILES * panel + lrow[0],
                         16 * NB_PANEL_TILES * panel + lrow[1]};
    typename Policy::table tab;
    if (last_of_panel) tab = pol.prefetch(row0, in);

    if (on[0] || on[1]) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        double b[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t) b[t] = x_cur[(t * 4 + s) * 64 + lane];
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (on[j]) {
            const double a = w_cur[tile[j] * NB_TILE + s * 64 + lane];
#pragma unroll
            for (int t = 0; t < TPW; ++t) acc[j][t] = MFMA(a, b[t], acc[j][t]);
          }
      }
    }
    if (last_of_panel) {
      // the panel's rows are complete
      pol.fold(acc, part, flag, tab, row0, in);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < TPW; ++t) acc[j][t] = nb_d4{0.0, 0.0, 0.0, 0.0};
    }
    if (more && stager) write_x(x_nxt, kt_n);
    wsrc = wsrc_n;
    kt = kt_n;
    panel = panel_n;
    nrt = nrt_n;
    return more;
  };

  // chunk (0, 0) into the a buffers
  nb_copy_tiles(wsrc, w_a, nrt, wave, lane);
  if (stager) {
    load_x(0);
    write_x(x_a, 0);
  }
  for (;;) {
    if (!step(w_a, x_a, w_b, x_b)) break;
    if (!step(w_b, x_b, w_a, x_a)) break;
  }

  // the four lanes of a point, then the wavefronts in order
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    double v = part[t];
    unsigned f = flag[t];
    v += __shfl_xor(v, 16);
    if constexpr (FLAGS) f |= (unsigned)__shfl_xor((int)f, 16);
    v += __shfl_xor(v, 32);
    if constexpr (FLAGS) f |= (unsigned)__shfl_xor((int)f, 32);
    if (lane < 16) {
      red[wave * PB + 16 * t + lane] = v;
      if constexpr (FLAGS) redf[wave * PB + 16 * t + lane] = f;
    }
  }
  if (stager) pol.publish(sp, sq);
  __syncthreads();
  if (tid < PB && row0 + tid < n) {
    double v = red[tid];
    unsigned f = 0u;
    if constexpr (FLAGS) f = redf[tid];
#pragma unroll
    for (int w = 1; w < NB_PANEL_WAVES; ++w) {
      v += red[w * PB + tid];
      if constexpr (FLAGS) f |= redf[w * PB + tid];
    }
    out[row0 + tid] = pol.result(v, f, tid);
  }
}

// One workgroup per 16 TPW rows of the batch
template <int TPW, class Kernel, class... Args>
int nb_panel_launch(Kernel kernel, long long n, hipStream_t stream,
                    Args... args) {
  const long long blocks = (n + 16 * TPW - 1) / (16 * TPW);
  if (blocks > 0x7fffffffll) {
    nb_set_error("n = %lld is too large for one launch", n);
    return NB_ERR_UNSUPPORTED;
  }
  (void)hipGetLastError();
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks),
                     dim3(64 * NB_PANEL_WAVES), 0, stream, args...);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}

}  // namespace
