// The two purely geometric queries of ONE bound, for tiles of 16 points per
// wavefront on the matrix cores (nb_tile.h: load_points, ell_eval):
//
//  * r2 (nb_neural_score of a bound without emulators -- the quadratic form of
//    GaussianLikelihood): out_f64[2 i] = |B_inv (x_i - c)|^2 against the
//    ellipsoid of neural bound 0 (bounds/basic.py:340), out_f64[2 i + 1] = 0.
//  * count (nb_member_count): out_u8[i] = number of outer members whose box
//    limits and ellipsoid contain x_i (the k of bounds/union.py:316-319),
//    without the unit-cube clip of the union.
//
// Rows are taken as they are: proposals and likelihood arguments already live
// in the frame of the bound, so there is no periodic recentring.
//
// A workgroup handles 128 rows per pass (4 wavefronts x 2 tiles up to
// n_dim = 64, where two tiles share every A operand; 8 x 1 beyond, where two
// tiles would not fit 256 registers) and strides over the passes.  The
// ellipsoid block is copied to LDS by the whole workgroup: once if there is a
// single block, else per member and pass.
#include "nb_common.h"
#include "nb_launch.h"

#include "nb_tile.h"

namespace {

struct GeomArgs {
  const nb_gd* blob;
  int count;                      // 0: r2 of neural bound 0, 1: member count
  const nb_gd* x;                 // (n, n_dim)
  long long n;
  double* out_f64;                // r2: (n, 2)
  unsigned char* out_u8;          // count: (n)
  unsigned long long* counters;   // optional: [0] outer-member point evals,
                                  // [1] neural-ellipsoid point evals
};

template <int DT, int TPW, int NW>
__global__ void __launch_bounds__(64 * NW) nb_geom_kernel(GeomArgs a) {
  constexpr int BLK = nb_ell_block_size(DT);
  extern __shared__ __attribute__((aligned(16))) double blk_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lg = lane >> 4;
  const double* hdr = (const double*)a.blob;
  const int n_dim = (int)nb_hdr(hdr, NB_H_NDIM);
  const bool count = a.count != 0;
  const int n_blk = count ? (int)nb_hdr(hdr, NB_H_K) : 1;
  const nb_gd* blk0 =
      a.blob + nb_hdr(hdr, count ? NB_H_OFF_MEMBERS : NB_H_OFF_NEURAL);
  const long long blk_stride = nb_hdr(hdr, NB_H_ELL_STRIDE);
  const long long n_super = (a.n + 16 * NW * TPW - 1) / (16 * NW * TPW);
  unsigned long long n_rows = 0;
  bool staged = false;            // workgroup-uniform, like every loop bound

  for (long long sup = blockIdx.x; sup < n_super; sup += gridDim.x) {
    long long pt[TPW];
    bool valid[TPW];
    int k_cnt[TPW];
    double r2_out[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      pt[t] = ((sup * NW + wave) * TPW + t) * 16 + (lane & 15);
      valid[t] = pt[t] < a.n;
      k_cnt[t] = 0;
      r2_out[t] = 0.0;
      n_rows += __popcll(__ballot(valid[t] && lg == 0));
    }
    double xin[TPW][4 * DT];
    load_points<DT, TPW>(a.x, pt, valid, n_dim, a.n, lane, xin);

    for (int m = 0; m < n_blk; ++m) {
      if (!staged) {
        const nb_gd* src = blk0 + m * blk_stride;
        __syncthreads();                           // readers of the last block
        for (int i = 2 * threadIdx.x; i < BLK; i += 2 * 64 * NW)
          *(double2*)(blk_lds + i) = *(const NB_G double2*)(src + i);
        __syncthreads();
        staged = n_blk == 1;
      }
      double y[TPW][4 * DT], r2[TPW];
      bool box_bad[TPW];
      ell_eval<DT, TPW>(blk_lds, n_dim, xin, lane, y, box_bad, r2);
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        k_cnt[t] += (!box_bad[t] && r2[t] < 1.0) ? 1 : 0;
        r2_out[t] = r2[t];
      }
    }

#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      if (valid[t] && lg == 0) {
        if (count) {
          a.out_u8[pt[t]] = (unsigned char)k_cnt[t];
        } else {
          a.out_f64[2 * pt[t]] = r2_out[t];
          a.out_f64[2 * pt[t] + 1] = 0.0;
        }
      }
    }
  }
  if (a.counters != nullptr && lane == 0)
    atomicAdd(&a.counters[count ? 0 : 1],
              (unsigned long long)n_blk * n_rows);
}

template <int DT>
int launch_geom(const GeomArgs& a, hipStream_t stream) {
  constexpr int TPW = DT <= 4 ? 2 : 1, NW = DT <= 4 ? 4 : 8;
  constexpr size_t lds = nb_ell_block_size(DT) * sizeof(double);
  if (const int rc = nb_allow_lds<nb_geom_kernel<DT, TPW, NW>>(lds)) return rc;
  const long long n_super = (a.n + 16 * NW * TPW - 1) / (16 * NW * TPW);
  // one workgroup per CU, striding over the 128-row passes
  const long long blocks = n_super < 256 ? n_super : 256;
  hipLaunchKernelGGL((nb_geom_kernel<DT, TPW, NW>), dim3((unsigned)blocks),
                     dim3(64 * NW), lds, stream, a);
  return NB_OK;
}

}  // namespace

int nb_launch_geom(const double* blob_dev, int dt, int count, const double* x,
                   long long n, double* out_f64, unsigned char* out_u8,
                   hipStream_t stream) {
  if (n <= 0) return NB_OK;
  GeomArgs a;
  a.blob = (const nb_gd*)blob_dev; a.count = count; a.x = (const nb_gd*)x;
  a.n = n; a.out_f64 = out_f64; a.out_u8 = out_u8;
  a.counters = nb_eval_counters();
  const int rc = nb_tile_dispatch(
      dt, [&](auto t) { return launch_geom<t()>(a, stream); });
  if (rc != NB_OK) return rc;
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}
