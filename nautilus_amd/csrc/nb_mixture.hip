// Log-density of a weighted, full-covariance Gaussian mixture in one kernel
// (the user-side likelihood callable of reference sampler.py:863-873):
//     log L(x) = logsumexp_k [ a_k - 1/2 |L_k^-1 (x - mu_k)|^2 ],
//     a_k = log w_k - D/2 log 2 pi - sum_i log (L_k)_ii,  Sigma_k = L_k L_k^T
// and, optionally, the index of the largest term.
//
// Algorithmic traffic: 8 D bytes read + 8 (+ 4) written per point, K D (D + 1)
// flop per point.  The quadratic form is the contraction of nb_stream.hip
// (nb_quadform.h) with the same operand layout; what is new is the loop over
// the components AROUND a point that stays in registers:
//  * a wavefront owns TPW tiles of 16 points; a point's row is read once, with
//    the pair loads and the permuted K order of nb_stream.hip, and kept raw.
//    Per component the centred operand d = x - mu_k is formed in registers
//    (mu_k from LDS, 4 distinct 16-byte addresses per read);
//  * a component is one record of the blob (nb_layout.h,
//    nb_mixture_record): its lower-triangular
//    L_k^-1 as K-permuted 16x16 tiles, mu_k zero padded to 16 DT, a_k.  Where
//    all K records fit the LDS of a CU they are copied once per workgroup and
//    stay for its whole loop over points.  Otherwise they stream through two
//    LDS regions: while the matrix cores work on one, global_load_lds fills
//    the other with the record after it (one barrier per component; every
//    wavefront of the workgroup then walks the components in step, and a
//    staged record serves the 8 TPW tiles of the workgroup).  Two records fit
//    up to n_dim 128 (2 x 74 KB), so no single-buffered variant exists;
//  * r^2 is reduced over the 4 lanes of a point; the term folds into a running
//    (max, sum scaled by exp(-max)) pair in fp64, so no K-wide array of terms
//    exists anywhere.  The label is the first k that attains the maximum.
#include "nb_common.h"
#include "nb_launch.h"
#include "nb_quadform.h"

#include <cfloat>

namespace {

constexpr int MX_WAVES = 8;                     // wavefronts of a workgroup
constexpr size_t MX_LDS_BYTES = 160 * 1024;     // LDS of a CU

typedef const void __attribute__((address_space(1))) * mx_gptr;
typedef void __attribute__((address_space(3))) * mx_lptr;

// asynchronous global -> LDS copy of n_doubles (a multiple of 128) by the
// whole workgroup: every wavefront moves 1 KB chunks (destination = uniform
// base + lane * 16); complete after vmcnt(0) and a workgroup barrier
__device__ __forceinline__ void mx_copy(const nb_gd* __restrict__ src,
                                        double* dst, int n_doubles, int wave,
                                        int lane) {
  for (int c = wave * 128; c < n_doubles; c += MX_WAVES * 128)
    __builtin_amdgcn_global_load_lds((mx_gptr)(src + c + 2 * lane),
                                     (mx_lptr)(dst + c), 16, 0, 0);
}

// s_waitcnt vmcnt(0) (expcnt and lgkmcnt left at their maxima)
__device__ __forceinline__ void mx_wait_copies() {
  __builtin_amdgcn_s_waitcnt(0x0F70);
}

// the raw rows of the TPW tiles of group `grp` in the permuted K order: slot
// (2j + o) <-> feature 8j + 2lg + o.  No masking: a slot past n_dim holds an
// element of the point's own row (the clamped address) and meets exact zeros
// in the tiles; a tile past the end of the batch holds the last row.
template <int DT, int TPW>
__device__ __forceinline__ void mx_load_rows(const double* __restrict__ x,
                                             long long n, int n_dim,
                                             long long grp, int lane,
                                             double (&xr)[TPW][4 * DT]) {
  const int li = lane & 15, lg = lane >> 4;
  const bool even = (n_dim & 1) == 0;
  if (n_dim == 1) {
    // (a pair load would reach in front of or behind the array)
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const long long pt = (grp * TPW + t) * 16 + li;
      const double v0 = x[pt < n ? pt : n - 1];
#pragma unroll
      for (int s = 0; s < 4 * DT; ++s) xr[t][s] = v0;
    }
  } else {
    // odd n_dim: the pair that holds the row's last feature is read one
    // element earlier -- (x[D-2], x[D-1]) -- so that nothing behind the array
    // is touched.  The addresses are selects, not branches: all loads of a
    // group issue back to back
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const long long pt = (grp * TPW + t) * 16 + li;
      const double* row = x + (pt < n ? pt : n - 1) * n_dim;
#pragma unroll
      for (int j = 0; j < 2 * DT; ++j) {
        const int f = 8 * j + 2 * lg;
        const bool half = !even && f + 1 == n_dim;
        const int at = even ? (f < n_dim ? f : n_dim - 2)
                            : (f + 1 < n_dim ? f : (half ? f - 1 : 0));
        const nb_d2u v = *(const nb_d2u*)(row + at);
        xr[t][2 * j] = half ? v.y : v.x;
        xr[t][2 * j + 1] = v.y;
      }
    }
  }
}

// running logsumexp of a tile's points: max, sum of exp(term - max), argmax
struct MxFold { double best, sum; int arg; };

// folds component k, whose record sits at `wl` in LDS, into the TPW tiles
template <int DT, int TPW, int KL, bool SMALL>
__device__ __forceinline__ void mx_component(const double* wl, int n_dim,
                                             int lane, int k,
                                             const double (&xr)[TPW][4 * DT],
                                             MxFold (&acc)[TPW]) {
  constexpr int NT = DT * (DT + 1) / 2;
  const int lg = lane >> 4;
  const double* mu = wl + NT * NB_TILE;
  const double coef = mu[16 * DT];
  double d[TPW][4 * DT];
#pragma unroll
  for (int j = 0; j < 2 * DT; ++j) {
    const double2 m = *(const double2*)(mu + 8 * j + 2 * lg);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      d[t][2 * j] = xr[t][2 * j] - m.x;
      d[t][2 * j + 1] = xr[t][2 * j + 1] - m.y;
    }
  }
  double part[TPW];
  if constexpr (DT >= 5)
    stream_quadform_ahead<DT, TPW, KL, SMALL>(wl, lane, d, part);
  else
    stream_quadform<DT, TPW, KL, SMALL>(wl, n_dim, lane, d, part);
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    double r2 = part[t];
    r2 += __shfl_xor(r2, 16);
    r2 += __shfl_xor(r2, 32);
    const double term = fma(-0.5, r2, coef);
    const bool up = term > acc[t].best;            // strict: the first maximum
    const double e = exp(up ? acc[t].best - term : term - acc[t].best);
    acc[t].sum = up ? fma(acc[t].sum, e, 1.0) : acc[t].sum + e;
    acc[t].best = up ? term : acc[t].best;
    acc[t].arg = up ? k : acc[t].arg;
  }
}

template <int TPW>
__device__ __forceinline__ void mx_reset(MxFold (&acc)[TPW]) {
#pragma unroll
  for (int t = 0; t < TPW; ++t) acc[t] = MxFold{-DBL_MAX, 0.0, 0};
}

template <int TPW>
__device__ __forceinline__ void mx_store(const MxFold (&acc)[TPW],
                                         long long grp, int lane, long long n,
                                         double* __restrict__ out,
                                         int* __restrict__ label) {
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const long long pt = (grp * TPW + t) * 16 + (lane & 15);
    if ((lane >> 4) == 0 && pt < n) {
      out[pt] = acc[t].best + log(acc[t].sum);
      if (label != nullptr) label[pt] = acc[t].arg;
    }
  }
}

// All n_comp records fit the LDS: copied once, every wavefront then walks its
// groups of tiles on its own.
template <int DT, int TPW, int KL, bool SMALL>
__global__ void __launch_bounds__(64 * MX_WAVES)
nb_mixture_resident_kernel(const double* __restrict__ blob, int n_dim,
                           int n_comp, const double* __restrict__ x,
                           long long n, double* __restrict__ out,
                           int* __restrict__ label) {
  constexpr int CS = nb_mixture_record(DT);
  extern __shared__ __attribute__((aligned(16))) double mx_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  mx_copy((const nb_gd*)blob, mx_lds, n_comp * CS, wave, lane);
  mx_wait_copies();
  __syncthreads();

  const long long n_groups = (n + 16 * TPW - 1) / (16 * TPW);
  for (long long grp = (long long)blockIdx.x * MX_WAVES + wave; grp < n_groups;
       grp += (long long)gridDim.x * MX_WAVES) {
    double xr[TPW][4 * DT];
    mx_load_rows<DT, TPW>(x, n, n_dim, grp, lane, xr);
    MxFold acc[TPW];
    mx_reset<TPW>(acc);
    for (int k = 0; k < n_comp; ++k)
      mx_component<DT, TPW, KL, SMALL>(mx_lds + k * CS, n_dim, lane, k, xr,
                                       acc);
    mx_store<TPW>(acc, grp, lane, n, out, label);
  }
}

// The records stream through two LDS regions: while the matrix cores work on
// one, the record after it arrives in the other.  One barrier per component:
// behind it the record has landed in every wavefront's share of its region
// and nobody reads the other region any more.  The wavefronts of a workgroup
// walk the components in step (workgroup-uniform trip counts: a wavefront
// without points of its own works on the last row and stores nothing), and a
// staged record serves the 8 TPW tiles of the workgroup.  The regions are two
// arrays, and the component loop is unrolled by two so that each access names
// its array: the compiler's wait for a copy in flight then falls only in
// front of reads of the region being filled.
template <int DT, int TPW, int KL, bool SMALL>
__global__ void __launch_bounds__(64 * MX_WAVES)
nb_mixture_stream_kernel(const double* __restrict__ blob, int n_dim,
                         int n_comp, const double* __restrict__ x, long long n,
                         double* __restrict__ out, int* __restrict__ label) {
  constexpr int CS = nb_mixture_record(DT);
  __shared__ __attribute__((aligned(16))) double reg_a[CS];
  __shared__ __attribute__((aligned(16))) double reg_b[CS];
  const nb_gd* rec = (const nb_gd*)blob;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  mx_copy(rec, reg_a, CS, wave, lane);             // record 0

  const long long n_groups = (n + 16 * TPW - 1) / (16 * TPW);
  const long long stride = (long long)gridDim.x * MX_WAVES;
  for (long long base = (long long)blockIdx.x * MX_WAVES; base < n_groups;
       base += stride) {
    const long long grp = base + wave;
    const bool more = base + stride < n_groups;    // another round follows
    double xr[TPW][4 * DT];
    mx_load_rows<DT, TPW>(x, n, n_dim, grp, lane, xr);
    MxFold acc[TPW];
    mx_reset<TPW>(acc);
    // every round starts with record 0 in (or on its way to) region a
    for (int k = 0; k < n_comp; k += 2) {
      mx_wait_copies();
      __syncthreads();
      if (k + 1 < n_comp)
        mx_copy(rec + (size_t)(k + 1) * CS, reg_b, CS, wave, lane);
      mx_component<DT, TPW, KL, SMALL>(reg_a, n_dim, lane, k, xr, acc);
      if (k + 1 < n_comp) {
        mx_wait_copies();
        __syncthreads();
        if (k + 2 < n_comp)
          mx_copy(rec + (size_t)(k + 2) * CS, reg_a, CS, wave, lane);
        else if (more)
          mx_copy(rec, reg_a, CS, wave, lane);
        mx_component<DT, TPW, KL, SMALL>(reg_b, n_dim, lane, k + 1, xr, acc);
      } else if (more) {
        // odd n_comp: region a is free once every wavefront is through
        __syncthreads();
        mx_copy(rec, reg_a, CS, wave, lane);
      }
    }
    mx_store<TPW>(acc, grp, lane, n, out, label);
  }
}

template <int DT, int KL, bool SMALL>
int launch_variant(const double* blob, int n_dim, int n_comp, const double* x,
                   long long n, double* out, int* label, hipStream_t stream) {
  // tiles per wavefront: the raw rows AND the centred operands of a component
  // are live together, 16 DT registers per tile
  constexpr int TPW = (DT <= 2) ? 4 : (DT <= 4 ? 2 : 1);
  constexpr size_t record = (size_t)nb_mixture_record(DT) * sizeof(double);
  const long long n_groups = (n + 16 * TPW - 1) / (16 * TPW);
  long long blocks = (n_groups + MX_WAVES - 1) / MX_WAVES;
  (void)hipGetLastError();
  if ((size_t)n_comp * record > MX_LDS_BYTES) {
    if (blocks > 256) blocks = 256;                // one workgroup per CU
    hipLaunchKernelGGL((nb_mixture_stream_kernel<DT, TPW, KL, SMALL>),
                       dim3((unsigned)blocks), dim3(64 * MX_WAVES), 0, stream,
                       blob, n_dim, n_comp, x, n, out, label);
    NB_HIP_CHECK(hipGetLastError());
    return NB_OK;
  }
  const size_t lds = (size_t)n_comp * record;
  constexpr auto kernel = nb_mixture_resident_kernel<DT, TPW, KL, SMALL>;
  if (const int rc = nb_allow_lds<kernel>(lds)) return rc;
  // as many workgroups as the LDS lets a CU hold (at most two by registers),
  // on 256 CUs
  const long long per_cu = MX_LDS_BYTES / lds < 2 ? 1 : 2;
  if (blocks > 256 * per_cu) blocks = 256 * per_cu;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64 * MX_WAVES), lds,
                     stream, blob, n_dim, n_comp, x, n, out, label);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}

}  // namespace

// blob: n_comp records of nb_mixture_record(DT) doubles (nb_pack.h,
// nb_mixture_create): DT(DT+1)/2 lower-triangular 16x16 tiles of
// W[k][h] = L^-1[h][k] with the K permutation of nb_stream.hip, then mu zero
// padded to 16 DT, then a_k.
int nb_launch_mixture(const double* blob, int n_dim, int n_comp,
                      const double* x, long long n, double* out, int* label,
                      hipStream_t stream) {
  if (n <= 0) return NB_OK;
  return nb_row_dispatch(n_dim, [&](auto dt, auto kl, auto small) {
    return launch_variant<dt(), kl(), small()>(blob, n_dim, n_comp, x, n, out,
                                               label, stream);
  });
}
