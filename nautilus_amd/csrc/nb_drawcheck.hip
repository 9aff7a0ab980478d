// Diagnostic entries for the Box-Muller arithmetic of the proposal draw
// (nb_draw.h): the functions themselves, word by word, for the tests.  Not on
// any hot path.
#include "nb_common.h"
#include "../../include/nautilus_hip.h"

#include "nb_draw.h"

namespace {

__global__ void __launch_bounds__(256)
nb_draw_words_kernel(const uint32_t* __restrict__ w0,
                     const uint32_t* __restrict__ w1, long long n,
                     double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = w0[i], b = w1[i];
  double sn, cs, z0, z1;
  draw_sincos(nb_unit32(b), sn, cs);
  draw_normal_pair(a, b, z0, z1);
  double* o = out + 5 * i;
  o[0] = draw_log(nb_unit32(a));
  o[1] = sn;
  o[2] = cs;
  o[3] = z0;
  o[4] = z1;
}

// A wavefront visits tiles of SW_TILE consecutive words (aligned to SW_TILE,
// so that a tile lies in one chunk: chunk_words is a multiple of it), 64 words
// per step, one per lane.
constexpr int SW_TILE = 4096;

// |got - lib| in ulp of lib (finite), as the bits of a float: non-negative
// floats order like their bits.  NaN counts as +inf.
__device__ __forceinline__ unsigned long long sweep_key(double got, double lib,
                                                        uint32_t w) {
  float d = 0.0f;
  if (got != lib) {
    d = INFINITY;
    if (lib != 0.0) {
      const float f = (float)(fabs(got - lib) / ldexp(1.0, ilogb(lib) - 52));
      if (f <= 3.0e38f) d = f;
    }
  }
  return ((unsigned long long)__float_as_uint(d) << 32) | w;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(v, o);
    v = other > v ? other : v;
  }
  return v;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// stats: [0..2] words with a bad log / sine / cosine, then for each of the
// three n_chunks keys (largest difference from the library, its word), chunk
// c holding the words of [(chunk0 + c) chunk_words, (chunk0 + c + 1)
// chunk_words).  Zeroed before the launch.
__global__ void __launch_bounds__(256)
nb_draw_sweep_kernel(unsigned long long first, unsigned long long count,
                     unsigned long long chunk_words, unsigned long long chunk0,
                     long long n_chunks, unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const unsigned long long wave =
      (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const unsigned long long n_waves = (unsigned long long)gridDim.x * 4;
  const unsigned long long tile_end = (first + count - 1) / SW_TILE + 1;
  unsigned long long bad[3] = {0, 0, 0};
  for (unsigned long long tile = first / SW_TILE + wave; tile < tile_end;
       tile += n_waves) {
    unsigned long long key[3] = {0, 0, 0};
    for (int j = 0; j < SW_TILE / 64; ++j) {
      const unsigned long long w64 = tile * SW_TILE + j * 64 + lane;
      if (w64 < first || w64 - first >= count) continue;
      const uint32_t w = (uint32_t)w64;
      const double u = nb_unit32(w);
      double got[3], lib[3];
      got[0] = draw_log(u);
      draw_sincos(u, got[1], got[2]);
      lib[0] = log(u);
      sincospi(2.0 * u, &lib[1], &lib[2]);
      bad[0] += !(got[0] < 0.0 && got[0] > -INFINITY);
      bad[1] += !(fabs(got[1]) <= 1.0);
      bad[2] += !(fabs(got[2]) <= 1.0);
#pragma unroll
      for (int f = 0; f < 3; ++f) {
        const unsigned long long k = sweep_key(got[f], lib[f], w);
        key[f] = k > key[f] ? k : key[f];
      }
    }
    const unsigned long long chunk = tile * SW_TILE / chunk_words - chunk0;
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const unsigned long long k = wave_max(key[f]);
      if (lane == 0) atomicMax(&stats[3 + f * n_chunks + chunk], k);
    }
  }
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const unsigned long long s = wave_sum(bad[f]);
    if (lane == 0 && s != 0) atomicAdd(&stats[f], s);
  }
}

}  // namespace

int nb_draw_words(const uint32_t* w0_dev, const uint32_t* w1_dev, int64_t n,
                  double* out_dev, void* stream) {
  if (n <= 0) return NB_OK;
  if (w0_dev == nullptr || w1_dev == nullptr || out_dev == nullptr) {
    nb_set_error("nb_draw_words: null argument");
    return NB_ERR_ARG;
  }
  hipLaunchKernelGGL(nb_draw_words_kernel, dim3((unsigned)((n + 255) / 256)),
                     dim3(256), 0, (hipStream_t)stream, w0_dev, w1_dev,
                     (long long)n, out_dev);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}

int nb_draw_sweep(uint64_t first, uint64_t count, uint64_t chunk_words,
                  uint64_t* stats_dev, void* stream) {
  const uint64_t all = 1ull << 32;
  if (stats_dev == nullptr || first >= all || count > all - first ||
      chunk_words == 0 || chunk_words % SW_TILE != 0) {
    nb_set_error("nb_draw_sweep: words %llu + %llu beyond 2^32, or chunks of "
                 "%llu words (a positive multiple of %d)",
                 (unsigned long long)first, (unsigned long long)count,
                 (unsigned long long)chunk_words, SW_TILE);
    return NB_ERR_ARG;
  }
  const int64_t n_chunks =
      count == 0 ? 0
                 : (int64_t)((first + count - 1) / chunk_words -
                             first / chunk_words + 1);
  if (n_chunks > NB_DRAW_SWEEP_MAX_CHUNKS) {
    nb_set_error("nb_draw_sweep: %lld chunks (at most %d)",
                 (long long)n_chunks, NB_DRAW_SWEEP_MAX_CHUNKS);
    return NB_ERR_ARG;
  }
  NB_HIP_CHECK(hipMemsetAsync(stats_dev, 0, (3 + 3 * n_chunks) * 8,
                              (hipStream_t)stream));
  if (count == 0) return NB_OK;
  const uint64_t tiles = (first + count - 1) / SW_TILE - first / SW_TILE + 1;
  const uint64_t blocks = (tiles + 3) / 4;
  hipLaunchKernelGGL(nb_draw_sweep_kernel,
                     dim3((unsigned)(blocks < 2048 ? blocks : 2048)),
                     dim3(256), 0, (hipStream_t)stream,
                     (unsigned long long)first, (unsigned long long)count,
                     (unsigned long long)chunk_words,
                     (unsigned long long)(first / chunk_words),
                     (long long)n_chunks, (unsigned long long*)stats_dev);
  NB_HIP_CHECK(hipGetLastError());
  return NB_OK;
}
