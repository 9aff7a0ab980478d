// Shared device/host definitions for the nautilus hot path on gfx950 (MI355X).
//
// Everything is fp64, like the reference (all arrays are
// float64 C-contiguous (N, D)).  Wavefront = 64 lanes, hard-coded.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nb_layout.h"   // sizes, offsets, header words, error codes

#define NB_WAVE 64

typedef double nb_d4 __attribute__((ext_vector_type(4)));
// a pair of doubles at an 8-byte-aligned address: one 16-byte load
// (global_load_dwordx4 needs dword alignment only) -- the rows of an odd n_dim
typedef double nb_d2u __attribute__((ext_vector_type(2), aligned(8)));

// Pointers to global memory, typed as such for device code.  A pointer the
// compiler cannot trace back to a kernel argument -- loaded from a descriptor
// in memory, or laundered through an empty asm -- is a generic ("flat")
// pointer to it: every access becomes flat_load / flat_store, which count
// against the LDS counter as well (each wait for an LDS read then also waits
// for every global load in flight) and cannot use scalar-base addressing.
// (Casting back and forth does not help: the optimiser folds the round trip;
// the pointer has to keep the address space in its type.)
#if defined(__HIP_DEVICE_COMPILE__)
#define NB_G __attribute__((address_space(1)))
#else
#define NB_G
#endif
typedef NB_G double nb_gd;
typedef NB_G int nb_gi;

// header word i of a bound blob (nb_layout.h)
__host__ __device__ inline int64_t nb_hdr(const double* blob, int i) {
  return ((const int64_t*)blob)[i];
}

// One (bound, neural bound) group of a two-stage query (nb_cand.hip ->
// nb_eval_fast.hip, BATCH): built on the host when a bound / a bound list is
// created, read by the second stage per 128-point pass.
struct FastGroup {
  const double* nb;               // neural block inside the bound's blob
  const double* shift;            // the bound's periodic shift block or null
  int E;                          // networks
  int b;                          // position of the bound in its list
};

// ---------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11).  Stream layout: DESIGN.md "RNG
// contract" / oracle/philox.py.
// ---------------------------------------------------------------------------
#define NB_TAG_CTRL 0u
#define NB_TAG_NORMAL 1u
#define NB_TAG_CUBE 2u

struct nb_u4 { uint32_t x, y, z, w; };

__host__ __device__ inline nb_u4 nb_philox(uint32_t c0, uint32_t c1, uint32_t c2,
                                           uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  nb_u4 o = {c0, c1, c2, c3};
  return o;
}

__host__ __device__ inline double nb_unit(uint32_t hi, uint32_t lo) {
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6)) *
         (1.0 / 9007199254740992.0);
}

// uniform in (0, 1) from ONE word: (w + 1/2) / 2^32 (the normals of the
// proposal draw: 2^-32 is far below anything a direction on the sphere can
// resolve statistically, and a Philox call then feeds two Box-Muller pairs)
__host__ __device__ inline double nb_unit32(uint32_t w) {
  return ((double)w + 0.5) * (1.0 / 4294967296.0);
}

// two uniforms in [0,1) for proposal g, block, tag
__host__ __device__ inline void nb_uniform_pair(uint64_t seed, uint64_t g,
                                                uint32_t block, uint32_t tag,
                                                double& u0, double& u1) {
  nb_u4 w = nb_philox((uint32_t)g, (uint32_t)(g >> 32), block, tag,
                      (uint32_t)seed, (uint32_t)(seed >> 32));
  u0 = nb_unit(w.x, w.y);
  u1 = nb_unit(w.z, w.w);
}

// a failed HIP call inside an export: record it (nb_layout.h) and return
#define NB_HIP_CHECK(expr)                                                   \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) {                                                  \
      nb_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),    \
                   __FILE__, __LINE__);                                      \
      return NB_ERR_HIP;                                                     \
    }                                                                        \
  } while (0)
