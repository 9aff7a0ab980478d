// Asynchronous global -> LDS copy of operand tiles, shared by the two panel
// kernels (nb_chi2.hip, nb_fold.hip): device code only.
#pragma once
#include "nb_common.h"

namespace {

typedef const void __attribute__((address_space(1))) * nb_gptr;
typedef void __attribute__((address_space(3))) * nb_lptr;

// s_waitcnt vmcnt(0) (expcnt and lgkmcnt left at their maxima)
__device__ __forceinline__ void nb_wait_copies() {
  __builtin_amdgcn_s_waitcnt(0x0F70);
}

// n_tiles operand tiles by the whole workgroup of WAVES wavefronts in 1 KB
// pieces (destination = uniform base + lane * 16)
template <int WAVES>
__device__ __forceinline__ void nb_copy_tiles(const nb_gd* __restrict__ src,
                                              double* dst, int n_tiles,
                                              int wave, int lane) {
  for (int c = wave; c < 2 * n_tiles; c += WAVES)
    __builtin_amdgcn_global_load_lds((nb_gptr)(src + c * 128 + 2 * lane),
                                     (nb_lptr)(dst + c * 128), 16, 0, 0);
}

}  // namespace
