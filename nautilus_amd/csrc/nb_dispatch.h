// Which instantiation a launcher picks: the kernels on rows of n_dim doubles
// are compiled once per number of 16-wide tiles, and the streaming ones once
// more per shape of the last, partly filled tile.  Both rules live here and
// nowhere else.  Plain C++ without HIP, so that tests/dispatch_check.cpp builds
// it on its own.  The idiom is that of nb_stream_dispatch (nb_launch.h): a
// generic lambda receives the compile-time value as a tag argument,
//   nb_tile_dispatch(dt, [&](auto t) { return launch<t()>(args); });
#pragma once

#include <type_traits>

#include "nb_layout.h"

// augmented rows (x, 1): nb_mvee.hip, nb_gmm.hip and layer 1 of the trainer
#define NB_MAX_AUG_DT (NB_MAX_DT + 1)

// launch(std::integral_constant<int, T>()) for the T in 1..MAX that equals
// `tiles`; any other count, zero and negative included, has no kernel
template <int MAX = NB_MAX_DT, int T = 1, class F>
int nb_tile_dispatch(int tiles, F launch) {
  if constexpr (T > MAX) {
    nb_set_error("no kernel for %d tiles of 16 (1..%d are compiled)", tiles,
                 MAX);
    return NB_ERR_UNSUPPORTED;
  } else {
    if (tiles == T) return launch(std::integral_constant<int, T>());
    return nb_tile_dispatch<MAX, T + 1>(tiles, launch);
  }
}

// The last tile of a row of n_dim: kl = k-steps of 4 that hold real features
// (whole pairs of them: 4 DT, or 4 DT - 2 when the upper half of the last tile
// is padding); small = the last row tile has at most four real rows, so a
// 4x4x4 product covers it (nb_stream.hip).  small implies kl = 4 DT - 2.
struct nb_tail {
  int kl;
  bool small;
};
constexpr nb_tail nb_tail_of(int n_dim) {
  return {2 * ((n_dim + 7) >> 3), (n_dim & 15) >= 1 && (n_dim & 15) <= 4};
}

// launch(DT, KL, SMALL) as tags, for the three variants the streaming kernels
// (nb_stream.hip, nb_mixture.hip) are compiled in per tile count:
// <4 DT, false>, <4 DT - 2, true>, <4 DT - 2, false>.
// device.mixture_launch_shape repeats it for the tests.
template <class F>
int nb_row_dispatch(int n_dim, F launch) {
  return nb_tile_dispatch((n_dim + 15) / 16, [&](auto dt) {
    constexpr int DT = decltype(dt)::value;
    const nb_tail t = nb_tail_of(n_dim);
    if (t.kl == 4 * DT)
      return launch(dt, std::integral_constant<int, 4 * DT>(),
                    std::false_type());
    // (beyond 64 dimensions -- one or two tiles per wavefront -- the 4x4x4
    // tiles pay since the operands are read ahead: stream_quadform_ahead)
    if (t.small)
      return launch(dt, std::integral_constant<int, 4 * DT - 2>(),
                    std::true_type());
    return launch(dt, std::integral_constant<int, 4 * DT - 2>(),
                  std::false_type());
  });
}
