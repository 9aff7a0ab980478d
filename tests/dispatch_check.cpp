// The launchers' choice of instantiation (nautilus_amd/csrc/nb_dispatch.h, the
// very header the kernel files include) built on its own.  Run by
// tests/test_dispatch.py.  Prints, space separated:
//
//   row <n_dim> <rc> <DT> <KL> <SMALL> <kl> <small>   n_dim 1..128: what
//     nb_row_dispatch chose (tags) and what nb_tail_of gave (values)
//   tile <MAX> <tiles> <rc> <T> <error set: 0 / 1>    MAX 8 and 9, tiles
//     -1..10: what nb_tile_dispatch chose (T = 0: the lambda did not run)
//   over 129 <rc> <error set>                         nb_row_dispatch(129)
#include <cstdarg>
#include <cstdio>

#include "nb_dispatch.h"

static bool g_error;

void nb_set_error(const char*, ...) { g_error = true; }

template <int MAX>
static void tiles() {
  for (int t = -1; t <= 10; ++t) {
    int chosen = 0;
    g_error = false;
    const int rc = nb_tile_dispatch<MAX>(t, [&](auto tag) {
      chosen = tag();
      return NB_OK;
    });
    printf("tile %d %d %d %d %d\n", MAX, t, rc, chosen, (int)g_error);
  }
}

int main() {
  for (int n_dim = 1; n_dim <= 128; ++n_dim) {
    int dt = 0, kl = 0, sm = -1;
    const int rc = nb_row_dispatch(n_dim, [&](auto d, auto k, auto s) {
      dt = d(); kl = k(); sm = s();
      return NB_OK;
    });
    const nb_tail t = nb_tail_of(n_dim);
    printf("row %d %d %d %d %d %d %d\n", n_dim, rc, dt, kl, sm, t.kl,
           (int)t.small);
  }
  tiles<NB_MAX_DT>();
  tiles<NB_MAX_AUG_DT>();
  // a row past the last tile count has no kernel either
  g_error = false;
  const int rc = nb_row_dispatch(129, [](auto, auto, auto) { return NB_OK; });
  printf("over 129 %d %d\n", rc, (int)g_error);
  return 0;
}
