// The host arithmetic of the emulator trainer (nautilus_amd/csrc/
// nb_train_plan.h, the very header nb_mlp_train.hip includes) built on its
// own.  Run by tests/test_train_plan.py.
//
//   train_plan_check plan [late_only shape]...
//     for kt1 = 1 .. 9: "rounds kt1 <records of g_jobs_rounds>", then for
//     (-1, -1) and every (late_only, shape) given: "jobs kt1 late_only shape
//     <records of g_plan>" and "sched kt1 late_only shape <its schedule>"
//   train_plan_check pack n_dim dir
//     packs the network whose weight W_l[k][h] (bias: k = rows of the layer) is
//     weight_value(l, k, h), and writes dir/w.bin (pack_network's w), dir/wt.bin
//     (its transposed tiles) and dir/back.bin (unpack_network of w: coefs and
//     intercepts of layer 1, of layer 2, ...) as raw doubles
//   train_plan_check consts
//     "NAME value" for the constants the tests would otherwise retype
//   train_plan_check xcds
//     for n = 1 .. MAX_RESIDENT + 1 networks, every mask of XCDs in use and
//     resident_allowed = 0, 1: "n mask allowed two_launch owned" and the
//     network (-1 = none) of place 0, place 1 of XCD 0, of XCD 1, ...
//   train_plan_check layout
//     for kt1 = 1 .. 9 and max_iter = 1, 2, 9999, 10000: "kt1 max_iter", the
//     double offsets W M V WT stash curve scal of pool_layout, per_net, and
//     the bytes of the block of 1 and of 16 networks
//   train_plan_check stash kt1 batch rows...
//     "large rowt per_net": stash_choice of networks with these rows, and
//     the doubles of one network in a large stash of rowt row tiles
//   train_plan_check steps rows batch
//     "batch steps_per_epoch" of epoch_steps
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define NB_H1 100      // nb_common.h (the header checks the figures)
#define NB_H2 50
#define NB_H3 20
#define NB_HT1 7
#define NB_HT2 4
#define NB_HT3 2
#define NB_TILE 256
#include "nb_train_plan.h"

namespace {

double weight_value(int l, int k, int h) {
  return (l + 1) * 100000.0 + k * 1000.0 + h + 0.25;
}

void print_line(const char* what, int kt1, const int* forced,
                const std::vector<int>& v) {
  printf("%s %d", what, kt1);
  if (forced != nullptr) printf(" %d %d", forced[0], forced[1]);
  for (int x : v) printf(" %d", x);
  printf("\n");
}

bool write_doubles(const std::string& path, const std::vector<double>& v) {
  FILE* f = fopen(path.c_str(), "wb");
  if (f == nullptr) return false;
  const bool ok = fwrite(v.data(), sizeof(double), v.size(), f) == v.size();
  return fclose(f) == 0 && ok;
}

int plan(int argc, char** argv) {
  std::vector<int> forced = {-1, -1};
  for (int i = 2; i + 1 < argc; i += 2) {
    forced.push_back(atoi(argv[i]));
    forced.push_back(atoi(argv[i + 1]));
  }
  for (int kt1 = 1; kt1 <= 9; ++kt1) {
    print_line("rounds", kt1, nullptr, g_jobs_rounds(kt1));
    for (size_t f = 0; f < forced.size(); f += 2) {
      std::vector<int> jobs, sched;
      g_plan(kt1, forced[f], forced[f + 1], jobs, sched);
      print_line("jobs", kt1, &forced[f], jobs);
      print_line("sched", kt1, &forced[f], sched);
    }
  }
  return 0;
}

int pack(int n_dim, const std::string& dir) {
  const int kt1 = (n_dim + 1 + 15) / 16;
  std::vector<std::vector<double>> c(4), b(4), c2(4), b2(4);
  const double* cp[4]; const double* bp[4];
  double* cp2[4]; double* bp2[4];
  for (int l = 0; l < 4; ++l) {
    const NetLayer y = net_layer(l, n_dim, kt1);
    for (int k = 0; k < y.rows; ++k)
      for (int h = 0; h < y.cols; ++h) c[l].push_back(weight_value(l, k, h));
    for (int h = 0; h < y.cols; ++h) b[l].push_back(weight_value(l, y.rows, h));
    c2[l].assign(c[l].size(), -1.0);
    b2[l].assign(b[l].size(), -1.0);
    cp[l] = c[l].data(); bp[l] = b[l].data();
    cp2[l] = c2[l].data(); bp2[l] = b2[l].data();
  }
  std::vector<double> w(3, -1.0), wt(5, -1.0);     // (pack_network sizes them)
  pack_network(n_dim, kt1, cp, bp, w, wt);
  unpack_network(n_dim, kt1, w.data(), cp2, bp2);
  std::vector<double> back;
  for (int l = 0; l < 4; ++l) {
    back.insert(back.end(), c2[l].begin(), c2[l].end());
    back.insert(back.end(), b2[l].begin(), b2[l].end());
  }
  if (!write_doubles(dir + "/w.bin", w) || !write_doubles(dir + "/wt.bin", wt) ||
      !write_doubles(dir + "/back.bin", back)) {
    fprintf(stderr, "cannot write under %s\n", dir.c_str());
    return 1;
  }
  return 0;
}

int consts() {
  printf("JOBS_SLOT %zu\nSCHED_SLOT %zu\nOFF_POOL %zu\n", JOBS_SLOT, SCHED_SLOT,
         OFF_POOL);
  printf("XCD_SLOTS %d\nG_ROWT %d\nXCD_COUNT %d\nMAX_RESIDENT %d\n", XCD_SLOTS,
         G_ROWT, XCD_COUNT, MAX_RESIDENT);
  printf("SMALL_BATCH %d\n", SMALL_BATCH);
  return 0;
}

int xcds() {
  for (int n = 1; n <= MAX_RESIDENT + 1; ++n)
    for (unsigned mask = 0; mask < (1u << XCD_COUNT); ++mask)
      for (int allowed = 0; allowed < 2; ++allowed) {
        const XcdPlan p = plan_xcds(n, mask, allowed != 0);
        printf("%d %u %d %d %u", n, mask, allowed, (int)p.two_launch, p.owned);
        if (p.map.n_nets != n) return 1;
        for (int x = 0; x < XCD_COUNT; ++x)
          printf(" %d %d", p.map.net[x][0], p.map.net[x][1]);
        printf("\n");
      }
  return 0;
}

int layout() {
  const int max_iters[4] = {1, 2, 9999, 10000};
  for (int kt1 = 1; kt1 <= 9; ++kt1)
    for (int max_iter : max_iters) {
      const PoolLayout p =
          pool_layout(kt1, (long long)net_layer(4, 1, kt1).off, max_iter);
      printf("%d %d %lld %lld %lld %lld %lld %lld %lld %lld %zu %zu\n", kt1,
             max_iter, p.W, p.M, p.V, p.WT, p.stash, p.curve, p.scal,
             p.per_net, block_bytes(p.per_net, 1), block_bytes(p.per_net, 16));
    }
  return 0;
}

int stash(int argc, char** argv) {
  std::vector<long long> rows;
  for (int i = 4; i < argc; ++i) rows.push_back(atoll(argv[i]));
  const StashChoice c = stash_choice(rows, atoi(argv[3]));
  printf("%d %d %lld\n", (int)c.large, c.rowt,
         large_per_net(c.rowt, atoi(argv[2])));
  return 0;
}

int steps(long long rows, int batch) {
  const EpochSteps e = epoch_steps(rows, batch);
  printf("%d %d\n", e.batch, e.steps);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && strcmp(argv[1], "plan") == 0) return plan(argc, argv);
  if (argc == 4 && strcmp(argv[1], "pack") == 0)
    return pack(atoi(argv[2]), argv[3]);
  if (argc == 2 && strcmp(argv[1], "consts") == 0) return consts();
  if (argc == 2 && strcmp(argv[1], "xcds") == 0) return xcds();
  if (argc == 2 && strcmp(argv[1], "layout") == 0) return layout();
  if (argc >= 5 && strcmp(argv[1], "stash") == 0) return stash(argc, argv);
  if (argc == 4 && strcmp(argv[1], "steps") == 0)
    return steps(atoll(argv[2]), atoi(argv[3]));
  fprintf(stderr, "usage: %s plan [late_only shape]... | pack n_dim dir | "
          "consts | xcds | layout | stash kt1 batch rows... | steps rows "
          "batch\n", argv[0]);
  return 2;
}
