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

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && strcmp(argv[1], "plan") == 0) return plan(argc, argv);
  if (argc == 4 && strcmp(argv[1], "pack") == 0)
    return pack(atoi(argv[2]), argv[3]);
  fprintf(stderr, "usage: %s plan [late_only shape]... | pack n_dim dir\n",
          argv[0]);
  return 2;
}
