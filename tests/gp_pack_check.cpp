// The packer of the Gaussian-process likelihood (pack_gp of
// nautilus_amd/csrc/nb_pack.h, the very header nb_api.hip includes) built on
// its own.  Run by tests/test_pack_gp.py, once as it is and once under the
// address and undefined-behaviour sanitizers.
//
//   gp_pack_check dir
//     runs every case: writes the packed image as raw doubles to
//     dir/<case>.bin (empty after a refusal) and prints one line per case, tab
//     separated: case, return code, doubles of the image, recorded error text
//     (empty after a success)
//
// Every input is a closed form of its indices, written out again in
// test_pack_gp.py: data[j] = 3000000 + j, sigma2[j] = 1 / 2 + j, dist[j][k] =
// 1000 max(j, k) + min(j, k) + 1 / 2 off the diagonal.  All of them are
// nonzero and distinct, so that a swapped or transposed index cannot hide.
#include <cstdarg>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "nb_pack.h"

static char g_error[1024];

void nb_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

namespace {

const double inf = std::numeric_limits<double>::infinity();
const double nan_ = std::numeric_limits<double>::quiet_NaN();

std::string g_dir;
bool g_failed = false;

struct Gp {
  int p;
  std::vector<double> data, sigma2, dist;
  bool with_sigma2 = true, with_dist = true, with_data = true,
       with_out = true;
  int kernel = NB_GP_MATERN32;
  double log_norm = -0.5;
  explicit Gp(int n) : p(n) {
    const int m = n > 0 ? n : 1;               // arrays of the refusals too
    for (int j = 0; j < m; ++j) {
      data.push_back(3000000.0 + j);
      sigma2.push_back(0.5 + j);
    }
    dist.assign((size_t)m * m, 0.0);
    for (int j = 0; j < m; ++j)
      for (int k = 0; k < m; ++k)
        if (j != k)
          dist[(size_t)j * m + k] =
              1000.0 * (j > k ? j : k) + (j > k ? k : j) + 0.5;
  }
  void run(const char* name) {
    std::vector<double> image;
    int handle = 0;
    g_error[0] = 0;
    const int rc = pack_gp(p, with_data ? data.data() : nullptr,
                           with_sigma2 ? sigma2.data() : nullptr,
                           with_dist ? dist.data() : nullptr, kernel,
                           log_norm, with_out ? &handle : nullptr, &image);
    const size_t count = rc == NB_OK ? image.size() : 0;
    const std::string path = g_dir + "/" + name + ".bin";
    FILE* f = fopen(path.c_str(), "wb");
    if (f == nullptr ||
        (count > 0 && fwrite(image.data(), 8, count, f) != count) ||
        fclose(f) != 0) {
      fprintf(stderr, "cannot write %s\n", path.c_str());
      g_failed = true;
    }
    printf("%s\t%d\t%zu\t%s\n", name, rc, count, rc != NB_OK ? g_error : "");
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s dir\n", argv[0]);
    return 2;
  }
  g_dir = argv[1];
  for (int p : {1, 2, 16, 17, 37, 64, 127, 128}) {
    Gp g(p);
    g.run(("gp_" + std::to_string(p)).c_str());
  }
  { Gp g(37); g.with_dist = false; g.run("gp_37_no_dist"); }
  { Gp g(37); g.with_sigma2 = false; g.run("gp_37_no_sigma2"); }
  { Gp g(5); g.kernel = NB_GP_SQEXP; g.run("gp_5_first_kernel"); }
  { Gp g(5); g.kernel = NB_GP_MATERN52; g.run("gp_5_last_kernel"); }
  // refusals
  { Gp g(0); g.run("gp_no_data_points"); }
  { Gp g(129); g.run("gp_too_many"); }
  { Gp g(5); g.kernel = -1; g.run("gp_kernel_below"); }
  { Gp g(5); g.kernel = 4; g.run("gp_kernel_above"); }
  { Gp g(5); g.with_data = false; g.run("gp_null_data"); }
  { Gp g(5); g.with_out = false; g.run("gp_null_out"); }
  { Gp g(5); g.log_norm = nan_; g.run("gp_log_norm"); }
  { Gp g(5); g.data[3] = inf; g.run("gp_data_inf"); }
  { Gp g(5); g.data[4] = nan_; g.run("gp_data_nan"); }
  { Gp g(5); g.sigma2[2] = -0.5; g.run("gp_sigma2_negative"); }
  { Gp g(5); g.sigma2[1] = inf; g.run("gp_sigma2_inf"); }
  { Gp g(5); g.dist[3 * 5 + 1] = 7.0; g.run("gp_dist_asymmetric"); }
  { Gp g(5); g.dist[1 * 5 + 3] = 7.0; g.run("gp_dist_asymmetric_upper"); }
  {
    Gp g(5);
    g.dist[4 * 5 + 2] = g.dist[2 * 5 + 4] = -1.0;
    g.run("gp_dist_negative");
  }
  {
    Gp g(5);
    g.dist[4 * 5 + 0] = g.dist[0 * 5 + 4] = inf;
    g.run("gp_dist_inf");
  }
  {
    Gp g(5);
    g.dist[2 * 5 + 1] = g.dist[1 * 5 + 2] = nan_;
    g.run("gp_dist_nan");
  }
  { Gp g(5); g.dist[3 * 5 + 3] = 1.0; g.run("gp_dist_diagonal"); }
  return g_failed ? 1 : 0;
}
