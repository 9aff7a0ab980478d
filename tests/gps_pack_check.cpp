// The packer of the Gaussian-process likelihood of an ordered series (pack_gps
// of nautilus_amd/csrc/nb_pack.h, the very header nb_api.hip includes) built
// on its own.  Run by tests/test_pack_gps.py, once as it is and once under the
// address and undefined-behaviour sanitizers.
//
//   gps_pack_check dir
//     runs every case: writes the packed image as raw doubles to
//     dir/<case>.bin (empty after a refusal) and prints one line per case, tab
//     separated: case, return code, doubles of the image, recorded error text
//     (empty after a success)
//
// Every input is a closed form of its index, written out again in
// test_pack_gps.py: t[j] = j (j + 1) / 2 + 1 / 4 (so that every step j is
// another number), data[j] = 3000000 + j, sigma2[j] = 1 / 2 + j.
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

struct Gps {
  int p;
  std::vector<double> t, data, sigma2;
  bool with_sigma2 = true, with_t = true, with_data = true, with_out = true;
  int kernel = NB_GPS_MATERN32;
  double log_norm = -0.5;
  explicit Gps(int n) : p(n) {
    const int m = n > 0 ? n : 1;               // arrays of the refusals too
    for (int j = 0; j < m; ++j) {
      t.push_back(0.5 * j * (j + 1.0) + 0.25);
      data.push_back(3000000.0 + j);
      sigma2.push_back(0.5 + j);
    }
  }
  void run(const char* name) {
    std::vector<double> image;
    int handle = 0;
    g_error[0] = 0;
    const int rc = pack_gps(p, with_t ? t.data() : nullptr,
                            with_data ? data.data() : nullptr,
                            with_sigma2 ? sigma2.data() : nullptr, kernel,
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
  for (int p : {1, 2, 31, 32, 33, 65, 1000}) {
    Gps g(p);
    g.run(("gps_" + std::to_string(p)).c_str());
  }
  { Gps g(37); g.with_sigma2 = false; g.run("gps_37_no_sigma2"); }
  { Gps g(5); g.kernel = NB_GPS_EXP; g.run("gps_5_first_kernel"); }
  { Gps g(5); g.kernel = NB_GPS_SHO; g.run("gps_5_last_kernel"); }
  { Gps g(5); g.t[2] = g.t[1]; g.t[3] = g.t[1]; g.run("gps_5_equal_times"); }
  { Gps g(NB_GPS_MAX_DATA); g.run("gps_most"); }
  // refusals
  { Gps g(0); g.run("gps_no_data_points"); }
  { Gps g(NB_GPS_MAX_DATA + 1); g.run("gps_too_many"); }
  { Gps g(5); g.kernel = -1; g.run("gps_kernel_below"); }
  { Gps g(5); g.kernel = 4; g.run("gps_kernel_above"); }
  { Gps g(5); g.with_t = false; g.run("gps_null_t"); }
  { Gps g(5); g.with_data = false; g.run("gps_null_data"); }
  { Gps g(5); g.with_out = false; g.run("gps_null_out"); }
  { Gps g(5); g.log_norm = nan_; g.run("gps_log_norm"); }
  { Gps g(5); g.t[0] = -inf; g.run("gps_t_inf_first"); }
  { Gps g(5); g.t[4] = inf; g.run("gps_t_inf_last"); }
  { Gps g(5); g.t[2] = nan_; g.run("gps_t_nan"); }
  { Gps g(5); g.t[3] = g.t[1]; g.run("gps_t_decreases"); }
  { Gps g(5); g.t[1] = -1.0; g.run("gps_t_decreases_at_once"); }
  {
    Gps g(5);
    g.t[0] = g.t[1] = -1.5e308;
    g.t[2] = g.t[3] = g.t[4] = 1.5e308;
    g.run("gps_step_overflows");
  }
  { Gps g(5); g.data[3] = inf; g.run("gps_data_inf"); }
  { Gps g(5); g.data[4] = nan_; g.run("gps_data_nan"); }
  { Gps g(5); g.sigma2[2] = -0.5; g.run("gps_sigma2_negative"); }
  { Gps g(5); g.sigma2[1] = inf; g.run("gps_sigma2_inf"); }
  return g_failed ? 1 : 0;
}
