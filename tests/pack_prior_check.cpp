// pack_prior_table of the library (nautilus_amd/csrc/nb_pack.h, the very
// header nb_api.hip includes) on tables with the closed-form kinds 7 to 17,
// built on its own like pack_check.cpp.  Run by tests/test_pack_prior.py.
//
//   pack_prior_check dir
//     runs every case: writes the packed image as raw bytes to dir/<case>.bin
//     (empty after a refusal) and prints one line per case, tab separated:
//     case, return code, level (-1 after a refusal), bytes of the image,
//     recorded error text (empty after a success)
//
// The inputs are those of pack_check.cpp's prior cases: loc[j] = 1 / 2 + j,
// scale[j] = 5 / 4 + j / 4, shapes 11 + j and 21 + j unless a case sets them,
// key k with value 3 / 8 + k.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
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

struct Prior {
  std::vector<uint8_t> kind;
  std::vector<double> loc, scale, shape0, shape1, key_value;
  std::vector<int32_t> key_column;
  explicit Prior(const std::vector<int>& kinds) {
    for (size_t j = 0; j < kinds.size(); ++j) {
      kind.push_back((uint8_t)kinds[j]);
      loc.push_back(0.5 + j);
      scale.push_back(1.25 + j / 4.0);
      shape0.push_back(11.0 + j);
      shape1.push_back(21.0 + j);
    }
    keys({-1});
  }
  Prior& shapes(int j, double a, double b) {
    shape0[j] = a;
    shape1[j] = b;
    return *this;
  }
  Prior& keys(const std::vector<int32_t>& columns) {
    key_column = columns;
    key_value.clear();
    for (size_t k = 0; k < columns.size(); ++k) key_value.push_back(0.375 + k);
    return *this;
  }
  void run(const char* name) {
    std::vector<unsigned char> image;
    int handle = 0, level = -1;
    g_error[0] = 0;
    const int rc = pack_prior_table(
        (int32_t)kind.size(), kind.data(), loc.data(), scale.data(),
        shape0.data(), shape1.data(), (int32_t)key_column.size(),
        key_column.data(), key_value.data(), &handle, &image, &level);
    const size_t bytes = rc == NB_OK ? image.size() : 0;
    const std::string path = g_dir + "/" + name + ".bin";
    FILE* f = fopen(path.c_str(), "wb");
    if (f == nullptr || (bytes > 0 && fwrite(image.data(), 1, bytes, f) != bytes) ||
        fclose(f) != 0) {
      fprintf(stderr, "cannot write %s\n", path.c_str());
      g_failed = true;
    }
    printf("%s\t%d\t%d\t%zu\t%s\n", name, rc, rc == NB_OK ? level : -1, bytes,
           rc != NB_OK ? g_error : "");
  }
};

// a two-column table {0, kind} whose second column has the shape a
void refusal(const char* name, int kind, double a) {
  Prior({0, kind}).shapes(1, a, 99.0).run(name);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s dir\n", argv[0]);
    return 2;
  }
  g_dir = argv[1];
  // the levels of tables with a closed-form kind
  Prior({0, 7}).run("level3_a");
  Prior({2, 9, 14}).shapes(0, 0.5, 8.0).run("level3_b");
  Prior({1, 8}).run("level4");
  Prior({5, 15}).shapes(0, 36.0, 40.0).shapes(1, 3.0, 99.0).run("level5");
  Prior({15, 5, 0}).shapes(0, 0.5, 99.0).shapes(1, -inf, -38.0).run("level5_b");
  Prior({13, 3}).shapes(0, 2.5, 99.0).shapes(1, 0.75, 99.0).run("level4_b");
  Prior({17}).shapes(0, 0.25, 99.0).run("level3_c");
  // ... and of the four tables of pack_check.cpp, unchanged
  Prior({0, 1, 2, 3, 4, 5, 5, 5}).shapes(2, 0.5, 8.0).shapes(3, 0.75, 99.0)
      .shapes(5, -1.5, 2.0).shapes(6, 0.5, 2.5).shapes(7, -3.0, -1.0)
      .run("prior_8");
  Prior({5, 5, 5}).shapes(0, 36.0, 40.0).shapes(1, -40.0, -36.0)
      .shapes(2, 36.0, inf).run("prior_tails");
  Prior({0, 2}).shapes(1, 0.5, 8.0).run("prior_level0");
  Prior({0, 1}).keys({-1, 1}).run("prior_keys");
  // every closed-form kind in one table, 13 and 17 twice, with three keys
  Prior({7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 13, 17})
      .shapes(6, 2.5, 99.0).shapes(8, 3.0, 99.0).shapes(9, 0.2, 99.0)
      .shapes(10, 0.3, 99.0).shapes(11, 1.0, 99.0).shapes(12, 1.0, 99.0)
      .keys({12, -1, 6}).run("closed_13");
  // the ends of triang's range and a subnormal reciprocal are fine
  Prior({17, 17, 13}).shapes(0, 0.0, 99.0).shapes(1, 1.0, 99.0)
      .shapes(2, 1e308, 99.0).run("closed_ends");
  // refusals: shapes
  refusal("weibull_zero", 13, 0.0);
  refusal("weibull_negative", 13, -2.0);
  refusal("weibull_inf", 13, inf);
  refusal("weibull_nan", 13, nan_);
  refusal("weibull_tiny", 13, 1e-320);           // 1 / c overflows
  refusal("pareto_negative", 15, -1.0);
  refusal("pareto_zero", 15, 0.0);
  refusal("pareto_inf", 15, inf);
  refusal("powerlaw_zero", 16, 0.0);
  refusal("powerlaw_nan", 16, nan_);
  refusal("powerlaw_inf", 16, inf);
  refusal("triang_above", 17, 1.5);
  refusal("triang_below", 17, -0.25);
  refusal("triang_nan", 17, nan_);
  refusal("triang_inf", 17, inf);
  // ... loc and scale of a closed-form column, as for every kind
  { Prior p({0, 7}); p.scale[1] = 0.0; p.run("cauchy_scale"); }
  { Prior p({0, 14}); p.loc[1] = inf; p.run("rayleigh_loc"); }
  // ... and kinds: 6 stays internal, 18 does not exist
  Prior({0, 6}).run("kind6");
  Prior({7, 6}).run("kind6_after_closed");
  Prior({0, 18}).run("kind18");
  Prior({17, 255}).shapes(0, 0.5, 99.0).run("kind255");
  return g_failed ? 1 : 0;
}
