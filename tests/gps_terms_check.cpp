// The argument checks and the slot plan of the Gaussian-process series
// likelihood (plan_gps_terms of nautilus_amd/csrc/nb_pack.h for a sum of
// terms, the very header nb_api.hip includes: all of nb_gps_create_terms but
// pack_gps and the upload; plan_gps_one for one term) built on its own.  Run
// by tests/test_pack_gps_terms.py, once as it is and once under the address
// and undefined-behaviour sanitizers.
//
//   gps_terms_check
//     runs every case and prints one line per case, tab separated: case,
//     return code, the plan as "n_terms kind.. col.. col_q.. col_s width
//     states" (empty after a refusal), doubles of the image pack_gps then
//     makes of five data points (0 after a refusal), recorded error text
//     (empty after a success)
//
// A case named k<codes>, such as k31 or k303, is those kernel codes in that
// order; every sequence of two or three codes 0..3 is run.  one<code> is the
// plan of nb_gps_create for that kernel.
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "nb_pack.h"

static char g_error[1024];
static const double T[5] = {0.25, 1.25, 3.25, 6.25, 10.25};
static const double DATA[5] = {3.0, 4.0, 5.0, 6.0, 7.0};

void nb_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof g_error, fmt, ap);
  va_end(ap);
}

namespace {

std::string plan_text(const nb_gps_plan& plan) {
  std::string text = std::to_string(plan.n_terms);
  for (int i = 0; i < plan.n_terms; ++i)
    text += " " + std::to_string(plan.kind[i]);
  for (int i = 0; i < plan.n_terms; ++i)
    text += " " + std::to_string(plan.col[i]);
  for (int i = 0; i < plan.n_terms; ++i)
    text += " " + std::to_string(plan.col_q[i]);
  return text + " " + std::to_string(plan.col_s) + " " +
         std::to_string(plan.width) + " " + std::to_string(plan.states);
}

// prints the line of a case whose plan was made
void finish(const char* name, const nb_gps_plan& plan) {
  int handle = 0;
  std::vector<double> image;
  const int rc = pack_gps(5, T, DATA, nullptr, plan.kind[0], -0.5, &handle,
                          &image);
  printf("%s\t%d\t%s\t%zu\t%s\n", name, rc, plan_text(plan).c_str(),
         rc == NB_OK ? image.size() : (size_t)0, rc != NB_OK ? g_error : "");
}

struct Terms {
  std::vector<int32_t> kernels;
  int n_terms;
  bool with_kernels = true, with_t = true, with_data = true, with_out = true;
  explicit Terms(std::vector<int32_t> k)
      : kernels(std::move(k)), n_terms((int)kernels.size()) {}
  void run(const char* name) {
    int handle = 0;
    nb_gps_plan plan;
    g_error[0] = 0;
    const int rc = plan_gps_terms(
        n_terms, with_kernels ? kernels.data() : nullptr,
        with_t ? T : nullptr, with_data ? DATA : nullptr,
        with_out ? &handle : nullptr, &plan);
    if (rc == NB_OK)
      finish(name, plan);
    else
      printf("%s\t%d\t\t0\t%s\n", name, rc, g_error);
  }
};

}  // namespace

int main() {
  for (int a = 0; a < 4; ++a) {
    g_error[0] = 0;
    finish(("one" + std::to_string(a)).c_str(), plan_gps_one(a));
    for (int b = 0; b < 4; ++b) {
      Terms({a, b}).run(
          ("k" + std::to_string(a) + std::to_string(b)).c_str());
      for (int c = 0; c < 4; ++c)
        Terms({a, b, c}).run(("k" + std::to_string(a) + std::to_string(b) +
                              std::to_string(c)).c_str());
    }
  }
  // refusals
  { Terms g({0, 1}); g.n_terms = 0; g.run("no_terms"); }
  Terms({3}).run("one_term");
  Terms({0, 0, 0, 0}).run("four_terms");
  { Terms g({0, 1}); g.n_terms = -2; g.run("negative_terms"); }
  Terms({4, 0}).run("code_above");
  Terms({0, 1, -1}).run("code_below");
  Terms({0, 7, 9}).run("two_bad_codes");
  { Terms g({0, 1}); g.with_kernels = false; g.run("null_kernels"); }
  { Terms g({0, 1}); g.with_t = false; g.run("null_t"); }
  { Terms g({0, 1}); g.with_data = false; g.run("null_data"); }
  { Terms g({0, 1}); g.with_out = false; g.run("null_out"); }
  // a NULL pointer is named before the number of terms
  { Terms g({0}); g.with_out = false; g.run("null_out_one_term"); }
  return 0;
}
