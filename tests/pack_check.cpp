// The host packers of the library (nautilus_amd/csrc/nb_pack.h, the very
// header nb_api.hip includes) built on their own.  Run by tests/test_pack.py.
//
//   pack_check all dir | pack_check <case> dir
//     runs every case (or the one named): writes the packed image as raw bytes
//     to dir/<case>.bin (empty after a refusal) and prints one line per case,
//     tab separated: case, return code, prior-table level (-1: none), bytes of
//     the image, recorded error text (empty after a success)
//
// Every input is a closed form of its indices, written out again in
// test_pack.py; within a case all input numbers are nonzero and distinct, so
// that a swapped or transposed index cannot hide.
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

std::string g_only, g_dir;
bool g_failed = false, g_ran = false;

bool wanted(const char* name) { return g_only == "all" || g_only == name; }

void emit(const char* name, int rc, int level, const void* image,
          size_t bytes) {
  if (rc != NB_OK) bytes = 0;
  const std::string path = g_dir + "/" + name + ".bin";
  FILE* f = fopen(path.c_str(), "wb");
  if (f == nullptr || (bytes > 0 && fwrite(image, 1, bytes, f) != bytes) ||
      fclose(f) != 0) {
    fprintf(stderr, "cannot write %s\n", path.c_str());
    g_failed = true;
  }
  printf("%s\t%d\t%d\t%zu\t%s\n", name, rc, level, bytes,
         rc != NB_OK ? g_error : "");
  g_ran = true;
}

// ---- bounds ----------------------------------------------------------------

// Ellipsoid number e of a case over n dimensions: B_inv, B lower triangular
// with 1000 (1 + e) + i + j / 1024 and 1000 (11 + e) + i + j / 1024 at (i, j),
// c[i] = 1000 (21 + e) + i + 1 / 2
struct Ell {
  std::vector<double> c, B, B_inv;
  std::vector<int32_t> idx;
  nb_member_desc desc(bool with_idx, int free_dims) const {
    nb_member_desc m;
    m.n_ell = (int32_t)c.size();
    m.idx_ell = with_idx ? idx.data() : nullptr;
    m.c = c.data();
    m.B = B.data();
    m.B_inv = B_inv.data();
    m.free_dims = free_dims;
    return m;
  }
};

Ell make_ell(int e, const std::vector<int32_t>& idx) {
  const int n = (int)idx.size();
  Ell l;
  l.idx = idx;
  l.c.resize(n);
  l.B.assign((size_t)n * n, 0.0);
  l.B_inv.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) {
    l.c[i] = 1000.0 * (21 + e) + i + 0.5;
    for (int j = 0; j <= i; ++j) {
      l.B_inv[(size_t)i * n + j] = 1000.0 * (1 + e) + i + j / 1024.0;
      l.B[(size_t)i * n + j] = 1000.0 * (11 + e) + i + j / 1024.0;
    }
  }
  return l;
}

std::vector<int32_t> iota(int n) {
  std::vector<int32_t> v(n);
  for (int i = 0; i < n; ++i) v[i] = i;
  return v;
}

// Emulator of neural bound m with E networks: mean[f] = 31000 + 1000 m + f +
// 1 / 4, scale[f] = 41000 + 1000 m + f + 1 / 8; layer l (0-3) of network e
// has W[k][h] = 100000 (8 m + 4 e + l + 1) + 1000 k + h + 1 / 4, the bias as
// row k = fan-in
struct Mlp {
  std::vector<double> mean, scale;
  std::vector<std::vector<double>> coefs, intercepts;
  std::vector<const double*> cp, ip;
  nb_mlp_desc d;
};

void make_mlp(Mlp* p, int m, int n_dim, int E) {
  const int rows[4] = {n_dim, NB_H1, NB_H2, NB_H3};
  const int cols[4] = {NB_H1, NB_H2, NB_H3, 1};
  for (int f = 0; f < n_dim; ++f) {
    p->mean.push_back(31000.0 + 1000.0 * m + f + 0.25);
    p->scale.push_back(41000.0 + 1000.0 * m + f + 0.125);
  }
  for (int e = 0; e < E; ++e)
    for (int l = 0; l < 4; ++l) {
      const double base = 100000.0 * (8 * m + 4 * e + l + 1) + 0.25;
      std::vector<double> w, b;
      for (int k = 0; k < rows[l]; ++k)
        for (int h = 0; h < cols[l]; ++h) w.push_back(base + 1000.0 * k + h);
      for (int h = 0; h < cols[l]; ++h)
        b.push_back(base + 1000.0 * rows[l] + h);
      p->coefs.push_back(w);
      p->intercepts.push_back(b);
    }
  for (size_t i = 0; i < p->coefs.size(); ++i) {
    p->cp.push_back(p->coefs[i].data());
    p->ip.push_back(p->intercepts[i].data());
  }
  p->d.n_networks = E;
  p->d.mean = p->mean.data();
  p->d.scale = p->scale.data();
  p->d.coefs = p->cp.data();
  p->d.intercepts = p->ip.data();
}

// A bound description and what it points to.  Members are ellipsoids 0, 1,
// the neural bounds' ellipsoids 5, 6 (full); neural bound m has
// score_predict_min = 5 / 8 + m and, where given, radius2 = 15 / 2 + m;
// log_v_all[m] = -3 / 2 - 3 m / 4; periodic centre i is 1 / 8 + i / 16.
struct Bound {
  std::vector<Ell> ells;
  std::vector<nb_member_desc> members;
  std::vector<Mlp> mlps;
  std::vector<nb_neural_desc> neural;
  std::vector<double> log_v_all, centers;
  std::vector<int32_t> periodic;
  nb_bound_desc d;

  explicit Bound(int n_dim) {
    std::memset(&d, 0, sizeof d);
    d.n_dim = n_dim;
    ells.reserve(8);
    mlps.reserve(4);
  }
  void member(const std::vector<int32_t>& idx, bool with_idx, int free_dims) {
    ells.push_back(make_ell((int)members.size(), idx));
    members.push_back(ells.back().desc(with_idx, free_dims));
  }
  // E < 0: no emulator (mlp NULL)
  void neural_bound(int E, bool with_radius) {
    const int m = (int)neural.size();
    ells.push_back(make_ell(5 + m, iota(d.n_dim)));
    nb_neural_desc nd;
    nd.ellipsoid = ells.back().desc(false, 0);
    nd.mlp = nullptr;
    if (E >= 0) {
      mlps.emplace_back();
      make_mlp(&mlps.back(), m, d.n_dim, E);
      nd.mlp = &mlps.back().d;
    }
    nd.score_predict_min = 0.625 + m;
    nd.radius2 = with_radius ? 7.5 + m : 0.0;
    neural.push_back(nd);
  }
  void volumes() {
    for (size_t m = 0; m < members.size(); ++m)
      log_v_all.push_back(-1.5 - 0.75 * m);
  }
  void periodic_dims(const std::vector<int32_t>& dims) {
    periodic = dims;
    for (size_t i = 0; i < dims.size(); ++i)
      centers.push_back(0.125 + i / 16.0);
  }
  void run(const char* name) {
    finish();
    run_as_is(name);
  }
  void finish() {
    d.n_members = (int32_t)members.size();
    d.members = members.empty() ? nullptr : members.data();
    d.log_v_all = log_v_all.empty() ? nullptr : log_v_all.data();
    d.n_neural = (int32_t)neural.size();
    d.neural = neural.empty() ? nullptr : neural.data();
    d.n_periodic = (int32_t)periodic.size();
    d.periodic = periodic.empty() ? nullptr : periodic.data();
    d.centers = centers.empty() ? nullptr : centers.data();
  }
  void run_as_is(const char* name) {
    BoundLayout layout;
    std::vector<double> blob;
    g_error[0] = 0;
    const int rc = pack_bound(&d, &layout, &blob);
    emit(name, rc, -1, blob.data(), blob.size() * sizeof(double));
  }
};

void bound_cases() {
  if (wanted("b1")) {
    Bound b(1);
    b.member(iota(1), false, 0);
    b.run("b1");
  }
  if (wanted("b2")) {
    Bound b(16);
    b.member(iota(16), false, 0);
    b.member({0, 3, 7, 8, 15}, true, 0);
    b.d.unit_cube = 1;
    b.volumes();
    b.neural_bound(2, true);
    b.run("b2");
  }
  if (wanted("b3")) {
    Bound b(15);
    b.neural_bound(1, false);
    b.run("b3");
  }
  if (wanted("b4")) {
    Bound b(17);
    b.member(iota(17), false, 0);
    b.member({}, true, 1);
    b.periodic_dims({0, 16});
    b.neural_bound(1, true);
    b.run("b4");
  }
  if (wanted("b5")) {
    Bound b(33);
    b.member(iota(33), false, 0);
    b.run("b5");
  }
  if (wanted("b6")) {
    Bound b(3);
    b.member(iota(3), false, 0);
    b.neural_bound(1, true);
    b.neural_bound(1, true);
    b.run("b6");
  }
  if (wanted("b7")) {
    Bound b(2);
    b.neural_bound(-1, true);
    b.run("b7");
  }
  // refusals
  if (wanted("b_ndim0")) {
    Bound b(0);
    b.run("b_ndim0");
  }
  if (wanted("b_ndim129")) {
    Bound b(129);
    b.run("b_ndim129");
  }
  if (wanted("b_negative_k")) {
    Bound b(2);
    b.member(iota(2), false, 0);
    b.finish();
    b.d.n_members = -1;
    b.run_as_is("b_negative_k");
  }
  if (wanted("b_members_null")) {
    Bound b(2);
    b.d.n_members = 1;
    b.run_as_is("b_members_null");
  }
  if (wanted("b_network_counts")) {
    Bound b(2);
    b.neural_bound(1, true);
    b.neural_bound(2, true);
    b.run("b_network_counts");
  }
  if (wanted("b_neural_not_full")) {
    Bound b(3);
    b.neural_bound(1, true);
    b.neural[0].ellipsoid.n_ell = 2;
    b.run("b_neural_not_full");
  }
  if (wanted("b_periodic_count")) {
    Bound b(2);
    b.member(iota(2), false, 0);
    b.periodic_dims({0, 1, 1});
    b.run("b_periodic_count");
  }
  if (wanted("b_periodic_no_centers")) {
    Bound b(2);
    b.member(iota(2), false, 0);
    b.periodic_dims({0});
    b.finish();
    b.d.centers = nullptr;
    b.run_as_is("b_periodic_no_centers");
  }
  if (wanted("b_periodic_range")) {
    Bound b(2);
    b.member(iota(2), false, 0);
    b.periodic_dims({0, 2});
    b.run("b_periodic_range");
  }
  if (wanted("b_member_n_ell")) {
    Bound b(2);
    b.member(iota(3), false, 0);
    b.run("b_member_n_ell");
  }
  if (wanted("b_idx_order")) {
    Bound b(4);
    b.member({0, 2, 2}, true, 0);
    b.run("b_idx_order");
  }
  if (wanted("b_upper_nonzero")) {
    Bound b(3);
    b.member(iota(3), false, 0);
    b.ells[0].B_inv[1 * 3 + 2] = 0.5;
    b.run("b_upper_nonzero");
  }
  if (wanted("b_two_defects")) {
    Bound b(4);
    b.member({0, 2, 2}, true, 0);
    b.periodic_dims({4});
    b.run("b_two_defects");
  }
}

// ---- likelihood tables -----------------------------------------------------

// Mixture: means[c][h] = 500 + 100 c + h + 1 / 2, chol_inv of component c
// 1000 (1 + c) + h + k / 1024 at (h, k <= h), log_coef[c] = -3 / 4 - c
struct Mixture {
  int n_dim, n_comp;
  std::vector<double> means, chol_inv, log_coef;
  Mixture(int d, int k) : n_dim(d), n_comp(k) {
    for (int c = 0; c < k; ++c) {
      log_coef.push_back(-0.75 - c);
      for (int h = 0; h < d; ++h) {
        means.push_back(500.0 + 100.0 * c + h + 0.5);
        for (int j = 0; j < d; ++j)
          chol_inv.push_back(j <= h ? 1000.0 * (1 + c) + h + j / 1024.0 : 0.0);
      }
    }
  }
  void run(const char* name, int n_components) {
    std::vector<double> image;
    int handle = 0;
    g_error[0] = 0;
    const int rc = pack_mixture(n_dim, n_components, means.data(),
                                chol_inv.data(), log_coef.data(), &handle,
                                &image);
    emit(name, rc, -1, image.data(), image.size() * sizeof(double));
  }
};

void mixture_cases() {
  const int shapes[3][2] = {{1, 1}, {17, 2}, {33, 2}};
  for (const auto& s : shapes) {
    const std::string name =
        "mix_" + std::to_string(s[0]) + "_" + std::to_string(s[1]);
    if (wanted(name.c_str())) Mixture(s[0], s[1]).run(name.c_str(), s[1]);
  }
  if (wanted("mix_log_coef")) {
    Mixture m(3, 2);
    m.log_coef[1] = inf;
    m.run("mix_log_coef", 2);
  }
  if (wanted("mix_mean")) {
    Mixture m(3, 2);
    m.means[3 + 2] = nan_;
    m.run("mix_mean", 2);
  }
  if (wanted("mix_upper")) {
    Mixture m(3, 2);
    m.chol_inv[9 + 0 * 3 + 2] = 0.5;
    m.run("mix_upper", 2);
  }
  if (wanted("mix_diagonal")) {
    Mixture m(3, 2);
    m.chol_inv[2 * 3 + 2] = 0.0;
    m.run("mix_diagonal", 2);
  }
  if (wanted("mix_0")) Mixture(3, 1).run("mix_0", 0);
  if (wanted("mix_4097")) Mixture(3, 1).run("mix_4097", 4097);
}

// Data likelihood: data[k] = 3000000 + k, chol_inv 1 + 1024 h + k at
// (h, k <= h), inv_sigma[k] = 1 / 2 + k
struct Chi2 {
  int n;
  std::vector<double> data, chol_inv, inv_sigma;
  double log_norm = -2.5;
  explicit Chi2(int n_data) : n(n_data) {
    for (int h = 0; h < n; ++h) {
      data.push_back(3000000.0 + h);
      inv_sigma.push_back(0.5 + h);
      for (int k = 0; k < n; ++k)
        chol_inv.push_back(k <= h ? 1.0 + 1024.0 * h + k : 0.0);
    }
  }
  void run(const char* name, bool full, bool diag) {
    std::vector<double> image;
    int handle = 0;
    g_error[0] = 0;
    const int rc = pack_chi2(n, data.data(), full ? chol_inv.data() : nullptr,
                             diag ? inv_sigma.data() : nullptr, log_norm,
                             &handle, &image);
    emit(name, rc, -1, image.data(), image.size() * sizeof(double));
  }
};

void chi2_cases() {
  for (int n : {1, 16, 17, 257}) {
    const std::string name = "chi2_" + std::to_string(n);
    if (wanted(name.c_str())) Chi2(n).run(name.c_str(), true, false);
  }
  if (wanted("chi2_diag_3")) Chi2(3).run("chi2_diag_3", false, true);
  if (wanted("chi2_neither")) Chi2(3).run("chi2_neither", false, false);
  if (wanted("chi2_both")) Chi2(3).run("chi2_both", true, true);
  if (wanted("chi2_data")) {
    Chi2 c(3);
    c.data[1] = nan_;
    c.run("chi2_data", true, false);
  }
  if (wanted("chi2_inv_sigma")) {
    Chi2 c(3);
    c.inv_sigma[2] = 0.0;
    c.run("chi2_inv_sigma", false, true);
  }
  if (wanted("chi2_upper")) {
    Chi2 c(3);
    c.chol_inv[0 * 3 + 1] = 0.5;
    c.run("chi2_upper", true, false);
  }
  if (wanted("chi2_log_norm")) {
    Chi2 c(3);
    c.log_norm = inf;
    c.run("chi2_log_norm", true, false);
  }
}

// Poisson tables: counts[j] = 2000000 + j, exposure[j] = 4000000 + j,
// background[j] = 5000000 + j; response (n_data x n_src, leading dimension
// ld) 1 + 1024 j + c at (j, c), 9e9 in the padding of a row
struct Counts {
  int n, n_src;
  int64_t ld;
  std::vector<double> counts, exposure, background, response;
  Counts(int n_data, int n_source, int pad)
      : n(n_data), n_src(n_source), ld(n_source + pad) {
    for (int j = 0; j < n; ++j) {
      counts.push_back(2000000.0 + j);
      exposure.push_back(4000000.0 + j);
      background.push_back(5000000.0 + j);
      for (int c = 0; c < ld; ++c)
        response.push_back(c < n_src ? 1.0 + 1024.0 * j + c : 9e9);
    }
  }
  void run(const char* name, bool with_tables) {
    std::vector<double> image;
    int handle = 0;
    g_error[0] = 0;
    const int rc = pack_poisson(n, counts.data(),
                                with_tables ? exposure.data() : nullptr,
                                with_tables ? background.data() : nullptr,
                                -1.25, &handle, &image);
    emit(name, rc, -1, image.data(), image.size() * sizeof(double));
  }
  void run_fold(const char* name, int64_t ld_response) {
    std::vector<double> image;
    int handle = 0;
    g_error[0] = 0;
    const int rc = pack_fold_poisson(n, n_src, counts.data(), response.data(),
                                     ld_response, exposure.data(),
                                     background.data(), -1.25, &handle, &image);
    emit(name, rc, -1, image.data(), image.size() * sizeof(double));
  }
};

void poisson_cases() {
  if (wanted("po_3")) {
    Counts c(3, 1, 0);
    c.counts[1] = 0.0;
    c.run("po_3", false);
  }
  if (wanted("po_3_tables")) {
    Counts c(3, 1, 0);
    c.counts[1] = 0.0;
    c.run("po_3_tables", true);
  }
  // every refusal of a bin
  const struct { const char* name; int which; double v; } bad[] = {
      {"po_count_negative", 0, -1.0},   {"po_count_nan", 0, nan_},
      {"po_count_tiny", 0, 1e-310},     {"po_exposure_zero", 1, 0.0},
      {"po_exposure_inf", 1, inf},      {"po_background_negative", 2, -0.5},
      {"po_background_nan", 2, nan_}};
  for (const auto& b : bad)
    if (wanted(b.name)) {
      Counts c(3, 1, 0);
      (b.which == 0 ? c.counts : b.which == 1 ? c.exposure : c.background)[2] =
          b.v;
      c.run(b.name, true);
    }
  const int shapes[4][3] = {{1, 1, 0}, {16, 16, 0}, {17, 5, 0}, {257, 17, 3}};
  for (const auto& s : shapes) {
    const std::string name =
        "fold_" + std::to_string(s[0]) + "_" + std::to_string(s[1]);
    if (wanted(name.c_str())) {
      Counts c(s[0], s[1], s[2]);
      c.run_fold(name.c_str(), c.ld);
    }
  }
  if (wanted("fold_response")) {
    Counts c(3, 2, 1);
    c.response[1 * 3 + 1] = inf;
    c.run_fold("fold_response", c.ld);
  }
  if (wanted("fold_ld")) {
    Counts c(3, 2, 0);
    c.run_fold("fold_ld", 1);
  }
}

// Noise likelihood: data[j] = 3000000 + j, sigma2[j] = 1 / 2 + j
void noise_case(const char* name, bool with_sigma2, int bad) {
  if (!wanted(name)) return;
  std::vector<double> data, sigma2, image;
  for (int j = 0; j < 3; ++j) {
    data.push_back(3000000.0 + j);
    sigma2.push_back(0.5 + j);
  }
  if (bad == 1) data[1] = inf;
  if (bad == 2) sigma2[2] = -0.5;
  int handle = 0;
  g_error[0] = 0;
  const int rc = pack_noise(3, data.data(),
                            with_sigma2 ? sigma2.data() : nullptr, -0.5,
                            &handle, &image);
  emit(name, rc, -1, image.data(), image.size() * sizeof(double));
}

// ---- prior tables ----------------------------------------------------------

// loc[j] = 1 / 2 + j, scale[j] = 5 / 4 + j / 4; the shapes of a column that
// has none are 11 + j and 21 + j; key k has value 3 / 8 + k
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
  void shapes(int j, double a, double b) { shape0[j] = a; shape1[j] = b; }
  void keys(const std::vector<int32_t>& columns) {
    key_column = columns;
    key_value.clear();
    for (size_t k = 0; k < columns.size(); ++k) key_value.push_back(0.375 + k);
  }
  void run(const char* name) {
    if (!wanted(name)) return;
    std::vector<unsigned char> image;
    int handle = 0, level = -1;
    g_error[0] = 0;
    const int rc = pack_prior_table(
        (int32_t)kind.size(), kind.data(), loc.data(), scale.data(),
        shape0.data(), shape1.data(), (int32_t)key_column.size(),
        key_column.data(), key_value.data(), &handle, &image, &level);
    emit(name, rc, rc == NB_OK ? level : -1, image.data(), image.size());
  }
};

void prior_cases() {
  {
    Prior p({0, 1, 2, 3, 4, 5, 5, 5});
    p.shapes(2, 0.5, 8.0);
    p.shapes(3, 0.75, 99.0);
    p.shapes(5, -1.5, 2.0);
    p.shapes(6, 0.5, 2.5);
    p.shapes(7, -3.0, -1.0);
    p.run("prior_8");
  }
  {
    Prior p({5, 5, 5});
    p.shapes(0, 36.0, 40.0);
    p.shapes(1, -40.0, -36.0);
    p.shapes(2, 36.0, inf);
    p.run("prior_tails");
  }
  {
    Prior p({0, 2});
    p.shapes(1, 0.5, 8.0);
    p.run("prior_level0");
  }
  {
    Prior p({0, 1});
    p.keys({-1, 1});
    p.run("prior_keys");
  }
  // refusals
  { Prior p({0, 6}); p.run("prior_kind6"); }
  { Prior p({0, 1}); p.scale[1] = 0.0; p.run("prior_scale"); }
  { Prior p({0, 2}); p.shapes(1, 8.0, 8.0); p.run("prior_loguniform"); }
  { Prior p({0, 3}); p.shapes(1, 0.0, 99.0); p.run("prior_lognormal"); }
  { Prior p({0, 5}); p.shapes(1, 2.0, 2.0); p.run("prior_truncnorm"); }
  { Prior p({0, 5}); p.shapes(1, 2e150, inf); p.run("prior_truncnorm_max"); }
  { Prior p({0, 1}); p.keys({-1, 2}); p.run("prior_key_column"); }
  { Prior p({0, 1}); p.keys({}); p.run("prior_no_keys"); }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s all|<case> dir\n", argv[0]);
    return 2;
  }
  g_only = argv[1];
  g_dir = argv[2];
  bound_cases();
  mixture_cases();
  chi2_cases();
  poisson_cases();
  noise_case("noise_3", false, 0);
  noise_case("noise_3_sigma2", true, 0);
  noise_case("noise_data", true, 1);
  noise_case("noise_sigma2", true, 2);
  prior_cases();
  if (!g_ran) fprintf(stderr, "no case named %s\n", argv[1]);
  return g_failed || !g_ran ? 1 : 0;
}
