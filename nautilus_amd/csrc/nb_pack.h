// Host packers: every image the kernels read (nb_layout.h), built from the
// descriptions of the C ABI.  Plain C++17 without HIP, so that
// tests/pack_check.cpp builds it on its own; internal linkage, for the one
// translation unit that uploads the images (nb_api.hip).  Each packer returns
// NB_OK or records a message with nb_set_error (defined by the includer's
// program) and returns the code of the refusal.
#pragma once

#include "nb_layout.h"
#include "../../include/nautilus_hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

namespace {

const double INF = std::numeric_limits<double>::infinity();

inline void put_i64(std::vector<double>& buf, size_t at, int64_t v) {
  std::memcpy(&buf[at], &v, sizeof v);
}

// Lower-triangular n x n matrix (row-major, leading dimension ld) as the
// dt (dt + 1) / 2 tiles of the stream block and of a mixture record, with the
// K permutation of nb_stream.hip (slot 4kt+s of lane group lg <-> feature
// 16kt + 8(s>>1) + 2lg + (s&1)); dst is zero where nothing is written
void put_tri_tiles(double* dst, int dt, int n, const double* lower, size_t ld) {
  for (int ht = 0; ht < dt; ++ht)
    for (int kt = 0; kt <= ht; ++kt)
      for (int s4 = 0; s4 < 4; ++s4)
        for (int lg = 0; lg < 4; ++lg)
          for (int l = 0; l < 16; ++l) {
            const int k = 16 * kt + 8 * (s4 >> 1) + 2 * lg + (s4 & 1);
            const int h = 16 * ht + l;
            if (h < n && k <= h)
              dst[((size_t)(ht * (ht + 1)) / 2 + kt) * NB_TILE + s4 * 64 +
                  lg * 16 + l] = lower[h * ld + k];
          }
}

// ---- the bound blob --------------------------------------------------------

// Where everything lives in the blob of one bound (offsets and strides in
// doubles; off_stream / off_shift are positions even where the block is
// absent, the header holds 0 then)
struct BoundLayout {
  int n_dim = 0, dt = 0, dp = 0, K = 0, M = 0, E = 0, kt1 = 0;
  bool unit_cube = false, single_full = false, periodic = false;
  int64_t ell_size = 0, net_stride = 0, neural_stride = 0, draw_stride = 0;
  int64_t off_cdf = 0, off_ulo = 0, off_uhi = 0, off_members = 0,
          off_neural = 0, off_draw = 0, off_stream = 0, off_shift = 0;
  int64_t total = 0;
};

int bound_layout(const nb_bound_desc* d, BoundLayout* out) {
  BoundLayout& L = *out;
  const int n_dim = d->n_dim;
  if (n_dim < 1 || n_dim > 16 * NB_MAX_DT) {
    nb_set_error("n_dim=%d unsupported (1..%d)", n_dim, 16 * NB_MAX_DT);
    return NB_ERR_UNSUPPORTED;
  }
  const int dt = (n_dim + 15) / 16, dp = 16 * dt;
  const int K = d->n_members, M = d->n_neural;
  if (K < 0 || M < 0 || (K > 0 && d->members == nullptr) ||
      (M > 0 && d->neural == nullptr)) {
    nb_set_error("inconsistent member / neural counts");
    return NB_ERR_ARG;
  }
  int E = 0;
  for (int m = 0; m < M; ++m) {
    const int e = d->neural[m].mlp ? d->neural[m].mlp->n_networks : 0;
    if (m > 0 && e != E) {
      nb_set_error("all neural bounds must have the same number of networks");
      return NB_ERR_ARG;
    }
    E = e;
    if (d->neural[m].ellipsoid.n_ell != n_dim) {
      nb_set_error("NeuralBound ellipsoid must span all dimensions");
      return NB_ERR_ARG;
    }
  }
  L.n_dim = n_dim; L.dt = dt; L.dp = dp; L.K = K; L.M = M; L.E = E;
  L.kt1 = (n_dim + 1 + 15) / 16;
  L.unit_cube = d->unit_cube != 0;
  L.ell_size = nb_ell_block_size(dt);
  L.net_stride = (int64_t)nb_net_tiles(L.kt1) * NB_TILE;
  L.neural_stride = L.ell_size + 2 + 2 * dp + (int64_t)E * L.net_stride;
  L.draw_stride = 2 + 4 * dp + (int64_t)dp * (dp + 1) / 2 + 16;

  int64_t off = NB_HDR;
  L.off_cdf = off; off += ((K > 0 ? K : 1) + 1) / 2 * 2;
  L.off_ulo = off; off += dp;
  L.off_uhi = off; off += dp;
  L.off_members = off; off += (int64_t)K * L.ell_size;
  L.off_neural = off; off += (int64_t)M * L.neural_stride;
  L.off_draw = off; off += (int64_t)K * L.draw_stride;
  L.single_full = (K == 1 && M == 0 && !d->unit_cube &&
                   d->members[0].n_ell == n_dim);
  L.off_stream = off;
  if (L.single_full) off += dp + (int64_t)dt * (dt + 1) / 2 * NB_TILE;
  if (d->n_periodic < 0 || d->n_periodic > n_dim ||
      (d->n_periodic > 0 && (d->periodic == nullptr || d->centers == nullptr))) {
    nb_set_error("bad periodic description");
    return NB_ERR_ARG;
  }
  L.periodic = d->n_periodic > 0;
  L.off_shift = off;
  if (L.periodic) off += 2 * dp;
  L.total = off;
  return NB_OK;
}

void put_header(const BoundLayout& L, std::vector<double>& buf) {
  put_i64(buf, NB_H_NDIM, L.n_dim);
  put_i64(buf, NB_H_DT, L.dt);
  put_i64(buf, NB_H_K, L.K);
  put_i64(buf, NB_H_USECUBE, L.unit_cube ? 1 : 0);
  put_i64(buf, NB_H_M, L.M);
  put_i64(buf, NB_H_E, L.E);
  put_i64(buf, NB_H_OFF_CDF, L.off_cdf);
  put_i64(buf, NB_H_OFF_ULO, L.off_ulo);
  put_i64(buf, NB_H_OFF_UHI, L.off_uhi);
  put_i64(buf, NB_H_OFF_MEMBERS, L.off_members);
  put_i64(buf, NB_H_ELL_STRIDE, L.ell_size);
  put_i64(buf, NB_H_OFF_NEURAL, L.off_neural);
  put_i64(buf, NB_H_NEURAL_STRIDE, L.neural_stride);
  put_i64(buf, NB_H_OFF_DRAW, L.off_draw);
  put_i64(buf, NB_H_DRAW_STRIDE, L.draw_stride);
  put_i64(buf, NB_H_NET_STRIDE, L.net_stride);
  put_i64(buf, NB_H_KT1, L.kt1);
  put_i64(buf, NB_H_TOTAL, L.total);
  put_i64(buf, NB_H_OFF_STREAM, L.single_full ? L.off_stream : 0);
  put_i64(buf, NB_H_OFF_SHIFT, L.periodic ? L.off_shift : 0);
}

// fills one ell block at buf[at ...]; returns false on invalid input
bool fill_ell_block(std::vector<double>& buf, size_t at, int n_dim, int dt,
                    const nb_member_desc& m, bool is_neural) {
  const int dp = 16 * dt;
  if (m.n_ell < 0 || m.n_ell > n_dim) {
    nb_set_error("member n_ell=%d out of range for n_dim=%d", m.n_ell, n_dim);
    return false;
  }
  put_i64(buf, at, m.n_ell);
  double* lo = &buf[at + 2];
  double* hi = lo + dp;
  double* c = hi + dp;
  double* tiles = c + dp;
  std::vector<int> idx(m.n_ell);
  std::vector<char> is_ell(n_dim, 0);
  for (int i = 0; i < m.n_ell; ++i) {
    idx[i] = m.idx_ell ? m.idx_ell[i] : i;
    if (idx[i] < 0 || idx[i] >= n_dim || (i > 0 && idx[i] <= idx[i - 1])) {
      nb_set_error("idx_ell must be strictly increasing within [0, n_dim)");
      return false;
    }
    is_ell[idx[i]] = 1;
  }
  bool any_box = false;
  for (int f = 0; f < dp; ++f) {
    const bool boxed = f < n_dim && !is_ell[f] && !m.free_dims && !is_neural;
    const int sl = nb_slot_of_feature(f);
    lo[sl] = boxed ? 0.0 : -INF;
    hi[sl] = boxed ? 1.0 : INF;
    c[sl] = 0.0;
    any_box |= boxed;
  }
  // [1]: members: "has finite box limits" (nb_cand.hip skips the box test
  // otherwise); neural blocks: the squared bounding radius, set by the caller
  put_i64(buf, at + 1, any_box ? 1 : 0);
  for (int i = 0; i < m.n_ell; ++i) c[nb_slot_of_feature(idx[i])] = m.c[i];
  for (int i = 0; i < m.n_ell; ++i) {
    for (int j = 0; j < m.n_ell; ++j) {
      const double v = m.B_inv[(size_t)i * m.n_ell + j];
      if (j > i) {
        if (v != 0.0) {
          nb_set_error("B_inv must be lower triangular (basic.py:308-309)");
          return false;
        }
        continue;
      }
      // W0[k][h] = B_inv[h][k]; the K index of the tile is stored in slot
      // order: tile (kt, ht), k-step s, lane (li, lg) at s*64 + lg*16 + li
      const int h = idx[i], k = idx[j];
      const int sl = nb_slot_of_feature(k);          // = 4*ks + lg
      const int ks = sl >> 2, lgk = sl & 3;
      tiles[((size_t)(ks >> 2) * dt + (h >> 4)) * NB_TILE + (ks & 3) * 64 +
            lgk * 16 + (h & 15)] = v;
    }
  }
  return true;
}

void put_weight(double* tiles, int ht_n, int k, int h, double v) {
  tiles[((size_t)(k >> 4) * ht_n + (h >> 4)) * NB_TILE + (k & 15) * 16 +
        (h & 15)] = v;
}

void fill_net(double* net, int n_dim, int kt1, const double* const* coefs,
              const double* const* intercepts) {
  double* w1 = net;
  double* w2 = w1 + (size_t)kt1 * NB_HT1 * NB_TILE;
  double* w3 = w2 + (size_t)NB_HT1 * NB_HT2 * NB_TILE;
  double* w4 = w3 + (size_t)NB_HT2 * NB_HT3 * NB_TILE;
  for (int k = 0; k < n_dim; ++k)
    for (int h = 0; h < NB_H1; ++h)
      put_weight(w1, NB_HT1, k, h, coefs[0][(size_t)k * NB_H1 + h]);
  for (int h = 0; h < NB_H1; ++h)
    put_weight(w1, NB_HT1, n_dim, h, intercepts[0][h]);
  for (int k = 0; k < NB_H1; ++k)
    for (int h = 0; h < NB_H2; ++h)
      put_weight(w2, NB_HT2, k, h, coefs[1][(size_t)k * NB_H2 + h]);
  for (int h = 0; h < NB_H2; ++h)
    put_weight(w2, NB_HT2, NB_H1, h, intercepts[1][h]);
  for (int k = 0; k < NB_H2; ++k)
    for (int h = 0; h < NB_H3; ++h)
      put_weight(w3, NB_HT3, k, h, coefs[2][(size_t)k * NB_H3 + h]);
  for (int h = 0; h < NB_H3; ++h)
    put_weight(w3, NB_HT3, NB_H2, h, intercepts[2][h]);
  for (int k = 0; k < NB_H3; ++k) put_weight(w4, 1, k, 0, coefs[3][k]);
  put_weight(w4, 1, NB_H3, 0, intercepts[3][0]);
}

// member CDF over softmax(log_v_all), union.py:308
void fill_cdf(double* cdf, int K, const double* log_v_all) {
  double mx = -INF;
  for (int m = 0; m < K; ++m)
    mx = std::fmax(mx, log_v_all ? log_v_all[m] : 0.0);
  std::vector<double> p(K);
  double sum = 0.0;
  for (int m = 0; m < K; ++m) {
    p[m] = std::exp((log_v_all ? log_v_all[m] : 0.0) - mx);
    sum += p[m];
  }
  double run = 0.0;
  for (int m = 0; m < K; ++m) {
    run += p[m] / sum;
    cdf[m] = run;
  }
  cdf[K - 1] = 1.0;
}

// compact draw block of a member (whose idx_ell fill_ell_block has checked)
void fill_draw_block(std::vector<double>& buf, size_t at, int n_dim, int dp,
                     const nb_member_desc& md) {
  std::vector<char> is_ell(n_dim, 0);
  for (int i = 0; i < md.n_ell; ++i)
    is_ell[md.idx_ell ? md.idx_ell[i] : i] = 1;
  int nc = 0;
  for (int f = 0; f < n_dim; ++f) {
    if (!is_ell[f] && !md.free_dims) {
      put_i64(buf, at + 2 + dp + nc, f);
      ++nc;
    }
  }
  put_i64(buf, at, md.n_ell);
  put_i64(buf, at + 1, nc);
  // slot of every column: ellipsoid dims first, then the cube dims
  {
    int cube_slot = md.n_ell;
    for (int f = 0; f < n_dim; ++f)
      if (!is_ell[f]) put_i64(buf, at + 2 + 2 * dp + f, cube_slot++);
  }
  for (int i = 0; i < md.n_ell; ++i) {
    const int f = md.idx_ell ? md.idx_ell[i] : i;
    put_i64(buf, at + 2 + i, f);
    put_i64(buf, at + 2 + 2 * dp + f, i);
    buf[at + 2 + 3 * dp + i] = md.c[i];
    for (int j = 0; j <= i; ++j)
      buf[at + 2 + 4 * dp + (size_t)i * (i + 1) / 2 + j] =
          md.B[(size_t)i * md.n_ell + j];
  }
}

// bounding sphere of a neural bound's ellipsoid without a radius from the
// caller: lambda_max(B B^T) <= min(Gershgorin, ||B||_F^2), conservatively
double fallback_radius2(const nb_member_desc& ell) {
  const int n = ell.n_ell;
  const double* B = ell.B;
  double fro = 0.0, ger = 0.0;
  for (int i = 0; i < n * n; ++i) fro += B[i] * B[i];
  for (int i = 0; i < n; ++i) {
    double rowsum = 0.0;
    for (int j = 0; j < n; ++j) {
      double aij = 0.0;
      for (int k = 0; k < n; ++k) aij += B[i * n + k] * B[j * n + k];
      rowsum += std::fabs(aij);
    }
    ger = std::fmax(ger, rowsum);
  }
  return std::fmin(fro, ger) * (1.0 + 1e-9);
}

// the blob of a bound: everything nb_bound_create checks and fills before it
// uploads
int pack_bound(const nb_bound_desc* d, BoundLayout* layout,
               std::vector<double>* blob) {
  const int rc = bound_layout(d, layout);
  if (rc != NB_OK) return rc;
  const BoundLayout& L = *layout;
  const int n_dim = L.n_dim, dt = L.dt, dp = L.dp;
  std::vector<double>& buf = *blob;
  buf.assign((size_t)L.total, 0.0);
  put_header(L, buf);
  for (int i = 0; i < d->n_periodic; ++i) {
    const int f = d->periodic[i];
    if (f < 0 || f >= n_dim) {
      nb_set_error("periodic index %d out of range", f);
      return NB_ERR_ARG;
    }
    // periodic.py:69-71: the forward shift adds (-center + 0.5)
    buf[L.off_shift + nb_slot_of_feature(f)] = -d->centers[i] + 0.5;
    buf[L.off_shift + dp + nb_slot_of_feature(f)] = 1.0;
  }
  if (L.single_full) {
    // stream block: c, then the tiles of B_inv
    const nb_member_desc& md = d->members[0];
    for (int i = 0; i < n_dim; ++i) buf[L.off_stream + i] = md.c[i];
    put_tri_tiles(&buf[L.off_stream + dp], dt, n_dim, md.B_inv, (size_t)n_dim);
  }
  if (L.K > 0) fill_cdf(&buf[L.off_cdf], L.K, d->log_v_all);
  for (int f = 0; f < dp; ++f) {
    const bool boxed = d->unit_cube && f < n_dim;
    buf[L.off_ulo + nb_slot_of_feature(f)] = boxed ? 0.0 : -INF;
    buf[L.off_uhi + nb_slot_of_feature(f)] = boxed ? 1.0 : INF;
  }

  for (int m = 0; m < L.K; ++m) {
    const nb_member_desc& md = d->members[m];
    if (!fill_ell_block(buf, L.off_members + m * L.ell_size, n_dim, dt, md,
                        false))
      return NB_ERR_ARG;
    fill_draw_block(buf, L.off_draw + m * L.draw_stride, n_dim, dp, md);
  }

  for (int m = 0; m < L.M; ++m) {
    const nb_neural_desc& nd = d->neural[m];
    const size_t at = L.off_neural + m * L.neural_stride;
    if (!fill_ell_block(buf, at, n_dim, dt, nd.ellipsoid, true))
      return NB_ERR_ARG;
    buf[at + L.ell_size] = nd.score_predict_min - 1e-9;   // bounds/neural.py:125
    // bounding sphere of the ellipsoid: x inside => |x - c|^2 <= radius2
    buf[at + 1] = nd.radius2 > 0.0 ? nd.radius2 : fallback_radius2(nd.ellipsoid);
    double* mean = &buf[at + L.ell_size + 2];
    double* scale = mean + dp;
    for (int f = 0; f < dp; ++f) { mean[f] = 0.0; scale[f] = 1.0; }
    if (nd.mlp != nullptr) {
      for (int f = 0; f < n_dim; ++f) {
        mean[f] = nd.mlp->mean[f];
        scale[f] = 1.0 / nd.mlp->scale[f];   // the kernel multiplies
      }
      for (int e = 0; e < L.E; ++e)
        fill_net(scale + dp + (size_t)e * L.net_stride, n_dim, L.kt1,
                 nd.mlp->coefs + 4 * e, nd.mlp->intercepts + 4 * e);
    }
  }
  return NB_OK;
}

// ---- the prior table -------------------------------------------------------

// Phi(x) in extended precision; exact in the lower tail, where it is used
long double pt_phi(double x) {
  return 0.5L * erfcl(-(long double)x / sqrtl(2.0L));
}

// the constants of pt_truncnorm: Phi(a), 1 - Phi(b) and the mass between,
// each from the tail it lives in
void pt_truncnorm_constants(double a, double b, double* out3) {
  const long double cdf_a = pt_phi(a), sf_b = pt_phi(-b);
  long double mass;
  if (a > 0.0) {
    mass = pt_phi(-a) - sf_b;
  } else if (b < 0.0) {
    mass = pt_phi(b) - cdf_a;
  } else {                                  // straddles 0: two positive terms
    mass = 0.5L * (erfl((long double)b / sqrtl(2.0L)) +
                   erfl(-(long double)a / sqrtl(2.0L)));
  }
  out3[0] = (double)cdf_a;
  out3[1] = (double)sf_b;
  out3[2] = (double)mass;
}

// log erfcx(x / sqrt 2) for x >= NB_PRIOR_LOG_SPACE from the asymptotic series
// erfcx(y) = 1 / (y sqrt pi) sum_k (-1)^k (2k - 1)!! / (2 y^2)^k, whose terms
// fall by 2 y^2 / (2k + 1) > 600 each there
long double pt_log_erfcx_tail(double x) {
  const long double y = (long double)x / sqrtl(2.0L);
  long double term = 1.0L, sum = 1.0L;
  for (int k = 1; k <= 12; ++k) {
    term *= -(long double)(2 * k - 1) / (2.0L * y * y);
    sum += term;
  }
  return logl(sum) - logl(y) - 0.5L * logl(acosl(-1.0L));
}

// the constants of pt_truncnorm_log for [a, b], a >= NB_PRIOR_LOG_SPACE
void pt_truncnorm_log_constants(double a, double b, double* out3) {
  const long double log_ea = pt_log_erfcx_tail(a);
  long double r0 = 0.0L, r1 = 1.0L;
  if (std::isfinite(b)) {
    const long double log_r0 = pt_log_erfcx_tail(b) - log_ea -
        0.5L * ((long double)b - a) * ((long double)b + a);
    r0 = expl(log_r0);
    r1 = -expm1l(log_r0);
  }
  out3[0] = (double)log_ea;
  out3[1] = (double)r0;
  out3[2] = (double)r1;
}

// The one shape of a closed-form kind (13 weibull_min, 15 pareto, 16
// powerlaw: positive, finite, with a finite reciprocal -- the kernel
// multiplies by it; 17 triang: in [0, 1]); false and the error text otherwise
bool pt_check_shape(int kind, int j, double a) {
  if (kind == 17) {
    if (a >= 0.0 && a <= 1.0) return true;
    nb_set_error("parameter %d: triangular needs a shape 0 <= c <= 1", j);
    return false;
  }
  if (a > 0.0 && std::isfinite(a) && std::isfinite(1.0 / a)) return true;
  nb_set_error("parameter %d: %s needs a finite shape %s > 0 with a finite "
               "reciprocal", j,
               kind == 13 ? "Weibull" : kind == 15 ? "Pareto" : "power law",
               kind == 13 ? "c" : kind == 15 ? "b" : "a");
  return false;
}

// The byte image of a prior table (nb_layout.h) and the kernel variant it
// needs: 0 kinds 0 and 2 only, 1 with the normal families, 2 with log-space
// truncnorm; 3 more with a closed-form kind (7 to 17).  `out` is the handle
// pointer of the caller, tested for NULL with the other arguments (so in
// every table packer below).
int pack_prior_table(int32_t n_dim, const uint8_t* kind, const double* loc,
                     const double* scale, const double* shape0,
                     const double* shape1, int32_t n_keys,
                     const int32_t* key_column, const double* key_value,
                     const void* out, std::vector<unsigned char>* image,
                     int* level) {
  if (out == nullptr || n_dim < 1 || n_dim > 16 * NB_MAX_DT || n_keys < 1 ||
      kind == nullptr || loc == nullptr || scale == nullptr ||
      shape0 == nullptr || shape1 == nullptr || key_column == nullptr ||
      key_value == nullptr) {
    nb_set_error("bad prior table arguments");
    return NB_ERR_ARG;
  }
  const size_t d = (size_t)n_dim;
  std::vector<double> par(NB_PRIOR_NPAR * d, 0.0);
  std::vector<unsigned char> kind_dev(kind, kind + d);
  for (int j = 0; j < n_dim; ++j) {
    const double a = shape0[j], b = shape1[j];
    if (kind[j] == 6 || kind[j] > 17) {
      nb_set_error("prior kind %d of parameter %d is not supported", kind[j], j);
      return NB_ERR_UNSUPPORTED;
    }
    if (!std::isfinite(loc[j]) || !(scale[j] > 0.0) ||
        !std::isfinite(scale[j])) {
      nb_set_error("parameter %d: loc must be finite and scale positive", j);
      return NB_ERR_ARG;
    }
    par[0 * d + j] = loc[j];
    par[1 * d + j] = scale[j];
    if (kind[j] == 2) {
      if (!(a > 0.0) || !(a < b) || !std::isfinite(b)) {
        nb_set_error("parameter %d: log-uniform needs 0 < a < b < inf", j);
        return NB_ERR_ARG;
      }
      par[2 * d + j] = std::log(a);
      par[3 * d + j] = std::log(b) - std::log(a);
    } else if (kind[j] == 3) {
      if (!(a > 0.0) || !std::isfinite(a)) {
        nb_set_error("parameter %d: log-normal needs a shape s > 0", j);
        return NB_ERR_ARG;
      }
      par[2 * d + j] = a;
    } else if (kind[j] == 5) {
      if (!(a < b)) {
        nb_set_error("parameter %d: truncated normal needs a < b", j);
        return NB_ERR_ARG;
      }
      if (a > NB_PRIOR_TRUNCNORM_MAX || b < -NB_PRIOR_TRUNCNORM_MAX) {
        nb_set_error("parameter %d: a truncated normal whose interval lies "
                     "more than %g standard deviations from the mean is not "
                     "supported", j, (double)NB_PRIOR_TRUNCNORM_MAX);
        return NB_ERR_UNSUPPORTED;
      }
      double c3[3];
      if (a > NB_PRIOR_LOG_SPACE || b < -NB_PRIOR_LOG_SPACE) {
        // far tail: kind 6 on the interval mirrored to the right
        const double sign = a > 0.0 ? 1.0 : -1.0;
        const double lo = a > 0.0 ? a : -b, hi = a > 0.0 ? b : -a;
        kind_dev[j] = 6;
        par[2 * d + j] = lo;
        par[3 * d + j] = hi;
        pt_truncnorm_log_constants(lo, hi, c3);
        par[7 * d + j] = sign;
      } else {
        par[2 * d + j] = a;
        par[3 * d + j] = b;
        pt_truncnorm_constants(a, b, c3);
      }
      for (int t = 0; t < 3; ++t) par[(4 + t) * d + j] = c3[t];
    } else if (kind[j] == 13 || kind[j] == 15 || kind[j] == 16) {
      if (!pt_check_shape(kind[j], j, a)) return NB_ERR_ARG;
      par[2 * d + j] = 1.0 / a;             // rounded once, as scipy forms it
    } else if (kind[j] == 17) {
      if (!pt_check_shape(kind[j], j, a)) return NB_ERR_ARG;
      par[2 * d + j] = a;
      par[3 * d + j] = 1.0 - a;
    }
  }
  for (int k = 0; k < n_keys; ++k)
    if (key_column[k] < -1 || key_column[k] >= n_dim) {
      nb_set_error("key %d refers to column %d of %d", k, key_column[k], n_dim);
      return NB_ERR_ARG;
    }
  const size_t bytes = (NB_PRIOR_NPAR * d + (size_t)n_keys) * sizeof(double) +
                       (size_t)n_keys * sizeof(int) + d;
  image->assign(bytes, 0);
  unsigned char* at = image->data();
  std::memcpy(at, par.data(), NB_PRIOR_NPAR * d * sizeof(double));
  at += NB_PRIOR_NPAR * d * sizeof(double);
  std::memcpy(at, key_value, (size_t)n_keys * sizeof(double));
  at += (size_t)n_keys * sizeof(double);
  std::memcpy(at, key_column, (size_t)n_keys * sizeof(int));
  at += (size_t)n_keys * sizeof(int);
  std::memcpy(at, kind_dev.data(), d);
  int base = 0, closed = 0;
  for (int j = 0; j < n_dim; ++j) {
    if (kind[j] >= 7) {
      closed = 3;
      continue;
    }
    const int need = kind_dev[j] == 6 ? 2 : (kind[j] != 0 && kind[j] != 2);
    if (need > base) base = need;
  }
  *level = base + closed;
  return NB_OK;
}

// ---- the likelihood tables -------------------------------------------------

// Components of a mixture for nb_mixture.hip: records of
// nb_mixture_record(dt) doubles
int pack_mixture(int32_t n_dim, int32_t n_components, const double* means,
                 const double* chol_inv, const double* log_coef,
                 const void* out, std::vector<double>* image) {
  if (out == nullptr || means == nullptr || chol_inv == nullptr ||
      log_coef == nullptr || n_dim < 1 || n_dim > 16 * NB_MAX_DT ||
      n_components < 1 || n_components > NB_MIXTURE_MAX_COMPONENTS) {
    nb_set_error("bad mixture arguments (n_dim 1..%d, 1..%d components)",
                 16 * NB_MAX_DT, NB_MIXTURE_MAX_COMPONENTS);
    return NB_ERR_ARG;
  }
  const int dt = (n_dim + 15) / 16;
  const size_t d = (size_t)n_dim, cs = (size_t)nb_mixture_record(dt);
  const size_t nt = (size_t)dt * (dt + 1) / 2;
  std::vector<double>& host = *image;
  host.assign(cs * (size_t)n_components, 0.0);
  for (int c = 0; c < n_components; ++c) {
    const double* li = chol_inv + (size_t)c * d * d;
    const double* mu = means + (size_t)c * d;
    if (!std::isfinite(log_coef[c])) {
      nb_set_error("component %d: log_coef is not finite", c);
      return NB_ERR_ARG;
    }
    for (int h = 0; h < n_dim; ++h) {
      if (!std::isfinite(mu[h])) {
        nb_set_error("component %d: mean %d is not finite", c, h);
        return NB_ERR_ARG;
      }
      for (int k = 0; k < n_dim; ++k) {
        const double v = li[h * d + k];
        if (!std::isfinite(v) || (k > h && v != 0.0) || (k == h && !(v > 0.0))) {
          nb_set_error("component %d: chol_inv must be finite and lower "
                       "triangular with a positive diagonal (entry %d, %d)",
                       c, h, k);
          return NB_ERR_ARG;
        }
      }
    }
    double* rec = &host[cs * (size_t)c];
    put_tri_tiles(rec, dt, n_dim, li, d);
    double* tail = rec + nt * NB_TILE;
    for (int h = 0; h < n_dim; ++h) tail[h] = mu[h];
    tail[16 * dt] = log_coef[c];
  }
  return NB_OK;
}

// Appends the rows x cols matrix a (row-major, leading dimension ld) to the
// image as operand tiles in panel order, zero padded (nb_layout.h,
// nb_operand_index); lower: the lower triangle only, the k-tiles of a panel
// ending at its last row tile
void put_panel_tiles(std::vector<double>* image, const double* a, size_t ld,
                     size_t rows, size_t cols, bool lower) {
  const int dt = (int)((rows + 15) / 16);
  const auto k_tiles = [&](int pn) {
    return lower ? std::min(NB_PANEL_TILES * (pn + 1), dt)
                 : (int)((cols + 15) / 16);
  };
  const auto row_tiles = [&](int pn) {
    return std::min(NB_PANEL_TILES, dt - NB_PANEL_TILES * pn);
  };
  const int n_panels = (dt + NB_PANEL_TILES - 1) / NB_PANEL_TILES;
  size_t tiles = 0;
  for (int pn = 0; pn < n_panels; ++pn)
    tiles += (size_t)row_tiles(pn) * (size_t)k_tiles(pn);
  const size_t at = image->size();
  image->resize(at + tiles * NB_TILE, 0.0);
  double* tile = image->data() + at;
  for (int pn = 0; pn < n_panels; ++pn)
    for (int kt = 0; kt < k_tiles(pn); ++kt)
      for (int ti = 0; ti < row_tiles(pn); ++ti, tile += NB_TILE)
        for (int l = 0; l < 16; ++l) {
          const size_t h = 16 * (size_t)(NB_PANEL_TILES * pn + ti) + l;
          if (h >= rows) break;
          for (int c = 0; c < 16; ++c) {
            const size_t k = 16 * (size_t)kt + c;
            if (k < cols && (!lower || k <= h))
              tile[nb_operand_index(l, c)] = a[h * ld + k];
          }
        }
}

// Data vector and W = L^-1 (or 1 / sigma) for nb_chi2.hip (nb_layout.h,
// nb_chi2_w_offset)
int pack_chi2(int32_t n_data, const double* data, const double* chol_inv,
              const double* inv_sigma, double log_norm, const void* out,
              std::vector<double>* image) {
  if (out == nullptr || data == nullptr || n_data < 1 ||
      n_data > NB_CHI2_MAX_DATA ||
      (chol_inv == nullptr) == (inv_sigma == nullptr) ||
      !std::isfinite(log_norm)) {
    nb_set_error("bad data likelihood arguments (n_data 1..%d, exactly one "
                 "of chol_inv and inv_sigma, a finite log_norm)",
                 NB_CHI2_MAX_DATA);
    return NB_ERR_ARG;
  }
  const size_t p = (size_t)n_data;
  for (size_t k = 0; k < p; ++k)
    if (!std::isfinite(data[k])) {
      nb_set_error("data %zu is not finite", k);
      return NB_ERR_ARG;
    }
  std::vector<double>& host = *image;
  if (inv_sigma != nullptr) {
    host.assign(2 * p, 0.0);
    for (size_t k = 0; k < p; ++k) {
      if (!std::isfinite(inv_sigma[k]) || !(inv_sigma[k] > 0.0)) {
        nb_set_error("inv_sigma %zu must be positive and finite", k);
        return NB_ERR_ARG;
      }
      host[k] = data[k];
      host[p + k] = inv_sigma[k];
    }
    return NB_OK;
  }
  for (size_t h = 0; h < p; ++h)
    for (size_t k = 0; k < p; ++k) {
      const double v = chol_inv[h * p + k];
      if (!std::isfinite(v) || (k > h && v != 0.0) || (k == h && !(v > 0.0))) {
        nb_set_error("chol_inv must be finite and lower triangular with a "
                     "positive diagonal (entry %zu, %zu)", h, k);
        return NB_ERR_ARG;
      }
    }
  host.assign((size_t)nb_chi2_w_offset((n_data + 15) / 16), 0.0);
  for (size_t k = 0; k < p; ++k) host[k] = data[k];
  put_panel_tiles(&host, chol_inv, p, p, p, true);
  return NB_OK;
}

// one bin of a Poisson table: false (and the error text) unless the count,
// exposure and background are what nb_poisson_create documents
bool po_check_bin(size_t j, double k, double e, double b) {
  if (!std::isfinite(k) || k < 0.0) {
    nb_set_error("count %zu must be finite and not negative", j);
    return false;
  }
  if (k > 0.0 && !std::isfinite(1.0 / k)) {
    nb_set_error("count %zu is positive but too small: 1 / k is not finite",
                 j);
    return false;
  }
  if (!std::isfinite(e) || !(e > 0.0)) {
    nb_set_error("exposure %zu must be positive and finite", j);
    return false;
  }
  if (!std::isfinite(b) || b < 0.0) {
    nb_set_error("background %zu must be finite and not negative", j);
    return false;
  }
  return true;
}

// Counts, their reciprocals, exposure and background for nb_poisson.hip
int pack_poisson(int32_t n_data, const double* counts, const double* exposure,
                 const double* background, double log_const, const void* out,
                 std::vector<double>* image) {
  if (out == nullptr || counts == nullptr || n_data < 1 ||
      n_data > NB_POISSON_MAX_DATA || !std::isfinite(log_const)) {
    nb_set_error("bad Poisson likelihood arguments (n_data 1..%d, counts, a "
                 "finite log_const)", NB_POISSON_MAX_DATA);
    return NB_ERR_ARG;
  }
  const size_t p = (size_t)n_data;
  std::vector<double>& host = *image;
  host.assign(4 * p, 0.0);
  for (size_t j = 0; j < p; ++j) {
    const double k = counts[j];
    const double e = exposure != nullptr ? exposure[j] : 1.0;
    const double b = background != nullptr ? background[j] : 0.0;
    if (!po_check_bin(j, k, e, b)) return NB_ERR_ARG;
    host[j] = k;
    host[p + j] = k > 0.0 ? 1.0 / k : 0.0;
    host[2 * p + j] = e;
    host[3 * p + j] = b;
  }
  return NB_OK;
}

// The table of pack_poisson and the response matrix for nb_fold.hip
// (nb_layout.h, nb_fold_r_offset)
int pack_fold_poisson(int32_t n_data, int32_t n_src, const double* counts,
                      const double* response, int64_t ld_response,
                      const double* exposure, const double* background,
                      double log_const, const void* out,
                      std::vector<double>* image) {
  // the sizes before any array is read
  const bool sizes = n_data >= 1 && n_data <= NB_POISSON_MAX_DATA &&
                     n_src >= 1 && n_src <= NB_FOLD_MAX_SOURCE &&
                     ((int64_t)(n_data + 15) / 16) * ((n_src + 15) / 16) * 256 <=
                         NB_FOLD_MAX_RESPONSE;
  if (out == nullptr || counts == nullptr || response == nullptr || !sizes ||
      ld_response < n_src || !std::isfinite(log_const)) {
    nb_set_error("bad folded Poisson likelihood arguments (n_data 1..%d, "
                 "n_src 1..%d, ceil16(n_data) ceil16(n_src) <= %d, counts, "
                 "response with ld_response >= n_src, a finite log_const)",
                 NB_POISSON_MAX_DATA, NB_FOLD_MAX_SOURCE,
                 NB_FOLD_MAX_RESPONSE);
    return NB_ERR_ARG;
  }
  const size_t p = (size_t)n_data, ks = (size_t)n_src;
  const int dt = (n_data + 15) / 16;
  const size_t pp = 16 * (size_t)dt;             // padded table arrays
  std::vector<double>& host = *image;
  host.assign(nb_fold_r_offset(dt), 0.0);
  for (size_t j = 0; j < pp; ++j) host[2 * pp + j] = 1.0;
  for (size_t j = 0; j < p; ++j) {
    const double k = counts[j];
    const double e = exposure != nullptr ? exposure[j] : 1.0;
    const double b = background != nullptr ? background[j] : 0.0;
    if (!po_check_bin(j, k, e, b)) return NB_ERR_ARG;
    host[j] = k;
    host[pp + j] = k > 0.0 ? 1.0 / k : 0.0;
    host[2 * pp + j] = e;
    host[3 * pp + j] = b;
    for (size_t c = 0; c < ks; ++c)
      if (!std::isfinite(response[j * (size_t)ld_response + c])) {
        nb_set_error("response entry (%zu, %zu) is not finite", j, c);
        return NB_ERR_ARG;
      }
  }
  put_panel_tiles(&host, response, (size_t)ld_response, p, ks, false);
  return NB_OK;
}

// Data and sigma^2 for nb_noise.hip
int pack_noise(int32_t n_data, const double* data, const double* sigma2,
               double log_norm, const void* out, std::vector<double>* image) {
  if (out == nullptr || data == nullptr || n_data < 1 ||
      n_data > NB_NOISE_MAX_DATA || !std::isfinite(log_norm)) {
    nb_set_error("bad noise likelihood arguments (n_data 1..%d, data, a "
                 "finite log_norm)", NB_NOISE_MAX_DATA);
    return NB_ERR_ARG;
  }
  const size_t p = (size_t)n_data;
  std::vector<double>& host = *image;
  host.assign(2 * p, 0.0);
  for (size_t j = 0; j < p; ++j) {
    if (!std::isfinite(data[j])) {
      nb_set_error("data point %zu must be finite", j);
      return NB_ERR_ARG;
    }
    host[j] = data[j];
    if (sigma2 == nullptr) continue;
    if (!std::isfinite(sigma2[j]) || sigma2[j] < 0.0) {
      nb_set_error("sigma2 %zu must be finite and not negative", j);
      return NB_ERR_ARG;
    }
    host[p + j] = sigma2[j];
  }
  return NB_OK;
}

// Data, sigma^2 and the distance tiles for nb_gp.hip (nb_layout.h,
// nb_gp_tile / nb_gp_index); dist may be absent
int pack_gp(int32_t n_data, const double* data, const double* sigma2,
            const double* dist, int32_t kernel, double log_norm,
            const void* out, std::vector<double>* image) {
  if (out == nullptr || data == nullptr || n_data < 1 ||
      n_data > NB_GP_MAX_DATA || kernel < NB_GP_SQEXP ||
      kernel > NB_GP_MATERN52 || !std::isfinite(log_norm)) {
    nb_set_error("bad Gaussian-process likelihood arguments (n_data 1..%d, "
                 "data, a kernel NB_GP_SQEXP .. NB_GP_MATERN52, a finite "
                 "log_norm)", NB_GP_MAX_DATA);
    return NB_ERR_ARG;
  }
  const size_t p = (size_t)n_data;
  const int t = (n_data + 15) / 16;
  std::vector<double>& host = *image;
  host.assign((size_t)nb_gp_table_doubles(t, dist != nullptr), 0.0);
  for (size_t j = 0; j < p; ++j) {
    if (!std::isfinite(data[j])) {
      nb_set_error("data point %zu must be finite", j);
      return NB_ERR_ARG;
    }
    host[j] = data[j];
    if (sigma2 == nullptr) continue;
    if (!std::isfinite(sigma2[j]) || sigma2[j] < 0.0) {
      nb_set_error("sigma2 %zu must be finite and not negative", j);
      return NB_ERR_ARG;
    }
    host[16 * (size_t)t + j] = sigma2[j];
  }
  if (dist == nullptr) return NB_OK;
  double* tiles = host.data() + nb_gp_dist_offset(t);
  for (size_t j = 0; j < p; ++j)
    for (size_t k = 0; k <= j; ++k) {
      const double v = dist[j * p + k];
      if (!std::isfinite(v) || v < 0.0 || v != dist[k * p + j] ||
          (j == k && v != 0.0)) {
        nb_set_error("dist entry (%zu, %zu) must be finite, not negative, "
                     "equal to entry (%zu, %zu) and zero on the diagonal",
                     j, k, k, j);
        return NB_ERR_ARG;
      }
      tiles[(size_t)nb_gp_tile((int)(j / 16), (int)(k / 16)) * NB_TILE +
            nb_gp_index((int)(j % 16), (int)(k % 16))] = v;
    }
  return NB_OK;
}

// The steps t_j - t_j-1, data and sigma^2 for nb_gps_filter.h (nb_layout.h,
// NB_GPS_STRIDE doubles per datum)
int pack_gps(int32_t n_data, const double* t, const double* data,
             const double* sigma2, int32_t kernel, double log_norm,
             const void* out, std::vector<double>* image) {
  if (out == nullptr || t == nullptr || data == nullptr || n_data < 1 ||
      n_data > NB_GPS_MAX_DATA || kernel < NB_GPS_EXP ||
      kernel > NB_GPS_SHO || !std::isfinite(log_norm)) {
    nb_set_error("bad Gaussian-process series likelihood arguments (n_data "
                 "1..%d, t, data, a kernel NB_GPS_EXP .. NB_GPS_SHO, a finite "
                 "log_norm)", NB_GPS_MAX_DATA);
    return NB_ERR_ARG;
  }
  const size_t p = (size_t)n_data;
  std::vector<double>& host = *image;
  host.assign(nb_gps_table_doubles(n_data), 0.0);
  for (size_t j = 0; j < p; ++j) {
    double* e = host.data() + NB_GPS_STRIDE * j;
    if (!std::isfinite(t[j])) {
      nb_set_error("t %zu must be finite", j);
      return NB_ERR_ARG;
    }
    if (j > 0) {
      if (t[j] < t[j - 1]) {
        nb_set_error("t must not decrease: t %zu is below t %zu", j, j - 1);
        return NB_ERR_ARG;
      }
      const double dt = t[j] - t[j - 1];
      if (!std::isfinite(dt)) {
        nb_set_error("t %zu is too far from t %zu: the step is not finite",
                     j, j - 1);
        return NB_ERR_ARG;
      }
      e[NB_GPS_DT] = dt;
    }
    if (!std::isfinite(data[j])) {
      nb_set_error("data point %zu must be finite", j);
      return NB_ERR_ARG;
    }
    e[NB_GPS_DATA] = data[j];
    if (sigma2 == nullptr) continue;
    if (!std::isfinite(sigma2[j]) || sigma2[j] < 0.0) {
      nb_set_error("sigma2 %zu must be finite and not negative", j);
      return NB_ERR_ARG;
    }
    e[NB_GPS_SIGMA2] = sigma2[j];
  }
  return NB_OK;
}

static_assert(NB_GPS_MAX_TERMS == 3, "the slots of nb_gps_plan (nb_layout.h)");

constexpr int gps_plan_states(int kernel) {
  return kernel == NB_GPS_EXP ? 1 : kernel == NB_GPS_MATERN52 ? 3 : 2;
}

// The plan of one term, whose hyper row is (a, l, s[, q]); pack_gps checks
// the kernel.
nb_gps_plan plan_gps_one(int32_t kernel) {
  nb_gps_plan p;
  p.n_terms = 1;
  p.kind[0] = kernel;
  p.col_q[0] = kernel == NB_GPS_SHO ? 3 : 0;
  p.col_s = 2;
  p.width = kernel == NB_GPS_SHO ? 4 : 3;
  p.states = gps_plan_states(kernel);
  return p;
}

// The checks of nb_gps_create_terms that nb_gps_create does not have, and
// the plan; pack_gps checks the rest and packs the same image.
int plan_gps_terms(int32_t n_terms, const int32_t* kernels, const double* t,
                   const double* data, const void* out, nb_gps_plan* plan) {
  if (kernels == nullptr || t == nullptr || data == nullptr ||
      out == nullptr) {
    nb_set_error("the Gaussian-process series likelihood of a sum of terms "
                 "needs kernels, t, data and out: no NULL pointer");
    return NB_ERR_ARG;
  }
  if (n_terms < 2 || n_terms > NB_GPS_MAX_TERMS) {
    nb_set_error("the Gaussian-process series likelihood of a sum takes 2..%d "
                 "terms, not %d (one term goes through nb_gps_create)",
                 NB_GPS_MAX_TERMS, (int)n_terms);
    return NB_ERR_ARG;
  }
  nb_gps_plan p;
  p.n_terms = n_terms;
  int first[NB_GPS_MAX_TERMS];                   // of a term, caller's order
  int column = 0;
  for (int i = 0; i < n_terms; ++i) {
    if (kernels[i] < NB_GPS_EXP || kernels[i] > NB_GPS_SHO) {
      nb_set_error("term %d of the Gaussian-process series likelihood has "
                   "kernel %d: not one of NB_GPS_EXP .. NB_GPS_SHO", i,
                   (int)kernels[i]);
      return NB_ERR_ARG;
    }
    first[i] = column;
    column += kernels[i] == NB_GPS_SHO ? 3 : 2;
    p.states += gps_plan_states(kernels[i]);
  }
  if (p.states > NB_GPS_MAX_STATES) {
    nb_set_error("the terms of the Gaussian-process series likelihood have %d "
                 "states (exp 1, matern32 2, matern52 3, sho 2): at most %d, "
                 "in at most %d terms", p.states, NB_GPS_MAX_STATES,
                 NB_GPS_MAX_TERMS);
    return NB_ERR_ARG;
  }
  p.col_s = column;
  p.width = column + 1;
  // a stable insertion sort of at most three
  int order[NB_GPS_MAX_TERMS] = {0, 1, 2};
  for (int i = 1; i < n_terms; ++i)
    for (int j = i; j > 0 && kernels[order[j]] < kernels[order[j - 1]]; --j) {
      const int swap = order[j];
      order[j] = order[j - 1];
      order[j - 1] = swap;
    }
  for (int i = 0; i < n_terms; ++i) {
    p.kind[i] = kernels[order[i]];
    p.col[i] = first[order[i]];
    p.col_q[i] = p.kind[i] == NB_GPS_SHO ? p.col[i] + 2 : 0;
  }
  *plan = p;
  return NB_OK;
}

}  // namespace
