// The layout contract between the host packers (nb_pack.h) and the kernels:
// sizes, offsets and header words of everything the host builds and the device
// reads.  Plain C++ without HIP -- constexpr functions are host and device
// functions under hipcc -- so that tests/pack_check.cpp builds it on its own.
// nb_common.h includes it for every kernel file.
#pragma once

#include <stddef.h>
#include <stdint.h>

#define NB_MAX_DT 8          // n_dim <= 128
#define NB_H1 100            // hidden sizes of the emulator, nautilus/neural.py:80
#define NB_H2 50
#define NB_H3 20
#define NB_HT1 7             // 16-wide tiles covering the hidden layers
#define NB_HT2 4
#define NB_HT3 2
#define NB_TILE 256          // doubles in one 16x16 tile
#define NB_PRIOR_NPAR 8      // rows of a prior table (nb_transform.hip, PT_*)

// ---------------------------------------------------------------------------
// Device "bound blob": one contiguous array of doubles per bound, built on the
// host by pack_bound (nb_pack.h) and uploaded once by nb_bound_create.  The
// first NB_HDR doubles hold integers (stored as int64 bit patterns) describing
// the layout; all offsets are in doubles from the start of the blob.  With
// DP = 16 DT:
//
//   hdr[0] n_dim D          hdr[1] DT = ceil(D/16)     hdr[2] K outer members
//   hdr[3] use_cube         hdr[4] M neural bounds     hdr[5] E nets per bound
//   hdr[6] off_cdf (K doubles, padded to even)          hdr[7] off_ulo (DP)
//   hdr[8] off_uhi (DP)     hdr[9] off_members (K ell blocks, stride ell_stride)
//   hdr[10] ell_stride      hdr[11] off_neural (M neural blocks)
//   hdr[12] neural_stride   hdr[13] off_draw (K draw blocks)  hdr[14] draw_stride
//   hdr[15] mlp_net_stride  hdr[16] KT1 (k-tiles of MLP layer 1 incl. bias row)
//   hdr[17] total doubles   hdr[18] off_stream (single full ellipsoid without
//                           a cube only, else 0; after the draw blocks)
//   hdr[19] off_shift (0 = no periodic dimensions; after the stream block)
//
// Slot order.  A vector of DP per-dimension values (limits, centres, shifts)
// is stored in the order the ellipsoid stage holds its K operands: feature f
// at slot nb_slot_of_feature(f) = 16 (f / 16) + 4 (2 ((f / 8) % 2) + f % 2) +
// (f % 8) / 2, i.e. k-step ks = slot / 4 of lane group lg = slot % 4 holds
// feature 8 (ks / 2) + 2 lg + ks % 2.
//
// Header, CDF, ulo / uhi (the unit cube of a union, slot order, -+inf where
// not boxed): nb_geom.hip, nb_cand.hip, nb_eval_fast.hip, nb_kernels.hip.
//
// Ell block (member of the outer union, or ellipsoid of a neural bound); read
// by nb_geom.hip, nb_cand.hip, nb_eval_fast.hip and nb_transform.hip:
//   [0]            n_ell (as int64 bits; 0 => pure cube member, no MFMA work)
//   [1]            members: 1 if any limit is finite, else 0 (int64 bits);
//                  neural bounds: the squared bounding radius (a double)
//   [2 .. 2+DP)    lo   lower limit (0 for cube dims, -inf else), slot order
//   [..+DP)        hi   upper limit (1 for cube dims, +inf else), slot order
//   [..+DP)        c    centre embedded in full-D order (0 for cube dims),
//                  slot order
//   [.. DT*DT tiles)  W0[k][h] = B_inv[h][k] embedded in full-D order, as
//                  16x16 tiles [kt][ht] with the K index in slot order: with
//                  sl = nb_slot_of_feature(k), ks = sl / 4, lg = sl % 4 the
//                  element lives in tile (ks / 4, h / 16) at
//                  (ks % 4) * 64 + lg * 16 + h % 16
// Neural block = ell block, then (nb_eval_fast.hip):
//   thr, pad       score_predict_min - 1e-9 (bounds/neural.py:125)
//   mean[DP], inv_scale[DP]   in feature order (0 and 1 beyond D)
//   E nets, each: L1 tiles [KT1][7], L2 [7][4], L3 [4][2], L4 [2][1];
//   weights W_l[k][h] with the bias stored as row k = K_l, zero padded, in
//   tile (k / 16, h / 16), element (kk, hh) at kk*16+hh
// Draw block (compact, for the per-proposal VALU draw of nb_draw.h):
//   n_ell, n_cube, idx_ell[DP], idx_cube[DP], slot_of_column[DP] (as int64
//   bits), c[n_ell->DP], B packed lower-triangular row-major [DP*(DP+1)/2]
// Stream block (nb_stream.hip): c[DP] in feature order, then the DT(DT+1)/2
//   lower-triangular tiles of B_inv written by put_tri_tiles (nb_pack.h): tile
//   (ht, kt), kt <= ht, is number ht (ht + 1) / 2 + kt; in it k-step s of lane
//   group lg holds column 16 kt + 8 (s / 2) + 2 lg + s % 2 of row 16 ht + l at
//   s * 64 + lg * 16 + l
// Shift block: shift[DP], on[DP] in slot order; contains() tests
//   frac(x + shift) where on (bounds/periodic.py:50-72)
// ---------------------------------------------------------------------------
#define NB_HDR 32

enum {
  NB_H_NDIM = 0, NB_H_DT, NB_H_K, NB_H_USECUBE, NB_H_M, NB_H_E, NB_H_OFF_CDF,
  NB_H_OFF_ULO, NB_H_OFF_UHI, NB_H_OFF_MEMBERS, NB_H_ELL_STRIDE,
  NB_H_OFF_NEURAL, NB_H_NEURAL_STRIDE, NB_H_OFF_DRAW, NB_H_DRAW_STRIDE,
  NB_H_NET_STRIDE, NB_H_KT1, NB_H_TOTAL, NB_H_OFF_STREAM, NB_H_OFF_SHIFT
};

// K permutation of the ellipsoid stage (nb_tile.h / nb_stream.hip): slot
// (ks, lg) <-> feature 8*(ks>>1) + 2*lg + (ks&1).
constexpr int nb_slot_of_feature(int f) {
  return 4 * (2 * (f >> 3) + (f & 1)) + ((f & 7) >> 1);
}

constexpr int nb_ell_block_size(int dt) {
  return 2 + 3 * dt * 16 + dt * dt * NB_TILE;   // even => 16-byte aligned tiles
}
// tiles of one network given KT1
constexpr int nb_net_tiles(int kt1) {
  return kt1 * NB_HT1 + NB_HT1 * NB_HT2 + NB_HT2 * NB_HT3 + NB_HT3 * 1;
}

// One component of a Gaussian mixture (nb_mixture.hip) is a record of
// DT(DT+1)/2 tiles of L^-1 (put_tri_tiles, as in the stream block), then a
// tail: mu[16 DT], a_k, padding up to a multiple of the 1 KB a wavefront
// copies per global_load_lds instruction
constexpr int nb_mixture_tail(int dt) {
  return (16 * dt + 1 + 127) / 128 * 128;
}
constexpr int nb_mixture_record(int dt) {
  return dt * (dt + 1) / 2 * NB_TILE + nb_mixture_tail(dt);
}

// Operand tile of the likelihoods that stream model rows (nb_chi2.hip,
// nb_fold.hip): element (row l, column c) of a 16x16 tile; lane group c / 4 of
// k-step c % 4 holds column c (what a staging thread of the kernel reads as
// 32 contiguous bytes of a model row).  The matrix of such a likelihood is
// stored as operand tiles, zero padded, in PANEL ORDER, the order the panel
// driver (nb_panel.h) walks them: panels of NB_PANEL_TILES row tiles; per
// panel its k-tiles (all of them, or of a lower-triangular matrix 0 .. the
// panel's last row tile); per k-tile the panel's row tiles.
constexpr int nb_operand_index(int l, int c) {
  return (c & 3) * 64 + (c >> 2) * 16 + l;
}
#define NB_PANEL_TILES 16

// Gaussian likelihood of a data vector (nb_chi2.hip).  Full covariance: the
// blob is d zero padded to 16 DT doubles (rounded up to the 1 KB of a
// global_load_lds piece), then the lower triangle of W = L^-1 in panel order.
// Diagonal covariance: d [P], then 1 / sigma [P].
constexpr int nb_chi2_w_offset(int dt) {
  return (16 * dt + 127) / 128 * 128;
}

// Poisson likelihood of binned counts (nb_poisson.hip).  The table is four
// arrays of P doubles: k, 1 / k (0 where k = 0), exposure, background.
//
// Gaussian likelihood with a variance that depends on the point
// (nb_noise.hip).  The table is two arrays of P doubles: d, sigma^2.
//
// Poisson likelihood behind a response matrix (nb_fold.hip).  The blob is the
// Poisson table with each array zero padded to 16 DT doubles (1 for the
// exposure), then all of R (P x K) in panel order.
constexpr size_t nb_fold_r_offset(int dt) {
  return 64 * (size_t)dt;
}

// Gaussian-process likelihood (nb_gp.hip), T = ceil(P / 16).  The table is d
// and sigma^2, each zero padded to 16 T doubles, then -- unless the handle was
// made without distances -- the distance matrix as the T (T + 1) / 2 tiles of
// its lower triangle: tile (ti, tj), tj <= ti, is number nb_gp_tile(ti, tj)
// and holds element (row 16 ti + r, column 16 tj + c) at nb_gp_index(r, c),
// column-major, so that k-step s of an fp64 MFMA operand is the 64 contiguous
// doubles from 64 s on.  Rows and columns from P on hold zeros, and so does
// the part of a diagonal tile above the diagonal.  The kernel keeps K in LDS
// in the same order (nb_gp_lds_doubles: the tiles, the residual, the pivots,
// the y of a panel, 16 reciprocals and a flag word).
constexpr int nb_gp_tile(int ti, int tj) { return ti * (ti + 1) / 2 + tj; }
constexpr int nb_gp_index(int r, int c) { return 16 * c + r; }
constexpr int nb_gp_tiles(int t) { return t * (t + 1) / 2; }
constexpr int nb_gp_dist_offset(int t) { return 32 * t; }
constexpr int nb_gp_table_doubles(int t, bool with_dist) {
  return nb_gp_dist_offset(t) + (with_dist ? nb_gp_tiles(t) * NB_TILE : 0);
}
constexpr int nb_gp_lds_doubles(int t) {
  return nb_gp_tiles(t) * NB_TILE + 2 * 16 * t + 16 + 16 + 2;
}
// wavefronts of a workgroup at T tiles
constexpr int nb_gp_waves(int t) { return t <= 2 ? 1 : t <= 4 ? 2 : 4; }

// Gaussian-process likelihood of an ordered series (nb_gps_filter.h).  The
// table is NB_GPS_STRIDE doubles per datum j: dt_j = t_j - t_j-1 rounded once
// (dt_0 = 0), d_j, sigma_j^2 and a zero -- 32 aligned bytes, one scalar load of
// the wavefront per step.  The kernel stages the model's rows through LDS in
// blocks of NB_GPS_BLOCK columns.
#define NB_GPS_STRIDE 4
#define NB_GPS_DT 0
#define NB_GPS_DATA 1
#define NB_GPS_SIGMA2 2
#define NB_GPS_BLOCK 32
constexpr size_t nb_gps_table_doubles(int p) {
  return (size_t)NB_GPS_STRIDE * (size_t)p;
}

// Where the kernel finds the one to three terms in a row of the hyper input
// (plan_gps_one, plan_gps_terms of nb_pack.h): the slots are the terms sorted
// by kernel code, equal codes in the caller's order; kind[I] is the code of
// slot I, col[I] the column of its (a, l) and, for NB_GPS_SHO, col_q[I] that
// of its q (0 otherwise: not read); col_s is the column of s.  One term's row
// is (a, l, s[, q]); a sum's holds (a, l[, q]) per term in the CALLER's order
// and s in its last column, col_s = width - 1.
struct nb_gps_plan {
  int n_terms = 0;
  int kind[3] = {0, 0, 0};                       // NB_GPS_MAX_TERMS
  int col[3] = {0, 0, 0};
  int col_q[3] = {0, 0, 0};
  int col_s = 0;
  int width = 0;                                 // doubles of a hyper row
  int states = 0;
};

// Prior table (nb_transform.hip, PT_* rows): one allocation holding
// par[NB_PRIOR_NPAR][n_dim], key_value[n_keys], key_column[n_keys] (int) and
// kind[n_dim] (bytes), in that order (doubles first, so everything is aligned).

// ---------------------------------------------------------------------------
// error handling for the C ABI
// ---------------------------------------------------------------------------
#define NB_OK 0
#define NB_ERR_ARG 1
#define NB_ERR_HIP 2
#define NB_ERR_UNSUPPORTED 3

void nb_set_error(const char* fmt, ...);
