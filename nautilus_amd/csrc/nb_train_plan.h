// Host arithmetic of the emulator trainer (nb_mlp_train.hip): where a weight
// lives in the tile-major buffers, which workgroup updates which weight tile
// in the gradient phase, which XCDs a resident trainer owns, how its device
// memory is laid out and how many steps an epoch has.  Plain C++17 without
// HIP, so that tests/train_plan_check.cpp builds it on its own; internal
// linkage, like the rest of the trainer's one translation unit.  The includer
// brings the layer shapes (nb_common.h; the test program its own):
#pragma once

#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

static_assert(NB_H1 == 100 && NB_H2 == 50 && NB_H3 == 20 && NB_HT1 == 7 &&
              NB_HT2 == 4 && NB_HT3 == 2 && NB_TILE == 256,
              "g_early spells out the 7 x 4, 4 x 2 and 2 x 1 tiles");

namespace {

constexpr int MAXB = 208;        // minibatch rows padded to 16 (batch <= 200)
constexpr int G_ROWT = MAXB / 16;   // 16-row tiles of a minibatch
constexpr int XCD_SLOTS = 32;            // workgroups per network: one per CU
constexpr int G_JOB_INTS = 5;     // layer (0..3), kt0, nk, ht0, nh

// Weight tiles (W: [kt][ht], contraction index c = input unit; WT: [ht][kt],
// c = output unit) are stored so that a lane finds the operands of two
// consecutive k-steps side by side: k-step 2 P + j of the tile row covers
// c = 8 P + 2 lg + j (lg = lane / 16), and element (c, r) of a tile lives at
// ((c / 8) * 64 + ((c / 2) % 4) * 16 + r) * 2 + c % 2 -- one 16-byte load per
// lane and PAIR of k-steps, 1 KB contiguous per wavefront.  A CU's texture
// path moves ~26 B / clk with 8-byte and ~53 B / clk with 16-byte loads per
// lane (profiles/tools/l2_read_bench.hip), and the forward / backward phase is made of
// waiting for exactly these operands.  (constexpr: host and device)
constexpr int tile_index(int c, int r) {
  return ((c >> 3) * 64 + ((c >> 1) & 3) * 16 + r) * 2 + (c & 1);
}

void put_w(double* tiles, int ht_n, int k, int h, double v) {
  tiles[((size_t)(k >> 4) * ht_n + (h >> 4)) * NB_TILE +
        tile_index(k & 15, h & 15)] = v;
}
double get_w(const double* tiles, int ht_n, int k, int h) {
  return tiles[((size_t)(k >> 4) * ht_n + (h >> 4)) * NB_TILE +
               tile_index(k & 15, h & 15)];
}
// transposed copy: tiles [ht][kt], element (hh, kk)
void put_wt(double* tiles, int kt_n, int k, int h, double v) {
  tiles[((size_t)(h >> 4) * kt_n + (k >> 4)) * NB_TILE +
        tile_index(h & 15, k & 15)] = v;
}

// Layer l (0-3) of a network: W[k][h], k < rows, the bias as row k = rows, in
// kt_n x ht_n tiles from double `off` of the network's buffer on; the
// transposed tiles (layers 2-4: the backward pass's operands) from `wt_off`
// of theirs.  l = 4: the sizes of the two buffers.
struct NetLayer { int rows, cols, kt_n, ht_n; size_t off, wt_off; };
constexpr NetLayer net_layer(int l, int n_dim, int kt1) {
  const int rows[5] = {n_dim, NB_H1, NB_H2, NB_H3, 0};
  const int cols[5] = {NB_H1, NB_H2, NB_H3, 1, 0};
  const int kt_n[5] = {kt1, NB_HT1, NB_HT2, NB_HT3, 0};
  const int ht_n[5] = {NB_HT1, NB_HT2, NB_HT3, 1, 0};
  NetLayer y = {rows[l], cols[l], kt_n[l], ht_n[l], 0, 0};
  for (int i = 0; i < l; ++i) {
    y.off += (size_t)kt_n[i] * ht_n[i] * NB_TILE;
    if (i > 0) y.wt_off += (size_t)kt_n[i] * ht_n[i] * NB_TILE;
  }
  return y;
}

// coefs[l]: (rows, cols) row-major, icpts[l]: (cols) -> the tiles w and the
// transposed tiles wt, zero padded
void pack_network(int n_dim, int kt1, const double* const* coefs,
                  const double* const* icpts, std::vector<double>& w,
                  std::vector<double>& wt) {
  w.assign(net_layer(4, n_dim, kt1).off, 0.0);
  wt.assign(net_layer(4, n_dim, kt1).wt_off, 0.0);
  for (int l = 0; l < 4; ++l) {
    const NetLayer y = net_layer(l, n_dim, kt1);
    for (int k = 0; k <= y.rows; ++k)
      for (int h = 0; h < y.cols; ++h) {
        const double v =
            k < y.rows ? coefs[l][(size_t)k * y.cols + h] : icpts[l][h];
        put_w(w.data() + y.off, y.ht_n, k, h, v);
        if (l > 0) put_wt(wt.data() + y.wt_off, y.kt_n, k, h, v);
      }
  }
}
void unpack_network(int n_dim, int kt1, const double* w, double* const* coefs,
                    double* const* icpts) {
  for (int l = 0; l < 4; ++l) {
    const NetLayer y = net_layer(l, n_dim, kt1);
    for (int k = 0; k <= y.rows; ++k)
      for (int h = 0; h < y.cols; ++h)
        *(k < y.rows ? &coefs[l][(size_t)k * y.cols + h] : &icpts[l][h]) =
            get_w(w + y.off, y.ht_n, k, h);
  }
}

// The job list of the forms without a schedule (two launches per step; two
// networks per XCD): blocks of up to 2 x 2 tiles per layer, shaped so that a
// network needs at most 32 jobs at every n_dim (two rounds of 16 workgroups).
std::vector<int> g_jobs_rounds(int kt1) {
  std::vector<int> jobs;
  auto blocks = [&](int layer, int kt_n, int ht_n, int bk, int bh) {
    for (int kt = 0; kt < kt_n; kt += bk)
      for (int ht = 0; ht < ht_n; ht += bh) {
        const int rec[G_JOB_INTS] = {layer, kt, kt + bk <= kt_n ? bk : 1, ht,
                                     ht + bh <= ht_n ? bh : 1};
        jobs.insert(jobs.end(), rec, rec + G_JOB_INTS);
      }
  };
  // layer 1 (kt1 x 7 tiles): pairs along k up to 64 dimensions, 2 x 2 beyond
  blocks(0, kt1, NB_HT1, 2, kt1 <= 4 ? 1 : 2);
  // layer 2 (7 x 4): pairs along h, 2 x 2 where layer 1 needs the workgroups
  blocks(1, NB_HT1, NB_HT2, kt1 >= 7 ? 2 : 1, 2);
  blocks(2, NB_HT2, NB_HT3, 2, 2);      // layer 3 (4 x 2)
  blocks(3, NB_HT3, 1, 2, 1);           // layer 4 (2 x 1)
  return jobs;
}

// The jobs of the G phase (see g_job) and their schedule on the 32 workgroups
// of a resident network.
//
// Jobs: blocks of nk x nh (1 or 2 each) weight tiles of one layer.  Measured
// on the resident kernel (profiles/r04/second_session/train_phases_*.txt) a
// job costs about 2.2 k ticks + 0.8 k per operand column block + 1.35 k per
// tile (MFMA chains, reduction, Adam, stores).
//
// Schedule: the G_ROWT workgroups with a row tile run FB; the other 19 start
// an EARLY job each -- the 38 tiles of the layers 2-4 -- G_HEAD ticks before
// the barrier that ends FB opens, and are free for a LATE job when they are
// through; the layer-1 tiles are all late.  Searched: the block shape of the
// late jobs (the job that ends last is split while that shortens the phase),
// and the number of workgroups without a row tile that are kept for a late
// job ONLY -- the early jobs then move together, pairs of them becoming 2 x 2
// blocks.  (n_dim 50: thirteen 2-tile late jobs on the FB workgroups, the
// fourteenth on a workgroup of its own, sixteen 2-tile early jobs and two of
// 3 x 1 tiles.)  G_HEAD is small: the report of the upper stash takes three
// round trips to the L2 (store acknowledgement, counter, poll) of ~500 ticks.
constexpr double G_HEAD = 3.0;
static double g_cost(int nk, int nh) {
  return 2.2 + 0.8 * (nk + nh) + 1.35 * nk * nh;
}
struct GRec { int layer, kt0, nk, ht0, nh; };

static void g_blocks(std::vector<GRec>& out, int layer, int kt_n, int ht_n,
                     int bk, int bh) {
  for (int kt = 0; kt < kt_n; kt += bk)
    for (int ht = 0; ht < ht_n; ht += bh)
      out.push_back({layer, kt, kt + bk <= kt_n ? bk : kt_n - kt, ht,
                     ht + bh <= ht_n ? bh : 1});
}

// the early jobs (the 38 tiles of the layers 2-4): 19 of two tiles, or fewer
// with 3 x 1 jobs among them -- level 1: layer 3 as (3, 3, 2) tiles instead of
// four pairs; levels 2, 3: the columns of one / both output-tile pairs of
// layer 2 as (3, 2, 2) along k instead of seven 1 x 2 jobs per pair
static std::vector<GRec> g_early(int level) {
  std::vector<GRec> out;
  if (level >= 1) {                              // layer 3 (4 x 2 tiles)
    out.push_back({2, 0, 3, 0, 1});
    out.push_back({2, 0, 3, 1, 1});
    out.push_back({2, 3, 1, 0, 2});
  } else {
    g_blocks(out, 2, NB_HT2, NB_HT3, 2, 1);
  }
  for (int ht = 0; ht < NB_HT2; ht += 2) {       // layer 2 (7 x 4 tiles)
    if (level >= 2 + ht / 2) {
      for (int h = ht; h < ht + 2; ++h) {
        out.push_back({1, 0, 3, h, 1});
        out.push_back({1, 3, 2, h, 1});
        out.push_back({1, 5, 2, h, 1});
      }
    } else {
      for (int kt = 0; kt < NB_HT1; ++kt) out.push_back({1, kt, 1, ht, 2});
    }
  }
  out.push_back({3, 0, 2, 0, 1});                // layer 4 (2 x 1 tiles)
  return out;
}

struct GPlan {
  std::vector<GRec> early, late;
  std::vector<int> early_slot, late_slot;
  double span = 1e30;
};

// the dearest late job to the workgroup that is free first, and so on
static double g_pair(const std::vector<GRec>& late,
                     const std::vector<std::pair<double, int>>& free_at,
                     std::vector<int>& slot_of, int& critical) {
  std::vector<int> idx(late.size());
  for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int)i;
  std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) {
    return g_cost(late[x].nk, late[x].nh) > g_cost(late[y].nk, late[y].nh);
  });
  slot_of.assign(late.size(), -1);
  double span = 0.0;
  critical = -1;
  for (size_t r = 0; r < idx.size(); ++r) {
    const int j = idx[r];
    const double end = free_at[r].first + g_cost(late[j].nk, late[j].nh);
    slot_of[j] = free_at[r].second;
    if (end > span) { span = end; critical = j; }
  }
  return span;
}

// jobs: records of G_JOB_INTS ints; sched: (early, late) job index per
// workgroup, -1 = none.  f_lo, f_sh >= 0 (experiments) force the number of
// late-only workgroups / the block shape of the late jobs instead of taking
// the cost model's choice.
void g_plan(int kt1, int f_lo, int f_sh, std::vector<int>& jobs,
            std::vector<int>& sched) {
  const int n_free = XCD_SLOTS - G_ROWT;
  GPlan best;
  const int shapes[5][2] = {{2, 1}, {1, 2}, {3, 1}, {2, 2}, {1, 1}};
  for (int late_only = 0; late_only <= 3; ++late_only) {
    if (f_lo >= 0 && late_only != f_lo) continue;
    const std::vector<GRec> early = g_early(late_only);
    if ((int)early.size() + late_only != n_free) continue;
    // when the workgroups are free for a late job
    std::vector<std::pair<double, int>> free_at;
    std::vector<int> early_slot(early.size());
    double early_end = 0.0;
    for (int w = 0; w < G_ROWT + late_only; ++w) free_at.push_back({0.0, w});
    for (size_t i = 0; i < early.size(); ++i) {
      const int w = G_ROWT + late_only + (int)i;
      double c = g_cost(early[i].nk, early[i].nh) - G_HEAD;
      if (c < 0.0) c = 0.0;
      if (c > early_end) early_end = c;
      free_at.push_back({c, w});
      early_slot[i] = w;
    }
    std::stable_sort(free_at.begin(), free_at.end(),
                     [](const std::pair<double, int>& x,
                        const std::pair<double, int>& y) {
                       return x.first < y.first;
                     });
    for (int si = 0; si < 5; ++si) {
      if (f_sh >= 0 && si != f_sh) continue;
      const int* sh = shapes[si];
      std::vector<GRec> late;
      g_blocks(late, 0, kt1, NB_HT1, sh[0], sh[1]);
      while ((int)late.size() <= XCD_SLOTS) {
        std::vector<int> slot_of;
        int crit;
        double span = g_pair(late, free_at, slot_of, crit);
        if (early_end > span) span = early_end;
        if (span < best.span - 1e-9) {
          best.span = span; best.early = early; best.late = late;
          best.early_slot = early_slot; best.late_slot = slot_of;
        }
        GRec& c = late[crit];
        if (c.nk * c.nh == 1) break;
        GRec half = c;
        if (c.nk == 3) { c.nk = 2; half.nk = 1; half.kt0 += 2; }
        else if (c.nk == 2) { c.nk = 1; half.nk = 1; half.kt0 += 1; }
        else { c.nh = 1; half.nh = 1; half.ht0 += 1; }
        late.push_back(half);
      }
    }
  }
  jobs.clear();
  sched.clear();
  if (best.late.empty()) return;   // (the kernel then runs g_jobs_rounds)
  sched.assign(2 * XCD_SLOTS, -1);
  for (size_t i = 0; i < best.early.size(); ++i) {
    const GRec& r = best.early[i];
    const int rec[G_JOB_INTS] = {r.layer, r.kt0, r.nk, r.ht0, r.nh};
    sched[2 * best.early_slot[i]] = (int)jobs.size() / G_JOB_INTS;
    jobs.insert(jobs.end(), rec, rec + G_JOB_INTS);
  }
  for (size_t j = 0; j < best.late.size(); ++j) {
    const GRec& r = best.late[j];
    const int rec[G_JOB_INTS] = {r.layer, r.kt0, r.nk, r.ht0, r.nh};
    sched[2 * best.late_slot[j] + 1] = (int)jobs.size() / G_JOB_INTS;
    jobs.insert(jobs.end(), rec, rec + G_JOB_INTS);
  }
}

// ---- XCD ownership ----------------------------------------------------------
constexpr int XCD_COUNT = 8;
constexpr int MAX_RESIDENT = 16;   // networks of one resident launch
// networks of the XCDs: up to two per XCD (two workgroups per CU), -1 = none
// (the resident kernel takes it by value)
struct XcdMap {
  int n_nets;
  int net[XCD_COUNT][2];
};

// A resident network takes one workgroup slot on every CU of an XCD (of two
// per CU).  Every trainer owns its XCDs exclusively -- two resident kernels
// that each hold a part of an XCD could wait for each other -- and puts
// one network on each while they last, two beyond that (16 networks on the
// 8 XCDs); a trainer that finds too few free XCDs trains with two launches
// per step instead.  in_use: the XCDs of the live resident trainers;
// resident_allowed: no switch asks for two launches and workgroups are dealt
// out over the XCDs as the resident kernel expects.
// owned: the XCDs of `map`, which the caller adds to in_use.
struct XcdPlan { bool two_launch; unsigned owned; XcdMap map; };
XcdPlan plan_xcds(int n_networks, unsigned in_use, bool resident_allowed) {
  int xs[XCD_COUNT], n_free = 0;                 // the free XCDs, lowest first
  for (int x = 0; x < XCD_COUNT; ++x)
    if (!(in_use & (1u << x))) xs[n_free++] = x;
  XcdPlan p;
  p.two_launch = n_networks > MAX_RESIDENT || !resident_allowed ||
                 n_networks > 2 * n_free;
  p.owned = 0;
  p.map.n_nets = n_networks;
  for (int x = 0; x < XCD_COUNT; ++x) p.map.net[x][0] = p.map.net[x][1] = -1;
  if (p.two_launch) return p;
  // as many XCDs as there are networks (up to the free ones), the
  // networks dealt out round-robin
  const int n_use = std::min(n_networks, n_free);
  for (int i = 0; i < n_networks; ++i) p.map.net[xs[i % n_use]][i / n_use] = i;
  for (int j = 0; j < n_use; ++j) p.owned |= 1u << xs[j];
  return p;
}

// ---- layout of the device memory --------------------------------------------
// units of the activations / deltas of the layers 1-4 in the stash (the bias
// unit included, padded to 16)
constexpr int LD1 = 112, LD2 = 64, LD3 = 32, LD4 = 16;
constexpr int SMALL_BATCH = 200;    // largest batch of the compile-time layout
static_assert(SMALL_BATCH <= MAXB, "the stash in the pool holds MAXB rows");
// doubles of a stash of `rows` rows (a multiple of 16), `ld0` input units:
// A0 A1 A2 A3 D1 D2 D3 D4  (constexpr: host and device)
constexpr long long stash_doubles(long long rows, int ld0) {
  return rows * (ld0 + 2 * (LD1 + LD2 + LD3) + LD4);
}

// ONE allocation for everything the kernels touch -- [barrier counters, 12
// KB][network records, 1 KB][job lists, 1 + 2 KB][weights, moments, stash, loss
// curve and scalars of every network] -- so that the small arrays lie the
// same way relative to each other and to the pool in every process (as
// separate allocations they landed wherever the allocator had a slot, and
// the step time followed).  (The includer checks its counters and network
// records against OFF_NETS and OFF_JOBS.)
constexpr size_t OFF_NETS = 12288, OFF_JOBS = 13312, OFF_SCHED = 14336,
                 OFF_POOL = 32768;
// bytes for the job list without a schedule / for [schedule][its job records]
constexpr size_t JOBS_SLOT = OFF_SCHED - OFF_JOBS,
                 SCHED_SLOT = OFF_POOL - OFF_SCHED;
static_assert(OFF_NETS < OFF_JOBS && OFF_JOBS < OFF_SCHED &&
              OFF_SCHED < OFF_POOL, "trainer block layout");

// a network's part of the pool: the offsets of its buffers, as they lie, and
// its size, in doubles (n_w: doubles of the weight tiles)
struct PoolLayout { long long W, M, V, WT, stash, curve, scal, per_net; };
PoolLayout pool_layout(int kt1, long long n_w, int max_iter) {
  PoolLayout p;
  p.W = 0; p.M = n_w; p.V = 2 * n_w; p.WT = 3 * n_w;
  p.stash = p.WT + (long long)net_layer(4, 1, kt1).wt_off;
  p.curve = p.stash + stash_doubles(MAXB, 16 * kt1);
  p.scal = p.curve + ((max_iter + 1) & ~1LL);         // 16-byte alignment
  // (32 scalars; a multiple of 4 KB: no line of one network's record next to
  // another's)
  p.per_net = (p.scal + 32 + 511) / 512 * 512;
  return p;
}

// bytes of the block (whole 2 MB fragments: the mapping of a block that ends
// inside one was seen to cost up to a microsecond per step)
size_t block_bytes(long long per_net, int n_networks) {
  const size_t frag = 2u << 20;
  return (OFF_POOL + (size_t)per_net * n_networks * sizeof(double) + frag - 1) /
         frag * frag;
}

// The stash follows the largest minibatch any network sees (batch clipped to
// its rows, as scikit-learn does): up to SMALL_BATCH rows the stash in the
// pool (G_ROWT row tiles), beyond it one laid out for the batch, with the
// loss partials of its row tiles behind it.
struct StashChoice { bool large; int rowt; };
StashChoice stash_choice(const std::vector<long long>& rows, int batch) {
  long long eff = 0;
  for (long long n : rows) eff = std::max(eff, std::min(n, (long long)batch));
  const bool large = eff > SMALL_BATCH;
  return {large, large ? (int)((eff + 15) / 16) : G_ROWT};
}
// doubles of one network in a large stash of `rowt` row tiles
long long large_per_net(int rowt, int kt1) {
  return (stash_doubles(16LL * rowt, 16 * kt1) + rowt + 511) / 512 * 512;
}

// ---- steps ------------------------------------------------------------------
// the minibatch of a network of n rows and its Adam steps per epoch
struct EpochSteps { int batch, steps; };
EpochSteps epoch_steps(long long n, int batch) {
  const int b = (int)std::min(n, (long long)batch);
  return {b, (int)((n + b - 1) / b)};
}

}  // namespace
