// Dense emulator layers on the matrix cores as ONE operand pipeline per stage
// (used by nb_eval_fast.hip): out[h] = act(sum_k in[k] W[k][h]) for the T
// tiles of 16 points a wavefront holds.
//
// Operand mapping on v_mfma_f64_16x16x4_f64: rows i = output units, cols j =
// the 16 points of the tile, K = input units.  Lane l holds for point (l & 15)
// the inputs 4 ks + (l >> 4), ks = 0, 1, ... (one B operand per k-step).  The
// C/D layout (col = l & 15, row = (l >> 4) + 4 reg) is exactly the B-operand
// layout of the next layer, so activations never leave the registers between
// layers.  Weights are A operands from 16x16 tile-major storage in LDS
// (nb_layout.h): one contiguous 512-byte row of a tile per MFMA, conflict-free
// ds_read_b64.  The bias is row k = K of the weights; the input carries a
// constant 1 there (fl_pad writes it for the next layer).
//
// The hidden sizes (100, 50, 20, 1) leave 4, 2, 4 and 1 units in the last
// 16-wide tile of a layer.  Those run on v_mfma_f64_4x4x4_4b_f64 instead of a
// full tile: four 4x4x4 blocks = the same 4 units for 4 x 4 points, 16 cycles
// instead of 64.  Register layout (measured on gfx950): A lane i + 4 b + 16 k,
// B lane p + 16 k, D lane p + 16 i with p = 4 b + j -- the B operand is the
// one of the 16x16x4 instruction and D is its register 0, so the result is
// directly k-step 4 (HT - 1) of the next layer.  The A operand is gathered
// from the unchanged tile-major weights (fl_read_a: element (kk, hh) of the
// last tile, hh = lane & 3).
//
// Schedule.  A layer is cut into blocks of SPLIT output tiles (fewer live
// accumulators per block, more operand reuse within it); inside a block the
// k-steps are the outer loop and the block's tiles the inner one, so every B
// operand meets all A operands of its k-step and the accumulators are
// independent.  Only the last NGUARD k-steps depend on the runtime input
// count; the others form one basic block.  On top of that:
//  * the A operands of the first k-step of a block are read by the block
//    BEFORE it (during its last k-step), across block and layer boundaries,
//    so the LDS latency is exposed once per stage, not once per block;
//  * ReLU is applied by the consumer (one v_max_f64 per B operand and k-step,
//    hidden behind the MFMAs): a producer applying it at the end of a block
//    would wait for the matrix pipe to drain;
//  * the weight DMA of the next stage is sliced into the k-steps (`tick`):
//    issued in one burst at the start of a stage it stalls the issuing
//    wavefronts on the 64 B/clk fill path of the CU.
// Summation order per output unit: k-steps ascending, one accumulator.
#pragma once
#include "nb_tile.h"

namespace {

constexpr int fl_blk_end(int HT, int H0, int SPLIT) {
  return (HT - 1 - H0 > SPLIT) ? H0 + SPLIT : HT;
}

// output tiles [H0, H1) of a layer with HT tiles (+ its partial last tile if
// H1 == HT): NF full 16-unit tiles, NA operands per k-step
template <int HT, int H0, int H1>
struct FlShape {
  static constexpr int NFL = HT - 1;
  static constexpr bool REM = (H1 == HT);
  static constexpr int NF = (REM ? NFL : H1) - H0;
  static constexpr int NA = NF + (REM ? 1 : 0);
};

template <int HT, int H0, int H1>
__device__ __forceinline__ void fl_read_a(
    const double* w, int ks, int lane, double (&a)[FlShape<HT, H0, H1>::NA]) {
  using S = FlShape<HT, H0, H1>;
  const double* wk = w + (ks >> 2) * HT * NB_TILE + (ks & 3) * 64;
#pragma unroll
  for (int h = 0; h < S::NF; ++h) a[h] = wk[(H0 + h) * NB_TILE + lane];
  // partial tile on v_mfma_f64_4x4x4_4b: element (kk, hh = lane & 3)
  if constexpr (S::REM)
    a[S::NF] = wk[S::NFL * NB_TILE + (lane >> 4) * 16 + (lane & 3)];
}

// One block.  a0 = operands of k-step 0 (reads issued by the caller); `next`
// issues the reads of whatever follows this block, `tick` may issue one DMA
// instruction (called every TICK_P k-steps).  The last NGUARD k-steps depend
// on the runtime count ks_n and are not pipelined.  PD = k-steps the operand
// reads run ahead of the MFMAs (1 where the accumulators need the registers;
// more for the small last layers, whose k-steps are shorter than the LDS
// latency).
template <int T, int KSMAX, int NGUARD, int HT, int H0, int H1, bool RELU_IN,
          int TICK_P, int PD, int NIN, int NOUT, class Next, class Tick>
__device__ __forceinline__ void fl_block(
    const double* w, int ks_n, const double (&in)[T][NIN], int lane,
    double (&out)[T][NOUT], const double (&a0)[FlShape<HT, H0, H1>::NA],
    Next&& next, Tick&& tick) {
  using S = FlShape<HT, H0, H1>;
  constexpr int NF = S::NF, NA = S::NA, NFL = S::NFL;
  constexpr bool REM = S::REM;
  constexpr int KS_U = KSMAX - NGUARD;
  static_assert(KS_U >= 1 && KS_U >= PD && PD >= 1, "prefetch distance");
  constexpr int R = PD + 1;
  nb_d4 acc[T][NF > 0 ? NF : 1];
  double rem[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int h = 0; h < (NF > 0 ? NF : 1); ++h)
      acc[t][h] = nb_d4{0.0, 0.0, 0.0, 0.0};
    rem[t] = 0.0;
  }
  auto step = [&](int ks, const double (&a)[NA]) __attribute__((always_inline)) {
    double b[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
      b[t] = RELU_IN ? fmax(in[t][ks], 0.0) : in[t][ks];
#pragma unroll
    for (int h = 0; h < NF; ++h)
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t][h] = MFMA(a[h], b[t], acc[t][h]);
    if constexpr (REM) {
#pragma unroll
      for (int t = 0; t < T; ++t) rem[t] = MFMA4(a[NF], b[t], rem[t]);
    }
  };
  // a use of the operands: the compiler's s_waitcnt lands here, before the
  // next reads are issued
  auto arrived = [&](const double (&a)[NA]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NA; ++i) asm volatile("" ::"v"(a[i]));
  };
  double a[R][NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) a[0][i] = a0[i];
#pragma unroll
  for (int i = 1; i < PD; ++i) fl_read_a<HT, H0, H1>(w, i, lane, a[i]);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int ks = 0; ks < KS_U; ++ks) {
    arrived(a[ks % R]);
    __builtin_amdgcn_sched_barrier(0);
    if (ks + PD < KS_U)
      fl_read_a<HT, H0, H1>(w, ks + PD, lane, a[(ks + PD) % R]);
    else if (ks + PD == KS_U) next();
    if (ks % TICK_P == 0) tick();
    __builtin_amdgcn_sched_barrier(0);
    step(ks, a[ks % R]);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int ks = KS_U; ks < KSMAX; ++ks) {
    if (ks < ks_n) {
      double ag[NA];
      fl_read_a<HT, H0, H1>(w, ks, lane, ag);
      step(ks, ag);
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int h = 0; h < NF; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[t][4 * (H0 + h) + r] = acc[t][h][r];
    if constexpr (REM) out[t][4 * NFL] = rem[t];
  }
}

// K-chunked form of fl_block for a layer whose weights exceed an LDS region
// (layer 1 for n_dim > 64): k-steps [KS_LO, KS_HI) of all output tiles of the
// layer, `out` carries the pre-activations between the chunks, `w` is the
// chunk in LDS (k-tile index relative to KS_LO / 4).  The runtime-guarded
// k-steps are the last three of the layer.
template <int T, int KSMAX, int HT, int KS_LO, int KS_HI, int TICK_P, int NIN,
          int NOUT, class Tick>
__device__ __forceinline__ void fl_chunk(
    const double* w, int ks_n, const double (&in)[T][NIN], int lane,
    double (&out)[T][NOUT], Tick&& tick) {
  using S = FlShape<HT, 0, HT>;
  constexpr int NF = S::NF, NA = S::NA, NFL = S::NFL;
  static_assert(KS_LO % 4 == 0 && KS_LO < KS_HI && KS_HI <= KSMAX, "chunk");
  constexpr bool FIRST = (KS_LO == 0);
  constexpr int KS_U = (KS_HI < KSMAX - 3) ? KS_HI : KSMAX - 3;
  static_assert(KS_U > KS_LO, "at least one unguarded k-step per chunk");
  nb_d4 acc[T][NF];
  double rem[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int h = 0; h < NF; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc[t][h][r] = FIRST ? 0.0 : out[t][4 * h + r];
    rem[t] = FIRST ? 0.0 : out[t][4 * NFL];
  }
  auto step = [&](int ks, const double (&a)[NA]) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < NF; ++h)
#pragma unroll
      for (int t = 0; t < T; ++t)
        acc[t][h] = MFMA(a[h], in[t][ks], acc[t][h]);
#pragma unroll
    for (int t = 0; t < T; ++t) rem[t] = MFMA4(a[NF], in[t][ks], rem[t]);
  };
  auto arrived = [&](const double (&a)[NA]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NA; ++i) asm volatile("" ::"v"(a[i]));
  };
  double a[2][NA];
  fl_read_a<HT, 0, HT>(w, 0, lane, a[0]);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int ks = KS_LO; ks < KS_U; ++ks) {
    const int i = ks - KS_LO;
    arrived(a[i & 1]);
    __builtin_amdgcn_sched_barrier(0);
    if (ks + 1 < KS_U) fl_read_a<HT, 0, HT>(w, i + 1, lane, a[(i + 1) & 1]);
    if (i % TICK_P == 0) tick();
    __builtin_amdgcn_sched_barrier(0);
    step(ks, a[i & 1]);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int ks = (KS_LO > KS_U ? KS_LO : KS_U); ks < KS_HI; ++ks) {
    if (ks < ks_n) {
      double ag[NA];
      fl_read_a<HT, 0, HT>(w, ks - KS_LO, lane, ag);
      step(ks, ag);
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int h = 0; h < NF; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[t][4 * h + r] = acc[t][h][r];
    out[t][4 * NFL] = rem[t];
  }
}

// a layer = blocks of SPLIT output tiles chained through their first operands
template <int T, int SPLIT, int KSMAX, int NGUARD, int HT, bool RELU_IN,
          int TICK_P, int PD, int H0, int NIN, int NOUT, class Next, class Tick>
__device__ __forceinline__ void fl_layer_from(
    const double* w, int ks_n, const double (&in)[T][NIN], int lane,
    double (&out)[T][NOUT],
    const double (&a0)[FlShape<HT, H0, fl_blk_end(HT, H0, SPLIT)>::NA],
    Next&& next, Tick&& tick) {
  constexpr int H1 = fl_blk_end(HT, H0, SPLIT);
  if constexpr (H1 < HT) {
    constexpr int H2 = fl_blk_end(HT, H1, SPLIT);
    double a1[FlShape<HT, H1, H2>::NA];
    fl_block<T, KSMAX, NGUARD, HT, H0, H1, RELU_IN, TICK_P, PD>(
        w, ks_n, in, lane, out, a0,
        [&]() __attribute__((always_inline)) {
          fl_read_a<HT, H1, H2>(w, 0, lane, a1);
        },
        tick);
    fl_layer_from<T, SPLIT, KSMAX, NGUARD, HT, RELU_IN, TICK_P, PD, H1>(
        w, ks_n, in, lane, out, a1, next, tick);
  } else {
    fl_block<T, KSMAX, NGUARD, HT, H0, HT, RELU_IN, TICK_P, PD>(
        w, ks_n, in, lane, out, a0, next, tick);
  }
}

// operands of the first k-step of a layer (block 0)
template <int SPLIT, int HT>
struct FlFirst {
  static constexpr int H1 = fl_blk_end(HT, 0, SPLIT);
  static constexpr int NA = FlShape<HT, 0, H1>::NA;
};
template <int SPLIT, int HT>
__device__ __forceinline__ void fl_read_first(
    const double* w, int lane, double (&a)[FlFirst<SPLIT, HT>::NA]) {
  fl_read_a<HT, 0, FlFirst<SPLIT, HT>::H1>(w, 0, lane, a);
}

// registers 1..3 of a layer's partial last tile: zero padding, except the
// constant 1 that feeds the next layer's bias row (k-step ONE_KS, lane group
// ONE_LG; it may share the register of the partial tile, 50 = 48 + 2)
template <int T, int HT, int ONE_KS, int ONE_LG, int NOUT>
__device__ __forceinline__ void fl_pad(double (&out)[T][NOUT], int lane) {
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int r = 1; r < 4; ++r) {
      const int idx = 4 * (HT - 1) + r;
      out[t][idx] = (idx == ONE_KS && (lane >> 4) == ONE_LG) ? 1.0 : 0.0;
    }
  if constexpr (ONE_KS >= 0 && ONE_KS == 4 * (HT - 1)) {
    if ((lane >> 4) == ONE_LG) {
#pragma unroll
      for (int t = 0; t < T; ++t) out[t][ONE_KS] = 1.0;
    }
  }
}

}  // namespace
