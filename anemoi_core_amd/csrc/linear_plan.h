// Which kernel a GEMM of linear.hip runs, on which tile, and how many trailing rows ride on the VALU: the whole decision, as one
// pure host function.  Plain C++17 - no HIP, no pointers, no statics - so it can be asked without a GPU (anemoi_linear_plan in
// include/anemoi_hip.h, ops.linear_plan in Python, tests/test_linear_plan_cpu.py).  linear.hip only launches what plan_gemm returns.
#pragma once
#include <stdint.h>

namespace anemoi {

// the epilogue a kernel is instantiated with (PRE: also store GELU's argument - training)
enum : int { EPI_RES = 1, EPI_GATHER = 2, EPI_GELU = 4, EPI_STATS = 8, EPI_LNFOLD = 16, EPI_PRE = 32 };

// Every environment switch of the dispatch, read once per process (gemm_switches() in linear.hip).  The defaults are the product's.
struct GemmSwitches {
  int big = -1;             // ANEMOI_GEMM_BIG: -1 the cost model decides, 0 never, otherwise every O >= 64
  int big_mi = 5;           // ANEMOI_GEMM_BIG_MI: 5 = 160-row big tiles where they pay, 10 = 320 rows always
  int big_mi5_t320 = 512;   // ANEMOI_GEMM_BIG_MI5_T320: 160-row tiles up to this many 320-row tiles
  bool pp = true;           // ANEMOI_GEMM_PP: ping-pong wave schedule of the 192/256-row ring kernels
  bool splitwave = true;    // ANEMOI_GEMM_SPLITWAVE: 8-wave 64 x 128 tiles for at most one round of tiles
  bool narrow = true;       // ANEMOI_GEMM_NARROW: 160 x 128 tiles for narrow outputs with a long K
  bool narrow64 = false;    // ANEMOI_GEMM_NARROW64 (experiments build only): the same tile on 64-wide stages, 4-deep ring
  int fast_epi = 1;         // ANEMOI_GEMM_FAST_EPI: interior tiles of anemoi_linear_fwd take the fast epilogue
  int lnfold_small_rows = 4096;  // ANEMOI_LNFOLD_SMALL_ROWS: the fold's consumer runs on the 64/192-row kernels below this
  int lnfold_mi5 = 1;       // ANEMOI_LNFOLD_MI5: the consumer's big tile has 160 rows also beyond one round
};

enum class GemmRole : int32_t { Plain = 0, PlainPre = 1, StatsProducer = 2, FoldConsumer = 3, SplitK = 4 };

struct GemmProblem {
  GemmRole role = GemmRole::Plain;
  int n_rows = 0, O = 0, K1 = 0, K2 = 0;
  bool residual = false, gather = false, gelu = false;
  int splits = 1;
  bool f32_atomic = false;
  bool mfma_eligible = false, ring_eligible = false;  // linear.hip: they look at pointers and leading dimensions
};

enum class GemmKernel : int32_t { Generic = 0, Mfma128 = 1, Ring = 2, SplitWave = 3, BigTile = 4 };

struct GemmPlan {
  GemmKernel kernel = GemmKernel::Generic;
  int tile_m = 64, tile_n = 64;
  bool pingpong = false;
  int stage_k = 16;                         // K elements per LDS stage
  int mi = 0, wr = 0, kg = 0, stages = 0;   // split-wave: MI, WR, KG, STAGES; big tile: MI, STAGES; ring: STAGES
  int epi = 0;                              // EPI_* bits of the instantiation (0 on the generic and 128^2 kernels: runtime epilogue)
  int main_rows = 0;                        // rows the tiles cover
  int tail_rows = 0;                        // rows [main_rows, main_rows + tail_rows) are computed on the VALU, a column per wave
  int ln_tail_begin = 0x7fffffff;           // fold consumer on small tiles: rows >= this take their statistics from the row itself
};

// THE tail rule.  A few rows beyond a multiple of the 320-row tile (the icosphere's 10 * 4^r + 2 nodes) are computed on the VALU at
// the end of the same kernel, a column per wave, instead of costing a whole extra round of tiles.  The LayerNorm fold depends on it
// from both sides: the producer writes no strip sums for exactly these rows, the consumer takes exactly their statistics from the rows.
inline int peeled_tail_rows(int n_rows) {
  const int rem = n_rows % 320;
  return rem > 0 && rem <= 32 && n_rows > 320 ? rem : 0;
}
// The narrow 160 x 128 kernel without statistics peels by its own tile height.  (With statistics it must follow peeled_tail_rows: a
// remainder of 161..192 mod 320 goes through a ragged last tile, which writes the strip sums of every valid row.)
inline int peeled_tail_rows_160(int n_rows) {
  const int rem = n_rows % 160;
  return rem > 0 && rem <= 32 && n_rows > 160 ? rem : 0;
}

// Estimated duration [us] of one launch on 256 CUs.  Both terms are measured rates: the K-loop moves (TBM + TBN) * 128 B
// of operands per K-step at the ~44 GB/s per CU the LDS-DMA path sustains next to running MFMAs, the epilogue writes
// TBM * TBN outputs at ~0.09 ns each; every round of tiles pays both.
inline double tile_cost_us(int tbm, int tbn, int rows, int O, int nk) {
  const int64_t tiles = (int64_t)((rows + tbm - 1) / tbm) * ((O + tbn - 1) / tbn);
  const double rounds = (double)((tiles + 255) / 256);
  return rounds * (nk * (tbm + tbn) * 2.9e-3 + (double)tbm * tbn * 0.09e-3);
}

namespace plan_detail {

inline int64_t tiles(int rows, int tm, int O, int tn) { return (int64_t)((rows + tm - 1) / tm) * ((O + tn - 1) / tn); }
inline double ring_cost_us(const GemmProblem& p, int tile_m) { return tile_cost_us(tile_m, 128, p.n_rows, p.O, (p.K1 + p.K2) / 64); }

inline GemmPlan on(GemmPlan g, GemmKernel kernel, int tile_m, int tile_n, int stage_k, int stages, int mi = 0, int wr = 0, int kg = 0) {
  g.kernel = kernel, g.tile_m = tile_m, g.tile_n = tile_n, g.stage_k = stage_k, g.stages = stages, g.mi = mi, g.wr = wr, g.kg = kg;
  return g;
}
inline GemmPlan ring(GemmPlan g, int tile_m, bool pingpong) {
  g.pingpong = pingpong;
  return on(g, GemmKernel::Ring, tile_m, 128, 64, 3);
}
inline GemmPlan splitwave(GemmPlan g, int mi, int wr, int kg, int stages, int stage_k) {
  return on(g, GemmKernel::SplitWave, 16 * mi * wr, 128, stage_k, stages, mi, wr, kg);
}
inline GemmPlan bigtile(GemmPlan g, int mi, int tail) {  // the tail rows ride on the VALU at the end of the same kernel
  g.main_rows -= tail, g.tail_rows = tail;
  return on(g, GemmKernel::BigTile, 32 * mi, 256, 64, 2, mi);
}

// the K split over wave groups needs one unsplit K of whole 128-wide stages and a plain store
inline bool one_k_of_128(const GemmProblem& p) { return p.K2 == 0 && p.K1 % 128 == 0 && p.splits == 1 && !p.f32_atomic; }

// Narrow outputs with a long K in ONE round of 160 x 128 tiles (MLP-2 of the hidden mesh: [10242 x 2048] -> 512 = 64 x 4 tiles + 2
// tail rows): 128-wide K stages, K split over two wave groups (linear_mfma_splitwave_kernel<.., 5, 2, 2, 2>).  Measured on
// MI355X: 33.3 us against 34.5 on the 192 x 128 ring kernel; at K = 512 (projection) it is 1.2 us SLOWER, hence K >= 1024.
inline bool narrow_fits(const GemmProblem& p, const GemmSwitches& s, int main_rows) {
  const int64_t t160 = tiles(main_rows, 160, p.O, 128);
  return s.narrow && t160 > 128 && t160 <= 256 && p.K1 >= 1024 && one_k_of_128(p);
}
inline GemmPlan narrow(GemmPlan g, const GemmSwitches& s, int tail) {
  g.main_rows -= tail, g.tail_rows = tail;
  return s.narrow64 ? splitwave(g, 5, 2, 2, 4, 64) : splitwave(g, 5, 2, 2, 2, 128);
}

// Few tiles (small M, e.g. one rank's rows of a sharded mesh): 64 x 128 tiles on more CUs; the K-loop of a lone tile is bound by
// the ~40 cycles a CU needs per 1-KiB LDS-DMA piece, i.e. by the tile's operand bytes, like the model says.  At most one round of
// them: every tile gets 8 waves (K split over wave groups) instead of 2 (also with the row-statistics epilogue: the projection of
// a sharded mesh's block).
inline bool small_tiles_pay(const GemmProblem& p, double c3, double c4) { return ring_cost_us(p, 64) < 0.9 * (c3 < c4 ? c3 : c4); }
inline GemmPlan small_tiles(GemmPlan g, const GemmProblem& p, bool eight_waves) {
  if (eight_waves && tiles(p.n_rows, 64, p.O, 128) <= 256 && one_k_of_128(p)) return splitwave(g, 4, 1, 4, 3, 128);
  return ring(g, 64, false);
}

// The DMA-ring family for one epilogue: big tile, narrow, small tiles, or the 192 / 256-row ring kernel.
inline GemmPlan ring_family(GemmPlan g, const GemmProblem& p, const GemmSwitches& s) {
  const double c3 = ring_cost_us(p, 192), c4 = ring_cost_us(p, 256);
  const int tail = peeled_tail_rows(p.n_rows), main_rows = p.n_rows - tail;
  const double cb = tile_cost_us(320, 256, main_rows, p.O, (p.K1 + p.K2) / 64) + (tail ? 0.5 : 0.0);
  if (s.big >= 0 ? (s.big != 0 && p.O >= 64) : cb < 0.95 * (c3 < c4 ? c3 : c4)) {
    // Up to one round of 320 x 256 tiles: every CU ends its only tile at the same moment and the whole output (42 MB at
    // [10242 x 512] -> 2048) is written behind the last K-step: ~8 us at the ~5 TB/s HBM takes writes, with nothing to overlap
    // (tools/gemm_phase_timing.py).  160 x 256 tiles instead: two per CU, the first tile's output drains under the second
    // tile's K-loop, whose rate is set by the MFMAs (power-limited clock: 1.9 us per 320-row K-step on random data against
    // 0.7 us for its DMA, tools/dma_rate_probe.hip), not by the 44 % extra operand bytes.
    // ... and up to two rounds of them (GraphConv's [81840 x 512] -> 512 edge GEMMs: 8.66 -> 8.36 ms per GNN forward); beyond
    // that the drain is hidden anyway and the 320-row tile's lower operand traffic wins (N320: 15.5 against 15.85 ms)
    const bool half = s.big_mi == 5 && tiles(main_rows, 320, p.O, 256) <= s.big_mi5_t320;
    return bigtile(g, half ? 5 : 10, tail);
  }
  if ((g.epi & (EPI_STATS | EPI_LNFOLD | EPI_PRE)) == 0) {
    const int tail160 = peeled_tail_rows_160(p.n_rows);
    if (narrow_fits(p, s, p.n_rows - tail160)) return narrow(g, s, tail160);
  }
  if (small_tiles_pay(p, c3, c4)) return small_tiles(g, p, s.splitwave);
  return ring(g, c3 < c4 ? 192 : 256, s.pp);
}

// y = act(LN(x) W^T + b) from the producer's strip sums
inline GemmPlan fold_consumer(GemmPlan g, const GemmProblem& p, const GemmSwitches& s) {
  const int tail = peeled_tail_rows(p.n_rows);
  // few rows (one rank's share of a sharded mesh, small meshes): a round of big tiles leaves most of the chip idle (642 rows =
  // 3 x 8 tiles on 256 CUs) - the 64 x 128 kernels take the fold through their epilogue, statistics read from L1
  if (p.n_rows < s.lnfold_small_rows) {
    if (tail) g.ln_tail_begin = p.n_rows - tail;
    if (small_tiles_pay(p, ring_cost_us(p, 192), ring_cost_us(p, 256))) return small_tiles(g, p, true);
    // in between (a few thousand rows: the res-4 mesh, 2 562): the 192 x 128 kernel of the plain GEMM of the shape, lock-step
    // schedule (the ping-pong one spills 80 registers with the fold)
    return ring(g, 192, false);
  }
  // 160-row tiles also beyond one round (40 320-row mapper GEMMs): the fold's epilogue has no registers to spare at 160
  // accumulators per lane (MI = 10: +7 us on [40320 x 512] -> 1024), at 80 it is free; ANEMOI_LNFOLD_MI5=0 restores the rule
  const int main_rows = p.n_rows - tail;
  const bool half = (tiles(main_rows, 320, p.O, 256) <= 256 || s.lnfold_mi5) && main_rows % 160 == 0;  // two 160 x 256 tiles per CU
  return bigtile(g, half ? 5 : 10, tail);
}

}  // namespace plan_detail

inline GemmPlan plan_gemm(const GemmProblem& p, const GemmSwitches& s) {
  using namespace plan_detail;
  GemmPlan g;
  g.main_rows = p.n_rows;
  const int act = p.gelu ? EPI_GELU : 0;
  switch (p.role) {
    case GemmRole::SplitK:  // 64 x 128 tiles (many tiles from a small output), lock-step schedule, plain epilogue
      return ring(g, 64, false);
    case GemmRole::FoldConsumer:
      g.epi = EPI_LNFOLD | act;
      return fold_consumer(g, p, s);
    case GemmRole::StatsProducer: {
      // y = x W^T + b + residual, plus the row statistics of y for the LayerNorm the next GEMM folds in; without a residual: the
      // embedding in front of a mapper's LayerNorm.  Tail rows carry no strip sums, so they are peeled by THE tail rule only.
      g.epi = (p.residual ? EPI_RES : 0) | EPI_STATS;
      const int tail = peeled_tail_rows(p.n_rows);
      if (narrow_fits(p, s, p.n_rows - tail)) return narrow(g, s, tail);
      return ring_family(g, p, s);  // the kernel choice of the same shape without statistics (big tiles at 40 320 rows)
    }
    case GemmRole::Plain:
    case GemmRole::PlainPre:
      break;
  }
  if (!p.mfma_eligible) return g;  // any dtype / any K, O: 64 x 64 tiles on the VALU
  if (!p.ring_eligible) {
    g.kernel = GemmKernel::Mfma128;
    g.tile_m = g.tile_n = 128, g.stage_k = 64, g.stages = 2;
    return g;
  }
  g.epi = (p.residual ? EPI_RES : 0) | (p.gather ? EPI_GATHER : 0) | act | (p.role == GemmRole::PlainPre ? EPI_PRE : 0);
  return ring_family(g, p, s);
}

}  // namespace anemoi
