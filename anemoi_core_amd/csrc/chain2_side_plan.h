// How many workgroups a block-tail launch of gt_chain2.hip gets, and how a side job's panels are shared out among the workgroups behind
// them (anemoi_gt_chain2_side_fwd).  Plain C++17 - no HIP, no pointers, no statics - so it can be checked without a GPU.
#pragma once
#include <stdint.h>

namespace anemoi {

constexpr int kChipCus = 256;  // MI355X: 8 XCDs x 32 CUs; one 512-thread chain workgroup per CU (LDS)

// Workgroups of a tail of n_tiles panels: one per panel up to the chip; beyond, as many as make the rounds even (`even`; max_grid: the
// experiments build's cap on a round)
inline int chain2_grid(int n_tiles, bool even = true, int max_grid = kChipCus) {
  int grid = n_tiles < kChipCus ? n_tiles : kChipCus;
  if (even && n_tiles > kChipCus) {
    const int rounds = (n_tiles + max_grid - 1) / max_grid;
    grid = (n_tiles + rounds - 1) / rounds;
  }
  return grid;
}

struct Chain2SidePlan {
  int host_grid = 0;        // the tail's workgroups
  int riders = 0;           // workgroups behind them: rider i walks panels first + i, first + i + riders, ... < end
  int first = 0, end = 0;
};

// cap = 0: every CU the tail leaves idle; > 0: at most that many riders.  Never more riders than panels.  false: the tail leaves no CU idle
// (or there is no tail to ride on) - nothing is launched.
inline bool plan_chain2_side(int host_tiles, int host_grid, int side_first, int side_panels, int cap, Chain2SidePlan& out) {
  out = Chain2SidePlan{};
  if (host_tiles <= 0 || host_grid <= 0 || host_grid >= kChipCus) return false;
  int riders = kChipCus - host_grid;
  if (cap > 0 && cap < riders) riders = cap;
  if (side_panels < riders) riders = side_panels;
  out.host_grid = host_grid;
  out.riders = riders;
  out.first = side_first;
  out.end = side_first + side_panels;
  return true;
}

}  // namespace anemoi
