// Which kernel a chain entry point runs (gt_chain2.hip, gt_chain2_side.hip, gt_rowchain.hip, gt_cluster_chain.hip, gt_embed_fold.hip,
// gnn_chain.hip), on how many rows per panel, on how many workgroups, with how much LDS - and which shapes it takes at all: the whole
// decision, as one pure host function.  Plain C++17 - no HIP, no pointers, no statics - so it can be asked without a GPU
// (anemoi_chain_plan in include/anemoi_hip.h, ops.chain_plan in Python, tests/test_chain_plan_cpu.py).  The .hip files only launch
// what plan_chain returns; Python keeps no copy of this geometry.
#pragma once
#include <stdint.h>

#include "anemoi_hip.h"

namespace anemoi {

// ---------------------------------------------------------------------------------------------------------------- the one set of constants
constexpr int kXcds = 8, kCusPerXcd = 32;
constexpr int kChipCus = kXcds * kCusPerXcd;  // MI355X: 256 CUs; one 512-thread chain workgroup per CU (LDS)
constexpr int kCh = 512;                      // channels of the residual stream (8 waves x 64 columns)
constexpr int kPanel = 48;                    // panel rows (3 MFMA row bands)
constexpr int kGnnEdgeRows = 64;              // the GraphConv edge / MLP chain's cap on a panel (4 row bands); the node chain's is kPanel
constexpr int kClusterSize = 4;               // CUs of one XCD that share a panel of the cluster chain
constexpr int kVecMaxElems = 6144;            // chain2: 12 KiB of per-column vectors in LDS: 512 + hidden + 512 + q_out <= 6144
constexpr int kVecMaxElemsTl = 5120;          // its instrumented instantiation gives 2 KiB of that region to its stamps
constexpr int kRowChainMaxQ = 4 * kCh;        // widest projection of the row chain and of the cluster chain
constexpr int kRowChainPipeMaxIn = 256;       // the pipelined row chain parks the next panel's rows in 6 registers per lane
constexpr int kEfRows = 80, kEfThreads = 256; // embed fold: rows per workgroup, threads
constexpr int kEfMaxIn = 256, kEfMaxQ = 2048; // its widest input row and projection

// LDS of the 512-thread chain kernels: three [48 x 512] 16-bit panels, the row-statistics partials of `waves` waves, then the vectors
constexpr int kRowBytes = kCh * 2;
constexpr int kBufBytes = kPanel * kRowBytes;
constexpr int kRedOff = 3 * kBufBytes;
constexpr int vec_off(int waves) { return kRedOff + kPanel * waves * 2 * 4; }
constexpr int kChainSmem = vec_off(8);  // (no vectors in LDS: the GraphConv node chain keeps its in registers)
constexpr int kChain2Lds = vec_off(4) + kVecMaxElems * 2;
constexpr int kChain2TlLds = vec_off(4) + kVecMaxElemsTl * 2 + 8 * 48 * 8;  // + [8 waves][48 slots] stamps
constexpr int kRowChainLds = vec_off(8) + (kCh + kRowChainMaxQ) * 2;
constexpr int kRowChainPipeLds = vec_off(4) + (kCh + kRowChainMaxQ) * 2;
constexpr int max_of(int a, int b) { return a > b ? a : b; }
constexpr int kChain2SideLds = max_of(kChain2Lds, max_of(kRowChainLds, kRowChainPipeLds));  // the tail's LDS or the riders', whichever is larger
constexpr int kClusterLds = vec_off(8) + (2 * kCh + 4 * kCh + kRowChainMaxQ) * 2;
constexpr int kGnnEdgeLds = 2 * kGnnEdgeRows * kRowBytes + kGnnEdgeRows * 8 * 2 * 4;
constexpr int ef_lds(int qc) { return kEfRows * 512 + kEfRows * 4 * 2 * 4 + 4 * 16 * 256 + (kCh + 3 * kCh * qc) * 4; }
// (each kernel's own header static_asserts that its layout is the one priced here)

// ---------------------------------------------------------------------------------------------------------------- switches, problem, plan
// Every environment switch that bears on launch geometry, read once per process (chain_switches() in chain_host.h).  The defaults are
// the product's.  The two readers of ANEMOI_CHAIN_ROWS clamp differently, and both clamps are kept: the block tails ignore a value
// above kPanel, the GraphConv chains lower it to their cap.
struct ChainSwitches {
  int chain_rows = 0;        // ANEMOI_CHAIN_ROWS (0 .. 64; 0: the rules below)
  int gnn_node_rows = 0;     // ANEMOI_GNN_NODE_ROWS (experiments build; 0 .. kPanel): rows per panel of the node chain alone
  bool even_grid = true;     // ANEMOI_CHAIN2_EVEN_GRID (experiments build)
  int max_grid = kChipCus;   // ANEMOI_CHAIN2_MAX_GRID (experiments build; 8 .. kChipCus): fewer CUs per round
  bool timeline_built = false;  // the experiments build carries the instrumented instantiations
};

enum class ChainKind : int32_t { BlockTail = 0, BlockTailSide, ClusterTail, RowChain, RowChainPanels, EmbedFold, GnnEdge, GnnMlp, GnnNode };
enum class ChainKernel : int32_t {
  None = 0,        // nothing to launch
  Chain2Full,      // gt_chain2_kernel<T>: every CU busy
  Chain2Part,      // gt_chain2_kernel<T, false, true>: fewer workgroups than CUs
  Chain2TlFull,    // the instrumented instantiations of the two
  Chain2TlPart,
  Chain2Side,      // gt_chain2_kernel<T, false, true, true>: a tail with riders (gt_chain2_side.hip)
  Cluster,
  RowChainSingle,  // gt_rowchain_kernel: the single-panel schedule
  RowChainPipe,    // gt_rowchain_pipe_kernel: the two wave groups on different panels
  EmbedFold,
  GnnEdge,
  GnnMlp,
  GnnNode,
};
// the instantiation as the host code names it, its dtype argument dropped
constexpr const char* chain_kernel_name(ChainKernel k) {
  switch (k) {
    case ChainKernel::None: return "none";
    case ChainKernel::Chain2Full: return "gt_chain2_kernel";
    case ChainKernel::Chain2Part: return "gt_chain2_kernel<false,true>";
    case ChainKernel::Chain2TlFull: return "gt_chain2_kernel<true>";
    case ChainKernel::Chain2TlPart: return "gt_chain2_kernel<true,true>";
    case ChainKernel::Chain2Side: return "gt_chain2_kernel<false,true,true>";
    case ChainKernel::Cluster: return "gt_cluster_chain_kernel";
    case ChainKernel::RowChainSingle: return "gt_rowchain_kernel";
    case ChainKernel::RowChainPipe: return "gt_rowchain_pipe_kernel";
    case ChainKernel::EmbedFold: return "gt_embed_fold_kernel";
    case ChainKernel::GnnEdge: return "gnn_edge_chain_kernel";
    case ChainKernel::GnnMlp: return "gnn_edge_chain_kernel<true>";
    case ChainKernel::GnnNode: return "gnn_node_chain_kernel";
  }
  return "?";
}

struct ChainProblem {
  ChainKind kind = ChainKind::BlockTail;
  int n_rows = 0;
  int in_features = 0;     // row chain, embed fold, GraphConv MLP
  int hidden = 0;          // block and cluster tails
  int q_out_features = 0;
  int rows_per_tile = 0;   // the caller's panel rows (0: the library's)
  anemoi_dtype_t dtype = ANEMOI_BF16;
  bool timeline = false;   // a timeline buffer is given
  int first_panel = 0, panels = 0;  // RowChainPanels: the range; BlockTailSide: the side job's panels that ride
  // BlockTailSide: the side job (a row chain) and the cap on its riders (0: every idle CU)
  int side_rows = 0, side_in_features = 0, side_q_out_features = 0, side_rows_per_tile = 0, side_cap = 0;
};

struct ChainPlan {
  int status = ANEMOI_OK;  // ANEMOI_OK, ANEMOI_E_UNSUPPORTED or ANEMOI_E_INVALID: what the entry point returns for the shape
  const char* why = "";    // the rule that refused it
  ChainKernel kernel = ChainKernel::None;
  int rows_per_panel = 0, panels = 0;
  int grid = 0, threads = 0, lds_bytes = 0;
  int rounds = 0;          // panels of the busiest workgroup
  int idle_cus = 0;        // CUs without a workgroup in every round
  // BlockTailSide: riders behind host_grid tail workgroups; rider i walks panels first + i, first + i + riders, ... < end of the side job
  int host_grid = 0, riders = 0, first = 0, end = 0;
  bool side_pipelined = false;
  // RowChain / RowChainPanels: the job's panels, the schedule the WHOLE job has, and the rows the launch covers (a range: the job shifted
  // to its first row)
  int job_panels = 0;
  bool pipelined = false;
  int64_t row_begin = 0;
  int n_rows = 0;
};

// ---------------------------------------------------------------------------------------------------------------- the rules
constexpr int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// Workgroups of a launch over n_tiles panels: one per panel up to the chip; beyond, as many as make the rounds even (854 panels: 4 rounds
// of 214 instead of 3 of 256 + 86) - the CUs of an XCD share that L2's bandwidth, so a round of 27 CUs per XCD is faster than one of 32.
// even = false: always the chip; max_grid: the experiments build's cap on a round.
constexpr int even_rounds_grid(int n_tiles, bool even = true, int max_grid = kChipCus) {
  if (n_tiles <= kChipCus) return n_tiles;
  return even ? ceil_div(n_tiles, ceil_div(n_tiles, max_grid)) : kChipCus;
}

// Which schedule a row-chain job of n_tiles panels runs: several rounds and a narrow input -> pipelined.  The two schedules round
// differently (statistics merged from four or eight partials, the embedding's bias first or last): whoever computes a PART of a job - the
// riders of a block tail, the launch of the panels no tail hosted - takes the schedule of the whole job, so that a panel's bits do not
// depend on where it ran.
constexpr bool rowchain_pipelined(int n_tiles, int in_features) {
  return n_tiles > even_rounds_grid(n_tiles) && in_features <= kRowChainPipeMaxIn;
}

// Rows per panel of the GraphConv chains: whole rounds of panels over the chip, the panels as even as the cap allows.
// tests/chain_refs.py panel_split restates this; tests/test_chain_plan_cpu.py holds the two together.
constexpr int gnn_rows_per_tile(int n_rows, int cap, int forced) {
  if (forced > 0) return forced < cap ? forced : cap;
  const int64_t rounds = ((int64_t)n_rows + kChipCus * cap - 1) / (kChipCus * cap);
  const int64_t r = ((int64_t)n_rows + kChipCus * rounds - 1) / (kChipCus * rounds);
  return (int)(r < 1 ? 1 : (r > cap ? cap : r));
}

// Rows per panel of the block tails: always the TALLEST panels (48 rows), i.e. the fewest CUs - every busy CU streams the whole layer's
// weights whatever its panel's height, and the CUs of an XCD share that L2's bandwidth: 10 242 rows as 214 panels of 48 instead of 250
// of 41 is 4 % of the O96 forward; multi-round launches even out the ROUNDS instead, not the panel heights
// (profiles/r05_chain2_touch_coverage.txt).  ANEMOI_CHAIN_ROWS=n forces n rows (<= 48).
constexpr int tail_rows_per_tile(const ChainSwitches& sw) { return sw.chain_rows > 0 && sw.chain_rows <= kPanel ? sw.chain_rows : kPanel; }

inline ChainPlan refuse(int status, const char* why) {
  ChainPlan p;
  p.status = status;
  p.why = why;
  return p;
}
inline void set_panels(ChainPlan& p, int n_rows, int rows_per_panel, int grid) {
  p.n_rows = n_rows;
  p.rows_per_panel = rows_per_panel;
  p.panels = ceil_div(n_rows, rows_per_panel);
  p.grid = grid < 0 ? (p.panels < kChipCus ? p.panels : kChipCus) : grid;
  p.rounds = ceil_div(p.panels, p.grid);
  p.idle_cus = p.grid < kChipCus ? kChipCus - p.grid : 0;
}

// The checks come in the order the entry points made them, so that a shape with two faults gets the code it always got.  An empty plan
// (status OK, kernel None): nothing to do.
inline ChainPlan plan_chain(const ChainProblem& q, const ChainSwitches& sw) {
  const bool bits16 = q.dtype == ANEMOI_BF16 || q.dtype == ANEMOI_F16;
  ChainPlan p;
  p.threads = 512;
  switch (q.kind) {
    case ChainKind::BlockTail: {
      if (!bits16) return refuse(ANEMOI_E_INVALID, "16-bit model dtypes only");
      if (q.n_rows < 0) return refuse(ANEMOI_E_INVALID, "n_rows must not be negative");
      if (q.n_rows == 0) return ChainPlan{};
      const bool narrow = q.q_out_features > 0 && q.q_out_features < kCh;  // a narrow trailing projection: 128, 256 or 384 columns
      if (!(q.hidden > 0 && q.hidden % kCh == 0 && q.q_out_features >= 0 && q.q_out_features % (narrow ? 128 : kCh) == 0))
        return refuse(ANEMOI_E_INVALID, "hidden must be a multiple of 512, q_out_features a multiple of 512 (or 128, 256, 384)");
      if (2 * kCh + q.hidden + q.q_out_features > (q.timeline ? kVecMaxElemsTl : kVecMaxElems))
        return refuse(ANEMOI_E_UNSUPPORTED, "the per-column vectors must fit their LDS region");
      if (q.timeline && !sw.timeline_built)
        return refuse(ANEMOI_E_UNSUPPORTED, "the in-kernel timeline is part of the experiments build only (python -m anemoi_core_amd.build --experiments)");
      const int rpt = q.rows_per_tile > 0 ? q.rows_per_tile : tail_rows_per_tile(sw);
      if (rpt > kPanel) return refuse(ANEMOI_E_INVALID, "rows_per_tile exceeds the 48-row panel");
      set_panels(p, q.n_rows, rpt, even_rounds_grid(ceil_div(q.n_rows, rpt), sw.even_grid, sw.max_grid));
      const bool part = p.grid < kChipCus;
      p.kernel = q.timeline ? (part ? ChainKernel::Chain2TlPart : ChainKernel::Chain2TlFull) : (part ? ChainKernel::Chain2Part : ChainKernel::Chain2Full);
      p.lds_bytes = q.timeline ? kChain2TlLds : kChain2Lds;
      return p;
    }
    case ChainKind::BlockTailSide: {
      ChainProblem host = q;
      host.kind = ChainKind::BlockTail;
      const ChainPlan tail = plan_chain(host, sw);
      if (tail.status != ANEMOI_OK) return tail;
      if (q.timeline) return refuse(ANEMOI_E_INVALID, "no in-kernel timeline beside a side job");
      if (q.first_panel < 0 || q.panels < 0 || q.side_cap < 0) return refuse(ANEMOI_E_INVALID, "side_first_panel, side_panels and side_blocks must not be negative");
      // (the side job's own preconditions: a job the row chain cannot take is the caller's to launch some other way)
      ChainProblem job;
      job.kind = ChainKind::RowChain;
      job.n_rows = q.side_rows, job.in_features = q.side_in_features, job.q_out_features = q.side_q_out_features;
      job.rows_per_tile = q.side_rows_per_tile, job.dtype = q.dtype;
      const ChainPlan side = plan_chain(job, sw);
      if (side.status != ANEMOI_OK) return refuse(ANEMOI_E_UNSUPPORTED, side.why);
      if ((int64_t)q.first_panel + q.panels > side.panels) return refuse(ANEMOI_E_INVALID, "the panel range reaches beyond the side job");
      if (tail.grid == 0 || tail.grid >= kChipCus) return refuse(ANEMOI_E_UNSUPPORTED, "the tail leaves no compute unit idle (launch the two pieces separately)");
      // cap = 0: every CU the tail leaves idle; > 0: at most that many riders.  Never more riders than panels; none: the tail alone.
      int riders = kChipCus - tail.grid;
      if (q.side_cap > 0 && q.side_cap < riders) riders = q.side_cap;
      if (q.panels < riders) riders = q.panels;
      p = tail;
      p.host_grid = tail.grid;
      if (riders == 0) return p;
      p.kernel = ChainKernel::Chain2Side;
      p.lds_bytes = kChain2SideLds;
      p.riders = riders;
      p.grid = tail.grid + riders;
      p.first = q.first_panel;
      p.end = q.first_panel + q.panels;
      p.job_panels = side.panels;
      p.side_pipelined = side.pipelined;
      return p;
    }
    case ChainKind::ClusterTail: {
      if (!bits16) return refuse(ANEMOI_E_INVALID, "16-bit model dtypes only");
      if (q.n_rows < 0) return refuse(ANEMOI_E_INVALID, "n_rows must not be negative");
      if (q.n_rows == 0) return ChainPlan{};
      if (q.hidden != kClusterSize * kCh) return refuse(ANEMOI_E_UNSUPPORTED, "the cluster of four splits a hidden width of 2048");
      if (!(q.q_out_features >= 0 && q.q_out_features % kCh == 0 && q.q_out_features <= kRowChainMaxQ))
        return refuse(ANEMOI_E_INVALID, "q_out_features must be a multiple of 512 up to 2048");
      // clusters per XCD, at most 8: 8 clusters x 4 members = the XCD's 32 CUs
      const int per_xcd = ceil_div(ceil_div(q.n_rows, kPanel), kXcds);
      set_panels(p, q.n_rows, kPanel, (per_xcd < kCusPerXcd / kClusterSize ? per_xcd : kCusPerXcd / kClusterSize) * kClusterSize * kXcds);
      p.rounds = ceil_div(p.panels, p.grid / kClusterSize);
      p.kernel = ChainKernel::Cluster;
      p.lds_bytes = kClusterLds;
      return p;
    }
    case ChainKind::RowChain:
    case ChainKind::RowChainPanels: {
      if (!bits16) return refuse(ANEMOI_E_INVALID, "16-bit model dtypes only");
      if (q.n_rows < 0) return refuse(ANEMOI_E_INVALID, "n_rows must not be negative");
      const bool range = q.kind == ChainKind::RowChainPanels;
      int job_panels = 0;
      int rpt = kPanel;
      if (q.n_rows > 0) {
        if (!(q.in_features > 0 && q.in_features <= kCh && q.in_features % 8 == 0))
          return refuse(ANEMOI_E_INVALID, "in_features must be a multiple of 8 up to 512 (rows move as 16-byte pieces)");
        if (!(q.q_out_features > 0 && q.q_out_features % kCh == 0 && q.q_out_features <= kRowChainMaxQ))
          return refuse(ANEMOI_E_INVALID, "q_out_features must be a multiple of 512 up to 2048");
        if (q.rows_per_tile > 0) rpt = q.rows_per_tile;
        if (rpt > kPanel) return refuse(ANEMOI_E_INVALID, "rows_per_tile exceeds the 48-row panel");
        job_panels = ceil_div(q.n_rows, rpt);
      }
      if (range && !(q.first_panel >= 0 && q.panels >= 0 && (int64_t)q.first_panel + q.panels <= job_panels))
        return refuse(ANEMOI_E_INVALID, "the panel range reaches beyond the job");
      const int panels = range ? q.panels : job_panels;
      if (panels == 0) return ChainPlan{};
      p.row_begin = range ? (int64_t)q.first_panel * rpt : 0;
      const int64_t row_end = range ? p.row_begin + (int64_t)panels * rpt : q.n_rows;
      set_panels(p, (int)((row_end < q.n_rows ? row_end : (int64_t)q.n_rows) - p.row_begin), rpt, even_rounds_grid(panels));
      p.panels = panels;
      p.job_panels = job_panels;
      p.pipelined = rowchain_pipelined(job_panels, q.in_features);
      p.kernel = p.pipelined ? ChainKernel::RowChainPipe : ChainKernel::RowChainSingle;
      p.lds_bytes = p.pipelined ? kRowChainPipeLds : kRowChainLds;
      return p;
    }
    case ChainKind::EmbedFold: {
      if (!(q.n_rows >= 0 && q.in_features > 0 && q.q_out_features > 0)) return refuse(ANEMOI_E_INVALID, "n_rows, in_features or q_out_features out of range");
      if (!bits16 || q.in_features > kEfMaxIn || q.in_features % 8 != 0 || q.q_out_features % kCh != 0 || q.q_out_features > kEfMaxQ)
        return refuse(ANEMOI_E_UNSUPPORTED, "not eligible (16-bit dtypes, 512 channels, in_features a multiple of 8 up to 256, q_out_features a multiple of 512 up to 2048)");
      if (q.n_rows == 0) return ChainPlan{};
      set_panels(p, q.n_rows, kEfRows, ceil_div(q.n_rows, kEfRows));
      p.idle_cus = 0;  // (two workgroups per CU: not a one-per-CU launch)
      p.threads = kEfThreads;
      p.kernel = ChainKernel::EmbedFold;
      p.lds_bytes = ef_lds(q.q_out_features / kCh);
      return p;
    }
    case ChainKind::GnnEdge:
    case ChainKind::GnnMlp:
    case ChainKind::GnnNode: {
      if (!bits16) return refuse(ANEMOI_E_INVALID, "16-bit model dtypes only");
      if (q.n_rows < 0) return refuse(ANEMOI_E_INVALID, "n_rows must not be negative");
      if (q.kind == ChainKind::GnnMlp && !(q.in_features >= 128 && q.in_features <= kCh && q.in_features % 128 == 0))
        return refuse(ANEMOI_E_INVALID, "in_features is the zero-padded width: 128, 256, 384 or 512");
      if (q.n_rows == 0) return ChainPlan{};
      const bool node = q.kind == ChainKind::GnnNode;
      int rpt = gnn_rows_per_tile(q.n_rows, node ? kPanel : kGnnEdgeRows, sw.chain_rows);
      if (node && sw.gnn_node_rows > 0) rpt = sw.gnn_node_rows;
      set_panels(p, q.n_rows, rpt, -1);
      p.kernel = node ? ChainKernel::GnnNode : q.kind == ChainKind::GnnMlp ? ChainKernel::GnnMlp : ChainKernel::GnnEdge;
      p.lds_bytes = node ? kChainSmem : kGnnEdgeLds;
      return p;
    }
  }
  return refuse(ANEMOI_E_INVALID, "unknown kind");
}

}  // namespace anemoi
