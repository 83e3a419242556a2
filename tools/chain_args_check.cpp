// Host-only check of the chain entry points' argument validation and launches (all but anemoi_gt_chain2_side_fwd, whose translation unit
// has tools/chain2_side_args_check.cpp): csrc/gt_chain2.hip, gt_rowchain.hip, gt_cluster_chain.hip, gt_embed_fold.hip and gnn_chain.hip compiled
// for the HOST with their kernel launches replaced by a recorder, driven over valid and invalid argument blocks.  Every recorded launch must
// be what plan_chain (csrc/chain_plan.h) says for the shape.  Nothing is launched; no GPU needed.
//
//   hipcc --cuda-host-only -x hip -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         -I include -I anemoi_core_amd/csrc tools/chain_args_check.cpp -o /tmp/chain_args_check && /tmp/chain_args_check
//
// With --record it prints one JSON row per call instead (the call, the return code, the recorded launch): the rows of
// tests/golden/chain_plan_recorded.json were printed that way by the entry points as they stood BEFORE plan_chain existed.
#include "chain_check_common.h"

#include "chain2_core.h"
#include "gnn_chain_args.h"
#include "rowchain_core.h"
namespace anemoi {
struct Chain2Args;
struct ClusterArgs;
struct EmbedFoldArgs;
struct NodeChainArgs;
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const Chain2Args& a);
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const RowChainArgs& a);
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const ClusterArgs& a);
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const EmbedFoldArgs& a);
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const EdgeChainArgs& a);
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const NodeChainArgs& a);
}  // namespace anemoi

#include "gt_chain2.hip"
#include "gt_rowchain.hip"
#include "gt_cluster_chain.hip"
#include "gt_embed_fold.hip"
#include "gnn_chain.hip"

namespace anemoi {
template <typename A>
static Record& push(const char* kernel, dim3 grid, dim3 block, int smem, const A& a) {
  Record r;
  r.kernel = kernel_name(kernel);
  r.grid = (int)grid.x; r.block = (int)block.x; r.smem = smem; r.n_rows = a.n_rows;
  g_launches.push_back(r);
  return g_launches.back();
}
template <typename A>
static void push_tiled(const char* kernel, dim3 grid, dim3 block, int smem, const A& a) {
  Record& r = push(kernel, grid, block, smem, a);
  r.rows_per_tile = a.rows_per_tile; r.n_tiles = a.n_tiles;
}
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const Chain2Args& a) { push_tiled(kernel, grid, block, smem, a); }
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const ClusterArgs& a) { push_tiled(kernel, grid, block, smem, a); }
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const EdgeChainArgs& a) { push_tiled(kernel, grid, block, smem, a); }
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const NodeChainArgs& a) { push_tiled(kernel, grid, block, smem, a); }
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const EmbedFoldArgs& a) { push(kernel, grid, block, smem, a); }
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const RowChainArgs& a) {
  push_tiled(kernel, grid, block, smem, a);
  g_launches.back().row_begin = (long long)((reinterpret_cast<uintptr_t>(a.x) - kRowChainX) / (2 * (uintptr_t)a.ld_x));
}
}  // namespace anemoi

static bool g_record = false;

#if __has_include("chain_plan.h")
#include "chain_plan.h"
// the recorded launch against the plan of the same shape
static void expect_plan(const char* what, anemoi::ChainProblem q, int rc, const Record* r) {
  using namespace anemoi;
  const ChainPlan p = plan_chain(q, chain_switches());  // (the process's switches, as the entry points read them)
  EXPECT(rc == (int)p.status, "%s n_rows %d: rc %d, the plan says %d", what, q.n_rows, rc, (int)p.status);
  if (rc != ANEMOI_OK) return;
  EXPECT((r == nullptr) == (p.grid == 0), "%s n_rows %d: launch %d, planned grid %d", what, q.n_rows, r != nullptr, p.grid);
  if (r == nullptr || p.grid == 0) return;
  EXPECT(r->kernel == chain_kernel_name(p.kernel) && r->grid == p.grid && r->block == p.threads && r->smem == p.lds_bytes,
         "%s n_rows %d: %s <<<%d, %d, %d>>>, planned %s <<<%d, %d, %d>>>", what, q.n_rows, r->kernel.c_str(), r->grid, r->block, r->smem,
         chain_kernel_name(p.kernel), p.grid, p.threads, p.lds_bytes);
  if (q.kind == ChainKind::EmbedFold) return;  // (no panels in its argument block)
  EXPECT(r->rows_per_tile == p.rows_per_panel && r->n_tiles == p.panels && r->n_rows == p.n_rows && r->row_begin == p.row_begin,
         "%s n_rows %d: %d rows x %d panels over %d rows from %lld, planned %d x %d over %d from %lld", what, q.n_rows, r->rows_per_tile, r->n_tiles,
         r->n_rows, r->row_begin, p.rows_per_panel, p.panels, p.n_rows, (long long)p.row_begin);
}
#define PLAN(kind_, ...)                                    \
  do {                                                      \
    anemoi::ChainProblem q_;                                \
    q_.kind = anemoi::ChainKind::kind_;                     \
    __VA_ARGS__;                                            \
    expect_plan(#kind_, q_, rc, r);                         \
  } while (0)
#else
#define PLAN(...) (void)0
#endif

static const int kRows[] = {0, 1, 47, 48, 49, 255 * 48, 255 * 48 + 1, 256 * 48 - 1, 256 * 48, 256 * 48 + 1, 12336, 2 * 256 * 48, 2 * 256 * 48 + 1,
                            10242, 40320, 40962, 542080};

// rc and the one launch (or none) of the call just made
static const Record* one_launch(int rc) {
  EXPECT(g_launches.size() <= 1 && (rc == ANEMOI_OK || g_launches.empty()), "rc %d with %zu launches", rc, g_launches.size());
  return g_launches.empty() ? nullptr : &g_launches[0];
}

static void block_tail(int n, int hidden, int q_out, int rpt, anemoi_dtype_t dt) {
  auto a = host_block(n, q_out, hidden, rpt);
  g_launches.clear();
  const int rc = anemoi_gt_chain2_fwd(&a, dt, nullptr);
  const Record* r = one_launch(rc);
  if (g_record) print_row("block_tail", {n, hidden, q_out, rpt, dt}, rc, r);
  PLAN(BlockTail, q_.n_rows = n; q_.hidden = hidden; q_.q_out_features = q_out; q_.rows_per_tile = rpt; q_.dtype = dt);
}

static void cluster(int n, int hidden, int q_out, anemoi_dtype_t dt) {
  anemoi_gt_cluster_chain_args_t a;
  memset(&a, 0, sizeof a);
  a.attn = P(0x10000); a.ld_attn = 512; a.x_res = P(0x20000); a.ld_x = 512; a.wp = P(0x30000); a.w1 = P(0x40000); a.hidden = hidden; a.w2 = P(0x50000);
  a.wq = q_out ? P(0x60000) : nullptr; a.q_out_features = q_out; a.vec = P(0x70000); a.ln1_eps = a.lnq_eps = 1e-5f;
  a.x_out = P(0x80000); a.ld_out = 512; a.q_out = q_out ? P(0x90000) : nullptr; a.ld_q = q_out > 8 ? q_out : 8;
  a.workspace = P(0x100000); a.workspace_bytes = anemoi_gt_cluster_chain_workspace_bytes(); a.n_rows = n; a.channels = 512;
  g_launches.clear();
  const int rc = anemoi_gt_cluster_chain_fwd(&a, dt, nullptr);
  const Record* r = one_launch(rc);
  if (g_record) print_row("cluster", {n, hidden, q_out, dt}, rc, r);
  PLAN(ClusterTail, q_.n_rows = n; q_.hidden = hidden; q_.q_out_features = q_out; q_.dtype = dt);
}

static void row_chain(int n, int k_in, int q_out, int rpt, anemoi_dtype_t dt) {
  auto a = side_block(n, k_in, q_out, rpt);
  g_launches.clear();
  const int rc = anemoi_gt_rowchain_fwd(&a, dt, nullptr);
  const Record* r = one_launch(rc);
  if (g_record) print_row("row_chain", {n, k_in, q_out, rpt, dt}, rc, r);
  PLAN(RowChain, q_.n_rows = n; q_.in_features = k_in; q_.q_out_features = q_out; q_.rows_per_tile = rpt; q_.dtype = dt);
}

static void row_chain_panels(int n, int k_in, int q_out, int first, int panels, anemoi_dtype_t dt) {
  auto a = side_block(n, k_in, q_out);
  g_launches.clear();
  const int rc = anemoi_gt_rowchain_panels_fwd(&a, first, panels, dt, nullptr);
  const Record* r = one_launch(rc);
  if (g_record) print_row("row_chain_panels", {n, k_in, q_out, first, panels, dt}, rc, r);
  PLAN(RowChainPanels, q_.n_rows = n; q_.in_features = k_in; q_.q_out_features = q_out; q_.first_panel = first; q_.panels = panels; q_.dtype = dt);
  if (rc == ANEMOI_OK && r != nullptr) {  // the rows of the range, and nothing beyond the job
    const long long r0 = (long long)first * 48, r1 = r0 + (long long)panels * 48;
    EXPECT(r->row_begin == r0 && r->n_rows == (int)((r1 < n ? r1 : n) - r0) && r->n_tiles == panels && r->rows_per_tile == 48,
           "panels [%d, +%d) of %d rows: rows [%lld, +%d)", first, panels, n, r->row_begin, r->n_rows);
  }
}

static void embed_fold(int n, int k_in, int q_out, anemoi_dtype_t dt) {
  anemoi_gt_embed_fold_args_t a;
  memset(&a, 0, sizeof a);
  a.x = P(0x10000); a.ld_x = k_in; a.in_features = k_in; a.we = P(0x20000); a.wc = P(0x30000); a.q_out_features = q_out; a.vec = reinterpret_cast<const float*>(P(0x40000));
  a.ln_eps = 1e-5f; a.q_out = P(0x50000); a.ld_q = q_out; a.n_rows = n; a.channels = 512;
  g_launches.clear();
  const int rc = anemoi_gt_embed_fold_fwd(&a, dt, nullptr);
  const Record* r = one_launch(rc);
  if (g_record) print_row("embed_fold", {n, k_in, q_out, dt}, rc, r);
  PLAN(EmbedFold, q_.n_rows = n; q_.in_features = k_in; q_.q_out_features = q_out; q_.dtype = dt);
}

static void graphconv(int n, int mlp_in, anemoi_dtype_t dt) {
  void* const v = P(0x10000);
  const int32_t* const idx = reinterpret_cast<const int32_t*>(P(0x20000));
  g_launches.clear();
  int rc = anemoi_gnn_edge_chain_fwd(v, 512, v, 512, idx, v, 512, idx, v, v, v, v, v, v, v, v, 1e-5f, v, 512, n, 512, dt, nullptr);
  const Record* r = one_launch(rc);
  if (g_record) print_row("gnn_edge", {n, dt}, rc, r);
  PLAN(GnnEdge, q_.n_rows = n; q_.dtype = dt);
  g_launches.clear();
  rc = anemoi_gnn_mlp_chain_fwd(v, 512, mlp_in, v, v, v, v, v, v, v, v, 1e-5f, nullptr, 0, v, 512, n, 512, dt, nullptr);
  r = one_launch(rc);
  if (g_record) print_row("gnn_mlp", {n, mlp_in, dt}, rc, r);
  PLAN(GnnMlp, q_.n_rows = n; q_.in_features = mlp_in; q_.dtype = dt);
  g_launches.clear();
  rc = anemoi_gnn_node_chain_fwd(v, 512, v, 512, v, v, v, v, v, v, v, v, 1e-5f, v, 512, nullptr, nullptr, 0, nullptr, 0, n, 512, dt, nullptr);
  r = one_launch(rc);
  if (g_record) print_row("gnn_node", {n, dt}, rc, r);
  PLAN(GnnNode, q_.n_rows = n; q_.dtype = dt);
}

int main(int argc, char** argv) {
  g_record = argc > 1 && strcmp(argv[1], "--record") == 0;
  // ---- block tails
  for (int n : kRows) {
    for (int hidden : {512, 2048, 4096})
      for (int q_out : {0, 128, 256, 384, 512, 2048, 3072, 3584}) block_tail(n, hidden, q_out, 0, ANEMOI_BF16);
    for (int rpt : {17, 41, 48, 49}) block_tail(n, 2048, 2048, rpt, ANEMOI_BF16);
    block_tail(n, 2000, 0, 0, ANEMOI_BF16);
    block_tail(n, 2048, 100, 0, ANEMOI_BF16);
    block_tail(n, 2048, 3584, 49, ANEMOI_BF16);  // (two refusals at once: the vector limit is asked first)
    block_tail(n, 2048, 2048, 0, ANEMOI_F16);
    block_tail(n, 2048, 2048, 0, ANEMOI_F32);
  }
  block_tail(-1, 2048, 0, 0, ANEMOI_BF16);
  // ---- cluster tails: 1, 8, 9, 64 and 65 panels (32, 32, 64, 256 and 256 workgroups)
  for (int n : {0, 1, 48, 8 * 48, 8 * 48 + 1, 9 * 48, 64 * 48, 64 * 48 + 1, 65 * 48, 10242, 40962}) {
    for (int q_out : {0, 512, 2048, 2560, 100}) cluster(n, 2048, q_out, ANEMOI_BF16);
    cluster(n, 512, 0, ANEMOI_BF16);
    cluster(n, 4096, 0, ANEMOI_F16);
    cluster(n, 2048, 512, ANEMOI_F16);
    cluster(n, 2048, 512, ANEMOI_F32);
  }
  // ---- row chains and their panel ranges
  for (int n : kRows) {
    for (int k_in : {8, 128, 192, 256, 264, 512, 100, 520})
      for (int q_out : {512, 2048, 2560}) row_chain(n, k_in, q_out, 0, ANEMOI_BF16);
    for (int rpt : {17, 48, 49}) row_chain(n, 192, 1024, rpt, ANEMOI_BF16);
    row_chain(n, 192, 1024, 0, ANEMOI_F16);
    row_chain(n, 192, 1024, 0, ANEMOI_F32);
    row_chain(n, 192, 0, 0, ANEMOI_BF16);
  }
  for (int job : {1, 256, 257, 840}) {
    const int n = job * 48 - 5;  // the last panel ragged
    for (int k_in : {192, 256, 264, 512})
      for (int first : {0, job / 2, job - 1})
        for (int panels : {0, 1, 3, job - first, job - first + 1}) row_chain_panels(n, k_in, 1024, first, panels, ANEMOI_BF16);
    row_chain_panels(n, 192, 1024, -1, 1, ANEMOI_BF16);
    row_chain_panels(n, 192, 1024, 0, -1, ANEMOI_BF16);
    row_chain_panels(n, 100, 1024, 0, 1, ANEMOI_BF16);
    row_chain_panels(n, 192, 2560, 0, 1, ANEMOI_BF16);
    row_chain_panels(n, 192, 1024, 0, 1, ANEMOI_F16);
    row_chain_panels(n, 192, 1024, 0, 1, ANEMOI_F32);
  }
  row_chain_panels(0, 192, 1024, 0, 0, ANEMOI_BF16);
  row_chain_panels(0, 192, 1024, 0, 1, ANEMOI_BF16);
  // ---- embed fold
  for (int n : kRows) {
    for (int k_in : {8, 64, 72, 256, 264, 100, 0})
      for (int q_out : {512, 2048, 2560, 0}) embed_fold(n, k_in, q_out, ANEMOI_BF16);
    embed_fold(n, 64, 1024, ANEMOI_F16);
    embed_fold(n, 64, 1024, ANEMOI_F32);
  }
  embed_fold(-1, 64, 1024, ANEMOI_BF16);
  embed_fold(79, 64, 1024, ANEMOI_BF16);
  embed_fold(80, 64, 1024, ANEMOI_BF16);
  embed_fold(81, 64, 1024, ANEMOI_BF16);
  // ---- the GraphConv chains: the row ladders of tests/chain_refs.py (LADDER_EDGE, LADDER_NODE) and the counts above
  std::vector<int> ladder = {1, 2, 47, 48, 49, 63, 64, 65, 256, 257, 16385, 32763, 32769, 12289, 24571, 24577};
  for (int r : {4, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64}) ladder.push_back(256 * r - 3);
  for (int n : kRows) ladder.push_back(n);
  for (int n : ladder) graphconv(n, 512, ANEMOI_BF16);
  for (int mlp_in : {128, 256, 384, 0, 100, 640}) graphconv(40962, mlp_in, ANEMOI_F16);
  graphconv(0, 100, ANEMOI_BF16);  // (the embedding MLP refuses its width before it looks at the rows)
  graphconv(40962, 512, ANEMOI_F32);
  graphconv(-1, 512, ANEMOI_BF16);
  // ---- pointers, alignment and leading dimensions: looked at by the entry points, not by the plan
  {
    auto a = host_block(149, 2048, 2048);
    auto b = a; b.attn = P(0x10008);
    EXPECT(anemoi_gt_chain2_fwd(&b, ANEMOI_BF16, nullptr) == ANEMOI_E_INVALID, "tail alignment");
    b = a; b.ld_q = 1024;
    EXPECT(anemoi_gt_chain2_fwd(&b, ANEMOI_BF16, nullptr) == ANEMOI_E_INVALID, "tail ld_q");
    b = a; b.w1 = nullptr;
    EXPECT(anemoi_gt_chain2_fwd(&b, ANEMOI_BF16, nullptr) == ANEMOI_E_INVALID, "tail null operand");
    b = a; b.channels = 256;
    EXPECT(anemoi_gt_chain2_fwd(&b, ANEMOI_BF16, nullptr) == ANEMOI_E_INVALID, "tail channels");
    EXPECT(anemoi_gt_chain2_fwd(nullptr, ANEMOI_BF16, nullptr) == ANEMOI_E_INVALID, "tail null block");
    auto s = side_block(347, 192, 1024);
    auto t = s; t.x = P(kRowChainX + 4);
    EXPECT(anemoi_gt_rowchain_fwd(&t, ANEMOI_BF16, nullptr) == ANEMOI_E_INVALID, "row chain alignment");
    t = s; t.ld_q = 512;
    EXPECT(anemoi_gt_rowchain_fwd(&t, ANEMOI_BF16, nullptr) == ANEMOI_E_INVALID, "row chain ld_q");
    t = s; t.q_out = nullptr;
    EXPECT(anemoi_gt_rowchain_panels_fwd(&t, 0, 1, ANEMOI_BF16, nullptr) == ANEMOI_E_INVALID, "row chain null output");
    t = s; t.channels = 256;
    EXPECT(anemoi_gt_rowchain_fwd(&t, ANEMOI_BF16, nullptr) == ANEMOI_E_INVALID, "row chain channels");
    EXPECT(anemoi_gt_rowchain_fwd(nullptr, ANEMOI_BF16, nullptr) == ANEMOI_E_INVALID, "row chain null block");
    EXPECT(anemoi_gt_cluster_chain_fwd(nullptr, ANEMOI_BF16, nullptr) == ANEMOI_E_INVALID, "cluster null block");
    EXPECT(anemoi_gt_embed_fold_fwd(nullptr, ANEMOI_BF16, nullptr) == ANEMOI_E_INVALID, "embed fold null block");
    // the GraphConv edge and MLP chains check their operands in one place: the code, and the text under the entry point's own name
    void* const v = P(0x10000);
    void* const odd = P(0x10004);
    const int32_t* const idx = reinterpret_cast<const int32_t*>(P(0x20000));
    const auto refused = [](int rc, const char* text) { return rc == ANEMOI_E_INVALID && strcmp(anemoi::g_err, text) == 0; };
    const char* const kNull = "gnn_edge_chain_fwd: null operand";
    const char* const kAlign = "gnn_edge_chain_fwd: operand alignment / leading dimensions";
    EXPECT(refused(anemoi_gnn_edge_chain_fwd(v, 512, nullptr, 512, idx, v, 512, idx, v, v, v, v, v, v, v, v, 1e-5f, v, 512, 65, 512, ANEMOI_BF16, nullptr), kNull), "edge null g1");
    EXPECT(refused(anemoi_gnn_edge_chain_fwd(v, 512, v, 512, idx, v, 512, nullptr, v, v, v, v, v, v, v, v, 1e-5f, v, 512, 65, 512, ANEMOI_BF16, nullptr), kNull), "edge null idx2");
    EXPECT(refused(anemoi_gnn_edge_chain_fwd(v, 512, v, 512, idx, v, 512, idx, v, v, v, v, v, v, nullptr, v, 1e-5f, v, 512, 65, 512, ANEMOI_BF16, nullptr), kNull), "edge null ln_w");
    EXPECT(anemoi_gnn_edge_chain_fwd(v, 512, v, 512, idx, v, 512, idx, v, v, v, v, v, v, v, nullptr, 1e-5f, v, 512, 65, 512, ANEMOI_BF16, nullptr) == ANEMOI_OK, "edge without ln_b");
    EXPECT(refused(anemoi_gnn_edge_chain_fwd(v, 512, odd, 512, idx, v, 512, idx, v, v, v, v, v, v, v, v, 1e-5f, v, 512, 65, 512, ANEMOI_BF16, nullptr), kAlign), "edge g1 alignment");
    EXPECT(refused(anemoi_gnn_edge_chain_fwd(v, 512, v, 510, idx, v, 512, idx, v, v, v, v, v, v, v, v, 1e-5f, v, 512, 65, 512, ANEMOI_BF16, nullptr), kAlign), "edge ld_g1");
    EXPECT(refused(anemoi_gnn_edge_chain_fwd(v, 504, v, 512, idx, v, 512, idx, v, v, v, v, v, v, v, v, 1e-5f, v, 512, 65, 512, ANEMOI_BF16, nullptr), kAlign), "edge ld_e");
    EXPECT(anemoi_gnn_edge_chain_fwd(v, 512, nullptr, 512, idx, v, 512, idx, v, v, v, v, v, v, v, v, 1e-5f, v, 512, 0, 512, ANEMOI_BF16, nullptr) == ANEMOI_OK, "edge no rows: operands not looked at");
    const char* const kMlpNull = "gnn_mlp_chain_fwd: null operand";
    const char* const kMlpAlign = "gnn_mlp_chain_fwd: operand alignment / leading dimensions";
    EXPECT(refused(anemoi_gnn_mlp_chain_fwd(nullptr, 256, 256, v, v, v, v, v, v, v, v, 1e-5f, nullptr, 0, v, 512, 65, 512, ANEMOI_F16, nullptr), kMlpNull), "mlp null x");
    EXPECT(anemoi_gnn_mlp_chain_fwd(v, 256, 256, v, v, v, v, v, v, v, v, 1e-5f, nullptr, 0, v, 512, 65, 512, ANEMOI_F16, nullptr) == ANEMOI_OK, "mlp 256 columns wide, no residual");
    EXPECT(refused(anemoi_gnn_mlp_chain_fwd(v, 248, 256, v, v, v, v, v, v, v, v, 1e-5f, nullptr, 0, v, 512, 65, 512, ANEMOI_F16, nullptr), kMlpAlign), "mlp ld_x below in_features");
    EXPECT(refused(anemoi_gnn_mlp_chain_fwd(v, 256, 256, v, v, v, v, v, v, v, v, 1e-5f, v, 510, v, 512, 65, 512, ANEMOI_F16, nullptr), kMlpAlign), "mlp ld_res");
    EXPECT(refused(anemoi_gnn_mlp_chain_fwd(v, 256, 256, v, v, v, v, v, v, v, v, 1e-5f, odd, 512, v, 512, 65, 512, ANEMOI_F16, nullptr), kMlpAlign), "mlp residual alignment");
    EXPECT(anemoi_gnn_mlp_chain_fwd(v, 256, 256, v, v, v, v, v, v, v, v, 1e-5f, v, 512, v, 512, 65, 512, ANEMOI_F16, nullptr) == ANEMOI_OK, "mlp with residual");
  }
  if (!g_record) printf("chain entry points: %d checks, %d failures\n", g_cases, g_fail);
  return g_fail ? 1 : 0;
}
