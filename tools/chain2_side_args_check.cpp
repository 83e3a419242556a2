// Host-only check of anemoi_gt_chain2_side_fwd's argument validation and launch plan: the entry point of csrc/gt_chain2.hip compiled for the
// HOST (csrc/gt_chain2_side.hip) with its kernel launches replaced by a recorder, driven over valid and invalid argument blocks.  Nothing is launched; no GPU needed.
// (The other chain entry points: tools/chain_args_check.cpp; --record as there.)
//
//   hipcc --cuda-host-only -x hip -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         -I include -I anemoi_core_amd/csrc tools/chain2_side_args_check.cpp -o /tmp/chain2_side_args_check && /tmp/chain2_side_args_check
#include "chain_check_common.h"

#include "chain2_core.h"
#include "rowchain_core.h"
namespace anemoi {
struct Chain2Args;
struct Chain2SideArgs;
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const Chain2SideArgs& a);
}  // namespace anemoi

#include "gt_chain2_side.hip"

// (the tail alone is the other translation unit's entry point: recorded as a delegation)
static int g_delegated = 0;
extern "C" int anemoi_gt_chain2_fwd(const anemoi_gt_chain2_args_t*, anemoi_dtype_t, void*) {
  ++g_delegated;
  return ANEMOI_OK;
}

namespace anemoi {
static void record_launch(const char* kernel, dim3 grid, dim3 block, int smem, const Chain2SideArgs& a) {
  Record r;
  r.kernel = kernel_name(kernel);
  r.grid = (int)grid.x; r.block = (int)block.x; r.smem = smem; r.n_rows = a.n_rows; r.rows_per_tile = a.rows_per_tile; r.n_tiles = a.n_tiles;
  r.host_grid = a.host_grid; r.first = a.side_first; r.end = a.side_end; r.riders = a.side_blocks; r.pipe = a.side_pipe; r.side_tiles = a.side.n_tiles;
  g_launches.push_back(r);
}
}  // namespace anemoi

static bool g_record = false;
static int side_call(anemoi_gt_chain2_args_t* h, anemoi_gt_rowchain_args_t* s, int first, int count, int cap, anemoi_dtype_t dt) {
  g_launches.clear();
  g_delegated = 0;
  anemoi::g_err[0] = 0;
  const int rc = anemoi_gt_chain2_side_fwd(h, s, first, count, cap, dt, nullptr);
  // (the table describes shapes: calls with a faulty pointer, leading dimension or channel count are checked below and not printed)
  const bool shapes_only = h != nullptr && s != nullptr && h->attn == P(0x10000) && h->ld_q == h->q_out_features && h->channels == 512 && s->x == P(kRowChainX) &&
                           s->q_out != nullptr && s->ld_q == s->q_out_features && s->channels == 512;
  if (g_record && shapes_only)
    print_row("block_tail_side", {h->n_rows, h->hidden, h->q_out_features, h->rows_per_tile, s->n_rows, s->in_features, s->q_out_features, s->rows_per_tile,
                                  first, count, cap, dt},
              rc, g_launches.empty() ? nullptr : &g_launches[0], g_delegated == 1);
  return rc;
}

// the workgroups of a tail of `tiles` panels, restated: one per panel up to the chip, beyond as many as make the rounds even
static int tail_grid(int tiles) {
  if (tiles <= 256) return tiles;
  const int rounds = (tiles + 255) / 256;
  return (tiles + rounds - 1) / rounds;
}

int main(int argc, char** argv) {
  using namespace anemoi;
  g_record = argc > 1 && strcmp(argv[1], "--record") == 0;
  const int smem_side = kChain2SideSmem;
  // ---- valid blocks: the recorded launch is the plan
  for (int host_rows : {1, 47, 48, 149, 10242, 12240 - 48, 12240, 12288 - 1, 12288, 12289, 12336, 24576, 24577, 40962, 542080}) {
    for (int side_rows : {1, 48, 347, 40320}) {
      const int tiles = (host_rows + 47) / 48, side_tiles = (side_rows + 47) / 48;
      const int grid = tail_grid(tiles);
      for (int first : {0, 3, side_tiles - 1, side_tiles}) {
        if (first < 0 || first > side_tiles) continue;
        for (int count : {0, 1, 4, side_tiles - first}) {
          if (count < 0 || first + count > side_tiles) continue;
          for (int cap : {0, 1, 2, 300}) {
            for (anemoi_dtype_t dt : {ANEMOI_BF16, ANEMOI_F16}) {
              if (dt == ANEMOI_F16 && (cap != 0 || first != 0)) continue;  // (the dtype picks the instantiation and nothing else)
              auto h = host_block(host_rows, 2048);
              auto s = side_block(side_rows, 192, 1024);
              const int rc = side_call(&h, &s, first, count, cap, dt);
              if (grid >= 256) {
                EXPECT(rc == ANEMOI_E_UNSUPPORTED && g_launches.empty(), "host %d side %d rc %d launches %zu", host_rows, side_rows, rc, g_launches.size());
                continue;
              }
              if (count == 0) {  // the tail alone
                EXPECT(rc == ANEMOI_OK && g_launches.empty() && g_delegated == 1, "no panels: rc %d, %d delegations", rc, g_delegated);
                continue;
              }
              EXPECT(rc == ANEMOI_OK && g_launches.size() == 1 && g_delegated == 0, "host %d side %d first %d count %d cap %d rc %d", host_rows, side_rows, first, count, cap, rc);
              if (rc != ANEMOI_OK || g_launches.size() != 1) continue;
              const Record& r = g_launches[0];
              int riders = 256 - grid;
              if (cap > 0 && cap < riders) riders = cap;
              if (count < riders) riders = count;
              EXPECT(r.kernel == "gt_chain2_kernel<false,true,true>" && r.host_grid == grid && r.riders == riders && r.grid == grid + riders && r.grid <= 256 && r.block == 512 && r.smem == smem_side,
                     "grid %d host_grid %d riders %d (want %d + %d)", r.grid, r.host_grid, r.riders, grid, riders);
              EXPECT(r.first == first && r.end == first + count && r.end <= r.side_tiles && r.side_tiles == side_tiles && r.n_tiles == tiles && r.pipe == (side_tiles > 256 ? 1 : 0),
                     "panels [%d, %d) of %d", r.first, r.end, r.side_tiles);
            }
          }
        }
      }
    }
  }
  for (int k_in : {256, 264})  // (264: the first width whose riders are not pipelined)
    for (int host_rows : {149, 10242}) {
      auto h = host_block(host_rows, 2048);
      auto s = side_block(40320, k_in, 1024);
      const int rc = side_call(&h, &s, 0, 4, 0, ANEMOI_BF16);
      EXPECT(rc == ANEMOI_OK && g_launches.size() == 1 && g_launches[0].pipe == (k_in <= 256), "side in_features %d: rc %d", k_in, rc);
    }
  // ---- invalid blocks: the code, and nothing launched
  auto expect_refused = [&](const char* what, int want, anemoi_gt_chain2_args_t* h, anemoi_gt_rowchain_args_t* s, int first, int count, int cap,
                            anemoi_dtype_t dt = ANEMOI_BF16, bool with_text = true) {
    const int rc = side_call(h, s, first, count, cap, dt);
    EXPECT(rc == want && g_launches.empty() && (g_err[0] != 0 || !with_text), "%s: rc %d (want %d), launches %zu", what, rc, want, g_launches.size());
  };
  {
    auto h = host_block(149, 2048);
    auto s = side_block(347, 192, 1024);
    expect_refused("null host block", ANEMOI_E_INVALID, nullptr, &s, 0, 8, 0);
    expect_refused("null side block", ANEMOI_E_INVALID, &h, nullptr, 0, 8, 0);
    expect_refused("fp32", ANEMOI_E_INVALID, &h, &s, 0, 8, 0, ANEMOI_F32);
    expect_refused("negative first", ANEMOI_E_INVALID, &h, &s, -1, 8, 0);
    expect_refused("negative count", ANEMOI_E_INVALID, &h, &s, 0, -1, 0);
    expect_refused("negative cap", ANEMOI_E_INVALID, &h, &s, 0, 8, -1);
    expect_refused("range beyond the job", ANEMOI_E_INVALID, &h, &s, 3, 6, 0);
    expect_refused("range overflow", ANEMOI_E_INVALID, &h, &s, 0x7fffffff, 0x7fffffff, 0);
    auto b = h; b.channels = 256;
    expect_refused("host channels", ANEMOI_E_INVALID, &b, &s, 0, 8, 0);
    b = h; b.attn = P(0x10008);
    expect_refused("host alignment", ANEMOI_E_INVALID, &b, &s, 0, 8, 0);
    b = h; b.ld_q = 1024;
    expect_refused("host ld_q", ANEMOI_E_INVALID, &b, &s, 0, 8, 0);
    b = h; b.hidden = 2000;
    expect_refused("host hidden", ANEMOI_E_INVALID, &b, &s, 0, 8, 0);
    b = h; b.rows_per_tile = 49;
    expect_refused("host rows_per_tile", ANEMOI_E_INVALID, &b, &s, 0, 8, 0);
    b = host_block(149, 4096);
    expect_refused("host vectors beyond LDS", ANEMOI_E_UNSUPPORTED, &b, &s, 0, 8, 0, ANEMOI_BF16, false);  // (anemoi_gt_chain2_fwd's quiet refusal)
    b = host_block(0, 2048);
    expect_refused("no tail to ride on", ANEMOI_E_UNSUPPORTED, &b, &s, 0, 8, 0);
    b = host_block(256 * 48, 2048);
    expect_refused("full tail", ANEMOI_E_UNSUPPORTED, &b, &s, 0, 8, 0);
    // the side job's own preconditions: unsupported (the caller launches it some other way)
    auto t = s; t.in_features = 100;
    expect_refused("side in_features", ANEMOI_E_UNSUPPORTED, &h, &t, 0, 8, 0);
    t = s; t.in_features = 520; t.ld_x = 520;
    expect_refused("side in_features > 512", ANEMOI_E_UNSUPPORTED, &h, &t, 0, 8, 0);
    t = s; t.q_out_features = 2560; t.ld_q = 2560;
    expect_refused("side q_out", ANEMOI_E_UNSUPPORTED, &h, &t, 0, 8, 0);
    t = s; t.x = P(kRowChainX + 4);
    expect_refused("side alignment", ANEMOI_E_UNSUPPORTED, &h, &t, 0, 8, 0);
    t = s; t.q_out = nullptr;
    expect_refused("side null output", ANEMOI_E_UNSUPPORTED, &h, &t, 0, 8, 0);
    t = s; t.ld_q = 512;
    expect_refused("side ld_q", ANEMOI_E_UNSUPPORTED, &h, &t, 0, 8, 0);
    t = s; t.channels = 256;
    expect_refused("side channels", ANEMOI_E_UNSUPPORTED, &h, &t, 0, 8, 0);
    t = s; t.rows_per_tile = 64;
    expect_refused("side rows_per_tile", ANEMOI_E_UNSUPPORTED, &h, &t, 0, 8, 0);
  }
  if (!g_record) printf("chain2 side entry point: %d checks, %d failures\n", g_cases, g_fail);
  return g_fail ? 1 : 0;
}
