// Row-resident embedding chain for gfx950 (round 6): one side of a GraphTransformer mapper in ONE launch -
//
//     y     = x W_e^T + b_e                         (emb_nodes_src / emb_nodes_dst: Linear(in, 512), layers/mapper.py:480-597, 600-704 of the reference)
//     q_out = LN(y) [W_a; W_b ...]^T + b            (the block's layer_norm_attention_src + [lin_key; lin_value], or layer_norm_attention_dest +
//                                                    [lin_query; lin_self]: layers/block.py:981-984)
//
// instead of the embedding GEMM (which wrote y and its row statistics) + the LayerNorm-fold GEMM (which read y back): for the 40 320-row sides
// of the O96 mappers y is a 41-MB round trip through HBM, and on the SOURCE side of the encoder it is needed by nobody else (the block
// returns the source rows untouched): with x_out = NULL y never exists in memory.
//
// The machinery is csrc/gt_chain2.hip's (chain2_core.h): a workgroup keeps a panel of <= 48 rows in LDS, weights are fragment-major images
// streamed L2 -> registers -> MFMA, the LayerNorm is the plain fp32 LayerNorm of the ROUNDED 16-bit rows applied without its affine part (the
// caller folds gamma / beta into the projection: wq = image of W diag(gamma), dq = W beta + b), accumulators start at their bias.  The
// single-panel schedule is a device function of rowchain_core.h (a block tail's idle workgroups run it too: gt_chain2.hip).
#include "rowchain_core.h"

namespace anemoi {

// (the single-panel schedule: rowchain_core.h)
template <typename T>
__global__ __launch_bounds__(512, 1) void gt_rowchain_kernel(RowChainArgs a) {
  rowchain_panels<T>(a, GridWalk{});
}

// ---------------------------------------------------------------------------------------------------------------- several panel rounds: pipelined
// With more panels than CUs a workgroup walks a LIST of panels, and the single-panel schedule above spends ~21 us per round of which only ~12 are the
// weight stream (1.2 MB per panel through the CU's L1 path).  Here the two wave groups work on DIFFERENT panels: group A (waves 0-3, 128 columns each)
// computes y = x W_e^T + b_e, its statistics and LayerNorm for panel s while group B (waves 4-7) runs the projection chunks of panel s - 1:
//
//     phase 1   A: LN(y)(s-1), parked in its accumulators since the last step -> bufN; the rows of x(s), requested a step ago -> bufX
//     phase 2   A: request x(s+1); acc = b_e; GEMM on bufX; rounded y in registers + row statistics     B: chunk 0 of panel s-1 on bufN -> staged -> global
//     phase 3   A: y -> global (staged through bufX, if wanted); LN(y) in registers                    B: chunks 1 .. of panel s-1
//
// one s_barrier behind each phase (both groups: the hardware barrier counts all eight waves), n + 1 steps for n panels.  LDS: bufX, bufN, group B's
// staging buffer (48 KB each) + the partials + the vectors.  in_features <= 256 (the parked rows of x(s+1) are 6 registers per lane).
// (kRc2Vec, XRowsA, PipeCtx and the two roles: rowchain_core.h - the riders of a block tail run them too)
template <typename T>
__global__ __launch_bounds__(512, 1) void gt_rowchain_pipe_kernel(RowChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  PipeCtx c;
  c.tid = tid & 255;
  c.lane = tid & 63;
  const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  c.wq = w8 & 3;
  c.loff = c.lane * 16;
  c.b0 = (int)blockIdx.x;
  c.grid = (int)gridDim.x;
  if (c.b0 >= a.n_tiles) return;
  c.n = (a.n_tiles - c.b0 + c.grid - 1) / c.grid;
  {  // the per-column vectors -> LDS (visible behind the prologue's barrier)
    const int n16 = (512 + 512 * a.qc) / 8;  // <= 320
    if (tid < n16) reinterpret_cast<u32x4*>(smem + kRc2Vec)[tid] = reinterpret_cast<const u32x4*>(a.vec)[tid];
  }
  if (w8 < 4) pipe_role_a<T>(a, c, smem);
  else pipe_role_b<T>(a, c, smem);
}

// the plan's kernel: the single-panel schedule, or - several rounds of panels - the two wave groups on different panels
template <typename T>
static int launch_rowchain(const RowChainArgs& a, const ChainPlan& plan, hipStream_t st) {
  if (plan.kernel == ChainKernel::RowChainSingle) {
    ANEMOI_CHAIN_LAUNCH((gt_rowchain_kernel<T>), kRowChainSmem, plan, st, a);
    return check_launch("gt_rowchain_kernel");
  }
  ANEMOI_CHAIN_LAUNCH((gt_rowchain_pipe_kernel<T>), kRowChain2Smem, plan, st, a);
  return check_launch("gt_rowchain_pipe_kernel");
}

}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_gt_rowchain_fwd(const anemoi_gt_rowchain_args_t* p, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(p != nullptr, "gt_rowchain_fwd: null argument block");
  RowChainArgs a;
  ChainPlan plan;
  const int rc = rowchain_args(p, rowchain_problem(p, dtype), "gt_rowchain_fwd", a, plan);
  if (rc != ANEMOI_OK || plan.grid == 0) return rc;
  hipStream_t st = as_stream(stream);
  return dtype == ANEMOI_BF16 ? launch_rowchain<bf16_t>(a, plan, st) : launch_rowchain<f16_t>(a, plan, st);
}

extern "C" int anemoi_gt_rowchain_panels_fwd(const anemoi_gt_rowchain_args_t* p, int32_t first_panel, int32_t panels, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(p != nullptr, "gt_rowchain_panels_fwd: null argument block");
  RowChainArgs a;
  ChainPlan plan;
  const int rc = rowchain_args(p, rowchain_problem(p, dtype, ChainKind::RowChainPanels, first_panel, panels), "gt_rowchain_panels_fwd", a, plan);
  if (rc != ANEMOI_OK || plan.grid == 0) return rc;
  // the plan's schedule is the WHOLE job's (a panel's bits do not depend on which launch computes it), on the range's rows: the job shifted to its first row
  const int64_t es = 2;
  a.x = static_cast<const char*>(a.x) + plan.row_begin * a.ld_x * es;
  if (a.xout != nullptr) a.xout = static_cast<char*>(a.xout) + plan.row_begin * a.ld_out * es;
  a.qout = static_cast<char*>(a.qout) + plan.row_begin * a.ld_q * es;
  a.n_rows = plan.n_rows;
  a.n_tiles = plan.panels;
  hipStream_t st = as_stream(stream);
  return dtype == ANEMOI_BF16 ? launch_rowchain<bf16_t>(a, plan, st) : launch_rowchain<f16_t>(a, plan, st);
}
