// Which kernel an edge-attention entry point runs (gt_attention.hip, gt_attention_bwd.hip), on which lane layout, with how much LDS
// and on how many workgroups: the whole decision, as one pure host function, plus the one ladder that turns its answer into template
// arguments.  Plain C++17 - no HIP - so it can be asked without a GPU (anemoi_gt_attention_plan in include/anemoi_hip.h,
// ops.gt_attention_plan in Python, tests/test_attention_plan_cpu.py).  The two .hip files only launch what plan_attention returns.
#pragma once
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "anemoi_hip.h"

namespace anemoi {

void set_error(const char* fmt, ...);  // lib.cpp

#ifndef ANEMOI_ATTN_WPB
#define ANEMOI_ATTN_WPB 4
#endif
constexpr int kWavesPerBlock = ANEMOI_ATTN_WPB;  // forward kernels: one destination per wave (a build-time tuning knob, tools/build_alt.sh)
constexpr int kBwdWaves = 4;                     // backward kernels
constexpr int kGenericMaxC = 256;                // the generic forward keeps a head's accumulator in private memory
constexpr int kWgradBlocks = 256;                // partial rows of dW' (anemoi_gt_attention_fused_edge_bwd_partial_floats)

enum class AttnOp : int32_t { Fwd = 0, FwdFusedEdge = 1, Bwd = 2, BwdFusedEdge = 3 };
enum class AttnRoute : int32_t { Unsupported = 0, Generic = 1, Wave = 2 };

struct AttnPlan {
  AttnRoute route = AttnRoute::Unsupported;  // Wave: one wave64 per row; Generic: one thread per (row, head); Unsupported: the entry point refuses
  int vec = 0, lph = 0;       // Wave: channels per lane, lanes per head
  int fe_pad = 0;             // fused-edge ops: the padded edge-feature count (a template argument on the wave route)
  bool kv_adjacent = false;   // fused-edge forward on the wave route: the instantiation that reads v behind k through one address
  int lds_bytes = 0;          // dynamic LDS of the destination pass (the W' image)
  unsigned grid_dst = 0;      // workgroups of the destination pass / of the forward
  unsigned grid_src = 0;      // backward: workgroups of the source pass
  unsigned grid_wgrad = 0;    // fused-edge backward: workgroups (= partial rows) of the weight-gradient kernel
};

// LDS image of W' = [W_e | b_e | 0] of the fused-edge kernels: per lane a chunk of VEC*FE_PAD floats (+4 floats of padding so that
// 16 consecutive lanes' ds_read_b128 hit 16 distinct 16-byte bank slots).
constexpr int w_image_chunk(int vec, int fe_pad) { return vec * fe_pad + 4; }
template <int VEC, int FE_PAD>
struct WLayout {
  static constexpr int kChunk = w_image_chunk(VEC, FE_PAD);
  static constexpr int kFloats = 64 * kChunk;
};
constexpr int64_t w_image_bytes(int vec, int fe_pad) { return 64 * (int64_t)w_image_chunk(vec, fe_pad) * (int64_t)sizeof(float); }
constexpr int64_t kMaxDynamicLds = 64 * 1024;  // the default dynamic-LDS limit: no kernel of the family raises it

constexpr bool pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

// The wave layout: one wave covers a row of D = H*C channels exactly, VEC = D/64 contiguous channels per lane, a head = LPH = C/VEC
// adjacent lanes inside one DPP row.  The kernels are instantiated for VEC, LPH in {1, 2, 4, 8, 16} (with_lane_layout below).
inline bool wave_layout(int H, int C, int* vec, int* lph) {
  const int D = H * C;
  if (D % 64 != 0) return false;
  const int v = D / 64;
  if (!pow2(v) || v > 16 || C % v != 0 || !pow2(C / v) || C / v > 16) return false;
  *vec = v, *lph = C / v;
  return true;
}

// The fused-edge backward is built for the shapes the production configs train: 512 channels with C = 32 / 64, 256 channels with
// C = 32, and the 64-channel test models (C = 16 / 8).  Everything else trains through the materialised-E op.
constexpr bool fused_bwd_pair(int vec, int lph) {
  return (vec == 8 && (lph == 4 || lph == 8)) || (vec == 4 && lph == 8) || (vec == 1 && (lph == 16 || lph == 8));
}

// Alignment is a fact the caller computes from its pointers and strides: every operand 16-byte aligned and every leading dimension a
// multiple of `elems` elements (a null operand passes the pointer test; its stride is tested like any other, so absent operands
// come in with ld = 0 where the op does not look at their stride).
struct RowOperand {
  const void* p;
  int64_t ld;
};
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool rows_aligned(std::initializer_list<RowOperand> operands, int64_t elems) {
  for (const RowOperand& o : operands)
    if (!al16(o.p) || o.ld % elems != 0) return false;
  return true;
}
// The multiple differs between the directions, and the difference is inherited, not designed: the forward asks for 8 elements of
// every dtype, the backwards for 16 bytes' worth (8 for 16-bit, 4 for fp32).  An fp32 call with ld % 8 == 4 therefore runs the
// generic forward and the wave backward.  Both are correct; making them one rule would change which kernel such calls run.
inline int64_t align_elems(AttnOp op, int elem_size) {
  return op == AttnOp::Fwd || op == AttnOp::FwdFusedEdge ? 8 : 16 / elem_size;
}
// v = the D columns behind k in one buffer (the fused projection's layout) and every row offset fits 32 bits
inline bool kv_rows_adjacent(const void* k, const void* v, int64_t ldk, int64_t ldv, int D, int n_src, int elem_size) {
  return static_cast<const char*>(v) == static_cast<const char*>(k) + (int64_t)D * elem_size && ldv == ldk &&
         (int64_t)n_src * ldk < (int64_t(1) << 32);
}

inline unsigned blocks_for(int64_t items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// blocks_per_cu: ANEMOI_ATTN_BLOCKS_PER_CU as read once per process (0 = the rule below)
inline AttnPlan plan_attention(AttnOp op, int H, int C, int fe_pad, int n_dst, int n_src, bool aligned, bool kv_adjacent,
                               int blocks_per_cu) {
  const bool fwd = op == AttnOp::Fwd || op == AttnOp::FwdFusedEdge;
  const bool fused = op == AttnOp::FwdFusedEdge || op == AttnOp::BwdFusedEdge;
  AttnPlan p;
  p.fe_pad = fused ? fe_pad : 0;
  int vec = 0, lph = 0;
  bool wave = aligned && wave_layout(H, C, &vec, &lph);
  if (wave && fused)  // FE_PAD is a template argument, and the W' image must fit the default dynamic LDS
    wave = (fe_pad == 4 || fe_pad == 8 || fe_pad == 12 || fe_pad == 16) && w_image_bytes(vec, fe_pad) <= kMaxDynamicLds;
  if (wave && op == AttnOp::BwdFusedEdge) wave = fused_bwd_pair(vec, lph);
  if (!wave) {
    // one thread per (row, head): any H, C, any alignment; the fused-edge backward has no such kernel
    if (op == AttnOp::BwdFusedEdge || (fwd && C > kGenericMaxC)) return p;
    p.route = AttnRoute::Generic;
    p.grid_dst = blocks_for((int64_t)n_dst * H, 128);
    if (!fwd) p.grid_src = blocks_for((int64_t)n_src * H, 128);
    return p;
  }
  p.route = AttnRoute::Wave;
  p.vec = vec, p.lph = lph;
  if (fused) p.lds_bytes = (int)w_image_bytes(vec, fe_pad);
  if (!fwd) p.grid_src = blocks_for(n_src, kBwdWaves);
  switch (op) {
    case AttnOp::Fwd:
      p.grid_dst = blocks_for(n_dst, kWavesPerBlock);
      break;
    case AttnOp::FwdFusedEdge: {
      // persistent grid: a few workgroups per CU (LDS 25 KiB each, 5-7 waves/SIMD by registers); every wave walks destinations
      // d, d + total_waves, ... so the W' staging is paid once per workgroup.  How many: with the locality-preserving work order
      // the number of destinations in flight per XCD is also the size of the window whose K|V rows should stay in the L2 -
      // measured on MI355X (profiles/r03_attention_blocks_per_cu.txt, three repetitions): 10 242 destinations 27.4 / 26.9 / 26.1 us
      // at 5 / 6 / 7 workgroups per CU, 40 962 destinations 80.6 / 89.6 / 84.2 us (5 workgroups = 640 waves per XCD = exactly 8
      // destinations per wave, and the smallest window); forwards: O96 2.991 / 2.991 / 2.973 ms, O96 -> res 6 8.69 / 8.81 / 8.76 ms,
      // N320 15.21 / 15.68 / 15.39 ms.  ANEMOI_ATTN_BLOCKS_PER_CU overrides the rule.
      const int per_cu = blocks_per_cu > 0 ? blocks_per_cu : (n_dst >= 20000 ? 5 : 7);
      const unsigned blocks = blocks_for(n_dst, kWavesPerBlock), max_blocks = 256u * per_cu;
      p.grid_dst = ((blocks < max_blocks ? blocks : max_blocks) + 7) & ~7u;  // a whole number of workgroups per XCD
      p.kv_adjacent = kv_adjacent;
      break;
    }
    case AttnOp::Bwd:
      p.grid_dst = blocks_for(n_dst, kBwdWaves);
      break;
    case AttnOp::BwdFusedEdge: {  // persistent waves over the destinations: the W' staging is paid once per workgroup
      const unsigned blocks = blocks_for(n_dst, kBwdWaves);
      p.grid_dst = blocks < 256 * 6 ? blocks : 256 * 6;
      p.grid_wgrad = blocks < (unsigned)kWgradBlocks ? blocks : kWgradBlocks;
      break;
    }
  }
  return p;
}

// ---------------------------------------------------------------------------------------------- plan -> template arguments
// f(integral_constant VEC, integral_constant LPH) for the plan's lane layout.  kFusedBwdPairsOnly: only the pairs of fused_bwd_pair
// are instantiated (the others cannot be planned for that op).
template <int N>
using int_c = std::integral_constant<int, N>;

template <bool kFusedBwdPairsOnly = false, typename F>
int with_lane_layout(const AttnPlan& p, F&& f) {
  auto lanes = [&](auto vec_c) {
    constexpr int VEC = decltype(vec_c)::value;
    auto go = [&](auto lph_c) {
      if constexpr (!kFusedBwdPairsOnly || fused_bwd_pair(VEC, decltype(lph_c)::value)) return f(vec_c, lph_c);
      return (int)ANEMOI_E_UNSUPPORTED;
    };
    switch (p.lph) {
      case 1: return go(int_c<1>{});
      case 2: return go(int_c<2>{});
      case 4: return go(int_c<4>{});
      case 8: return go(int_c<8>{});
      case 16: return go(int_c<16>{});
      default: return (int)ANEMOI_E_UNSUPPORTED;
    }
  };
  int rc = ANEMOI_E_UNSUPPORTED;
  switch (p.vec) {
    case 1: rc = lanes(int_c<1>{}); break;
    case 2: rc = lanes(int_c<2>{}); break;
    case 4: rc = lanes(int_c<4>{}); break;
    case 8: rc = lanes(int_c<8>{}); break;
    case 16: rc = lanes(int_c<16>{}); break;
  }
  if (rc == ANEMOI_E_UNSUPPORTED) set_error("gt_attention: no kernel is built for the planned lane layout VEC=%d LPH=%d", p.vec, p.lph);
  return rc;
}

// f(integral_constant FE_PAD) for the plan's padded edge-feature count
template <typename F>
int with_fe_pad(const AttnPlan& p, F&& f) {
  switch (p.fe_pad) {
    case 4: return f(int_c<4>{});
    case 8: return f(int_c<8>{});
    case 12: return f(int_c<12>{});
    case 16: return f(int_c<16>{});
    default: set_error("gt_attention: no kernel is built for the planned fe_pad=%d", p.fe_pad); return ANEMOI_E_UNSUPPORTED;
  }
}

}  // namespace anemoi
