// Edge attention, forward: what stands in front of the fused-edge forward kernel - build-time knobs, the packed dot product, the
// deferred-max threshold.  gt_attention.hip and csrc/experiments/gt_attention_r05_variants.hip each include this, define THEIR
// gt_attn_fused_edge_fwd_kernel<T, VEC, LPH, FE_PAD, KVADJ>, and then include gt_attention_fwd_host.h (every other kernel of the
// forward, the launches and the C entry points).  WLayout, kWavesPerBlock and the launch plan come from gt_attention_plan.h.
#pragma once
#include <type_traits>

#include "common.h"
#include "gt_attention_plan.h"

namespace anemoi {

#ifndef ANEMOI_ATTN_MIN_WAVES
#define ANEMOI_ATTN_MIN_WAVES (16 / ANEMOI_ATTN_WPB)
#endif
using f32x2 = __attribute__((ext_vector_type(2))) float;

// <a, b> over a lane's VEC channels.  16-bit types use v_dot2c_f32_{bf16,f16} on the packed pairs as loaded (exact
// products, fp32 accumulation): no per-element conversion of the K row.
template <typename T, int VEC>
__device__ __forceinline__ float dot_rows(const Vec<T, VEC>& a, const Vec<T, VEC>& b) {
  float acc = 0.f;
  if constexpr (sizeof(T) == 2 && (VEC % 2 == 0)) {
    const uint32_t* pa = reinterpret_cast<const uint32_t*>(&a);
    const uint32_t* pb = reinterpret_cast<const uint32_t*>(&b);
#pragma unroll
    for (int i = 0; i < VEC / 2; ++i) {
      if constexpr (std::is_same<T, bf16_t>::value) {
        typedef __attribute__((ext_vector_type(2))) __bf16 bf2;
        acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf2, pa[i]), __builtin_bit_cast(bf2, pb[i]), acc, false);
      } else {
        typedef __attribute__((ext_vector_type(2))) _Float16 h2;
        acc = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, pa[i]), __builtin_bit_cast(h2, pb[i]), acc, false);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc = fmaf(to_float(a.v[i]), to_float(b.v[i]), acc);
  }
  return acc;
}

// Deferred running max: the rescale of the accumulators only runs (wave-uniform branch) when some head's score
// exceeds its running max by more than this; otherwise p = exp(s - m_old) <= e^8 is accumulated directly (fp32
// accumulators; the value after the final division is the same).
constexpr float kDeferThr = 8.0f;

}  // namespace anemoi
