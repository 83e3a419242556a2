// The matrix-core primitives every MFMA kernel of the library uses (linear.hip, wgrad.hip, the chain kernels through chain_core.h,
// the window attention through window_attention_core.h): the operand / accumulator register types of v_mfma_f32_16x16x32_{bf16,f16},
// the instruction itself selected by the element type, and the address-space pointer types of the LDS-DMA builtin.
#pragma once
#include "common.h"

namespace anemoi {

using frag8 = __attribute__((ext_vector_type(8))) short;  // 8 x 16-bit operand elements (4 VGPRs)
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;

// D = A B + C on one 16 x 16 tile, 32 deep: lane l holds row (l & 15), k = 8 (l >> 4) .. + 7 of both operands and 4 rows
// 4 (l >> 4) .. + 3 of column (l & 15) of the result.  The operands are taken by const reference on purpose: by value, the
// window-attention backward kernels (whose own copy took references) compile to different code; the kernels that passed values
// compile to the same code either way.
template <typename T>
__device__ __forceinline__ f32x4 mfma16(const frag8& a, const frag8& b, const f32x4& c);
template <>
__device__ __forceinline__ f32x4 mfma16<bf16_t>(const frag8& a, const frag8& b, const f32x4& c) {
  using bf8 = __attribute__((ext_vector_type(8))) __bf16;
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4 mfma16<f16_t>(const frag8& a, const frag8& b, const f32x4& c) {
  using h8 = __attribute__((ext_vector_type(8))) _Float16;
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

// source and destination of __builtin_amdgcn_global_load_lds (global -> LDS without a register round trip)
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

}  // namespace anemoi
