// What the window attention's forward and backward kernels share (csrc/window_attention.hip, csrc/window_attention_bwd.hip): the operand
// types of mfma_f32_16x16x32 and the conversions around it.
#pragma once
#include "common.h"
#include "mma.h"

namespace anemoi {

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

template <typename T>
__device__ __forceinline__ short to_bits(float x) {
  return (short)__builtin_bit_cast(uint16_t, from_float<T>(x));
}

// The A operand of a GEMM whose contraction runs over the rows of a tile, from the tile's transposed LDS image [d][tile rows]: row `row`,
// k step s, in the k order of the lanes that hold the B operand (k slot 8g + j = tile row 32 s + 16 (j / 4) + 4 g + j % 4).
__device__ __forceinline__ frag8 transposed_frag(const uint16_t* img, int stride, int row, int s, int g) {
  const uint16_t* r = img + row * stride + 32 * s + 4 * g;
  const u32x2 lo4 = *reinterpret_cast<const u32x2*>(r);
  const u32x2 hi4 = *reinterpret_cast<const u32x2*>(r + 16);
  return __builtin_bit_cast(frag8, u32x4{lo4.x, lo4.y, hi4.x, hi4.y});
}

}  // namespace

}  // namespace anemoi
