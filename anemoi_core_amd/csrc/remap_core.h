// The element-wise maps of the remapper (reference preprocessing/remapper.py + mappings.py), one device function shared by the stand-alone
// kernel (remap_columns_kernel) and the ordered output column program (kinds >= 16 of column_program: kind = 16 + op).
//
// The reference evaluates every map as a SEQUENCE of in-place torch ops on the column, so each op rounds to the data dtype (16-bit types
// compute in fp32 and round after every op) and fp32 never sees an FMA; rnd<T> is that rounding.  torch's scalar pow takes exponent 0.5 as
// sqrt, 2 as x * x, 3 as x * x * x and 1 as a copy: the host encodes which in the flags (bits 4..7).  Clamps are comparisons, never
// fmaxf / fminf, so a NaN stays a NaN through every op, as through torch.clamp; a lower clamp tests <=, so that -0.0 under a bound of 0.0
// becomes +0.0 as through the max of torch's device clamp.  A division by a SCALAR is, in torch's device kernels, a
// multiplication by the scalar's fp32 reciprocal: the tables carry that reciprocal (the host forms it, 1.f / float(divisor)).
#pragma once
#include "common.h"

namespace anemoi {

enum RemapOp : int {
  REMAP_NONE = 0,
  REMAP_LOG1P = 1,       // log1p(x)
  REMAP_EXPM1 = 2,       // expm1(x)
  REMAP_POWER = 3,       // p0 = lambda, p1 = 1 - lambda: [clip | count x < 0]; x^lambda, or lambda x + (1 - lambda) where the power is > 1 (tangent)
  REMAP_POWER_INV = 4,   // p0 = 1 / lambda (exponent), p1 = 1 - lambda, p2 = rcp(lambda): clamp(min 0)^p0, or (x - p1) p2 where that is > 1
  REMAP_BOXCOX = 5,      // p0 = lambda != 0, p1 = rcp(lambda): [clip | count x < 0]; ((x^lambda) - 1) p1
  REMAP_BOXCOX_INV = 6,  // p0 = lambda, p1 = 1 / lambda: clamp(x lambda + 1, min 0)^(1 / lambda)
  REMAP_LOG = 7,         // boxcox with lambda = 0: count x <= 0; log(x)
  REMAP_EXP = 8,
  REMAP_ATANH = 9,       // p0 = tanh(rho), p1 = rcp(rho): atanh(((2 x) - 1) p0) p1
  REMAP_ATANH_INV = 10,  // p0 = rcp(tanh(rho)), p1 = rho: clamp((tanh(x p1) p0 + 1) 0.5, 0, 1)
  REMAP_ASINH = 11,      // p0 = c: asinh(x c)
  REMAP_ASINH_INV = 12,  // p0 = rcp(c): sinh(x) p0
  REMAP_DISPLACE = 13,   // x <= p0 -> p1 (lower), THEN x >= p2 -> p3 (upper); p0 = lower atom + eps, p2 = upper atom - eps
  REMAP_CLAMP = 14,      // p0 = lower, p1 = upper (flags say which exist)
  REMAP_AFFINE = 15,     // p0 = scale, p1 = shift: x scale, then + shift
  REMAP_AFFINE_INV = 16  // p0 = rcp(scale), p1 = shift: (x - shift) p0
};

constexpr int kRemapClip = 1, kRemapTangent = 2, kRemapLower = 4, kRemapUpper = 8;  // flags; bits 4..7: how pow is taken (remap_pow)

// One torch op's rounding: the value is pinned in a VGPR (no FMA contraction across it, no fused fp16 conversion - see mul_f32 in
// model_edge.hip), then rounded to T and widened again.
template <typename T>
__device__ __forceinline__ float rnd(float t) {
  asm("" : "+v"(t));
  if constexpr (sizeof(T) == 4)
    return t;
  else
    return to_float(from_float<T>(t));
}

__device__ __forceinline__ float remap_pow(float v, float e, int mode) {
  switch (mode) {
    case 1: return sqrtf(v);
    case 2: return v * v;
    case 3: return v * v * v;
    case 4: return v;
    default: return powf(v, e);
  }
}

// v: the element as fp32 (exact for every T).  `bad` is set where the reference's forward domain assertion would fail (x >= 0, or x > 0 for
// the logarithm, both false for NaN, as the reference's `.all()` has it); the result is what torch computes without the assertion.
template <typename T>
__device__ __forceinline__ float remap_apply(float v, int op, int flags, float p0, float p1, float p2, float p3, bool& bad) {
  const int mode = (flags >> 4) & 15;
  switch (op) {
    case REMAP_LOG1P: return rnd<T>(log1pf(v));
    case REMAP_EXPM1: return rnd<T>(expm1f(v));
    case REMAP_POWER: {
      if (flags & kRemapClip)
        v = v <= 0.f ? 0.f : v;
      else
        bad = !(v >= 0.f);
      const float pw = rnd<T>(remap_pow(v, p0, mode));
      if (!(flags & kRemapTangent)) return pw;
      const float lin = rnd<T>(rnd<T>(v * p0) + p1);
      return pw > 1.f ? lin : pw;  // the reference tests the tensor pow_ has already overwritten
    }
    case REMAP_POWER_INV: {
      const float lin = rnd<T>(rnd<T>(v - p1) * p2);
      v = v <= 0.f ? 0.f : v;
      const float pw = rnd<T>(remap_pow(v, p0, mode));
      return ((flags & kRemapTangent) && pw > 1.f) ? lin : pw;
    }
    case REMAP_BOXCOX: {
      if (flags & kRemapClip)
        v = v <= 0.f ? 0.f : v;
      else
        bad = !(v >= 0.f);
      return rnd<T>(rnd<T>(rnd<T>(remap_pow(v, p0, mode)) - 1.f) * p1);
    }
    case REMAP_BOXCOX_INV: {
      float t = rnd<T>(rnd<T>(v * p0) + 1.f);
      t = t <= 0.f ? 0.f : t;
      return rnd<T>(remap_pow(t, p1, mode));
    }
    case REMAP_LOG: bad = !(v > 0.f); return rnd<T>(logf(v));
    case REMAP_EXP: return rnd<T>(expf(v));
    case REMAP_ATANH: {
      float t = rnd<T>(v * 2.f);
      t = rnd<T>(t - 1.f);
      t = rnd<T>(t * p0);
      t = rnd<T>(atanhf(t));
      return rnd<T>(t * p1);
    }
    case REMAP_ATANH_INV: {
      float t = rnd<T>(v * p1);
      t = rnd<T>(tanhf(t));
      t = rnd<T>(t * p0);
      t = rnd<T>(t + 1.f);
      t = rnd<T>(t * 0.5f);
      if (t <= 0.f) t = 0.f;
      if (t > 1.f) t = 1.f;
      return t;
    }
    case REMAP_ASINH: return rnd<T>(asinhf(rnd<T>(v * p0)));
    case REMAP_ASINH_INV: return rnd<T>(rnd<T>(sinhf(v)) * p0);
    case REMAP_DISPLACE:
      if ((flags & kRemapLower) && v <= p0) v = p1;
      if ((flags & kRemapUpper) && v >= p2) v = p3;
      return v;
    case REMAP_CLAMP:
      if ((flags & kRemapLower) && v <= p0) v = p0;
      if ((flags & kRemapUpper) && v > p1) v = p1;
      return v;
    case REMAP_AFFINE: return rnd<T>(rnd<T>(v * p0) + p1);
    case REMAP_AFFINE_INV: return rnd<T>(rnd<T>(v - p1) * p0);
    default: return v;
  }
}

}  // namespace anemoi
