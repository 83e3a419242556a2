// What rowwise.hip and rowwise_bwd.hip share: the register-resident row (one wave64 per row, a lane owns VEC contiguous elements of
// every 64*VEC-column chunk, CH chunks), the host rule that picks (VEC, CH) for a launch, and the dispatchers that turn the picked
// runtime values into template arguments.  tests/test_rowwise_backward_gpu.py::_path restates pick_vec / pick_chunks.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "common.h"

namespace anemoi {

constexpr int kMaxChunks = 8;  // register-resident chunks per lane (template CH): D <= 64*VEC*CH

// Load a row into registers as float: x[lane*VEC + t*64*VEC + j], t < nchunks.
template <typename T, int VEC, int CH>
__device__ __forceinline__ void load_row(const T* __restrict__ p, int D, int lane, float (&r)[CH][VEC]) {
#pragma unroll
  for (int t = 0; t < CH; ++t) {
    const int c = (t * 64 + lane) * VEC;
    if (c < D) {
      load_vec<T, VEC>(p + c, r[t]);
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) r[t][j] = 0.f;
    }
  }
}

template <typename T, int VEC, int CH>
__device__ __forceinline__ void store_row(T* __restrict__ p, int D, int lane, const float (&r)[CH][VEC]) {
#pragma unroll
  for (int t = 0; t < CH; ++t) {
    const int c = (t * 64 + lane) * VEC;
    if (c < D) store_vec<T, VEC>(p + c, r[t]);
  }
}

// Pick the widest vector width (in elements) such that rows stay 16-byte-or-narrower aligned and D % VEC == 0.
template <typename T>
inline int pick_vec(int D, std::initializer_list<int64_t> lds, std::initializer_list<const void*> ptrs) {
  int vec = 16 / (int)sizeof(T);  // 16-byte accesses
  auto ok = [&](int v) {
    if (D % v) return false;
    for (int64_t ld : lds)
      if (ld % v) return false;
    for (const void* p : ptrs)
      if (p && (reinterpret_cast<uintptr_t>(p) % (v * sizeof(T)))) return false;
    return true;
  };
  while (vec > 1 && !ok(vec)) vec >>= 1;
  return vec;
}

// smallest power-of-two chunk count covering D, or 0 if the row does not fit in registers
inline int pick_chunks(int D, int vec) {
  for (int ch = 1; ch <= kMaxChunks; ch *= 2)
    if (D <= 64 * vec * ch) return ch;
  return 0;
}

// Runtime vec in {1, 2, 4, 8} -> f(std::integral_constant<int, vec>): in f, `V()` is a template argument.  Returns false, without
// calling f, for any other value: the caller words the error.  f is instantiated for all four widths whatever the element type, so
// a kernel keeps its <float, 8> instantiations although pick_vec never selects them.
template <int... Vs, typename F>
inline bool dispatch_one_of(int v, F&& f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

template <typename F>
inline bool dispatch_vec(int vec, F&& f) {
  return dispatch_one_of<1, 2, 4, 8>(vec, f);
}

// Runtime (vec, chunks) in {1, 2, 4, 8}^2 -> f(integral_constant vec, integral_constant chunks); false for anything else.
template <typename F>
inline bool dispatch_vec_chunks(int vec, int ch, F&& f) {
  bool hit = false;
  dispatch_vec(vec, [&](auto V) { hit = dispatch_one_of<1, 2, 4, 8>(ch, [&](auto C) { f(V, C); }); });
  return hit;
}

}  // namespace anemoi
