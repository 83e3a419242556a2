// What the window attention's forward and backward share (csrc/window_attention.hip, csrc/window_attention_bwd.hip): the phases of the
// three MFMA kernels, each written once, and the host half of the two entry points.
//
// The skeleton.  A workgroup of four waves owns 64 rows (queries, or keys in the key pass) of one (sequence, head), each wave a strip of
// 16 of them, one row per lane column c.  It streams the tiles of the other side that meet the band of its rows:
//   band arithmetic   win_window, win_band, win_tiles, tile_meets_band, tile_is_full, in_band: plain constexpr integer functions, host and
//                     device.  anemoi_window_attention_plan asks them without a GPU and tests/test_window_attention_plan_cpu.py brute-forces
//                     them against in_band for every block, wave and tile.
//   score             win_score / win_prob (log2 domain, exp2) and plain_score / plain_prob (fp32 kernels, expf): tanh cap and ALiBi once
//   owned rows        load_row_frags: a row as the B operand X[row][8 g + j + 32 s], zeros out of range
//   tile streaming    load_tile_pair (global -> registers, chunk e = tid + 256 u, zeros from `hi` on), store_tile_rows ([ROWS][D + 8]) and
//                     store_tile_transposed ([D][ROWS + 8], a 2-byte scatter); the kernel places its two barriers around the stores
//   the two GEMMs     score_block / score_block_pair (row-major image x owned fragments), accumulate_transposed (transposed image x P or dT)
//   pack_kslot        a lane's values (sb, r = 0..3) -> k slots [sb >> 1][4 (sb & 1) + r], the order transposed_frag reads the image in
//   store_row_frags   acc * factor -> Vec<T, 4> at 16 db + 4 g
// Free function templates over register arrays taken by reference (profiles/r22_gemm_helpers_check.txt on why not structs).
#pragma once
#include <initializer_list>
#include <type_traits>

#include "common.h"
#include "mma.h"

namespace anemoi {

namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr int kWinWaves = 4;
constexpr int kWinOwn = 16 * kWinWaves;  // rows (queries / keys) a workgroup owns
enum WinPass : int32_t { kWinFwd = 0, kWinBwdQuery = 1, kWinBwdKey = 2 };
// rows of a streamed tile: the key pass keeps four LDS images and halves the tile at d = 128 to stay under 48 KB
constexpr int win_tile_rows(int pass, int d) { return pass == kWinBwdKey && d == 128 ? 32 : 64; }

// ---------------------------------------------------------------------------------------------- band arithmetic (no HIP types)
// a window of seq_len - 1 or more covers every key: unbounded (and no band edge such as first + 64 + w can overflow int32)
constexpr int win_window(int window, int seq_len) { return (window < 0 || window >= seq_len - 1) ? -1 : window; }

struct WinBand {
  int lo, hi;  // the rows of the other side that rows [first, first + count) attend: [lo, hi)
};
constexpr WinBand win_band(int first, int count, int w, int N) {
  if (w < 0) return {0, N};
  return {first - w > 0 ? first - w : 0, first + count + w < N ? first + count + w : N};
}
constexpr int win_tiles(const WinBand& b, int rows) { return (b.hi - b.lo + rows - 1) / rows; }
// does tile [t0, t0 + rows) hold a row within w of the wave's strip [s0, s0 + 16)?
constexpr bool tile_meets_band(int t0, int rows, int s0, int w) { return w < 0 || !(t0 > s0 + 15 + w || t0 + rows - 1 < s0 - w); }
// is every (tile row, strip row) pair in the band and the sequence, so that in_band need not be asked?
constexpr bool tile_is_full(int t0, int rows, int s0, int N, int w) {
  return t0 + rows - 1 < N && s0 + 15 < N && (w < 0 || (t0 + rows - 1 - s0 <= w && s0 + 15 - t0 <= w));
}
// THE band: rows i and j of a sequence of N attend each other.  = i < N && j < N && (w < 0 || |i - j| <= w); the distance is asked first
// because that order keeps every kernel's registers at what the inline masks had (profiles/r24_window_attention_helpers_check.txt).
constexpr bool in_band(int i, int j, int N, int w) { return (w < 0 || (i < j ? j - i : i - j) <= w) && i < N && j < N; }

// ---------------------------------------------------------------------------------------------- score
// fp32 kernels: the score of (query i, key j) from the raw dot product, and dT / dS if asked for
__device__ __forceinline__ float plain_score(float dot, int i, int j, float scale, float softcap, float slope, float* dt_ds = nullptr) {
  float s = dot * scale;
  if (dt_ds) *dt_ds = 1.f;
  if (softcap > 0.f) {
    const float th = tanhf(s / softcap);
    s = softcap * th;
    if (dt_ds) *dt_ds = 1.f - th * th;
  }
  return s - slope * (float)abs(i - j);
}
__device__ __forceinline__ float plain_prob(float dot, int i, int j, float lse, float scale, float softcap, float slope, float& dt_ds) {
  return expf(plain_score(dot, i, j, scale, softcap, slope, &dt_ds) - lse);
}
// MFMA kernels: the same score in the log2 domain (sl2e = scale * log2(e); FANCY: softcap and / or ALiBi)
template <bool FANCY>
__device__ __forceinline__ float win_score(float dot, int i, int j, float sl2e, float scale, float softcap, float slope,
                                           float* dt_ds = nullptr) {
  if constexpr (FANCY) return plain_score(dot, i, j, scale, softcap, slope, dt_ds) * kLog2e;
  if (dt_ds) *dt_ds = 1.f;
  return dot * sl2e;
}
// p = exp(s - lse) with lse2 = lse * log2(e)
template <bool FANCY>
__device__ __forceinline__ float win_prob(float dot, int i, int j, float lse2, float sl2e, float scale, float softcap, float slope,
                                          float& dt_ds) {
  return __builtin_amdgcn_exp2f(win_score<FANCY>(dot, i, j, sl2e, scale, softcap, slope, &dt_ds) - lse2);
}

// ---------------------------------------------------------------------------------------------- MFMA phases
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

template <typename T>
__device__ __forceinline__ short to_bits(float x) {
  return (short)__builtin_bit_cast(uint16_t, from_float<T>(x));
}

// where a lane stands: (sequence b, head h) of blockIdx.y, the workgroup's first owned row, the wave's strip and the lane's own row
struct WinLane {
  int h, tid, g, c, first, strip, own;
  int64_t row0;  // first row of the sequence
};
__device__ __forceinline__ WinLane win_lane(int N, int H) {
  WinLane p;
  const int bh = blockIdx.y, b = bh / H, lane = threadIdx.x & 63;
  p.h = bh - b * H, p.tid = threadIdx.x, p.g = lane >> 4, p.c = lane & 15;
  p.first = blockIdx.x * kWinOwn, p.strip = p.first + 16 * (p.tid >> 6), p.own = p.strip + p.c;
  p.row0 = (int64_t)b * N;
  return p;
}

// row `row` of a strided operand as B-operand fragments X[row][col0 + 32 s .. + 7] (col0 = h D + 8 g); zeros if the row is out of range
template <typename T, int D>
__device__ __forceinline__ void load_row_frags(frag8 (&f)[D / 32], const void* x, int64_t ld, int64_t row, int64_t col0, bool in_range) {
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
    if (in_range)
      f[s] = *reinterpret_cast<const frag8*>((const T*)x + row * ld + col0 + 32 * s);
    else
      f[s] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
  }
}

// 16-byte chunks per thread of a [ROWS][D] tile: chunk e = tid + 256 u is (row e / (D / 8), 8 columns at 8 (e % (D / 8)))
template <int ROWS, int D>
constexpr int tile_loads() {
  static_assert(ROWS * (D / 8) % (64 * kWinWaves) == 0 && ROWS * (D / 8) >= 64 * kWinWaves, "tile loads");
  return ROWS * (D / 8) / (64 * kWinWaves);
}

// global -> registers: rows [t0, t0 + ROWS) of two operands of the sequence that begins at row row0, columns from col0 = h D; rows from
// `hi` on are zeros.  One bounds test serves both operands: every kernel streams two.
template <typename T, int ROWS, int D, int LOADS>
__device__ __forceinline__ void load_tile_pair(frag8 (&xr)[LOADS], frag8 (&yr)[LOADS], const T* x, int64_t ldx, const T* y, int64_t ldy, int64_t row0,
                                               int64_t col0, int t0, int hi, int tid) {
  static_assert(LOADS == tile_loads<ROWS, D>(), "tile registers");
#pragma unroll
  for (int u = 0; u < LOADS; ++u) {
    const int e = tid + u * 64 * kWinWaves, row = t0 + e / (D / 8), col = 8 * (e % (D / 8));
    if (row < hi) {
      xr[u] = *reinterpret_cast<const frag8*>(x + (row0 + row) * ldx + col0 + col);
      yr[u] = *reinterpret_cast<const frag8*>(y + (row0 + row) * ldy + col0 + col);
    } else {
      xr[u] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
      yr[u] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
}
// registers -> the row-major LDS image [ROWS][D + 8] (16 B of padding against bank conflicts): the A operand of score_block
template <int ROWS, int D, int LOADS>
__device__ __forceinline__ void store_tile_rows(uint16_t* img, const frag8 (&reg)[LOADS], int tid) {
  static_assert(LOADS == tile_loads<ROWS, D>(), "tile registers");
#pragma unroll
  for (int u = 0; u < LOADS; ++u) {
    const int e = tid + u * 64 * kWinWaves;
    *reinterpret_cast<frag8*>(img + (e / (D / 8)) * (D + 8) + 8 * (e % (D / 8))) = reg[u];
  }
}
// registers -> the transposed LDS image [D][ROWS + 8]: the A operand of accumulate_transposed
template <int ROWS, int D, int LOADS>
__device__ __forceinline__ void store_tile_transposed(uint16_t* img, const frag8 (&reg)[LOADS], int tid) {
  static_assert(LOADS == tile_loads<ROWS, D>(), "tile registers");
#pragma unroll
  for (int u = 0; u < LOADS; ++u) {
    const int e = tid + u * 64 * kWinWaves, row = e / (D / 8), col = 8 * (e % (D / 8));
#pragma unroll
    for (int x = 0; x < 8; ++x) img[(col + x) * (ROWS + 8) + row] = (uint16_t)reg[u][x];
  }
}

// [tile row 16 sb + 4 g + r][owned row c] of (tile) (owned rows)^T: the A operand from the row-major image
template <typename T, int D>
__device__ __forceinline__ f32x4 score_block(const uint16_t* img, int sb, const frag8 (&own)[D / 32], int g, int c) {
  f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < D / 32; ++s) z = mfma16<T>(*reinterpret_cast<const frag8*>(img + (16 * sb + c) * (D + 8) + 8 * g + 32 * s), own[s], z);
  return z;
}

// two score blocks of one tile row strip at once, their MFMAs in turn: the backward passes' S and dP.  score_block twice (two dependent
// chains) measured 0.8 - 1.5 % slower in the key pass.
template <typename T, int D>
__device__ __forceinline__ void score_block_pair(f32x4& x, f32x4& y, const uint16_t* ximg, const uint16_t* yimg, int sb, const frag8 (&xown)[D / 32],
                                                 const frag8 (&yown)[D / 32], int g, int c) {
  x = f32x4{0.f, 0.f, 0.f, 0.f}, y = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
    const frag8 xa = *reinterpret_cast<const frag8*>(ximg + (16 * sb + c) * (D + 8) + 8 * g + 32 * s);
    const frag8 ya = *reinterpret_cast<const frag8*>(yimg + (16 * sb + c) * (D + 8) + 8 * g + 32 * s);
    x = mfma16<T>(xa, xown[s], x);
    y = mfma16<T>(ya, yown[s], y);
  }
}

// the lane's four values of tile rows 16 sb + 4 g .. + 3 into the k slots accumulate_transposed contracts them from: value (sb, r) goes to
// [sb >> 1][4 (sb & 1) + r].  Four at a time on purpose: converted one by one, the fp16 query pass fused each product with its conversion
// (v_fma_mixlo_f16, one rounding where the pair of v_mul_f32 and v_cvt_pk_f16_f32 has two) and dq lost bit-equality.
template <typename T, int NF>
__device__ __forceinline__ void pack_kslot(frag8 (&f)[NF], int sb, const f32x4& x) {
#pragma unroll
  for (int r = 0; r < 4; ++r) f[sb >> 1][4 * (sb & 1) + r] = to_bits<T>(x[r]);
}

// The A operand of a GEMM whose contraction runs over the rows of a tile, from the tile's transposed LDS image [d][tile rows]: row `row`,
// k step s, in the k order of the lanes that hold the B operand (k slot 8g + j = tile row 32 s + 16 (j / 4) + 4 g + j % 4).
__device__ __forceinline__ frag8 transposed_frag(const uint16_t* img, int stride, int row, int s, int g) {
  const uint16_t* r = img + row * stride + 32 * s + 4 * g;
  const u32x2 lo4 = *reinterpret_cast<const u32x2*>(r);
  const u32x2 hi4 = *reinterpret_cast<const u32x2*>(r + 16);
  return __builtin_bit_cast(frag8, u32x4{lo4.x, lo4.y, hi4.x, hi4.y});
}
// acc^T[d 16 db + 4 g + r][owned row c] += X^T[d][tile rows] P[tile rows][owned row], P packed by pack_kslot.  The k step is the outer
// loop (each block still sums its steps in order): with the blocks outside, one forward instantiation took 4 VGPRs more.
template <typename T, int ROWS, int D>
__device__ __forceinline__ void accumulate_transposed(f32x4 (&acc)[D / 16], const uint16_t* img, const frag8 (&pf)[ROWS / 32], int g, int c) {
#pragma unroll
  for (int s = 0; s < ROWS / 32; ++s) {
#pragma unroll
    for (int db = 0; db < D / 16; ++db) acc[db] = mfma16<T>(transposed_frag(img, ROWS + 8, 16 * db + c, s, g), pf[s], acc[db]);
  }
}

// the lane's four columns 16 db + 4 g .. + 3 of every block of its owned row (x: at column h D of that row), acc * factor
template <typename T, int D>
__device__ __forceinline__ void store_row_frags(T* x, const f32x4 (&acc)[D / 16], float factor, int g) {
#pragma unroll
  for (int db = 0; db < D / 16; ++db) {
    Vec<T, 4> o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o.v[r] = from_float<T>(acc[db][r] * factor);
    *reinterpret_cast<Vec<T, 4>*>(x + 16 * db + 4 * g) = o;
  }
}

// ---------------------------------------------------------------------------------------------- host
struct WinOperand {
  const void* p;
  int64_t ld;
};
// What both entry points ask of their arguments; `fn` is the entry point's name in the messages.  An empty call (no rows) is not asked
// about leading dimensions or scale.  Order: these run before the entry points' own checks (null pointers, `passes`), so a call wrong
// in two ways can name another fault than it did when each entry point carried its own list.
inline int win_check_args(const char* fn, int batch, int seq_len, int H, int d, anemoi_dtype_t dtype, std::initializer_list<int64_t> lds,
                          float scale) {
  ANEMOI_REQUIRE(batch >= 0 && seq_len >= 0 && H > 0 && d > 0, "%s: bad sizes batch=%d seq_len=%d H=%d d=%d", fn, batch, seq_len, H, d);
  if (d != 32 && d != 64 && d != 128) {
    set_error("%s: head dimension %d not supported; supported: 32, 64, 128", fn, d);
    return ANEMOI_E_UNSUPPORTED;
  }
  ANEMOI_REQUIRE(dtype == ANEMOI_F32 || dtype == ANEMOI_BF16 || dtype == ANEMOI_F16, "%s: bad dtype %d", fn, (int)dtype);
  ANEMOI_REQUIRE((int64_t)batch * H < 65536, "%s: batch * H = %lld too large", fn, (long long)batch * H);
  if (batch == 0 || seq_len == 0) return ANEMOI_OK;
  for (int64_t ld : lds) ANEMOI_REQUIRE(ld >= (int64_t)H * d, "%s: leading dimension smaller than H*d=%lld", fn, (long long)H * d);
  ANEMOI_REQUIRE(scale > 0.f, "%s: scale must be positive", fn);
  return ANEMOI_OK;
}
// rows that vectors of `elems` 16-bit elements can be moved from or to: the pointer and the leading dimension
inline bool win_rows_aligned(std::initializer_list<WinOperand> operands, int elems) {
  for (const WinOperand& o : operands)
    if ((uintptr_t)o.p % (2 * elems) != 0 || o.ld % elems != 0) return false;
  return true;
}
// f(T{}, integral_constant D, bool_constant FANCY) for a 16-bit dtype, a supported head dimension and the softcap / ALiBi switch
template <typename F>
int with_win_instance(anemoi_dtype_t dtype, int d, bool fancy, F&& f) {
  auto dims = [&](auto t, auto fancy_c) {
    switch (d) {
      case 32: return f(t, std::integral_constant<int, 32>{}, fancy_c);
      case 64: return f(t, std::integral_constant<int, 64>{}, fancy_c);
      default: return f(t, std::integral_constant<int, 128>{}, fancy_c);
    }
  };
  auto types = [&](auto fancy_c) { return dtype == ANEMOI_BF16 ? dims(bf16_t{}, fancy_c) : dims(f16_t{}, fancy_c); };
  return fancy ? types(std::true_type{}) : types(std::false_type{});
}

}  // namespace

}  // namespace anemoi
