// Spherical-harmonic transforms on a grid of latitude rings (regular or reduced), two launches per direction, and the row-wise combine of
// the spectral Ornstein residual.  The reference (layers/spectral_helpers.py:109-553) runs one torch.fft.rfft / irfft launch PER RING on a
// reduced grid (:261-262, :472-475; 192 launches at O96) between a transposing copy and two einsums over a dense [m, l, k] table.
//
//   forward   ring kernel      X[f, k, m] = (2 pi / n_k) sum_j x[f, s_k + j] e^{-2 pi i ((j m) mod n_k) / n_k}   m <= n_k / 2, else 0
//             Legendre kernel  c[f, l, m] = sum_k X[f, k, m] W[l, k, m]                                           l >= m, else 0
//   inverse   Legendre kernel  Y[f, k, m] = sum_{l >= m} c[f, l, m] lscale[f % S, l] P[l, k, m]                   m <= n_k / 2
//             ring kernel      y[f, s_k + j] = Re Y_0 + sum_{1 <= m < n_k / 2, m < M} 2 Re(Y_m e^{+2 pi i ((j m) mod n_k) / n_k})
//                                              (+ Re Y_{n_k / 2} (-1)^j for even n_k with n_k / 2 < M)            = irfft(., n_k, "forward")
//
// Everything is fp32 with fp32 accumulation in a fixed order (no atomics: bitwise reproducible).  Twiddles e^{-2 pi i t / n_k}, t < n_k, come
// from a table the caller built in float64 (ring k's at [s_k, s_k + n_k), like its points) and are indexed with the INTEGER (j m) mod n_k,
// kept by addition: no sin / cos is evaluated here.  The Legendre tables are laid out [l, k, m], m fastest: a wave's 64 lanes are 64 adjacent
// modes, so the table, the ring spectra [f, k, m] and the coefficients [f, l, m] are all read and written in contiguous 256 / 512 byte runs.
// The grid side is addressed in place: field f = (g, c) of `n_groups` x `n_cols` lives at base + g * gs + cols[c] + point * ps, which is
// column cols[c] of a [G, grid, V] tensor (gs = grid V, ps = V) or row f of a [F, grid] one (gs = grid, ps = 1, n_cols = 1).
//
// Tiling, LDS bound and grids: sht_plan.h.  What was measured: DESIGN.md, the section on the spherical-harmonic transforms.
#include <type_traits>

#include "common.h"
#include "sht_plan.h"

namespace anemoi {
namespace {

struct GridSide {
  float* base;  // read-only for the forward
  int64_t gs, ps;
  const int32_t* cols;
  int32_t n_cols;
};

struct ShtArgs {
  GridSide g;
  const int32_t* ring_off;  // [K + 1]
  const float2* tw;         // [grid]
  const float* table;       // [L, K, M]
  float2* spec;             // ring spectra [F, K, M] (workspace)
  float2* coeffs;           // [F, L, M]
  const float* lscale;      // [S, L] or null
  int32_t n_scale;
  int32_t F, K, M, chunk;
};

__device__ __forceinline__ int64_t field_offset(const GridSide& g, int f) {
  const int grp = f / g.n_cols, c = f - grp * g.n_cols;
  return (int64_t)grp * g.gs + (g.cols ? g.cols[c] : c);
}

// ------------------------------------------------------------------------------------------------------------- forward: ring DFTs
template <int FT>
__global__ __launch_bounds__(kShtRingThreads) void sht_ring_fwd_kernel(ShtArgs a) {
  extern __shared__ float sx[];  // [chunk][FT]: a pass of the ring's points, FT fields each (read as a broadcast by every lane)
  __shared__ int64_t foff[FT];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int m = blockIdx.y * kShtRingThreads + tid;
  const int f0 = blockIdx.z * FT;
  const int s = a.ring_off[k], n = a.ring_off[k + 1] - s;
  if (tid < FT) foff[tid] = f0 + tid < a.F ? field_offset(a.g, f0 + tid) : -1;
  const bool active = m < a.M, live = active && m <= n / 2;
  const float2* __restrict__ tw = a.tw + s;
  float re[FT], im[FT];
#pragma unroll
  for (int t = 0; t < FT; ++t) re[t] = im[t] = 0.f;
  int idx = 0;  // (j m) mod n
  for (int j0 = 0; j0 < n; j0 += a.chunk) {
    const int cn = min(a.chunk, n - j0);
    __syncthreads();  // the previous pass is consumed (and foff is written)
    for (int e = tid; e < cn * FT; e += kShtRingThreads) {
      int j, t;
      if (a.g.ps == 1) {  // field-contiguous: adjacent lanes read adjacent points
        t = e / cn, j = e - t * cn;
      } else {  // point-major: adjacent lanes read the tile's columns of one point
        j = e / FT, t = e - j * FT;
      }
      const int64_t o = foff[t];
      sx[j * FT + t] = o >= 0 ? a.g.base[o + (int64_t)(s + j0 + j) * a.g.ps] : 0.f;
    }
    __syncthreads();
    if (live) {
      for (int j = 0; j < cn; ++j) {
        const float2 w = tw[idx];
#pragma unroll
        for (int t = 0; t < FT; ++t) {
          const float v = sx[j * FT + t];
          re[t] = fmaf(v, w.x, re[t]);
          im[t] = fmaf(v, w.y, im[t]);
        }
        idx += m;
        if (idx >= n) idx -= n;
      }
    }
  }
  if (!active) return;
  const float scale = live ? (float)(6.283185307179586476925286766559 / (double)n) : 0.f;
#pragma unroll
  for (int t = 0; t < FT; ++t)
    if (f0 + t < a.F) a.spec[((int64_t)(f0 + t) * a.K + k) * a.M + m] = make_float2(re[t] * scale, im[t] * scale);
}

// ------------------------------------------------------------------------------------------------------------- forward: Legendre step
// A thread owns mode m and kShtLegFwdPerThread adjacent degrees (1: more per thread measured slower, sht_plan.h).
template <int FT>
__global__ __launch_bounds__(64 * kShtLegWaves) void sht_leg_fwd_kernel(ShtArgs a) {
  constexpr int R = kShtLegFwdPerThread;
  const int m = blockIdx.x * 64 + (threadIdx.x & 63);
  const int l0 = (blockIdx.y * kShtLegWaves + (threadIdx.x >> 6)) * R;
  const int f0 = blockIdx.z * FT;
  if (m >= a.M || l0 >= a.M) return;
  float re[R][FT], im[R][FT];
  const float2* xp[FT];
#pragma unroll
  for (int t = 0; t < FT; ++t) {
#pragma unroll
    for (int r = 0; r < R; ++r) re[r][t] = im[r][t] = 0.f;
    xp[t] = a.spec + (int64_t)min(f0 + t, a.F - 1) * a.K * a.M + m;
  }
  const int64_t row = (int64_t)a.K * a.M;
  int lr[R];  // rows past the table's end read its last row and are not written
#pragma unroll
  for (int r = 0; r < R; ++r) lr[r] = min(l0 + r, a.M - 1);
  if (l0 + R - 1 >= m) {  // W[l, k, m] = 0 for l < m: a thread whose degrees are all below m does no work
    const float* __restrict__ wp = a.table + m;
    for (int k = 0; k < a.K; ++k) {
      float w[R];
#pragma unroll
      for (int r = 0; r < R; ++r) w[r] = wp[lr[r] * row + (int64_t)k * a.M];
#pragma unroll
      for (int t = 0; t < FT; ++t) {
        const float2 v = xp[t][(int64_t)k * a.M];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          re[r][t] = fmaf(v.x, w[r], re[r][t]);
          im[r][t] = fmaf(v.y, w[r], im[r][t]);
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int l = l0 + r;
    if (l >= a.M) break;
    const bool zero = l < m;  // written as exact zeros, whatever the spectra hold
#pragma unroll
    for (int t = 0; t < FT; ++t)
      if (f0 + t < a.F) a.coeffs[((int64_t)(f0 + t) * a.M + l) * a.M + m] = zero ? make_float2(0.f, 0.f) : make_float2(re[r][t], im[r][t]);
  }
}

// ------------------------------------------------------------------------------------------------------------- inverse: Legendre step
// A thread owns mode m and kShtLegInvPerThread adjacent rings: the coefficients c[f, l, m] are loaded once for all of them.
template <int FT>
__global__ __launch_bounds__(64 * kShtLegWaves) void sht_leg_inv_kernel(ShtArgs a) {
  constexpr int R = kShtLegInvPerThread;
  const int m = blockIdx.x * 64 + (threadIdx.x & 63);
  const int k0 = (blockIdx.y * kShtLegWaves + (threadIdx.x >> 6)) * R;
  const int f0 = blockIdx.z * FT;
  if (m >= a.M || k0 >= a.K) return;
  int kr[R];
  bool need[R];  // the ring step never reads modes past n_k / 2
  bool any = false;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    kr[r] = min(k0 + r, a.K - 1);
    need[r] = k0 + r < a.K && m <= (a.ring_off[kr[r] + 1] - a.ring_off[kr[r]]) / 2;
    any = any || need[r];
  }
  if (!any) return;
  float re[R][FT], im[R][FT];
  const float2* cp[FT];
  const float* sp[FT];
#pragma unroll
  for (int t = 0; t < FT; ++t) {
#pragma unroll
    for (int r = 0; r < R; ++r) re[r][t] = im[r][t] = 0.f;
    const int f = min(f0 + t, a.F - 1);
    cp[t] = a.coeffs + (int64_t)f * a.M * a.M + m;
    sp[t] = a.lscale ? a.lscale + (int64_t)(f % a.n_scale) * a.M : nullptr;
  }
  const float* __restrict__ pp = a.table + m;
  const int64_t row = (int64_t)a.K * a.M;
  // from the tile's first mode on, for the whole wave: P[l, k, m] = 0 where l < m, so those terms add exact zeros
  for (int l = blockIdx.x * 64; l < a.M; ++l) {
    float p[R];
#pragma unroll
    for (int r = 0; r < R; ++r) p[r] = pp[l * row + (int64_t)kr[r] * a.M];
#pragma unroll
    for (int t = 0; t < FT; ++t) {
      float2 c = cp[t][(int64_t)l * a.M];
      if (sp[t]) {
        const float sc = sp[t][l];
        c.x *= sc, c.y *= sc;
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        re[r][t] = fmaf(c.x, p[r], re[r][t]);
        im[r][t] = fmaf(c.y, p[r], im[r][t]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (!need[r]) continue;
#pragma unroll
    for (int t = 0; t < FT; ++t)
      if (f0 + t < a.F) a.spec[((int64_t)(f0 + t) * a.K + k0 + r) * a.M + m] = make_float2(re[r][t], im[r][t]);
  }
}

// ------------------------------------------------------------------------------------------------------------- inverse: ring synthesis
template <int FT>
__global__ __launch_bounds__(kShtRingThreads) void sht_ring_inv_kernel(ShtArgs a) {
  extern __shared__ float sx[];
  float2* sy = reinterpret_cast<float2*>(sx);  // [chunk][FT]: a pass of the ring's modes, FT fields each
  __shared__ int64_t foff[FT];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int s = a.ring_off[k], n = a.ring_off[k + 1] - s;
  if ((int)(blockIdx.y * kShtRingThreads) >= n) return;  // the whole workgroup lies past this ring's end
  const int j = blockIdx.y * kShtRingThreads + tid;
  const int f0 = blockIdx.z * FT;
  if (tid < FT) foff[tid] = f0 + tid < a.F ? field_offset(a.g, f0 + tid) : -1;
  const bool live = j < n;
  const int mtop = min(a.M, n / 2 + 1);  // modes beyond n / 2 are dropped, fewer are zero-extended
  const float2* __restrict__ tw = a.tw + s;
  float acc[FT];
#pragma unroll
  for (int t = 0; t < FT; ++t) acc[t] = 0.f;
  int idx = 0;  // (j m) mod n
  for (int m0 = 0; m0 < mtop; m0 += a.chunk) {
    const int cn = min(a.chunk, mtop - m0);
    __syncthreads();
    for (int e = tid; e < cn * FT; e += kShtRingThreads) {
      const int t = e / cn, mm = e - t * cn;
      sy[mm * FT + t] = f0 + t < a.F ? a.spec[((int64_t)(f0 + t) * a.K + k) * a.M + m0 + mm] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    if (live) {
      for (int mm = 0; mm < cn; ++mm) {
        const int m = m0 + mm;
        const bool real_mode = m == 0 || 2 * m == n;  // mode 0 and the Nyquist mode: counted once, imaginary part ignored
        float2 w = tw[idx];
        if (real_mode) w = make_float2(m == 0 ? 1.f : ((j & 1) ? -1.f : 1.f), 0.f);
        const float c = real_mode ? 1.f : 2.f;
#pragma unroll
        for (int t = 0; t < FT; ++t) {
          const float2 y = sy[mm * FT + t];
          acc[t] = fmaf(c, fmaf(y.x, w.x, y.y * w.y), acc[t]);  // w = (cos, -sin): Re(Y e^{+i theta}) = Yr cos - Yi sin
        }
        idx += j;
        if (idx >= n) idx -= n;
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int t = 0; t < FT; ++t)
    if (f0 + t < a.F) a.g.base[foff[t] + (int64_t)(s + j) * a.g.ps] = acc[t];
}

template <typename F>
int with_field_tile(int ft, F&& f) {
  switch (ft) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: set_error("sht: no kernel is built for the planned field tile %d", ft); return ANEMOI_E_UNSUPPORTED;
  }
}

int check_common(const char* what, const GridSide& g, int32_t n_groups, const int32_t* ring_off, int32_t n_rings, int32_t max_ring,
                 const void* tw, const void* table, const void* coeffs, const void* ws, int64_t ws_bytes, const ShtPlan& p) {
  ANEMOI_REQUIRE(n_groups >= 0 && g.n_cols >= 0, "%s: bad field counts %d x %d", what, n_groups, g.n_cols);
  if ((int64_t)n_groups * g.n_cols == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(g.base && ring_off && tw && table && coeffs && ws, "%s: null pointer", what);
  ANEMOI_REQUIRE(g.gs >= 0 && g.ps >= 1, "%s: group stride %lld / point stride %lld", what, (long long)g.gs, (long long)g.ps);
  ANEMOI_REQUIRE(ws_bytes >= p.workspace_bytes, "%s: workspace of %lld bytes, %lld needed", what, (long long)ws_bytes, (long long)p.workspace_bytes);
  ANEMOI_REQUIRE(p.lds_bytes <= kShtRingLdsBytes, "%s: planned %d bytes of LDS", what, p.lds_bytes);
  return ANEMOI_OK;
}

// ------------------------------------------------------------------------------------------------------------- Ornstein combine
struct CombineArgs {
  const float* x;
  int64_t gs, ps;
  const int32_t* prog_cols;
  const int32_t* reg_cols;
  const float* fields;  // [2 + R, grid, n_prog]: gain, mu, beta_i
  const int32_t* trunc_map;
  const float* lowpass;  // [G, grid, n_trunc]
  const float* walias;   // [grid, n_trunc]
  float* out;            // [G, grid, n_prog]
  float* x_filtered;     // null, or where xt of the truncated columns is written (x's addressing; may be x itself)
  int32_t n_reg, n_trunc, n_groups, n_grid, n_prog;
};

__global__ __launch_bounds__(256) void ornstein_combine_kernel(CombineArgs a) {
  const int64_t per_group = (int64_t)a.n_grid * a.n_prog;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per_group * a.n_groups) return;
  const int g = (int)(i / per_group);
  const int64_t pc = i - (int64_t)g * per_group;  // point * n_prog + c
  const int p = (int)(pc / a.n_prog), c = (int)(pc - (int64_t)p * a.n_prog);
  const float* __restrict__ row = a.x + (int64_t)g * a.gs + (int64_t)p * a.ps;
  float v = row[a.prog_cols[c]];
  const int tc = a.trunc_map ? a.trunc_map[c] : -1;
  if (tc >= 0) {
    const float lp = a.lowpass[((int64_t)g * a.n_grid + p) * a.n_trunc + tc];
    if (a.walias) {
      const float w = a.walias[(int64_t)p * a.n_trunc + tc];
      v = w * v + (1.f - w) * lp;
    } else {
      v = lp;
    }
    // (in place on x: this thread alone reads and writes the element, and the host refuses regressors among the truncated columns)
    if (a.x_filtered) a.x_filtered[(int64_t)g * a.gs + (int64_t)p * a.ps + a.prog_cols[c]] = v;
  }
  float o = a.fields[pc] * v + a.fields[per_group + pc];
  for (int r = 0; r < a.n_reg; ++r) o += a.fields[(int64_t)(2 + r) * per_group + pc] * row[a.reg_cols[r]];
  a.out[i] = o;
}

}  // namespace
}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_sht_plan(int32_t direction, int32_t n_fields, const int32_t* lons_per_lat, int32_t n_rings, int32_t truncation,
                               anemoi_sht_plan_t* out) {
  ANEMOI_REQUIRE(out, "sht_plan: null out");
  ANEMOI_REQUIRE(direction == 0 || direction == 1, "sht_plan: direction %d is neither 0 (forward) nor 1 (inverse)", direction);
  ANEMOI_REQUIRE(lons_per_lat && n_rings > 0, "sht_plan: a grid of %d rings", n_rings);
  int max_ring = 0;
  for (int k = 0; k < n_rings; ++k) {
    ANEMOI_REQUIRE(lons_per_lat[k] > 0, "sht_plan: ring %d has %d points", k, lons_per_lat[k]);
    max_ring = lons_per_lat[k] > max_ring ? lons_per_lat[k] : max_ring;
  }
  ShtPlan p;
  const int rc = plan_sht((ShtDir)direction, n_fields, n_rings, max_ring, truncation, &p);
  out->field_tile = p.ft, out->chunk = p.chunk, out->lds_bytes = p.lds_bytes, out->lds_bound = kShtRingLdsBytes;
  out->ring_threads = kShtRingThreads, out->leg_rows = p.leg_rows;
  for (int i = 0; i < 3; ++i) out->ring_grid[i] = p.ring_grid[i], out->leg_grid[i] = p.leg_grid[i];
  out->workspace_bytes = p.workspace_bytes;
  return rc;
}

extern "C" int anemoi_sht_fwd(const float* x, int64_t gs, int64_t ps, const int32_t* cols, int32_t n_groups, int32_t n_cols,
                              const int32_t* ring_offsets, int32_t n_rings, int32_t max_ring, int32_t truncation, const float* twiddles,
                              const float* wleg, float* coeffs, float* workspace, int64_t workspace_bytes, void* stream) {
  ShtPlan p;
  const int64_t F = (int64_t)n_groups * n_cols;
  int rc = plan_sht(ShtDir::Forward, F < 0 ? 0 : F, n_rings, max_ring, truncation, &p);
  if (rc != ANEMOI_OK) return rc;
  GridSide g{const_cast<float*>(x), gs, ps, cols, n_cols};
  rc = check_common("sht_fwd", g, n_groups, ring_offsets, n_rings, max_ring, twiddles, wleg, coeffs, workspace, workspace_bytes, p);
  if (rc != ANEMOI_OK || F == 0) return rc;
  ShtArgs a{g, ring_offsets, (const float2*)twiddles, wleg, (float2*)workspace, (float2*)coeffs, nullptr, 1, (int32_t)F, n_rings,
            truncation + 1, p.chunk};
  hipStream_t s = as_stream(stream);
  return with_field_tile(p.ft, [&](auto ft_c) {
    constexpr int FT = decltype(ft_c)::value;
    hipLaunchKernelGGL((sht_ring_fwd_kernel<FT>), dim3(p.ring_grid[0], p.ring_grid[1], p.ring_grid[2]), dim3(kShtRingThreads), p.lds_bytes, s, a);
    const int r = check_launch("sht_ring_fwd_kernel");
    if (r != ANEMOI_OK) return r;
    hipLaunchKernelGGL((sht_leg_fwd_kernel<FT>), dim3(p.leg_grid[0], p.leg_grid[1], p.leg_grid[2]), dim3(64 * kShtLegWaves), 0, s, a);
    return check_launch("sht_leg_fwd_kernel");
  });
}

extern "C" int anemoi_sht_inv(const float* coeffs, const float* lscale, int32_t n_scale, const int32_t* ring_offsets, int32_t n_rings,
                              int32_t max_ring, int32_t truncation, const float* twiddles, const float* pleg, float* y, int64_t gs, int64_t ps,
                              const int32_t* cols, int32_t n_groups, int32_t n_cols, float* workspace, int64_t workspace_bytes, void* stream) {
  ShtPlan p;
  const int64_t F = (int64_t)n_groups * n_cols;
  int rc = plan_sht(ShtDir::Inverse, F < 0 ? 0 : F, n_rings, max_ring, truncation, &p);
  if (rc != ANEMOI_OK) return rc;
  ANEMOI_REQUIRE(!lscale || n_scale >= 1, "sht_inv: lscale with %d rows", n_scale);
  GridSide g{y, gs, ps, cols, n_cols};
  rc = check_common("sht_inv", g, n_groups, ring_offsets, n_rings, max_ring, twiddles, pleg, coeffs, workspace, workspace_bytes, p);
  if (rc != ANEMOI_OK || F == 0) return rc;
  ShtArgs a{g, ring_offsets, (const float2*)twiddles, pleg, (float2*)workspace, (float2*)const_cast<float*>(coeffs), lscale,
            lscale ? n_scale : 1, (int32_t)F, n_rings, truncation + 1, p.chunk};
  hipStream_t s = as_stream(stream);
  return with_field_tile(p.ft, [&](auto ft_c) {
    constexpr int FT = decltype(ft_c)::value;
    hipLaunchKernelGGL((sht_leg_inv_kernel<FT>), dim3(p.leg_grid[0], p.leg_grid[1], p.leg_grid[2]), dim3(64 * kShtLegWaves), 0, s, a);
    const int r = check_launch("sht_leg_inv_kernel");
    if (r != ANEMOI_OK) return r;
    hipLaunchKernelGGL((sht_ring_inv_kernel<FT>), dim3(p.ring_grid[0], p.ring_grid[1], p.ring_grid[2]), dim3(kShtRingThreads), p.lds_bytes, s, a);
    return check_launch("sht_ring_inv_kernel");
  });
}

extern "C" int anemoi_ornstein_combine_fwd(const float* x, int64_t gs, int64_t ps, const int32_t* prog_cols, const int32_t* reg_cols,
                                           int32_t n_reg, const float* fields, const int32_t* trunc_map, const float* lowpass, int32_t n_trunc,
                                           const float* walias, float* x_filtered, float* out, int32_t n_groups, int32_t n_grid, int32_t n_prog,
                                           void* stream) {
  ANEMOI_REQUIRE(n_groups >= 0 && n_grid >= 0 && n_prog >= 0 && n_reg >= 0 && n_trunc >= 0, "ornstein_combine_fwd: bad sizes G=%d grid=%d prog=%d R=%d T=%d",
                 n_groups, n_grid, n_prog, n_reg, n_trunc);
  const int64_t total = (int64_t)n_groups * n_grid * n_prog;
  if (total == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && prog_cols && fields && out && (reg_cols || n_reg == 0), "ornstein_combine_fwd: null pointer");
  ANEMOI_REQUIRE(!trunc_map || (lowpass && n_trunc > 0), "ornstein_combine_fwd: a truncation map without the low-pass fields");
  ANEMOI_REQUIRE(!walias || trunc_map, "ornstein_combine_fwd: anti-aliasing weights without a truncation map");
  ANEMOI_REQUIRE(gs >= 0 && ps >= 1, "ornstein_combine_fwd: group stride %lld / point stride %lld", (long long)gs, (long long)ps);
  ANEMOI_REQUIRE((total + 255) / 256 < (int64_t)1 << 31, "ornstein_combine_fwd: %lld elements", (long long)total);
  ANEMOI_REQUIRE(!x_filtered || trunc_map, "ornstein_combine_fwd: x_filtered without a truncation map");
  CombineArgs a{x, gs, ps, prog_cols, reg_cols, fields, trunc_map, lowpass, walias, out, x_filtered, n_reg, n_trunc, n_groups, n_grid, n_prog};
  hipLaunchKernelGGL(ornstein_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), a);
  return check_launch("ornstein_combine_kernel");
}
