// Row-wise HBM-bound kernels: LayerNorm, GraphConv edge epilogue (LayerNorm + residual + dst segment sum),
// row gather.  One 64-lane wavefront per row; a lane owns VEC contiguous elements per 64*VEC chunk, so every
// global access is a full-width coalesced vector load/store (16 B per lane for bf16 at VEC=8).
//
// Reference semantics: torch.nn.LayerNorm (eps inside sqrt, biased variance, affine) as instantiated by
// layer_kernels.LayerNorm (models/src/anemoi/models/layers/utils.py:107-121); GraphConv's
// "edge_mlp(...) + edge_attr" followed by scatter-sum (models/src/anemoi/models/layers/conv.py:73-81).
//
// rowwise_common.h holds what this file shares with rowwise_bwd.hip: load_row / store_row, the (VEC, CH) pick rule and the
// dispatchers from the picked values to template arguments; the dtype switch is dispatch_dtype (common.h).
#include <stdlib.h>

#include <algorithm>

#include "remap_core.h"
#include "rowwise_common.h"

namespace anemoi {

constexpr int kRowWaves = 4;   // waves (rows) per block

// In-register LayerNorm of one row held across the wave: two-pass (mean, then centred variance).
template <typename T, int VEC, int CH>
__device__ __forceinline__ void normalise_row(float (&r)[CH][VEC], int D, int lane, const T* __restrict__ gamma,
                                              const T* __restrict__ beta, float eps, float gadd = 0.f) {
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < CH; ++t)
#pragma unroll
    for (int j = 0; j < VEC; ++j) s += r[t][j];
  const float mean = wave_sum(s) / (float)D;
  float ss = 0.f;
#pragma unroll
  for (int t = 0; t < CH; ++t) {
    const int c = (t * 64 + lane) * VEC;
    if (c < D) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float dlt = r[t][j] - mean;
        ss = fmaf(dlt, dlt, ss);
      }
    }
  }
  const float rstd = rsqrtf(wave_sum(ss) / (float)D + eps);
#pragma unroll
  for (int t = 0; t < CH; ++t) {
    const int c = (t * 64 + lane) * VEC;
    if (c < D) {
      float g[VEC], b[VEC];
      load_vec<T, VEC>(gamma + c, g);
      if (beta != nullptr) {
        load_vec<T, VEC>(beta + c, b);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) b[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) r[t][j] = fmaf((r[t][j] - mean) * rstd, g[j] + gadd, b[j]);
    }
  }
}

template <typename T, int VEC, int CH>
__global__ __launch_bounds__(64 * kRowWaves) void layernorm_fwd_kernel(const T* __restrict__ x, int64_t ldx,
                                                                       const T* __restrict__ gamma,
                                                                       const T* __restrict__ beta,
                                                                       const T* __restrict__ residual, int64_t ldr,
                                                                       T* __restrict__ y, int64_t ldy, int n_rows,
                                                                       int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int rowi = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  if (rowi >= n_rows) return;
  float r[CH][VEC];
  load_row<T, VEC, CH>(x + (int64_t)rowi * ldx, D, lane, r);
  normalise_row<T, VEC, CH>(r, D, lane, gamma, beta, eps);
  if (residual != nullptr) {
    float rs[CH][VEC];
    load_row<T, VEC, CH>(residual + (int64_t)rowi * ldr, D, lane, rs);
#pragma unroll
    for (int t = 0; t < CH; ++t)
#pragma unroll
      for (int j = 0; j < VEC; ++j) r[t][j] += rs[t][j];
  }
  store_row<T, VEC, CH>(y + (int64_t)rowi * ldy, D, lane, r);
}

// Quarter-wave variant for D = 16 * 8 * CHQ 16-bit elements (D = 512: CHQ = 4): FOUR rows per wave, 16 lanes per row, every lane
// owns CHQ 16-byte chunks of its row (chunk c covers columns (c * 16 + l16) * 8 ..): 4x fewer waves than one row per wave, CHQ
// independent loads in flight per lane, and the two reductions stay inside a DPP row (4 butterfly steps instead of 6).
template <typename T, int CHQ, int LPR = 16>
__global__ __launch_bounds__(64 * kRowWaves) void layernorm_fwd_q_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ gamma,
                                                                         const T* __restrict__ beta, const T* __restrict__ residual,
                                                                         int64_t ldr, T* __restrict__ y, int64_t ldy, int n_rows, float eps) {
  constexpr int D = LPR * 8 * CHQ, RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, l16 = lane % LPR;
  const int rowi = (blockIdx.x * kRowWaves + (threadIdx.x >> 6)) * RPW + lane / LPR;
  const bool live = rowi < n_rows;
  const int64_t r = live ? rowi : n_rows - 1;  // lanes past the end recompute the last row and do not store
  float v[CHQ][8];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CHQ; ++c) {
    load_vec<T, 8>(x + r * ldx + (c * LPR + l16) * 8, v[c]);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[c][j];
  }
  const float mean = group_sum<LPR>(s) * (1.0f / D);
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < CHQ; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[c][j] -= mean;
      ss = fmaf(v[c][j], v[c][j], ss);
    }
  const float rstd = rsqrtf(group_sum<LPR>(ss) * (1.0f / D) + eps);
#pragma unroll
  for (int c = 0; c < CHQ; ++c) {
    const int col = (c * LPR + l16) * 8;
    float g[8], b[8], o[8];
    load_vec<T, 8>(gamma + col, g);
    if (beta != nullptr) {
      load_vec<T, 8>(beta + col, b);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) b[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = fmaf(v[c][j] * rstd, g[j], b[j]);
    if (residual != nullptr) {
      float rs[8];
      load_vec<T, 8>(residual + r * ldr + col, rs);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] += rs[j];
    }
    if (live) store_vec<T, 8>(y + r * ldy + col, o);
  }
}

// ConditionalLayerNorm (reference layers/normalization.py:34-94): y = LN(x) * (scale[row] + 1) + shift[row] with per-row
// modulation tensors (the two Linear maps of the conditioning, computed by one fused GEMM); lds = 0 broadcasts one row.
template <typename T, int VEC, int CH>
__global__ __launch_bounds__(64 * kRowWaves) void cond_layernorm_fwd_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ scale,
                                                                            int64_t lds, const T* __restrict__ shift, int64_t ldsh,
                                                                            T* __restrict__ y, int64_t ldy, int n_rows, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int rowi = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  if (rowi >= n_rows) return;
  float r[CH][VEC];
  load_row<T, VEC, CH>(x + (int64_t)rowi * ldx, D, lane, r);
  normalise_row<T, VEC, CH>(r, D, lane, scale + (int64_t)rowi * lds, shift + (int64_t)rowi * ldsh, eps, 1.0f);
  store_row<T, VEC, CH>(y + (int64_t)rowi * ldy, D, lane, r);
}

// ConditionalLayerNorm with the modulation computed IN the kernel (anemoi_cond_layernorm_proj_fwd):
//   y[r, :] = LN(x[r, :]) * (1 + cond[r, :] . Ws^T + bs) + (cond[r, :] . Wb^T + bb)  [+ residual[r, :]]
// for a conditioning width C <= kCondMax, where "the two Linear maps of the conditioning" are a handful of FMAs per output element: no
// [N, 2D] modulation tensor is written and read back.  w is the C-major image [C][2][D] of [scale.weight ; bias.weight] (row c = column c
// of both weights: a lane's VEC columns are contiguous), bias is [2][D].  One wave per row as in cond_layernorm_fwd_kernel, but the waves
// walk the rows with a grid stride so that what a lane needs of the image - the 2 C weights of its own columns - is fetched once per
// wave, not once per row.  Where the image lives (MODE):
//   kWReg    C <= kCondReg and one 16-byte chunk of row per lane (D <= 512 16-bit, D <= 256 fp32 at full vector width): in registers
//            (the hot shape D = 512, C = 4: 80 values per lane with the biases, 118 VGPRs in all, four waves per SIMD);
//   kWLds    the whole image fits the CU's LDS (160 KiB; 128 KiB at D = 1024, C = 32 in 16 bit): staged once per workgroup, then
//            conflict-free ds_read of VEC contiguous elements per lane (lanes read consecutive addresses);
//   kWGlobal larger images (fp32 at D = 1024, C = 32 is 256 KiB): read through L1 / L2 for every row.
// A row's C conditioning values are loaded by lanes 0 .. C-1 (element loads: any alignment, column slices) and broadcast with
// v_readlane; the modulation is accumulated in fp32 and never rounded to T.  The next row's x is in flight while a row is computed.
constexpr int kCondMax = 32;
constexpr int kCondReg = 4;
constexpr int kProjWaves = 8;
constexpr int kLdsBytes = 160 * 1024;
enum { kWReg = 0, kWLds = 1, kWGlobal = 2 };

template <typename T, int VEC, int CH, int MODE>
__global__ __launch_bounds__(64 * kProjWaves) void cond_layernorm_proj_fwd_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ cond,
                                                                                  int64_t ldc, const T* __restrict__ w, const T* __restrict__ bias,
                                                                                  const T* __restrict__ residual, int64_t ldr, T* __restrict__ y,
                                                                                  int64_t ldy, int n_rows, int D, int C, float eps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char proj_smem[];
  using V = Vec<T, VEC>;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kProjWaves + (threadIdx.x >> 6));
  const int n_waves = gridDim.x * kProjWaves;
  const T* wsrc = w;
  const T* bsrc = bias;
  if constexpr (MODE == kWLds) {
    T* s = reinterpret_cast<T*>(proj_smem);
    const int nw = 2 * C * D, nb = 2 * D;  // both multiples of VEC
    for (int i = threadIdx.x * VEC; i < nw; i += 64 * kProjWaves * VEC) *reinterpret_cast<V*>(s + i) = *reinterpret_cast<const V*>(w + i);
    for (int i = threadIdx.x * VEC; i < nb; i += 64 * kProjWaves * VEC) *reinterpret_cast<V*>(s + nw + i) = *reinterpret_cast<const V*>(bias + i);
    __syncthreads();
    wsrc = s;
    bsrc = s + nw;
  }
  V wr[MODE == kWReg ? kCondReg : 1][2][CH], br[2][CH];
  if constexpr (MODE == kWReg) {
#pragma unroll
    for (int t = 0; t < CH; ++t) {
      const int col = (t * 64 + lane) * VEC;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) br[h][t].v[j] = from_float<T>(0.f);
        if (col < D) br[h][t] = *reinterpret_cast<const V*>(bias + h * D + col);
#pragma unroll
        for (int c = 0; c < kCondReg; ++c) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) wr[c][h][t].v[j] = from_float<T>(0.f);
          if (c < C && col < D) wr[c][h][t] = *reinterpret_cast<const V*>(w + (int64_t)(2 * c + h) * D + col);
        }
      }
    }
  }
  if (wave >= n_rows) return;
  float r[CH][VEC];
  load_row<T, VEC, CH>(x + (int64_t)wave * ldx, D, lane, r);
  for (int rowi = wave; rowi < n_rows; rowi += n_waves) {
    const int nxt = rowi + n_waves < n_rows ? rowi + n_waves : rowi;  // the last trip re-reads its own row (an L1 hit) and drops it
    float rn[CH][VEC];
    load_row<T, VEC, CH>(x + (int64_t)nxt * ldx, D, lane, rn);
    const float cv = lane < C ? to_float(cond[(int64_t)rowi * ldc + lane]) : 0.f;
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < CH; ++t)
#pragma unroll
      for (int j = 0; j < VEC; ++j) s += r[t][j];
    const float mean = wave_sum(s) / (float)D;
    float ss = 0.f;
#pragma unroll
    for (int t = 0; t < CH; ++t) {
      if ((t * 64 + lane) * VEC < D) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float dlt = r[t][j] - mean;
          ss = fmaf(dlt, dlt, ss);
        }
      }
    }
    const float rstd = rsqrtf(wave_sum(ss) / (float)D + eps);
#pragma unroll
    for (int t = 0; t < CH; ++t) {
      const int col = (t * 64 + lane) * VEC;
      if (col < D) {
        float sc[VEC], sh[VEC];
        if constexpr (MODE == kWReg) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            sc[j] = to_float(br[0][t].v[j]);
            sh[j] = to_float(br[1][t].v[j]);
          }
#pragma unroll
          for (int c = 0; c < kCondReg; ++c) {
            const float cc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cv), c));
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              sc[j] = fmaf(cc, to_float(wr[c][0][t].v[j]), sc[j]);
              sh[j] = fmaf(cc, to_float(wr[c][1][t].v[j]), sh[j]);
            }
          }
        } else {
          load_vec<T, VEC>(bsrc + col, sc);
          load_vec<T, VEC>(bsrc + D + col, sh);
          for (int c = 0; c < C; ++c) {
            const float cc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cv), c));
            float ws[VEC], wb[VEC];
            load_vec<T, VEC>(wsrc + (2 * c) * D + col, ws);
            load_vec<T, VEC>(wsrc + (2 * c + 1) * D + col, wb);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
              sc[j] = fmaf(cc, ws[j], sc[j]);
              sh[j] = fmaf(cc, wb[j], sh[j]);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) r[t][j] = fmaf((r[t][j] - mean) * rstd, 1.0f + sc[j], sh[j]);
        if (residual != nullptr) {
          float rs[VEC];
          load_vec<T, VEC>(residual + (int64_t)rowi * ldr + col, rs);
#pragma unroll
          for (int j = 0; j < VEC; ++j) r[t][j] += rs[j];
        }
      }
    }
    store_row<T, VEC, CH>(y + (int64_t)rowi * ldy, D, lane, r);
#pragma unroll
    for (int t = 0; t < CH; ++t)
#pragma unroll
      for (int j = 0; j < VEC; ++j) r[t][j] = rn[t][j];
  }
}

// e_new = LN(z) + e_old (LN optional) ; agg[d] = sum over the in-edges of d (dst-sorted => contiguous rows).
template <typename T, int VEC, int CH>
__global__ __launch_bounds__(64 * kRowWaves) void edge_ln_res_segsum_kernel(
    const T* __restrict__ z, int64_t ldz, const T* __restrict__ e_old, int64_t lde, const T* __restrict__ gamma,
    const T* __restrict__ beta, float eps, const int32_t* __restrict__ colptr, T* __restrict__ e_new, int64_t ldn,
    T* __restrict__ agg, int64_t ldagg, int n_dst, int D) {
  const int lane = threadIdx.x & 63;
  const int d = __builtin_amdgcn_readfirstlane(blockIdx.x * kRowWaves + (threadIdx.x >> 6));
  if (d >= n_dst) return;
  const int beg = __builtin_amdgcn_readfirstlane(colptr[d]);
  const int end = __builtin_amdgcn_readfirstlane(colptr[d + 1]);
  float sum[CH][VEC];
#pragma unroll
  for (int t = 0; t < CH; ++t)
#pragma unroll
    for (int j = 0; j < VEC; ++j) sum[t][j] = 0.f;
  for (int m = beg; m < end; ++m) {
    float r[CH][VEC], eo[CH][VEC];
    load_row<T, VEC, CH>(z + (int64_t)m * ldz, D, lane, r);
    load_row<T, VEC, CH>(e_old + (int64_t)m * lde, D, lane, eo);
    if (gamma != nullptr) normalise_row<T, VEC, CH>(r, D, lane, gamma, beta, eps);
#pragma unroll
    for (int t = 0; t < CH; ++t)
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        r[t][j] += eo[t][j];
      }
    store_row<T, VEC, CH>(e_new + (int64_t)m * ldn, D, lane, r);
    // accumulate what was actually stored (storage precision), matching scatter(sum) over the stored e_new
#pragma unroll
    for (int t = 0; t < CH; ++t)
#pragma unroll
      for (int j = 0; j < VEC; ++j) sum[t][j] += to_float(from_float<T>(r[t][j]));
  }
  store_row<T, VEC, CH>(agg + (int64_t)d * ldagg, D, lane, sum);
}

// Quarter-wave variant for 512 16-bit channels (the GNN's edge rows): still one wave per destination, but FOUR of its in-edges at
// a time - 16 lanes per edge row, CHQ 16-byte chunks per lane, so 2 * CHQ loads per lane are in flight instead of 2, the LayerNorm
// reductions stay inside a DPP row, and the loads of the next four rows are issued before the current four are normalised.  A
// destination of the processor mesh has ~8 in-edges: two trips through the loop instead of eight dependent ones.  The per-row
// arithmetic is the one of the kernel above; the segment sum adds the lane groups' partial sums (fp32) at the end.
// <T, 2, 32> is the half-wave form (two rows at a time, 32 lanes per row, half the registers).
template <typename T, int CHQ, int LPR = 16>
__global__ __launch_bounds__(64 * kRowWaves) void edge_ln_res_segsum_kernel_mr(
    const T* __restrict__ z, int64_t ldz, const T* __restrict__ e_old, int64_t lde, const T* __restrict__ gamma,
    const T* __restrict__ beta, float eps, const int32_t* __restrict__ colptr, T* __restrict__ e_new, int64_t ldn,
    T* __restrict__ agg, int64_t ldagg, int n_dst) {
  constexpr int D = LPR * 8 * CHQ, RPW = 64 / LPR;
  using V8 = Vec<T, 8>;
  const int lane = threadIdx.x & 63, l16 = lane % LPR, g = lane / LPR;
  const int d = __builtin_amdgcn_readfirstlane(blockIdx.x * kRowWaves + (threadIdx.x >> 6));
  if (d >= n_dst) return;
  const int beg = __builtin_amdgcn_readfirstlane(colptr[d]);
  const int end = __builtin_amdgcn_readfirstlane(colptr[d + 1]);
  V8 gq[CHQ], bq[CHQ];
#pragma unroll
  for (int c = 0; c < CHQ; ++c) {
    gq[c] = *reinterpret_cast<const V8*>(gamma + (c * LPR + l16) * 8);
    if (beta != nullptr) {
      bq[c] = *reinterpret_cast<const V8*>(beta + (c * LPR + l16) * 8);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) bq[c].v[j] = from_float<T>(0.f);
    }
  }
  float sum[CHQ][8];
#pragma unroll
  for (int c = 0; c < CHQ; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) sum[c][j] = 0.f;
  V8 zq[CHQ], eq[CHQ];
  const auto fetch = [&](int m0, V8(&zz)[CHQ], V8(&ee)[CHQ]) {  // groups past the segment's end re-read its last row and drop the result
    const int64_t m = min(m0 + g, end - 1);
#pragma unroll
    for (int c = 0; c < CHQ; ++c) {
      zz[c] = *reinterpret_cast<const V8*>(z + m * ldz + (c * LPR + l16) * 8);
      ee[c] = *reinterpret_cast<const V8*>(e_old + m * lde + (c * LPR + l16) * 8);
    }
  };
  if (beg < end) fetch(beg, zq, eq);
  for (int m0 = beg; m0 < end; m0 += RPW) {
    V8 zn[CHQ], en[CHQ];
    const bool more = m0 + RPW < end;  // wave-uniform
    if (more) fetch(m0 + RPW, zn, en);
    const bool live = m0 + g < end;
    float v[CHQ][8];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CHQ; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[c][j] = to_float(zq[c].v[j]);
        s += v[c][j];
      }
    const float mean = group_sum<LPR>(s) * (1.0f / D);
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < CHQ; ++c)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[c][j] -= mean;
        ss = fmaf(v[c][j], v[c][j], ss);
      }
    const float rstd = rsqrtf(group_sum<LPR>(ss) * (1.0f / D) + eps);
#pragma unroll
    for (int c = 0; c < CHQ; ++c) {
      V8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        o.v[j] = from_float<T>(fmaf(v[c][j] * rstd, to_float(gq[c].v[j]), to_float(bq[c].v[j])) + to_float(eq[c].v[j]));
        if (live) sum[c][j] += to_float(o.v[j]);  // what is stored (storage precision), as scatter(sum) over the stored e_new sees it
      }
      if (live) *reinterpret_cast<V8*>(e_new + (int64_t)(m0 + g) * ldn + (c * LPR + l16) * 8) = o;
    }
    if (more) {
#pragma unroll
      for (int c = 0; c < CHQ; ++c) {
        zq[c] = zn[c];
        eq[c] = en[c];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CHQ; ++c) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr (LPR <= 16) sum[c][j] += __shfl_xor(sum[c][j], 16, 64);
      if constexpr (LPR <= 32) sum[c][j] += __shfl_xor(sum[c][j], 32, 64);
    }
    if (g == 0) store_vec<T, 8>(agg + (int64_t)d * ldagg + (c * LPR + l16) * 8, sum[c]);
  }
}

template <typename T, int VEC>
__global__ __launch_bounds__(64 * kRowWaves) void gather_rows_kernel(const T* __restrict__ x, int64_t ldx,
                                                                     const int32_t* __restrict__ idx,
                                                                     T* __restrict__ out, int64_t ldo, int n_out, int D) {
  const int lane = threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * kRowWaves + (threadIdx.x >> 6));
  if (i >= n_out) return;
  const int s = __builtin_amdgcn_readfirstlane(idx[i]);
  for (int c = lane * VEC; c < D; c += 64 * VEC) {
    *reinterpret_cast<Vec<T, VEC>*>(out + (int64_t)i * ldo + c) = *reinterpret_cast<const Vec<T, VEC>*>(x + (int64_t)s * ldx + c);
  }
}

// Output boundings at the model edge (reference layers/bounding.py:81-307), all configured boundings in ONE pass: a thread
// owns a row and applies the column program in order (ops: int32 [n_ops][4] = kind, column, total column, unused;
// params: fp32 [n_ops][2] = min / max or the normalised minimum).  kind: 1 relu, 2 leaky relu, 3 relu above a minimum,
// 4 leaky relu above a minimum, 5 hardtanh, 6 leaky hardtanh, 7 hardtanh * x[total], 8 leaky hardtanh * x[total]
// (slopes 0.01 as in torch / layers/activations.py:16-42), 9 de-normalisation (x - p0) / p1 (preprocessing/normalizer.py:217-252).
template <typename T>
__global__ void bound_columns_kernel(T* __restrict__ x, int64_t ldx, int n_rows, const int32_t* __restrict__ ops,
                                     const float* __restrict__ params, int n_ops) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  T* row = x + (int64_t)r * ldx;
  for (int i = 0; i < n_ops; ++i) {
    const int kind = ops[4 * i], col = ops[4 * i + 1], tot = ops[4 * i + 2];
    const float p0 = params[2 * i], p1 = params[2 * i + 1];
    float v = to_float(row[col]);
    auto leaky = [](float t) { return t > 0.f ? t : 0.01f * t; };
    auto lht = [&](float t) { return t < p0 ? p0 + 0.01f * (t - p0) : (t > p1 ? p1 + 0.01f * (t - p1) : t); };
    // comparisons, not fmaxf / fminf (which return the non-NaN operand): a NaN stays a NaN, as through torch.relu / hardtanh / clamp
    auto relu = [](float t) { return t < 0.f ? 0.f : t; };
    auto clamp = [&](float t) { return t < p0 ? p0 : (t > p1 ? p1 : t); };
    switch (kind) {
      case 1: v = relu(v); break;
      case 2: v = leaky(v); break;
      case 3: v = relu(v - p0) + p0; break;
      case 4: v = leaky(v - p0) + p0; break;
      case 5: v = clamp(v); break;
      case 6: v = lht(v); break;
      case 7: v = to_float(from_float<T>(clamp(v))) * to_float(row[tot]); break;
      case 8: v = to_float(from_float<T>(lht(v))) * to_float(row[tot]); break;
      case 9: v = to_float(from_float<T>(v - p0)) / p1; break;  // InputNormalizer.inverse_transform: x.subtract_(add).div_(mul) (normalizer.py:246-252)
      default: break;
    }
    row[col] = from_float<T>(v);
  }
}

// Output assembly at the model edge (reference models/encoder_processor_decoder.py:145-163 for batch = ensemble = time = 1):
// out[n, v] = x_out[n, v] + (col_map[v] >= 0 ? x_skip[n, col_map[v]] : 0) - the residual (SkipConnection) added onto the
// prognostic columns - in one pass instead of clone + index_select + index_add_.
template <typename T, int Q>
__global__ void assemble_output_kernel(const T* __restrict__ x_out, int64_t ldx, const T* __restrict__ skip, int64_t lds,
                                       const int32_t* __restrict__ col_map, T* __restrict__ out, int64_t ldo, int n_rows, int n_cols) {
  const int per_row = n_cols / Q;  // Q columns per thread (8-byte moves for 16-bit types when the widths / strides allow)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * per_row) return;
  const int n = (int)(i / per_row), v0 = (int)(i % per_row) * Q;
  Vec<T, Q> a = *reinterpret_cast<const Vec<T, Q>*>(x_out + (int64_t)n * ldx + v0), o;
#pragma unroll
  for (int j = 0; j < Q; ++j) {
    float val = to_float(a.v[j]);
    const int m = col_map[v0 + j];
    if (m >= 0) val = to_float(from_float<T>(val)) + to_float(skip[(int64_t)n * lds + m]);
    o.v[j] = from_float<T>(val);
  }
  *reinterpret_cast<Vec<T, Q>*>(out + (int64_t)n * ldo + v0) = o;
}

// Input assembly at the model edge for batch = ensemble = 1 (reference models/encoder_processor_decoder.py:98-143,
// "batch time ensemble grid vars -> (batch ensemble grid) (time vars)" + cat with the node attributes):
//   out[n, :] = [ x[0, n, :] | ... | x[T-1, n, :] | attrs[n, :] | 0 ... ]   (width W >= T*V + A: the alignment zeros of the embedding GEMMs)
// in one pass instead of a permute-copy and a cat.  Q elements per thread (Q = 4 when V, A, W and the row strides allow 8-byte moves).
template <typename T, int Q>
__global__ void assemble_input_kernel(const T* __restrict__ x, int64_t ld_t, int64_t ldx, int T_steps, int V, const T* __restrict__ attrs,
                                      int64_t lda, int A, T* __restrict__ out, int64_t ldo, int W, int n_rows) {
  const int per_row = W / Q;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * per_row) return;
  const int n = (int)(i / per_row), c = (int)(i % per_row) * Q;
  Vec<T, Q> v{};
  if (c < T_steps * V) {
    const int t = c / V, cv = c % V;  // V % Q == 0: a group never straddles two time steps
    v = *reinterpret_cast<const Vec<T, Q>*>(x + t * ld_t + (int64_t)n * ldx + cv);
  } else if (c < T_steps * V + A) {
    v = *reinterpret_cast<const Vec<T, Q>*>(attrs + (int64_t)n * lda + (c - T_steps * V));
  }
  *reinterpret_cast<Vec<T, Q>*>(out + (int64_t)n * ldo + c) = v;
}

// x * m + a with the two roundings of torch's `x.mul_(m).add_(a)` (no FMA contraction): bit-equal to the reference's
// InputNormalizer.transform in fp32 (preprocessing/normalizer.py:154-190).
__device__ __forceinline__ float mul_then_add(float x, float m, float a) {
#pragma clang fp contract(off)
  const float t = x * m;
  return t + a;
}

// x * m as an fp32 VALUE, whatever is done with it next.  A product that is then converted to fp16 is otherwise selected as one
// v_fma_mixlo_f16 (with or without fp contraction), which rounds the exact product to fp16 once; torch rounds it to fp32 first, and
// the two differ where that fp32 value is a tie between two fp16 values (one element in 2^14).  The empty asm pins the product in a
// VGPR, so the conversion is an instruction of its own.
__device__ __forceinline__ float mul_f32(float x, float m) {
  float t = x * m;
  asm("" : "+v"(t));
  return t;
}

// Input assembly WITH the input normaliser as a column program (scope row f4): as assemble_input_kernel, and the time /
// variable columns become x * mul[v] + add[v] (fp32 arithmetic, one pass over the input).  The input may be wider than
// the model dtype (fp32 data into a 16-bit model): TI -> fp32 -> TO.
template <typename TI, typename TO>
__global__ void assemble_input_norm_kernel(const TI* __restrict__ x, int64_t ld_t, int64_t ldx, int T_steps, int V, const float* __restrict__ mul,
                                           const float* __restrict__ add, const TO* __restrict__ attrs, int64_t lda, int A, TO* __restrict__ out,
                                           int64_t ldo, int W, int n_rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * W) return;
  const int n = (int)(i / W), c = (int)(i % W);
  float v = 0.f;
  if (c < T_steps * V) {
    const int t = c / V, cv = c % V;
    v = to_float(x[t * ld_t + (int64_t)n * ldx + cv]);
    if (mul != nullptr) v = mul_then_add(v, mul[cv], add[cv]);
  } else if (c < T_steps * V + A) {
    v = to_float(attrs[(int64_t)n * lda + (c - T_steps * V)]);
  }
  out[(int64_t)n * ldo + c] = from_float<TO>(v);
}

// The same for 16-bit outputs whose width is a multiple of 8: a thread produces 8 consecutive columns and stores them as one 16-byte
// vector (the GNN embeddings' zero-padded [M, 128] inputs are mostly padding: 25 us -> a few at 81 840 rows).
template <typename TI, typename TO>
__global__ void assemble_input_norm_vec8_kernel(const TI* __restrict__ x, int64_t ld_t, int64_t ldx, int T_steps, int V, const float* __restrict__ mul,
                                                const float* __restrict__ add, const TO* __restrict__ attrs, int64_t lda, int A, TO* __restrict__ out,
                                                int64_t ldo, int W, int n_rows) {
  const int per_row = W >> 3;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * per_row) return;
  const int n = (int)(i / per_row), c0 = (int)(i % per_row) << 3;
  Vec<TO, 8> o;
  if (T_steps == 1 && A == 0) {  // a plain cast + zero-pad of [N, V] rows (the GNN embeddings' inputs): no divisions
    const TI* xr = x + (int64_t)n * ldx;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      float v = c < V ? to_float(xr[c]) : 0.f;
      if (mul != nullptr && c < V) v = mul_then_add(v, mul[c], add[c]);
      o.v[j] = from_float<TO>(v);
    }
    *reinterpret_cast<Vec<TO, 8>*>(out + (int64_t)n * ldo + c0) = o;
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c0 + j;
    float v = 0.f;
    if (c < T_steps * V) {
      const int t = c / V, cv = c % V;
      v = to_float(x[t * ld_t + (int64_t)n * ldx + cv]);
      if (mul != nullptr) v = mul_then_add(v, mul[cv], add[cv]);
    } else if (c < T_steps * V + A) {
      v = to_float(attrs[(int64_t)n * lda + (c - T_steps * V)]);
    }
    o.v[j] = from_float<TO>(v);
  }
  *reinterpret_cast<Vec<TO, 8>*>(out + (int64_t)n * ldo + c0) = o;
}

// Output assembly with the skip connection taken from the RAW input (normalised on the fly) - the counterpart of
// assemble_input_norm_kernel: out[n, v] = x_out[n, v] + (col_map[v] >= 0 ? skip[n, m] * mul[m] + add[m] : 0), m = col_map[v].
// x_out is in the model dtype (TM), skip and out in the caller's data dtype (TS): the reference adds the residual in the
// input's dtype (x_out.to(dtype=x.dtype), models/encoder_processor_decoder.py:145-158).
template <typename TM, typename TS>
__global__ void assemble_output_norm_kernel(const TM* __restrict__ x_out, int64_t ldx, const TS* __restrict__ skip, int64_t lds,
                                            const int32_t* __restrict__ col_map, const float* __restrict__ mul, const float* __restrict__ add,
                                            TS* __restrict__ out, int64_t ldo, int n_rows, int n_cols) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * n_cols) return;
  const int n = (int)(i / n_cols), v = (int)(i % n_cols);
  float val = to_float(from_float<TS>(to_float(x_out[(int64_t)n * ldx + v])));
  const int m = col_map[v];
  if (m >= 0) {
    float sk = to_float(skip[(int64_t)n * lds + m]);
    if (mul != nullptr) sk = to_float(from_float<TS>(mul_then_add(sk, mul[m], add[m])));
    val += sk;
  }
  out[(int64_t)n * ldo + v] = from_float<TS>(val);
}

// y[r, c] = x[r, c] * mul[c] + add[c] (inverse = 0) or (x[r, c] - add[c]) / mul[c] (inverse = 1): InputNormalizer.transform /
// inverse_transform as a stand-alone kernel (preprocessing/normalizer.py:154-252); may run in place (y == x).
template <typename T>
__global__ void affine_columns_kernel(const T* __restrict__ x, int64_t ldx, T* __restrict__ y, int64_t ldy, const float* __restrict__ mul,
                                      const float* __restrict__ add, int inverse, int n_rows, int V) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * V) return;
  const int r = (int)(i / V), c = (int)(i % V);
  const float v = to_float(x[(int64_t)r * ldx + c]);
  float o;
  if (inverse) {
    o = to_float(from_float<T>(v - add[c])) / mul[c];  // subtract_ then div_: two roundings in T like torch's in-place ops
  } else {
    if constexpr (sizeof(T) == 4) {
      o = mul_then_add(v, mul[c], add[c]);  // two fp32 roundings, never an FMA
    } else {
      o = to_float(from_float<T>(mul_f32(v, mul[c])));  // mul_ rounds to T (through fp32, as torch does), then add_ rounds again
      o = o + add[c];
    }
  }
  y[(int64_t)r * ldy + c] = from_float<T>(o);
}

// ---- imputers at the model edges (reference preprocessing/imputer.py) ---------------------------------------------------------------
// The imputation program is a per-column table over the V input columns: kind_src int32 [V][2] = (kind, source column), value fp32 [V].
// kind 0: the column is not imputed; 1: a NaN becomes value[c] (rounded to the data dtype on the host, so the fp32 entry is exact);
// 2: a NaN becomes the element of column `source` at the same position (CopyImputer).  A source column is never itself imputed (the host
// refuses such programs), so an in-place launch reads no element another thread writes.
template <typename T>
__device__ __forceinline__ float impute_one(float v, bool is_nan, const T* __restrict__ row, int kind, int src, float value) {
  if (kind == 0 || !is_nan) return v;
  return kind == 1 ? value : to_float(row[src]);
}

// Stand-alone imputer over x [batch, time, ensemble, grid, V] (element strides ld_b, ld_t, ld_e, ld_n; columns contiguous): the NaN test of
// an element is isnan of ensemble member 0 at the same (batch, time, grid, column) - imputer.py:116-134 keeps the first member's locations -
// and applies to every member.  A thread owns one (batch, time, grid, column) and walks the members, member 0's test read before any store,
// so y may alias x.  mask (may be null): bool [batch, grid, V], the NaN locations of time step 0, one byte per element.
template <typename T>
__global__ void impute_columns_kernel(const T* x, int64_t ld_b, int64_t ld_t, int64_t ld_e, int64_t ld_n, T* y, int64_t yd_b,  // (y may be x)
                                      int64_t yd_t, int64_t yd_e, int64_t yd_n, const int32_t* __restrict__ kind_src, const float* __restrict__ value,
                                      uint8_t* __restrict__ mask, int B, int T_steps, int E, int N, int V) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T_steps * N * V) return;
  const int c = (int)(i % V);
  const int n = (int)((i / V) % N);
  const int t = (int)((i / ((int64_t)V * N)) % T_steps);
  const int b = (int)(i / ((int64_t)V * N * T_steps));
  const T* xr = x + b * ld_b + t * ld_t + (int64_t)n * ld_n;
  T* yr = y + b * yd_b + t * yd_t + (int64_t)n * yd_n;
  const int kind = kind_src[2 * c], src = kind_src[2 * c + 1];
  const float val = value[c];
  const bool is_nan = isnan(to_float(xr[c]));
  if (mask != nullptr && t == 0) mask[((int64_t)b * N + n) * V + c] = is_nan ? 1 : 0;
  if (kind == 0 && x == y) return;
  for (int e = 0; e < E; ++e) {
    const T* xe = xr + e * ld_e;
    const T in = xe[c];
    yr[e * yd_e + c] = (kind == 0 || !is_nan) ? in : from_float<T>(impute_one<T>(0.f, true, xe, kind, src, val));
  }
}

// BaseImputer.inverse_transform (imputer.py:243-279): y[b, m, n, c] = NaN where mask[b, n, src_of[c]] (src_of[c] >= 0), else x[b, m, n, c];
// x / y [batch, M, grid, V_out] contiguous rows of ldx / ldy elements, mask bool [batch, grid, ldm].  In place (y == x) only the restored
// elements are stored.
template <typename T>
__global__ void restore_nan_columns_kernel(const T* x, int64_t ldx, T* y, int64_t ldy, const uint8_t* __restrict__ mask,  // (y may be x)
                                           int64_t ldm, int n_mask_cols, const int32_t* __restrict__ src_of, int B, int M, int N, int V) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * M * N * V) return;
  const int c = (int)(i % V);
  const int64_t row = i / V;
  const int n = (int)(row % N);
  const int b = (int)(row / ((int64_t)N * M));
  const int s = src_of[c];
  const bool hit = s >= 0 && s < n_mask_cols && mask[((int64_t)b * N + n) * ldm + s] != 0;
  if (hit)
    y[row * ldy + c] = from_float<T>(__builtin_nanf(""));
  else if (x != y)
    y[row * ldy + c] = x[row * ldx + c];
}

// assemble_input_norm_kernel with the imputation program in front of the normaliser: every raw element is tested and imputed within its OWN
// time step (the copy source is read from the same step and row), then x * mul + add with the same two fp32 roundings; the NaN locations of
// step 0 go to mask bool [N][ldm] in the same pass.
template <typename TI, typename TO>
__global__ void assemble_input_impute_kernel(const TI* __restrict__ x, int64_t ld_t, int64_t ldx, int T_steps, int V, const int32_t* __restrict__ kind_src,
                                             const float* __restrict__ value, uint8_t* __restrict__ mask, int64_t ldm, const float* __restrict__ mul,
                                             const float* __restrict__ add, const TO* __restrict__ attrs, int64_t lda, int A, TO* __restrict__ out,
                                             int64_t ldo, int W, int n_rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * W) return;
  const int n = (int)(i / W), c = (int)(i % W);
  float v = 0.f;
  if (c < T_steps * V) {
    const int t = c / V, cv = c % V;
    const TI* xr = x + t * ld_t + (int64_t)n * ldx;
    v = to_float(xr[cv]);
    const bool is_nan = isnan(v);
    if (t == 0) mask[(int64_t)n * ldm + cv] = is_nan ? 1 : 0;
    if (is_nan) v = impute_one<TI>(v, true, xr, kind_src[2 * cv], kind_src[2 * cv + 1], value[cv]);
    if (mul != nullptr) v = mul_then_add(v, mul[cv], add[cv]);
  } else if (c < T_steps * V + A) {
    v = to_float(attrs[(int64_t)n * lda + (c - T_steps * V)]);
  }
  out[(int64_t)n * ldo + c] = from_float<TO>(v);
}

// The same for 16-bit outputs whose width is a multiple of 8 (one 16-byte store per thread), as assemble_input_norm_vec8_kernel.  A group
// of 8 columns that lies within step 0 owns 8 consecutive mask bytes: they leave as two 4-byte stores where the mask rows allow it
// (ldm % 4 == 0, base 4-byte aligned - then n * ldm + c0 is a multiple of 4), else byte by byte.  The program entry of a column is one
// 8-byte load; its value is read only where a NaN is replaced.
template <typename TI, typename TO>
__global__ void assemble_input_impute_vec8_kernel(const TI* __restrict__ x, int64_t ld_t, int64_t ldx, int T_steps, int V,
                                                  const int32_t* __restrict__ kind_src, const float* __restrict__ value, uint8_t* __restrict__ mask,
                                                  int64_t ldm, const float* __restrict__ mul, const float* __restrict__ add,
                                                  const TO* __restrict__ attrs, int64_t lda, int A, TO* __restrict__ out, int64_t ldo, int W, int n_rows) {
  const int per_row = W >> 3;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * per_row) return;
  const int n = (int)(i / per_row), c0 = (int)(i % per_row) << 3;
  const bool packed = c0 + 8 <= V && (ldm & 3) == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  uint32_t bits[2] = {0u, 0u};
  Vec<TO, 8> o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c0 + j;
    float v = 0.f;
    if (c < T_steps * V) {
      const int t = c / V, cv = c % V;
      const TI* xr = x + t * ld_t + (int64_t)n * ldx;
      v = to_float(xr[cv]);
      const bool is_nan = isnan(v);
      if (packed)
        bits[j >> 2] |= (is_nan ? 1u : 0u) << (8 * (j & 3));
      else if (t == 0)
        mask[(int64_t)n * ldm + cv] = is_nan ? 1 : 0;
      if (is_nan) {
        const int2 ks = reinterpret_cast<const int2*>(kind_src)[cv];
        if (ks.x != 0) v = ks.x == 1 ? value[cv] : to_float(xr[ks.y]);
      }
      if (mul != nullptr) v = mul_then_add(v, mul[cv], add[cv]);
    } else if (c < T_steps * V + A) {
      v = to_float(attrs[(int64_t)n * lda + (c - T_steps * V)]);
    }
    o.v[j] = from_float<TO>(v);
  }
  if (packed) {
    uint32_t* m = reinterpret_cast<uint32_t*>(mask + (int64_t)n * ldm + c0);
    m[0] = bits[0];
    m[1] = bits[1];
  }
  *reinterpret_cast<Vec<TO, 8>*>(out + (int64_t)n * ldo + c0) = o;
}

// assemble_output_norm_kernel whose RAW skip is imputed by the same program before it is normalised.
template <typename TM, typename TS>
__global__ void assemble_output_impute_kernel(const TM* __restrict__ x_out, int64_t ldx, const TS* __restrict__ skip, int64_t lds,
                                              const int32_t* __restrict__ col_map, const int32_t* __restrict__ kind_src, const float* __restrict__ value,
                                              const float* __restrict__ mul, const float* __restrict__ add, TS* __restrict__ out, int64_t ldo, int n_rows,
                                              int n_cols) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * n_cols) return;
  const int n = (int)(i / n_cols), v = (int)(i % n_cols);
  float val = to_float(from_float<TS>(to_float(x_out[(int64_t)n * ldx + v])));
  const int m = col_map[v];
  if (m >= 0) {
    const TS* sr = skip + (int64_t)n * lds;
    float sk = to_float(sr[m]);
    if (isnan(sk)) sk = impute_one<TS>(sk, true, sr, kind_src[2 * m], kind_src[2 * m + 1], value[m]);
    if (mul != nullptr) sk = to_float(from_float<TS>(mul_then_add(sk, mul[m], add[m])));
    val += sk;
  }
  out[(int64_t)n * ldo + v] = from_float<TS>(val);
}

// bound_columns_kernel with one more kind, 10: NaN where mask[r, tot] (BaseImputer.inverse_transform as an op of the output column program,
// appended after the op-9 de-normalisations; `tot` is the mask column).  The kinds 1..9 are those of bound_columns_kernel, statement for
// statement; that kernel is kept as it is for the programs without a mask.
// EXT (anemoi_column_program; the instantiation without it is the kernel as it was): the kinds of the post-processors and the remapper's
// inverse.  11: p0 where row[tot] == 0 (ConditionalZeroPostprocessor); 12: NaN where row[tot] is NaN (ConditionalNaNPostprocessor) - both
// read the masking column as the ops before them left it, so the host orders a fill OF the masking column after the fills it masks;
// 16 + op: the RemapOp `op` (remap_core.h) with flags = ops[4 i + 3] and a third parameter as the float bits of ops[4 i + 2].
template <typename T, bool EXT>
__global__ void bound_columns_mask_kernel(T* __restrict__ x, int64_t ldx, int n_rows, const int32_t* __restrict__ ops, const float* __restrict__ params,
                                          int n_ops, const uint8_t* __restrict__ mask, int64_t ldm, int n_mask_cols) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  T* row = x + (int64_t)r * ldx;
  for (int i = 0; i < n_ops; ++i) {
    const int kind = ops[4 * i], col = ops[4 * i + 1], tot = ops[4 * i + 2];
    const float p0 = params[2 * i], p1 = params[2 * i + 1];
    float v = to_float(row[col]);
    auto leaky = [](float t) { return t > 0.f ? t : 0.01f * t; };
    auto lht = [&](float t) { return t < p0 ? p0 + 0.01f * (t - p0) : (t > p1 ? p1 + 0.01f * (t - p1) : t); };
    auto relu = [](float t) { return t < 0.f ? 0.f : t; };
    auto clamp = [&](float t) { return t < p0 ? p0 : (t > p1 ? p1 : t); };
    switch (kind) {
      case 1: v = relu(v); break;
      case 2: v = leaky(v); break;
      case 3: v = relu(v - p0) + p0; break;
      case 4: v = leaky(v - p0) + p0; break;
      case 5: v = clamp(v); break;
      case 6: v = lht(v); break;
      case 7: v = to_float(from_float<T>(clamp(v))) * to_float(row[tot]); break;
      case 8: v = to_float(from_float<T>(lht(v))) * to_float(row[tot]); break;
      case 9: v = to_float(from_float<T>(v - p0)) / p1; break;
      case 10:
        if ((unsigned)tot >= (unsigned)n_mask_cols || mask[(int64_t)r * ldm + tot] == 0) continue;  // every other bit of the row stays
        v = __builtin_nanf("");
        break;
      default:
        if constexpr (EXT) {
          if (kind == 11) {
            if (!(to_float(row[tot]) == 0.f)) continue;
            v = p0;
          } else if (kind == 12) {
            if (!isnan(to_float(row[tot]))) continue;
            v = __builtin_nanf("");
          } else if (kind >= 16) {
            bool bad = false;
            v = remap_apply<T>(v, kind - 16, ops[4 * i + 3], p0, p1, __int_as_float(tot), 0.f, bad);
          }
        }
        break;
    }
    row[col] = from_float<T>(v);
  }
}

// Stand-alone Remapper.transform / inverse_transform over x [batch, time, ensemble, grid, V] (element strides ld_b .. ld_n, columns
// contiguous; y likewise and may alias x).  The program is a per-column table: op_flags int32 [V][2] = (RemapOp, flags), par fp32 [V][4].
// A thread owns one element of one ACTIVE column: `active` int32 [n_active] lists the columns whose op is not REMAP_NONE, so an in-place
// launch neither loads nor stores the others (2-4 of ~80 columns in a typical configuration); active == nullptr walks all V columns (out
// of place, where every element is copied).  viol (may be null): int32 [V], entry c counts the elements of column c that fail the reference's
// domain assertion, with an ordinary atomic add - rare by construction, the host reads it once after the launch.
template <typename T>
__global__ void remap_columns_kernel(const T* x, int64_t ld_b, int64_t ld_t, int64_t ld_e, int64_t ld_n, T* y, int64_t yd_b, int64_t yd_t,  // (y may be x)
                                     int64_t yd_e, int64_t yd_n, const int32_t* __restrict__ op_flags, const float* __restrict__ par,
                                     const int32_t* __restrict__ active, int n_active, int32_t* viol, int B, int T_steps, int E, int N, int V) {
  const int per_row = active != nullptr ? n_active : V;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T_steps * E * N * per_row) return;
  const int a = (int)(i % per_row);
  int64_t row = i / per_row;
  const int n = (int)(row % N);
  row /= N;
  const int e = (int)(row % E);
  row /= E;
  const int t = (int)(row % T_steps), b = (int)(row / T_steps);
  const int c = active != nullptr ? active[a] : a;
  const int2 of = reinterpret_cast<const int2*>(op_flags)[c];
  const float4 p = reinterpret_cast<const float4*>(par)[c];
  const T in = x[b * ld_b + t * ld_t + e * ld_e + (int64_t)n * ld_n + c];
  bool bad = false;
  const T out = of.x == REMAP_NONE ? in : from_float<T>(remap_apply<T>(to_float(in), of.x, of.y, p.x, p.y, p.z, p.w, bad));
  y[b * yd_b + t * yd_t + e * yd_e + (int64_t)n * yd_n + c] = out;
  if (bad && viol != nullptr) atomicAdd(viol + c, 1);
}

// One raw element of the chain [imputer]? Remapper InputNormalizer: impute (kind_src == nullptr: no imputer), remap forward with the
// roundings of the RAW dtype TI (the module runs on the raw tensor), then x * mul + add as the other assembly kernels.  Nothing is counted
// here: the chain's one-off first-batch check runs the member modules, with their assertion, on a copy.
template <typename TI>
__device__ __forceinline__ float edge_chain_one(float v, const TI* __restrict__ row, int cv, const int32_t* __restrict__ kind_src,
                                                const float* __restrict__ value, const int32_t* __restrict__ op_flags, const float* __restrict__ par,
                                                const float* __restrict__ mul, const float* __restrict__ add) {
  if (kind_src != nullptr && isnan(v)) {
    const int2 ks = reinterpret_cast<const int2*>(kind_src)[cv];
    if (ks.x != 0) v = ks.x == 1 ? value[cv] : to_float(row[ks.y]);
  }
  const int2 of = reinterpret_cast<const int2*>(op_flags)[cv];
  if (of.x != REMAP_NONE) {
    const float4 p = reinterpret_cast<const float4*>(par)[cv];
    bool bad = false;
    v = remap_apply<TI>(v, of.x, of.y, p.x, p.y, p.z, p.w, bad);
  }
  if (mul != nullptr) v = mul_then_add(v, mul[cv], add[cv]);
  return v;
}

// assemble_input_impute_kernel with the remap program between the imputation program (optional: kind_src / value / mask all null) and
// the normaliser.  The NaN mask of step 0 is that of the RAW input, as the imputer's own transform records it.
template <typename TI, typename TO>
__global__ void assemble_input_remap_kernel(const TI* __restrict__ x, int64_t ld_t, int64_t ldx, int T_steps, int V, const int32_t* __restrict__ kind_src,
                                            const float* __restrict__ value, uint8_t* __restrict__ mask, int64_t ldm,
                                            const int32_t* __restrict__ op_flags, const float* __restrict__ par, const float* __restrict__ mul,
                                            const float* __restrict__ add, const TO* __restrict__ attrs, int64_t lda, int A, TO* __restrict__ out,
                                            int64_t ldo, int W, int n_rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * W) return;
  const int n = (int)(i / W), c = (int)(i % W);
  float v = 0.f;
  if (c < T_steps * V) {
    const int t = c / V, cv = c % V;
    const TI* xr = x + t * ld_t + (int64_t)n * ldx;
    v = to_float(xr[cv]);
    if (mask != nullptr && t == 0) mask[(int64_t)n * ldm + cv] = isnan(v) ? 1 : 0;
    v = edge_chain_one<TI>(v, xr, cv, kind_src, value, op_flags, par, mul, add);
  } else if (c < T_steps * V + A) {
    v = to_float(attrs[(int64_t)n * lda + (c - T_steps * V)]);
  }
  out[(int64_t)n * ldo + c] = from_float<TO>(v);
}

// The same for 16-bit outputs whose width is a multiple of 8 (one 16-byte store per thread), as assemble_input_impute_vec8_kernel; the
// mask bytes of step 0 are stored one by one.
template <typename TI, typename TO>
__global__ void assemble_input_remap_vec8_kernel(const TI* __restrict__ x, int64_t ld_t, int64_t ldx, int T_steps, int V,
                                                 const int32_t* __restrict__ kind_src, const float* __restrict__ value, uint8_t* __restrict__ mask,
                                                 int64_t ldm, const int32_t* __restrict__ op_flags, const float* __restrict__ par,
                                                 const float* __restrict__ mul, const float* __restrict__ add, const TO* __restrict__ attrs, int64_t lda,
                                                 int A, TO* __restrict__ out, int64_t ldo, int W, int n_rows) {
  const int per_row = W >> 3;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * per_row) return;
  const int n = (int)(i / per_row), c0 = (int)(i % per_row) << 3;
  Vec<TO, 8> o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c0 + j;
    float v = 0.f;
    if (c < T_steps * V) {
      const int t = c / V, cv = c % V;
      const TI* xr = x + t * ld_t + (int64_t)n * ldx;
      v = to_float(xr[cv]);
      if (mask != nullptr && t == 0) mask[(int64_t)n * ldm + cv] = isnan(v) ? 1 : 0;
      v = edge_chain_one<TI>(v, xr, cv, kind_src, value, op_flags, par, mul, add);
    } else if (c < T_steps * V + A) {
      v = to_float(attrs[(int64_t)n * lda + (c - T_steps * V)]);
    }
    o.v[j] = from_float<TO>(v);
  }
  *reinterpret_cast<Vec<TO, 8>*>(out + (int64_t)n * ldo + c0) = o;
}

// assemble_output_impute_kernel whose RAW skip goes through the same chain: impute (optional), remap forward, normalise.
template <typename TM, typename TS>
__global__ void assemble_output_remap_kernel(const TM* __restrict__ x_out, int64_t ldx, const TS* __restrict__ skip, int64_t lds,
                                             const int32_t* __restrict__ col_map, const int32_t* __restrict__ kind_src, const float* __restrict__ value,
                                             const int32_t* __restrict__ op_flags, const float* __restrict__ par, const float* __restrict__ mul,
                                             const float* __restrict__ add, TS* __restrict__ out, int64_t ldo, int n_rows, int n_cols) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * n_cols) return;
  const int n = (int)(i / n_cols), v = (int)(i % n_cols);
  float val = to_float(from_float<TS>(to_float(x_out[(int64_t)n * ldx + v])));
  const int m = col_map[v];
  if (m >= 0) {
    const TS* sr = skip + (int64_t)n * lds;
    float sk = edge_chain_one<TS>(to_float(sr[m]), sr, m, kind_src, value, op_flags, par, nullptr, nullptr);
    if (mul != nullptr) sk = to_float(from_float<TS>(mul_then_add(sk, mul[m], add[m])));
    val += sk;
  }
  out[(int64_t)n * ldo + v] = from_float<TS>(val);
}

template <typename T>
static int layernorm_launch(const void* x, int64_t ldx, const void* gamma, const void* beta, const void* residual,
                            int64_t ldr, void* y, int64_t ldy, int n_rows, int D, float eps, hipStream_t st) {
  const int vec = pick_vec<T>(D, {ldx, ldy, residual ? ldr : (int64_t)0}, {x, y, gamma, beta, residual});
  const int ch = pick_chunks(D, vec);
  ANEMOI_REQUIRE(ch > 0, "layernorm_fwd: D=%d too large for the register-resident row (max %d at vector width %d)", D, 64 * vec * kMaxChunks, vec);
  static const int quarter = [] { const char* e = getenv("ANEMOI_LN_QUARTER"); return e ? atoi(e) : 1; }();
  if (quarter && sizeof(T) == 2 && vec == 8 && D == 512 && n_rows > 0) {
    // The 512-channel rows of the hot path: the quarter-wave kernel, 4 rows per wave and 16 lanes per row.  (The variant with
    // 8 rows per wave and 8 lanes per row was measured slower, +55 us per forward, and is not built.)
    const int rows_per_block = 4 * kRowWaves;
    hipLaunchKernelGGL((layernorm_fwd_q_kernel<T, 4>), dim3((n_rows + rows_per_block - 1) / rows_per_block), dim3(64 * kRowWaves), 0, st,
                       (const T*)x, ldx, (const T*)gamma, (const T*)beta, (const T*)residual, ldr, (T*)y, ldy, n_rows, eps);
    return check_launch("layernorm_fwd_q_kernel");
  }
  const dim3 grid((n_rows + kRowWaves - 1) / kRowWaves), block(64 * kRowWaves);
  const bool hit = dispatch_vec_chunks(vec, ch, [&](auto V, auto C) {
    hipLaunchKernelGGL((layernorm_fwd_kernel<T, V(), C()>), grid, block, 0, st, (const T*)x, ldx, (const T*)gamma, (const T*)beta,
                       (const T*)residual, ldr, (T*)y, ldy, n_rows, D, eps);
  });
  ANEMOI_REQUIRE(hit, "layernorm_fwd: bad vector width");
  return check_launch("layernorm_fwd_kernel");
}

template <typename T>
static int cond_layernorm_launch(const void* x, int64_t ldx, const void* scale, int64_t lds, const void* shift, int64_t ldsh, void* y,
                                 int64_t ldy, int n_rows, int D, float eps, hipStream_t st) {
  const int vec = pick_vec<T>(D, {ldx, ldy, lds, ldsh}, {x, y, scale, shift});
  const int ch = pick_chunks(D, vec);
  ANEMOI_REQUIRE(ch > 0, "cond_layernorm_fwd: D=%d too large for the register-resident row", D);
  const dim3 grid((n_rows + kRowWaves - 1) / kRowWaves), block(64 * kRowWaves);
  const bool hit = dispatch_vec_chunks(vec, ch, [&](auto V, auto C) {
    hipLaunchKernelGGL((cond_layernorm_fwd_kernel<T, V(), C()>), grid, block, 0, st, (const T*)x, ldx, (const T*)scale, lds,
                       (const T*)shift, ldsh, (T*)y, ldy, n_rows, D, eps);
  });
  ANEMOI_REQUIRE(hit, "cond_layernorm_fwd: bad vector width");
  return check_launch("cond_layernorm_fwd_kernel");
}

static int cu_count() {
  static int cached[64];
  int d = 0;
  (void)hipGetDevice(&d);
  int n = (d >= 0 && d < 64) ? cached[d] : 0;
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n <= 0) n = 256;
    if (d >= 0 && d < 64) cached[d] = n;
  }
  return n;
}

template <typename T, int VEC, int CH>
static int cond_proj_launch_vc(const T* x, int64_t ldx, const T* cond, int64_t ldc, const T* w, const T* bias, const T* residual, int64_t ldr, T* y,
                               int64_t ldy, int n_rows, int D, int C, float eps, hipStream_t st) {
  constexpr bool kRegOk = CH * VEC * sizeof(T) <= 16;  // one 16-byte chunk per lane: twice that costs 226 VGPRs (two waves per SIMD)
  const size_t image = (size_t)(2 * C + 2) * D * sizeof(T);
  const int blocks_needed = (n_rows + kProjWaves - 1) / kProjWaves;
  const dim3 block(64 * kProjWaves);
  // workgroups of 8 waves per CU.  Register form: 2 (two waves per SIMD, each with two rows in flight, and a wave amortises its weights over
  // ~10 rows of the 40 968-row hot shape) - measured at D = 512, C = 4, bf16, with / without residual: 25.8 / 23.0 us at 2, 29.2 / 26.5 at 4,
  // 32.8 / 28.7 at 8.  LDS form: as many images as fit, 4 at most (D = 1024, C = 4: 50.4 / 44.2 us at 2, 49.2 / 41.8 at 4, 50.2 / 43.6 at 8).
  static const int reg_per_cu = env_int(getenv("ANEMOI_CLNP_BLOCKS_PER_CU"), 2, 1, 8);
  if constexpr (kRegOk) {
    if (C <= kCondReg) {
      const dim3 grid(std::min(blocks_needed, cu_count() * reg_per_cu));
      hipLaunchKernelGGL((cond_layernorm_proj_fwd_kernel<T, VEC, CH, kWReg>), grid, block, 0, st, x, ldx, cond, ldc, w, bias, residual, ldr, y, ldy,
                         n_rows, D, C, eps);
      return check_launch("cond_layernorm_proj_fwd_kernel");
    }
  }
  if (image <= (size_t)kLdsBytes) {
    static PerDeviceOnce once;
    once.run([&] {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cond_layernorm_proj_fwd_kernel<T, VEC, CH, kWLds>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    });
    const int per_cu = std::max(1, std::min(4, (int)(kLdsBytes / image)));
    const dim3 grid(std::min(blocks_needed, cu_count() * per_cu));
    hipLaunchKernelGGL((cond_layernorm_proj_fwd_kernel<T, VEC, CH, kWLds>), grid, block, image, st, x, ldx, cond, ldc, w, bias, residual, ldr, y, ldy,
                       n_rows, D, C, eps);
    return check_launch("cond_layernorm_proj_fwd_kernel");
  }
  const dim3 grid(std::min(blocks_needed, cu_count() * 4));
  hipLaunchKernelGGL((cond_layernorm_proj_fwd_kernel<T, VEC, CH, kWGlobal>), grid, block, 0, st, x, ldx, cond, ldc, w, bias, residual, ldr, y, ldy,
                     n_rows, D, C, eps);
  return check_launch("cond_layernorm_proj_fwd_kernel");
}

template <typename T>
static int cond_layernorm_proj_launch(const void* x, int64_t ldx, const void* cond, int64_t ldc, const void* w, const void* bias, const void* residual,
                                      int64_t ldr, void* y, int64_t ldy, int n_rows, int D, int C, float eps, hipStream_t st) {
  const int vec = pick_vec<T>(D, {ldx, ldy, residual ? ldr : (int64_t)0}, {x, y, residual, w, bias});
  const int ch = pick_chunks(D, vec);
  ANEMOI_REQUIRE(ch > 0, "cond_layernorm_proj_fwd: D=%d too large for the register-resident row", D);
  int rc = ANEMOI_E_INVALID;
  const bool hit = dispatch_vec_chunks(vec, ch, [&](auto V, auto CC) {
    rc = cond_proj_launch_vc<T, V(), CC()>((const T*)x, ldx, (const T*)cond, ldc, (const T*)w, (const T*)bias, (const T*)residual, ldr, (T*)y, ldy,
                                           n_rows, D, C, eps, st);
  });
  ANEMOI_REQUIRE(hit, "cond_layernorm_proj_fwd: bad vector width");
  return rc;
}

template <typename T>
static int edge_launch(const void* z, int64_t ldz, const void* e_old, int64_t lde, const void* gamma, const void* beta,
                       float eps, const int32_t* colptr, void* e_new, int64_t ldn, void* agg, int64_t ldagg, int n_dst,
                       int D, hipStream_t st) {
  const int vec = pick_vec<T>(D, {ldz, lde, ldn, ldagg}, {z, e_old, e_new, agg, gamma, beta});
  const int ch = pick_chunks(D, vec);
  ANEMOI_REQUIRE(ch > 0, "edge_ln_residual_segment_sum_fwd: D=%d too large (max %d)", D, 64 * vec * kMaxChunks);
  const dim3 grid((n_dst + kRowWaves - 1) / kRowWaves), block(64 * kRowWaves);
  static const int quarter = env_int(getenv("ANEMOI_SEGSUM_QUARTER"), 2, 0, 3);  // rows per wave at a time: 1 -> four, 2 -> two, 3 -> one
  if constexpr (sizeof(T) == 2) {
    if (quarter && vec == 8 && D == 512 && gamma != nullptr && n_dst > 0) {  // the GNN's 512-channel edge rows
      if (quarter == 1)
        hipLaunchKernelGGL((edge_ln_res_segsum_kernel_mr<T, 4, 16>), grid, block, 0, st, (const T*)z, ldz, (const T*)e_old, lde, (const T*)gamma,
                           (const T*)beta, eps, colptr, (T*)e_new, ldn, (T*)agg, ldagg, n_dst);
      else if (quarter == 2)
        hipLaunchKernelGGL((edge_ln_res_segsum_kernel_mr<T, 2, 32>), grid, block, 0, st, (const T*)z, ldz, (const T*)e_old, lde, (const T*)gamma,
                           (const T*)beta, eps, colptr, (T*)e_new, ldn, (T*)agg, ldagg, n_dst);
      else
        hipLaunchKernelGGL((edge_ln_res_segsum_kernel_mr<T, 1, 64>), grid, block, 0, st, (const T*)z, ldz, (const T*)e_old, lde, (const T*)gamma,
                           (const T*)beta, eps, colptr, (T*)e_new, ldn, (T*)agg, ldagg, n_dst);
      return check_launch("edge_ln_res_segsum_kernel_mr");
    }
  }
  const bool hit = dispatch_vec_chunks(vec, ch, [&](auto V, auto C) {
    hipLaunchKernelGGL((edge_ln_res_segsum_kernel<T, V(), C()>), grid, block, 0, st, (const T*)z, ldz, (const T*)e_old, lde, (const T*)gamma,
                       (const T*)beta, eps, colptr, (T*)e_new, ldn, (T*)agg, ldagg, n_dst, D);
  });
  ANEMOI_REQUIRE(hit, "edge_ln_residual_segment_sum_fwd: bad vector width");
  return check_launch("edge_ln_res_segsum_kernel");
}

template <typename T>
static int gather_launch(const void* x, int64_t ldx, const int32_t* idx, void* out, int64_t ldo, int n_out, int D,
                         hipStream_t st) {
  const int vec = pick_vec<T>(D, {ldx, ldo}, {x, out});
  const dim3 grid((n_out + kRowWaves - 1) / kRowWaves), block(64 * kRowWaves);
  const bool hit = dispatch_vec(vec, [&](auto V) {
    hipLaunchKernelGGL((gather_rows_kernel<T, V()>), grid, block, 0, st, (const T*)x, ldx, idx, (T*)out, ldo, n_out, D);
  });
  ANEMOI_REQUIRE(hit, "gather_rows: bad vector width");
  return check_launch("gather_rows_kernel");
}

}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_layernorm_fwd(const void* x, int64_t ldx, const void* gamma, const void* beta, const void* residual,
                                    int64_t ldr, void* y, int64_t ldy, int32_t n_rows, int32_t D, float eps,
                                    anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && D > 0 && ldx >= D && ldy >= D && (!residual || ldr >= D), "layernorm_fwd: bad sizes n_rows=%d D=%d", n_rows, D);
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && y && gamma, "layernorm_fwd: null pointer");
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return layernorm_launch<T>(x, ldx, gamma, beta, residual, ldr, y, ldy, n_rows, D, eps, as_stream(stream));
  });
}

extern "C" int anemoi_edge_ln_residual_segment_sum_fwd(const void* z, int64_t ldz, const void* e_old, int64_t lde,
                                                       const void* gamma, const void* beta, float eps,
                                                       const int32_t* colptr, void* e_new, int64_t ldn, void* agg,
                                                       int64_t ldagg, int32_t n_dst, int32_t D, anemoi_dtype_t dtype,
                                                       void* stream) {
  ANEMOI_REQUIRE(n_dst >= 0 && D > 0 && ldz >= D && lde >= D && ldn >= D && ldagg >= D, "edge_ln_residual_segment_sum_fwd: bad sizes");
  if (n_dst == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(z && e_old && e_new && agg && colptr, "edge_ln_residual_segment_sum_fwd: null pointer");
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return edge_launch<T>(z, ldz, e_old, lde, gamma, beta, eps, colptr, e_new, ldn, agg, ldagg, n_dst, D, as_stream(stream));
  });
}

extern "C" int anemoi_gather_rows(const void* x, int64_t ldx, const int32_t* idx, void* out, int64_t ldo, int32_t n_out,
                                  int32_t D, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_out >= 0 && D > 0 && ldx >= D && ldo >= D, "gather_rows: bad sizes");
  if (n_out == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && idx && out, "gather_rows: null pointer");
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return gather_launch<T>(x, ldx, idx, out, ldo, n_out, D, as_stream(stream));
  });
}

extern "C" int anemoi_cond_layernorm_fwd(const void* x, int64_t ldx, const void* scale, int64_t lds, const void* shift, int64_t ldsh,
                                         void* y, int64_t ldy, int32_t n_rows, int32_t D, float eps, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && D > 0 && ldx >= D && ldy >= D && (lds == 0 || lds >= D) && (ldsh == 0 || ldsh >= D), "cond_layernorm_fwd: bad sizes");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && y && scale && shift, "cond_layernorm_fwd: null pointer");
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return cond_layernorm_launch<T>(x, ldx, scale, lds, shift, ldsh, y, ldy, n_rows, D, eps, as_stream(stream));
  });
}

extern "C" int anemoi_cond_layernorm_proj_fwd(const void* x, int64_t ldx, const void* cond, int64_t ldc, const void* w, const void* bias,
                                              const void* residual, int64_t ldr, void* y, int64_t ldy, int32_t n_rows, int32_t D, int32_t C,
                                              float eps, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && D > 0 && C > 0 && ldx >= D && ldy >= D && ldc >= C && (!residual || ldr >= D),
                 "cond_layernorm_proj_fwd: bad sizes n_rows=%d D=%d C=%d", n_rows, D, C);
  if (C > kCondMax) {
    set_error("cond_layernorm_proj_fwd: C=%d conditioning channels, the in-kernel modulation takes 1 to %d", C, kCondMax);
    return ANEMOI_E_UNSUPPORTED;
  }
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && cond && w && bias && y, "cond_layernorm_proj_fwd: null pointer");
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    return cond_layernorm_proj_launch<T>(x, ldx, cond, ldc, w, bias, residual, ldr, y, ldy, n_rows, D, C, eps, as_stream(stream));
  });
}

extern "C" int anemoi_bound_columns(void* x, int64_t ldx, int32_t n_rows, int32_t n_cols, const int32_t* ops, const float* params,
                                    int32_t n_ops, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && n_cols > 0 && ldx >= n_cols && n_ops >= 0, "bound_columns: bad sizes");
  if (n_rows == 0 || n_ops == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && ops && params, "bound_columns: null pointer");
  const dim3 grid((n_rows + 255) / 256), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((bound_columns_kernel<T>), grid, block, 0, st, (T*)x, ldx, n_rows, ops, params, n_ops);
    return check_launch("bound_columns_kernel");
  });
}

extern "C" int anemoi_assemble_output(const void* x_out, int64_t ldx, const void* x_skip, int64_t lds, const int32_t* col_map, void* out,
                                      int64_t ldo, int32_t n_rows, int32_t n_cols, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && n_cols > 0 && ldx >= n_cols && ldo >= n_cols, "assemble_output: bad sizes");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x_out && x_skip && col_map && out, "assemble_output: null pointer");
  const size_t es = dtype == ANEMOI_F32 ? 4 : 2;
  const bool q4 = n_cols % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && reinterpret_cast<uintptr_t>(x_out) % (4 * es) == 0 &&
                  reinterpret_cast<uintptr_t>(out) % (4 * es) == 0;
  const int64_t n = (int64_t)n_rows * (n_cols / (q4 ? 4 : 1));
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    dispatch_one_of<1, 4>(q4 ? 4 : 1, [&](auto Q) {
      hipLaunchKernelGGL((assemble_output_kernel<T, Q()>), grid, block, 0, st, (const T*)x_out, ldx, (const T*)x_skip, lds, col_map, (T*)out,
                         ldo, n_rows, n_cols);
    });
    return check_launch("assemble_output_kernel");
  });
}

extern "C" int anemoi_assemble_input(const void* x, int64_t ld_t, int64_t ldx, int32_t T_steps, int32_t V, const void* attrs, int64_t lda,
                                     int32_t A, void* out, int64_t ldo, int32_t W, int32_t n_rows, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && T_steps > 0 && V > 0 && A >= 0 && W >= T_steps * V + A && ldo >= W && ldx >= V && (A == 0 || lda >= A),
                 "assemble_input: bad sizes");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && out && (A == 0 || attrs), "assemble_input: null pointer");
  const size_t es = dtype == ANEMOI_F32 ? 4 : 2;
  auto al = [&](const void* p, int q) { return p == nullptr || reinterpret_cast<uintptr_t>(p) % (q * es) == 0; };
  const bool q4 = V % 4 == 0 && A % 4 == 0 && W % 4 == 0 && ld_t % 4 == 0 && ldx % 4 == 0 && lda % 4 == 0 && ldo % 4 == 0 && al(x, 4) &&
                  al(attrs, 4) && al(out, 4);
  const int q = q4 ? 4 : 1;
  const int64_t n = (int64_t)n_rows * (W / q);
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    dispatch_one_of<1, 4>(q, [&](auto Q) {
      hipLaunchKernelGGL((assemble_input_kernel<T, Q()>), grid, block, 0, st, (const T*)x, ld_t, ldx, T_steps, V, (const T*)attrs, lda, A,
                         (T*)out, ldo, W, n_rows);
    });
    return check_launch("assemble_input_kernel");
  });
}

// The two entry points below take TWO dtypes and build exactly the pairs a caller can ask for - the model dtype with itself or
// with fp32 data - so the second type is chosen inside one dispatch_dtype instead of by nesting two.
extern "C" int anemoi_assemble_input_norm(const void* x, anemoi_dtype_t x_dtype, int64_t ld_t, int64_t ldx, int32_t T_steps, int32_t V,
                                          const float* col_mul, const float* col_add, const void* attrs, int64_t lda, int32_t A, void* out,
                                          int64_t ldo, int32_t W, int32_t n_rows, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && T_steps > 0 && V > 0 && A >= 0 && W >= T_steps * V + A && ldo >= W && ldx >= V && (A == 0 || lda >= A),
                 "assemble_input_norm: bad sizes");
  ANEMOI_REQUIRE((col_mul == nullptr) == (col_add == nullptr), "assemble_input_norm: col_mul and col_add go together");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && out && (A == 0 || attrs), "assemble_input_norm: null pointer");
  ANEMOI_REQUIRE(x_dtype == dtype || x_dtype == ANEMOI_F32, "assemble_input_norm: the input is in the model dtype or fp32");
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using TO = typename decltype(t)::type;
    const bool wide_in = x_dtype == ANEMOI_F32;  // TI = float, else TI = TO
    if constexpr (sizeof(TO) == 2) {
      if (W % 8 == 0 && ldo % 8 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        const int64_t n8 = (int64_t)n_rows * (W / 8);
        const dim3 grid8((unsigned)((n8 + 255) / 256)), block8(256);
        if (wide_in)
          hipLaunchKernelGGL((assemble_input_norm_vec8_kernel<float, TO>), grid8, block8, 0, st, (const float*)x, ld_t, ldx, T_steps, V, col_mul,
                             col_add, (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
        else
          hipLaunchKernelGGL((assemble_input_norm_vec8_kernel<TO, TO>), grid8, block8, 0, st, (const TO*)x, ld_t, ldx, T_steps, V, col_mul,
                             col_add, (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
        return check_launch("assemble_input_norm_vec8_kernel");
      }
    }
    const int64_t n = (int64_t)n_rows * W;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (wide_in)
      hipLaunchKernelGGL((assemble_input_norm_kernel<float, TO>), grid, block, 0, st, (const float*)x, ld_t, ldx, T_steps, V, col_mul, col_add,
                         (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
    else
      hipLaunchKernelGGL((assemble_input_norm_kernel<TO, TO>), grid, block, 0, st, (const TO*)x, ld_t, ldx, T_steps, V, col_mul, col_add,
                         (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
    return check_launch("assemble_input_norm_kernel");
  });
}

extern "C" int anemoi_assemble_output_norm(const void* x_out, int64_t ldx, anemoi_dtype_t model_dtype, const void* x_skip, int64_t lds,
                                           const int32_t* col_map, const float* col_mul, const float* col_add, void* out, int64_t ldo,
                                           int32_t n_rows, int32_t n_cols, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && n_cols > 0 && ldx >= n_cols && ldo >= n_cols, "assemble_output_norm: bad sizes");
  ANEMOI_REQUIRE((col_mul == nullptr) == (col_add == nullptr), "assemble_output_norm: col_mul and col_add go together");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x_out && x_skip && col_map && out, "assemble_output_norm: null pointer");
  ANEMOI_REQUIRE(model_dtype == dtype || dtype == ANEMOI_F32, "assemble_output_norm: the output is in the model dtype or fp32");
  const int64_t n = (int64_t)n_rows * n_cols;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(model_dtype, [&](auto t) {
    using TM = typename decltype(t)::type;
    if (dtype == ANEMOI_F32)  // TS = float, else TS = TM
      hipLaunchKernelGGL((assemble_output_norm_kernel<TM, float>), grid, block, 0, st, (const TM*)x_out, ldx, (const float*)x_skip, lds, col_map,
                         col_mul, col_add, (float*)out, ldo, n_rows, n_cols);
    else
      hipLaunchKernelGGL((assemble_output_norm_kernel<TM, TM>), grid, block, 0, st, (const TM*)x_out, ldx, (const TM*)x_skip, lds, col_map,
                         col_mul, col_add, (TM*)out, ldo, n_rows, n_cols);
    return check_launch("assemble_output_norm_kernel");
  });
}

extern "C" int anemoi_affine_columns(const void* x, int64_t ldx, void* y, int64_t ldy, const float* col_mul, const float* col_add,
                                     int32_t inverse, int32_t n_rows, int32_t V, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && V > 0 && ldx >= V && ldy >= V, "affine_columns: bad sizes");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && y && col_mul && col_add, "affine_columns: null pointer");
  const int64_t n = (int64_t)n_rows * V;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((affine_columns_kernel<T>), grid, block, 0, st, (const T*)x, ldx, (T*)y, ldy, col_mul, col_add, inverse, n_rows, V);
    return check_launch("affine_columns_kernel");
  });
}

// ---- imputers (see the kernels above) ------------------------------------------------------------------------------------------------------
extern "C" int anemoi_impute_columns(const void* x, int64_t ld_b, int64_t ld_t, int64_t ld_e, int64_t ld_n, void* y, int64_t yd_b, int64_t yd_t,
                                     int64_t yd_e, int64_t yd_n, const int32_t* kind_src, const float* value, void* mask, int32_t B, int32_t T_steps,
                                     int32_t E, int32_t N, int32_t V, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(B >= 0 && T_steps >= 0 && E >= 0 && N >= 0 && V > 0 && ld_n >= V && yd_n >= V, "impute_columns: bad sizes");
  const int64_t n = (int64_t)B * T_steps * N * V;
  if (n == 0 || E == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && y && kind_src && value, "impute_columns: null pointer");
  ANEMOI_REQUIRE((n + 255) / 256 <= 0x7fffffffLL, "impute_columns: too many elements for one launch");
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((impute_columns_kernel<T>), grid, block, 0, st, (const T*)x, ld_b, ld_t, ld_e, ld_n, (T*)y, yd_b, yd_t, yd_e, yd_n, kind_src,
                       value, (uint8_t*)mask, B, T_steps, E, N, V);
    return check_launch("impute_columns_kernel");
  });
}

extern "C" int anemoi_restore_nan_columns(const void* x, int64_t ldx, void* y, int64_t ldy, const void* mask, int64_t ldm, int32_t n_mask_cols,
                                          const int32_t* src_of, int32_t B, int32_t M, int32_t N, int32_t V, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(B >= 0 && M >= 0 && N >= 0 && V > 0 && ldx >= V && ldy >= V && n_mask_cols > 0 && ldm >= n_mask_cols, "restore_nan_columns: bad sizes");
  const int64_t n = (int64_t)B * M * N * V;
  if (n == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && y && mask && src_of, "restore_nan_columns: null pointer");
  ANEMOI_REQUIRE((n + 255) / 256 <= 0x7fffffffLL, "restore_nan_columns: too many elements for one launch");
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((restore_nan_columns_kernel<T>), grid, block, 0, st, (const T*)x, ldx, (T*)y, ldy, (const uint8_t*)mask, ldm, n_mask_cols, src_of, B, M, N, V);
    return check_launch("restore_nan_columns_kernel");
  });
}

extern "C" int anemoi_assemble_input_impute(const void* x, anemoi_dtype_t x_dtype, int64_t ld_t, int64_t ldx, int32_t T_steps, int32_t V,
                                            const int32_t* kind_src, const float* value, void* mask, int64_t ldm, const float* col_mul,
                                            const float* col_add, const void* attrs, int64_t lda, int32_t A, void* out, int64_t ldo, int32_t W,
                                            int32_t n_rows, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && T_steps > 0 && V > 0 && A >= 0 && W >= T_steps * V + A && ldo >= W && ldx >= V && (A == 0 || lda >= A) && ldm >= V,
                 "assemble_input_impute: bad sizes");
  ANEMOI_REQUIRE((col_mul == nullptr) == (col_add == nullptr), "assemble_input_impute: col_mul and col_add go together");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && out && kind_src && value && mask && (A == 0 || attrs), "assemble_input_impute: null pointer");
  ANEMOI_REQUIRE(x_dtype == dtype || x_dtype == ANEMOI_F32, "assemble_input_impute: the input is in the model dtype or fp32");
  hipStream_t st = as_stream(stream);
  uint8_t* mk = (uint8_t*)mask;
  return dispatch_dtype(dtype, [&](auto t) {
    using TO = typename decltype(t)::type;
    const bool wide_in = x_dtype == ANEMOI_F32;  // TI = float, else TI = TO
    if constexpr (sizeof(TO) == 2) {
      if (W % 8 == 0 && ldo % 8 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        const int64_t n8 = (int64_t)n_rows * (W / 8);
        const dim3 grid8((unsigned)((n8 + 255) / 256)), block8(256);
        if (wide_in)
          hipLaunchKernelGGL((assemble_input_impute_vec8_kernel<float, TO>), grid8, block8, 0, st, (const float*)x, ld_t, ldx, T_steps, V, kind_src,
                             value, mk, ldm, col_mul, col_add, (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
        else
          hipLaunchKernelGGL((assemble_input_impute_vec8_kernel<TO, TO>), grid8, block8, 0, st, (const TO*)x, ld_t, ldx, T_steps, V, kind_src, value,
                             mk, ldm, col_mul, col_add, (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
        return check_launch("assemble_input_impute_vec8_kernel");
      }
    }
    const int64_t n = (int64_t)n_rows * W;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (wide_in)
      hipLaunchKernelGGL((assemble_input_impute_kernel<float, TO>), grid, block, 0, st, (const float*)x, ld_t, ldx, T_steps, V, kind_src, value, mk, ldm,
                         col_mul, col_add, (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
    else
      hipLaunchKernelGGL((assemble_input_impute_kernel<TO, TO>), grid, block, 0, st, (const TO*)x, ld_t, ldx, T_steps, V, kind_src, value, mk, ldm,
                         col_mul, col_add, (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
    return check_launch("assemble_input_impute_kernel");
  });
}

extern "C" int anemoi_assemble_output_impute(const void* x_out, int64_t ldx, anemoi_dtype_t model_dtype, const void* x_skip, int64_t lds,
                                             const int32_t* col_map, const int32_t* kind_src, const float* value, const float* col_mul,
                                             const float* col_add, void* out, int64_t ldo, int32_t n_rows, int32_t n_cols, anemoi_dtype_t dtype,
                                             void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && n_cols > 0 && ldx >= n_cols && ldo >= n_cols, "assemble_output_impute: bad sizes");
  ANEMOI_REQUIRE((col_mul == nullptr) == (col_add == nullptr), "assemble_output_impute: col_mul and col_add go together");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x_out && x_skip && col_map && out && kind_src && value, "assemble_output_impute: null pointer");
  ANEMOI_REQUIRE(model_dtype == dtype || dtype == ANEMOI_F32, "assemble_output_impute: the output is in the model dtype or fp32");
  const int64_t n = (int64_t)n_rows * n_cols;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(model_dtype, [&](auto t) {
    using TM = typename decltype(t)::type;
    if (dtype == ANEMOI_F32)  // TS = float, else TS = TM
      hipLaunchKernelGGL((assemble_output_impute_kernel<TM, float>), grid, block, 0, st, (const TM*)x_out, ldx, (const float*)x_skip, lds, col_map,
                         kind_src, value, col_mul, col_add, (float*)out, ldo, n_rows, n_cols);
    else
      hipLaunchKernelGGL((assemble_output_impute_kernel<TM, TM>), grid, block, 0, st, (const TM*)x_out, ldx, (const TM*)x_skip, lds, col_map, kind_src,
                         value, col_mul, col_add, (TM*)out, ldo, n_rows, n_cols);
    return check_launch("assemble_output_impute_kernel");
  });
}

extern "C" int anemoi_bound_columns_mask(void* x, int64_t ldx, int32_t n_rows, int32_t n_cols, const int32_t* ops, const float* params, int32_t n_ops,
                                         const void* mask, int64_t ldm, int32_t n_mask_cols, int32_t n_nan_ops, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && n_cols > 0 && ldx >= n_cols && n_ops >= 0 && n_nan_ops >= 0 && n_nan_ops <= n_ops, "bound_columns_mask: bad sizes");
  ANEMOI_REQUIRE(n_nan_ops == 0 || mask != nullptr, "bound_columns_mask: the program has ops of kind 10 (NaN where mask) but no mask was given");
  if (mask == nullptr) return anemoi_bound_columns(x, ldx, n_rows, n_cols, ops, params, n_ops, dtype, stream);
  ANEMOI_REQUIRE(n_mask_cols > 0 && ldm >= n_mask_cols, "bound_columns_mask: bad mask sizes");
  if (n_rows == 0 || n_ops == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && ops && params, "bound_columns_mask: null pointer");
  const dim3 grid((n_rows + 255) / 256), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((bound_columns_mask_kernel<T, false>), grid, block, 0, st, (T*)x, ldx, n_rows, ops, params, n_ops, (const uint8_t*)mask, ldm, n_mask_cols);
    return check_launch("bound_columns_mask_kernel");
  });
}

// ---- remapper and post-processors (see remap_core.h and the kernels above) -------------------------------------------------------------
extern "C" int anemoi_remap_columns(const void* x, int64_t ld_b, int64_t ld_t, int64_t ld_e, int64_t ld_n, void* y, int64_t yd_b, int64_t yd_t,
                                    int64_t yd_e, int64_t yd_n, const int32_t* op_flags, const float* par, const int32_t* active, int32_t n_active,
                                    int32_t* violations, int32_t B, int32_t T_steps, int32_t E, int32_t N, int32_t V, anemoi_dtype_t dtype,
                                    void* stream) {
  ANEMOI_REQUIRE(B >= 0 && T_steps >= 0 && E >= 0 && N >= 0 && V > 0 && ld_n >= V && yd_n >= V, "remap_columns: bad sizes");
  ANEMOI_REQUIRE(n_active >= 0 && n_active <= V, "remap_columns: n_active must lie in [0, V]");
  ANEMOI_REQUIRE(active != nullptr || x != y || n_active == V, "remap_columns: an in-place launch takes the list of active columns");
  const int64_t n = (int64_t)B * T_steps * E * N * (active != nullptr ? n_active : V);
  if (n == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && y && op_flags && par, "remap_columns: null pointer");
  ANEMOI_REQUIRE((reinterpret_cast<uintptr_t>(op_flags) & 7) == 0 && (reinterpret_cast<uintptr_t>(par) & 15) == 0,
                 "remap_columns: the program tables must be 8- / 16-byte aligned");
  ANEMOI_REQUIRE((n + 255) / 256 <= 0x7fffffffLL, "remap_columns: too many elements for one launch");
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((remap_columns_kernel<T>), grid, block, 0, st, (const T*)x, ld_b, ld_t, ld_e, ld_n, (T*)y, yd_b, yd_t, yd_e, yd_n, op_flags, par,
                       active, n_active, violations, B, T_steps, E, N, V);
    return check_launch("remap_columns_kernel");
  });
}

extern "C" int anemoi_column_program(void* x, int64_t ldx, int32_t n_rows, int32_t n_cols, const int32_t* ops, const float* params, int32_t n_ops,
                                     const void* mask, int64_t ldm, int32_t n_mask_cols, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && n_cols > 0 && ldx >= n_cols && n_ops >= 0, "column_program: bad sizes");
  ANEMOI_REQUIRE(mask == nullptr ? n_mask_cols == 0 : (n_mask_cols > 0 && ldm >= n_mask_cols), "column_program: bad mask sizes");
  if (n_rows == 0 || n_ops == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && ops && params, "column_program: null pointer");
  const dim3 grid((n_rows + 255) / 256), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((bound_columns_mask_kernel<T, true>), grid, block, 0, st, (T*)x, ldx, n_rows, ops, params, n_ops, (const uint8_t*)mask, ldm, n_mask_cols);
    return check_launch("column_program_kernel");
  });
}

static bool remap_tables_aligned(const int32_t* op_flags, const float* par, const int32_t* kind_src) {
  return (reinterpret_cast<uintptr_t>(op_flags) & 7) == 0 && (reinterpret_cast<uintptr_t>(par) & 15) == 0 && (reinterpret_cast<uintptr_t>(kind_src) & 7) == 0;
}

extern "C" int anemoi_assemble_input_remap(const void* x, anemoi_dtype_t x_dtype, int64_t ld_t, int64_t ldx, int32_t T_steps, int32_t V,
                                           const int32_t* kind_src, const float* value, void* mask, int64_t ldm, const int32_t* op_flags,
                                           const float* par, const float* col_mul, const float* col_add, const void* attrs, int64_t lda, int32_t A,
                                           void* out, int64_t ldo, int32_t W, int32_t n_rows, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && T_steps > 0 && V > 0 && A >= 0 && W >= T_steps * V + A && ldo >= W && ldx >= V && (A == 0 || lda >= A),
                 "assemble_input_remap: bad sizes");
  ANEMOI_REQUIRE((col_mul == nullptr) == (col_add == nullptr), "assemble_input_remap: col_mul and col_add go together");
  ANEMOI_REQUIRE((kind_src == nullptr) == (value == nullptr) && (kind_src == nullptr) == (mask == nullptr),
                 "assemble_input_remap: the imputation program, its values and the mask go together");
  ANEMOI_REQUIRE(mask == nullptr || ldm >= V, "assemble_input_remap: bad mask sizes");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && out && op_flags && par && (A == 0 || attrs), "assemble_input_remap: null pointer");
  ANEMOI_REQUIRE(remap_tables_aligned(op_flags, par, kind_src), "assemble_input_remap: the program tables must be 8- / 16-byte aligned");
  ANEMOI_REQUIRE(x_dtype == dtype || x_dtype == ANEMOI_F32, "assemble_input_remap: the input is in the model dtype or fp32");
  hipStream_t st = as_stream(stream);
  uint8_t* mk = (uint8_t*)mask;
  return dispatch_dtype(dtype, [&](auto t) {
    using TO = typename decltype(t)::type;
    const bool wide_in = x_dtype == ANEMOI_F32;  // TI = float, else TI = TO
    if constexpr (sizeof(TO) == 2) {
      if (W % 8 == 0 && ldo % 8 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        const int64_t n8 = (int64_t)n_rows * (W / 8);
        const dim3 grid8((unsigned)((n8 + 255) / 256)), block8(256);
        if (wide_in)
          hipLaunchKernelGGL((assemble_input_remap_vec8_kernel<float, TO>), grid8, block8, 0, st, (const float*)x, ld_t, ldx, T_steps, V, kind_src,
                             value, mk, ldm, op_flags, par, col_mul, col_add, (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
        else
          hipLaunchKernelGGL((assemble_input_remap_vec8_kernel<TO, TO>), grid8, block8, 0, st, (const TO*)x, ld_t, ldx, T_steps, V, kind_src, value,
                             mk, ldm, op_flags, par, col_mul, col_add, (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
        return check_launch("assemble_input_remap_vec8_kernel");
      }
    }
    const int64_t n = (int64_t)n_rows * W;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (wide_in)
      hipLaunchKernelGGL((assemble_input_remap_kernel<float, TO>), grid, block, 0, st, (const float*)x, ld_t, ldx, T_steps, V, kind_src, value, mk, ldm,
                         op_flags, par, col_mul, col_add, (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
    else
      hipLaunchKernelGGL((assemble_input_remap_kernel<TO, TO>), grid, block, 0, st, (const TO*)x, ld_t, ldx, T_steps, V, kind_src, value, mk, ldm,
                         op_flags, par, col_mul, col_add, (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
    return check_launch("assemble_input_remap_kernel");
  });
}

extern "C" int anemoi_assemble_output_remap(const void* x_out, int64_t ldx, anemoi_dtype_t model_dtype, const void* x_skip, int64_t lds,
                                            const int32_t* col_map, const int32_t* kind_src, const float* value, const int32_t* op_flags,
                                            const float* par, const float* col_mul, const float* col_add, void* out, int64_t ldo, int32_t n_rows,
                                            int32_t n_cols, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && n_cols > 0 && ldx >= n_cols && ldo >= n_cols, "assemble_output_remap: bad sizes");
  ANEMOI_REQUIRE((col_mul == nullptr) == (col_add == nullptr), "assemble_output_remap: col_mul and col_add go together");
  ANEMOI_REQUIRE((kind_src == nullptr) == (value == nullptr), "assemble_output_remap: the imputation program and its values go together");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x_out && x_skip && col_map && out && op_flags && par, "assemble_output_remap: null pointer");
  ANEMOI_REQUIRE(remap_tables_aligned(op_flags, par, kind_src), "assemble_output_remap: the program tables must be 8- / 16-byte aligned");
  ANEMOI_REQUIRE(model_dtype == dtype || dtype == ANEMOI_F32, "assemble_output_remap: the output is in the model dtype or fp32");
  const int64_t n = (int64_t)n_rows * n_cols;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(model_dtype, [&](auto t) {
    using TM = typename decltype(t)::type;
    if (dtype == ANEMOI_F32)  // TS = float, else TS = TM
      hipLaunchKernelGGL((assemble_output_remap_kernel<TM, float>), grid, block, 0, st, (const TM*)x_out, ldx, (const float*)x_skip, lds, col_map,
                         kind_src, value, op_flags, par, col_mul, col_add, (float*)out, ldo, n_rows, n_cols);
    else
      hipLaunchKernelGGL((assemble_output_remap_kernel<TM, TM>), grid, block, 0, st, (const TM*)x_out, ldx, (const TM*)x_skip, lds, col_map, kind_src,
                         value, op_flags, par, col_mul, col_add, (TM*)out, ldo, n_rows, n_cols);
    return check_launch("assemble_output_remap_kernel");
  });
}
