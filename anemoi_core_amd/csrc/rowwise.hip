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
