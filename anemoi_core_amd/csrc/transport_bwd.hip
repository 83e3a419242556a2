// Backward of the three launches around the denoiser network of the EDM diffusion model (transport.hip): the gradients of the noise MLP's
// parameters, of the node attributes the input assembly concatenates, and of the network's output rows.  As in the forward, every per-call
// scalar (sigma, the conditioning values) is read from DEVICE memory, so a captured training step replays.  fp32 accumulation in a fixed
// order, plain stores with one owner per output element, no atomics: two runs, or a replay, give the same bits.
#include "transport_core.h"  // the forward's own EDM coefficients and conditioning vector

namespace anemoi {
namespace {

constexpr int kBwdThreads = 256;

// ---------------------------------------------------------------------------------------------- 1. noise conditioning, stage 1
// grid (G, tiles of destination 0 + tiles of destination 1), the forward's tiling: workgroup (g, tile) sums the rows of its tile of dOut_k
// column by column and writes cond_dim fp32 partials to ws[(g tiles + tile) cond_dim + col].  VEC columns per load (16 bytes when VEC > 1);
// thread t owns column chunk t % chunks of the rows t / chunks, t / chunks + rows_per_pass, ..; the per-thread sums meet in LDS and are
// folded by a halving tree whose shape depends on the launch shape alone.
template <typename T, int VEC>
__global__ __launch_bounds__(kBwdThreads) void noise_cond_bwd_partial_kernel(const T* __restrict__ d0, int64_t rows0, int64_t ld0, int tiles0,
                                                                             const T* __restrict__ d1, int64_t rows1, int64_t ld1,
                                                                             int cond_dim, float* __restrict__ ws) {
  __shared__ float red[kBwdThreads * VEC];
  const int g = blockIdx.x, t = threadIdx.x;
  const bool first = (int)blockIdx.y < tiles0;
  const T* d = first ? d0 : d1;
  const int64_t rows = first ? rows0 : rows1, ld = first ? ld0 : ld1;
  const int64_t r0 = (int64_t)(first ? blockIdx.y : blockIdx.y - tiles0) * kCondTileRows;
  const int n_rows = (int)(rows - r0 < kCondTileRows ? rows - r0 : kCondTileRows);
  d += ((int64_t)g * rows + r0) * ld;
  const int chunks = cond_dim / VEC, rows_per_pass = kBwdThreads / chunks;  // chunks <= 32: rows_per_pass >= 8
  const int rr = t / chunks, c0 = (t - rr * chunks) * VEC;
  if (rr < rows_per_pass) {
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
    for (int row = rr; row < n_rows; row += rows_per_pass) {
      float v[VEC];
      load_vec<T, VEC>(d + (int64_t)row * ld + c0, v);
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[j] += v[j];
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) red[rr * cond_dim + c0 + j] = acc[j];
  }
  int n = rows_per_pass, p2 = 1;
  while (p2 < n) p2 <<= 1;
  for (int s = p2 >> 1; s > 0; s >>= 1) {
    __syncthreads();
    for (int i = t; i < s * cond_dim; i += kBwdThreads) {
      const int r = i / cond_dim;
      if (r + s < n) red[i] += red[i + s * cond_dim];
    }
    n = n < s ? n : s;
  }
  __syncthreads();
  if (t < cond_dim) ws[((int64_t)g * gridDim.y + blockIdx.y) * cond_dim + t] = red[t];
}

// ---------------------------------------------------------------------------------------------- 1. noise conditioning, stage 2
// One workgroup.  Per group, in group order: s = the sum of the group's partials in tile order; e, p, h recomputed by the forward's helper;
// db2 += s, dW2 += s h^T, dh = W2^T s, dp = dh silu'(p), db1 += dp, dW1 += dp e^T.  Thread t holds the running sums of the weight elements
// t, t + 256, .. in registers and writes them once.
template <typename TV, typename TW>
__global__ __launch_bounds__(kBwdThreads) void noise_cond_bwd_kernel(const float* __restrict__ ws, int tiles, const TV* __restrict__ values,
                                                                     int transform, const float* __restrict__ freq, const float* __restrict__ pi,
                                                                     const TW* __restrict__ w1, const TW* __restrict__ b1, const TW* __restrict__ w2,
                                                                     const TW* __restrict__ b2, float* __restrict__ dw1, float* __restrict__ db1,
                                                                     float* __restrict__ dw2, float* __restrict__ db2, int G, int C, int cond_dim) {
  constexpr int kW1 = kNoiseChannelsMax * kNoiseChannelsMax / kBwdThreads, kW2 = kNoiseCondMax * kNoiseChannelsMax / kBwdThreads;
  __shared__ float emb[kNoiseChannelsMax], pre[kNoiseChannelsMax], hid[kNoiseChannelsMax], cnd[kNoiseCondMax], s[kNoiseCondMax], dp[kNoiseChannelsMax];
  const int t = threadIdx.x;
  float a_w1[kW1], a_w2[kW2], a_b1 = 0.f, a_b2 = 0.f;
#pragma unroll
  for (int j = 0; j < kW1; ++j) a_w1[j] = 0.f;
#pragma unroll
  for (int j = 0; j < kW2; ++j) a_w2[j] = 0.f;
  for (int g = 0; g < G; ++g) {
    if (t < cond_dim) {
      float acc = 0.f;
      for (int tile = 0; tile < tiles; ++tile) acc += ws[((int64_t)g * tiles + tile) * cond_dim + t];
      s[t] = acc;
    }
    noise_cond_vector<TW>((float)values[g], transform, freq, pi, w1, b1, w2, b2, C, cond_dim, emb, pre, hid, cnd);  // (ends with a barrier)
    if (t < cond_dim) a_b2 += s[t];
#pragma unroll
    for (int j = 0; j < kW2; ++j) {
      const int i = t + j * kBwdThreads;
      if (i < cond_dim * C) a_w2[j] = fmaf(s[i / C], hid[i % C], a_w2[j]);
    }
    if (t < C) {
      float dh = 0.f;
      for (int o = 0; o < cond_dim; ++o) dh = fmaf(to_float(w2[o * C + t]), s[o], dh);
      const float p = pre[t], sig = 1.0f / (1.0f + expf(-p));
      const float v = dh * (sig * (1.0f + p * (1.0f - sig)));
      dp[t] = v;
      a_b1 += v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kW1; ++j) {
      const int i = t + j * kBwdThreads;
      if (i < C * C) a_w1[j] = fmaf(dp[i / C], emb[i % C], a_w1[j]);
    }
    __syncthreads();  // the next group overwrites s, emb, dp
  }
  if (t < cond_dim) db2[t] = a_b2;
  if (t < C) db1[t] = a_b1;
#pragma unroll
  for (int j = 0; j < kW2; ++j) {
    const int i = t + j * kBwdThreads;
    if (i < cond_dim * C) dw2[i] = a_w2[j];
  }
#pragma unroll
  for (int j = 0; j < kW1; ++j) {
    const int i = t + j * kBwdThreads;
    if (i < C * C) dw1[i] = a_w1[j];
  }
}

// ---------------------------------------------------------------------------------------------- 2. input assembly
// d_attrs[n, a] = the sum over the groups, in group order, of the attribute columns of the assembled rows' gradient.
template <typename T>
__global__ __launch_bounds__(kBwdThreads) void transport_assemble_bwd_kernel(const T* __restrict__ d_rows, int64_t ldr, int col0, T* __restrict__ d_attrs,
                                                                             int64_t lda, int G, int N, int A) {
  const int64_t idx = (int64_t)blockIdx.x * kBwdThreads + threadIdx.x;
  if (idx >= (int64_t)N * A) return;
  const int64_t n = idx / A;
  const int a = (int)(idx - n * A);
  float acc = 0.f;
  for (int g = 0; g < G; ++g) acc += to_float(d_rows[((int64_t)g * N + n) * ldr + col0 + a]);
  d_attrs[n * lda + a] = from_float<T>(acc);
}

// ---------------------------------------------------------------------------------------------- 3. output assembly
// One element of d_pred [B E N, P] per thread: columns below T_out V_out take c_out times the matching element of dOut, read through its five
// element strides (any of them may be 0: an expanded gradient); the columns beyond are zeros.
template <typename TP, typename TG, typename TS>
__global__ __launch_bounds__(kBwdThreads) void edm_output_bwd_kernel(const TG* __restrict__ d_out, int64_t gs_b, int64_t gs_t, int64_t gs_e, int64_t gs_n,
                                                                     int64_t gs_v, const TS* __restrict__ sigma, float sd, float sd2, int precondition,
                                                                     TP* __restrict__ d_pred, int64_t ldp, int P, int E, int N, int T_out, int V_out,
                                                                     int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kBwdThreads + threadIdx.x;  // over [B E N, P]
  if (idx >= total) return;
  const int64_t row = idx / P;
  const int col = (int)(idx - row * P);
  float r = 0.f;
  if (col < T_out * V_out) {
    const int g = (int)(row / N), n = (int)(row - (int64_t)g * N), b = g / E, e = g - b * E, t = col / V_out, v = col - t * V_out;
    r = (float)d_out[b * gs_b + t * gs_t + e * gs_e + n * gs_n + v * gs_v];
    if (precondition) r = __fmul_rn(edm_coefficients((float)sigma[g], sd, sd2).c_out, r);
  }
  d_pred[row * ldp + col] = from_float<TP>(r);
}

int64_t cond_tiles(int64_t rows) { return (rows + kCondTileRows - 1) / kCondTileRows; }

}  // namespace
}  // namespace anemoi

using namespace anemoi;

extern "C" int64_t anemoi_noise_cond_bwd_workspace_bytes(int64_t rows0, int64_t rows1, int32_t G, int32_t cond_dim) {
  if (rows0 < 0 || rows1 < 0 || G < 0 || cond_dim < 0) return 0;
  return (int64_t)G * (cond_tiles(rows0) + cond_tiles(rows1)) * cond_dim * (int64_t)sizeof(float);
}

extern "C" int anemoi_noise_cond_bwd(const void* d_out0, int64_t rows0, int64_t ld0, const void* d_out1, int64_t rows1, int64_t ld1,
                                     anemoi_dtype_t dtype, const void* values, int32_t values_f64, int32_t transform, const float* frequencies,
                                     const float* pi, const void* w1, const void* b1, const void* w2, const void* b2, anemoi_dtype_t w_dtype,
                                     float* d_w1, float* d_b1, float* d_w2, float* d_b2, void* workspace, int64_t workspace_bytes, int32_t G, int32_t C,
                                     int32_t cond_dim, void* stream) {
  ANEMOI_REQUIRE(values && frequencies && w1 && b1 && w2 && b2 && d_w1 && d_b1 && d_w2 && d_b2, "noise_cond_bwd: null pointer");
  ANEMOI_REQUIRE(G >= 0 && C >= 2 && C % 2 == 0 && cond_dim >= 1, "noise_cond_bwd: bad shape G=%d C=%d cond_dim=%d", G, C, cond_dim);
  ANEMOI_REQUIRE(transform == 0 || transform == 1, "noise_cond_bwd: transform %d (0 = identity, 1 = log / 4)", transform);
  if (C > kNoiseChannelsMax || cond_dim > kNoiseCondMax) {
    set_error("noise_cond_bwd: C=%d, cond_dim=%d beyond the built limits %d, %d", C, cond_dim, kNoiseChannelsMax, kNoiseCondMax);
    return ANEMOI_E_UNSUPPORTED;
  }
  if (d_out0 == nullptr) rows0 = 0;
  if (d_out1 == nullptr) rows1 = 0;
  ANEMOI_REQUIRE(rows0 >= 0 && rows1 >= 0 && (rows0 == 0 || ld0 >= cond_dim) && (rows1 == 0 || ld1 >= cond_dim),
                 "noise_cond_bwd: bad gradient rows=%lld,%lld ld=%lld,%lld", (long long)rows0, (long long)rows1, (long long)ld0, (long long)ld1);
  const int64_t tiles0 = cond_tiles(rows0), tiles1 = cond_tiles(rows1), tiles = tiles0 + tiles1;
  ANEMOI_REQUIRE(tiles <= 65535, "noise_cond_bwd: %lld row tiles exceed the grid", (long long)tiles);
  const int64_t need = anemoi_noise_cond_bwd_workspace_bytes(rows0, rows1, G, cond_dim);
  ANEMOI_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need), "noise_cond_bwd: workspace of %lld bytes, %lld needed",
                 (long long)workspace_bytes, (long long)need);
  hipStream_t st = as_stream(stream);
  float* ws = (float*)workspace;
  int rc = ANEMOI_OK;
  if (G > 0 && tiles > 0) {
    const dim3 grid((unsigned)G, (unsigned)tiles);
    rc = dispatch_dtype(dtype, [&](auto td) {
      using T = typename decltype(td)::type;
      constexpr int kVec = 16 / (int)sizeof(T);
      auto aligned = [&](const void* p, int64_t rows, int64_t ld) {
        return rows == 0 || (ld % kVec == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0);
      };
      if (cond_dim % kVec == 0 && aligned(d_out0, rows0, ld0) && aligned(d_out1, rows1, ld1)) {
        hipLaunchKernelGGL((noise_cond_bwd_partial_kernel<T, kVec>), grid, dim3(kBwdThreads), 0, st, (const T*)d_out0, rows0, ld0, (int)tiles0,
                           (const T*)d_out1, rows1, ld1, cond_dim, ws);
      } else {
        hipLaunchKernelGGL((noise_cond_bwd_partial_kernel<T, 1>), grid, dim3(kBwdThreads), 0, st, (const T*)d_out0, rows0, ld0, (int)tiles0,
                           (const T*)d_out1, rows1, ld1, cond_dim, ws);
      }
      return check_launch("noise_cond_bwd_partial_kernel");
    });
    if (rc != ANEMOI_OK) return rc;
  }
  // (G = 0 or no rows at all: stage 2 alone writes zeros)
  return dispatch_real(values_f64, [&](auto tv) {
    using TV = typename decltype(tv)::type;
    return dispatch_dtype(w_dtype, [&](auto tw) {
      using TW = typename decltype(tw)::type;
      hipLaunchKernelGGL((noise_cond_bwd_kernel<TV, TW>), dim3(1), dim3(kBwdThreads), 0, st, ws, (int)tiles, (const TV*)values, transform, frequencies,
                         pi, (const TW*)w1, (const TW*)b1, (const TW*)w2, (const TW*)b2, d_w1, d_b1, d_w2, d_b2, G, C, cond_dim);
      return check_launch("noise_cond_bwd_kernel");
    });
  });
}

extern "C" int anemoi_transport_assemble_input_bwd(const void* d_rows, int64_t ldr, int32_t col0, void* d_attrs, int64_t lda, int32_t G, int32_t N,
                                                   int32_t A, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(d_rows && d_attrs, "transport_assemble_input_bwd: null pointer");
  ANEMOI_REQUIRE(G >= 0 && N >= 0 && A >= 1 && col0 >= 0 && ldr >= (int64_t)col0 + A && lda >= A,
                 "transport_assemble_input_bwd: bad shape G=%d N=%d A=%d col0=%d ldr=%lld lda=%lld", G, N, A, col0, (long long)ldr, (long long)lda);
  ANEMOI_REQUIRE(grid_fits((int64_t)N * A), "transport_assemble_input_bwd: %lld elements exceed the grid", (long long)N * A);
  if (N == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto td) {
    using T = typename decltype(td)::type;
    hipLaunchKernelGGL((transport_assemble_bwd_kernel<T>), grid_for((int64_t)N * A), dim3(kBwdThreads), 0, st, (const T*)d_rows, ldr, col0, (T*)d_attrs,
                       lda, G, N, A);
    return check_launch("transport_assemble_bwd_kernel");
  });
}

extern "C" int anemoi_edm_output_bwd(const void* d_out, int32_t d_out_f64, int64_t gs_b, int64_t gs_t, int64_t gs_e, int64_t gs_n, int64_t gs_v,
                                     const void* sigma, int32_t sigma_f64, double sigma_data, int32_t precondition, void* d_pred, int64_t ldp,
                                     int32_t P, anemoi_dtype_t pred_dtype, int32_t B, int32_t E, int32_t N, int32_t T_out, int32_t V_out, void* stream) {
  ANEMOI_REQUIRE(d_out && d_pred, "edm_output_bwd: null pointer");
  ANEMOI_REQUIRE(B >= 0 && E >= 1 && N >= 0 && T_out >= 1 && V_out >= 1 && P >= (int64_t)T_out * V_out && ldp >= P,
                 "edm_output_bwd: bad shape B=%d E=%d N=%d T_out=%d V_out=%d P=%d ldp=%lld", B, E, N, T_out, V_out, P, (long long)ldp);
  ANEMOI_REQUIRE(gs_b >= 0 && gs_t >= 0 && gs_e >= 0 && gs_n >= 0 && gs_v >= 0, "edm_output_bwd: negative stride");
  ANEMOI_REQUIRE(!precondition || sigma != nullptr, "edm_output_bwd: the preconditioning needs sigma");
  const int64_t total = (int64_t)B * E * N * P;
  ANEMOI_REQUIRE((int64_t)B * E < (1ll << 31) && grid_fits(total), "edm_output_bwd: %lld elements exceed the grid", (long long)total);
  if (total == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  const float sd = (float)sigma_data, sd2 = (float)(sigma_data * sigma_data);
  return dispatch_dtype(pred_dtype, [&](auto tp) {
    using TP = typename decltype(tp)::type;
    return dispatch_real(d_out_f64, [&](auto tg) {
      using TG = typename decltype(tg)::type;
      return dispatch_real(sigma_f64, [&](auto ts) {
        using TS = typename decltype(ts)::type;
        hipLaunchKernelGGL((edm_output_bwd_kernel<TP, TG, TS>), grid_for(total), dim3(kBwdThreads), 0, st, (const TG*)d_out, gs_b, gs_t, gs_e, gs_n, gs_v,
                           (const TS*)sigma, sd, sd2, precondition, (TP*)d_pred, ldp, P, E, N, T_out, V_out, total);
        return check_launch("edm_output_bwd_kernel");
      });
    });
  });
}
