// The thin layer around the denoiser network of the EDM diffusion model (models/transport_encoder_processor_decoder.py, transport/,
// samplers/transport_samplers.py): the noise conditioning, the two model edges with the EDM preconditioning, and the solver update.
// Four element-wise kernels; every per-call scalar (sigma, the solver's coefficients) is read from DEVICE memory, so that a captured launch
// replays for every step of a sampler.  Plain stores, one owner per output element, no atomics: results do not depend on the launch order.
#include "transport_core.h"  // the EDM coefficients and the conditioning vector, shared with the backward kernels (transport_bwd.hip)

#include <type_traits>

namespace anemoi {
namespace {

// ---------------------------------------------------------------------------------------------- 1. noise conditioning
// grid (G, tiles of destination 0 + tiles of destination 1); every workgroup recomputes the group's conditioning vector (C / 2 sin / cos
// pairs, C x C and cond_dim x C multiply-adds) and writes it into its tile of rows.
template <typename TV, typename TW, typename TO>
__global__ __launch_bounds__(256) void noise_cond_kernel(const TV* __restrict__ values, int transform, const float* __restrict__ freq,
                                                         const float* __restrict__ pi, const TW* __restrict__ w1, const TW* __restrict__ b1,
                                                         const TW* __restrict__ w2, const TW* __restrict__ b2, TO* __restrict__ out0,
                                                         int64_t rows0, int64_t ld0, int tiles0, TO* __restrict__ out1, int64_t rows1,
                                                         int64_t ld1, int C, int cond_dim) {
  __shared__ float emb[kNoiseChannelsMax], hid[kNoiseChannelsMax], cnd[kNoiseCondMax];
  const int g = blockIdx.x, t = threadIdx.x;
  noise_cond_vector<TW>((float)values[g], transform, freq, pi, w1, b1, w2, b2, C, cond_dim, emb, nullptr, hid, cnd);
  const bool first = (int)blockIdx.y < tiles0;
  TO* out = first ? out0 : out1;
  const int64_t rows = first ? rows0 : rows1, ld = first ? ld0 : ld1;
  const int64_t r0 = (int64_t)(first ? blockIdx.y : blockIdx.y - tiles0) * kCondTileRows;
  const int n_rows = (int)(rows - r0 < kCondTileRows ? rows - r0 : kCondTileRows);
  out += ((int64_t)g * rows + r0) * ld;
  for (int i = t; i < n_rows * cond_dim; i += 256) {
    const int row = i / cond_dim, col = i - row * cond_dim;
    out[(int64_t)row * ld + col] = from_float<TO>(cnd[col]);
  }
}

// ---------------------------------------------------------------------------------------------- 2. input assembly
// One value of the assembled row (g, n): [x steps | c_in y steps | node attributes | zeros].
template <typename TO, typename TY>
__device__ __forceinline__ float assembled_value(int col, const float* __restrict__ x_row, int64_t xs_t, int V_in, int in_cols,
                                                 const TY* __restrict__ y_row, int64_t ys_t, int V_out, int out_cols, float c_in,
                                                 const TO* __restrict__ attr_row, int A) {
  if (col < in_cols) {
    const int t = col / V_in;
    return x_row[t * xs_t + (col - t * V_in)];
  }
  col -= in_cols;
  if (col < out_cols) {
    const int t = col / V_out;
    return __fmul_rn(c_in, (float)y_row[t * ys_t + (col - t * V_out)]);  // (y is cast to the data dtype before the multiply)
  }
  col -= out_cols;
  return col < A ? to_float(attr_row[col]) : 0.f;
}

template <typename TO, typename TY, typename TS, int VEC>
__global__ __launch_bounds__(256) void transport_assemble_kernel(const float* __restrict__ x, int64_t xs_b, int64_t xs_t, int64_t xs_e, int64_t xs_n,
                                                                 const TY* __restrict__ y, int64_t ys_b, int64_t ys_t, int64_t ys_e, int64_t ys_n,
                                                                 const TS* __restrict__ sigma, float sd, float sd2, int scale,
                                                                 const TO* __restrict__ attrs, int64_t lda, int A, TO* __restrict__ out, int64_t ldo,
                                                                 int W, int E, int N, int T_in, int V_in, int T_out, int V_out, int64_t n_rows) {
  const int chunks = W / VEC;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_rows * chunks) return;
  const int64_t row = idx / chunks;
  const int c0 = (int)(idx - row * chunks) * VEC;
  const int g = (int)(row / N), n = (int)(row - (int64_t)g * N), b = g / E, e = g - b * E;
  const float c_in = scale ? edm_coefficients((float)sigma[g], sd, sd2).c_in : 1.0f;
  const float* x_row = x + b * xs_b + e * xs_e + n * xs_n;
  const TY* y_row = y + b * ys_b + e * ys_e + n * ys_n;
  const TO* attr_row = attrs + n * lda;
  float vals[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j)
    vals[j] = assembled_value<TO, TY>(c0 + j, x_row, xs_t, V_in, T_in * V_in, y_row, ys_t, V_out, T_out * V_out, c_in, attr_row, A);
  store_vec<TO, VEC>(out + row * ldo + c0, vals);
}

// ---------------------------------------------------------------------------------------------- 3. output assembly
template <typename TP, typename TY, typename TS, typename TD>
__global__ __launch_bounds__(256) void edm_output_kernel(const TP* __restrict__ pred, int64_t ldp, const TY* __restrict__ y, int64_t ys_b, int64_t ys_t,
                                                         int64_t ys_e, int64_t ys_n, const TS* __restrict__ sigma, float sd, float sd2, int precondition,
                                                         TD* __restrict__ out, int E, int N, int T_out, int V_out, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // over [B, T_out, E, N, V_out], the output's own layout
  if (idx >= total) return;
  int64_t q = idx / V_out;
  const int v = (int)(idx - q * V_out);
  const int n = (int)(q % N);
  q /= N;
  const int e = (int)(q % E);
  q /= E;
  const int t = (int)(q % T_out), b = (int)(q / T_out);
  const int g = b * E + e;
  float r = to_float(pred[((int64_t)g * N + n) * ldp + t * V_out + v]);
  if (precondition) {
    const EdmCoefficients c = edm_coefficients((float)sigma[g], sd, sd2);
    const float yd = (float)y[b * ys_b + t * ys_t + e * ys_e + n * ys_n + v];
    r = __fadd_rn(__fmul_rn(c.c_skip, yd), __fmul_rn(c.c_out, r));
  }
  out[idx] = (TD)r;
}

// ---------------------------------------------------------------------------------------------- 4. solver update
enum : int { HEUN_PREDICT = 0, HEUN_CORRECT = 1, HEUN_FINAL = 2, DPMPP_FIRST = 3, DPMPP_MULTI = 4, DPMPP_FINAL = 5 };

// params (fp64, device): [0] sigma_eff  [1] sigma_next  [2] eps  [3] sigma_next / sigma  [4] exp(-h) - 1  [5] c1  [6] c2
// [7] DPM++ only: != 0 rounds the updated state to fp32, the data dtype the reference keeps it in between steps.
// R: the solver's precision; the parameters are rounded to it first, as the reference's schedule is cast to the solver dtype.
template <typename R, int MODE>
__global__ __launch_bounds__(256) void edm_update_kernel(const double* __restrict__ params, R* __restrict__ y, const R* __restrict__ D,
                                                         R* __restrict__ aux1, R* __restrict__ aux2, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if constexpr (MODE == HEUN_PREDICT || MODE == HEUN_FINAL) {
    const R s_eff = (R)params[0], s_next = (R)params[1], eps = (R)params[2];
    const R d1 = (y[i] - D[i]) / (s_eff + eps);
    const R y_next = y[i] + (s_next - s_eff) * d1;
    if constexpr (MODE == HEUN_PREDICT) {
      aux1[i] = d1;
      aux2[i] = y_next;
    } else {
      y[i] = y_next;
    }
  } else if constexpr (MODE == HEUN_CORRECT) {
    const R s_eff = (R)params[0], s_next = (R)params[1], eps = (R)params[2];
    const R d2 = (aux2[i] - D[i]) / (s_next + eps);
    y[i] = y[i] + (s_next - s_eff) * (aux1[i] + d2) / (R)2;
  } else if constexpr (MODE == DPMPP_FIRST || MODE == DPMPP_MULTI) {
    const R ratio = (R)params[3], em1 = (R)params[4];
    const R d = D[i];
    R dm = d;
    if constexpr (MODE == DPMPP_MULTI) dm = (R)params[5] * d + (R)params[6] * aux1[i];
    R v = ratio * y[i] - em1 * dm;
    if (params[7] != 0.0) v = (R)(float)v;  // transport_samplers.py:283: y leaves every update in the data dtype
    y[i] = v;
    aux1[i] = d;
  } else {
    y[i] = D[i];
  }
}

}  // namespace
}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_noise_cond_fwd(const void* values, int32_t values_f64, int32_t transform, const float* frequencies, const float* pi,
                                     const void* w1, const void* b1, const void* w2, const void* b2, anemoi_dtype_t w_dtype, void* out0,
                                     int64_t rows0, int64_t ld0, void* out1, int64_t rows1, int64_t ld1, int32_t G, int32_t C, int32_t cond_dim,
                                     anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(values && frequencies && w1 && b1 && w2 && b2, "noise_cond_fwd: null pointer");
  ANEMOI_REQUIRE(G >= 0 && C >= 2 && C % 2 == 0 && cond_dim >= 1, "noise_cond_fwd: bad shape G=%d C=%d cond_dim=%d", G, C, cond_dim);
  ANEMOI_REQUIRE(transform == 0 || transform == 1, "noise_cond_fwd: transform %d (0 = identity, 1 = log / 4)", transform);
  if (C > kNoiseChannelsMax || cond_dim > kNoiseCondMax) {
    set_error("noise_cond_fwd: C=%d, cond_dim=%d beyond the built limits %d, %d", C, cond_dim, kNoiseChannelsMax, kNoiseCondMax);
    return ANEMOI_E_UNSUPPORTED;
  }
  if (out0 == nullptr) rows0 = 0;
  if (out1 == nullptr) rows1 = 0;
  ANEMOI_REQUIRE(rows0 >= 0 && rows1 >= 0 && (rows0 == 0 || ld0 >= cond_dim) && (rows1 == 0 || ld1 >= cond_dim),
                 "noise_cond_fwd: bad destination rows=%lld,%lld ld=%lld,%lld", (long long)rows0, (long long)rows1, (long long)ld0, (long long)ld1);
  const int64_t tiles0 = (rows0 + kCondTileRows - 1) / kCondTileRows, tiles1 = (rows1 + kCondTileRows - 1) / kCondTileRows;
  ANEMOI_REQUIRE(tiles0 + tiles1 <= 65535, "noise_cond_fwd: %lld row tiles exceed the grid", (long long)(tiles0 + tiles1));
  if (G == 0 || tiles0 + tiles1 == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)G, (unsigned)(tiles0 + tiles1));
  return dispatch_real(values_f64, [&](auto tv) {
    using TV = typename decltype(tv)::type;
    return dispatch_dtype(w_dtype, [&](auto tw) {
      using TW = typename decltype(tw)::type;
      return dispatch_dtype(dtype, [&](auto to) {
        using TO = typename decltype(to)::type;
        hipLaunchKernelGGL((noise_cond_kernel<TV, TW, TO>), grid, dim3(256), 0, st, (const TV*)values, transform, frequencies, pi, (const TW*)w1,
                           (const TW*)b1, (const TW*)w2, (const TW*)b2, (TO*)out0, rows0, ld0, (int)tiles0, (TO*)out1, rows1, ld1, C, cond_dim);
        return check_launch("noise_cond_kernel");
      });
    });
  });
}

extern "C" int anemoi_transport_assemble_input(const float* x, int64_t xs_b, int64_t xs_t, int64_t xs_e, int64_t xs_n, const void* y, int32_t y_f64,
                                               int64_t ys_b, int64_t ys_t, int64_t ys_e, int64_t ys_n, const void* sigma, int32_t sigma_f64,
                                               double sigma_data, int32_t scale, const void* attrs, int64_t lda, int32_t A, void* out, int64_t ldo,
                                               int32_t W, int32_t B, int32_t E, int32_t N, int32_t T_in, int32_t V_in, int32_t T_out, int32_t V_out,
                                               anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(x && y && out, "transport_assemble_input: null pointer");
  ANEMOI_REQUIRE(B >= 0 && E >= 1 && N >= 0 && T_in >= 1 && V_in >= 1 && T_out >= 1 && V_out >= 1 && A >= 0,
                 "transport_assemble_input: bad shape B=%d E=%d N=%d T_in=%d V_in=%d T_out=%d V_out=%d A=%d", B, E, N, T_in, V_in, T_out, V_out, A);
  const int64_t cols = (int64_t)T_in * V_in + (int64_t)T_out * V_out + A;
  ANEMOI_REQUIRE(W >= cols && ldo >= W && cols < (1ll << 30), "transport_assemble_input: W=%d ldo=%lld against %lld columns", W, (long long)ldo,
                 (long long)cols);
  ANEMOI_REQUIRE(A == 0 || (attrs != nullptr && lda >= A), "transport_assemble_input: attrs missing or lda=%lld < A=%d", (long long)lda, A);
  ANEMOI_REQUIRE(!scale || sigma != nullptr, "transport_assemble_input: the c_in scale needs sigma");
  const int64_t n_rows = (int64_t)B * E * N;
  ANEMOI_REQUIRE((int64_t)B * E < (1ll << 31) && grid_fits(n_rows * W), "transport_assemble_input: %lld rows x %d exceed the grid", (long long)n_rows, W);
  if (n_rows == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  const float sd = (float)sigma_data, sd2 = (float)(sigma_data * sigma_data);
  return dispatch_dtype(dtype, [&](auto to) {
    using TO = typename decltype(to)::type;
    return dispatch_real(y_f64, [&](auto ty) {
      using TY = typename decltype(ty)::type;
      return dispatch_real(sigma_f64, [&](auto ts) {
        using TS = typename decltype(ts)::type;
        // a 16-bit output whose rows are whole 16-byte groups takes the 8-column path (model_edge.hip's rule)
        const bool vec8 = sizeof(TO) == 2 && W % 8 == 0 && ldo % 8 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
        if (vec8) {
          hipLaunchKernelGGL((transport_assemble_kernel<TO, TY, TS, 8>), grid_for(n_rows * (W / 8)), dim3(256), 0, st, x, xs_b, xs_t, xs_e, xs_n,
                             (const TY*)y, ys_b, ys_t, ys_e, ys_n, (const TS*)sigma, sd, sd2, scale, (const TO*)attrs, lda, A, (TO*)out, ldo, W, E, N,
                             T_in, V_in, T_out, V_out, n_rows);
        } else {
          hipLaunchKernelGGL((transport_assemble_kernel<TO, TY, TS, 1>), grid_for(n_rows * W), dim3(256), 0, st, x, xs_b, xs_t, xs_e, xs_n,
                             (const TY*)y, ys_b, ys_t, ys_e, ys_n, (const TS*)sigma, sd, sd2, scale, (const TO*)attrs, lda, A, (TO*)out, ldo, W, E, N,
                             T_in, V_in, T_out, V_out, n_rows);
        }
        return check_launch("transport_assemble_kernel");
      });
    });
  });
}

extern "C" int anemoi_edm_output(const void* pred, int64_t ldp, anemoi_dtype_t pred_dtype, const void* y, int32_t y_f64, int64_t ys_b, int64_t ys_t,
                                 int64_t ys_e, int64_t ys_n, const void* sigma, int32_t sigma_f64, double sigma_data, int32_t precondition, void* out,
                                 int32_t out_f64, int32_t B, int32_t E, int32_t N, int32_t T_out, int32_t V_out, void* stream) {
  ANEMOI_REQUIRE(pred && out, "edm_output: null pointer");
  ANEMOI_REQUIRE(B >= 0 && E >= 1 && N >= 0 && T_out >= 1 && V_out >= 1 && ldp >= (int64_t)T_out * V_out,
                 "edm_output: bad shape B=%d E=%d N=%d T_out=%d V_out=%d ldp=%lld", B, E, N, T_out, V_out, (long long)ldp);
  ANEMOI_REQUIRE(!precondition || (y != nullptr && sigma != nullptr), "edm_output: the preconditioning needs y and sigma");
  const int64_t total = (int64_t)B * T_out * E * N * V_out;
  ANEMOI_REQUIRE((int64_t)B * E < (1ll << 31) && grid_fits(total), "edm_output: %lld elements exceed the grid", (long long)total);
  if (total == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  const float sd = (float)sigma_data, sd2 = (float)(sigma_data * sigma_data);
  return dispatch_dtype(pred_dtype, [&](auto tp) {
    using TP = typename decltype(tp)::type;
    return dispatch_real(y_f64, [&](auto ty) {
      using TY = typename decltype(ty)::type;
      return dispatch_real(sigma_f64, [&](auto ts) {
        using TS = typename decltype(ts)::type;
        return dispatch_real(out_f64, [&](auto td) {
          using TD = typename decltype(td)::type;
          hipLaunchKernelGGL((edm_output_kernel<TP, TY, TS, TD>), grid_for(total), dim3(256), 0, st, (const TP*)pred, ldp, (const TY*)y, ys_b, ys_t,
                             ys_e, ys_n, (const TS*)sigma, sd, sd2, precondition, (TD*)out, E, N, T_out, V_out, total);
          return check_launch("edm_output_kernel");
        });
      });
    });
  });
}

template <typename R, int MODE>
static int edm_update_launch(const double* params, void* y, const void* D, void* aux1, void* aux2, int64_t n, hipStream_t st) {
  hipLaunchKernelGGL((edm_update_kernel<R, MODE>), grid_for(n), dim3(256), 0, st, params, (R*)y, (const R*)D, (R*)aux1, (R*)aux2, n);
  return check_launch("edm_update_kernel");
}

extern "C" int anemoi_edm_update(int32_t mode, const double* params, void* y, const void* D, void* aux1, void* aux2, int64_t n, int32_t solver_f64,
                                 void* stream) {
  ANEMOI_REQUIRE(mode >= HEUN_PREDICT && mode <= DPMPP_FINAL, "edm_update: unknown mode %d", mode);
  ANEMOI_REQUIRE(params && y && D && n >= 0 && grid_fits(n), "edm_update: null pointer or bad size %lld", (long long)n);
  ANEMOI_REQUIRE(aux1 != nullptr || mode == HEUN_FINAL || mode == DPMPP_FINAL, "edm_update: mode %d needs aux1 (d1 | D_old)", mode);
  ANEMOI_REQUIRE(aux2 != nullptr || (mode != HEUN_PREDICT && mode != HEUN_CORRECT), "edm_update: mode %d needs aux2 (y_next)", mode);
  if (n == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  return dispatch_real(solver_f64, [&](auto tr) {
    using R = typename decltype(tr)::type;
    switch (mode) {
      case HEUN_PREDICT: return edm_update_launch<R, HEUN_PREDICT>(params, y, D, aux1, aux2, n, st);
      case HEUN_CORRECT: return edm_update_launch<R, HEUN_CORRECT>(params, y, D, aux1, aux2, n, st);
      case HEUN_FINAL: return edm_update_launch<R, HEUN_FINAL>(params, y, D, aux1, aux2, n, st);
      case DPMPP_FIRST: return edm_update_launch<R, DPMPP_FIRST>(params, y, D, aux1, aux2, n, st);
      case DPMPP_MULTI: return edm_update_launch<R, DPMPP_MULTI>(params, y, D, aux1, aux2, n, st);
      default: return edm_update_launch<R, DPMPP_FINAL>(params, y, D, aux1, aux2, n, st);
    }
  });
}
