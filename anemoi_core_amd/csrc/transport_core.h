// What the forward kernels of the EDM diffusion edges (transport.hip) and their backward kernels (transport_bwd.hip) both evaluate: the
// fp32 EDM coefficients of one group and the per-group conditioning vector.  Both translation units include this header, so a quantity
// the backward recomputes is the forward's, bit for bit.
#pragma once
#include "common.h"

namespace anemoi {

constexpr int kNoiseChannelsMax = 64;  // C: width of the noise embedding and of the first Linear
constexpr int kNoiseCondMax = 32;      // cond_dim: width of the conditioning rows
constexpr int kCondTileRows = 512;     // rows of one destination a workgroup of the noise-conditioning kernels covers

inline dim3 grid_for(int64_t n_threads) { return dim3((unsigned)((n_threads + 255) / 256)); }
inline bool grid_fits(int64_t n_threads) { return (n_threads + 255) / 256 <= 0x7fffffffll; }

// precision flag of the C ABI (0 = fp32, 1 = fp64) -> f(type_tag<float | double>)
template <typename F>
int dispatch_real(int32_t is_f64, F&& f) {
  return is_f64 ? f(type_tag<double>{}) : f(type_tag<float>{});
}

// The EDM coefficients of one group in fp32, every operation rounded on its own in the order the reference's tensor expressions are
// evaluated (transport/objectives.py:209-211): t = sd^2 + sigma^2, c_in = 1 / sqrt(t), c_skip = sd^2 / t, c_out = (sigma sd) / sqrt(t).
struct EdmCoefficients {
  float c_in, c_skip, c_out;
};
__device__ __forceinline__ EdmCoefficients edm_coefficients(float sigma, float sd, float sd2) {
  const float t = __fadd_rn(__fmul_rn(sigma, sigma), sd2);
  const float r = __fsqrt_rn(t);
  return {__fdiv_rn(1.0f, r), __fdiv_rn(sd2, t), __fdiv_rn(__fmul_rn(sigma, sd), r)};
}

// The conditioning vector of one group, computed by a whole workgroup (thread t = threadIdx.x; blockDim.x >= C, cond_dim): v, or log(v) / 4
// (transform 1); the C / 2 sin | cos pairs; p = W1 e + b1; h = SiLU(p); c = W2 h + b2.  Leaves e in emb[C], h in hid[C], c in cnd[cond_dim]
// and, when ``pre`` is given, p in pre[C] (LDS); ends with a barrier, so every thread may read all of them.
template <typename TW>
__device__ __forceinline__ void noise_cond_vector(float v, int transform, const float* __restrict__ freq, const float* __restrict__ pi,
                                                  const TW* __restrict__ w1, const TW* __restrict__ b1, const TW* __restrict__ w2,
                                                  const TW* __restrict__ b2, int C, int cond_dim, float* emb, float* pre, float* hid, float* cnd) {
  const int t = threadIdx.x, half = C / 2;
  if (transform == 1) v = __fdiv_rn(logf(v), 4.0f);
  if (t < half) {
    float a = __fmul_rn(v, freq[t]);
    if (pi != nullptr) a = __fmul_rn(__fmul_rn(a, 2.0f), pi[0]);
    emb[t] = sinf(a);  // (the precise functions: the argument reaches hundreds of radians)
    emb[half + t] = cosf(a);
  }
  __syncthreads();
  if (t < C) {
    float acc = 0.f;
    for (int k = 0; k < C; ++k) acc = fmaf(to_float(w1[t * C + k]), emb[k], acc);
    acc += to_float(b1[t]);
    if (pre != nullptr) pre[t] = acc;
    hid[t] = acc / (1.0f + expf(-acc));  // SiLU
  }
  __syncthreads();
  if (t < cond_dim) {
    float acc = 0.f;
    for (int k = 0; k < C; ++k) acc = fmaf(to_float(w2[t * C + k]), hid[k], acc);
    cnd[t] = acc + to_float(b2[t]);
  }
  __syncthreads();
}

}  // namespace anemoi
