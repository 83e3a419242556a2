// The almost-fair kernel CRPS of an ensemble and its gradient: the one loss an ensemble model trains with.  pred [B, T, E, N, V] and
// target [B, T, 1, N, V] are read in place through their element strides; a column (b, t, n, v) is E members and one target.  A thread
// holds the E members of its columns in registers and ranks them with E^2 compares:
//   s_m = sum_j sign(x_m - x_j)                                       (sign(0) = 0)
//   crps = (1/E) sum_m |x_m - y| + coef sum_m (x_m - y) s_m,           coef = -(alpha / (E (E - 1)) + (1 - alpha) / E^2)
//          (sum_m x_m s_m = sum_{i<j} |x_i - x_j|, ties included: the value of both reference backends)
//   d crps / d x_m = sign(x_m - y) / E + coef s_m = -coef (r sign(x_m - y) - s_m),   r = E (E - 1) / (E - 1 + alpha)
// (sum_m s_m = 0, so the target may be subtracted inside the rank sum: the products then cancel at the size of the ensemble's spread
// about the target instead of at the size of the values.  r is an integer at alpha = 0 and 1, so a gradient that is zero in exact
// arithmetic - the largest member above the target under the fair CRPS - is computed as exactly zero.)
// Nothing of size E^2, and no gradient tensor, ever exists in memory: the backward recomputes the ranks from pred and target.
// Deterministic: stage one sums a workgroup's weighted columns per variable in LDS in a fixed order and writes one fp32 row of partials,
// stage two (one workgroup, fp64 accumulators) sums the rows in a fixed order; plain stores, no atomics.  The upstream gradient is read
// from DEVICE memory, so a captured training step replays.
#include "rowwise_common.h"  // pick_vec, dispatch_one_of

namespace anemoi {
namespace {

constexpr int kCrpsThreads = 256;
constexpr int kCrpsTile = 1024;         // consecutive (n, v) elements of one (b, t) per tile: four columns per thread, whatever VEC
constexpr int kCrpsMaxE = 16;           // members held in registers
constexpr int kCrpsMaxV = 4096;         // variables whose partial sums fit the LDS of either stage
constexpr int kCrpsTargetGroups = 1024; // stage-one workgroups aimed at (four per CU): the rows stage two has to sum
constexpr int kCrpsReduceThreads = 1024;

// What both kernels are told about the tensors.  Strides in elements; the variable axis is contiguous.
struct CrpsTensors {
  const void* pred;
  const void* target;
  const float* w_grid;
  const float* w_var;   // or null: 1
  const float* w_time;  // or null: 1
  int64_t ps_b, ps_t, ps_e, ps_n, ts_b, ts_t, ts_n;
  int32_t T, N, V, target_f32, ignore_nans;
};

template <typename T, int VEC>
__device__ __forceinline__ void load_target(const CrpsTensors& a, int64_t off, float (&y)[VEC]) {
  if (a.target_f32) {
    load_vec<float, VEC>((const float*)a.target + off, y);
  } else {
    load_vec<T, VEC>((const T*)a.target + off, y);
  }
}

// The column of one thread: the members x[m][j] and the target y[j] of VEC neighbouring variables of grid point n, as fp32.
template <typename T, int E, int VEC>
__device__ __forceinline__ void load_columns(const CrpsTensors& a, int b, int t, int n, int v0, float (&x)[E][VEC], float (&y)[VEC]) {
  const T* p = (const T*)a.pred + b * a.ps_b + t * a.ps_t + n * a.ps_n + v0;
#pragma unroll
  for (int m = 0; m < E; ++m) load_vec<T, VEC>(p + m * a.ps_e, x[m]);
  load_target<T, VEC>(a, b * a.ts_b + t * a.ts_t + n * a.ts_n + v0, y);
}

// s_m = sum_j sign(x_m - x_j) of column j0: two compares per ordered pair, nothing stored.
template <int E, int VEC>
__device__ __forceinline__ int rank_sum(const float (&x)[E][VEC], int m, int j0) {
  int s = 0;
#pragma unroll
  for (int j = 0; j < E; ++j) s += (int)(x[m][j0] > x[j][j0]) - (int)(x[m][j0] < x[j][j0]);
  return s;
}

template <int E, int VEC>
__device__ __forceinline__ bool has_nan(const float (&x)[E][VEC], float y, int j0) {
  bool bad = y != y;
#pragma unroll
  for (int m = 0; m < E; ++m) bad |= x[m][j0] != x[m][j0];
  return bad;
}

__device__ __forceinline__ float column_weight(const CrpsTensors& a, float w_bt_n, int v) { return a.w_var ? w_bt_n * a.w_var[v] : w_bt_n; }

// ---------------------------------------------------------------------------------------------- forward, stage 1
// grid (groups, B T): workgroup (g, bt) owns the tiles g tiles_per_group .. of the N V elements of (b, t).  Per tile every thread writes
// its four weighted column values to LDS (zeros past N V and for ignored NaN columns); then slot (r, v) = thread r V + v adds the
// tile's values of variable v, every R-th of them from the r-th on, to its running sum (R = 256 / V sub-sums per variable, 1 for
// V >= 256, where a thread owns several variables).  The R sub-sums meet at the end in r order: ws[(bt groups + g) V + v].
template <typename T, int E, int VEC>
__global__ __launch_bounds__(kCrpsThreads) void crps_fwd_partial_kernel(CrpsTensors a, float inv_e, float coef, int tiles, int tiles_per_group,
                                                                        float* __restrict__ ws) {
  extern __shared__ float crps_lds[];
  float* vals = crps_lds;           // [kCrpsTile]
  float* part = crps_lds + kCrpsTile;  // [R V]
  const int tid = threadIdx.x, bt = blockIdx.y, b = bt / a.T, t = bt - b * a.T;
  const int V = a.V, NV = a.N * V;
  const int R = V < kCrpsThreads ? kCrpsThreads / V : 1, slots = R * V;
  for (int slot = tid; slot < slots; slot += kCrpsThreads) part[slot] = 0.f;
  const float wt = a.w_time ? a.w_time[t] : 1.f;
  const int first = blockIdx.x * tiles_per_group, last = min(first + tiles_per_group, tiles);
  for (int tile = first; tile < last; ++tile) {
    const int f_tile = tile * kCrpsTile;
#pragma unroll
    for (int it = 0; it < 4 / VEC; ++it) {
      const int i = (it * kCrpsThreads + tid) * VEC, f = f_tile + i;
      float out[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) out[j] = 0.f;
      if (f < NV) {  // VEC divides V: the VEC elements are in range, and of one grid point, together
        const int n = f / V, v0 = f - n * V;
        float x[E][VEC], y[VEC];
        load_columns<T, E, VEC>(a, b, t, n, v0, x, y);
        const float w_bt_n = wt * a.w_grid[n];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          if (a.ignore_nans && has_nan<E, VEC>(x, y[j], j)) continue;
          float mae = 0.f, spread = 0.f;
#pragma unroll
          for (int m = 0; m < E; ++m) {
            const float d = x[m][j] - y[j];
            mae += fabsf(d);
            spread = fmaf(d, (float)rank_sum<E, VEC>(x, m, j), spread);
          }
          out[j] = column_weight(a, w_bt_n, v0 + j) * fmaf(spread, coef, mae * inv_e);
        }
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) vals[i + j] = out[j];
    }
    __syncthreads();
    const int phase = f_tile % V;  // the variable of the tile's first element
    for (int slot = tid; slot < slots; slot += kCrpsThreads) {
      const int r = slot / V, v = slot - r * V;
      float acc = part[slot];
      for (int i = (v >= phase ? v - phase : v - phase + V) + r * V; i < kCrpsTile; i += slots) acc += vals[i];
      part[slot] = acc;
    }
    __syncthreads();
  }
  for (int v = tid; v < V; v += kCrpsThreads) {
    float acc = 0.f;
    for (int r = 0; r < R; ++r) acc += part[r * V + v];
    ws[((int64_t)bt * gridDim.x + blockIdx.x) * V + v] = acc;
  }
}

// ---------------------------------------------------------------------------------------------- forward, stage 2
// One workgroup.  Slot (r, v) sums every R-th partial row of variable v from the r-th on in fp64 (R = 1024 / V, 1 for V >= 1024); thread v
// adds the R sub-sums in r order and scales by 1 / B: loss[v] (squash 0).  Squash 1 / 2: thread 0 adds the V values in order; 1 divides
// by V.
__global__ __launch_bounds__(kCrpsReduceThreads) void crps_reduce_kernel(const float* __restrict__ ws, int rows, int V, double inv_b, int squash,
                                                                         float* __restrict__ loss) {
  __shared__ double sub[kCrpsMaxV];
  const int tid = threadIdx.x;
  const int R = V < kCrpsReduceThreads ? kCrpsReduceThreads / V : 1, slots = R * V;
  for (int slot = tid; slot < slots; slot += kCrpsReduceThreads) {
    const int r = slot / V, v = slot - r * V;
    double acc = 0.0;
    for (int row = r; row < rows; row += R) acc += (double)ws[(int64_t)row * V + v];
    sub[slot] = acc;
  }
  __syncthreads();
  for (int v = tid; v < V; v += kCrpsReduceThreads) {
    double acc = 0.0;
    for (int r = 0; r < R; ++r) acc += sub[r * V + v];
    acc *= inv_b;
    if (squash == 0) loss[v] = (float)acc;
    sub[v] = acc;  // (slot (0, v) is this thread's own)
  }
  if (squash == 0) return;
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    for (int v = 0; v < V; ++v) acc += sub[v];
    loss[0] = (float)(squash == 1 ? acc / V : acc);
  }
}

// ---------------------------------------------------------------------------------------------- backward
// grid (tiles, B T), the forward's columns per thread.  d_pred [B, T, E, N, V] contiguous, every element written:
//   d_pred[b, t, m, n, v] = upstream[v us] * w * (scale_k * (r sign(x_m - y) - s_m)),  scale_k = -coef / B (/ V under squash "avg").
template <typename T, int E, int VEC>
__global__ __launch_bounds__(kCrpsThreads) void crps_bwd_kernel(CrpsTensors a, float r_sign, float scale_k, const float* __restrict__ upstream,
                                                                int64_t us, T* __restrict__ d_pred) {
  const int tid = threadIdx.x, bt = blockIdx.y, b = bt / a.T, t = bt - b * a.T;
  const int V = a.V, NV = a.N * V;
  const float wt = a.w_time ? a.w_time[t] : 1.f;
  T* d = d_pred + (int64_t)bt * E * NV;
#pragma unroll
  for (int it = 0; it < 4 / VEC; ++it) {
    const int f = blockIdx.x * kCrpsTile + (it * kCrpsThreads + tid) * VEC;
    if (f >= NV) continue;
    const int n = f / V, v0 = f - n * V;
    float x[E][VEC], y[VEC], wu[VEC];
    load_columns<T, E, VEC>(a, b, t, n, v0, x, y);
    const float w_bt_n = wt * a.w_grid[n];
    bool skip[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      wu[j] = column_weight(a, w_bt_n, v0 + j);
      skip[j] = a.ignore_nans && has_nan<E, VEC>(x, y[j], j);
    }
#pragma unroll
    for (int m = 0; m < E; ++m) {
      float g[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float sgn = (float)((int)(x[m][j] > y[j]) - (int)(x[m][j] < y[j]));
        const float q = fmaf(sgn, r_sign, -(float)rank_sum<E, VEC>(x, m, j));
        g[j] = skip[j] ? 0.f : __fmul_rn(__fmul_rn(__fmul_rn(q, scale_k), wu[j]), upstream[(v0 + j) * us]);
      }
      store_vec<T, VEC>(d + (int64_t)m * NV + f, g);
    }
  }
}

// ---------------------------------------------------------------------------------------------- host
int crps_tiles(int64_t nv) { return (int)((nv + kCrpsTile - 1) / kCrpsTile); }

// Stage-one workgroups per (b, t) and the tiles each of them owns: about kCrpsTargetGroups workgroups in all, none of them empty.
void crps_split(int tiles, int64_t bt, int* groups, int* tiles_per_group) {
  const int64_t want = (kCrpsTargetGroups + bt - 1) / (bt > 0 ? bt : 1);
  const int per = (int)((tiles + want - 1) / want);
  *tiles_per_group = per > 0 ? per : 1;
  *groups = (tiles + *tiles_per_group - 1) / *tiles_per_group;
}

template <typename F>
int dispatch_ensemble(int E, F&& f) {
  int rc = ANEMOI_E_UNSUPPORTED;
  dispatch_one_of<2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(E, [&](auto e) { rc = f(e); });
  return rc;
}

// The checks both entries share, the tensor block of the kernels and the vector width: the widest of 4, 2, 1 that divides V and every
// stride and that both base addresses are aligned to (rowwise_common.h: pick_vec, per element type).
template <typename T>
int crps_vec(const CrpsTensors& a) {
  int vec = pick_vec<T>(a.V, {a.ps_b, a.ps_t, a.ps_e, a.ps_n}, {a.pred});
  const std::initializer_list<int64_t> ts = {a.ts_b, a.ts_t, a.ts_n};
  const int tvec = a.target_f32 ? pick_vec<float>(a.V, ts, {a.target}) : pick_vec<T>(a.V, ts, {a.target});
  vec = vec < tvec ? vec : tvec;
  return vec < 4 ? vec : 4;
}

int crps_check(const char* who, CrpsTensors* a, const void* pred, int64_t ps_b, int64_t ps_t, int64_t ps_e, int64_t ps_n, anemoi_dtype_t pred_dtype,
               const void* target, int64_t ts_b, int64_t ts_t, int64_t ts_n, anemoi_dtype_t target_dtype, const float* w_grid, const float* w_var,
               const float* w_time, double alpha, int32_t ignore_nans, int32_t B, int32_t T, int32_t E, int32_t N, int32_t V) {
  ANEMOI_REQUIRE(E != 1, "%s: Ensemble size must be greater than 1.", who);
  if (E > kCrpsMaxE) {
    set_error("%s: ensemble size %d beyond the built limit %d", who, E, kCrpsMaxE);
    return ANEMOI_E_UNSUPPORTED;
  }
  if (V > kCrpsMaxV) {
    set_error("%s: %d variables beyond the built limit %d", who, V, kCrpsMaxV);
    return ANEMOI_E_UNSUPPORTED;
  }
  if ((pred_dtype != ANEMOI_F32 && pred_dtype != ANEMOI_BF16) || (target_dtype != ANEMOI_F32 && target_dtype != pred_dtype)) {
    set_error("%s: pred fp32 or bf16 and target fp32 or pred's dtype, got dtypes %d, %d", who, (int)pred_dtype, (int)target_dtype);
    return ANEMOI_E_UNSUPPORTED;
  }
  ANEMOI_REQUIRE(pred && target && w_grid, "%s: null pointer", who);
  ANEMOI_REQUIRE(B >= 1 && T >= 1 && E >= 2 && N >= 1 && V >= 1, "%s: bad shape B=%d T=%d E=%d N=%d V=%d", who, B, T, E, N, V);
  ANEMOI_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "%s: alpha must be in the range [0, 1], got %g", who, alpha);
  ANEMOI_REQUIRE(ps_b >= 0 && ps_t >= 0 && ps_e >= 0 && ps_n >= 0 && ts_b >= 0 && ts_t >= 0 && ts_n >= 0, "%s: negative stride", who);
  ANEMOI_REQUIRE((int64_t)N * V < (1ll << 31) && (int64_t)B * T <= 65535, "%s: N V = %lld or B T = %lld exceed the grid", who, (long long)N * V,
                 (long long)B * T);
  *a = CrpsTensors{pred, target, w_grid, w_var, w_time, ps_b, ps_t, ps_e, ps_n, ts_b, ts_t, ts_n, T, N, V, target_dtype == ANEMOI_F32, ignore_nans != 0};
  return ANEMOI_OK;
}

double crps_coef(double alpha, int E) { return -(alpha / ((double)E * (E - 1)) + (1.0 - alpha) / ((double)E * E)); }

// f(type tag, E, VEC) for the pred dtype, ensemble size and vector width of a checked call.
template <typename F>
int crps_dispatch(const CrpsTensors& a, anemoi_dtype_t pred_dtype, int E, F&& f) {
  return dispatch_dtype(pred_dtype, [&](auto tp) {
    using T = typename decltype(tp)::type;
    if constexpr (std::is_same_v<T, f16_t>) {
      return (int)ANEMOI_E_UNSUPPORTED;  // (crps_check has refused it by name)
    } else {
      return dispatch_ensemble(E, [&](auto e) {
        int rc = ANEMOI_E_INVALID;
        dispatch_one_of<1, 2, 4>(crps_vec<T>(a), [&](auto vec) { rc = f(tp, e, vec); });
        return rc;
      });
    }
  });
}

}  // namespace
}  // namespace anemoi

using namespace anemoi;

extern "C" int64_t anemoi_crps_workspace_bytes(int32_t B, int32_t T, int32_t N, int32_t V) {
  if (B < 1 || T < 1 || N < 1 || V < 1) return 0;
  int groups, per;
  crps_split(crps_tiles((int64_t)N * V), (int64_t)B * T, &groups, &per);
  return (int64_t)B * T * groups * V * (int64_t)sizeof(float);
}

extern "C" int anemoi_crps_fwd(const void* pred, int64_t ps_b, int64_t ps_t, int64_t ps_e, int64_t ps_n, anemoi_dtype_t pred_dtype, const void* target,
                               int64_t ts_b, int64_t ts_t, int64_t ts_n, anemoi_dtype_t target_dtype, const float* w_grid, const float* w_var,
                               const float* w_time, double alpha, int32_t ignore_nans, int32_t squash, float* loss, void* workspace,
                               int64_t workspace_bytes, int32_t B, int32_t T, int32_t E, int32_t N, int32_t V, void* stream) {
  CrpsTensors a;
  const int ok = crps_check("crps_fwd", &a, pred, ps_b, ps_t, ps_e, ps_n, pred_dtype, target, ts_b, ts_t, ts_n, target_dtype, w_grid, w_var, w_time, alpha,
                            ignore_nans, B, T, E, N, V);
  if (ok != ANEMOI_OK) return ok;
  ANEMOI_REQUIRE(loss != nullptr && squash >= 0 && squash <= 2, "crps_fwd: loss pointer or squash %d (0 per variable, 1 avg, 2 sum)", squash);
  const int64_t need = anemoi_crps_workspace_bytes(B, T, N, V);
  ANEMOI_REQUIRE(workspace != nullptr && workspace_bytes >= need, "crps_fwd: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                 (long long)need);
  const int tiles = crps_tiles((int64_t)N * V);
  int groups, per;
  crps_split(tiles, (int64_t)B * T, &groups, &per);
  const float inv_e = (float)(1.0 / E), coef = (float)crps_coef(alpha, E);
  const int R = V < kCrpsThreads ? kCrpsThreads / V : 1;
  const size_t lds = (size_t)(kCrpsTile + R * V) * sizeof(float);
  hipStream_t st = as_stream(stream);
  float* ws = (float*)workspace;
  const int rc = crps_dispatch(a, pred_dtype, E, [&](auto tp, auto e, auto vec) {
    using T_ = typename decltype(tp)::type;
    hipLaunchKernelGGL((crps_fwd_partial_kernel<T_, decltype(e)::value, decltype(vec)::value>), dim3((unsigned)groups, (unsigned)(B * T)),
                       dim3(kCrpsThreads), lds, st, a, inv_e, coef, tiles, per, ws);
    return check_launch("crps_fwd_partial_kernel");
  });
  if (rc != ANEMOI_OK) return rc;
  hipLaunchKernelGGL(crps_reduce_kernel, dim3(1), dim3(kCrpsReduceThreads), 0, st, (const float*)ws, B * T * groups, V, 1.0 / B, squash, loss);
  return check_launch("crps_reduce_kernel");
}

extern "C" int anemoi_crps_bwd(const void* pred, int64_t ps_b, int64_t ps_t, int64_t ps_e, int64_t ps_n, anemoi_dtype_t pred_dtype, const void* target,
                               int64_t ts_b, int64_t ts_t, int64_t ts_n, anemoi_dtype_t target_dtype, const float* w_grid, const float* w_var,
                               const float* w_time, double alpha, int32_t ignore_nans, int32_t squash, const float* upstream, int64_t us, void* d_pred,
                               int32_t B, int32_t T, int32_t E, int32_t N, int32_t V, void* stream) {
  CrpsTensors a;
  const int ok = crps_check("crps_bwd", &a, pred, ps_b, ps_t, ps_e, ps_n, pred_dtype, target, ts_b, ts_t, ts_n, target_dtype, w_grid, w_var, w_time, alpha,
                            ignore_nans, B, T, E, N, V);
  if (ok != ANEMOI_OK) return ok;
  ANEMOI_REQUIRE(upstream != nullptr && d_pred != nullptr && squash >= 0 && squash <= 2, "crps_bwd: null pointer or squash %d", squash);
  ANEMOI_REQUIRE(squash == 0 ? (us == 0 || us == 1) : us == 0, "crps_bwd: upstream stride %lld (a scalar under squash, [V] with stride 0 or 1 without)",
                 (long long)us);
  const double k = -crps_coef(alpha, E);
  const float r_sign = (float)((double)E * (E - 1) / (E - 1 + alpha)), scale_k = (float)(k / B / (squash == 1 ? V : 1));
  hipStream_t st = as_stream(stream);
  return crps_dispatch(a, pred_dtype, E, [&](auto tp, auto e, auto vec) {
    using T_ = typename decltype(tp)::type;
    hipLaunchKernelGGL((crps_bwd_kernel<T_, decltype(e)::value, decltype(vec)::value>), dim3((unsigned)crps_tiles((int64_t)N * V), (unsigned)(B * T)),
                       dim3(kCrpsThreads), 0, st, a, r_sign, scale_k, upstream, us, (T_*)d_pred);
    return check_launch("crps_bwd_kernel");
  });
}
