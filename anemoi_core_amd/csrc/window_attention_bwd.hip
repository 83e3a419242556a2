// Sliding-window (banded) multi-head self-attention, backward, for gfx950.
//
// Spec: the derivative of csrc/window_attention.hip.  For query i and key j of one sequence with |i - j| <= w:
//   t = <q_i, k_j> * scale;  s = softcap * tanh(t / softcap) if softcap > 0 else t;  s -= slope_h |i - j|;  p = exp(s - lse_i)
//   Delta_i = <dO_i, O_i>;  dP_ij = <dO_i, v_j>;  dS_ij = p_ij (dP_ij - Delta_i);  dT_ij = dS_ij (1 - tanh^2(t / softcap)) or dS_ij
//   dq_i = scale sum_j dT_ij k_j;  dk_j = scale sum_i dT_ij q_i;  dv_j = sum_i p_ij dO_i.
// The slopes get no gradient.
//
// Two passes, both recomputing S / P from q, k and the forward's log-sum-exp; every output element is written by exactly one lane in a
// fixed summation order: no atomics, bitwise reproducible.
//   query pass: the forward's decomposition - a workgroup of four waves owns 64 queries of one (sequence, head) and visits the 64-key
//               tiles that meet its band; writes dq and Delta (fp32 [rows, H] workspace).
//   key pass:   a workgroup owns 64 keys, each wave 16 of them, and visits the query tiles that meet [k0 - w, k0 + 63 + w] ∩ [0, N);
//               reads Delta, writes dk and dv.
// The work of both is proportional to N (2w + 1).
//
// 16-bit path (mfma_f32_16x16x32, fp32 accumulators).  As in the forward the scores are computed transposed, so that a lane holds 16
// scores of ONE owned row (query pass: S^T = K Q^T, lane = query; key pass: S = Q K^T, lane = key) and P / dT feed the second GEMM as
// its B operand in the registers they were computed in (k slot 8g + j of step s = tile row 32 s + 16 (j / 4) + 4 g + j % 4).  The
// streamed tile sits in LDS row-major (A operand of the score GEMMs) and transposed (A operand of the gradient GEMMs).  exp2 with
// log2(e) folded in; band and sequence masks are evaluated only on tiles that cross an edge, and a masked score gives an exact 0.
// The key pass streams 64-query tiles for d <= 64 and 32-query tiles for d = 128, which keeps its four LDS images under 48 KB.
//
// fp32 path: one wave per (query, head) and one per (key, head), plain and exact (expf, sequential dots) - a correctness path.
#include "window_attention_core.h"

namespace anemoi {

namespace {

constexpr int kWaves = 4;
constexpr int kOwn = 16 * kWaves;  // rows (queries / keys) a workgroup owns

struct WinBwdArgs {
  const void* q;
  int64_t ldq;
  const void* k;
  int64_t ldk;
  const void* v;
  int64_t ldv;
  const void* out;
  int64_t ldo;
  const void* d_out;
  int64_t ldg;
  const float* lse;
  void* dq;
  int64_t lddq;
  void* dk;
  int64_t lddk;
  void* dv;
  int64_t lddv;
  float* delta;
  const float* slopes;
  int batch, N, H, d, window;
  float scale, softcap;
  hipStream_t stream;
};

// p = exp(s - lse) of query i, key j from the raw dot product (lse2 = lse * log2(e)), and dt_ds = dT / dS (FANCY: softcap and / or ALiBi)
template <bool FANCY>
__device__ __forceinline__ float win_prob(float dot, int i, int j, float lse2, float sl2e, float scale, float softcap, float slope,
                                          float& dt_ds) {
  if constexpr (!FANCY) {
    dt_ds = 1.f;
    return __builtin_amdgcn_exp2f(dot * sl2e - lse2);
  } else {
    float s = dot * scale;
    dt_ds = 1.f;
    if (softcap > 0.f) {
      const float th = tanhf(s / softcap);
      s = softcap * th;
      dt_ds = 1.f - th * th;
    }
    s -= slope * (float)abs(i - j);
    return __builtin_amdgcn_exp2f(s * kLog2e - lse2);
  }
}

// ---------------------------------------------------------------------------------------------- 16-bit, MFMA: query pass (dq, Delta)
template <typename T, int D, bool FANCY>
__global__ __launch_bounds__(64 * kWaves) void win_attn_bwd_query_kernel(WinBwdArgs a) {
  constexpr int KT = 64;         // keys per tile
  constexpr int RS = D + 8;      // row stride of the row-major K / V images (16 B of padding against bank conflicts)
  constexpr int TS = KT + 8;     // row stride of the transposed K image
  constexpr int CH = D / 8;      // 16-byte chunks per row
  constexpr int LOADS = KT * CH / (64 * kWaves);
  static_assert(LOADS >= 1 && KT * CH % (64 * kWaves) == 0, "tile loads");
  __shared__ __attribute__((aligned(16))) uint16_t k_lds[KT * RS];
  __shared__ __attribute__((aligned(16))) uint16_t v_lds[KT * RS];
  __shared__ __attribute__((aligned(16))) uint16_t kt_lds[D * TS];

  const int N = a.N, H = a.H, w = a.window;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int q0 = blockIdx.x * kOwn;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int qw = q0 + wave * 16;  // this wave's first query
  const int64_t row0 = (int64_t)b * N;
  const T* __restrict__ kp = (const T*)a.k;
  const T* __restrict__ vp = (const T*)a.v;

  const int lo = w < 0 ? 0 : max(0, q0 - w);
  const int hi = w < 0 ? N : min(N, q0 + kOwn + w);
  const int ntiles = (hi - lo + KT - 1) / KT;

  // q and dO of this lane's query as B operands: X[qw + c][8g + j + 32 s]; Delta from dO and O in the same layout
  const int qi = qw + c;
  // Delta comes out of the same MFMA as dP does (the diagonal of O dO^T): where a query attends a single key, out = v and dP - Delta
  // is an exact 0, as it is in exact arithmetic.
  frag8 qf[D / 32], gf[D / 32];
  float lse2 = 0.f;
  f32x4 od = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
    qf[s] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
    gf[s] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
    frag8 of = frag8{0, 0, 0, 0, 0, 0, 0, 0};
    if (qi < N) {
      const int64_t col = (int64_t)h * D + 8 * g + 32 * s;
      qf[s] = *reinterpret_cast<const frag8*>((const T*)a.q + (row0 + qi) * a.ldq + col);
      gf[s] = *reinterpret_cast<const frag8*>((const T*)a.d_out + (row0 + qi) * a.ldg + col);
      of = *reinterpret_cast<const frag8*>((const T*)a.out + (row0 + qi) * a.ldo + col);
    }
    od = mfma16<T>(of, gf[s], od);  // [query 4 g + r][query c]
  }
  const float diag = (c & 3) == 0 ? od[0] : (c & 3) == 1 ? od[1] : (c & 3) == 2 ? od[2] : od[3];
  const float delta = __shfl(diag, 16 * (c >> 2) + c, 64);  // the lane of this query with g = c / 4 holds its diagonal element
  if (qi < N) {
    lse2 = a.lse[(row0 + qi) * H + h] * kLog2e;
    if (g == 0) a.delta[(row0 + qi) * H + h] = delta;
  }
  const float sl2e = a.scale * kLog2e;
  const float slope = (FANCY && a.slopes) ? a.slopes[h] : 0.f;

  f32x4 acc[D / 16];
#pragma unroll
  for (int db = 0; db < D / 16; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the tile loader: chunk e of this thread = (key e / CH, 8 columns at 8 (e % CH)); keys beyond the range are zeros
  frag8 kreg[LOADS], vreg[LOADS];
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      const int e = tid + u * 64 * kWaves, key = e / CH, col = 8 * (e % CH);
      const int j = kt + key;
      if (j < hi) {
        kreg[u] = *reinterpret_cast<const frag8*>(kp + (row0 + j) * a.ldk + (int64_t)h * D + col);
        vreg[u] = *reinterpret_cast<const frag8*>(vp + (row0 + j) * a.ldv + (int64_t)h * D + col);
      } else {
        kreg[u] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
        vreg[u] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
  };
  if (ntiles > 0) load_tile(lo);

  for (int t = 0; t < ntiles; ++t) {
    const int kt = lo + t * KT;
    __syncthreads();  // every wave is done with the previous tile
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      const int e = tid + u * 64 * kWaves, key = e / CH, col = 8 * (e % CH);
      *reinterpret_cast<frag8*>(k_lds + key * RS + col) = kreg[u];
      *reinterpret_cast<frag8*>(v_lds + key * RS + col) = vreg[u];
#pragma unroll
      for (int x = 0; x < 8; ++x) kt_lds[(col + x) * TS + key] = (uint16_t)kreg[u][x];
    }
    __syncthreads();
    if (t + 1 < ntiles) load_tile(kt + KT);  // in flight while this tile is worked on

    const int klast = kt + KT - 1;
    if (w >= 0 && (kt > qw + 15 + w || klast < qw - w)) continue;
    const bool full = klast < N && qw + 15 < N && (w < 0 || (klast - qw <= w && qw + 15 - kt <= w));

    // S^T and dP^T [key 16 sb + 4 g + r][query c]
    frag8 tf[2];
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) {
      f32x4 st = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < D / 32; ++s) {
        const frag8 kf = *reinterpret_cast<const frag8*>(k_lds + (16 * sb + c) * RS + 8 * g + 32 * s);
        const frag8 vf = *reinterpret_cast<const frag8*>(v_lds + (16 * sb + c) * RS + 8 * g + 32 * s);
        st = mfma16<T>(kf, qf[s], st);
        dp = mfma16<T>(vf, gf[s], dp);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = kt + 16 * sb + 4 * g + r;
        float dt_ds;
        float p = win_prob<FANCY>(st[r], qi, j, lse2, sl2e, a.scale, a.softcap, slope, dt_ds);
        if (!full && !(j < N && qi < N && (w < 0 || abs(qi - j) <= w))) p = 0.f;
        tf[sb >> 1][4 * (sb & 1) + r] = to_bits<T>(p * (dp[r] - delta) * dt_ds);
      }
    }
    // dq^T[d 16 db + 4 g + r][query c] += K^T[d][keys] dT^T[keys][query]
#pragma unroll
    for (int db = 0; db < D / 16; ++db) {
#pragma unroll
      for (int s = 0; s < 2; ++s) acc[db] = mfma16<T>(transposed_frag(kt_lds, TS, 16 * db + c, s, g), tf[s], acc[db]);
    }
  }

  if (qi >= N) return;
  T* __restrict__ dqp = (T*)a.dq + (row0 + qi) * a.lddq + (int64_t)h * D;
#pragma unroll
  for (int db = 0; db < D / 16; ++db) {
    Vec<T, 4> o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o.v[r] = from_float<T>(acc[db][r] * a.scale);
    *reinterpret_cast<Vec<T, 4>*>(dqp + 16 * db + 4 * g) = o;
  }
}

// ---------------------------------------------------------------------------------------------- 16-bit, MFMA: key pass (dk, dv)
template <typename T, int D, bool FANCY>
__global__ __launch_bounds__(64 * kWaves) void win_attn_bwd_key_kernel(WinBwdArgs a) {
  constexpr int QT = D == 128 ? 32 : 64;  // queries per tile
  constexpr int RS = D + 8;               // row stride of the row-major Q / dO images
  constexpr int TS = QT + 8;              // row stride of the transposed Q / dO images
  constexpr int CH = D / 8;
  constexpr int LOADS = QT * CH / (64 * kWaves);
  static_assert(LOADS >= 1 && QT * CH % (64 * kWaves) == 0, "tile loads");
  __shared__ __attribute__((aligned(16))) uint16_t q_lds[QT * RS];
  __shared__ __attribute__((aligned(16))) uint16_t g_lds[QT * RS];
  __shared__ __attribute__((aligned(16))) uint16_t qt_lds[D * TS];
  __shared__ __attribute__((aligned(16))) uint16_t gt_lds[D * TS];
  __shared__ __attribute__((aligned(16))) float lse_lds[QT];
  __shared__ __attribute__((aligned(16))) float delta_lds[QT];

  const int N = a.N, H = a.H, w = a.window;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int k0 = blockIdx.x * kOwn;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int kw = k0 + wave * 16;  // this wave's first key
  const int64_t row0 = (int64_t)b * N;
  const T* __restrict__ qp = (const T*)a.q;
  const T* __restrict__ gp = (const T*)a.d_out;

  // query range of the workgroup: the band of its keys
  const int lo = w < 0 ? 0 : max(0, k0 - w);
  const int hi = w < 0 ? N : min(N, k0 + kOwn + w);
  const int ntiles = (hi - lo + QT - 1) / QT;

  // k and v of this lane's key as B operands: X[kw + c][8g + j + 32 s]
  const int kj = kw + c;
  frag8 kf[D / 32], vf[D / 32];
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
    kf[s] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
    vf[s] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
    if (kj < N) {
      const int64_t col = (int64_t)h * D + 8 * g + 32 * s;
      kf[s] = *reinterpret_cast<const frag8*>((const T*)a.k + (row0 + kj) * a.ldk + col);
      vf[s] = *reinterpret_cast<const frag8*>((const T*)a.v + (row0 + kj) * a.ldv + col);
    }
  }
  const float sl2e = a.scale * kLog2e;
  const float slope = (FANCY && a.slopes) ? a.slopes[h] : 0.f;

  f32x4 acck[D / 16], accv[D / 16];
#pragma unroll
  for (int db = 0; db < D / 16; ++db) {
    acck[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    accv[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // the tile loader: chunk e = (query e / CH, 8 columns at 8 (e % CH)); the first QT threads also carry lse and Delta of one query
  frag8 qreg[LOADS], greg[LOADS];
  float lreg = 0.f, dreg = 0.f;
  auto load_tile = [&](int qt) {
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      const int e = tid + u * 64 * kWaves, row = e / CH, col = 8 * (e % CH);
      const int i = qt + row;
      if (i < hi) {
        qreg[u] = *reinterpret_cast<const frag8*>(qp + (row0 + i) * a.ldq + (int64_t)h * D + col);
        greg[u] = *reinterpret_cast<const frag8*>(gp + (row0 + i) * a.ldg + (int64_t)h * D + col);
      } else {
        qreg[u] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
        greg[u] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    }
    if (tid < QT) {
      const int i = qt + tid;
      lreg = i < hi ? a.lse[(row0 + i) * H + h] * kLog2e : 0.f;
      dreg = i < hi ? a.delta[(row0 + i) * H + h] : 0.f;
    }
  };
  if (ntiles > 0) load_tile(lo);

  for (int t = 0; t < ntiles; ++t) {
    const int qt = lo + t * QT;
    __syncthreads();  // every wave is done with the previous tile
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      const int e = tid + u * 64 * kWaves, row = e / CH, col = 8 * (e % CH);
      *reinterpret_cast<frag8*>(q_lds + row * RS + col) = qreg[u];
      *reinterpret_cast<frag8*>(g_lds + row * RS + col) = greg[u];
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        qt_lds[(col + x) * TS + row] = (uint16_t)qreg[u][x];
        gt_lds[(col + x) * TS + row] = (uint16_t)greg[u][x];
      }
    }
    if (tid < QT) {
      lse_lds[tid] = lreg;
      delta_lds[tid] = dreg;
    }
    __syncthreads();
    if (t + 1 < ntiles) load_tile(qt + QT);  // in flight while this tile is worked on

    const int qlast = qt + QT - 1;
    if (w >= 0 && (qt > kw + 15 + w || qlast < kw - w)) continue;
    const bool full = qlast < N && kw + 15 < N && (w < 0 || (qlast - kw <= w && kw + 15 - qt <= w));

    // S and dP [query 16 sb + 4 g + r][key c]
    frag8 pf[QT / 32], tf[QT / 32];
#pragma unroll
    for (int sb = 0; sb < QT / 16; ++sb) {
      f32x4 st = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < D / 32; ++s) {
        const frag8 qa = *reinterpret_cast<const frag8*>(q_lds + (16 * sb + c) * RS + 8 * g + 32 * s);
        const frag8 ga = *reinterpret_cast<const frag8*>(g_lds + (16 * sb + c) * RS + 8 * g + 32 * s);
        st = mfma16<T>(qa, kf[s], st);
        dp = mfma16<T>(ga, vf[s], dp);
      }
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_lds + 16 * sb + 4 * g);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(delta_lds + 16 * sb + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = qt + 16 * sb + 4 * g + r;
        float dt_ds;
        float p = win_prob<FANCY>(st[r], i, kj, l4[r], sl2e, a.scale, a.softcap, slope, dt_ds);
        if (!full && !(i < N && kj < N && (w < 0 || abs(i - kj) <= w))) p = 0.f;
        pf[sb >> 1][4 * (sb & 1) + r] = to_bits<T>(p);
        tf[sb >> 1][4 * (sb & 1) + r] = to_bits<T>(p * (dp[r] - d4[r]) * dt_ds);
      }
    }
    // dv^T[d 16 db + 4 g + r][key c] += dO^T[d][queries] P[queries][key];  dk^T likewise from Q^T and dT
#pragma unroll
    for (int db = 0; db < D / 16; ++db) {
#pragma unroll
      for (int s = 0; s < QT / 32; ++s) {
        accv[db] = mfma16<T>(transposed_frag(gt_lds, TS, 16 * db + c, s, g), pf[s], accv[db]);
        acck[db] = mfma16<T>(transposed_frag(qt_lds, TS, 16 * db + c, s, g), tf[s], acck[db]);
      }
    }
  }

  if (kj >= N) return;
  T* __restrict__ dkp = (T*)a.dk + (row0 + kj) * a.lddk + (int64_t)h * D;
  T* __restrict__ dvp = (T*)a.dv + (row0 + kj) * a.lddv + (int64_t)h * D;
#pragma unroll
  for (int db = 0; db < D / 16; ++db) {
    Vec<T, 4> ok, ov;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      ok.v[r] = from_float<T>(acck[db][r] * a.scale);
      ov.v[r] = from_float<T>(accv[db][r]);
    }
    *reinterpret_cast<Vec<T, 4>*>(dkp + 16 * db + 4 * g) = ok;
    *reinterpret_cast<Vec<T, 4>*>(dvp + 16 * db + 4 * g) = ov;
  }
}

// ---------------------------------------------------------------------------------------------- any dtype, plain
// p and dT / dS of (query i, key j) from the raw dot product, exactly as win_attn_plain_kernel forms the score
__device__ __forceinline__ float plain_prob(float dot, int i, int j, float lse, float scale, float softcap, float slope, float& dt_ds) {
  float s = dot * scale;
  dt_ds = 1.f;
  if (softcap > 0.f) {
    const float th = tanhf(s / softcap);
    s = softcap * th;
    dt_ds = 1.f - th * th;
  }
  s -= slope * (float)abs(i - j);
  return expf(s - lse);
}

// one wave per (query, head): dq and Delta
template <typename T>
__global__ __launch_bounds__(64) void win_attn_bwd_query_plain_kernel(WinBwdArgs a) {
  __shared__ float q_s[128];
  __shared__ float g_s[128];
  __shared__ float o_s[128];
  __shared__ float t_s[64];
  const int N = a.N, H = a.H, D = a.d, w = a.window;
  const int i = blockIdx.x, bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x;
  const int64_t row0 = (int64_t)b * N;
  const T* __restrict__ qp = (const T*)a.q + (row0 + i) * a.ldq + (int64_t)h * D;
  const T* __restrict__ gp = (const T*)a.d_out + (row0 + i) * a.ldg + (int64_t)h * D;
  const T* __restrict__ op = (const T*)a.out + (row0 + i) * a.ldo + (int64_t)h * D;
  const T* __restrict__ kp = (const T*)a.k + row0 * a.ldk + (int64_t)h * D;
  const T* __restrict__ vp = (const T*)a.v + row0 * a.ldv + (int64_t)h * D;
  for (int x = lane; x < D; x += 64) {
    q_s[x] = to_float(qp[x]);
    g_s[x] = to_float(gp[x]);
    o_s[x] = to_float(op[x]);
  }
  __syncthreads();
  // summed in the order of dP below: where a query attends a single key, out = v and dP - Delta is an exact 0
  float delta = 0.f;
  for (int x = 0; x < D; ++x) delta = fmaf(g_s[x], o_s[x], delta);
  const float lse = a.lse[(row0 + i) * H + h];
  if (lane == 0) a.delta[(row0 + i) * H + h] = delta;
  const int lo = w < 0 ? 0 : max(0, i - w);
  const int hi = w < 0 ? N : min(N, i + w + 1);
  const float slope = a.slopes ? a.slopes[h] : 0.f;
  float d0 = 0.f, d1 = 0.f;
  for (int j0 = lo; j0 < hi; j0 += 64) {
    const int j = j0 + lane;
    float dt = 0.f;
    if (j < hi) {
      const T* kr = kp + (int64_t)j * a.ldk;
      const T* vr = vp + (int64_t)j * a.ldv;
      float dot = 0.f, dp = 0.f;
      for (int x = 0; x < D; ++x) {
        dot = fmaf(q_s[x], to_float(kr[x]), dot);
        dp = fmaf(g_s[x], to_float(vr[x]), dp);
      }
      float dt_ds;
      const float p = plain_prob(dot, i, j, lse, a.scale, a.softcap, slope, dt_ds);
      dt = p * (dp - delta) * dt_ds;
    }
    t_s[lane] = dt;
    __syncthreads();
    const int n = min(64, hi - j0);
    for (int jj = 0; jj < n; ++jj) {
      const T* kr = kp + (int64_t)(j0 + jj) * a.ldk;
      const float tj = t_s[jj];
      if (lane < D) d0 = fmaf(tj, to_float(kr[lane]), d0);
      if (lane + 64 < D) d1 = fmaf(tj, to_float(kr[lane + 64]), d1);
    }
    __syncthreads();
  }
  T* __restrict__ dqp = (T*)a.dq + (row0 + i) * a.lddq + (int64_t)h * D;
  if (lane < D) dqp[lane] = from_float<T>(d0 * a.scale);
  if (lane + 64 < D) dqp[lane + 64] = from_float<T>(d1 * a.scale);
}

// one wave per (key, head): dk and dv
template <typename T>
__global__ __launch_bounds__(64) void win_attn_bwd_key_plain_kernel(WinBwdArgs a) {
  __shared__ float k_s[128];
  __shared__ float v_s[128];
  __shared__ float p_s[64];
  __shared__ float t_s[64];
  const int N = a.N, H = a.H, D = a.d, w = a.window;
  const int j = blockIdx.x, bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x;
  const int64_t row0 = (int64_t)b * N;
  const T* __restrict__ kp = (const T*)a.k + (row0 + j) * a.ldk + (int64_t)h * D;
  const T* __restrict__ vp = (const T*)a.v + (row0 + j) * a.ldv + (int64_t)h * D;
  const T* __restrict__ qp = (const T*)a.q + row0 * a.ldq + (int64_t)h * D;
  const T* __restrict__ gp = (const T*)a.d_out + row0 * a.ldg + (int64_t)h * D;
  for (int x = lane; x < D; x += 64) {
    k_s[x] = to_float(kp[x]);
    v_s[x] = to_float(vp[x]);
  }
  __syncthreads();
  const int lo = w < 0 ? 0 : max(0, j - w);
  const int hi = w < 0 ? N : min(N, j + w + 1);
  const float slope = a.slopes ? a.slopes[h] : 0.f;
  float k0 = 0.f, k1 = 0.f, v0 = 0.f, v1 = 0.f;
  for (int i0 = lo; i0 < hi; i0 += 64) {
    const int i = i0 + lane;
    float p = 0.f, dt = 0.f;
    if (i < hi) {
      const T* qr = qp + (int64_t)i * a.ldq;
      const T* gr = gp + (int64_t)i * a.ldg;
      float dot = 0.f, dp = 0.f;
      for (int x = 0; x < D; ++x) {
        dot = fmaf(to_float(qr[x]), k_s[x], dot);
        dp = fmaf(to_float(gr[x]), v_s[x], dp);
      }
      float dt_ds;
      p = plain_prob(dot, i, j, a.lse[(row0 + i) * H + h], a.scale, a.softcap, slope, dt_ds);
      dt = p * (dp - a.delta[(row0 + i) * H + h]) * dt_ds;
    }
    p_s[lane] = p;
    t_s[lane] = dt;
    __syncthreads();
    const int n = min(64, hi - i0);
    for (int ii = 0; ii < n; ++ii) {
      const T* qr = qp + (int64_t)(i0 + ii) * a.ldq;
      const T* gr = gp + (int64_t)(i0 + ii) * a.ldg;
      const float pi = p_s[ii], ti = t_s[ii];
      if (lane < D) {
        v0 = fmaf(pi, to_float(gr[lane]), v0);
        k0 = fmaf(ti, to_float(qr[lane]), k0);
      }
      if (lane + 64 < D) {
        v1 = fmaf(pi, to_float(gr[lane + 64]), v1);
        k1 = fmaf(ti, to_float(qr[lane + 64]), k1);
      }
    }
    __syncthreads();
  }
  T* __restrict__ dkp = (T*)a.dk + (row0 + j) * a.lddk + (int64_t)h * D;
  T* __restrict__ dvp = (T*)a.dv + (row0 + j) * a.lddv + (int64_t)h * D;
  if (lane < D) {
    dkp[lane] = from_float<T>(k0 * a.scale);
    dvp[lane] = from_float<T>(v0);
  }
  if (lane + 64 < D) {
    dkp[lane + 64] = from_float<T>(k1 * a.scale);
    dvp[lane + 64] = from_float<T>(v1);
  }
}

template <typename T, int D>
int launch_mfma(const WinBwdArgs& a, int passes) {
  const dim3 grid((unsigned)((a.N + kOwn - 1) / kOwn), (unsigned)(a.batch * a.H)), block(64 * kWaves);
  const bool fancy = a.softcap > 0.f || a.slopes;
  if (passes & ANEMOI_WINDOW_BWD_QUERY_PASS) {
    if (fancy)
      hipLaunchKernelGGL((win_attn_bwd_query_kernel<T, D, true>), grid, block, 0, a.stream, a);
    else
      hipLaunchKernelGGL((win_attn_bwd_query_kernel<T, D, false>), grid, block, 0, a.stream, a);
    if (int rc = check_launch("win_attn_bwd_query_kernel")) return rc;
  }
  if (passes & ANEMOI_WINDOW_BWD_KEY_PASS) {
    if (fancy)
      hipLaunchKernelGGL((win_attn_bwd_key_kernel<T, D, true>), grid, block, 0, a.stream, a);
    else
      hipLaunchKernelGGL((win_attn_bwd_key_kernel<T, D, false>), grid, block, 0, a.stream, a);
    if (int rc = check_launch("win_attn_bwd_key_kernel")) return rc;
  }
  return ANEMOI_OK;
}

template <typename T>
int dispatch_16(const WinBwdArgs& a, int passes) {
  switch (a.d) {
    case 32: return launch_mfma<T, 32>(a, passes);
    case 64: return launch_mfma<T, 64>(a, passes);
    default: return launch_mfma<T, 128>(a, passes);
  }
}

bool aligned(const void* p, int64_t ld, int elems) {
  return ((uintptr_t)p % (2 * elems) == 0) && (ld % elems == 0);
}

}  // namespace

}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_window_attention_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* out,
                                           int64_t ldo, const void* d_out, int64_t ldg, const float* lse, void* dq, int64_t lddq, void* dk,
                                           int64_t lddk, void* dv, int64_t lddv, float* delta, int32_t batch, int32_t seq_len, int32_t H,
                                           int32_t d, int32_t window, float scale, float softcap, const float* alibi_slopes, int32_t passes,
                                           anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(batch >= 0 && seq_len >= 0 && H > 0 && d > 0, "window_attention_bwd: bad sizes batch=%d seq_len=%d H=%d d=%d", batch, seq_len,
                 H, d);
  if (d != 32 && d != 64 && d != 128) {
    set_error("window_attention_bwd: head dimension %d not supported; supported: 32, 64, 128", d);
    return ANEMOI_E_UNSUPPORTED;
  }
  ANEMOI_REQUIRE(dtype == ANEMOI_F32 || dtype == ANEMOI_BF16 || dtype == ANEMOI_F16, "window_attention_bwd: bad dtype %d", (int)dtype);
  ANEMOI_REQUIRE((int64_t)batch * H < 65536, "window_attention_bwd: batch * H = %lld too large", (long long)batch * H);
  ANEMOI_REQUIRE(passes > 0 && (passes & ~ANEMOI_WINDOW_BWD_BOTH_PASSES) == 0, "window_attention_bwd: bad passes %d", passes);
  if (batch == 0 || seq_len == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(q && k && v && out && d_out && lse && delta, "window_attention_bwd: null pointer");
  ANEMOI_REQUIRE(!(passes & ANEMOI_WINDOW_BWD_QUERY_PASS) || dq, "window_attention_bwd: null dq");
  ANEMOI_REQUIRE(!(passes & ANEMOI_WINDOW_BWD_KEY_PASS) || (dk && dv), "window_attention_bwd: null dk / dv");
  const int64_t A = (int64_t)H * d;
  ANEMOI_REQUIRE(ldq >= A && ldk >= A && ldv >= A && ldo >= A && ldg >= A && lddq >= A && lddk >= A && lddv >= A,
                 "window_attention_bwd: leading dimension smaller than H*d=%lld", (long long)A);
  ANEMOI_REQUIRE(scale > 0.f, "window_attention_bwd: scale must be positive");
  // normalised as the forward does: a window of seq_len - 1 or more is unbounded, so no band edge can overflow int32
  const int w = (window < 0 || window >= seq_len - 1) ? -1 : window;
  WinBwdArgs a{q, ldq, k, ldk, v, ldv, out, ldo, d_out, ldg, lse, dq, lddq, dk, lddk, dv, lddv, delta, alibi_slopes,
               batch, seq_len, H, d, w, scale, softcap, as_stream(stream)};
  if (dtype == ANEMOI_F32) {
    const dim3 grid((unsigned)seq_len, (unsigned)(batch * H)), block(64);
    if (passes & ANEMOI_WINDOW_BWD_QUERY_PASS) {
      hipLaunchKernelGGL(win_attn_bwd_query_plain_kernel<float>, grid, block, 0, a.stream, a);
      if (int rc = check_launch("win_attn_bwd_query_plain_kernel")) return rc;
    }
    if (passes & ANEMOI_WINDOW_BWD_KEY_PASS) {
      hipLaunchKernelGGL(win_attn_bwd_key_plain_kernel<float>, grid, block, 0, a.stream, a);
      if (int rc = check_launch("win_attn_bwd_key_plain_kernel")) return rc;
    }
    return ANEMOI_OK;
  }
  // 16-byte loads of q / k / v / out / d_out rows, 8-byte stores of dq / dk / dv rows
  ANEMOI_REQUIRE(aligned(q, ldq, 8) && aligned(k, ldk, 8) && aligned(v, ldv, 8) && aligned(out, ldo, 8) && aligned(d_out, ldg, 8),
                 "window_attention_bwd: 16-bit q / k / v / out / d_out need 16-byte aligned rows (pointer and leading dimension)");
  ANEMOI_REQUIRE((!dq || aligned(dq, lddq, 4)) && (!dk || aligned(dk, lddk, 4)) && (!dv || aligned(dv, lddv, 4)),
                 "window_attention_bwd: 16-bit dq / dk / dv need 8-byte aligned rows (pointer and leading dimension)");
  return dtype == ANEMOI_BF16 ? dispatch_16<bf16_t>(a, passes) : dispatch_16<f16_t>(a, passes);
}
