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
// 16-bit path (mfma_f32_16x16x32, fp32 accumulators), on the phases of window_attention_core.h.  As in the forward the scores are
// computed transposed, so that a lane holds 16 scores of ONE owned row (query pass: S^T = K Q^T, lane = query; key pass: S = Q K^T,
// lane = key) and P / dT feed the second GEMM as its B operand in the registers they were computed in.  The streamed tile sits in LDS
// row-major (A operand of the score GEMMs) and transposed (A operand of the gradient GEMMs): the query pass keeps K in both forms and V
// row-major, the key pass Q and dO in both forms plus the lse / Delta strips of the tile's queries.  exp2 with log2(e) folded in; band
// and sequence masks are evaluated only on tiles that cross an edge, and a masked score gives an exact 0.  The key pass streams 64-query
// tiles for d <= 64 and 32-query tiles for d = 128, which keeps its four LDS images under 48 KB.
//
// fp32 path: one wave per (query, head) and one per (key, head), plain and exact (expf, sequential dots) - a correctness path.
#include "window_attention_core.h"

namespace anemoi {

namespace {

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

// ---------------------------------------------------------------------------------------------- 16-bit, MFMA: query pass (dq, Delta)
template <typename T, int D, bool FANCY>
__global__ __launch_bounds__(64 * kWinWaves) void win_attn_bwd_query_kernel(WinBwdArgs a) {
  constexpr int KT = win_tile_rows(kWinBwdQuery, D);  // keys per tile
  __shared__ __attribute__((aligned(16))) uint16_t k_lds[KT * (D + 8)];
  __shared__ __attribute__((aligned(16))) uint16_t v_lds[KT * (D + 8)];
  __shared__ __attribute__((aligned(16))) uint16_t kt_lds[D * (KT + 8)];

  const int N = a.N, H = a.H, w = a.window;
  const WinLane p = win_lane(N, H);
  const int h = p.h, q0 = p.first, tid = p.tid, g = p.g, c = p.c, qw = p.strip;
  const int64_t row0 = p.row0;
  const T* __restrict__ kp = (const T*)a.k;
  const T* __restrict__ vp = (const T*)a.v;
  const WinBand band = win_band(q0, kWinOwn, w, N);
  const int lo = band.lo, hi = band.hi, ntiles = win_tiles(band, KT);
  const int qi = qw + c;
  // q, dO and O of this lane's query as B operands.  Delta comes out of the same MFMA as dP does (the diagonal of O dO^T): where a
  // query attends a single key, out = v and dP - Delta is an exact 0, as it is in exact arithmetic.
  frag8 qf[D / 32], gf[D / 32], of[D / 32];
  float lse2 = 0.f;
  load_row_frags<T, D>(qf, a.q, a.ldq, row0 + qi, (int64_t)h * D + 8 * g, qi < N);
  load_row_frags<T, D>(gf, a.d_out, a.ldg, row0 + qi, (int64_t)h * D + 8 * g, qi < N);
  load_row_frags<T, D>(of, a.out, a.ldo, row0 + qi, (int64_t)h * D + 8 * g, qi < N);
  f32x4 od = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < D / 32; ++s) od = mfma16<T>(of[s], gf[s], od);
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

  frag8 kreg[tile_loads<KT, D>()], vreg[tile_loads<KT, D>()];
  auto load_tile = [&](int kt) { load_tile_pair<T, KT, D>(kreg, vreg, kp, a.ldk, vp, a.ldv, row0, (int64_t)h * D, kt, hi, tid); };
  if (ntiles > 0) load_tile(lo);

  for (int t = 0; t < ntiles; ++t) {
    const int kt = lo + t * KT;
    __syncthreads();  // every wave is done with the previous tile
    store_tile_rows<KT, D>(k_lds, kreg, tid);
    store_tile_rows<KT, D>(v_lds, vreg, tid);
    store_tile_transposed<KT, D>(kt_lds, kreg, tid);
    __syncthreads();
    if (t + 1 < ntiles) load_tile(kt + KT);  // in flight while this tile is worked on

    if (!tile_meets_band(kt, KT, qw, w)) continue;
    const bool full = tile_is_full(kt, KT, qw, N, w);
    frag8 tf[2];
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) {
      f32x4 st, dp, dt;  // S^T and dP^T [key 16 sb + 4 g + r][query c] -> dT^T
      score_block_pair<T, D>(st, dp, k_lds, v_lds, sb, qf, gf, g, c);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = kt + 16 * sb + 4 * g + r;
        float dt_ds;
        float pr = win_prob<FANCY>(st[r], qi, j, lse2, sl2e, a.scale, a.softcap, slope, dt_ds);
        if (!full && !in_band(qi, j, N, w)) pr = 0.f;
        dt[r] = pr * (dp[r] - delta) * dt_ds;
      }
      pack_kslot<T>(tf, sb, dt);
    }
    accumulate_transposed<T, KT, D>(acc, kt_lds, tf, g, c);  // dq^T += K^T dT^T
  }

  if (qi >= N) return;
  store_row_frags<T, D>((T*)a.dq + (row0 + qi) * a.lddq + (int64_t)h * D, acc, a.scale, g);
}

// ---------------------------------------------------------------------------------------------- 16-bit, MFMA: key pass (dk, dv)
template <typename T, int D, bool FANCY>
__global__ __launch_bounds__(64 * kWinWaves) void win_attn_bwd_key_kernel(WinBwdArgs a) {
  constexpr int QT = win_tile_rows(kWinBwdKey, D);  // queries per tile
  __shared__ __attribute__((aligned(16))) uint16_t q_lds[QT * (D + 8)];
  __shared__ __attribute__((aligned(16))) uint16_t g_lds[QT * (D + 8)];
  __shared__ __attribute__((aligned(16))) uint16_t qt_lds[D * (QT + 8)];
  __shared__ __attribute__((aligned(16))) uint16_t gt_lds[D * (QT + 8)];
  __shared__ __attribute__((aligned(16))) float lse_lds[QT];
  __shared__ __attribute__((aligned(16))) float delta_lds[QT];

  const int N = a.N, H = a.H, w = a.window;
  const WinLane p = win_lane(N, H);
  const int g = p.g, c = p.c, tid = p.tid, kj = p.own;
  const T* __restrict__ qp = (const T*)a.q;
  const T* __restrict__ gp = (const T*)a.d_out;
  const WinBand band = win_band(p.first, kWinOwn, w, N);  // the queries of the workgroup's keys
  const int ntiles = (band.hi - band.lo + QT - 1) / QT;  // = win_tiles(band, QT), see below

  // Three phases of this kernel stay spelt out: through win_tiles, load_row_frags and accumulate_transposed the same arithmetic compiled
  // to 4 VGPRs more in some instantiations (profiles/r24_window_attention_helpers_check.txt), which the refactor's check does not allow.
  frag8 kf[D / 32], vf[D / 32];  // k and v of this lane's key as B operands (load_row_frags twice, under one test)
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
    kf[s] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
    vf[s] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
    if (kj < N) {
      const int64_t col = (int64_t)p.h * D + 8 * g + 32 * s;
      kf[s] = *reinterpret_cast<const frag8*>((const T*)a.k + (p.row0 + kj) * a.ldk + col);
      vf[s] = *reinterpret_cast<const frag8*>((const T*)a.v + (p.row0 + kj) * a.ldv + col);
    }
  }
  const float sl2e = a.scale * kLog2e;
  const float slope = (FANCY && a.slopes) ? a.slopes[p.h] : 0.f;

  f32x4 acck[D / 16], accv[D / 16];
#pragma unroll
  for (int db = 0; db < D / 16; ++db) {
    acck[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    accv[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // with a tile's rows the first QT threads carry lse (in the log2 domain) and Delta of one of its queries
  frag8 qreg[tile_loads<QT, D>()], greg[tile_loads<QT, D>()];
  float lreg = 0.f, dreg = 0.f;
  auto load_tile = [&](int qt) {
    load_tile_pair<T, QT, D>(qreg, greg, qp, a.ldq, gp, a.ldg, p.row0, (int64_t)p.h * D, qt, band.hi, tid);
    if (tid < QT) {
      const int i = qt + tid;
      lreg = i < band.hi ? a.lse[(p.row0 + i) * H + p.h] * kLog2e : 0.f;
      dreg = i < band.hi ? a.delta[(p.row0 + i) * H + p.h] : 0.f;
    }
  };
  if (ntiles > 0) load_tile(band.lo);

  for (int t = 0; t < ntiles; ++t) {
    const int qt = band.lo + t * QT;
    __syncthreads();  // every wave is done with the previous tile
    store_tile_rows<QT, D>(q_lds, qreg, tid);
    store_tile_rows<QT, D>(g_lds, greg, tid);
    store_tile_transposed<QT, D>(qt_lds, qreg, tid);
    store_tile_transposed<QT, D>(gt_lds, greg, tid);
    if (tid < QT) {
      lse_lds[tid] = lreg;
      delta_lds[tid] = dreg;
    }
    __syncthreads();
    if (t + 1 < ntiles) load_tile(qt + QT);  // in flight while this tile is worked on

    if (!tile_meets_band(qt, QT, p.strip, w)) continue;
    const bool full = tile_is_full(qt, QT, p.strip, N, w);

    // S and dP [query 16 sb + 4 g + r][key c] -> P and dT
    frag8 pf[QT / 32], tf[QT / 32];
#pragma unroll
    for (int sb = 0; sb < QT / 16; ++sb) {
      f32x4 st, dp;
      score_block_pair<T, D>(st, dp, q_lds, g_lds, sb, kf, vf, g, c);
      const f32x4 l4 = *reinterpret_cast<const f32x4*>(lse_lds + 16 * sb + 4 * g);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(delta_lds + 16 * sb + 4 * g);
      f32x4 p4, dt;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = qt + 16 * sb + 4 * g + r;
        float dt_ds;
        float pr = win_prob<FANCY>(st[r], i, kj, l4[r], sl2e, a.scale, a.softcap, slope, dt_ds);
        if (!full && !in_band(i, kj, N, w)) pr = 0.f;
        p4[r] = pr;
        dt[r] = pr * (dp[r] - d4[r]) * dt_ds;
      }
      pack_kslot<T>(pf, sb, p4);
      pack_kslot<T>(tf, sb, dt);
    }
    // dv^T += dO^T P and dk^T += Q^T dT: accumulate_transposed twice, the two accumulators step by step in turn
#pragma unroll
    for (int db = 0; db < D / 16; ++db) {
#pragma unroll
      for (int s = 0; s < QT / 32; ++s) {
        accv[db] = mfma16<T>(transposed_frag(gt_lds, QT + 8, 16 * db + c, s, g), pf[s], accv[db]);
        acck[db] = mfma16<T>(transposed_frag(qt_lds, QT + 8, 16 * db + c, s, g), tf[s], acck[db]);
      }
    }
  }

  if (kj >= N) return;
  store_row_frags<T, D>((T*)a.dk + (p.row0 + kj) * a.lddk + (int64_t)p.h * D, acck, a.scale, g);
  store_row_frags<T, D>((T*)a.dv + (p.row0 + kj) * a.lddv + (int64_t)p.h * D, accv, 1.f, g);
}

// ---------------------------------------------------------------------------------------------- any dtype, plain
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
  const int lo = win_band(i, 1, w, N).lo, hi = win_band(i, 1, w, N).hi;
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
  const int lo = win_band(j, 1, w, N).lo, hi = win_band(j, 1, w, N).hi;
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

}  // namespace

}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_window_attention_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* out,
                                           int64_t ldo, const void* d_out, int64_t ldg, const float* lse, void* dq, int64_t lddq, void* dk,
                                           int64_t lddk, void* dv, int64_t lddv, float* delta, int32_t batch, int32_t seq_len, int32_t H,
                                           int32_t d, int32_t window, float scale, float softcap, const float* alibi_slopes, int32_t passes,
                                           anemoi_dtype_t dtype, void* stream) {
  if (int rc = win_check_args("window_attention_bwd", batch, seq_len, H, d, dtype, {ldq, ldk, ldv, ldo, ldg, lddq, lddk, lddv}, scale)) return rc;
  ANEMOI_REQUIRE(passes > 0 && (passes & ~ANEMOI_WINDOW_BWD_BOTH_PASSES) == 0, "window_attention_bwd: bad passes %d", passes);
  if (batch == 0 || seq_len == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(q && k && v && out && d_out && lse && delta, "window_attention_bwd: null pointer");
  ANEMOI_REQUIRE(!(passes & ANEMOI_WINDOW_BWD_QUERY_PASS) || dq, "window_attention_bwd: null dq");
  ANEMOI_REQUIRE(!(passes & ANEMOI_WINDOW_BWD_KEY_PASS) || (dk && dv), "window_attention_bwd: null dk / dv");
  const WinBwdArgs a{q, ldq, k, ldk, v, ldv, out, ldo, d_out, ldg, lse, dq, lddq, dk, lddk, dv, lddv, delta, alibi_slopes,
                     batch, seq_len, H, d, win_window(window, seq_len), scale, softcap, as_stream(stream)};
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
  // 16-byte loads of q / k / v / out / d_out rows, 8-byte stores of dq / dk / dv rows (an absent gradient is not asked about)
  ANEMOI_REQUIRE(win_rows_aligned({{q, ldq}, {k, ldk}, {v, ldv}, {out, ldo}, {d_out, ldg}}, 8),
                 "window_attention_bwd: 16-bit q / k / v / out / d_out need 16-byte aligned rows (pointer and leading dimension)");
  ANEMOI_REQUIRE(win_rows_aligned({{dq, dq ? lddq : 0}, {dk, dk ? lddk : 0}, {dv, dv ? lddv : 0}}, 4),
                 "window_attention_bwd: 16-bit dq / dk / dv need 8-byte aligned rows (pointer and leading dimension)");
  return with_win_instance(dtype, d, softcap > 0.f || alibi_slopes, [&](auto t, auto d_c, auto fancy_c) {
    using T = decltype(t);
    constexpr int D = decltype(d_c)::value;
    constexpr bool FANCY = decltype(fancy_c)::value;
    const dim3 grid((unsigned)((a.N + kWinOwn - 1) / kWinOwn), (unsigned)(a.batch * a.H)), block(64 * kWinWaves);
    if (passes & ANEMOI_WINDOW_BWD_QUERY_PASS) {
      hipLaunchKernelGGL((win_attn_bwd_query_kernel<T, D, FANCY>), grid, block, 0, a.stream, a);
      if (int rc = check_launch("win_attn_bwd_query_kernel")) return rc;
    }
    if (passes & ANEMOI_WINDOW_BWD_KEY_PASS) {
      hipLaunchKernelGGL((win_attn_bwd_key_kernel<T, D, FANCY>), grid, block, 0, a.stream, a);
      if (int rc = check_launch("win_attn_bwd_key_kernel")) return rc;
    }
    return (int)ANEMOI_OK;
  });
}
