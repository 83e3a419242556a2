// Sliding-window (banded) multi-head self-attention, forward, for gfx950.
//
// Spec: the reference's MultiHeadSelfAttention with flash-attention semantics (models/src/anemoi/models/layers/attention.py:41-262,
// 362-520): rows are (batch grid), query i of a sequence attends keys j of the same sequence with |i - j| <= w (w < 0: all keys),
//   s = <q_i, k_j> * scale;  s = softcap * tanh(s / softcap) if softcap > 0;  s -= slope_h * |i - j| if ALiBi;
//   out_i = sum_j softmax_j(s) v_j,  lse_i = ln sum_j exp(s_j - max) + max.
//
// 16-bit path (flash-style, mfma_f32_16x16x32), on the phases of window_attention_core.h: a workgroup of four waves owns 64 query rows
// of one (sequence, head); only the 64-key tiles that meet [q0 - w, q1 + w] ∩ [0, N) are visited, so the work is N (2w + 1), not N^2.
// It keeps K row-major and V transposed in LDS; the next tile's rows are loaded into registers while the current one is worked on.  The
// scores are computed transposed, S^T = K Q^T, so that a lane holds 16 scores of ONE query (4 key groups x 4 registers): the softmax
// statistics - this kernel's own part - need two cross-lane steps per tile, and the probabilities feed P V (as O^T = V^T P^T) in the
// registers they were computed in.  log2(e) * scale is folded into one multiply and exp2.  A score outside the band or the sequence is
// -inf before the exponential, i.e. an exact 0; the masks are evaluated only on the tiles that cross a band or sequence edge.
//
// fp32 path: one wave per (query, head), plain and exact (expf, sequential dots) - a correctness path, not a fast one.
// anemoi_window_attention_plan (at the end) answers for all three MFMA kernels, forward and backward, from the same band functions.
#include "window_attention_core.h"

namespace anemoi {

namespace {

struct WinArgs {
  const void* q;
  int64_t ldq;
  const void* k;
  int64_t ldk;
  const void* v;
  int64_t ldv;
  void* out;
  int64_t ldo;
  float* lse;
  const float* slopes;
  int batch, N, H, d, window;
  float scale, softcap;
  hipStream_t stream;
};

// ---------------------------------------------------------------------------------------------- 16-bit, MFMA
template <typename T, int D, bool FANCY>
__global__ __launch_bounds__(64 * kWinWaves) void win_attn_mfma_kernel(WinArgs a) {
  constexpr int KT = win_tile_rows(kWinFwd, D);  // keys per tile
  constexpr int VS = KT + 8;                     // V^T tile row stride
  __shared__ __attribute__((aligned(16))) uint16_t k_lds[KT * (D + 8)];
  __shared__ __attribute__((aligned(16))) uint16_t vt_lds[D * VS];

  const int N = a.N, H = a.H, w = a.window;
  const WinLane p = win_lane(N, H);
  const int h = p.h, q0 = p.first, tid = p.tid, g = p.g, c = p.c, qw = p.strip;
  const int64_t row0 = p.row0;
  const T* __restrict__ kp = (const T*)a.k;
  const T* __restrict__ vp = (const T*)a.v;
  const WinBand band = win_band(q0, kWinOwn, w, N);  // the keys of the workgroup's queries
  const int lo = band.lo, hi = band.hi, ntiles = win_tiles(band, KT);
  // Three phases of this kernel stay spelt out - the owned-row load (load_row_frags), the element mask (in_band) and the accumulate
  // GEMM (accumulate_transposed): through the helpers an instantiation took 4 VGPRs more, or the d = 64 kernel ran 1 % longer.  And
  // the loader is called through a lambda, here and in the query pass: called directly, twice, the d = 64 kernels ran 3.7 % (with a
  // window) and 6 % longer.  profiles/r24_window_attention_helpers_check.txt has the figures.
  const int qi = qw + c;
  frag8 qf[D / 32];  // Q of this lane's query as the B operand of S^T = K Q^T: Q[qw + c][8g + j + 32 s]
#pragma unroll
  for (int s = 0; s < D / 32; ++s) {
    if (qi < N)
      qf[s] = *reinterpret_cast<const frag8*>((const T*)a.q + (row0 + qi) * a.ldq + (int64_t)h * D + 8 * g + 32 * s);
    else
      qf[s] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  const float sl2e = a.scale * kLog2e;
  const float slope = (FANCY && a.slopes) ? a.slopes[h] : 0.f;

  f32x4 acc[D / 16];
#pragma unroll
  for (int db = 0; db < D / 16; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  frag8 kreg[tile_loads<KT, D>()], vreg[tile_loads<KT, D>()];
  auto load_tile = [&](int kt) { load_tile_pair<T, KT, D>(kreg, vreg, kp, a.ldk, vp, a.ldv, row0, (int64_t)h * D, kt, hi, tid); };
  if (ntiles > 0) load_tile(lo);

  for (int t = 0; t < ntiles; ++t) {
    const int kt = lo + t * KT;
    __syncthreads();  // every wave is done with the previous tile
    store_tile_rows<KT, D>(k_lds, kreg, tid);
    store_tile_transposed<KT, D>(vt_lds, vreg, tid);
    __syncthreads();
    if (t + 1 < ntiles) load_tile(kt + KT);  // in flight while this tile is worked on

    if (!tile_meets_band(kt, KT, qw, w)) continue;
    const bool full = tile_is_full(kt, KT, qw, N, w);
    f32x4 st[4];  // S^T[key 16 sb + 4 g + r][query c]
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) st[sb] = score_block<T, D>(k_lds, sb, qf, g, c);
    float mx = -INFINITY;
#pragma unroll
    for (int sb = 0; sb < 4; ++sb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = kt + 16 * sb + 4 * g + r;
        float x = win_score<FANCY>(st[sb][r], qi, j, sl2e, a.scale, a.softcap, slope);
        if (!full && !(j < N && (w < 0 || abs(qi - j) <= w))) x = -INFINITY;  // = in_band(qi, j, N, w) where qi < N
        st[sb][r] = x;
        mx = fmaxf(mx, x);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m, mx);
    const float base = m_new == -INFINITY ? 0.f : m_new;  // a query with no key yet: every p is 0, nothing is rescaled into a NaN
    const float corr = __builtin_amdgcn_exp2f(m - base);
    m = m_new;
    l *= corr;
#pragma unroll
    for (int db = 0; db < D / 16; ++db) acc[db] *= corr;
    frag8 pf[2];
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st[sb][r] = __builtin_amdgcn_exp2f(st[sb][r] - base);
        l += st[sb][r];
      }
      pack_kslot<T>(pf, sb, st[sb]);
    }
    // O^T[d 16 db + 4 g + r][query c] += V^T[d][keys] P^T[keys][query]
#pragma unroll
    for (int db = 0; db < D / 16; ++db) {
#pragma unroll
      for (int s = 0; s < 2; ++s) acc[db] = mfma16<T>(transposed_frag(vt_lds, VS, 16 * db + c, s, g), pf[s], acc[db]);
    }
  }
  // the row sum over the four key groups of the query
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (qi >= N) return;
  const float inv = l > 0.f ? 1.f / l : 0.f;
  store_row_frags<T, D>((T*)a.out + (row0 + qi) * a.ldo + (int64_t)h * D, acc, inv, g);
  if (a.lse && g == 0) a.lse[(row0 + qi) * H + h] = (m + log2f(l)) * kLn2;
}

// ---------------------------------------------------------------------------------------------- any dtype, plain
template <typename T>
__global__ __launch_bounds__(64) void win_attn_plain_kernel(WinArgs a) {
  __shared__ float q_s[128];
  __shared__ float p_s[64];
  const int N = a.N, H = a.H, D = a.d, w = a.window;
  const int i = blockIdx.x, bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int lane = threadIdx.x;
  const int64_t row0 = (int64_t)b * N;
  const T* __restrict__ qp = (const T*)a.q + (row0 + i) * a.ldq + (int64_t)h * D;
  const T* __restrict__ kp = (const T*)a.k + row0 * a.ldk + (int64_t)h * D;
  const T* __restrict__ vp = (const T*)a.v + row0 * a.ldv + (int64_t)h * D;
  for (int x = lane; x < D; x += 64) q_s[x] = to_float(qp[x]);
  __syncthreads();
  const int lo = win_band(i, 1, w, N).lo, hi = win_band(i, 1, w, N).hi;
  const float slope = a.slopes ? a.slopes[h] : 0.f;
  float m = -INFINITY, l = 0.f, o0 = 0.f, o1 = 0.f;
  for (int j0 = lo; j0 < hi; j0 += 64) {
    const int j = j0 + lane;
    float s = -INFINITY;
    if (j < hi) {
      const T* kr = kp + (int64_t)j * a.ldk;
      float dot = 0.f;
      for (int x = 0; x < D; ++x) dot = fmaf(q_s[x], to_float(kr[x]), dot);
      s = plain_score(dot, i, j, a.scale, a.softcap, slope);
    }
    float mx = s;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float m_new = fmaxf(m, mx);  // finite: key j0 (>= lo) is in the band
    const float corr = expf(m - m_new);
    const float p = j < hi ? expf(s - m_new) : 0.f;
    m = m_new;
    l = l * corr + wave_sum(p);
    o0 *= corr;
    o1 *= corr;
    p_s[lane] = p;
    __syncthreads();
    const int n = min(64, hi - j0);
    for (int jj = 0; jj < n; ++jj) {
      const T* vr = vp + (int64_t)(j0 + jj) * a.ldv;
      const float pj = p_s[jj];
      if (lane < D) o0 = fmaf(pj, to_float(vr[lane]), o0);
      if (lane + 64 < D) o1 = fmaf(pj, to_float(vr[lane + 64]), o1);
    }
    __syncthreads();
  }
  T* __restrict__ op = (T*)a.out + (row0 + i) * a.ldo + (int64_t)h * D;
  if (lane < D) op[lane] = from_float<T>(o0 / l);
  if (lane + 64 < D) op[lane + 64] = from_float<T>(o1 / l);
  if (a.lse && lane == 0) a.lse[(row0 + i) * H + h] = m + logf(l);
}

}  // namespace

}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_window_attention_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out,
                                           int64_t ldo, float* lse, int32_t batch, int32_t seq_len, int32_t H, int32_t d, int32_t window,
                                           float scale, float softcap, const float* alibi_slopes, anemoi_dtype_t dtype, void* stream) {
  if (int rc = win_check_args("window_attention_fwd", batch, seq_len, H, d, dtype, {ldq, ldk, ldv, ldo}, scale)) return rc;
  if (batch == 0 || seq_len == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(q && k && v && out, "window_attention_fwd: null pointer");
  const WinArgs a{q, ldq, k, ldk, v, ldv, out, ldo, lse, alibi_slopes, batch, seq_len, H, d, win_window(window, seq_len), scale, softcap,
                  as_stream(stream)};
  if (dtype == ANEMOI_F32) {
    hipLaunchKernelGGL(win_attn_plain_kernel<float>, dim3((unsigned)seq_len, (unsigned)(batch * H)), dim3(64), 0, a.stream, a);
    return check_launch("win_attn_plain_kernel");
  }
  // 16-byte loads of q / k / v rows, 8-byte stores of out rows
  ANEMOI_REQUIRE(win_rows_aligned({{q, ldq}, {k, ldk}, {v, ldv}}, 8) && win_rows_aligned({{out, ldo}}, 4),
                 "window_attention_fwd: 16-bit q / k / v need 16-byte aligned rows (pointer and leading dimension), out 8-byte aligned rows");
  return with_win_instance(dtype, d, softcap > 0.f || alibi_slopes, [&](auto t, auto d_c, auto fancy_c) {
    const dim3 grid((unsigned)((a.N + kWinOwn - 1) / kWinOwn), (unsigned)(a.batch * a.H)), block(64 * kWinWaves);
    hipLaunchKernelGGL((win_attn_mfma_kernel<decltype(t), decltype(d_c)::value, decltype(fancy_c)::value>), grid, block, 0, a.stream, a);
    return check_launch("win_attn_mfma_kernel");
  });
}

// Host-only: what the kernels of `pass` do with the rows of one wave, from the band functions the kernels call.  fp32 (the plain kernels):
// a workgroup is one wave and owns one row, every tile of its band is visited, and a tile is full if no lane of it reaches `hi`.
extern "C" int anemoi_window_attention_plan(int32_t pass, int32_t seq_len, int32_t d, int32_t window, anemoi_dtype_t dtype, int32_t block,
                                            int32_t wave, anemoi_window_attention_plan_t* out, int32_t* tile_class, int32_t tile_capacity) {
  ANEMOI_REQUIRE(out != nullptr && (tile_class != nullptr || tile_capacity <= 0), "window_attention_plan: null out");
  ANEMOI_REQUIRE(pass >= kWinFwd && pass <= kWinBwdKey, "window_attention_plan: unknown pass %d", pass);
  if (int rc = win_check_args("window_attention_plan", 1, seq_len, 1, d, dtype, {}, 1.f)) return rc;
  const bool plain = dtype == ANEMOI_F32;
  const int own = plain ? 1 : kWinOwn, grid_x = (seq_len + own - 1) / own;
  ANEMOI_REQUIRE(block >= 0 && block < (grid_x > 0 ? grid_x : 1) && wave >= 0 && wave < (plain ? 1 : kWinWaves),
                 "window_attention_plan: no block %d, wave %d", block, wave);
  const int w = win_window(window, seq_len), rows = win_tile_rows(plain ? kWinFwd : pass, d), first = block * own, strip = first + 16 * wave;
  const WinBand band = win_band(first, own, w, seq_len);
  *out = anemoi_window_attention_plan_t{w, own, grid_x, rows, band.lo, band.hi, win_tiles(band, rows)};
  for (int t = 0; t < out->ntiles && t < tile_capacity; ++t) {
    const int t0 = band.lo + t * rows;
    if (plain)
      tile_class[t] = t0 + rows <= band.hi ? ANEMOI_WINDOW_TILE_FULL : ANEMOI_WINDOW_TILE_MASKED;
    else
      tile_class[t] = !tile_meets_band(t0, rows, strip, w)          ? ANEMOI_WINDOW_TILE_SKIPPED
                      : tile_is_full(t0, rows, strip, seq_len, w) ? ANEMOI_WINDOW_TILE_FULL
                                                                  : ANEMOI_WINDOW_TILE_MASKED;
  }
  return ANEMOI_OK;
}
