// Sliding-window (banded) multi-head self-attention, forward, for gfx950.
//
// Spec: the reference's MultiHeadSelfAttention with flash-attention semantics (models/src/anemoi/models/layers/attention.py:41-262,
// 362-520): rows are (batch grid), query i of a sequence attends keys j of the same sequence with |i - j| <= w (w < 0: all keys),
//   s = <q_i, k_j> * scale;  s = softcap * tanh(s / softcap) if softcap > 0;  s -= slope_h * |i - j| if ALiBi;
//   out_i = sum_j softmax_j(s) v_j,  lse_i = ln sum_j exp(s_j - max) + max.
//
// 16-bit path (flash-style, mfma_f32_16x16x32): a workgroup of four waves owns 64 query rows of one (sequence, head); each wave 16 of
// them.  Only the 64-key tiles that meet [q0 - w, q1 + w] ∩ [0, N) are visited, so the work is N (2w + 1), not N^2.  A tile's K rows
// ([key][d]) and V^T ([d][key]) sit in LDS, shared by the four waves; the next tile's rows are loaded into registers while the current
// one is worked on.  The scores are computed transposed, S^T = K Q^T, so that a lane holds 16 scores of ONE query (4 key groups x 4
// registers): the softmax statistics need two cross-lane steps per tile, and the probabilities feed P V (as O^T = V^T P^T) in the
// registers they were computed in - the k order of that MFMA is permuted to match (key of k slot 8g + j = 16(2s + j/4) + 4g + j%4).
// log2(e) * scale is folded into one multiply and exp2.  A score outside the band or the sequence is -inf before the exponential, i.e.
// an exact 0; the masks are evaluated only on the tiles that cross a band or sequence edge.
//
// fp32 path: one wave per (query, head), plain and exact (expf, sequential dots) - a correctness path, not a fast one.
#include "window_attention_core.h"

namespace anemoi {

namespace {

constexpr int kWinWaves = 4;
constexpr int kWinQ = 16 * kWinWaves;  // query rows per workgroup
constexpr int kWinK = 64;              // keys per tile

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

// the score of query i, key j from the raw dot product, in the log2 domain (FANCY: softcap and / or ALiBi)
template <bool FANCY>
__device__ __forceinline__ float win_score(float dot, int i, int j, float sl2e, float scale, float softcap, float slope) {
  if constexpr (!FANCY) {
    return dot * sl2e;
  } else {
    float s = dot * scale;
    if (softcap > 0.f) s = softcap * tanhf(s / softcap);
    s -= slope * (float)abs(i - j);
    return s * kLog2e;
  }
}

// ---------------------------------------------------------------------------------------------- 16-bit, MFMA
template <typename T, int D, bool FANCY>
__global__ __launch_bounds__(64 * kWinWaves) void win_attn_mfma_kernel(WinArgs a) {
  constexpr int KS = D + 8;       // K tile row stride in elements (16 B of padding against bank conflicts)
  constexpr int VS = kWinK + 8;   // V^T tile row stride
  constexpr int CH = D / 8;       // 16-byte chunks per row
  constexpr int LOADS = kWinK * CH / (64 * kWinWaves);  // 16-byte chunks per thread and tile (K and V each)
  static_assert(LOADS >= 1 && kWinK * CH % (64 * kWinWaves) == 0, "tile loads");
  __shared__ __attribute__((aligned(16))) uint16_t k_lds[kWinK * KS];
  __shared__ __attribute__((aligned(16))) uint16_t vt_lds[D * VS];

  const int N = a.N, H = a.H, w = a.window;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int q0 = blockIdx.x * kWinQ;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const int qw = q0 + wave * 16;  // this wave's first query
  const int64_t row0 = (int64_t)b * N;
  const T* __restrict__ qp = (const T*)a.q;
  const T* __restrict__ kp = (const T*)a.k;
  const T* __restrict__ vp = (const T*)a.v;

  // key range of the workgroup: the band of its query rows
  const int lo = w < 0 ? 0 : max(0, q0 - w);
  const int hi = w < 0 ? N : min(N, q0 + kWinQ + w);
  const int ntiles = (hi - lo + kWinK - 1) / kWinK;

  // Q of this lane's query as the B operand of S^T = K Q^T: Q[qw + c][8g + j + 32 s]
  const int qi = qw + c;
  frag8 qf[D / 32];
  {
#pragma unroll
    for (int s = 0; s < D / 32; ++s) {
      if (qi < N)
        qf[s] = *reinterpret_cast<const frag8*>(qp + (row0 + qi) * a.ldq + (int64_t)h * D + 8 * g + 32 * s);
      else
        qf[s] = frag8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  const float sl2e = a.scale * kLog2e;
  const float slope = (FANCY && a.slopes) ? a.slopes[h] : 0.f;

  f32x4 acc[D / 16];
#pragma unroll
  for (int db = 0; db < D / 16; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  // the tile loader: chunk e of this thread = (key e / CH, 8 columns at 8 (e % CH)); keys beyond the range are zeros
  frag8 kreg[LOADS], vreg[LOADS];
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      const int e = tid + u * 64 * kWinWaves, key = e / CH, col = 8 * (e % CH);
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
    const int kt = lo + t * kWinK;
    __syncthreads();  // every wave is done with the previous tile
#pragma unroll
    for (int u = 0; u < LOADS; ++u) {
      const int e = tid + u * 64 * kWinWaves, key = e / CH, col = 8 * (e % CH);
      *reinterpret_cast<frag8*>(k_lds + key * KS + col) = kreg[u];
#pragma unroll
      for (int x = 0; x < 8; ++x) vt_lds[(col + x) * VS + key] = (uint16_t)vreg[u][x];
    }
    __syncthreads();
    if (t + 1 < ntiles) load_tile(kt + kWinK);  // in flight while this tile is worked on

    // does the tile meet this wave's band at all, and does it need the masks?
    const int klast = kt + kWinK - 1;
    if (w >= 0 && (kt > qw + 15 + w || klast < qw - w)) continue;
    const bool full = klast < N && qw + 15 < N && (w < 0 || (klast - qw <= w && qw + 15 - kt <= w));

    // S^T[key 16 sb + 4 g + r][query c]
    f32x4 st[4];
#pragma unroll
    for (int sb = 0; sb < 4; ++sb) {
      f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < D / 32; ++s) {
        const frag8 kf = *reinterpret_cast<const frag8*>(k_lds + (16 * sb + c) * KS + 8 * g + 32 * s);
        z = mfma16<T>(kf, qf[s], z);
      }
      st[sb] = z;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int sb = 0; sb < 4; ++sb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = kt + 16 * sb + 4 * g + r;
        float x = win_score<FANCY>(st[sb][r], qi, j, sl2e, a.scale, a.softcap, slope);
        if (!full && !(j < N && (w < 0 || abs(qi - j) <= w))) x = -INFINITY;
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
    for (int sb = 0; sb < 4; ++sb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(st[sb][r] - base);
        l += p;
        pf[sb >> 1][4 * (sb & 1) + r] = to_bits<T>(p);
      }
    // O^T[d 16 db + 4 g + r][query c] += V^T[d][keys] P^T[keys][query]; k slot 8g + j of step s is key 32 s + 16 (j / 4) + 4 g + j % 4
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
  T* __restrict__ op = (T*)a.out + (row0 + qi) * a.ldo + (int64_t)h * D;
#pragma unroll
  for (int db = 0; db < D / 16; ++db) {
    Vec<T, 4> o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o.v[r] = from_float<T>(acc[db][r] * inv);
    *reinterpret_cast<Vec<T, 4>*>(op + 16 * db + 4 * g) = o;
  }
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
  const int lo = w < 0 ? 0 : max(0, i - w);
  const int hi = w < 0 ? N : min(N, i + w + 1);
  const float slope = a.slopes ? a.slopes[h] : 0.f;
  float m = -INFINITY, l = 0.f, o0 = 0.f, o1 = 0.f;
  for (int j0 = lo; j0 < hi; j0 += 64) {
    const int j = j0 + lane;
    float s = -INFINITY;
    if (j < hi) {
      const T* kr = kp + (int64_t)j * a.ldk;
      float dot = 0.f;
      for (int x = 0; x < D; ++x) dot = fmaf(q_s[x], to_float(kr[x]), dot);
      s = dot * a.scale;
      if (a.softcap > 0.f) s = a.softcap * tanhf(s / a.softcap);
      s -= slope * (float)abs(i - j);
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

template <typename T, int D>
int launch_mfma(const WinArgs& a) {
  const dim3 grid((unsigned)((a.N + kWinQ - 1) / kWinQ), (unsigned)(a.batch * a.H)), block(64 * kWinWaves);
  if (a.softcap > 0.f || a.slopes)
    hipLaunchKernelGGL((win_attn_mfma_kernel<T, D, true>), grid, block, 0, a.stream, a);
  else
    hipLaunchKernelGGL((win_attn_mfma_kernel<T, D, false>), grid, block, 0, a.stream, a);
  return check_launch("win_attn_mfma_kernel");
}

template <typename T>
int dispatch_16(const WinArgs& a) {
  switch (a.d) {
    case 32: return launch_mfma<T, 32>(a);
    case 64: return launch_mfma<T, 64>(a);
    default: return launch_mfma<T, 128>(a);
  }
}

bool aligned(const void* p, int64_t ld, int elems) {
  return ((uintptr_t)p % 16 == 0) && (ld % elems == 0);
}

}  // namespace

}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_window_attention_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out,
                                           int64_t ldo, float* lse, int32_t batch, int32_t seq_len, int32_t H, int32_t d, int32_t window,
                                           float scale, float softcap, const float* alibi_slopes, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(batch >= 0 && seq_len >= 0 && H > 0 && d > 0, "window_attention_fwd: bad sizes batch=%d seq_len=%d H=%d d=%d", batch, seq_len,
                 H, d);
  if (d != 32 && d != 64 && d != 128) {
    set_error("window_attention_fwd: head dimension %d not supported; supported: 32, 64, 128", d);
    return ANEMOI_E_UNSUPPORTED;
  }
  ANEMOI_REQUIRE(dtype == ANEMOI_F32 || dtype == ANEMOI_BF16 || dtype == ANEMOI_F16, "window_attention_fwd: bad dtype %d", (int)dtype);
  ANEMOI_REQUIRE((int64_t)batch * H < 65536, "window_attention_fwd: batch * H = %lld too large", (long long)batch * H);
  if (batch == 0 || seq_len == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(q && k && v && out, "window_attention_fwd: null pointer");
  const int64_t A = (int64_t)H * d;
  ANEMOI_REQUIRE(ldq >= A && ldk >= A && ldv >= A && ldo >= A, "window_attention_fwd: leading dimension smaller than H*d=%lld", (long long)A);
  ANEMOI_REQUIRE(scale > 0.f, "window_attention_fwd: scale must be positive");
  // a window of seq_len - 1 or more covers every key: unbounded (and no band edge such as q0 + 64 + w can overflow int32)
  const int w = (window < 0 || window >= seq_len - 1) ? -1 : window;
  WinArgs a{q, ldq, k, ldk, v, ldv, out, ldo, lse, alibi_slopes, batch, seq_len, H, d, w, scale, softcap, as_stream(stream)};
  if (dtype == ANEMOI_F32) {
    hipLaunchKernelGGL(win_attn_plain_kernel<float>, dim3((unsigned)seq_len, (unsigned)(batch * H)), dim3(64), 0, a.stream, a);
    return check_launch("win_attn_plain_kernel");
  }
  // 16-byte loads of q / k / v rows, 8-byte stores of out rows
  ANEMOI_REQUIRE(aligned(q, ldq, 8) && aligned(k, ldk, 8) && aligned(v, ldv, 8) && (uintptr_t)out % 8 == 0 && ldo % 4 == 0,
                 "window_attention_fwd: 16-bit q / k / v need 16-byte aligned rows (pointer and leading dimension), out 8-byte aligned rows");
  return dtype == ANEMOI_BF16 ? dispatch_16<bf16_t>(a) : dispatch_16<f16_t>(a);
}
