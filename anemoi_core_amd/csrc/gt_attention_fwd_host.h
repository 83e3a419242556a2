// Edge attention, forward: everything but the fused-edge forward kernel - the materialised-E wave kernel, the generic kernel, the
// pack kernels, the launches (from the plan of gt_attention_plan.h) and the C entry points.  Included at the END of a translation
// unit that has defined gt_attn_fused_edge_fwd_kernel<T, VEC, LPH, FE_PAD, KVADJ> behind gt_attention_core.h: gt_attention.hip (the
// product's kernel) and csrc/experiments/gt_attention_r05_variants.hip (the measured-and-superseded ones).
#pragma once
#include "gt_attention_core.h"

namespace anemoi {

template <int VEC>
struct EdgeRow {
  float k[VEC];
  float v[VEC];
  float e[VEC];
};

// ---------------------------------------------------------------------------------------------- fast path
template <typename T, int VEC, int LPH, bool HAS_E>
__global__ __launch_bounds__(64 * kWavesPerBlock) void gt_attn_fwd_kernel(
    const T* __restrict__ q, int64_t ldq, const T* __restrict__ k, int64_t ldk, const T* __restrict__ v, int64_t ldv,
    const T* __restrict__ e, int64_t lde, const int32_t* __restrict__ row, const int32_t* __restrict__ colptr,
    const T* __restrict__ addend, int64_t ldadd, T* __restrict__ out, int64_t ldo, float* __restrict__ lse, int n_dst,
    int H, float scale, float drop_p, uint64_t drop_seed) {
  const int lane = threadIdx.x & 63;
  const int d = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
  if (d >= n_dst) return;
  const int beg = __builtin_amdgcn_readfirstlane(colptr[d]);
  const int end = __builtin_amdgcn_readfirstlane(colptr[d + 1]);
  const int c0 = lane * VEC;
  const float inv_keep = 1.0f / (1.0f - drop_p);

  float qv[VEC], acc[VEC];
  load_vec<T, VEC>(q + (int64_t)d * ldq + c0, qv);
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    qv[j] *= scale;
    acc[j] = 0.f;
  }
  float m = -INFINITY, l = 0.f;

  EdgeRow<VEC> cur, nxt;
  auto fetch = [&](int ei, EdgeRow<VEC>& r) {
    const int s = __builtin_amdgcn_readfirstlane(row[ei]);
    load_vec<T, VEC>(k + (int64_t)s * ldk + c0, r.k);
    load_vec<T, VEC>(v + (int64_t)s * ldv + c0, r.v);
    if constexpr (HAS_E) load_vec<T, VEC>(e + (int64_t)ei * lde + c0, r.e);
  };
  if (beg < end) fetch(beg, nxt);
  for (int ei = beg; ei < end; ++ei) {
    cur = nxt;
    if (ei + 1 < end) fetch(ei + 1, nxt);
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if constexpr (HAS_E) {
        cur.k[j] += cur.e[j];
        cur.v[j] += cur.e[j];
      }
      dot = fmaf(qv[j], cur.k[j], dot);
    }
    dot = group_sum<LPH>(dot);
    const float m_new = fmaxf(m, dot);
    const float corr = __expf(m - m_new);  // first edge: exp(-inf) = 0
    const float p = __expf(dot - m_new);
    l = fmaf(l, corr, p);
    // dropout acts on the NORMALISED weight: the denominator sums every edge, the numerator the kept ones (scaled by 1 / (1 - p))
    const float pv = drop_p > 0.f ? p * attn_dropout_scale(drop_seed, ei, lane / LPH, drop_p, inv_keep) : p;
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = fmaf(acc[j], corr, pv * cur.v[j]);
    m = m_new;
  }

  const float inv = (end > beg) ? 1.0f / l : 0.f;
  float o[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) o[j] = acc[j] * inv;
  if (addend != nullptr) {
    float a[VEC];
    load_vec<T, VEC>(addend + (int64_t)d * ldadd + c0, a);
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] += a[j];
  }
  store_vec<T, VEC>(out + (int64_t)d * ldo + c0, o);
  if (lse != nullptr && (lane % LPH) == 0) lse[(int64_t)d * H + lane / LPH] = (end > beg) ? m + __logf(l) : 0.f;
}

// ---------------------------------------------------------------------------------------------- generic path
// Any (H, C): one thread per (destination, head), serial over edges and channels.  Used for shapes the
// wave-per-row layout cannot express (D not a multiple of 64, non power-of-two lanes per head — e.g. the
// reference's own test shapes H in {2,6}, C in {4,6}).  Correctness path, not a performance path.
template <typename T>
__global__ void gt_attn_fwd_generic_kernel(const T* __restrict__ q, int64_t ldq, const T* __restrict__ k, int64_t ldk,
                                           const T* __restrict__ v, int64_t ldv, const T* __restrict__ e, int64_t lde,
                                           const float* __restrict__ feat, int fe, int fe_pad,
                                           const float* __restrict__ w_packed,
                                           const int32_t* __restrict__ row, const int32_t* __restrict__ colptr,
                                           const T* __restrict__ addend, int64_t ldadd, T* __restrict__ out,
                                           int64_t ldo, float* __restrict__ lse, int n_dst, int H, int C, float scale,
                                           float drop_p, uint64_t drop_seed) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)n_dst * H) return;
  const int d = (int)(t / H), h = (int)(t % H);
  const int beg = colptr[d], end = colptr[d + 1];
  const float inv_keep = 1.0f / (1.0f - drop_p);
  float acc[kGenericMaxC];  // private (scratch-memory) fp32 accumulator
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  float m = -INFINITY, l = 0.f;
  const T* qp = q + (int64_t)d * ldq + h * C;
  for (int ei = beg; ei < end; ++ei) {
    const int s = row[ei];
    const T* kp = k + (int64_t)s * ldk + h * C;
    const T* vp = v + (int64_t)s * ldv + h * C;
    float dot = 0.f;
    for (int c = 0; c < C; ++c) {
      float ee = 0.f;
      if (e != nullptr) ee = to_float(e[(int64_t)ei * lde + h * C + c]);
      if (feat != nullptr) {
        ee = 0.f;  // the bias rides on the constant-1 feature column fe
        for (int f = 0; f < fe_pad; ++f) ee = fmaf(feat[(int64_t)ei * fe_pad + f], w_packed[(int64_t)(h * C + c) * fe_pad + f], ee);
      }
      dot = fmaf(to_float(qp[c]) * scale, to_float(kp[c]) + ee, dot);
    }
    const float m_new = fmaxf(m, dot);
    const float corr = expf(m - m_new), p = expf(dot - m_new);
    l = l * corr + p;
    const float pv = drop_p > 0.f ? p * attn_dropout_scale(drop_seed, ei, h, drop_p, inv_keep) : p;
    for (int c = 0; c < C; ++c) {
      float ee = 0.f;
      if (e != nullptr) ee = to_float(e[(int64_t)ei * lde + h * C + c]);
      if (feat != nullptr) {
        ee = 0.f;  // the bias rides on the constant-1 feature column fe
        for (int f = 0; f < fe_pad; ++f) ee = fmaf(feat[(int64_t)ei * fe_pad + f], w_packed[(int64_t)(h * C + c) * fe_pad + f], ee);
      }
      acc[c] = acc[c] * corr + pv * (to_float(vp[c]) + ee);
    }
    m = m_new;
  }
  const float inv = (end > beg) ? 1.0f / l : 0.f;
  for (int c = 0; c < C; ++c) {
    float o = acc[c] * inv;
    if (addend != nullptr) o += to_float(addend[(int64_t)d * ldadd + h * C + c]);
    out[(int64_t)d * ldo + h * C + c] = from_float<T>(o);
  }
  if (lse != nullptr) lse[(int64_t)d * H + h] = (end > beg) ? m + logf(l) : 0.f;
}

// W' = [W_e | b_e | 0] as fp32 [D][fe_pad]
template <typename T>
__global__ void pack_edge_weights_kernel(const T* __restrict__ w, const T* __restrict__ b, float* __restrict__ out, int D,
                                         int fe, int fe_pad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D * fe_pad) return;
  const int c = i / fe_pad, f = i % fe_pad;
  out[i] = f < fe ? to_float(w[(int64_t)c * fe + f]) : ((f == fe && b != nullptr) ? to_float(b[c]) : 0.f);
}

template <typename T>
__global__ void pack_edge_features_kernel(const T* __restrict__ ea, int64_t ld, float* __restrict__ out, int M, int fe,
                                          int fe_pad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)M * fe_pad) return;
  const int m = (int)(i / fe_pad), f = (int)(i % fe_pad);
  out[i] = f < fe ? to_float(ea[(int64_t)m * ld + f]) : (f == fe ? 1.0f : 0.0f);
}

// ---------------------------------------------------------------------------------------------- dispatch
struct AttnArgs {
  const void *q, *k, *v, *e;
  int64_t ldq, ldk, ldv, lde;
  const float* feat;
  int fe, fe_pad;
  const float* w_packed;
  const int32_t *row, *colptr;
  const int32_t* order = nullptr;
  const void* addend;
  int64_t ldadd;
  void* out;
  int64_t ldo;
  float* lse;
  int n_dst, n_src, H, C;
  hipStream_t stream;
  float drop_p = 0.f;      // attention dropout (materialised-E op only): probability and the seed of the replayable mask
  uint64_t drop_seed = 0;
};

// ANEMOI_ATTN_BLOCKS_PER_CU (workgroups per CU of the fused-edge forward, 0 / unset = the plan's rule) and ANEMOI_ATTN_OUT_WT
// (write-through output stores): read once per process
static int attn_blocks_per_cu() {
  static const int v = env_int(getenv("ANEMOI_ATTN_BLOCKS_PER_CU"), 0, 0, 32);
  return v;
}
static int attn_out_wt() {
  static const int v = env_int(getenv("ANEMOI_ATTN_OUT_WT"), 0, 0, 1);
  return v;
}

template <typename T>
static AttnPlan plan_of(const AttnArgs& a) {
  const int D = a.H * a.C;
  // the wave kernels move whole 16-byte vectors (gt_attention_plan.h: align_elems on why the forward's multiple is 8 for every dtype)
  const bool aligned = rows_aligned({{a.q, a.ldq}, {a.k, a.ldk}, {a.v, a.ldv}, {a.out, a.ldo}, {a.e, a.e ? a.lde : 0},
                                     {a.addend, a.addend ? a.ldadd : 0}, {a.feat, 0}, {a.w_packed, 0}},
                                    align_elems(AttnOp::Fwd, sizeof(T)));
  return plan_attention(a.feat ? AttnOp::FwdFusedEdge : AttnOp::Fwd, a.H, a.C, a.fe_pad, a.n_dst, a.n_src, aligned,
                        kv_rows_adjacent(a.k, a.v, a.ldk, a.ldv, D, a.n_src, sizeof(T)), attn_blocks_per_cu());
}

template <typename T>
static int launch(const AttnArgs& a) {
  const AttnPlan p = plan_of<T>(a);
  const float scale = 1.0f / sqrtf((float)a.C);
  // (the wave kernels are named first: the compiler emits kernels in the order the host code names them, and the hot kernels keep
  // their place in the code object that way)
  const dim3 grid(p.grid_dst), block(64 * kWavesPerBlock);
  if (p.route == AttnRoute::Wave)
    return with_lane_layout(p, [&](auto vec_c, auto lph_c) {
      constexpr int VEC = decltype(vec_c)::value, LPH = decltype(lph_c)::value;
      if (a.feat == nullptr) {
        auto kern = a.e != nullptr ? gt_attn_fwd_kernel<T, VEC, LPH, true> : gt_attn_fwd_kernel<T, VEC, LPH, false>;
        hipLaunchKernelGGL(kern, grid, block, 0, a.stream, (const T*)a.q, a.ldq, (const T*)a.k, a.ldk, (const T*)a.v, a.ldv,
                           (const T*)a.e, a.e != nullptr ? a.lde : (int64_t)0, a.row, a.colptr, (const T*)a.addend, a.ldadd, (T*)a.out,
                           a.ldo, a.lse, a.n_dst, a.H, scale, a.drop_p, a.drop_seed);
        return check_launch("gt_attn_fwd_kernel");
      }
      // fused lin_edge: a persistent grid (the plan's), the W' image in dynamic LDS
      return with_fe_pad(p, [&](auto fe_pad_c) {
        constexpr int FE_PAD = decltype(fe_pad_c)::value;
        auto kern = p.kv_adjacent ? gt_attn_fused_edge_fwd_kernel<T, VEC, LPH, FE_PAD, true> : gt_attn_fused_edge_fwd_kernel<T, VEC, LPH, FE_PAD, false>;
        hipLaunchKernelGGL(kern, grid, block, p.lds_bytes, a.stream, (const T*)a.q, a.ldq, (const T*)a.k, a.ldk, (const T*)a.v, a.ldv,
                           a.feat, a.w_packed, a.row, a.colptr, a.order, (const T*)a.addend, a.ldadd, (T*)a.out, a.ldo, a.lse, a.n_dst,
                           a.H, scale, attn_out_wt());
        return check_launch("gt_attn_fused_edge_fwd_kernel");
      });
    });
  if (p.route == AttnRoute::Unsupported) {
    set_error("gt_attention: channels per head C=%d not supported (fast path needs H*C %% 64 == 0 and a power-of-two "
              "C*64/(H*C) <= 16; generic path needs C <= %d)", a.C, kGenericMaxC);
    return ANEMOI_E_UNSUPPORTED;
  }
  hipLaunchKernelGGL((gt_attn_fwd_generic_kernel<T>), dim3(p.grid_dst), dim3(128), 0, a.stream, (const T*)a.q, a.ldq, (const T*)a.k, a.ldk,
                     (const T*)a.v, a.ldv, (const T*)a.e, a.lde, a.feat, a.fe, a.fe_pad, a.w_packed, a.row, a.colptr, (const T*)a.addend,
                     a.ldadd, (T*)a.out, a.ldo, a.lse, a.n_dst, a.H, a.C, scale, a.drop_p, a.drop_seed);
  return check_launch("gt_attn_fwd_generic_kernel");
}

static int dispatch(const AttnArgs& a, anemoi_dtype_t dtype) {
  return dispatch_dtype(dtype, [&](auto t) { return launch<typename decltype(t)::type>(a); });
}

}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_gt_attention_dropout_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                       const void* e, int64_t lde, const int32_t* row, const int32_t* colptr,
                                       const void* addend, int64_t ldadd, void* out, int64_t ldo, float* lse,
                                       int32_t n_dst, int32_t n_src, int32_t H, int32_t C, float drop_p, uint64_t drop_seed,
                                       anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "gt_attention_dropout_fwd: dropout probability %g outside [0, 1)", (double)drop_p);
  ANEMOI_REQUIRE(H < 65536, "gt_attention_dropout_fwd: the mask's counter holds 16 bits of head index, got H=%d", H);
  ANEMOI_REQUIRE(n_dst >= 0 && n_src >= 0 && H > 0 && C > 0, "gt_attention_dropout_fwd: bad sizes n_dst=%d n_src=%d H=%d C=%d", n_dst, n_src, H, C);
  if (n_dst == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(q && k && v && out && colptr, "gt_attention_dropout_fwd: null q/k/v/out/colptr");
  const int D = H * C;
  ANEMOI_REQUIRE(ldq >= D && ldk >= D && ldv >= D && ldo >= D && (!e || lde >= D) && (!addend || ldadd >= D),
                 "gt_attention_dropout_fwd: leading dimension smaller than H*C=%d", D);
  AttnArgs a{q, k, v, e, ldq, ldk, ldv, lde, nullptr, 0, 0, nullptr, row, colptr, nullptr, addend, ldadd, out, ldo, lse, n_dst, n_src, H, C, as_stream(stream)};
  a.drop_p = drop_p;
  a.drop_seed = drop_seed;
  return dispatch(a, dtype);
}

extern "C" int anemoi_gt_attention_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                       const void* e, int64_t lde, const int32_t* row, const int32_t* colptr,
                                       const void* addend, int64_t ldadd, void* out, int64_t ldo, float* lse,
                                       int32_t n_dst, int32_t n_src, int32_t H, int32_t C, anemoi_dtype_t dtype,
                                       void* stream) {
  return anemoi_gt_attention_dropout_fwd(q, ldq, k, ldk, v, ldv, e, lde, row, colptr, addend, ldadd, out, ldo, lse, n_dst, n_src, H, C, 0.f, 0,
                                         dtype, stream);
}

// keep-scale of every (edge, head) as the kernels derive it: what a caller (or a test) needs to restate the op with an explicit mask
__global__ void attn_dropout_mask_kernel(float* __restrict__ out, int64_t n, int H, float p, uint64_t seed) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = attn_dropout_scale(seed, (int)(i / H), (int)(i % H), p, 1.0f / (1.0f - p));
}

extern "C" int anemoi_attention_dropout_mask(float* out, int32_t n_edges, int32_t H, float drop_p, uint64_t drop_seed, void* stream) {
  ANEMOI_REQUIRE(n_edges >= 0 && H > 0 && H < 65536 && drop_p >= 0.f && drop_p < 1.f, "attention_dropout_mask: bad arguments M=%d H=%d p=%g", n_edges, H, (double)drop_p);
  const int64_t n = (int64_t)n_edges * H;
  if (n == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(out, "attention_dropout_mask: null output");
  hipLaunchKernelGGL(attn_dropout_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), out, n, H, drop_p, drop_seed);
  return check_launch("attn_dropout_mask_kernel");
}

extern "C" int anemoi_gt_attention_fused_edge_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                                  int64_t ldv, const float* edge_feat, int32_t fe_pad,
                                                  const float* w_packed, const int32_t* row, const int32_t* colptr,
                                                  const int32_t* dst_order, const void* addend, int64_t ldadd, void* out, int64_t ldo, float* lse,
                                                  int32_t n_dst, int32_t n_src, int32_t H, int32_t C,
                                                  anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_dst >= 0 && n_src >= 0 && H > 0 && C > 0, "gt_attention_fused_edge_fwd: bad sizes");
  if (n_dst == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(q && k && v && out && colptr && edge_feat && w_packed, "gt_attention_fused_edge_fwd: null pointer");
  ANEMOI_REQUIRE(fe_pad >= 4 && fe_pad % 4 == 0, "gt_attention_fused_edge_fwd: fe_pad must be a positive multiple of 4, got %d", fe_pad);
  const int D = H * C;
  ANEMOI_REQUIRE(ldq >= D && ldk >= D && ldv >= D && ldo >= D && (!addend || ldadd >= D), "gt_attention_fused_edge_fwd: leading dimension smaller than H*C=%d", D);
  AttnArgs a{q, k, v, nullptr, ldq, ldk, ldv, 0, edge_feat, fe_pad - 1, fe_pad, w_packed, row, colptr, dst_order, addend, ldadd, out, ldo, lse, n_dst, n_src, H, C, as_stream(stream)};
  return dispatch(a, dtype);
}

extern "C" int anemoi_pack_edge_weights(const void* w_edge, const void* b_edge, float* out, int32_t D, int32_t fe,
                                        int32_t fe_pad, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(D > 0 && fe > 0 && fe_pad == 4 * ((fe + 1 + 3) / 4), "pack_edge_weights: bad sizes D=%d fe=%d fe_pad=%d", D, fe, fe_pad);
  ANEMOI_REQUIRE(w_edge && out, "pack_edge_weights: null pointer");
  const int n = D * fe_pad;
  const dim3 grid((n + 255) / 256), block(256);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((pack_edge_weights_kernel<T>), grid, block, 0, as_stream(stream), (const T*)w_edge, (const T*)b_edge, out, D, fe, fe_pad);
    return check_launch("pack_edge_weights_kernel");
  });
}

extern "C" int anemoi_pack_edge_features(const void* edge_attr, int64_t ld, float* out, int32_t M, int32_t fe,
                                         int32_t fe_pad, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(M >= 0 && fe > 0 && fe_pad == 4 * ((fe + 1 + 3) / 4) && ld >= fe, "pack_edge_features: bad sizes M=%d fe=%d fe_pad=%d", M, fe, fe_pad);
  if (M == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(edge_attr && out, "pack_edge_features: null pointer");
  const int64_t n = (int64_t)M * fe_pad;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((pack_edge_features_kernel<T>), grid, block, 0, as_stream(stream), (const T*)edge_attr, ld, out, M, fe, fe_pad);
    return check_launch("pack_edge_features_kernel");
  });
}

extern "C" int anemoi_gt_attention_plan(int32_t op, int32_t H, int32_t C, int32_t fe_pad, int32_t n_dst, int32_t n_src, int32_t rows_aligned,
                                        int32_t kv_adjacent, anemoi_dtype_t dtype, anemoi_gt_attention_plan_t* out) {
  ANEMOI_REQUIRE(out != nullptr, "gt_attention_plan: null out");
  ANEMOI_REQUIRE(op >= (int)AttnOp::Fwd && op <= (int)AttnOp::BwdFusedEdge, "gt_attention_plan: unknown op %d", op);
  ANEMOI_REQUIRE(dtype == ANEMOI_F32 || dtype == ANEMOI_BF16 || dtype == ANEMOI_F16, "gt_attention_plan: unknown dtype %d", (int)dtype);
  ANEMOI_REQUIRE(n_dst >= 0 && n_src >= 0 && H > 0 && C > 0, "gt_attention_plan: bad sizes n_dst=%d n_src=%d H=%d C=%d", n_dst, n_src, H, C);
  const bool fused = op == (int)AttnOp::FwdFusedEdge || op == (int)AttnOp::BwdFusedEdge;
  ANEMOI_REQUIRE(!fused || (fe_pad >= 4 && fe_pad % 4 == 0), "gt_attention_plan: fe_pad must be a positive multiple of 4, got %d", fe_pad);
  const AttnPlan p = plan_attention((AttnOp)op, H, C, fe_pad, n_dst, n_src, rows_aligned != 0, kv_adjacent != 0, attn_blocks_per_cu());
  *out = {(int32_t)p.route, p.vec, p.lph, p.fe_pad, p.kv_adjacent, p.lds_bytes, p.grid_dst, p.grid_src, p.grid_wgrad};
  if (p.route == AttnRoute::Unsupported) {
    set_error("gt_attention_plan: the entry point of op %d does not take H=%d C=%d fe_pad=%d%s", op, H, C, fe_pad, rows_aligned ? "" : " on unaligned rows");
    return ANEMOI_E_UNSUPPORTED;
  }
  return ANEMOI_OK;
}
