// Fused graph-transformer edge attention (forward) for gfx950.
//
// Spec: the reference's _gt_fwd Triton kernel (models/src/anemoi/models/triton/gt.py:81-179) and
// GraphTransformerConv (models/src/anemoi/models/layers/conv.py:84-147).  Not a port: the Triton kernel
// runs one program per destination with [H,C] register tiles; here one 64-lane wavefront owns one
// destination row of D = H*C channels, each lane holds VEC = D/64 contiguous channels (a 16-byte load
// for bf16 at D=512), a head spans LPH = C/VEC adjacent lanes and the per-head <q,k> dot is finished
// with a DPP butterfly inside the row.  Online softmax state (m, l) and the accumulator stay in fp32
// registers; the edge loop is software-pipelined one edge ahead.
//
// EDGE_FUSED variant: E = edge_attr @ W_e^T + b_e is never formed.  Using linearity,
//   <q_h, k_h + W_h a + b_h>       = <q_h,k_h> + sum_f a_f <q_h, W_h[:,f]> + <q_h,b_h>
//   sum_e p_e (v_h + W_h a_e + b_h) = sum_e p_e v_h + W_h (sum_e p_e a_e) + b_h sum_e p_e
// so per destination we build qw[h][f] once (W' = [W_e | b_e] staged in LDS), per edge we only touch the
// fe_pad fp32 edge features (wave-uniform -> scalar loads) and at the end apply W' to the weighted feature
// sum.  HBM traffic per layer drops from 2(4ND + MD) to 2*4ND + 4*M*fe_pad bytes.
//
// This file: the fused-edge forward kernel.  In front of it gt_attention_core.h (build-time knobs, the packed dot product), behind
// it gt_attention_fwd_host.h (the materialised-E, generic and pack kernels, the launches, the C entry points); which kernel a call
// runs is decided by plan_attention (gt_attention_plan.h).  csrc/experiments/gt_attention_r05_variants.hip is built the same way
// around its own kernel.
#include "gt_attention_core.h"

namespace anemoi {

// Where a destination's loads are requested (profiles/r05_attention_header_ab.txt, same-box A/Bs): the source ids travel WITH the q slice,
// ahead of the qw set-up (-6 % of the launch), and the scalar part of the next header (id, edge range) one destination ahead.  The
// round-5 variants that were measured slower or equal - first header beside the W' staging, first ring fill ahead of the qw set-up,
// next header behind the edge loop, the lane split of the feature terms, the timing-only ablation builds - live in
// csrc/experiments/gt_attention_r05_variants.hip (tools/build_alt.sh builds them into an alternative library for same-box A/Bs).
constexpr int kAttnPF = 3;  // edges of K|V rows in flight per wave (modulo-unrolled ring, counted waits)

// ---------------------------------------------------------------------------------------------- fused lin_edge
// (the LDS image of W' = [W_e | b_e | 0] is WLayout of gt_attention_plan.h)
template <typename T, int VEC, int LPH, int FE_PAD, bool KVADJ>
__global__ __launch_bounds__(64 * kWavesPerBlock, ANEMOI_ATTN_MIN_WAVES) void gt_attn_fused_edge_fwd_kernel(
    const T* __restrict__ q, int64_t ldq, const T* __restrict__ k, int64_t ldk, const T* __restrict__ v, int64_t ldv,
    const float* __restrict__ feat, const float* __restrict__ w_packed, const int32_t* __restrict__ row,
    const int32_t* __restrict__ colptr, const int32_t* __restrict__ order, const T* __restrict__ addend, int64_t ldadd,
    T* __restrict__ out, int64_t ldo, float* __restrict__ lse, int n_dst, int H, float scale, int out_wt) {
  using L = WLayout<VEC, FE_PAD>;
  extern __shared__ __attribute__((aligned(16))) float w_lds[];  // [64][kChunk]
  const int lane = threadIdx.x & 63;
  const int c0 = lane * VEC;

  // XCD-aware persistent schedule.  Workgroup b runs on XCD b % 8 (observed dispatch order; only speed depends on
  // it).  Each XCD gets one CONTIGUOUS slice of the destination range, so the K/V rows its waves gather (the mesh
  // neighbourhood of that slice: nodes are latitude/longitude sorted) stay resident in that XCD's 4 MiB L2 instead of
  // every L2 pulling every row from the fabric (8x the traffic).  Inside a slice, waves take destinations round-robin.
  const int xcd = blockIdx.x & 7;
  const int blocks_in_xcd = (gridDim.x - xcd + 7) >> 3;
  const int waves_in_xcd = blocks_in_xcd * kWavesPerBlock;
  const int wave_in_xcd = __builtin_amdgcn_readfirstlane((blockIdx.x >> 3) * kWavesPerBlock + (threadIdx.x >> 6));
  const int per_xcd = (n_dst + 7) >> 3;
  const int d_lo = xcd * per_xcd;
  const int d_hi = min(n_dst, d_lo + per_xcd);

  using Raw = Vec<T, VEC>;  // a row slice as loaded (converted to fp32 only when consumed)
  // The header of a destination: its id and edge range (scalar registers, requested ONE DESTINATION AHEAD - the first one's in front of
  // the W' staging - so that a destination starts with its q slice and source ids, not with colptr), its q row slice and the source
  // ids of its first 64 in-edges.
  const int i0 = d_lo + wave_in_xcd;
  int h_d = 0, h_beg = 0, h_end = 0, h_src = 0;
  Raw h_q;
  auto load_scalars = [&](int i, int& d, int& beg, int& end) {
    d = order ? __builtin_amdgcn_readfirstlane(order[i]) : i;
    beg = __builtin_amdgcn_readfirstlane(colptr[d]);
    end = __builtin_amdgcn_readfirstlane(colptr[d + 1]);
  };
  int n_d = 0, n_beg = 0, n_end = 0;
  if (i0 < d_hi) load_scalars(i0, n_d, n_beg, n_end);
  // Stage W' = [W_e | b_e | 0] (fp32 [D][FE_PAD], packed once on the host side of the ABI) into LDS: all 16-byte
  // loads are issued before the first write (one memory round trip per workgroup).
  {
    constexpr int kQ = FE_PAD / 4;                 // float4 per channel row
    constexpr int kTotal = 64 * VEC * kQ;          // float4 in the image
    constexpr int kIter = (kTotal + 64 * kWavesPerBlock - 1) / (64 * kWavesPerBlock);
    float4 tmp[kIter];
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
      const int idx = threadIdx.x + it * 64 * kWavesPerBlock;
      tmp[it] = idx < kTotal ? reinterpret_cast<const float4*>(w_packed)[idx] : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
      const int idx = threadIdx.x + it * 64 * kWavesPerBlock;
      if (idx < kTotal) {
        const int c = idx / kQ, qq = idx % kQ;  // channel c, features 4 qq .. 4 qq + 3 -> chunk layout [feature][channel]
        float* dst = w_lds + (c / VEC) * L::kChunk + (qq * 4) * VEC + (c % VEC);
        dst[0] = tmp[it].x;
        dst[VEC] = tmp[it].y;
        dst[2 * VEC] = tmp[it].z;
        dst[3 * VEC] = tmp[it].w;
      }
    }
  }
  __syncthreads();
  const float* wl = w_lds + lane * L::kChunk;

  const float sl2e = scale * 1.4426950408889634f;  // p = 2^((s' - m') * scale * log2 e)
  const float thr = kDeferThr / scale;
  constexpr int PF = kAttnPF;

  // `order` (optional): the destination processed at position i.  The ~768 destinations an XCD works on at one moment are
  // then a compact patch of the mesh instead of a whole latitude ring, so the K|V rows they gather fit that XCD's L2
  // (layers/graphcache.py builds it from the graph; outputs are written at their own rows, the result does not depend on it).
  for (int i = i0; i < d_hi; i += waves_in_xcd) {
    // W' lives in LDS and is re-read per destination: without this barrier the compiler hoists all VEC*FE_PAD values
    // into registers across the loop (256 VGPRs, 1 wave/SIMD) and the kernel becomes latency-bound.
    asm volatile("" ::: "memory");
    h_d = n_d, h_beg = n_beg, h_end = n_end;
    h_q = *reinterpret_cast<const Raw*>(q + (int64_t)h_d * ldq + c0);
    h_src = (lane < h_end - h_beg) ? row[h_beg + lane] : 0;
    if (i + waves_in_xcd < d_hi) load_scalars(i + waves_in_xcd, n_d, n_beg, n_end);
    const int d = h_d, beg = h_beg, end = h_end;
    const Raw q_raw = h_q;
    float qv[VEC], acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      qv[j] = to_float(q_raw.v[j]);
      acc[j] = 0.f;
    }
    // Scores are kept in units of 1/scale (s' = <q, k + e>, the softmax argument is scale * s'): the scale rides in the
    // exponent's multiplier (one multiply per edge less).
    // Edge loop in chunks of 64: the source ids of a chunk are fetched with ONE coalesced load (lane j holds
    // row[chunk + j]) and broadcast with v_readlane, so row loads never wait on a dependent scalar load.
    int chunk = beg, n = min(64, end - beg), my_src = h_src;  // the first chunk's ids came with the header
    Raw kb[PF], vb[PF];
    float fb[PF][FE_PAD];
    auto fetch = [&](int j, Raw& kr, Raw& vr, float (&fr)[FE_PAD]) {
      j = min(j, n - 1);  // refills past the end re-read the last edge: an UNCONDITIONAL load keeps the ring registers
                          // free of select/copy code (a conditional one made the compiler wait for the load at once)
      const int s = __builtin_amdgcn_readlane(my_src, j);
      const float* a = feat + (int64_t)(chunk + j) * FE_PAD;  // wave-uniform address -> scalar loads
      if constexpr (KVADJ) {
        // v = the D columns after k in the same buffer (the fused projection's layout): ONE address and an immediate
        // offset; the row offset in 32 bits (checked at launch) - 13 scalar instructions fewer per edge, and this
        // kernel is bound by instruction issue
        const T* kp = k + (uint32_t)((uint32_t)s * (uint32_t)ldk) + c0;
        kr = *reinterpret_cast<const Raw*>(kp);
        vr = *reinterpret_cast<const Raw*>(kp + 64 * VEC);
      } else {
        kr = *reinterpret_cast<const Raw*>(k + (int64_t)s * ldk + c0);
        vr = *reinterpret_cast<const Raw*>(v + (int64_t)s * ldv + c0);
      }
#pragma unroll
      for (int f = 0; f < FE_PAD; ++f) fr[f] = a[f];
    };
    // qw[f] = (1/LPH) * sum over the head's channels of q[c] * W'[c][f]  (pre-divided: every lane of the
    // head adds the same edge-feature term before the head butterfly).
    float qw[FE_PAD], sf[FE_PAD];
#pragma unroll
    for (int f = 0; f < FE_PAD; ++f) {
      // W' is stored [feature][channel] per lane: the VEC channels of a feature are contiguous (16-byte LDS reads) and
      // the channel pairs map onto packed FMAs without shuffles, here and in the final W' * sum(p a)
      float t = 0.f;
      if constexpr (VEC % 2 == 0) {
        f32x2 t2 = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < VEC; j += 2)
          t2 = __builtin_elementwise_fma(f32x2{qv[j], qv[j + 1]}, *reinterpret_cast<const f32x2*>(wl + f * VEC + j), t2);
        t = t2[0] + t2[1];
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) t = fmaf(qv[j], wl[f * VEC + j], t);
      }
      qw[f] = group_sum<LPH>(t) * (1.0f / LPH);
      sf[f] = 0.f;
    }
    float m = -INFINITY, l = 0.f;

    for (; chunk < end; chunk += 64) {
      if (chunk != beg) {
        n = min(64, end - chunk);
        my_src = (lane < n) ? row[chunk + lane] : 0;
      }
#pragma unroll
      for (int st = 0; st < PF; ++st) fetch(st, kb[st], vb[st], fb[st]);
      // Edges in GROUPS of PF inside ONE basic block: the ring slots always hold loaded rows (refills past the end re-read the last edge), an edge
      // beyond the chunk gets the score -inf (weight 0).  The group's scores are formed first, the running max is checked ONCE per group, and
      // the scheduler can interleave the PF independent dependency chains (the per-edge form below is one basic block per edge: dependent
      // packed FMAs back to back, a wait state each, and a scalar bound check + two branches per edge).  The hidden mesh's in-degrees are
      // multiples of 6 and the decoder's exactly 3: no padded edge there.  Same-box A/B against the per-edge loop (round 5's, in
      // csrc/experiments/gt_attention_r05_variants.hip): O96 -0.2 %, res 6 -0.2 %, N320 -0.6 % per forward; 88 instead of 94 VGPRs; per edge 60 instead of
      // 68 issue slots (2 s_nop instead of 8, 0.7 branches instead of 3) - profiles/r06_attention_grouped_ab.txt.
      for (int j0 = 0; j0 < n; j0 += PF) {
        float dots[PF];
#pragma unroll
        for (int st = 0; st < PF; ++st) {
          float dot = dot_rows<T, VEC>(q_raw, kb[st]);
          if constexpr (FE_PAD % 2 == 0) {
            f32x2 d2[2] = {{dot, 0.f}, {0.f, 0.f}};
#pragma unroll
            for (int f = 0; f < FE_PAD; f += 2)
              d2[(f / 2) & 1] = __builtin_elementwise_fma(f32x2{fb[st][f], fb[st][f + 1]}, f32x2{qw[f], qw[f + 1]}, d2[(f / 2) & 1]);
            d2[0] += d2[1];
            dot = d2[0][0] + d2[0][1];
          } else {
#pragma unroll
            for (int f = 0; f < FE_PAD; ++f) dot = fmaf(fb[st][f], qw[f], dot);
          }
          dot = group_sum<LPH>(dot);
          dots[st] = (j0 + st < n) ? dot : -INFINITY;  // (wave-uniform condition)
        }
        float mx = dots[0];
#pragma unroll
        for (int st = 1; st < PF; ++st) mx = fmaxf(mx, dots[st]);
        if (__builtin_amdgcn_ballot_w64(mx > m + thr) != 0) {  // always in the first group, rare afterwards
          const float m_new = fmaxf(m, mx);
          const float corr = __builtin_amdgcn_exp2f((m - m_new) * sl2e);  // 2^(-inf) = 0 in the first group
          l *= corr;
#pragma unroll
          for (int jj = 0; jj < VEC; ++jj) acc[jj] *= corr;
#pragma unroll
          for (int f = 0; f < FE_PAD; ++f) sf[f] *= corr;
          m = m_new;
        }
#pragma unroll
        for (int st = 0; st < PF; ++st) {
          const float p = __builtin_amdgcn_exp2f((dots[st] - m) * sl2e);  // 2^(-inf) = 0 for an edge beyond the chunk
          l += p;
#pragma unroll
          for (int jj = 0; jj < VEC; ++jj) acc[jj] = fmaf(p, to_float(vb[st].v[jj]), acc[jj]);
#pragma unroll
          for (int f = 0; f < FE_PAD; ++f) sf[f] = fmaf(p, fb[st][f], sf[f]);
          fetch(j0 + st + PF, kb[st], vb[st], fb[st]);
        }
      }
    }

    asm volatile("" ::: "memory");
    const float inv = (end > beg) ? 1.0f / l : 0.f;
    float o[VEC];
    if constexpr (VEC % 2 == 0) {
      f32x2 o2[VEC / 2];
#pragma unroll
      for (int j = 0; j < VEC; j += 2) o2[j / 2] = f32x2{acc[j], acc[j + 1]};
#pragma unroll
      for (int f = 0; f < FE_PAD; ++f) {
        const f32x2 s2 = {sf[f], sf[f]};
#pragma unroll
        for (int j = 0; j < VEC; j += 2) o2[j / 2] = __builtin_elementwise_fma(s2, *reinterpret_cast<const f32x2*>(wl + f * VEC + j), o2[j / 2]);
      }
#pragma unroll
      for (int j = 0; j < VEC; j += 2) {
        o[j] = o2[j / 2][0] * inv;
        o[j + 1] = o2[j / 2][1] * inv;
      }
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float t = acc[j];
#pragma unroll
        for (int f = 0; f < FE_PAD; ++f) t = fmaf(sf[f], wl[f * VEC + j], t);
        o[j] = t * inv;
      }
    }
    if (addend != nullptr) {
      float ad[VEC];
      load_vec<T, VEC>(addend + (int64_t)d * ldadd + c0, ad);
#pragma unroll
      for (int j = 0; j < VEC; ++j) o[j] += ad[j];
    }
    if constexpr (sizeof(T) * VEC == 16) {
      if (out_wt) {
        // write-through store (sc1): the output row is read by ANOTHER kernel, so keeping its line in this XCD's L2 only
        // evicts K|V rows that later destinations of the window still gather (ANEMOI_ATTN_OUT_WT, measured A/B in DESIGN.md)
        typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
        Vec<T, VEC> tmp;
#pragma unroll
        for (int j = 0; j < VEC; ++j) tmp.v[j] = from_float<T>(o[j]);
        T* dstp = out + (int64_t)d * ldo + c0;
        asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dstp), "v"(__builtin_bit_cast(u32x4, tmp)) : "memory");
      } else {
        store_vec<T, VEC>(out + (int64_t)d * ldo + c0, o);
      }
    } else {
      store_vec<T, VEC>(out + (int64_t)d * ldo + c0, o);
    }
    if (lse != nullptr && (lane % LPH) == 0) lse[(int64_t)d * H + lane / LPH] = (end > beg) ? m * scale + __logf(l) : 0.f;
  }
}

}  // namespace anemoi

#include "gt_attention_fwd_host.h"
