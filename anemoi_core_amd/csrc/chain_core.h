// Shared device code of the row-resident chain kernels (gt_chain2 / gt_cluster_chain / gt_rowchain.hip: GraphTransformer block tails and
// mapper sides; gnn_chain.hip: GraphConv edge / node MLPs).  A workgroup of 8 waves owns a panel of <= 48 rows x 512 channels in LDS
// (16-byte slots XOR-swizzled by the row); a wave owns a 64-column slab of each GEMM's output (or, role-split, a 128-column one:
// chain2_core.h) and streams its B fragments from a fragment-major weight image straight into a register ring (see
// experiments/gt_chain.hip for the measurements behind each choice).  Here: the 64-column GEMM segment, the panel layout, the lanes'
// coordinates in it, the LayerNorm statistics and the epilogue forms of both wave layouts.
#pragma once
#include "chain_host.h"
#include "mma.h"

namespace anemoi {

using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;

// four 16-bit values travel as two dwords (plain registers: a struct of four halves tempts the compiler into scratch)
template <typename T>
__device__ __forceinline__ void unpack4(u32x2 p, float (&o)[4]);
template <>
__device__ __forceinline__ void unpack4<bf16_t>(u32x2 p, float (&o)[4]) {
  o[0] = __uint_as_float(p[0] << 16);
  o[1] = __uint_as_float(p[0] & 0xffff0000u);
  o[2] = __uint_as_float(p[1] << 16);
  o[3] = __uint_as_float(p[1] & 0xffff0000u);
}
template <>
__device__ __forceinline__ void unpack4<f16_t>(u32x2 p, float (&o)[4]) {
  // (element-wise through 16-bit integers: with a bit_cast of each dword to a 2-vector of halves hipcc 7.2 dropped the second
  // dword and converted the first one twice - found by the f16 parity tests)
  const unsigned lo = p[0], hi = p[1];
  o[0] = (float)__builtin_bit_cast(_Float16, (unsigned short)(lo & 0xffffu));
  o[1] = (float)__builtin_bit_cast(_Float16, (unsigned short)(lo >> 16));
  o[2] = (float)__builtin_bit_cast(_Float16, (unsigned short)(hi & 0xffffu));
  o[3] = (float)__builtin_bit_cast(_Float16, (unsigned short)(hi >> 16));
}
template <typename T>
__device__ __forceinline__ u32x2 pack4(const float (&v)[4]) {
  const T a = from_float<T>(v[0]), b = from_float<T>(v[1]), c = from_float<T>(v[2]), d = from_float<T>(v[3]);
  return u32x2{(unsigned)__builtin_bit_cast(unsigned short, a) | ((unsigned)__builtin_bit_cast(unsigned short, b) << 16),
               (unsigned)__builtin_bit_cast(unsigned short, c) | ((unsigned)__builtin_bit_cast(unsigned short, d) << 16)};
}
// (halves: two conversions + one v_pack_b32_f16 per dword instead of a shift and an or - with 96 values per lane in an epilogue the
// longer form made the role-split chain's f16 instantiation spill)
template <>
__device__ __forceinline__ u32x2 pack4<f16_t>(const float (&v)[4]) {
  using h2 = __attribute__((ext_vector_type(2))) _Float16;
  const h2 lo = {(_Float16)v[0], (_Float16)v[1]}, hi = {(_Float16)v[2], (_Float16)v[3]};
  return u32x2{__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
}
// this lane's 4 values of each of the wave's 4 column blocks of a parameter vector (bias, gamma, beta), loaded EARLY - before
// the GEMM whose epilogue uses them: vmcnt retires in order, so a load issued behind the weight ring's prefetches could only be
// waited for together with them (a full L2 latency exposed at every epilogue)
template <typename T>
__device__ __forceinline__ void load_cols(const T* __restrict__ p, int wave, int g, u32x2 (&o)[4]) {
  asm volatile("" : "+v"(g));  // (else the per-lane address is hoisted to the kernel's entry and spilled around the GEMM segments)
#pragma unroll
  for (int ni = 0; ni < 4; ++ni) o[ni] = *reinterpret_cast<const u32x2*>(p + wave * 64 + ni * 16 + g * 4);
}

// kCh, kPanel and the LDS map of every kernel of the family (three panel buffers | [48 rows][waves][2] fp32 LayerNorm partials | the per-column
// vectors: kRowBytes, kBufBytes, kRedOff, vec_off, kChainSmem) are chain_plan.h's: the launch plan prices the same layout
constexpr int kSlab = 16 * 4096;            // one segment of a wave's weight stream: 16 K-steps x (4 fragments x 1 KiB)
constexpr int kTlOff = kChainSmem;          // instrumented instantiation only: [8 waves][kTlSlots] stamps, copied out at the end

// a pointer the compiler must keep in scalar registers (it is wave-uniform by construction): the loads then take the
// "SGPR base + 32-bit VGPR offset + immediate" form instead of a 64-bit VGPR address per fragment group
typedef const __attribute__((address_space(1))) char* gptr_t;  // a GLOBAL pointer: an integer round trip must not degrade the loads to flat_load
__device__ __forceinline__ gptr_t uniform_ptr(const char* p) {
  const uint64_t v = reinterpret_cast<uint64_t>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return reinterpret_cast<gptr_t>(((uint64_t)hi << 32) | lo);
}
typedef const __attribute__((address_space(1))) frag8* gfrag_t;

// 16 K-steps (K = 512) of this wave's 48 x 64 tile: A fragments from the swizzled LDS panel, B fragments from the register
// ring (filled 4 K-steps ago), the ring slot refilled right behind its MFMAs with the fragments of 4 K-steps ahead - of this
// segment or, in its last group, of the NEXT segment (`nxt`), so the stream never drains across the epilogues.
// sched_barrier pins the issue order: left alone the scheduler sinks all 16 loads to the end of the loop body and the
// waitcnt pass then drains the queue at the top (measured with tools/weight_stream_probe.hip).
struct NoHook {
  __device__ __forceinline__ void operator()(int) const {}
};
template <typename T, int NB = 3, typename Hook = NoHook>
__device__ __forceinline__ void gemm_seg(const unsigned char* abuf, int lane, frag8 (&bq)[4][4], const char* cur, const char* nxt,
                                         uint32_t loff, f32x4 (&acc)[NB][4], Hook hook = Hook(), int nq = 4, int flip = -1) {  // cur / nxt: wave-uniform (SGPR) bases, loff = lane * 16
  // flip >= 0 (experiment): the wave raises its issue priority in every other group of 4 K-steps - flip = 0 / 1 for the two waves of a SIMD
  // nq: groups of 4 K-steps (K = 128 nq; 4 = the 512-wide segment every caller but the MLP chain's first GEMM uses)
  asm volatile("" : "+v"(lane));
  const int x = lane & 15, ks = lane >> 4;
  const unsigned char* arow = abuf + x * kRowBytes;
  // the A fragments of K-step st+1 are requested BEFORE the MFMAs of step st (12 more registers): with one set of fragment
  // registers every step exposed three LDS round trips in front of its MFMAs (a third of a segment's time, in-kernel timeline)
  frag8 fa[NB];
#pragma unroll
  for (int mi = 0; mi < NB; ++mi) fa[mi] = *reinterpret_cast<const frag8*>(arow + mi * 16 * kRowBytes + ((ks ^ x) << 4));
  const int last = nq * 4 - 1;
#pragma unroll 1
  for (int q = 0; q < nq; ++q) {
    const char* pfg = q < nq - 1 ? cur + (q + 1) * 16384 : nxt;
    hook(q);  // side traffic of the caller, a quarter of it per group of 4 K-steps (the edge chain's next panel)
    if (flip >= 0) {
      if ((q + flip) & 1) __builtin_amdgcn_s_setprio(1);
      else __builtin_amdgcn_s_setprio(0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int st = q * 4 + j;
      const int sn = st < last ? st + 1 : last;  // (the last step re-reads its own fragments: no branch in the stream)
      frag8 fn[NB];
#pragma unroll
      for (int mi = 0; mi < NB; ++mi) fn[mi] = *reinterpret_cast<const frag8*>(arow + mi * 16 * kRowBytes + (((sn * 4 + ks) ^ x) << 4));
      __builtin_amdgcn_sched_barrier(0);  // (else the scheduler sinks these reads behind the MFMAs, into the registers they free)
#pragma unroll
      for (int mi = 0; mi < NB; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = mfma16<T>(bq[j][ni], fa[mi], acc[mi][ni]);  // D^T: lane = row x, 4 consecutive columns
      {
        const gptr_t pj = uniform_ptr(pfg + j * 4096);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) bq[j][ni] = *reinterpret_cast<gfrag_t>(pj + loff + ni * 1024);
      }
#pragma unroll
      for (int mi = 0; mi < NB; ++mi) fa[mi] = fn[mi];
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (flip >= 0) __builtin_amdgcn_s_setprio(0);
}

__device__ __forceinline__ void lds_barrier() {  // LDS writes of all waves visible; global loads in flight (the weight ring) stay in flight
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---------------------------------------------------------------------------------------------------------------- the panel and its epilogues
// One layout serves every kernel of the family: row r, 16-byte slot s of a panel buffer sits at panel_off(r, s).  Two wave layouts work on
// it, told apart by NI, the 16-column blocks a wave owns of each GEMM's output: NI = 4 (eight waves x 64 columns, acc[mi][0..3]) and
// NI = 8 (four waves x 128 columns, acc[mi][0..7]).  In both, lane = row mi*16 + x, 4 consecutive columns w*16*NI + ni*16 + g*4 + r.
__device__ __forceinline__ int panel_off(int row, int slot16) { return row * kRowBytes + ((slot16 ^ (row & 15)) << 4); }
// (the address itself, summed left to right: the row term joins the buffer's wave-uniform base and the swizzled slot stays the only
// per-lane term, where `buf + panel_off(..)` would carry the row into every lane's offset)
template <typename B>
__device__ __forceinline__ B* panel_at(B* buf, int row, int slot16) { return buf + row * kRowBytes + ((slot16 ^ (row & 15)) << 4); }
template <int NI>
constexpr int kWaves = kCh / (16 * NI);  // waves that share a row (= partials per row)

// Row streams (panel rows in, output rows out) are touched once per launch.  ANEMOI_CHAIN2_NT (build-time mask): 1 = the loads carry the
// non-temporal hint, so that in the XCD's L2 they do not push out the WEIGHTS, which all 32 CUs of the XCD read - and, in multi-round
// launches, read again (res 6 forward -2.4 %); 2 = the stores too (O96 +1.7 %: the attention launch behind reads them - off); 4 = the
// stores write through (sc1) instead of sitting dirty in this XCD's L2 until the end of the kernel (O96 -0.4 % on one box, 0 on the next).
// Default 1.
#ifndef ANEMOI_CHAIN2_NT
#define ANEMOI_CHAIN2_NT 1
#endif
__device__ __forceinline__ u32x4 stream_load(const u32x4* p) {
  if constexpr ((ANEMOI_CHAIN2_NT & 1) != 0) return __builtin_nontemporal_load(p);
  else return *p;
}
__device__ __forceinline__ void stream_store(u32x4 v, u32x4* p) {
  if constexpr ((ANEMOI_CHAIN2_NT & 2) != 0) __builtin_nontemporal_store(v, p);
  else if constexpr ((ANEMOI_CHAIN2_NT & 4) != 0) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");  // write-through
  else *p = v;
}

// Per-lane coordinates, re-derived from an OPAQUE copy of the lane id at the start of every phase: the epilogues' address
// arithmetic (a few dozen registers of LDS / global offsets per phase) is invariant over the panel loop, LICM hoists all of it
// to the kernel's entry, and the allocator then spills it around the GEMM segments (scratch reloads retire in order behind the
// weight ring: every reload would drain it).  Behind the barrier the values are computed where they are used.
// (The 128-column layout pins the wave index too, the 64-column one the lane only: each as its kernels were tuned.)
template <int NI>
struct LaneCols {
  int x, g;
  int coff[NI];  // LDS byte offset (inside a panel row) of this lane's 4 columns of column block ni: slot = w*2*NI + ni*2 + (g>>1), swizzled by the row
};
template <int NI>
__device__ __forceinline__ LaneCols<NI> lane_cols(int lane, int w) {
  if constexpr (NI == 8) asm volatile("" : "+v"(lane), "+s"(w));
  else asm volatile("" : "+v"(lane));
  LaneCols<NI> c;
  c.x = lane & 15;
  c.g = lane >> 4;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) c.coff[ni] = (((w * 2 * NI + ni * 2 + (c.g >> 1)) ^ c.x) << 4) + (c.g & 1) * 8;
  return c;
}

template <typename T, int NB = 3>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[NB][4]) {
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// LayerNorm statistics are the plain fp32 statistics of the ROUNDED 16-bit rows, in two steps with no E[x^2] - mean^2 cancellation:
// row_partial: (mean, M2) of one row over this wave's 16 NI columns, from the lane's values a[0..NI-1] (fp32 images of the rounded values);
// every lane of the wave takes part (shuffles), the lanes with g == 0 then store the row's partial as red[row][w] (kWaves<NI> per row);
template <int NI>
__device__ __forceinline__ float2 row_partial(const f32x4* a) {
  float s = 0.f;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) s += (a[ni][0] + a[ni][1]) + (a[ni][2] + a[ni][3]);
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  const float mw = s * (1.0f / (float)(16 * NI));
  float q = 0.f;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float d = a[ni][r] - mw;
      q = fmaf(d, d, q);
    }
  q += __shfl_xor(q, 16, 64);
  q += __shfl_xor(q, 32, 64);
  return make_float2(mw, q);
}
// merge_partials: the W waves' partials of a row merged in wave order (Chan et al.): M2 = sum M2_w + n_w sum (mean_w - mean)^2
template <int W>
__device__ __forceinline__ void merge_partials(const float* red, int row, float eps, float& mu, float& rstd) {
  static_assert(W == 4 || W == 8, "four 128-column or eight 64-column partials per row");
  const f32x4* pr = reinterpret_cast<const f32x4*>(red + row * (2 * W));
  float m2;
  if constexpr (W == 8) {
    const f32x4 p0 = pr[0], p1 = pr[1], p2 = pr[2], p3 = pr[3];
    mu = (((p0[0] + p0[2]) + (p1[0] + p1[2])) + ((p2[0] + p2[2]) + (p3[0] + p3[2]))) * 0.125f;
    m2 = ((p0[1] + p0[3]) + (p1[1] + p1[3])) + ((p2[1] + p2[3]) + (p3[1] + p3[3]));
    const float d0 = p0[0] - mu, d1 = p0[2] - mu, d2 = p1[0] - mu, d3 = p1[2] - mu;
    const float d4 = p2[0] - mu, d5 = p2[2] - mu, d6 = p3[0] - mu, d7 = p3[2] - mu;
    m2 = fmaf(64.0f, ((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) + ((d4 * d4 + d5 * d5) + (d6 * d6 + d7 * d7)), m2);
  } else {
    const f32x4 p0 = pr[0], p1 = pr[1];
    mu = ((p0[0] + p0[2]) + (p1[0] + p1[2])) * 0.25f;
    const float d0 = p0[0] - mu, d1 = p0[2] - mu, d2 = p1[0] - mu, d3 = p1[2] - mu;
    m2 = fmaf(128.0f, (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3), (p0[1] + p0[3]) + (p1[1] + p1[3]));
  }
  rstd = rsqrtf(m2 * (1.0f / (float)kCh) + eps);
}

// Row statistics of the panel rows held as v[mi][ni][r] (64-column layout).  ONE barrier inside; `red` may be reused after the NEXT
// barrier of the caller.
template <typename T, int NB = 3>
__device__ __forceinline__ void panel_row_stats(const f32x4 (&v)[NB][4], float eps, float* red, int wave, int x, int g, float (&mean)[NB], float (&rstd)[NB]) {
#pragma unroll
  for (int mi = 0; mi < NB; ++mi) {
    const float2 p = row_partial<4>(v[mi]);
    if (g == 0) *reinterpret_cast<float2*>(red + ((mi * 16 + x) * 8 + wave) * 2) = p;
  }
  lds_barrier();
#pragma unroll
  for (int mi = 0; mi < NB; ++mi) merge_partials<8>(red, mi * 16 + x, eps, mean[mi], rstd[mi]);
}

// LayerNorm of the panel rows held as v[mi][ni][r] and store of the normalised rows (model dtype) into the LDS panel `dst`.  gm / bt:
// this lane's gamma / beta (packed, loaded before the GEMM).  One barrier inside (the partials), one after (the panel is complete).
template <typename T>
__device__ __forceinline__ void panel_layernorm(f32x4 (&v)[3][4], const u32x2 (&gm)[4], const u32x2 (&bt)[4], float eps, unsigned char* dst,
                                                float* red, int wave, int lane) {
  const LaneCols<4> lc = lane_cols<4>(lane, wave);
  float mean[3], rstd[3];
  panel_row_stats<T>(v, eps, red, wave, lc.x, lc.g, mean, rstd);
#pragma unroll
  for (int mi = 0; mi < 3; ++mi) {
    unsigned char* drow = dst + (mi * 16 + lc.x) * kRowBytes;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      float gv[4], bv[4], o[4];
      unpack4<T>(gm[ni], gv);
      unpack4<T>(bt[ni], bv);
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = fmaf((v[mi][ni][r] - mean[mi]) * rstd[mi], gv[r], bv[r]);
      *reinterpret_cast<u32x2*>(drow + lc.coff[ni]) = pack4<T>(o);
    }
  }
  lds_barrier();
}

// The wave's 48 x 64 output block (packed rows pk[mi][ni]: lane = row mi*16 + x, 4 columns) to global memory as whole 128-byte
// lines: through a wave-private LDS strip (row m, 16-byte slot s at m*128 + ((s ^ ((m >> 1) & 7)) << 4): conflict-free for the
// 8-byte writes in the MFMA layout and for the 16-byte row-major read-back), 6 stores of 16 bytes per lane.  `out` = address of
// (panel row 0, the wave's first column); the wave's own LDS operations are ordered: no barrier.
template <typename T, int NB = 3>
__device__ __forceinline__ void store_block_via_strip(const u32x2 (&pk)[NB][4], unsigned char* strip, T* out, int64_t ld, int nr, int lane, int wave) {
  const LaneCols<4> lc = lane_cols<4>(lane, wave);
#pragma unroll
  for (int mi = 0; mi < NB; ++mi) {
    const int m = mi * 16 + lc.x;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      *reinterpret_cast<u32x2*>(strip + m * 128 + (((ni * 2 + (lc.g >> 1)) ^ ((m >> 1) & 7)) << 4) + (lc.g & 1) * 8) = pk[mi][ni];
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const int rl = (lc.g << 1) | (lc.x >> 3), sl = lc.x & 7;  // lane >> 3, lane & 7
#pragma unroll
  for (int it = 0; it < 2 * NB; ++it) {
    const int m = it * 8 + rl;
    const u32x4 v = *reinterpret_cast<const u32x4*>(strip + m * 128 + ((sl ^ ((m >> 1) & 7)) << 4));
    if (m < nr) *reinterpret_cast<u32x4*>(out + (int64_t)m * ld + sl * 8) = v;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the strip may be rewritten
}

// ---- the phases of a panel in the 64-column layout (acc[mi][0..3], eight waves x 64 columns), named once: a kernel's panel loop is
// load, gemm_seg, one of these, barrier.  pb / pg / pt: this lane's packed columns of a bias / gamma / beta (load_cols, requested
// before the GEMM).  None of them holds a barrier, and only ring_head a scheduling fence: the order of a panel's phases stays in the
// kernels, next to the measurements behind it.  Each takes the lane's coordinates from lane_cols itself: the opaque lane id stays per phase.

// the weight ring's first fill: the 4 fragments of each of the first 4 K-steps of the stream at `w` (wave-uniform), pinned in issue order
__device__ __forceinline__ void ring_head(frag8 (&bq)[4][4], const char* w, uint32_t loff) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      bq[j][ni] = *reinterpret_cast<gfrag_t>(uniform_ptr(w + j * 4096) + loff + ni * 1024);
      __builtin_amdgcn_sched_barrier(0);
    }
}

// load_cols of the vector at p + col0, or zeros for a vector that is not there (a LayerNorm without bias, a projection without one)
template <typename T>
__device__ __forceinline__ void load_cols_or_zero(const void* p, int wave, int g, u32x2 (&o)[4], int col0 = 0) {
  if (p != nullptr) {
    load_cols<T>((const T*)p + col0, wave, g, o);
  } else {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) o[ni] = u32x2{0u, 0u};
  }
}

// One column block of a row band: acc + bias, GELU unless gelu is false, rounded to the model dtype
template <typename T>
__device__ __forceinline__ u32x2 bias_act4(const f32x4& v, u32x2 pb, bool gelu) {
  float bias[4], t[4];
  unpack4<T>(pb, bias);
#pragma unroll
  for (int r = 0; r < 4; ++r) t[r] = v[r] + bias[r];
  if (gelu) {
    gelu_fast2(t[0], t[1]);
    gelu_fast2(t[2], t[3]);
  }
  return pack4<T>(t);
}
// The wave's block through bias_act4 into the panel buffer `dst` (its own columns) ...
template <typename T, int NB>
__device__ __forceinline__ void bias_act_rows(const f32x4 (&acc)[NB][4], const u32x2 (&pb)[4], unsigned char* dst, int lane, int wave, bool gelu = true) {
  const LaneCols<4> lc = lane_cols<4>(lane, wave);
#pragma unroll
  for (int mi = 0; mi < NB; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) *reinterpret_cast<u32x2*>(dst + (mi * 16 + lc.x) * kRowBytes + lc.coff[ni]) = bias_act4<T>(acc[mi][ni], pb[ni], gelu);
}
// ... or into registers first (bias_act_pack) and from there into the buffer (put_rows): the form for a block that goes over the operand
// it was computed from, with the caller's barrier between the two - and, on its own, for a block on its way to store_block_via_strip
template <typename T, int NB>
__device__ __forceinline__ void bias_act_pack(const f32x4 (&acc)[NB][4], const u32x2 (&pb)[4], u32x2 (&pk)[NB][4], bool gelu) {
#pragma unroll
  for (int mi = 0; mi < NB; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) pk[mi][ni] = bias_act4<T>(acc[mi][ni], pb[ni], gelu);
}
template <typename T, int NB>
__device__ __forceinline__ void put_rows(const u32x2 (&pk)[NB][4], unsigned char* dst, int lane, int wave) {
  const LaneCols<4> lc = lane_cols<4>(lane, wave);
#pragma unroll
  for (int mi = 0; mi < NB; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) *reinterpret_cast<u32x2*>(dst + (mi * 16 + lc.x) * kRowBytes + lc.coff[ni]) = pk[mi][ni];
}
// acc <- the fp32 image of (acc + bias) rounded to the model dtype, as a Linear's output is: the input of panel_row_stats
template <typename T, int NB>
__device__ __forceinline__ void bias_round_rows(f32x4 (&acc)[NB][4], const u32x2 (&pb)[4]) {
#pragma unroll
  for (int mi = 0; mi < NB; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      float t[4];
      unpack4<T>(bias_act4<T>(acc[mi][ni], pb[ni], false), t);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[mi][ni][r] = t[r];
    }
}

// pk = LayerNorm(acc) + residual, rounded once: fma((acc - mean) rstd, gamma, beta) + res - the arithmetic of layernorm_fwd followed by
// the residual add, which is edge_ln_res_segsum's.  res(mi, ni): this lane's 4 packed residual values of row band mi, column block ni
// (from registers or from a panel in LDS).
template <typename T, int NB, typename Res>
__device__ __forceinline__ void layernorm_residual_pack(const f32x4 (&acc)[NB][4], const float (&mean)[NB], const float (&rstd)[NB], const u32x2 (&pg)[4],
                                                        const u32x2 (&pt)[4], Res res, u32x2 (&pk)[NB][4]) {
#pragma unroll
  for (int mi = 0; mi < NB; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      float gv[4], bv[4], rv[4], o[4];
      unpack4<T>(pg[ni], gv);
      unpack4<T>(pt[ni], bv);
      unpack4<T>(res(mi, ni), rv);
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = fmaf((acc[mi][ni][r] - mean[mi]) * rstd[mi], gv[r], bv[r]) + rv[r];
      pk[mi][ni] = pack4<T>(o);
    }
}

// ---- epilogues of a wave's 48 x 16 NI block held as acc[mi][0..NI-1] (wave w of kWaves<NI>), on the swizzled panel buffers

// acc[mi][ni] = vec[col0 + column] (+ the panel values at the lane's positions of `rows`): the accumulators of a GEMM start at its bias (+ residual)
template <typename T, int NI, bool ROWS>
__device__ __forceinline__ void init_acc(f32x4 (&acc)[3][8], const unsigned char* vec, int col0, const unsigned char* rows, int lane, int w) {
  const LaneCols<NI> lc = lane_cols<NI>(lane, w);
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    float b[4];
    unpack4<T>(*reinterpret_cast<const u32x2*>(vec + (col0 + w * (16 * NI) + ni * 16 + lc.g * 4) * 2), b);
#pragma unroll
    for (int mi = 0; mi < 3; ++mi) {
      if (ROWS) {
        float r[4];
        unpack4<T>(*reinterpret_cast<const u32x2*>(rows + (mi * 16 + lc.x) * kRowBytes + lc.coff[ni]), r);
        acc[mi][ni] = f32x4{b[0] + r[0], b[1] + r[1], b[2] + r[2], b[3] + r[3]};
      } else {
        acc[mi][ni] = f32x4{b[0], b[1], b[2], b[3]};
      }
    }
  }
}

// The wave's block rounded to the model dtype into the panel buffer `dst` (its own columns).
// ADD: first + vec[col0 + column] (Bias), or + vec[col0 + column] + the values `dst` holds at the same positions (BiasRows: a projection's
// bias and the skip rows; each lane rewrites the positions it read).
// STATS: acc keeps the ROUNDED values; per-wave (mean, M2) of every row over the wave's columns -> red[row][w].
// STORE = false: the rounded values stay in acc only (dst unused) - the pipelined row chain keeps a panel in registers across a barrier.
enum class Add { None, Bias, BiasRows };
template <typename T, int NI, Add ADD, bool STATS, bool STORE = true>
__device__ __forceinline__ void round_rows(f32x4 (&acc)[3][8], unsigned char* dst, float* red, int lane, int w, const unsigned char* vec = nullptr, int col0 = 0) {
  const LaneCols<NI> lc = lane_cols<NI>(lane, w);
  u32x2 rb[NI], rr[NI];
  if constexpr (ADD == Add::Bias) {  // (once, outside the row-band loop)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) rb[ni] = *reinterpret_cast<const u32x2*>(vec + (col0 + w * (16 * NI) + ni * 16 + lc.g * 4) * 2);
  }
#pragma unroll
  for (int mi = 0; mi < 3; ++mi) {
    unsigned char* drow = dst + (mi * 16 + lc.x) * kRowBytes;
    // (BiasRows: the reads of half a 128-column row band are requested together, pinned - the ring's next fragments are live here: all 48 reads
    // at once spill, one pair at a time exposes an LDS round trip twelve times)
    if constexpr (ADD == Add::BiasRows) {
#pragma unroll
      for (int h = 0; h < NI / 4; ++h) {
#pragma unroll
        for (int ni = 4 * h; ni < 4 * h + 4; ++ni) {
          rb[ni] = *reinterpret_cast<const u32x2*>(vec + (col0 + w * (16 * NI) + ni * 16 + lc.g * 4) * 2);
          rr[ni] = *reinterpret_cast<const u32x2*>(drow + lc.coff[ni]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float o[4] = {acc[mi][ni][0], acc[mi][ni][1], acc[mi][ni][2], acc[mi][ni][3]};
      if constexpr (ADD != Add::None) {
        float b[4];
        unpack4<T>(rb[ni], b);
        if constexpr (ADD == Add::BiasRows) {
          float r[4];
          unpack4<T>(rr[ni], r);
#pragma unroll
          for (int k = 0; k < 4; ++k) o[k] += b[k] + r[k];
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) o[k] += b[k];
        }
      }
      const u32x2 pk = pack4<T>(o);
      if constexpr (STORE) *reinterpret_cast<u32x2*>(drow + lc.coff[ni]) = pk;
      if (STATS) {
        unpack4<T>(pk, o);
        acc[mi][ni] = f32x4{o[0], o[1], o[2], o[3]};
      }
    }
    if (STATS) {
      const float2 p = row_partial<NI>(acc[mi]);
      if (lc.g == 0) *reinterpret_cast<float2*>(red + ((mi * 16 + lc.x) * kWaves<NI> + w) * 2) = p;
    }
  }
}

// GELU of the wave's block, rounded to the model dtype into the panel buffer `dst` (its own columns).  Column block by column block,
// pinned: left alone the scheduler interleaves all 48 polynomial chains and spills 32 registers around them.
template <typename T, int NI>
__device__ __forceinline__ void gelu_rows(const f32x4 (&acc)[3][8], unsigned char* dst, int lane, int w) {
  const LaneCols<NI> lc = lane_cols<NI>(lane, w);
#pragma unroll
  for (int mi = 0; mi < 3; ++mi) {
    unsigned char* drow = dst + (mi * 16 + lc.x) * kRowBytes;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float o[4] = {acc[mi][ni][0], acc[mi][ni][1], acc[mi][ni][2], acc[mi][ni][3]};
      gelu_fast2(o[0], o[1]);
      gelu_fast2(o[2], o[3]);
      *reinterpret_cast<u32x2*>(drow + lc.coff[ni]) = pack4<T>(o);
      if (ni & 1) __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// LayerNorm without the affine part: the waves' partials of each row merged, the rounded values in acc normalised and stored (model dtype)
// into the panel buffer `dst`.
template <typename T, int NI>
__device__ __forceinline__ void normalise_rows(const f32x4 (&acc)[3][8], const float* red, float eps, unsigned char* dst, int lane, int w) {
  const LaneCols<NI> lc = lane_cols<NI>(lane, w);
#pragma unroll
  for (int mi = 0; mi < 3; ++mi) {
    float mu, rstd;
    merge_partials<kWaves<NI>>(red, mi * 16 + lc.x, eps, mu, rstd);
    const float nm = -mu * rstd;
    unsigned char* drow = dst + (mi * 16 + lc.x) * kRowBytes;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = fmaf(acc[mi][ni][r], rstd, nm);
      *reinterpret_cast<u32x2*>(drow + lc.coff[ni]) = pack4<T>(o);
    }
  }
}
// The same in REGISTERS: acc <- (acc - mean) rstd, unrounded (a round_rows writes - and rounds - it later)
template <typename T, int NI>
__device__ __forceinline__ void normalise_regs(f32x4 (&acc)[3][8], const float* red, float eps, int lane, int w) {
  const LaneCols<NI> lc = lane_cols<NI>(lane, w);
#pragma unroll
  for (int mi = 0; mi < 3; ++mi) {
    float mu, rstd;
    merge_partials<kWaves<NI>>(red, mi * 16 + lc.x, eps, mu, rstd);
    const float nm = -mu * rstd;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[mi][ni][r] = fmaf(acc[mi][ni][r], rstd, nm);
  }
}

// The wave's staged block (panel layout, its own columns) to global memory as row pieces of 32 NI bytes: 2 NI lanes per row
template <typename T, int NI>
__device__ __forceinline__ void store_staged(const unsigned char* strip, T* out, int64_t ld, int nr, int lane, int w) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave reads back only what it wrote itself: no barrier
  asm volatile("" : "+v"(lane), "+s"(w));
  constexpr int kLpr = 2 * NI, kRpi = 64 / kLpr;  // lanes per row, rows per iteration
  const int rl = lane >> (NI == 8 ? 4 : 3), sl = lane & (kLpr - 1);
#pragma unroll
  for (int it = 0; it < kPanel / kRpi; ++it) {
    const int row = it * kRpi + rl;
    const u32x4 v = *reinterpret_cast<const u32x4*>(panel_at(strip, row, w * kLpr + sl));
    if (row < nr) stream_store(v, reinterpret_cast<u32x4*>(out + (int64_t)row * ld + w * (16 * NI) + sl * 8));
  }
}

}  // namespace anemoi
