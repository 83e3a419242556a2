// Shared device code of the ROLE-SPLIT row-resident chain kernels (round 5; gt_chain2.hip: the GraphTransformer block tail; round 6:
// gt_rowchain.hip: the mappers' embedding -> LayerNorm -> projection chains; experiments/gnn_chain2.hip: GraphConv's edge MLP).  The workgroup's eight waves form two groups of four (waves w and w + 4 share a SIMD); a wave owns a 48 x 128
// output slab of its group's GEMM segment: 24 accumulator quads, the three A fragments of a K-step shared by eight column blocks, its
// 8 KiB of weights per K-step through a register ring of only two K-steps (tools/role_split_probe.hip: one such group pulls the weight
// stream through the CU's L1 path as fast as eight 64-column waves do, in 200 registers).  What the groups do differs per kernel; the
// pieces here are the GEMM segments, the weight rings' prologues, the row loads and the L2 warm-up of weights one step ahead (the panel
// layout and the epilogue forms: chain_core.h).
#pragma once
#include "chain_core.h"

namespace anemoi {

// 16 K-steps (K = 512) of this wave's 48 x 128 tile.  A fragments from the swizzled LDS panel (the next K-step's requested before this
// one's MFMAs), B fragments from a register ring of two K-steps x 8 fragments, each slot refilled right behind its three MFMAs with
// the fragment of two K-steps ahead - of this segment or, in its last pair, of the wave's NEXT segment (`nxt`).  The wave's 128
// columns are two adjacent 64-column slabs of the fragment-major image: streams `cur` and `cur + cs`.
// nq: pairs of K-steps (K = 64 nq; 8 = the 512-wide segment every caller but a narrow first GEMM uses).
template <typename T>
__device__ __forceinline__ void gemm128(const unsigned char* abuf, int lane, frag8 (&ring)[2][8], const char* cur, int64_t cs, const char* nxt,
                                        int64_t ns, uint32_t loff, f32x4 (&acc)[3][8], int nq = 8) {
  asm volatile("" : "+v"(lane));
  const int x = lane & 15, ks = lane >> 4;
  const unsigned char* arow = abuf + x * kRowBytes;
  frag8 fa[3];
#pragma unroll
  for (int mi = 0; mi < 3; ++mi) fa[mi] = *reinterpret_cast<const frag8*>(arow + mi * 16 * kRowBytes + ((ks ^ x) << 4));
  const int last = 2 * nq - 1;
#pragma unroll 1
  for (int q = 0; q < nq; ++q) {
    const char* p0 = q < nq - 1 ? cur + (q + 1) * 8192 : nxt;
    const char* p1 = q < nq - 1 ? cur + cs + (q + 1) * 8192 : nxt + ns;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int st = q * 2 + j;
      const int sn = st < last ? st + 1 : last;  // (the last step re-reads its own fragments: no branch in the stream)
      frag8 fn[3];
#pragma unroll
      for (int mi = 0; mi < 3; ++mi) fn[mi] = *reinterpret_cast<const frag8*>(arow + mi * 16 * kRowBytes + (((sn * 4 + ks) ^ x) << 4));
      __builtin_amdgcn_sched_barrier(0);
      const gptr_t g0 = uniform_ptr(p0 + j * 4096), g1 = uniform_ptr(p1 + j * 4096);
#pragma unroll
      for (int ni = 0; ni < 8; ++ni) {
#pragma unroll
        for (int mi = 0; mi < 3; ++mi) acc[mi][ni] = mfma16<T>(ring[j][ni], fa[mi], acc[mi][ni]);  // D^T: lane = row x, 4 consecutive columns
        ring[j][ni] = *reinterpret_cast<gfrag_t>((ni < 4 ? g0 : g1) + loff + (ni & 3) * 1024);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int mi = 0; mi < 3; ++mi) fa[mi] = fn[mi];
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// The same for a 48 x 64 tile (ONE 64-column slab of the image, acc[mi][0..3]) on the SAME ring registers, as four K-steps x 4 fragments:
// K-step j of the stream sits in ring[j & 1][(j >> 1) * 4 + ni].  Used where all eight waves of the workgroup share ONE segment (the
// projection: 512 columns = 8 waves x 64), so that its epilogue is spread over eight waves instead of four.  In its last group of four
// K-steps the slots are refilled with the first fragments of the wave's NEXT segment in the layout gemm128 expects (two K-steps of the
// two slabs `nxt`, `nxt + ns`); a gemm128 hands over to a gemm64 with ns = 8192 (K-steps 2, 3 of the one slab behind K-steps 0, 1).
// ng: groups of four K-steps (K = 128 ng; 4 = the 512-wide segment; fewer: a narrow first GEMM on a zero-padded operand).
template <typename T>
__device__ __forceinline__ void gemm64(const unsigned char* abuf, int lane, frag8 (&ring)[2][8], const char* cur, const char* nxt, int64_t ns,
                                       uint32_t loff, f32x4 (&acc)[3][8], int ng = 4) {
  asm volatile("" : "+v"(lane));
  const int x = lane & 15, ks = lane >> 4;
  const unsigned char* arow = abuf + x * kRowBytes;
  frag8 fa[3];
#pragma unroll
  for (int mi = 0; mi < 3; ++mi) fa[mi] = *reinterpret_cast<const frag8*>(arow + mi * 16 * kRowBytes + ((ks ^ x) << 4));
  const int last = ng * 4 - 1;
#pragma unroll 1
  for (int q = 0; q < ng; ++q) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int st = q * 4 + j;
      const int sn = st < last ? st + 1 : last;  // (the last step re-reads its own fragments: no branch in the stream)
      frag8 fn[3];
#pragma unroll
      for (int mi = 0; mi < 3; ++mi) fn[mi] = *reinterpret_cast<const frag8*>(arow + mi * 16 * kRowBytes + (((sn * 4 + ks) ^ x) << 4));
      __builtin_amdgcn_sched_barrier(0);
      const char* pf = q < ng - 1 ? cur + (q + 1) * 16384 + j * 4096 : (j < 2 ? nxt + j * 4096 : nxt + ns + (j - 2) * 4096);
      const gptr_t g0 = uniform_ptr(pf);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
        for (int mi = 0; mi < 3; ++mi) acc[mi][ni] = mfma16<T>(ring[j & 1][(j >> 1) * 4 + ni], fa[mi], acc[mi][ni]);
        ring[j & 1][(j >> 1) * 4 + ni] = *reinterpret_cast<gfrag_t>(g0 + loff + ni * 1024);
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int mi = 0; mi < 3; ++mi) fa[mi] = fn[mi];
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}
// the wave's first weight fragments of a gemm64 segment (four K-steps of the one slab)
__device__ __forceinline__ void ring_prologue64(frag8 (&ring)[2][8], const char* f0, uint32_t loff) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const gptr_t g0 = uniform_ptr(f0 + j * 4096);
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      ring[j & 1][(j >> 1) * 4 + ni] = *reinterpret_cast<gfrag_t>(g0 + loff + ni * 1024);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// 12 whole rows of the panel (rows wq*12 ..) from global memory into a panel buffer; rows beyond the panel are zero
template <typename T, typename Between>
__device__ __forceinline__ void load_rows12(const T* src, int64_t ld, int r0, int nr, unsigned char* dst, int lane, int wq, Between between) {
  asm volatile("" : "+v"(lane), "+s"(wq));  // (else the twelve LDS addresses are hoisted out of the panel loop and spilled around the GEMM segments)
  u32x4 v[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const int row = wq * 12 + i;
    v[i] = stream_load(reinterpret_cast<const u32x4*>(src + (int64_t)(r0 + min(row, nr - 1)) * ld + lane * 8));
  }
  __builtin_amdgcn_sched_barrier(0);
  between();  // (loads the caller wants queued BEHIND the rows)
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    const int row = wq * 12 + i;
    *reinterpret_cast<u32x4*>(panel_at(dst, row, lane)) = row < nr ? v[i] : u32x4{0u, 0u, 0u, 0u};
  }
}
// the wave's first weight fragments (two K-steps of both 64-column streams)
__device__ __forceinline__ void ring_prologue(frag8 (&ring)[2][8], const char* f0, int64_t fs, uint32_t loff) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const gptr_t g0 = uniform_ptr(f0 + j * 4096), g1 = uniform_ptr(f0 + fs + j * 4096);
#pragma unroll
    for (int ni = 0; ni < 8; ++ni) {
      ring[j][ni] = *reinterpret_cast<gfrag_t>((ni < 4 ? g0 : g1) + loff + (ni & 3) * 1024);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}
// L2 warm-up of a weight segment one step ahead of its use.  All CUs of an XCD walk the same weight stream at the same time behind a ring
// of only two K-steps, so a line that misses the XCD's L2 (in a 16-layer model every layer's weights have left the caches since the
// last forward) exposes the HBM latency to all 32 of them at once.  Each CU therefore TOUCHES its 1/32 share of the segments of the
// NEXT step - one dword per 128-byte line, 64 lines per instruction - from group A's waves right behind their GEMM, where the
// epilogue that follows hides the latency; by the time a ring asks for the lines they are in the L2 (observed: workgroup b runs on XCD
// b % 8, so b / 8 numbers the CUs of an XCD - for speed only: a different placement warms less, nothing depends on it).
// A segment = the 512 x 512 weight of one group step: eight 64-KiB slabs `piece` bytes apart; `half` selects 64 of the CU's 128 lines.
struct Warm {
  unsigned v[3];
  int first, end;  // PART: this lane's first line of the wave's share, one past the share's last line
  int n_it;        // PART: loads per touch (wave-uniform)
};
// PART = false: all 256 CUs work, workgroup b touches the fixed 1/32 share (b >> 3) & 31 (observed: b runs on XCD b % 8), its line recomputed
// from the workgroup id at every touch (nothing kept live).  PART = true (a launch of fewer than 256 workgroups): the launch's workgroups on
// my XCD share the segment's 4096 lines out among themselves - ALL of them (10 242 rows = 214 panels of 48: 26 or 27 CUs per XCD; with a
// fixed 1/32 share each, 16 % of every weight stayed cold: the O96 forward 2.81 instead of 2.55 ms, profiles/r05_chain2_touch_coverage.txt).
// Two waves per share (`half`), up to 192 lines per wave = full coverage from 11 workgroups per XCD on; the bounds are computed once per kernel.
// GIVEN: the workgroups that share the weights are the first n_wg of the grid (the rest of the launch does other work), not all of it.
template <bool PART, bool GIVEN = false>
__device__ __forceinline__ void warm_init(Warm& w, int half, int lane, int n_wg = 0) {
  w.v[0] = w.v[1] = w.v[2] = 0u;
  if constexpr (PART) {
    const int xcd = (int)blockIdx.x & 7;
    const int n_cu = ((GIVEN ? n_wg : (int)gridDim.x) - xcd + 7) >> 3;
    const int s = (int)blockIdx.x >> 3;
    const int lo = (s * 4096) / n_cu, hi = ((s + 1) * 4096) / n_cu;
    const int mid = lo + ((hi - lo + 1) >> 1);
    w.first = (half ? mid : lo) + lane;
    w.end = half ? hi : mid;
    w.n_it = __builtin_amdgcn_readfirstlane((w.end - (half ? mid : lo) + 63) >> 6);
  }
}
template <bool PART>
__device__ __forceinline__ void touch_share(Warm& w, const char* seg, int64_t piece, int half, int lane) {
  if constexpr (!PART) {
    const int line = (((int)blockIdx.x >> 3) & 31) * 128 + half * 64 + lane;  // 0 .. 4095
    w.v[0] = *reinterpret_cast<const unsigned*>(seg + (int64_t)(line >> 9) * piece + (line & 511) * 128);
  } else {
    int line = w.first;
    asm volatile("" : "+v"(line));  // (else the line addresses of every call site are computed up front and live - spilled - through the kernel)
#pragma unroll
    for (int it = 0; it < 3; ++it) {
      if (it < w.n_it) {  // (wave-uniform)
        const int l = min(line, w.end - 1);  // (lanes beyond the share re-touch its last line: no divergence)
        w.v[it] = *reinterpret_cast<const unsigned*>(seg + (int64_t)(l >> 9) * piece + (l & 511) * 128);
        line += 64;
      }
    }
  }
}
// (the touched values must stay "in use" until the next touch: the compiler then keeps their registers and counts the loads)
template <bool PART>
__device__ __forceinline__ void touch_done(Warm& w) {
  if constexpr (PART) asm volatile("" : "+v"(w.v[0]), "+v"(w.v[1]), "+v"(w.v[2]));
  else asm volatile("" : "+v"(w.v[0]));
}

}  // namespace anemoi
