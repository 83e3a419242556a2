// The single-panel schedule of the row-resident embedding chain (gt_rowchain.hip) as a device function, so that other launches can run it
// on workgroups of their own: gt_rowchain_kernel walks (blockIdx.x, gridDim.x, n_tiles); the SIDE instantiation of gt_chain2_kernel
// (gt_chain2.hip) lets the workgroups a block tail leaves idle walk a slice of another job's panels.  Per panel:
//
//     S0  all: x rows -> bufA (columns beyond in_features zero: the image of W_e is zero-padded to a multiple of 128 columns)
//     E   all eight waves: y = x W_e^T (48 x 64 tile per wave, K = 128 ng) + b_e, rounded -> bufC, per-wave row statistics
//     L   all: LayerNorm (no affine) of y from registers -> bufB;  group B: y rows -> global (if wanted);  the NEXT panel's x rows requested
//     Q_c group A: chunk 2c, group B: chunk 2c+1 of the projection: acc = dq[chunk]; GEMM on bufB; rounded -> the group's staging buffer (A: bufA,
//         B: bufC, each wave its own 128 columns) -> whole 256-byte row pieces to global
#pragma once
#include "chain2_core.h"

namespace anemoi {

struct RowChainArgs {
  const void* x;   int64_t ld_x;  int k_in;  // [n_rows, k_in] input rows (k_in % 8 == 0, <= 512)
  const char* we;  int ng;                   // embedding, fragment-major [512, 128 ng] (zero columns beyond k_in)
  const char* wq;  int qc;                   // projection with the LayerNorm's gamma folded in, fragment-major [512 qc, 512]
  const void* vec;                           // [b_e (512) | dq (512 qc)], model dtype
  float eps;
  void* xout;      int64_t ld_out;           // optional [n_rows, 512]: y
  void* qout;      int64_t ld_q;             // [n_rows, 512 qc]
  int n_rows, rows_per_tile, n_tiles;
};
constexpr int kRcVecOff = vec_off(8);  // the per-column vectors (16-bit), behind the [48 rows][8 waves][2] partials: 512 + 512 qc <= 2560
constexpr int kRcVecMax = 2560;
constexpr int kRowChainSmem = kRcVecOff + kRcVecMax * 2;
static_assert(kRowChainSmem <= 160 * 1024, "LDS budget");
static_assert(kRowChainSmem == kRowChainLds && kRcVecMax == kCh + kRowChainMaxQ, "chain_plan.h prices this layout");

// A panel of input rows: 48 rows x spr = 16 ng sixteen-byte slots (slots beyond the row's k_in / 8 are zero), shared out among the 512
// threads (<= 6 slots each), requested into registers and stored to the swizzled panel later - the request of the NEXT panel rides under
// the projection GEMMs of this one.
struct XRows {
  u32x4 v[6];
  __device__ __forceinline__ void request(const void* x, int64_t ld, int k_in, int ng, int r0, int nr, int tid, int es) {
    const int spr = 16 * ng, n = kPanel * spr, kin16 = k_in >> 3;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int i = tid + 512 * k;
      if (k * 512 < n) {  // (wave-uniform)
        const int row = min(i / spr, kPanel - 1), slot = i % spr;
        const bool live = row < nr && slot < kin16 && i < n;
        const unsigned char* p = reinterpret_cast<const unsigned char*>(x) + ((int64_t)(r0 + min(row, nr - 1)) * ld + min(slot, kin16 - 1) * 8) * es;
        const u32x4 t = stream_load(reinterpret_cast<const u32x4*>(p));
        v[k] = live ? t : u32x4{0u, 0u, 0u, 0u};
      }
    }
  }
  __device__ __forceinline__ void store(unsigned char* buf, int ng, int tid) {
    const int spr = 16 * ng, n = kPanel * spr;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int i = tid + 512 * k;
      if (i < n) {
        const int row = i / spr, slot = i % spr;
        *reinterpret_cast<u32x4*>(panel_at(buf, row, slot)) = v[k];
      }
    }
  }
};

// Which panels a workgroup walks: first(), first() + stride(), ... < end().  (Asked where the schedule needs them, not up front: the
// whole-launch walk then compiles to the code the kernel had before it became a function.)
struct GridWalk {  // the launch is the job: (blockIdx.x, gridDim.x, n_tiles)
  __device__ __forceinline__ int first() const { return blockIdx.x; }
  __device__ __forceinline__ int stride() const { return (int)gridDim.x; }
  __device__ __forceinline__ int end(const RowChainArgs& a) const { return a.n_tiles; }
};
struct SliceWalk {  // a slice of the job's panels on some of a launch's workgroups
  int first_, stride_, end_;
  __device__ __forceinline__ int first() const { return first_; }
  __device__ __forceinline__ int stride() const { return stride_; }
  __device__ __forceinline__ int end(const RowChainArgs&) const { return end_; }
};

// The walk's panels of the job `a` (all 512 threads; the launch's dynamic LDS from its start: kRowChainSmem bytes).
template <typename T, typename Walk>
__device__ __forceinline__ void rowchain_panels(const RowChainArgs& a, const Walk w) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const bufA = smem;
  unsigned char* const bufB = smem + kBufBytes;
  unsigned char* const bufC = smem + 2 * kBufBytes;
  float* const red = reinterpret_cast<float*>(smem + kRedOff);
  const unsigned char* const vec = smem + kRcVecOff;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6), wq = w8 & 3, grp = w8 >> 2;  // waves wq and wq + 4 share a SIMD
  const uint32_t loff = lane * 16;
  const int qc = a.qc, ng = a.ng;
  const int64_t se = (int64_t)ng * 16384;  // one 64-column slab of the embedding image: 4 ng K-steps x 4 KiB
  const char* const wes = a.we + (int64_t)w8 * se;
  auto wqc = [&](int k) { return a.wq + (int64_t)(8 * k + 2 * wq) * kSlab; };
  int tile = w.first();
  if (tile >= w.end(a)) return;
  frag8 ring[2][8];
  f32x4 acc[3][8];
  XRows xr;
  // the first panel's rows, then the per-column vectors and the weight ring's first fragments behind them (loads return in order)
  {
    const int r0 = tile * a.rows_per_tile;
    xr.request(a.x, a.ld_x, a.k_in, ng, r0, min(a.rows_per_tile, a.n_rows - r0), tid, (int)sizeof(T));
    const int n16 = (512 + 512 * qc) / 8;  // <= 320
    u32x4 vv = reinterpret_cast<const u32x4*>(a.vec)[min(tid, n16 - 1)];
    ring_prologue64(ring, wes, loff);
    xr.store(bufA, ng, tid);
    if (tid < n16) reinterpret_cast<u32x4*>(smem + kRcVecOff)[tid] = vv;
    lds_barrier();
  }
  const bool mine_any = grp < qc;  // this group has at least one chunk of the projection
  for (;;) {
    const int r0 = tile * a.rows_per_tile;
    const int nr = min(a.rows_per_tile, a.n_rows - r0);
    // E: y = x W_e^T + b_e -> bufC (rounded), row statistics
#pragma unroll
    for (int mi = 0; mi < 3; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    gemm64<T>(bufA, lane, ring, wes, mine_any ? wqc(grp) : wes, mine_any ? (int64_t)kSlab : (int64_t)8192, loff, acc, ng);
    round_rows<T, 4, Add::Bias, true>(acc, bufC, red, lane, w8, vec);
    lds_barrier();  // y and the partials are complete; every wave is behind its last read of the x rows
    // L: LayerNorm (no affine) -> bufB; y -> global by group B (each wave its own 128 columns: the columns it will stage its chunk in)
    normalise_rows<T, 4>(acc, red, a.eps, bufB, lane, w8);
    if (a.xout != nullptr && grp == 1) store_staged<T, 8>(bufC, (T*)a.xout + (int64_t)r0 * a.ld_out, a.ld_out, nr, lane, wq);
    const int tile_next = tile + w.stride();
    const bool more = tile_next < w.end(a);
    if (more) {
      const int rn = tile_next * a.rows_per_tile;
      xr.request(a.x, a.ld_x, a.k_in, ng, rn, min(a.rows_per_tile, a.n_rows - rn), tid, (int)sizeof(T));
    }
    lds_barrier();
    // Q: this group's chunks of the projection
    unsigned char* const stage = grp == 0 ? bufA : bufC;
    for (int k = grp; k < qc; k += 2) {
      init_acc<T, 8, false>(acc, vec, 512 + 512 * k, nullptr, lane, wq);
      const bool last = k + 2 >= qc;
      gemm128<T>(bufB, lane, ring, wqc(k), kSlab, last ? wes : wqc(k + 2), last ? (int64_t)8192 : (int64_t)kSlab, loff, acc);
      round_rows<T, 8, Add::None, false>(acc, stage, nullptr, lane, wq);
      store_staged<T, 8>(stage, (T*)a.qout + (int64_t)r0 * a.ld_q + k * kCh, a.ld_q, nr, lane, wq);
    }
    lds_barrier();  // every wave is behind its last read of bufB and of its staging columns
    if (!more) break;
    tile = tile_next;
    xr.store(bufA, ng, tid);
    lds_barrier();
  }
}

// ---------------------------------------------------------------------------------------------------------------- several panel rounds: pipelined
// (the schedule is described in gt_rowchain.hip, in front of gt_rowchain_pipe_kernel)
constexpr int kRc2Vec = vec_off(4);  // (four waves' partials)
constexpr int kRowChain2Smem = kRc2Vec + kRcVecMax * 2;
static_assert(kRowChain2Smem <= 160 * 1024, "LDS budget");
static_assert(kRowChain2Smem == kRowChainPipeLds, "chain_plan.h prices this layout");

struct XRowsA {  // a panel of input rows shared out among group A's 256 threads: <= 6 sixteen-byte slots each (in_features <= 256)
  u32x4 v[6];
  __device__ __forceinline__ void request(const void* x, int64_t ld, int k_in, int ng, int r0, int nr, int t, int es) {
    const int spr = 16 * ng, n = kPanel * spr, kin16 = k_in >> 3;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int i = t + 256 * k;
      if (k * 256 < n) {  // (wave-uniform)
        const int row = min(i / spr, kPanel - 1), slot = i % spr;
        const bool live = row < nr && slot < kin16 && i < n;
        const unsigned char* p = reinterpret_cast<const unsigned char*>(x) + ((int64_t)(r0 + min(row, nr - 1)) * ld + min(slot, kin16 - 1) * 8) * es;
        const u32x4 tv = stream_load(reinterpret_cast<const u32x4*>(p));
        v[k] = live ? tv : u32x4{0u, 0u, 0u, 0u};
      }
    }
  }
  __device__ __forceinline__ void store(unsigned char* buf, int ng, int t) {
    const int spr = 16 * ng, n = kPanel * spr;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int i = t + 256 * k;
      if (i < n) {
        const int row = i / spr, slot = i % spr;
        *reinterpret_cast<u32x4*>(panel_at(buf, row, slot)) = v[k];
      }
    }
  }
};

struct PipeCtx {
  int lane, wq, tid;
  uint32_t loff;
  int b0, grid, n;  // this workgroup's panels: b0, b0 + grid, ... (n of them)
};
__device__ __forceinline__ void pipe_rows(const RowChainArgs& a, const PipeCtx& c, int s, int& r0, int& nr) {
  r0 = (c.b0 + s * c.grid) * a.rows_per_tile;
  nr = min(a.rows_per_tile, a.n_rows - r0);
}

// Both roles execute the SAME barriers: one behind the prologue, three per step (behind phases 1, 2, 3), n + 1 steps.
template <typename T>
__device__ __forceinline__ void pipe_role_a(const RowChainArgs& a, const PipeCtx& c, unsigned char* smem) {
  unsigned char* const bufX = smem;
  unsigned char* const bufN = smem + kBufBytes;
  float* const red = reinterpret_cast<float*>(smem + kRedOff);
  const unsigned char* const vec = smem + kRc2Vec;
  const int lane = c.lane, wq = __builtin_amdgcn_readfirstlane(c.wq), ng = a.ng, n = c.n;
  const int64_t se = (int64_t)ng * 16384;  // one 64-column slab of the embedding image
  const char* const wes = a.we + (int64_t)(2 * wq) * se;
  frag8 ring[2][8];
  f32x4 acc[3][8];
  XRowsA xr;
  {
    int r0, nr;
    pipe_rows(a, c, 0, r0, nr);
    xr.request(a.x, a.ld_x, a.k_in, ng, r0, nr, c.tid, (int)sizeof(T));
    ring_prologue(ring, wes, se, c.loff);
    xr.store(bufX, ng, c.tid);
    lds_barrier();
  }
  for (int s = 0; s <= n; ++s) {
    // phase 1: LN(y)(s-1), parked in the accumulators -> bufN (rounded here); the rows of x(s) -> bufX
    if (s >= 1) {
      round_rows<T, 8, Add::None, false>(acc, bufN, nullptr, lane, wq);
      if (s < n) xr.store(bufX, ng, c.tid);
    }
    lds_barrier();
    // phase 2: y = x W_e^T + b_e, rounded in registers, per-wave row statistics; x(s+1) requested
    if (s < n) {
      if (s + 1 < n) {
        int rn, nrn;
        pipe_rows(a, c, s + 1, rn, nrn);
        xr.request(a.x, a.ld_x, a.k_in, ng, rn, nrn, c.tid, (int)sizeof(T));
      }
      init_acc<T, 8, false>(acc, vec, 0, nullptr, lane, wq);
      gemm128<T>(bufX, lane, ring, wes, se, wes, se, c.loff, acc, 2 * ng);
      round_rows<T, 8, Add::None, true, false>(acc, nullptr, red, lane, wq);
    }
    lds_barrier();
    // phase 3: y -> global (staged through bufX: every wave of the group is behind its last read of the x rows); LN(y) in registers
    if (s < n) {
      if (a.xout != nullptr) {
        int r0, nr;
        pipe_rows(a, c, s, r0, nr);
        round_rows<T, 8, Add::None, false>(acc, bufX, nullptr, lane, wq);
        store_staged<T, 8>(bufX, (T*)a.xout + (int64_t)r0 * a.ld_out, a.ld_out, nr, lane, wq);
      }
      normalise_regs<T, 8>(acc, red, a.eps, lane, wq);
    }
    lds_barrier();
  }
}

template <typename T>
__device__ __forceinline__ void pipe_role_b(const RowChainArgs& a, const PipeCtx& c, unsigned char* smem) {
  unsigned char* const bufN = smem + kBufBytes;
  unsigned char* const bufS = smem + 2 * kBufBytes;
  const unsigned char* const vec = smem + kRc2Vec;
  const int lane = c.lane, wq = __builtin_amdgcn_readfirstlane(c.wq), qc = a.qc, n = c.n;
  auto wqc = [&](int k) { return a.wq + (int64_t)(8 * k + 2 * wq) * kSlab; };
  frag8 ring[2][8];
  f32x4 acc[3][8];
  ring_prologue(ring, wqc(0), kSlab, c.loff);
  lds_barrier();
  for (int s = 0; s <= n; ++s) {
    int rp, nrp;
    pipe_rows(a, c, s - 1, rp, nrp);
    lds_barrier();  // phase 1 is group A's
    // phase 2: chunk 0 of the projection of panel s - 1
    if (s >= 1) {
      init_acc<T, 8, false>(acc, vec, 512, nullptr, lane, wq);
      gemm128<T>(bufN, lane, ring, wqc(0), kSlab, qc > 1 ? wqc(1) : wqc(0), kSlab, c.loff, acc);
      round_rows<T, 8, Add::None, false>(acc, bufS, nullptr, lane, wq);
      store_staged<T, 8>(bufS, (T*)a.qout + (int64_t)rp * a.ld_q, a.ld_q, nrp, lane, wq);
    }
    lds_barrier();
    // phase 3: its other chunks
    if (s >= 1) {
      for (int k = 1; k < qc; ++k) {
        init_acc<T, 8, false>(acc, vec, 512 + 512 * k, nullptr, lane, wq);
        gemm128<T>(bufN, lane, ring, wqc(k), kSlab, k + 1 < qc ? wqc(k + 1) : wqc(0), kSlab, c.loff, acc);
        round_rows<T, 8, Add::None, false>(acc, bufS, nullptr, lane, wq);
        store_staged<T, 8>(bufS, (T*)a.qout + (int64_t)rp * a.ld_q + k * kCh, a.ld_q, nrp, lane, wq);
      }
    }
    lds_barrier();
  }
}


// The pipelined schedule on this workgroup's panels b0, b0 + stride, ... < end of the job (all 512 threads; dynamic LDS: kRowChain2Smem bytes).
template <typename T>
__device__ __forceinline__ void rowchain_pipe_panels(const RowChainArgs& a, int b0, int stride, int end) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  PipeCtx c;
  c.tid = tid & 255;
  c.lane = tid & 63;
  const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  c.wq = w8 & 3;
  c.loff = c.lane * 16;
  c.b0 = b0;
  c.grid = stride;
  if (c.b0 >= end) return;
  c.n = (end - c.b0 + c.grid - 1) / c.grid;
  {  // the per-column vectors -> LDS (visible behind the prologue's barrier)
    const int n16 = (512 + 512 * a.qc) / 8;  // <= 320
    if (tid < n16) reinterpret_cast<u32x4*>(smem + kRc2Vec)[tid] = reinterpret_cast<const u32x4*>(a.vec)[tid];
  }
  if (w8 < 4) pipe_role_a<T>(a, c, smem);
  else pipe_role_b<T>(a, c, smem);
}

// The argument block of the C ABI -> the kernel's: the shape is the plan's to judge (chain_plan.h: grid, schedule - rowchain_pipelined on why a
// part of a job takes the schedule of the whole job), the operands are judged here (`who`: the entry point's name in the messages).
// ANEMOI_OK with an empty plan: nothing to do.
inline ChainProblem rowchain_problem(const anemoi_gt_rowchain_args_t* p, anemoi_dtype_t dtype, ChainKind kind = ChainKind::RowChain, int first_panel = 0,
                                     int panels = 0) {
  ChainProblem q;
  q.kind = kind;
  q.n_rows = p->n_rows, q.in_features = p->in_features, q.q_out_features = p->q_out_features, q.rows_per_tile = p->rows_per_tile, q.dtype = dtype;
  q.first_panel = first_panel, q.panels = panels;
  return q;
}
inline int rowchain_args(const anemoi_gt_rowchain_args_t* p, const ChainProblem& q, const char* who, RowChainArgs& a, ChainPlan& plan) {
  a = RowChainArgs{};
  ANEMOI_REQUIRE(p->channels == kCh, "%s: channels=%d (this kernel is built for %d)", who, p->channels, kCh);
  plan = plan_chain(q, chain_switches());
  if (plan.status != ANEMOI_OK) return chain_refused(who, q, plan);
  if (p->n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(p->x && p->we && p->wq && p->vec && p->q_out, "%s: null operand", who);
  ANEMOI_REQUIRE(al16(p->x) && al16(p->we) && al16(p->wq) && al16(p->vec) && al16(p->x_out) && al16(p->q_out), "%s: operands must be 16-byte aligned", who);
  ANEMOI_REQUIRE(p->ld_x >= p->in_features && p->ld_x % 8 == 0 && p->ld_q >= p->q_out_features && p->ld_q % 8 == 0 &&
                     (p->x_out == nullptr || (p->ld_out >= kCh && p->ld_out % 8 == 0)),
                 "%s: leading dimensions too small or not multiples of 8 elements", who);
  a.x = p->x; a.ld_x = p->ld_x; a.k_in = p->in_features;
  a.we = (const char*)p->we; a.ng = (p->in_features + 127) / 128;
  a.wq = (const char*)p->wq; a.qc = p->q_out_features / kCh;
  a.vec = p->vec;
  a.eps = p->ln_eps;
  a.xout = p->x_out; a.ld_out = p->ld_out;
  a.qout = p->q_out; a.ld_q = p->ld_q;
  a.n_rows = p->n_rows;
  a.rows_per_tile = p->rows_per_tile > 0 ? p->rows_per_tile : kPanel;
  a.n_tiles = (a.n_rows + a.rows_per_tile - 1) / a.rows_per_tile;
  return ANEMOI_OK;
}

}  // namespace anemoi
