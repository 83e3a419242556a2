// The source side of a GraphTransformer mapper from RAW rows with a composed weight, for gfx950 (anemoi_gt_embed_fold_fwd) -
//
//     e     = x W_e^T + b_e                         (emb_nodes_src: Linear(in, 512), layers/mapper.py:556-566 of the reference)
//     q_out = LN(e) [W_k; W_v]^T + b                (layer_norm_attention_src + [lin_key; lin_value]: layers/block.py:981-984)
//
// where nobody reads e (the forward mapper does not update its source rows; the statistics are those of e ROUNDED to the model dtype).  With W_g = W diag(gamma) and d = W beta + b the LayerNorm
// between the two Linears is a per-row shift and scale, so
//
//     q_out[j] = rstd_j ((W_g W_e) x_j + W_g b_e - mean_j rowsum(W_g)) + d = rstd_j (W_c x_j + u - mean_j s) + d
//
// is ONE GEMM over K = in_features with the composed weight W_c = W_g W_e; e is needed only for its row statistics and lives in
// accumulators.  Replaces the pair anemoi_linear_stats_fwd + anemoi_linear_lnfold_fwd on this side (e written, 41 MB at 40 320 rows, and
// read back; 2 N K (512 + q_out) flops instead of 2 N 512 (K + q_out)) and loses no [rows x 512] panel of LDS to e.
//
// A workgroup of four waves owns 80 rows of x in LDS (512-byte rows, 16-byte slots XOR-swizzled by the row: the chain kernels' panel
// layout at K <= 256) and needs 72.5 KiB of LDS at q_out = 1024: two workgroups per CU, one wave of each per SIMD, nothing shared but the
// weight lines in the CU's L1 (a 160-row workgroup of eight waves took the same time alone and 13 us more in the forward).  Wave w:
// all 80 rows (5 MFMA row bands), columns 128 w .. + 128 of each 512-column pass: 40 accumulator quads; every weight fragment
// (fragment-major images, ops.pack_weight_frag, L2 -> registers) feeds five MFMAs and is replaced right behind them by the fragment of
// the NEXT K-step - a full K-step (40 MFMAs) of cover for its latency in a ring of one K-step.  Phase 1: e over all 512 columns,
// rounded to the model dtype as the pair does, per-wave (mean, M2) of the rounded values merged in wave order (chain_core.h: no
// E[x^2] - mean^2).  Phase 2: q_out in 512-column passes over the same rows, accumulators started at u, epilogue
// rstd acc + (d - rstd mean s), rounded, staged per row band through a wave-private LDS strip and stored as whole 256-byte row pieces.
// No communication between workgroups.
#include "chain_core.h"

namespace anemoi {

constexpr int kEfBands = 5, kEfWaves = 4;  // (kEfRows, kEfThreads, kEfMaxQ: chain_plan.h)
static_assert(kEfRows == 16 * kEfBands && kEfThreads == 64 * kEfWaves, "chain_plan.h plans this tile");
constexpr int kEfRowBytes = 512;                        // 256 16-bit columns: the widest K
constexpr int kEfRedOff = kEfRows * kEfRowBytes;         // [80 rows][4 waves][2] fp32 partials
constexpr int kEfStripOff = kEfRedOff + kEfRows * 4 * 2 * 4;
constexpr int kEfStripBytes = 16 * 256;                  // one row band of a wave's 128 columns
constexpr int kEfVecOff = kEfStripOff + kEfWaves * kEfStripBytes;
constexpr int kEfVecMax = kCh + 3 * kEfMaxQ;             // fp32 [b_e | u | s | d]
constexpr int ef_smem(int qc) { return kEfVecOff + (kCh + 3 * kCh * qc) * 4; }
constexpr int kEfXIt = kEfRows * 32 / kEfThreads, kEfVecIt = (kEfVecMax / 4 + kEfThreads - 1) / kEfThreads;  // 16-byte pieces per thread, at most
static_assert(ef_smem(kEfMaxQ / kCh) <= 160 * 1024, "LDS budget");
static_assert(ef_smem(1) == ef_lds(1) && ef_smem(kEfMaxQ / kCh) == ef_lds(kEfMaxQ / kCh) && kEfRowBytes == 2 * kEfMaxIn, "chain_plan.h prices this layout");

struct EmbedFoldArgs {
  const void* x;   int64_t ld_x;  int k_in;  // [n_rows, k_in] rows (k_in % 8 == 0, <= 256)
  const char* we;  const char* wc;           // fragment-major [512, 32 nks] and [512 qc, 32 nks] (zero columns beyond k_in)
  int nks, qc;
  const float* vec;                          // [b_e (512) | u | s | d (512 qc each)]
  float eps;
  void* qout;      int64_t ld_q;
  int n_rows;
};

// nks K-steps of this wave's 80 x 128 tile: A fragments from the swizzled rows (this K-step's held, the next one's requested behind
// their last use), B fragments from `ring`, each slot refilled behind its five MFMAs with the same fragment of the next K-step - in
// the last step with the first K-step of the wave's NEXT GEMM (`nxt`).  cs / ns: bytes between the two 64-column slabs of a stream.
template <typename T>
__device__ __forceinline__ void embed_fold_gemm(const unsigned char* arow, int x, int ks, frag8 (&ring)[8], const char* cur, int64_t cs, const char* nxt,
                                                int64_t ns, uint32_t loff, f32x4 (&acc)[kEfBands][8], int nks) {
  frag8 fa[kEfBands];
#pragma unroll
  for (int mi = 0; mi < kEfBands; ++mi) fa[mi] = *reinterpret_cast<const frag8*>(arow + mi * 16 * kEfRowBytes + ((ks ^ x) << 4));
#pragma unroll 1
  for (int st = 0; st < nks; ++st) {
    const bool last = st == nks - 1;
    const gptr_t g0 = uniform_ptr(last ? nxt : cur + (st + 1) * 4096), g1 = uniform_ptr(last ? nxt + ns : cur + cs + (st + 1) * 4096);
    const int aoff = ((((last ? st : st + 1) * 4 + ks) ^ x) << 4);  // (the last step re-reads its own fragments: no branch in the stream)
#pragma unroll
    for (int ni = 0; ni < 8; ++ni) {
#pragma unroll
      for (int mi = 0; mi < kEfBands; ++mi) {
        acc[mi][ni] = mfma16<T>(ring[ni], fa[mi], acc[mi][ni]);  // D^T: lane = row x, 4 consecutive columns
        if (ni == 7) fa[mi] = *reinterpret_cast<const frag8*>(arow + mi * 16 * kEfRowBytes + aoff);
      }
      ring[ni] = *reinterpret_cast<gfrag_t>((ni < 4 ? g0 : g1) + loff + (ni & 3) * 1024);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kEfThreads, 2) void gt_embed_fold_kernel(EmbedFoldArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* const red = reinterpret_cast<float*>(smem + kEfRedOff);
  float* const vec = reinterpret_cast<float*>(smem + kEfVecOff);
  const int tid = threadIdx.x, lane = tid & 63;
  const int c = __builtin_amdgcn_readfirstlane(tid >> 6);  // the wave: columns 128 c .. of every pass
  const uint32_t loff = lane * 16;
  const int x = lane & 15, g = lane >> 4;
  const int r0 = (int)blockIdx.x * kEfRows, nr = min(kEfRows, a.n_rows - r0);
  const int nks = a.nks, qc = a.qc;
  const int64_t slab = (int64_t)nks * 4096;  // one 64-column slab of either image
  const char* const we = a.we + (int64_t)(2 * c) * slab;
  auto wcp = [&](int p) { return a.wc + (int64_t)(8 * p + 2 * c) * slab; };
  frag8 ring[8];
  {  // the rows, the per-column vectors and the ring's first fragments: all requested, then stored
    const int spr = nks * 4, n = kEfRows * spr, kin16 = a.k_in >> 3;  // 16-byte slots per row (<= 32), of the tile
    const int nv = (kCh + 3 * kCh * qc) / 4;
    u32x4 v[kEfXIt], vv[kEfVecIt];
#pragma unroll
    for (int k = 0; k < kEfXIt; ++k) {
      const int i = tid + kEfThreads * k;
      if (k * kEfThreads < n) {  // (wave-uniform)
        const int row = min(i / spr, kEfRows - 1), slot = i % spr;
        const bool live = row < nr && slot < kin16 && i < n;
        const unsigned char* p = reinterpret_cast<const unsigned char*>(a.x) + ((int64_t)(r0 + min(row, nr - 1)) * a.ld_x + min(slot, kin16 - 1) * 8) * 2;
        const u32x4 t = stream_load(reinterpret_cast<const u32x4*>(p));
        v[k] = live ? t : u32x4{0u, 0u, 0u, 0u};
      }
    }
#pragma unroll
    for (int k = 0; k < kEfVecIt; ++k)
      if (k * kEfThreads < nv) vv[k] = reinterpret_cast<const u32x4*>(a.vec)[min(tid + kEfThreads * k, nv - 1)];
    {
      const gptr_t g0 = uniform_ptr(we), g1 = uniform_ptr(we + slab);
#pragma unroll
      for (int ni = 0; ni < 8; ++ni) ring[ni] = *reinterpret_cast<gfrag_t>((ni < 4 ? g0 : g1) + loff + (ni & 3) * 1024);
    }
#pragma unroll
    for (int k = 0; k < kEfXIt; ++k) {
      const int i = tid + kEfThreads * k;
      if (i < n) {
        const int row = i / spr, slot = i % spr;
        *reinterpret_cast<u32x4*>(smem + row * kEfRowBytes + ((slot ^ (row & 15)) << 4)) = v[k];
      }
    }
#pragma unroll
    for (int k = 0; k < kEfVecIt; ++k)
      if (tid + kEfThreads * k < nv) reinterpret_cast<u32x4*>(vec)[tid + kEfThreads * k] = vv[k];
    lds_barrier();
  }
  const unsigned char* const arow = smem + x * kEfRowBytes;
  f32x4 acc[kEfBands][8];
  // ---- phase 1: e = x W_e^T + b_e in accumulators, rounded; row statistics of the rounded values
#pragma unroll
  for (int ni = 0; ni < 8; ++ni) {
    const f32x4 b = *reinterpret_cast<const f32x4*>(vec + c * 128 + ni * 16 + g * 4);
#pragma unroll
    for (int mi = 0; mi < kEfBands; ++mi) acc[mi][ni] = b;
  }
  embed_fold_gemm<T>(arow, x, g, ring, we, slab, wcp(0), slab, loff, acc, nks);
#pragma unroll
  for (int mi = 0; mi < kEfBands; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 8; ++ni) {
      float o[4] = {acc[mi][ni][0], acc[mi][ni][1], acc[mi][ni][2], acc[mi][ni][3]};
      unpack4<T>(pack4<T>(o), o);
      acc[mi][ni] = f32x4{o[0], o[1], o[2], o[3]};
    }
    const float2 p = row_partial<8>(acc[mi]);
    if (g == 0) *reinterpret_cast<float2*>(red + ((mi * 16 + x) * 4 + c) * 2) = p;
  }
  lds_barrier();
  float ra[kEfBands], rb[kEfBands];  // out = ra acc + (rb s + d)
#pragma unroll
  for (int mi = 0; mi < kEfBands; ++mi) {
    float mu, rstd;
    merge_partials<4>(red, mi * 16 + x, a.eps, mu, rstd);
    ra[mi] = rstd;
    rb[mi] = -mu * rstd;
  }
  // ---- phase 2: q_out in 512-column passes with the composed weight
  unsigned char* const strip = smem + kEfStripOff + c * kEfStripBytes;
  const float* const vu = vec + kCh;
  const float* const vs = vu + kCh * qc;
  const float* const vd = vs + kCh * qc;
  T* const out = static_cast<T*>(a.qout);
#pragma unroll 1
  for (int p = 0; p < qc; ++p) {
    const int col0 = p * kCh + c * 128;
#pragma unroll
    for (int ni = 0; ni < 8; ++ni) {
      const f32x4 u = *reinterpret_cast<const f32x4*>(vu + col0 + ni * 16 + g * 4);
#pragma unroll
      for (int mi = 0; mi < kEfBands; ++mi) acc[mi][ni] = u;
    }
    const char* const cur = wcp(p);
    embed_fold_gemm<T>(arow, x, g, ring, cur, slab, p + 1 < qc ? wcp(p + 1) : cur, slab, loff, acc, nks);
    // (the epilogue's coordinates from an OPAQUE copy of the lane id: its 20 row addresses are invariant over the passes, and hoisted out of
    // the loop they are spilled around the GEMM)
    int le = lane;
    asm volatile("" : "+v"(le));
    const int xe = le & 15, ge = le >> 4;
    T* const orow = out + (int64_t)(r0 + ge) * a.ld_q + col0 + xe * 8;
#pragma unroll
    for (int mi = 0; mi < kEfBands; ++mi) {
#pragma unroll
      for (int ni = 0; ni < 8; ++ni) {
        const f32x4 s4 = *reinterpret_cast<const f32x4*>(vs + col0 + ni * 16 + ge * 4);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(vd + col0 + ni * 16 + ge * 4);
        float o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = fmaf(ra[mi], acc[mi][ni][r], fmaf(rb[mi], s4[r], d4[r]));
        *reinterpret_cast<u32x2*>(strip + xe * 256 + (((ni * 2 + (ge >> 1)) ^ xe) << 4) + (ge & 1) * 8) = pack4<T>(o);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave reads back only what it wrote itself: no barrier
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int sr = it * 4 + ge, row = mi * 16 + sr;  // 16 lanes per 256-byte row piece
        const u32x4 t = *reinterpret_cast<const u32x4*>(strip + sr * 256 + ((xe ^ sr) << 4));
        if (row < nr) stream_store(t, reinterpret_cast<u32x4*>(orow + (int64_t)(mi * 16 + it * 4) * a.ld_q));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the strip may be rewritten
    }
  }
}

}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_gt_embed_fold_fwd(const anemoi_gt_embed_fold_args_t* p, anemoi_dtype_t dtype, void* stream) {
  const char* who = "gt_embed_fold_fwd";
  ANEMOI_REQUIRE(p != nullptr, "%s: null argument block", who);
  ChainProblem q;
  q.kind = ChainKind::EmbedFold;
  q.n_rows = p->n_rows, q.in_features = p->in_features, q.q_out_features = p->q_out_features, q.dtype = dtype;
  ChainPlan plan = plan_chain(q, chain_switches());
  if (plan.status == ANEMOI_OK && p->channels != kCh) plan = refuse(ANEMOI_E_UNSUPPORTED, "built for 512 channels");
  if (plan.status != ANEMOI_OK || plan.grid == 0) return chain_refused(who, q, plan);
  ANEMOI_REQUIRE(p->x && p->we && p->wc && p->vec && p->q_out, "%s: null operand", who);
  ANEMOI_REQUIRE(al16(p->x) && al16(p->we) && al16(p->wc) && al16(p->vec) && al16(p->q_out), "%s: operands must be 16-byte aligned", who);
  ANEMOI_REQUIRE(p->ld_x >= p->in_features && p->ld_x % 8 == 0 && p->ld_q >= p->q_out_features && p->ld_q % 8 == 0,
                 "%s: leading dimensions too small or not multiples of 8 elements", who);
  EmbedFoldArgs a;
  a.x = p->x; a.ld_x = p->ld_x; a.k_in = p->in_features;
  a.we = static_cast<const char*>(p->we); a.wc = static_cast<const char*>(p->wc);
  a.nks = 2 * ((p->in_features + 63) / 64); a.qc = p->q_out_features / kCh;
  a.vec = p->vec; a.eps = p->ln_eps;
  a.qout = p->q_out; a.ld_q = p->ld_q;
  a.n_rows = p->n_rows;
  hipStream_t st = as_stream(stream);
  if (dtype == ANEMOI_BF16) ANEMOI_CHAIN_LAUNCH((gt_embed_fold_kernel<bf16_t>), ef_smem(kEfMaxQ / kCh), plan, st, a);
  else ANEMOI_CHAIN_LAUNCH((gt_embed_fold_kernel<f16_t>), ef_smem(kEfMaxQ / kCh), plan, st, a);
  return check_launch("gt_embed_fold_kernel");
}
