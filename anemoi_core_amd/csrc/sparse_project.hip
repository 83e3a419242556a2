// Sparse projection of node rows: y = A f(x) for a CSR matrix A [n_dst, n_src] that is a constant of the model (the truncated residual's
// down / up matrices, layers/residual.py TruncatedConnection; the reference runs torch.sparse.mm between two permute copies per projection,
// layers/sparse_projector.py:78-104).
//
//   y[b, m, c] = sum_{e in [indptr[m], indptr[m+1])} w[e] * f(x[b, indices[e], cols[c]]),      f(v) = v * mul[c] + add[c]
//
// Layout.  The rows are NARROW (a few to a few hundred columns, i.e. a few hundred bytes), so a wave per destination row would idle most
// of its lanes: a destination row belongs to a group of G lanes (G a power of two sized from the column count), 64 / G rows per wave.  The
// batch entries are further columns of the same row (virtual column j = b * C + c), so that a row's indices and weights are read once for
// all of them.  A lane owns the virtual columns j0, j0 + G, ... in passes of kU register accumulators; the entry loop is unrolled by kE, so a
// lane keeps up to kU * kE gathers in flight (a group of 32 lanes with 80 bf16 columns: 4 source rows = 640 B per group, 1.25 KiB per wave).
// Entries are added in CSR order into one fp32 accumulator per element and there are no atomics: results are bitwise reproducible.
//
// What bounds it (measured: DESIGN.md section 11, profiles/r09_truncation_time.json).  Every entry is one gathered row slice.  An up-projection
// (3 nearest coarse rows per fine row) runs at 3-4 TB/s of gathered bytes, its source rows re-read from cache; an fp32 down-projection reaches
// 6.5-6.9 TB/s of gathered bytes at N320.  16-bit rows are SLOWER than fp32 rows (element-granular 2-byte loads: bound by load instructions,
// not bytes; pairing adjacent selected columns is the open lever).  A wave runs as long as its heaviest row: ragged rows cost 1.3-1.9x per
// entry at O96 -> O48 (median 14, max 50 entries; the whole launch is 18-25 us) and nothing at N320 -> O96 (median 52, max 56), so rows are
// not split.
#include "common.h"

namespace anemoi {
namespace {

constexpr int kU = 4;  // register accumulators (virtual columns) per lane and pass
constexpr int kE = 4;  // entries (gathered source rows) in flight per lane group

struct SpArgs {
  const void* x;
  int64_t ldx, bsx, bsx_in;
  const int32_t* indptr;
  const int32_t* indices;
  const float* w;
  const int32_t* cols;
  const float* mul;
  const float* add;
  void* y;
  int64_t ldy, bsy;
  int32_t batch, inner, n_dst, n_src, V, C;
  int32_t log2g;
};

template <typename TX, typename TY>
__global__ __launch_bounds__(256) void sparse_project_kernel(SpArgs a) {
  const int G = 1 << a.log2g;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rows_per_wave = 64 >> a.log2g;
  const int64_t m64 = ((int64_t)blockIdx.x * 4 + wave) * rows_per_wave + (lane >> a.log2g);
  if (m64 >= a.n_dst) return;
  const int m = (int)m64;
  const int g = lane & (G - 1);
  const int J = a.batch * a.C;
  const int beg = a.indptr[m], end = a.indptr[m + 1];
  const TX* __restrict__ xp = (const TX*)a.x;
  TY* __restrict__ yp = (TY*)a.y;
  for (int j0 = g; j0 < J; j0 += G * kU) {
    int64_t off[kU], yoff[kU];
    float mu[kU], ad[kU], acc[kU];
    bool ok[kU], st[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int j = j0 + u * G;
      st[u] = j < J;
      const int b = st[u] ? j / a.C : 0;
      const int c = st[u] ? j - b * a.C : 0;
      const int col = a.cols ? a.cols[c] : c;
      ok[u] = st[u] && (unsigned)col < (unsigned)a.V;  // a column outside x contributes nothing
      const int bo = b / a.inner;  // batch entry b = (bo, bi) of x's two leading dimensions
      off[u] = (int64_t)bo * a.bsx + (int64_t)(b - bo * a.inner) * a.bsx_in + (ok[u] ? col : 0);
      yoff[u] = (int64_t)b * a.bsy + (int64_t)m * a.ldy + c;
      mu[u] = a.mul ? a.mul[c] : 1.f;
      ad[u] = a.add ? a.add[c] : 0.f;
      acc[u] = 0.f;
    }
    const bool affine = a.mul || a.add;
    int e = beg;
    for (; e + kE <= end; e += kE) {
      int idx[kE];
      float wv[kE];
      float v[kE][kU];
#pragma unroll
      for (int i = 0; i < kE; ++i) {
        idx[i] = a.indices[e + i];
        wv[i] = a.w[e + i];
      }
#pragma unroll
      for (int i = 0; i < kE; ++i) {
        const bool in = (unsigned)idx[i] < (unsigned)a.n_src;  // an index outside x contributes nothing (and is never dereferenced)
        const TX* __restrict__ row = xp + (int64_t)(in ? idx[i] : 0) * a.ldx;
        if (!in) wv[i] = 0.f;
#pragma unroll
        for (int u = 0; u < kU; ++u) v[i][u] = (ok[u] && in) ? to_float(row[off[u]]) : 0.f;
      }
#pragma unroll
      for (int i = 0; i < kE; ++i) {  // CSR order
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const float fv = affine ? __fadd_rn(__fmul_rn(v[i][u], mu[u]), ad[u]) : v[i][u];  // two roundings, as the normaliser's own kernel
          acc[u] = fmaf(wv[i], fv, acc[u]);
        }
      }
    }
    for (; e < end; ++e) {
      const int idx = a.indices[e];
      const bool in = (unsigned)idx < (unsigned)a.n_src;
      const float wv = in ? a.w[e] : 0.f;
      const TX* __restrict__ row = xp + (int64_t)(in ? idx : 0) * a.ldx;
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const float v = (ok[u] && in) ? to_float(row[off[u]]) : 0.f;
        const float fv = affine ? __fadd_rn(__fmul_rn(v, mu[u]), ad[u]) : v;
        acc[u] = fmaf(wv, fv, acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u)
      if (st[u]) yp[yoff[u]] = from_float<TY>(ok[u] ? acc[u] : 0.f);
  }
}

template <typename TX, typename TY>
int launch(const SpArgs& a, hipStream_t stream) {
  const int rows_per_block = 4 * (64 >> a.log2g);
  const unsigned grid = (unsigned)(((int64_t)a.n_dst + rows_per_block - 1) / rows_per_block);
  hipLaunchKernelGGL((sparse_project_kernel<TX, TY>), dim3(grid), dim3(256), 0, stream, a);
  return check_launch("sparse_project_kernel");
}

}  // namespace
}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_sparse_project_fwd(const void* x, int64_t ldx, int64_t bsx, int32_t batch_inner, int64_t bsx_inner, int32_t n_src,
                                         int32_t n_cols_x, const int32_t* indptr,
                                         const int32_t* indices, const float* w, const int32_t* cols, const float* mul, const float* add, void* y,
                                         int64_t ldy, int64_t bsy, int32_t batch, int32_t n_dst, int32_t C, anemoi_dtype_t x_dtype,
                                         anemoi_dtype_t y_dtype, void* stream) {
  ANEMOI_REQUIRE(batch >= 0 && n_dst >= 0 && n_src >= 0 && C >= 0 && n_cols_x >= 0, "sparse_project_fwd: bad sizes batch=%d n_dst=%d n_src=%d C=%d V=%d",
                 batch, n_dst, n_src, C, n_cols_x);
  ANEMOI_REQUIRE(x_dtype == ANEMOI_F32 || x_dtype == ANEMOI_BF16 || x_dtype == ANEMOI_F16, "sparse_project_fwd: bad x dtype %d", (int)x_dtype);
  ANEMOI_REQUIRE(y_dtype == ANEMOI_F32 || y_dtype == x_dtype, "sparse_project_fwd: y must be fp32 or of x's dtype");
  ANEMOI_REQUIRE((int64_t)batch * C < (int64_t)1 << 30, "sparse_project_fwd: batch * C = %lld too large", (long long)batch * C);
  ANEMOI_REQUIRE(batch_inner >= 1 && batch % batch_inner == 0, "sparse_project_fwd: batch=%d is not a multiple of batch_inner=%d", batch, batch_inner);
  if (batch == 0 || n_dst == 0 || C == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x || n_src == 0, "sparse_project_fwd: null x");
  ANEMOI_REQUIRE(y && indptr, "sparse_project_fwd: null pointer");
  ANEMOI_REQUIRE(cols || C <= n_cols_x, "sparse_project_fwd: C=%d exceeds the %d columns of x (no column list given)", C, n_cols_x);
  ANEMOI_REQUIRE(ldx >= n_cols_x && ldy >= C, "sparse_project_fwd: leading dimension smaller than the row");
  // lanes per destination row: the power of two that covers the batch * C virtual columns in one pass of kU accumulators
  const int64_t J = (int64_t)batch * C;
  int log2g = 0;
  while (log2g < 6 && ((int64_t)kU << log2g) < J) ++log2g;
  SpArgs a{x, ldx, bsx, bsx_inner, indptr, indices, w, cols, mul, add, y, ldy, bsy, batch, batch_inner, n_dst, n_src, n_cols_x, C, log2g};
  hipStream_t s = as_stream(stream);
  if (x_dtype == ANEMOI_F32) return launch<float, float>(a, s);
  if (x_dtype == ANEMOI_BF16) return y_dtype == ANEMOI_F32 ? launch<bf16_t, float>(a, s) : launch<bf16_t, bf16_t>(a, s);
  return y_dtype == ANEMOI_F32 ? launch<f16_t, float>(a, s) : launch<f16_t, f16_t>(a, s);
}
