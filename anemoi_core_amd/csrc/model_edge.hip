// Model-edge kernels: what runs once per forward on the raw input and on the model's output (reference
// models/encoder_processor_decoder.py:98-163 with the pre- / post-processor chains of models/base.py:303-391 fused in).
//
//   input assembly    out[n] = [ stage(x[0, n, :]) | ... | stage(x[T-1, n, :]) | attrs[n, :] | 0 ... ]
//   output assembly   out[n, v] = x_out[n, v] + stage(x_skip[n, col_map[v]])
//   column program    the boundings, the de-normalisation and the inverse ops of the post chain, in place and in order
//
// `stage` is ONE per-element chain, edge_chain_one<TI, IMPUTE, REMAP>: impute, remap forward, x * mul + add.  The imputer and the
// remapper are compile-time flags of the kernels (four combinations), the normaliser a run-time null test; the column program is one
// switch whose higher kinds are compiled out of the lower LEVELs.  The stand-alone kernels of the same modules (affine / impute /
// restore_nan / remap columns) and the pure-copy assemblies (assemble_input_kernel / assemble_output_kernel: vector moves, no
// conversion) are here as well.
#include "remap_core.h"
#include "rowwise_common.h"

namespace anemoi {

// Output assembly at the model edge (reference models/encoder_processor_decoder.py:145-163 for batch = ensemble = time = 1):
// out[n, v] = x_out[n, v] + (col_map[v] >= 0 ? x_skip[n, col_map[v]] : 0) - the residual (SkipConnection) added onto the
// prognostic columns - in one pass instead of clone + index_select + index_add_.
template <typename T, int Q>
__global__ void assemble_output_kernel(const T* __restrict__ x_out, int64_t ldx, const T* __restrict__ skip, int64_t lds,
                                       const int32_t* __restrict__ col_map, T* __restrict__ out, int64_t ldo, int n_rows, int n_cols) {
  const int per_row = n_cols / Q;  // Q columns per thread (8-byte moves for 16-bit types when the widths / strides allow)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * per_row) return;
  const int n = (int)(i / per_row), v0 = (int)(i % per_row) * Q;
  Vec<T, Q> a = *reinterpret_cast<const Vec<T, Q>*>(x_out + (int64_t)n * ldx + v0), o;
#pragma unroll
  for (int j = 0; j < Q; ++j) {
    float val = to_float(a.v[j]);
    const int m = col_map[v0 + j];
    if (m >= 0) val = to_float(from_float<T>(val)) + to_float(skip[(int64_t)n * lds + m]);
    o.v[j] = from_float<T>(val);
  }
  *reinterpret_cast<Vec<T, Q>*>(out + (int64_t)n * ldo + v0) = o;
}

// Input assembly at the model edge for batch = ensemble = 1 (reference models/encoder_processor_decoder.py:98-143,
// "batch time ensemble grid vars -> (batch ensemble grid) (time vars)" + cat with the node attributes):
//   out[n, :] = [ x[0, n, :] | ... | x[T-1, n, :] | attrs[n, :] | 0 ... ]   (width W >= T*V + A: the alignment zeros of the embedding GEMMs)
// in one pass instead of a permute-copy and a cat.  Q elements per thread (Q = 4 when V, A, W and the row strides allow 8-byte moves).
template <typename T, int Q>
__global__ void assemble_input_kernel(const T* __restrict__ x, int64_t ld_t, int64_t ldx, int T_steps, int V, const T* __restrict__ attrs,
                                      int64_t lda, int A, T* __restrict__ out, int64_t ldo, int W, int n_rows) {
  const int per_row = W / Q;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * per_row) return;
  const int n = (int)(i / per_row), c = (int)(i % per_row) * Q;
  Vec<T, Q> v{};
  if (c < T_steps * V) {
    const int t = c / V, cv = c % V;  // V % Q == 0: a group never straddles two time steps
    v = *reinterpret_cast<const Vec<T, Q>*>(x + t * ld_t + (int64_t)n * ldx + cv);
  } else if (c < T_steps * V + A) {
    v = *reinterpret_cast<const Vec<T, Q>*>(attrs + (int64_t)n * lda + (c - T_steps * V));
  }
  *reinterpret_cast<Vec<T, Q>*>(out + (int64_t)n * ldo + c) = v;
}

// x * m + a with the two roundings of torch's `x.mul_(m).add_(a)` (no FMA contraction): bit-equal to the reference's
// InputNormalizer.transform in fp32 (preprocessing/normalizer.py:154-190).
__device__ __forceinline__ float mul_then_add(float x, float m, float a) {
#pragma clang fp contract(off)
  const float t = x * m;
  return t + a;
}

// x * m as an fp32 VALUE, whatever is done with it next.  A product that is then converted to fp16 is otherwise selected as one
// v_fma_mixlo_f16 (with or without fp contraction), which rounds the exact product to fp16 once; torch rounds it to fp32 first, and
// the two differ where that fp32 value is a tie between two fp16 values (one element in 2^14).  The empty asm pins the product in a
// VGPR, so the conversion is an instruction of its own.
__device__ __forceinline__ float mul_f32(float x, float m) {
  float t = x * m;
  asm("" : "+v"(t));
  return t;
}

// y[r, c] = x[r, c] * mul[c] + add[c] (inverse = 0) or (x[r, c] - add[c]) / mul[c] (inverse = 1): InputNormalizer.transform /
// inverse_transform as a stand-alone kernel (preprocessing/normalizer.py:154-252); may run in place (y == x).
template <typename T>
__global__ void affine_columns_kernel(const T* __restrict__ x, int64_t ldx, T* __restrict__ y, int64_t ldy, const float* __restrict__ mul,
                                      const float* __restrict__ add, int inverse, int n_rows, int V) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * V) return;
  const int r = (int)(i / V), c = (int)(i % V);
  const float v = to_float(x[(int64_t)r * ldx + c]);
  float o;
  if (inverse) {
    o = to_float(from_float<T>(v - add[c])) / mul[c];  // subtract_ then div_: two roundings in T like torch's in-place ops
  } else {
    if constexpr (sizeof(T) == 4) {
      o = mul_then_add(v, mul[c], add[c]);  // two fp32 roundings, never an FMA
    } else {
      o = to_float(from_float<T>(mul_f32(v, mul[c])));  // mul_ rounds to T (through fp32, as torch does), then add_ rounds again
      o = o + add[c];
    }
  }
  y[(int64_t)r * ldy + c] = from_float<T>(o);
}

// ---- imputers (reference preprocessing/imputer.py) ------------------------------------------------------------------------------------
// The imputation program is a per-column table over the V input columns: kind_src int32 [V][2] = (kind, source column), value fp32 [V].
// kind 0: the column is not imputed; 1: a NaN becomes value[c] (rounded to the data dtype on the host, so the fp32 entry is exact);
// 2: a NaN becomes the element of column `source` at the same position (CopyImputer).  A source column is never itself imputed (the host
// refuses such programs), so an in-place launch reads no element another thread writes.

// Stand-alone imputer over x [batch, time, ensemble, grid, V] (element strides ld_b, ld_t, ld_e, ld_n; columns contiguous): the NaN test of
// an element is isnan of ensemble member 0 at the same (batch, time, grid, column) - imputer.py:116-134 keeps the first member's locations -
// and applies to every member.  A thread owns one (batch, time, grid, column) and walks the members, member 0's test read before any store,
// so y may alias x.  mask (may be null): bool [batch, grid, V], the NaN locations of time step 0, one byte per element.
template <typename T>
__global__ void impute_columns_kernel(const T* x, int64_t ld_b, int64_t ld_t, int64_t ld_e, int64_t ld_n, T* y, int64_t yd_b,  // (y may be x)
                                      int64_t yd_t, int64_t yd_e, int64_t yd_n, const int32_t* __restrict__ kind_src, const float* __restrict__ value,
                                      uint8_t* __restrict__ mask, int B, int T_steps, int E, int N, int V) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T_steps * N * V) return;
  const int c = (int)(i % V);
  const int n = (int)((i / V) % N);
  const int t = (int)((i / ((int64_t)V * N)) % T_steps);
  const int b = (int)(i / ((int64_t)V * N * T_steps));
  const T* xr = x + b * ld_b + t * ld_t + (int64_t)n * ld_n;
  T* yr = y + b * yd_b + t * yd_t + (int64_t)n * yd_n;
  const int kind = kind_src[2 * c], src = kind_src[2 * c + 1];
  const float val = value[c];
  const bool is_nan = isnan(to_float(xr[c]));
  if (mask != nullptr && t == 0) mask[((int64_t)b * N + n) * V + c] = is_nan ? 1 : 0;
  if (kind == 0 && x == y) return;
  for (int e = 0; e < E; ++e) {
    const T* xe = xr + e * ld_e;
    const T in = xe[c];
    yr[e * yd_e + c] = (kind == 0 || !is_nan) ? in : from_float<T>(kind == 1 ? val : to_float(xe[src]));
  }
}

// BaseImputer.inverse_transform (imputer.py:243-279): y[b, m, n, c] = NaN where mask[b, n, src_of[c]] (src_of[c] >= 0), else x[b, m, n, c];
// x / y [batch, M, grid, V_out] contiguous rows of ldx / ldy elements, mask bool [batch, grid, ldm].  In place (y == x) only the restored
// elements are stored.
template <typename T>
__global__ void restore_nan_columns_kernel(const T* x, int64_t ldx, T* y, int64_t ldy, const uint8_t* __restrict__ mask,  // (y may be x)
                                           int64_t ldm, int n_mask_cols, const int32_t* __restrict__ src_of, int B, int M, int N, int V) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * M * N * V) return;
  const int c = (int)(i % V);
  const int64_t row = i / V;
  const int n = (int)(row % N);
  const int b = (int)(row / ((int64_t)N * M));
  const int s = src_of[c];
  const bool hit = s >= 0 && s < n_mask_cols && mask[((int64_t)b * N + n) * ldm + s] != 0;
  if (hit)
    y[row * ldy + c] = from_float<T>(__builtin_nanf(""));
  else if (x != y)
    y[row * ldy + c] = x[row * ldx + c];
}

// ---- remapper (reference preprocessing/remapper.py; the maps are in remap_core.h) ----------------------------------------------------
// Stand-alone Remapper.transform / inverse_transform over x [batch, time, ensemble, grid, V] (element strides ld_b .. ld_n, columns
// contiguous; y likewise and may alias x).  The program is a per-column table: op_flags int32 [V][2] = (RemapOp, flags), par fp32 [V][4].
// A thread owns one element of one ACTIVE column: `active` int32 [n_active] lists the columns whose op is not REMAP_NONE, so an in-place
// launch neither loads nor stores the others (2-4 of ~80 columns in a typical configuration); active == nullptr walks all V columns (out
// of place, where every element is copied).  viol (may be null): int32 [V], entry c counts the elements of column c that fail the reference's
// domain assertion, with an ordinary atomic add - rare by construction, the host reads it once after the launch.
template <typename T>
__global__ void remap_columns_kernel(const T* x, int64_t ld_b, int64_t ld_t, int64_t ld_e, int64_t ld_n, T* y, int64_t yd_b, int64_t yd_t,  // (y may be x)
                                     int64_t yd_e, int64_t yd_n, const int32_t* __restrict__ op_flags, const float* __restrict__ par,
                                     const int32_t* __restrict__ active, int n_active, int32_t* viol, int B, int T_steps, int E, int N, int V) {
  const int per_row = active != nullptr ? n_active : V;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)B * T_steps * E * N * per_row) return;
  const int a = (int)(i % per_row);
  int64_t row = i / per_row;
  const int n = (int)(row % N);
  row /= N;
  const int e = (int)(row % E);
  row /= E;
  const int t = (int)(row % T_steps), b = (int)(row / T_steps);
  const int c = active != nullptr ? active[a] : a;
  const int2 of = reinterpret_cast<const int2*>(op_flags)[c];
  const float4 p = reinterpret_cast<const float4*>(par)[c];
  const T in = x[b * ld_b + t * ld_t + e * ld_e + (int64_t)n * ld_n + c];
  bool bad = false;
  const T out = of.x == REMAP_NONE ? in : from_float<T>(remap_apply<T>(to_float(in), of.x, of.y, p.x, p.y, p.z, p.w, bad));
  y[b * yd_b + t * yd_t + e * yd_e + (int64_t)n * yd_n + c] = out;
  if (bad && viol != nullptr) atomicAdd(viol + c, 1);
}

// ---- the staged chain [imputer]? [Remapper]? [InputNormalizer]? on the way into the model ----------------------------------------------
// One raw element v = row[cv] of the chain.  IMPUTE: a NaN is replaced as the program entry of its column says (one 8-byte load; the value
// is read only where a NaN is replaced, the copy source from the same row, i.e. the same time step).  REMAP: the forward map of the column
// with the roundings of the RAW dtype TI (the module runs on the raw tensor).  Then x * mul + add with two fp32 roundings (mul == nullptr:
// no normaliser).  Nothing is counted here: the chain's one-off first-batch check runs the member modules, with their assertion, on a copy.
template <typename TI, bool IMPUTE, bool REMAP>
__device__ __forceinline__ float edge_chain_one(float v, const TI* __restrict__ row, int cv, const int32_t* __restrict__ kind_src,
                                                const float* __restrict__ value, const int32_t* __restrict__ op_flags, const float* __restrict__ par,
                                                const float* __restrict__ mul, const float* __restrict__ add) {
  if constexpr (IMPUTE) {
    if (isnan(v)) {
      const int2 ks = reinterpret_cast<const int2*>(kind_src)[cv];
      if (ks.x != 0) v = ks.x == 1 ? value[cv] : to_float(row[ks.y]);
    }
  }
  if constexpr (REMAP) {
    const int2 of = reinterpret_cast<const int2*>(op_flags)[cv];
    if (of.x != REMAP_NONE) {
      const float4 p = reinterpret_cast<const float4*>(par)[cv];
      bool bad = false;
      v = remap_apply<TI>(v, of.x, of.y, p.x, p.y, p.z, p.w, bad);
    }
  }
  if (mul != nullptr) v = mul_then_add(v, mul[cv], add[cv]);
  return v;
}

// Input assembly with the chain on every time / variable column (scope row f4): as assemble_input_kernel, one element per thread, fp32
// arithmetic, one pass over the input.  The input may be wider than the model dtype (fp32 data into a 16-bit model): TI -> fp32 -> TO.
// IMPUTE: the NaN locations of step 0 of the RAW input go to mask bool [N][ldm] in the same pass, as the imputer's own transform records them.
template <typename TI, typename TO, bool IMPUTE, bool REMAP>
__global__ void assemble_input_chain_kernel(const TI* __restrict__ x, int64_t ld_t, int64_t ldx, int T_steps, int V, const int32_t* __restrict__ kind_src,
                                            const float* __restrict__ value, uint8_t* __restrict__ mask, int64_t ldm,
                                            const int32_t* __restrict__ op_flags, const float* __restrict__ par, const float* __restrict__ mul,
                                            const float* __restrict__ add, const TO* __restrict__ attrs, int64_t lda, int A, TO* __restrict__ out,
                                            int64_t ldo, int W, int n_rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * W) return;
  const int n = (int)(i / W), c = (int)(i % W);
  float v = 0.f;
  if (c < T_steps * V) {
    const int t = c / V, cv = c % V;
    const TI* xr = x + t * ld_t + (int64_t)n * ldx;
    v = to_float(xr[cv]);
    if constexpr (IMPUTE) {
      if (t == 0) mask[(int64_t)n * ldm + cv] = isnan(v) ? 1 : 0;
    }
    v = edge_chain_one<TI, IMPUTE, REMAP>(v, xr, cv, kind_src, value, op_flags, par, mul, add);
  } else if (c < T_steps * V + A) {
    v = to_float(attrs[(int64_t)n * lda + (c - T_steps * V)]);
  }
  out[(int64_t)n * ldo + c] = from_float<TO>(v);
}

// The same for 16-bit outputs whose width is a multiple of 8: a thread produces 8 consecutive columns and stores them as one 16-byte
// vector (the GNN embeddings' zero-padded [M, 128] inputs are mostly padding: 25 us -> a few at 81 840 rows).  IMPUTE: a group of 8
// columns that lies within step 0 owns 8 consecutive mask bytes: they leave as two 4-byte stores where the mask rows allow it
// (ldm % 4 == 0, base 4-byte aligned - then n * ldm + c0 is a multiple of 4), else byte by byte.
template <typename TI, typename TO, bool IMPUTE, bool REMAP>
__global__ void assemble_input_chain_vec8_kernel(const TI* __restrict__ x, int64_t ld_t, int64_t ldx, int T_steps, int V,
                                                 const int32_t* __restrict__ kind_src, const float* __restrict__ value, uint8_t* __restrict__ mask,
                                                 int64_t ldm, const int32_t* __restrict__ op_flags, const float* __restrict__ par,
                                                 const float* __restrict__ mul, const float* __restrict__ add, const TO* __restrict__ attrs, int64_t lda,
                                                 int A, TO* __restrict__ out, int64_t ldo, int W, int n_rows) {
  const int per_row = W >> 3;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * per_row) return;
  const int n = (int)(i / per_row), c0 = (int)(i % per_row) << 3;
  Vec<TO, 8> o;
  if constexpr (!IMPUTE && !REMAP) {
    if (T_steps == 1 && A == 0) {  // a plain cast + zero-pad of [N, V] rows (the GNN embeddings' inputs): no divisions
      const TI* xr = x + (int64_t)n * ldx;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        float v = c < V ? to_float(xr[c]) : 0.f;
        if (mul != nullptr && c < V) v = mul_then_add(v, mul[c], add[c]);
        o.v[j] = from_float<TO>(v);
      }
      *reinterpret_cast<Vec<TO, 8>*>(out + (int64_t)n * ldo + c0) = o;
      return;
    }
  }
  bool packed = false;
  if constexpr (IMPUTE) packed = c0 + 8 <= V && (ldm & 3) == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  uint32_t bits[2] = {0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c0 + j;
    float v = 0.f;
    if (c < T_steps * V) {
      const int t = c / V, cv = c % V;
      const TI* xr = x + t * ld_t + (int64_t)n * ldx;
      v = to_float(xr[cv]);
      if constexpr (IMPUTE) {
        const bool is_nan = isnan(v);
        if (packed)
          bits[j >> 2] |= (is_nan ? 1u : 0u) << (8 * (j & 3));
        else if (t == 0)
          mask[(int64_t)n * ldm + cv] = is_nan ? 1 : 0;
      }
      v = edge_chain_one<TI, IMPUTE, REMAP>(v, xr, cv, kind_src, value, op_flags, par, mul, add);
    } else if (c < T_steps * V + A) {
      v = to_float(attrs[(int64_t)n * lda + (c - T_steps * V)]);
    }
    o.v[j] = from_float<TO>(v);
  }
  if (packed) {
    uint32_t* m = reinterpret_cast<uint32_t*>(mask + (int64_t)n * ldm + c0);
    m[0] = bits[0];
    m[1] = bits[1];
  }
  *reinterpret_cast<Vec<TO, 8>*>(out + (int64_t)n * ldo + c0) = o;
}

// Output assembly with the skip connection taken from the RAW input, which goes through the same chain on the fly - the counterpart of
// assemble_input_chain_kernel: out[n, v] = x_out[n, v] + (col_map[v] >= 0 ? chain(skip[n, m]) : 0), m = col_map[v], the normalised skip
// rounded to TS before the add.  x_out is in the model dtype (TM), skip and out in the caller's data dtype (TS): the reference adds the
// residual in the input's dtype (x_out.to(dtype=x.dtype), models/encoder_processor_decoder.py:145-158).
template <typename TM, typename TS, bool IMPUTE, bool REMAP>
__global__ void assemble_output_chain_kernel(const TM* __restrict__ x_out, int64_t ldx, const TS* __restrict__ skip, int64_t lds,
                                             const int32_t* __restrict__ col_map, const int32_t* __restrict__ kind_src, const float* __restrict__ value,
                                             const int32_t* __restrict__ op_flags, const float* __restrict__ par, const float* __restrict__ mul,
                                             const float* __restrict__ add, TS* __restrict__ out, int64_t ldo, int n_rows, int n_cols) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n_rows * n_cols) return;
  const int n = (int)(i / n_cols), v = (int)(i % n_cols);
  float val = to_float(from_float<TS>(to_float(x_out[(int64_t)n * ldx + v])));
  const int m = col_map[v];
  if (m >= 0) {
    const TS* sr = skip + (int64_t)n * lds;
    float sk = edge_chain_one<TS, IMPUTE, REMAP>(to_float(sr[m]), sr, m, kind_src, value, op_flags, par, nullptr, nullptr);
    if (mul != nullptr) sk = to_float(from_float<TS>(mul_then_add(sk, mul[m], add[m])));
    val += sk;
  }
  out[(int64_t)n * ldo + v] = from_float<TS>(val);
}

// ---- the output column program -------------------------------------------------------------------------------------------------------------
// All configured boundings (reference layers/bounding.py:81-307) and what follows them on the output, in ONE in-place pass: a thread owns a
// row and applies the program in order (ops: int32 [n_ops][4] = kind, column, total column, unused; params: fp32 [n_ops][2] = min / max
// or the normalised minimum).
//   LEVEL 0  kind 1 relu, 2 leaky relu, 3 relu above a minimum, 4 leaky relu above a minimum, 5 hardtanh, 6 leaky hardtanh, 7 hardtanh *
//            x[total], 8 leaky hardtanh * x[total] (slopes 0.01 as in torch / layers/activations.py:16-42), 9 de-normalisation
//            (x - p0) / p1 (preprocessing/normalizer.py:217-252)
//   LEVEL 1  and 10: NaN where mask[r, total] (BaseImputer.inverse_transform, appended after the op-9 de-normalisations; `total` is the
//            mask column)
//   LEVEL 2  and the kinds of the post-processors and the remapper's inverse.  11: p0 where row[total] == 0
//            (ConditionalZeroPostprocessor); 12: NaN where row[total] is NaN (ConditionalNaNPostprocessor) - both read the masking column
//            as the ops before them left it, so the host orders a fill OF the masking column after the fills it masks; 16 + op: the
//            RemapOp `op` (remap_core.h) with flags = ops[4 i + 3] and a third parameter as the float bits of ops[4 i + 2].
// A kind above the LEVEL leaves its column as it is; the code of the higher kinds is not in the lower instantiations, so a program of
// kinds 1..10 runs no libm code.
template <typename T, int LEVEL>
__global__ void column_program_kernel(T* __restrict__ x, int64_t ldx, int n_rows, const int32_t* __restrict__ ops, const float* __restrict__ params,
                                      int n_ops, const uint8_t* __restrict__ mask, int64_t ldm, int n_mask_cols) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  T* row = x + (int64_t)r * ldx;
  for (int i = 0; i < n_ops; ++i) {
    const int kind = ops[4 * i], col = ops[4 * i + 1], tot = ops[4 * i + 2];
    const float p0 = params[2 * i], p1 = params[2 * i + 1];
    float v = to_float(row[col]);
    auto leaky = [](float t) { return t > 0.f ? t : 0.01f * t; };
    auto lht = [&](float t) { return t < p0 ? p0 + 0.01f * (t - p0) : (t > p1 ? p1 + 0.01f * (t - p1) : t); };
    // comparisons, not fmaxf / fminf (which return the non-NaN operand): a NaN stays a NaN, as through torch.relu / hardtanh / clamp
    auto relu = [](float t) { return t < 0.f ? 0.f : t; };
    auto clamp = [&](float t) { return t < p0 ? p0 : (t > p1 ? p1 : t); };
    switch (kind) {
      case 1: v = relu(v); break;
      case 2: v = leaky(v); break;
      case 3: v = relu(v - p0) + p0; break;
      case 4: v = leaky(v - p0) + p0; break;
      case 5: v = clamp(v); break;
      case 6: v = lht(v); break;
      case 7: v = to_float(from_float<T>(clamp(v))) * to_float(row[tot]); break;
      case 8: v = to_float(from_float<T>(lht(v))) * to_float(row[tot]); break;
      case 9: v = to_float(from_float<T>(v - p0)) / p1; break;  // InputNormalizer.inverse_transform: x.subtract_(add).div_(mul) (normalizer.py:246-252)
      case 10:
        if constexpr (LEVEL >= 1) {
          if ((unsigned)tot >= (unsigned)n_mask_cols || mask[(int64_t)r * ldm + tot] == 0) continue;  // every other bit of the row stays
          v = __builtin_nanf("");
        }
        break;
      default:
        if constexpr (LEVEL >= 2) {
          if (kind == 11) {
            if (!(to_float(row[tot]) == 0.f)) continue;
            v = p0;
          } else if (kind == 12) {
            if (!isnan(to_float(row[tot]))) continue;
            v = __builtin_nanf("");
          } else if (kind >= 16) {
            bool bad = false;
            v = remap_apply<T>(v, kind - 16, ops[4 * i + 3], p0, p1, __int_as_float(tot), 0.f, bad);
          }
        }
        break;
    }
    row[col] = from_float<T>(v);
  }
}

// ---- host side of the chain entry points: every check and the route choice, once ------------------------------------------------------
// The stage tables of a chain; a group is null where the chain has no such stage.
struct ChainTables {
  const int32_t* kind_src;  // imputation program ...
  const float* value;       // ... and its values
  const int32_t* op_flags;  // remap program ...
  const float* par;         // ... and its parameters
  const float* mul;         // normaliser
  const float* add;
};

// The groups are complete, the tables the kernels read with 8- / 16-byte loads are aligned, and the two dtypes of the call are one of the
// pairs that are built: the model dtype with itself or with fp32 data (`data`: the dtype of the raw side, `model`: of the model's side).
static int check_chain(const char* what, const ChainTables& s, anemoi_dtype_t data, anemoi_dtype_t model, const char* pair) {
  auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  ANEMOI_REQUIRE((s.mul == nullptr) == (s.add == nullptr), "%s: col_mul and col_add go together", what);
  ANEMOI_REQUIRE((s.kind_src == nullptr) == (s.value == nullptr), "%s: the imputation program and its values go together", what);
  ANEMOI_REQUIRE((s.op_flags == nullptr) == (s.par == nullptr), "%s: the remap program and its parameters go together", what);
  ANEMOI_REQUIRE(!misaligned(s.op_flags, 8) && !misaligned(s.par, 16) && !misaligned(s.kind_src, 8),
                 "%s: the program tables must be 8- / 16-byte aligned", what);
  ANEMOI_REQUIRE(data == model || data == ANEMOI_F32, "%s: %s is in the model dtype or fp32", what, pair);
  return ANEMOI_OK;
}

// (imputer present, remapper present) -> f(bool_constant, bool_constant)
template <typename F>
static void dispatch_stages(const ChainTables& s, F&& f) {
  dispatch_one_of<0, 1, 2, 3>((s.kind_src != nullptr ? 1 : 0) + (s.op_flags != nullptr ? 2 : 0), [&](auto S) {
    f(std::bool_constant<(S() & 1) != 0>{}, std::bool_constant<(S() & 2) != 0>{});
  });
}

static dim3 grid_for(int64_t n_threads) { return dim3((unsigned)((n_threads + 255) / 256)); }

// TI: the raw input's type, TO: the model's.  A 16-bit output whose rows are whole 16-byte groups takes the 8-column kernel.
template <typename TI, typename TO>
static int assemble_input_chain_launch(const void* x, int64_t ld_t, int64_t ldx, int T_steps, int V, const ChainTables& s, uint8_t* mask, int64_t ldm,
                                       const void* attrs, int64_t lda, int A, void* out, int64_t ldo, int W, int n_rows, hipStream_t st) {
  const bool vec8 = sizeof(TO) == 2 && W % 8 == 0 && ldo % 8 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  dispatch_stages(s, [&](auto I, auto R) {
    if constexpr (sizeof(TO) == 2) {
      if (vec8) {
        hipLaunchKernelGGL((assemble_input_chain_vec8_kernel<TI, TO, I(), R()>), grid_for((int64_t)n_rows * (W / 8)), dim3(256), 0, st, (const TI*)x,
                           ld_t, ldx, T_steps, V, s.kind_src, s.value, mask, ldm, s.op_flags, s.par, s.mul, s.add, (const TO*)attrs, lda, A, (TO*)out,
                           ldo, W, n_rows);
        return;
      }
    }
    hipLaunchKernelGGL((assemble_input_chain_kernel<TI, TO, I(), R()>), grid_for((int64_t)n_rows * W), dim3(256), 0, st, (const TI*)x, ld_t, ldx,
                       T_steps, V, s.kind_src, s.value, mask, ldm, s.op_flags, s.par, s.mul, s.add, (const TO*)attrs, lda, A, (TO*)out, ldo, W, n_rows);
  });
  return check_launch(vec8 ? "assemble_input_chain_vec8_kernel" : "assemble_input_chain_kernel");
}

// TM: the model's type (x_out), TS: the raw skip's and the output's.
template <typename TM, typename TS>
static int assemble_output_chain_launch(const void* x_out, int64_t ldx, const void* x_skip, int64_t lds, const int32_t* col_map, const ChainTables& s,
                                        void* out, int64_t ldo, int n_rows, int n_cols, hipStream_t st) {
  dispatch_stages(s, [&](auto I, auto R) {
    hipLaunchKernelGGL((assemble_output_chain_kernel<TM, TS, I(), R()>), grid_for((int64_t)n_rows * n_cols), dim3(256), 0, st, (const TM*)x_out, ldx,
                       (const TS*)x_skip, lds, col_map, s.kind_src, s.value, s.op_flags, s.par, s.mul, s.add, (TS*)out, ldo, n_rows, n_cols);
  });
  return check_launch("assemble_output_chain_kernel");
}

}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_assemble_output(const void* x_out, int64_t ldx, const void* x_skip, int64_t lds, const int32_t* col_map, void* out,
                                      int64_t ldo, int32_t n_rows, int32_t n_cols, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && n_cols > 0 && ldx >= n_cols && ldo >= n_cols, "assemble_output: bad sizes");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x_out && x_skip && col_map && out, "assemble_output: null pointer");
  const size_t es = dtype == ANEMOI_F32 ? 4 : 2;
  const bool q4 = n_cols % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && reinterpret_cast<uintptr_t>(x_out) % (4 * es) == 0 &&
                  reinterpret_cast<uintptr_t>(out) % (4 * es) == 0;
  const int64_t n = (int64_t)n_rows * (n_cols / (q4 ? 4 : 1));
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    dispatch_one_of<1, 4>(q4 ? 4 : 1, [&](auto Q) {
      hipLaunchKernelGGL((assemble_output_kernel<T, Q()>), grid, block, 0, st, (const T*)x_out, ldx, (const T*)x_skip, lds, col_map, (T*)out,
                         ldo, n_rows, n_cols);
    });
    return check_launch("assemble_output_kernel");
  });
}

extern "C" int anemoi_assemble_input(const void* x, int64_t ld_t, int64_t ldx, int32_t T_steps, int32_t V, const void* attrs, int64_t lda,
                                     int32_t A, void* out, int64_t ldo, int32_t W, int32_t n_rows, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && T_steps > 0 && V > 0 && A >= 0 && W >= T_steps * V + A && ldo >= W && ldx >= V && (A == 0 || lda >= A),
                 "assemble_input: bad sizes");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && out && (A == 0 || attrs), "assemble_input: null pointer");
  const size_t es = dtype == ANEMOI_F32 ? 4 : 2;
  auto al = [&](const void* p, int q) { return p == nullptr || reinterpret_cast<uintptr_t>(p) % (q * es) == 0; };
  const bool q4 = V % 4 == 0 && A % 4 == 0 && W % 4 == 0 && ld_t % 4 == 0 && ldx % 4 == 0 && lda % 4 == 0 && ldo % 4 == 0 && al(x, 4) &&
                  al(attrs, 4) && al(out, 4);
  const int q = q4 ? 4 : 1;
  const int64_t n = (int64_t)n_rows * (W / q);
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    dispatch_one_of<1, 4>(q, [&](auto Q) {
      hipLaunchKernelGGL((assemble_input_kernel<T, Q()>), grid, block, 0, st, (const T*)x, ld_t, ldx, T_steps, V, (const T*)attrs, lda, A,
                         (T*)out, ldo, W, n_rows);
    });
    return check_launch("assemble_input_kernel");
  });
}

// The two chain entry points take TWO dtypes and build exactly the pairs a caller can ask for - the model dtype with itself or with fp32
// data - so the second type is chosen inside one dispatch_dtype instead of by nesting two.
extern "C" int anemoi_assemble_input_chain(const void* x, anemoi_dtype_t x_dtype, int64_t ld_t, int64_t ldx, int32_t T_steps, int32_t V,
                                           const int32_t* kind_src, const float* value, void* mask, int64_t ldm, const int32_t* op_flags,
                                           const float* par, const float* col_mul, const float* col_add, const void* attrs, int64_t lda, int32_t A,
                                           void* out, int64_t ldo, int32_t W, int32_t n_rows, anemoi_dtype_t dtype, void* stream) {
  const char* what = "assemble_input_chain";
  const ChainTables s{kind_src, value, op_flags, par, col_mul, col_add};
  ANEMOI_REQUIRE(n_rows >= 0 && T_steps > 0 && V > 0 && A >= 0 && W >= T_steps * V + A && ldo >= W && ldx >= V && (A == 0 || lda >= A),
                 "%s: bad sizes", what);
  if (const int rc = check_chain(what, s, x_dtype, dtype, "the input")) return rc;
  ANEMOI_REQUIRE((kind_src == nullptr) == (mask == nullptr), "%s: the imputation program, its values and the mask go together", what);
  ANEMOI_REQUIRE(mask == nullptr || ldm >= V, "%s: bad mask sizes", what);
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && out && (A == 0 || attrs), "%s: null pointer", what);
  return dispatch_dtype(dtype, [&](auto t) {
    using TO = typename decltype(t)::type;
    auto launch = x_dtype == ANEMOI_F32 ? &assemble_input_chain_launch<float, TO> : &assemble_input_chain_launch<TO, TO>;
    return launch(x, ld_t, ldx, T_steps, V, s, (uint8_t*)mask, ldm, attrs, lda, A, out, ldo, W, n_rows, as_stream(stream));
  });
}

extern "C" int anemoi_assemble_output_chain(const void* x_out, int64_t ldx, anemoi_dtype_t model_dtype, const void* x_skip, int64_t lds,
                                            const int32_t* col_map, const int32_t* kind_src, const float* value, const int32_t* op_flags,
                                            const float* par, const float* col_mul, const float* col_add, void* out, int64_t ldo, int32_t n_rows,
                                            int32_t n_cols, anemoi_dtype_t dtype, void* stream) {
  const char* what = "assemble_output_chain";
  const ChainTables s{kind_src, value, op_flags, par, col_mul, col_add};
  ANEMOI_REQUIRE(n_rows >= 0 && n_cols > 0 && ldx >= n_cols && ldo >= n_cols, "%s: bad sizes", what);
  if (const int rc = check_chain(what, s, dtype, model_dtype, "the output")) return rc;
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x_out && x_skip && col_map && out, "%s: null pointer", what);
  return dispatch_dtype(model_dtype, [&](auto t) {
    using TM = typename decltype(t)::type;
    auto launch = dtype == ANEMOI_F32 ? &assemble_output_chain_launch<TM, float> : &assemble_output_chain_launch<TM, TM>;
    return launch(x_out, ldx, x_skip, lds, col_map, s, out, ldo, n_rows, n_cols, as_stream(stream));
  });
}

extern "C" int anemoi_affine_columns(const void* x, int64_t ldx, void* y, int64_t ldy, const float* col_mul, const float* col_add,
                                     int32_t inverse, int32_t n_rows, int32_t V, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && V > 0 && ldx >= V && ldy >= V, "affine_columns: bad sizes");
  if (n_rows == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && y && col_mul && col_add, "affine_columns: null pointer");
  const int64_t n = (int64_t)n_rows * V;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((affine_columns_kernel<T>), grid, block, 0, st, (const T*)x, ldx, (T*)y, ldy, col_mul, col_add, inverse, n_rows, V);
    return check_launch("affine_columns_kernel");
  });
}

extern "C" int anemoi_impute_columns(const void* x, int64_t ld_b, int64_t ld_t, int64_t ld_e, int64_t ld_n, void* y, int64_t yd_b, int64_t yd_t,
                                     int64_t yd_e, int64_t yd_n, const int32_t* kind_src, const float* value, void* mask, int32_t B, int32_t T_steps,
                                     int32_t E, int32_t N, int32_t V, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(B >= 0 && T_steps >= 0 && E >= 0 && N >= 0 && V > 0 && ld_n >= V && yd_n >= V, "impute_columns: bad sizes");
  const int64_t n = (int64_t)B * T_steps * N * V;
  if (n == 0 || E == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && y && kind_src && value, "impute_columns: null pointer");
  ANEMOI_REQUIRE((n + 255) / 256 <= 0x7fffffffLL, "impute_columns: too many elements for one launch");
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((impute_columns_kernel<T>), grid, block, 0, st, (const T*)x, ld_b, ld_t, ld_e, ld_n, (T*)y, yd_b, yd_t, yd_e, yd_n, kind_src,
                       value, (uint8_t*)mask, B, T_steps, E, N, V);
    return check_launch("impute_columns_kernel");
  });
}

extern "C" int anemoi_restore_nan_columns(const void* x, int64_t ldx, void* y, int64_t ldy, const void* mask, int64_t ldm, int32_t n_mask_cols,
                                          const int32_t* src_of, int32_t B, int32_t M, int32_t N, int32_t V, anemoi_dtype_t dtype, void* stream) {
  ANEMOI_REQUIRE(B >= 0 && M >= 0 && N >= 0 && V > 0 && ldx >= V && ldy >= V && n_mask_cols > 0 && ldm >= n_mask_cols, "restore_nan_columns: bad sizes");
  const int64_t n = (int64_t)B * M * N * V;
  if (n == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && y && mask && src_of, "restore_nan_columns: null pointer");
  ANEMOI_REQUIRE((n + 255) / 256 <= 0x7fffffffLL, "restore_nan_columns: too many elements for one launch");
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((restore_nan_columns_kernel<T>), grid, block, 0, st, (const T*)x, ldx, (T*)y, ldy, (const uint8_t*)mask, ldm, n_mask_cols, src_of, B, M, N, V);
    return check_launch("restore_nan_columns_kernel");
  });
}

extern "C" int anemoi_remap_columns(const void* x, int64_t ld_b, int64_t ld_t, int64_t ld_e, int64_t ld_n, void* y, int64_t yd_b, int64_t yd_t,
                                    int64_t yd_e, int64_t yd_n, const int32_t* op_flags, const float* par, const int32_t* active, int32_t n_active,
                                    int32_t* violations, int32_t B, int32_t T_steps, int32_t E, int32_t N, int32_t V, anemoi_dtype_t dtype,
                                    void* stream) {
  ANEMOI_REQUIRE(B >= 0 && T_steps >= 0 && E >= 0 && N >= 0 && V > 0 && ld_n >= V && yd_n >= V, "remap_columns: bad sizes");
  ANEMOI_REQUIRE(n_active >= 0 && n_active <= V, "remap_columns: n_active must lie in [0, V]");
  ANEMOI_REQUIRE(active != nullptr || x != y || n_active == V, "remap_columns: an in-place launch takes the list of active columns");
  const int64_t n = (int64_t)B * T_steps * E * N * (active != nullptr ? n_active : V);
  if (n == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && y && op_flags && par, "remap_columns: null pointer");
  ANEMOI_REQUIRE((reinterpret_cast<uintptr_t>(op_flags) & 7) == 0 && (reinterpret_cast<uintptr_t>(par) & 15) == 0,
                 "remap_columns: the program tables must be 8- / 16-byte aligned");
  ANEMOI_REQUIRE((n + 255) / 256 <= 0x7fffffffLL, "remap_columns: too many elements for one launch");
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    hipLaunchKernelGGL((remap_columns_kernel<T>), grid, block, 0, st, (const T*)x, ld_b, ld_t, ld_e, ld_n, (T*)y, yd_b, yd_t, yd_e, yd_n, op_flags, par,
                       active, n_active, violations, B, T_steps, E, N, V);
    return check_launch("remap_columns_kernel");
  });
}

// LEVEL (see column_program_kernel): 2 where the host built the tables with extended kinds, else 1 with a mask, else 0.
extern "C" int anemoi_column_program(void* x, int64_t ldx, int32_t n_rows, int32_t n_cols, const int32_t* ops, const float* params, int32_t n_ops,
                                     const void* mask, int64_t ldm, int32_t n_mask_cols, int32_t n_nan_ops, int32_t extended, anemoi_dtype_t dtype,
                                     void* stream) {
  ANEMOI_REQUIRE(n_rows >= 0 && n_cols > 0 && ldx >= n_cols && n_ops >= 0 && n_nan_ops >= 0 && n_nan_ops <= n_ops, "column_program: bad sizes");
  ANEMOI_REQUIRE(n_nan_ops == 0 || mask != nullptr, "column_program: the program has ops of kind 10 (NaN where mask) but no mask was given");
  ANEMOI_REQUIRE(mask == nullptr ? n_mask_cols == 0 : (n_mask_cols > 0 && ldm >= n_mask_cols), "column_program: bad mask sizes");
  if (n_rows == 0 || n_ops == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(x && ops && params, "column_program: null pointer");
  const dim3 grid((n_rows + 255) / 256), block(256);
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto t) {
    using T = typename decltype(t)::type;
    dispatch_one_of<0, 1, 2>(extended ? 2 : (mask != nullptr ? 1 : 0), [&](auto L) {
      hipLaunchKernelGGL((column_program_kernel<T, L()>), grid, block, 0, st, (T*)x, ldx, n_rows, ops, params, n_ops, (const uint8_t*)mask, ldm,
                         n_mask_cols);
    });
    return check_launch("column_program_kernel");
  });
}
