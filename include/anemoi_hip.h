/*
 * anemoi_hip.h — C ABI of libanemoi_hip.so: the MI355X (gfx950) kernels behind the
 * anemoi-models encoder-processor-decoder hot path.
 *
 * The reference (ecmwf/anemoi-core) is pure Python: it has no FFI of its own.  Its kernel boundary
 * is the registered PyTorch op  anemoi::graph_transformer_attention(q,k,v,e,row,colptr,...)
 * (models/src/anemoi/models/triton/gt.py:390-428) plus the torch.nn layers chosen through
 * ``layer_kernels`` (models/src/anemoi/models/layers/utils.py:87-142).  Each entry point below names
 * the reference interface it replaces.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *  - plain pointers and sizes only; all pointers are DEVICE pointers unless stated otherwise;
 *  - row-major matrices with an explicit leading dimension ``ld*`` counted in ELEMENTS;
 *  - ``dtype`` selects the storage type of every floating tensor of the call (accumulation is
 *    always fp32); indices are int32 (the reference uses int64 at its op boundary, gt.py:413-414,
 *    the host wrapper converts once because the graph is static; N, M < 2^31);
 *  - ``stream`` is a hipStream_t passed as void*; kernels are enqueued, never synchronised;
 *  - return value 0 = success, otherwise a negative ANEMOI_E_* code; anemoi_hip_last_error()
 *    returns a thread-local message.  Nothing is allocated or freed by the library, except the
 *    peer-exchange arenas of anemoi_peer_alloc / anemoi_peer_free (memory other PROCESSES map
 *    through hipIpc cannot come from the caller's caching allocator).
 */
#ifndef ANEMOI_HIP_H
#define ANEMOI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (The EDM diffusion entries - anemoi_noise_cond_fwd, anemoi_transport_assemble_input, anemoi_edm_output, anemoi_edm_update - were added at
 * 25 without a bump: they only add entry points, every earlier signature keeps its meaning.  The same holds for their backward entries -
 * anemoi_noise_cond_bwd (+ _workspace_bytes), anemoi_transport_assemble_input_bwd, anemoi_edm_output_bwd - added at 26.) */
#define ANEMOI_HIP_ABI_VERSION 26

typedef enum { ANEMOI_F32 = 0, ANEMOI_BF16 = 1, ANEMOI_F16 = 2 } anemoi_dtype_t;
typedef enum { ANEMOI_ACT_NONE = 0, ANEMOI_ACT_GELU = 1 } anemoi_act_t;

#define ANEMOI_OK 0
#define ANEMOI_E_INVALID (-1)   /* bad argument (shape, dtype, alignment, null pointer) */
#define ANEMOI_E_UNSUPPORTED (-2)
#define ANEMOI_E_LAUNCH (-3)    /* hipGetLastError() != hipSuccess after the launch */

int anemoi_hip_abi_version(void);
const char* anemoi_hip_last_error(void);

/* Fused graph-transformer edge attention, forward.
 * Replaces: anemoi::graph_transformer_attention / _gt_fwd (triton/gt.py:81-179, 390-428) and
 * GraphTransformerConv (layers/conv.py:84-147).
 *   for every destination node d, head h, over the in-edges e=(s->d) in CSC order:
 *     score = <q[d,h,:], k[s,h,:] + E[e,h,:]> / sqrt(C);  a = softmax_e(score)
 *     out[d,h,:] = sum_e a * (v[s,h,:] + E[e,h,:])  (+ addend[d,h,:] if addend != NULL)
 *     lse[d,h]   = max + log(sum exp)               (if lse != NULL; 0 for empty d)
 * q,out,addend: [n_dst, H*C]; k,v: [n_src, H*C]; e: [M, H*C] in CSC (dst-sorted) order or NULL
 * (no edge term); row[M] = source id per edge; colptr[n_dst+1].  Zero-in-degree d -> out = addend or 0. */
int anemoi_gt_attention_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                            const void* e, int64_t lde, const int32_t* row, const int32_t* colptr,
                            const void* addend, int64_t ldadd, void* out, int64_t ldo, float* lse,
                            int32_t n_dst, int32_t n_src, int32_t H, int32_t C, anemoi_dtype_t dtype, void* stream);

/* Backward of the op above (materialised E).
 * Replaces: anemoi::graph_transformer_attention_backward = _gt_bwd_dst_pass + _gt_bwd_src_pass (triton/gt.py:182-376,
 * 447-492) and its autograd registration (triton/gt.py:526-556).
 *   out, lse: the forward's results; d_out: gradient of out [n_dst, H*C];
 *   row/colptr: CSC as in the forward; rowptr[n_src+1], edge_ids[M] (CSC edge ids grouped by source), edge_dst[M]
 *   (destination of every CSC edge): the reverse CSR of the same graph (triton/utils.py:25-70);
 *   dq [n_dst, H*C], dk, dv [n_src, H*C], de [M, H*C] (CSC order): outputs, every row written (zeros where a node has no
 *   edges);  p_ws, ds_ws: fp32 workspace [M, H] each (per-edge softmax weight and score gradient, handed from the
 *   destination pass to the source pass).  Deterministic: no atomics. */
int anemoi_gt_attention_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                            const void* e, int64_t lde, const void* out, int64_t ldo, const float* lse,
                            const void* d_out, int64_t lddo, const int32_t* row, const int32_t* colptr,
                            const int32_t* rowptr, const int32_t* edge_ids, const int32_t* edge_dst,
                            void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, void* de, int64_t ldde,
                            float* p_ws, float* ds_ws, int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t H, int32_t C,
                            anemoi_dtype_t dtype, void* stream);

/* The two ops above with DROPOUT on the softmax weights (training mode of the reference's conv: layers/conv.py:145,
 * `alpha = dropout(alpha, p, training)` after the segment softmax): out[d] = sum_e c_e alpha_e (v_s + E_e) with c_e = 0 (dropped,
 * probability drop_p) or 1 / (1 - drop_p); the softmax itself (and lse) sums every edge.  The keep decision of (CSC edge, head) is
 * a pure function of (drop_seed, edge, head) - a counter-based generator, csrc/common.h: attn_dropout_scale - so the backward takes
 * the SAME (drop_p, drop_seed) and re-derives the mask instead of reading a stored one.  drop_p = 0 is the plain op, bit for bit
 * (anemoi_gt_attention_fwd / _bwd are these entry points with drop_p = 0).  anemoi_attention_dropout_mask writes c_e as fp32
 * [n_edges, H]: what a caller needs to restate the op with an explicit mask (tests/test_attention_dropout_gpu.py). */
int anemoi_gt_attention_dropout_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                    const void* e, int64_t lde, const int32_t* row, const int32_t* colptr,
                                    const void* addend, int64_t ldadd, void* out, int64_t ldo, float* lse,
                                    int32_t n_dst, int32_t n_src, int32_t H, int32_t C, float drop_p, uint64_t drop_seed,
                                    anemoi_dtype_t dtype, void* stream);
int anemoi_gt_attention_dropout_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                    const void* e, int64_t lde, const void* out, int64_t ldo, const float* lse,
                                    const void* d_out, int64_t lddo, const int32_t* row, const int32_t* colptr,
                                    const int32_t* rowptr, const int32_t* edge_ids, const int32_t* edge_dst,
                                    void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, void* de, int64_t ldde,
                                    float* p_ws, float* ds_ws, int32_t n_dst, int32_t n_src, int32_t n_edges, int32_t H, int32_t C,
                                    float drop_p, uint64_t drop_seed, anemoi_dtype_t dtype, void* stream);
int anemoi_attention_dropout_mask(float* out, int32_t n_edges, int32_t H, float drop_p, uint64_t drop_seed, void* stream);

/* Same op with ``lin_edge`` fused: E[e] = edge_attr[e] @ w_edge^T + b_edge is never materialised.
 * Replaces: lin_edge(...) + the op above (layers/block.py:623-635 + triton/gt.py:81-179).
 * edge_feat: fp32 [M, fe_pad] with fe_pad = 4*ceil((Fe+1)/4): columns [0,Fe) = edge_attr, column Fe = 1.0
 * (carries the bias), the rest 0 (anemoi_pack_edge_features);  w_packed: fp32 [H*C, fe_pad] = [w_edge | b_edge | 0]
 * (anemoi_pack_edge_weights).  Both are built once per static graph / parameter version.
 * dst_order (NULL = 0, 1, 2, ...): a permutation of the destinations giving the order in which the kernel WORKS on them (the
 * reference's kernel takes program id = destination, triton/gt.py:100); every XCD processes a contiguous eighth of it, so an
 * order that keeps mesh neighbours together keeps the gathered K|V rows in that XCD's L2.  The result does not depend on it. */
int anemoi_gt_attention_fused_edge_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                       const float* edge_feat, int32_t fe_pad, const float* w_packed,
                                       const int32_t* row, const int32_t* colptr, const int32_t* dst_order, const void* addend, int64_t ldadd,
                                       void* out, int64_t ldo, float* lse, int32_t n_dst, int32_t n_src, int32_t H,
                                       int32_t C, anemoi_dtype_t dtype, void* stream);

/* Backward of the fused-edge op (scope row f1): dq / dk / dv as anemoi_gt_attention_bwd, plus d_w_packed fp32 [H*C, fe_pad]
 * (= [d w_edge | d b_edge | .]) and, when d_edge_feat != NULL, d_edge_feat fp32 [M, fe_pad] (gradient of the edge attributes,
 * CSC order); E and dE are never materialised.  `out` / `lse`: the forward's results; when the forward ran with an addend pass the
 * same rows as `addend` (o = out - addend is formed in the kernel); `d_addend` (nullable) receives the addend's gradient (= d_out)
 * from the same pass.  Workspaces (fp32):
 * p_ws, ds_ws [M, H]; sf_ws, qg_ws [n_dst, H, 2, fe_pad] (qg_ws only with d_edge_feat); part_ws
 * [anemoi_gt_attention_fused_edge_bwd_partial_floats].  Shapes outside the fused fast path return ANEMOI_E_UNSUPPORTED (train
 * through anemoi_gt_attention_bwd with a materialised E then).  Replaces the autograd of lin_edge + the op
 * (layers/block.py:623-635, triton/gt.py:182-376). */
int64_t anemoi_gt_attention_fused_edge_bwd_partial_floats(int32_t H, int32_t C, int32_t fe_pad);
int anemoi_gt_attention_fused_edge_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                       const float* edge_feat, int32_t fe_pad, const float* w_packed, const void* out, int64_t ldo,
                                       const float* lse, const void* d_out, int64_t lddo, const int32_t* row, const int32_t* colptr,
                                       const int32_t* rowptr, const int32_t* edge_ids, const int32_t* edge_dst, void* dq,
                                       int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv, float* d_w_packed,
                                       float* d_edge_feat, float* p_ws, float* ds_ws, float* sf_ws, float* qg_ws, float* part_ws,
                                       const void* addend, int64_t ldadd, void* d_addend, int64_t lddadd, int32_t n_dst,
                                       int32_t n_src, int32_t n_edges, int32_t H, int32_t C, anemoi_dtype_t dtype, void* stream);

/* Which kernel the four edge-attention ops above run for a shape, and on what launch geometry: the decision of
 * csrc/gt_attention_plan.h, asked without launching anything.  HOST-ONLY: no HIP call, no device needed.  op: 0 anemoi_gt_attention_fwd
 * (and _dropout_fwd), 1 anemoi_gt_attention_fused_edge_fwd, 2 anemoi_gt_attention_bwd (and _dropout_bwd), 3
 * anemoi_gt_attention_fused_edge_bwd;  fe_pad is read by the fused-edge ops only.  Two facts about the operands come from the caller:
 * rows_aligned (every pointer 16-byte aligned, every leading dimension a multiple of 8 elements for the forwards and of 16 bytes for
 * the backwards - what contiguous torch tensors of these shapes satisfy) and kv_adjacent (v is the H*C columns behind k in one buffer
 * whose row offsets fit 32 bits; op 1 only).  ANEMOI_ATTN_BLOCKS_PER_CU is that of the calling process.  ANEMOI_E_UNSUPPORTED where
 * the op's entry point would refuse the shape (`out` is filled all the same).
 *   route: 0 unsupported, 1 generic kernel (one thread per row and head), 2 wave kernel (one wave64 per row);  vec, lph: channels per
 *   lane and lanes per head of the wave kernel (0 otherwise);  fe_pad, kv_adjacent: as instantiated;  lds_bytes: dynamic LDS of the
 *   forward / destination pass;  grid_dst, grid_src, grid_wgrad: workgroups of the forward or destination pass, of the backward's
 *   source pass and of the fused-edge backward's weight-gradient kernel (0: not launched). */
typedef struct {
  int32_t route, vec, lph, fe_pad, kv_adjacent, lds_bytes;
  uint32_t grid_dst, grid_src, grid_wgrad;
} anemoi_gt_attention_plan_t;
int anemoi_gt_attention_plan(int32_t op, int32_t H, int32_t C, int32_t fe_pad, int32_t n_dst, int32_t n_src, int32_t rows_aligned,
                             int32_t kv_adjacent, anemoi_dtype_t dtype, anemoi_gt_attention_plan_t* out);

/* Pack lin_edge's parameters for the fused op: out fp32 [D, fe_pad] = [w_edge [D,Fe] | b_edge [D] (or 0) | 0...]. */
int anemoi_pack_edge_weights(const void* w_edge, const void* b_edge, float* out, int32_t D, int32_t fe, int32_t fe_pad,
                             anemoi_dtype_t dtype, void* stream);

/* Pack edge attributes for the fused op: out fp32 [M, fe_pad] = [edge_attr | 1 | 0...]. */
int anemoi_pack_edge_features(const void* edge_attr, int64_t ld, float* out, int32_t M, int32_t fe, int32_t fe_pad,
                              anemoi_dtype_t dtype, void* stream);

/* LayerNorm over the last dimension (eps inside the sqrt, affine; beta may be NULL), optional fused residual:
 *   y = LayerNorm(x) * gamma + beta (+ residual).
 * Replaces: torch.nn.LayerNorm / AutocastLayerNorm via layer_kernels.LayerNorm
 * (layers/utils.py:107-121, layers/normalization.py:19-31) and the "MLP(...LayerNorm) + x" tail of the GraphConv
 * blocks (layers/block.py:391, 469).  x, y, residual: [n_rows, D]. */
int anemoi_layernorm_fwd(const void* x, int64_t ldx, const void* gamma, const void* beta, const void* residual,
                         int64_t ldr, void* y, int64_t ldy, int32_t n_rows, int32_t D, float eps, anemoi_dtype_t dtype,
                         void* stream);

/* ConditionalLayerNorm forward (layers/normalization.py:34-94): y = LN(x) * (scale[row] + 1) + shift[row]; scale / shift are
 * per-row modulation tensors [n_rows, D] (leading dimension 0 = one row for all), e.g. the two halves of one fused
 * Linear(cond).  No affine parameters of its own. */
int anemoi_cond_layernorm_fwd(const void* x, int64_t ldx, const void* scale, int64_t lds, const void* shift, int64_t ldsh,
                              void* y, int64_t ldy, int32_t n_rows, int32_t D, float eps, anemoi_dtype_t dtype, void* stream);

/* ConditionalLayerNorm forward with the modulation computed in the kernel - no [n_rows, 2D] tensor between the conditioning's two
 * Linear maps and the LayerNorm (layers/normalization.py:34-94 in one launch):
 *   y[r, :] = LN(x[r, :]) * (1 + cond[r, :] . Ws^T + bs) + (cond[r, :] . Wb^T + bb)  (+ residual[r, :])
 * cond: [n_rows, C], leading dimension ldc >= C, any element alignment (column slices allowed), C in 1 .. 32 (beyond:
 * ANEMOI_E_UNSUPPORTED - run anemoi_linear_fwd + anemoi_cond_layernorm_fwd).  w: the C-major image [C][2][D] of
 * [scale.weight ; bias.weight] (w[c][0][d] = Ws[d][c], w[c][1][d] = Wb[d][c]), bias: [2][D] = [scale.bias ; bias.bias], both
 * contiguous in the model dtype and built once per weight version.  The modulation is accumulated in fp32 and not rounded
 * to the model dtype.  D: every width anemoi_cond_layernorm_fwd accepts. */
int anemoi_cond_layernorm_proj_fwd(const void* x, int64_t ldx, const void* cond, int64_t ldc, const void* w, const void* bias,
                                   const void* residual, int64_t ldr, void* y, int64_t ldy, int32_t n_rows, int32_t D, int32_t C,
                                   float eps, anemoi_dtype_t dtype, void* stream);

/* Backward of anemoi_cond_layernorm_fwd: d_x [n_rows, D] and d_scale [n_rows, D] = d_y * x^ (per row; d_shift = d_y needs no kernel); the
 * gradients of the conditioning's two Linear maps follow from d_scale / d_shift through anemoi_linear_fwd. */
int anemoi_cond_layernorm_bwd(const void* x, int64_t ldx, const void* scale, int64_t lds, const void* d_y, int64_t lddy,
                              void* d_x, int64_t lddx, void* d_scale, int64_t ldds, int32_t n_rows, int32_t D, float eps,
                              anemoi_dtype_t dtype, void* stream);

/* Input assembly at the model edge for batch = ensemble = 1 (models/encoder_processor_decoder.py:98-143): out[n] = [x[0, n, :] | ... |
 * x[T-1, n, :] | attrs[n, :] | zeros up to W], x time slices ld_t elements apart, rows ldx apart.  Replaces the permute-copy, the cat
 * with the node attributes and the zero padding of the embedding GEMMs' K dimension. */
int anemoi_assemble_input(const void* x, int64_t ld_t, int64_t ldx, int32_t T_steps, int32_t V, const void* attrs, int64_t lda, int32_t A,
                          void* out, int64_t ldo, int32_t W, int32_t n_rows, anemoi_dtype_t dtype, void* stream);

/* Output assembly at the model edge for batch = ensemble = output steps = 1 (models/encoder_processor_decoder.py:145-163):
 * out[n, v] = x_out[n, v] + x_skip[n, col_map[v]] where col_map[v] >= 0 (the SkipConnection residual on the prognostic
 * columns), else x_out[n, v].  Replaces clone + index_select + index_add_. */
int anemoi_assemble_output(const void* x_out, int64_t ldx, const void* x_skip, int64_t lds, const int32_t* col_map, void* out,
                           int64_t ldo, int32_t n_rows, int32_t n_cols, anemoi_dtype_t dtype, void* stream);

/* LayerNorm backward.  Replaces: autograd of layer_kernels.LayerNorm (layers/utils.py:107-121).
 *   d_x [n_rows, D] (same dtype), d_gamma / d_beta fp32 [D] (either may be NULL; both NULL: no column sums);
 *   workspace: anemoi_reduce_workspace_bytes(D) bytes of fp32 scratch (per-wave partial column sums, added in a fixed
 *   order by a second kernel: deterministic, no atomics).  Statistics are recomputed from x (nothing saved by the forward).
 *   n_rows == 0 (here and in anemoi_colsum): the row pointers may be NULL, the sums are written as zeros. */
int64_t anemoi_reduce_workspace_bytes(int32_t D);
int anemoi_layernorm_bwd(const void* x, int64_t ldx, const void* gamma, const void* d_y, int64_t lddy, void* d_x,
                         int64_t lddx, float* d_gamma, float* d_beta, float* workspace, int32_t n_rows, int32_t D,
                         float eps, anemoi_dtype_t dtype, void* stream);

/* out[c] = sum_r x[r, c] in fp32 (bias gradient of torch.nn.Linear); same workspace and determinism as above. */
int anemoi_colsum(const void* x, int64_t ldx, float* out, float* workspace, int32_t n_rows, int32_t D,
                  anemoi_dtype_t dtype, void* stream);

/* d_pre = d_y * gelu'(pre), gelu'(x) = Phi(x) + x phi(x) (exact erf form; autograd of torch.nn.GELU, layers/utils.py:111). */
int anemoi_gelu_bwd(const void* pre, int64_t ldp, const void* d_y, int64_t lddy, void* d_pre, int64_t lddp,
                    int32_t n_rows, int32_t D, anemoi_dtype_t dtype, void* stream);

/* y = gelu(x), exact erf form: torch.nn.GELU as selected by `layer_kernels.Activation` (layers/utils.py:111) when it runs
 * as a stand-alone module, e.g. inside the reference's own MLP (layers/mlp.py:158-169).  The fused blocks of this package
 * apply GELU in the epilogue of the preceding GEMM instead. */
int anemoi_gelu_fwd(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t n_rows, int32_t D, anemoi_dtype_t dtype, void* stream);

/* LayerNorm folded into the GEMMs around it (inference).  For y = LN(x; gamma, beta) W^T + b:
 *     y = rstd (x (W diag gamma)^T - mean c) + d,   c = row sums of W diag(gamma),  d = W beta + b
 * so the normalisation needs only the per-row mean / rstd of x, and those come for free from the GEMM that PRODUCED x:
 *  - anemoi_linear_stats_fwd: y = x W^T + bias + residual (as anemoi_linear_fwd; residual may be NULL: the embedding in
 *    front of a mapper's LayerNorm, layers/mapper.py:556-570) and stats_out[n_rows][O/64][2] (fp32) =
 *    (sum, sum of squares) of every 64-column strip of the stored (rounded) output row.  Plain stores, one per (row, strip):
 *    no atomics, no zeroing, deterministic.  O and K multiples of 64.
 *  - anemoi_linear_lnfold_fwd: y = act(LN(x) W^T + b) from raw x [n_rows, K], w_scaled = W diag(gamma) [O, K], fp32 c, d [O]
 *    and stats_in = the producer's statistics of x (strips * 64 == K).  Partials are added in a fixed order.
 *  The pair is a two-kernel protocol with ONE tail rule on both sides (peeled_tail_rows in csrc/linear_plan.h: the "+ 2" of an
 *  icosphere's 10 * 4^r + 2 nodes): the producer may compute the rows that rule names outside its tiles and leaves their
 *  stats_out entries UNWRITTEN; the consumer never reads them - it takes the statistics of exactly those rows from the rows
 *  themselves.  Every other row has its strip sums written (ragged last tiles included).  anemoi_linear_plan tells which rows:
 *  [main_rows, n_rows) of the producer's plan.
 * Replaces the two LayerNorm launches of a GraphTransformerProcessorBlock (layer_norm_attention / layer_norm_mlp_dst,
 * layers/block.py:1237, 1271) and layer_norm_attention_src / _dest of a GraphTransformerMapperBlock (layers/block.py:979-984)
 * in the unsharded inference path.  Returns ANEMOI_E_UNSUPPORTED for shapes / alignments the
 * ring kernels do not take (the caller falls back to LayerNorm + anemoi_linear_fwd). */
int anemoi_linear_stats_fwd(const void* x, int64_t ldx, int32_t K, const void* w, int64_t ldw, const void* bias,
                            const void* residual, int64_t ldr, void* y, int64_t ldy, float* stats_out, int32_t n_rows,
                            int32_t O, anemoi_dtype_t dtype, void* stream);
int anemoi_linear_lnfold_fwd(const void* x, int64_t ldx, int32_t K, const void* w_scaled, int64_t ldw, const float* ln_c,
                             const float* ln_d, const float* stats_in, int32_t strips, float eps, anemoi_act_t act, void* y,
                             int64_t ldy, int32_t n_rows, int32_t O, anemoi_dtype_t dtype, void* stream);

/* y[n_rows, O] (fp32, ZEROED BY THE CALLER) += x[n_rows, K] @ w[O, K]^T with the reduction split into ``splits`` chunks that
 * run on different CUs and accumulate with fp32 atomics: the weight-gradient GEMM dW = dZ^T X of torch.nn.Linear's autograd
 * (small output, reduction over 10^4..10^5 rows).  16-bit operands, K a multiple of 64 * splits. */
int anemoi_linear_splitk_f32(const void* x, int64_t ldx, const void* w, int64_t ldw, float* y, int64_t ldy, int32_t n_rows,
                             int32_t O, int32_t K, int32_t splits, anemoi_dtype_t dtype, void* stream);

/* Weight gradient of torch.nn.Linear without HBM transposes: dw[o, i] = sum_r dz[r, o] * x[r, i] (16-bit operands, fp32
 * accumulation; O, I, lddz, ldx multiples of 8).  The row-major tiles are read through the LDS transpose read; the reduction is
 * split over workgroups into fp32 partial tiles in `workspace` (anemoi_linear_wgrad_workspace_bytes bytes) summed in fixed order:
 * deterministic, no atomics.  `db` (nullable, [O]) receives the bias gradient = column sums of dz, accumulated by the same kernel.
 * Autograd of block.py:623-635 / mlp.py:158-169 (scope row f1). */
int64_t anemoi_linear_wgrad_workspace_bytes(int32_t n_rows, int32_t O, int32_t I);
int anemoi_linear_wgrad(const void* dz, int64_t lddz, const void* x, int64_t ldx, void* dw, int64_t lddw, void* db, void* workspace,
                        int32_t n_rows, int32_t O, int32_t I, anemoi_dtype_t dtype, void* stream);

/* Linear layer with fused epilogue.  Replaces torch.nn.Linear (+ GELU + residual add) as used by
 * get_qkve / projection / MLP (layers/block.py:623-635,1268-1271; layers/mlp.py:158-169).
 *   y[n, o] = act( sum_k A[n,k] * w[o,k] + bias[o] + g1[idx1[n], o] + g2[idx2[n], o] ) + residual[n, o]
 * A = [x | x2] concatenated along K (x: [n_rows,K1], x2: [n_rows,K2] or NULL with K2=0);  w: [O, K1+K2]
 * row-major (torch layout);  bias, g1/idx1, g2/idx2, residual optional (NULL).  The gather-add terms
 * serve GraphConv's first edge-MLP layer (layers/conv.py:73-76: cat[x_i, x_j, e] @ W^T is split into
 * two node-level products gathered per edge and one edge-level product). */
int anemoi_linear_fwd(const void* x, int64_t ldx, int32_t K1, const void* x2, int64_t ldx2, int32_t K2, const void* w,
                      int64_t ldw, const void* bias, const void* g1, int64_t ldg1, const int32_t* idx1, const void* g2,
                      int64_t ldg2, const int32_t* idx2, const void* residual, int64_t ldr, void* y, int64_t ldy,
                      int32_t n_rows, int32_t O, anemoi_act_t act, anemoi_dtype_t dtype, void* stream);

/* Same, and the pre-activation z (the argument of GELU) is stored to y_pre as well: training keeps it for GELU's backward
 * instead of recomputing it with a second GEMM (scope row f1).  act must be GELU and the shape one of the DMA-ring GEMM shapes
 * (16-bit, K multiple of 64); otherwise ANEMOI_E_UNSUPPORTED and nothing is launched. */
int anemoi_linear_fwd_pre(const void* x, int64_t ldx, int32_t K1, const void* x2, int64_t ldx2, int32_t K2, const void* w,
                          int64_t ldw, const void* bias, const void* g1, int64_t ldg1, const int32_t* idx1, const void* g2,
                          int64_t ldg2, const int32_t* idx2, const void* residual, int64_t ldr, void* y, int64_t ldy, void* y_pre,
                          int64_t ldy_pre, int32_t n_rows, int32_t O, anemoi_act_t act, anemoi_dtype_t dtype, void* stream);

/* Which kernel the GEMM entry points above run for a shape, and how they split its rows: the decision of csrc/linear_plan.h, asked
 * without launching anything.  HOST-ONLY: no HIP call, no device needed.  role: 0 anemoi_linear_fwd, 1 anemoi_linear_fwd_pre,
 * 2 anemoi_linear_stats_fwd, 3 anemoi_linear_lnfold_fwd, 4 anemoi_linear_splitk_f32;  epilogue_bits: 1 residual, 2 gather-add, 4 GELU.
 * The operands are taken to be contiguous and 16-byte aligned (ldx = K1, ldx2 = K2, ldw = K1 + K2, every other ld = O), and the
 * environment switches are those of the calling process.  ANEMOI_E_UNSUPPORTED where the entry point itself would refuse the shape.
 *   kernel: 0 generic (VALU), 1 128 x 128 register-staged MFMA, 2 DMA ring, 3 split-wave (K split over wave groups), 4 big tile;
 *   tile_m x tile_n: the output tile; stage_k: K elements per LDS stage; mi, wr, kg, stages: the template arguments of the kernels
 *   that have them (0 otherwise); epi: the epilogue the kernel is instantiated with (1 residual, 2 gather-add, 4 GELU, 8 row
 *   statistics, 16 LayerNorm fold, 32 pre-activation store);  rows [0, main_rows) run on the tiles, [main_rows, main_rows +
 *   tail_rows) on the VALU at the end of the same kernel; a fold consumer on the small tiles takes the statistics of the rows from
 *   ln_tail_begin on from the rows themselves (INT32_MAX: of none). */
typedef struct {
  int32_t kernel, tile_m, tile_n, pingpong, stage_k, mi, wr, kg, stages, epi, main_rows, tail_rows, ln_tail_begin;
} anemoi_linear_plan_t;
int anemoi_linear_plan(int32_t role, int32_t n_rows, int32_t O, int32_t K1, int32_t K2, int32_t epilogue_bits, anemoi_dtype_t dtype,
                       anemoi_linear_plan_t* out);

/* GraphConv edge epilogue + aggregation, one pass over the dst-sorted edges (no atomics).
 * Replaces: MLP.layer_norm + "+ edge_attr" + scatter(sum) (layers/conv.py:73-81, layers/mlp.py:176-178).
 *   e_new[m,:] = LayerNorm(z[m,:]) + e_old[m,:];   agg[d,:] = sum_{m in in(d)} e_new[m,:]
 * z, e_old, e_new: [M, D]; agg: [n_dst, D]; gamma/beta: [D] (gamma NULL -> no LayerNorm). */
int anemoi_edge_ln_residual_segment_sum_fwd(const void* z, int64_t ldz, const void* e_old, int64_t lde,
                                            const void* gamma, const void* beta, float eps, const int32_t* colptr,
                                            void* e_new, int64_t ldn, void* agg, int64_t ldagg, int32_t n_dst,
                                            int32_t D, anemoi_dtype_t dtype, void* stream);

/* Row gather: out[i,:] = x[idx[i],:].  Packs the halo send buffer (distributed/primitives.py:455). */
int anemoi_gather_rows(const void* x, int64_t ldx, const int32_t* idx, void* out, int64_t ldo, int32_t n_out, int32_t D,
                       anemoi_dtype_t dtype, void* stream);

/* out[r] = sum over i in [ptr[r], ptr[r+1]) of x[ids ? ids[i] : i]  (fp32 accumulation; deterministic).
 * Adjoint of the row gathers: with ids = NULL and ptr = colptr it sums the contiguous in-edge rows of every destination,
 * with (ptr, ids) = the reverse CSR (rowptr, edge_ids) the out-edge rows of every source.  Replaces: autograd of the
 * x_i / x_j index_select in GraphConv (layers/conv.py:66-81) and of scatter(sum). */
int anemoi_segment_sum_rows(const void* x, int64_t ldx, const int32_t* ptr, const int32_t* ids, void* out, int64_t ldo,
                            int32_t n_out, int32_t D, anemoi_dtype_t dtype, void* stream);

/* out[i] = a[i] + b[idx[i]]: adjoint of scatter(sum) + the carried edge gradient in GraphConv's backward. */
int anemoi_gather_add_rows(const void* a, int64_t lda, const void* b, int64_t ldb, const int32_t* idx, void* out, int64_t ldo,
                           int32_t n_out, int32_t D, anemoi_dtype_t dtype, void* stream);

/* out[c][r] = x[r][c] (r < n_rows), 0 for n_rows <= r < n_pad.  Builds the K-contiguous operands of the weight-gradient GEMM
 * dW = dZ^T X (autograd of torch.nn.Linear), whose reduction runs over the rows. */
int anemoi_transpose_pad(const void* x, int64_t ldx, void* out, int64_t ldo, int32_t n_rows, int32_t n_cols, int32_t n_pad,
                         anemoi_dtype_t dtype, void* stream);

/* Gated feed-forward layers (GatedMLPLayer, layers/mlp.py:25-59): out[r, c] = act(gv[r, c]) * gv[r, D + c], with
 * gv = [gate_proj(x) | value_proj(x)] from ONE fused projection.  kind: 0 sigmoid ("glu"), 1 SiLU ("swiglu"), 2 GELU erf
 * ("geglu"), 3 ReLU ("reglu").  anemoi_glu_bwd returns d_gv [n_rows, 2D] = [d_out * value * act'(gate) | d_out * act(gate)]. */
int anemoi_glu_fwd(const void* gate_value, int64_t ldgv, void* out, int64_t ldo, int32_t n_rows, int32_t D, int32_t kind,
                   anemoi_dtype_t dtype, void* stream);
int anemoi_glu_bwd(const void* gate_value, int64_t ldgv, const void* d_out, int64_t lddo, void* d_gate_value, int64_t lddgv,
                   int32_t n_rows, int32_t D, int32_t kind, anemoi_dtype_t dtype, void* stream);

/* ---- input normaliser at the model edges (scope row f4) ---------------------------------------------------------------
 * The reference normalises the batch before the model and de-normalises its output after it
 * (`pre_processors` / `post_processors` around `forward` in models/base.py:303-391; `InputNormalizer.transform`:
 * x * _norm_mul + _norm_add per variable, `inverse_transform`: (x - _norm_add) / _norm_mul, preprocessing/normalizer.py:154-252).
 * Here the transform rides in the kernels that touch every input / output element anyway. */

/* Stand-alone InputNormalizer.transform (inverse = 0: y = x * mul[c] + add[c]) / inverse_transform (inverse = 1:
 * y = (x - add[c]) / mul[c]) over the last dimension of a [n_rows, V] view; y may alias x (in_place). */
int anemoi_affine_columns(const void* x, int64_t ldx, void* y, int64_t ldy, const float* col_mul, const float* col_add,
                          int32_t inverse, int32_t n_rows, int32_t V, anemoi_dtype_t dtype, void* stream);

/* ---- imputers at the model edges -------------------------------------------------------------------------------------------
 * The reference's imputers (preprocessing/imputer.py) replace NaN in configured input variables before the normaliser and put NaN back
 * into the model's output where the input's first time step had it.  The IMPUTATION PROGRAM is a per-column table over the V input columns:
 * kind_src int32 [V][2] = (kind, source column), value fp32 [V].  kind 0: not imputed; 1: NaN -> value[c] (rounded to the data dtype on
 * the host, so the fp32 entry is exact); 2: NaN -> the element of column `source` at the same position (CopyImputer; a source column is
 * never itself imputed).  Masks are bool tensors, one byte per element, written with ordinary vector stores. */

/* Stand-alone BaseImputer.transform over x [batch, time, ensemble, grid, V] (element strides ld_b .. ld_n, columns contiguous; y likewise
 * and may alias x): the NaN test of an element is that of ensemble member 0 at the same (batch, time, grid, column) and applies to every
 * member; each time step has its own.  mask (NULL: none): bool [batch, grid, V], the NaN locations of time step 0, member 0, ALL columns. */
int anemoi_impute_columns(const void* x, int64_t ld_b, int64_t ld_t, int64_t ld_e, int64_t ld_n, void* y, int64_t yd_b, int64_t yd_t,
                          int64_t yd_e, int64_t yd_n, const int32_t* kind_src, const float* value, void* mask, int32_t B, int32_t T_steps,
                          int32_t E, int32_t N, int32_t V, anemoi_dtype_t dtype, void* stream);

/* Stand-alone BaseImputer.inverse_transform: y[b, m, n, c] = NaN where src_of[c] >= 0 and mask[b, n, src_of[c]], else x[b, m, n, c];
 * x / y [batch, M, grid, V] with rows ldx / ldy apart (y may alias x: only the restored elements are stored), mask bool [batch, grid, ldm]
 * with n_mask_cols columns, src_of int32 [V] (-1: the column is left alone). */
int anemoi_restore_nan_columns(const void* x, int64_t ldx, void* y, int64_t ldy, const void* mask, int64_t ldm, int32_t n_mask_cols,
                               const int32_t* src_of, int32_t B, int32_t M, int32_t N, int32_t V, anemoi_dtype_t dtype, void* stream);

/* ---- remapper and post-processors at the model edges ----------------------------------------------------------------------------
 * The reference's Remapper (preprocessing/remapper.py, mappings.py) maps single variables through log1p / sqrt / power / boxcox / atanh /
 * asinh / displaced boundary atoms / an affine map before the normaliser, and back on the output; its post-processors
 * (preprocessing/postprocessor.py) clamp output variables or fill them where a masking variable is zero / NaN.  A REMAP OP is one
 * direction of one map: 0 none, 1 log1p, 2 expm1, 3 power, 4 power inverse, 5 boxcox, 6 boxcox inverse, 7 log, 8 exp, 9 atanh,
 * 10 atanh inverse, 11 asinh, 12 asinh inverse, 13 displace atoms, 14 clamp, 15 affine, 16 affine inverse; flags: 1 clip negatives,
 * 2 tangent-linear above one, 4 / 8 a lower / upper bound exists, bits 4..7 how the power is taken (0 powf, 1 sqrt, 2 x*x, 3 x*x*x,
 * 4 copy - torch's scalar pow).  Every step of a map rounds to the data dtype, as the reference's in-place torch ops do; where a map
 * divides by a scalar parameter the table holds its fp32 reciprocal and the kernel multiplies, as torch's device kernels do. */

/* Stand-alone Remapper.transform / inverse_transform over x [batch, time, ensemble, grid, V] (element strides ld_b .. ld_n, columns
 * contiguous; y likewise and may alias x).  op_flags int32 [V][2] = (remap op, flags), par fp32 [V][4] (8- / 16-byte aligned).
 * active int32 [n_active]: the columns whose op is not 0 - only those are loaded and stored (required in place); NULL: all V columns (out
 * of place).  violations (NULL: none): int32 [V], entry c counts the elements of column c that fail the reference's forward domain assertion. */
int anemoi_remap_columns(const void* x, int64_t ld_b, int64_t ld_t, int64_t ld_e, int64_t ld_n, void* y, int64_t yd_b, int64_t yd_t,
                         int64_t yd_e, int64_t yd_n, const int32_t* op_flags, const float* par, const int32_t* active, int32_t n_active,
                         int32_t* violations, int32_t B, int32_t T_steps, int32_t E, int32_t N, int32_t V, anemoi_dtype_t dtype, void* stream);

/* ---- the staged chain at the model edges (ABI 23) ---------------------------------------------------------------------------------
 * The pre-processor chain [imputer]? [Remapper]? [InputNormalizer]? rides in the kernels that touch every input element anyway.  Each
 * optional stage is a pointer group that is NULL as a whole where the chain has no such stage:
 *   kind_src / value (/ mask)   the imputation program above;
 *   op_flags / par              the FORWARD remap program (int32 [V][2], fp32 [V][4], 8- / 16-byte aligned), each step rounded to the RAW dtype;
 *   col_mul / col_add           the normaliser, fp32 [V]: x * col_mul[v] + col_add[v], two fp32 roundings like torch's mul_ / add_. */

/* anemoi_assemble_input whose T * V time / variable columns go through the chain: every raw element is tested and imputed within its own
 * time step (the copy source is read from the same step and row), remapped, normalised.  `x` may be fp32 (x_dtype) while `attrs` / `out`
 * are in the model `dtype`.  mask (with the imputation program): bool [n_rows][ldm], the NaN locations of step 0 of the RAW input, written
 * in the same pass.  A 16-bit output with W % 8 == 0, ldo % 8 == 0 and a 16-byte-aligned `out` takes the 8-column kernel. */
int anemoi_assemble_input_chain(const void* x, anemoi_dtype_t x_dtype, int64_t ld_t, int64_t ldx, int32_t T_steps, int32_t V,
                                const int32_t* kind_src, const float* value, void* mask, int64_t ldm, const int32_t* op_flags, const float* par,
                                const float* col_mul, const float* col_add, const void* attrs, int64_t lda, int32_t A, void* out, int64_t ldo,
                                int32_t W, int32_t n_rows, anemoi_dtype_t dtype, void* stream);

/* anemoi_assemble_output with the skip connection read from the RAW input, which goes through the same chain on the fly (the tables span
 * the skip's columns): out[n, v] = x_out[n, v] + (col_map[v] >= 0 ? chain(x_skip[n, m]) : 0), m = col_map[v].  x_out in `model_dtype`;
 * x_skip / out in `dtype` (= model_dtype or fp32: the reference adds the residual in the input's dtype,
 * models/encoder_processor_decoder.py:145-158).  The de-normalisation of the result is op 9 of anemoi_column_program. */
int anemoi_assemble_output_chain(const void* x_out, int64_t ldx, anemoi_dtype_t model_dtype, const void* x_skip, int64_t lds,
                                 const int32_t* col_map, const int32_t* kind_src, const float* value, const int32_t* op_flags, const float* par,
                                 const float* col_mul, const float* col_add, void* out, int64_t ldo, int32_t n_rows, int32_t n_cols,
                                 anemoi_dtype_t dtype, void* stream);

/* The output column program, in place and in order: the boundings (layers/bounding.py:81-307; models/encoder_processor_decoder.py:160-162)
 * and what follows them on the output.  ops: int32 [n_ops][4] = (kind, column, total column, 0); params: fp32 [n_ops][2].
 *   kind 1 ReluBounding, 2 LeakyReluBounding, 3 / 4 Normalized(Leaky)ReluBounding (params[0] = the normalised minimum), 5 / 6
 *   (Leaky)HardtanhBounding (min, max), 7 / 8 (Leaky)FractionBounding (min, max; times column ``total``), 9 de-normalisation
 *   (x - params[0]) / params[1] = InputNormalizer.inverse_transform of that column (preprocessing/normalizer.py:217-252);
 *   with a mask bool [n_rows][ldm] (n_mask_cols columns; NULL with n_mask_cols = 0: none): 10 "NaN where mask[n, src]", encoded
 *   (10, dst column, src mask column, 0) and appended after the op-9 de-normalisations.  n_nan_ops: how many ops of kind 10 the caller
 *   knows the program to hold; n_nan_ops > 0 with mask == NULL is an error;
 *   with extended != 0 (the host says so when it builds the tables; they live in device memory): 11 "p0 where x[n, total column] == 0",
 *   12 "NaN where x[n, total column] is NaN" - both read the row as the ops before them left it - and 16 + r: remap op r, with
 *   flags = ops[i][3] and its third parameter as the float bits of ops[i][2].
 * A kind the call does not enable leaves its column as it is. */
int anemoi_column_program(void* x, int64_t ldx, int32_t n_rows, int32_t n_cols, const int32_t* ops, const float* params, int32_t n_ops,
                          const void* mask, int64_t ldm, int32_t n_mask_cols, int32_t n_nan_ops, int32_t extended, anemoi_dtype_t dtype,
                          void* stream);

/* ---- device-initiated row exchange between the ranks of a model-parallel group (scope row e) ----------------------------
 * The reference exchanges node rows with host-issued NCCL collectives: the per-layer halo all-to-all
 * (`_halo_exchange` = dist.all_to_all_single with per-peer splits, distributed/primitives.py:422-460, called from
 * GraphTransformerProcessorBlock.forward, layers/block.py:1159-1172), the all-gather of shards (`_gather`,
 * primitives.py:60-183) and the source-row sync of the mappers (distributed/khop_edges.py:386-392).  On one MI355X node
 * the same data movement is ONE kernel of the rank's own stream per exchange: it stores the rows straight into the peers'
 * receive buffers (peer memory mapped with hipIpc; xGMI is point to point, every link carries only its own rows), publishes
 * them with a system-scope release + an epoch flag, and waits for the flags of the peers it receives from.  Being a plain
 * kernel node it is captured with the rest of the forward: one hipGraph per rank, no host in the loop
 * (anemoi_core_amd/distributed/peer.py holds the host side; RCCL stays available as the fallback wire).
 *
 * Memory.  anemoi_peer_alloc returns zeroed device memory of one of three kinds; anemoi_peer_export writes the
 * ANEMOI_PEER_HANDLE_BYTES-byte hipIpc handle other processes pass to anemoi_peer_open (never the exporting process itself);
 * anemoi_peer_close unmaps.  Handles travel over the caller's control plane (torch.distributed object collectives). */
#define ANEMOI_PEER_MEM_DEFAULT 0     /* hipMalloc: receive buffers, read by later kernels of the receiving stream */
#define ANEMOI_PEER_MEM_FINEGRAINED 1 /* hipExtMallocWithFlags(hipDeviceMallocFinegrained) */
#define ANEMOI_PEER_MEM_UNCACHED 2    /* hipExtMallocWithFlags(hipDeviceMallocUncached): flag words polled while a peer writes */
#define ANEMOI_PEER_HANDLE_BYTES 64
int anemoi_peer_alloc(void** ptr, int64_t bytes, int32_t kind);
int anemoi_peer_free(void* ptr);
int anemoi_peer_export(void* ptr, void* handle_out /* host, 64 bytes */);
int anemoi_peer_open(const void* handle /* host, 64 bytes */, void** ptr_out);
int anemoi_peer_close(void* ptr);

/* One exchange of one channel.  Packed row i of the send order is src[(send_index ? send_index[i] : i)] (row_bytes bytes, a
 * multiple of 16, ld_src_bytes apart); `table` is int64 [6][n_peers] in device memory: remote_base (address of this rank's
 * first row in peer p's receive buffer), remote_flag (address of the word peer p polls for this rank), send_begin,
 * send_count (rows of the packed order for peer p), signal (1: publish the epoch to p), expect (1: wait for p's epoch).
 * local_flags = this rank's words of the channel: [n_peers flags | seq | ticket] (uint32, ANEMOI_PEER_MEM_UNCACHED).  total_rows
 * may be 0 (signal / expect only: the forward-level barrier).  A peer that does not show up within timeout_ticks (100 MHz
 * wall clock) sets *status = 0x80000000 | peer instead of hanging the device.  `status` points at a block of >= 5 words:
 * [0] the time-out word, [2] exchanges run, [3] ticks summed over them between "my rows released" and "every expected flag
 * seen", [4] the longest such wait (diagnostics; the caller may zero them between forwards). */
int anemoi_peer_exchange_rows(const void* src, int64_t ld_src_bytes, const int32_t* send_index, const int64_t* table,
                              int32_t n_peers, int32_t row_bytes, int32_t total_rows, uint32_t* local_flags, uint32_t* status,
                              int64_t timeout_ticks, void* stream);

/* ---- row-resident layer chain (csrc/gt_chain2.hip) -----------------------------------------------------------------------------
 * Everything of a GraphTransformer block that is local to a node row, after the edge attention, as ONE launch:
 *     x1   = attn W_p^T + b_p + x_res                       projection + skip            (layers/block.py:1263-1266)
 *     h    = GELU(LayerNorm(x1; ln1) W_1^T + b_1)           node_dst_mlp, first Linear   (layers/block.py:1268-1271, layers/mlp.py:158-169)
 *     x2   = h W_2^T + b_2 + x1;  x_out = x2 [+ extra]      second Linear + skip [+ the model's latent skip, added to the ROUNDED
 *                                                           block output as `x_latent_proc + x_latent` does,
 *                                                           models/encoder_processor_decoder.py:295-296]
 *     q_out = LayerNorm(x_out; lnq) W_q^T + b_q             optional: the NEXT block's layer_norm_attention + fused
 *                                                           [lin_query; lin_key; lin_value; lin_self] (layers/block.py:1237-1245)
 * replacing four anemoi_linear_* launches per block (and the LayerNorm fold's statistics hand-off between them).  A workgroup keeps a
 * panel of <= 48 rows in LDS through the whole chain and streams the weights from L2 straight into MFMA operand registers; the
 * hidden activations [n_rows, hidden] are never written.  The workgroup's eight waves form two groups of four that work DIFFERENT
 * GEMM segments (group A: projection, MLP first Linear + GELU, even chunks of the trailing projection; group B: MLP second Linear, odd
 * chunks), so that one group's epilogue runs beside the other group's MFMA and weight stream.
 *
 * Weights are FRAGMENT-MAJOR images made once per parameter version (ops.pack_weight_frag): for W [O, K] row-major (O % 64 == 0,
 * K % 32 == 0) the image is [O/64 slabs][K/32 k-steps][4 column blocks][4 k-slots][16 rows][8 elements], i.e. element
 * (slab, ks, ni, kslot, row, e) = W[slab*64 + ni*16 + row][ks*32 + kslot*8 + e] - one contiguous KiB per MFMA B fragment.
 *
 * The two LayerNorms are computed as fp32 statistics of the rounded rows and applied WITHOUT their affine part, the normalised row
 * rounded to the model dtype; the affine part is folded by the caller into the Linear that follows (ops.gt_layer_chain2 does it once
 * per parameter version):
 *     w1 = fragment-major image of W_1 diag(gamma_1) (rounded to the model dtype),   d1 = W_1 beta_1 + b_1
 *     wq = fragment-major image of W_q diag(gamma_q),                                 dq = W_q beta_q + b_q
 * and every bias enters as the START value of its GEMM's accumulators: vec = [b_p (512) | d1 (hidden) | b_2 (512) | dq (q_out_features)]
 * in the model dtype, kept in LDS (2*512 + hidden + q_out_features <= 6144, else ANEMOI_E_UNSUPPORTED).  With BOTH extra and a trailing
 * projection the projection reads LayerNorm(x2 + extra): the decoder's layer_norm_attention_src + [lin_key; lin_value] behind the last processor
 * block and the latent skip (encoder_processor_decoder.py:295-296, layers/block.py:981-984).  q_out_features: a multiple of 512, or 128 / 256 /
 * 384 (a NARROW trailing projection: the decoder's node_data_extractor, layers/mapper.py:688-704, zero-padded to a multiple of 128 rows); x_out
 * may be NULL when there is a trailing projection and no extra (x2 is then not written).  channels must be 512; hidden a multiple of 512;
 * 16-bit dtypes; all row pointers 16-byte aligned, all leading dimensions multiples of 8 elements.
 * rows_per_tile = 0 lets the
 * library choose (anemoi_gt_chain_rows_per_tile: 48). */
typedef struct anemoi_gt_chain2_args {
  const void* attn;   int64_t ld_attn;    /* [n_rows, channels]   attention output + self term */
  const void* x_res;  int64_t ld_x;       /* [n_rows, channels]   the block's input */
  const void* wp;                         /* projection, fragment-major [channels, channels] */
  const void* w1;     int32_t hidden;     /* fragment-major [hidden, channels], layer_norm_mlp_dst's gamma folded in */
  const void* w2;                         /* fragment-major [channels, hidden] */
  const void* wq;     int32_t q_out_features; /* fragment-major [q_out_features, channels], the next block's gamma folded in; 0: none */
  const void* vec;                        /* [b_p | d1 | b_2 | dq], model dtype, 16-byte aligned */
  float ln1_eps;      float lnq_eps;
  const void* extra;  int64_t ld_extra;   /* optional [n_rows, channels] or NULL */
  void* x_out;        int64_t ld_out;     /* [n_rows, channels] */
  void* q_out;        int64_t ld_q;       /* [n_rows, q_out_features] */
  int32_t n_rows;     int32_t channels;   int32_t rows_per_tile;
  void* timeline;     /* must be NULL (ANEMOI_E_UNSUPPORTED otherwise); the experiments build of the library takes a uint64
                         [min(256, panels)][8 waves][48] buffer for its instrumented instantiation (tools/chain2_timeline.py) */
} anemoi_gt_chain2_args_t;
int anemoi_gt_chain2_fwd(const anemoi_gt_chain2_args_t* args, anemoi_dtype_t dtype, void* stream);
int anemoi_gt_chain_rows_per_tile(int32_t n_rows);

/* ---- row-resident embedding chain of a GraphTransformer mapper side (round 6; csrc/gt_rowchain.hip) ---------------------------------
 * One side of a GraphTransformer mapper in ONE launch:
 *     y     = x W_e^T + b_e                       emb_nodes_src / emb_nodes_dst = Linear(in, 512)      (layers/mapper.py:556-566, 688-694)
 *     q_out = LayerNorm(y) [W_a; W_b]^T + b       layer_norm_attention_src + [lin_key; lin_value] or
 *                                                 layer_norm_attention_dest + [lin_query; lin_self]      (layers/block.py:981-984)
 * replacing anemoi_linear_stats_fwd (the embedding GEMM + row statistics) and anemoi_linear_lnfold_fwd (the projection with the folded
 * LayerNorm).  x_out = NULL: y is never written (the encoder's source side: the block returns the source rows untouched).
 *   x  [n_rows, in_features], in_features a multiple of 8 up to 512;
 *   we fragment-major image (see anemoi_gt_chain2_fwd) of W_e zero-padded to [512, 128 ceil(in_features / 128)];
 *   wq fragment-major image of [W_a; W_b] diag(gamma) [q_out_features, 512] (the LayerNorm's affine part folded in by the caller,
 *      ops.gt_row_chain), vec = [b_e (512) | W beta + b (q_out_features)] in the model dtype;
 *   channels must be 512, q_out_features a multiple of 512 up to 2048, 16-bit dtypes, row pointers 16-byte aligned. */
typedef struct anemoi_gt_rowchain_args {
  const void* x;      int64_t ld_x;       int32_t in_features;
  const void* we;                         /* fragment-major [channels, 128 ceil(in_features / 128)] */
  const void* wq;     int32_t q_out_features; /* fragment-major [q_out_features, channels] */
  const void* vec;                        /* [b_e | dq], model dtype, 16-byte aligned */
  float ln_eps;
  void* x_out;        int64_t ld_out;     /* optional [n_rows, channels] or NULL */
  void* q_out;        int64_t ld_q;       /* [n_rows, q_out_features] */
  int32_t n_rows;     int32_t channels;   int32_t rows_per_tile;  /* rows_per_tile = 0: 48 */
} anemoi_gt_rowchain_args_t;
int anemoi_gt_rowchain_fwd(const anemoi_gt_rowchain_args_t* args, anemoi_dtype_t dtype, void* stream);
/* Panels [first_panel, first_panel + panels) of that job (48-row panels, or rows_per_tile) as a launch of their own, with the schedule the
 * WHOLE job's launch has (more than one round of panels and in_features <= 256: the pipelined kernel, else the single-panel one; the two
 * round differently), so that a row's bits do not depend on which launch computed it. */
int anemoi_gt_rowchain_panels_fwd(const anemoi_gt_rowchain_args_t* args, int32_t first_panel, int32_t panels, anemoi_dtype_t dtype, void* stream);

/* ---- the source side of a mapper from raw rows with a composed weight (csrc/gt_embed_fold.hip) ------------------------------------
 * q_out = LayerNorm(x W_e^T + b_e) [W_a; W_b]^T + b with the embedded rows e = x W_e^T + b_e kept in accumulators (nobody reads them: the
 * forward mapper does not update its source rows).  With W_g = [W_a; W_b] diag(gamma) and d = [W_a; W_b] beta + b:
 *     q_out[j] = rstd_j (W_c x_j + u - mean_j s) + d,   W_c = W_g W_e,  u = W_g b_e,  s = rowsum(W_g)
 * (mean_j, rstd_j: the plain fp32 LayerNorm statistics of e_j ROUNDED to the model dtype, as the GEMM pair forms them).  Replaces the pair
 * anemoi_linear_stats_fwd (emb_nodes_src, layers/mapper.py:556-566) + anemoi_linear_lnfold_fwd (layer_norm_attention_src + [lin_key;
 * lin_value], layers/block.py:981-984) on that side: e is neither written nor read back, and the projection is one GEMM over K = in_features.
 *   we, wc: fragment-major images (ops.pack_weight_frag) of W_e [512, Kp] and of W_c [q_out_features, Kp] rounded ONCE to the model dtype,
 *           Kp = 64 ceil(in_features / 64), columns beyond in_features zero (ops.compose_embedding_projection);
 *   vec = [b_e (512) | u | s | d (q_out_features each)] in fp32.
 * ANEMOI_E_UNSUPPORTED (nothing launched, the caller keeps the pair) unless: 16-bit dtype, channels 512, in_features a multiple of 8 up to
 * 256, q_out_features a multiple of 512 up to 2048.  Any n_rows >= 0; x, q_out rows 16-byte aligned (ld multiples of 8 elements). */
typedef struct anemoi_gt_embed_fold_args {
  const void* x;      int64_t ld_x;       int32_t in_features;
  const void* we;                         /* fragment-major [channels, Kp] */
  const void* wc;     int32_t q_out_features; /* fragment-major [q_out_features, Kp] */
  const float* vec;   float ln_eps;
  void* q_out;        int64_t ld_q;       /* [n_rows, q_out_features] */
  int32_t n_rows;     int32_t channels;
} anemoi_gt_embed_fold_args_t;
int anemoi_gt_embed_fold_fwd(const anemoi_gt_embed_fold_args_t* args, anemoi_dtype_t dtype, void* stream);

/* ---- a block tail that carries a side job (csrc/gt_chain2.hip, SIDE instantiation) ------------------------------------------------
 * anemoi_gt_chain2_fwd(args) and, in the SAME launch, panels [side_first_panel, side_first_panel + side_panels) of the row chain
 * `side` (48-row panels of its rows, rows_per_tile as in anemoi_gt_rowchain_fwd) on workgroups of their own behind the tail's: a tail of
 * fewer than 256 panels per round leaves compute units idle, and work that does not depend on the tail can run there.  The two jobs
 * share nothing but the launch; each computes exactly what its own entry point computes (the riders run the schedule the whole side job's
 * launch has: anemoi_gt_rowchain_panels_fwd).  side_blocks = 0: one rider per idle compute
 * unit (256 - the tail's workgroups per round); > 0: at most that many.  A rider walks its panels with stride riders.
 * ANEMOI_E_UNSUPPORTED, nothing launched: the tail leaves no compute unit idle (256 workgroups per round, or no rows at all), or the
 * side job fails anemoi_gt_rowchain_fwd's preconditions - the caller launches the two pieces separately.  Every argument check of the
 * two entry points applies; side_panels = 0 launches the tail alone. */
int anemoi_gt_chain2_side_fwd(const anemoi_gt_chain2_args_t* args, const anemoi_gt_rowchain_args_t* side, int32_t side_first_panel,
                              int32_t side_panels, int32_t side_blocks, anemoi_dtype_t dtype, void* stream);

/* Which kernel a chain entry point launches for a shape, on how many rows per panel, workgroups and bytes of LDS: the decision of
 * csrc/chain_plan.h, asked without launching anything.  HOST-ONLY: no HIP call, no device needed.  kind: 0 anemoi_gt_chain2_fwd,
 * 1 anemoi_gt_chain2_side_fwd, 2 anemoi_gt_cluster_chain_fwd, 3 anemoi_gt_rowchain_fwd, 4 anemoi_gt_rowchain_panels_fwd,
 * 5 anemoi_gt_embed_fold_fwd, 6 anemoi_gnn_edge_chain_fwd, 7 anemoi_gnn_mlp_chain_fwd, 8 anemoi_gnn_node_chain_fwd (and its segsum
 * form).  The problem holds the shape fields of that entry point's arguments (the others are not read): first_panel / panels are the
 * range of kind 4 and the side job's riding panels of kind 1, whose side job is side_* with side_cap = side_blocks.  Returns what the
 * entry point returns for the shape with well-formed operands (null, alignment and leading-dimension checks look at pointers and stay
 * in the entry points): ANEMOI_OK, ANEMOI_E_UNSUPPORTED or ANEMOI_E_INVALID; `out` is written for ANEMOI_OK only.  kernel: 0 nothing
 * to launch, 1 gt_chain2 on every CU, 2 below the chip, 3 / 4 their instrumented forms, 5 with riders, 6 cluster, 7 row chain
 * single-panel, 8 pipelined, 9 embed fold, 10 / 11 / 12 GraphConv edge / MLP / node.  rounds: panels of the busiest workgroup;
 * idle_cus: CUs without a workgroup in every round.  Kind 1: host_grid tail workgroups, riders behind them on panels [first, end) of the
 * side job, side_pipelined its schedule.  Kinds 3, 4: job_panels and pipelined describe the WHOLE job, n_rows rows from row_begin are
 * the launch's.  Under the environment switches of this process (ANEMOI_CHAIN_ROWS; the experiments build's grid switches). */
typedef struct anemoi_chain_problem {
  int32_t kind, n_rows, in_features, hidden, q_out_features, rows_per_tile, dtype, timeline, first_panel, panels;
  int32_t side_rows, side_in_features, side_q_out_features, side_rows_per_tile, side_cap;
} anemoi_chain_problem_t;
typedef struct anemoi_chain_plan {
  int32_t kernel, rows_per_panel, panels, grid, threads, lds_bytes, rounds, idle_cus;
  int32_t host_grid, riders, first, end, side_pipelined;
  int32_t job_panels, pipelined, n_rows;
  int64_t row_begin;
} anemoi_chain_plan_t;
int anemoi_chain_plan(const anemoi_chain_problem_t* problem, anemoi_chain_plan_t* out);

/* ---- cluster chain: the block tail for FEW rows (round 6; csrc/gt_cluster_chain.hip) ----------------------------------------------
 * What anemoi_gt_chain2_fwd computes (same operands, same folded LayerNorms, same vec layout with hidden = 2048:
 * [b_p 512 | d1 2048 | b_2 512 | dq q_out_features]), organised for block tails of a few thousand rows - a rank's share of a sharded
 * mesh, small hidden meshes: FOUR CUs of one XCD own a 48-row panel as a tensor-parallel group over the MLP's hidden width (each streams
 * the projection, one 512-column chunk of the first Linear, the matching K-slice of the second Linear and one chunk of the trailing
 * projection: 2 MiB instead of 6.5 MiB per layer), exchange the second Linear's fp32 partial sums ONCE per panel through `workspace`
 * (agent-scope stores / loads + an atomic counter per cluster) and add them in member order, so that every member holds the same x2.
 * Replaces layers/block.py:1263-1273 (+ :1237-1245 of the next block) like the chain; hidden must be 2048, q_out_features <= 2048.
 *   ln_out (nullable): LayerNorm_attn'(x2) WITHOUT its affine part [n_rows, 512] - what a sharded block sends to its halo peers;
 *   workspace: anemoi_gt_cluster_chain_workspace_bytes() bytes, 128-byte aligned, ZERO at allocation and then owned by the library (the
 *   cluster counters in it are monotonic across launches); one workspace per device and stream of launches.
 * A cluster's four workgroups must be resident together (the launch uses at most one workgroup per CU); a member that waits for a
 * partner for more than ~1 s traps: the launch fails, it never returns partial sums. */
typedef struct anemoi_gt_cluster_chain_args {
  const void* attn;   int64_t ld_attn;    /* [n_rows, channels]   attention output + self term */
  const void* x_res;  int64_t ld_x;       /* [n_rows, channels]   the block's input */
  const void* wp;                         /* projection, fragment-major [channels, channels] */
  const void* w1;     int32_t hidden;     /* fragment-major [hidden, channels], layer_norm_mlp_dst's gamma folded in; hidden = 2048 */
  const void* w2;                         /* fragment-major [channels, hidden] */
  const void* wq;     int32_t q_out_features; /* fragment-major [q_out_features, channels], the next block's gamma folded in; 0: none */
  const void* vec;                        /* [b_p | d1 | b_2 | dq], model dtype, 16-byte aligned */
  float ln1_eps;      float lnq_eps;
  const void* extra;  int64_t ld_extra;   /* optional [n_rows, channels] or NULL (not together with q_out / ln_out) */
  void* x_out;        int64_t ld_out;     /* [n_rows, channels] */
  void* q_out;        int64_t ld_q;       /* [n_rows, q_out_features] */
  void* ln_out;       int64_t ld_ln;      /* optional [n_rows, channels] */
  void* q_out2;       int64_t ld_q2;      int32_t q_split;  /* optional second destination of the trailing projection: its 512-column chunks
                                             q_split, q_split + 1, ... go to q_out2 [n_rows, q_out_features - 512 q_split] instead of q_out (a
                                             sharded block: q | self for its own rows, k | v into the head of the buffer its halo rows arrive in);
                                             q_out2 = NULL: everything to q_out */
  void* workspace;    int64_t workspace_bytes;
  int32_t n_rows;     int32_t channels;
} anemoi_gt_cluster_chain_args_t;
int anemoi_gt_cluster_chain_fwd(const anemoi_gt_cluster_chain_args_t* args, anemoi_dtype_t dtype, void* stream);
int64_t anemoi_gt_cluster_chain_workspace_bytes(void);

/* ---- row-resident chains of the GraphConv (GNN) processor block (round 4; csrc/gnn_chain.hip) ------------------------------------
 * GraphConv (layers/conv.py:29-81) in its gather-add form, with an edge MLP of three Linears (mlp_extra_layers = 0):
 *     e_new = LayerNorm(W_2 gelu(W_1 gelu(W_e e + g1[idx1] + g2[idx2] + b_0) + b_1) + b_2; ln) + e
 * where g1 = x_dst W_i^T and g2 = x_src W_j^T are node-level rows gathered by the edge's destination / source, W_e = the edge
 * columns of the first Linear's weight.  ONE launch instead of three edge-level GEMMs + the LayerNorm / residual half of
 * anemoi_edge_ln_residual_segment_sum_fwd (whose arithmetic and rounding points it keeps: the GEMM outputs rounded to the model
 * dtype, one rounding of LayerNorm(z) + e); the scatter-sum over e_new is anemoi_segment_sum_rows.  w0 / w1 / w2 are fragment-major
 * images (see anemoi_gt_chain2_fwd) of [512, 512] weights. */
int anemoi_gnn_edge_chain_fwd(const void* e, int64_t ld_e, const void* g1, int64_t ld_g1, const int32_t* idx1, const void* g2, int64_t ld_g2,
                              const int32_t* idx2, const void* w0, const void* b0, const void* w1, const void* b1, const void* w2, const void* b2,
                              const void* ln_w, const void* ln_b, float eps, void* e_new, int64_t ld_o, int32_t n_rows, int32_t channels,
                              anemoi_dtype_t dtype, void* stream);
/* An embedding MLP of the GNN mappers / processor as ONE launch (the edge chain without gathered rows):
 *   out = LayerNorm(W_2 gelu(W_1 gelu(W_0 x + b_0) + b_1) + b_2) [+ res]
 * Replaces: MLP.forward for `emb_edges` / `emb_nodes_src` / `emb_nodes_dst` (layers/mlp.py:29-100 as built at
 * layers/mapper.py:640-700 and layers/processor.py GNNProcessor: Linear -> GELU -> Linear -> GELU -> Linear -> LayerNorm).
 *   x [n_rows, in_features] with in_features in {128, 256, 384, 512} (the caller zero-pads the raw width; ld_x >= in_features);
 *   w0: fragment-major image of the [512, in_features] weight (zero columns for the padding), w1 / w2: of [512, 512];
 *   res (nullable): [n_rows, 512] rows added after the LayerNorm. */
int anemoi_gnn_mlp_chain_fwd(const void* x, int64_t ld_x, int32_t in_features, const void* w0, const void* b0, const void* w1, const void* b1,
                             const void* w2, const void* b2, const void* ln_w, const void* ln_b, float eps, const void* res, int64_t ld_res,
                             void* out, int64_t ld_o, int32_t n_rows, int32_t channels, anemoi_dtype_t dtype, void* stream);

/* The node MLP of a GraphConv block (layers/block.py:392-394; MLP of three Linears + LayerNorm, layers/mlp.py:97-179) with its skip:
 *     x_out = LayerNorm(W_c gelu(W_b gelu(W_a [x | agg] + b_a) + b_b) + b_c; ln) + x
 * and optionally t_out = x_out W_t^T [+ b_t] - the NEXT block's stacked node-level terms [x W_i^T | x W_j^T] its edge chain gathers.
 * wa [512, 1024], wb, wc [512, 512], wt [t_out_features, 512] fragment-major. */
int anemoi_gnn_node_chain_fwd(const void* x, int64_t ld_x, const void* agg, int64_t ld_a, const void* wa, const void* ba, const void* wb,
                              const void* bb, const void* wc, const void* bc, const void* ln_w, const void* ln_b, float eps, void* x_out,
                              int64_t ld_o, const void* wt, const void* bt, int32_t t_out_features, void* t_out, int64_t ld_t, int32_t n_rows,
                              int32_t channels, anemoi_dtype_t dtype, void* stream);
/* The same launch with GraphConv's scatter-sum inside it (layers/conv.py:81: `out = scatter(edge_attr_new, edge_index[1], reduce="sum")`):
 * instead of an aggregated table the kernel takes the EDGE rows edge_rows [M, 512] (sorted by destination) and seg_ptr [n_rows + 1] (the CSC
 * column pointer) and forms agg[n] = sum of the rows [seg_ptr[n], seg_ptr[n+1]) in fp32, in edge order, rounded once - the arithmetic of
 * anemoi_segment_sum_rows - while it loads the panel.  Saves that launch, the [N, 512] table it writes and its read-back. */
int anemoi_gnn_node_chain_segsum_fwd(const void* x, int64_t ld_x, const void* edge_rows, int64_t ld_e, const int32_t* seg_ptr, const void* wa,
                                     const void* ba, const void* wb, const void* bb, const void* wc, const void* bc, const void* ln_w,
                                     const void* ln_b, float eps, void* x_out, int64_t ld_o, const void* wt, const void* bt,
                                     int32_t t_out_features, void* t_out, int64_t ld_t, int32_t n_rows, int32_t channels,
                                     anemoi_dtype_t dtype, void* stream);


/* Sliding-window (banded) multi-head self-attention, forward.
 * Replaces: MultiHeadSelfAttention.attention_computation with its flash-attention / SDPA wrappers (layers/attention.py:41-262, 283-316,
 * 362-520): rows are (batch seq_len), head h is columns [h d, (h+1) d) of every operand; query i attends keys j of its own sequence with
 * |i - j| <= window (window < 0 or >= seq_len - 1: all of them):
 *     s = <q_i, k_j> * scale;  s = softcap tanh(s / softcap)  (softcap > 0);  s -= alibi_slopes[h] |i - j|  (alibi_slopes != NULL)
 *     out_i = sum_j softmax_j(s) v_j;  lse[i, h] = ln sum_j exp(s_j)  (fp32 [batch seq_len, H], if lse != NULL)
 * q, k, v, out: [batch seq_len, >= H d] with their own leading dimensions (column slices of one [rows, 3A] buffer work as they are);
 * alibi_slopes: fp32 [H] or NULL.  d in {32, 64, 128}, otherwise ANEMOI_E_UNSUPPORTED.  16-bit operands need 16-byte aligned rows of
 * q / k / v and 8-byte aligned rows of out.  The work is proportional to seq_len (2 window + 1); no allocation, no synchronisation. */
int anemoi_window_attention_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out, int64_t ldo,
                                float* lse, int32_t batch, int32_t seq_len, int32_t H, int32_t d, int32_t window, float scale, float softcap,
                                const float* alibi_slopes, anemoi_dtype_t dtype, void* stream);

/* Backward of the op above.
 * Replaces: autograd through MultiHeadSelfAttention.attention_computation (layers/attention.py:41-262; the reference differentiates its
 * flash-attention / SDPA call).  With t = <q_i, k_j> * scale, s the capped and biased score of the forward and p = exp(s - lse[i, h]):
 *     Delta_i = <d_out_i, out_i>;  dP = <d_out_i, v_j>;  dS = p (dP - Delta_i);  dT = dS (1 - tanh^2(t / softcap))  (softcap > 0) or dS
 *     dq_i = scale sum_j dT k_j;  dk_j = scale sum_i dT q_i;  dv_j = sum_i p d_out_i          (alibi_slopes get no gradient)
 * Two launches that both recompute the scores: the query pass writes dq and delta, the key pass reads delta and writes dk and dv;
 * `passes` selects them (ANEMOI_WINDOW_BWD_BOTH_PASSES in product code; one pass alone is for timing, and the key pass alone needs the
 * delta of an earlier query pass).  out, lse: the forward's results (lse fp32 [batch seq_len, H]); delta: fp32 [batch seq_len, H]
 * workspace of the caller; every operand has its own leading dimension, so dq / dk / dv can be the three column slices of one
 * [rows, 3A] gradient buffer.  No atomics: every element is summed in a fixed order, bitwise reproducible.  Shapes, window
 * normalisation and d as in the forward; 16-bit operands need 16-byte aligned rows of the inputs and 8-byte aligned rows of dq / dk / dv.
 * The work is proportional to seq_len (2 window + 1); no allocation, no synchronisation. */
#define ANEMOI_WINDOW_BWD_QUERY_PASS 1
#define ANEMOI_WINDOW_BWD_KEY_PASS 2
#define ANEMOI_WINDOW_BWD_BOTH_PASSES 3
int anemoi_window_attention_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const void* out, int64_t ldo,
                                const void* d_out, int64_t ldg, const float* lse, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv,
                                int64_t lddv, float* delta, int32_t batch, int32_t seq_len, int32_t H, int32_t d, int32_t window, float scale,
                                float softcap, const float* alibi_slopes, int32_t passes, anemoi_dtype_t dtype, void* stream);

/* What the kernels of the two ops above do with a sequence of seq_len rows, asked without launching anything (ABI 26).  HOST-ONLY: no HIP
 * call, no device needed; the answer comes from the band functions of csrc/window_attention_core.h that the kernels themselves call.
 * pass: 0 the forward, 1 the backward's query pass, 2 its key pass.  A workgroup owns rows_per_block rows of one (sequence, head) - queries,
 * or keys in the key pass - and streams tiles of tile_rows rows of the other side, tile t = rows [lo + t tile_rows, + tile_rows), ntiles of
 * them, rows from `hi` on read as zeros; 16-bit dtypes: 64 owned rows, wave 0..3 a strip of 16 of them; fp32: one row and one wave.
 *   window: as normalised (-1 = unbounded);  grid_x: workgroups per (sequence, head) = ceil(seq_len / rows_per_block);
 *   tile_class[t] (the first min(ntiles, tile_capacity) tiles; NULL with tile_capacity 0 to ask for the sizes only) for workgroup `block`
 *   and wave `wave`: 0 the wave skips the tile (it holds no row in the band of the wave's rows), 1 it masks element by element, 2 every
 *   pair is in the band and the sequence and no mask is evaluated.
 * d, seq_len and dtype are refused as the ops refuse them. */
#define ANEMOI_WINDOW_TILE_SKIPPED 0
#define ANEMOI_WINDOW_TILE_MASKED 1
#define ANEMOI_WINDOW_TILE_FULL 2
typedef struct {
  int32_t window, rows_per_block, grid_x, tile_rows, lo, hi, ntiles;
} anemoi_window_attention_plan_t;
int anemoi_window_attention_plan(int32_t pass, int32_t seq_len, int32_t d, int32_t window, anemoi_dtype_t dtype, int32_t block, int32_t wave,
                                 anemoi_window_attention_plan_t* out, int32_t* tile_class, int32_t tile_capacity);

/* Sparse projection of node rows by a constant CSR matrix, forward (and, on the transposed matrix, backward).
 * Replaces: SparseProjector._project_flattened (layers/sparse_projector.py:78-104: permute copy, torch.sparse.mm, permute copy) as
 * TruncatedConnection uses it twice (layers/residual.py:275-296), with the column selection of the residual's prognostic variables and the
 * input normaliser folded in:
 *     y[b, m, c] = sum_{e in [indptr[m], indptr[m+1])} w[e] * f(x[b, indices[e], cols[c]]),   f(v) = v * mul[c] + add[c]
 * x: [batch, n_src, n_cols_x] of x_dtype, row stride ldx in elements; the batch index b = bo * batch_inner + bi addresses x at
 * bo * bsx + bi * bsx_inner (two leading dimensions with strides of their own, batch_inner >= 1 dividing batch: the [B, E] of a time-step slice
 * of [B, T, E, N, V] is read in place); y: [batch, n_dst, C] of y_dtype (fp32 or x_dtype), row stride ldy, batch stride bsy; indptr [n_dst + 1], indices [nnz] int32 and
 * w [nnz] fp32: the CSR matrix, rows = destinations; cols: int32 [C] or NULL (the first C columns); mul, add: fp32 [C] or NULL (1 and 0).
 * Entries are summed in CSR order in fp32 without atomics (bitwise reproducible); a row without entries yields zeros; an index outside
 * [0, n_src) or a column outside [0, n_cols_x) contributes nothing and is never dereferenced. */
int anemoi_sparse_project_fwd(const void* x, int64_t ldx, int64_t bsx, int32_t batch_inner, int64_t bsx_inner, int32_t n_src, int32_t n_cols_x,
                              const int32_t* indptr,
                              const int32_t* indices, const float* w, const int32_t* cols, const float* mul, const float* add, void* y,
                              int64_t ldy, int64_t bsy, int32_t batch, int32_t n_dst, int32_t C, anemoi_dtype_t x_dtype, anemoi_dtype_t y_dtype,
                              void* stream);

/* ---- spherical-harmonic transforms and the spectral Ornstein residual (ABI 25) ----------------------------------------------------
 * A grid of K latitude rings, ring k holding n_k points at [s_k, s_k + n_k) of the flattened grid (ring_offsets: int32 [K + 1] = s_0 .. s_K,
 * device); M = L = truncation + 1, 0 < truncation <= K.  Everything is fp32 with fp32 accumulation.  Constant tables of the caller (device):
 *   twiddles  fp32 [grid, 2]: entry s_k + t = (cos, -sin)(2 pi t / n_k), built in float64 and rounded once;
 *   wleg      fp32 [L, K, M]: the quadrature-weighted normalised associated Legendre functions W[m, l, k], stored m fastest;
 *   pleg      fp32 [L, K, M]: the synthesis functions P[m, l, k], stored m fastest.
 * The grid side of either direction is addressed in place: field f = g * n_cols + c (g < n_groups, c < n_cols) lives at
 * base + g * gs + (cols ? cols[c] : c) + point * ps (elements): columns of a [G, grid, V] tensor (gs = grid V, ps = V) or the rows of a
 * [F, grid] one (n_groups = F, n_cols = 1, gs = grid, ps = 1).  coeffs: [F, L, M] complex as interleaved (re, im) fp32.  workspace: the
 * ring spectra, anemoi_sht_plan's workspace_bytes = F K M 8 bytes.  Each transform is two launches on `stream`; nothing is allocated or
 * synchronised, so a call captures into a hipGraph.  Sums run in a fixed order without atomics: bitwise reproducible. */

/* How a transform is tiled (csrc/sht_plan.h), asked without launching anything.  HOST-ONLY: no HIP call, no device needed, and
 * lons_per_lat is a HOST array of n_rings ring lengths.  direction: 0 forward, 1 inverse.  ANEMOI_E_INVALID for a truncation outside
 * [1, n_rings] or a ring without points (`out` is filled with zeros then).
 * Replaces: nothing in the reference, which launches one torch.fft call per ring (layers/spectral_helpers.py:261-262, 472-475) and has
 * no launch geometry of its own to ask about.
 *   field_tile: fields per workgroup (1, 2, 4, 8);  chunk: points (forward) or modes (inverse) the ring kernel stages per pass;
 *   lds_bytes: that kernel's dynamic LDS = field_tile chunk (4 | 8) <= lds_bound, whatever the ring length;  ring_grid: (rings, tiles of
 *   ring_threads modes | points, field tiles);  leg_grid: (tiles of 64 modes, tiles of leg_rows degrees | rings, field tiles). */
typedef struct {
  int32_t field_tile, chunk, lds_bytes, lds_bound, ring_threads, leg_rows;
  uint32_t ring_grid[3], leg_grid[3];
  int64_t workspace_bytes;
} anemoi_sht_plan_t;
int anemoi_sht_plan(int32_t direction, int32_t n_fields, const int32_t* lons_per_lat, int32_t n_rings, int32_t truncation,
                    anemoi_sht_plan_t* out);

/* Forward transform, grid -> coefficients.
 * Replaces: SphericalHarmonicTransform.forward (layers/spectral_helpers.py:317-340) with its per-ring rfft loop (:227-264) and the
 * "(b t e v) p" transposing copy of its callers (layers/spectral_transforms.py:254-261, 360-369).
 *   X[f, k, m] = (2 pi / n_k) sum_j x[f, s_k + j] exp(-2 pi i ((j m) mod n_k) / n_k) for m <= n_k / 2, 0 beyond (zero-filled, not aliased);
 *   coeffs[f, l, m] = sum_k X[f, k, m] W[m, l, k]; zeros are written where l < m.
 * max_ring = max n_k (the host does not read ring_offsets). */
int anemoi_sht_fwd(const float* x, int64_t gs, int64_t ps, const int32_t* cols, int32_t n_groups, int32_t n_cols, const int32_t* ring_offsets,
                   int32_t n_rings, int32_t max_ring, int32_t truncation, const float* twiddles, const float* wleg, float* coeffs,
                   float* workspace, int64_t workspace_bytes, void* stream);

/* Inverse transform, coefficients -> grid.
 * Replaces: InverseSphericalHarmonicTransform.forward (layers/spectral_helpers.py:530-553) with its per-ring irfft loop (:448-477), and
 * the per-degree filter multiply in front of it (layers/residual.py:549, 557).
 *   Y[f, k, m] = sum_{l >= m} coeffs[f, l, m] lscale[f % n_scale, l] P[m, l, k]         (lscale: fp32 [n_scale, L] or NULL = 1)
 *   y[f, s_k + j] = Re Y_0 + sum_{1 <= m < n_k / 2, m < M} 2 Re(Y_m exp(+2 pi i ((j m) mod n_k) / n_k)), plus Re(Y_{n_k / 2}) (-1)^j for
 *   even n_k with n_k / 2 < M: irfft(., n_k, norm="forward").  Every point of every field of y is written. */
int anemoi_sht_inv(const float* coeffs, const float* lscale, int32_t n_scale, const int32_t* ring_offsets, int32_t n_rings, int32_t max_ring,
                   int32_t truncation, const float* twiddles, const float* pleg, float* y, int64_t gs, int64_t ps, const int32_t* cols,
                   int32_t n_groups, int32_t n_cols, float* workspace, int64_t workspace_bytes, void* stream);

/* The spectral Ornstein residual's row-wise step, one launch.
 * Replaces: SpectralOrnsteinConnection._learnable and the blend of _truncate_with_anti_aliasing (layers/residual.py:546-576): two
 * rearranges, an indexed in-place assignment, the gain / mu / regressor broadcasts and the zero-filled scatter of forward (:585-588).
 *   out[g, p, c] = gain[p, c] xt + mu[p, c] + sum_i beta_i[p, c] x[g, p, reg_cols[i]],   x[g, p, v] at x + g gs + p ps + v
 *   xt = x[g, p, prog_cols[c]] where trunc_map is NULL or trunc_map[c] < 0; otherwise, with t = trunc_map[c], xt = lowpass[g, p, t]
 *   (walias NULL) or walias[p, t] x + (1 - walias[p, t]) lowpass[g, p, t].  x_filtered (NULL, or a tensor addressed like x; x itself is
 *   allowed when no regressor is a truncated column): receives xt in the truncated columns, the side effect of the reference's
 *   _apply_truncation on its caller's input (:560-563), which its model feeds to the encoder.
 * fields: fp32 [2 + n_reg, n_grid, n_prog] = gain, mu, beta_0 ..; lowpass: [n_groups, n_grid, n_trunc]; walias: [n_grid, n_trunc];
 * out: the compact skip [n_groups, n_grid, n_prog]; prog_cols [n_prog], reg_cols [n_reg], trunc_map [n_prog]: int32. */
int anemoi_ornstein_combine_fwd(const float* x, int64_t gs, int64_t ps, const int32_t* prog_cols, const int32_t* reg_cols, int32_t n_reg,
                                const float* fields, const int32_t* trunc_map, const float* lowpass, int32_t n_trunc, const float* walias,
                                float* x_filtered, float* out, int32_t n_groups, int32_t n_grid, int32_t n_prog, void* stream);

/* ---- The EDM diffusion model's edges and solver step (csrc/transport.hip).  anemoi_dtype_t has no float64: a tensor that may be held in
 * the solver's precision carries its own flag `*_f64` (0 = fp32, 1 = fp64).  Every per-call scalar - sigma, the solver's coefficients - is
 * read from DEVICE memory, so a captured launch replays for every step of a sampler.  G = batch x ensemble groups, rows ordered
 * "(batch ensemble grid)"; x, y: [B, T, E, N, V] addressed by element strides with a contiguous last dimension. ---- */

/* The conditioning rows of one denoiser call.
 * Replaces: AnemoiTransportModelEncProcDec._embed_noise_conditioning, _make_noise_emb (twice) and _generate_noise_conditioning
 * (models/transport_encoder_processor_decoder.py:138-151, 171-201), the embedders (layers/diffusion.py:23-25, 36-38), the c_noise of
 * EDMDiffusionModelObjective._get_preconditioning (transport/objectives.py:212) and the cast of _expand_scalar_condition
 * (samplers/transport_samplers.py:34-39).
 *   v = float(values[g]);  transform 1: v = log(v) / 4;  arg_j = v frequencies[j], with pi != NULL ((v f_j) 2) pi[0], every product rounded
 *   to fp32;  emb = [sin(arg) | cos(arg)] (C values);  cond = W2 silu(W1 emb + b1) + b2, fp32 accumulation;
 *   out_k[(g rows_k + r), 0:cond_dim] = cond for r < rows_k, k = 0, 1 (a NULL destination is skipped; rows_k = 1 yields cond itself).
 * w1 [C, C], b1 [C], w2 [cond_dim, C], b2 [cond_dim] in w_dtype; outputs in dtype; C even, <= 64; cond_dim <= 32 (ANEMOI_E_UNSUPPORTED
 * beyond). */
int anemoi_noise_cond_fwd(const void* values, int32_t values_f64, int32_t transform, const float* frequencies, const float* pi, const void* w1,
                          const void* b1, const void* w2, const void* b2, anemoi_dtype_t w_dtype, void* out0, int64_t rows0, int64_t ld0,
                          void* out1, int64_t rows1, int64_t ld1, int32_t G, int32_t C, int32_t cond_dim, anemoi_dtype_t dtype, void* stream);

/* The denoiser network's input rows.
 * Replaces: AnemoiTransportModelEncProcDec._assemble_input (models/transport_encoder_processor_decoder.py:99-125), the c_in y_noised of
 * EDMDiffusionModelObjective.forward (transport/objectives.py:118, 211), the cast of the sampler's y_model
 * (samplers/transport_samplers.py:159) and the zero padding of the embedding GEMM's K dimension.
 *   out[(g, n), :] = [ x[g, t, n, :] t < T_in | c_in[g] float(y[g, t, n, :]) t < T_out | attrs[n, :] | zeros up to W ]
 *   c_in[g] = 1 / sqrt(sigma_data^2 + sigma[g]^2) in fp32 (scale = 0: 1, sigma is not read).
 * x: fp32; y: fp32 or fp64; sigma [G]: fp32 or fp64, cast to fp32 first; attrs [N, A] and out [G N, W] (ldo >= W) in dtype. */
int anemoi_transport_assemble_input(const float* x, int64_t xs_b, int64_t xs_t, int64_t xs_e, int64_t xs_n, const void* y, int32_t y_f64,
                                    int64_t ys_b, int64_t ys_t, int64_t ys_e, int64_t ys_n, const void* sigma, int32_t sigma_f64,
                                    double sigma_data, int32_t scale, const void* attrs, int64_t lda, int32_t A, void* out, int64_t ldo,
                                    int32_t W, int32_t B, int32_t E, int32_t N, int32_t T_in, int32_t V_in, int32_t T_out, int32_t V_out,
                                    anemoi_dtype_t dtype, void* stream);

/* The denoised state from the network's output rows.
 * Replaces: AnemoiTransportModelEncProcDec._assemble_output (models/transport_encoder_processor_decoder.py:127-136), the
 * c_skip y_noised + c_out pred of EDMDiffusionModelObjective.forward (transport/objectives.py:124, 209-210) and the cast of the
 * sampler's D1_solver (samplers/transport_samplers.py:170, 197, 254).
 *   out[b, t, e, n, v] = c_skip[g] float(y[b, t, e, n, v]) + c_out[g] pred[(g, n), t V_out + v],  g = b E + e,
 *   c_skip = sd^2 / (sigma^2 + sd^2), c_out = sigma sd / sqrt(sigma^2 + sd^2), all in fp32 (precondition = 0: the rearrange and cast alone).
 * pred in pred_dtype (ldp >= T_out V_out); out: contiguous [B, T_out, E, N, V_out], fp32 or fp64. */
int anemoi_edm_output(const void* pred, int64_t ldp, anemoi_dtype_t pred_dtype, const void* y, int32_t y_f64, int64_t ys_b, int64_t ys_t,
                      int64_t ys_e, int64_t ys_n, const void* sigma, int32_t sigma_f64, double sigma_data, int32_t precondition, void* out,
                      int32_t out_f64, int32_t B, int32_t E, int32_t N, int32_t T_out, int32_t V_out, void* stream);

/* The solver arithmetic of one sampler step, element-wise over n values in the solver's precision.
 * Replaces: EDMHeunSampler.sample's update (samplers/transport_samplers.py:170-210) and DPMpp2MSampler.sample's
 * (samplers/transport_samplers.py:254-283).
 * params: 8 fp64 values on the device, rounded to the solver's precision first:
 *   [0] sigma_eff  [1] sigma_next  [2] eps  [3] sigma_next / sigma  [4] exp(-h) - 1  [5] c1  [6] c2  [7] round32 (modes 3, 4).
 *   mode 0 HEUN_PREDICT: d1 = (y - D) / (sigma_eff + eps); aux1 = d1; aux2 = y + (sigma_next - sigma_eff) d1
 *   mode 1 HEUN_CORRECT: d2 = (aux2 - D) / (sigma_next + eps); y += (sigma_next - sigma_eff) (aux1 + d2) / 2
 *   mode 2 HEUN_FINAL:   y = the predictor's y_next (computed from y and D; aux1, aux2 unused)
 *   mode 3 DPMPP_FIRST:  y = [3] y - [4] D; aux1 = D                 (aux1 is not read)
 *   mode 4 DPMPP_MULTI:  y = [3] y - [4] ([5] D + [6] aux1); aux1 = D
 *                        (both: with [7] != 0 the new y is rounded to fp32 first, the data dtype the reference keeps it in, :283)
 *   mode 5 DPMPP_FINAL:  y = D */
int anemoi_edm_update(int32_t mode, const double* params, void* y, const void* D, void* aux1, void* aux2, int64_t n, int32_t solver_f64,
                      void* stream);

/* ---- Backward of the three launches around the denoiser network (csrc/transport_bwd.hip): what torch autograd derives for the reference's
 * tensor expressions named above.  fp32 accumulation in a fixed order, plain stores with one owner per element, no atomics, no host
 * synchronisation, every per-call scalar read from DEVICE memory: a captured training step replays bit-equal.  The conditioning vector
 * and the EDM coefficients are the forward's own (csrc/transport_core.h). ---- */

/* Bytes of fp32 workspace anemoi_noise_cond_bwd needs: one partial per (group, 512-row tile of destination 0 then 1, column). */
int64_t anemoi_noise_cond_bwd_workspace_bytes(int64_t rows0, int64_t rows1, int32_t G, int32_t cond_dim);

/* Gradients of the noise MLP's parameters from the gradients of the conditioning rows (anemoi_noise_cond_fwd's outputs).
 *   s_g = sum_k sum_r d_out_k[(g rows_k + r), 0:cond_dim]     stage 1: one partial per (group, tile), then summed in tile order
 *   e, p = W1 e + b1, h = silu(p) recomputed as the forward computes them;  over the groups in order:
 *   d_b2 = sum_g s_g;  d_w2 = sum_g s_g h_g^T;  dh = W2^T s_g;  dp = dh sigmoid(p) (1 + p (1 - sigmoid(p)));  d_b1 = sum_g dp;
 *   d_w1 = sum_g dp e_g^T.
 * d_out_k in dtype with leading dimension ld_k (NULL or rows_k = 0: absent); rows are read with 16-byte loads when cond_dim, ld_k and the
 * base address allow.  d_w1 [C, C], d_b1 [C], d_w2 [cond_dim, C], d_b2 [cond_dim]: fp32, every element written.  There is no gradient
 * to values, frequencies or pi.  Two launches. */
int anemoi_noise_cond_bwd(const void* d_out0, int64_t rows0, int64_t ld0, const void* d_out1, int64_t rows1, int64_t ld1, anemoi_dtype_t dtype,
                          const void* values, int32_t values_f64, int32_t transform, const float* frequencies, const float* pi, const void* w1,
                          const void* b1, const void* w2, const void* b2, anemoi_dtype_t w_dtype, float* d_w1, float* d_b1, float* d_w2,
                          float* d_b2, void* workspace, int64_t workspace_bytes, int32_t G, int32_t C, int32_t cond_dim, void* stream);

/* Gradient of the node attributes anemoi_transport_assemble_input concatenates (its only differentiable operand: the trainable columns are
 * a Parameter):  d_attrs[n, a] = sum_g float(d_rows[(g N + n), col0 + a]), groups in order, fp32 accumulation, written in dtype.
 * col0 = T_in V_in + T_out V_out; the alignment columns past the attributes are not read. */
int anemoi_transport_assemble_input_bwd(const void* d_rows, int64_t ldr, int32_t col0, void* d_attrs, int64_t lda, int32_t G, int32_t N, int32_t A,
                                        anemoi_dtype_t dtype, void* stream);

/* Gradient of the network's output rows from the gradient of anemoi_edm_output's result:
 *   d_pred[(g N + n), t V_out + v] = round(c_out[g] float(d_out[b, t, e, n, v]))  (precondition = 0: c_out = 1), c_out as in the forward;
 *   d_pred[(g N + n), T_out V_out .. P - 1] = 0: the whole row of P columns is written (the decoder's backward reads all of it).
 * d_out: fp32 or fp64, read in place through its five element strides, each >= 0 (0: an expanded gradient).  There is no gradient to y or
 * sigma. */
int anemoi_edm_output_bwd(const void* d_out, int32_t d_out_f64, int64_t gs_b, int64_t gs_t, int64_t gs_e, int64_t gs_n, int64_t gs_v,
                          const void* sigma, int32_t sigma_f64, double sigma_data, int32_t precondition, void* d_pred, int64_t ldp, int32_t P,
                          anemoi_dtype_t pred_dtype, int32_t B, int32_t E, int32_t N, int32_t T_out, int32_t V_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ANEMOI_HIP_H */
