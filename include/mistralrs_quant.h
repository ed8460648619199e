/*
 * include/mistralrs_quant.h -- C ABI of libmistralrsquant.so (gfx950 / MI355X).
 *
 * Drop-in for the static library `libmistralrsquant.a` that mistralrs-quant's build.rs links
 * (mistralrs-quant/build.rs:220-228,247-249).  Every entry point below has the SAME symbol name
 * and argument list as the CUDA launcher it replaces; `stream` carries a hipStream_t where the
 * reference passes a cudaStream_t.  Rust-side declarations: mistralrs-quant/src/gguf/ffi.rs,
 * src/rotary/ffi.rs, src/utils/ffi.rs.  Reference-side binding: see INTEGRATION.md.
 *
 * Contract: the caller owns every buffer (inputs, outputs, scratch); nothing here
 * allocates or frees device memory; every call only enqueues work on `stream` (graph-capturable);
 * pointers are raw device addresses; weights are unmodified GGUF block bytes, row-major [N][K/blk].
 */
#ifndef MISTRALRS_QUANT_H
#define MISTRALRS_QUANT_H
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- activation -> Q8_1 (36-byte blocks: half d, half sum(x), 32 x int8), rows zero-padded to
 *      kx_padded (a multiple of 512: MATRIX_ROW_PADDING, fast_mmvq.rs:21).
 *      replaces mmvq_gguf.cu:1606-1641; caller: gguf/fast_mmvq.rs:340-383 */
void launch_mmvq_gguf_quantize_q8_1_bf16(const void *x, void *vy, int kx, int kx_padded, int num_rows, void *stream);
void launch_mmvq_gguf_quantize_q8_1_f16(const void *x, void *vy, int kx, int kx_padded, int num_rows, void *stream);
void launch_mmvq_gguf_quantize_q8_1_f32(const void *x, void *vy, int kx, int kx_padded, int num_rows, void *stream);

/* the MoE paths' copies of the same quantizer (kernels/indexed_moe/indexed_moe.cu:673-808,1016-1023 ; Rust: src/gguf/ffi.rs:16-60 ;
 * callers gguf/cuda.rs:514-588,1340-1640).  launch_quantize_q8_1: f32 input, grid of `num_blocks_x` blocks of 256 columns per row */
void launch_quantize_q8_1(const float *x, void *vy, int kx, int kx_padded, int num_blocks_x, int num_rows, void *stream);
void launch_quantize_q8_1_bf16(const void *x, void *vy, int kx, int kx_padded, int num_rows, void *stream);
void launch_quantize_q8_1_f16(const void *x, void *vy, int kx, int kx_padded, int num_rows, void *stream);

/* ---- decode GEMV, batch 1..8:  dst[j*stride_col_dst + row] = W[row,:] . y_j
 *      <t> in q4_0 q4_1 q5_0 q5_1 q8_0 q2_k q3_k q4_k q5_k q6_k ; <d> in f32 f16 bf16
 *      replaces mmvq_gguf.cu:1322-1600 (MMVQ_LAUNCHER_PLAIN / _FUSED_GLU / _FUSED_QKV);
 *      callers: gguf/fast_mmvq.rs:299 (plain), :472 (fused_glu), :682 (fused_qkv).
 *      ncols_x = K (unpadded), stride_col_y = Q8_1 blocks per batch column (kx_padded/32).
 *      fused_glu: dst = act(gate.y) * (up.y), activation codes 0 silu 1 gelu 2 relu 3 gelu_erf 4 sigmoid
 *      fused_qkv: X_dst[j*nrows_X + row] */
#define MRS_DECL_MMVQ(t, d)                                                                                        \
  void launch_mmvq_gguf_##t##_##d##_plain(const void *vx, const void *vy, void *dst, int ncols_x, int nrows_x,     \
                                          int stride_col_y, int stride_col_dst, int b_size, void *stream);        \
  void launch_mmvq_gguf_##t##_##d##_fused_glu(const void *vx_gate, const void *vx_up, const void *vy, void *dst,   \
                                              int ncols_x, int nrows_x, int stride_col_y, int stride_col_dst,      \
                                              int b_size, int activation, void *stream);                           \
  void launch_mmvq_gguf_##t##_##d##_fused_qkv(const void *vx_q, const void *vx_k, const void *vx_v, const void *vy, \
                                              void *q_dst, void *k_dst, void *v_dst, int ncols_x, int nrows_q,     \
                                              int nrows_k, int nrows_v, int stride_col_y, int b_size, void *stream);
#define MRS_DECL_MMVQ_T(t) MRS_DECL_MMVQ(t, f32) MRS_DECL_MMVQ(t, f16) MRS_DECL_MMVQ(t, bf16)
MRS_DECL_MMVQ_T(q4_0) MRS_DECL_MMVQ_T(q4_1) MRS_DECL_MMVQ_T(q5_0) MRS_DECL_MMVQ_T(q5_1) MRS_DECL_MMVQ_T(q8_0)
MRS_DECL_MMVQ_T(q2_k) MRS_DECL_MMVQ_T(q3_k) MRS_DECL_MMVQ_T(q4_k) MRS_DECL_MMVQ_T(q5_k) MRS_DECL_MMVQ_T(q6_k)
#undef MRS_DECL_MMVQ_T
#undef MRS_DECL_MMVQ

/* ---- indexed MoE forward: out[task][row] = W[indices[task]][row] . y[input_dim1 == 1 ? task / topk : task], task = token * topk + slot.
 *      all_weights: E stacked packed matrices [n][k / blk]; all_inputs: Q8_1 rows of k_padded / 32 blocks; all_outputs f32 [batch*topk][n].
 *      replaces kernels/indexed_moe/indexed_moe.cu:806-1157 ; Rust: src/gguf/ffi.rs:100-260 ; caller gguf/cuda.rs:514-588
 *      (qmatmul_indexed_moe_forward <- GgufMatMul::gather_forward_raw, gguf/mod.rs:485-516).  q8_1 here is Q8_1 as a WEIGHT format (ffi.rs:268): per block
 *      d_w d_x <q,u> + 4 s_w s_x, the literal result of the reference's four vec_dot_q8_1_q8_1 calls per block (indexed_moe.cu:483-502). */
#define MRS_DECL_IMOE(t)                                                                                                          \
  void launch_indexed_moe_forward_##t##_q8_1(const void *all_weights, const void *all_inputs, const unsigned int *indices,         \
                                             float *all_outputs, int n, int k, int batch, int topk, int k_padded, int input_dim1, \
                                             void *stream);
MRS_DECL_IMOE(q4_0) MRS_DECL_IMOE(q4_1) MRS_DECL_IMOE(q5_0) MRS_DECL_IMOE(q5_1) MRS_DECL_IMOE(q8_0) MRS_DECL_IMOE(q8_1)
MRS_DECL_IMOE(q2k) MRS_DECL_IMOE(q3k) MRS_DECL_IMOE(q4k) MRS_DECL_IMOE(q5k) MRS_DECL_IMOE(q6k)
#undef MRS_DECL_IMOE

/* ---- fused MoE decode pair (f32 in/out, Q8_1 activations, task = token * topk + slot, e = indices[task]):
 *        gate_up:  out[task][row]   = (up_w[e][row] . y[token]) * act(gate_w[e][row] . y[token])   act_type 0 gelu_pytorch_tanh, else silu
 *        down_agg: out[token][row] += topk_weights[task] * (w[e][row] . y[task])                    f32 atomics; caller zero-fills out
 *      replaces kernels/indexed_moe/indexed_moe.cu:1336-1477,1618-1726 ; Rust: src/gguf/ffi.rs:520-890 ; caller gguf/cuda.rs:1427-1640
 *      (moe_gemv_fused_gate_up / moe_gemv_down_aggregate <- FastExpertsWeights::forward_*, moe/experts/backends.rs:969-1100) */
#define MRS_DECL_MOE_DECODE(t)                                                                                                      \
  void launch_moe_gemv_fused_gate_up_##t##_q8_1(const void *gate_weights, const void *up_weights, const void *all_inputs,            \
                                                const unsigned int *indices, float *all_outputs, int n, int k, int batch, int topk,  \
                                                int k_padded, int act_type, void *stream);                                          \
  void launch_moe_gemv_down_aggregate_##t##_q8_1(const void *all_weights, const void *all_inputs, const unsigned int *indices,       \
                                                 const float *topk_weights, float *all_outputs, int n, int k, int batch, int topk,   \
                                                 int k_padded, void *stream);
MRS_DECL_MOE_DECODE(q4_0) MRS_DECL_MOE_DECODE(q4_1) MRS_DECL_MOE_DECODE(q5_0) MRS_DECL_MOE_DECODE(q5_1) MRS_DECL_MOE_DECODE(q8_0) MRS_DECL_MOE_DECODE(q8_1)
MRS_DECL_MOE_DECODE(q2k) MRS_DECL_MOE_DECODE(q3k) MRS_DECL_MOE_DECODE(q4k) MRS_DECL_MOE_DECODE(q5k) MRS_DECL_MOE_DECODE(q6k)
#undef MRS_DECL_MOE_DECODE

/* ---- MoE prompt path: route dispatch -> grouped GEMM -> weighted reduce.
 *      launch_moe_dispatch: counting sort of topk_ids[total_assignments] by expert: expert_bounds[num_experts + 1] (exclusive prefix of the
 *        counts), sorted_token_ids[pos] = flat route index, sorted_source_ids[pos] = flat / topk (may be NULL); expert_counts /
 *        expert_cursors [num_experts] are caller scratch and end up as counts / bounds[e + 1] like the reference's.  The order inside an
 *        expert's segment is ascending flat index (the reference's atomic cursors leave it unspecified).
 *      launch_moe_grouped_gemm_<t>: for sorted position ti in [bounds[e], bounds[e+1]), flat = sorted_token_ids[ti]:
 *        y row = input_dim1 == 0 ? ti : input_dim1 == 1 ? flat / topk : flat ;  acc = W[e][row] . y ;
 *        topk_weights ? atomicAdd(out[flat / topk][row], acc * topk_weights[flat]) : out[ti][row] = acc      (f32)
 *      launch_moe_weighted_reduce_flat*: out[token][h] = sum_slot float(in[token][slot][h]) * w[token][slot], f32 accumulate, -> int status
 *        (_flat: f32 -> f32, _flat_bf16: f32 -> bf16, _f16_input: f16 -> f16, _bf16_input: bf16 -> bf16)
 *      replaces kernels/moe_grouped/moe_grouped.cu:630-1235 ; Rust: src/gguf/ffi.rs:285-500 ; callers gguf/cuda.rs:590-930,1340-1420 */
void launch_moe_dispatch(const int32_t *topk_ids, int32_t *expert_bounds, int32_t *sorted_token_ids, int32_t *sorted_source_ids,
                         int total_assignments, int num_experts, int topk, int32_t *expert_counts, int32_t *expert_cursors, void *stream);
#define MRS_DECL_MOE_GROUPED(t)                                                                                                     \
  void launch_moe_grouped_gemm_##t(const void *all_weights, const void *all_inputs, const int32_t *expert_bounds,                    \
                                   const int32_t *sorted_token_ids, const float *topk_weights, float *all_outputs, int N, int K,     \
                                   int K_padded, int num_experts, int topk, int input_dim1, void *stream);
MRS_DECL_MOE_GROUPED(q4_0) MRS_DECL_MOE_GROUPED(q4_1) MRS_DECL_MOE_GROUPED(q5_0) MRS_DECL_MOE_GROUPED(q5_1) MRS_DECL_MOE_GROUPED(q8_0) MRS_DECL_MOE_GROUPED(q8_1)
MRS_DECL_MOE_GROUPED(q2k) MRS_DECL_MOE_GROUPED(q3k) MRS_DECL_MOE_GROUPED(q4k) MRS_DECL_MOE_GROUPED(q5k) MRS_DECL_MOE_GROUPED(q6k)
#undef MRS_DECL_MOE_GROUPED
int launch_moe_weighted_reduce_flat(const void *inputs, const float *topk_weights, void *outputs, int num_tokens, int hidden, int topk,
                                    void *stream);
int launch_moe_weighted_reduce_flat_bf16(const void *inputs, const float *topk_weights, void *outputs, int num_tokens, int hidden,
                                         int topk, void *stream);
int launch_moe_weighted_reduce_flat_f16_input(const void *inputs, const float *topk_weights, void *outputs, int num_tokens, int hidden,
                                              int topk, void *stream);
int launch_moe_weighted_reduce_flat_bf16_input(const void *inputs, const float *topk_weights, void *outputs, int num_tokens, int hidden,
                                               int topk, void *stream);

/* ---- dense (unquantized) decode GEMV:  Y[b][row] = T( sum_k A[row][k] X[b][k] + (has_bias ? bias[row] : 0) ), A [M, K], X [B, K], Y [B, M],
 *      f32 accumulation, batch_size 1..8 (anything else runs batch 1, as the reference's dispatch).
 *      replaces kernels/gemv/gemv.cu:50-282 ; Rust: src/gemv/ffi.rs:12-56 ; callers src/gemv/mod.rs:250-470 */
void launch_gemv_bf16(const void *A, const void *X, const void *bias, void *Y, int M, int K, int batch_size, bool has_bias, void *stream);
void launch_gemv_f16(const void *A, const void *X, const void *bias, void *Y, int M, int K, int batch_size, bool has_bias, void *stream);
void launch_gemv_f32(const void *A, const void *X, const void *bias, void *Y, int M, int K, int batch_size, bool has_bias, void *stream);

/* ---- RoPE, in place, arithmetic in the tensor dtype.  `rot_dim` = number of rotated PAIRS (= cos/sin row
 *      length); is_neox: pairs (i, i+rot_dim) else interleaved (2i, 2i+1); dtype 0 f16, 1 bf16, 2 f32.
 *      replaces kernels/rotary/rotary.cu:122-196 ; Rust: src/rotary/ffi.rs ; caller rotary/mod.rs:851 */
void rotary_embedding(void *query, void *key, void *cos_cache, void *sin_cache, int32_t is_neox, int32_t head_size,
                      int64_t num_tokens, int32_t rot_dim, int32_t num_heads, int32_t num_kv_heads, int64_t query_stride,
                      int64_t key_stride, uint32_t dtype, int64_t stream);
void rotary_embedding_positions(void *query, void *key, void *cos_cache, void *sin_cache, void *positions,
                                int32_t is_neox, int32_t head_size, int64_t num_tokens, int32_t rot_dim, int32_t seq_len,
                                int32_t num_heads, int32_t num_kv_heads, int64_t query_stride, int64_t key_stride,
                                uint32_t dtype, int64_t stream);

/* ---- out = T(act(float a)) * b, strided rows.  replaces kernels/ops/ops.cu:946-971 ; Rust: src/utils/ffi.rs:274-306 */
void fused_glu_f16(const void *a, const void *b, void *output, uint32_t rows, uint32_t cols, uint32_t a_row_stride,
                   uint32_t b_row_stride, int activation, void *stream);
void fused_glu_bf16(const void *a, const void *b, void *output, uint32_t rows, uint32_t cols, uint32_t a_row_stride,
                    uint32_t b_row_stride, int activation, void *stream);
void fused_glu_f32(const void *a, const void *b, void *output, uint32_t rows, uint32_t cols, uint32_t a_row_stride,
                   uint32_t b_row_stride, int activation, void *stream);

/* ---- MMQ: prompt-sized quantized matmul behind fast_mmq.rs (shared_lhs / fused_qkv / fused_glu / fused_ffn, gguf/fast_mmq.rs:388-447,528-821).
 *      Step 1, activations -> block_q8_1_mmq (144 B per 128 values: 16 header bytes + 128 x int8; block index (i0/128)*ne1 + i1; header
 *      D4 = 4 x f32 d, DS4 = 4 x (half d, half sum x), D2S6 = 2 x half d (per 64) + 6 x half sum (per 16, first 96 values); kernels/mmq_gguf/
 *      mmq_gguf.cuh:64-89).  x [ne1 rows][s01 stride] of type_x (0 = f32, 1 = f16, 30 = bf16), `ids` optional row gather, ne00 = K,
 *      ne0 = padded K.  The _glu variants quantize activation(gate) * up (product formed in the input dtype).
 *      replaces kernels/mmq_gguf/mmq_quantize.cu:104-198,236-325 (kernels), :386-476 (launchers); Rust: src/gguf/ffi.rs:1313-1408 */
#define MRS_DECL_MMQ_QUANTIZE(L)                                                                                                               \
  void launch_mmq_quantize_q8_1_##L(const void *x, const int32_t *ids, void *vy, int type_x, int64_t ne00, int64_t s01, int64_t s02, int64_t s03, \
                                    int64_t ne0, int64_t ne1, int64_t ne2, int64_t ne3, void *stream);                                           \
  void launch_mmq_quantize_glu_q8_1_##L##_f32(const float *gate, const float *up, const int32_t *ids, void *vy, int64_t ne00, int64_t s01,       \
                                              int64_t ne0, int64_t ne1, int activation, void *stream);                                           \
  void launch_mmq_quantize_glu_q8_1_##L(const void *gate, const void *up, const int32_t *ids, void *vy, int type_x, int64_t ne00, int64_t s01,   \
                                        int64_t ne0, int64_t ne1, int activation, void *stream);
MRS_DECL_MMQ_QUANTIZE(D4) MRS_DECL_MMQ_QUANTIZE(DS4) MRS_DECL_MMQ_QUANTIZE(D2S6)
#undef MRS_DECL_MMQ_QUANTIZE
/*      Step 2, dst[col * nrows_x + row] = W[row, :] . y_col  (type_dst 0 = f32, 1 = f16, 30 = bf16); the layout of y is fixed by <t>:
 *      DS4 for q4_0 q4_1 q5_1 q4_k q5_k, D2S6 for q2_k, D4 for q5_0 q8_0 q3_k q6_k (mmq_gguf.cuh:100-135).  stride_row_x in blocks.
 *      tmp_fixup / cc / nsm / smpbo / warp_size belong to the reference's stream-k tiling and are accepted and ignored.  _moe: y columns are
 *      the routes in expert-sorted order, expert e owns [expert_bounds[e], expert_bounds[e+1]) and channel e of x, column j lands in dst
 *      column ids_dst[j] (f32, column stride stride_col_dst).
 *      replaces kernels/mmq_gguf/mmq_instance_<t>.cu:216-259 and DEFINE_MMQ_MOE_LAUNCHER (mmq_gguf.cuh:3968-4010); Rust: ffi.rs:1410-1452,
 *      callers fast_mmq.rs:421-437 (dense), gguf/cuda.rs (grouped MoE prompt path).  MI355X note: these entry points keep fast_mmq.rs linking and
 *      numerically equivalent (integer dots on the stored Q8_1 images and partial sums), as LDS-tiled i8 MFMA kernels (csrc/mmq.hip,
 *      profiles/round3_mmq.md); the C++ runner's own prompt paths are mrs_gemm_qi (the decode engine's arithmetic, default) and the fused
 *      block-dequant -> bf16 MFMA GEMM mrs_gemm_q_* (selectable), both in include/mrs_hip_ext.h. */
#define MRS_DECL_MMQ(t)                                                                                                                        \
  void launch_mmq_gguf_##t(void *tmp_fixup, const void *x, const void *y, void *dst, int64_t ncols_x, int64_t nrows_x, int64_t ncols_y,          \
                           int64_t stride_row_x, int64_t stride_col_dst, int cc, int nsm, int64_t smpbo, int warp_size, int type_dst,            \
                           void *stream);                                                                                                        \
  void launch_mmq_gguf_##t##_moe(void *tmp_fixup, const void *x, const void *y, const int32_t *ids_dst, const int32_t *expert_bounds, void *dst, \
                                 int64_t ncols_x, int64_t nrows_x, int64_t ncols_dst, int64_t stride_row_x, int64_t stride_col_dst,              \
                                 int64_t num_experts, int64_t ncols_max, int cc, int nsm, int64_t smpbo, int warp_size, void *stream);
MRS_DECL_MMQ(q4_0) MRS_DECL_MMQ(q4_1) MRS_DECL_MMQ(q5_0) MRS_DECL_MMQ(q5_1) MRS_DECL_MMQ(q8_0)
MRS_DECL_MMQ(q2_k) MRS_DECL_MMQ(q3_k) MRS_DECL_MMQ(q4_k) MRS_DECL_MMQ(q5_k) MRS_DECL_MMQ(q6_k)
#undef MRS_DECL_MMQ

/* ---- HQQ: unpack + dequantize (axis-0 groups).  Wq [h][w] packed (u8; i32 with ten 3-bit fields for 3 bit), scale / zero [w] of the
 *      output dtype, out [P*h][w], P = 1/2/4/8/10 values per packed element, most significant first:
 *          out[(c*h + r)*w + j] = (T(q_c(r, j)) - zero[j]) * scale[j]     evaluated in T
 *      NO stream argument (default stream), as the reference.  replaces kernels/hqq/hqq.cu:26-80,94-155,171-230,278-345,399-468 ;
 *      Rust: src/hqq/ffi.rs:1-74 ; caller HqqLayer::dequantize (hqq/mod.rs:874-1090) <- forward / dequantize_w (:1092-1100,1163-1171) */
#define MRS_DECL_HQQ(name)                                                                                     \
  void dequantize_##name##_f32(const void *wq_packed, const void *scale, const void *zero, void *out, int h, int w);  \
  void dequantize_##name##_f16(const void *wq_packed, const void *scale, const void *zero, void *out, int h, int w);  \
  void dequantize_##name##_bf16(const void *wq_packed, const void *scale, const void *zero, void *out, int h, int w);
MRS_DECL_HQQ(8bit_u8_kernel) MRS_DECL_HQQ(4bit_u8_kernel) MRS_DECL_HQQ(2bit_u8_kernel) MRS_DECL_HQQ(1bit_u8_kernel) MRS_DECL_HQQ(3bit_32_kernel)
#undef MRS_DECL_HQQ
/* ---- HQQ bit packing: input [num_input_elements rows][input_width] of unpacked values, output row r packs rows r + i*step
 *      (step = rows / P), i = 0 most significant.  replaces kernels/hqq/hqq_bitpack.cu:7-206 ; Rust: src/hqq/bitpack_ffi.rs:1-40 ;
 *      caller HqqBits::bitpack_type (hqq/mod.rs:150-400) */
void launch_pack_1bit_kernel(const uint8_t *d_input, uint8_t *d_output, size_t num_input_elements, size_t input_width, void *stream);
void launch_pack_2bit_kernel(const uint8_t *d_input, uint8_t *d_output, size_t num_input_elements, size_t input_width, void *stream);
void launch_pack_3bit_kernel(const uint32_t *d_input, int32_t *d_output, size_t num_input_elements, size_t input_width, void *stream);
void launch_pack_4bit_kernel(const uint8_t *d_input, uint8_t *d_output, size_t num_input_elements, size_t input_width, void *stream);
void launch_pack_8bit_kernel(const uint8_t *d_input, uint8_t *d_output, size_t num_elements, void *stream);

/* ---- MXFP4 (GPT-OSS): out = input . W^T (+ bias) straight from the packed tensor.  weight [N][K/2] u8, two E2M1 values per byte (low nibble =
 *      element k, high nibble = k + 1; magnitudes {0, .5, 1, 1.5, 2, 3, 4, 6}, bit 3 = sign); weight_scale [N][K/32] u8 E8M0, scale byte s means
 *      f32_from_bits(s << 23) (s = 0 -> 0.0; s = 255 is outside the contract); K % 32 == 0.  Products exact in f32, f32 accumulation, bias added in
 *      f32 after the K sum, one rounding to the output type.  MoE: weights [E][N][K/2], weight_scales [E][N][K/32], biases [E][N], indices
 *      [num_tokens][topk] u32, output [num_tokens][topk][N]; input [num_tokens][K] (every slot of a token reads the same row) or, with
 *      input_has_topk_dim, [num_tokens][topk][K]; an expert id >= num_experts reads nothing and leaves its output row untouched.  The indexed and the
 *      grouped entry points compute the same result for any num_tokens (the reference takes the grouped one when num_tokens > 1, ops.rs:380-400).
 *      The *_wmma_* entry points of ffi.rs:33-57,129-161 are gated behind has_mxfp4_wmma_kernels there and are not part of this library.
 *      replaces kernels/mxfp4/mxfp4_gemm.cu ; Rust: src/mxfp4/ffi.rs:7-31,59-127 ; callers mxfp4/ops.rs:16-214 (mxfp4_matmul), :313-614
 *      (mxfp4_indexed_moe_gemm) <- MXFP4Layer::forward_raw / gather_forward_raw (mxfp4/mod.rs:106-182) */
void launch_mxfp4_matmul_f16(const void *input, const uint8_t *weight, const uint8_t *weight_scale, const void *bias, void *output, int M, int N, int K,
                             bool has_bias, void *stream);
void launch_mxfp4_matmul_bf16(const void *input, const uint8_t *weight, const uint8_t *weight_scale, const void *bias, void *output, int M, int N, int K,
                              bool has_bias, void *stream);
void launch_mxfp4_indexed_moe_gemm_f16(const void *input, const uint8_t *weights, const uint8_t *weight_scales, const void *biases, const uint32_t *indices,
                                       void *output, int num_tokens, int topk, int num_experts, int N, int K, bool has_bias, bool input_has_topk_dim, void *stream);
void launch_mxfp4_indexed_moe_gemm_bf16(const void *input, const uint8_t *weights, const uint8_t *weight_scales, const void *biases, const uint32_t *indices,
                                        void *output, int num_tokens, int topk, int num_experts, int N, int K, bool has_bias, bool input_has_topk_dim, void *stream);
void launch_mxfp4_moe_grouped_gemm_f16(const void *input, const uint8_t *weights, const uint8_t *weight_scales, const void *biases, const uint32_t *indices,
                                       void *output, int num_tokens, int topk, int num_experts, int N, int K, bool has_bias, bool input_has_topk_dim, void *stream);
void launch_mxfp4_moe_grouped_gemm_bf16(const void *input, const uint8_t *weights, const uint8_t *weight_scales, const void *biases, const uint32_t *indices,
                                        void *output, int num_tokens, int topk, int num_experts, int N, int K, bool has_bias, bool input_has_topk_dim, void *stream);
/*      LDS bytes one workgroup may use on the current device (the device attribute; mxfp4/ffi.rs:93, caller ops.rs:379) */
int mxfp4_get_max_smem_optin(void);
/* MI355X-native addition (not in the reference ABI): the route of the last mxfp4 launch of this process -- 1 streaming GEMV (M <= 8), 2 bf16 MFMA tile,
 * 3 per-slot MoE GEMV, 4 grouped MoE tile, 5 f16 dense in GEMV chunks of 8 rows; see csrc/mxfp4.hip */
int mxfp4_last_route(void);

/* ---- Blockwise FP8 (HF `quant_method: fp8, fmt: e4m3, weight_block_size: [bsy, bsx]`): weight [N][K] bytes, OCP E4M3FN (bias 7, no infinities, 0x7f / 0xff NaN,
 *      max 448); scale f32 [ceil(N / bsy)][scale_row_stride], element (n, k) uses scale[(n / bsy) * stride + k / bsx]; block sizes are any positive integers and
 *      N, K, height, width need not be multiples of them.  Experts: weights [E][N][K], the scale of expert e starts at e * ceil(N / bsy) * scale_row_stride.
 *      Dequantize: out[pos] = T(f32(w[pos]) * scale), pos = y * weight_row_stride + x: one f32 product, one conversion (a NaN byte gives NaN).
 *      Quantize: scale = max(absmax / 448, 1e-12) (correctly rounded f32 division, absmax over the block's in-range elements), q = e4m3_satfinite_rne(f16_rne(
 *      clamp(f32(v) / scale, +-448))) -- the f32 -> f16 -> e4m3 double rounding is the reference's; inputs are finite.
 *      Matmul / MoE: out = input . W^T, no bias (the layer adds it in T afterwards).  Every product exact in f32; the products of one scale block are summed
 *      in f32, that partial sum enters the running f32 sum as fma(scale, partial, total); one rounding to the output type.  indices [num_tokens][topk] u32,
 *      output [num_tokens][topk][N]; input [num_tokens][K] or, with input_has_topk_dim, [num_tokens][topk][K]; an expert id >= num_experts reads nothing and
 *      leaves its output row untouched.  Activation pointers need only their element's alignment.  Fast routes need K % 16 == 0, block_size_x % 16 == 0 and
 *      a 16-byte aligned weight base; anything else takes a correct, untuned kernel (csrc/blockwise_fp8.hip).
 *      The sm90 entry points of ffi.rs (mistralrs_cutlass_fp8_*, mistralrs_deepgemm_*, mistralrs_fp8_quantize_activation_*) are gated behind cfgs a HIP build
 *      leaves unset and are not part of this library.
 *      replaces kernels/blockwise_fp8/blockwise_fp8.cu, blockwise_fp8_gemm.cu ; Rust: src/blockwise_fp8/ffi.rs:127-271 ; callers blockwise_fp8/ops.rs
 *      (fp8_blockwise_dequantize, fp8_blockwise_quantize, fp8_blockwise_matmul, fp8_indexed_moe_gemm) <- BlockwiseFP8Linear (blockwise_fp8/mod.rs:180-317) */
#define MRS_DECL_FP8BW(tag)                                                                                                                                  \
  void launch_dequant_fp8_blockwise_kernel_##tag(const uint8_t *d_weight, const float *d_scale, void *d_output, int weight_height, int weight_width,          \
                                                 int weight_row_stride, int scale_stride, int weight_block_size_y, int weight_block_size_x, void *stream);   \
  void launch_quant_fp8_blockwise_kernel_##tag(const void *d_input, uint8_t *d_weight, float *d_scale, int weight_height, int weight_width,                   \
                                               int weight_row_stride, int scale_stride, int weight_block_size_y, int weight_block_size_x, void *stream);
MRS_DECL_FP8BW(f32) MRS_DECL_FP8BW(f16) MRS_DECL_FP8BW(bf16)
#undef MRS_DECL_FP8BW
void launch_fp8_matmul_f16(const void *input, const uint8_t *weight, const float *weight_scale, void *output, int M, int N, int K, int scale_row_stride,
                           int block_size_y, int block_size_x, void *stream);
void launch_fp8_matmul_bf16(const void *input, const uint8_t *weight, const float *weight_scale, void *output, int M, int N, int K, int scale_row_stride,
                            int block_size_y, int block_size_x, void *stream);
void launch_fp8_indexed_moe_gemm_f16(const void *input, const uint8_t *weights, const float *weight_scales, const uint32_t *indices, void *output, int num_tokens,
                                     int topk, int num_experts, int N, int K, int scale_row_stride, int block_size_y, int block_size_x, bool input_has_topk_dim,
                                     void *stream);
void launch_fp8_indexed_moe_gemm_bf16(const void *input, const uint8_t *weights, const float *weight_scales, const uint32_t *indices, void *output, int num_tokens,
                                      int topk, int num_experts, int N, int K, int scale_row_stride, int block_size_y, int block_size_x, bool input_has_topk_dim,
                                      void *stream);
/* MI355X-native addition (not in the reference ABI): the route of the last blockwise-FP8 matmul / MoE launch of this process -- 1 streaming GEMV (M <= 8),
 * 2 16-bit MFMA tile, 3 per-slot MoE GEMV, 4 grouped MoE tile, 5 general (unaligned K / block size / base); see csrc/blockwise_fp8.hip */
int fp8_blockwise_last_route(void);

/* ---- AFQ (affine 2/3/4/6/8-bit, the MLX checkpoint format; `--isq 2|3|4|6|8`): w_q u32 [N][K * bits / 32], element j of a row in bits [j * bits, (j + 1) * bits) of
 *      the row's little-endian bit stream (3- and 6-bit codes may straddle two words; the byte-wise view of the 3- / 6-bit symbols is the same stream; a row is
 *      4-byte aligned only); scales / biases T [N][K / group], group 32 / 64 / 128, K % group == 0; weight = q * scale + bias.
 *      Dequantize / embedding: T(fmaf(q, scale, bias)), one conversion.  Quantize: the reference's CPU rule (afq/ops.rs:1534-1622) for every width: scale =
 *      (max - min) / (2^bits - 1) (1 when |max - min| < 1e-12), bias = min, q = clamp(roundf((w - bias) / scale)), true f32 divisions, f32 scale and bias.
 *      qmv / qmm: y [m][n] = x [m][k] . W^T; both names dispatch by m: streaming GEMV (m <= 8), code-operand MFMA tile (bf16 / f16), GEMV chunks (f32).
 *      f32 accumulation in the grouped form sum_g (s_g sum x q + b_g sum x), one rounding to T.  NO stream argument (null stream), as the reference.
 *      replaces kernels/afq/afq.cu, afq_gemm.cu ; Rust: src/afq/ffi.rs ; callers afq/ops.rs (afq_quantize_op, afq_dequantize_op, afq_embedding_op, afq_mm_op)
 *      <- AfqLayer (afq/mod.rs) */
#define MRS_DECL_AFQ(B, G, T, tag, WQ)                                                                                                                 \
  void afq_dequantize_##B##bit_gs##G##_##tag(const WQ *w_q, const T *scales, const T *biases, T *output, int rows, int cols);                          \
  void afq_embedding_##B##bit_gs##G##_##tag(const uint8_t *w_q, const T *scales, const T *biases, const uint32_t *ids, T *output, int num_ids, int hidden); \
  void afq_qmv_##B##bit_gs##G##_##tag(const T *x, const WQ *w_q, const T *scales, const T *biases, T *y, int m, int n, int k);
#define MRS_DECL_AFQ_P2(B, G, T, tag)                                                                                                                  \
  MRS_DECL_AFQ(B, G, T, tag, uint32_t)                                                                                                                 \
  void afq_quantize_##B##bit_gs##G##_##tag(const T *w, uint32_t *w_q, T *scales, T *biases, int rows, int cols);                                       \
  void afq_qmm_##B##bit_gs##G##_##tag(const T *x, const uint32_t *w_q, const T *scales, const T *biases, T *y, int m, int n, int k);
#define MRS_DECL_AFQ_G(G, T, tag)                                                                                                                      \
  MRS_DECL_AFQ_P2(2, G, T, tag) MRS_DECL_AFQ(3, G, T, tag, uint8_t) MRS_DECL_AFQ_P2(4, G, T, tag) MRS_DECL_AFQ(6, G, T, tag, uint8_t) MRS_DECL_AFQ_P2(8, G, T, tag)
#define MRS_DECL_AFQ_T(T, tag) MRS_DECL_AFQ_G(32, T, tag) MRS_DECL_AFQ_G(64, T, tag) MRS_DECL_AFQ_G(128, T, tag)
MRS_DECL_AFQ_T(float, f32)
MRS_DECL_AFQ_T(uint16_t, f16)  /* IEEE half bits */
MRS_DECL_AFQ_T(uint16_t, bf16) /* bfloat16 bits */
#undef MRS_DECL_AFQ_T
#undef MRS_DECL_AFQ_G
#undef MRS_DECL_AFQ_P2
#undef MRS_DECL_AFQ
/* MI355X-native additions (not in the reference ABI): the stream-taking launchers behind the symbols above and behind mrs_afq_matmul /
 * mrs_afq_indexed_moe_gemm of include/mrs_hip_ext.h (same arguments, see there), and the route of the last AFQ matmul / MoE launch of this process -- 1 streaming
 * GEMV (M <= 8), 2 code-operand MFMA tile, 3 per-slot MoE GEMV, 4 grouped MoE tile, 5 f32 dense in GEMV chunks of 8 rows; see csrc/afq.hip */
int launch_afq_matmul(const void *x, const void *w_q, const void *scales, const void *biases, const void *bias, void *y, int M, int N, int K, int bits, int group,
                      int dtype, void *stream);
int launch_afq_indexed_moe_gemm(const void *x, const void *w_q, const void *scales, const void *biases, const void *bias, const uint32_t *indices, void *y,
                                int num_tokens, int topk, int num_experts, int N, int K, int bits, int group, int dtype, int input_has_topk_dim, void *stream);
int afq_last_route(void);

/* ---- GPTQ / AWQ (`quantization_config.quant_method` "gptq" / "awq"): qweight u32 [K * bits / 32][N], column n holds its K codes as one little-endian bit stream
 *      down the rows (3-bit codes 10 and 21 of every 32 straddle two words); qzeros u32 [G][N * bits / 32], the same stream along N; scales f16 [G][N]; g_idx i32
 *      [K], any map from row to group (act-order), values in [0, G) (not checked here); bits 2 / 3 / 4 / 8; K % 32 == 0, N % 32 == 0.
 *      W[k][n] = f16_rne((q - (z + 1)) * s), z + 1 not wrapped: one f16 multiply of an exact integer, the value of the reference's reconstruct_gptq.
 *      reconstruct_gptq: out f16 [size_k][size_n] row-major.  gemm_half_q_half_alt: out [m][n] = f16_rne(sum_k a[m][k] W[k][n]) with f32 accumulation, every
 *      element written once by a plain store (the reference accumulates in f16 with atomicAdd into a zeroed output); any m (streaming GEMV for m <= 8, f16 MFMA
 *      tile above) and bits 2 / 3 / 4 / 8 (the reference: 4 / 8).  NO stream argument (null stream), as the reference.
 *      reconstruct_exllama and gemm_half_q_half_cuda_part are NOT declared: they take exllama-shuffled weights, and the reference's gptq_linear always builds its
 *      layers with use_exllama = false; the Marlin routes are an NVIDIA layout.
 *      replaces kernels/gptq/q_gemm.cu ; Rust: src/gptq/ffi.rs ; caller GptqLayer::gptq_gemm (gptq/gptq_cuda.rs:176-283) */
void reconstruct_gptq(const uint32_t *b_q_weight, const uint32_t *b_qzeros, const uint16_t *b_scales, const int *b_q_perm, uint16_t *out, int size_k, int size_n,
                      int groups, int bit);
void gemm_half_q_half_alt(const uint16_t *a, const uint32_t *b_q_weight, const uint32_t *b_qzeros, const uint16_t *b_scales, const int *b_g_idx, uint16_t *out, int m,
                          int n, int k, int bit);
/* MI355X-native additions (not in the reference ABI): the stream-taking launchers behind the symbols above and behind mrs_gptq_matmul / mrs_gptq_reconstruct /
 * mrs_awq_repack of include/mrs_hip_ext.h (same arguments, see there); zero_offset is 1 for GPTQ tensors and 0 for AWQ tensors after launch_awq_repack.  Each
 * returns 0, or -1 for arguments outside the kernels (-2 / -3: launch too large / launch error).  gptq_last_route: the route of the last GPTQ matmul of this
 * process -- 1 streaming GEMV (M <= 8), 2 f16 MFMA tile; see csrc/gptq.hip */
int launch_gptq_matmul(const void *x, const void *qweight, const void *qzeros, const void *scales, const void *g_idx, const void *bias, void *y, int M, int N, int K,
                       int groups, int bits, int zero_offset, void *stream);
int launch_gptq_reconstruct(const void *qweight, const void *qzeros, const void *scales, const void *g_idx, void *out, int K, int N, int groups, int bits,
                            int zero_offset, void *stream);
int launch_awq_repack(const void *qweight, const void *qzeros, void *qweight_out, void *qzeros_out, void *g_idx_out, int K, int N, int groups, int group_size,
                      int bits, void *stream);
int gptq_last_route(void);

/* MI355X-native addition (not in the reference ABI): tile policy of the int8-MFMA MMQ kernels, see csrc/mmq.hip */
void mrs_mmq_set_small_tiles_below(int n);

#ifdef __cplusplus
}
#endif
#endif
