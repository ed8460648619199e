/*
 * include/mistralrs_paged_attn.h -- C ABI of libmistralrspagedattention.so (gfx950 / MI355X).
 *
 * Drop-in for `libmistralrspagedattention.a` (mistralrs-paged-attn/build.rs:146-158,213-215).
 * Same symbols and argument lists as mistralrs-paged-attn/src/cuda/ffi.rs; `stream` is a hipStream_t.
 * dtype codes: 0 = f16, 1 = bf16, 2 = f32, 3 = fp8-e4m3 cache (OCP E4M3FN; block sizes 16 / 32; needs k_scale / v_scale:
 * stored = fp8_sat_rne(x / scale), read as T(float(fp8) * scale), quantization/fp8/nvidia/quant_utils.cuh:24-29,187-217).
 * Cache layouts (mistralrs-core/src/paged_attention/cache_engine.rs:458-484):
 *   K cache [num_blocks, kv_heads, head_size/x, block_size, x],  x = 16 / sizeof(cache element)
 *   V cache [num_blocks, kv_heads, head_size, block_size]
 * Launch errors terminate the process like the reference's CUDA_CHECK (reshape_and_cache_kernel.cu:16-24).
 */
#ifndef MISTRALRS_PAGED_ATTN_H
#define MISTRALRS_PAGED_ATTN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
typedef void *mrs_stream_t; /* hipStream_t */

/* ffi.rs:96-116 ; kernel reshape_and_cache_kernel.cu.  slot < 0 (= _PAD_SLOT_ID) is skipped. */
void reshape_and_cache(void *key, void *value, void *key_cache, void *value_cache, int64_t *slot_mapping,
                       int32_t num_tokens, int32_t num_heads, int32_t head_size, int32_t block_size, int32_t x,
                       int32_t key_stride, int32_t value_stride, mrs_stream_t stream, uint32_t dtype,
                       uint32_t cache_dtype, float *k_scale, float *v_scale);

/* ffi.rs:248-267 ; gather_kv_cache_kernel.cu: paged -> dense [num_tokens, kv_heads, head_size] */
void gather_kv_cache(void *key_cache, void *value_cache, void *k_out, void *v_out, float *k_scale, float *v_scale,
                     const int *block_table, const int *cu_seq_lens, int32_t num_tokens, int32_t num_seqs,
                     int32_t block_size, int32_t block_table_stride, int32_t num_kv_heads, int32_t head_size, int32_t x,
                     mrs_stream_t stream, uint32_t out_dtype, uint32_t cache_dtype);

/* ffi.rs:269-348 ; pagedattention_v1_*.cu.  One query token per sequence. softcapping == 1.0 disables it. */
#define MRS_DECL_PA_V1(d)                                                                                           \
  void paged_attention_v1_##d(void *out, void *query, void *key_cache, void *value_cache, void *alibi_slopes,       \
                              int32_t num_kv_heads, float scale, float softcapping, uint32_t *block_tables,         \
                              uint32_t *context_lens, int32_t block_size, int32_t max_context_len, int32_t num_seqs, \
                              int32_t num_heads, int32_t head_size, int32_t max_num_blocks_per_seq, int32_t q_stride, \
                              int32_t kv_block_stride, int32_t kv_head_stride, mrs_stream_t stream,                  \
                              uint32_t cache_dtype, float *k_scale, float *v_scale, const float *sinks);
MRS_DECL_PA_V1(f16) MRS_DECL_PA_V1(bf16) MRS_DECL_PA_V1(f32)
#undef MRS_DECL_PA_V1

/* ffi.rs:350-438 ; pagedattention_v2_*.cu: 512-token partitions + log-sum-exp merge.
 * exp_sums/max_logits [seqs, heads, parts] f32, tmp_out [seqs, heads, parts, head_size] in the query dtype,
 * parts = ceil(max_context_len / 512) (backend/paged_attention.rs:353-365). */
#define MRS_DECL_PA_V2(d)                                                                                            \
  void paged_attention_v2_##d(void *out, float *exp_sums, float *max_logits, void *tmp_out, void *query,             \
                              void *key_cache, void *value_cache, void *alibi_slopes, int32_t num_kv_heads,          \
                              float scale, float softcapping, uint32_t *block_tables, uint32_t *context_lens,        \
                              int32_t block_size, int32_t max_context_len, int32_t num_seqs, int32_t num_heads,      \
                              int32_t head_size, int32_t max_num_blocks_per_seq, int32_t q_stride,                   \
                              int32_t kv_block_stride, int32_t kv_head_stride, mrs_stream_t stream,                  \
                              uint32_t cache_dtype, float *k_scale, float *v_scale, const float *sinks);
MRS_DECL_PA_V2(f16) MRS_DECL_PA_V2(bf16) MRS_DECL_PA_V2(f32)
#undef MRS_DECL_PA_V2

/* ffi.rs:440-... ; copy_blocks_kernel.cu: block_mapping = int64 (src, dst) pairs; *_cache_ptrs = per-layer base addresses */
void copy_blocks_bf16(void *key_cache_ptrs, void *value_cache_ptrs, const void *block_mapping, int32_t num_layers,
                      int32_t num_pairs, int32_t numel_per_block_key, int32_t numel_per_block_value, int64_t stream);
void copy_blocks_f16(void *key_cache_ptrs, void *value_cache_ptrs, const void *block_mapping, int32_t num_layers,
                     int32_t num_pairs, int32_t numel_per_block_key, int32_t numel_per_block_value, int64_t stream);
void copy_blocks_f32(void *key_cache_ptrs, void *value_cache_ptrs, const void *block_mapping, int32_t num_layers,
                     int32_t num_pairs, int32_t numel_per_block_key, int32_t numel_per_block_value, int64_t stream);
void copy_blocks_u8(void *key_cache_ptrs, void *value_cache_ptrs, const void *block_mapping, int32_t num_layers,
                    int32_t num_pairs, int32_t numel_per_block_key, int32_t numel_per_block_value, int64_t stream);

/* MI355X-native (not in the reference): explicit (query dtype, cache dtype) pair -- f32 activations over a
 * bf16 cache for the fused decode path.  v2 != 0 selects the partitioned kernel + reduce. */
void mrs_paged_attention_f32_bf16(int v2, void *out, float *exp_sums, float *max_logits, void *tmp_out, const void *query,
                                  const void *key_cache, const void *value_cache, const void *alibi_slopes,
                                  int num_kv_heads, float scale, float softcapping, const uint32_t *block_tables,
                                  const uint32_t *context_lens, int block_size, int max_context_len, int num_seqs,
                                  int num_heads, int head_size, int max_num_blocks_per_seq, int q_stride,
                                  int kv_block_stride, int kv_head_stride, void *stream, const float *sinks);
/* MI355X-native decode attention of the fused path: split-KV (one wave per 32-token KV chunk of a GQA group), then one
 * merge kernel that writes the result as Q8_1 blocks (o_proj's activation format).  Replaces the run
 * paged_attention_v1/v2 -> launch_mmvq_gguf_quantize_q8_1 of the reference decode step (paged_attention.rs:1477-1561,
 * fast_mmvq.rs:340-383).  Workspace sizes use max_parts = mrs_decode_attention_max_splits(max_context_len).  Returns 0, or -1 if the shape is
 * not supported (block_size 32, head_size 64/128). */
int mrs_decode_attention_max_splits(int max_context_len);
int mrs_decode_attention_q8_1_f32_bf16(void *y_q8_1, int y_stride_blocks, float *exp_sums, float *max_logits, void *tmp_out,
                                       const void *query, const void *key_cache, const void *value_cache, int num_kv_heads,
                                       float scale, const uint32_t *block_tables, const uint32_t *context_lens, int block_size,
                                       int max_context_len, int num_seqs, int num_heads, int head_size,
                                       int max_num_blocks_per_seq, int q_stride, int kv_block_stride, int kv_head_stride,
                                       void *stream);
/* decode engine: the same split-KV kernel with f32 probabilities (reference CPU path) and an f32 result out [seqs][heads * 128];
 * kv_dtype 1 = bf16 pages, 0 = f16 pages; head_size 128, block_size 32 */
int mrs_decode_attention_f32_f32_bf16(float *out, float *exp_sums, float *max_logits, void *tmp_out, const void *query, const void *key_cache,
                                      const void *value_cache, int num_kv_heads, float scale, const uint32_t *block_tables,
                                      const uint32_t *context_lens, int block_size, int max_context_len, int num_seqs, int num_heads, int head_size,
                                      int max_num_blocks_per_seq, int q_stride, int kv_block_stride, int kv_head_stride, int kv_dtype, void *stream);
/* ffi.rs:484-510 ; update_kvscales.cu:46-150: *k_scales = max(*k_scales, absmax(k) / 240), same for v (fp8 KV-cache scale tracking,
 * backend/scale_update.rs:81-105); k, v: num_elements values of the named dtype */
void update_kv_scales_f32(void *k, void *v, const long num_elements, float *k_scales, float *v_scales, int64_t stream);
void update_kv_scales_f16(void *k, void *v, const long num_elements, float *k_scales, float *v_scales, int64_t stream);
void update_kv_scales_bf16(void *k, void *v, const long num_elements, float *k_scales, float *v_scales, int64_t stream);

/* ffi.rs `flash_attn_sinks_*` ; flash_attn_sinks.cu: causal prompt attention with per-head sinks on dense tensors.
 * Q, O [B, H, q_len, D]; K, V [B, Hkv, kv_len, D]; sinks f32 [H] or NULL; window_size 0 = causal only.  The mask is aligned to the
 * bottom right: row r attends keys max(0, r + kv_len - q_len - W + 1) .. r + kv_len - q_len.  D in 64/80/96/112/128/192/256, anything
 * else launches nothing.  varlen: Q, O padded [B, H, max_q_len, D]; K, V packed [total_kv, Hkv, D]; cu_seqlens_* u32 [B + 1]; rows
 * past a sequence's q length are not written. */
#define MRS_DECL_FAS(d)                                                                                                \
  void flash_attn_sinks_##d(const void *Q, const void *K, const void *V, void *O, const float *sinks, float scale,     \
                            int batch_size, int q_len, int kv_len, int num_heads, int num_kv_heads, int head_dim,      \
                            int window_size, void *stream);                                                            \
  void flash_attn_sinks_varlen_##d(const void *Q, const void *K, const void *V, void *O, const float *sinks,           \
                                   const unsigned *cu_seqlens_q, const unsigned *cu_seqlens_k, float scale,            \
                                   int batch_size, int max_q_len, int num_heads, int num_kv_heads, int head_dim,       \
                                   int window_size, void *stream);
MRS_DECL_FAS(f16) MRS_DECL_FAS(bf16) MRS_DECL_FAS(f32)
#undef MRS_DECL_FAS

/* Multi-head latent attention (DeepSeek-V2 / V3) on a paged latent cache; dtype 0 = f16, 1 = bf16, 2 = f32 (cache ops only).
 *   ckv_cache [num_blocks, block_size, kv_lora_rank]   kpe_cache [num_blocks, block_size, kpe_head_dim]
 * ffi.rs:118-132 ; concat_and_cache_mla_kernel.cu: token i goes to slot slot_mapping[i] (int64; < 0 is skipped); ckv_stride / kpe_stride are
 * the input row strides in elements. */
void concat_and_cache_mla(const void *ckv, const void *k_pe, void *ckv_cache, void *kpe_cache, const int64_t *slot_mapping,
                          int num_tokens, int kv_lora_rank, int kpe_head_dim, int block_size, int ckv_stride, int kpe_stride,
                          mrs_stream_t stream, uint32_t dtype);
/* ffi.rs:231-246 ; gather_mla_cache_kernel.cu: paged -> dense [num_tokens, kv_lora_rank] / [num_tokens, kpe_head_dim]; token i is position
 * i - cu_seq_lens[s] of sequence s = token_to_seq[i], in block block_table[s * block_table_stride + position / block_size]. */
void gather_mla_cache(const void *ckv_cache, const void *kpe_cache, void *ckv_out, void *kpe_out, const int *block_table,
                      const int *cu_seq_lens, const int *token_to_seq, int num_tokens, int block_size, int block_table_stride,
                      int kv_lora_rank, int kpe_head_dim, mrs_stream_t stream, uint32_t dtype);
/* ffi.rs:134-157: one query token per request over kv_lora_rank 512 / kpe_head_dim 64, f16 or bf16, page_size 16 or 32.
 * q_nope [batch, heads, 512], q_pe [batch, heads, 64], out [batch, heads, 512]; request b owns pages
 * kv_indices[kv_indptr[b] .. kv_indptr[b + 1]) and (pages - 1) * page_size + kv_last_page_len[b] keys (none without a page: zeros).
 * Returns 0, or non-zero for f32 (no kernel: stated deviation), another page size, window_left >= 0 or logits_soft_cap != 0.  The four tile-plan
 * pointers and rope_scale / rope_theta are not read (Q and K arrive rotated); without a workspace this entry runs one KV split. */
int flashinfer_mla_decode(const void *q_nope, const void *q_pe, const void *ckv_cache, const void *kpe_cache, const int *kv_indptr,
                          const int *kv_indices, const int *kv_last_page_len, void *out, int batch_size, int num_qo_heads,
                          int page_size, float sm_scale, int window_left, float logits_soft_cap, float rope_scale, float rope_theta,
                          const int *request_indices, const int *kv_tile_indices, const int *o_indptr, const int *kv_chunk_size_ptr,
                          uint32_t dtype, mrs_stream_t stream);
/* MI355X-native: the same decode with the context split num_splits ways over the grid (batch, head blocks, num_splits) and merged by a second
 * small launch; lengths are read on the device only, so the call can be captured in a graph.  workspace: f32, 16-byte aligned, at least
 * mla_decode_workspace_bytes(batch_size, num_qo_heads, num_splits) bytes (0 for one split, which writes the output with one launch). */
size_t mla_decode_workspace_bytes(int batch_size, int num_qo_heads, int num_splits);
int launch_mla_decode(const void *q_nope, const void *q_pe, const void *ckv_cache, const void *kpe_cache, const int *kv_indptr,
                      const int *kv_indices, const int *kv_last_page_len, void *out, int batch_size, int num_qo_heads, int page_size,
                      float sm_scale, int num_splits, void *workspace, size_t workspace_bytes, uint32_t dtype, mrs_stream_t stream);

/* GQA decode over an HND paged cache (the reference's FlashInfer back end, flashinfer_decode.cu / backend/flashinfer.rs); codes as above.
 *   key_cache / value_cache [num_pages, kv_heads, page_size, head_size]; an E4M3 cache (cache_dtype 3) holds value / scale, scales passed by value.
 * Token i goes to slot slot_mapping[i] (int64; < 0 is skipped): element (h, d) lands at ((slot / bs * H + h) * bs + slot % bs) * D + d.
 * key_stride / value_stride are the input row strides in elements.  dtype f16 / bf16 / f32, cache_dtype the same or 3. */
void reshape_and_cache_flashinfer(void *key, void *value, void *key_cache, void *value_cache, int64_t *slot_mapping, int32_t num_tokens,
                                  int32_t num_heads, int32_t head_size, int32_t block_size, int32_t key_stride, int32_t value_stride,
                                  float k_scale, float v_scale, uint32_t dtype, uint32_t cache_dtype, mrs_stream_t stream);
/* paged -> dense [num_tokens, kv_heads, head_size]; token i is position i - cu_seq_lens[s] of the sequence s with cu_seq_lens[s] <= i < cu_seq_lens[s + 1]
 * (binary search), in page block_table[s * block_table_stride + position / block_size].  E4M3 pages come back as float(code) * scale. */
void gather_kv_cache_flashinfer(void *key_cache, void *value_cache, void *k_out, void *v_out, const int32_t *block_table,
                                const int32_t *cu_seq_lens, int32_t num_tokens, int32_t num_seqs, int32_t block_size,
                                int32_t block_table_stride, int32_t num_kv_heads, int32_t head_size, uint32_t out_dtype, uint32_t cache_dtype,
                                float k_scale, float v_scale, mrs_stream_t stream);
/* One query token per request; q [batch, heads, head_size] with element strides q_stride_n / q_stride_h, o [batch, heads, head_size] contiguous.
 * Request b owns pages kv_indices[kv_indptr[b] .. kv_indptr[b + 1]) and (pages - 1) * page_size + kv_last_page_len[b] keys (none without a page: zeros).
 * Grid entry bx < padded_batch_size does nothing when block_valid_mask[bx] == 0 (one byte each, the reference's bool); otherwise it serves request
 * request_indices[bx], keys [t c, (t + 1) c) with t = kv_tile_indices[bx], c = *kv_chunk_size_ptr (read on the device; a multiple of page_size), and
 * writes partial row o_indptr[b] + t; a second launch merges rows o_indptr[b] .. o_indptr[b + 1] in index order.  With tmp_v == NULL the KV is not
 * partitioned: the entry with t == 0 covers all keys of its request.  window_left < 0: no window, else key i is visible iff
 * i + 1 + window_left >= kv_len; logits_soft_cap <= 0: no cap.  DEVIATION from the reference: tmp_v is F32 [padded_batch_size, heads, head_size]
 * (there: the query dtype), so a split adds no rounding; tmp_s f32 [padded_batch_size, heads] holds the log-sum-exp.  All pointers 16-byte aligned
 * except q (2).  Returns 0, or non-zero WITHOUT launching for what it does not serve: f32 queries (1), a cache dtype that is neither the query's
 * nor E4M3 (2), head_size other than 64 / 128 / 256 (3), page_size other than 16 / 32 (4), heads not a multiple of kv_heads or more than 16 heads
 * per KV head (5), bad scratch or alignment (6); 7 is a failed launch. */
int32_t flashinfer_decode(void *q, void *key_cache, void *value_cache, const int32_t *kv_indptr, const int32_t *kv_indices,
                          const int32_t *kv_last_page_len, const int32_t *request_indices, const int32_t *kv_tile_indices,
                          const int32_t *o_indptr, const int32_t *kv_chunk_size_ptr, const uint8_t *block_valid_mask, void *o, void *tmp_v,
                          void *tmp_s, int32_t batch_size, int32_t padded_batch_size, int32_t num_qo_heads, int32_t num_kv_heads,
                          int32_t head_size, int32_t page_size, int32_t q_stride_n, int32_t q_stride_h, float sm_scale, int32_t window_left,
                          float logits_soft_cap, float k_scale, float v_scale, uint32_t dtype, uint32_t cache_dtype, mrs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
