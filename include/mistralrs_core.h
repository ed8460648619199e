/*
 * include/mistralrs_core.h -- C ABI of libmistralrscuda.so, hot-path subset (gfx950 / MI355X).
 *
 * Drop-in symbols for the part of `libmistralrscuda.a` (mistralrs-core/build.rs:59-70) that the
 * Llama / Mistral / Mixtral decode graph touches.  Rust declarations: mistralrs-core/src/cuda/ffi.rs:75-140.
 * GDN / SSM / dflash / unquantized MoE kernels of that library are out of scope.
 */
#ifndef MISTRALRS_CORE_H
#define MISTRALRS_CORE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* residual_dst = T(x + residual); norm_dst = T(residual_dst * rsqrt(mean(residual_dst^2) + eps) * weight)
 * replaces mistralrs-core/src/cuda/sort.cu:352-460,701-727 ; ffi.rs:108-140 */
#define MRS_DECL_NORMS(d)                                                                                              \
  void add_rms_norm_##d(const void *x, const void *residual, const void *weight, void *residual_dst, void *norm_dst,   \
                        int nrows, int ncols, float eps, int64_t stream);                                              \
  /* dst = T((residual + x * rsqrt(mean(x^2) + eps) * weight) * scale[0])   sort.cu:244-350 ; ffi.rs:75-107 */         \
  void rms_norm_residual_##d(const void *x, const void *residual, const void *weight, const void *scale, void *dst,    \
                             int nrows, int ncols, float eps, int64_t stream);                                         \
  /* MI355X-native: plain RMSNorm = candle_nn::ops::rms_norm as called by RmsNorm::forward (layers.rs:403-414) */      \
  void mrs_rms_norm_##d(const void *x, const void *weight, void *dst, int nrows, int ncols, float eps, int64_t stream);
MRS_DECL_NORMS(f32) MRS_DECL_NORMS(f16) MRS_DECL_NORMS(bf16)
#undef MRS_DECL_NORMS

/* MoE router: softmax / sigmoid / raw scores over n_experts logits per row -> top_k (ids, weights), ties to the lowest expert id.
 * score_mode 0 raw, 1 softmax, 2 sigmoid; weight_mode 0 score, 1 softmax over the picked raw logits, 2 sigmoid(raw); optional
 * selection_bias / expert_scale [n_experts] (NULL = none), clamp, renormalise by max(sum, norm_min), output_scale.  n_experts in
 * {1,2,4,8,16,32,64,128,256,512,576}, other values are ignored like the reference's switch.
 * replaces mistralrs-core/src/cuda/sort.cu:1097-1470 ; ffi.rs:523-579 ; caller ops.rs:259-336 (moe_router_topk) */
#include <stdbool.h>
void moe_router_topk_f32(const void *logits, float *weights, uint32_t *ids, const float *selection_bias, const float *expert_scale, int n_rows,
                         int n_experts, int top_k, int score_mode, int weight_mode, bool renormalize, bool clamp_logits, float clamp_min,
                         float clamp_max, float norm_min, float output_scale, int64_t stream);
void moe_router_topk_f16(const void *logits, float *weights, uint32_t *ids, const float *selection_bias, const float *expert_scale, int n_rows,
                         int n_experts, int top_k, int score_mode, int weight_mode, bool renormalize, bool clamp_logits, float clamp_min,
                         float clamp_max, float norm_min, float output_scale, int64_t stream);
void moe_router_topk_bf16(const void *logits, float *weights, uint32_t *ids, const float *selection_bias, const float *expert_scale, int n_rows,
                          int n_experts, int top_k, int score_mode, int weight_mode, bool renormalize, bool clamp_logits, float clamp_min,
                          float clamp_max, float norm_min, float output_scale, int64_t stream);

/* Sampling: top-k of one f32 logits row over a large vocabulary + the pieces of the full-softmax normaliser (Sampler::sample_topk_on_device, sampler.rs:1171-1260;
 * with top-k set, top-p / min-p / the draw stay on the host; the draw WITHOUT top-k runs on the device, see categorical_large_f32_packed_batched below).  The caller owns every buffer: block_values / block_indices [nrows][nblocks][k], block_maxes / block_sums
 * [nrows][nblocks] (workspace, nblocks = ceil(ncols / chunk_size)), packed_out [nrows][2k + 2] = k values, k indices as f32, denom, max(x / T).
 * Order: value descending, index ascending on ties; NaN and -inf are never selected, missing entries are (-inf, 0).  1 <= k <= 128, chunk_size <= 4096 (the
 * reference's host wrapper passes 2048).  replaces mistralrs-core/src/cuda/sort.cu:1502-1823,2146-2206 ; ffi.rs:583-624 ; caller ops.rs:691-1000 */
void topk_large_f32(const float *input, float *block_values, uint32_t *block_indices, float *block_maxes, float *block_sums, float *values_out,
                    uint32_t *indices_out, float *softmax_info_out, int ncols, int k, int chunk_size, int nblocks, float inv_temperature, int64_t stream);
void topk_large_f32_packed(const float *input, float *block_values, uint32_t *block_indices, float *block_maxes, float *block_sums, float *packed_out,
                           int ncols, int k, int chunk_size, int nblocks, float inv_temperature, int64_t stream);
void topk_large_f32_packed_batched(const float *input, const float *inv_temperatures, float *block_values, uint32_t *block_indices, float *block_maxes,
                                   float *block_sums, float *packed_out, int nrows, int ncols, int k, int chunk_size, int nblocks, int64_t stream);

/* Greedy sampling: arg-max of f32 logits rows.  block_values / block_indices [nrows][nblocks] are workspace; packed_out [nrows][2] = (max logit, token id as f32),
 * token_ids_out [nrows] (either may be NULL).  Lowest index on ties; a row holding a NaN reports token 0xffffffff and (NaN, NaN); a row of -inf reports token 0.
 * replaces mistralrs-core/src/cuda/sort.cu:1825-1912,2071-2143,2207-2238 ; ffi.rs:643-665 ; callers ops.rs:1232-2050 (cuda_top1_logits_f32_*) */
void top1_large_f32_packed(const float *input, float *block_values, uint32_t *block_indices, float *packed_out, uint32_t *token_ids_out, int ncols, int chunk_size,
                           int nblocks, int64_t stream);
void top1_large_f32_packed_batched(const float *input, float *block_values, uint32_t *block_indices, float *packed_out, uint32_t *token_ids_out, int nrows, int ncols,
                                   int chunk_size, int nblocks, int64_t stream);

/* Temperature sampling over the whole vocabulary (top_k unset, top_p / min_p inactive): one draw per row from softmax(x * inv_temperature) at the caller's uniform.
 * The caller owns every buffer: block_values / block_sums [nrows][nblocks] (workspace), packed_out [nrows][2] = (token id as f32, log-probability of that token
 * under the full softmax at that temperature).  block_values[row][chunk] = the chunk's largest raw logit (NaN if the chunk holds a NaN, -inf if nothing is above
 * -inf); block_sums[row][chunk] = sum over the chunk of expf(x * invT - block_value * invT) (NaN if the chunk holds a NaN, 0 when the chunk maximum is -inf).
 * Per row: gmax = max_b(block_values) * invT; denom = sum_b block_sums[b] * expf(block_values[b] * invT - gmax), added in chunk order;
 * target = min(u * denom, nextafterf(denom, -inf)); the chunk is the first whose running mass exceeds target; inside it the token is the LOWEST index with weight > 0
 * whose inclusive cumulative weight exceeds the remaining target (if rounding leaves none: the chunk's last index with weight > 0).  A token of weight 0 (a -inf logit,
 * underflow) is never returned.  The row reports (NaN, NaN) when invT is not finite or <= 0, u is outside [0, 1) or not finite, gmax is not finite (a NaN anywhere in
 * the row, a +inf logit, a row of -inf), or denom is not finite or <= 0; other rows of the launch are unaffected.  Returns without launching when nrows < 1, ncols < 1,
 * chunk_size < 1 or > 4096, or nblocks * chunk_size < ncols; any chunk_size in 1..4096 is served (the reference's host wrapper passes 2048).  The order of the f32
 * additions inside a chunk is this library's (per-thread runs + a lane scan), not the reference's tree: tokens agree wherever u is not within f32 rounding of a boundary.
 * replaces mistralrs-core/src/cuda/sort.cu:1825-2069,2240-2257 ; ffi.rs:666 ; callers ops.rs:1347-1500, pipeline/sampling.rs:999-1018, sampler.rs:649-652,744-764 */
void categorical_large_f32_packed_batched(const float *input, const float *inv_temperatures, const float *uniforms, float *block_values, float *block_sums,
                                          float *packed_out, int nrows, int ncols, int chunk_size, int nblocks, int64_t stream);

/* Top-p / min-p sampling over the WHOLE row, no top-k (this library's own symbol: the reference leaves the device here, sampler.rs:649-655, 1605-1662).  One draw per
 * row from softmax(x * inv_temperatures[row]) restricted to the kept set: top-p keeps every logit >= x*, the largest logit at which the mass of the strictly greater
 * logits is still below top_ps[row] * total (ALL logits tied at x* are kept); min-p keeps the tokens whose weight relative to the largest exceeds min_ps[row]; a cut value
 * outside (0, 1), NaN included, is inactive.  The cumulative kept mass is inverted in token order at uniforms[row] in [0, 1).  Masses are fixed-point integers
 * (weight * 2^39, truncated), so the result is bit-identical across launches, batch rows and neighbours.  Workspaces block_values / block_sums [nrows][nblocks] as for
 * categorical_large_f32_packed_batched; packed_out [nrows][4] = token id as f32, its log-probability under the FULL softmax, x* (-inf without top-p), kept mass / total
 * mass.  An unusable row (see the categorical entry) reports four NaNs.  Returns without launching on the shapes the categorical entry refuses. */
void mrs_nucleus_large_f32_packed_batched(const float *input, const float *inv_temperatures, const float *uniforms, const float *top_ps, const float *min_ps,
                                          float *block_values, float *block_sums, float *packed_out, int nrows, int ncols, int chunk_size, int nblocks,
                                          int64_t stream);

/* Speculative decoding, the verifier: the rounds of nseq sequences in one launch group (this library's own symbol: the reference loops on the host over full-vocabulary
 * probability vectors -- mistralrs-core/src/speculative/verifier.rs:44-115 greedy verification, :200-290 the accept loop, :339-473 the stochastic rule).  Sequence s
 * owns the rows seq_rows[s] .. seq_rows[s + 1] (1..8 of them) of target_logits [total_rows][ncols] f32; with n = rows - 1 drafts, row i judges draft_ids[row i] and the
 * last row is the bonus row (its draft_ids entry is ignored); n = 0 is a plain draw.  modes[s]: 0 greedy, 1 temperature; inv_temperatures[s]; uniforms [total_rows][2] =
 * (the accept draw u0, the draw u1 used if this row ends the round); draft_logits [total_rows][ncols] or NULL (a deterministic proposer: q is one-hot on the draft).
 * Outputs: n_accepted [nseq], out_tokens [nseq][8] = the accepted drafts, then the continuation token, then -1.
 *   greedy: a row's winner is what mrs_sample_greedy_advance picks on it (largest value, lowest index on ties, -0.0 ranks with +0.0); n_accepted = the longest prefix with
 *   winner == draft, the continuation is the winner of row n_accepted.
 *   temperature: p = softmax(target * inv_t), q = softmax(draft * inv_t), each as the categorical entry computes it (gmax, denom in chunk order), p_d = expf(x_d * inv_t -
 *   gmax) / denom; accept = q_d > 0 ? min(1, p_d / q_d) : (p_d > 0 ? 1 : 0) (draft_logits NULL: q_d = 1), accepted iff u0 < accept.  At the first rejected row the
 *   continuation inverts the cumulative sums of max(p - q, 0) (NULL: p with the draft zeroed) at u1 -- chunk masses in chunk order, the categorical entry's rule inside
 *   the chunk -- or is drawn from p when that sum is not positive.  With every draft accepted the bonus row is categorical_large_f32_packed_batched's draw at u1, bit for bit.
 * Rows after the one that ends the round are never read and may hold NaN.  A sequence reports n_accepted = -1 (and eight -1 tokens) when a row that decides is unusable --
 * a NaN in it (either mode); in temperature mode also a +inf logit, a row of -inf, inv_t not finite or <= 0, u0 / u1 outside [0, 1), a draft id outside the row -- or when
 * its row count is outside 1..8 or its mode unknown; other sequences are unaffected.  The caller owns `workspace`, >= mrs_spec_verify_workspace_bytes(total_rows, nseq,
 * nblocks) bytes, 8-byte aligned.  Returns without launching (nothing is written) when nseq < 1, total_rows < nseq or > 8 * nseq or > 65535, the workspace is too small,
 * or on the shapes the categorical entry refuses.  Four launches on the caller's stream, no allocation. */
size_t mrs_spec_verify_workspace_bytes(int total_rows, int nseq, int nblocks);
void mrs_spec_verify_f32_batched(const float *target_logits, const float *draft_logits, const int32_t *draft_ids, const int32_t *seq_rows, const int32_t *modes,
                                 const float *inv_temperatures, const float *uniforms, void *workspace, size_t workspace_bytes, int32_t *n_accepted, int32_t *out_tokens,
                                 int nseq, int total_rows, int ncols, int chunk_size, int nblocks, int64_t stream);

/* Sampler pre-processing: dst [n] = x [n] (f32), then for the n_tokens listed token ids (ids >= n ignored): penalties -- skipped where count <= 0;
 * v -= count * frequency_penalty + presence_penalty; if repetition_penalty != 1: v = v > 0 ? v / rp : v * rp -- or additive biases.
 * replaces mistralrs-core/src/cuda/sort.cu:8-110 ; ffi.rs:45-65 ; callers sampler.rs:1113-1169 */
void apply_sparse_penalties_f32(const void *x, void *dst, const uint32_t *token_ids, const float *counts, int n, int n_tokens, float frequency_penalty,
                                float presence_penalty, float repetition_penalty, int64_t stream);
void apply_sparse_logits_bias_f32(const void *x, void *dst, const uint32_t *token_ids, const float *biases, int n, int n_tokens, int64_t stream);

/* The same pre-processing for every row of a step in ONE launch, from the raw token history (this library's own symbol: the reference has no batched device plan for a
 * request with penalties, sampler.rs:617-631).  Row r's context is ctx_tokens[ctx_offsets[r] .. ctx_offsets[r + 1]); a token counts as generated iff its position in
 * that context is >= min(prompt_lens[r], length).  With g = generated occurrences and s = all occurrences of a token: v = x; g > 0: v -= fmaf(g, frequency, presence);
 * s > 0 and repetition != 1: v = v > 0 ? v / repetition : v * repetition; listed in bias_ids[bias_offsets[r] .. bias_offsets[r + 1]): v += bias -- bit for bit the chain
 * apply_sparse_penalties_f32(generated counts, f, p, 1) -> apply_sparse_penalties_f32(all counts, 0, 0, rp) -> apply_sparse_logits_bias_f32 (sampler.rs:1111-1145).
 * Token ids >= ncols are ignored; bias ids are unique within a row; bias_offsets == NULL: no bias.  x == dst is allowed.  The device counts with integer LDS atomics only,
 * so dst is a function of the row's inputs alone.  Grid (ceil(ncols / chunk_size), nrows): returns without launching on nrows <= 0 or > 65535, ncols <= 0, or a
 * chunk_size outside 1..4096. */
void mrs_penalties_f32_batched(const float *x, float *dst, const uint32_t *ctx_tokens, const int32_t *ctx_offsets, const int32_t *prompt_lens,
                               const float *frequency_penalties, const float *presence_penalties, const float *repetition_penalties, const uint32_t *bias_ids,
                               const float *bias_values, const int32_t *bias_offsets, int nrows, int ncols, int chunk_size, int64_t stream);

#ifdef __cplusplus
}
#endif
#endif
