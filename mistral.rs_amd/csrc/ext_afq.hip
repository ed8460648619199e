// ext_afq.hip -- the stream-taking native AFQ entry points (include/mrs_hip_ext.h): matmul and MoE gather forward to the launchers of afq.hip in
// libmistralrsquant.so; the row dequantizer (AfqLayer::dequantize_w, embedding_forward) and the quantizer are the kernels of afq_core.cuh.
// dtype codes: 0 = f32, 1 = f16, 2 = bf16.  Every function returns 0, or < 0 for arguments outside the kernels (-1), a launch too large (-2) or a launch error (-3).
#include "afq_core.cuh"

extern "C" {

int launch_afq_matmul(const void *x, const void *w_q, const void *scales, const void *biases, const void *bias, void *y, int M, int N, int K, int bits, int group,
                      int dtype, void *stream);
int launch_afq_indexed_moe_gemm(const void *x, const void *w_q, const void *scales, const void *biases, const void *bias, const uint32_t *indices, void *y,
                                int num_tokens, int topk, int num_experts, int N, int K, int bits, int group, int dtype, int input_has_topk_dim, void *stream);

int mrs_afq_matmul(const void *x, const void *w_q, const void *scales, const void *biases, const void *bias, void *y, int M, int N, int K, int bits, int group,
                   int dtype, void *stream) {
  return launch_afq_matmul(x, w_q, scales, biases, bias, y, M, N, K, bits, group, dtype, stream);
}

int mrs_afq_indexed_moe_gemm(const void *x, const void *w_q, const void *scales, const void *biases, const void *bias, const uint32_t *indices, void *y,
                             int num_tokens, int topk, int num_experts, int N, int K, int bits, int group, int dtype, int input_has_topk_dim, void *stream) {
  return launch_afq_indexed_moe_gemm(x, w_q, scales, biases, bias, indices, y, num_tokens, topk, num_experts, N, K, bits, group, dtype, input_has_topk_dim, stream);
}

int mrs_afq_dequantize_rows(const void *w_q, const void *scales, const void *biases, const uint32_t *ids, int64_t rows, int K, int bits, int group, int dtype,
                            void *out, void *stream) {
  if (dtype == 0) return mrs::afq_dequant_rows<float>(w_q, scales, biases, ids, out, rows, K, bits, group, stream);
  if (dtype == 1) return mrs::afq_dequant_rows<mrs::f16_t>(w_q, scales, biases, ids, out, rows, K, bits, group, stream);
  if (dtype == 2) return mrs::afq_dequant_rows<mrs::bf16_t>(w_q, scales, biases, ids, out, rows, K, bits, group, stream);
  return -1;
}

int mrs_afq_quantize(const void *w, void *w_q, void *scales, void *biases, int64_t rows, int K, int bits, int group, int dtype, void *stream) {
  if (dtype == 0) return mrs::afq_quantize<float>(w, w_q, scales, biases, rows, K, bits, group, stream);
  if (dtype == 1) return mrs::afq_quantize<mrs::f16_t>(w, w_q, scales, biases, rows, K, bits, group, stream);
  if (dtype == 2) return mrs::afq_quantize<mrs::bf16_t>(w, w_q, scales, biases, rows, K, bits, group, stream);
  return -1;
}

}  // extern "C"
