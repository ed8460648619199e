// ext_gptq.hip -- the stream-taking native GPTQ / AWQ entry points (include/mrs_hip_ext.h): matmul, reconstruct and the AWQ repack forward to the launchers of
// gptq.hip in libmistralrsquant.so, where the format and the arithmetic are stated.
// Every function returns 0, or < 0 for arguments outside the kernels (-1), a launch too large (-2) or a launch error (-3).
#include <stdint.h>

extern "C" {

int launch_gptq_matmul(const void *x, const void *qweight, const void *qzeros, const void *scales, const void *g_idx, const void *bias, void *y, int M, int N, int K,
                       int groups, int bits, int zero_offset, void *stream);
int launch_gptq_reconstruct(const void *qweight, const void *qzeros, const void *scales, const void *g_idx, void *out, int K, int N, int groups, int bits,
                            int zero_offset, void *stream);
int launch_awq_repack(const void *qweight, const void *qzeros, void *qweight_out, void *qzeros_out, void *g_idx_out, int K, int N, int groups, int group_size,
                      int bits, void *stream);

int mrs_gptq_matmul(const void *x, const void *qweight, const void *qzeros, const void *scales, const void *g_idx, const void *bias, void *y, int M, int N, int K,
                    int groups, int bits, int zero_offset, void *stream) {
  return launch_gptq_matmul(x, qweight, qzeros, scales, g_idx, bias, y, M, N, K, groups, bits, zero_offset, stream);
}

int mrs_gptq_reconstruct(const void *qweight, const void *qzeros, const void *scales, const void *g_idx, void *out, int K, int N, int groups, int bits,
                         int zero_offset, void *stream) {
  return launch_gptq_reconstruct(qweight, qzeros, scales, g_idx, out, K, N, groups, bits, zero_offset, stream);
}

int mrs_awq_repack(const void *qweight, const void *qzeros, void *qweight_out, void *qzeros_out, void *g_idx_out, int K, int N, int groups, int group_size, int bits,
                   void *stream) {
  return launch_awq_repack(qweight, qzeros, qweight_out, qzeros_out, g_idx_out, K, N, groups, group_size, bits, stream);
}

}  // extern "C"
