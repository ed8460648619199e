// ext_bnb.hip -- the stream-taking native bitsandbytes entry points (include/mrs_hip_ext.h): dequantize and matmul forward to the launchers of bnb.hip in
// libmistralrsquant.so, where the format and the arithmetic are stated.
// Every function returns 0, or < 0 for arguments outside the kernels (-1), a launch too large (-2) or a launch error (-3).
#include <stdint.h>

extern "C" {

int launch_bnb_dequantize(const void *weight, const void *absmax, const float *code, const float *nested_absmax, const float *nested_quant_map, void *out,
                          long long n, int blocksize, int nested_blocksize, float nested_offset, int qtype, int dtype, void *stream);
int launch_bnb_matmul(const void *x, const void *weight, const void *absmax, const float *nested_absmax, const float *nested_quant_map, const void *bias, void *y,
                      float *workspace, int M, int N, int K, int blocksize, int nested_blocksize, float nested_offset, int qtype, int dtype, void *stream);

int mrs_bnb_dequantize(const void *weight, const void *absmax, const float *code, const float *nested_absmax, const float *nested_quant_map, void *out, long long n,
                       int blocksize, int nested_blocksize, float nested_offset, int qtype, int dtype, void *stream) {
  return launch_bnb_dequantize(weight, absmax, code, nested_absmax, nested_quant_map, out, n, blocksize, nested_blocksize, nested_offset, qtype, dtype, stream);
}

int mrs_bnb_matmul(const void *x, const void *weight, const void *absmax, const float *nested_absmax, const float *nested_quant_map, const void *bias, void *y,
                   float *workspace, int M, int N, int K, int blocksize, int nested_blocksize, float nested_offset, int qtype, int dtype, void *stream) {
  return launch_bnb_matmul(x, weight, absmax, nested_absmax, nested_quant_map, bias, y, workspace, M, N, K, blocksize, nested_blocksize, nested_offset, qtype, dtype,
                           stream);
}

}  // extern "C"
