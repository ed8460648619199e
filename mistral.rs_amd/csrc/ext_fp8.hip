// ext_fp8.hip -- the stream-taking native per-tensor FP8 entry points (include/mrs_hip_ext.h): quantize, dequantize and the W8A8 matmul forward to the launchers of
// fp8_pertensor.hip in libmistralrsquant.so, where the format and the arithmetic are stated.  `dtype`: 0 f32, 1 f16, 2 bf16 (the matmul: 1 or 2).
// Every function returns 0, or < 0 for arguments outside the kernels (-1), a launch too large (-2) or a launch error (-3).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

extern "C" {

#define MRS_FP8_DECL(tag)                                                                                                                            \
  int launch_fp8_pertensor_quantize_dynamic_##tag(const void *in, uint8_t *q, size_t n, float *state, hipStream_t stream);                           \
  int launch_fp8_pertensor_quantize_static_##tag(const void *in, uint8_t *q, size_t n, const float *scale, hipStream_t stream);                      \
  int launch_fp8_pertensor_dequantize_##tag(const uint8_t *w, const float *scale, const int32_t *ids, void *out, long long rows, int K, hipStream_t stream);
MRS_FP8_DECL(f32)
MRS_FP8_DECL(f16)
MRS_FP8_DECL(bf16)
#undef MRS_FP8_DECL
int launch_fp8_pertensor_matmul_f16(const uint8_t *xq, const uint8_t *wq, const float *dq_x, const float *dq_w, const void *bias, void *out, int M, int N, int K,
                                    hipStream_t stream);
int launch_fp8_pertensor_matmul_bf16(const uint8_t *xq, const uint8_t *wq, const float *dq_x, const float *dq_w, const void *bias, void *out, int M, int N, int K,
                                     hipStream_t stream);

#define MRS_FP8_BY_DTYPE(call_f32, call_f16, call_bf16) \
  switch (dtype) {                                      \
  case 0: return call_f32;                              \
  case 1: return call_f16;                              \
  case 2: return call_bf16;                             \
  default: return -1;                                   \
  }

int mrs_fp8_quantize_dynamic(const void *in, void *q, size_t n, float *state, int dtype, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  MRS_FP8_BY_DTYPE(launch_fp8_pertensor_quantize_dynamic_f32(in, (uint8_t *)q, n, state, st), launch_fp8_pertensor_quantize_dynamic_f16(in, (uint8_t *)q, n, state, st),
                   launch_fp8_pertensor_quantize_dynamic_bf16(in, (uint8_t *)q, n, state, st))
}

int mrs_fp8_quantize_static(const void *in, void *q, size_t n, const float *scale, int dtype, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  MRS_FP8_BY_DTYPE(launch_fp8_pertensor_quantize_static_f32(in, (uint8_t *)q, n, scale, st), launch_fp8_pertensor_quantize_static_f16(in, (uint8_t *)q, n, scale, st),
                   launch_fp8_pertensor_quantize_static_bf16(in, (uint8_t *)q, n, scale, st))
}

int mrs_fp8_dequantize(const void *w, const float *scale, const int32_t *ids, void *out, long long rows, int K, int dtype, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  MRS_FP8_BY_DTYPE(launch_fp8_pertensor_dequantize_f32((const uint8_t *)w, scale, ids, out, rows, K, st),
                   launch_fp8_pertensor_dequantize_f16((const uint8_t *)w, scale, ids, out, rows, K, st),
                   launch_fp8_pertensor_dequantize_bf16((const uint8_t *)w, scale, ids, out, rows, K, st))
}

int mrs_fp8_matmul(const void *xq, const void *wq, const float *dq_x, const float *dq_w, const void *bias, void *out, int M, int N, int K, int dtype, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  if (dtype == 1) return launch_fp8_pertensor_matmul_f16((const uint8_t *)xq, (const uint8_t *)wq, dq_x, dq_w, bias, out, M, N, K, st);
  if (dtype == 2) return launch_fp8_pertensor_matmul_bf16((const uint8_t *)xq, (const uint8_t *)wq, dq_x, dq_w, bias, out, M, N, K, st);
  return -1;
}

}  // extern "C"
