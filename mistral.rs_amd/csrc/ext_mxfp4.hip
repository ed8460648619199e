// ext_mxfp4.hip -- MXFP4 row dequantizer: out row r = dequantized row ids[r] (or r) of a [*, K/2] blocks / [*, K/32] scales pair, as f32, f16 or bf16.
//
// Role: MXFP4Layer::dequantize_w and embedding_forward_raw (mistralrs-quant/src/mxfp4/mod.rs:87-103,615-707), which the reference runs on the
// CPU through DEQUANT_LUT[scale][nibble]; the f32 value table[nibble] * f32_from_bits(scale << 23) is formed exactly and converted once.
// One thread owns one 32-element block: a 16-byte load, one scale byte, 128 / 64 bytes of stores.
#include "mxfp4_core.cuh"

namespace mrs {

template <class T>
__global__ void __launch_bounds__(256) mxfp4_dequant_rows_kernel(const uint8_t *__restrict__ blocks, const uint8_t *__restrict__ scales, const int32_t *__restrict__ ids,
                                                                 T *__restrict__ out, long long rows, int nb) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * nb) return;
  const long long r = i / nb;
  const int b = (int)(i - r * nb);
  const long long src = ids ? (long long)ids[r] : r;
  const int4 q = ld16_a2(blocks + ((size_t)src * nb + b) * 16);
  const float s = mxfp4_scale(scales[(size_t)src * nb + b]);
  const uint32_t qs[4] = {(uint32_t)q.x, (uint32_t)q.y, (uint32_t)q.z, (uint32_t)q.w};
  T *dst = out + ((size_t)r * nb + b) * 32;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float w[8];
    mxfp4_word(qs[j], s, w);
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[8 * j + e] = from_f<T>(w[e]);
  }
}

}  // namespace mrs

extern "C" int mrs_mxfp4_dequantize_rows(const void *blocks, const void *scales, const int32_t *ids, int64_t rows, int K, int out_dtype, void *out, void *stream) {
  if (!blocks || !scales || !out || rows < 0 || K <= 0 || (K & 31) || out_dtype < 0 || out_dtype > 2) return -1;
  if (rows == 0) return 0;
  const int nb = K >> 5;
  const long long total = rows * nb, grid = (total + 255) / 256;
  if (grid > 0x7fffffffLL) return -2;
  const uint8_t *b = (const uint8_t *)blocks, *s = (const uint8_t *)scales;
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == 0) hipLaunchKernelGGL((mrs::mxfp4_dequant_rows_kernel<float>), dim3((unsigned)grid), dim3(256), 0, st, b, s, ids, (float *)out, rows, nb);
  else if (out_dtype == 1) hipLaunchKernelGGL((mrs::mxfp4_dequant_rows_kernel<mrs::f16_t>), dim3((unsigned)grid), dim3(256), 0, st, b, s, ids, (mrs::f16_t *)out, rows, nb);
  else hipLaunchKernelGGL((mrs::mxfp4_dequant_rows_kernel<mrs::bf16_t>), dim3((unsigned)grid), dim3(256), 0, st, b, s, ids, (mrs::bf16_t *)out, rows, nb);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
