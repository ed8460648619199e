// afq_core.cuh -- AFQ (affine 2/3/4/6/8-bit, the MLX checkpoint format) decode, row dequantizer and quantizer shared by afq.hip and ext_afq.hip.
//
// Format (mistralrs-quant/src/afq/ops.rs:1529-1767): w_q u32 [N][K * bits / 32]; element j of a row occupies bits [j * bits, (j + 1) * bits) of the row's
// little-endian bit stream, so a 3- or 6-bit code may straddle two words and 32 consecutive k are exactly `bits` whole words (a "unit").  A row starts on a
// 4-byte boundary and on nothing wider (K = 96 at 3 bits is 36 bytes): every weight load here assumes 4-byte alignment only.  scales / biases T [N][K / group],
// group in {32, 64, 128}; weight = q * scale + bias with q the unsigned code.
//
// Dequantize, every type and path: T(fmaf((float)q, (float)scale, (float)bias)), one round-to-nearest-even conversion.
// Quantize (ops.rs:1534-1622, the reference's CPU back-end): per group, in f32, scale = 1 if |max - min| < 1e-12 else (max - min) / (2^bits - 1), bias = min,
// q = clamp(roundf((w - bias) / scale), 0, 2^bits - 1) with the unrounded f32 scale and bias, correctly rounded divisions, round half away from zero; scale
// and bias are stored as RNE conversions to T.
#pragma once
#include "mxfp4_core.cuh"  // unpack2

namespace mrs {

typedef uint32_t afq_u2 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t afq_u4 __attribute__((ext_vector_type(4), aligned(4)));

__host__ __device__ constexpr bool afq_bits_ok(int bits) { return bits == 2 || bits == 3 || bits == 4 || bits == 6 || bits == 8; }
// group 32 / 64 / 128 -> 0 / 1 / 2 (units per group = 1 << shift), anything else -> -1
__host__ __device__ constexpr int afq_group_shift(int group) { return group == 32 ? 0 : group == 64 ? 1 : group == 128 ? 2 : -1; }

// the BITS words of one unit (32 k), from a 4-byte aligned address; NT: streamed once, kept out of the caches' way
template <int BITS, bool NT> __device__ __forceinline__ void afq_load_unit(const uint32_t *p, uint32_t (&w)[BITS]) {
  auto ld4 = [](const uint32_t *q) { return NT ? __builtin_nontemporal_load((const afq_u4 *)q) : *(const afq_u4 *)q; };
  auto ld2 = [](const uint32_t *q) { return NT ? __builtin_nontemporal_load((const afq_u2 *)q) : *(const afq_u2 *)q; };
  if constexpr (BITS >= 4) {
    const afq_u4 v = ld4(p);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    if constexpr (BITS == 8) {
      const afq_u4 u = ld4(p + 4);
      w[4] = u.x; w[5] = u.y; w[6] = u.z; w[7] = u.w;
    } else if constexpr (BITS == 6) {
      const afq_u2 u = ld2(p + 4);
      w[4] = u.x; w[5] = u.y;
    }
  } else {
    const afq_u2 v = ld2(p);
    w[0] = v.x; w[1] = v.y;
    if constexpr (BITS == 3) w[2] = NT ? __builtin_nontemporal_load(p + 2) : p[2];
  }
}

// code j (0..31, a constant after unrolling) of a unit
template <int BITS> __device__ __forceinline__ uint32_t afq_code(const uint32_t (&w)[BITS], int j) {
  const int bit = j * BITS, wd = bit >> 5, sh = bit & 31;
  uint32_t q = w[wd] >> sh;
  if (sh + BITS > 32) q |= w[wd + 1] << (32 - sh);  // never taken for the unit's last code: it ends on the unit's last bit
  return q & ((1u << BITS) - 1u);
}

// 8 consecutive T at a 16-byte aligned LDS address -> f32
template <class T> __device__ __forceinline__ void afq_x8(const T *p, float (&a)[8]) {
  if constexpr (sizeof(T) == 4) {
    const float4 u = *(const float4 *)p, v = *(const float4 *)(p + 4);
    a[0] = u.x; a[1] = u.y; a[2] = u.z; a[3] = u.w; a[4] = v.x; a[5] = v.y; a[6] = v.z; a[7] = v.w;
  } else {
    const int4 v = *(const int4 *)p;
    unpack2<T>((uint32_t)v.x, a[0], a[1]);
    unpack2<T>((uint32_t)v.y, a[2], a[3]);
    unpack2<T>((uint32_t)v.z, a[4], a[5]);
    unpack2<T>((uint32_t)v.w, a[6], a[7]);
  }
}

// ------------------------------------------------------------------------------------------------ dequantize rows (dequantize_w, embedding_forward)
// One thread owns one unit: `bits` words in, 32 T out.  Row r of the output is row ids[r] (or r) of the packed matrix.
template <class T, int BITS>
__global__ void __launch_bounds__(256) afq_dequant_rows_kernel(const uint32_t *__restrict__ wq, const T *__restrict__ sc, const T *__restrict__ bi,
                                                               const uint32_t *__restrict__ ids, T *__restrict__ out, long long rows, int nu, int gshift) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * nu) return;
  const long long r = i / nu;
  const int u = (int)(i - r * nu);
  const long long src = ids ? (long long)ids[r] : r;
  uint32_t w[BITS];
  afq_load_unit<BITS, false>(wq + ((size_t)src * nu + u) * BITS, w);
  const size_t g = (size_t)src * (nu >> gshift) + (u >> gshift);
  const float s = to_f<T>(sc[g]), b = to_f<T>(bi[g]);
  T *dst = out + ((size_t)r * nu + u) * 32;
#pragma unroll
  for (int j = 0; j < 32; ++j) dst[j] = from_f<T>(fmaf((float)afq_code<BITS>(w, j), s, b));
}

template <class T, int BITS>
static int afq_dequant_rows_bits(const uint32_t *wq, const T *sc, const T *bi, const uint32_t *ids, T *out, long long rows, int K, int gshift, hipStream_t st) {
  const int nu = K >> 5;
  const long long grid = (rows * nu + 255) / 256;
  if (grid > 0x7fffffffLL) return -2;
  hipLaunchKernelGGL((afq_dequant_rows_kernel<T, BITS>), dim3((unsigned)grid), dim3(256), 0, st, wq, sc, bi, ids, out, rows, nu, gshift);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

template <class T>
static int afq_dequant_rows(const void *wq, const void *sc, const void *bi, const uint32_t *ids, void *out, long long rows, int K, int bits, int group, void *stream) {
  const int gs = afq_group_shift(group);
  if (!wq || !sc || !bi || !out || rows < 0 || K <= 0 || !afq_bits_ok(bits) || gs < 0 || K % group) return -1;
  if (rows == 0) return 0;
  const uint32_t *w = (const uint32_t *)wq;
  const T *s = (const T *)sc, *b = (const T *)bi;
  T *o = (T *)out;
  hipStream_t st = (hipStream_t)stream;
  switch (bits) {
  case 2: return afq_dequant_rows_bits<T, 2>(w, s, b, ids, o, rows, K, gs, st);
  case 3: return afq_dequant_rows_bits<T, 3>(w, s, b, ids, o, rows, K, gs, st);
  case 4: return afq_dequant_rows_bits<T, 4>(w, s, b, ids, o, rows, K, gs, st);
  case 6: return afq_dequant_rows_bits<T, 6>(w, s, b, ids, o, rows, K, gs, st);
  default: return afq_dequant_rows_bits<T, 8>(w, s, b, ids, o, rows, K, gs, st);
  }
}

// ------------------------------------------------------------------------------------------------ quantize
// One wave per group, four groups per workgroup.  Element e of the group sits in lane e & 63, register e >> 6; the codes go through LDS as bytes and lane i
// assembles word i of the group's group * bits / 32 words (<= 32), so every packed word is written once, whole.
template <class T, int BITS>
__global__ void __launch_bounds__(256) afq_quantize_kernel(const T *__restrict__ w, uint32_t *__restrict__ wq, T *__restrict__ sc, T *__restrict__ bi,
                                                           long long groups, int group) {
  __shared__ uint8_t codes[4][128];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * 4 + wave;
  const bool live = g < groups;  // uniform over the wave; no early return: the workgroup meets at the barrier
  constexpr float LEVELS = (float)((1u << BITS) - 1u);
  float v[2] = {0.0f, 0.0f};
  float lo = 3.402823466e+38f, hi = -3.402823466e+38f;
  if (live) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int e = lane + 64 * t;
      if (e < group) {
        v[t] = to_f<T>(w[(size_t)g * group + e]);
        lo = fminf(lo, v[t]);
        hi = fmaxf(hi, v[t]);
      }
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, d, 64));
    hi = fmaxf(hi, __shfl_xor(hi, d, 64));
  }
  const float range = hi - lo;
  const float scale = fabsf(range) < 1e-12f ? 1.0f : __fdiv_rn(range, LEVELS);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int e = lane + 64 * t;
    if (e < group) codes[wave][e] = (uint8_t)(uint32_t)fminf(fmaxf(roundf(__fdiv_rn(v[t] - lo, scale)), 0.0f), LEVELS);
  }
  __syncthreads();
  const int words = (group >> 5) * BITS;
  if (live && lane < words) {
    const int first = (32 * lane) / BITS, last = (32 * lane + 31) / BITS;  // elements with a bit in this word
    uint32_t word = 0;
    for (int e = first; e <= last; ++e) {
      const int sh = e * BITS - 32 * lane;
      const uint32_t q = codes[wave][e];
      word |= sh >= 0 ? q << sh : q >> -sh;
    }
    wq[(size_t)g * words + lane] = word;
  }
  if (live && lane == 0) {
    sc[g] = from_f<T>(scale);
    bi[g] = from_f<T>(lo);
  }
}

template <class T>
static int afq_quantize(const void *w, void *wq, void *sc, void *bi, long long rows, int K, int bits, int group, void *stream) {
  if (!w || !wq || !sc || !bi || rows < 0 || K <= 0 || !afq_bits_ok(bits) || afq_group_shift(group) < 0 || K % group) return -1;
  const long long groups = rows * (K / group), grid = (groups + 3) / 4;
  if (groups == 0) return 0;
  if (grid > 0x7fffffffLL) return -2;
  hipStream_t st = (hipStream_t)stream;
#define MRS_AFQ_Q(B) \
  hipLaunchKernelGGL((afq_quantize_kernel<T, B>), dim3((unsigned)grid), dim3(256), 0, st, (const T *)w, (uint32_t *)wq, (T *)sc, (T *)bi, groups, group)
  switch (bits) {
  case 2: MRS_AFQ_Q(2); break;
  case 3: MRS_AFQ_Q(3); break;
  case 4: MRS_AFQ_Q(4); break;
  case 6: MRS_AFQ_Q(6); break;
  default: MRS_AFQ_Q(8); break;
  }
#undef MRS_AFQ_Q
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace mrs
