// fp8_pertensor.hip -- per-tensor FP8 (OCP E4M3 bytes + ONE f32 scale per tensor): scalar conversions, the dynamic / static per-tensor quantizer, dequantize with an
// optional row gather, and the W8A8 matmul on the FP8 matrix cores, MI355X / gfx950, wave64.
//
// Behind FP8Linear (mistralrs-quant/src/fp8/{mod,quantize}.rs, ISQ type F8E4M3, UQFF serde type 3) and PerTensorFP8Linear (src/pertensor_fp8/).  Drop-in for the
// six launch_*_fp8 / launch_fp8_to_* symbols of src/scalar_fp8/ffi.rs; the launch_fp8_pertensor_* symbols are this project's own (the reference's W8A8 forward
// is a cuBLASLt call).  DESIGN 4.18 carries the contract; in short:
//
//   fp8 -> T            exact (T = f32 / f16 / bf16); the NaN bytes 0x7f / 0xff give NaN.
//   T -> fp8            e4m3_satfinite_rne(f16_rne(clamp(f32(v), +-448))): the chain of the blockwise quantizer, its f32 -> f16 -> e4m3 double rounding included.
//   dynamic quantizer   amax = max |f32(x)| over the tensor; s = min(448 / amax, 448) (amax == 0: s = 448); dq = 1 / s; q = T->fp8(f32(x) * s).  Correctly rounded
//                       f32 division, one f32 product.  amax, s, dq live in a device `state` (f32 [3 + 1024]: the three values, then the per-workgroup maxima of
//                       the two-stage reduction); no host synchronisation, no atomics, the same bits on every run (max does not depend on order).
//   static quantizer    q = T->fp8(f32(x) / scale), the correctly rounded division; scale an f32 on the device (a null pointer means 1: the scalar conversion).
//   dequantize          T(f32(w) * scale): one f32 product, one RNE conversion; optional i32 row ids gather rows (the embedding); null scale means 1.
//   matmul              out[m][n] = RNE_T(fmaf(S, dq_x * dq_w, f32(bias[n]))), S = sum_k f32(xq[m][k]) f32(wq[n][k]): every product of two E4M3 values is exact in f32,
//                       dq_x * dq_w is one f32 product, T = bf16 / f16; dq_x, dq_w are read by the kernel from device pointers.  Route 3 adds the products in f32.
//                       Routes 1 and 2 add them on the FP8 matrix core, and that is NOT an f32 sum: inside one MFMA every product is cut toward zero onto the grid
//                       2^(e - 13), e the exponent of the instruction's largest product (measured: scripts/probe_fp8_mfma.py); the instructions' results are
//                       added in f32.  S is exact when the products of each instruction lie on its grid.
//
// Matmul routes (fp8_pertensor_last_route).  "fast" means K % 16 == 0 and 16-byte aligned xq / wq bases.  No element is converted on routes 1 and 2: the stored
// bytes ARE the MFMA operands.  A lane's 16-byte piece feeds two MFMAs (its low and its high 8 bytes); A and B pieces are cut the same way, so the k order inside
// an instruction is the same on both sides and the sum is over the right pairs.
//   1  fast, M <= 16   skinny GEMV on v_mfma_f32_16x16x32_fp8_fp8.  A wave owns 16 weight rows and streams them from HBM straight into the B operand (lane l: row
//                      l & 15, 16 bytes at k + 16 (l >> 4), non-temporal).  The A operand is xq: rows < M staged once per workgroup in LDS as bytes, 4096 k at a time,
//                      rows >= M are zeros in registers.  8 waves per workgroup = (row groups) x (k slices); the split is a function of N and K only; the f32 partials
//                      meet in LDS and are summed in slice order.  Nothing depends on M: a row of an M = 16 call has the bits of its own M = 1 call.
//   2  fast, M > 16    128 x 128 x 128 byte tile on v_mfma_f32_32x32x16_fp8_fp8: xq and wq tiles staged in LDS as raw bytes (rows padded to 144 B), the next tile
//                      prefetched into registers behind the MFMAs, 4 waves of 64 x 64 f32 accumulators, scale and bias in the epilogue.  Edge tiles in M, N, K.
//   3  anything else   one wave per output element, byte loads, the integer decode of common.cuh.  Correct, untuned.
#include "common.cuh"

namespace mrs {

static int g_fp8pt_route = 0;

typedef float f8p_f32x4 __attribute__((ext_vector_type(4)));
typedef float f8p_f32x16 __attribute__((ext_vector_type(16)));

constexpr int F8P_PARTIALS = 1024;  // per-workgroup maxima of the absmax reduction, state[3 ..]
constexpr int F8P_FUSED_MAX = 32768;  // elements up to which one workgroup runs absmax and the quantizer in one launch

__device__ __forceinline__ int4 f8p_ld16nt(const void *p) { int4_a16 v = __builtin_nontemporal_load((const int4_a16 *)p); return make_int4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ long f8p_lo(int4 v) { return (long)(((uint64_t)(uint32_t)v.y << 32) | (uint32_t)v.x); }
__device__ __forceinline__ long f8p_hi(int4 v) { return (long)(((uint64_t)(uint32_t)v.w << 32) | (uint32_t)v.z); }

// T -> fp8 of the contract, v already in f32
__device__ __forceinline__ uint8_t f8p_encode(float v) {
  if (v > 448.0f) v = 448.0f;
  if (v < -448.0f) v = -448.0f;
  return float_to_fp8_e4m3(half_bits_to_float(float_to_half_bits(v)));  // f32 -> f16 -> e4m3: the two roundings of the blockwise quantizer
}

// the f32 product is a value of its own: without the barrier the f16 form becomes one v_fma_mixlo_f16, a single rounding
template <class T> __device__ __forceinline__ T f8p_round(float v) {
  asm volatile("" : "+v"(v));
  return from_f<T>(v);
}

// 16 consecutive elements from `in + i0` as f32; elements at or past n are 0.  `in` is aligned to its element only.
template <class T> __device__ __forceinline__ void f8p_load16(const T *__restrict__ in, size_t i0, size_t n, float (&v)[16]) {
  if (i0 + 16 <= n) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int4 q = ld16_a4(in + i0 + 4 * j);
        v[4 * j] = __int_as_float(q.x); v[4 * j + 1] = __int_as_float(q.y); v[4 * j + 2] = __int_as_float(q.z); v[4 * j + 3] = __int_as_float(q.w);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int4 q = ld16_a2(in + i0 + 8 * j);
        const uint32_t w[4] = {(uint32_t)q.x, (uint32_t)q.y, (uint32_t)q.z, (uint32_t)q.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[8 * j + 2 * e] = to_f<T>(__builtin_bit_cast(T, (uint16_t)(w[e] & 0xFFFFu)));
          v[8 * j + 2 * e + 1] = to_f<T>(__builtin_bit_cast(T, (uint16_t)(w[e] >> 16)));
        }
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j) v[j] = i0 + j < n ? to_f<T>(in[i0 + j]) : 0.0f;
  }
}

__device__ __forceinline__ float f8p_amax16(const float (&v)[16]) {
  float a = 0.0f;
#pragma unroll
  for (int j = 0; j < 16; ++j) a = fmaxf(a, fabsf(v[j]));
  return a;
}

// 16 codes of one unit to q + i0: one 16-byte store when VEC (q 16-byte aligned) and the unit is whole
template <bool VEC> __device__ __forceinline__ void f8p_store16(uint8_t *__restrict__ q, size_t i0, size_t n, const uint8_t (&c)[16]) {
  if (VEC && i0 + 16 <= n) {
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = (uint32_t)c[4 * j] | ((uint32_t)c[4 * j + 1] << 8) | ((uint32_t)c[4 * j + 2] << 16) | ((uint32_t)c[4 * j + 3] << 24);
    *(int4 *)(q + i0) = make_int4((int)w[0], (int)w[1], (int)w[2], (int)w[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (i0 + j < n) q[i0 + j] = c[j];
  }
}

// maximum over the workgroup (blockDim.x a multiple of 64, at most 1024), returned to every thread
__device__ __forceinline__ float f8p_block_max(float a, float *sh) {
  a = wave_max(a);
  __syncthreads();  // earlier reads of sh are done
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  float m = 0.0f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) m = fmaxf(m, sh[w]);
  return m;
}

__device__ __forceinline__ void f8p_write_scales(float amax, float *__restrict__ state) {
  float s = 448.0f / amax;       // correctly rounded; amax == 0 gives +inf
  if (!(s < 448.0f)) s = 448.0f;  // the reference's clamp of the scale (fp8/quantize.rs:31-33)
  state[0] = amax;
  state[1] = s;
  state[2] = 1.0f / s;
}

// ------------------------------------------------------------------------------------------------ absmax (two stages) and the quantizers
template <class T> __global__ void __launch_bounds__(256) fp8_pertensor_absmax_kernel(const T *__restrict__ in, size_t n, float *__restrict__ state) {
  __shared__ float sh[4];
  const size_t units = (n + 15) >> 4;
  float a = 0.0f, v[16];
  for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (size_t)gridDim.x * 256) {
    f8p_load16<T>(in, u << 4, n, v);
    a = fmaxf(a, f8p_amax16(v));
  }
  a = f8p_block_max(a, sh);
  if (threadIdx.x == 0) state[3 + blockIdx.x] = a;
}

__global__ void __launch_bounds__(256) fp8_pertensor_absmax_final_kernel(float *__restrict__ state, int parts) {
  __shared__ float sh[4];
  float a = 0.0f;
  for (int i = threadIdx.x; i < parts; i += 256) a = fmaxf(a, state[3 + i]);
  a = f8p_block_max(a, sh);
  if (threadIdx.x == 0) f8p_write_scales(a, state);
}

// DIV: q = T->fp8(x / *sp) (static; null sp = 1), else q = T->fp8(x * *sp) (dynamic: sp = state + 1)
template <class T, bool DIV, bool VEC>
__global__ void __launch_bounds__(256) fp8_pertensor_quantize_kernel(const T *__restrict__ in, uint8_t *__restrict__ q, size_t n, const float *__restrict__ sp) {
  const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x, i0 = u << 4;
  if (i0 >= n) return;
  const float s = sp ? *sp : 1.0f;
  float v[16];
  uint8_t c[16];
  f8p_load16<T>(in, i0, n, v);
#pragma unroll
  for (int j = 0; j < 16; ++j) c[j] = f8p_encode(DIV ? v[j] / s : v[j] * s);
  f8p_store16<VEC>(q, i0, n, c);
}

// small tensors (a decode step's activations): absmax, the scales and the quantizer in one workgroup, one launch.  The same bits as the staged path.
template <class T, bool VEC>
__global__ void __launch_bounds__(1024) fp8_pertensor_quantize_fused_kernel(const T *__restrict__ in, uint8_t *__restrict__ q, size_t n, float *__restrict__ state) {
  __shared__ float sh[16];
  const size_t units = (n + 15) >> 4;
  float a = 0.0f, v[16];
  for (size_t u = threadIdx.x; u < units; u += 1024) {
    f8p_load16<T>(in, u << 4, n, v);
    a = fmaxf(a, f8p_amax16(v));
  }
  a = f8p_block_max(a, sh);
  if (threadIdx.x == 0) f8p_write_scales(a, state);
  float s = 448.0f / a;
  if (!(s < 448.0f)) s = 448.0f;
  for (size_t u = threadIdx.x; u < units; u += 1024) {
    uint8_t c[16];
    f8p_load16<T>(in, u << 4, n, v);
#pragma unroll
    for (int j = 0; j < 16; ++j) c[j] = f8p_encode(v[j] * s);
    f8p_store16<VEC>(q, u << 4, n, c);
  }
}

// ------------------------------------------------------------------------------------------------ dequantize (optional row gather)
// one thread per 16 consecutive output elements of the flat [rows][K] output (`total` = rows K); output element i comes from row ids[i / K] (or i / K) of w.
// VEC: 16-byte aligned w / out, and K % 16 == 0 when rows are gathered, so that a whole unit is one 16-byte load inside one row.
template <class T, bool VEC>
__global__ void __launch_bounds__(256) fp8_pertensor_dequant_kernel(const uint8_t *__restrict__ w, const float *__restrict__ sp, const int32_t *__restrict__ ids,
                                                                    T *__restrict__ out, long long total, int K) {
  const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) << 4;
  if (i0 >= total) return;
  const float s = sp ? *sp : 1.0f;
  if (VEC && i0 + 16 <= total) {
    const int4 q = ld16_a16(ids ? w + (size_t)ids[i0 / K] * K + i0 % K : w + i0);
    const uint32_t qw[4] = {(uint32_t)q.x, (uint32_t)q.y, (uint32_t)q.z, (uint32_t)q.w};
    union {
      T t[16];
      int4_a16 v[sizeof(T)];
    } o;
#pragma unroll
    for (int j = 0; j < 16; ++j) o.t[j] = f8p_round<T>(fp8_e4m3_to_float((uint8_t)(qw[j >> 2] >> (8 * (j & 3)))) * s);
#pragma unroll
    for (int j = 0; j < (int)sizeof(T); ++j) ((int4_a16 *)(out + i0))[j] = o.v[j];
  } else {
    for (long long i = i0; i < i0 + 16 && i < total; ++i)
      out[i] = f8p_round<T>(fp8_e4m3_to_float(ids ? w[(size_t)ids[i / K] * K + i % K] : w[i]) * s);
  }
}

// ------------------------------------------------------------------------------------------------ route 1: skinny FP8 MFMA GEMV
constexpr int F8G_KC = 4096;         // xq bytes of a row staged at a time
constexpr int F8G_LD = F8G_KC + 16;  // LDS row stride: the 16-byte reads of 16 rows land on 16 different bank groups
constexpr int F8G_WAVES = 8;

// k slices per workgroup (1, 2, 4 or 8; the other factor of the 8 waves is row groups of 16): a function of N and K only.  Whole row groups per wave until the
// grid fills the chip, then K is split.
static int f8g_slices(int N, int K) {
  const int groups = (N + 15) / 16;
  int rg = F8G_WAVES;
  while (rg > 1 && (groups + rg - 1) / rg < 512) rg >>= 1;
  int ks = F8G_WAVES / rg;
  while (ks > 1 && K < 128 * ks) ks >>= 1;  // a slice is at least one 128-k step
  return ks;
}

template <class T>
__global__ void __launch_bounds__(512) fp8_pertensor_gemv_kernel(const uint8_t *__restrict__ xq, const uint8_t *__restrict__ wq, const float *__restrict__ dqx,
                                                                 const float *__restrict__ dqw, const T *__restrict__ bias, T *__restrict__ out, int M, int N, int K,
                                                                 int ks) {
  __shared__ float red[F8G_WAVES * 256];                             // [wave][register][lane]
  extern __shared__ __attribute__((aligned(16))) uint8_t f8g_xs[];   // [M][F8G_LD]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rgs = F8G_WAVES / ks, rg = wave / ks, sl = wave - rg * ks;
  const int r = lane & 15, g = lane >> 4;
  const int n = (blockIdx.x * rgs + rg) * 16 + r;
  const bool live = n < N, arow = r < M;
  const uint8_t *wr = wq + (size_t)(live ? n : 0) * K;
  const uint8_t *xr = f8g_xs + (arow ? r : 0) * F8G_LD;
  f8p_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int k0 = 0; k0 < K; k0 += F8G_KC) {
    const int kc = min(F8G_KC, K - k0), c16 = kc >> 4;
    __syncthreads();  // the previous chunk's reads are done
    for (int i = tid; i < M * c16; i += 512) {
      const int m = i / c16, c = i - m * c16;
      *(int4 *)(f8g_xs + m * F8G_LD + c * 16) = ld16_a16(xq + (size_t)m * K + k0 + c * 16);
    }
    __syncthreads();
    // this wave's slice of the chunk: whole 128-k steps, a function of K only
    const int span = (((kc + ks - 1) / ks) + 127) & ~127, kb = sl * span, ke = min(kb + span, kc);
#pragma unroll 2
    for (int k = kb; k < ke; k += 128) {
      const int ka = k + 16 * g, kh = ka + 64;  // this lane's two 16-byte pieces; a piece at or past kc is zeros on both sides
      const int4 z = make_int4(0, 0, 0, 0);
      const int4 w0 = (live && ka < kc) ? f8p_ld16nt(wr + k0 + ka) : z;
      const int4 w1 = (live && kh < kc) ? f8p_ld16nt(wr + k0 + kh) : z;
      const int4 a0 = (arow && ka < kc) ? *(const int4 *)(xr + ka) : z;
      const int4 a1 = (arow && kh < kc) ? *(const int4 *)(xr + kh) : z;
      acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(f8p_lo(a0), f8p_lo(w0), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(f8p_hi(a0), f8p_hi(w0), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(f8p_lo(a1), f8p_lo(w1), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(f8p_hi(a1), f8p_hi(w1), acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[wave * 256 + j * 64 + lane] = acc[j];
  __syncthreads();
  // C/D map of the 16x16 shapes: column (weight row) = lane & 15, row (activation row) = 4 (lane >> 4) + register
  const float sc = dqx[0] * dqw[0];
  for (int i = tid; i < rgs * 256; i += 512) {
    const int og = i >> 8, e = i & 255, m = 4 * ((e & 63) >> 4) + (e >> 6), on = (blockIdx.x * rgs + og) * 16 + (e & 15);
    float v = red[og * ks * 256 + e];
    for (int s = 1; s < ks; ++s) v += red[(og * ks + s) * 256 + e];  // slice order: fixed
    if (m < M && on < N) out[(size_t)m * N + on] = f8p_round<T>(fmaf(v, sc, bias ? to_f<T>(bias[on]) : 0.0f));
  }
}

// ------------------------------------------------------------------------------------------------ route 2: FP8 MFMA tile GEMM
constexpr int F8T = 128;          // tile edge in M, N and K (bytes)
constexpr int F8T_LD = F8T + 16;  // LDS row stride (144 B), as the 16-bit tiles of blockwise_fp8.hip

struct Fp8PtTileLds {
  uint8_t a[F8T * F8T_LD];  // xq [row][k]
  uint8_t b[F8T * F8T_LD];  // wq [n][k]
};

// A operand = xq [row][k], B operand = wq [n][k]; lane l of a wave reads the 16 bytes at k = 32 s + 16 (l >> 5) of row / column l & 31 and feeds its low 8 bytes to one
// v_mfma_f32_32x32x16_fp8_fp8 and its high 8 to the next.  Wave (wm, wn) owns the 64 x 64 block at (64 wm, 64 wn) of the tile.
template <class T>
__global__ void __launch_bounds__(256) fp8_pertensor_tile_kernel(const uint8_t *__restrict__ xq, const uint8_t *__restrict__ wq, const float *__restrict__ dqx,
                                                                 const float *__restrict__ dqw, const T *__restrict__ bias, T *__restrict__ out, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) Fp8PtTileLds L;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5, wm = wv >> 1, wn = wv & 1;
  const int m0 = blockIdx.y * F8T, n0 = blockIdx.x * F8T;
  // staging roles: the 16-byte piece at byte pc of rows pr + 32 i (8 threads read one row's 128 bytes)
  const int pc = (tid & 7) * 16, pr = tid >> 3;
  const uint8_t *arow[4], *brow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lr = pr + 32 * i;
    arow[i] = m0 + lr < M ? xq + (size_t)(m0 + lr) * K : nullptr;
    brow[i] = n0 + lr < N ? wq + (size_t)(n0 + lr) * K : nullptr;
  }
  int4 ra[4], rb[4];
  auto fetch = [&](int k0) {
    const bool in = k0 + pc < K;  // K % 16 == 0: a piece is whole or absent; absent pieces and rows are zeros
#pragma unroll
    for (int i = 0; i < 4; ++i) ra[i] = (arow[i] && in) ? ld16_a16(arow[i] + k0 + pc) : make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) rb[i] = (brow[i] && in) ? ld16_a16(brow[i] + k0 + pc) : make_int4(0, 0, 0, 0);
  };

  f8p_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  fetch(0);
  for (int k0 = 0; k0 < K; k0 += F8T) {
    __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(int4 *)&L.a[(pr + 32 * i) * F8T_LD + pc] = ra[i];
      *(int4 *)&L.b[(pr + 32 * i) * F8T_LD + pc] = rb[i];
    }
    __syncthreads();
    if (k0 + F8T < K) fetch(k0 + F8T);  // in flight behind the MFMAs
#pragma unroll
    for (int s = 0; s < F8T / 32; ++s) {
      if (k0 + 32 * s < K) {  // uniform; a half step past K multiplies staged zeros
        const int kk = 32 * s + 16 * h;
        int4 fa[2], fb[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          fa[i] = *(const int4 *)&L.a[(wm * 64 + i * 32 + r) * F8T_LD + kk];
          fb[i] = *(const int4 *)&L.b[(wn * 64 + i * 32 + r) * F8T_LD + kk];
        }
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(f8p_lo(fa[mi]), f8p_lo(fb[ni]), acc[mi][ni], 0, 0, 0);
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(f8p_hi(fa[mi]), f8p_hi(fb[ni]), acc[mi][ni], 0, 0, 0);
          }
      }
    }
  }
  // C/D map of the 32x32 shapes: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const float sc = dqx[0] * dqw[0];
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int col = n0 + wn * 64 + ni * 32 + r;
    if (col < N) {
      const float bv = bias ? to_f<T>(bias[col]) : 0.0f;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int row = m0 + wm * 64 + mi * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
          if (row < M) out[(size_t)row * N + col] = f8p_round<T>(fmaf(acc[mi][ni][j], sc, bv));
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------ route 3: general
// one wave per output element: row blockIdx.y + row0, column 4 blockIdx.x + wave
template <class T>
__global__ void __launch_bounds__(256) fp8_pertensor_general_kernel(const uint8_t *__restrict__ xq, const uint8_t *__restrict__ wq, const float *__restrict__ dqx,
                                                                    const float *__restrict__ dqw, const T *__restrict__ bias, T *__restrict__ out, int N, int K,
                                                                    int row0) {
  const int row = row0 + blockIdx.y, lane = threadIdx.x & 63, n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const uint8_t *xr = xq + (size_t)row * K, *wr = wq + (size_t)n * K;
  float p = 0.0f;
  for (int k = lane; k < K; k += 64) p = fmaf(fp8_e4m3_to_float(xr[k]), fp8_e4m3_to_float(wr[k]), p);
  p = wave_sum(p);
  if (lane == 0) out[(size_t)row * N + n] = f8p_round<T>(fmaf(p, dqx[0] * dqw[0], bias ? to_f<T>(bias[n]) : 0.0f));
}

// ------------------------------------------------------------------------------------------------ launchers
static int f8p_done() { return hipGetLastError() == hipSuccess ? 0 : -3; }

template <class T> static int f8p_absmax(const void *in, size_t n, float *state, hipStream_t st) {
  if (!state || (n && !in)) return -1;
  const size_t units = (n + 15) >> 4, want = (units + 255) / 256;
  const int parts = (int)(want < 1 ? 1 : want > (size_t)F8P_PARTIALS ? (size_t)F8P_PARTIALS : want);
  hipLaunchKernelGGL((fp8_pertensor_absmax_kernel<T>), dim3(parts), dim3(256), 0, st, (const T *)in, n, state);
  hipLaunchKernelGGL(fp8_pertensor_absmax_final_kernel, dim3(1), dim3(256), 0, st, state, parts);
  return f8p_done();
}

// grid of one thread per 16 elements
static bool f8p_grid(size_t n, unsigned &grid) {
  const size_t g = (((n + 15) >> 4) + 255) / 256;
  grid = (unsigned)g;
  return g <= 0x7fffffffULL;
}

template <class T> static int f8p_quant_dynamic(const void *in, uint8_t *q, size_t n, float *state, hipStream_t st) {
  if (!state || (n && (!in || !q))) return -1;
  const bool vec = ((uintptr_t)q & 15) == 0;
  unsigned grid;
  if (!f8p_grid(n, grid)) return -2;
  if (n <= (size_t)F8P_FUSED_MAX) {
    if (vec) hipLaunchKernelGGL((fp8_pertensor_quantize_fused_kernel<T, true>), dim3(1), dim3(1024), 0, st, (const T *)in, q, n, state);
    else hipLaunchKernelGGL((fp8_pertensor_quantize_fused_kernel<T, false>), dim3(1), dim3(1024), 0, st, (const T *)in, q, n, state);
    return f8p_done();
  }
  const int rc = f8p_absmax<T>(in, n, state, st);
  if (rc) return rc;
  if (vec) hipLaunchKernelGGL((fp8_pertensor_quantize_kernel<T, false, true>), dim3(grid), dim3(256), 0, st, (const T *)in, q, n, (const float *)(state + 1));
  else hipLaunchKernelGGL((fp8_pertensor_quantize_kernel<T, false, false>), dim3(grid), dim3(256), 0, st, (const T *)in, q, n, (const float *)(state + 1));
  return f8p_done();
}

template <class T> static int f8p_quant_static(const void *in, uint8_t *q, size_t n, const float *scale, hipStream_t st) {
  if (n == 0) return 0;
  if (!in || !q) return -1;
  unsigned grid;
  if (!f8p_grid(n, grid)) return -2;
  if (((uintptr_t)q & 15) == 0) hipLaunchKernelGGL((fp8_pertensor_quantize_kernel<T, true, true>), dim3(grid), dim3(256), 0, st, (const T *)in, q, n, scale);
  else hipLaunchKernelGGL((fp8_pertensor_quantize_kernel<T, true, false>), dim3(grid), dim3(256), 0, st, (const T *)in, q, n, scale);
  return f8p_done();
}

template <class T> static int f8p_dequant(const uint8_t *w, const float *scale, const int32_t *ids, void *out, long long rows, int K, hipStream_t st) {
  if (rows < 0 || K < 0) return -1;
  if (rows == 0 || K == 0) return 0;
  if (!w || !out || rows > 0x7fffffffffffffffLL / K) return -1;
  const long long total = rows * K, grid = (((total + 15) >> 4) + 255) / 256;
  if (grid > 0x7fffffffLL) return -2;
  if ((((uintptr_t)w | (uintptr_t)out) & 15) == 0 && (!ids || (K & 15) == 0))
    hipLaunchKernelGGL((fp8_pertensor_dequant_kernel<T, true>), dim3((unsigned)grid), dim3(256), 0, st, w, scale, ids, (T *)out, total, K);
  else hipLaunchKernelGGL((fp8_pertensor_dequant_kernel<T, false>), dim3((unsigned)grid), dim3(256), 0, st, w, scale, ids, (T *)out, total, K);
  return f8p_done();
}

template <class T>
static int f8p_matmul(const uint8_t *xq, const uint8_t *wq, const float *dqx, const float *dqw, const void *bias, void *out, int M, int N, int K, hipStream_t st) {
  if (M < 0 || N <= 0 || K <= 0 || !xq || !wq || !dqx || !dqw || !out) return -1;
  if (M == 0) return 0;
  const T *b = (const T *)bias;
  T *o = (T *)out;
  const bool fast = (K & 15) == 0 && (((uintptr_t)xq | (uintptr_t)wq) & 15) == 0;
  if (!fast) {
    g_fp8pt_route = 3;
    for (int r0 = 0; r0 < M; r0 += 65535)  // grid.y limit
      hipLaunchKernelGGL((fp8_pertensor_general_kernel<T>), dim3((N + 3) / 4, min(65535, M - r0)), dim3(256), 0, st, xq, wq, dqx, dqw, b, o, N, K, r0);
  } else if (M <= 16) {
    g_fp8pt_route = 1;
    const int ks = f8g_slices(N, K), rgs = F8G_WAVES / ks, lds = M * F8G_LD;
    if (lds + (int)sizeof(float) * F8G_WAVES * 256 > 60 * 1024) lds_attr_once((const void *)fp8_pertensor_gemv_kernel<T>, 16 * F8G_LD);
    hipLaunchKernelGGL((fp8_pertensor_gemv_kernel<T>), dim3(((N + 15) / 16 + rgs - 1) / rgs), dim3(64 * F8G_WAVES), (size_t)lds, st, xq, wq, dqx, dqw, b, o, M, N, K, ks);
  } else {
    if ((M + F8T - 1) / F8T > 65535) return -2;
    g_fp8pt_route = 2;
    hipLaunchKernelGGL((fp8_pertensor_tile_kernel<T>), dim3((N + F8T - 1) / F8T, (M + F8T - 1) / F8T), dim3(256), 0, st, xq, wq, dqx, dqw, b, o, M, N, K);
  }
  return f8p_done();
}

}  // namespace mrs

extern "C" {

// ---- the reference's scalar conversions (scalar_fp8/ffi.rs): the static quantizer / the dequantizer with scale 1
#define MRS_FP8_SCALAR(tag, T)                                                                                                  \
  void launch_fp8_to_##tag##_kernel(const uint8_t *d_input, T *d_output, size_t num_elements, hipStream_t stream) {             \
    (void)mrs::f8p_dequant<T>(d_input, nullptr, nullptr, d_output, (long long)num_elements, 1, stream); /* flat: rows of one */ \
  }                                                                                                                             \
  void launch_##tag##_to_fp8_kernel(const T *d_input, uint8_t *d_output, size_t num_elements, hipStream_t stream) {             \
    (void)mrs::f8p_quant_static<T>(d_input, d_output, num_elements, nullptr, stream);                                           \
  }
MRS_FP8_SCALAR(f32, float)
MRS_FP8_SCALAR(f16, mrs::f16_t)
MRS_FP8_SCALAR(bf16, mrs::bf16_t)
#undef MRS_FP8_SCALAR

#define MRS_FP8_PERTENSOR(tag, T)                                                                                                                        \
  int launch_fp8_pertensor_absmax_##tag(const void *in, size_t n, float *state, hipStream_t stream) { return mrs::f8p_absmax<T>(in, n, state, stream); } \
  int launch_fp8_pertensor_quantize_dynamic_##tag(const void *in, uint8_t *q, size_t n, float *state, hipStream_t stream) {                              \
    return mrs::f8p_quant_dynamic<T>(in, q, n, state, stream);                                                                                           \
  }                                                                                                                                                      \
  int launch_fp8_pertensor_quantize_static_##tag(const void *in, uint8_t *q, size_t n, const float *scale, hipStream_t stream) {                         \
    return mrs::f8p_quant_static<T>(in, q, n, scale, stream);                                                                                            \
  }                                                                                                                                                      \
  int launch_fp8_pertensor_dequantize_##tag(const uint8_t *w, const float *scale, const int32_t *ids, void *out, long long rows, int K,                  \
                                            hipStream_t stream) {                                                                                        \
    return mrs::f8p_dequant<T>(w, scale, ids, out, rows, K, stream);                                                                                     \
  }
MRS_FP8_PERTENSOR(f32, float)
MRS_FP8_PERTENSOR(f16, mrs::f16_t)
MRS_FP8_PERTENSOR(bf16, mrs::bf16_t)
#undef MRS_FP8_PERTENSOR

int launch_fp8_pertensor_matmul_f16(const uint8_t *xq, const uint8_t *wq, const float *dq_x, const float *dq_w, const void *bias, void *out, int M, int N, int K,
                                    hipStream_t stream) {
  return mrs::f8p_matmul<mrs::f16_t>(xq, wq, dq_x, dq_w, bias, out, M, N, K, stream);
}
int launch_fp8_pertensor_matmul_bf16(const uint8_t *xq, const uint8_t *wq, const float *dq_x, const float *dq_w, const void *bias, void *out, int M, int N, int K,
                                     hipStream_t stream) {
  return mrs::f8p_matmul<mrs::bf16_t>(xq, wq, dq_x, dq_w, bias, out, M, N, K, stream);
}

int fp8_pertensor_state_floats(void) { return 3 + mrs::F8P_PARTIALS; }
int fp8_pertensor_last_route(void) { return mrs::g_fp8pt_route; }

}  // extern "C"
