// gptq.hip -- GPTQ / AWQ (2/3/4/8-bit codes, f16 scales, act-order g_idx) reconstruct, matmul and AWQ repack kernels and the reference's GPTQ C ABI, MI355X /
// gfx950, wave64.
//
// Drop-in for the non-exllama, non-Marlin symbols of mistralrs-quant/src/gptq/ffi.rs (reconstruct_gptq, gemm_half_q_half_alt; no stream argument: the null
// stream), behind GptqLayer (gptq/gptq_cuda.rs), plus the stream-taking launchers launch_gptq_matmul / launch_gptq_reconstruct / launch_awq_repack that the
// native entry points of ext_gptq.hip forward to.
//
// Format (GPTQ layout, the one every matmul kernel here reads): qweight u32 [K * bits / 32][N], column n holds its K codes as one little-endian bit stream
// down the rows (32 consecutive k = `bits` whole word rows, a "unit"; 3-bit codes 10 and 21 of a unit straddle two words); qzeros u32 [G][N * bits / 32],
// the same stream along N; scales f16 [G][N]; g_idx i32 [K], any map from row to group (act-order); bits in {2, 3, 4, 8}; K % 32 == 0 and N % 32 == 0.
// The g_idx values are trusted to lie in [0, G): the host mirror checks them once at load time.
//
// Weight, every route: W[k][n] = f16_rne((q - (z + zero_offset)) * s) -- the integer q - z - zero_offset in [-256, 255] is exact in f16 and the product is ONE
// f16 multiply (v_pk_mul_f16 on a pair of rows), exactly `__hmul(__int2half_rn(q - z - 1), s)` of the reference's reconstruct_gptq.  z + zero_offset is not
// wrapped: a stored 15 at 4 bits means 16.  zero_offset is 1 for GPTQ checkpoints and 0 for AWQ ones after launch_awq_repack.
// Output, every route: y[m][n] = f16_rne(sum_k x[m][k] W[k][n] + bias[n]) with f32 accumulation (a product of two f16 values is exact in f32), the bias added
// in f32 before the ONE rounding.  The reference rounds twice, f16(f16(acc) + bias), and its gemm_half_q_half_alt accumulates in f16 with atomics.
// Every output element is written once by a plain store; nothing depends on what the output held; the same launch gives the same bits.
//
// Routes:
//   1  M <= 8   streaming GEMV on the checkpoint layout: lane = column (64 columns per workgroup, a word row is one coalesced 256-byte read), the units of K
//               dealt round-robin over the workgroup's waves, so g_idx[k] and the activations are wave-uniform reads; a column keeps its group's scale and zero
//               until g_idx changes.  Per-wave f32 partials meet in LDS and are summed in wave order.  The number of waves depends on N and K only and a
//               row's chain does not depend on M: a row of an M = 8 call has the bits of its M = 1 call.
//   2  M > 8    LDS-staged 64 x 128 x 128 tile on v_mfma_f32_32x32x16_f16: the B operand is W itself, decoded once per workgroup (one thread per column and
//               unit) into LDS as f16, so act-order needs nothing special; f32 accumulators, the bias in the epilogue.  Untuned.
#include "afq_core.cuh"  // afq_code: code j of a 32-code little-endian unit; unpack2

namespace mrs {

static int g_gptq_route = 0;

typedef _Float16 gptq_h2 __attribute__((ext_vector_type(2)));
typedef _Float16 gptq_f16x8 __attribute__((ext_vector_type(8)));
typedef float gptq_f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ constexpr bool gptq_bits_ok(int bits) { return bits == 2 || bits == 3 || bits == 4 || bits == 8; }

// stored zero point of column n in one qzeros row
template <int BITS> __device__ __forceinline__ int gptq_zero(const uint32_t *zrow, int n) {
  const int bit = n * BITS, wd = bit >> 5, sh = bit & 31;
  uint32_t z = zrow[wd] >> sh;
  if (BITS == 3 && sh > 29) z |= zrow[wd + 1] << (32 - sh);  // N % 32 == 0: a row is whole 3-word units, a straddle never leaves the row
  return (int)(z & ((1u << BITS) - 1u));
}

// One column's scale and zero, kept while g_idx stays on the same group.
struct GptqCol {
  int g, zo;  // current group (-1: none yet), stored zero + zero_offset
  f16_t s;
};

// The 32 weights of one unit of column n as 16 f16 pairs (rows 2 j, 2 j + 1): wd = the unit's BITS words, gi = g_idx + the unit's first row.
template <int BITS>
__device__ __forceinline__ void gptq_unit(const uint32_t (&wd)[BITS], const int *__restrict__ gi, const f16_t *__restrict__ sc, const uint32_t *__restrict__ qz,
                                          int N, int n, int off, GptqCol &c, gptq_h2 (&w)[16]) {
  const int zw = (N * BITS) >> 5;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    gptq_h2 d, s;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int g = gi[2 * j + e];
      if (g != c.g) {
        c.g = g;
        c.s = sc[(size_t)g * N + n];
        c.zo = gptq_zero<BITS>(qz + (size_t)g * zw, n) + off;
      }
      d[e] = (f16_t)((int)afq_code<BITS>(wd, 2 * j + e) - c.zo);
      s[e] = c.s;
    }
    w[j] = d * s;
  }
}

// ------------------------------------------------------------------------------------------------ reconstruct: f16 [K][N]
template <int BITS>
__global__ void __launch_bounds__(256) gptq_reconstruct_kernel(const uint32_t *__restrict__ qw, const uint32_t *__restrict__ qz, const f16_t *__restrict__ sc,
                                                               const int *__restrict__ gidx, f16_t *__restrict__ out, int N, int K, int off) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)(K >> 5) * N) return;
  const int u = (int)(i / N), n = (int)(i - (long long)u * N);
  uint32_t wd[BITS];
#pragma unroll
  for (int b = 0; b < BITS; ++b) wd[b] = qw[((size_t)u * BITS + b) * N + n];
  GptqCol c = {-1, 0, (f16_t)0.0f};
  gptq_h2 w[16];
  gptq_unit<BITS>(wd, gidx + 32 * u, sc, qz, N, n, off, c, w);
  f16_t *dst = out + (size_t)u * 32 * N + n;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    dst[(size_t)(2 * j) * N] = w[j][0];
    dst[(size_t)(2 * j + 1) * N] = w[j][1];
  }
}

// ------------------------------------------------------------------------------------------------ route 1: streaming GEMV
constexpr int GQ_MAXW = 16;  // waves per workgroup at most

template <int BITS, int MR>
__global__ void __launch_bounds__(1024) gptq_gemv_kernel(const f16_t *__restrict__ x, const uint32_t *__restrict__ qw, const uint32_t *__restrict__ qz,
                                                         const f16_t *__restrict__ sc, const int *__restrict__ gidx, const f16_t *__restrict__ bias,
                                                         f16_t *__restrict__ y, int M, int N, int K, int off) {
  __shared__ float red[GQ_MAXW * MR * 64];  // [wave][row][lane]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), nw = (int)(blockDim.x >> 6);
  const int col = blockIdx.x * 64 + lane, n = col < N ? col : N - 1;  // lanes past N decode the last column and write nothing
  const int nu = K >> 5;
  float acc[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) acc[m] = 0.0f;
  GptqCol c = {-1, 0, (f16_t)0.0f};
  for (int u = wave; u < nu; u += nw) {
    uint32_t wd[BITS];
#pragma unroll
    for (int b = 0; b < BITS; ++b) wd[b] = __builtin_nontemporal_load(qw + ((size_t)u * BITS + b) * N + n);
    gptq_h2 w[16];
    gptq_unit<BITS>(wd, gidx + 32 * u, sc, qz, N, n, off, c, w);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      float wf[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        wf[2 * e] = (float)w[4 * jj + e][0];
        wf[2 * e + 1] = (float)w[4 * jj + e][1];
      }
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        // rows past M read row M - 1 again and are not written; x may start on any 2-byte boundary
        const int4 v = ld16_a2(x + (size_t)(m < M ? m : M - 1) * K + 32 * u + 8 * jj);
        float a[8];
        unpack2<f16_t>((uint32_t)v.x, a[0], a[1]);
        unpack2<f16_t>((uint32_t)v.y, a[2], a[3]);
        unpack2<f16_t>((uint32_t)v.z, a[4], a[5]);
        unpack2<f16_t>((uint32_t)v.w, a[6], a[7]);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[m] = fmaf(a[e], wf[e], acc[m]);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MR; ++m) red[(wave * MR + m) * 64 + lane] = acc[m];
  __syncthreads();
  for (int i = threadIdx.x; i < MR * 64; i += blockDim.x) {
    const int m = i >> 6, l = i & 63, oc = blockIdx.x * 64 + l;
    float v = red[m * 64 + l];
    for (int wv = 1; wv < nw; ++wv) v += red[(wv * MR + m) * 64 + l];  // wave order: fixed
    if (oc < N && m < M) y[(size_t)m * N + oc] = (f16_t)(v + (bias ? (float)bias[oc] : 0.0f));
  }
}

// waves per workgroup: enough for ~4096 waves on the chip, one unit per wave at least; a function of N and K only
static int gptq_gemv_waves(int N, int K) {
  const int wgs = (N + 63) / 64, nu = K >> 5;
  int nw = (4096 + wgs - 1) / wgs;
  if (nw > GQ_MAXW) nw = GQ_MAXW;
  if (nw > nu) nw = nu;
  return nw < 1 ? 1 : nw;
}

template <int BITS, int MR>
static void gptq_gemv_rows(const f16_t *x, const uint32_t *qw, const uint32_t *qz, const f16_t *sc, const int *gidx, const f16_t *bias, f16_t *y, int M, int N,
                           int K, int off, hipStream_t st) {
  hipLaunchKernelGGL((gptq_gemv_kernel<BITS, MR>), dim3((N + 63) / 64), dim3(64 * gptq_gemv_waves(N, K)), 0, st, x, qw, qz, sc, gidx, bias, y, M, N, K, off);
}

// ------------------------------------------------------------------------------------------------ route 2: MFMA tile on the reconstructed W
constexpr int GTM = 64, GTN = 128, GTK = 128;
constexpr int GLD = GTK + 8;  // LDS row stride in f16 (272 B), as the AFQ tile: the 16-byte fragment reads of 32 consecutive rows spread over the banks

struct GptqTileLds {
  uint16_t a[GTM * GLD];  // x [row][k]
  uint16_t b[GTN * GLD];  // W [n][k]
};

// A operand = activations [row][k], B operand = W [n][k]; lane l of a wave holds k = 8 (l >> 5) + j of row / column l & 31 in element j (as csrc/afq.hip).
template <int BITS>
__global__ void __launch_bounds__(256) gptq_tile_kernel(const f16_t *__restrict__ x, const uint32_t *__restrict__ qw, const uint32_t *__restrict__ qz,
                                                        const f16_t *__restrict__ sc, const int *__restrict__ gidx, const f16_t *__restrict__ bias,
                                                        f16_t *__restrict__ y, int M, int N, int K, int off) {
  __shared__ __attribute__((aligned(16))) GptqTileLds L;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5, nu = K >> 5;
  const int m0 = blockIdx.y * GTM, n0 = blockIdx.x * GTN;
  // staging roles: A chunks (row (tid >> 4) + 16 i, 8 k at acol); B units (column tid & 127: coalesced word rows; unit (tid >> 7) + 2 i, uniform over a wave)
  const int acol = (tid & 15) * 8, bl = tid & 127, bu = tid >> 7;
  const int bn = n0 + bl < N ? n0 + bl : N - 1;  // columns past N stage the last column; their outputs are not written
  const f16_t *arow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lr = m0 + (tid >> 4) + 16 * i;
    arow[i] = lr < M ? x + (size_t)lr * K : nullptr;
  }
  int4 ra[4];
  uint32_t rb[2][BITS];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) ra[i] = (arow[i] && k0 + acol < K) ? ld16_a2(arow[i] + k0 + acol) : make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int gu = (k0 >> 5) + bu + 2 * i;
#pragma unroll
      for (int b = 0; b < BITS; ++b) rb[i][b] = gu < nu ? qw[((size_t)gu * BITS + b) * N + bn] : 0u;
    }
  };

  gptq_f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[i][j] = 0.0f;
  GptqCol c = {-1, 0, (f16_t)0.0f};

  fetch(0);
  for (int k0 = 0; k0 < K; k0 += GTK) {
    __syncthreads();  // the previous step's fragment reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) *(int4 *)&L.a[((tid >> 4) + 16 * i) * GLD + acol] = ra[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int uu = bu + 2 * i, gu = (k0 >> 5) + uu;
      uint16_t *dst = &L.b[bl * GLD + uu * 32];
      if (gu < nu) {  // uniform over the wave
        gptq_h2 w[16];
        gptq_unit<BITS>(rb[i], gidx + 32 * gu, sc, qz, N, bn, off, c, w);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          uint32_t p[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) p[e] = __builtin_bit_cast(uint32_t, w[4 * jj + e]);
          *(int4 *)(dst + 8 * jj) = make_int4((int)p[0], (int)p[1], (int)p[2], (int)p[3]);
        }
      } else {  // past K: zeros against the zero-filled activations
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) *(int4 *)(dst + 8 * jj) = make_int4(0, 0, 0, 0);
      }
    }
    __syncthreads();
    if (k0 + GTK < K) fetch(k0 + GTK);  // in flight behind the MFMAs
    const int steps = (K - k0 < GTK ? K - k0 : GTK) >> 4;
    for (int s = 0; s < steps; ++s) {
      const int kk = 16 * s + 8 * h;
      const gptq_f16x8 fb = *(const gptq_f16x8 *)&L.b[(wv * 32 + r) * GLD + kk];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
        acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const gptq_f16x8 *)&L.a[(mi * 32 + r) * GLD + kk], fb, acc[mi], 0, 0, 0);
    }
  }
  // C/D map of the 32x32 shapes: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int col = n0 + wv * 32 + r;
  if (col < N) {
    const float bv = bias ? (float)bias[col] : 0.0f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int lr = m0 + mi * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
        if (lr < M) y[(size_t)lr * N + col] = (f16_t)(acc[mi][j] + bv);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ AWQ -> GPTQ layout
// AWQ packs along N with the in-word position of logical column j of a word being undo(j) = (j >> 1) + (pack / 2) (j & 1): {0,4,1,5,2,6,3,7} at 4 bits,
// {0,2,1,3} at 8 (the table of the reference's awq_marlin_repack_kernel).  One thread per output word of qweight [K * bits / 32][N], then of qzeros
// [G][N * bits / 32], then per g_idx entry; every output word is assembled in a register and written once.
template <int BITS>
__global__ void __launch_bounds__(256) awq_repack_kernel(const uint32_t *__restrict__ qw_in, const uint32_t *__restrict__ qz_in, uint32_t *__restrict__ qw_out,
                                                         uint32_t *__restrict__ qz_out, int *__restrict__ gidx_out, int K, int N, int groups, int group_size) {
  constexpr int PACK = 32 / BITS;
  constexpr uint32_t MASK = (1u << BITS) - 1u;
  const long long nqw = (long long)(K / PACK) * N, nqz = (long long)groups * (N / PACK);
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < nqw) {
    const int rw = (int)(i / N), n = (int)(i - (long long)rw * N), j = n % PACK, sh = ((j >> 1) + (PACK / 2) * (j & 1)) * BITS;
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < PACK; ++e) word |= ((qw_in[(size_t)(rw * PACK + e) * (N / PACK) + n / PACK] >> sh) & MASK) << (e * BITS);
    qw_out[i] = word;
    return;
  }
  i -= nqw;
  if (i < nqz) {
    const uint32_t v = qz_in[i];
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < PACK; ++j) word |= ((v >> (((j >> 1) + (PACK / 2) * (j & 1)) * BITS)) & MASK) << (j * BITS);
    qz_out[i] = word;
    return;
  }
  i -= nqz;
  if (i < K) gidx_out[i] = (int)(i / group_size);
}

// ------------------------------------------------------------------------------------------------ launchers
static bool gptq_args_ok(const void *qw, const void *qz, const void *sc, const void *gidx, int N, int K, int bits, int off) {
  return qw && qz && sc && gidx && N > 0 && K > 0 && (N & 31) == 0 && (K & 31) == 0 && gptq_bits_ok(bits) && (off == 0 || off == 1);
}

template <int BITS>
static void gptq_matmul_bits(const f16_t *x, const uint32_t *qw, const uint32_t *qz, const f16_t *sc, const int *gidx, const f16_t *bias, f16_t *y, int M, int N,
                             int K, int off, hipStream_t st) {
  if (M <= 8) {
    g_gptq_route = 1;
    // the register rows are padded to 1, 2, 4 or 8
    if (M == 1) gptq_gemv_rows<BITS, 1>(x, qw, qz, sc, gidx, bias, y, M, N, K, off, st);
    else if (M == 2) gptq_gemv_rows<BITS, 2>(x, qw, qz, sc, gidx, bias, y, M, N, K, off, st);
    else if (M <= 4) gptq_gemv_rows<BITS, 4>(x, qw, qz, sc, gidx, bias, y, M, N, K, off, st);
    else gptq_gemv_rows<BITS, 8>(x, qw, qz, sc, gidx, bias, y, M, N, K, off, st);
  } else {
    g_gptq_route = 2;
    hipLaunchKernelGGL((gptq_tile_kernel<BITS>), dim3((N + GTN - 1) / GTN, (M + GTM - 1) / GTM), dim3(256), 0, st, x, qw, qz, sc, gidx, bias, y, M, N, K, off);
  }
}

static int gptq_matmul(const void *x, const void *qw, const void *qz, const void *sc, const void *gidx, const void *bias, void *y, int M, int N, int K, int bits,
                       int off, void *stream) {
  if (!x || !y || M < 0 || !gptq_args_ok(qw, qz, sc, gidx, N, K, bits, off)) return -1;
  if (M == 0) return 0;
  if ((M + GTM - 1) / GTM > 65535) return -2;
#define MRS_GPTQ_MM(B)                                                                                                                                          \
  gptq_matmul_bits<B>((const f16_t *)x, (const uint32_t *)qw, (const uint32_t *)qz, (const f16_t *)sc, (const int *)gidx, (const f16_t *)bias, (f16_t *)y, M, N, \
                      K, off, (hipStream_t)stream)
  switch (bits) {
  case 2: MRS_GPTQ_MM(2); break;
  case 3: MRS_GPTQ_MM(3); break;
  case 4: MRS_GPTQ_MM(4); break;
  default: MRS_GPTQ_MM(8); break;
  }
#undef MRS_GPTQ_MM
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

static int gptq_reconstruct(const void *qw, const void *qz, const void *sc, const void *gidx, void *out, int K, int N, int bits, int off, void *stream) {
  if (!out || !gptq_args_ok(qw, qz, sc, gidx, N, K, bits, off)) return -1;
  const long long grid = ((long long)(K >> 5) * N + 255) / 256;
  if (grid > 0x7fffffffLL) return -2;
#define MRS_GPTQ_RC(B)                                                                                                                                  \
  hipLaunchKernelGGL((gptq_reconstruct_kernel<B>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)qw, (const uint32_t *)qz, \
                     (const f16_t *)sc, (const int *)gidx, (f16_t *)out, N, K, off)
  switch (bits) {
  case 2: MRS_GPTQ_RC(2); break;
  case 3: MRS_GPTQ_RC(3); break;
  case 4: MRS_GPTQ_RC(4); break;
  default: MRS_GPTQ_RC(8); break;
  }
#undef MRS_GPTQ_RC
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace mrs

extern "C" {

int launch_gptq_matmul(const void *x, const void *qweight, const void *qzeros, const void *scales, const void *g_idx, const void *bias, void *y, int M, int N, int K,
                       int groups, int bits, int zero_offset, void *stream) {
  if (groups <= 0) return -1;
  return mrs::gptq_matmul(x, qweight, qzeros, scales, g_idx, bias, y, M, N, K, bits, zero_offset, stream);
}

int launch_gptq_reconstruct(const void *qweight, const void *qzeros, const void *scales, const void *g_idx, void *out, int K, int N, int groups, int bits,
                            int zero_offset, void *stream) {
  if (groups <= 0) return -1;
  return mrs::gptq_reconstruct(qweight, qzeros, scales, g_idx, out, K, N, bits, zero_offset, stream);
}

int launch_awq_repack(const void *qweight, const void *qzeros, void *qweight_out, void *qzeros_out, void *g_idx_out, int K, int N, int groups, int group_size,
                      int bits, void *stream) {
  if (!qweight || !qzeros || !qweight_out || !qzeros_out || !g_idx_out || K <= 0 || N <= 0 || (K & 31) || (N & 31) || (bits != 4 && bits != 8) || group_size <= 0 ||
      K % group_size || groups != K / group_size)
    return -1;
  const int pack = 32 / bits;
  const long long total = (long long)(K / pack) * N + (long long)groups * (N / pack) + K, grid = (total + 255) / 256;
  if (grid > 0x7fffffffLL) return -2;
  if (bits == 4)
    hipLaunchKernelGGL((mrs::awq_repack_kernel<4>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)qweight, (const uint32_t *)qzeros,
                       (uint32_t *)qweight_out, (uint32_t *)qzeros_out, (int *)g_idx_out, K, N, groups, group_size);
  else
    hipLaunchKernelGGL((mrs::awq_repack_kernel<8>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)qweight, (const uint32_t *)qzeros,
                       (uint32_t *)qweight_out, (uint32_t *)qzeros_out, (int *)g_idx_out, K, N, groups, group_size);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

int gptq_last_route(void) { return mrs::g_gptq_route; }

// ---- the reference's symbols (gptq/ffi.rs): GPTQ layout, zero offset 1, null stream, no return value.  gemm_half_q_half_alt takes any m and bits 2 / 3 / 4 / 8.
void reconstruct_gptq(const uint32_t *b_q_weight, const uint32_t *b_qzeros, const uint16_t *b_scales, const int *b_q_perm, uint16_t *out, int size_k, int size_n,
                      int groups, int bit) {
  (void)groups;
  (void)mrs::gptq_reconstruct(b_q_weight, b_qzeros, b_scales, b_q_perm, out, size_k, size_n, bit, 1, nullptr);
}

void gemm_half_q_half_alt(const uint16_t *a, const uint32_t *b_q_weight, const uint32_t *b_qzeros, const uint16_t *b_scales, const int *b_g_idx, uint16_t *out, int m,
                          int n, int k, int bit) {
  (void)mrs::gptq_matmul(a, b_q_weight, b_qzeros, b_scales, b_g_idx, nullptr, out, m, n, k, bit, 1, nullptr);
}

}  // extern "C"
