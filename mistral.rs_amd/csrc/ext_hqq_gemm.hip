// ext_hqq_gemm.hip -- fused HQQ dequant-GEMM for prompts (M > 8): out = x . W_hat^T (+ bias) straight from the packed 4-bit / 8-bit HQQ tensor on
// v_mfma_f32_32x32x16_{bf16,f16}; group size 64, axis 0, T in {bf16, f16}.  DESIGN 4.20.
//
// Format (ext_hqq_gemv.hip:7-9, hqq.hip:8-12): the [N, K] weight is viewed as [64, w], w = N K / 64, R = N / 64; element (n, k) sits in group row g = n / R and
// column j = (n % R) K + k; scale / zero are [w] in T; 8 bit: byte [g][j]; 4 bit: byte [r][j] holds group row r (high nibble) and r + 32 (low nibble).
// W_hat(n, k) = RNE_T(RNE_T(f32(q) - zero[j]) * scale[j]), the bits of dequantize_{4,8}bit_u8_kernel_*; y[m][n] = RNE_T(sum_k x W_hat + bias[n]) with f32
// accumulation and the bias added in f32 before the one rounding.
//
// Tile.  The 64 output rows that share one (scale, zero) K-vector lie R apart in the output, so an output tile is GR = 8 group rows x NL = 16 adjacent n_lo:
// TN = 128 columns, column c = 16 gi + nl is output row grow(gi) R + nl0 + nl (4 bit: the 4 packed rows 4 pt .. 4 pt + 3 give gi 0..3 from the high and gi 4..7
// from the low nibbles, grow = 4 pt + (gi & 3) + 32 (gi >> 2); 8 bit: grow = 8 pt + gi).  A lane's 32 accumulator columns are two runs of 16 adjacent outputs
// (32 bytes each); one (scale, zero) piece serves 8 group rows.  Per k-step of TK = 64 the packed bytes of the tile are 16-byte pieces (16 k of one packed row
// and n_lo): one per thread for 4 bit (32 weights), two for 8 bit, fetched with non-temporal loads into registers behind the previous step's MFMAs together with
// the A chunks; the step after next's scale / zero pieces (16 n_lo x 64 k, one 16-byte piece per thread) go through a double-buffered LDS block, so a step
// costs two barriers.  Each workgroup decodes its B tile once per k-step into LDS as T values (row stride 72 elements); 4 waves share it: TM = 128 rows
// (2 x 2 waves of 64 x 64) when M > 64, TM = 64 (4 waves of 64 x 32) otherwise, so the decode is spread over 128 rows whenever M has them.
// Small grids split K over gridDim.z workgroups (f32 partials in the caller's workspace, summed in split order by hqq_split_sum_kernel: no atomics, the split
// count is a function of M, N and K).  K past the end and n_lo past R are staged as zeros; rows past M and columns past R are not written.
#include "mxfp4_core.cuh"  // unpack2
#include <hip/hip_runtime.h>

namespace mrs {
namespace hqqg {

constexpr int TN = 128, TK = 64, NL = 16, LD = TK + 8, NT = 256;
constexpr int MAX_SPLIT = 8, MIN_SPLIT_STEPS = 8, TARGET_WGS = 256;  // a split holds at least 8 k-steps (512 k); one workgroup per CU is the target

typedef __bf16 hg_bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 hg_f16x2 __attribute__((ext_vector_type(2)));
typedef float hg_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 hg_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 hg_f16x8 __attribute__((ext_vector_type(8)));
typedef float hg_f32x16 __attribute__((ext_vector_type(16)));

// two f32 -> the bits of two T (RNE), the first in the low half
template <class T> __device__ __forceinline__ uint32_t rne2(float a, float b) {
  const hg_f32x2 v = {a, b};
  if constexpr (__is_same(T, bf16_t)) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, hg_bf16x2));
  else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, hg_f16x2));
}
// two weights: RNE_T(RNE_T(q - z) * s), both roundings explicit as hqqv::deq (q - z and the product of two T values are exact in f32)
template <class T> __device__ __forceinline__ uint32_t deq2(uint32_t q0, uint32_t q1, float z0, float z1, float s0, float s1) {
  float d0, d1;
  unpack2<T>(rne2<T>((float)q0 - z0, (float)q1 - z1), d0, d1);
  return rne2<T>(d0 * s0, d1 * s1);
}

template <class T> __device__ __forceinline__ hg_f32x16 mfma(const uint16_t *a, const uint16_t *b, hg_f32x16 c) {
  if constexpr (__is_same(T, bf16_t))
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const hg_bf16x8 *)a, *(const hg_bf16x8 *)b, c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const hg_f16x8 *)a, *(const hg_f16x8 *)b, c, 0, 0, 0);
}

struct Args {
  const uint8_t *wq; const void *scale, *zero, *x, *bias; void *out; float *ws;
  int N, K, M, ldx, ldo, nlt, sps;  // nlt = n_lo tiles per packed-row tile, sps = k-steps per split
};

// grid (8 nlt, M tiles, splits).  A operand = activations [row][k], B operand = W_hat [column][k]; lane l of a wave holds k = 8 (l >> 5) + j of row / column
// l & 31 in element j (as csrc/afq.hip).
template <int BITS, class T, int TM>
__global__ void __launch_bounds__(NT) hqq_gemm_kernel(const Args a) {
  constexpr int NP = BITS == 4 ? 1 : 2, PR = BITS == 4 ? 4 : 8;  // packed pieces per thread and k-step; packed rows per tile
  constexpr int NA = TM / 32, NI = TM == 128 ? 2 : 1;           // A chunks per thread; 32-column blocks per wave
  __shared__ __attribute__((aligned(16))) uint16_t La[TM * LD];      // x [row][k]
  __shared__ __attribute__((aligned(16))) uint16_t Lb[TN * LD];      // W_hat [column][k]
  __shared__ __attribute__((aligned(16))) uint16_t Lsz[2][2][NL * TK];  // [buffer][scale | zero][n_lo][k]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int K = a.K, R = a.N / 64, M = a.M;
  const size_t w = (size_t)R * K;
  const int pt = blockIdx.x / a.nlt, nl0 = (blockIdx.x % a.nlt) * NL, m0 = blockIdx.y * TM;
  const int nsteps = (K + TK - 1) / TK, s0 = blockIdx.z * a.sps, s1 = min(nsteps, s0 + a.sps);
  const int kend = min(K, s1 * TK);
  // staging roles.  B piece: 16 k at bk of n_lo nl0 + bnl, packed row PR pt + bpr (+ 4 for the second piece of 8 bit); scale (threads 0..127) / zero piece: 8 k
  // at zk of n_lo nl0 + znl; A chunk i: row (tid >> 3) + 32 i, 8 k at acol
  const int bk = (tid & 3) * 16, bnl = (tid >> 2) & 15, bpr = tid >> 6;
  const bool bok = nl0 + bnl < R;
  const uint8_t *bp = a.wq + (size_t)(pt * PR + bpr) * w + (size_t)(bok ? nl0 + bnl : 0) * K + bk;
  const int zk = (tid & 7) * 8, znl = (tid >> 3) & 15, zw = tid >> 7;
  const bool zok = nl0 + znl < R;
  const T *zp = (const T *)(zw ? a.zero : a.scale) + (size_t)(zok ? nl0 + znl : 0) * K + zk;
  const int acol = (tid & 7) * 8;
  const T *arow[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int lr = m0 + (tid >> 3) + 32 * i;
    arow[i] = lr < M ? (const T *)a.x + (size_t)lr * a.ldx : nullptr;
  }

  int4 ra[NA], rb[NP], rsz;
  auto fetch = [&](int k0) {  // K % 16 == 0: a piece is inside K or past it, never across
#pragma unroll
    for (int i = 0; i < NP; ++i) rb[i] = (bok && k0 + bk < K) ? ld16nt_a4(bp + (size_t)(4 * i) * w + k0) : make_int4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NA; ++i) ra[i] = (arow[i] && k0 + acol < K) ? ld16_a2(arow[i] + k0 + acol) : make_int4(0, 0, 0, 0);
  };
  auto fetch_sz = [&](int k0) { rsz = (zok && k0 + zk < kend) ? ld16_a16(zp + k0) : make_int4(0, 0, 0, 0); };

  hg_f32x16 acc[2][NI];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[mi][ni][j] = 0.0f;
  const int rbase = TM == 128 ? (wv >> 1) * 64 : 0, cbase = TM == 128 ? (wv & 1) * 64 : wv * 32;

  int k0 = s0 * TK, buf = 0;
  if (k0 < kend) {  // the first pieces are requested before anything is staged
    fetch_sz(k0);
    fetch(k0);
    *(int4 *)&Lsz[0][zw][znl * TK + zk] = rsz;
    fetch_sz(k0 + TK);
  }
  for (; k0 < kend; k0 += TK, buf ^= 1) {
    __syncthreads();  // the previous step's fragment reads are done; this step's scale / zero block is visible
#pragma unroll
    for (int i = 0; i < NA; ++i) *(int4 *)&La[((tid >> 3) + 32 * i) * LD + acol] = ra[i];
    {
      const uint16_t *ls = &Lsz[buf][0][bnl * TK + bk], *lz = &Lsz[buf][1][bnl * TK + bk];
      const int4 sv0 = *(const int4 *)ls, sv1 = *(const int4 *)(ls + 8), zv0 = *(const int4 *)lz, zv1 = *(const int4 *)(lz + 8);
      const uint32_t sw[8] = {(uint32_t)sv0.x, (uint32_t)sv0.y, (uint32_t)sv0.z, (uint32_t)sv0.w, (uint32_t)sv1.x, (uint32_t)sv1.y, (uint32_t)sv1.z, (uint32_t)sv1.w};
      const uint32_t zz[8] = {(uint32_t)zv0.x, (uint32_t)zv0.y, (uint32_t)zv0.z, (uint32_t)zv0.w, (uint32_t)zv1.x, (uint32_t)zv1.y, (uint32_t)zv1.z, (uint32_t)zv1.w};
      float s[16], z[16];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        unpack2<T>(sw[e], s[2 * e], s[2 * e + 1]);
        unpack2<T>(zz[e], z[2 * e], z[2 * e + 1]);
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const uint32_t q[4] = {(uint32_t)rb[i].x, (uint32_t)rb[i].y, (uint32_t)rb[i].z, (uint32_t)rb[i].w};
        uint32_t hi[8], lo[8];  // byte e of dword d is k = bk + 4 d + e
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const int e = 4 * d + 2 * p;
            const uint32_t b0 = (q[d] >> (16 * p)) & 0xff, b1 = (q[d] >> (16 * p + 8)) & 0xff;
            if constexpr (BITS == 4) {
              hi[2 * d + p] = deq2<T>(b0 >> 4, b1 >> 4, z[e], z[e + 1], s[e], s[e + 1]);
              lo[2 * d + p] = deq2<T>(b0 & 15, b1 & 15, z[e], z[e + 1], s[e], s[e + 1]);
            } else {
              hi[2 * d + p] = deq2<T>(b0, b1, z[e], z[e + 1], s[e], s[e + 1]);
            }
          }
        uint16_t *dst = &Lb[((bpr + 4 * i) * NL + bnl) * LD + bk];
        *(int4 *)dst = make_int4((int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]);
        *(int4 *)(dst + 8) = make_int4((int)hi[4], (int)hi[5], (int)hi[6], (int)hi[7]);
        if constexpr (BITS == 4) {  // the low nibbles are group rows + 32: tile columns + 64
          *(int4 *)(dst + 64 * LD) = make_int4((int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3]);
          *(int4 *)(dst + 64 * LD + 8) = make_int4((int)lo[4], (int)lo[5], (int)lo[6], (int)lo[7]);
        }
      }
    }
    *(int4 *)&Lsz[buf ^ 1][zw][znl * TK + zk] = rsz;  // the next step's block: its last readers passed this step's first barrier
    __syncthreads();
    if (k0 + TK < kend) {  // in flight behind the MFMAs
      fetch(k0 + TK);
      fetch_sz(k0 + 2 * TK);
    }
#pragma unroll
    for (int st = 0; st < TK / 16; ++st) {
      const int kk = 16 * st + 8 * h;
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const uint16_t *fb = &Lb[(cbase + ni * 32 + r) * LD + kk];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) acc[mi][ni] = mfma<T>(&La[(rbase + mi * 32 + r) * LD + kk], fb, acc[mi][ni]);
      }
    }
  }
  // C/D map of the 32x32 shapes: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const bool split = gridDim.z > 1;
  T *out = (T *)a.out;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int c = cbase + ni * 32 + r, gi = c >> 4, nl = nl0 + (c & 15);
    if (nl >= R) continue;
    const int n = (BITS == 4 ? pt * 4 + (gi & 3) + 32 * (gi >> 2) : pt * 8 + gi) * R + nl;
    const float bv = (a.bias && !split) ? to_f<T>(((const T *)a.bias)[n]) : 0.0f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int lr = m0 + rbase + mi * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
        if (lr < M) {
          if (split) a.ws[((size_t)blockIdx.z * M + lr) * a.N + n] = acc[mi][ni][j];
          else out[(size_t)lr * a.ldo + n] = from_f<T>(acc[mi][ni][j] + bv);
        }
      }
  }
}

// second stage of a split launch: the partials of an output element are added in split order, then the bias, then the one rounding
template <class T>
__global__ void __launch_bounds__(256) hqq_split_sum_kernel(const float *__restrict__ ws, const T *__restrict__ bias, T *__restrict__ out, int M, int N, int ldo,
                                                            int splits) {
  const size_t MN = (size_t)M * N, i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= MN) return;
  const int m = (int)(i / N), n = (int)(i - (size_t)m * N);
  float v = ws[i];
  for (int s = 1; s < splits; ++s) v += ws[(size_t)s * MN + i];
  out[(size_t)m * ldo + n] = from_f<T>(v + (bias ? to_f<T>(bias[n]) : 0.0f));
}

static int tile_rows(int M) { return M <= 64 ? 64 : 128; }

// K splits: a function of M, N and K only
static int splits(int M, int N, int K) {
  const int tm = tile_rows(M), nlt = (N / 64 + NL - 1) / NL;
  const long long tiles = 8LL * nlt * ((M + tm - 1) / tm);
  const int nsteps = (K + TK - 1) / TK;
  long long s = TARGET_WGS / tiles;
  if (s > MAX_SPLIT) s = MAX_SPLIT;
  if (s > nsteps / MIN_SPLIT_STEPS) s = nsteps / MIN_SPLIT_STEPS;
  return s < 1 ? 1 : (int)s;
}

template <int BITS, class T> static int launch(Args a, hipStream_t st) {
  const int tm = tile_rows(a.M), sp = splits(a.M, a.N, a.K), nsteps = (a.K + TK - 1) / TK;
  if (sp > 1 && !a.ws) return -1;  // the split is a function of the shape; a caller asks mrs_hqq_gemm_workspace_floats and brings the floats
  const int mt = (a.M + tm - 1) / tm;
  if (mt > 65535) return -2;
  a.nlt = (a.N / 64 + NL - 1) / NL;
  a.sps = (nsteps + sp - 1) / sp;
  const dim3 grid(8 * a.nlt, mt, sp);
  if (tm == 64) hipLaunchKernelGGL((hqq_gemm_kernel<BITS, T, 64>), grid, dim3(NT), 0, st, a);
  else hipLaunchKernelGGL((hqq_gemm_kernel<BITS, T, 128>), grid, dim3(NT), 0, st, a);
  if (sp > 1) {
    const size_t mn = (size_t)a.M * a.N;
    hipLaunchKernelGGL((hqq_split_sum_kernel<T>), dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, st, (const float *)a.ws, (const T *)a.bias, (T *)a.out, a.M, a.N,
                       a.ldo, sp);
  }
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace hqqg
}  // namespace mrs

// x [M][ldx], out [M][ldo], scale / zero [N K / 64], bias [N] or NULL, all of dtype 1 = f16 or 2 = bf16; wq = the packed tensor of HqqLayer ([32, N K / 64] bytes
// for 4 bit, [64, N K / 64] for 8 bit; group size 64, axis 0).  workspace: mrs_hqq_gemm_workspace_floats(N, K, M) floats (may be NULL when that is 0).  Takes the
// stream it is given and does not synchronise.  Returns 0; -1 = arguments outside the kernel (other bit widths, N % 64, K % 16, f32, pointers that are not
// 16-byte aligned, a missing workspace: the caller keeps dequantize + dense matmul); -2 = too many row tiles; -3 = launch error.
extern "C" int mrs_hqq_gemm(int bits, int dtype, const void *wq, const void *scale, const void *zero, const void *bias, const void *x, int ldx, void *out, int ldo,
                            int N, int K, int M, float *workspace, void *stream) {
  using namespace mrs::hqqg;
  if ((bits != 4 && bits != 8) || (dtype != 1 && dtype != 2) || N <= 0 || K <= 0 || M <= 0 || N % 64 || K % 16 || ldx < K || ldo < N || !wq || !scale || !zero ||
      !x || !out)
    return -1;
  if ((((uintptr_t)wq | (uintptr_t)scale | (uintptr_t)zero | (uintptr_t)x | (uintptr_t)out | (uintptr_t)workspace) & 15) || ((uintptr_t)bias & 1)) return -1;
  const Args a{(const uint8_t *)wq, scale, zero, x, bias, out, workspace, N, K, M, ldx, ldo, 0, 0};
  hipStream_t st = (hipStream_t)stream;
  if (bits == 4) return dtype == 1 ? launch<4, mrs::f16_t>(a, st) : launch<4, mrs::bf16_t>(a, st);
  return dtype == 1 ? launch<8, mrs::f16_t>(a, st) : launch<8, mrs::bf16_t>(a, st);
}

extern "C" size_t mrs_hqq_gemm_workspace_floats(int N, int K, int M) {
  if (N <= 0 || K <= 0 || M <= 0 || N % 64) return 0;
  const int s = mrs::hqqg::splits(M, N, K);
  return s > 1 ? (size_t)s * M * N : 0;
}
