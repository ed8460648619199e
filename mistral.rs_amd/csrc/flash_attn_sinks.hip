// flash_attn_sinks.hip -- causal / sliding-window prompt attention with per-head sinks on dense Q / K / V, on the gfx950 matrix cores.
//
// Role in the reference: the two prefill ops of every model with attention sinks (GPT-OSS), mistralrs-paged-attn/src/cuda/flash_attn_sinks.cu
// (`flash_attn_sinks`, `flash_attn_sinks_varlen`; called from mistralrs-core/src/attention/backends/sinks.rs).  Semantics:
//   dense   Q, O [B, H, q_len, D]      K, V [B, Hkv, kv_len, D]
//   varlen  Q, O [B, H, max_q_len, D]  K, V [total_kv, Hkv, D], lengths from cu_seqlens_q / cu_seqlens_k; rows >= the sequence's q_len are not written
//   row r attends keys max(0, r + off - W + 1) .. r + off (W > 0) or 0 .. r + off (W == 0), off = kv_len - q_len; after the key loop the sink joins
//   the denominator only; out = O * (l > 0 ? 1 / l : 0).
//
// MI355X design.  One wave owns 32 query rows of one head.  A workgroup holds NW waves that read the same K / V: the heads of one KV head for one
// 32-row query tile (G = H / Hkv >= 3), or NW consecutive query tiles of one head (G <= 2).  Per 32-key tile:
//   * the workgroup copies the K and V tile from global memory into registers with coalesced 16-byte loads -- the NEXT tile's loads are issued before
//     the current tile's MFMAs -- and from there into LDS.  K goes in row-major with a 16-byte row pad, so the A fragment of S^T = K Q^T (lane = key,
//     8 consecutive dims) is one conflict-free ds_read_b128.  V is written TRANSPOSED, [d][key] with two keys packed per 32-bit word and a row of 18
//     words: the B fragment of O += P V (lane = d, 2 x 4 consecutive keys) is two ds_read_b64, conflict-free on the read side (18 d mod 64 hits
//     every even bank once per 32 lanes) and on the write side (a wave writes 4 chunks x 16 key pairs: banks 16 c + p).  The transposing LDS loads of
//     gfx950 were not used: the packed-pair write costs 8 ds_write_b32 per 32 bytes once per workgroup, while the reads, which every wave repeats,
//     are plain 8-byte reads either way;
//   * S^T = K Q^T on v_mfma_f32_32x32x16_{bf16,f16} with the Q^T fragments resident in registers; a lane then holds 16 keys of ONE query, so the
//     online softmax is register math plus one exchange with lane ^ 32; P is rounded to the tensor dtype and is, in place, the A fragment of O += P V
//     (the key order inside a 16-key MFMA step is free as long as V is read in the same order);
//   * key tiles before the window of every row of the workgroup, or after its last causal key, are never loaded; a wave skips the tiles outside its own
//     rows' range (it still helps to stage them);
//   * keys >= kv_len and dims >= D (80 -> 96, 112 -> 128) are zeros written into LDS, never read from memory.
// f32 tensors keep f32 arithmetic on v_mfma_f32_32x32x2f32 in the same frame (K, V staged as f32, V row-major: the k = 2 B fragment is a scalar
// read, no transpose needed; P not rounded).  At D = 192 / 256 the f32 K and V tiles share one LDS region (they would not fit side by side in 64 KiB),
// take two more barriers per tile and are copied without the register prefetch.  The f32 path is correct, not tuned.
#include "common.cuh"
#include "mistralrs_paged_attn.h"
#include <float.h>

namespace mrs {
namespace fas {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

template <class T> struct Mma;
template <> struct Mma<bf16_t> {
  static __device__ __forceinline__ f32x16 run(uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ unsigned pk(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
  }
};
template <> struct Mma<f16_t> {
  static __device__ __forceinline__ f32x16 run(uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ unsigned pk(float a, float b) {
    const f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
  }
};
template <> struct Mma<float> {};

struct Args {
  const void *q, *k, *v;
  void *o;
  const float *sinks;
  const unsigned *cu_q, *cu_k;  // varlen only
  float scale;
  int q_rows;   // rows of Q / O per (batch, head): q_len, or max_q_len for varlen
  int kv_len;   // dense only
  int H, Hkv, D, W;
  int hpb, qpb, chunks;  // heads and query tiles per workgroup (hpb * qpb = NW); head chunks per KV head
};

constexpr int KT = 32;  // keys per tile

template <class T, int DP> struct Lds {
  static constexpr bool F32 = sizeof(T) == 4;
  static constexpr bool ALIAS = F32 && DP >= 192;
  static constexpr int K_ROW = F32 ? (DP + 4) * 4 : DP * 2 + 16;  // bytes
  static constexpr int V_ROW = F32 ? (DP + 8) * 4 : 18 * 4;       // f32: per key; 16-bit: per d (16 key pairs + 2 pad words)
  static constexpr int K_BYTES = KT * K_ROW;
  static constexpr int V_BYTES = F32 ? KT * V_ROW : DP * V_ROW;
  static constexpr int V_OFF = ALIAS ? 0 : K_BYTES;
  static constexpr int BYTES = ALIAS ? (K_BYTES > V_BYTES ? K_BYTES : V_BYTES) : K_BYTES + V_BYTES;
};

template <class T, int DP, int NW>
__global__ void __launch_bounds__(64 * NW) flash_attn_sinks_kernel(const Args a) {
  using L = Lds<T, DP>;
  constexpr bool F32 = L::F32, ALIAS = L::ALIAS;
  constexpr int NT = 64 * NW;
  constexpr int EPC = 16 / (int)sizeof(T);         // elements per 16-byte chunk
  constexpr int NCH = DP / EPC;                    // chunks per (padded) row
  constexpr int NKI = (KT * NCH + NT - 1) / NT;    // K chunks per thread and tile
  constexpr int NVU = F32 ? KT * NCH : (KT / 2) * NCH;  // V units: f32 one chunk, 16-bit the same chunk of two consecutive keys
  constexpr int NVI = (NVU + NT - 1) / NT;
  constexpr int NDT = DP / 32;
  __shared__ __attribute__((aligned(16))) unsigned char smem[L::BYTES];
  __shared__ __attribute__((aligned(16))) float bc[NW][32];  // per-wave broadcast of per-query factors

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int ql = lane & 31, kh = lane >> 5;
  const int b = blockIdx.z;
  const int G = a.H / a.Hkv;
  const int kvh = blockIdx.y / a.chunks, hl = (blockIdx.y % a.chunks) * a.hpb + wave % a.hpb;
  const int head = kvh * G + min(hl, G - 1);
  const int qt = blockIdx.x * a.qpb + wave / a.hpb;

  int q_len, kv_len;
  size_t kv_base, kv_row;  // element offsets of this (batch, KV head)'s key 0 and between keys
  if (a.cu_q) {
    q_len = (int)(a.cu_q[b + 1] - a.cu_q[b]);
    kv_len = (int)(a.cu_k[b + 1] - a.cu_k[b]);
    kv_row = (size_t)a.Hkv * a.D;
    kv_base = (size_t)a.cu_k[b] * kv_row + (size_t)kvh * a.D;
  } else {
    q_len = a.q_rows;
    kv_len = a.kv_len;
    kv_row = a.D;
    kv_base = ((size_t)b * a.Hkv + kvh) * (size_t)kv_len * a.D;
  }
  const int q_first = blockIdx.x * a.qpb * 32;
  if (q_first >= q_len) return;  // whole workgroup, before any barrier
  const int q_last = min(q_first + a.qpb * 32, q_len) - 1;
  const int off = kv_len - q_len;
  const int kv_start = a.W > 0 ? max(0, q_first + off - a.W + 1) : 0;
  const int kv_end = min(kv_len, q_last + off + 1);

  // this wave's rows and the key range they can see
  const int wq0 = qt * 32;
  const bool wave_on = hl < G && wq0 < q_len;
  const int w_hi = min(wq0 + 31, q_len - 1) + off;
  const int w_lo = a.W > 0 ? max(0, wq0 + off - a.W + 1) : 0;
  // this lane's query (column of S^T)
  const int qrow = wq0 + ql;
  const bool q_ok = wave_on && qrow < q_len;
  const int hi = q_ok ? qrow + off : -1;
  const int lo = a.W > 0 ? max(0, qrow + off - a.W + 1) : 0;
  const size_t qo_base = (((size_t)b * a.H + head) * a.q_rows) * a.D;

  // ---- Q^T fragments, resident for the whole key loop
  uint4 qf[F32 ? 1 : DP / 16];
  float qs[F32 ? DP / 2 : 1];
  {
    const T *qp = (const T *)a.q + qo_base + (size_t)min(qrow, q_len - 1) * a.D;
    if constexpr (F32) {  // MFMA step (s, i) multiplies dims 8 s + 4 kh + i
#pragma unroll
      for (int s = 0; s < DP / 8; ++s) {
        const int d = 8 * s + 4 * kh;
        const float4 x = d < a.D ? *(const float4 *)(qp + d) : make_float4(0.f, 0.f, 0.f, 0.f);
        qs[4 * s] = x.x; qs[4 * s + 1] = x.y; qs[4 * s + 2] = x.z; qs[4 * s + 3] = x.w;
      }
    } else {  // lane (query ql, half kh) holds dims 16 ds + 8 kh .. + 8
#pragma unroll
      for (int ds = 0; ds < DP / 16; ++ds) {
        const int d = 16 * ds + 8 * kh;
        qf[ds] = d < a.D ? *(const uint4 *)(qp + d) : make_uint4(0, 0, 0, 0);
      }
    }
  }
  f32x16 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m = -FLT_MAX, l = 0.f;

  // ---- staging: global -> registers -> LDS
  uint4 kreg[NKI], vreg[F32 ? NVI : 2 * NVI];
  const T *kg = (const T *)a.k + kv_base, *vg = (const T *)a.v + kv_base;
  auto load_k = [&](int t0) {
#pragma unroll
    for (int i = 0; i < NKI; ++i) {
      const int u = tid + i * NT, key = u / NCH, c = u % NCH;
      const bool ok = u < KT * NCH && t0 + key < kv_end && c * EPC < a.D;
      kreg[i] = ok ? *(const uint4 *)(kg + (size_t)(t0 + key) * kv_row + c * EPC) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_k = [&]() {
#pragma unroll
    for (int i = 0; i < NKI; ++i) {
      const int u = tid + i * NT, key = u / NCH, c = u % NCH;
      if (u < KT * NCH) *(uint4 *)(smem + key * L::K_ROW + c * 16) = kreg[i];
    }
  };
  auto load_v = [&](int t0) {
#pragma unroll
    for (int i = 0; i < NVI; ++i) {
      const int u = tid + i * NT;
      if constexpr (F32) {
        const int key = u / NCH, c = u % NCH;
        const bool ok = u < NVU && t0 + key < kv_end && c * EPC < a.D;
        vreg[i] = ok ? *(const uint4 *)(vg + (size_t)(t0 + key) * kv_row + c * EPC) : make_uint4(0, 0, 0, 0);
      } else {  // a wave takes 4 chunks x 16 key pairs: lane -> (pair p, chunk c)
        const int c = 4 * (u >> 6) + (lane & 3), key = 2 * (lane >> 2);
        const bool ok = u < NVU && c * EPC < a.D;
        const T *p = vg + (size_t)(t0 + key) * kv_row + c * EPC;
        vreg[2 * i] = ok && t0 + key < kv_end ? *(const uint4 *)p : make_uint4(0, 0, 0, 0);
        vreg[2 * i + 1] = ok && t0 + key + 1 < kv_end ? *(const uint4 *)(p + kv_row) : make_uint4(0, 0, 0, 0);
      }
    }
  };
  auto store_v = [&]() {
#pragma unroll
    for (int i = 0; i < NVI; ++i) {
      const int u = tid + i * NT;
      if (u >= NVU) continue;
      if constexpr (F32) {
        const int key = u / NCH, c = u % NCH;
        *(uint4 *)(smem + L::V_OFF + key * L::V_ROW + c * 16) = vreg[i];
      } else {  // transposed: word [d][p] = (V[2p][d], V[2p + 1][d])
        const int c = 4 * (u >> 6) + (lane & 3), p = lane >> 2;
        unsigned *vt = (unsigned *)(smem + L::V_OFF) + (c * 8) * 18 + p;
        const unsigned e[4] = {vreg[2 * i].x, vreg[2 * i].y, vreg[2 * i].z, vreg[2 * i].w};
        const unsigned f[4] = {vreg[2 * i + 1].x, vreg[2 * i + 1].y, vreg[2 * i + 1].z, vreg[2 * i + 1].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          vt[(2 * j) * 18] = (e[j] & 0xffffu) | (f[j] << 16);
          vt[(2 * j + 1) * 18] = (e[j] >> 16) | (f[j] & 0xffff0000u);
        }
      }
    }
  };

  if constexpr (!ALIAS)
    if (kv_start < kv_end) {
      load_k(kv_start);
      load_v(kv_start);
    }
  for (int t0 = kv_start; t0 < kv_end; t0 += KT) {
    const bool more = t0 + KT < kv_end;
    const bool need = wave_on && t0 <= w_hi && t0 + KT > w_lo;  // wave-uniform
    if constexpr (ALIAS) load_k(t0);  // no register prefetch here: Q^T alone takes half of the vector registers
    store_k();
    if constexpr (!ALIAS) store_v();
    __syncthreads();
    if constexpr (!ALIAS)
      if (more) {
        load_k(t0 + KT);
        load_v(t0 + KT);
      }
    float p[16];
    if (need) {
      // ---- S^T = K Q^T (32 keys x 32 queries)
      f32x16 sacc;
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
      if constexpr (F32) {
        const float *kp = (const float *)(smem + ql * L::K_ROW) + 4 * kh;
#pragma unroll
        for (int s = 0; s < DP / 8; ++s) {
          const float4 x = *(const float4 *)(kp + 8 * s);
          sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, qs[4 * s], sacc, 0, 0, 0);
          sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, qs[4 * s + 1], sacc, 0, 0, 0);
          sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, qs[4 * s + 2], sacc, 0, 0, 0);
          sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, qs[4 * s + 3], sacc, 0, 0, 0);
        }
      } else {
        const unsigned char *kp = smem + ql * L::K_ROW + kh * 16;
#pragma unroll
        for (int ds = 0; ds < DP / 16; ++ds) sacc = Mma<T>::run(*(const uint4 *)(kp + ds * 32), qf[ds], sacc);
      }
      // ---- online softmax for query column ql: this lane holds keys (r & 3) + 8 (r >> 2) + 4 kh of the tile
      float sv[16], mx = -FLT_MAX;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kpos = t0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
        sv[r] = kpos >= lo && kpos <= hi ? sacc[r] * a.scale : -FLT_MAX;
        mx = fmaxf(mx, sv[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m, mx);
      const float alpha = F32 ? expf(m - mn) : __expf(m - mn);
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = sv[r] > -FLT_MAX ? (F32 ? expf(sv[r] - mn) : __expf(sv[r] - mn)) : 0.f;
        ps += p[r];
      }
      ps += __shfl_xor(ps, 32, 64);
      l = l * alpha + ps;
      m = mn;
      // ---- rescale O: accumulator register r of a lane belongs to query row (r & 3) + 8 (r >> 2) + 4 kh
      if (kh == 0) bc[wave][ql] = alpha;
      float ar[16];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float4 t4 = *(const float4 *)(&bc[wave][8 * g4 + 4 * kh]);
        ar[4 * g4] = t4.x; ar[4 * g4 + 1] = t4.y; ar[4 * g4 + 2] = t4.z; ar[4 * g4 + 3] = t4.w;
      }
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= ar[r];
    }
    if constexpr (ALIAS) {
      __syncthreads();
      load_v(t0);
      store_v();
      __syncthreads();
    }
    if (need) {
      // ---- O += P V
      if constexpr (F32) {
        const float *vp = (const float *)(smem + L::V_OFF) + ql;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float *vr = vp + ((j & 3) + 8 * (j >> 2) + 4 * kh) * (L::V_ROW / 4);
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[j], vr[dt * 32], o[dt], 0, 0, 0);
        }
      } else {  // P fragments are the S^T registers in place, rounded to the tensor dtype
        const unsigned *vp = (const unsigned *)(smem + L::V_OFF) + ql * 18 + 2 * kh;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const uint4 pf = make_uint4(Mma<T>::pk(p[8 * s], p[8 * s + 1]), Mma<T>::pk(p[8 * s + 2], p[8 * s + 3]),
                                      Mma<T>::pk(p[8 * s + 4], p[8 * s + 5]), Mma<T>::pk(p[8 * s + 6], p[8 * s + 7]));
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            const uint2 v0 = *(const uint2 *)(vp + dt * 32 * 18 + 8 * s), v1 = *(const uint2 *)(vp + dt * 32 * 18 + 8 * s + 4);
            o[dt] = Mma<T>::run(pf, make_uint4(v0.x, v0.y, v1.x, v1.y), o[dt]);
          }
        }
      }
    }
    __syncthreads();
  }
  if (!wave_on) return;

  // ---- the sink joins the denominator only; normalise and store
  float fac;
  {
    float al = 1.f;
    if (a.sinks) {
      const float sk = a.sinks[head];
      const float mn = fmaxf(m, sk);
      al = expf(m - mn);
      l = l * al + expf(sk - mn);
    }
    fac = l > 0.f ? al / l : 0.f;
  }
  if (kh == 0) bc[wave][ql] = fac;
  float inv[16];
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const float4 t4 = *(const float4 *)(&bc[wave][8 * g4 + 4 * kh]);
    inv[4 * g4] = t4.x; inv[4 * g4 + 1] = t4.y; inv[4 * g4 + 2] = t4.z; inv[4 * g4 + 3] = t4.w;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = wq0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
    if (row < q_len) {
      T *op = (T *)a.o + qo_base + (size_t)row * a.D + ql;
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
        if (dt * 32 + ql < a.D) op[dt * 32] = from_f<T>(o[dt][r] * inv[r]);
    }
  }
}

template <class T, int DP> static void launch_dp(const Args &a0, int batch, hipStream_t s) {
  Args a = a0;
  const int G = a.H / a.Hkv;
  int nw;
  if (G <= 2) {  // several query tiles of one head
    nw = 4; a.hpb = 1; a.qpb = 4; a.chunks = G;
  } else {       // the heads of one KV head, in chunks of nw
    // D = 192 / 256 always take 4 waves (a wave of a chunk past G idles): 256 threads leave each wave the full 512 registers, and 4 waves keep the
    // staging share per thread small enough for the f32 kernel to stay out of scratch
    nw = DP >= 192 ? 4 : G % 8 == 0 ? 8 : G % 4 == 0 ? 4 : G % 3 == 0 ? 3 : 4;
    a.hpb = nw; a.qpb = 1; a.chunks = (G + nw - 1) / nw;
  }
  const dim3 grid((a.q_rows + 32 * a.qpb - 1) / (32 * a.qpb), a.Hkv * a.chunks, batch);
  if (nw == 4) hipLaunchKernelGGL((flash_attn_sinks_kernel<T, DP, 4>), grid, dim3(256), 0, s, a);
  else if constexpr (DP < 192) {
    if (nw == 3) hipLaunchKernelGGL((flash_attn_sinks_kernel<T, DP, 3>), grid, dim3(192), 0, s, a);
    else hipLaunchKernelGGL((flash_attn_sinks_kernel<T, DP, 8>), grid, dim3(512), 0, s, a);
  }
}

template <class T>
static void launch(const void *Q, const void *K, const void *V, void *O, const float *sinks, const unsigned *cu_q, const unsigned *cu_k, float scale,
                   int batch, int q_rows, int kv_len, int H, int Hkv, int D, int W, void *stream) {
  if (batch <= 0 || q_rows <= 0 || H <= 0 || Hkv <= 0 || H % Hkv) return;
  const Args a{Q, K, V, O, sinks, cu_q, cu_k, scale, q_rows, kv_len, H, Hkv, D, W > 0 ? W : 0, 0, 0, 0};
  hipStream_t s = (hipStream_t)stream;
  switch (D) {  // any other head size launches nothing, like the reference
  case 64: launch_dp<T, 64>(a, batch, s); break;
  case 80: case 96: launch_dp<T, 96>(a, batch, s); break;
  case 112: case 128: launch_dp<T, 128>(a, batch, s); break;
  case 192: launch_dp<T, 192>(a, batch, s); break;
  case 256: launch_dp<T, 256>(a, batch, s); break;
  default: return;
  }
  const hipError_t e = hipGetLastError();  // a launch error ends the process, like the reference's FA_CUDA_CHECK
  if (e != hipSuccess) {
    fprintf(stderr, "flash_attn_sinks: launch failed: %s\n", hipGetErrorString(e));
    abort();
  }
}

}  // namespace fas
}  // namespace mrs

#define MRS_FAS_ENTRY(tag, T)                                                                                                                        \
  extern "C" void flash_attn_sinks_##tag(const void *Q, const void *K, const void *V, void *O, const float *sinks, float scale, int batch_size,      \
                                         int q_len, int kv_len, int num_heads, int num_kv_heads, int head_dim, int window_size, void *stream) {     \
    mrs::fas::launch<T>(Q, K, V, O, sinks, nullptr, nullptr, scale, batch_size, q_len, kv_len, num_heads, num_kv_heads, head_dim, window_size,       \
                        stream);                                                                                                                     \
  }                                                                                                                                                  \
  extern "C" void flash_attn_sinks_varlen_##tag(const void *Q, const void *K, const void *V, void *O, const float *sinks,                            \
                                                const unsigned *cu_seqlens_q, const unsigned *cu_seqlens_k, float scale, int batch_size,             \
                                                int max_q_len, int num_heads, int num_kv_heads, int head_dim, int window_size, void *stream) {       \
    if (!cu_seqlens_q || !cu_seqlens_k) return;                                                                                                      \
    mrs::fas::launch<T>(Q, K, V, O, sinks, cu_seqlens_q, cu_seqlens_k, scale, batch_size, max_q_len, 0, num_heads, num_kv_heads, head_dim,           \
                        window_size, stream);                                                                                                        \
  }
MRS_FAS_ENTRY(f16, mrs::f16_t)
MRS_FAS_ENTRY(bf16, mrs::bf16_t)
MRS_FAS_ENTRY(f32, float)
#undef MRS_FAS_ENTRY
