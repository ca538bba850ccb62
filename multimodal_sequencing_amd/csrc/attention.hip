// Fused multi-head attention, head_dim 64, flash-style (no T x T materialisation), fwd + bwd.
// Replaces BertAttention.forward (lxrt/modeling.py:398-425) and nn.MultiheadAttention in the
// CLIP ViT blocks (clip/model.py:219-221). See include/mmseq.h for the layout contract.
//
// Workgroup = 4 waves; each wave owns 16 rows (queries in fwd / dQ, keys in dK/dV); the
// 64-row tiles of the other operand are staged through LDS ([64][80] bf16: a 160-byte row
// stride makes both the 16-byte row reads and the ds_read_b64_tr_b16 transposed reads
// bank-conflict-free). MFMA 16x16x32 bf16 (perf) or 16x16x4 f32 (parity), f32 softmax.
//
// fwd  (swapped QK^T, guide §B "Fused attention"): S^T = K Q^T puts the query on the lane and the
//      keys in registers, so row max / row sum are in-lane plus two xor-shuffles; P^T is then
//      directly the B operand of O^T = V^T P^T (V^T fragments by transposed reads).
// bwd  two deterministic kernels (no float atomics):
//      dkdv: per key tile, sweep the queries: S, dP with the key on the lane; dV^T += dO^T P and
//            dK^T += Q^T dS take P / dS straight from the accumulators.
//      dq:   per query tile, sweep the keys with the swapped form; dQ^T += K^T dS^T.
#include "gemm_common.h"
#include "launch_plan.h"
#include <type_traits>

namespace {

using namespace mmseq_plan;  // grids, LDS bytes and kernel choice of the bf16 fast kernels

constexpr int HD = 64;       // head dim
constexpr int QT = 64;       // rows per workgroup tile
constexpr float NEG = -1e30f;

template <typename TI> struct ACfg;
template <> struct ACfg<unsigned short> { static constexpr int LD = 80, VE = 8; };
template <> struct ACfg<float> { static constexpr int LD = 68, VE = 4; };

template <typename TI> struct V16;
template <> struct V16<unsigned short> { typedef u16x8 T; };
template <> struct V16<float> { typedef f32x4 T; };

struct AttnArgs {
  int P, T, heads;
  const void* qkv; int64_t ld_qkv, q_off, k_off, v_off;
  const float* key_bias; float scale;
  const void* out; int64_t ld_out;
  const void* dout; int64_t ld_dout;
  float* lse; float* delta;
  void* dqkv; int64_t ld_dqkv;
  void* o_w;  // fwd output
  Drop drop;  // attention-probability dropout
  uint64_t* bits;  // bf16 fast path: keep-mask words [(p*heads+h)*T + q][nkt2], bit j = key 64*kt + j
  int nkt2;        // key tiles per row, rounded up to even (16-byte rows for the dK/dV staging)
  // tail fold (bf16 dK/dV kernel): when 1 <= T % 128 <= 16 the last 128-row block of each (pair,
  // head) also owns rows tail0 .. T-1 (tail0 = 128 * (T / 128)); 0 = no fold. nxq = row blocks.
  // dK/dV launches: blocks x = xoff .. xoff + nxl - 1 of every (pair, head) (the tail block runs in
  // a launch of its own, so the other blocks' kernel carries no tail state)
  int tail0, nxq, xoff, nxl;
  // query rows per pair (bf16 fast kernels; the other kernels take Tq == T): queries 0 .. Tq-1 of
  // every pair against all T keys; O / dO hold Tq rows per pair (row p * Tq + q)
  int Tq;
  // bf16 forward, Q8: the output in MX-fp8 (fp8.hip layout) instead of bf16: e4m3 [P*T][ldq8] +
  // packed scales for (P*T, heads*64) columns
  uint8_t* q8; int64_t ldq8; uint8_t* q8s;
};

// Stage rows [r0, r0+64) of one head's 64-wide slice into LDS tile s ([64][LD]); zero-fill >= T.
template <typename TI>
__device__ __forceinline__ void stage_tile(TI* s, const TI* base, int64_t ld, int r0, int T,
                                           int tid) {
  typedef typename V16<TI>::T V;
  constexpr int VE = ACfg<TI>::VE, LD = ACfg<TI>::LD;
  constexpr int CPR = HD / VE;             // chunks per row
  constexpr int NCH = (QT * CPR) / 256;    // chunks per thread
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    int L = c * 256 + tid;
    int r = L / CPR, cc = L % CPR;
    V v;
    if (r0 + r < T) {
      v = *reinterpret_cast<const V*>(base + (int64_t)(r0 + r) * ld + cc * VE);
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) v[e] = 0;
    }
    *reinterpret_cast<V*>(s + r * LD + cc * VE) = v;
  }
}

// bf16 fragment helpers (LD = 80)
__device__ __forceinline__ bf16x8_t row_frag(const unsigned short* s, int rb, int ks, int lane) {
  const unsigned short* p = s + (rb + (lane & 15)) * 80 + ks * 32 + (lane >> 4) * 8;
  return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8*>(p));
}
__device__ __forceinline__ bf16x8_t tr_frag(const unsigned short* s, int cb, int ks, int lane) {
  int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
  const unsigned short* a0 = s + (ks * 32 + 4 * g + q) * 80 + cb + 4 * p;
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MMSEQ_LDS s16x4*)(a0));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MMSEQ_LDS s16x4*)(a0 + 16 * 80));
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
// registers of a 16x16 f32 accumulator pair (sub-tiles 2ks, 2ks+1) -> bf16 B/A fragment
__device__ __forceinline__ bf16x8_t pack_pair(const f32x4& x, const f32x4& y) {
  u16x8 v = {f2bf(x[0]), f2bf(x[1]), f2bf(x[2]), f2bf(x[3]),
             f2bf(y[0]), f2bf(y[1]), f2bf(y[2]), f2bf(y[3])};
  return __builtin_bit_cast(bf16x8_t, v);
}
// load a row fragment (16 rows at r0, lane row i, 8 contiguous cols at ks*32+8g) from global
__device__ __forceinline__ bf16x8_t glob_row_frag(const unsigned short* base, int64_t ld, int r,
                                                  int T, int ks, int lane) {
  u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  if (r < T) v = *reinterpret_cast<const u16x8*>(base + (int64_t)r * ld + ks * 32 + (lane >> 4) * 8);
  return __builtin_bit_cast(bf16x8_t, v);
}

template <typename TI>
__device__ __forceinline__ f32x4 mfma16(const bf16x8_t& a, const bf16x8_t& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// ============================================================================================
// forward
// ============================================================================================
template <typename TI>
__global__ __launch_bounds__(256) void attn_fwd_kernel(AttnArgs a) {
  constexpr int LD = ACfg<TI>::LD;
  __shared__ __attribute__((aligned(16))) TI sK[QT * LD];
  __shared__ __attribute__((aligned(16))) TI sV[QT * LD];
  __shared__ float sBias[QT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int h = blockIdx.y, p = blockIdx.z;
  const int q0 = blockIdx.x * QT + wave * 16;
  const int T = a.T;
  const TI* base = reinterpret_cast<const TI*>(a.qkv) + (int64_t)p * T * a.ld_qkv;
  const TI* Qb = base + a.q_off + h * HD;
  const TI* Kb = base + a.k_off + h * HD;
  const TI* Vb = base + a.v_off + h * HD;
  const float* kb_bias = a.key_bias ? a.key_bias + (int64_t)p * T : nullptr;

  f32x4 o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) o[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m = NEG, l = 0.f;

  // Q fragments (B operand of S^T = K Q^T): lane (g,i) -> Q[q0+i][...]
  bf16x8_t qf[2];
  float qs[16];
  if constexpr (sizeof(TI) == 2) {
    qf[0] = glob_row_frag((const unsigned short*)Qb, a.ld_qkv, q0 + i, T, 0, lane);
    qf[1] = glob_row_frag((const unsigned short*)Qb, a.ld_qkv, q0 + i, T, 1, lane);
  } else {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
      qs[kk] = (q0 + i < T) ? ((const float*)Qb)[(int64_t)(q0 + i) * a.ld_qkv + kk * 4 + g] : 0.f;
  }

  const int nkt = (T + QT - 1) / QT;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * QT;
    stage_tile<TI>(sK, Kb, a.ld_qkv, k0, T, tid);
    stage_tile<TI>(sV, Vb, a.ld_qkv, k0, T, tid);
    if (tid < QT) {
      int key = k0 + tid;
      sBias[tid] = key < T ? (kb_bias ? kb_bias[key] : 0.f) : NEG;
    }
    __syncthreads();
    f32x4 s[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      s[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if constexpr (sizeof(TI) == 2) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          s[kb] = mfma16<TI>(row_frag((const unsigned short*)sK, kb * 16, ks, lane), qf[ks], s[kb]);
      } else {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
          s[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(((const float*)sK)[(kb * 16 + i) * LD + kk * 4 + g],
                                                        qs[kk], s[kb], 0, 0, 0);
      }
    }
    float mx = m;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = s[kb][r] * a.scale + sBias[kb * 16 + 4 * g + r];
        s[kb][r] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float alpha = __expf(m - mx);
    m = mx;
    float rs = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float e = __expf(s[kb][r] - m);
        s[kb][r] = e;
        rs += e;
      }
    rs += __shfl_xor(rs, 16, 64);
    rs += __shfl_xor(rs, 32, 64);
    l = l * alpha + rs;
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] *= alpha;
    if (a.drop.thr) {  // the normaliser l keeps the undropped probabilities (dropout after softmax)
      const uint64_t rowi = (((uint64_t)p * a.heads + h) * T + (q0 + i)) * (uint64_t)((T + 3) & ~3) + k0;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kb][r] *= drop_mul(a.drop, rowi + kb * 16 + 4 * g + r);
    }
    if constexpr (sizeof(TI) == 2) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_t pf = pack_pair(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
        for (int d = 0; d < 4; ++d)
          o[d] = mfma16<TI>(tr_frag((const unsigned short*)sV, d * 16, ks, lane), pf, o[d]);
      }
    } else {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int d = 0; d < 4; ++d)
            o[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                ((const float*)sV)[(kb * 16 + 4 * g + r) * LD + d * 16 + i], s[kb][r], o[d], 0, 0, 0);
    }
    __syncthreads();
  }
  const int q = q0 + i;
  if (q < T) {
    const float inv = 1.0f / l;
    TI* op = reinterpret_cast<TI*>(a.o_w) + ((int64_t)p * T + q) * a.ld_out + h * HD;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) Elem<TI>::st(op + d * 16 + 4 * g + r, o[d][r] * inv);
    if (g == 0) a.lse[((int64_t)p * a.heads + h) * T + q] = m + __logf(l);
  }
}

// ============================================================================================
// backward: delta = rowsum(dO * O)
// ============================================================================================
template <typename TI>
__global__ __launch_bounds__(256) void attn_delta_kernel(AttnArgs a) {
  // one wave per (p, t) row handles all heads: lane covers 64 dims of one head at a time
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  const int64_t rows = (int64_t)a.P * a.T;
  if (row >= rows) return;
  const int p = row / a.T, t = row % a.T;
  const TI* o = reinterpret_cast<const TI*>(a.out) + row * a.ld_out;
  const TI* dO = reinterpret_cast<const TI*>(a.dout) + row * a.ld_dout;
  for (int h = 0; h < a.heads; ++h) {
    float v = Elem<TI>::ld(o + h * HD + lane) * Elem<TI>::ld(dO + h * HD + lane);
    v = wave_sum(v);
    if (lane == 0) a.delta[((int64_t)p * a.heads + h) * a.T + t] = v;
  }
}

// ============================================================================================
// backward: dK, dV (per 64-key tile; each wave owns 16 keys; queries swept through LDS)
// ============================================================================================
template <typename TI>
__global__ __launch_bounds__(256) void attn_dkdv_kernel(AttnArgs a) {
  constexpr int LD = ACfg<TI>::LD;
  __shared__ __attribute__((aligned(16))) TI sQ[QT * LD];
  __shared__ __attribute__((aligned(16))) TI sdO[QT * LD];
  __shared__ float sL[QT], sD[QT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int h = blockIdx.y, p = blockIdx.z;
  const int key0 = blockIdx.x * QT + wave * 16;
  const int T = a.T;
  const TI* base = reinterpret_cast<const TI*>(a.qkv) + (int64_t)p * T * a.ld_qkv;
  const TI* Qb = base + a.q_off + h * HD;
  const TI* Kb = base + a.k_off + h * HD;
  const TI* Vb = base + a.v_off + h * HD;
  const TI* dOb = reinterpret_cast<const TI*>(a.dout) + (int64_t)p * T * a.ld_dout + h * HD;
  const float* lse = a.lse + ((int64_t)p * a.heads + h) * T;
  const float* dl = a.delta + ((int64_t)p * a.heads + h) * T;
  // this lane's key (lane i) bias
  const int mykey = key0 + i;
  const float kbias = mykey < T ? (a.key_bias ? a.key_bias[(int64_t)p * T + mykey] : 0.f) : NEG;

  // K, V fragments in registers (B operand with key on the lane: B[k=d][col=key])
  bf16x8_t kf[2], vf[2];
  float ks_[16], vs_[16];
  if constexpr (sizeof(TI) == 2) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kf[ks] = glob_row_frag((const unsigned short*)Kb, a.ld_qkv, mykey, T, ks, lane);
      vf[ks] = glob_row_frag((const unsigned short*)Vb, a.ld_qkv, mykey, T, ks, lane);
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      ks_[kk] = mykey < T ? ((const float*)Kb)[(int64_t)mykey * a.ld_qkv + kk * 4 + g] : 0.f;
      vs_[kk] = mykey < T ? ((const float*)Vb)[(int64_t)mykey * a.ld_qkv + kk * 4 + g] : 0.f;
    }
  }
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    dk[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
    dv[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const int nqt = (T + QT - 1) / QT;
  for (int qt = 0; qt < nqt; ++qt) {
    const int qb0 = qt * QT;
    stage_tile<TI>(sQ, Qb, a.ld_qkv, qb0, T, tid);
    stage_tile<TI>(sdO, dOb, a.ld_dout, qb0, T, tid);
    if (tid < QT) {
      int q = qb0 + tid;
      sL[tid] = q < T ? lse[q] : 1e30f;   // exp(s - 1e30) = 0 for padded queries
      sD[tid] = q < T ? dl[q] : 0.f;
    }
    __syncthreads();
    // S[q][key] and dP[q][key]: 4 query sub-tiles of 16 (rows 4g+r), key on the lane
    f32x4 s[4], dp[4];
#pragma unroll
    for (int qs = 0; qs < 4; ++qs) {
      s[qs] = (f32x4){0.f, 0.f, 0.f, 0.f};
      dp[qs] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if constexpr (sizeof(TI) == 2) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          s[qs] = mfma16<TI>(row_frag((const unsigned short*)sQ, qs * 16, ks, lane), kf[ks], s[qs]);
          dp[qs] = mfma16<TI>(row_frag((const unsigned short*)sdO, qs * 16, ks, lane), vf[ks], dp[qs]);
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
          s[qs] = __builtin_amdgcn_mfma_f32_16x16x4f32(((const float*)sQ)[(qs * 16 + i) * LD + kk * 4 + g],
                                                        ks_[kk], s[qs], 0, 0, 0);
          dp[qs] = __builtin_amdgcn_mfma_f32_16x16x4f32(((const float*)sdO)[(qs * 16 + i) * LD + kk * 4 + g],
                                                         vs_[kk], dp[qs], 0, 0, 0);
        }
      }
    }
    // P = exp(S*scale + bias - lse[q]);  dS = P * (dP - D[q])
#pragma unroll
    for (int qs = 0; qs < 4; ++qs)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int qi = qs * 16 + 4 * g + r;
        float pv = __expf(s[qs][r] * a.scale + kbias - sL[qi]);
        const float mul = drop_mul(a.drop, (((uint64_t)p * a.heads + h) * T + qb0 + qi) *
                                               (uint64_t)((T + 3) & ~3) + mykey);
        s[qs][r] = pv * mul;
        dp[qs][r] = pv * (dp[qs][r] * mul - sD[qi]);
      }
    // dV^T[d][key] += dO^T[d][q] P[q][key];  dK^T[d][key] += Q^T[d][q] dS[q][key]
    if constexpr (sizeof(TI) == 2) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_t pf = pack_pair(s[2 * ks], s[2 * ks + 1]);
        bf16x8_t dsf = pack_pair(dp[2 * ks], dp[2 * ks + 1]);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          dv[d] = mfma16<TI>(tr_frag((const unsigned short*)sdO, d * 16, ks, lane), pf, dv[d]);
          dk[d] = mfma16<TI>(tr_frag((const unsigned short*)sQ, d * 16, ks, lane), dsf, dk[d]);
        }
      }
    } else {
#pragma unroll
      for (int qs = 0; qs < 4; ++qs)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            int qi = qs * 16 + 4 * g + r;
            dv[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(((const float*)sdO)[qi * LD + d * 16 + i],
                                                          s[qs][r], dv[d], 0, 0, 0);
            dk[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(((const float*)sQ)[qi * LD + d * 16 + i],
                                                          dp[qs][r], dk[d], 0, 0, 0);
          }
    }
    __syncthreads();
  }
  if (mykey < T) {
    TI* dq = reinterpret_cast<TI*>(a.dqkv) + ((int64_t)p * T + mykey) * a.ld_dqkv;
    TI* dkp = dq + a.k_off + h * HD;
    TI* dvp = dq + a.v_off + h * HD;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        Elem<TI>::st(dkp + d * 16 + 4 * g + r, dk[d][r] * a.scale);
        Elem<TI>::st(dvp + d * 16 + 4 * g + r, dv[d][r]);
      }
  }
}

// ============================================================================================
// backward: dQ (per 64-query tile; each wave owns 16 queries; keys swept through LDS)
// ============================================================================================
template <typename TI>
__global__ __launch_bounds__(256) void attn_dq_kernel(AttnArgs a) {
  constexpr int LD = ACfg<TI>::LD;
  __shared__ __attribute__((aligned(16))) TI sK[QT * LD];
  __shared__ __attribute__((aligned(16))) TI sV[QT * LD];
  __shared__ float sBias[QT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int h = blockIdx.y, p = blockIdx.z;
  const int q0 = blockIdx.x * QT + wave * 16;
  const int T = a.T;
  const int myq = q0 + i;
  const TI* base = reinterpret_cast<const TI*>(a.qkv) + (int64_t)p * T * a.ld_qkv;
  const TI* Qb = base + a.q_off + h * HD;
  const TI* Kb = base + a.k_off + h * HD;
  const TI* Vb = base + a.v_off + h * HD;
  const TI* dOb = reinterpret_cast<const TI*>(a.dout) + (int64_t)p * T * a.ld_dout + h * HD;
  const float* kb_bias = a.key_bias ? a.key_bias + (int64_t)p * T : nullptr;
  const float L = myq < T ? a.lse[((int64_t)p * a.heads + h) * T + myq] : 1e30f;
  const float D = myq < T ? a.delta[((int64_t)p * a.heads + h) * T + myq] : 0.f;

  bf16x8_t qf[2], of[2];
  float qs_[16], os_[16];
  if constexpr (sizeof(TI) == 2) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[ks] = glob_row_frag((const unsigned short*)Qb, a.ld_qkv, myq, T, ks, lane);
      of[ks] = glob_row_frag((const unsigned short*)dOb, a.ld_dout, myq, T, ks, lane);
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      qs_[kk] = myq < T ? ((const float*)Qb)[(int64_t)myq * a.ld_qkv + kk * 4 + g] : 0.f;
      os_[kk] = myq < T ? ((const float*)dOb)[(int64_t)myq * a.ld_dout + kk * 4 + g] : 0.f;
    }
  }
  f32x4 dq[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) dq[d] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nkt = (T + QT - 1) / QT;
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * QT;
    stage_tile<TI>(sK, Kb, a.ld_qkv, k0, T, tid);
    stage_tile<TI>(sV, Vb, a.ld_qkv, k0, T, tid);
    if (tid < QT) {
      int key = k0 + tid;
      sBias[tid] = key < T ? (kb_bias ? kb_bias[key] : 0.f) : NEG;
    }
    __syncthreads();
    f32x4 s[4], dp[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      s[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
      dp[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if constexpr (sizeof(TI) == 2) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          s[kb] = mfma16<TI>(row_frag((const unsigned short*)sK, kb * 16, ks, lane), qf[ks], s[kb]);
          dp[kb] = mfma16<TI>(row_frag((const unsigned short*)sV, kb * 16, ks, lane), of[ks], dp[kb]);
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
          s[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(((const float*)sK)[(kb * 16 + i) * LD + kk * 4 + g],
                                                        qs_[kk], s[kb], 0, 0, 0);
          dp[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(((const float*)sV)[(kb * 16 + i) * LD + kk * 4 + g],
                                                         os_[kk], dp[kb], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pv = __expf(s[kb][r] * a.scale + sBias[kb * 16 + 4 * g + r] - L);
        const float mul =
            drop_mul(a.drop, (((uint64_t)p * a.heads + h) * T + myq) * (uint64_t)((T + 3) & ~3) + k0 +
                                 kb * 16 + 4 * g + r);
        dp[kb][r] = pv * (dp[kb][r] * mul - D);
      }
    if constexpr (sizeof(TI) == 2) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        bf16x8_t dsf = pack_pair(dp[2 * ks], dp[2 * ks + 1]);
#pragma unroll
        for (int d = 0; d < 4; ++d)
          dq[d] = mfma16<TI>(tr_frag((const unsigned short*)sK, d * 16, ks, lane), dsf, dq[d]);
      }
    } else {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int d = 0; d < 4; ++d)
            dq[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                ((const float*)sK)[(kb * 16 + 4 * g + r) * LD + d * 16 + i], dp[kb][r], dq[d], 0, 0, 0);
    }
    __syncthreads();
  }
  if (myq < T) {
    TI* dqp = reinterpret_cast<TI*>(a.dqkv) + ((int64_t)p * T + myq) * a.ld_dqkv + a.q_off + h * HD;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) Elem<TI>::st(dqp + d * 16 + 4 * g + r, dq[d][r] * a.scale);
  }
}


// ============================================================================================
// bf16 fast path (perf mode): 4 waves x 32 rows per workgroup (two 16-row groups per wave share
// every K/V (or Q/dO) fragment read), 64-row tiles of the swept operand double-buffered in LDS by
// LDS-DMA (one barrier per tile), exp2-domain softmax with the scale folded into one FMA.
// LDS images are [64 rows][64] bf16 (128-B rows) with 16-B chunk c of row r stored at
// c ^ (((r >> 1) & 3) << 1): conflict-free for BOTH the ds_read_b128 row-fragment reads
// (lane groups of the 16x16x32 operand) and the ds_read_b64_tr_b16 transposed reads, so one image
// serves S / dP (rows) and dV / dK / dQ (columns). The swizzle is applied to the DMA source.
// Dropout element index: ((p * heads + h) * T + q) * Tp4 + key, Tp4 = T rounded up to a multiple of
// 4, so the four keys 4g .. 4g + 3 of a lane are one hash quad (common.h) in the forward and dQ
// kernels.
// ============================================================================================
using mmseq_gemm_detail::rsrc_t;
using mmseq_gemm_detail::make_rsrc;
using mmseq_gemm_detail::dma16;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int IMG = 64 * 64;  // elements per [64][64] image

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// per-lane LDS-DMA source offset (bytes) of a 1 KB piece (8 rows x 128 B) for row stride ld
__device__ __forceinline__ uint32_t dma_lane_off(int lane, int64_t ld) {
  return (uint32_t)((lane >> 3) * ld * 2 + (((lane & 7) ^ (((lane >> 4) & 3) << 1)) << 4));
}
// row-fragment offset (elements) for rows rb..rb+15 (rb % 16 == 0): lane (g, i) -> row rb + i,
// chunk ks * 4 + g
__device__ __forceinline__ int row_off(int lane, int ks) {
  const int g = lane >> 4, i = lane & 15;
  return i * 64 + (((ks * 4 + g) ^ (((i >> 1) & 3) << 1)) << 3);
}
// transposed-fragment offset (elements) for output rows d*16..+15 (columns of the image) and
// k-rows 4g + q (+16 for the high half, + 32 ks): lane (g, i = 4q + p)
__device__ __forceinline__ int tr_off(int lane, int d) {
  const int g = lane >> 4, i = lane & 15, q = i >> 2, pp = i & 3;
  const int v = (2 * g + (q >> 1)) & 3;
  return (4 * g + q) * 64 + ((2 * (d ^ v) + (pp >> 1)) << 3) + (pp & 1) * 4;
}
__device__ __forceinline__ bf16x8_t lds_row(const unsigned short* img, int off) {
  return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8*>(img + off));
}
__device__ __forceinline__ bf16x8_t lds_tr(const unsigned short* img, int off) {
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MMSEQ_LDS s16x4*)(img + off));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MMSEQ_LDS s16x4*)(img + off + 16 * 64));
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
// Consume register loads before the tile loop: the compiler then places its vmcnt wait for them
// here, once, rather than at their first use inside the loop (where, since vmcnt retires in
// order, it would also wait out that iteration's in-flight K/V prefetch).
template <typename V>
__device__ __forceinline__ void settle(const V& v) { asm volatile("" ::"v"(v)); }
__device__ __forceinline__ f32x4 mma(const bf16x8_t& a, const bf16x8_t& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// max / sum over lanes l, l ^ 16, l ^ 32, l ^ 48 with the gfx950 row swaps (no ds_bpermute, no
// lane index arithmetic): permlane16_swap pairs rows (0,1), (2,3); permlane32_swap the two halves
__device__ __forceinline__ float xlane_max4(float v) {
  const uint32_t u = __float_as_uint(v);
  const auto r16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const float m = fmaxf(__uint_as_float(r16[0]), __uint_as_float(r16[1]));
  const uint32_t w = __float_as_uint(m);
  const auto r32 = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return fmaxf(__uint_as_float(r32[0]), __uint_as_float(r32[1]));
}
__device__ __forceinline__ float xlane_sum4(float v) {
  const uint32_t u = __float_as_uint(v);
  const auto r16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const float m = __uint_as_float(r16[0]) + __uint_as_float(r16[1]);
  const uint32_t w = __float_as_uint(m);
  const auto r32 = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return __uint_as_float(r32[0]) + __uint_as_float(r32[1]);
}

// MX-fp8 copy of one head's 64 gradient columns of a row of dQ|dK|dV (the backward's Q8 output for
// config 5's fp8 QKV dgrad): v4[d][r] * mul is column col0 + 16 d + 4 g + r; 32-column block b holds
// d = 2b, 2b + 1 of the four lanes g of the row, quantised like mmseq_quant_mxfp8 of the bf16 values
// (the layout of the packed [rows][3 * heads * 64] operand; padding-row scales zeroed by the host)
__device__ __forceinline__ void q8_head_row(const AttnArgs& a, int64_t row, int col0, const f32x4* v4,
                                            float mul, int g) {
  const int KB = 6 * a.heads;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    float v[8], amax = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] = bf2f(f2bf(v4[2 * b + (e >> 2)][e & 3] * mul));
      amax = fmaxf(amax, fabsf(v[e]));
    }
    amax = xlane_max4(amax);
    int ex = amax > 0.f ? (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 : -127;
    ex = max(-127, min(127, ex - 8));
    const float sc = ldexpf(1.f, -ex);
    if (g == 0)
      a.q8s[((row >> 6) * KB + (col0 >> 5) + b) * 64 + (row & 15) * 4 + ((row >> 4) & 3)] = (uint8_t)(ex + 127);
#pragma unroll
    for (int dd = 0; dd < 2; ++dd) {
      const float s0 = fminf(448.f, fmaxf(-448.f, v[4 * dd] * sc));
      const float s1 = fminf(448.f, fmaxf(-448.f, v[4 * dd + 1] * sc));
      const float s2 = fminf(448.f, fmaxf(-448.f, v[4 * dd + 2] * sc));
      const float s3 = fminf(448.f, fmaxf(-448.f, v[4 * dd + 3] * sc));
      int pk = __builtin_amdgcn_cvt_pk_fp8_f32(s0, s1, 0, false);
      pk = __builtin_amdgcn_cvt_pk_fp8_f32(s2, s3, pk, true);
      *reinterpret_cast<int*>(a.q8 + row * a.ldq8 + col0 + (2 * b + dd) * 16 + 4 * g) = pk;
    }
  }
}
// A operand of all-ones (bf16 1.0): mma(ONES, P, acc) adds each query column's sum of P to all
// four of its accumulator rows
__device__ __forceinline__ bf16x8_t bf16_ones() {
  const u16x8 v = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
  return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ rsrc_t head_rsrc(const void* base, int64_t row0, int64_t ld, int64_t col,
                                            int T) {
  const unsigned short* b = reinterpret_cast<const unsigned short*>(base) + row0 * ld + col;
  return make_rsrc(b, ((int64_t)(T - 1) * ld + 64) * 2);
}

// Prologue loads through buffer descriptors: rows / indices past the descriptor's range read as
// zero without a branch, so the compiler issues every prologue load straight-line and waits once
// (a bounds branch around a load gets its own wait at the branch's first use)
__device__ __forceinline__ bf16x8_t buf_row_frag(rsrc_t r, int row, int64_t ld, int ks, int lane) {
  typedef unsigned int u32x4b __attribute__((ext_vector_type(4)));
  const uint32_t off = (uint32_t)(((int64_t)row * ld + ks * 32 + (lane >> 4) * 8) * 2);
  return __builtin_bit_cast(bf16x8_t, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}
__device__ __forceinline__ float buf_f32(rsrc_t r, int idx) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (uint32_t)idx * 4u, 0, 0));
}

// 1-D grid over (row block, head, pair) with an XCD-aware order: the blocks that share one
// (pair, head) K/V (or Q/dO) slice get consecutive work indices on ONE XCD (blocks b, b+8, ...
// share an XCD under round-robin dispatch), so the slice is fetched into that XCD's L2 once.
struct BlkIdx { int x, h, p; };
__device__ __forceinline__ BlkIdx attn_block(int nx, int heads) {
  const int nb = gridDim.x, b = blockIdx.x;
  const int q8 = nb >> 3, r8 = nb & 7, xcd = b & 7;
  const int w = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (b >> 3);
  BlkIdx r;
  r.x = w % nx;
  const int rest = w / nx;
  r.h = rest % heads;
  r.p = rest / heads;
  return r;
}

// ---- forward ---------------------------------------------------------------------------------
// keep bits of a packed bf16 pair from one dropout hash word: half u of word x is kept iff
// u >= thr (as drop_sel). Packed 16-bit ops, no compares: s = sat(u - (thr - 1)) is >= 1 exactly
// when kept, k = min(s, 1) is the keep bit of each half (inline asm: the compiler turns the
// elementwise form back into two compares and four selects)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t keep_bits2(uint32_t x, uint32_t thr1x2, uint32_t ones) {
  uint32_t t, k;
  asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(t) : "v"(x), "s"(thr1x2));
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(k) : "v"(t), "v"(ones));
  return k;
}
// a packed bf16 pair with its dropped halves zeroed: each 16-bit half times its keep bit (0 or 1),
// one v_pk_mul_lo_u16 instead of the AND with the mask 0 - k (bit-identical)
__device__ __forceinline__ uint32_t keep_apply2(uint32_t w, uint32_t k) {
  uint32_t r;
  asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(r) : "v"(w), "v"(k));
  return r;
}
__device__ __forceinline__ uint32_t opaque_u32(uint32_t x) {  // a value the compiler cannot
  asm("v_mov_b32 %0, %1" : "=v"(x) : "v"(x));                  // rematerialise inside the loop
  return x;
}
__device__ __forceinline__ uint32_t hash_mixed(uint32_t x) {  // drop_mix with the final xor-shift
  x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu;       // (whose halves drop_sel compares) last
  return x ^ (x >> 16);
}

// Forward tail block: the last query block of a (pair, head) when it holds 1-16 rows (T % 128 in
// [1, 16]: T = 513 leaves 1, the ViT's T = 393 leaves 9). Those rows are one 16-row MFMA group, and
// one wave sweeping all T keys for them kept the whole workgroup slot for as long as a full block
// while three of its waves idled. Here the four waves split the keys instead: 32-key chunk c goes
// to wave c % 4, which stages it by LDS-DMA into its own 8 KB of the K / V ring (K rows at +0, V at
// +4 KB: the first 32 rows of the 64-key image layout, so the fragment offsets are the main loop's)
// and runs the same online softmax / dropout / P V on it. The four partial (m, l, O) then merge in
// wave order through LDS (exact for any reference m: O and l are relative to their own m).
// Per score the arithmetic is the main loop's (same scale, bias, hash index, keep decision); only
// the order of the key-chunk sums differs.
template <int DMODE, bool WIDE, bool Q8>
__device__ __forceinline__ void attn_fwd_tail(const AttnArgs& a, unsigned short* smem, int p, int h,
                                              int q0) {
  constexpr bool DROP = DMODE != 0;
  float* sBias = reinterpret_cast<float*>(smem + 4 * IMG);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i = lane & 15;
  const int T = a.T;
  const int nkt = (T + 63) >> 6, nch = (T + 31) >> 5;
  const int64_t ld = a.ld_qkv;
  const rsrc_t rk = head_rsrc(a.qkv, (int64_t)p * T, ld, a.k_off + h * 64, T);
  const rsrc_t rv = head_rsrc(a.qkv, (int64_t)p * T, ld, a.v_off + h * 64, T);
  const uint32_t loff = dma_lane_off(lane, ld);
  unsigned short* kimg = smem + wave * 4096;  // this wave's 8 KB: K rows 0-31, then V rows 0-31
  unsigned short* vimg = kimg + 2048;
  auto stage = [&](int c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t vo = loff + (uint32_t)((int64_t)(c * 32 + e * 8) * ld * 2);
      dma16(rk, kimg + e * 512, vo);
      dma16(rv, vimg + e * 512, vo);
    }
  };
  if (wave < nch) stage(wave);
  const float* kbias = a.key_bias ? a.key_bias + (int64_t)p * T : nullptr;
  int* sZero = reinterpret_cast<int*>(sBias + nkt * 64);
  const rsrc_t rkb = make_rsrc(kbias, kbias ? (int64_t)T * 4 : 0);
  for (int tt = wave; tt < nkt; tt += 4) {
    const int k = tt * 64 + lane;
    const float bv = k < T ? buf_f32(rkb, k) * LOG2E : -1e30f;
    sBias[k] = bv;
    const bool z = __ballot(bv != 0.f) == 0;
    if (lane == 0) sZero[tt] = z;
  }
  const rsrc_t rq = head_rsrc(a.qkv, (int64_t)p * T, ld, a.q_off + h * 64, T);
  bf16x8_t qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) qf[ks] = buf_row_frag(rq, q0 + i, ld, ks, lane);
  const rsrc_t rbits = DMODE == 2 ? make_rsrc(a.bits + ((int64_t)p * a.heads + h) * T * a.nkt2,
                                              (int64_t)T * a.nkt2 * 8)
                                  : make_rsrc(a.qkv, 0);
  const uint32_t boff0 = (uint32_t)(((q0 + i) * a.nkt2 * 4 + g) * 2);
  const int ro0 = row_off(lane, 0), ro1 = row_off(lane, 1);
  int to[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) to[d] = tr_off(lane, d);
  const float c = a.scale * LOG2E;
  const uint64_t drow = (((uint64_t)p * a.heads + h) * T + (q0 + i)) * (uint64_t)((T + 3) & ~3);
  const uint32_t prow = opaque_u32((uint32_t)(drow >> 2) + g);
  const uint32_t thr1x2 = (a.drop.thr - 1) * 0x10001u, ones2 = opaque_u32(0x10001u);
  const bf16x8_t ones = bf16_ones();
  f32x4 o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) o[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m = -1e30f;
  f32x4 lsum = (f32x4){0.f, 0.f, 0.f, 0.f};
  __syncthreads();  // key bias of every tile in LDS
  for (int ch = wave; ch < nch; ch += 4) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's chunk landed (its own DMA)
    const int t = ch >> 1, half = ch & 1;
    const int nkb = min(2, (T - ch * 32 + 15) >> 4);  // 16-key blocks holding a valid key
    f32x4 s[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      if (kk < nkb) {
        const bf16x8_t k0 = lds_row(kimg, kk * 1024 + ro0), k1 = lds_row(kimg, kk * 1024 + ro1);
        s[kk] = mma(k1, qf[1], mma(k0, qf[0], (f32x4){0.f, 0.f, 0.f, 0.f}));
      } else {
        s[kk] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
    const bool zb = __builtin_amdgcn_readfirstlane(sZero[t]) != 0;
    float mx = -1e30f;
    if (zb) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kk][r]);
      mx *= c;
    } else {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (kk >= nkb) continue;
        const f32x4 b = *reinterpret_cast<const f32x4*>(sBias + t * 64 + (2 * half + kk) * 16 + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float x = fmaf(s[kk][r], c, b[r]);
          s[kk][r] = x;
          mx = fmaxf(mx, x);
        }
      }
    }
    if (__ballot(mx > m + 8.f) != 0) {
      const float mn = fmaxf(m, xlane_max4(mx));
      const float alpha = ex2(m - mn);
      m = mn;
      lsum *= alpha;
#pragma unroll
      for (int d = 0; d < 4; ++d) o[d] *= alpha;
    }
    if (zb) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kk][r] = ex2(fmaf(s[kk][r], c, -m));
    } else {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (kk >= nkb) {
          s[kk] = (f32x4){0.f, 0.f, 0.f, 0.f};
          continue;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) s[kk][r] = ex2(s[kk][r] - m);
      }
    }
    bf16x8_t pf = pack_pair(s[0], s[1]);
    lsum = mma(ones, pf, lsum);
    if (DROP) {  // as the main loop: dword j = 2 kk + q2 of pf is kb = 2 half + kk of tile t
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      u32x4 w = __builtin_bit_cast(u32x4, pf);
      uint32_t acc = 0;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (kk >= nkb) continue;
        const int kb = 2 * half + kk;
        uint32_t hq;
        if (WIDE) {
          hq = drop_hash(a.drop, (drow + t * 64 + kb * 16 + 4 * g) >> 2);
        } else {
          const uint32_t x = ((prow + (uint32_t)(t * 16 + kb * 4)) ^ a.drop.k0) + a.drop.k1;
          hq = hash_mixed(x ^ (x >> 16));
        }
#pragma unroll
        for (int q2 = 0; q2 < 2; ++q2) {
          const uint32_t hx = q2 ? drop_hash2(hq) : hq;
          const uint32_t k = keep_bits2(hx, thr1x2, ones2);
          w[2 * kk + q2] = keep_apply2(w[2 * kk + q2], k);
          if (DMODE == 2) acc |= k << (2 * (2 * kb + q2));
        }
      }
      pf = __builtin_bit_cast(bf16x8_t, w);
      if (DMODE == 2) {  // byte `half` of the row's 16-bit slice g of tile t (the other byte is
                         // the other chunk's, written by another wave)
        const uint32_t kb16 = (acc & 0x5555u) | ((acc >> 15) & 0xAAAAu);
        __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(kb16 >> (8 * half)), rbits,
                                             boff0 + t * 8 + half, 0, 0);
      }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = mma(lds_tr(vimg, to[d]), pf, o[d]);
    if (ch + 4 < nch) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this chunk's LDS reads done
      stage(ch + 4);
    }
  }
  // merge: wave w's (m, l, O) for its lane at float [w][lane][0..17] of the K / V ring
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();  // every wave's LDS reads (and DMA) done before the ring is overwritten
  float* sM = reinterpret_cast<float*>(smem);
  float* mine = sM + (wave * 64 + lane) * 18;
  mine[0] = m;
  mine[1] = lsum[0];
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int r = 0; r < 4; ++r) mine[2 + 4 * d + r] = o[d][r];
  __syncthreads();
  if (wave != 0) return;
  float mw[4], M = -1e30f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    mw[w] = sM[(w * 64 + lane) * 18];
    M = fmaxf(M, mw[w]);
  }
  float L = 0.f;
  f32x4 O[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) O[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float* src = sM + (w * 64 + lane) * 18;
    const float sc = ex2(mw[w] - M);
    L = fmaf(src[1], sc, L);
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int r = 0; r < 4; ++r) O[d][r] = fmaf(src[2 + 4 * d + r], sc, O[d][r]);
  }
  const int q = q0 + i;
  if (q < a.Tq) {
    const float inv = (DROP ? a.drop.scale : 1.0f) / L;
    if (Q8) {  // as the main loop's MX-fp8 output (and the training forward's bf16 copy)
      const int64_t row = (int64_t)p * a.Tq + q;
      const int KB = a.heads * 2;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        float v[8], amax = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = bf2f(f2bf(O[2 * b + (e >> 2)][e & 3] * inv));
          amax = fmaxf(amax, fabsf(v[e]));
        }
        amax = xlane_max4(amax);
        int ex = amax > 0.f ? (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 : -127;
        ex = max(-127, min(127, ex - 8));
        const float sc = ldexpf(1.f, -ex);
        if (g == 0)
          a.q8s[((row >> 6) * KB + h * 2 + b) * 64 + (row & 15) * 4 + ((row >> 4) & 3)] = (uint8_t)(ex + 127);
#pragma unroll
        for (int dd = 0; dd < 2; ++dd) {
          const float s0 = fminf(448.f, fmaxf(-448.f, v[4 * dd] * sc));
          const float s1 = fminf(448.f, fmaxf(-448.f, v[4 * dd + 1] * sc));
          const float s2 = fminf(448.f, fmaxf(-448.f, v[4 * dd + 2] * sc));
          const float s3 = fminf(448.f, fmaxf(-448.f, v[4 * dd + 3] * sc));
          int pk = __builtin_amdgcn_cvt_pk_fp8_f32(s0, s1, 0, false);
          pk = __builtin_amdgcn_cvt_pk_fp8_f32(s2, s3, pk, true);
          *reinterpret_cast<int*>(a.q8 + row * a.ldq8 + h * 64 + (2 * b + dd) * 16 + 4 * g) = pk;
        }
        if (a.o_w) {
          unsigned short* op = reinterpret_cast<unsigned short*>(a.o_w) + row * a.ld_out + h * 64 + 4 * g;
#pragma unroll
          for (int dd = 0; dd < 2; ++dd) {
            typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;
            *reinterpret_cast<u16x4*>(op + (2 * b + dd) * 16) =
                (u16x4){f2bf(v[4 * dd]), f2bf(v[4 * dd + 1]), f2bf(v[4 * dd + 2]), f2bf(v[4 * dd + 3])};
          }
        }
      }
    } else {
      unsigned short* op = reinterpret_cast<unsigned short*>(a.o_w) + ((int64_t)p * a.Tq + q) * a.ld_out +
                           h * 64 + 4 * g;
#pragma unroll
      for (int d = 0; d < 4; ++d) Vec4<unsigned short>::st(op + d * 16, O[d] * inv);
    }
    if (g == 0) a.lse[((int64_t)p * a.heads + h) * T + q] = (M + __builtin_amdgcn_logf(L)) * LN2;
  }
}

template <int DMODE, bool WIDE, bool Q8 = false>  // dropout: 0 none, 1 counter hash, 2 counter
                                 // hash + keep bits out; WIDE: dropout pair indices >= 2^32 (64-bit
                                 // index arithmetic); Q8: MX-fp8 output (eval, the O-proj operand)
// (four workgroups per CU everywhere but the 64-bit-index dropout forms: <= 128 VGPRs since the
// forward has no per-tile row max and keeps scalar row sums, so the lane-derived LDS and DMA offsets
// are held across the loop rather than recomputed per tile: T = 393 forward -9 %)
__global__ __launch_bounds__(256, DMODE != 0 && WIDE ? 3 : 4) void attn_fwd_bf16_kernel(AttnArgs a) {
  constexpr bool DROP = DMODE != 0;
  extern __shared__ __attribute__((aligned(16))) unsigned short smem[];  // 2 x (K, V) + bias
  float* sBias = reinterpret_cast<float*>(smem + 4 * IMG);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i = lane & 15;
  const int T = a.T;
  const BlkIdx bi = attn_block((a.Tq + 127) >> 7, a.heads);
  const int h = bi.h, p = bi.p;
  // the last 1-16 rows of T (bit-identical whether or not the launch covers only Tq < T rows)
  if (((T - 1) & 127) < 16 && bi.x == (T - 1) >> 7) {
    attn_fwd_tail<DMODE, WIDE, Q8>(a, smem, p, h, bi.x * 128);
    return;
  }
  const int nkt = (T + 63) >> 6;
  const int qw = bi.x * 128 + wave * 32;
  const bool active = qw < a.Tq;
  const int64_t ld = a.ld_qkv;
  const rsrc_t rk = head_rsrc(a.qkv, (int64_t)p * T, ld, a.k_off + h * 64, T);
  const rsrc_t rv = head_rsrc(a.qkv, (int64_t)p * T, ld, a.v_off + h * 64, T);
  const uint32_t loff = dma_lane_off(lane, ld);
  // keep-bit slices (DMODE 2): ushort g of word [q][t] of this (p, h), byte offset from its base
  const rsrc_t rbits = DMODE == 2 ? make_rsrc(a.bits + ((int64_t)p * a.heads + h) * T * a.nkt2,
                                              (int64_t)T * a.nkt2 * 8)
                                  : make_rsrc(a.qkv, 0);
  const uint32_t boff0 = (uint32_t)(((qw + i) * a.nkt2 * 4 + g) * 2);
  auto stage = [&](int t) {
    unsigned short* kimg = smem + (t & 1) * 2 * IMG;
    uint32_t lo = loff;  // a copy by value: reading the capture in the loop compiles to other scalar code
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int pc = wave * 2 + e;
      const uint32_t vo = lo + (uint32_t)((int64_t)(t * 64 + pc * 8) * ld * 2);
      dma16(rk, kimg + pc * 512, vo);
      dma16(rv, kimg + IMG + pc * 512, vo);
    }
  };
  stage(0);
  // the prologue's global loads (this wave's key-bias tiles for T <= 1024, the Q fragments) are
  // all issued before the first is consumed: one memory round trip beside tile 0's DMA
  const float* kbias = a.key_bias ? a.key_bias + (int64_t)p * T : nullptr;
  int* sZero = reinterpret_cast<int*>(sBias + nkt * 64);  // tile t's key bias is all zero
  const rsrc_t rkb = make_rsrc(kbias, kbias ? (int64_t)T * 4 : 0);
  float kbv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) kbv[j] = buf_f32(rkb, (wave + 4 * j) * 64 + lane);
  const rsrc_t rq = head_rsrc(a.qkv, (int64_t)p * T, ld, a.q_off + h * 64, T);
  bf16x8_t qf[2][2];
#pragma unroll
  for (int grp = 0; grp < 2; ++grp)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[grp][ks] = buf_row_frag(rq, qw + grp * 16 + i, ld, ks, lane);
  auto put_bias = [&](int tt, float raw) {
    const int k = tt * 64 + lane;
    const float bv = k < T ? raw * LOG2E : -1e30f;
    sBias[k] = bv;
    const bool z = __ballot(bv != 0.f) == 0;
    if (lane == 0) sZero[tt] = z;
  };
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (wave + 4 * j < nkt) put_bias(wave + 4 * j, kbv[j]);
  for (int tt = wave + 16; tt < nkt; tt += 4) put_bias(tt, buf_f32(rkb, tt * 64 + lane));
#pragma unroll
  for (int grp = 0; grp < 2; ++grp)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) settle(qf[grp][ks]);

  const float c = a.scale * LOG2E;
  const int Tp4 = (T + 3) & ~3;
  uint64_t drow[2];
  uint32_t prow[2];  // narrow quad index of (row, key 4g) in tile 0
#pragma unroll
  for (int grp = 0; grp < 2; ++grp) {
    drow[grp] = (((uint64_t)p * a.heads + h) * T + (qw + grp * 16 + i)) * Tp4;
    prow[grp] = opaque_u32((uint32_t)(drow[grp] >> 2) + g);
  }
  const uint32_t thr1x2 = (a.drop.thr - 1) * 0x10001u, ones2 = opaque_u32(0x10001u);

  f32x4 o[2][4];
  float m[2] = {-1e30f, -1e30f};
  float lsum[2] = {0.f, 0.f};  // row sums (a lane's four accumulator rows of a tile sum are equal)
  const bf16x8_t ones = bf16_ones();
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int grp = 0; grp < 2; ++grp)
#pragma unroll
    for (int d = 0; d < 4; ++d) o[grp][d] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // One key tile of this wave's rows. FULL: all four 16-key blocks valid (every tile but the last).
  // maxpath false: the fast exponentials of the comment below, refused (returns false, nothing
  // written) when a row's tile sum exceeds 2^8.
  auto tile = [&](const int t, auto fullc, const bool maxpath) -> bool {
    constexpr bool FULL = decltype(fullc)::value;
    const unsigned short* kimg = smem + (t & 1) * 2 * IMG;
    const unsigned short* vimg = kimg + IMG;
    const int ro0 = row_off(lane, 0), ro1 = row_off(lane, 1);
    int to[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) to[d] = tr_off(lane, d);
    // 16-key blocks holding a valid key (the last tile of T = 64n + 1 has one): the others are
    // all masked (p = 0), so their MFMAs and softmax work are skipped
    const int nkb = FULL ? 4 : min(4, (T - t * 64 + 15) >> 4);
    // all-zero key bias in this tile (the usual case: ViT, and every visual-key tile of the joint
    // encoder): the scale folds into the exponent's FMA, no per-score bias add
    const bool zb = __builtin_amdgcn_readfirstlane(sZero[t]) != 0;
    bf16x8_t pf[2][2];
    // The first tile runs the max path. Later tiles first take the exponentials against the
    // running max as it stands and keep them when no row's sum over the tile, rounded to bf16,
    // exceeds 2^8: that bounds every P of the tile at 2^8 (up to that rounding), which the
    // accumulators take without rescaling, so the result matches the max path's up to rounding
    // (not bit for bit: the max path may move m where this keeps it). Otherwise the wave runs the
    // tile again by the max path (redo), its scores recomputed from the K tile still in LDS
    // (holding them across the attempt would spill). Saves the per-tile row max (16 max, a scale
    // and a vote per 16-row group).
    {
      f32x4 s[2][4];
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        if (kb < nkb) {
          const bf16x8_t k0 = lds_row(kimg, kb * 1024 + ro0), k1 = lds_row(kimg, kb * 1024 + ro1);
#pragma unroll
          for (int grp = 0; grp < 2; ++grp) {
            s[grp][kb] = mma(k0, qf[grp][0], (f32x4){0.f, 0.f, 0.f, 0.f});
            s[grp][kb] = mma(k1, qf[grp][1], s[grp][kb]);
          }
        } else {
#pragma unroll
          for (int grp = 0; grp < 2; ++grp) s[grp][kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
      }
      float ts[2];
#pragma unroll
      for (int grp = 0; grp < 2; ++grp) {
        if (!zb) {
#pragma unroll
          for (int kb = 0; kb < 4; ++kb) {
            if (kb >= nkb) continue;
            const f32x4 b = *reinterpret_cast<const f32x4*>(sBias + t * 64 + kb * 16 + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) s[grp][kb][r] = fmaf(s[grp][kb][r], c, b[r]);
          }
        }
        if (maxpath) {
          float mx = -1e30f;
#pragma unroll
          for (int kb = 0; kb < 4; ++kb) {
            if (!zb && kb >= nkb) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[grp][kb][r]);
          }
          if (zb) mx *= c;  // c > 0
          // lazy rescaling: the running max only moves (and O, l are rescaled) when some row's
          // tile max exceeds it by more than 8 (log2 units), so unrescaled probabilities stay
          // <= 2^8; O / l and the LSE m + log2(l) are exact for any reference m. The four lanes
          // of a row share m, so the vote over each lane's partial max decides the same as over
          // the row max, and the cross-lane reduction runs only when a row's max moves
          if (__ballot(mx > m[grp] + 8.f) != 0) {
            const float mn = fmaxf(m[grp], xlane_max4(mx));
            const float alpha = ex2(m[grp] - mn);
            m[grp] = mn;
            lsum[grp] *= alpha;
#pragma unroll
            for (int d = 0; d < 4; ++d) o[grp][d] *= alpha;
          }
        }
        const float mn = m[grp];
        if (zb) {
          const float nm = -mn;
#pragma unroll
          for (int kb = 0; kb < 4; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[grp][kb][r] = ex2(fmaf(s[grp][kb][r], c, nm));
        } else {
#pragma unroll
          for (int kb = 0; kb < 4; ++kb) {
            if (kb >= nkb) {
              s[grp][kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
              continue;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) s[grp][kb][r] = ex2(s[grp][kb][r] - mn);
          }
        }
        pf[grp][0] = pack_pair(s[grp][0], s[grp][1]);
        pf[grp][1] = pack_pair(s[grp][2], s[grp][3]);
        // row sums of the bf16 P (undropped: dropout acts after the softmax normalisation) by MFMA
        f32x4 ta = mma(ones, pf[grp][0], zero4);
        if (nkb > 2) ta = mma(ones, pf[grp][1], ta);
        ts[grp] = ta[0];
      }
      if (!maxpath && __ballot(ts[0] > 256.f || ts[1] > 256.f) != 0) {
        return false;
      }
      lsum[0] += ts[0];
      lsum[1] += ts[1];
    }
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {
      if (DROP) {  // dropped scores are zeroed in the packed P (one multiply per pair of keys), the
                   // 1/(1-p) of the kept ones is applied with the final normalisation.
                   // dword j = 2 kb + q2 of the packed P holds keys 16 kb + 4g + 2 q2 + {0, 1}: the
                   // two halves of hash word q2 of the keys' quad (h, then h2), keep bits 2j and
                   // 2j + 1 of the row's 16-bit slice
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        u32x4 w[2] = {__builtin_bit_cast(u32x4, pf[grp][0]), __builtin_bit_cast(u32x4, pf[grp][1])};
        uint32_t acc = 0;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
          if (kb >= nkb) continue;  // all keys >= T: p = 0, keep bits never read
          uint32_t hq;
          if (WIDE) {
            hq = drop_hash(a.drop, (drow[grp] + t * 64 + kb * 16 + 4 * g) >> 2);
          } else {  // drop_hash with the quad index < 2^32 (its high word 0)
            const uint32_t x = ((prow[grp] + (uint32_t)(t * 16 + kb * 4)) ^ a.drop.k0) + a.drop.k1;
            hq = hash_mixed(x ^ (x >> 16));
          }
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) {
            const uint32_t hx = q2 ? drop_hash2(hq) : hq;
            const uint32_t k = keep_bits2(hx, thr1x2, ones2);
            const int j = 2 * kb + q2;
            w[kb >> 1][j & 3] = keep_apply2(w[kb >> 1][j & 3], k);
            if (DMODE == 2) acc |= k << (2 * j);
          }
        }
        pf[grp][0] = __builtin_bit_cast(bf16x8_t, w[0]);
        pf[grp][1] = __builtin_bit_cast(bf16x8_t, w[1]);
        if (DMODE == 2) {  // bits 2j (low halves) and 16 + 2j (high halves) -> 2j and 2j + 1
          const uint32_t kb16 = (acc & 0x5555u) | ((acc >> 15) & 0xAAAAu);
          // rows q >= T fall outside the descriptor and are dropped
          __builtin_amdgcn_raw_buffer_store_b16((unsigned short)kb16, rbits,
                                                boff0 + grp * 16 * a.nkt2 * 8 + t * 8, 0, 0);
        }
      }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const bf16x8_t v0 = lds_tr(vimg, to[d]), v1 = lds_tr(vimg, 32 * 64 + to[d]);
#pragma unroll
      for (int grp = 0; grp < 2; ++grp) {
        o[grp][d] = mma(v0, pf[grp][0], o[grp][d]);
        if (nkb > 2) o[grp][d] = mma(v1, pf[grp][1], o[grp][d]);
      }
    }
    return true;
  };
  // redo: this wave runs tile t again by the max path (its fast exponentials were refused); the
  // repeat skips the barrier and the staging, so every wave still meets one barrier per tile
  bool redo = false;
  for (int t = 0; t < nkt - 1;) {
    if (!redo) {
      // vmcnt retires in issue order: an active wave's two keep-bit stores of tile t - 1 are newer
      // than tile t's DMA, so waiting down to 2 covers the DMA without waiting for the store acks
      // (a raw s_barrier: __syncthreads' fence would add a vmcnt(0) for the stores)
      if (DMODE == 2 && active && t > 0)
        asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      // tile t landed everywhere; buffer (t + 1) & 1 no longer read
      stage(t + 1);
    }
    if (active && !tile(t, std::true_type{}, t == 0 || redo)) {
      redo = true;
      continue;
    }
    redo = false;
    ++t;
  }
  // the last tile (its valid 16-key blocks only), by the max path
  if (DMODE == 2 && active && nkt > 1)
    asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  else
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if (active) tile(nkt - 1, std::false_type{}, true);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (!active) return;
#pragma unroll
  for (int grp = 0; grp < 2; ++grp) {
    const float lt = lsum[grp];
    const int q = qw + grp * 16 + i;
    if (q < a.Tq) {
      const float inv = (DROP ? a.drop.scale : 1.0f) / lt;
      if (Q8) {  // MX-fp8 of the bf16-rounded output (bit-identical to bf16 out + mmseq_quant_mxfp8):
                 // block b of the head's 64 columns = d 2b, 2b+1 of the four lanes g of query i
        const int64_t row = (int64_t)p * a.Tq + q;
        const int KB = a.heads * 2;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          float v[8], amax = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            v[e] = bf2f(f2bf(o[grp][2 * b + (e >> 2)][e & 3] * inv));
            amax = fmaxf(amax, fabsf(v[e]));
          }
          amax = xlane_max4(amax);
          int ex = amax > 0.f ? (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 : -127;
          ex = max(-127, min(127, ex - 8));
          const float sc = ldexpf(1.f, -ex);
          if (g == 0)
            a.q8s[((row >> 6) * KB + h * 2 + b) * 64 + (row & 15) * 4 + ((row >> 4) & 3)] = (uint8_t)(ex + 127);
#pragma unroll
          for (int dd = 0; dd < 2; ++dd) {
            const float s0 = fminf(448.f, fmaxf(-448.f, v[4 * dd] * sc));
            const float s1 = fminf(448.f, fmaxf(-448.f, v[4 * dd + 1] * sc));
            const float s2 = fminf(448.f, fmaxf(-448.f, v[4 * dd + 2] * sc));
            const float s3 = fminf(448.f, fmaxf(-448.f, v[4 * dd + 3] * sc));
            int pk = __builtin_amdgcn_cvt_pk_fp8_f32(s0, s1, 0, false);
            pk = __builtin_amdgcn_cvt_pk_fp8_f32(s2, s3, pk, true);
            *reinterpret_cast<int*>(a.q8 + row * a.ldq8 + h * 64 + (2 * b + dd) * 16 + 4 * g) = pk;
          }
          if (a.o_w) {  // training: the bf16 output too (the backward's O), the same rounded values
            unsigned short* op = reinterpret_cast<unsigned short*>(a.o_w) + row * a.ld_out + h * 64 + 4 * g;
#pragma unroll
            for (int dd = 0; dd < 2; ++dd) {
              typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;
              *reinterpret_cast<u16x4*>(op + (2 * b + dd) * 16) =
                  (u16x4){f2bf(v[4 * dd]), f2bf(v[4 * dd + 1]), f2bf(v[4 * dd + 2]), f2bf(v[4 * dd + 3])};
            }
          }
        }
      } else {
        unsigned short* op = reinterpret_cast<unsigned short*>(a.o_w) + ((int64_t)p * a.Tq + q) * a.ld_out +
                             h * 64 + 4 * g;
#pragma unroll
        for (int d = 0; d < 4; ++d) Vec4<unsigned short>::st(op + d * 16, o[grp][d] * inv);
      }
      if (g == 0) a.lse[((int64_t)p * a.heads + h) * T + q] = (m[grp] + __builtin_amdgcn_logf(lt)) * LN2;
    }
  }
}

// ---- forward, 32x32x16 MFMA (variant 2) ------------------------------------------------------
// Workgroup = 2 waves = 128 query rows of one (pair, head); a wave owns 64 rows = two 32-row
// q-blocks that share every K / V fragment read (LDS traffic per MFMA half of the 16x16 kernel,
// and the 32-cycle MFMA leaves 24 issue cycles of VALU beside it instead of 8).
//  S^T = K Q^T per 32-key block: A = K rows (ds_read_b128), B = Q^T (registers for the whole
//  sweep). The accumulator has the query on the lane (l & 31) and 16 of the block's keys in its
//  registers (key (j & 3) + 8 (j >> 2) + 4 (l >> 5) for register j), so the online softmax is
//  in-lane; the two lane halves hold disjoint keys of the same query and only meet when the
//  running max moves (lazy rescale, threshold 8 in log2 units) and at the end (row sum).
//  P^T is the bf16-packed accumulator itself: registers 8s'..8s'+7 are the B operand of k-step s'
//  of O^T = V^T P^T (guide §3 'An accumulator tile as the next MFMA's operand'); the A operand
//  V^T is read by ds_read_b64_tr_b16 in that permuted key order.
// LDS image per tile and operand: [64 keys][64 dims] bf16, 128-B rows, 16-B chunk c of row r at
// c ^ g((r >> 1) & 7), g(x) = ((x & 1) << 2) | (x >> 1): the b128 K-row reads (16-lane groups of
// 16 distinct rows) and the transposed V reads (rows r and r + 2 in different 64-B halves) are
// both conflict-free. The swizzle is applied to the LDS-DMA source.
typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ uint32_t sign_mask(uint32_t x) {  // x >> 31 arithmetic, opaque
  uint32_t r;
  asm("v_ashrrev_i32 %0, 31, %1" : "=v"(r) : "v"(x));
  return r;
}
__device__ __forceinline__ int sw32(int r) {
  const int x = (r >> 1) & 7;
  return ((x & 1) << 2) | (x >> 1);
}
__device__ __forceinline__ f32x16 mma32(const bf16x8_t& a, const bf16x8_t& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// bf16 B/A fragment from accumulator registers 8s .. 8s + 7
__device__ __forceinline__ bf16x8_t pack8(const f32x16& x, int s) {
  u16x8 v = {f2bf(x[8 * s + 0]), f2bf(x[8 * s + 1]), f2bf(x[8 * s + 2]), f2bf(x[8 * s + 3]),
             f2bf(x[8 * s + 4]), f2bf(x[8 * s + 5]), f2bf(x[8 * s + 6]), f2bf(x[8 * s + 7])};
  return __builtin_bit_cast(bf16x8_t, v);
}

// DMODE: dropout 0 none, 1 counter hash, 2 counter hash + keep bits out; WIDE: dropout pair
// indices reach 2^32 (the low word can wrap inside a tile)
template <int DMODE, bool WIDE>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_fwd32_kernel(AttnArgs a) {
  constexpr bool DROP = DMODE != 0;
  extern __shared__ __attribute__((aligned(16))) unsigned short smem[];  // 2 x (K, V) + bias
  const int T = a.T;
  const int nkt = (T + 63) >> 6;
  float* sBias = reinterpret_cast<float*>(smem + 4 * IMG);
  int* sZero = reinterpret_cast<int*>(sBias + nkt * 64);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hh = lane >> 5, r32 = lane & 31;
  const BlkIdx bi = attn_block((T + 127) >> 7, a.heads);
  const int h = bi.h, p = bi.p;
  const int qw = bi.x * 128 + wave * 64;
  const int nqb = qw < T ? min(2, (T - qw + 31) >> 5) : 0;  // wave-uniform
  const int64_t ld = a.ld_qkv;
  const rsrc_t rk = head_rsrc(a.qkv, (int64_t)p * T, ld, a.k_off + h * 64, T);
  const rsrc_t rv = head_rsrc(a.qkv, (int64_t)p * T, ld, a.v_off + h * 64, T);
  // LDS-DMA piece = 8 rows x 128 B; lane -> row 8 pc + (lane >> 3), stored chunk lane & 7, source
  // chunk (lane & 7) ^ g(4 (pc & 1) + (lane >> 4))
  uint32_t soff[2];
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int x = 4 * par + (lane >> 4);
    const int g = ((x & 1) << 2) | (x >> 1);
    soff[par] = (uint32_t)((lane >> 3) * ld * 2 + (((lane & 7) ^ g) << 4));
  }
  auto stage = [&](int t) {
    unsigned short* kimg = smem + (t & 1) * 2 * IMG;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int pc = wave * 4 + e;
      const uint32_t vo = soff[pc & 1] + (uint32_t)((int64_t)(t * 64 + pc * 8) * ld * 2);
      dma16(rk, kimg + pc * 512, vo);
      dma16(rv, kimg + IMG + pc * 512, vo);
    }
  };
  stage(0);
  const float* kbias = a.key_bias ? a.key_bias + (int64_t)p * T : nullptr;
  const float inv_scale = 1.0f / a.scale;
  for (int tt = wave; tt < nkt; tt += 2) {
    const int k = tt * 64 + lane;
    const float bv = k < T ? (kbias ? kbias[k] * inv_scale : 0.f) : -1e30f;
    sBias[k] = bv;
    const bool z = __ballot(bv != 0.f) == 0;
    if (lane == 0) sZero[tt] = z;
  }
  // Q^T fragments (B operand): lane (r32, hh) of q-block qb, k-step s: Q[row][16 s + 8 hh ..]
  const unsigned short* Qb = reinterpret_cast<const unsigned short*>(a.qkv) + (int64_t)p * T * ld +
                             a.q_off + h * 64;
  bf16x8_t qf[2][4];
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const int q = qw + qb * 32 + r32;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (q < T) v = *reinterpret_cast<const u16x8*>(Qb + (int64_t)q * ld + 16 * s + 8 * hh);
      qf[qb][s] = __builtin_bit_cast(bf16x8_t, v);
      settle(qf[qb][s]);
    }
  }
  // fragment offsets (elements): K rows kb * 32 + r32 (+ 2048 kb), chunk 2 s + hh
  const int sw = sw32(r32);
  int koff[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) koff[s] = r32 * 64 + (((2 * s + hh) ^ sw) << 3);
  // V^T: read e of k-step s (+ 1024 s), d-block db: lane 4q + pp of its 16-lane group addresses
  // key row 8 e + 4 hh + q, columns 32 db + 16 gi + 4 pp
  int voff[2][2];
  {
    const int gi = (lane >> 4) & 1, q4 = (lane >> 2) & 3, pp = lane & 3;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int r = 8 * e + 4 * hh + q4;
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        const int ch = db * 4 + gi * 2 + (pp >> 1);
        voff[e][db] = r * 64 + ((ch ^ sw32(r)) << 3) + 4 * (pp & 1);
      }
    }
  }
  const float c = a.scale * LOG2E;
  const int Tp4 = (T + 3) & ~3;
  const rsrc_t rbits = DMODE == 2 ? make_rsrc(a.bits + ((int64_t)p * a.heads + h) * T * a.nkt2,
                                              (int64_t)T * a.nkt2 * 8)
                                  : make_rsrc(a.qkv, 0);

  f32x16 o[2][2];
  float m[2] = {-1e30f, -1e30f}, l[2] = {0.f, 0.f};
#pragma unroll
  for (int qb = 0; qb < 2; ++qb)
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int j = 0; j < 16; ++j) o[qb][db][j] = 0.f;

  for (int t = 0; t < nkt; ++t) {
    // tile t landed everywhere (counted wait: a DMODE-2 wave's keep-bit stores of tile t - 1 are
    // newer than tile t's DMA); buffer (t + 1) & 1 no longer read
    if (DMODE == 2 && t > 0 && nqb > 0)
      asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (t + 1 < nkt) stage(t + 1);
    if (nqb == 0) continue;
    const unsigned short* kimg = smem + (t & 1) * 2 * IMG;
    const unsigned short* vimg = kimg + IMG;
    const bool zb = __builtin_amdgcn_readfirstlane(sZero[t]) != 0;
    // One code path for every tile: the last tile's keys >= T carry a -1e30 bias and the tail
    // wave's rows >= T have Q = 0 (their outputs are not stored), so nothing is bounds-checked.
    // S^T for both q-blocks (the K fragments die after these MFMAs)
    f32x16 sc[2][2];
    {
      bf16x8_t kf[2][4];
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int s = 0; s < 4; ++s) kf[kb][s] = lds_row(kimg, kb * 2048 + koff[s]);
#pragma unroll
      for (int qb = 0; qb < 2; ++qb)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          sc[qb][kb] = mma32(kf[kb][0], qf[qb][0], (f32x16){});  // C = inline 0
#pragma unroll
          for (int s = 1; s < 4; ++s) sc[qb][kb] = mma32(kf[kb][s], qf[qb][s], sc[qb][kb]);
        }
    }
    if (!zb) {  // additive key mask, stored in raw-score units (bias / scale)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const f32x4 b = *reinterpret_cast<const f32x4*>(sBias + t * 64 + kb * 32 + 8 * jj + 4 * hh);
#pragma unroll
          for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int r = 0; r < 4; ++r) sc[qb][kb][4 * jj + r] += b[r];
        }
    }
    __builtin_amdgcn_sched_barrier(0);  // keep the V reads behind the K fragments' last use
    // V^T fragments, issued now and consumed after the softmax
    bf16x8_t vf[2][4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (MMSEQ_LDS s16x4*)(vimg + s * 1024 + voff[0][db]));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (MMSEQ_LDS s16x4*)(vimg + s * 1024 + voff[1][db]));
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        vf[db][s] = __builtin_bit_cast(bf16x8_t, v);
      }
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
      float mx = -1e30f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int j = 0; j < 16; ++j) mx = fmaxf(mx, sc[qb][kb][j]);
      mx *= c;  // c > 0
      // lazy rescaling: the running max (shared by the two lane halves of a query) only moves
      // when some row's tile max exceeds it by more than 8 (log2 units)
      if (__ballot(mx > m[qb] + 8.f) != 0) {
        const float mfull = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m[qb], mfull);
        const float alpha = ex2(m[qb] - mn);
        m[qb] = mn;
        l[qb] *= alpha;
#pragma unroll
        for (int db = 0; db < 2; ++db) o[qb][db] *= alpha;
      }
      const float nm = -m[qb];
      float rs = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float e = ex2(fmaf(sc[qb][kb][j], c, nm));
          sc[qb][kb][j] = e;
          rs += e;
        }
      l[qb] += rs;
      if (DROP) {  // the normaliser keeps the undropped probabilities (dropout after softmax)
        const int q = qw + qb * 32 + r32;
        // quad index (row base + key) / 4 = dp4 + key / 4: the row base is a multiple of 4 and
        // key / 4 < 16, so the low word never wraps when WIDE is false (checked on the host), and
        // otherwise the high word takes the carry
        const uint64_t dp4 = ((((uint64_t)p * a.heads + h) * T + q) * Tp4 + t * 64) >> 2;
        const uint32_t dlo = (uint32_t)dp4, dhi = (uint32_t)(dp4 >> 32);
        const uint32_t H0 = dhi ^ a.drop.k1, H1 = (dhi + 1u) ^ a.drop.k1;
        const uint32_t thr = a.drop.thr;
        uint32_t wb[2] = {0u, 0u};
        uint32_t hq = 0;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
          for (int j = 0; j < 16; j += 2) {
            const int key = kb * 32 + (j & 3) + 8 * (j >> 2) + 4 * hh;  // even; j & 3: 0 or 2
            if ((j & 3) == 0) {  // the quad of keys key .. key + 3
              const uint32_t lo = dlo + (uint32_t)(key >> 2);
              const uint32_t hw = WIDE ? (lo < dlo ? H1 : H0) : H0;
              hq = drop_mix((lo ^ a.drop.k0) + hw);  // = drop_hash(quad index)
            }
            const uint32_t hs = (j & 3) ? drop_hash2(hq) : hq;
            // all-ones where dropped (half < thr), as plain VALU values: the shift is opaque asm so
            // the compiler cannot turn it into a compare + select (64 lane masks in SGPRs spill)
            const uint32_t d0 = sign_mask((hs & 0xFFFFu) - thr);
            const uint32_t d1 = sign_mask((hs >> 16) - thr);
            sc[qb][kb][j] = __uint_as_float(__float_as_uint(sc[qb][kb][j]) & ~d0);
            sc[qb][kb][j + 1] = __uint_as_float(__float_as_uint(sc[qb][kb][j + 1]) & ~d1);
            if (DMODE == 2) {  // bit of key jj: 16 ((jj >> 2) & 3) + 4 (jj >> 4) + (jj & 3)
              const int pos = 16 * hh + 8 * kb + 4 * (j >> 3) + (j & 3);
              wb[(j >> 2) & 1] |= ((~d0 & 1u) | (~d1 & 2u)) << pos;
            }
          }
        }
        if (DMODE == 2) {
          wb[0] |= __shfl_xor(wb[0], 32, 64);
          wb[1] |= __shfl_xor(wb[1], 32, 64);
          // rows q >= T fall outside the descriptor and are dropped; lane half 1 stores nothing
          const uint32_t bo = (uint32_t)((q * a.nkt2 + t) * 8);
          __builtin_amdgcn_raw_buffer_store_b32(wb[0], rbits, hh ? 0xFFFFFFF0u : bo, 0, 0);
          __builtin_amdgcn_raw_buffer_store_b32(wb[1], rbits, hh ? 0xFFFFFFF0u : bo + 4, 0, 0);
        }
      }
    }
    // O^T += V^T P^T (P^T = the bf16-packed score registers)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int qb = 0; qb < 2; ++qb) {
        const bf16x8_t pf = pack8(sc[qb][s >> 1], s & 1);
#pragma unroll
        for (int db = 0; db < 2; ++db) o[qb][db] = mma32(vf[db][s], pf, o[qb][db]);
      }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (nqb == 0) return;
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    if (qb >= nqb) break;
    const float lt = l[qb] + __shfl_xor(l[qb], 32, 64);
    const int q = qw + qb * 32 + r32;
    if (q < T) {
      const float inv = (DROP ? a.drop.scale : 1.0f) / lt;
      unsigned short* op = reinterpret_cast<unsigned short*>(a.o_w) + ((int64_t)p * T + q) * a.ld_out +
                           h * 64 + 4 * hh;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const f32x4 v = {o[qb][db][4 * jj], o[qb][db][4 * jj + 1], o[qb][db][4 * jj + 2],
                           o[qb][db][4 * jj + 3]};
          Vec4<unsigned short>::st(op + db * 32 + 8 * jj, v * inv);
        }
      if (hh == 0) a.lse[((int64_t)p * a.heads + h) * T + q] = (m[qb] + __builtin_amdgcn_logf(lt)) * LN2;
    }
  }
}

// ---- backward: dQ (per 128-query block, keys swept), also writes delta = rowsum(dO * O) --------
// without dropout four workgroups per CU (127 VGPRs); the dropout modes need 142-148 (three)
template <int DMODE>  // dropout: 0 none, 1 counter hash, 2 keep bits from the forward
__global__ __launch_bounds__(256, DMODE == 0 ? 4 : 2) void attn_dq_bf16_kernel(AttnArgs a) {
  constexpr bool DROP = DMODE != 0;
  extern __shared__ __attribute__((aligned(16))) unsigned short smem[];
  float* sBias = reinterpret_cast<float*>(smem + 4 * IMG);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i = lane & 15;
  const int T = a.T;
  const BlkIdx bi = attn_block((a.Tq + 127) >> 7, a.heads);
  const int h = bi.h, p = bi.p;
  const int nkt = (T + 63) >> 6;
  const int qw = bi.x * 128 + wave * 32;
  const bool active = qw < a.Tq;
  const int64_t ld = a.ld_qkv;
  const rsrc_t rk = head_rsrc(a.qkv, (int64_t)p * T, ld, a.k_off + h * 64, T);
  const rsrc_t rv = head_rsrc(a.qkv, (int64_t)p * T, ld, a.v_off + h * 64, T);
  const uint32_t loff = dma_lane_off(lane, ld);
  // keep-bit slices (DMODE 2) written by the forward; rows q >= T read as zero
  const rsrc_t rbits = DMODE == 2 ? make_rsrc(a.bits + ((int64_t)p * a.heads + h) * T * a.nkt2,
                                              (int64_t)T * a.nkt2 * 8)
                                  : make_rsrc(a.qkv, 0);
  const uint32_t boff0 = (uint32_t)(((qw + i) * a.nkt2 * 4 + g) * 2);
  auto stage = [&](int t) {
    unsigned short* kimg = smem + (t & 1) * 2 * IMG;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int pc = wave * 2 + e;
      const uint32_t vo = loff + (uint32_t)((int64_t)(t * 64 + pc * 8) * ld * 2);
      dma16(rk, kimg + pc * 512, vo);
      dma16(rv, kimg + IMG + pc * 512, vo);
    }
  };
  stage(0);
  // the prologue's global loads (key bias for T <= 1024, Q / dO / O fragments, LSE) are all issued
  // before the first is consumed: one memory round trip beside tile 0's DMA
  const float* kbias = a.key_bias ? a.key_bias + (int64_t)p * T : nullptr;
  const rsrc_t rkb = make_rsrc(kbias, kbias ? (int64_t)T * 4 : 0);
  float kbv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) kbv[j] = buf_f32(rkb, tid + 256 * j);
  bf16x8_t qf[2][2], of[2][2], ovf[2][2];
  float L2[2], Dd[2];
  const rsrc_t rq = head_rsrc(a.qkv, (int64_t)p * T, ld, a.q_off + h * 64, T);
  // O / dO: Tq rows per pair (rows >= Tq read as zero: their dS and dQ are zero)
  const rsrc_t rdo = head_rsrc(a.dout, (int64_t)p * a.Tq, a.ld_dout, h * 64, a.Tq);
  const rsrc_t rout = head_rsrc(a.out, (int64_t)p * a.Tq, a.ld_out, h * 64, a.Tq);
  const rsrc_t rlse = make_rsrc(a.lse + ((int64_t)p * a.heads + h) * T, (int64_t)T * 4);
#pragma unroll
  for (int grp = 0; grp < 2; ++grp) {
    const int q = qw + grp * 16 + i;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[grp][ks] = buf_row_frag(rq, q, ld, ks, lane);
      of[grp][ks] = buf_row_frag(rdo, q, a.ld_dout, ks, lane);
      ovf[grp][ks] = buf_row_frag(rout, q, a.ld_out, ks, lane);
    }
    L2[grp] = buf_f32(rlse, q);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = tid + 256 * j;
    if (k < nkt * 64) sBias[k] = k < T ? kbv[j] * LOG2E : -1e30f;
  }
  for (int k = tid + 1024; k < nkt * 64; k += 256) sBias[k] = k < T ? buf_f32(rkb, k) * LOG2E : -1e30f;
#pragma unroll
  for (int grp = 0; grp < 2; ++grp) {
    const int q = qw + grp * 16 + i;
    float dot = 0.f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const u16x8 x = __builtin_bit_cast(u16x8, of[grp][ks]), y = __builtin_bit_cast(u16x8, ovf[grp][ks]);
#pragma unroll
      for (int e = 0; e < 8; ++e) dot = fmaf(bf2f(x[e]), bf2f(y[e]), dot);
    }
    dot += __shfl_xor(dot, 16, 64);
    dot += __shfl_xor(dot, 32, 64);
    Dd[grp] = dot;
    const int64_t ri = ((int64_t)p * a.heads + h) * T + q;
    L2[grp] = q < a.Tq ? L2[grp] * LOG2E : 1e30f;
    if (q < a.Tq && g == 0) a.delta[ri] = dot;  // rows >= Tq stay untouched (mmseq_attn_bwd_rows)
    settle(qf[grp][0]);
    settle(qf[grp][1]);
    settle(L2[grp]);
  }
  const float c = a.scale * LOG2E;
  const int Tp4 = (T + 3) & ~3;
  uint64_t drow[2];
#pragma unroll
  for (int grp = 0; grp < 2; ++grp)
    drow[grp] = (((uint64_t)p * a.heads + h) * T + (qw + grp * 16 + i)) * Tp4;
  // keep-bit mode (three workgroups per CU, register room): the row's -L/c as the S MFMAs'
  // accumulator input, so P = 2^(S c + key bias) in one FMA (the no-dropout kernel, at four
  // workgroups per CU, has no room for the two replicated tuples)
  constexpr bool DQ_LINIT = DMODE == 2;
  f32x4 linit[2];
#pragma unroll
  for (int grp = 0; grp < 2; ++grp) {
    const float nl = -L2[grp] / c;
    linit[grp] = (f32x4){nl, nl, nl, nl};
  }
  f32x4 dq[2][4];
#pragma unroll
  for (int grp = 0; grp < 2; ++grp)
#pragma unroll
    for (int d = 0; d < 4; ++d) dq[grp][d] = (f32x4){0.f, 0.f, 0.f, 0.f};

  uint32_t kwn[2] = {0xFFFFu, 0xFFFFu};  // keep slices of the next tile (DMODE 2)
  if (DMODE == 2 && active) {
#pragma unroll
    for (int grp = 0; grp < 2; ++grp)
      kwn[grp] = __builtin_amdgcn_raw_buffer_load_b16(rbits, boff0 + grp * 16 * a.nkt2 * 8, 0, 0);
  }
  for (int t = 0; t < nkt; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const uint32_t kw16[2] = {kwn[0], kwn[1]};
    if (DMODE == 2) {  // landed with the wait above; settling here keeps the compiler's wait out
      settle(kw16[0]);  // of the tile body (it would cover the prefetch DMA issued below)
      settle(kw16[1]);
    }
    if (t + 1 < nkt) stage(t + 1);
    if (DMODE == 2 && active) {  // keep slices of tile t + 1, consumed next round (past the last
                                 // tile this reads the next row's word or, at the end, zero)
#pragma unroll
      for (int grp = 0; grp < 2; ++grp)
        kwn[grp] = __builtin_amdgcn_raw_buffer_load_b16(rbits, boff0 + grp * 16 * a.nkt2 * 8 + (t + 1) * 8, 0, 0);
    }
    // issued here, a whole tile ahead of the wait at the next tile's top (left to the scheduler they
    // sank to the end of the tile body, and that wait then exposed their memory latency)
    if (DMODE == 2) __builtin_amdgcn_sched_barrier(0);
    if (!active) continue;
    const unsigned short* kimg = smem + (t & 1) * 2 * IMG;
    const unsigned short* vimg = kimg + IMG;
    int ro0, ro1, to[4];
    {
      uint32_t ln = (uint32_t)lane;  // no dropout (four workgroups per CU, <= 128 VGPRs): the lane-
      // derived LDS offsets are recomputed per tile instead of held across the loop
      if (DMODE == 0) asm volatile("v_mov_b32 %0, %1" : "=v"(ln) : "v"(ln));
      ro0 = row_off((int)ln, 0);
      ro1 = row_off((int)ln, 1);
#pragma unroll
      for (int d = 0; d < 4; ++d) to[d] = tr_off((int)ln, d);
    }
    f32x4 s[2][4], dp[2][4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const bf16x8_t k0 = lds_row(kimg, kb * 1024 + ro0), k1 = lds_row(kimg, kb * 1024 + ro1);
      const bf16x8_t v0 = lds_row(vimg, kb * 1024 + ro0), v1 = lds_row(vimg, kb * 1024 + ro1);
#pragma unroll
      for (int grp = 0; grp < 2; ++grp) {
        s[grp][kb] = mma(k0, qf[grp][0], DQ_LINIT ? linit[grp] : (f32x4){0.f, 0.f, 0.f, 0.f});
        s[grp][kb] = mma(k1, qf[grp][1], s[grp][kb]);
        dp[grp][kb] = mma(v0, of[grp][0], (f32x4){0.f, 0.f, 0.f, 0.f});
        dp[grp][kb] = mma(v1, of[grp][1], dp[grp][kb]);
      }
    }
    f32x4 bias[4];
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      bias[kb] = *reinterpret_cast<const f32x4*>(sBias + t * 64 + kb * 16 + 4 * g);
    const uint32_t scale_u = __float_as_uint(a.drop.scale);
    bf16x8_t dsf[2][2];
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) {
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        float dm[4] = {1.f, 1.f, 1.f, 1.f};
        if (DMODE == 1) drop_mul_pairs<2>(a.drop, drow[grp] + t * 64 + kb * 16 + 4 * g, dm);
        if (DMODE == 2) {
#pragma unroll
          for (int r = 0; r < 4; ++r)  // 0 or 1/(1-p): the scale's bits ANDed with the sign-extended bit
            dm[r] = __uint_as_float((uint32_t)__builtin_amdgcn_sbfe((int)kw16[grp], kb * 4 + r, 1) & scale_u);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv = DQ_LINIT ? ex2(fmaf(s[grp][kb][r], c, bias[kb][r]))
                                  : ex2(fmaf(s[grp][kb][r], c, bias[kb][r]) - L2[grp]);
          dp[grp][kb][r] = pv * fmaf(dp[grp][kb][r], dm[r], -Dd[grp]);
        }
      }
      dsf[grp][0] = pack_pair(dp[grp][0], dp[grp][1]);
      dsf[grp][1] = pack_pair(dp[grp][2], dp[grp][3]);
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const bf16x8_t k0 = lds_tr(kimg, to[d]), k1 = lds_tr(kimg, 32 * 64 + to[d]);
#pragma unroll
      for (int grp = 0; grp < 2; ++grp) {
        dq[grp][d] = mma(k0, dsf[grp][0], dq[grp][d]);
        dq[grp][d] = mma(k1, dsf[grp][1], dq[grp][d]);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (!active) return;
#pragma unroll
  for (int grp = 0; grp < 2; ++grp) {
    const int q = qw + grp * 16 + i;
    if (q < T) {
      unsigned short* dqp = reinterpret_cast<unsigned short*>(a.dqkv) +
                            ((int64_t)p * T + q) * a.ld_dqkv + a.q_off + h * 64 + 4 * g;
#pragma unroll
      for (int d = 0; d < 4; ++d) Vec4<unsigned short>::st(dqp + d * 16, dq[grp][d] * a.scale);
      if (a.q8) q8_head_row(a, (int64_t)p * T + q, (int)a.q_off + h * 64, dq[grp], a.scale, g);
    }
  }
}

// rows >= Tq have no query (a Tq < T backward, mmseq_attn_bwd_rows): their dQ slice of head h is
// zero; the dK / dV kernel, which owns every key row, writes it
__device__ __forceinline__ void zero_dq(const AttnArgs& a, unsigned short* row, int h, int g) {
  unsigned short* dqp = row + a.q_off + h * 64 + 4 * g;
#pragma unroll
  for (int d = 0; d < 4; ++d) Vec4<unsigned short>::st(dqp + d * 16, (f32x4){0.f, 0.f, 0.f, 0.f});
}

// ---- backward: dK, dV (per 128-key block, queries swept; key on the MFMA lane) ----------------
// FOLD: this launch holds the tail blocks (x = nxq - 1 when a.tail0 > 0); the kernel without it
// carries none of the tail keys' registers (dK/dV<2>: 251 -> 212 VGPRs, <0>: 234 -> 166, i.e. three
// waves per SIMD instead of two)
// Plain blocks of the keep-bit / no-dropout modes: three workgroups per CU (<= 168 VGPRs); in the
// keep-bit one the lane-derived LDS offsets are recomputed in every tile (volatile lane copy) rather
// than held across the loop, which at 168 registers spilled them into reloads whose vmcnt wait also
// drained the next tile's DMA.
template <int DMODE, bool FOLD>  // dropout: 0 none, 1 counter hash, 2 keep bits from the forward
__global__ __launch_bounds__(256, FOLD || DMODE == 1 ? 2 : 3) void attn_dkdv_bf16_kernel(AttnArgs a) {
  constexpr bool DROP = DMODE != 0;
  extern __shared__ __attribute__((aligned(16))) unsigned short smem[];  // 2 x (Q, dO) + lse, D
  const int T = a.T, Tq = a.Tq;
  const int nqt = (Tq + 63) >> 6;  // the queries swept: rows < Tq (the others have dO = 0)
  float* sL = reinterpret_cast<float*>(smem + 4 * IMG);
  float* sD = sL + nqt * 64;
  // keep-bit words of the q-tile for this block's two key tiles: [2 buffers][64 q][4 dwords]
  unsigned short* sBits = reinterpret_cast<unsigned short*>(sD + nqt * 64);
  // tail fold (a.tail0 > 0, see tail_fold): the tail keys' keep words [2][64 q][4 dwords] and their
  // K / V row fragments [4][64 lanes] x 16 B
  unsigned short* sBitsT = sBits + 1024;
  u16x8* sKVt = reinterpret_cast<u16x8*>(sBitsT + 1024);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i = lane & 15;
  BlkIdx bi = attn_block(a.nxl, a.heads);
  bi.x += a.xoff;
  const int h = bi.h, p = bi.p;
  const int kw = bi.x * 128 + wave * 32;
  const bool active = kw < T;
  // tail block: it also owns keys tail0 .. T-1 (one 16-key group); the query sweep of that group is
  // split over the waves (wave w takes the 16-query block w of every tile) and the four partial
  // dK / dV tiles are summed in wave order at the end (deterministic); not in the counter-hash mode
  // (DMODE 1: its registers go to the hashed keep masks; the host does not fold it)
  const bool tailb = FOLD && DMODE != 1 && a.tail0 > 0 && bi.x == a.nxq - 1;
  const int64_t ld = a.ld_qkv;
  const rsrc_t rq = head_rsrc(a.qkv, (int64_t)p * T, ld, a.q_off + h * 64, T);
  const rsrc_t ro = head_rsrc(a.dout, (int64_t)p * Tq, a.ld_dout, h * 64, Tq);
  const uint32_t loffq = dma_lane_off(lane, ld), loffo = dma_lane_off(lane, a.ld_dout);
  const int64_t bh = (int64_t)p * a.heads + h;
  const rsrc_t rbits = DMODE == 2 ? make_rsrc(a.bits + bh * T * a.nkt2, (int64_t)T * a.nkt2 * 8)
                                  : make_rsrc(a.qkv, 0);
  const int kt0 = 2 * bi.x;  // this block's first key tile
  auto stage = [&](int t) {
    unsigned short* qimg = smem + (t & 1) * 2 * IMG;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int pc = wave * 2 + e;
      dma16(rq, qimg + pc * 512, loffq + (uint32_t)((int64_t)(t * 64 + pc * 8) * ld * 2));
      dma16(ro, qimg + IMG + pc * 512, loffo + (uint32_t)((int64_t)(t * 64 + pc * 8) * a.ld_dout * 2));
    }
    if (DMODE == 2 && wave == 0)  // 64 rows x 16 B: words (kt0, kt0 + 1) of queries t*64 + lane
      dma16(rbits, sBits + (t & 1) * 512,
            (uint32_t)((((int64_t)(t * 64 + lane)) * a.nkt2 + kt0) * 8));
    if (DMODE == 2 && tailb && wave == 1)  // words (kt0 + 2, kt0 + 3): the tail keys' tile
      dma16(rbits, sBitsT + (t & 1) * 512,
            (uint32_t)((((int64_t)(t * 64 + lane)) * a.nkt2 + kt0 + 2) * 8));
  };
  stage(0);
  // the prologue's global loads (LSE / delta rows for T <= 1024, the key and value fragments, the
  // key bias, the tail keys) are all issued before the first is consumed: one memory round trip
  // (beside tile 0's DMA) instead of one per loop iteration and fragment group
  const int64_t rb = ((int64_t)p * a.heads + h) * T;
  const rsrc_t rlse = make_rsrc(a.lse + rb, (int64_t)T * 4), rdel = make_rsrc(a.delta + rb, (int64_t)T * 4);
  float lv[4], dlv[4];
  // sL: L (log2 units) for DMODE 1; for DMODE 0 and 2 (no dropout, keep bits read) -L / c (the S
  // MFMAs' accumulator input, below)
  constexpr bool LINIT = DMODE != 1;  // -L/c as the S MFMAs' input
  const float nic = LINIT ? -1.f / (a.scale * LOG2E) : 1.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lv[j] = buf_f32(rlse, tid + 256 * j);
    dlv[j] = buf_f32(rdel, tid + 256 * j);
  }
  const rsrc_t rk = head_rsrc(a.qkv, (int64_t)p * T, ld, a.k_off + h * 64, T);
  const rsrc_t rv = head_rsrc(a.qkv, (int64_t)p * T, ld, a.v_off + h * 64, T);
  const float* kbias = a.key_bias ? a.key_bias + (int64_t)p * T : nullptr;
  const rsrc_t rkb = make_rsrc(kbias, kbias ? (int64_t)T * 4 : 0);
  bf16x8_t kf[2][2], vf[2][2];
  float kb2[2];
#pragma unroll
  for (int grp = 0; grp < 2; ++grp) {
    const int key = kw + grp * 16 + i;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kf[grp][ks] = buf_row_frag(rk, key, ld, ks, lane);
      vf[grp][ks] = buf_row_frag(rv, key, ld, ks, lane);
    }
    kb2[grp] = buf_f32(rkb, key);
  }
  float kb2t = 0.f;
  u16x8 kvt[4];
  if (tailb) {  // block-uniform
    const int key = a.tail0 + i;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      kvt[ks] = __builtin_bit_cast(u16x8, buf_row_frag(rk, key, ld, ks, lane));
      kvt[2 + ks] = __builtin_bit_cast(u16x8, buf_row_frag(rv, key, ld, ks, lane));
    }
    kb2t = buf_f32(rkb, key);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = tid + 256 * j;
    if (q < nqt * 64) {
      sL[q] = (q < Tq ? lv[j] * LOG2E : 1e30f) * nic;  // exp2(x - 1e30) = 0 for padded queries
      sD[q] = q < Tq ? -dlv[j] : 0.f;
    }
  }
  for (int q = tid + 1024; q < nqt * 64; q += 256) {
    sL[q] = (q < Tq ? buf_f32(rlse, q) * LOG2E : 1e30f) * nic;
    sD[q] = q < Tq ? -buf_f32(rdel, q) : 0.f;
  }
  if (tailb && wave == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) sKVt[e * 64 + lane] = kvt[e];
  }
#pragma unroll
  for (int grp = 0; grp < 2; ++grp) {
    const int key = kw + grp * 16 + i;
    kb2[grp] = key < T ? kb2[grp] * LOG2E : -1e30f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      settle(kf[grp][ks]);
      settle(vf[grp][ks]);
    }
    settle(kb2[grp]);
  }
  if (tailb) {
    kb2t = a.tail0 + i < T ? kb2t * LOG2E : -1e30f;
    settle(kb2t);
  } else {
    kb2t = -1e30f;
  }
  const float c = a.scale * LOG2E;
  const int Tp4 = (T + 3) & ~3;
  f32x4 dk[2][4], dv[2][4], dkt[4], dvt[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    dkt[d] = dvt[d] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int grp = 0; grp < 2; ++grp) dk[grp][d] = dv[grp][d] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  for (int t = 0; t < nqt; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + 1 < nqt) stage(t + 1);
    if (!active) continue;
    const unsigned short* qimg = smem + (t & 1) * 2 * IMG;
    const unsigned short* oimg = qimg + IMG;
    int ro0, ro1, to[4];
    {
      uint32_t ln = (uint32_t)lane;  // the 3-workgroup keep-bit kernel: not hoisted out of the loop,
      // and rebuilt from mbcnt (a copy of a held lane value was itself spilled, its reload a
      // vmcnt(0) behind the tile's LDS-DMA)
      if (DMODE == 2 && !FOLD)
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
      ro0 = row_off((int)ln, 0);
      ro1 = row_off((int)ln, 1);
#pragma unroll
      for (int d = 0; d < 4; ++d) to[d] = tr_off((int)ln, d);
    }
    // dropout multiplier of element (grp, qs, r): 0 or 1/(1-p), as the bits of the scale ANDed with
    // a sign-extended 1-bit field (v_bfe_i32 + v_and per element)
    const uint32_t scale_u = __float_as_uint(a.drop.scale);
    // DMODE 2: word (kt0 + (wave >> 1)) of a row holds this wave's keys; key j (0..63 in its
    // tile) sits at bit ((j >> 2) & 3) * 16 + (j >> 4) * 4 + (j & 3) (16-bit slice per forward lane
    // group). With j = (wave & 1) * 32 + grp * 16 + i that bit is in dword (i >> 3) & 1 of the word
    // at position pos0 + 4 grp: one 32-bit LDS read per query serves both groups, and the element's
    // multiplier is extracted straight from it
    const uint32_t* bw = reinterpret_cast<const uint32_t*>(sBits + (t & 1) * 512) +
                         (wave >> 1) * 2 + ((i >> 3) & 1);
    const uint32_t pos0 = ((i >> 2) & 1) * 16 + (wave & 1) * 8 + (i & 3);
    // DMODE 1: keep bits of this lane's 32 (q, key) elements, bit grp*16 + qs*4 + r, hashed before
    // the MFMAs (few live registers); (q, key) -> index (rb + q) * Tp4 + key
    uint32_t keep = 0xFFFFFFFFu;
    if (DMODE == 1) {
      keep = 0;
      const uint64_t dbase = (uint64_t)(rb + t * 64 + 4 * g) * (uint64_t)Tp4 + kw + i;
#pragma unroll
      for (int grp = 0; grp < 2; ++grp)
#pragma unroll
        for (int qs = 0; qs < 4; ++qs)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const uint64_t idx = dbase + (uint64_t)((qs * 16 + r) * Tp4 + grp * 16);
            const uint32_t hq = drop_hash(a.drop, idx >> 2);
            const uint32_t h = (idx & 2) ? drop_hash2(hq) : hq;
            const uint32_t u = (idx & 1) ? (h >> 16) : (h & 0xFFFFu);
            keep |= (u >= a.drop.thr ? 1u : 0u) << (grp * 16 + qs * 4 + r);
          }
    }
    __builtin_amdgcn_sched_barrier(0);  // keep the hashing ahead of the MFMAs (register pressure)
    // two halves of the 64-query tile (k-step ks of the dV / dK products = queries 32ks..+31):
    // S[q][key], dP[q][key] with the key on the lane (q = qs*16 + 4g + r, key = grp*16 + i), then
    // P / dS, then dV^T[d][key] += dO^T[d][q] P[q][key] and dK^T[d][key] += Q^T[d][q] dS[q][key]
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // DMODE 0 and 2 (LINIT): the row term of P enters as the S MFMAs' accumulator input: S starts at
      // -L/c (sL holds it), so S c = Q K^T c - L (sD holds -D; as dP's accumulator input, and in
      // the keep-bit kernel as S's, it spilled)
      // (each accumulator's input read from LDS on its own: a shared register copy would be copied)
      f32x4 s[2][2], dp[2][2];
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int qs = 2 * ks + h2;
        const f32x4* lrow = reinterpret_cast<const f32x4*>(sL + t * 64 + qs * 16 + 4 * g);
        const bf16x8_t q0 = lds_row(qimg, qs * 1024 + ro0), q1 = lds_row(qimg, qs * 1024 + ro1);
        const bf16x8_t o0 = lds_row(oimg, qs * 1024 + ro0), o1 = lds_row(oimg, qs * 1024 + ro1);
#pragma unroll
        for (int grp = 0; grp < 2; ++grp) {
          s[grp][h2] = mma(q0, kf[grp][0], LINIT ? *lrow : (f32x4){0.f, 0.f, 0.f, 0.f});
          s[grp][h2] = mma(q1, kf[grp][1], s[grp][h2]);
          dp[grp][h2] = mma(o0, vf[grp][0], (f32x4){0.f, 0.f, 0.f, 0.f});
          dp[grp][h2] = mma(o1, vf[grp][1], dp[grp][h2]);
        }
      }
      uint32_t kw32[2][4];  // DMODE 2: keep words of queries (2ks + h2) * 16 + 4g + r (read after
                            // the MFMAs: fewer registers live across them)
      if (DMODE == 2) {
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
          for (int r = 0; r < 4; ++r) kw32[h2][r] = bw[((2 * ks + h2) * 16 + 4 * g + r) * 4];
      }
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int qs = 2 * ks + h2;
        const f32x4 Dq = *reinterpret_cast<const f32x4*>(sD + t * 64 + qs * 16 + 4 * g);
        f32x4 Lq = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (!LINIT) Lq = *reinterpret_cast<const f32x4*>(sL + t * 64 + qs * 16 + 4 * g);
#pragma unroll
        for (int grp = 0; grp < 2; ++grp)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float pv = !LINIT ? ex2(fmaf(s[grp][h2][r], c, kb2[grp]) - Lq[r])
                                  : ex2(fmaf(s[grp][h2][r], c, kb2[grp]));
            float mk = 1.f;
            if (DMODE == 2)
              mk = __uint_as_float((uint32_t)__builtin_amdgcn_sbfe((int)kw32[h2][r], pos0 + 4 * grp, 1) & scale_u);
            if (DMODE == 1) mk = ((keep >> (grp * 16 + qs * 4 + r)) & 1u) ? a.drop.scale : 0.f;
            s[grp][h2][r] = DROP ? pv * mk : pv;
            dp[grp][h2][r] = pv * (DROP ? fmaf(dp[grp][h2][r], mk, Dq[r]) : dp[grp][h2][r] + Dq[r]);
          }
      }
      bf16x8_t pf[2], dsf[2];
#pragma unroll
      for (int grp = 0; grp < 2; ++grp) {
        pf[grp] = pack_pair(s[grp][0], s[grp][1]);
        dsf[grp] = pack_pair(dp[grp][0], dp[grp][1]);
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const bf16x8_t ov = lds_tr(oimg, ks * 32 * 64 + to[d]);
        const bf16x8_t qv = lds_tr(qimg, ks * 32 * 64 + to[d]);
#pragma unroll
        for (int grp = 0; grp < 2; ++grp) {
          dv[grp][d] = mma(ov, pf[grp], dv[grp][d]);
          dk[grp][d] = mma(qv, dsf[grp], dk[grp][d]);
        }
      }
    }
    if (tailb) {  // the tail keys against this wave's 16-query block of the tile
      asm volatile("" ::: "memory");  // keeps this work in the branch (not speculated into every block)
      const int qs = wave, ks = wave >> 1;
      const bf16x8_t q0 = lds_row(qimg, qs * 1024 + ro0), q1 = lds_row(qimg, qs * 1024 + ro1);
      const bf16x8_t o0 = lds_row(oimg, qs * 1024 + ro0), o1 = lds_row(oimg, qs * 1024 + ro1);
      const f32x4 Lq = *reinterpret_cast<const f32x4*>(sL + t * 64 + qs * 16 + 4 * g);
      const f32x4 Dq = *reinterpret_cast<const f32x4*>(sD + t * 64 + qs * 16 + 4 * g);
      f32x4 st = mma(q0, __builtin_bit_cast(bf16x8_t, sKVt[lane]), LINIT ? Lq : (f32x4){0.f, 0.f, 0.f, 0.f});
      st = mma(q1, __builtin_bit_cast(bf16x8_t, sKVt[64 + lane]), st);
      f32x4 dpt = mma(o0, __builtin_bit_cast(bf16x8_t, sKVt[128 + lane]), (f32x4){0.f, 0.f, 0.f, 0.f});
      dpt = mma(o1, __builtin_bit_cast(bf16x8_t, sKVt[192 + lane]), dpt);
      // DMODE 2: tail key j = i of its tile: bit ((i >> 2) & 1) * 16 + (i & 3), dword (i >> 3) & 1
      const uint32_t* bwt = reinterpret_cast<const uint32_t*>(sBitsT + (t & 1) * 512) + ((i >> 3) & 1);
      const uint32_t post = ((i >> 2) & 1) * 16 + (i & 3);
      const uint64_t dbt = (uint64_t)(rb + t * 64 + qs * 16 + 4 * g) * (uint64_t)Tp4 + a.tail0 + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = !LINIT ? ex2(fmaf(st[r], c, kb2t) - Lq[r]) : ex2(fmaf(st[r], c, kb2t));
        float mk = 1.f;
        if (DMODE == 2)
          mk = __uint_as_float((uint32_t)__builtin_amdgcn_sbfe((int)bwt[(qs * 16 + 4 * g + r) * 4], post, 1) & scale_u);
        if (DMODE == 1) mk = drop_mul(a.drop, dbt + (uint64_t)r * Tp4);
        st[r] = DROP ? pv * mk : pv;
        dpt[r] = pv * (DROP ? fmaf(dpt[r], mk, Dq[r]) : dpt[r] + Dq[r]);
      }
      // the block's 16 queries sit in the low (qs even) or high (qs odd) half of k-step ks
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      const bf16x8_t pft = (qs & 1) ? pack_pair(z, st) : pack_pair(st, z);
      const bf16x8_t dsft = (qs & 1) ? pack_pair(z, dpt) : pack_pair(dpt, z);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const bf16x8_t ov = lds_tr(oimg, ks * 32 * 64 + to[d]);
        const bf16x8_t qv = lds_tr(qimg, ks * 32 * 64 + to[d]);
        dvt[d] = mma(ov, pft, dvt[d]);
        dkt[d] = mma(qv, dsft, dkt[d]);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (tailb) {  // every wave of the tail block is active (its first key is < T)
    float* red = reinterpret_cast<float*>(smem);  // [3 waves][32 floats][64 lanes] = 24 KB
    __syncthreads();  // all waves are past their last LDS read of the images
    if (wave > 0) {
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          red[((wave - 1) * 32 + d * 4 + r) * 64 + lane] = dkt[d][r];
          red[((wave - 1) * 32 + 16 + d * 4 + r) * 64 + lane] = dvt[d][r];
        }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int w = 0; w < 3; ++w)
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            dkt[d][r] += red[(w * 32 + d * 4 + r) * 64 + lane];
            dvt[d][r] += red[(w * 32 + 16 + d * 4 + r) * 64 + lane];
          }
      const int key = a.tail0 + i;
      if (key < T) {
        unsigned short* row = reinterpret_cast<unsigned short*>(a.dqkv) + ((int64_t)p * T + key) * a.ld_dqkv;
        unsigned short* dkp = row + a.k_off + h * 64 + 4 * g;
        unsigned short* dvp = row + a.v_off + h * 64 + 4 * g;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          Vec4<unsigned short>::st(dkp + d * 16, dkt[d] * a.scale);
          Vec4<unsigned short>::st(dvp + d * 16, dvt[d]);
        }
        if (a.q8) {
          q8_head_row(a, (int64_t)p * T + key, (int)a.k_off + h * 64, dkt, a.scale, g);
          q8_head_row(a, (int64_t)p * T + key, (int)a.v_off + h * 64, dvt, 1.f, g);
        }
        if (key >= Tq) zero_dq(a, row, h, g);
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int grp = 0; grp < 2; ++grp) {
    const int key = kw + grp * 16 + i;
    if (key < T) {
      unsigned short* row = reinterpret_cast<unsigned short*>(a.dqkv) + ((int64_t)p * T + key) * a.ld_dqkv;
      unsigned short* dkp = row + a.k_off + h * 64 + 4 * g;
      unsigned short* dvp = row + a.v_off + h * 64 + 4 * g;
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        Vec4<unsigned short>::st(dkp + d * 16, dk[grp][d] * a.scale);
        Vec4<unsigned short>::st(dvp + d * 16, dv[grp][d]);
      }
      if (a.q8) {
        q8_head_row(a, (int64_t)p * T + key, (int)a.k_off + h * 64, dk[grp], a.scale, g);
        q8_head_row(a, (int64_t)p * T + key, (int)a.v_off + h * 64, dv[grp], 1.f, g);
      }
      if (key >= Tq) zero_dq(a, row, h, g);
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

mmseq_status check_common(int P, int T, int heads, const void* qkv, int64_t ld, int64_t qo,
                          int64_t ko, int64_t vo, mmseq_dtype dt) {
  MMSEQ_REQUIRE(P >= 0 && T > 0 && heads > 0, "attn: bad sizes P=%d T=%d heads=%d", P, T, heads);
  MMSEQ_REQUIRE(dt == MMSEQ_F32 || dt == MMSEQ_BF16, "attn: bad dtype");
  const int ve = dt == MMSEQ_BF16 ? 8 : 4;
  MMSEQ_REQUIRE(aligned16(qkv) && ld % ve == 0 && qo % ve == 0 && ko % ve == 0 && vo % ve == 0,
                "attn: qkv must be 16-byte aligned with ld/offsets multiple of %d", ve);
  MMSEQ_REQUIRE(qo + heads * 64 <= ld && ko + heads * 64 <= ld && vo + heads * 64 <= ld,
                "attn: head slices exceed the row");
  return MMSEQ_OK;
}

// the fields every entry fills alike; each adds its own outputs
AttnArgs attn_args(int P, int T, int Tq, int heads, const void* qkv, int64_t ld_qkv, int64_t q_off,
                   int64_t k_off, int64_t v_off, const float* key_bias, float scale,
                   const mmseq_dropout* drop, const uint64_t* keep_bits) {
  AttnArgs a = {};
  a.P = P; a.T = T; a.Tq = Tq; a.heads = heads; a.qkv = qkv; a.ld_qkv = ld_qkv;
  a.q_off = q_off; a.k_off = k_off; a.v_off = v_off; a.key_bias = key_bias; a.scale = scale;
  a.drop = make_drop(drop);
  a.bits = const_cast<uint64_t*>(keep_bits);  // read and written by the bf16 fast kernels alone
  a.nkt2 = attn_nkt2(T);
  return a;
}

// bf16 fast kernels by [dmode][wide or fold]. Without dropout there is no pair index, so dmode 0
// has the narrow form only; the counter-hash dK/dV never folds.
typedef void (*AttnKernel)(AttnArgs);
typedef const AttnKernel FwdFamily[3][2];
FwdFamily FWD32 = {{attn_fwd32_kernel<0, false>, attn_fwd32_kernel<0, false>},
                   {attn_fwd32_kernel<1, false>, attn_fwd32_kernel<1, true>},
                   {attn_fwd32_kernel<2, false>, attn_fwd32_kernel<2, true>}};
FwdFamily FWD16 = {{attn_fwd_bf16_kernel<0, false>, attn_fwd_bf16_kernel<0, false>},
                   {attn_fwd_bf16_kernel<1, false>, attn_fwd_bf16_kernel<1, true>},
                   {attn_fwd_bf16_kernel<2, false>, attn_fwd_bf16_kernel<2, true>}};
FwdFamily FWD16_Q8 = {{attn_fwd_bf16_kernel<0, false, true>, attn_fwd_bf16_kernel<0, false, true>},
                      {attn_fwd_bf16_kernel<1, false, true>, attn_fwd_bf16_kernel<1, true, true>},
                      {attn_fwd_bf16_kernel<2, false, true>, attn_fwd_bf16_kernel<2, true, true>}};
const AttnKernel DQ16[3] = {attn_dq_bf16_kernel<0>, attn_dq_bf16_kernel<1>, attn_dq_bf16_kernel<2>};
const AttnKernel DKDV16[3][2] = {{attn_dkdv_bf16_kernel<0, false>, attn_dkdv_bf16_kernel<0, true>},
                                 {attn_dkdv_bf16_kernel<1, false>, nullptr},
                                 {attn_dkdv_bf16_kernel<2, false>, attn_dkdv_bf16_kernel<2, true>}};

void launch_fwd(FwdFamily& k, const AttnFwdPlan& p, const AttnArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k[p.dmode][p.wide], dim3(p.blocks), dim3(p.threads), (size_t)p.lds_bytes, s, a);
}

}  // namespace

static mmseq_status attn_fwd_impl(int P, int T, int Tq, int heads, const void* qkv, int64_t ld_qkv,
                                  int64_t q_off, int64_t k_off, int64_t v_off,
                                  const float* key_bias, float scale, void* out, int64_t ld_out,
                                  float* lse, mmseq_dtype dtype, const mmseq_dropout* drop,
                                  uint64_t* keep_bits, int variant, mmseq_stream stream) {
  mmseq_status st = check_common(P, T, heads, qkv, ld_qkv, q_off, k_off, v_off, dtype);
  if (st) return st;
  MMSEQ_REQUIRE(out && lse && ld_out >= heads * 64, "attn_fwd: bad out/lse");
  MMSEQ_REQUIRE(Tq >= 1 && Tq <= T && (Tq == T || (dtype == MMSEQ_BF16 && variant == 1)),
                "attn_fwd: Tq=%d (1 <= Tq <= T; Tq < T needs the bf16 variant-1 kernels)", Tq);
  if (P == 0) return MMSEQ_OK;
  AttnArgs a = attn_args(P, T, Tq, heads, qkv, ld_qkv, q_off, k_off, v_off, key_bias, scale, drop, keep_bits);
  a.o_w = out; a.ld_out = ld_out; a.lse = lse;
  dim3 grid((T + QT - 1) / QT, heads, P);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MMSEQ_BF16 && variant) {
    MMSEQ_REQUIRE(aligned16(out) && ld_out % 8 == 0, "attn_fwd: out must be 16-byte aligned rows");
    launch_fwd(variant == 2 ? FWD32 : FWD16,
               attn_fwd_plan(P, T, Tq, heads, variant, a.drop.thr != 0, keep_bits != nullptr), a, s);
  } else if (dtype == MMSEQ_BF16)
    hipLaunchKernelGGL(attn_fwd_kernel<unsigned short>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(attn_fwd_kernel<float>, grid, dim3(256), 0, s, a);
  return mmseq_check_launch("attn_fwd");
}

extern "C" mmseq_status mmseq_attn_fwd(int P, int T, int heads, const void* qkv, int64_t ld_qkv,
                                       int64_t q_off, int64_t k_off, int64_t v_off,
                                       const float* key_bias, float scale, void* out,
                                       int64_t ld_out, float* lse, mmseq_dtype dtype,
                                       const mmseq_dropout* drop, uint64_t* keep_bits,
                                       int variant, mmseq_stream stream) {
  return attn_fwd_impl(P, T, T, heads, qkv, ld_qkv, q_off, k_off, v_off, key_bias, scale, out, ld_out,
                       lse, dtype, drop, keep_bits, variant, stream);
}

extern "C" mmseq_status mmseq_attn_fwd_rows(int P, int T, int Tq, int heads, const void* qkv,
                                            int64_t ld_qkv, int64_t q_off, int64_t k_off,
                                            int64_t v_off, const float* key_bias, float scale,
                                            void* out, int64_t ld_out, float* lse,
                                            const mmseq_dropout* drop, uint64_t* keep_bits,
                                            mmseq_stream stream) {
  return attn_fwd_impl(P, T, Tq, heads, qkv, ld_qkv, q_off, k_off, v_off, key_bias, scale, out,
                       ld_out, lse, MMSEQ_BF16, drop, keep_bits, 1, stream);
}

static mmseq_status attn_bwd_impl(int P, int T, int Tq, int heads, const void* qkv, int64_t ld_qkv,
                                  int64_t q_off, int64_t k_off, int64_t v_off,
                                  const float* key_bias, float scale, const void* out,
                                  int64_t ld_out, const void* dout, int64_t ld_dout,
                                  const float* lse, float* delta, void* dqkv, int64_t ld_dqkv,
                                  mmseq_dtype dtype, const mmseq_dropout* drop,
                                  const uint64_t* keep_bits, int variant, void* q8, int64_t ldq8,
                                  void* q8_scales, mmseq_stream stream) {
  mmseq_status st = check_common(P, T, heads, qkv, ld_qkv, q_off, k_off, v_off, dtype);
  if (st) return st;
  const int ve = dtype == MMSEQ_BF16 ? 8 : 4;
  MMSEQ_REQUIRE(out && dout && lse && delta && dqkv, "attn_bwd: null buffer");
  MMSEQ_REQUIRE(aligned16(dout) && ld_dout % ve == 0, "attn_bwd: dout alignment");
  // dqkv holds dQ | dK | dV at qkv's column offsets with its own row stride, which may be narrower
  // than ld_qkv as long as every head slice fits the row. The 64-row kernels store single elements
  // (no multiple needed); the 128-row kernels store groups of four bf16 and are held to 16-byte
  // rows below.
  const int64_t hi_off = q_off > k_off ? (q_off > v_off ? q_off : v_off) : (k_off > v_off ? k_off : v_off);
  MMSEQ_REQUIRE(hi_off + (int64_t)heads * 64 <= ld_dqkv,
                "attn_bwd: head slices exceed the dqkv row (ld_dqkv=%lld)", (long long)ld_dqkv);
  MMSEQ_REQUIRE(Tq >= 1 && Tq <= T && (Tq == T || (dtype == MMSEQ_BF16 && variant && !q8)),
                "attn_bwd: Tq=%d (1 <= Tq <= T; Tq < T needs the bf16 fast kernels, no MX-fp8 copy)", Tq);
  if (P == 0) return MMSEQ_OK;
  AttnArgs a = attn_args(P, T, Tq, heads, qkv, ld_qkv, q_off, k_off, v_off, key_bias, scale, drop, keep_bits);
  a.out = out; a.ld_out = ld_out; a.dout = dout; a.ld_dout = ld_dout;
  a.lse = const_cast<float*>(lse); a.delta = delta; a.dqkv = dqkv; a.ld_dqkv = ld_dqkv;
  a.q8 = reinterpret_cast<uint8_t*>(q8); a.ldq8 = ldq8; a.q8s = reinterpret_cast<uint8_t*>(q8_scales);
  if (q8 && !(dtype == MMSEQ_BF16 && variant))
    return mmseq_set_error(MMSEQ_EUNSUPPORTED, "attn_bwd_mxfp8: the bf16 fast kernels only");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t rows = (int64_t)P * T;
  dim3 gd((unsigned)((rows + 3) / 4));
  dim3 grid((T + QT - 1) / QT, heads, P);
  if (dtype == MMSEQ_BF16 && variant) {
    MMSEQ_REQUIRE(aligned16(out) && ld_out % 8 == 0 && aligned16(dqkv) && ld_dqkv % 8 == 0,
                  "attn_bwd: out / dqkv must be 16-byte aligned rows");
    // dQ, then dK/dV in up to two launches: the blocks without the tail keys, and the tail block
    // (x = nplain) with the fold's state and LDS
    const AttnBwdPlan bp = attn_bwd_plan(P, T, Tq, heads, a.drop.thr != 0, keep_bits != nullptr);
    hipLaunchKernelGGL(DQ16[bp.dmode], dim3(bp.dq_blocks), dim3(256), (size_t)bp.dq_lds, s, a);
    AttnArgs ak = a;
    ak.tail0 = bp.tail0; ak.nxq = bp.nxq;
    ak.xoff = 0; ak.nxl = bp.nplain;
    if (bp.nplain)
      hipLaunchKernelGGL(DKDV16[bp.dmode][0], dim3(bp.plain_blocks), dim3(256), (size_t)bp.dkdv_lds, s, ak);
    ak.xoff = bp.nplain; ak.nxl = 1;
    if (bp.ntail)
      hipLaunchKernelGGL(DKDV16[bp.dmode][1], dim3(bp.tail_blocks), dim3(256), (size_t)bp.tail_lds, s, ak);
  } else if (dtype == MMSEQ_BF16) {
    hipLaunchKernelGGL(attn_delta_kernel<unsigned short>, gd, dim3(256), 0, s, a);
    hipLaunchKernelGGL(attn_dkdv_kernel<unsigned short>, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(attn_dq_kernel<unsigned short>, grid, dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(attn_delta_kernel<float>, gd, dim3(256), 0, s, a);
    hipLaunchKernelGGL(attn_dkdv_kernel<float>, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(attn_dq_kernel<float>, grid, dim3(256), 0, s, a);
  }
  return mmseq_check_launch("attn_bwd");
}

extern "C" mmseq_status mmseq_attn_bwd(int P, int T, int heads, const void* qkv, int64_t ld_qkv,
                                       int64_t q_off, int64_t k_off, int64_t v_off,
                                       const float* key_bias, float scale, const void* out,
                                       int64_t ld_out, const void* dout, int64_t ld_dout,
                                       const float* lse, float* delta, void* dqkv,
                                       int64_t ld_dqkv, mmseq_dtype dtype,
                                       const mmseq_dropout* drop, const uint64_t* keep_bits,
                                       int variant, mmseq_stream stream) {
  return attn_bwd_impl(P, T, T, heads, qkv, ld_qkv, q_off, k_off, v_off, key_bias, scale, out, ld_out,
                       dout, ld_dout, lse, delta, dqkv, ld_dqkv, dtype, drop, keep_bits, variant,
                       nullptr, 0, nullptr, stream);
}

extern "C" mmseq_status mmseq_attn_bwd_rows(int P, int T, int Tq, int heads, const void* qkv,
                                            int64_t ld_qkv, int64_t q_off, int64_t k_off,
                                            int64_t v_off, const float* key_bias, float scale,
                                            const void* out, int64_t ld_out, const void* dout,
                                            int64_t ld_dout, const float* lse, float* delta,
                                            void* dqkv, int64_t ld_dqkv, const mmseq_dropout* drop,
                                            const uint64_t* keep_bits, mmseq_stream stream) {
  return attn_bwd_impl(P, T, Tq, heads, qkv, ld_qkv, q_off, k_off, v_off, key_bias, scale, out, ld_out,
                       dout, ld_dout, lse, delta, dqkv, ld_dqkv, MMSEQ_BF16, drop, keep_bits, 1,
                       nullptr, 0, nullptr, stream);
}

extern "C" mmseq_status mmseq_attn_bwd_mxfp8(int P, int T, int heads, const void* qkv,
                                             int64_t ld_qkv, const float* key_bias, float scale,
                                             const void* out, int64_t ld_out, const void* dout,
                                             int64_t ld_dout, const float* lse, float* delta,
                                             void* dqkv, int64_t ld_dqkv,
                                             const mmseq_dropout* drop, const uint64_t* keep_bits,
                                             void* q8, int64_t ldq8, void* q8_scales,
                                             mmseq_stream stream) {
  const int64_t H = (int64_t)heads * 64;
  MMSEQ_REQUIRE(q8 && q8_scales && ldq8 >= 3 * H && ldq8 % 16 == 0 && ((uintptr_t)q8 & 15) == 0,
                "attn_bwd_mxfp8: q8 / ldq8");
  return attn_bwd_impl(P, T, T, heads, qkv, ld_qkv, 0, H, 2 * H, key_bias, scale, out, ld_out, dout,
                       ld_dout, lse, delta, dqkv, ld_dqkv, MMSEQ_BF16, drop, keep_bits, 1, q8, ldq8,
                       q8_scales, stream);
}

extern "C" int64_t mmseq_attn_keep_bits_words(int P, int T, int heads) {
  return keep_bits_words(P, T, heads);
}

extern "C" mmseq_status mmseq_attn_fwd_mxfp8_dual(int P, int T, int heads, const void* qkv,
                                                  int64_t ld_qkv, int64_t q_off, int64_t k_off,
                                                  int64_t v_off, const float* key_bias, float scale,
                                                  void* out, int64_t ld_out, float* lse,
                                                  const mmseq_dropout* drop, uint64_t* keep_bits,
                                                  void* q8, int64_t ldq8, void* q8_scales,
                                                  mmseq_stream stream) {
  mmseq_status st = check_common(P, T, heads, qkv, ld_qkv, q_off, k_off, v_off, MMSEQ_BF16);
  if (st) return st;
  MMSEQ_REQUIRE(lse && q8 && q8_scales && ldq8 >= heads * 64 && ldq8 % 16 == 0 &&
                    ((uintptr_t)q8 & 15) == 0,
                "attn_fwd_mxfp8: bad output (ldq8 % 16, 16-byte aligned)");
  MMSEQ_REQUIRE(!out || (ld_out >= heads * 64 && ld_out % 4 == 0 && ((uintptr_t)out & 7) == 0),
                "attn_fwd_mxfp8: bf16 out must be 8-byte aligned rows");
  if (P == 0) return MMSEQ_OK;
  AttnArgs a = attn_args(P, T, T, heads, qkv, ld_qkv, q_off, k_off, v_off, key_bias, scale, drop, keep_bits);
  a.lse = lse; a.o_w = out; a.ld_out = ld_out;
  a.q8 = reinterpret_cast<uint8_t*>(q8); a.ldq8 = ldq8; a.q8s = reinterpret_cast<uint8_t*>(q8_scales);
  launch_fwd(FWD16_Q8, attn_fwd_plan(P, T, T, heads, 1, a.drop.thr != 0, keep_bits != nullptr), a,
             reinterpret_cast<hipStream_t>(stream));
  return mmseq_check_launch("attn_fwd_mxfp8");
}

extern "C" mmseq_status mmseq_attn_fwd_mxfp8(int P, int T, int heads, const void* qkv, int64_t ld_qkv,
                                             int64_t q_off, int64_t k_off, int64_t v_off,
                                             const float* key_bias, float scale, float* lse,
                                             void* q8, int64_t ldq8, void* q8_scales,
                                             mmseq_stream stream) {
  return mmseq_attn_fwd_mxfp8_dual(P, T, heads, qkv, ld_qkv, q_off, k_off, v_off, key_bias, scale,
                                   nullptr, 0, lse, nullptr, nullptr, q8, ldq8, q8_scales, stream);
}
