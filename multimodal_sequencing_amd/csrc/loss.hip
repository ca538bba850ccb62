// Row selection on activations and the fused vocabulary cross-entropy of the text+image
// pretraining stage (lxrt/modeling.py:885-942 PISP row swap, :948-1009 MRM masking, :1157-1173 +
// :2260-2266 masked-LM loss). See include/mmseq.h for the contracts.
//
//   rows_gather  one 16-byte chunk per thread; the backward is a zero fill of din followed by a
//                scatter (src is unique, so plain stores: no atomics, bit-stable).
//   xent_fwd     one workgroup per row: online max / sum in fp32 over 16-byte loads, then one
//                workgroup sums the row losses and counts the kept rows in a fixed order.
//   xent_eval    the forward's kernel instantiated with K >= 0 (same traversal, same bits for lse
//                and the loss): it also ranks the gold word and keeps the K best columns in
//                per-thread sorted register lists, merged by K rounds of "best remaining head".
//   xent_bwd     dlogits over the logits in place; ignored rows and the ld - V padding columns are
//                written as exact zeros, so the buffer feeds the dgrad / wgrad GEMMs as it is.
#include <math.h>

#include <utility>

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

__device__ __forceinline__ int64_t row_off(int64_t r, const mmseq_rows& l) {
  const int64_t q = r / l.rpb;
  return q * l.bstride + (r - q * l.rpb) * l.ld;
}

// ---------------------------------------------------------------------------------------------
// rows gather: cpr = 16-byte chunks per row; in / out addressed in bytes (esz = element size)
__global__ __launch_bounds__(256) void rows_gather_kernel(int64_t nchunks, int cpr, int R_in, int esz,
                                                          const char* __restrict__ in, mmseq_rows inl,
                                                          const int32_t* __restrict__ src,
                                                          const uint8_t* __restrict__ keep,
                                                          char* __restrict__ out, mmseq_rows outl) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nchunks) return;
  const int64_t r = i / cpr;
  const int c = (int)(i - r * cpr);
  u32x4 v = {0u, 0u, 0u, 0u};
  const int s = src[r];
  // an index outside [0, R_in) reads nothing and gives a zero row
  if ((!keep || keep[r]) && (unsigned)s < (unsigned)R_in)
    v = *reinterpret_cast<const u32x4*>(in + row_off(s, inl) * esz + (int64_t)c * 16);
  *reinterpret_cast<u32x4*>(out + row_off(r, outl) * esz + (int64_t)c * 16) = v;
}

__global__ __launch_bounds__(256) void rows_zero_kernel(int64_t nchunks, int cpr, int esz,
                                                        char* __restrict__ out, mmseq_rows outl) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nchunks) return;
  const int64_t r = i / cpr;
  const int c = (int)(i - r * cpr);
  *reinterpret_cast<u32x4*>(out + row_off(r, outl) * esz + (int64_t)c * 16) = (u32x4){0u, 0u, 0u, 0u};
}

__global__ __launch_bounds__(256) void rows_scatter_kernel(int64_t nchunks, int cpr, int R_in, int esz,
                                                           const char* __restrict__ dout,
                                                           mmseq_rows doutl,
                                                           const int32_t* __restrict__ src,
                                                           const uint8_t* __restrict__ keep,
                                                           char* __restrict__ din, mmseq_rows dinl) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nchunks) return;
  const int64_t r = i / cpr;
  const int c = (int)(i - r * cpr);
  const int s = src[r];
  if ((unsigned)s >= (unsigned)R_in) return;  // nothing was read from it in the forward
  u32x4 v = {0u, 0u, 0u, 0u};
  if (!keep || keep[r])
    v = *reinterpret_cast<const u32x4*>(dout + row_off(r, doutl) * esz + (int64_t)c * 16);
  *reinterpret_cast<u32x4*>(din + row_off(s, dinl) * esz + (int64_t)c * 16) = v;
}

inline bool rows_ok(const void* p, const mmseq_rows& l, int esz) {
  const int64_t ve = 16 / esz;
  return ((uintptr_t)p % 16) == 0 && l.ld % ve == 0 && l.bstride % ve == 0;
}

// ---------------------------------------------------------------------------------------------
// cross-entropy. A chunk is 16 bytes: 8 bf16 or 4 fp32 logits.
template <typename T> struct Chunk;
template <> struct Chunk<unsigned short> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void ld(const unsigned short* p, float* x) {
    const u16x8 u = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = bf2f(u[e]);
  }
  static __device__ __forceinline__ void st(unsigned short* p, const float* x) {
    u16x8 u;
#pragma unroll
    for (int e = 0; e < 8; ++e) u[e] = f2bf(x[e]);
    *reinterpret_cast<u16x8*>(p) = u;
  }
};
template <> struct Chunk<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void ld(const float* p, float* x) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = u[e];
  }
  static __device__ __forceinline__ void st(float* p, const float* x) {
    *reinterpret_cast<f32x4*>(p) = (f32x4){x[0], x[1], x[2], x[3]};
  }
};

// (max, sum of exp(x - max)) pairs merge associatively; an empty partial is (-inf, 0)
__device__ __forceinline__ void ms_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) return;  // both empty
  s = s * expf(m - mn) + s2 * expf(m2 - mn);
  m = mn;
}

// evaluation: candidates are ordered by (value descending, column ascending), a total order, so
// the k best do not depend on how the partial lists are merged.
__device__ __forceinline__ bool cand_before(float v, int i, float v2, int i2) {
  return v > v2 || (v == v2 && i < i2);
}

// K candidates in registers, best first. Every index below is a compile-time constant after
// unrolling (a runtime index into a register array would become an indexed move).
template <int K> struct TopK {
  float v[K];
  int i[K];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < K; ++j) { v[j] = -INFINITY; i[j] = -1; }
  }
  // columns arrive in ascending order, so a candidate never precedes an equal value already held:
  // strict > places it behind. -inf (a replaced column) never enters. Branch-free: the K compares
  // are independent (the list is sorted, so they are monotone in j) and every slot picks among
  // itself, its left neighbour and x; a bubble from the tail would be a chain of K - 1 dependent
  // compare-exchanges, with one wave per SIMD nothing hides that latency.
  __device__ __forceinline__ void push(float x, int c) {
    bool gt[K];
#pragma unroll
    for (int j = 0; j < K; ++j) gt[j] = x > v[j];
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
      v[j] = gt[j] ? (gt[j - 1] ? v[j - 1] : x) : v[j];
      i[j] = gt[j] ? (gt[j - 1] ? i[j - 1] : c) : i[j];
    }
    v[0] = gt[0] ? x : v[0];
    i[0] = gt[0] ? c : i[0];
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int j = 0; j + 1 < K; ++j) { v[j] = v[j + 1]; i[j] = i[j + 1]; }
    v[K - 1] = -INFINITY;
    i[K - 1] = -1;
  }
};

// One traversal, two uses. K < 0 is the forward (mmseq_xent_fwd): every evaluation statement is
// discarded at compile time and rank / topk_* are unused. K >= 0 is the evaluation
// (mmseq_xent_eval): the same chunk order and the same wave-then-workgroup merge, so lse and
// loss_row get the same bits, plus the gold word's rank and the K best columns.
template <typename T, int K>
__global__ __launch_bounds__(256) void xent_fwd_kernel(int V, const T* __restrict__ logits, int64_t ld,
                                                       const int64_t* __restrict__ labels,
                                                       int64_t ignore_index, float* __restrict__ lse,
                                                       float* __restrict__ loss_row,
                                                       int32_t* __restrict__ rank,
                                                       int32_t* __restrict__ topk_idx,
                                                       float* __restrict__ topk_logit) {
  constexpr int CN = Chunk<T>::N;
  constexpr bool EVAL = K >= 0;
  __shared__ float sm[4], ss[4];
  const int row = blockIdx.x;
  const T* x = logits + (int64_t)row * ld;
  // evaluation: the gold logit is one broadcast read before the sweep; without a usable label
  // +inf counts nothing. `ahead`: columns that precede the gold one in the candidate order.
  __shared__ float hv[EVAL ? 2 : 1][4];
  __shared__ int sc[4], hi[EVAL ? 2 : 1][4];
  float gold = INFINITY;
  int glab = 0, ahead = 0;
  bool gold_ok = false;
  TopK<(K > 0 ? K : 1)> top;
  if constexpr (EVAL) {
    const int64_t lab = labels[row];
    gold_ok = lab != ignore_index && lab >= 0 && lab < V;
    if (gold_ok) { gold = Elem<T>::ld(x + lab); glab = (int)lab; }
    top.clear();
  }
  float m = -INFINITY, s = 0.f;
  // chunks that start below V; columns >= V inside the last one are loaded (they are inside the
  // row: ld >= V rounded up to the chunk) and replaced before anything is computed from them
  for (int c0 = threadIdx.x * CN; c0 < V; c0 += 256 * CN) {
    float v[CN];
    Chunk<T>::ld(x + c0, v);
    float cm = -INFINITY;
#pragma unroll
    for (int e = 0; e < CN; ++e) {
      if (c0 + e >= V) v[e] = -INFINITY;
      cm = fmaxf(cm, v[e]);
    }
    const float mn = fmaxf(m, cm);
    float cs = 0.f;
#pragma unroll
    for (int e = 0; e < CN; ++e) cs += expf(v[e] - mn);  // exp(-inf) = 0 for the replaced ones
    s = (m == -INFINITY ? 0.f : s * expf(m - mn)) + cs;
    m = mn;
    if constexpr (EVAL) {
#pragma unroll
      for (int e = 0; e < CN; ++e) {
        ahead += cand_before(v[e], c0 + e, gold, glab) ? 1 : 0;
        if constexpr (K > 0) top.push(v[e], c0 + e);
      }
    }
  }
  // wave, then workgroup, in a fixed order
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    ms_merge(m, s, m2, s2);
  }
  if constexpr (EVAL) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ahead += __shfl_xor(ahead, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sm[wave] = m;
    ss[wave] = s;
    if constexpr (EVAL) sc[wave] = ahead;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0], S = ss[0];
    for (int w = 1; w < 4; ++w) ms_merge(M, S, sm[w], ss[w]);
    const float l = M + logf(S);
    lse[row] = l;
    const int64_t lab = labels[row];
    float loss = 0.f;
    if (lab != ignore_index)  // a label outside [0, V) reads nothing and gives a NaN loss
      loss = (lab >= 0 && lab < V) ? l - Elem<T>::ld(x + lab) : NAN;
    loss_row[row] = loss;
    if constexpr (EVAL) rank[row] = gold_ok ? sc[0] + sc[1] + sc[2] + sc[3] : -1;
  }
  if constexpr (K > 0) {
    // K rounds of "best remaining head" over the 256 lists; the two buffers alternate, so one
    // barrier per round is enough
#pragma unroll
    for (int r = 0; r < K; ++r) {
      float bv = top.v[0];
      int bi = top.i[0];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (cand_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      if (lane == 0) { hv[r & 1][wave] = bv; hi[r & 1][wave] = bi; }
      __syncthreads();
      bv = hv[r & 1][0];
      bi = hi[r & 1][0];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        const float ov = hv[r & 1][w];
        const int oi = hi[r & 1][w];
        if (cand_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      // columns are unique over the threads: exactly one list holds the winner. bi < 0: every
      // list is empty (K > V) and the entry is (-1, -inf)
      if (bi >= 0 && top.i[0] == bi) top.pop();
      if (threadIdx.x == 0) {
        topk_idx[(int64_t)row * K + r] = bi;
        topk_logit[(int64_t)row * K + r] = bv;
      }
    }
  }
}

// totals[0..3] += (sum of loss_row over the kept rows, kept rows, rows with rank 0, rows with
// 0 <= rank < k), in double and in a fixed order
__global__ __launch_bounds__(256) void xent_totals_kernel(int M, int k,
                                                          const float* __restrict__ loss_row,
                                                          const int64_t* __restrict__ labels,
                                                          int64_t ignore_index,
                                                          const int32_t* __restrict__ rank,
                                                          double* __restrict__ totals) {
  __shared__ double ps[256];
  __shared__ int pc[3][256];
  double s = 0.0;
  int kept = 0, first = 0, ink = 0;
  for (int r = threadIdx.x; r < M; r += 256) {
    if (labels[r] != ignore_index) { s += (double)loss_row[r]; ++kept; }
    const int q = rank[r];
    first += q == 0 ? 1 : 0;
    ink += (q >= 0 && q < k) ? 1 : 0;
  }
  ps[threadIdx.x] = s;
  pc[0][threadIdx.x] = kept;
  pc[1][threadIdx.x] = first;
  pc[2][threadIdx.x] = ink;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
      ps[threadIdx.x] += ps[threadIdx.x + o];
#pragma unroll
      for (int j = 0; j < 3; ++j) pc[j][threadIdx.x] += pc[j][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    totals[0] += ps[0];
    totals[1] += (double)pc[0][0];
    totals[2] += (double)pc[1][0];
    totals[3] += (double)pc[2][0];
  }
}

// out[0] = sum(loss_row) / count, out[1] = count (kept rows), summed in a fixed order
__global__ __launch_bounds__(256) void xent_mean_kernel(int M, const float* __restrict__ loss_row,
                                                        const int64_t* __restrict__ labels,
                                                        int64_t ignore_index, float* __restrict__ out) {
  __shared__ float ps[256];
  __shared__ int pc[256];
  float s = 0.f;
  int c = 0;
  for (int r = threadIdx.x; r < M; r += 256) {
    if (labels[r] != ignore_index) { s += loss_row[r]; ++c; }
  }
  ps[threadIdx.x] = s;
  pc[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) {
      ps[threadIdx.x] += ps[threadIdx.x + o];
      pc[threadIdx.x] += pc[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = ps[0] / (float)pc[0];  // 0 / 0 = NaN with no kept row, as torch's mean reduction
    out[1] = (float)pc[0];
  }
}

constexpr int BWD_SEG = 256 * 8 * 4;  // columns per workgroup of the backward (any dtype)

template <typename T>
__global__ __launch_bounds__(256) void xent_bwd_kernel(int V, T* __restrict__ logits, int64_t ld,
                                                       const int64_t* __restrict__ labels,
                                                       int64_t ignore_index,
                                                       const float* __restrict__ lse,
                                                       const float* __restrict__ stats,
                                                       const float* __restrict__ g) {
  constexpr int CN = Chunk<T>::N;
  const int row = blockIdx.x;
  T* x = logits + (int64_t)row * ld;
  const int64_t lab = labels[row];
  const bool kept = lab != ignore_index;
  const float l = lse[row];
  const float scale = kept ? (g ? g[0] : 1.f) / stats[1] : 0.f;
  const int seg0 = blockIdx.y * BWD_SEG;
  const int seg1 = seg0 + BWD_SEG < (int)ld ? seg0 + BWD_SEG : (int)ld;
  for (int c0 = seg0 + threadIdx.x * CN; c0 < seg1; c0 += 256 * CN) {
    float v[CN];
    if (kept && c0 < V) {
      Chunk<T>::ld(x + c0, v);
#pragma unroll
      for (int e = 0; e < CN; ++e) {
        const int c = c0 + e;
        v[e] = c < V ? (expf(v[e] - l) - (c == lab ? 1.f : 0.f)) * scale : 0.f;
      }
    } else {
#pragma unroll
      for (int e = 0; e < CN; ++e) v[e] = 0.f;
    }
    Chunk<T>::st(x + c0, v);
  }
}

inline bool xent_ok(const void* p, int V, int64_t ld, int esz) {
  const int64_t ve = 16 / esz;
  return ((uintptr_t)p % 16) == 0 && ld % ve == 0 && ld >= V && ld < ((int64_t)1 << 31);
}

}  // namespace

extern "C" mmseq_status mmseq_rows_gather_fwd(int R_out, int R_in, int cols, const void* in,
                                              mmseq_rows inl, const int32_t* src,
                                              const uint8_t* keep, void* out, mmseq_rows outl,
                                              mmseq_dtype dtype, mmseq_stream stream) {
  MMSEQ_REQUIRE(R_out >= 0 && R_in >= 0 && cols >= 0, "rows_gather_fwd: bad sizes");
  MMSEQ_REQUIRE(dtype == MMSEQ_F32 || dtype == MMSEQ_BF16, "rows_gather_fwd: bad dtype");
  MMSEQ_REQUIRE(inl.rpb > 0 && outl.rpb > 0, "rows_gather_fwd: rpb must be > 0");
  if (R_out == 0 || cols == 0) return MMSEQ_OK;
  MMSEQ_REQUIRE(in && src && out, "rows_gather_fwd: null operand");
  const int esz = dtype == MMSEQ_BF16 ? 2 : 4;
  if (cols % 8 != 0 || !rows_ok(in, inl, esz) || !rows_ok(out, outl, esz))
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "rows_gather_fwd: cols %% 8 == 0 and 16-byte aligned rows only (cols=%d)",
                           cols);
  const int cpr = cols * esz / 16;
  const int64_t n = (int64_t)R_out * cpr;
  hipLaunchKernelGGL(rows_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), n, cpr, R_in, esz, (const char*)in, inl,
                     src, keep, (char*)out, outl);
  return mmseq_check_launch("rows_gather_fwd");
}

extern "C" mmseq_status mmseq_rows_gather_bwd(int R_out, int R_in, int cols, const void* dout,
                                              mmseq_rows doutl, const int32_t* src,
                                              const uint8_t* keep, void* din, mmseq_rows dinl,
                                              mmseq_dtype dtype, mmseq_stream stream) {
  MMSEQ_REQUIRE(R_out >= 0 && R_in >= 0 && cols >= 0, "rows_gather_bwd: bad sizes");
  MMSEQ_REQUIRE(dtype == MMSEQ_F32 || dtype == MMSEQ_BF16, "rows_gather_bwd: bad dtype");
  MMSEQ_REQUIRE(dinl.rpb > 0 && doutl.rpb > 0, "rows_gather_bwd: rpb must be > 0");
  if (R_in == 0 || cols == 0) return MMSEQ_OK;
  MMSEQ_REQUIRE(din && (R_out == 0 || (dout && src)), "rows_gather_bwd: null operand");
  const int esz = dtype == MMSEQ_BF16 ? 2 : 4;
  if (cols % 8 != 0 || !rows_ok(din, dinl, esz) || (R_out && !rows_ok(dout, doutl, esz)))
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "rows_gather_bwd: cols %% 8 == 0 and 16-byte aligned rows only (cols=%d)",
                           cols);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int cpr = cols * esz / 16;
  const int64_t nz = (int64_t)R_in * cpr, n = (int64_t)R_out * cpr;
  hipLaunchKernelGGL(rows_zero_kernel, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, s, nz, cpr,
                     esz, (char*)din, dinl);
  if (n)
    hipLaunchKernelGGL(rows_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n,
                       cpr, R_in, esz, (const char*)dout, doutl, src, keep, (char*)din, dinl);
  return mmseq_check_launch("rows_gather_bwd");
}

extern "C" mmseq_status mmseq_xent_fwd(int M, int V, const void* logits, int64_t ld,
                                       const int64_t* labels, int64_t ignore_index, float* lse,
                                       float* loss_row, float* stats, mmseq_dtype dtype,
                                       mmseq_stream stream) {
  MMSEQ_REQUIRE(M >= 0 && V >= 1, "xent_fwd: bad sizes M=%d V=%d", M, V);
  MMSEQ_REQUIRE(dtype == MMSEQ_F32 || dtype == MMSEQ_BF16, "xent_fwd: bad dtype");
  MMSEQ_REQUIRE(stats && (M == 0 || (logits && labels && lse && loss_row)), "xent_fwd: null operand");
  const int esz = dtype == MMSEQ_BF16 ? 2 : 4;
  if (M && !xent_ok(logits, V, ld, esz))
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "xent_fwd: 16-byte aligned rows with ld >= V only (V=%d ld=%lld)", V,
                           (long long)ld);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (M) {
    if (dtype == MMSEQ_BF16)
      hipLaunchKernelGGL((xent_fwd_kernel<unsigned short, -1>), dim3(M), dim3(256), 0, s, V,
                         (const unsigned short*)logits, ld, labels, ignore_index, lse, loss_row,
                         (int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr);
    else
      hipLaunchKernelGGL((xent_fwd_kernel<float, -1>), dim3(M), dim3(256), 0, s, V,
                         (const float*)logits, ld, labels, ignore_index, lse, loss_row,
                         (int32_t*)nullptr, (int32_t*)nullptr, (float*)nullptr);
  }
  hipLaunchKernelGGL(xent_mean_kernel, dim3(1), dim3(256), 0, s, M, loss_row, labels, ignore_index,
                     stats);
  return mmseq_check_launch("xent_fwd");
}

extern "C" mmseq_status mmseq_xent_mean(int M, const float* loss_row, const int64_t* labels,
                                        int64_t ignore_index, float* stats, mmseq_stream stream) {
  MMSEQ_REQUIRE(M >= 0, "xent_mean: bad size M=%d", M);
  MMSEQ_REQUIRE(stats && (M == 0 || (loss_row && labels)), "xent_mean: null operand");
  hipLaunchKernelGGL(xent_mean_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     M, loss_row, labels, ignore_index, stats);
  return mmseq_check_launch("xent_mean");
}

namespace {

template <typename T, int K>
void xent_eval_launch(int M, int V, const void* logits, int64_t ld, const int64_t* labels,
                      int64_t ignore_index, float* lse, float* loss_row, int32_t* rank,
                      int32_t* topk_idx, float* topk_logit, hipStream_t s) {
  hipLaunchKernelGGL((xent_fwd_kernel<T, K>), dim3(M), dim3(256), 0, s, V, (const T*)logits, ld,
                     labels, ignore_index, lse, loss_row, rank, topk_idx, topk_logit);
}

template <typename T, int... Ks>
void xent_eval_pick(std::integer_sequence<int, Ks...>, int k, int M, int V, const void* logits,
                    int64_t ld, const int64_t* labels, int64_t ignore_index, float* lse,
                    float* loss_row, int32_t* rank, int32_t* topk_idx, float* topk_logit,
                    hipStream_t s) {
  // one instantiation per k: the candidate lists are register arrays of exactly k entries
  ((k == Ks ? xent_eval_launch<T, Ks>(M, V, logits, ld, labels, ignore_index, lse, loss_row, rank,
                                      topk_idx, topk_logit, s)
            : (void)0),
   ...);
}

}  // namespace

extern "C" mmseq_status mmseq_xent_eval(int M, int V, const void* logits, int64_t ld,
                                        const int64_t* labels, int64_t ignore_index, int k,
                                        float* lse, float* loss_row, int32_t* rank,
                                        int32_t* topk_idx, float* topk_logit, double* totals,
                                        mmseq_dtype dtype, mmseq_stream stream) {
  MMSEQ_REQUIRE(M >= 0 && V >= 1, "xent_eval: bad sizes M=%d V=%d", M, V);
  MMSEQ_REQUIRE(k >= 0 && k <= MMSEQ_XENT_EVAL_MAX_K, "xent_eval: k=%d outside [0, %d]", k,
                MMSEQ_XENT_EVAL_MAX_K);
  MMSEQ_REQUIRE(dtype == MMSEQ_F32 || dtype == MMSEQ_BF16, "xent_eval: bad dtype");
  if (M == 0) return MMSEQ_OK;
  MMSEQ_REQUIRE(logits && labels && lse && loss_row && rank, "xent_eval: null operand");
  MMSEQ_REQUIRE(k == 0 || (topk_idx && topk_logit), "xent_eval: null top-k output with k=%d", k);
  const int esz = dtype == MMSEQ_BF16 ? 2 : 4;
  if (!xent_ok(logits, V, ld, esz))
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "xent_eval: 16-byte aligned rows with ld >= V only (V=%d ld=%lld)", V,
                           (long long)ld);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const auto ks = std::make_integer_sequence<int, MMSEQ_XENT_EVAL_MAX_K + 1>();
  if (dtype == MMSEQ_BF16)
    xent_eval_pick<unsigned short>(ks, k, M, V, logits, ld, labels, ignore_index, lse, loss_row,
                                   rank, topk_idx, topk_logit, s);
  else
    xent_eval_pick<float>(ks, k, M, V, logits, ld, labels, ignore_index, lse, loss_row, rank,
                          topk_idx, topk_logit, s);
  if (totals)
    hipLaunchKernelGGL(xent_totals_kernel, dim3(1), dim3(256), 0, s, M, k, loss_row, labels,
                       ignore_index, rank, totals);
  return mmseq_check_launch("xent_eval");
}

extern "C" mmseq_status mmseq_xent_bwd(int M, int V, void* logits, int64_t ld, const int64_t* labels,
                                       int64_t ignore_index, const float* lse, const float* stats,
                                       const float* g, mmseq_dtype dtype, mmseq_stream stream) {
  MMSEQ_REQUIRE(M >= 0 && V >= 1, "xent_bwd: bad sizes M=%d V=%d", M, V);
  MMSEQ_REQUIRE(dtype == MMSEQ_F32 || dtype == MMSEQ_BF16, "xent_bwd: bad dtype");
  if (M == 0) return MMSEQ_OK;
  MMSEQ_REQUIRE(logits && labels && lse && stats, "xent_bwd: null operand");
  const int esz = dtype == MMSEQ_BF16 ? 2 : 4;
  if (!xent_ok(logits, V, ld, esz))
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "xent_bwd: 16-byte aligned rows with ld >= V only (V=%d ld=%lld)", V,
                           (long long)ld);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(M, (unsigned)((ld + BWD_SEG - 1) / BWD_SEG));
  if (dtype == MMSEQ_BF16)
    hipLaunchKernelGGL(xent_bwd_kernel<unsigned short>, grid, dim3(256), 0, s, V,
                       (unsigned short*)logits, ld, labels, ignore_index, lse, stats, g);
  else
    hipLaunchKernelGGL(xent_bwd_kernel<float>, grid, dim3(256), 0, s, V, (float*)logits, ld, labels,
                       ignore_index, lse, stats, g);
  return mmseq_check_launch("xent_bwd");
}
