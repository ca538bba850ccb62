// mmseq_order_score_bwd: the gradient of mmseq_order_score's K scores per story with respect to
// the encoder output (doc, okey, hist, h0, c0) and the nine decoder weights, for sequence-level
// losses over a candidate list (include/mmseq.h).
//
// The entry recomputes the scorer's forward itself (the ABI keeps no state between calls) through
// pointer_decoder.h's setup and step, the code the scorer runs: R = B*K slots that never branch.
// It keeps h_t, c_t and the gate activations of every step in its workspace and then runs
//   1. one launch over all (slot, step): e, softmax, de, dA = de w_t (1 - a^2) per key, dq, and
//      the slot's partial rows of dw_t / db_t (a step's pointer part depends on the LSTM chain
//      only through q_t, so the steps need no order here),
//   2. the LSTM chain backwards, t = N-2 .. 0, two small GEMMs and one cell kernel per step,
//   3. GATHERS to the per-story rows: one workgroup per destination row (dGX[b][i], dokey[b][j],
//      dPROJ[g][b][i][j]) loops k ascending, then t ascending, and decides membership from the
//      slot's seq row. Nothing is scattered and there is no atomic anywhere: every sum has one
//      owner and one order, so two calls give the same bits,
//   4. the dense parts through mmseq_gemm / mmseq_gemm_wgrad (fp32, fixed-order split-K).
#include "pointer_decoder.h"

namespace {

constexpr int OG_CS_ROWS = 64;        // rows per partial of the two-level column sum
constexpr int64_t OG_SLAB = 1 << 20;  // floats of split-K scratch handed to the GEMMs

struct GradWs {  // float offsets, each a multiple of 4
  int64_t gx, proj, hs, cs, gates, q, dA, wpart, dh, dc, csum, slab, seq, bad, total;
  int64_t pstride;
};

GradWs grad_layout(int B, int N, int H, int K) {
  GradWs w;
  const int64_t R = (int64_t)B * K, T = N - 1;
  int64_t o = 0;
  w.pstride = up4((int64_t)B * N * N * H);
  w.gx = o; o += up4((int64_t)B * N * 4 * H);     // GX, later dGX
  w.proj = o; o += 4 * w.pstride;                 // PROJ, later dPROJ
  w.hs = o; o += up4((T + 1) * R * H);            // h_0 (= h0) .. h_T per slot
  w.cs = o; o += up4((T + 1) * R * H);
  w.gates = o; o += up4(T * R * 4 * H);           // gate activations, later dgates
  w.q = o; o += up4(T * R * H);                   // q_t, later dq_t
  w.dA = o; o += up4(T * R * N * H);              // a_t[j], later dA_t[j]
  w.wpart = o; o += up4(T * R * (H + 1));         // per (step, slot): dw_t partial [H], db_t [1]
  w.dh = o; o += up4(R * H);
  w.dc = o; o += up4(R * H);
  w.csum = o; o += up4((T * R + OG_CS_ROWS - 1) / OG_CS_ROWS * 4 * H);
  w.slab = o; o += OG_SLAB;
  w.seq = o; o += up4(R * BEAM_MAXN);               // int32 picks
  w.bad = o; o += up4(R);                         // int32, 1 = invalid candidate
  w.total = o;
  return w;
}

// mmseq_order_score's limits (every offset into the stacked per-step rows is 64-bit)
inline bool grad_supported(int B, int N, int H, int K) {
  if (!(B >= 0 && N >= 1 && N <= BEAM_MAXN && H >= 1 && K >= 1)) return false;
  if (!((int64_t)B * 32 * BEAM_MAXN * 4 < INT32_MAX / 2 && (int64_t)H * 4 * 4 < INT32_MAX / 2))
    return false;
  return (int64_t)B * K * 4 * H < INT32_MAX && (int64_t)B * K * BEAM_MAXN < INT32_MAX;
}

// One workgroup per slot (story b, candidate k): the candidate is validated before any of its
// entries forms an address (an invalid one runs as 0, 1, .., N-2 and is marked bad), h_0 / c_0
// rows <- (h0, c0).
__global__ __launch_bounds__(256) void og_init_kernel(int N, int H, int K,
                                                      const int64_t* __restrict__ orders,
                                                      int64_t story_stride,
                                                      const float* __restrict__ h0,
                                                      const float* __restrict__ c0,
                                                      float* __restrict__ h, float* __restrict__ c,
                                                      int* __restrict__ seq, int* __restrict__ bad) {
  const int64_t slot = blockIdx.x;
  const int b = (int)(slot / K), k = (int)(slot % K);
  const int64_t* cand = orders + (int64_t)b * story_stride + (int64_t)k * N;
  const bool ok = candidate_ok(cand, N);
  const int p = threadIdx.x;
  if (p < BEAM_MAXN) seq[slot * BEAM_MAXN + p] = p < N - 1 ? (ok ? (int)cand[p] : p) : 0;
  if (threadIdx.x == 0) bad[slot] = ok ? 0 : 1;
  for (int u = threadIdx.x; u < H; u += 256) {
    h[slot * H + u] = h0[(int64_t)b * H + u];
    c[slot * H + u] = c0[(int64_t)b * H + u];
  }
}

// The cell of step t that keeps its state: `g4` enters as h W_hh^T + b_hh and leaves
// as the gate activations (i, f, g, o); (h, c) of step t -> rows of step t + 1.
__global__ __launch_bounds__(256) void og_cell_kernel(int H, int K, int N, int t,
                                                      const float* __restrict__ gx,
                                                      const float* __restrict__ b_ih,
                                                      const int* __restrict__ seq,
                                                      float* __restrict__ g4all,
                                                      const float* __restrict__ c_in,
                                                      float* __restrict__ h_out,
                                                      float* __restrict__ c_out) {
  const int64_t slot = blockIdx.x;
  const int b = (int)(slot / K);
  const float* x = t > 0 ? gx + ((int64_t)b * N + seq[slot * BEAM_MAXN + t - 1]) * 4 * H : b_ih;
  float* g4 = g4all + slot * 4 * H;
  for (int u = threadIdx.x; u < H; u += 256) {
    const LstmCell r = lstm_cell(x, g4, H, u, c_in + slot * H + u);
    g4[u] = r.i; g4[H + u] = r.f; g4[2 * H + u] = r.g; g4[3 * H + u] = r.o;
    c_out[slot * H + u] = r.c2;
    h_out[slot * H + u] = r.h;
  }
}

// One workgroup per (step t, slot). First beam_score_kernel's forward (one wave per key j, the
// same sums in the same order: the loop is kept as a second copy) with
// a_t[j] = tanh(q + key + okey) kept in the dA rows; then
//   de[j] = G (p[j] - [j = y_t]) for j not pointed, exactly 0 where pointed (G = 0 for a bad slot)
//           with p[y_t] - 1 taken as -sum_{j != y_t} p[j]
//   dA[j][u] = de[j] w_t[u] (1 - a[j][u]^2),  dq[u] = sum_j dA[j][u] (j ascending, over q in place)
//   wpart[u] = sum_j de[j] a[j][u],  wpart[H] = sum_j de[j] (the others ascending, then the pick)
// one thread per column u in the second half.
__global__ __launch_bounds__(256) void og_score_bwd_kernel(int N, int H, int K, int64_t R,
                                                           float* __restrict__ q,
                                                           const float* __restrict__ proj,
                                                           int64_t proj_stride,
                                                           const float* __restrict__ okey,
                                                           const float* __restrict__ wt,
                                                           const float* __restrict__ bt,
                                                           const int* __restrict__ seq,
                                                           const int* __restrict__ bad,
                                                           const float* __restrict__ dnll,
                                                           float* __restrict__ dA,
                                                           float* __restrict__ wpart) {
  __shared__ float e[BEAM_MAXN];
  const int64_t row = blockIdx.x;  // t * R + slot
  const int t = (int)(row / R);
  const int64_t slot = row % R;
  const int b = (int)(slot / K);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned pointed = 0;
  for (int p = 0; p < t; ++p) pointed |= 1u << seq[slot * BEAM_MAXN + p];
  const int l1 = t > 0 ? seq[slot * BEAM_MAXN + t - 1] : 0;
  const int l2 = t > 1 ? seq[slot * BEAM_MAXN + t - 2] : 0;
  const int y = seq[slot * BEAM_MAXN + t];
  const float* P1 = proj;
  const float* P2 = proj + proj_stride;
  const float* PF = proj + 2 * proj_stride;
  const float* PB = proj + 3 * proj_stride;
  const int64_t sb = (int64_t)b * N;
  float* qr = q + row * H;
  float* ar = dA + row * N * H;
  const float fN = (float)N;
  for (int j = wave; j < N; j += 4) {
    const float* orow = okey + (sb + j) * H;
    const bool jlive = !((pointed >> j) & 1u);
    float acc = 0.f;
    for (int u = lane; u < H; u += 64) {
      float key = 0.f;
      if (t > 0) key += P1[((sb + l1) * N + j) * H + u];
      if (t > 1) key += P2[((sb + l2) * N + j) * H + u];
      if (jlive) {
        float f = 0.f, bk = 0.f;
        for (int i = 0; i < N; ++i) {
          if (i == j || ((pointed >> i) & 1u)) continue;
          f += PF[((sb + j) * N + i) * H + u];
          bk += PB[((sb + i) * N + j) * H + u];
        }
        key += f / fN;
        key += bk / fN;
      }
      const float a = tanhf(qr[u] + key + orow[u]);
      ar[(int64_t)j * H + u] = a;
      acc += wt[u] * a;
    }
    acc = wave_sum(acc);
    if (lane == 0) e[j] = jlive ? acc + bt[0] : -1e9f;
  }
  __syncthreads();  // e[] and the a rows (global, written by this workgroup) are visible
  float mx = -INFINITY;
  for (int j = 0; j < N; ++j) mx = fmaxf(mx, e[j]);
  float sum = 0.f;
  for (int j = 0; j < N; ++j) sum += expf(e[j] - mx);
  const float G = bad[slot] ? 0.f : dnll[slot];
  // de of the pick as minus the sum of the others (p_y - 1 = -sum_{j != y} p_j): no cancellation
  // where p_y is close to 1, and the step's logit gradients sum to zero as they do analytically
  float de[BEAM_MAXN];
  float others = 0.f;
#pragma unroll
  for (int j = 0; j < BEAM_MAXN; ++j) {
    const bool live = j < N && j != y && !((pointed >> j) & 1u);
    de[j] = live ? G * (expf(e[j] - mx) / sum) : 0.f;
    others += de[j];
  }
#pragma unroll
  for (int j = 0; j < BEAM_MAXN; ++j)
    if (j == y) de[j] = -others;
  float* wp = wpart + row * (H + 1);
  for (int u = threadIdx.x; u < H; u += 256) {
    const float w = wt[u];
    float dq = 0.f, dw = 0.f;
#pragma unroll
    for (int j = 0; j < BEAM_MAXN; ++j) {
      if (j < N) {
        const float a = ar[(int64_t)j * H + u];
        dw += de[j] * a;
        const float d = de[j] * w * (1.f - a * a);
        ar[(int64_t)j * H + u] = d;
        dq += d;
      }
    }
    qr[u] = dq;
    wp[u] = dw;
  }
  if (threadIdx.x == 0) {
    float db = 0.f;  // the others ascending, then the pick
#pragma unroll
    for (int j = 0; j < BEAM_MAXN; ++j) db += j == y ? 0.f : de[j];
#pragma unroll
    for (int j = 0; j < BEAM_MAXN; ++j) db += j == y ? de[j] : 0.f;
    wp[H] = db;
  }
}

// mmseq_lstm_cell_bwd's math on R rows, in place: act -> dgates, dc (NULL = zero) -> dc_prev
__global__ __launch_bounds__(256) void og_cell_bwd_kernel(int64_t n, int H, float* __restrict__ act,
                                                          const float* __restrict__ c,
                                                          const float* __restrict__ c_out,
                                                          const float* __restrict__ dh,
                                                          const float* dc_in, float* dc_out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int64_t r = idx / H;
  const int u = (int)(idx - r * H);
  float* a = act + r * 4 * H;
  const LstmCellGrad d = lstm_cell_bwd(a[u], a[H + u], a[2 * H + u], a[3 * H + u], c[idx],
                                       c_out[idx], dh[idx], dc_in ? dc_in[idx] : 0.f);
  a[u] = d.di;
  a[H + u] = d.df;
  a[2 * H + u] = d.dg;
  a[3 * H + u] = d.d_o;
  dc_out[idx] = d.dc_prev;
}

// One workgroup per story: dh0[b] = sum_k dh[b, k], dc0 likewise, k ascending.
__global__ __launch_bounds__(256) void og_gather_state_kernel(int H, int K,
                                                              const float* __restrict__ dh,
                                                              const float* __restrict__ dc,
                                                              float* __restrict__ dh0,
                                                              float* __restrict__ dc0) {
  const int64_t b = blockIdx.x;
  for (int u = threadIdx.x; u < H; u += 256) {
    float sh = 0.f, sc = 0.f;
    for (int k = 0; k < K; ++k) {
      sh += dh[(b * K + k) * H + u];
      sc += dc[(b * K + k) * H + u];
    }
    dh0[b * H + u] = sh;
    dc0[b * H + u] = sc;
  }
}

// One workgroup per GX row (b, i): dGX[b][i] = sum of dgates_t[b, k] over (k, t >= 1) with
// y_{t-1} = i, k ascending then t ascending.
__global__ __launch_bounds__(256) void og_gather_gx_kernel(int N, int H, int K, int64_t R,
                                                           const int* __restrict__ seq,
                                                           const float* __restrict__ dgates,
                                                           float* __restrict__ dgx) {
  const int64_t bi = blockIdx.x;
  const int b = (int)(bi / N), i = (int)(bi % N);
  const int H4 = 4 * H;
  for (int u = threadIdx.x; u < H4; u += 256) {
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
      const int64_t slot = (int64_t)b * K + k;
      for (int t = 1; t < N - 1; ++t)
        if (seq[slot * BEAM_MAXN + t - 1] == i) acc += dgates[((int64_t)t * R + slot) * H4 + u];
    }
    dgx[bi * H4 + u] = acc;
  }
}

// One workgroup per (b, i, j): over k ascending, t ascending, with v = dA_t[b, k][j]
//   dP0[b][i][j] = sum v where l1 = i (t >= 1),   dP1[b][i][j] = sum v where l2 = i (t >= 2)
//   m = (sum v where i != j and neither is pointed at t) / N -> dP3[b][i][j] and dP2[b][j][i]
//   i == j: dokey[b][j] = sum of every v
// (a pointed j has dA = 0 exactly, so its rows add zeros). Every element has this one writer.
__global__ __launch_bounds__(256) void og_gather_key_kernel(int N, int H, int K, int64_t R,
                                                            const int* __restrict__ seq,
                                                            const float* __restrict__ dA,
                                                            float* __restrict__ dproj,
                                                            int64_t proj_stride,
                                                            float* __restrict__ dokey) {
  const int64_t bij = blockIdx.x;
  const int j = (int)(bij % N), i = (int)(bij / N % N);
  const int64_t b = bij / ((int64_t)N * N);
  const float fN = (float)N;
  for (int u = threadIdx.x; u < H; u += 256) {
    float p0 = 0.f, p1 = 0.f, m = 0.f, all = 0.f;
    for (int k = 0; k < K; ++k) {
      const int64_t slot = b * K + k;
      const int* sq = seq + slot * BEAM_MAXN;
      unsigned pointed = 0;
      for (int t = 0; t < N - 1; ++t) {
        const bool c0 = t > 0 && sq[t - 1] == i;
        const bool c1 = t > 1 && sq[t - 2] == i;
        const bool cm = i != j && !((pointed >> i) & 1u) && !((pointed >> j) & 1u);
        if (c0 || c1 || cm || i == j) {
          const float v = dA[(((int64_t)t * R + slot) * N + j) * H + u];
          if (c0) p0 += v;
          if (c1) p1 += v;
          if (cm) m += v;
          all += v;
        }
        pointed |= 1u << sq[t];
      }
    }
    m = m / fN;
    dproj[bij * H + u] = p0;
    dproj[proj_stride + bij * H + u] = p1;
    dproj[2 * proj_stride + ((b * N + j) * N + i) * H + u] = m;
    dproj[3 * proj_stride + bij * H + u] = m;
    if (i == j) dokey[(b * N + j) * H + u] = all;
  }
}

// Two-level column sum in a fixed order: part[c][col] = sum of OG_CS_ROWS rows, then
// out[col] += sum_c part[c][col], c ascending.
__global__ __launch_bounds__(256) void og_colsum_part_kernel(int64_t rows, int cols,
                                                             const float* __restrict__ x,
                                                             int64_t ldx, float* __restrict__ part) {
  const int ncb = (cols + 255) / 256;  // column blocks per chunk of rows
  const int64_t chunk = blockIdx.x / ncb;
  const int col = (int)(blockIdx.x % ncb) * 256 + threadIdx.x;
  if (col >= cols) return;
  const int64_t r0 = chunk * OG_CS_ROWS;
  const int64_t r1 = r0 + OG_CS_ROWS < rows ? r0 + OG_CS_ROWS : rows;
  float v = 0.f;
  for (int64_t r = r0; r < r1; ++r) v += x[r * ldx + col];
  part[chunk * cols + col] = v;
}
__global__ __launch_bounds__(256) void og_colsum_final_kernel(int64_t chunks, int cols,
                                                              const float* __restrict__ part,
                                                              float* __restrict__ out,
                                                              float* __restrict__ out2) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= cols) return;
  float v = 0.f;
  for (int64_t c = 0; c < chunks; ++c) v += part[c * cols + col];
  out[col] += v;
  if (out2) out2[col] += v;
}

mmseq_status og_colsum(int64_t rows, int cols, const float* x, int64_t ldx, float* part, float* out,
                       float* out2, hipStream_t st) {
  const int64_t chunks = (rows + OG_CS_ROWS - 1) / OG_CS_ROWS;
  hipLaunchKernelGGL(og_colsum_part_kernel, dim3((unsigned)(chunks * ((cols + 255) / 256))), dim3(256), 0,
                     st, rows, cols, x, ldx, part);
  mmseq_status e = mmseq_check_launch("order_score_bwd colsum");
  if (e != MMSEQ_OK) return e;
  hipLaunchKernelGGL(og_colsum_final_kernel, dim3((cols + 255) / 256), dim3(256), 0, st, chunks,
                     cols, part, out, out2);
  return mmseq_check_launch("order_score_bwd colsum");
}

mmseq_status og_wgrad(int M, int Nn, int K, const float* A, int64_t lda, const float* Bm,
                      int64_t ldb, float* C, int64_t ldc, GemmSlab slab, mmseq_stream stream) {
  return mmseq_gemm_wgrad(M, Nn, K, A, lda, Bm, ldb, C, ldc, nullptr, MMSEQ_F32, MMSEQ_GEMM_AUTO,
                          slab.ptr, slab.bytes, stream);
}

}  // namespace

extern "C" int64_t mmseq_order_score_bwd_workspace(int B, int N, int H, int K) {
  if (!grad_supported(B, N, H, K)) return 0;
  return grad_layout(B, N, H, K).total * 4;
}

#define OG_TRY(call) \
  do { if ((e = (call)) != MMSEQ_OK) return e; } while (0)
#define OG_HIP(call)                                                                      \
  do {                                                                                    \
    hipError_t he_ = (call);                                                              \
    if (he_ != hipSuccess)                                                                \
      return mmseq_set_error(MMSEQ_EHIP, "order_score_bwd: %s", hipGetErrorString(he_)); \
  } while (0)

extern "C" mmseq_status mmseq_order_score_bwd(
    int B, int N, int H, int K, const float* doc, const float* okey, const float* hist,
    const float* h0, const float* c0, const float* w_ih, const float* b_ih, const float* w_hh,
    const float* b_hh, const float* w_q, const float* b_q, const float* w_pw, const float* w_t,
    const float* b_t, const float* wt_ih, const float* wt_hh, const float* wt_q, const float* wt_pw,
    const int64_t* orders, int64_t story_stride, const float* dnll, float* ddoc, float* dokey,
    float* dhist, float* dh0, float* dc0, float* dw_ih, float* db_ih, float* dw_hh, float* db_hh,
    float* dw_q, float* db_q, float* dw_pw, float* dw_t, float* db_t, void* workspace,
    int64_t workspace_bytes, mmseq_stream stream) {
  if (!grad_supported(B, N, H, K))
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "order_score_bwd: B=%d N=%d H=%d K=%d outside 1 <= N <= %d, 1 <= K, "
                           "B*K*4H < 2^31 (or B / H too large for 32-bit row counts)",
                           B, N, H, K, BEAM_MAXN);
  char why[DEC_WHY] = "";
  if (!(story_stride == 0 || story_stride >= (int64_t)K * N))
    snprintf(why, sizeof why, "story_stride %lld is neither 0 (shared list) nor >= K*N",
             (long long)story_stride);
  const DecoderWeights wt{w_ih, b_ih, w_hh, b_hh, w_q, b_q, w_pw, w_t, b_t};
  const GradWs L = grad_layout(B, N, H, K);
  mmseq_status e = decoder_require(
      "order_score_bwd", doc, okey, hist, h0, c0, wt,
      wt_ih && wt_hh && wt_q && wt_pw && orders && dnll && ddoc && dokey && dhist && dh0 && dc0 &&
          dw_ih && db_ih && dw_hh && db_hh && dw_q && db_q && dw_pw && dw_t && db_t,
      why, workspace, workspace_bytes, L.total * 4);
  if (e != MMSEQ_OK || B == 0) return e;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t BN = (int64_t)B * N;
  if (N == 1) {  // no step: the scores are constants
    OG_HIP(hipMemsetAsync(ddoc, 0, BN * H * 4, st));
    OG_HIP(hipMemsetAsync(dokey, 0, BN * H * 4, st));
    OG_HIP(hipMemsetAsync(dhist, 0, BN * N * (H + 2) * 4, st));
    OG_HIP(hipMemsetAsync(dh0, 0, (int64_t)B * H * 4, st));
    OG_HIP(hipMemsetAsync(dc0, 0, (int64_t)B * H * 4, st));
    return MMSEQ_OK;
  }
  float* ws = reinterpret_cast<float*>(workspace);
  const int R = B * K, T = N - 1, H4 = 4 * H, H2 = H + 2;
  const int64_t RH = (int64_t)R * H, RH4 = (int64_t)R * H4;
  int* seq = reinterpret_cast<int*>(ws + L.seq);
  int* bad = reinterpret_cast<int*>(ws + L.bad);
  float *gx = ws + L.gx, *proj = ws + L.proj, *hs = ws + L.hs, *cs = ws + L.cs;
  float *gates = ws + L.gates, *q = ws + L.q, *dA = ws + L.dA, *wpart = ws + L.wpart;
  float *dh = ws + L.dh, *dc = ws + L.dc, *csum = ws + L.csum;
  const GemmSlab slab{ws + L.slab, OG_SLAB * 4}, none{nullptr, 0};  // split-K scratch

  // ---- forward, keeping every step's state -----------------------------------------------------
  hipLaunchKernelGGL(og_init_kernel, dim3(R), dim3(256), 0, st, N, H, K, orders, story_stride, h0,
                     c0, hs, cs, seq, bad);
  OG_TRY(mmseq_check_launch("order_score_bwd init"));
  OG_TRY(story_setup(B, N, H, doc, hist, wt, gx, proj, L.pstride, stream));
  for (int t = 0; t < T; ++t) {
    float* gt = gates + t * RH4;
    OG_TRY(dec_gemm(R, H4, H, hs + t * RH, H, w_hh, H, gt, H4, b_hh, 0, none, stream));
    hipLaunchKernelGGL(og_cell_kernel, dim3(R), dim3(256), 0, st, H, K, N, t, gx, b_ih, seq, gt,
                       cs + t * RH, hs + (t + 1) * RH, cs + (t + 1) * RH);
    OG_TRY(mmseq_check_launch("order_score_bwd cell"));
    // per step, as the scorer runs it: the same rows give the same q bits
    OG_TRY(dec_gemm(R, H, H, hs + (t + 1) * RH, H, w_q, H, q + t * RH, H, b_q, 0, none, stream));
  }

  // ---- 1. the pointer part of every (step, slot) -----------------------------------------------
  hipLaunchKernelGGL(og_score_bwd_kernel, dim3((unsigned)((int64_t)T * R)), dim3(256), 0, st, N, H,
                     K, (int64_t)R, q, proj, L.pstride, okey, w_t, b_t, seq, bad, dnll, dA, wpart);
  OG_TRY(mmseq_check_launch("order_score_bwd score"));

  // ---- 2. the LSTM chain backwards ---------------------------------------------------------------
  const int64_t n = RH;
  for (int t = T - 1; t >= 0; --t) {
    float* gt = gates + t * RH4;
    OG_TRY(dec_gemm(R, H, H, q + t * RH, H, wt_q, H, dh, H, nullptr, t == T - 1 ? 0 : 1, slab,
                   stream));
    hipLaunchKernelGGL(og_cell_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, H,
                       gt, cs + t * RH, cs + (t + 1) * RH, dh, t == T - 1 ? nullptr : dc, dc);
    OG_TRY(mmseq_check_launch("order_score_bwd cell_bwd"));
    OG_TRY(dec_gemm(R, H, H4, gt, H4, wt_hh, H4, dh, H, nullptr, 0, slab, stream));
  }
  hipLaunchKernelGGL(og_gather_state_kernel, dim3(B), dim3(256), 0, st, H, K, dh, dc, dh0, dc0);
  OG_TRY(mmseq_check_launch("order_score_bwd gather_state"));

  // ---- 3. gathers to the per-story rows (GX and PROJ are dead: their rows take the gradients) ----
  hipLaunchKernelGGL(og_gather_key_kernel, dim3((unsigned)(BN * N)), dim3(256), 0, st, N, H, K,
                     (int64_t)R, seq, dA, proj, L.pstride, dokey);
  OG_TRY(mmseq_check_launch("order_score_bwd gather_key"));
  if (N > 2) {
    hipLaunchKernelGGL(og_gather_gx_kernel, dim3((unsigned)BN), dim3(256), 0, st, N, H, K,
                       (int64_t)R, seq, gates, gx);
    OG_TRY(mmseq_check_launch("order_score_bwd gather_gx"));
  }

  // ---- 4. dense parts ----------------------------------------------------------------------------
  const int64_t TR = (int64_t)T * R;
  if (N > 2) {
    OG_TRY(dec_gemm((int)BN, H, H4, gx, H4, wt_ih, H4, ddoc, H, nullptr, 0, slab, stream));
    OG_TRY(og_wgrad(H4, H, (int)BN, gx, H4, doc, H, dw_ih, H, slab, stream));
  } else {
    OG_HIP(hipMemsetAsync(ddoc, 0, BN * H * 4, st));
  }
  OG_TRY(og_wgrad(H4, H, (int)TR, gates, H4, hs, H, dw_hh, H, slab, stream));
  OG_TRY(og_colsum(TR, H4, gates, H4, csum, db_hh, db_ih, st));
  OG_TRY(og_wgrad(H, H, (int)TR, q, H, hs + RH, H, dw_q, H, slab, stream));
  OG_TRY(og_colsum(TR, H, q, H, csum, db_q, nullptr, st));
  for (int g = 0; g < 4; ++g) {
    OG_TRY(dec_gemm((int)(BN * N), H2, H, proj + g * L.pstride, H, wt_pw + (int64_t)g * H2 * H, H,
                   dhist, H2, nullptr, g > 0, slab, stream));
    OG_TRY(og_wgrad(H, H2, (int)(BN * N), proj + g * L.pstride, H, hist, H2,
                    dw_pw + (int64_t)g * H2, 4 * (int64_t)H2, slab, stream));
  }
  OG_TRY(og_colsum(TR, H, wpart, H + 1, csum, dw_t, nullptr, st));
  OG_TRY(og_colsum(TR, 1, wpart + H, H + 1, csum, db_t, nullptr, st));
  return MMSEQ_OK;
}
