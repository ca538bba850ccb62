// The pointer decoder's step (modeling_bert.py:1368-1402 BertForOrdering.step), written once for
// every entry that runs it: the beam, n-best, order_score, order_sample and order_tree (beam.hip),
// order_score_bwd (order_grad.hip) and the training decoder's LSTM cell (head.hip).
//
// Per call (story_setup): pw_k is linear, so the four blocks of its input are projected ONCE per
// story, and x W_ih^T + b_ih for x = doc[b][i] is one GEMM:
//   GX[b][i][:]         = W_ih doc[b][i] + b_ih
//   PROJ[g][b][i][j][:] = pw_k.weight[:, g(H+2):(g+1)(H+2)] hist[b][i][j]        g = 0..3
// Per step t of a slot with picks seq[0..t-1] (l1, l2 the last two, m = (i != j, neither pointed)):
//   (h, c)  = LSTM cell of (GX[l1] or b_ih at t = 0, h W_hh^T + b_hh, c)             lstm_cell
//   q       = W_q h + b_q
//   keys[j] = PROJ[0][l1][j] + PROJ[1][l2][j] + (sum_{j'} m PROJ[2][j][j']) / N
//                                             + (sum_{i}  m PROJ[3][i][j]) / N
//   e[j]    = w_t . tanh(q + keys[j] + okey[j]) + b_t, -1e9 where pointed
// The entries differ in where a slot's rows live and in what they do with e; the expressions, and
// with them the bits, are these.
#pragma once
#include "common.h"

constexpr int BEAM_MAXN = 16;  // sentences per story; the stride of every int32 pick (seq) row

inline int64_t up4(int64_t n) { return (n + 3) / 4 * 4; }

struct DecoderWeights {
  const float *w_ih, *b_ih, *w_hh, *b_hh, *w_q, *b_q, *w_pw, *w_t, *b_t;
};

struct GemmSlab {  // split-K scratch handed to mmseq_gemm; {nullptr, 0}: none
  float* ptr;
  int64_t bytes;
};

// C[M][Nn] (+)= A[M][K] B[Nn][K]^T (+ bias), fp32
inline mmseq_status dec_gemm(int M, int Nn, int K, const float* A, int64_t lda, const float* Bm,
                             int64_t ldb, float* C, int64_t ldc, const float* bias, int accumulate,
                             GemmSlab slab, mmseq_stream stream) {
  return mmseq_gemm(0, M, Nn, K, 1, A, lda, 0, Bm, ldb, 0, C, ldc, 0, bias, MMSEQ_ACT_NONE, nullptr,
                    nullptr, nullptr, 0, 0, 1.0f, accumulate, MMSEQ_F32, MMSEQ_F32, nullptr,
                    MMSEQ_GEMM_AUTO, slab.ptr, slab.bytes, stream);
}

// once per call: the input gates of every sentence (GX, read from step 1 on: N > 2) and the four
// projections of hist (PROJ, blocks `pstride` floats apart)
inline mmseq_status story_setup(int B, int N, int H, const float* doc, const float* hist,
                                const DecoderWeights& wt, float* gx, float* proj, int64_t pstride,
                                mmseq_stream stream) {
  mmseq_status e;
  if (N > 2 && (e = dec_gemm(B * N, 4 * H, H, doc, H, wt.w_ih, H, gx, 4 * H, wt.b_ih, 0,
                             GemmSlab{nullptr, 0}, stream)) != MMSEQ_OK)
    return e;
  for (int g = 0; g < 4; ++g)
    if ((e = dec_gemm(B * N * N, H, H + 2, hist, H + 2, wt.w_pw + (int64_t)g * (H + 2),
                      4 * (int64_t)(H + 2), proj + g * pstride, H, nullptr, 0, GemmSlab{nullptr, 0},
                      stream)) != MMSEQ_OK)
      return e;
  return MMSEQ_OK;
}

// The checks every decoder entry makes, in this order: the five encoder outputs, the nine weights
// and the entry's own buffers (`rest`) are there; the entry's own arguments are sound (`arg_error`:
// what is wrong with them, empty = nothing; `need` is not read then); the workspace is aligned and
// holds `need` bytes. The entries format arg_error into char[DEC_WHY] with snprintf, which cuts an
// over-long text short: the longest today has 83 characters, keep new ones below DEC_WHY.
constexpr int DEC_WHY = 128;
inline mmseq_status decoder_require(const char* what, const float* doc, const float* okey,
                                    const float* hist, const float* h0, const float* c0,
                                    const DecoderWeights& wt, bool rest, const char* arg_error,
                                    const void* workspace, int64_t workspace_bytes, int64_t need) {
  MMSEQ_REQUIRE(doc && okey && hist && h0 && c0 && wt.w_ih && wt.b_ih && wt.w_hh && wt.b_hh &&
                    wt.w_q && wt.b_q && wt.w_pw && wt.w_t && wt.b_t && rest,
                "%s: null buffer", what);
  MMSEQ_REQUIRE(!arg_error[0], "%s: %s", what, arg_error);
  MMSEQ_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 && workspace_bytes >= need,
                "%s: workspace must be 16-byte aligned and hold %lld bytes (got %lld)", what,
                (long long)need, (long long)workspace_bytes);
  return MMSEQ_OK;
}

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// LSTM cell (gate order i, f, g, o) of unit u: x and gh are the row's 4H pre-activations from the
// input and from h (both with their biases), c_prev points at the unit's cell state.
// c_prev is a POINTER on purpose, loaded after the gates: of the two products in f * c + i * g the
// compiler fuses one into an FMA and picks it by the order of the loads. Taking c by value changed
// that pick and the low bits of c in every entry. Do not change it to by-value.
struct LstmCell {
  float i, f, g, o, c2, h;
};
__device__ __forceinline__ LstmCell lstm_cell(const float* x, const float* gh, int H, int u,
                                              const float* c_prev) {
  LstmCell r;
  r.i = sigm(x[u] + gh[u]);
  r.f = sigm(x[H + u] + gh[H + u]);
  r.g = tanhf(x[2 * H + u] + gh[2 * H + u]);
  r.o = sigm(x[3 * H + u] + gh[3 * H + u]);
  r.c2 = r.f * *c_prev + r.i * r.g;
  r.h = r.o * tanhf(r.c2);
  return r;
}

// Its backward: the activations a, c_prev, c2 = c_out, dh and the gradient flowing into c_out ->
// the four pre-activation gradients and dc_prev.
struct LstmCellGrad {
  float di, df, dg, d_o, dc_prev;
};
__device__ __forceinline__ LstmCellGrad lstm_cell_bwd(float i, float f, float g, float o,
                                                      float c_prev, float c_out, float dhv,
                                                      float dc_next) {
  const float tc = tanhf(c_out);
  const float dc = dc_next + dhv * o * (1.f - tc * tc);
  LstmCellGrad r;
  r.di = dc * g * i * (1.f - i);
  r.df = dc * c_prev * f * (1.f - f);
  r.dg = dc * i * (1.f - g * g);
  r.d_o = dhv * tc * o * (1.f - o);
  r.dc_prev = dc * f;
  return r;
}

// the steps a slot has pointed at before step t
__device__ __forceinline__ unsigned pointed_mask(const int* seq_row, int t) {
  unsigned pointed = 0;
  for (int p = 0; p < t; ++p) pointed |= 1u << seq_row[p];
  return pointed;
}

// lowest zero bit of a mask that has one (fewer than N picks: one index is always free)
__device__ __forceinline__ int lowest_free(unsigned have) {
  int miss = 0;
  while ((have >> miss) & 1u) ++miss;
  return miss;
}

// A candidate order's N - 1 picks are a valid prefix (in range, none repeated). Every entry is
// checked BEFORE any forms an address: the caller runs an invalid candidate as 0, 1, .., N-2 so
// that every later indexed read stays in bounds. Every thread: the same N - 1 loads, no LDS, no
// barrier.
__device__ __forceinline__ bool candidate_ok(const int64_t* cand, int N) {
  unsigned have = 0;
  bool ok = true;
  for (int p = 0; p < N - 1; ++p) {
    const int64_t v = cand[p];
    const bool in = v >= 0 && v < N;
    const unsigned bit = in ? 1u << (int)v : 0u;
    ok = ok && in && !(have & bit);
    have |= bit;
  }
  return ok;
}
