// Posterior over candidate orders: K scored orders per story -> the normalised
// weights' marginals (position[t][s], before[a][c]), log mass, entropy, the heaviest candidate and
// the candidates that maximise the expected positional accuracy / Kendall's tau (minimum-risk
// decode under evaluate.cal_result's per-story metrics).
//
// One workgroup per story, K * N^2 work: latency-bound, no MFMA. Everything that is summed is
// summed in f64 in ascending candidate order by ONE thread per output element, so the result does
// not depend on the launch geometry and a sequential float64 restatement reproduces it
// (tests/order_posterior_ref.py); no atomics.
#include "common.h"

namespace {

constexpr int POST_MAXN = 16;   // the beam's BEAM_MAXN
constexpr int POST_TILE = 256;  // candidates staged in LDS per round = threads per workgroup

// candidate k of the story: valid iff its nll is finite and its N entries are a permutation of
// 0 .. N-1; every entry is checked before it is used as an index. ord[t] = step at position t,
// inv[s] = position of step s (both written only where valid).
__device__ __forceinline__ bool post_load(const int64_t* __restrict__ cand, float v, int N,
                                          unsigned char* ord, unsigned char* inv) {
  bool ok = v - v == 0.f;  // finite: +-inf and NaN give NaN
  unsigned have = 0;
  for (int t = 0; t < N; ++t) {
    const int64_t s = cand[t];
    const bool in = s >= 0 && s < N;
    const unsigned bit = in ? 1u << (int)s : 0u;
    ok = ok && in && !(have & bit);
    have |= bit;
    if (ord && ok) { ord[t] = (unsigned char)s; inv[(int)s] = (unsigned char)t; }
  }
  return ok;
}

__global__ __launch_bounds__(POST_TILE) void order_posterior_kernel(
    int N, int K, int mode, const int64_t* __restrict__ orders, int64_t story_stride,
    const float* __restrict__ nll, float* __restrict__ logz, float* __restrict__ position,
    float* __restrict__ before, float* __restrict__ entropy, int* __restrict__ map_index,
    float* __restrict__ map_prob, int* __restrict__ acc_index, int* __restrict__ tau_index,
    float* __restrict__ exp_acc, float* __restrict__ exp_tau) {
  __shared__ unsigned char s_ord[POST_TILE][POST_MAXN];
  __shared__ unsigned char s_inv[POST_TILE][POST_MAXN];
  __shared__ double s_w[POST_TILE], s_wx[POST_TILE];
  __shared__ double s_g[2][POST_TILE];
  __shared__ float s_v[POST_TILE];
  __shared__ int s_i[2][POST_TILE];
  __shared__ float s_pos[POST_MAXN * POST_MAXN], s_bef[POST_MAXN * POST_MAXN];
  const int b = blockIdx.x, tid = threadIdx.x, NN = N * N;
  const int64_t* ob = orders + (int64_t)b * story_stride;
  const float* nb = nll + (int64_t)b * K;

  // 1. the smallest valid nll and its lowest index: the heaviest candidate, and the shift of the
  //    exponentials. (-0.0 == +0.0: the two tie, as everywhere below.) Mode 1 weighs every valid
  //    candidate the same: all tie, and the first valid one is reported.
  float best = INFINITY;
  int bidx = -1;
  for (int k = tid; k < K; k += POST_TILE) {
    const float v = nb[k], key = mode == 0 ? v : 0.f;
    if (post_load(ob + (int64_t)k * N, v, N, nullptr, nullptr) && (bidx < 0 || key < best)) {
      best = key;
      bidx = k;
    }
  }
  s_v[tid] = best;
  s_i[0][tid] = bidx;
  __syncthreads();
  if (tid == 0) {
    for (int i = 1; i < POST_TILE; ++i) {
      const int ki = s_i[0][i];
      if (ki >= 0 && (bidx < 0 || s_v[i] < best || (s_v[i] == best && ki < bidx))) {
        best = s_v[i];
        bidx = ki;
      }
    }
    s_v[0] = best;
    s_i[0][0] = bidx;
  }
  __syncthreads();
  best = s_v[0];
  bidx = s_i[0][0];
  __syncthreads();
  if (bidx < 0) {  // no valid candidate
    if (tid < NN) { position[(int64_t)b * NN + tid] = 0.f; before[(int64_t)b * NN + tid] = 0.f; }
    if (tid == 0) {
      logz[b] = -INFINITY;
      entropy[b] = 0.f; map_prob[b] = 0.f; exp_acc[b] = 0.f; exp_tau[b] = 0.f;
      map_index[b] = -1; acc_index[b] = -1; tau_index[b] = -1;
    }
    return;
  }

  // 2. weights w_k = exp(best - nll_k) (mode 0) or 1 (mode 1), 0 where invalid, staged per tile;
  //    thread e < N^2 owns position / before entry e and adds the tile's weights in k order. Every
  //    thread adds Z = sum w and sum w x (x = best - nll) in that order too, so all hold the same.
  const int r = tid / N, c = tid - r * N;  // entry (t, s) of position, (a, c) of before
  double Z = 0.0, WX = 0.0, P = 0.0, Bf = 0.0;
  for (int k0 = 0; k0 < K; k0 += POST_TILE) {
    const int k = k0 + tid;
    double w = 0.0, x = 0.0;
    if (k < K) {
      const float v = nb[k];
      if (post_load(ob + (int64_t)k * N, v, N, s_ord[tid], s_inv[tid])) {
        x = mode == 0 ? (double)best - (double)v : 0.0;
        w = mode == 0 ? exp(x) : 1.0;
      }
    }
    s_w[tid] = w;
    s_wx[tid] = w * x;
    __syncthreads();
    const int n = K - k0 < POST_TILE ? K - k0 : POST_TILE;
    for (int i = 0; i < n; ++i) {
      const double wi = s_w[i];
      if (wi == 0.0) continue;  // invalid (or underflowed): its ord / inv rows are stale
      Z += wi;
      WX += s_wx[i];
      if (tid < NN) {
        if (s_ord[i][r] == c) P += wi;
        if (r != c && s_inv[i][r] < s_inv[i][c]) Bf += wi;
      }
    }
    __syncthreads();
  }
  if (tid < NN) {  // rounded once
    const float p = (float)(P / Z), q = (float)(Bf / Z);
    s_pos[tid] = p;
    s_bef[tid] = q;
    position[(int64_t)b * NN + tid] = p;
    before[(int64_t)b * NN + tid] = q;
  }
  if (tid == 0) {
    const double lz = log(Z);
    logz[b] = (float)(mode == 0 ? lz - (double)best : lz);
    entropy[b] = (float)(lz - WX / Z);
    map_index[b] = bidx;
    map_prob[b] = (float)(1.0 / Z);  // the heaviest weight is exp(0) = 1 (and 1 in mode 1)
  }
  __syncthreads();

  // 3. expected metrics of every valid candidate, in f64 from the f32-rounded matrices:
  //    gain_acc = (sum_t position[t][o_t]) / N, t ascending
  //    gain_tau = (sum_{i<j} before[o_i][o_j] - before[o_j][o_i]) / C(N,2), (i, j) lexicographic
  //    (N = 1: 1, as cal_result). The largest wins, ties to the lowest index.
  double ga = -1.0, gt = -2.0;  // below every gain (acc >= 0, tau >= -1)
  int ia = -1, it = -1;
  const double pairs = (double)(N * (N - 1) / 2);
  for (int k = tid; k < K; k += POST_TILE) {
    unsigned char o[POST_MAXN], inv[POST_MAXN];
    if (!post_load(ob + (int64_t)k * N, nb[k], N, o, inv)) continue;
    double a = 0.0, t2 = 0.0;
    for (int t = 0; t < N; ++t) a += (double)s_pos[t * N + o[t]];
    a /= (double)N;
    for (int i = 0; i < N; ++i)
      for (int j = i + 1; j < N; ++j)
        t2 += (double)s_bef[o[i] * N + o[j]] - (double)s_bef[o[j] * N + o[i]];
    t2 = N > 1 ? t2 / pairs : 1.0;
    if (a > ga) { ga = a; ia = k; }   // k ascends: the first of equals stays
    if (t2 > gt) { gt = t2; it = k; }
  }
  s_g[0][tid] = ga; s_i[0][tid] = ia;
  s_g[1][tid] = gt; s_i[1][tid] = it;
  __syncthreads();
  if (tid < 2) {
    double g = s_g[tid][0];
    int gi = s_i[tid][0];
    for (int i = 1; i < POST_TILE; ++i) {
      const int ki = s_i[tid][i];
      const double v = s_g[tid][i];
      if (ki >= 0 && (gi < 0 || v > g || (v == g && ki < gi))) { g = v; gi = ki; }
    }
    if (tid == 0) { acc_index[b] = gi; exp_acc[b] = (float)g; }
    else { tau_index[b] = gi; exp_tau[b] = (float)g; }
  }
}

}  // namespace

extern "C" mmseq_status mmseq_order_posterior(int B, int N, int K, int mode, const int64_t* orders,
                                              int64_t story_stride, const float* nll, float* logz,
                                              float* position, float* before, float* entropy,
                                              int32_t* map_index, float* map_prob,
                                              int32_t* mbr_acc_index, int32_t* mbr_tau_index,
                                              float* exp_acc, float* exp_tau, mmseq_stream stream) {
  if (B < 0 || N < 1 || N > POST_MAXN || K < 1)
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "order_posterior: B=%d N=%d K=%d outside B >= 0, 1 <= N <= %d, K >= 1", B,
                           N, K, POST_MAXN);
  MMSEQ_REQUIRE(mode == 0 || mode == 1, "order_posterior: mode %d is neither 0 (weights) nor 1 "
                "(uniform)", mode);
  MMSEQ_REQUIRE(orders && nll && logz && position && before && entropy && map_index && map_prob &&
                    mbr_acc_index && mbr_tau_index && exp_acc && exp_tau,
                "order_posterior: null buffer");
  MMSEQ_REQUIRE(story_stride == 0 || story_stride >= (int64_t)K * N,
                "order_posterior: story_stride %lld is neither 0 (shared list) nor >= K*N",
                (long long)story_stride);
  if (B == 0) return MMSEQ_OK;
  hipLaunchKernelGGL(order_posterior_kernel, dim3(B), dim3(POST_TILE), 0,
                     reinterpret_cast<hipStream_t>(stream), N, K, mode, orders, story_stride, nll,
                     logz, position, before, entropy, map_index, map_prob, mbr_acc_index,
                     mbr_tau_index, exp_acc, exp_tau);
  return mmseq_check_launch("order_posterior");
}
