// Decoding from the pairwise head. w[a][c] is the log-evidence that step a precedes
// step c; G(o) = sum_{i<j} w[o_i][o_j] scores an order, pnll = -G.
//
// mmseq_pairwise_order: the exact arg-max of G (a linear-ordering problem) and the distribution
// Q(o) ~ exp(G(o)) by dynamic programming over the 2^N subsets S of steps already placed: placing c
// after S adds g(S, c) = sum_{a in S} w[a][c], whatever the order inside S. One workgroup per
// story walks the subset lattice one popcount layer at a time (a barrier between layers); the two
// tables of 2^N doubles a pass needs live in LDS up to N = 11 (32 KiB) and in the caller's
// workspace at N = 12. Everything is f64, every sum is taken by ONE thread in a stated order, no
// atomics: the max path is a chain of f64 additions of f32 values that a numpy restatement
// reproduces to the bit (tests/pairwise_order_ref.py).
//
// mmseq_pairwise_score: pnll of K candidate orders per story, one thread per candidate, w and the
// workgroup's candidates staged in LDS (the order reads are one contiguous block per workgroup).
#include "common.h"

namespace {

constexpr int PW_MAXN = 12;       // 4096 states
constexpr int PW_LDS_N = 11;      // the two tables fit LDS up to here: 2 * 2048 * 8 B = 32 KiB
constexpr int PW_THREADS = 256;
constexpr int PW_STAGE = 128;     // subsets whose p(S, .) are staged in LDS per round: 12 KiB
constexpr int PW_SCORE_MAXN = 16;  // the beam's BEAM_MAXN
constexpr int PW_SCORE_TILE = 256;

__device__ __forceinline__ bool pw_finite(float v) { return v - v == 0.f; }  // +-inf, NaN: NaN

// g(S, c) = sum_{a in S} w[a][c], a ascending, from 0.0
__device__ __forceinline__ double pw_g(const double* w, int N, unsigned S, int c) {
  double g = 0.0;
  for (unsigned m = S; m; m &= m - 1) g += w[(__ffs(m) - 1) * N + c];
  return g;
}

// x into the two largest (t1 >= t2) of a multiset: equal values fill both
__device__ __forceinline__ void pw_top2(double x, double& t1, double& t2) {
  if (x > t1) { t2 = t1; t1 = x; }
  else if (x > t2) t2 = x;
}

// log sum_c exp(x_c) over the steps c of `cand`, c ascending, shifted by the largest x_c.
// FWD: x_c = ta[S ^ c] + g(S ^ c, c) (c leaves S); else x_c = g(S, c) + tb[S | c] (c joins S).
template <bool FWD>
__device__ __forceinline__ double pw_lse(const double* w, int N, unsigned S, unsigned cand,
                                         const double* tab) {
  double mx = -INFINITY;
  for (unsigned m = cand; m; m &= m - 1) {
    const int c = __ffs(m) - 1;
    const unsigned bit = 1u << c;
    const double x = FWD ? tab[S ^ bit] + pw_g(w, N, S ^ bit, c) : pw_g(w, N, S, c) + tab[S | bit];
    mx = x > mx ? x : mx;
  }
  double sum = 0.0;
  for (unsigned m = cand; m; m &= m - 1) {
    const int c = __ffs(m) - 1;
    const unsigned bit = 1u << c;
    const double x = FWD ? tab[S ^ bit] + pw_g(w, N, S ^ bit, c) : pw_g(w, N, S, c) + tab[S | bit];
    sum += exp(x - mx);
  }
  return mx + log(sum);
}

template <bool LDS>
__global__ __launch_bounds__(PW_THREADS) void pairwise_order_kernel(
    int N, const float* __restrict__ w, int64_t* __restrict__ order, float* __restrict__ pnll,
    float* __restrict__ margin, float* __restrict__ logz, float* __restrict__ position,
    float* __restrict__ before, float* __restrict__ entropy, double* __restrict__ ws) {
  __shared__ double s_tab[LDS ? 2 << PW_LDS_N : 2];
  __shared__ double s_w[PW_MAXN * PW_MAXN], s_bef[PW_MAXN * PW_MAXN];
  __shared__ double s_p[PW_STAGE * PW_MAXN];
  const int b = blockIdx.x, tid = threadIdx.x, NN = N * N;
  const unsigned states = 1u << N, full = states - 1;
  double* ta;
  if constexpr (LDS) ta = s_tab;
  else ta = ws + (int64_t)b * (2 << PW_MAXN);
  double* tb = ta + states;
  const int r = tid / N, c = tid - r * N;  // entry (t, s) of position, (a, c) of before

  bool bad = false;
  if (tid < NN) {
    const float v = w[(int64_t)b * NN + tid];
    bad = r != c && !pw_finite(v);
    s_w[tid] = r == c ? 0.0 : (double)v;
  }
  if (__syncthreads_or(bad)) {  // a non-finite off-diagonal weight: the invalid story
    if (tid < NN) { position[(int64_t)b * NN + tid] = 0.f; before[(int64_t)b * NN + tid] = 0.f; }
    if (tid < N) order[(int64_t)b * N + tid] = -1;
    if (tid == 0) { pnll[b] = INFINITY; margin[b] = 0.f; logz[b] = -INFINITY; entropy[b] = 0.f; }
    return;
  }

  // 1. the optimum. ta = h1, tb = h2: the best and second-best completion of S, as distinct orders
  if (tid == 0) { ta[full] = 0.0; tb[full] = -INFINITY; }
  __syncthreads();
  for (int p = N - 1; p >= 0; --p) {
    for (unsigned S = tid; S < states; S += PW_THREADS) {
      if (__popc(S) != p) continue;
      double t1 = -INFINITY, t2 = -INFINITY;
      for (unsigned m = full & ~S; m; m &= m - 1) {
        const int s = __ffs(m) - 1;
        const unsigned T = S | 1u << s;
        const double g = pw_g(s_w, N, S, s);
        pw_top2(g + ta[T], t1, t2);
        pw_top2(g + tb[T], t1, t2);
      }
      ta[S] = t1;
      tb[S] = t2;
    }
    __syncthreads();
  }
  if (tid == 0) {  // from the front: the lowest step that attains h1[S]
    unsigned S = 0;
    for (int t = 0; t < N; ++t) {
      int pick = -1;
      for (unsigned m = full & ~S; m && pick < 0; m &= m - 1) {
        const int s = __ffs(m) - 1;
        if (pw_g(s_w, N, S, s) + ta[S | 1u << s] == ta[S]) pick = s;
      }
      if (pick < 0) pick = __ffs(full & ~S) - 1;  // unreachable: h1[S] is one of the sums above
      order[(int64_t)b * N + t] = pick;
      S |= 1u << pick;
    }
    pnll[b] = (float)(-ta[0]);
    margin[b] = (float)(ta[0] - tb[0]);
  }
  __syncthreads();

  // 2. the distribution. ta = log alpha (mass of the ways to place S first), tb = log beta (mass
  //    of the ways to place the rest after S); layer i of alpha and layer N - i of beta per round
  if (tid == 0) { ta[0] = 0.0; tb[full] = 0.0; }
  __syncthreads();
  for (int i = 1; i <= N; ++i) {
    for (unsigned S = tid; S < states; S += PW_THREADS) {
      const int pc = __popc(S);
      if (pc == i) ta[S] = pw_lse<true>(s_w, N, S, S, ta);
      if (pc == N - i) tb[S] = pw_lse<false>(s_w, N, S, full & ~S, tb);
    }
    __syncthreads();
  }
  // 3. the marginals. p(S, s) = exp(((la[S] + g(S, s)) + lb[S | s]) - logz) is staged for
  //    PW_STAGE subsets at a time, each entry computed once by all threads; thread e < N^2 then
  //    adds its own entries in S order, so every sum runs over S ascending whatever the staging.
  const double lz = ta[full];
  double P = 0.0, Bf = 0.0;
  for (unsigned S0 = 0; S0 < states; S0 += PW_STAGE) {
    const int ns = states - S0 < PW_STAGE ? (int)(states - S0) : PW_STAGE;
    for (int i = tid; i < ns * N; i += PW_THREADS) {
      const unsigned S = S0 + i / N;
      const int s = i % N;
      const unsigned bit = 1u << s;
      s_p[i] = S & bit ? 0.0 : exp(ta[S] + pw_g(s_w, N, S, s) + tb[S | bit] - lz);
    }
    __syncthreads();
    if (tid < NN) {
      const unsigned cbit = 1u << c, rbit = 1u << r;
      for (int i = 0; i < ns; ++i) {
        const unsigned S = S0 + i;
        if (S & cbit) continue;
        const double pr = s_p[i * N + c];
        if (__popc(S) == r) P += pr;
        if (r != c && (S & rbit)) Bf += pr;
      }
    }
    __syncthreads();
  }
  if (tid < NN) {
    s_bef[tid] = Bf;
    position[(int64_t)b * NN + tid] = (float)P;
    before[(int64_t)b * NN + tid] = (float)Bf;
  }
  __syncthreads();
  if (tid == 0) {
    double e = 0.0;  // E_Q[G], (a, c) lexicographic
    for (int i = 0; i < NN; ++i)
      if (i / N != i % N) e += s_bef[i] * s_w[i];
    logz[b] = (float)lz;
    entropy[b] = (float)(lz - e);
  }
}

__global__ __launch_bounds__(PW_SCORE_TILE) void pairwise_score_kernel(
    int N, int K, const float* __restrict__ w, const int64_t* __restrict__ orders,
    int64_t story_stride, float* __restrict__ pnll) {
  __shared__ float s_w[PW_SCORE_MAXN * PW_SCORE_MAXN];
  __shared__ unsigned char s_ord[PW_SCORE_TILE * PW_SCORE_MAXN];
  const int b = blockIdx.y, tid = threadIdx.x, NN = N * N;
  const int k0 = blockIdx.x * PW_SCORE_TILE;
  const int n = K - k0 < PW_SCORE_TILE ? K - k0 : PW_SCORE_TILE;
  bool bad = false;
  if (tid < NN) {
    const float v = w[(int64_t)b * NN + tid];
    bad = tid / N != tid % N && !pw_finite(v);
    s_w[tid] = v;
  }
  // the workgroup's n * N entries are one contiguous block: consecutive lanes, consecutive entries.
  // An entry outside 0 .. N-1 is staged as 255 and fails the permutation check below.
  const int64_t* ob = orders + (int64_t)b * story_stride + (int64_t)k0 * N;
  for (int i = tid; i < n * N; i += PW_SCORE_TILE) {
    const int64_t s = ob[i];
    s_ord[i] = s >= 0 && s < N ? (unsigned char)s : (unsigned char)255;
  }
  bad = __syncthreads_or(bad);
  if (tid >= n) return;
  const unsigned char* o = s_ord + tid * N;
  unsigned have = 0;
  bool ok = !bad;
  for (int t = 0; t < N; ++t) {
    const unsigned bit = o[t] < N ? 1u << o[t] : 0u;
    ok = ok && bit && !(have & bit);
    have |= bit;
  }
  double g = 0.0;
  if (ok)
    for (int i = 0; i < N; ++i)
      for (int j = i + 1; j < N; ++j) g += (double)s_w[o[i] * N + o[j]];
  pnll[(int64_t)b * K + k0 + tid] = ok ? (float)(-g) : INFINITY;
}

int64_t pw_workspace(int B, int N) {
  if (N <= PW_LDS_N || B == 0) return 16;
  return (int64_t)B * (2 << PW_MAXN) * (int64_t)sizeof(double);
}

}  // namespace

extern "C" int64_t mmseq_pairwise_order_workspace(int B, int N) {
  if (B < 0 || N < 1 || N > PW_MAXN) return 0;
  return pw_workspace(B, N);
}

extern "C" mmseq_status mmseq_pairwise_order(int B, int N, const float* w, int64_t* order,
                                             float* pnll, float* margin, float* logz,
                                             float* position, float* before, float* entropy,
                                             void* workspace, int64_t workspace_bytes,
                                             mmseq_stream stream) {
  if (B < 0 || N < 1 || N > PW_MAXN)
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "pairwise_order: B=%d N=%d outside B >= 0, 1 <= N <= %d", B, N, PW_MAXN);
  MMSEQ_REQUIRE(w && order && pnll && margin && logz && position && before && entropy && workspace,
                "pairwise_order: null buffer");
  MMSEQ_REQUIRE(workspace_bytes >= pw_workspace(B, N) && ((uintptr_t)workspace & 15) == 0,
                "pairwise_order: workspace of %lld bytes, %lld needed, 16-byte aligned",
                (long long)workspace_bytes, (long long)pw_workspace(B, N));
  if (B == 0) return MMSEQ_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (N <= PW_LDS_N)
    hipLaunchKernelGGL(pairwise_order_kernel<true>, dim3(B), dim3(PW_THREADS), 0, st, N, w, order,
                       pnll, margin, logz, position, before, entropy, (double*)nullptr);
  else
    hipLaunchKernelGGL(pairwise_order_kernel<false>, dim3(B), dim3(PW_THREADS), 0, st, N, w, order,
                       pnll, margin, logz, position, before, entropy, (double*)workspace);
  return mmseq_check_launch("pairwise_order");
}

extern "C" mmseq_status mmseq_pairwise_score(int B, int N, int K, const float* w,
                                             const int64_t* orders, int64_t story_stride,
                                             float* pnll, mmseq_stream stream) {
  if (B < 0 || N < 1 || N > PW_SCORE_MAXN || K < 1)
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "pairwise_score: B=%d N=%d K=%d outside B >= 0, 1 <= N <= %d, K >= 1", B,
                           N, K, PW_SCORE_MAXN);
  MMSEQ_REQUIRE(w && orders && pnll, "pairwise_score: null buffer");
  MMSEQ_REQUIRE(story_stride == 0 || story_stride >= (int64_t)K * N,
                "pairwise_score: story_stride %lld is neither 0 (shared list) nor >= K*N",
                (long long)story_stride);
  const int tiles = (K + PW_SCORE_TILE - 1) / PW_SCORE_TILE;
  for (int b0 = 0; b0 < B; b0 += 65535) {  // grid.y holds the stories
    const int nb = B - b0 < 65535 ? B - b0 : 65535;
    hipLaunchKernelGGL(pairwise_score_kernel, dim3(tiles, nb), dim3(PW_SCORE_TILE), 0,
                       reinterpret_cast<hipStream_t>(stream), N, K, w + (int64_t)b0 * N * N,
                       orders + (int64_t)b0 * story_stride, story_stride,
                       pnll + (int64_t)b0 * K);
    const mmseq_status s = mmseq_check_launch("pairwise_score");
    if (s != MMSEQ_OK) return s;
  }
  return MMSEQ_OK;
}
