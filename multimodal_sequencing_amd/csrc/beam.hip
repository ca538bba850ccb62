// Batched beam-search ordering (modeling_bert.py:1368-1402 BertForOrdering.step, :1411-1552
// beam_search_pointer, generator.py:8-38 Beam) for B stories at once, beam state resident on the
// device: the whole decode is enqueued on one stream, with no host synchronisation and no copy to
// the host between enqueue and result (the per-story path does N - 1 round trips per story).
//
// Every story holds W fixed beam slots. All candidates of a story have the same length t at step
// t, so hypotheses finish only in the last step (t = N - 2), `valid` stays W until then, and the
// live count nb(t) = min(W, nb(t-1) * N), nb(0) = 1 is the same for every story and known on the
// host. The dense parts run over all B*W rows through mmseq_gemm; rows of slots >= nb hold
// whatever the workspace held and are never read by another row.
//
// The per-call setup and the step itself (GX, PROJ, cell, query, pointer energies) are
// pointer_decoder.h's. Every other entry here runs that setup and the same step (beam_step):
// mmseq_beam_search_nbest reports every finished hypothesis of the last selection, and
// mmseq_order_score runs K candidate orders per story as slots that never branch (W = nb = K,
// every slot entered with score 0) and, instead of selecting, adds each slot's own pick to its nll.
// mmseq_order_sample runs S such slots per story whose pick at every step is DRAWN from the step's
// distribution (ancestral sampling) with the counter hash of mmseq_mlm_mask.
// mmseq_order_tree scores ALL N! orders: the prefix tree walked level by level in chunks
// (order_tree_plan.h), a chunk being a beam of W = nb = cnt slots per story whose children enter
// with their parent's s entry, so that every shared prefix is stepped once.
#include "order_tree_plan.h"
#include "pointer_decoder.h"

namespace {

constexpr int BEAM_MAXW = 32;

struct BeamWs {  // float offsets into the workspace, each a multiple of 4 (16-byte rows)
  int64_t gx, proj, h[2], c[2], gh, q, s, score[2], seq[2], total;
};

BeamWs beam_layout(int B, int N, int H, int W) {
  BeamWs w;
  const int64_t R = (int64_t)B * W;
  int64_t o = 0;
  w.gx = o; o += up4((int64_t)B * N * 4 * H);
  w.proj = o; o += 4 * up4((int64_t)B * N * N * H);
  for (int i = 0; i < 2; ++i) { w.h[i] = o; o += up4(R * H); }
  for (int i = 0; i < 2; ++i) { w.c[i] = o; o += up4(R * H); }
  w.gh = o; o += up4(R * 4 * H);
  w.q = o; o += up4(R * H);
  w.s = o; o += up4(R * N);
  for (int i = 0; i < 2; ++i) { w.score[i] = o; o += up4(R); }
  for (int i = 0; i < 2; ++i) { w.seq[i] = o; o += up4(R * BEAM_MAXN); }  // int32 picks
  w.total = o;
  return w;
}

struct ScoreWs {  // mmseq_order_score: B stories x K slots that never branch, R = B*K rows
  int64_t gx, proj, h, c, gh, q, s, zero, seq, bad, total;
};

ScoreWs score_layout(int B, int N, int H, int K) {
  ScoreWs w;
  const int64_t R = (int64_t)B * K;
  int64_t o = 0;
  w.gx = o; o += up4((int64_t)B * N * 4 * H);
  w.proj = o; o += 4 * up4((int64_t)B * N * N * H);
  w.h = o; o += up4(R * H);
  w.c = o; o += up4(R * H);
  w.gh = o; o += up4(R * 4 * H);
  w.q = o; o += up4(R * H);
  w.s = o; o += up4(R * N);
  w.zero = o; o += up4(R);                // the score every slot enters a step with: 0
  w.seq = o; o += up4(R * BEAM_MAXN);     // int32 picks, written once by the init kernel
  w.bad = o; o += up4(R);                 // int32, 1 = invalid candidate
  w.total = o;
  return w;
}

// The optional n-best outputs of mmseq_beam_search_nbest (all NULL in mmseq_beam_search).
struct NBest {
  int64_t* orders;  // [B][W][N]
  float* scores;    // [B][W]
  int* count;       // [B]
};

// slot 0 of every story <- (h0, c0), score 0; N == 1: the order is [0]
__global__ __launch_bounds__(256) void beam_init_kernel(int N, int H, int W,
                                                        const float* __restrict__ h0,
                                                        const float* __restrict__ c0,
                                                        float* __restrict__ h, float* __restrict__ c,
                                                        float* __restrict__ score,
                                                        int64_t* __restrict__ order,
                                                        float* __restrict__ best, NBest nbest) {
  const int b = blockIdx.x;
  if (N == 1) {
    if (threadIdx.x == 0) {
      if (order) { order[b] = 0; best[b] = 0.f; }
      if (nbest.orders) {
        nbest.orders[(int64_t)b * W] = 0;
        nbest.scores[(int64_t)b * W] = 0.f;
        nbest.count[b] = 1;
      }
    }
    return;
  }
  const int64_t slot = (int64_t)b * W;
  for (int u = threadIdx.x; u < H; u += 256) {
    h[slot * H + u] = h0[(int64_t)b * H + u];
    c[slot * H + u] = c0[(int64_t)b * H + u];
  }
  if (threadIdx.x == 0) score[slot] = 0.f;
}

// LSTM cell (gates i, f, g, o) of the live slots, in place: x W_ih^T + b_ih is row `last` of the
// story's GX (t > 0) or b_ih alone (t = 0, x = 0); gh already holds h W_hh^T + b_hh.
__global__ __launch_bounds__(256) void beam_cell_kernel(int H, int W, int N, int t, int nb,
                                                        const float* __restrict__ gx,
                                                        const float* __restrict__ b_ih,
                                                        const float* __restrict__ gh,
                                                        const int* __restrict__ seq,
                                                        float* __restrict__ h, float* __restrict__ c) {
  const int64_t slot = blockIdx.x;
  const int b = (int)(slot / W), w = (int)(slot % W);
  if (w >= nb) return;
  const float* x = t > 0 ? gx + ((int64_t)b * N + seq[slot * BEAM_MAXN + t - 1]) * 4 * H : b_ih;
  const float* g4 = gh + slot * 4 * H;
  for (int u = threadIdx.x; u < H; u += 256) {
    const LstmCell r = lstm_cell(x, g4, H, u, c + slot * H + u);
    c[slot * H + u] = r.c2;
    h[slot * H + u] = r.h;
  }
}

// One workgroup per live slot: e[j] = tanh_linear(tanh(q + keys[j] + okey[j])), -1e9 where
// pointed, s[slot][j] = score[slot] - log_softmax(e)[j]. One wave per j, fixed summation order.
__global__ __launch_bounds__(256) void beam_score_kernel(int N, int H, int W, int t, int nb,
                                                         const float* __restrict__ q,
                                                         const float* __restrict__ proj,
                                                         int64_t proj_stride,
                                                         const float* __restrict__ okey,
                                                         const float* __restrict__ wt,
                                                         const float* __restrict__ bt,
                                                         const int* __restrict__ seq,
                                                         const float* __restrict__ score,
                                                         float* __restrict__ s) {
  __shared__ float e[BEAM_MAXN];
  const int64_t slot = blockIdx.x;
  const int b = (int)(slot / W), w = (int)(slot % W);
  if (w >= nb) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned pointed = 0;
  for (int p = 0; p < t; ++p) pointed |= 1u << seq[slot * BEAM_MAXN + p];
  const int l1 = t > 0 ? seq[slot * BEAM_MAXN + t - 1] : 0;
  const int l2 = t > 1 ? seq[slot * BEAM_MAXN + t - 2] : 0;
  const float* P1 = proj;
  const float* P2 = proj + proj_stride;
  const float* PF = proj + 2 * proj_stride;
  const float* PB = proj + 3 * proj_stride;
  const int64_t sb = (int64_t)b * N;  // story's first hist row block
  const float* qr = q + slot * H;
  const float fN = (float)N;  // both means divide by T (:1061-1062)
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
      acc += wt[u] * tanhf(qr[u] + key + orow[u]);
    }
    acc = wave_sum(acc);
    if (lane == 0) e[j] = jlive ? acc + bt[0] : -1e9f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float mx = -INFINITY;
    for (int j = 0; j < N; ++j) mx = fmaxf(mx, e[j]);
    float sum = 0.f;
    for (int j = 0; j < N; ++j) sum += expf(e[j] - mx);
    const float ls = logf(sum), sc = score[slot];
    for (int j = 0; j < N; ++j) s[slot * N + j] = sc - ((e[j] - mx) - ls);
  }
}

// One workgroup per story: the k smallest of the nb*N flat scores by (score, flat index) through
// a rank count in LDS (no sort, no dynamically indexed registers), the chosen entries become
// slots 0..k-1 of the next step in selection order with their parents' h', c'. In the last step
// the first selected entry is the story's best hypothesis (order / best, when asked for) and the
// selected entries that are permutations are the n-best list (nbest, when asked for).
__global__ __launch_bounds__(256) void beam_select_kernel(int N, int H, int W, int t, int nb, int k,
                                                          int last, const float* __restrict__ s,
                                                          const int* __restrict__ seq_cur,
                                                          int* __restrict__ seq_nxt,
                                                          float* __restrict__ score_nxt,
                                                          const float* __restrict__ h_cur,
                                                          const float* __restrict__ c_cur,
                                                          float* __restrict__ h_nxt,
                                                          float* __restrict__ c_nxt,
                                                          int64_t* __restrict__ order,
                                                          float* __restrict__ best, NBest nbest) {
  __shared__ float sh_s[BEAM_MAXW * BEAM_MAXN];
  __shared__ int sh_sel[BEAM_MAXW];
  __shared__ int sh_par[BEAM_MAXW];
  const int b = blockIdx.x, n = nb * N;
  const int64_t slot0 = (int64_t)b * W;
  for (int i = threadIdx.x; i < n; i += 256) sh_s[i] = s[slot0 * N + i];
  if (threadIdx.x < BEAM_MAXW) { sh_sel[threadIdx.x] = 0; sh_par[threadIdx.x] = 0; }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 256) {
    const float v = sh_s[i];
    int rank = 0;
    for (int o = 0; o < n; ++o) {
      const float x = sh_s[o];
      rank += (x < v || (x == v && o < i)) ? 1 : 0;
    }
    if (rank < k) sh_sel[rank] = i;
  }
  __syncthreads();
  if (last) {
    if (threadIdx.x == 0) {
      if (order) {
        const int i = sh_sel[0], w = i / N, j = i % N;
        unsigned have = 1u << j;
        for (int p = 0; p < t; ++p) {
          const int v = seq_cur[(slot0 + w) * BEAM_MAXN + p];
          order[(int64_t)b * N + p] = v;
          have |= 1u << v;
        }
        order[(int64_t)b * N + t] = j;
        order[(int64_t)b * N + t + 1] = lowest_free(have);  // N - 1 < N entries: one is free
        best[b] = sh_s[i];
      }
      if (nbest.orders) {
        // every selected entry in selection order; one that picked a pointed step anywhere on
        // its way (a repeated index, score ~1e9) is no permutation and is left out
        int cnt = 0;
        for (int r = 0; r < k; ++r) {
          const int i = sh_sel[r], w = i / N, j = i % N;
          unsigned have = 1u << j;
          bool ok = true;
          for (int p = 0; p < t; ++p) {
            const unsigned bit = 1u << seq_cur[(slot0 + w) * BEAM_MAXN + p];
            ok = ok && !(have & bit);
            have |= bit;
          }
          if (!ok) continue;
          int64_t* o = nbest.orders + ((int64_t)b * W + cnt) * N;
          for (int p = 0; p < t; ++p) o[p] = seq_cur[(slot0 + w) * BEAM_MAXN + p];
          o[t] = j;
          o[t + 1] = lowest_free(have);
          nbest.scores[(int64_t)b * W + cnt] = sh_s[i];
          ++cnt;
        }
        nbest.count[b] = cnt;
      }
    }
    return;
  }
  if (threadIdx.x < k) {
    const int r = threadIdx.x, i = sh_sel[r], w = i / N, j = i % N;
    for (int p = 0; p < t; ++p)
      seq_nxt[(slot0 + r) * BEAM_MAXN + p] = seq_cur[(slot0 + w) * BEAM_MAXN + p];
    seq_nxt[(slot0 + r) * BEAM_MAXN + t] = j;
    score_nxt[slot0 + r] = sh_s[i];
    sh_par[r] = w;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < k * H; idx += 256) {
    const int r = idx / H, u = idx - r * H;
    const int64_t src = (slot0 + sh_par[r]) * H + u, dst = (slot0 + r) * H + u;
    h_nxt[dst] = h_cur[src];
    c_nxt[dst] = c_cur[src];
  }
}

// mmseq_order_score, one workgroup per slot (story b, candidate k): the candidate's N - 1 picks
// are validated BEFORE any of them is used as an index; the whole seq row is written here, once
// (an invalid candidate runs as 0, 1, .., N-2 so that every later indexed read stays in bounds,
// and is marked bad), (h, c) <- (h0, c0), nll <- 0, or +inf with its step_nll row where bad.
__global__ __launch_bounds__(256) void order_init_kernel(int N, int H, int K,
                                                         const int64_t* __restrict__ orders,
                                                         int64_t story_stride,
                                                         const float* __restrict__ h0,
                                                         const float* __restrict__ c0,
                                                         float* __restrict__ h, float* __restrict__ c,
                                                         float* __restrict__ zero,
                                                         int* __restrict__ seq, int* __restrict__ bad,
                                                         float* __restrict__ nll,
                                                         float* __restrict__ step_nll) {
  const int64_t slot = blockIdx.x;
  const int b = (int)(slot / K), k = (int)(slot % K);
  if (N == 1) {
    if (threadIdx.x == 0) nll[slot] = 0.f;
    return;
  }
  const int64_t* cand = orders + (int64_t)b * story_stride + (int64_t)k * N;
  const bool ok = candidate_ok(cand, N);
  const int p = threadIdx.x;
  if (p < N - 1) seq[slot * BEAM_MAXN + p] = ok ? (int)cand[p] : p;
  if (threadIdx.x == 0) {
    bad[slot] = ok ? 0 : 1;
    zero[slot] = 0.f;
    nll[slot] = ok ? 0.f : INFINITY;
  }
  if (!ok && step_nll && threadIdx.x < N - 1) step_nll[slot * (N - 1) + threadIdx.x] = INFINITY;
  for (int u = threadIdx.x; u < H; u += 256) {
    h[slot * H + u] = h0[(int64_t)b * H + u];
    c[slot * H + u] = c0[(int64_t)b * H + u];
  }
}

// One thread per slot after beam_score_kernel of step t (entered with score 0, so s = -logp):
// the step's -logp of the slot's own t-th pick, added to nll in step order.
__global__ __launch_bounds__(256) void order_pick_kernel(int64_t R, int N, int t,
                                                         const float* __restrict__ s,
                                                         const int* __restrict__ seq,
                                                         const int* __restrict__ bad,
                                                         float* __restrict__ nll,
                                                         float* __restrict__ step_nll) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= R || bad[slot]) return;
  const float v = s[slot * N + seq[slot * BEAM_MAXN + t]];
  nll[slot] += v;
  if (step_nll) step_nll[slot * (N - 1) + t] = v;
}

// mmseq_order_sample, one workgroup per slot (story b, sample s): (h, c) <- (h0, c0), nll <- 0 and
// the score every step is entered with <- 0. N == 1: the order is [0].
__global__ __launch_bounds__(256) void sample_init_kernel(int N, int H, int S,
                                                          const float* __restrict__ h0,
                                                          const float* __restrict__ c0,
                                                          float* __restrict__ h, float* __restrict__ c,
                                                          float* __restrict__ zero,
                                                          int64_t* __restrict__ orders,
                                                          float* __restrict__ nll) {
  const int64_t slot = blockIdx.x;
  const int b = (int)(slot / S);
  if (threadIdx.x == 0) {
    nll[slot] = 0.f;
    if (N == 1) orders[slot] = 0;
  }
  if (N == 1) return;
  if (threadIdx.x == 0) zero[slot] = 0.f;
  for (int u = threadIdx.x; u < H; u += 256) {
    h[slot * H + u] = h0[(int64_t)b * H + u];
    c[slot * H + u] = c0[(int64_t)b * H + u];
  }
}

// One thread per slot after beam_score_kernel of step t (entered with score 0, so s = -logp): the
// slot's t-th pick by inversion of the step's distribution. u = (h >> 8) 2^-24 from the counter
// hash of mmseq_mlm_mask (two lowbias32 rounds) at element (story0 + b) 2^32 + (sample0 + s)(N-1)
// + t; j ascends over the unpointed steps with a running f32 sum of exp(-s_j) and the first j whose
// sum exceeds u * total is taken (total: the same sum to the end), else the last unpointed one.
__global__ __launch_bounds__(256) void sample_pick_kernel(int64_t R, int N, int S, int t,
                                                          uint32_t k0, uint32_t k1, uint32_t story0,
                                                          uint32_t sample0,
                                                          const float* __restrict__ s,
                                                          int* __restrict__ seq,
                                                          int64_t* __restrict__ orders,
                                                          float* __restrict__ nll,
                                                          float* __restrict__ u_out,
                                                          float* __restrict__ step_nlp) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= R) return;
  const uint32_t b = (uint32_t)(slot / S), smp = (uint32_t)(slot % S);
  const uint32_t lo = (sample0 + smp) * (uint32_t)(N - 1) + (uint32_t)t, hi = story0 + b;
  const uint32_t h = drop_mix(drop_mix(lo ^ k0) + (hi ^ k1));
  const float u = (float)(h >> 8) * 0x1p-24f;
  const unsigned pointed = pointed_mask(seq + slot * BEAM_MAXN, t);
  const float* row = s + slot * N;
  float total = 0.f;
  for (int j = 0; j < N; ++j)
    if (!((pointed >> j) & 1u)) total += expf(-row[j]);
  const float thr = u * total;
  float run = 0.f;
  int pick = -1, last = 0;
  for (int j = 0; j < N; ++j) {
    if ((pointed >> j) & 1u) continue;
    run += expf(-row[j]);
    last = j;
    if (pick < 0 && run > thr) pick = j;
  }
  if (pick < 0) pick = last;
  seq[slot * BEAM_MAXN + t] = pick;
  nll[slot] += row[pick];
  orders[slot * N + t] = pick;
  if (t == N - 2) {  // the last position is the one step left
    orders[slot * N + N - 1] = lowest_free(pointed | (1u << pick));
  }
  if (u_out) u_out[slot * (N - 1) + t] = u;
  if (step_nlp)
    for (int j = 0; j < N; ++j)
      step_nlp[(slot * (N - 1) + t) * N + j] = ((pointed >> j) & 1u) ? INFINITY : row[j];
}

inline bool beam_supported(int B, int N, int H, int W) {
  return B >= 0 && N >= 1 && N <= BEAM_MAXN && W >= 1 && W <= BEAM_MAXW && H >= 1 &&
         (int64_t)B * BEAM_MAXW * BEAM_MAXN * 4 < INT32_MAX / 2 && (int64_t)H * 4 * 4 < INT32_MAX / 2;
}

// the per-story limits of the beam, and B*K rows of 4H floats within 32-bit element counts
inline bool score_supported(int B, int N, int H, int K) {
  return beam_supported(B, N, H, 1) && K >= 1 && (int64_t)B * K * 4 * H < INT32_MAX &&
         (int64_t)B * K * BEAM_MAXN < INT32_MAX;
}

// step t of R = B*W slots, nb of them live per story: LSTM cell in place, query, s = score - logp
mmseq_status beam_step(int B, int N, int H, int W, int t, int nb, const DecoderWeights& wt,
                       const float* okey, const float* gx, const float* proj, int64_t pstride,
                       const int* seq, const float* score, float* h, float* c, float* gh, float* q,
                       float* s, mmseq_stream stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int R = B * W;
  mmseq_status e;
  const GemmSlab none{nullptr, 0};
  if ((e = dec_gemm(R, 4 * H, H, h, H, wt.w_hh, H, gh, 4 * H, wt.b_hh, 0, none, stream)) != MMSEQ_OK)
    return e;
  hipLaunchKernelGGL(beam_cell_kernel, dim3(R), dim3(256), 0, st, H, W, N, t, nb, gx, wt.b_ih, gh,
                     seq, h, c);
  if ((e = mmseq_check_launch("beam_cell")) != MMSEQ_OK) return e;
  if ((e = dec_gemm(R, H, H, h, H, wt.w_q, H, q, H, wt.b_q, 0, none, stream)) != MMSEQ_OK) return e;
  hipLaunchKernelGGL(beam_score_kernel, dim3(R), dim3(256), 0, st, N, H, W, t, nb, q, proj, pstride,
                     okey, wt.w_t, wt.b_t, seq, score, s);
  return mmseq_check_launch("beam_score");
}

// mmseq_beam_search (order / score) and mmseq_beam_search_nbest (nbest) are this one decode
mmseq_status beam_run(const char* what, int B, int N, int H, int W, const float* doc,
                      const float* okey, const float* hist, const float* h0, const float* c0,
                      const DecoderWeights& wt, int64_t* order, float* score, NBest nbest,
                      void* workspace, int64_t workspace_bytes, mmseq_stream stream) {
  if (!beam_supported(B, N, H, W))
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "%s: B=%d N=%d H=%d W=%d outside 1 <= N <= %d, 1 <= W <= %d "
                           "(or B*W*N / H too large for 32-bit row counts)",
                           what, B, N, H, W, BEAM_MAXN, BEAM_MAXW);
  const BeamWs L = beam_layout(B, N, H, W);
  mmseq_status e = decoder_require(
      what, doc, okey, hist, h0, c0, wt,
      (order && score) || (nbest.orders && nbest.scores && nbest.count), "", workspace,
      workspace_bytes, L.total * 4);
  if (e != MMSEQ_OK || B == 0) return e;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* ws = reinterpret_cast<float*>(workspace);
  float* hb[2] = {ws + L.h[0], ws + L.h[1]};
  float* cb[2] = {ws + L.c[0], ws + L.c[1]};
  float* sc[2] = {ws + L.score[0], ws + L.score[1]};
  int* sq[2] = {reinterpret_cast<int*>(ws + L.seq[0]), reinterpret_cast<int*>(ws + L.seq[1])};
  hipLaunchKernelGGL(beam_init_kernel, dim3(B), dim3(256), 0, st, N, H, W, h0, c0, hb[0], cb[0],
                     sc[0], order, score, nbest);
  e = mmseq_check_launch("beam_init");
  if (e != MMSEQ_OK || N == 1) return e;
  const int64_t pstride = up4((int64_t)B * N * N * H);
  if ((e = story_setup(B, N, H, doc, hist, wt, ws + L.gx, ws + L.proj, pstride, stream)) !=
      MMSEQ_OK)
    return e;
  int nb = 1;
  for (int t = 0; t < N - 1; ++t) {
    const int cur = t & 1, nxt = cur ^ 1, last = t == N - 2;
    const int n = nb * N, k = W < n ? W : n;
    if ((e = beam_step(B, N, H, W, t, nb, wt, okey, ws + L.gx, ws + L.proj, pstride, sq[cur],
                       sc[cur], hb[cur], cb[cur], ws + L.gh, ws + L.q, ws + L.s, stream)) != MMSEQ_OK)
      return e;
    hipLaunchKernelGGL(beam_select_kernel, dim3(B), dim3(256), 0, st, N, H, W, t, nb, k, last,
                       ws + L.s, sq[cur], sq[nxt], sc[nxt], hb[cur], cb[cur], hb[nxt], cb[nxt],
                       order, score, nbest);
    if ((e = mmseq_check_launch("beam_select")) != MMSEQ_OK) return e;
    nb = k;
  }
  return MMSEQ_OK;
}

// ------------------------------------------------------------------------------------------------
// mmseq_order_tree: all N! pointer scores from the prefix tree, walked level by level in chunks
// (order_tree_plan.h). A chunk holds nodes base .. base + cnt - 1 of its level for every story,
// rows [B][cnt]; every index below follows from the slot index and the chunk's base alone.

// r-th zero bit (ascending) of a mask that has more than r zero bits among its low bits
__device__ __forceinline__ int tree_nth_free(unsigned pointed, int r) {
  int j = 0;
  for (; j < BEAM_MAXN - 1; ++j) {  // bounded whatever the mask holds
    if ((pointed >> j) & 1u) continue;
    if (r == 0) break;
    --r;
  }
  return j;
}

// level 0: row b <- (h0, c0), entering score 0. N == 1: the one order's nll is 0.
__global__ __launch_bounds__(256) void tree_root_kernel(int N, int H, const float* __restrict__ h0,
                                                        const float* __restrict__ c0,
                                                        float* __restrict__ h, float* __restrict__ c,
                                                        float* __restrict__ score,
                                                        float* __restrict__ nll) {
  const int64_t b = blockIdx.x;
  if (N == 1) {
    if (threadIdx.x == 0) nll[b] = 0.f;
    return;
  }
  for (int u = threadIdx.x; u < H; u += 256) {
    h[b * H + u] = h0[b * H + u];
    c[b * H + u] = c0[b * H + u];
  }
  if (threadIdx.x == 0) score[b] = 0.f;
}

// One workgroup per child slot (story b, node cbase + j of level t, t >= 1 picks made): its parent
// is node i / (N-t+1) of level t - 1, row b * pcnt + (that - pbase) of the resident parent chunk,
// and its pick the (i % (N-t+1))-th zero bit of the parent's pointed mask. The child's pick row is
// the parent's plus the pick, its entering score the parent's s[pick], and its (h, c) the parent's
// post-step rows (the cell kernel updates in place, so they are copied): 16-byte accesses where
// H % 4 == 0 (every buffer offset is a multiple of 4 floats), a scalar path otherwise.
__global__ __launch_bounds__(256) void tree_expand_kernel(int N, int H, int t, int64_t cbase,
                                                          int64_t ccnt, int64_t pbase, int64_t pcnt,
                                                          const int* __restrict__ pseq,
                                                          const float* __restrict__ ps,
                                                          const float* __restrict__ ph,
                                                          const float* __restrict__ pc,
                                                          int* __restrict__ seq,
                                                          float* __restrict__ score,
                                                          float* __restrict__ h,
                                                          float* __restrict__ c) {
  const int64_t slot = blockIdx.x;
  const int64_t b = slot / ccnt, i = cbase + slot % ccnt;
  const int fan = N - t + 1;
  const int64_t prow = b * pcnt + (i / fan - pbase);
  const int r = (int)(i % fan);
  const unsigned pointed = pointed_mask(pseq + prow * BEAM_MAXN, t - 1);
  const int pick = tree_nth_free(pointed, r);
  if ((int)threadIdx.x < t - 1)
    seq[slot * BEAM_MAXN + threadIdx.x] = pseq[prow * BEAM_MAXN + threadIdx.x];
  if (threadIdx.x == 0) {
    seq[slot * BEAM_MAXN + t - 1] = pick;
    score[slot] = ps[prow * N + pick];
  }
  if ((H & 3) == 0) {
    const float4* sh = reinterpret_cast<const float4*>(ph + prow * H);
    const float4* sc = reinterpret_cast<const float4*>(pc + prow * H);
    float4* dh = reinterpret_cast<float4*>(h + slot * H);
    float4* dc = reinterpret_cast<float4*>(c + slot * H);
    for (int u = threadIdx.x; u < H / 4; u += 256) {
      dh[u] = sh[u];
      dc[u] = sc[u];
    }
  } else {
    for (int u = threadIdx.x; u < H; u += 256) {
      h[slot * H + u] = ph[prow * H + u];
      c[slot * H + u] = pc[prow * H + u];
    }
  }
}

// One thread per slot of a chunk of level N - 2 after its step: the two steps still unpointed,
// ascending, are the node's children 2i and 2i + 1 of level N - 1, i.e. two lexicographic ranks
// (N = 2: the root's both picks); their s entries are those orders' nll.
__global__ __launch_bounds__(256) void tree_leaf_kernel(int64_t R, int N, int64_t base, int64_t cnt,
                                                        int64_t leaves, const int* __restrict__ seq,
                                                        const float* __restrict__ s,
                                                        float* __restrict__ nll) {
  const int64_t slot = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (slot >= R) return;
  const int64_t b = slot / cnt, i = base + slot % cnt;
  const unsigned pointed = pointed_mask(seq + slot * BEAM_MAXN, N - 2);
  const int j0 = tree_nth_free(pointed, 0), j1 = tree_nth_free(pointed | (1u << j0), 0);
  nll[b * leaves + 2 * i] = s[slot * N + j0];
  nll[b * leaves + 2 * i + 1] = s[slot * N + j1];
}

// One thread per rank k < N!: the k-th permutation of 0 .. N-1 in lexicographic order, digit p of
// k in the factorial number system picking the digit-th still-unused value, ascending.
__global__ __launch_bounds__(256) void tree_unrank_kernel(int64_t leaves, int N,
                                                          int64_t* __restrict__ orders) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= leaves) return;
  int64_t f = leaves, rem = k;
  unsigned used = 0;
  for (int p = 0; p < N; ++p) {
    f /= N - p;  // (N - 1 - p)!
    const int j = tree_nth_free(used, (int)(rem / f));
    rem %= f;
    used |= 1u << j;
    orders[k * N + p] = j;
  }
}

inline bool tree_supported(int B, int N, int H) {
  if (N < 1 || N > order_tree::MAXN || !beam_supported(B, N, H, 1)) return false;
  int64_t leaves = 1;
  for (int i = 2; i <= N; ++i) leaves *= i;
  return (int64_t)B * leaves < INT32_MAX && (int64_t)B * N * 4 * H < INT32_MAX;
}

}  // namespace

extern "C" int64_t mmseq_beam_workspace(int B, int N, int H, int W) {
  if (!beam_supported(B, N, H, W)) return 0;
  return beam_layout(B, N, H, W).total * 4;
}


extern "C" mmseq_status mmseq_beam_search(int B, int N, int H, int W, const float* doc,
                                          const float* okey, const float* hist, const float* h0,
                                          const float* c0, const float* w_ih, const float* b_ih,
                                          const float* w_hh, const float* b_hh, const float* w_q,
                                          const float* b_q, const float* w_pw, const float* w_t,
                                          const float* b_t, int64_t* order, float* score,
                                          void* workspace, int64_t workspace_bytes,
                                          mmseq_stream stream) {
  return beam_run("beam_search", B, N, H, W, doc, okey, hist, h0, c0,
                  DecoderWeights{w_ih, b_ih, w_hh, b_hh, w_q, b_q, w_pw, w_t, b_t}, order, score,
                  NBest{nullptr, nullptr, nullptr}, workspace, workspace_bytes, stream);
}

extern "C" mmseq_status mmseq_beam_search_nbest(int B, int N, int H, int W, const float* doc,
                                                const float* okey, const float* hist,
                                                const float* h0, const float* c0, const float* w_ih,
                                                const float* b_ih, const float* w_hh,
                                                const float* b_hh, const float* w_q,
                                                const float* b_q, const float* w_pw,
                                                const float* w_t, const float* b_t, int64_t* orders,
                                                float* scores, int32_t* count, void* workspace,
                                                int64_t workspace_bytes, mmseq_stream stream) {
  return beam_run("beam_search_nbest", B, N, H, W, doc, okey, hist, h0, c0,
                  DecoderWeights{w_ih, b_ih, w_hh, b_hh, w_q, b_q, w_pw, w_t, b_t}, nullptr, nullptr,
                  NBest{orders, scores, count}, workspace, workspace_bytes, stream);
}

extern "C" int64_t mmseq_order_score_workspace(int B, int N, int H, int K) {
  if (!score_supported(B, N, H, K)) return 0;
  return score_layout(B, N, H, K).total * 4;
}

extern "C" mmseq_status mmseq_order_score(int B, int N, int H, int K, const float* doc,
                                          const float* okey, const float* hist, const float* h0,
                                          const float* c0, const float* w_ih, const float* b_ih,
                                          const float* w_hh, const float* b_hh, const float* w_q,
                                          const float* b_q, const float* w_pw, const float* w_t,
                                          const float* b_t, const int64_t* orders,
                                          int64_t story_stride, float* nll, float* step_nll,
                                          void* workspace, int64_t workspace_bytes,
                                          mmseq_stream stream) {
  if (!score_supported(B, N, H, K))
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "order_score: B=%d N=%d H=%d K=%d outside 1 <= N <= %d, 1 <= K, "
                           "B*K*4H < 2^31 (or B / H too large for 32-bit row counts)",
                           B, N, H, K, BEAM_MAXN);
  char why[DEC_WHY] = "";
  if (!(story_stride == 0 || story_stride >= (int64_t)K * N))
    snprintf(why, sizeof why, "story_stride %lld is neither 0 (shared list) nor >= K*N",
             (long long)story_stride);
  const DecoderWeights wt{w_ih, b_ih, w_hh, b_hh, w_q, b_q, w_pw, w_t, b_t};
  const ScoreWs L = score_layout(B, N, H, K);
  mmseq_status e = decoder_require("order_score", doc, okey, hist, h0, c0, wt, orders && nll, why,
                                   workspace, workspace_bytes, L.total * 4);
  if (e != MMSEQ_OK || B == 0) return e;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* ws = reinterpret_cast<float*>(workspace);
  const int R = B * K;
  int* seq = reinterpret_cast<int*>(ws + L.seq);
  int* bad = reinterpret_cast<int*>(ws + L.bad);
  hipLaunchKernelGGL(order_init_kernel, dim3(R), dim3(256), 0, st, N, H, K, orders, story_stride,
                     h0, c0, ws + L.h, ws + L.c, ws + L.zero, seq, bad, nll, step_nll);
  e = mmseq_check_launch("order_init");
  if (e != MMSEQ_OK || N == 1) return e;
  const int64_t pstride = up4((int64_t)B * N * N * H);
  if ((e = story_setup(B, N, H, doc, hist, wt, ws + L.gx, ws + L.proj, pstride, stream)) !=
      MMSEQ_OK)
    return e;
  for (int t = 0; t < N - 1; ++t) {  // every slot is live (nb = K) and enters with score 0
    if ((e = beam_step(B, N, H, K, t, K, wt, okey, ws + L.gx, ws + L.proj, pstride, seq,
                       ws + L.zero, ws + L.h, ws + L.c, ws + L.gh, ws + L.q, ws + L.s, stream)) !=
        MMSEQ_OK)
      return e;
    hipLaunchKernelGGL(order_pick_kernel, dim3((R + 255) / 256), dim3(256), 0, st, (int64_t)R, N, t,
                       ws + L.s, seq, bad, nll, step_nll);
    if ((e = mmseq_check_launch("order_pick")) != MMSEQ_OK) return e;
  }
  return MMSEQ_OK;
}

extern "C" int64_t mmseq_order_sample_workspace(int B, int N, int H, int S) {
  if (!score_supported(B, N, H, S)) return 0;
  return score_layout(B, N, H, S).total * 4;
}

extern "C" mmseq_status mmseq_order_sample(int B, int N, int H, int S, const float* doc,
                                           const float* okey, const float* hist, const float* h0,
                                           const float* c0, const float* w_ih, const float* b_ih,
                                           const float* w_hh, const float* b_hh, const float* w_q,
                                           const float* b_q, const float* w_pw, const float* w_t,
                                           const float* b_t, uint64_t seed, uint32_t stream_id,
                                           int story0, int sample0, int64_t* orders, float* nll,
                                           float* u, float* step_nlp, void* workspace,
                                           int64_t workspace_bytes, mmseq_stream stream) {
  if (!score_supported(B, N, H, S))
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "order_sample: B=%d N=%d H=%d S=%d outside 1 <= N <= %d, 1 <= S, "
                           "B*S*4H < 2^31 (or B / H too large for 32-bit row counts)",
                           B, N, H, S, BEAM_MAXN);
  char why[DEC_WHY] = "";
  if (!(story0 >= 0 && sample0 >= 0 && (int64_t)story0 + B < INT32_MAX &&
        ((int64_t)sample0 + S) * BEAM_MAXN < INT32_MAX))
    snprintf(why, sizeof why, "story0 %d / sample0 %d negative or beyond the 32-bit counter words",
             story0, sample0);
  const ScoreWs L = score_layout(B, N, H, S);  // the scorer's layout; its `bad` row is not used
  const DecoderWeights wt{w_ih, b_ih, w_hh, b_hh, w_q, b_q, w_pw, w_t, b_t};
  mmseq_status e = decoder_require("order_sample", doc, okey, hist, h0, c0, wt, orders && nll, why,
                                   workspace, workspace_bytes, L.total * 4);
  if (e != MMSEQ_OK || B == 0) return e;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  float* ws = reinterpret_cast<float*>(workspace);
  const int R = B * S;
  int* seq = reinterpret_cast<int*>(ws + L.seq);
  hipLaunchKernelGGL(sample_init_kernel, dim3(R), dim3(256), 0, st, N, H, S, h0, c0, ws + L.h,
                     ws + L.c, ws + L.zero, orders, nll);
  e = mmseq_check_launch("sample_init");
  if (e != MMSEQ_OK || N == 1) return e;
  const mmseq_dropout key = {0.5f, stream_id, seed};  // the dropout key schedule; p is not used
  const Drop d = make_drop(&key);
  const int64_t pstride = up4((int64_t)B * N * N * H);
  if ((e = story_setup(B, N, H, doc, hist, wt, ws + L.gx, ws + L.proj, pstride, stream)) !=
      MMSEQ_OK)
    return e;
  for (int t = 0; t < N - 1; ++t) {  // every slot is live (nb = S) and enters with score 0
    if ((e = beam_step(B, N, H, S, t, S, wt, okey, ws + L.gx, ws + L.proj, pstride, seq,
                       ws + L.zero, ws + L.h, ws + L.c, ws + L.gh, ws + L.q, ws + L.s, stream)) !=
        MMSEQ_OK)
      return e;
    hipLaunchKernelGGL(sample_pick_kernel, dim3((R + 255) / 256), dim3(256), 0, st, (int64_t)R, N, S,
                       t, d.k0, d.k1, (uint32_t)story0, (uint32_t)sample0, ws + L.s, seq, orders,
                       nll, u, step_nlp);
    if ((e = mmseq_check_launch("sample_pick")) != MMSEQ_OK) return e;
  }
  return MMSEQ_OK;
}

extern "C" int64_t mmseq_order_tree_workspace(int B, int N, int H, int64_t rows) {
  order_tree::Plan P;
  if (!tree_supported(B, N, H) || !order_tree::make_plan(B, N, H, rows, &P)) return 0;
  return P.total * 4;
}

extern "C" mmseq_status mmseq_order_tree(int B, int N, int H, const float* doc, const float* okey,
                                         const float* hist, const float* h0, const float* c0,
                                         const float* w_ih, const float* b_ih, const float* w_hh,
                                         const float* b_hh, const float* w_q, const float* b_q,
                                         const float* w_pw, const float* w_t, const float* b_t,
                                         int64_t rows, float* nll, int64_t* orders, void* workspace,
                                         int64_t workspace_bytes, mmseq_stream stream) {
  if (!tree_supported(B, N, H))
    return mmseq_set_error(MMSEQ_EUNSUPPORTED,
                           "order_tree: B=%d N=%d H=%d outside 1 <= N <= %d, B*N! < 2^31, "
                           "B*N*4H < 2^31 (or B / H beyond the beam's limits)",
                           B, N, H, order_tree::MAXN);
  order_tree::Plan P;
  char why[DEC_WHY] = "";
  if (rows < (int64_t)B * N)
    snprintf(why, sizeof why, "rows %lld below B*N = %lld", (long long)rows, (long long)B * N);
  else if (!order_tree::make_plan(B, N, H, rows, &P))
    snprintf(why, sizeof why, "no plan for rows %lld", (long long)rows);
  const DecoderWeights wt{w_ih, b_ih, w_hh, b_hh, w_q, b_q, w_pw, w_t, b_t};
  mmseq_status e = decoder_require("order_tree", doc, okey, hist, h0, c0, wt, nll != nullptr, why,
                                   workspace, workspace_bytes, why[0] ? 0 : P.total * 4);
  if (e != MMSEQ_OK) return e;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (orders) {
    hipLaunchKernelGGL(tree_unrank_kernel, dim3((unsigned)((P.leaves + 255) / 256)), dim3(256), 0,
                       st, P.leaves, N, orders);
    if ((e = mmseq_check_launch("tree_unrank")) != MMSEQ_OK) return e;
  }
  if (B == 0) return MMSEQ_OK;
  float* ws = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(tree_root_kernel, dim3(B), dim3(256), 0, st, N, H, h0, c0, ws + P.lv[0].h,
                     ws + P.lv[0].c, ws + P.lv[0].score, nll);
  if ((e = mmseq_check_launch("tree_root")) != MMSEQ_OK || N == 1) return e;
  if ((e = story_setup(B, N, H, doc, hist, wt, ws + P.gx, ws + P.proj, P.pstride, stream)) !=
      MMSEQ_OK)
    return e;
  e = MMSEQ_OK;
  order_tree::walk(P, [&](int t, int64_t base, int64_t cnt, int64_t pbase, int64_t pcnt) {
    const order_tree::Level& L = P.lv[t];
    const int R = (int)(B * cnt);
    int* seq = reinterpret_cast<int*>(ws + L.seq);
    if (t > 0) {
      const order_tree::Level& U = P.lv[t - 1];
      hipLaunchKernelGGL(tree_expand_kernel, dim3(R), dim3(256), 0, st, N, H, t, base, cnt, pbase,
                         pcnt, reinterpret_cast<const int*>(ws + U.seq), ws + U.s, ws + U.h,
                         ws + U.c, seq, ws + L.score, ws + L.h, ws + L.c);
      if ((e = mmseq_check_launch("tree_expand")) != MMSEQ_OK) return false;
    }
    // the chunk as a beam of W = nb = cnt live slots per story: slot / cnt is the story
    if ((e = beam_step(B, N, H, (int)cnt, t, (int)cnt, wt, okey, ws + P.gx, ws + P.proj, P.pstride,
                       seq, ws + L.score, ws + L.h, ws + L.c, ws + P.gh, ws + P.q, ws + L.s,
                       stream)) != MMSEQ_OK)
      return false;
    if (t == N - 2) {
      hipLaunchKernelGGL(tree_leaf_kernel, dim3((R + 255) / 256), dim3(256), 0, st, (int64_t)R, N,
                         base, cnt, P.leaves, seq, ws + L.s, nll);
      if ((e = mmseq_check_launch("tree_leaf")) != MMSEQ_OK) return false;
    }
    return true;
  });
  return e;
}
