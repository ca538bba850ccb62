// Pretraining inputs on device (text+image stage): dynamic MLM masking
// (trainers/train_utils.py:19-66 mask_tokens_sentence), the text of the sub-sampled steps
// (lxrt/modeling.py:1986-2032) and the ordered compaction of the labelled rows that sizes the
// masked-LM head's GEMMs.
//
// Integer work on a few thousand tokens per step, latency-bound: no MFMA, no LDS tiles beyond a
// story's cls positions, plain vector stores; the only atomic is the int32 bad-story counter.
#include "common.h"

namespace {

constexpr int kMaxSteps = 64;  // n_steps <= 64, as csrc/pairs.hip (one wave holds a story's steps)

// --- MLM masking: one thread per token, a pure function of (key, flat index) ----------------------
__global__ void __launch_bounds__(256) mlm_mask_kernel(
    int64_t n, int64_t* __restrict__ ids, int64_t* __restrict__ labels, int64_t pad_id,
    int64_t cls_id, int64_t mask_id, int64_t ignore_index, uint32_t span, uint32_t thr, uint32_t k0,
    uint32_t k1) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int64_t id = ids[e];
  // two lowbias32 rounds (one leaves a lag-64 correlation between the selection bits)
  const uint32_t h = drop_mix(drop_mix((uint32_t)e ^ k0) + ((uint32_t)((uint64_t)e >> 32) ^ k1));
  const bool selected = id != pad_id && id != cls_id && (h & 0xFFFFu) < thr;
  labels[e] = selected ? id : ignore_index;
  if (!selected) return;
  if ((h >> 16) < 52429u) {  // 80 %: round(0.8 * 2^16)
    ids[e] = mask_id;
    return;
  }
  const uint32_t h2 = drop_hash2(h);
  if ((h2 & 0xFFFFu) < 32768u) {  // half of the rest: a word of [cls_id + 1, vocab)
    const uint32_t h3 = drop_hash2(h2);
    ids[e] = cls_id + 1 + (int64_t)(((uint64_t)h3 * (uint64_t)span) >> 32);
  }
}

// --- sub-sampling: one wave per story ---------------------------------------------------------------
// cls positions by ballot over 64-token chunks (as pair_scan_kernel), then every lane walks the
// n_sub kept steps from LDS (uniform, n_sub <= 64) and the wave copies the [pad] output rows.
__global__ void __launch_bounds__(64) subsample_text_kernel(
    int L, int n_steps, int n_sub, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ mask, const int64_t* __restrict__ types,
    const int64_t* __restrict__ labels, const int64_t* __restrict__ sub_idx, int64_t cls_id,
    int64_t pad_id, int64_t ignore_index, int64_t* __restrict__ out_ids,
    int64_t* __restrict__ out_mask, int64_t* __restrict__ out_types,
    int64_t* __restrict__ out_labels, int* __restrict__ status) {
  __shared__ int s_cls[kMaxSteps];                      // position of the k-th cls token
  __shared__ int s_from[kMaxSteps], s_at[kMaxSteps + 1];  // kept step j: source start, output start
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t* row = ids + (int64_t)b * L;
  const uint64_t below = (1ull << lane) - 1ull;
  int ncls = 0;
  for (int base = 0; base < L; base += 64) {
    const int i = base + lane;
    const bool isc = i < L && row[i] == cls_id;
    const uint64_t mc = __ballot(isc);
    if (isc) {
      const int k = ncls + __popcll(mc & below);
      if (k < kMaxSteps) s_cls[k] = i;
    }
    ncls += __popcll(mc);
  }
  __syncthreads();
  const int per = L / n_steps, pad = per * n_sub;
  bool bad = false;
  int at = 0;
  for (int j = 0; j < n_sub; ++j) {
    const int64_t k = sub_idx[(int64_t)b * n_sub + j];
    int start = 0, end = 0;
    if (k < 0 || k >= n_steps || k >= ncls) {
      bad = true;  // no such step
    } else {
      start = s_cls[k];
      if (k == n_steps - 1) end = start + per;
      else if (k + 1 < ncls) end = s_cls[k + 1];
      else bad = true;  // the step's closing cls token is missing
    }
    if (!bad && (at + (end - start) > pad || end > L)) bad = true;
    if (bad) break;
    if (lane == 0) { s_from[j] = start; s_at[j] = at; }
    at += end - start;
  }
  if (lane == 0) {
    s_at[bad ? 0 : n_sub] = bad ? 0 : at;
    if (bad) atomicAdd(&status[0], 1);
  }
  __syncthreads();
  const int nseg = bad ? 0 : n_sub, filled = bad ? 0 : at;
  const int64_t in0 = (int64_t)b * L, out0 = (int64_t)b * pad;
  for (int t = lane; t < pad; t += 64) {
    const bool valid = t < filled;
    int64_t src = in0;
    if (valid) {
      int j = 0;
      while (j + 1 < nseg && s_at[j + 1] <= t) ++j;
      src += s_from[j] + (t - s_at[j]);
    }
    out_ids[out0 + t] = valid ? ids[src] : pad_id;
    out_mask[out0 + t] = valid ? mask[src] : 0;
    if (out_types) out_types[out0 + t] = valid ? types[src] : 0;
    if (out_labels) out_labels[out0 + t] = valid ? labels[src] : ignore_index;
  }
}

// --- ordered compaction: one workgroup walks the rows 1024 at a time --------------------------------
// Per chunk: a ballot per wave, the 16 wave counts through LDS (double-buffered: one barrier per
// chunk), every thread adds the counts of the waves before its own. The running total lives in a
// register of every thread, so the order is the row order and nothing is appended atomically.
constexpr int kCompactThreads = 1024;
__global__ void __launch_bounds__(kCompactThreads) rows_compact_kernel(
    int R, const int64_t* __restrict__ labels, int64_t ignore_index, int32_t* __restrict__ src,
    int64_t* __restrict__ out_labels, int32_t* __restrict__ count) {
  constexpr int kWaves = kCompactThreads / 64;
  __shared__ int s_cnt[2][kWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint64_t below = (1ull << lane) - 1ull;
  int total = 0, buf = 0;
  for (int64_t base = 0; base < R; base += kCompactThreads, buf ^= 1) {
    const int64_t i = base + tid;
    const int64_t v = i < R ? labels[i] : ignore_index;
    const bool keep = i < R && v != ignore_index;
    const uint64_t m = __ballot(keep);
    if (lane == 0) s_cnt[buf][wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const int c = s_cnt[buf][w];
      before += w < wave ? c : 0;
      all += c;
    }
    if (keep) {
      const int o = total + before + __popcll(m & below);
      src[o] = (int32_t)i;
      out_labels[o] = v;
    }
    total += all;
  }
  if (tid == 0) *count = total;
}

}  // namespace

extern "C" mmseq_status mmseq_mlm_mask(int B, int L, int64_t* input_ids, int64_t* labels,
                                       int64_t pad_id, int64_t cls_id, int64_t mask_id,
                                       int64_t vocab, int64_t ignore_index, float p, uint64_t seed,
                                       uint32_t stream_id, mmseq_stream stream) {
  MMSEQ_REQUIRE(B >= 0 && L > 0, "mlm_mask: bad sizes");
  const int64_t n = (int64_t)B * L;
  MMSEQ_REQUIRE(n < (1ll << 31), "mlm_mask: B * L must be below 2^31");
  MMSEQ_REQUIRE(vocab >= 1 && vocab < (1ll << 31) && cls_id >= -1 && cls_id < vocab - 1,
                "mlm_mask: 0 <= cls_id + 1 < vocab < 2^31 required (cls_id %lld, vocab %lld)",
                (long long)cls_id, (long long)vocab);
  MMSEQ_REQUIRE(p == p, "mlm_mask: p is NaN");
  MMSEQ_REQUIRE(input_ids && labels, "mlm_mask: null buffer");
  if (B == 0) return MMSEQ_OK;
  double t = floor((double)p * 65536.0 + 0.5);
  t = t < 0.0 ? 0.0 : (t > 65536.0 ? 65536.0 : t);
  const mmseq_dropout key = {0.5f, stream_id, seed};  // the dropout key schedule; p is not used
  const Drop d = make_drop(&key);
  hipLaunchKernelGGL(mlm_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), n, input_ids, labels, pad_id, cls_id,
                     mask_id, ignore_index, (uint32_t)(vocab - cls_id - 1), (uint32_t)t, d.k0, d.k1);
  return mmseq_check_launch("mlm_mask");
}

extern "C" mmseq_status mmseq_subsample_text(
    int B, int L, int n_steps, int n_sub, const int64_t* input_ids, const int64_t* attention_mask,
    const int64_t* token_type_ids, const int64_t* labels, const int64_t* sub_idx, int64_t cls_id,
    int64_t pad_id, int64_t ignore_index, int64_t* out_ids, int64_t* out_mask,
    int64_t* out_token_type, int64_t* out_labels, int32_t* status, mmseq_stream stream) {
  MMSEQ_REQUIRE(B >= 0 && L > 0 && n_steps >= 2 && n_steps <= kMaxSteps && n_sub >= 1 &&
                n_sub <= n_steps && L >= n_steps, "subsample_text: bad sizes");
  MMSEQ_REQUIRE(input_ids && attention_mask && sub_idx && out_ids && out_mask && status,
                "subsample_text: null buffer");
  MMSEQ_REQUIRE((token_type_ids != nullptr) == (out_token_type != nullptr) &&
                (labels != nullptr) == (out_labels != nullptr),
                "subsample_text: token types / labels need both their input and their output");
  if (B == 0) return MMSEQ_OK;
  hipLaunchKernelGGL(subsample_text_kernel, dim3(B), dim3(64), 0,
                     reinterpret_cast<hipStream_t>(stream), L, n_steps, n_sub, input_ids,
                     attention_mask, token_type_ids, labels, sub_idx, cls_id, pad_id, ignore_index,
                     out_ids, out_mask, out_token_type, out_labels, (int*)status);
  return mmseq_check_launch("subsample_text");
}

extern "C" mmseq_status mmseq_rows_compact(int R, const int64_t* labels, int64_t ignore_index,
                                           int32_t* src, int64_t* out_labels, int32_t* count,
                                           mmseq_stream stream) {
  MMSEQ_REQUIRE(R >= 0, "rows_compact: bad sizes");
  MMSEQ_REQUIRE(count && (R == 0 || (labels && src && out_labels)), "rows_compact: null buffer");
  hipLaunchKernelGGL(rows_compact_kernel, dim3(1), dim3(kCompactThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), R, labels, ignore_index, src, out_labels,
                     count);
  return mmseq_check_launch("rows_compact");
}
