// Split-K planning of the GEMM host side (gemm.hip): how many K splits a call takes, how long one
// split is and where its fp32 partials sit in the caller's workspace. Plain host C++ (no HIP, no
// state), so tests/gemm_plan_check.cpp checks it without a GPU. mmseq_gemm, mmseq_gemm_wgrad and
// mmseq_gemm_workspace_size take all of this arithmetic from here.
#pragma once
#include <cstdint>

namespace mmseq_gemm_plan {

struct SplitPlan {
  int splitk;           // K splits; 1 = unsplit (kchunk == K, no slab)
  int kchunk;           // K range of one split: a multiple of the kernel's K step when split
  int64_t slab_floats;  // partial slabs [splitk][M][N] at the start of the workspace (0 unsplit)
  int64_t cs_off;       // TN-256 bias partials [splitk][column tile][M]: float offset, -1 = none
  int64_t cs_floats;    // ... and their size (0 when none)
  int64_t bytes() const { return (slab_floats + cs_floats) * 4; }
};

constexpr int64_t kUnlimited = INT64_MAX;

// S wanted splits -> the plan that fits: S drops until S slabs (each with `cs_rows` more floats
// of bias partials) fit `ws_bytes`, kchunk is rounded up to the kernel's K step `step`, and the
// split count follows from the rounded chunk (so no split is empty)
inline SplitPlan fit_split(int64_t MN, int64_t cs_rows, int K, int64_t S, int step, int64_t ws_bytes) {
  while (S > 1 && S * (cs_rows + MN) * 4 > ws_bytes) --S;
  if (S > 1) {
    const int kchunk = (int)(((K + S - 1) / S + step - 1) / step * step);
    const int splitk = (K + kchunk - 1) / kchunk;
    if (splitk > 1) return {splitk, kchunk, splitk * MN, -1, 0};
  }
  return {1, K, 0, -1, 0};
}

inline int64_t tiles_of(int M, int N, int t) { return (int64_t)((M + t - 1) / t) * ((N + t - 1) / t); }

// 256 x 256 TN weight-gradient kernel: K split so that (tiles x splits) fills the CUs, at least
// 1024 of K per split. With a bias gradient every (split, column tile) has a partial row of M
// floats behind the slab when that fits (unsplit too); otherwise the first column tile adds its
// sums directly.
inline SplitPlan plan_tn256(int M, int N, int K, int num_cu, int64_t ws_bytes, bool bias) {
  const int64_t t256 = tiles_of(M, N, 256), tn256 = (N + 255) / 256;
  int64_t S = t256 < num_cu ? num_cu / t256 : 1;
  if (S > K / 1024) S = K / 1024 > 0 ? K / 1024 : 1;
  SplitPlan p = fit_split((int64_t)M * N, bias ? tn256 * M : 0, K, S, 128, ws_bytes);
  const int64_t cs = p.splitk * tn256 * M;
  if (bias && (p.slab_floats + cs) * 4 <= ws_bytes) { p.cs_off = p.slab_floats; p.cs_floats = cs; }
  return p;
}

// 128 x 128 TN kernel, fewer than 512 tiles: about 1024 workgroups, >= 16 K steps of 64 per split
inline SplitPlan plan_tn128(int M, int N, int K, int64_t ws_bytes) {
  const int64_t tiles = tiles_of(M, N, 128);
  if (tiles >= 512) return {1, K, 0, -1, 0};
  int64_t S = (1024 + tiles - 1) / tiles;
  if (S > K / 1024) S = K / 1024;
  return fit_split((int64_t)M * N, 0, K, S, 64, ws_bytes);
}

// fp32 kernel with few output tiles (< 128) and K >= 256: K over the CUs, >= 128 of K per split
inline SplitPlan plan_f32(int M, int N, int K, int num_cu, int64_t ws_bytes) {
  const int64_t tiles = tiles_of(M, N, 128);
  if (tiles >= 128 || K < 256) return {1, K, 0, -1, 0};
  int64_t S = (num_cu + tiles - 1) / tiles;
  if (S > K / 128) S = K / 128;
  return fit_split((int64_t)M * N, 0, K, S, 32, ws_bytes);
}

// Workspace bytes beyond which no plan changes: what each plan uses when nothing limits it
inline int64_t workspace_bound(int M, int N, int K, int num_cu) {
  const int64_t a = plan_tn256(M, N, K, num_cu, kUnlimited, true).bytes();
  const int64_t b = plan_tn128(M, N, K, kUnlimited).bytes();
  const int64_t c = plan_f32(M, N, K, num_cu, kUnlimited).bytes();
  return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

}  // namespace mmseq_gemm_plan
