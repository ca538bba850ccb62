// Chunk planner of mmseq_order_tree (include/mmseq.h, csrc/beam.hip): level widths, per-level chunk
// capacities, workspace offsets and the depth-first chunk schedule of the prefix tree over all N!
// orders. Plain C++ with no HIP dependency: the entry point includes it, and so can a stand-alone
// host program (tests/order_tree_plan_main.cpp runs it under the host sanitizers).
//
// Level t = 0 .. N-2 holds the prefixes with t picks made, width(t) = N! / (N-t)! per story; node
// i of level t has the N - t children i * (N-t) + r, r = 0 .. N-t-1 (the r-th still-unpointed
// step, ascending), so a node of level N-1 is an order's lexicographic rank. Every level owns ONE
// state buffer of cap(t) = min(width(t), rows / B) nodes per story; a chunk is the same node range
// [base, base + cnt) of every story, laid out [B][cnt], so that slot / cnt is the story (the form
// beam_step needs). The walk steps a chunk, then visits the chunks of its children one after the
// other, each to the bottom before the next: a chunk's parent is the chunk last stepped one level
// up and stays resident until all of its children are done. The schedule is a function of
// (B, N, rows) alone.
#pragma once
#include <cstdint>

namespace order_tree {

constexpr int MAXN = 9;       // 9! = 362880 orders
constexpr int SEQ_STRIDE = 16;  // int32 picks per slot row (BEAM_MAXN of csrc/beam.hip)

struct Level {
  int64_t width, cap;             // nodes per story; nodes per story the level's buffer holds
  int64_t h, c, s, score, seq;    // float offsets into the workspace, multiples of 4
};

struct Plan {
  int B, N, H;
  int levels;       // step levels: N - 1 (0 for N = 1)
  int64_t leaves;   // N!
  int64_t max_rows; // B * the largest cap: rows of the two scratch buffers gh and q
  int64_t gx, proj, pstride, gh, q, total;  // float offsets; total floats of the workspace
  int64_t chunks, steps;  // chunks over all levels; node-steps per story = sum_t width(t)
  Level lv[MAXN];
};

inline int64_t up4(int64_t n) { return (n + 3) / 4 * 4; }

// visit(t, base, cnt, pbase, pcnt) -> false stops the walk. (pbase, pcnt) is the resident chunk of
// level t - 1 that holds the parents of nodes base .. base + cnt - 1 (0, 0 for the root).
template <class F>
bool walk_level(const Plan& p, int t, int64_t base, int64_t cnt, int64_t pbase, int64_t pcnt,
                F& visit) {
  if (!visit(t, base, cnt, pbase, pcnt)) return false;
  if (t >= p.N - 2) return true;
  const int64_t fan = p.N - t, lo = base * fan, hi = (base + cnt) * fan, cap = p.lv[t + 1].cap;
  for (int64_t cb = lo; cb < hi; cb += cap)
    if (!walk_level(p, t + 1, cb, hi - cb < cap ? hi - cb : cap, base, cnt, visit)) return false;
  return true;
}

template <class F>
bool walk(const Plan& p, F visit) {
  if (p.N < 2) return true;
  return walk_level(p, 0, 0, 1, 0, 0, visit);
}

// false: B < 0, N outside 1 .. MAXN, H < 1, rows < B * N, or B * N rows of 4H floats beyond the
// 32-bit element counts of the dense parts. `rows` above that count is clamped to it.
inline bool make_plan(int B, int N, int H, int64_t rows, Plan* out) {
  if (B < 0 || N < 1 || N > MAXN || H < 1 || rows < (int64_t)B * N) return false;
  const int64_t Bq = B > 0 ? B : 1;
  int64_t lim = (INT32_MAX - 1) / (4 * (int64_t)H);        // rows * 4H < 2^31
  if (lim > (INT32_MAX - 1) / SEQ_STRIDE) lim = (INT32_MAX - 1) / SEQ_STRIDE;
  if (lim < Bq * N) return false;
  if (rows > lim) rows = lim;
  const int64_t per = rows / Bq > 0 ? rows / Bq : 1;       // nodes per story in one chunk
  Plan& p = *out;
  p.B = B; p.N = N; p.H = H;
  p.levels = N - 1;
  p.leaves = 1;
  for (int i = 2; i <= N; ++i) p.leaves *= i;
  int64_t o = 0;
  p.gx = o; o += up4((int64_t)B * N * 4 * H);
  p.pstride = up4((int64_t)B * N * N * H);
  p.proj = o; o += 4 * p.pstride;
  p.max_rows = 0;
  p.steps = 0;
  int64_t width = 1;
  for (int t = 0; t < p.levels; ++t) {
    Level& L = p.lv[t];
    L.width = width;
    L.cap = width < per ? width : per;
    const int64_t R = (int64_t)B * L.cap;
    if (R > p.max_rows) p.max_rows = R;
    L.h = o; o += up4(R * H);
    L.c = o; o += up4(R * H);
    L.s = o; o += up4(R * N);
    L.score = o; o += up4(R);
    L.seq = o; o += up4(R * SEQ_STRIDE);  // int32 picks
    p.steps += width;
    width *= N - t;
  }
  p.gh = o; o += up4(p.max_rows * 4 * H);
  p.q = o; o += up4(p.max_rows * H);
  p.total = o;
  p.chunks = 0;
  int64_t n = 0;
  walk(p, [&n](int, int64_t, int64_t, int64_t, int64_t) { ++n; return true; });
  p.chunks = n;
  return true;
}

}  // namespace order_tree
