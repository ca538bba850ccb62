// Stand-alone host check of the chunk planner of mmseq_order_tree (csrc/order_tree_plan.h), built
// by tests/test_order_tree.py with the host compiler and -fsanitize=address,undefined.
//   order_tree_plan_main N B H rows [N B H rows ...]
// walks the plan of every group of four arguments and verifies that every (level, node) is covered
// exactly once (a chunk holds the same node range of every story, so one count per node stands for
// all B stories), that every
// buffer's offset plus the extent a chunk uses lies within the workspace and overlaps no other
// buffer, that a chunk never holds more than `rows` slot rows, and that the parent chunk of every
// chunk is the resident chunk of the level above when the chunk is expanded. Prints
//   ok N B H rows chunks steps bytes
// per group and exits 0, or prints what failed and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "order_tree_plan.h"

namespace ot = order_tree;

static int fail(const char* what, long long a = 0, long long b = 0) {
  std::printf("FAILED: %s (%lld, %lld)\n", what, a, b);
  return 1;
}

static int check(int N, int B, int H, int64_t rows) {
  ot::Plan P;
  // what the planner must refuse
  if (ot::make_plan(B, 0, H, rows, &P)) return fail("N = 0 planned");
  if (ot::make_plan(B, ot::MAXN + 1, H, rows + 10 * (int64_t)B, &P)) return fail("N = 10 planned");
  if (B > 0 && ot::make_plan(B, N, H, (int64_t)B * N - 1, &P)) return fail("rows < B*N planned");
  if (!ot::make_plan(B, N, H, rows, &P)) return fail("no plan");

  // workspace: buffers within the total, none overlapping, all 16-byte aligned
  std::vector<std::pair<int64_t, int64_t>> bufs;  // (offset, extent) in floats
  bufs.push_back({P.gx, (int64_t)B * N * 4 * H});
  for (int g = 0; g < 4; ++g) bufs.push_back({P.proj + g * P.pstride, (int64_t)B * N * N * H});
  bufs.push_back({P.gh, P.max_rows * 4 * H});
  bufs.push_back({P.q, P.max_rows * H});
  int64_t width = 1, steps = 0;
  for (int t = 0; t < P.levels; ++t) {
    const ot::Level& L = P.lv[t];
    if (L.width != width) return fail("level width", t, L.width);
    if (L.cap < 1 || L.cap > L.width || (int64_t)B * L.cap > std::max<int64_t>(rows, B))
      return fail("level cap", t, L.cap);
    const int64_t R = (int64_t)B * L.cap;
    bufs.push_back({L.h, R * H});
    bufs.push_back({L.c, R * H});
    bufs.push_back({L.s, R * N});
    bufs.push_back({L.score, R});
    bufs.push_back({L.seq, R * ot::SEQ_STRIDE});
    steps += width;
    width *= N - t;
  }
  if (steps != P.steps) return fail("steps", steps, P.steps);
  std::sort(bufs.begin(), bufs.end());
  for (size_t i = 0; i < bufs.size(); ++i) {
    if (bufs[i].first % 4) return fail("unaligned offset", bufs[i].first);
    if (bufs[i].first < 0 || bufs[i].first + bufs[i].second > P.total)
      return fail("buffer beyond the workspace", bufs[i].first, bufs[i].second);
    if (i + 1 < bufs.size() && bufs[i].first + bufs[i].second > bufs[i + 1].first)
      return fail("buffers overlap", bufs[i].first, bufs[i + 1].first);
  }

  // the walk
  std::vector<std::vector<unsigned char>> seen(P.levels > 0 ? P.levels : 0);
  for (int t = 0; t < P.levels; ++t) seen[t].assign(P.lv[t].width, 0);
  std::vector<std::pair<int64_t, int64_t>> resident(ot::MAXN, {-1, -1});
  int64_t chunks = 0;
  const char* why = nullptr;
  const bool done = ot::walk(P, [&](int t, int64_t base, int64_t cnt, int64_t pbase, int64_t pcnt) {
    ++chunks;
    if (t < 0 || t >= P.levels) { why = "level out of range"; return false; }
    const ot::Level& L = P.lv[t];
    if (cnt < 1 || cnt > L.cap || base < 0 || base + cnt > L.width) {
      why = "chunk outside its level or above its buffer's capacity";
      return false;
    }
    if ((int64_t)B * cnt > std::max<int64_t>(rows, B)) { why = "chunk above rows"; return false; }
    if (t == 0) {
      if (base != 0 || cnt != 1) { why = "root chunk"; return false; }
    } else {
      const int64_t fan = N - t + 1;
      if (resident[t - 1] != std::make_pair(pbase, pcnt)) { why = "parent not resident"; return false; }
      if (base / fan < pbase || (base + cnt - 1) / fan >= pbase + pcnt) {
        why = "a node's parent lies outside the resident parent chunk";
        return false;
      }
    }
    resident[t] = {base, cnt};
    for (int u = t + 1; u < ot::MAXN; ++u) resident[u] = {-1, -1};  // overwritten from here down
    for (int64_t i = base; i < base + cnt; ++i) {
      if (seen[t][i]) { why = "node covered twice"; return false; }
      seen[t][i] = 1;
    }
    return true;
  });
  if (!done) return fail(why ? why : "walk stopped");
  for (int t = 0; t < P.levels; ++t)
    for (int64_t i = 0; i < P.lv[t].width; ++i)
      if (!seen[t][i]) return fail("node not covered", t, i);
  if (chunks != P.chunks) return fail("chunk count", chunks, P.chunks);
  std::printf("ok %d %d %d %lld %lld %lld %lld\n", N, B, H, (long long)rows, (long long)P.chunks,
              (long long)P.steps, (long long)(P.total * 4));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 5 || (argc - 1) % 4) return fail("usage: N B H rows [N B H rows ...]");
  for (int a = 1; a < argc; a += 4)
    if (check(std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 2]),
              std::atoll(argv[a + 3])))
      return 1;
  return 0;
}
