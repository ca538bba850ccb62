// Stand-alone check of csrc/gemm_plan.h (built and run by tests/test_gemm_plan.py, no GPU): sweeps
// the three split-K plans and exits nonzero unless every plan is well formed, fits the workspace it
// was given, stays within workspace_bound(), and is at the bound what it is with unlimited
// workspace. Then prints the plans of a few named cases for the test to compare.
#include <cstdio>
#include "gemm_plan.h"

using namespace mmseq_gemm_plan;

static long g_bad = 0;

static void fail(const char* what, const char* plan, int M, int N, int K, int cu, long long ws, int bias) {
  if (++g_bad <= 20)
    std::printf("FAIL %s: %s M=%d N=%d K=%d cu=%d ws=%lld bias=%d\n", what, plan, M, N, K, cu, ws, bias);
}

static bool same(const SplitPlan& a, const SplitPlan& b) {
  return a.splitk == b.splitk && a.kchunk == b.kchunk && a.slab_floats == b.slab_floats &&
         a.cs_off == b.cs_off && a.cs_floats == b.cs_floats;
}

// `p` planned with `ws` bytes; `at_bound` / `unlimited`: the same plan with workspace_bound() bytes
// and with no limit; `step`: the kernel's K step
static void check(const char* plan, const SplitPlan& p, const SplitPlan& at_bound, const SplitPlan& unlimited,
                  int step, int M, int N, int K, int cu, int64_t ws, int bias) {
#define CHECK(cond) if (!(cond)) fail(#cond, plan, M, N, K, cu, (long long)ws, bias)
  const int64_t bound = workspace_bound(M, N, K, cu);
  CHECK(p.splitk >= 1);
  CHECK(p.splitk > 1 || p.kchunk == K);
  CHECK(p.splitk > 1 || p.slab_floats == 0);
  CHECK(p.splitk == 1 || p.kchunk % step == 0);
  CHECK(p.splitk == 1 || ((int64_t)(p.splitk - 1) * p.kchunk < K && K <= (int64_t)p.splitk * p.kchunk));
  CHECK(p.splitk == 1 || p.slab_floats == (int64_t)p.splitk * M * N);
  CHECK(p.cs_off < 0 ? p.cs_floats == 0 : (p.cs_off == p.slab_floats && p.cs_floats > 0));
  CHECK(p.bytes() <= ws);
  CHECK(p.bytes() <= bound);
  CHECK(same(at_bound, unlimited));
#undef CHECK
}

static void show(const char* name, const SplitPlan& p) {
  std::printf("%s: splitk %d kchunk %d cs_off %lld\n", name, p.splitk, p.kchunk, (long long)p.cs_off);
}

int main() {
  const int MN[] = {8, 128, 256, 264, 520, 768, 2304, 3072};
  const int Ks[] = {64, 128, 200, 256, 1000, 1024, 1026, 4100, 12416, 16384, 20520};
  const int CUs[] = {1, 8, 64, 256, 304};
  const int64_t WS[] = {0, 4096, 8ll << 20, 256ll << 20};
  long cases = 0;
  for (int M : MN) for (int N : MN) for (int K : Ks) for (int cu : CUs) {
    const int64_t bound = workspace_bound(M, N, K, cu);
    for (int64_t ws : WS) {
      for (int bias = 0; bias < 2; ++bias) {
        check("tn256", plan_tn256(M, N, K, cu, ws, bias), plan_tn256(M, N, K, cu, bound, bias),
              plan_tn256(M, N, K, cu, kUnlimited, bias), 128, M, N, K, cu, ws, bias);
        ++cases;
      }
      check("tn128", plan_tn128(M, N, K, ws), plan_tn128(M, N, K, bound), plan_tn128(M, N, K, kUnlimited),
            64, M, N, K, cu, ws, 0);
      check("f32", plan_f32(M, N, K, cu, ws), plan_f32(M, N, K, cu, bound),
            plan_f32(M, N, K, cu, kUnlimited), 32, M, N, K, cu, ws, 0);
      cases += 2;
    }
  }
  std::printf("plans checked: %ld, failures: %ld\n", cases, g_bad);
  const int64_t MiB = 1 << 20;
  show("tn256 768x768x16384 bias 256MiB", plan_tn256(768, 768, 16384, 256, 256 * MiB, true));
  show("tn256 3072x768x20520 bias 256MiB", plan_tn256(3072, 768, 20520, 256, 256 * MiB, true));
  show("tn256 768x768x1000 bias 256MiB", plan_tn256(768, 768, 1000, 256, 256 * MiB, true));
  show("tn256 768x768x16384 bias 0", plan_tn256(768, 768, 16384, 256, 0, true));
  show("tn256 768x768x16384 bias 8MiB", plan_tn256(768, 768, 16384, 256, 8 * MiB, true));
  show("tn128 768x768x4100 256MiB", plan_tn128(768, 768, 4100, 256 * MiB));
  show("f32 16x768x768 256MiB", plan_f32(16, 768, 768, 256, 256 * MiB));
  return g_bad ? 1 : 0;
}
