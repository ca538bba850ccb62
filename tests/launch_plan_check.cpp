// Stand-alone check of csrc/launch_plan.h (built and run by tests/test_launch_plan.py, no GPU):
// sweeps the LayerNorm-backward plans, the two embedding-backward workspace layouts and the
// attention forward / backward plans, and exits nonzero unless every one is well formed: what a
// path uses fits the size query, the regions of a layout follow one another, the grids cover their
// rows, the keep-bit words are what the kernels index. Then prints the plans of a few named cases
// for the test to compare.
#include <cstdio>
#include "launch_plan.h"

using namespace mmseq_plan;

static long g_bad = 0, g_cases = 0;

#define CHECK(cond, ...)                                    \
  do {                                                      \
    if (!(cond) && ++g_bad <= 20) {                         \
      std::printf("FAIL %s: ", #cond);                      \
      std::printf(__VA_ARGS__);                             \
      std::printf("\n");                                    \
    }                                                       \
  } while (0)

// ---- LayerNorm backward ----
static void check_ln(int rows, int cols) {
  const int64_t query = ln_bwd_workspace(rows, cols);
  CHECK(colsum_plan(rows, cols).floats <= query, "rows=%d cols=%d", rows, cols);
  for (int f = 0; f < 32; ++f) {
    const bool fast16 = f & 1, dsum = f & 2, q = f & 4, di = f & 8, dd = f & 16;
    if (fast16 && (cols % 256 != 0 || cols > 1024)) continue;  // no such call
    if (q && !fast16) continue;                                 // rejected by the entry
    const LnBwdPlan p = ln_bwd_plan(rows, cols, fast16, dsum, q, di, dd);
    ++g_cases;
#define LN_CHECK(cond) CHECK(cond, "rows=%d cols=%d flags=%d", rows, cols, f)
    LN_CHECK(p.fast == fast16 && p.din == di && p.dxd == dd && p.q8 == q);
    LN_CHECK(p.floats <= query);
    LN_CHECK(p.rpb > 0 && p.rpb % 8 == 0);
    LN_CHECK((int64_t)p.nb * p.rpb >= rows);
    LN_CHECK((int64_t)(p.nb - 1) * p.rpb < rows);
    LN_CHECK(p.fast ? p.nb <= LN_MAX_NB16 : p.rpb == LN_RPB);
    LN_CHECK(!p.fast || p.rpb >= LN_RPB16);
    LN_CHECK(!p.fast || p.rpb == LN_RPB16 || p.nb > LN_MAX_NB16 / 2);  // the cap leaves the grid full
    // the kernels that exist: CS without input dropout and Q8, up to 768 columns, fast path only
    LN_CHECK(!p.cs || (p.fast && dsum && !p.din && !p.q8 && cols <= 768));
    LN_CHECK(p.pw == (p.cs ? 3 : 2));
    LN_CHECK(p.red_off == (int64_t)p.nb * p.pw * cols);
    LN_CHECK(p.floats >= p.red_off + reduce_extra(p.nb, p.pw * cols));
    LN_CHECK(!(dsum && !p.cs) || p.floats >= colsum_plan(rows, cols).floats);
#undef LN_CHECK
  }
}

// ---- embedding layouts: regions in order, each starting where the previous one ends ----
static void check_embed(int P, int Lt, int H, int ntok) {
  {
    const int64_t scatter_bytes = 16 * (int64_t)P * Lt + 4099;  // any number: not a multiple of 4
    const EmbedLnBwdLayout l = embed_ln_bwd_layout(P, Lt, H, scatter_bytes);
    const int64_t rows = (int64_t)P * Lt;
    ++g_cases;
#define E_CHECK(cond) CHECK(cond, "embed_ln P=%d Lt=%d H=%d", P, Lt, H)
    E_CHECK((int64_t)l.nb * EMBED_RPB >= rows && (int64_t)(l.nb - 1) * EMBED_RPB < rows);
    E_CHECK(l.de == 0);
    E_CHECK(l.ln == l.de + rows * H);
    E_CHECK(l.red == l.ln + (int64_t)l.nb * 2 * H);
    E_CHECK(l.cs == l.red + reduce_extra(l.nb, 2 * H));
    const int64_t cs_end = l.cs + (Lt > 1 ? colsum_plan(P, (Lt - 1) * H).floats : 0);
    E_CHECK(Lt > 1 ? cs_end > l.cs : cs_end == l.cs);
    E_CHECK(l.scatter >= cs_end && l.scatter - cs_end < 4 && l.scatter % 4 == 0);  // the 16-byte round-up
    E_CHECK(l.total == l.scatter + (scatter_bytes + 3) / 4);
    E_CHECK(l.total * 4 >= l.scatter * 4 + scatter_bytes);
#undef E_CHECK
  }
  {
    const int W = H;
    const VitEmbedBwdLayout l = vit_embed_bwd_layout(P, ntok, W);
    const int64_t rows = (int64_t)P * ntok;
    ++g_cases;
#define V_CHECK(cond) CHECK(cond, "vit_embed P=%d ntok=%d W=%d", P, ntok, W)
    V_CHECK((int64_t)l.nb * EMBED_RPB >= rows && (int64_t)(l.nb - 1) * EMBED_RPB < rows);
    V_CHECK(l.dx0 == 0);
    V_CHECK(l.ln == l.dx0 + (int64_t)P * W);
    V_CHECK(l.red == l.ln + (int64_t)l.nb * 2 * W);
    V_CHECK(l.sp == l.red + reduce_extra(l.nb, 2 * W));
    V_CHECK(l.s0 == l.sp + (int64_t)(ntok - 1) * W);
    V_CHECK(l.cs == l.s0 + W);
    V_CHECK(l.total >= l.cs + colsum_plan(P, (ntok - 1) * W).floats);
    V_CHECK(l.total >= l.cs + colsum_plan(P, W).floats);
    V_CHECK(l.total == l.cs + colsum_plan(P, (ntok - 1) * W).floats || l.total == l.cs + colsum_plan(P, W).floats);
#undef V_CHECK
  }
}

// ---- attention ----
static void check_attn(int P, int T, int Tq, int heads) {
  const int nkt = (T + 63) / 64;
  const int64_t bh = (int64_t)P * heads;
  for (int variant = 1; variant <= 2; ++variant)
    for (int dmode = 0; dmode < 3; ++dmode) {
      if (variant == 2 && Tq != T) continue;  // rejected by the entry
      const AttnFwdPlan p = attn_fwd_plan(P, T, Tq, heads, variant, dmode != 0, dmode == 2);
      ++g_cases;
#define A_CHECK(cond) CHECK(cond, "attn fwd P=%d T=%d Tq=%d v=%d dmode=%d", P, T, Tq, variant, dmode)
      A_CHECK(p.dmode == dmode);
      A_CHECK(p.threads == (variant == 2 ? 128u : 256u));
      A_CHECK(p.blocks % bh == 0 && (int64_t)(p.blocks / bh) * 128 >= Tq && (int64_t)(p.blocks / bh - 1) * 128 < Tq);
      A_CHECK(p.nkt2 % 2 == 0 && nkt <= p.nkt2 && p.nkt2 <= nkt + 1);
      A_CHECK(p.lds_bytes >= 2 * 2 * 64 * 64 * 2 + (int64_t)nkt * 64 * 4 && p.lds_bytes <= 160 * 1024);
      A_CHECK(keep_bits_words(P, T, heads) == bh * T * p.nkt2);
      A_CHECK(!p.wide);  // nothing in this sweep comes near 2^32 pairs
#undef A_CHECK
    }
  for (int dmode = 0; dmode < 3; ++dmode) {
    const AttnBwdPlan p = attn_bwd_plan(P, T, Tq, heads, dmode != 0, dmode == 2);
    const bool fold = T >= 128 && 1 <= T % 128 && T % 128 <= 16 && dmode != 1;
    ++g_cases;
#define A_CHECK(cond) CHECK(cond, "attn bwd P=%d T=%d Tq=%d dmode=%d", P, T, Tq, dmode)
    A_CHECK(p.dmode == dmode);
    A_CHECK(p.nkt2 % 2 == 0 && nkt <= p.nkt2 && p.nkt2 <= nkt + 1);
    A_CHECK(p.dq_blocks % bh == 0 && (int64_t)(p.dq_blocks / bh) * 128 >= Tq && (int64_t)(p.dq_blocks / bh - 1) * 128 < Tq);
    A_CHECK((p.tail0 != 0) == fold && p.ntail == (fold ? 1 : 0));
    A_CHECK(!fold || (p.tail0 == T / 128 * 128 && p.tail0 < T && T - p.tail0 <= 16));
    A_CHECK(p.nplain >= 0 && p.nplain + p.ntail == p.nxq);
    A_CHECK((p.nplain + p.ntail) * 128 + (fold ? 16 : 0) >= T);
    A_CHECK((p.nxq - 1) * 128 < T);
    A_CHECK(p.plain_blocks == (uint64_t)p.nplain * bh && p.tail_blocks == (uint64_t)p.ntail * bh);
    A_CHECK(p.tail_lds == p.dkdv_lds + 6144 && p.tail_lds <= 160 * 1024);
    A_CHECK(p.dq_lds < p.dkdv_lds);
#undef A_CHECK
  }
}

// `wide` is the parent's expression: pairs / 4 + 64 >= 2^32, with pairs = P * heads * T * ((T + 3) & ~3).
// Walk P to the boundary for a given T and check both sides of it.
static void check_wide(int T, int heads) {
  const unsigned __int128 per_pair = (unsigned __int128)heads * T * ((T + 3) & ~3);
  // smallest P with P * per_pair / 4 + 64 >= 2^32, i.e. P * per_pair >= 4 * (2^32 - 64)
  const unsigned __int128 need = (unsigned __int128)4 * ((1ull << 32) - 64);
  const int64_t p0 = (int64_t)((need + per_pair - 1) / per_pair);
  if (p0 < 2 || p0 > 2000000000) return;
  for (int variant = 1; variant <= 2; ++variant)
    for (int dmode = 0; dmode < 3; ++dmode) {
      const bool below = attn_fwd_plan((int)p0 - 1, T, T, heads, variant, dmode != 0, dmode == 2).wide;
      const bool at = attn_fwd_plan((int)p0, T, T, heads, variant, dmode != 0, dmode == 2).wide;
      const bool above = attn_fwd_plan((int)p0 + 1, T, T, heads, variant, dmode != 0, dmode == 2).wide;
      g_cases += 3;
      CHECK(!below && at && above, "wide T=%d heads=%d P0=%lld: %d %d %d", T, heads, (long long)p0, below, at, above);
    }
}

static void show_ln(int rows, int cols, bool fast16, bool dsum, bool di) {
  const LnBwdPlan p = ln_bwd_plan(rows, cols, fast16, dsum, false, di, false);
  std::printf("ln %dx%d %s%s%s: rpb %d nb %d cs %d pw %d red_off %lld floats %lld query %lld\n", rows, cols,
              fast16 ? "fast" : "generic", dsum ? " dsum" : "", di ? " din" : "", p.rpb, p.nb, (int)p.cs, p.pw,
              (long long)p.red_off, (long long)p.floats, (long long)ln_bwd_workspace(rows, cols));
}

static void show_attn(int T, int Tq) {
  const int P = 2, heads = 12;
  for (int variant = 1; variant <= (Tq == T ? 2 : 1); ++variant) {
    const AttnFwdPlan f = attn_fwd_plan(P, T, Tq, heads, variant, true, true);
    std::printf("attn T=%d Tq=%d fwd v%d: blocks %u threads %u lds %lld nkt2 %d wide %d\n", T, Tq, variant,
                f.blocks, f.threads, (long long)f.lds_bytes, f.nkt2, (int)f.wide);
  }
  for (int dmode = 1; dmode <= 2; ++dmode) {
    const AttnBwdPlan b = attn_bwd_plan(P, T, Tq, heads, true, dmode == 2);
    std::printf("attn T=%d Tq=%d bwd d%d: dq %u lds %lld | plain %u lds %lld | tail %u lds %lld | tail0 %d nxq %d\n",
                T, Tq, dmode, b.dq_blocks, (long long)b.dq_lds, b.plain_blocks, (long long)b.dkdv_lds,
                b.tail_blocks, (long long)b.tail_lds, b.tail0, b.nxq);
  }
  std::printf("attn T=%d keep words %lld\n", T, (long long)keep_bits_words(P, T, heads));
}

static void show_embed(int P, int Lt, int H) {
  const EmbedLnBwdLayout l = embed_ln_bwd_layout(P, Lt, H, 1001);
  std::printf("embed_ln %dx%dx%d scatter 1001 B: nb %d ln %lld red %lld cs %lld scatter %lld total %lld\n", P, Lt, H,
              l.nb, (long long)l.ln, (long long)l.red, (long long)l.cs, (long long)l.scatter, (long long)l.total);
}

static void show_vit(int P, int ntok, int W) {
  const VitEmbedBwdLayout l = vit_embed_bwd_layout(P, ntok, W);
  std::printf("vit_embed %dx%dx%d: nb %d ln %lld red %lld sp %lld s0 %lld cs %lld total %lld\n", P, ntok, W, l.nb,
              (long long)l.ln, (long long)l.red, (long long)l.sp, (long long)l.s0, (long long)l.cs, (long long)l.total);
}

int main() {
  const int ROWS[] = {1, 63, 64, 65, 127, 128, 129, 32767, 32768, 32769, 55368, 164160};
  const int COLS[] = {4, 252, 256, 768, 1024, 1028, 2048};
  for (int rows : ROWS) for (int cols : COLS) check_ln(rows, cols);
  const int Ps[] = {1, 2, 48}, Lts[] = {1, 2, 24, 120}, Hs[] = {4, 256, 320, 768, 1024}, NTOK[] = {3, 9, 99};
  for (int P : Ps) for (int Lt : Lts) for (int H : Hs) for (int ntok : NTOK) check_embed(P, Lt, H, ntok);
  for (int T = 1; T <= 1100; ++T) {
    const int Tqs[] = {1, T / 3 > 0 ? T / 3 : 1, T};
    for (int Tq : Tqs) check_attn(2, T, Tq, 12);
  }
  const int WT[] = {1, 64, 120, 393, 513, 1100};
  for (int T : WT) { check_wide(T, 12); check_wide(T, 1); }
  std::printf("plans checked: %ld, failures: %ld\n", g_cases, g_bad);
  show_ln(55368, 768, true, true, false);
  show_ln(55368, 768, true, true, true);
  show_ln(55368, 768, false, true, false);
  show_ln(432, 256, true, true, false);
  show_ln(432, 256, false, true, false);
  const int PT[] = {513, 393, 120, 144, 145};
  for (int T : PT) show_attn(T, T);
  show_attn(513, 171);
  show_embed(1, 1, 4);
  show_embed(3, 7, 100);
  show_embed(2, 65, 768);
  show_embed(257, 2, 4);
  show_vit(3, 9, 512);
  show_vit(257, 3, 320);
  return g_bad ? 1 : 0;
}
