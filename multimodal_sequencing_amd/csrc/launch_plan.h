// Launch plans of the LayerNorm, embedding, column-sum and attention host sides: grids, LDS bytes,
// kernel choice and workspace carve-ups, each formula once, read by the size query and by the launch
// alike. Plain host C++ (no HIP, no state), so tests/launch_plan_check.cpp checks it without a GPU.
#pragma once
#include <cstdint>

namespace mmseq_plan {

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// --- two-level reduction of per-workgroup partial rows (reduce.hip) ---
constexpr int RCH = 64;  // partial rows per level-1 workgroup

// level-1 workgroups over nb partial rows of W floats, and their scratch ([rows][W])
inline int reduce_rows(int nb) { return (int)ceil_div(nb, RCH); }
inline int64_t reduce_extra(int nb, int W) { return (int64_t)reduce_rows(nb) * W; }
// nb partial rows of W floats with their reduction scratch behind them
inline int64_t partials_floats(int nb, int W) { return (int64_t)nb * W + reduce_extra(nb, W); }

// --- column sums (elementwise.hip): CS_ROWS rows per partial row ---
constexpr int CS_ROWS = 256;

struct ColsumPlan {
  int nb;           // partial rows [nb][cols] at the start of the workspace
  int64_t red_off;  // float offset of the reduction scratch behind them
  int64_t floats;   // all of it
};

inline ColsumPlan colsum_plan(int rows, int cols) {
  const int nb = (int)ceil_div(rows, CS_ROWS);
  return {nb, (int64_t)nb * cols, partials_floats(nb, cols)};
}

// --- LayerNorm backward (layernorm.hip) ---
constexpr int LN_RPB = 128;       // rows per workgroup, generic kernel
constexpr int LN_RPB16 = 64;      // ... bf16 fast kernel, before the cap on its blocks
constexpr int LN_MAX_NB16 = 512;  // two per CU at the fast kernel's ~190 VGPRs: one resident round

struct LnBwdPlan {
  bool fast;           // the bf16 16-byte-row kernel (ln_bwd16_kernel), else the generic one
  int rpb, nb;         // rows per workgroup, workgroups
  bool din, dxd, q8;   // fast kernel: input dropout, dropped copy of dx, MX-fp8 copy
  bool cs;             // fast kernel: the column sums ride in it as a third partial row
  int pw;              // partial rows per workgroup are pw * cols floats wide ([nb][pw][cols])
  int64_t red_off;     // float offset of the reduction scratch (behind the partials)
  int64_t floats;      // workspace floats the call touches, the separate column-sum pass included
};

// fast16: bf16, cols 256..1024 (x256) and 16-byte rows; drop_dy: input dropout on; dsum / q /
// dx_drop: that output is asked for. The fast kernel takes at most LN_MAX_NB16 blocks, each over
// rpb rows (a multiple of 8, one row per half wave and step): 2.5-10x fewer dgamma / dbeta partial
// rows to write and reduce than 64-row blocks. The column sums ride in it where it has the
// registers (no input dropout, bf16 out; at cols 1024 it would spill); elsewhere they are a pass of
// their own over the written gradient, after the reduction has freed the workspace.
inline LnBwdPlan ln_bwd_plan(int rows, int cols, bool fast16, bool dsum, bool q, bool drop_dy, bool dx_drop) {
  LnBwdPlan p = {};
  p.fast = fast16;
  p.rpb = fast16 ? LN_RPB16 : LN_RPB;
  p.nb = (int)ceil_div(rows, p.rpb);
  if (fast16 && p.nb > LN_MAX_NB16) {
    p.rpb = (int)ceil_div(ceil_div(rows, LN_MAX_NB16), 8) * 8;
    p.nb = (int)ceil_div(rows, p.rpb);
  }
  p.din = drop_dy; p.dxd = dx_drop; p.q8 = q;
  p.cs = fast16 && dsum && !q && !drop_dy && cols <= 768;
  p.pw = p.cs ? 3 : 2;
  p.red_off = (int64_t)p.nb * p.pw * cols;
  p.floats = partials_floats(p.nb, p.pw * cols);
  if (dsum && !p.cs) {
    const int64_t c = colsum_plan(rows, cols).floats;
    if (c > p.floats) p.floats = c;
  }
  return p;
}

// What mmseq_layernorm_bwd_workspace reports: the fast kernel's three partial rows per block at its
// uncapped block count, or the column-sum pass. No path of ln_bwd_plan uses more (the plan check
// sweeps that); the capped and the generic paths use less.
inline int64_t ln_bwd_workspace(int rows, int cols) {
  const int64_t w = partials_floats((int)ceil_div(rows, LN_RPB16), 3 * cols);
  const int64_t c = colsum_plan(rows, cols).floats;
  return w > c ? w : c;
}

// --- embedding backward workspaces (embed.hip): float offsets into the caller's workspace ---
constexpr int EMBED_RPB = 64;  // rows per workgroup of the embedding backward kernels

struct EmbedLnBwdLayout {
  int nb;           // workgroups = LN partial rows
  int64_t de;       // [P * Lt][H] gradient of the embedding sum
  int64_t ln;       // [nb][2][H] dgamma / dbeta partials
  int64_t red;      // their reduction scratch
  int64_t cs;       // column-sum scratch of dpos (empty at Lt = 1)
  int64_t scatter;  // table scatter's keys, sort scratch and pieces, 16-byte aligned
  int64_t total;
};

// scatter_bytes: table_scatter_det_bytes(P * Lt, H)
inline EmbedLnBwdLayout embed_ln_bwd_layout(int P, int Lt, int H, int64_t scatter_bytes) {
  const int64_t rows = (int64_t)P * Lt;
  EmbedLnBwdLayout l = {};
  l.nb = (int)ceil_div(rows, EMBED_RPB);
  l.de = 0;
  l.ln = l.de + rows * H;
  l.red = l.ln + (int64_t)l.nb * 2 * H;
  l.cs = l.red + reduce_extra(l.nb, 2 * H);
  const int64_t cs_end = l.cs + (Lt > 1 ? colsum_plan(P, (Lt - 1) * H).floats : 0);
  l.scatter = (cs_end + 3) & ~3ll;
  l.total = l.scatter + (scatter_bytes + 3) / 4;
  return l;
}

struct VitEmbedBwdLayout {
  int nb;
  int64_t dx0;  // [P][W] gradient of the class-token rows
  int64_t ln;   // [nb][2][W] dgamma / dbeta partials
  int64_t red;  // their reduction scratch
  int64_t sp;   // (bf16 path) [ntok - 1][W] sums over pairs of dpatch
  int64_t s0;   // (bf16 path) [W] sums over pairs of dx0
  int64_t cs;   // column-sum scratch, for the larger of the two sums
  int64_t total;
};

inline VitEmbedBwdLayout vit_embed_bwd_layout(int P, int ntok, int W) {
  VitEmbedBwdLayout l = {};
  l.nb = (int)ceil_div((int64_t)P * ntok, EMBED_RPB);
  l.dx0 = 0;
  l.ln = l.dx0 + (int64_t)P * W;
  l.red = l.ln + (int64_t)l.nb * 2 * W;
  l.sp = l.red + reduce_extra(l.nb, 2 * W);
  l.s0 = l.sp + (int64_t)(ntok - 1) * W;
  l.cs = l.s0 + W;
  const int64_t a = colsum_plan(P, (ntok - 1) * W).floats, b = colsum_plan(P, W).floats;
  l.total = l.cs + (a > b ? a : b);
  return l;
}

// --- attention, bf16 fast kernels (attention.hip): 128-row blocks, 64-key tiles ---
inline int attn_nkt(int T) { return (T + 63) / 64; }           // key tiles
inline int attn_nkt2(int T) { return (attn_nkt(T) + 1) & ~1; }  // ... rounded up to even: keep-bit
                                                                // words per row (16-byte rows)
inline int64_t keep_bits_words(int P, int T, int heads) { return (int64_t)P * heads * T * attn_nkt2(T); }
inline unsigned attn_blocks(int nx, int heads, int P) { return (unsigned)((int64_t)nx * heads * P); }

constexpr int64_t ATTN_KV_LDS = 4 * 4096 * 2;  // K / V double buffer

struct AttnFwdPlan {
  unsigned blocks, threads;
  int64_t lds_bytes;
  int nkt2;
  int dmode;  // dropout: 0 none, 1 counter hash, 2 counter hash + keep bits written
  bool wide;  // the dropout pair index needs 64 bits (of no effect at dmode 0)
};

// variant 2 (32 x 32 MFMA, 128 threads; Tq == T) or 1 (256 threads)
inline AttnFwdPlan attn_fwd_plan(int P, int T, int Tq, int heads, int variant, bool dropout, bool keep_bits) {
  AttnFwdPlan p = {};
  p.blocks = attn_blocks((Tq + 127) / 128, heads, P);
  p.threads = variant == 2 ? 128 : 256;
  p.lds_bytes = ATTN_KV_LDS + (int64_t)attn_nkt(T) * (64 + 1) * 4;  // + the key-bias rows
  p.nkt2 = attn_nkt2(T);
  p.dmode = dropout ? (keep_bits ? 2 : 1) : 0;
  // largest dropout pair index + the in-tile key offset must stay below 2^32 for the narrow path
  p.wide = ((uint64_t)P * heads * T * (uint64_t)((T + 3) & ~3)) / 4 + 64 >= (1ull << 32);
  return p;
}

struct TailFold {
  int tail0;  // first tail row, 0 = no fold
  int nxq;    // row blocks per (pair, head)
};

// Row blocks of the tail-folding kernels: T = 128 n + r with 1 <= r <= 16 (T = 513, 393, 769 on the
// path) runs n blocks, the last one also owning the r tail rows, instead of n + 1 blocks whose last
// has one active wave; a block's time is set by its key sweep, not by how many of its rows are valid
// (DESIGN §7), so the n + 1-th block cost a full block.
inline TailFold tail_fold(int T, bool allow) {
  const int n = T / 128, r = T % 128;
  const bool fold = allow && n >= 1 && r >= 1 && r <= 16;
  return {fold ? n * 128 : 0, fold ? n : (T + 127) / 128};
}

struct AttnBwdPlan {
  int dmode;  // dropout: 0 none, 1 counter hash, 2 keep bits from the forward
  int nkt2;
  unsigned dq_blocks;  // dQ never folds: its tail state took it from three to two waves per SIMD
  int64_t dq_lds;      // (148 -> 236 VGPRs), slower at T = 513 and 393 than the extra block it saves
  // dK/dV: the blocks without the tail keys in one launch (x = 0 .. nplain - 1 of every pair and
  // head), the tail block (x = nplain when folded) in a second one with the fold's state and LDS.
  // The counter-hash mode runs unfolded (its registers are spent on the hashed keep masks).
  int tail0, nxq, nplain, ntail;
  unsigned plain_blocks, tail_blocks;
  int64_t dkdv_lds, tail_lds;
};

inline AttnBwdPlan attn_bwd_plan(int P, int T, int Tq, int heads, bool dropout, bool keep_bits) {
  AttnBwdPlan p = {};
  p.dmode = dropout ? (keep_bits ? 2 : 1) : 0;
  p.nkt2 = attn_nkt2(T);
  p.dq_blocks = attn_blocks((Tq + 127) / 128, heads, P);
  p.dq_lds = ATTN_KV_LDS + (int64_t)attn_nkt(T) * 64 * 4;  // + the key-bias row
  const TailFold f = tail_fold(T, p.dmode != 1);
  p.tail0 = f.tail0; p.nxq = f.nxq;
  p.ntail = f.tail0 ? 1 : 0;
  p.nplain = f.nxq - p.ntail;
  p.plain_blocks = attn_blocks(p.nplain, heads, P);
  p.tail_blocks = attn_blocks(p.ntail, heads, P);
  p.dkdv_lds = ATTN_KV_LDS + (int64_t)attn_nkt(T) * 64 * 4 * 2 + 2048;
  p.tail_lds = p.dkdv_lds + 6144;  // + the tail keys' keep words (2 KB) and K / V fragments (4 KB)
  return p;
}

}  // namespace mmseq_plan
