// Persistent 256 x 256 bf16 NT GEMM (forward Y = X W^T and dgrad dX = dY W over the 164k-row
// activations of the joint encoder and the ViT); see gemm_common.h for the shared epilogue.
#include "gemm_common.h"

using namespace mmseq_gemm_detail;

namespace {

// Compile-time-specialised epilogue for the 256 x 256 kernel: one lane owns 8 contiguous outputs
// of a row (two 16x16 tiles whose B rows are interleaved, see the kernel), so every access is
// 16 bytes. bf16 out; the host guarantees N % 8 == 0, ldc % 8 == 0, ldr % 8 == 0 and 16-byte
// aligned C / aux / dact / resid. Specialised per activation so the 16 unrolled copies stay small.
typedef unsigned short us;
__device__ __forceinline__ void ld8(const us* p, float* v) {
  const u16x8 u = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = bf2f(u[r]);
}
__device__ __forceinline__ void st8(us* p, const float* v) {
  u16x8 u;
#pragma unroll
  for (int r = 0; r < 8; ++r) u[r] = f2bf(v[r]);
  *reinterpret_cast<u16x8*>(p) = u;
}

// The epilogue runs in two phases so that no load waits behind a store to a possibly aliasing
// address (which serialises one full memory round trip per call): epi8_load issues the 16-byte
// operand reads (dact for BWD, else the residual; plus C when accumulating) of all 16 calls of a
// wave first, epi8 then computes and stores.
// one 16-byte operand per call: dact (BWD), else the residual, else C (accumulate); the host
// never sends the 256 kernels a residual together with accumulate
struct EpiIn { u16x8 x; };
template <bool BWD, bool Q8 = false, bool CHK = true>
__device__ __forceinline__ EpiIn epi8_load(const GemmArgs& a, int m, int n) {
  EpiIn in;
  in.x = (u16x8){0, 0, 0, 0, 0, 0, 0, 0};
  if (CHK && (m >= a.M || n >= a.N)) return in;
  // MX-fp8 output (Q8): ldc is the fp8 output's row stride, dact has the bf16 copy's (ldcb)
  const int64_t off = (int64_t)m * (Q8 ? a.ldcb : a.ldc) + n;
  if (BWD) in.x = *reinterpret_cast<const u16x8*>(reinterpret_cast<const us*>(a.dact) + off);
  else if (a.resid) in.x = *reinterpret_cast<const u16x8*>(reinterpret_cast<const us*>(a.resid) + (int64_t)m * a.ldr + n);
  else if (a.accumulate) in.x = *reinterpret_cast<const u16x8*>(reinterpret_cast<const us*>(a.C) + off);
  return in;
}

// Bias of a lane's 8 output columns n .. n + 7, loaded once per tile before any of its stores
// (vmcnt retires loads and stores in issue order: a bias load inside each call would wait for
// every store issued before it).
struct EpiBias { f32x4 b0, b1; };
__device__ __forceinline__ EpiBias epi_bias(const GemmArgs& a, int n) {
  EpiBias b;
  b.b0 = b.b1 = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (!a.bias || n >= a.N) return b;
  if ((((uintptr_t)a.bias) & 15) == 0) {  // wave-uniform: two 16-byte loads
    b.b0 = *reinterpret_cast<const f32x4*>(a.bias + n);
    b.b1 = *reinterpret_cast<const f32x4*>(a.bias + n + 4);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) { b.b0[r] = a.bias[n + r]; b.b1[r] = a.bias[n + 4 + r]; }
  }
  // consume here: otherwise the waitcnt state, merged over the per-call bounds branches, keeps
  // the loads "pending" and puts a vmcnt(0) (= every earlier store) in front of each call
  asm volatile("" ::"v"(b.b0), "v"(b.b1));
  return b;
}

// Activation-derivative table for the dgrad epilogues (dY * act'(z), z = the stored bf16
// pre-activation): act'(z) for every bf16 z with 2^-10 <= |z| < 8 (13 binades x 128 mantissas x
// 2 signs = 3328 fp32 entries, 13 KB of LDS), exact (libm erf / exp at kernel start). |z| outside
// clamps to the range ends, where act' is within 8e-4 of its limit (0.5 near 0; 0 or 1 beyond 8).
// One LDS gather per element instead of ~17 VALU slots of a fitted GELU' (two transcendentals).
// The table holds the EXACT derivative on purpose: the reference's backward is the exact GELU' (its
// forward the exact erf GELU), so the dgrad evaluates the reference's derivative at our stored
// pre-activation; the forward epilogue's fitted logistic (gelu_sig, 2.5e-5 abs) differs from it by
// <= 1.1e-4, far below the bf16 quantum. gelu_sig_grad (the fit's own derivative) is only used by
// the non-default two-block variant (gemm_nt_2b_kernel).
constexpr int DT_LO = 117 << 7;  // bf16 bits of 2^-10
constexpr int DT_N = 13 * 128;   // entries per sign
__device__ __forceinline__ int dtab_index(unsigned short u) {
  const int a = min(max((int)(u & 0x7FFFu) - DT_LO, 0), DT_N - 1);
  return a + (int)(u >> 15) * DT_N;
}
template <int ACT>
__device__ __forceinline__ void dtab_fill(float MMSEQ_LDS* tab) {
  for (int e = threadIdx.x; e < 2 * DT_N; e += blockDim.x) {
    const unsigned short u = (unsigned short)(((e / DT_N) << 15) | (e % DT_N + DT_LO));
    tab[e] = act_bwd(ACT, bf2f(u));
  }
}

// CHK = false: the whole 256 x 256 tile is inside C (no per-call bounds branches)
template <int ACT, bool BWD, bool XIN, bool DTAB = false, bool CHK = true>
__device__ __forceinline__ void epi8(const GemmArgs& a, int m, int n, f32x4 lo, f32x4 hi, const EpiIn& in,
                                     const EpiBias& bias, const float MMSEQ_LDS* dtab = nullptr) {
  if (CHK && (m >= a.M || n >= a.N)) return;
  float v[8];
  if (XIN) {  // scalar: the operand-reading variants sit at 256 VGPRs (packed pairs spill there)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] = fmaf(lo[r], a.alpha, bias.b0[r]);
      v[4 + r] = fmaf(hi[r], a.alpha, bias.b1[r]);
    }
  } else {
    bias_alpha8(v, lo, hi, a.alpha, bias.b0, bias.b1);
  }
  const int64_t off = (int64_t)m * a.ldc + n;
  if (BWD) {
    if (DTAB) {
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] *= dtab[dtab_index(in.x[r])];
    } else if (ACT == MMSEQ_ACT_GELU_ERF) {
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] *= gelu_sig_grad(bf2f(in.x[r]));
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] *= act_bwd_fast(ACT, bf2f(in.x[r]));
    }
  } else if (ACT) {
    if (a.aux) st8(reinterpret_cast<us*>(a.aux) + off, v);
    if (ACT == MMSEQ_ACT_GELU_ERF) {
      gelu_sig8(v);
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = act_fwd_fast(ACT, v[r]);
    }
  }
  if (!BWD && a.drop.thr) {  // m * N + n % 8 == 0 (N % 8 == 0, n % 8 == 0): one hash per quad;
    // the dgrad variants take no dropout (the host sends those to the generic kernels), which
    // keeps them off scratch (4 spilled VGPRs with the hash compiled in)
    float dm[8];
    drop_mul_pairs<4>(a.drop, (uint64_t)m * a.N + n, dm);
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] *= dm[r];
  }
  if (XIN && !BWD) {  // residual or C (accumulate); BWD + accumulate is rejected on the host
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] += bf2f(in.x[r]);
  }
  st8(reinterpret_cast<us*>(a.C) + off, v);
}

// MX-fp8 output of one (row block, 32-column half) call: the lane's 8 outputs (bias + activation
// exactly as epi8, then rounded to bf16 as a bf16 output would be) join the 3 other lanes with the
// same row (g = 0..3: 32 columns = one E8M0 block) for the block's amax, then quantise like
// mmseq_quant_mxfp8 (bit-identical to it on the bf16 output): 8 e4m3 bytes per lane, the scale
// byte into the wave's LDS slot (stored per tile by q8_scale_words); rows in [M, M rounded up to
// 64) get scale 0, as the quantiser writes.
// BWD (the fp8 dgrad of config 5): the output is (A B^T) * act'(dact) from the dgrad table instead,
// e.g. dz = dY W2 * GELU'(z), whose MX-fp8 copy is the next dgrad GEMM's operand.
// The E8M0 scale bytes: each call writes its rows' bytes into the wave's 256-byte LDS slot
// (`sq`: byte ((64-row group * 2 + column block) * 16 + row % 16) * 4 + 16-row group % 4, every
// lane group the same value), and q8_scale_words stores the slot once per tile, one 32-bit word
// per lane = the four 16-row groups' bytes of one row and column block, which is one word of the
// scale layout: one store per wave and tile instead of one byte store per call.
__device__ __forceinline__ void q8_scale_words(const GemmArgs& a, int mrow, int ncol,
                                               const uint8_t MMSEQ_LDS* sq, int lane) {
  // mrow: row (64-row group's first 16-row group) and ncol: the column block's first column, of
  // this lane's word (lane group g: 64-row group g >> 1, column block g & 1)
  const uint32_t w = *(const uint32_t MMSEQ_LDS*)(sq + 4 * lane);
  const int Mp = (a.M + 63) & ~63;
  if (mrow < Mp && ncol < a.N) {
    const int KB = a.N >> 5;
    const rsrc_t rq = make_rsrc(a.q8_scales, (int64_t)(Mp >> 6) * KB * 64);
    const uint32_t off = (uint32_t)(((mrow >> 6) * KB + (ncol >> 5)) * 64 + (mrow & 15) * 4);
    __builtin_amdgcn_raw_buffer_store_b32(w, rq, off, 0, 0);
  }
}
template <int ACT, bool BWD = false>
__device__ __forceinline__ void epi8_q8(const GemmArgs& a, int m, int n, int g, f32x4 lo, f32x4 hi,
                                        const EpiBias& bias, uint8_t MMSEQ_LDS* sqb,
                                        const EpiIn* din = nullptr,
                                        const float MMSEQ_LDS* dtab = nullptr) {
  float v[8];
  bias_alpha8(v, lo, hi, a.alpha, bias.b0, bias.b1);
  const bool in = m < a.M && n < a.N;
  const int64_t offb = (int64_t)m * a.ldcb + n;
  if (BWD) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] *= dtab[dtab_index(din->x[r])];
  } else {
    if (ACT && a.aux && in) st8(reinterpret_cast<us*>(a.aux) + offb, v);  // training: pre-activation
    if (ACT == MMSEQ_ACT_GELU_ERF) {
      gelu_sig8(v);
    } else if (ACT) {
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = act_fwd_fast(ACT, v[r]);
    }
  }
  float amax = 0.f;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    v[r] = bf2f(f2bf(v[r]));
    amax = fmaxf(amax, fabsf(v[r]));
  }
  if (a.cbf && in) st8(reinterpret_cast<us*>(a.cbf) + offb, v);  // training: the bf16 output too
  // max over lanes l ^ 16 and l ^ 32 with the gfx950 row swaps (no LDS round trip as with
  // ds_bpermute); amax >= 0, so its bit pattern orders like the value
  {
    uint32_t u = __float_as_uint(amax);
    const auto r16 = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    u = max(r16[0], r16[1]);
    const auto r32 = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    amax = __uint_as_float(max(r32[0], r32[1]));
  }
  int e = amax > 0.f ? (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 : -127;
  e = max(-127, min(127, e - 8));
  const float inv = ldexpf(1.f, -e);
  *sqb = (uint8_t)(m < a.M ? e + 127 : 0);  // rows in [M, M rounded up to 64) get scale 0
  if (!in) return;
  uint32_t w[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const float s0 = fminf(448.f, fmaxf(-448.f, v[4 * j] * inv));
    const float s1 = fminf(448.f, fmaxf(-448.f, v[4 * j + 1] * inv));
    const float s2 = fminf(448.f, fmaxf(-448.f, v[4 * j + 2] * inv));
    const float s3 = fminf(448.f, fmaxf(-448.f, v[4 * j + 3] * inv));
    int pk = __builtin_amdgcn_cvt_pk_fp8_f32(s0, s1, 0, false);
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(s2, s3, pk, true);
    w[j] = (uint32_t)pk;
  }
  typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
  *reinterpret_cast<u32x2*>(reinterpret_cast<uint8_t*>(a.C) + (int64_t)m * a.ldc + n) =
      (u32x2){w[0], w[1]};
}

// ---------------------------------------------------------------------------------------------
// Large NT kernel (forward / dgrad over the 164k-row activations): persistent 256 x 256 tiles,
// 8 waves (2 along M x 4 along N, 128 x 64 outputs each = 8 x 4 MFMA 16x16 tiles), BK = 64,
// one 512-thread workgroup per CU, the guide's 8-phase schedule (cdna_hip_programming.md §5):
//  * LDS: two K-tile buffers of 64 KB (A image [256][64] + B image [256][64], 128-B rows),
//    filled by LDS-DMA with the swizzle on the source (guide rule 21). A: chunk' = chunk ^
//    ((row >> 1) & 7). B fragments are row-permuted: MFMA row rho of the wave's j-th 16-column
//    tile reads B row 8 (rho >> 2) + 4 (j & 1) + (rho & 3) + 32 (j >> 1), so after the swapped
//    MFMA a lane holds 8 CONTIGUOUS outputs of one row across tiles (2t, 2t + 1) -> 16-byte
//    epilogue accesses; B swizzle chunk' = chunk ^ (((row >> 1) & 1) | (((row >> 3) & 3) << 1))
//    keeps those permuted 16-row reads conflict-free for the ds_read_b128 lane groups.
//  * A K-tile is four 16 KB "half-tiles" named by which fragment registers read them:
//    A_lo (rows 0-63 of each 128-row A half), A_hi, B_lo (rows {0-31, 64-95} of each B half), B_hi.
//  * Two K-tiles per iteration, four phases each; per phase: ds_read this phase's fragments,
//    stage one half-tile (2 LDS-DMA per lane), s_barrier, lgkmcnt(0), 16 MFMAs, s_barrier.
//    Reads: phase 1 A_lo + B_lo, 2 B_hi, 3 A_hi, 4 none (MFMA quadrants q0..q3 snake through
//    the registers). Waves 4-7 run one barrier behind waves 0-3 (stagger: one group's MFMAs
//    beside the other group's reads), so a region is restaged >= 2 phases after its last read;
//    the counted vmcnt(4) before the first barrier of phases 4 and 8 retires the K-tile read
//    next while two half-tiles stay in flight.
//  * Staging runs across tile boundaries: the last iteration of a tile stages the NEXT tile's
//    first K-tiles, so its loads fly during the epilogue (dummy zero-size loads past the end keep
//    the vmcnt arithmetic uniform). Preconditions (host): bf16, K % 128 == 0, batch 1, no split.
// ---------------------------------------------------------------------------------------------
constexpr int G_LDA_HALF = 16384;  // elements per 256 x 64 operand image

// Tile order: work item -> (M tile, N tile). For wide outputs (>= 8 N tiles) in groups of
// NT_GROUP_M M-tiles, N-major inside a group, so the 32 consecutive items one XCD runs together
// cover NT_GROUP_M A panels x 4 B panels instead of ~3 A panels x every B panel of the weight:
// L2->fabric reads (FETCH_SIZE) -23 % at N = 3072, same time; N = 2304 +1 % time. Narrow outputs
// (N = 768: 3 tiles per M row) keep the row-major order, which is faster there (870 vs 826 TF/s).
// The activation + pre-activation (aux) epilogue, which writes two outputs per tile, takes groups
// of NT_GROUP_M_AUX at >= 12 N tiles: at N = 3072 (the FC1 forward of a training step) 818-820
// TF/s with 16 against 783-787 with 8, at N = 2304 16 was slower (772 vs 792), the other
// epilogues equal either way (profiles/r6_v19_nt_group_m_ab.txt, r6_v20_nt_group_m_aux_ab.txt).
constexpr int NT_GROUP_M = 8, NT_GROUP_M_AUX = 16;
__device__ __forceinline__ void tile_mn(int tile, int tiles_n, int ntiles, int& tm, int& tn,
                                        bool aux2 = false) {
  const int GM = tiles_n >= 8 ? (aux2 && tiles_n >= 12 ? NT_GROUP_M_AUX : NT_GROUP_M) : 1;
  if (GM <= 1) {
    tm = tile / tiles_n;
    tn = tile - tm * tiles_n;
    return;
  }
  const int tiles_m = ntiles / tiles_n;
  const int per = GM * tiles_n;
  const int grp = tile / per, first = grp * GM;
  const int gm = min(tiles_m - first, GM);
  const int r = tile - grp * per;
  tm = first + r % gm;
  tn = r / gm;
}

// 8-row group (0..31 of the 256-row image) written by wave-instruction q (0..15) of half-tile X
__device__ __forceinline__ int g8_of(int X, int q) {
  // X: 0 = A_lo, 1 = B_lo, 2 = B_hi, 3 = A_hi
  if (X == 0) return (q & 7) + ((q >> 3) << 4);
  if (X == 3) return 8 + (q & 7) + ((q >> 3) << 4);
  if (X == 1) return (q & 3) + ((q >> 2) << 3);
  return 4 + (q & 3) + ((q >> 2) << 3);
}

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;
// the fp8 MFMA operand of a lane = its two 16-byte chunks ks = 0, 1 of the 128-byte row (K positions
// 16g .. 16g + 15 and 64 + 16g .. 64 + 16g + 15, the layout fp8.hip probed): exactly the two bf16
// fragments the same lane reads for the two 32-deep k-steps of a bf16 K-tile
__device__ __forceinline__ i32x8 cat8(const bf16x8_t& lo, const bf16x8_t& hi) {
  const i32x4 l = __builtin_bit_cast(i32x4, lo), h = __builtin_bit_cast(i32x4, hi);
  return (i32x8){l[0], l[1], l[2], l[3], h[0], h[1], h[2], h[3]};
}

// the block-scaled fp8 MFMA with its accumulator tied (dst = srcC) by an inline-asm constraint: the
// builtin form lets the register allocator move every accumulator to a fresh tuple, which in the
// 256-register 8-wave kernel spills 140-165 VGPRs
__device__ __forceinline__ void mfma_f8_acc(f32x4& c, const i32x8& a, const i32x8& b, uint32_t sa,
                                            uint32_t sb) {
  asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"
               : "+v"(c) : "v"(a), "v"(b), "v"(sa), "v"(sb));
}

// Q8: MX-fp8 output (epi8_q8). F8: MX-fp8 operands (BASELINE config 5's fp8 MFMA path): the same
// schedule with 128-byte K-tiles of 128 e4m3 (one v_mfma_scale_f32_16x16x128_f8f6f4 per 16 x 16
// output tile and phase, twice the FLOPs of the bf16 phase in the same cycles), plus the K-tile's
// E8M0 scales (256 B per 64-row group, one 16-lane LDS-DMA per wave, staged with half-tile A_hi)
template <int ACT, bool BWD, bool XIN, bool Q8 = false, bool F8 = false>
__global__ __launch_bounds__(512, 1) void gemm256_nt_kernel(GemmArgs a, int tiles_n, int ntiles,
                                                            int delay) {
  // 128 KB of K-tile buffers, then (dgrad variants) the 13 KB activation-derivative table or (F8)
  // the 2 x 2 KB scale buffers
  __shared__ __attribute__((aligned(16))) unsigned short
      smem[2 * 2 * G_LDA_HALF + (BWD ? 4 * DT_N : 0) + (F8 ? 2048 : 0) + 1024 + (Q8 ? 1024 : 0)];
  // F8: [2 buffers][A 1 KB | B 1 KB], after the dgrad variants' activation-derivative table
  unsigned short* const sscale = smem + 2 * 2 * G_LDA_HALF + (BWD ? 4 * DT_N : 0);
  // the tile's 256 bias values, [2 tiles][1 KB]: DMA'd by wave 0 before the tile's K-loop (older
  // than the first iteration's stages, so retired by its phase-4 counted wait and visible after
  // that phase's barrier), read by the epilogue from LDS. A global bias load in the epilogue was
  // its first wait, a vmcnt(0) (the compiler cannot see the in-flight LDS-DMA of the next tile's
  // first K-tiles, and that wait drained them).
  unsigned short* const sbias = smem + 2 * 2 * G_LDA_HALF + (BWD ? 4 * DT_N : 0) + (F8 ? 2048 : 0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // Q8: the wave's 256-byte slot for the tile's E8M0 scale bytes (q8_scale_words)
  uint8_t MMSEQ_LDS* const sq8 = (uint8_t MMSEQ_LDS*)(sbias + 1024) + wave * 256;
  const int wr = wave >> 2, wc = wave & 3;
  const int G = gridDim.x;
  const bool aux2 = ACT > 0 && !BWD && a.aux != nullptr;  // two outputs per tile (tile_mn)
  float MMSEQ_LDS* dtab = (float MMSEQ_LDS*)(smem + 2 * 2 * G_LDA_HALF);
  if (BWD) dtab_fill<ACT>(dtab);  // read after the prologue's barrier
  // XCD-aware order: the G/8 blocks sharing an XCD take consecutive tiles (shared A panels in L2)
  const int bid = blockIdx.x;
  const int first = xcd_item(bid, G);
  // Epilogue de-synchronisation: the blocks with one tile fewer than the busiest ones have that
  // tile's time as slack; they start `delay` shader cycles late, so their epilogue store bursts
  // fall in the other blocks' main loops instead of all CUs storing at once.
  if (delay > 0 && first < ntiles && (ntiles - 1 - first) / G < (ntiles - 1) / G) {
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
    while (__builtin_amdgcn_s_memtime() - t0 < (uint64_t)delay) __builtin_amdgcn_s_sleep(8);
  }
  const int nk = F8 ? a.K >> 7 : a.K >> 6;  // 128-byte K-tiles
  const int64_t lda_b = F8 ? a.lda : 2 * a.lda, ldb_b = F8 ? a.ldb : 2 * a.ldb;  // row bytes
  const int64_t kbytes = F8 ? a.K : 2 * a.K;
  const uint8_t* Ab = reinterpret_cast<const uint8_t*>(a.A);
  const uint8_t* Bb = reinterpret_cast<const uint8_t*>(a.B);
  const int KB32 = a.K >> 5;  // F8: E8M0 blocks per row
  // LDS image order: bf16 [A0 | B0 | A1 | B1] (K-tile buffer, then operand), F8 [A0 | A1 | B0 | B1]:
  // there every fragment read of both buffers is within the 64 KB immediate offset of one base
  // register per (operand, k-half); with the bf16 order the F8 kernels (which hold 16 more scale
  // and descriptor registers) spilled those bases and reloaded them inside the main loop, each
  // reload a vmcnt(0) that waited out the in-flight DMA
  constexpr int LBUF = F8 ? G_LDA_HALF : 2 * G_LDA_HALF;  // elements between the two buffers
  constexpr int LOPB = F8 ? 2 * G_LDA_HALF : G_LDA_HALF;  // elements to the B image

  // per-lane source offsets (bytes) for a 1 KB piece = 8 rows x 128 B; the swizzle term
  // ((row >> 1) & 7) = (lane >> 4) | 4 * (g8 & 1) depends on the parity of the 8-row group
  const int lr = lane >> 3, lc = lane & 7;
  const uint32_t offA0 = (uint32_t)(lr * lda_b + ((lc ^ (lane >> 4)) << 4));
  const uint32_t offA1 = (uint32_t)(lr * lda_b + ((lc ^ ((lane >> 4) | 4)) << 4));
  // B: swizzle term ((lane >> 4) & 1) | ((g8 & 3) << 1)
  const uint32_t offB0 = (uint32_t)(lr * ldb_b + ((lc ^ ((lane >> 4) & 1)) << 4));
  const uint32_t offB1 = (uint32_t)(lr * ldb_b + ((lc ^ (((lane >> 4) & 1) | 2)) << 4));
  const uint32_t offB2 = (uint32_t)(lr * ldb_b + ((lc ^ (((lane >> 4) & 1) | 4)) << 4));
  const uint32_t offB3 = (uint32_t)(lr * ldb_b + ((lc ^ (((lane >> 4) & 1) | 6)) << 4));

  // operand descriptors of the current and the next tile, computed once per tile (the tile order
  // costs integer divisions): past the last tile a zero-size range (zero-fill, no traffic)
  // F8: the scale arrays (one descriptor each for the whole kernel) and the first 64-row scale
  // group of a tile's A / B rows; past the last tile, groups whose offsets fall outside the array
  // (zero-fill, no traffic)
  const rsrc_t rBias = make_rsrc(a.bias, a.bias ? (int64_t)a.N * 4 : 0);  // columns >= N read 0
  const rsrc_t rSA = make_rsrc(a.f8_sa, F8 ? a.f8_sa_bytes : 0);
  const rsrc_t rSB = make_rsrc(a.f8_sb, F8 ? a.f8_sb_bytes : 0);
  struct Sc { int ga, gb; };
  auto descs = [&](int tile, rsrc_t& ra, rsrc_t& rb, Sc& sc) {
    if (tile < ntiles) {
      int tm, tn;
      tile_mn(tile, tiles_n, ntiles, tm, tn, aux2);
      const int m0 = tm * 256, n0 = tn * 256;
      ra = make_rsrc(Ab + (int64_t)m0 * lda_b, (int64_t)(a.M - m0 - 1) * lda_b + kbytes);
      rb = make_rsrc(Bb + (int64_t)n0 * ldb_b, (int64_t)(a.N - n0 - 1) * ldb_b + kbytes);
      sc.ga = m0 >> 6;
      sc.gb = n0 >> 6;
    } else {
      ra = rb = make_rsrc(Ab, 0);
      sc.ga = (int)(a.f8_sa_bytes / 64 / (KB32 > 0 ? KB32 : 1));
      sc.gb = (int)(a.f8_sb_bytes / 64 / (KB32 > 0 ? KB32 : 1));
    }
  };
  rsrc_t rAc, rBc, rAn, rBn;
  Sc scc{}, scn{};
  descs(first, rAc, rBc, scc);
  descs(first + G, rAn, rBn, scn);

  // stage half-tile X of K-tile kk of the current tile (kk >= nk: the next tile's K-tile kk - nk)
  auto stage = [&](int it, int kk, int X) {
    (void)it;
    const bool nxt = kk >= nk;
    if (nxt) kk -= nk;
    const bool isA = (X == 0 || X == 3);
    const rsrc_t r = isA ? (nxt ? rAn : rAc) : (nxt ? rBn : rBc);
    const int64_t ld = isA ? lda_b : ldb_b;
    unsigned short* img = smem + (kk & 1) * LBUF + (isA ? 0 : LOPB);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = wave * 2 + i;
      const int g8 = g8_of(X, q);
      const int gb = g8 & 3;
      const uint32_t lo = isA ? ((g8 & 1) ? offA1 : offA0)
                              : (gb == 0 ? offB0 : gb == 1 ? offB1 : gb == 2 ? offB2 : offB3);
      const uint32_t voff = lo + (uint32_t)(g8 * 8 * ld + kk * 128);
      dma16(r, img + g8 * 512, voff);
    }
    if (F8 && X == 3) {  // the K-tile's scales: waves 0-3 the A groups, 4-7 the B groups (16 lanes)
      const bool sa = wave < 4;
      const int grp = (sa ? (nxt ? scn.ga : scc.ga) : (nxt ? scn.gb : scc.gb)) + (wave & 3);
      const uint32_t so = (uint32_t)(((int64_t)grp * KB32 + 4 * kk) * 64 + lane * 16);
      unsigned short* dst = sscale + (kk & 1) * 1024 + wave * 128;
      if (sa) {
        if (lane < 16) dma16(rSA, dst, so);
      } else {
        if (lane < 16) dma16(rSB, dst, so);
      }
    }
  };

  // fragment read offsets (elements): row = base + l15, chunk (ks * 4 + (lane >> 4)) ^ (l15 >> 1)
  const int l15 = lane & 15;
  const int sw0 = ((lane >> 4) ^ (l15 >> 1)) << 3;
  const int sw1 = ((4 + (lane >> 4)) ^ (l15 >> 1)) << 3;
  const int arow = (wr * 128 + l15) * 64;
  const int hb = ((l15 >> 1) & 1) | ((l15 >> 2) << 1);
  const int swb0 = ((lane >> 4) ^ hb) << 3;
  const int swb1 = ((4 + (lane >> 4)) ^ hb) << 3;
  const int brow = LOPB + ((wc >> 1) * 128 + (wc & 1) * 64 + 8 * (l15 >> 2) + (l15 & 3)) * 64;
#define FR(base, t, ks) __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8*>( \
      smem + (base) + (t) * 1024 + ((ks) ? sw1 : sw0)))
#define FRB(base, j, ks) __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8*>( \
      smem + (base) + (4 * ((j) & 1) + 32 * ((j) >> 1)) * 64 + ((ks) ? swb1 : swb0)))

  // F8 scale dwords of the K-tile being computed (lane group b = lane >> 4 = its K block): A rows of
  // fragment i are 16-row block i & 3 of 64-row group wr * 2 + (i >> 2) (byte i & 3 of dword
  // i >> 2); B fragment j's permuted rows (brow / FRB) are all in group wc, row r64 = 8 (l15 >> 2) +
  // (l15 & 3) + 4 (j & 1) + 32 (j >> 1): dword j & 1, byte (l15 >> 3) + 2 (j >> 1)
  uint32_t scA[2] = {0u, 0u}, scB[2] = {0u, 0u};
  const int scb_sh = 8 * (l15 >> 3);
  const uint8_t* scbase = reinterpret_cast<const uint8_t*>(sscale) + (lane >> 4) * 64;
  auto read_scales = [&](int h) {
    const uint8_t* sp = scbase + h * 2048;
    scA[0] = *reinterpret_cast<const uint32_t*>(sp + (wr * 2) * 256 + l15 * 4);
    scA[1] = *reinterpret_cast<const uint32_t*>(sp + (wr * 2 + 1) * 256 + l15 * 4);
    const int rb = 8 * ((l15 >> 2) & 1) + (l15 & 3);
    scB[0] = *reinterpret_cast<const uint32_t*>(sp + 1024 + wc * 256 + rb * 4);
    scB[1] = *reinterpret_cast<const uint32_t*>(sp + 1024 + wc * 256 + (rb + 4) * 4);
  };
#define QUAD(I0, I1, J0, J1)                                                                      \
  if (F8) {                                                                                       \
    uint32_t sa_[I1 - I0], sb_[J1 - J0];                                                          \
    _Pragma("unroll") for (int i = I0; i < I1; ++i) sa_[i - I0] = scA[i >> 2] >> (8 * (i & 3));   \
    _Pragma("unroll") for (int j = J0; j < J1; ++j)                                               \
      sb_[j - J0] = scB[j & 1] >> (scb_sh + 16 * (j >> 1));                                       \
    /* asm MFMAs are invisible to the hazard recognizer: the scale VGPRs written by VALU get */    \
    /* explicit wait states before the first MFMA reads them */                                   \
    asm volatile("s_nop 4" ::"v"(sa_[0]), "v"(sa_[I1 - I0 - 1]), "v"(sb_[0]), "v"(sb_[J1 - J0 - 1])); \
    _Pragma("unroll") for (int i = I0; i < I1; ++i)                                               \
    _Pragma("unroll") for (int j = J0; j < J1; ++j)                                               \
      mfma_f8_acc(acc[i][j], fb8[j], fa8[i], sb_[j - J0], sa_[i - I0]);                           \
  } else {                                                                                        \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                              \
    _Pragma("unroll") for (int i = I0; i < I1; ++i)                                               \
    _Pragma("unroll") for (int j = J0; j < J1; ++j)                                               \
      acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j][ks], fa[i][ks], acc[i][j], 0, 0, 0); \
  }

  int it = 0;
  if (first >= ntiles) return;
  stage(0, 0, 0); stage(0, 0, 1); stage(0, 0, 2); stage(0, 0, 3);
  stage(0, 1, 0); stage(0, 1, 1);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (wr) __builtin_amdgcn_s_barrier();  // stagger: waves 4-7 one barrier behind

  f32x4 acc[8][4];
  bf16x8_t fa[8][2], fb[4][2];  // bf16: the fragments of the two 32-deep k-steps
  i32x8 fa8[8], fb8[4];         // F8: the same bytes as one 8-register operand (no copies)
#define LDA(i)                                                                  \
  do {                                                                          \
    if (F8) fa8[i] = cat8(FR(buf + arow, i, 0), FR(buf + arow, i, 1));          \
    else { fa[i][0] = FR(buf + arow, i, 0); fa[i][1] = FR(buf + arow, i, 1); }  \
  } while (0)
#define LDB(j)                                                                  \
  do {                                                                          \
    if (F8) fb8[j] = cat8(FRB(buf + brow, j, 0), FRB(buf + brow, j, 1));        \
    else { fb[j][0] = FRB(buf + brow, j, 0); fb[j][1] = FRB(buf + brow, j, 1); } \
  } while (0)
  for (int tile = first; tile < ntiles; tile += G, ++it) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (ACT >= 0 && wave == 0) {
      uint32_t ln;  // the lane index recomputed here (not a hoisted, possibly spilled lane constant)
      asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
      dma16(rBias, sbias + (it & 1) * 512, (uint32_t)(scc.gb * 256) + ln * 16u);
    }

    for (int s = 0; s < (nk >> 1); ++s) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {  // h = 0: even K-tile 2s, h = 1: odd K-tile 2s + 1
        const int buf = h * LBUF;
        // ---- phase 1 (5): A_lo + B_lo, quadrant (i 0-3, j 0-1)
#pragma unroll
        for (int i = 0; i < 4; ++i) LDA(i);
#pragma unroll
        for (int j = 0; j < 2; ++j) LDB(j);
        if (F8) read_scales(h);
        if (h == 0) stage(it, 2 * s + 1, 2); else stage(it, 2 * s + 2, 2);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        QUAD(0, 4, 0, 2)
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        // ---- phase 2 (6): B_hi, quadrant (i 0-3, j 2-3)
#pragma unroll
        for (int j = 2; j < 4; ++j) LDB(j);
        if (h == 0) stage(it, 2 * s + 1, 3); else stage(it, 2 * s + 2, 3);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        QUAD(0, 4, 2, 4)
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        // ---- phase 3 (7): A_hi, quadrant (i 4-7, j 2-3)
#pragma unroll
        for (int i = 4; i < 8; ++i) LDA(i);
        if (h == 0) stage(it, 2 * s + 2, 0); else stage(it, 2 * s + 3, 0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        QUAD(4, 8, 2, 4)
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        // ---- phase 4 (8): no reads, quadrant (i 4-7, j 0-1); retire the K-tile read next
        if (h == 0) stage(it, 2 * s + 2, 1); else stage(it, 2 * s + 3, 1);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        QUAD(4, 8, 0, 2)
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
      }
    }

    // ---- epilogue (the next tile's first K-tiles are already in flight)
    if (F8) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");  // asm MFMA results
    int tm, tn;
    tile_mn(tile, tiles_n, ntiles, tm, tn, aux2);
    const int m0 = tm * 256, n0 = tn * 256;
    // Q8: the lane index re-read per tile (volatile asm), so the epilogue's lane-derived offsets
    // are recomputed here instead of hoisted out of the tile loop, spilled and reloaded
    int lane_e = lane;
    if (Q8) asm volatile("v_mov_b32 %0, %1" : "=v"(lane_e) : "v"(lane));
    const int g = lane_e >> 4, ii = lane_e & 15;
    if (ACT < 0) {  // benchmark-only variant: main loop without the epilogue stores
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(acc[i][j]));
      rAc = rAn;
      rBc = rBn;
      scc = scn;
      descs(tile + 2 * G, rAn, rBn, scn);
      continue;
    }
    EpiBias bias0, bias1;
    {
      const float* sb = reinterpret_cast<const float*>(sbias + (it & 1) * 512) + wc * 64 + 8 * g;
      bias0.b0 = *reinterpret_cast<const f32x4*>(sb);
      bias0.b1 = *reinterpret_cast<const f32x4*>(sb + 4);
      bias1.b0 = *reinterpret_cast<const f32x4*>(sb + 32);
      bias1.b1 = *reinterpret_cast<const f32x4*>(sb + 36);
    }
    if (XIN) {
      // batches of 4 calls; the operand loads of batch h + 1 are issued before the stores of batch
      // h, and each batch is consumed (settled) once, so its wait never covers a store (vmcnt
      // retires in issue order; a consume inside the per-call bounds branches would wait vmcnt(0)).
      // (Three or four batches in flight spill: the fragment registers are not reused here.)
      // Interior tiles (the whole 256 x 256 tile inside C) run without per-call bounds branches.
#define XIN_EPI(CHK_) \
      EpiIn in[2][2][2]; \
_Pragma("unroll") \
      for (int i = 0; i < 2; ++i) \
_Pragma("unroll") \
        for (int t = 0; t < 2; ++t) \
          in[0][i][t] = epi8_load<BWD, Q8, CHK_>(a, m0 + wr * 128 + i * 16 + ii, n0 + wc * 64 + 32 * t + 8 * g); \
_Pragma("unroll") \
      for (int h = 0; h < 4; ++h) { \
        if (h + 1 < 4) { \
_Pragma("unroll") \
          for (int i = 0; i < 2; ++i) \
_Pragma("unroll") \
            for (int t = 0; t < 2; ++t) \
              in[(h + 1) & 1][i][t] = epi8_load<BWD, Q8, CHK_>(a, m0 + wr * 128 + (2 * h + 2 + i) * 16 + ii, \
                                                     n0 + wc * 64 + 32 * t + 8 * g); \
        } \
        asm volatile("" ::"v"(in[h & 1][0][0].x), "v"(in[h & 1][0][1].x), "v"(in[h & 1][1][0].x), \
                     "v"(in[h & 1][1][1].x)); \
_Pragma("unroll") \
        for (int i = 0; i < 2; ++i) \
_Pragma("unroll") \
          for (int t = 0; t < 2; ++t) { \
            if (Q8 && BWD) \
              epi8_q8<ACT, true>(a, m0 + wr * 128 + (2 * h + i) * 16 + ii, n0 + wc * 64 + 32 * t + 8 * g, g, \
                                 acc[2 * h + i][2 * t], acc[2 * h + i][2 * t + 1], t ? bias1 : bias0, \
                                 sq8 + (((2 * h + i) >> 2) * 2 + t) * 64 + ii * 4 + ((2 * h + i) & 3), \
                                 &in[h & 1][i][t], dtab); \
            else \
              epi8<ACT, BWD, true, BWD, CHK_>(a, m0 + wr * 128 + (2 * h + i) * 16 + ii, n0 + wc * 64 + 32 * t + 8 * g, \
                                        acc[2 * h + i][2 * t], acc[2 * h + i][2 * t + 1], in[h & 1][i][t], \
                                        t ? bias1 : bias0, dtab); \
          } \
      }
      if (!(Q8 && BWD) && (ACT == 0 || BWD) && m0 + 256 <= a.M && n0 + 256 <= a.N) {
        XIN_EPI(false)
      } else {
        XIN_EPI(true)
      }
#undef XIN_EPI
      if (Q8 && BWD)
        q8_scale_words(a, m0 + wr * 128 + (g >> 1) * 64 + ii, n0 + wc * 64 + 32 * (g & 1), sq8, lane_e);
    } else if (Q8) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          epi8_q8<ACT>(a, m0 + wr * 128 + i * 16 + ii, n0 + wc * 64 + 32 * t + 8 * g, g,
                       acc[i][2 * t], acc[i][2 * t + 1], t ? bias1 : bias0,
                       sq8 + ((i >> 2) * 2 + t) * 64 + ii * 4 + (i & 3));
      q8_scale_words(a, m0 + wr * 128 + (g >> 1) * 64 + ii, n0 + wc * 64 + 32 * (g & 1), sq8, lane_e);
    } else {
      const EpiIn none = {(u16x8){0, 0, 0, 0, 0, 0, 0, 0}};
      if (m0 + 256 <= a.M && n0 + 256 <= a.N) {  // interior tiles without the per-call bounds branches
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int t = 0; t < 2; ++t)
            epi8<ACT, BWD, false, false, false>(a, m0 + wr * 128 + i * 16 + ii, n0 + wc * 64 + 32 * t + 8 * g,
                                                acc[i][2 * t], acc[i][2 * t + 1], none, t ? bias1 : bias0);
      } else
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          epi8<ACT, BWD, false>(a, m0 + wr * 128 + i * 16 + ii, n0 + wc * 64 + 32 * t + 8 * g,
                                acc[i][2 * t], acc[i][2 * t + 1], none, t ? bias1 : bias0);
    }
    rAc = rAn;
    rBc = rBn;
    scc = scn;
    descs(tile + 2 * G, rAn, rBn, scn);
  }
#undef FR
#undef FRB
#undef QUAD
#undef LDA
#undef LDB
  if (!wr) __builtin_amdgcn_s_barrier();  // balance the stagger
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA may outlive the workgroup
}


// ---------------------------------------------------------------------------------------------
// Large TN kernel (weight gradients dW[M][N] (+)= sum_k dY[k][M] X[k][N] over the 164k rows):
// one 256 x 256 output tile x one K-split per 512-thread workgroup, the same 8-phase skeleton as
// the NT kernel, but the phases split the K-tile by k-half, so a phase reads fragments for every
// output column: phase 1 A(ks0, i 0-3) + B(ks0, j 0-3), 2 A(ks0, i 4-7), 3 A(ks1, i 0-3) +
// B(ks1), 4 A(ks1, i 4-7). Half-tiles are whole k-rows (A_ks0 = k 0-31 of the A image, ...), so
// LDS-DMA pieces are two 512-B rows. Images [64 k][256 m|n], 16-B chunk' = chunk ^ ((k & 7) << 1):
// the ds_read_b64_tr_b16 fragment reads (8 k-rows x 32 B per 32-lane half) are conflict-free.
// k order inside a 32-step is permuted identically for both operands (lane group g supplies
// k {4g..4g+3} U {16+4g..16+4g+3}). Rows past the split's end are zero-filled by the buffer range.
// Output: fp32, raw partial slab [split][M][N] when split > 1, else C (+)= the tile.
// Two instances. CS = false (no bias gradient): the MFMA bursts alone. CS = true: the column sums
// of dY for the bias gradient ride inside the bursts. A wave's register slots hold its A tiles
// rotated by wc, so the tile it sums is the first slot of every phase; the 16 VALU of a phase's
// sum (unpack, pair adds, chain) are pinned two behind each of the first eight MFMAs with
// sched_group_barrier, where the MFMA pipe is busy anyway; a block-uniform mask instead of a
// branch turns the sum off in K-tiles that belong to another column tile, so a phase stays one
// basic block. (In front of the burst the sums cost 9-12 % of the kernel; a branch around two
// copies of the burst spilled 230 VGPRs; without the split in two instances the bias-free calls
// carried the accumulator copies the allocator made for the branch.) 217 VGPRs with the sums, 228
// without, every accumulator in place, no scratch in either.
// ---------------------------------------------------------------------------------------------
template <bool CS>
__global__ __launch_bounds__(512, 1) void gemm256_tn_kernel(GemmArgs a, int tiles_n, int ntiles) {
  __shared__ __attribute__((aligned(16))) unsigned short smem[2 * 2 * G_LDA_HALF];  // 128 KB
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int G = gridDim.x;
  const int bid = blockIdx.x;
  const int item = xcd_item(bid, G);
  const int split = item / ntiles, tile = item - split * ntiles;
  const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
  const int m0 = tm * 256, n0 = tn * 256;
  const int kbeg = split * a.kchunk;
  const int kend = min(a.K, kbeg + a.kchunk);
  const int nk = (((kend - kbeg) + 127) >> 7) << 1;  // even number of 64-deep K-tiles
  const unsigned short* Ab = reinterpret_cast<const unsigned short*>(a.A);
  const unsigned short* Bb = reinterpret_cast<const unsigned short*>(a.B);
  const rsrc_t ra = make_rsrc(Ab + (int64_t)kbeg * a.lda + m0,
                              ((int64_t)(kend - kbeg - 1) * a.lda + (a.M - m0)) * 2);
  const rsrc_t rb = make_rsrc(Bb + (int64_t)kbeg * a.ldb + n0,
                              ((int64_t)(kend - kbeg - 1) * a.ldb + (a.N - n0)) * 2);
  const rsrc_t rz = make_rsrc(Ab, 0);

  // DMA piece = 2 k-rows x 512 B; lane -> row (lane >> 5), chunk lane & 31; swizzle term
  // ((row & 7) << 1) with row & 7 = 2 (q & 3) + (lane >> 5) for wave-instruction q
  uint32_t offA[4], offB[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int rr = 2 * v + (lane >> 5);
    const int c = (lane & 31) ^ (rr << 1);
    offA[v] = (uint32_t)((lane >> 5) * a.lda * 2 + c * 16);
    offB[v] = (uint32_t)((lane >> 5) * a.ldb * 2 + c * 16);
  }
  // half-tile X: 0 = A_ks0, 1 = B_ks0, 2 = A_ks1, 3 = B_ks1 (k-rows 32 (X >> 1) .. +31)
  auto stage = [&](int kk, int X) {
    const bool isA = (X & 1) == 0;
    const rsrc_t r = kk < nk ? (isA ? ra : rb) : rz;
    const int64_t ld = isA ? a.lda : a.ldb;
    unsigned short* img = smem + (kk & 1) * (2 * G_LDA_HALF) + (isA ? 0 : G_LDA_HALF);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int q = wave * 2 + i;
      const int row = (X >> 1) * 32 + 2 * q;
      const uint32_t lo = isA ? offA[q & 3] : offB[q & 3];
      const uint32_t voff = lo + (uint32_t)(((int64_t)kk * 64 + row) * ld * 2);
      dma16(r, img + row * 256, voff);
    }
  };

  // transposed fragment reads: lane (g, ii = 4 q' + p) reads k-row 4g + q' (+16) at column
  // base + 4p, i.e. chunk 2 (tile) + (p >> 1) XOR-swizzled by ((4g + q') & 7) << 1
  const int qq = (lane & 15) >> 2, pp = lane & 3;
  const int kr = 4 * (lane >> 4) + qq, t8 = kr & 7;
  int fA[8], fB[4];
  // Register slot i of a wave holds A tile ti(i): the four tiles of a phase rotated by wc, so the
  // tile whose column sums the wave owns (wc, 4 + wc) is always the phase's first slot and the
  // bias sums need no branch on wc inside the MFMA burst. Every accumulator still sees its K-tiles
  // in the same order, so the rotation changes no result.
  auto ti = [&](int i) { return (i & 4) | ((i + wc) & 3); };
#pragma unroll
  for (int i = 0; i < 8; ++i)
    fA[i] = kr * 256 + (((wr * 16 + 2 * ti(i) + (pp >> 1)) ^ (t8 << 1)) << 3) + (pp & 1) * 4;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    fB[j] = G_LDA_HALF + kr * 256 + (((wc * 8 + 2 * j + (pp >> 1)) ^ (t8 << 1)) << 3) + (pp & 1) * 4;
  auto frag = [&](int off) -> bf16x8_t {
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MMSEQ_LDS s16x4*)(smem + off));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MMSEQ_LDS s16x4*)(smem + off + 16 * 256));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8_t, v);
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  bf16x8_t fa[8], fb[4];
  // fused bias gradient (column sums of A = dY): wave wc sums A tiles wc (cs0) and 4 + wc (cs1),
  // its register slots 0 and 4, on the VALU between its MFMAs; lane (g, ii) holds the partial
  // over its k-slots of column wr*128 + i*16 + ii. With a partial slab (a.cs_slab) the tiles_n blocks that share an M-tile
  // split the work by K-tile (K-tile k goes to column tile k % tiles_n) and each writes its own
  // partial row [split * tiles_n + tn], so no block is slower than the others; without one, the
  // first column tile's blocks do it all (a.cs += directly).
  const bool cs_split = a.cs_slab != nullptr;
  const bool do_cs = CS && a.cs != nullptr && (cs_split || tn == 0);
  float cs0 = 0.f, cs1 = 0.f;
  // the summed fragment is the MFMA's own A fragment fa[I0] of the phase (no extra LDS read
  // or register: a separate transposed read of it held 4 more VGPRs in a kernel at 256)
  // on: all ones in the K-tiles this block sums, else 0 (the sum then adds +0.0, which leaves dst
  // as it is: dst starts at +0.0 and never becomes -0.0), so the burst has no branch in it
  auto cs_add = [&](float& dst, const bf16x8_t& f, uint32_t on) {
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    const u32x4 u = __builtin_bit_cast(u32x4, f);
    // (the chain starts at the first pair, not at 0: that differs only when every term is -0.0,
    // and then only in the sign of a zero that is added to dst, which is never -0.0)
    float t = __uint_as_float(u[0] << 16) + __uint_as_float(u[0] & 0xFFFF0000u);
#pragma unroll
    for (int e = 1; e < 4; ++e) t += __uint_as_float(u[e] << 16) + __uint_as_float(u[e] & 0xFFFF0000u);
    dst += __uint_as_float(__float_as_uint(t) & on);
  };

  stage(0, 0); stage(0, 1); stage(0, 2); stage(0, 3);
  stage(1, 1); stage(1, 0);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (wr) __builtin_amdgcn_s_barrier();  // stagger: waves 4-7 one barrier behind

#define TN_MFMAS(I0)                                                                    \
  _Pragma("unroll") for (int i = I0; i < I0 + 4; ++i)                                   \
  _Pragma("unroll") for (int j = 0; j < 4; ++j)                                         \
      acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
#define TN_PHASE(READS, STAGE, VMWAIT, I0, KS)                                          \
  READS;                                                                                \
  STAGE;                                                                                \
  __builtin_amdgcn_sched_barrier(0);                                                    \
  if (VMWAIT) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                          \
  __builtin_amdgcn_s_barrier();                                                         \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                    \
  __builtin_amdgcn_sched_barrier(0);                                                    \
  __builtin_amdgcn_s_setprio(1);                                                        \
  /* CS: the sums of the phase's own first fragment, issued between the MFMAs that read it */ \
  /* (two VALU after each of the first eight MFMAs), so the MFMA pipe never waits for them  */ \
  /* and the fragment dies with its phase; one basic block (a branch around two copies of  */ \
  /* the burst spilled 230 VGPRs)                                                          */ \
  if (CS) cs_add((I0) ? cs1 : cs0, fa[I0], cs_on);                                        \
  TN_MFMAS(I0)                                                                            \
  if (CS) {                                                                               \
    _Pragma("unroll") for (int p = 0; p < 9; ++p) {                                       \
      __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);                                    \
      __builtin_amdgcn_sched_group_barrier(0x2, 2, 0);                                    \
    }                                                                                     \
    __builtin_amdgcn_sched_group_barrier(0x8, 7, 0);                                      \
  }                                                                                       \
  __builtin_amdgcn_s_setprio(0);                                                        \
  __builtin_amdgcn_sched_barrier(0);                                                    \
  __builtin_amdgcn_s_barrier();

  int kmod = 0;
  for (int s = 0; s < (nk >> 1); ++s) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int buf = h * (2 * G_LDA_HALF);
      // block-uniform, and computed without a branch (the loop body stays one basic block, so
      // nothing of a phase can be sunk past it): this block sums the bias columns of K-tile
      // 2 s + h when kmod = (2 s + h) % tiles_n is its column tile
      const uint32_t cs_on = (uint32_t)(do_cs & (!cs_split | (kmod == tn))) ? ~0u : 0u;
      kmod = kmod + 1 == tiles_n ? 0 : kmod + 1;
      // phase 1 (5): ks0, i 0-3
      TN_PHASE(
          { _Pragma("unroll") for (int i = 0; i < 4; ++i) fa[i] = frag(buf + fA[i]);
            _Pragma("unroll") for (int j = 0; j < 4; ++j) fb[j] = frag(buf + fB[j]); },
          { if (h == 0) stage(2 * s + 1, 3); else stage(2 * s + 2, 3); }, false, 0, 0)
      // phase 2 (6): ks0, i 4-7
      TN_PHASE({ _Pragma("unroll") for (int i = 4; i < 8; ++i) fa[i] = frag(buf + fA[i]); },
               { if (h == 0) stage(2 * s + 1, 2); else stage(2 * s + 2, 2); }, false, 4, 0)
      // phase 3 (7): ks1, i 0-3
      TN_PHASE(
          { _Pragma("unroll") for (int i = 0; i < 4; ++i) fa[i] = frag(buf + 32 * 256 + fA[i]);
            _Pragma("unroll") for (int j = 0; j < 4; ++j) fb[j] = frag(buf + 32 * 256 + fB[j]); },
          { if (h == 0) stage(2 * s + 2, 1); else stage(2 * s + 3, 1); }, false, 0, 1)
      // phase 4 (8): ks1, i 4-7; retire the K-tile read next
      TN_PHASE({ _Pragma("unroll") for (int i = 4; i < 8; ++i) fa[i] = frag(buf + 32 * 256 + fA[i]); },
               { if (h == 0) stage(2 * s + 2, 0); else stage(2 * s + 3, 0); }, true, 4, 1)
    }
  }
#undef TN_PHASE
#undef TN_MFMAS
  if (!wr) __builtin_amdgcn_s_barrier();  // balance the stagger
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // the epilogue's lane coordinates from a lane index read here (volatile asm): derived from the
  // one read at kernel start they were hoisted above the K-loop and held registers through it
  // (two of them spilled in the bias variant)
  int g, ii;
  {
    uint32_t ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    g = (int)(ln >> 4);
    ii = (int)(ln & 15);
  }

  if (do_cs) {
    cs0 += __shfl_xor(cs0, 16, 64);
    cs0 += __shfl_xor(cs0, 32, 64);
    cs1 += __shfl_xor(cs1, 16, 64);
    cs1 += __shfl_xor(cs1, 32, 64);
    if (g == 0) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int m = m0 + wr * 128 + (q * 4 + wc) * 16 + ii;
        const float v = q ? cs1 : cs0;
        if (m < a.M) {
          if (cs_split) a.cs_slab[((int64_t)split * tiles_n + tn) * a.M + m] = v;
          else a.cs[m] += v;
        }
      }
    }
  }
  float* C = a.splitk > 1 ? a.slab + (int64_t)split * a.M * a.N : reinterpret_cast<float*>(a.C);
  const int64_t ldc = a.splitk > 1 ? a.N : a.ldc;
  // Two loops on the uniform accumulate flag: a C load anywhere in the store loop would put a
  // vmcnt(0) (= every earlier store, in-order retirement) in front of each store. Accumulate: the
  // C rows of i-step i + 1 are loaded before the stores of step i and consumed once per step.
  if (!(a.splitk == 1 && a.accumulate)) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + wr * 128 + ti(i) * 16 + ii;
        const int n = n0 + wc * 64 + j * 16 + 4 * g;
        if (m < a.M && n < a.N)  // N % 8 == 0: n .. n + 3 in range
          *reinterpret_cast<f32x4*>(C + (int64_t)m * ldc + n) = acc[i][j];
      }
  } else {
    auto ld = [&](int i, int j) {
      const int m = m0 + wr * 128 + ti(i) * 16 + ii;
      const int n = n0 + wc * 64 + j * 16 + 4 * g;
      return (m < a.M && n < a.N) ? *reinterpret_cast<const f32x4*>(C + (int64_t)m * ldc + n)
                                  : (f32x4){0.f, 0.f, 0.f, 0.f};
    };
    f32x4 cin[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) cin[0][j] = ld(0, j);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i + 1 < 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) cin[(i + 1) & 1][j] = ld(i + 1, j);
      }
      asm volatile("" ::"v"(cin[i & 1][0]), "v"(cin[i & 1][1]), "v"(cin[i & 1][2]), "v"(cin[i & 1][3]));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + wr * 128 + ti(i) * 16 + ii;
        const int n = n0 + wc * 64 + j * 16 + 4 * g;
        if (m < a.M && n < a.N)
          *reinterpret_cast<f32x4*>(C + (int64_t)m * ldc + n) = acc[i][j] + cin[i & 1][j];
      }
    }
  }
}


// ---------------------------------------------------------------------------------------------
// Two-blocks-per-CU NT kernel ("2B"): persistent 256 x 128 tiles, 4 waves (2 x 2, 128 x 64 per
// wave: the same fragment maps and 16-byte epilogue as above), BK = 32, a 3-stage LDS-DMA ring
// (24 KB per stage, 72 KB per block), one barrier per 32-deep k-step. Two workgroups share a CU
// and are NOT barrier-coupled, so one block's epilogue (stores, dropout hashing, residual loads)
// runs beside the other block's MFMAs instead of stalling the whole CU.
// Images: A [256][32] and B [128][32] bf16 (64-B rows); 16-B chunk c of row r stored at
// c ^ (((r >> 3) & 1) << 1): conflict-free for the row-fragment reads of both the plain A rows and
// the permuted B rows (8 (rho >> 2) + 4 (j & 1) + (rho & 3) + 32 (j >> 1)).
// ---------------------------------------------------------------------------------------------
constexpr int S2_STAGE = 256 * 32 + 128 * 32;  // elements per stage

template <int ACT, bool BWD, bool XIN>
__global__ __launch_bounds__(256, 2) void gemm_nt_2b_kernel(GemmArgs a, int tiles_n, int ntiles,
                                                             int /*delay: unused*/) {
  __shared__ __attribute__((aligned(16))) unsigned short smem[3 * S2_STAGE];  // 72 KB
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int G = gridDim.x;
  const int bid = blockIdx.x;
  const int first = xcd_item(bid, G);
  const int nk = a.K >> 5;  // 32-deep k-steps per tile
  const unsigned short* Ab = reinterpret_cast<const unsigned short*>(a.A);
  const unsigned short* Bb = reinterpret_cast<const unsigned short*>(a.B);

  // DMA piece = 16 rows x 64 B: lane -> row (lane >> 2), chunk lane & 3, swizzle ((lane >> 5) & 1) << 1
  const int sw = ((lane >> 5) & 1) << 1;
  const uint32_t offA = (uint32_t)((lane >> 2) * a.lda * 2 + (((lane & 3) ^ sw) << 4));
  const uint32_t offB = (uint32_t)((lane >> 2) * a.ldb * 2 + (((lane & 3) ^ sw) << 4));
  // stage k-step kk of tile iteration it (kk >= nk: the next tile's k-step kk - nk)
  auto stage = [&](int it, int kk) {
    if (kk >= nk) { kk -= nk; ++it; }
    const int tile = first + it * G;
    rsrc_t ra, rb;
    if (tile < ntiles) {
      const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
      const int m0 = tm * 256, n0 = tn * 128;
      ra = make_rsrc(Ab + (int64_t)m0 * a.lda, ((int64_t)(a.M - m0 - 1) * a.lda + a.K) * 2);
      rb = make_rsrc(Bb + (int64_t)n0 * a.ldb, ((int64_t)(a.N - n0 - 1) * a.ldb + a.K) * 2);
    } else {
      ra = rb = make_rsrc(Ab, 0);
    }
    unsigned short* st = smem + ((it * nk + kk) % 3) * S2_STAGE;  // ring slot of the global step
    // 24 pieces: 16 of A (rows 16p..), 8 of B; wave w issues pieces w, w + 4, ..., w + 20
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      const int pc = wave + 4 * e;
      if (pc < 16)
        dma16(ra, st + pc * 512, offA + (uint32_t)(((int64_t)pc * 16 * a.lda + kk * 32) * 2));
      else
        dma16(rb, st + 256 * 32 + (pc - 16) * 512,
              offB + (uint32_t)(((int64_t)(pc - 16) * 16 * a.ldb + kk * 32) * 2));
    }
  };

  // fragment offsets (elements within a stage): A rows wr*128 + i*16 + l15, chunk g;
  // B rows wc*64 + 8 (l15 >> 2) + (l15 & 3) + 4 (j & 1) + 32 (j >> 1), chunk g
  const int l15 = lane & 15, g = lane >> 4;
  const int hA = ((l15 >> 3) & 1) << 1;
  const int aoff = (wr * 128 + l15) * 32 + ((g ^ hA) << 3);
  const int rB = 8 * (l15 >> 2) + (l15 & 3);
  const int hB = ((rB >> 3) & 1) << 1;  // 4 (j & 1) and 32 (j >> 1) do not change (r >> 3) & 1
  const int boff = 256 * 32 + (wc * 64 + rB) * 32 + ((g ^ hB) << 3);

  if (first >= ntiles) return;
  stage(0, 0);
  stage(0, 1);
  int it = 0;
  f32x4 acc[8][4];
  for (int tile = first; tile < ntiles; tile += G, ++it) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < nk; ++kk) {
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // k-step kk landed (kk + 1 in flight)
      __builtin_amdgcn_s_barrier();  // ... for every wave; stage (kk + 2) % 3 no longer read
      __builtin_amdgcn_sched_barrier(0);
      stage(it, kk + 2);
      const unsigned short* st = smem + ((it * nk + kk) % 3) * S2_STAGE;
      bf16x8_t fa[8], fb[4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        fa[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8*>(st + aoff + i * 16 * 32));
#pragma unroll
      for (int j = 0; j < 4; ++j)
        fb[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8*>(
                                                 st + boff + (4 * (j & 1) + 32 * (j >> 1)) * 32));
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
    }
    const int tm = tile / tiles_n, tn = tile - tm * tiles_n;
    const int m0 = tm * 256, n0 = tn * 128;
    const int ii = lane & 15;
    const EpiBias bias0 = epi_bias(a, n0 + wc * 64 + 8 * g), bias1 = epi_bias(a, n0 + wc * 64 + 32 + 8 * g);
    if (XIN) {
      // batches of 4 calls; the operand loads of batch h + 1 are issued before the stores of batch
      // h, and each batch is consumed (settled) once, so its wait never covers a store (vmcnt
      // retires in issue order; a consume inside the per-call bounds branches would wait vmcnt(0))
      EpiIn in[2][2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          in[0][i][t] = epi8_load<BWD>(a, m0 + wr * 128 + i * 16 + ii, n0 + wc * 64 + 32 * t + 8 * g);
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        if (h + 1 < 4) {
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t)
              in[(h + 1) & 1][i][t] = epi8_load<BWD>(a, m0 + wr * 128 + (2 * h + 2 + i) * 16 + ii,
                                                     n0 + wc * 64 + 32 * t + 8 * g);
        }
        asm volatile("" ::"v"(in[h & 1][0][0].x), "v"(in[h & 1][0][1].x), "v"(in[h & 1][1][0].x),
                     "v"(in[h & 1][1][1].x));
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int t = 0; t < 2; ++t)
            epi8<ACT, BWD, true>(a, m0 + wr * 128 + (2 * h + i) * 16 + ii, n0 + wc * 64 + 32 * t + 8 * g,
                                 acc[2 * h + i][2 * t], acc[2 * h + i][2 * t + 1], in[h & 1][i][t],
                                 t ? bias1 : bias0);
      }
    } else {
      const EpiIn none = {(u16x8){0, 0, 0, 0, 0, 0, 0, 0}};
      if (m0 + 256 <= a.M && n0 + 256 <= a.N) {  // interior tiles without the per-call bounds branches
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int t = 0; t < 2; ++t)
            epi8<ACT, BWD, false, false, false>(a, m0 + wr * 128 + i * 16 + ii, n0 + wc * 64 + 32 * t + 8 * g,
                                                acc[i][2 * t], acc[i][2 * t + 1], none, t ? bias1 : bias0);
      } else
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          epi8<ACT, BWD, false>(a, m0 + wr * 128 + i * 16 + ii, n0 + wc * 64 + 32 * t + 8 * g,
                                acc[i][2 * t], acc[i][2 * t + 1], none, t ? bias1 : bias0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA may outlive the workgroup
}

// ---------------------------------------------------------------------------------------------
// Ping-pong NT kernel (bf16 forward / dgrad, every bf16 epilogue). One 512-thread workgroup per CU
// holds two independent 4-wave groups; each runs its own persistent sequence of 256 x 128 tiles
// through its own 3-slot LDS-DMA ring (BK = 32: A [256][32] + B [128][32] = 24 KB per slot). The
// groups share only the workgroup barrier: every barrier interval is one step of each group's
// static program, and group 1's program starts an odd number of intervals after group 0's, so
//  * in the main loop one group reads its fragments and issues its DMA ("load") while the other
//    runs its 32 MFMAs per wave ("compute"), the roles swapping every interval, and
//  * a group's epilogue (E intervals, its stores spread over them at ~16 B / cycle per CU, the
//    per-CU store rate) runs beside the other group's main loop instead of idling the CU's MFMA
//    pipes (the 8-wave kernel stops every MFMA pipe of the CU for its epilogue bursts).
// Per group: waves 2 x 2 of 128 x 64 outputs (8 x 4 MFMA 16x16 tiles, the fragment maps and the
// 16-byte epilogue lanes of the 256 x 256 kernel), images as gemm_nt_2b_kernel's (64-B rows, 16-B
// chunk c of row r at c ^ (((r >> 3) & 1) << 1)). Epilogue loads and stores are buffer operations
// on per-tile descriptors: rows past M fall outside the range and columns past N get an
// out-of-range offset, so every call issues exactly its loads and stores and the counted vmcnt
// waits (DMA, epilogue operand loads) stay exact. Preconditions as mmseq_gemm256_nt (K % 128 == 0).
// ---------------------------------------------------------------------------------------------
constexpr int PP_STAGE = 256 * 32 + 128 * 32;  // elements per ring slot (24 KB)

template <int ACT, bool BWD, bool XIN, bool AUX>
struct PPCfg {
  static constexpr int E = ACT < 0 ? 2 : ((AUX || BWD) ? 16 : 8);  // epilogue intervals (even)
  static constexpr int CPI = ACT < 0 ? 0 : 16 / E;                // 8-output calls per interval
  static constexpr int NL = ACT >= 0 && XIN ? 1 : 0;              // operand loads per call
  static constexpr int NS = ACT < 0 ? 0 : (AUX ? 2 : 1);          // stores per call
  static constexpr int EPO = (ACT < 0 ? 0 : 16) * (NL + NS);      // epilogue VMEM ops per tile
};

// vmcnt(N) with a compile-time N (N <= 63)
template <int N>
__device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N <= 63, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int ACT, bool BWD, bool XIN, bool AUX>
__global__ __launch_bounds__(512, 1) void gemm_pp_kernel(GemmArgs a, int tiles_n, int ntiles, int) {
  typedef PPCfg<ACT, BWD, XIN, AUX> Cf;
  constexpr int E = Cf::E, CPI = Cf::CPI, NL = Cf::NL, NS = Cf::NS, EPO = Cf::EPO;
  static_assert(E % 2 == 0 && 6 + EPO <= 63, "epilogue schedule");
  __shared__ __attribute__((aligned(16))) unsigned short
      smem[2 * 3 * PP_STAGE + 2 * 2 * 256 + (BWD ? 4 * DT_N : 0)];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2, w = wave & 3;
  const int wr = w >> 1, wc = w & 1;
  unsigned short* const ring = smem + grp * 3 * PP_STAGE;
  float MMSEQ_LDS* dtab = (float MMSEQ_LDS*)(smem + 2 * 3 * PP_STAGE + 2 * 2 * 256);
  if (BWD) dtab_fill<ACT>(dtab);
  __syncthreads();  // dtab visible; both groups pass it once
  const int G = gridDim.x;
  const int item = xcd_item(blockIdx.x, G);
  const int stride = 2 * G;
  const int first = 2 * item + grp;
  const int my_tiles = first < ntiles ? (ntiles - 1 - first) / stride + 1 : 0;
  const int n0t = 2 * item < ntiles ? (ntiles - 1 - 2 * item) / stride + 1 : 0;
  const int n1t = 2 * item + 1 < ntiles ? (ntiles - 2 - 2 * item) / stride + 1 : 0;
  const int nk = a.K >> 5;
  const int S = 2 * nk + E;
  const int OFF = (S >> 1) | 1;  // odd: the groups' load / compute roles alternate
  const int total = max(n0t * S, n1t > 0 ? OFF + n1t * S : 0);
  if (total == 0) return;

  const uint8_t* Ab = reinterpret_cast<const uint8_t*>(a.A);
  const uint8_t* Bb = reinterpret_cast<const uint8_t*>(a.B);
  const int64_t lda_b = 2 * a.lda, ldb_b = 2 * a.ldb;
  // DMA piece = 16 rows x 64 B: lane -> row lane >> 2, 16-B chunk (lane & 3) ^ swizzle
  const int psw = ((lane >> 5) & 1) << 1;
  const uint32_t offA = (uint32_t)((lane >> 2) * lda_b + (((lane & 3) ^ psw) << 4));
  const uint32_t offB = (uint32_t)((lane >> 2) * ldb_b + (((lane & 3) ^ psw) << 4));
  auto tile_desc = [&](int tile, rsrc_t& ra, rsrc_t& rb, int& m0, int& n0) {
    if (tile < ntiles) {
      int tm, tn;
      tile_mn(tile, tiles_n, ntiles, tm, tn);
      m0 = tm * 256;
      n0 = tn * 128;
      ra = make_rsrc(Ab + (int64_t)m0 * lda_b, (int64_t)(a.M - m0 - 1) * lda_b + 2 * a.K);
      rb = make_rsrc(Bb + (int64_t)n0 * ldb_b, (int64_t)(a.N - n0 - 1) * ldb_b + 2 * a.K);
    } else {
      ra = rb = make_rsrc(Ab, 0);
      m0 = n0 = 0;
    }
  };
  // k-step kk (of the tile whose A / B descriptors are given) into ring slot `slot`: 24 pieces,
  // wave w issues pieces w, w + 4, .., w + 20 (A pieces 0-15, B pieces 16-23)
  auto stage = [&](const rsrc_t& ra, const rsrc_t& rb, int kk, int slot) {
    unsigned short* st = ring + slot * PP_STAGE;
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      const int pc = w + 4 * e;
      if (pc < 16)
        dma16(ra, st + pc * 512, offA + (uint32_t)(pc * 16 * lda_b + kk * 64));
      else
        dma16(rb, st + 256 * 32 + (pc - 16) * 512, offB + (uint32_t)((pc - 16) * 16 * ldb_b + kk * 64));
    }
  };
  // fragment offsets (elements within a slot), as gemm_nt_2b_kernel
  const int l15 = lane & 15, g = lane >> 4, ii = lane & 15;
  const int hA = ((l15 >> 3) & 1) << 1;
  const int aoff = (wr * 128 + l15) * 32 + ((g ^ hA) << 3);
  const int rB = 8 * (l15 >> 2) + (l15 & 3);
  const int hB = ((rB >> 3) & 1) << 1;
  const int boff = 256 * 32 + (wc * 64 + rB) * 32 + ((g ^ hB) << 3);

  int tile = first;
  rsrc_t rAc, rBc, rAn, rBn;
  int m0, n0, m0n, n0n;
  tile_desc(tile, rAc, rBc, m0, n0);
  tile_desc(tile + stride, rAn, rBn, m0n, n0n);
  // prologue: k-steps 0 and 1 of the group's first tile (zero-size loads if it has none)
  stage(rAc, rBc, 0, 0);
  stage(rAc, rBc, 1, 1);
  vm_wait<6>();
  __builtin_amdgcn_s_barrier();
  int t = 0;  // intervals of this group's program done
  if (grp) {
    for (; t < OFF; ++t) __builtin_amdgcn_s_barrier();
  }
  const rsrc_t rBias = make_rsrc(a.bias, a.bias ? (int64_t)a.N * 4 : 0);
  f32x4 acc[8][4];
  bf16x8_t fa[8], fb[4];
  for (int it = 0; it < my_tiles; ++it) {
    float* sbias = reinterpret_cast<float*>(smem + 2 * 3 * PP_STAGE + (grp * 2 + (it & 1)) * 256);
    if (ACT >= 0 && w == 0 && lane < 32)  // the tile's 128 bias values (read in its epilogue)
      dma16(rBias, reinterpret_cast<unsigned short*>(sbias), (uint32_t)(n0 * 4) + (uint32_t)lane * 16u);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int base = (int)(((int64_t)it * nk) % 3);  // ring slot of the tile's k-step 0
    for (int k = 0; k < nk; ++k) {
      // ---- load(k): fragments of k-step k, DMA of k-step k + 2 (the next tile's 0 / 1 at the end)
      const unsigned short* st = ring + ((base + k) % 3) * PP_STAGE;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        fa[i] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8*>(st + aoff + i * 16 * 32));
#pragma unroll
      for (int j = 0; j < 4; ++j)
        fb[j] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8*>(
                                                 st + boff + (4 * (j & 1) + 32 * (j >> 1)) * 32));
      if (k + 2 < nk) stage(rAc, rBc, k + 2, (base + k + 2) % 3);
      else stage(rAn, rBn, k + 2 - nk, (base + k + 2) % 3);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      // ---- compute(k)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      // k-step k + 1 landed (its DMA is older than k + 2's; for k + 1 == 1 also older than the
      // previous tile's epilogue operations and this tile's bias DMA)
      if (k + 1 < nk) {
        if (k == 0 && it > 0) vm_wait<6 + EPO>();
        else vm_wait<6>();
      }
      __builtin_amdgcn_s_barrier();
    }
    t += 2 * nk;
    // ---- epilogue: E intervals of CPI calls each, beside the other group's main loop
    if (ACT >= 0) {
      const float* sbr = sbias;  // written by wave 0's DMA, retired by the k = 1 wait + barrier
      const int64_t rows_left = (int64_t)a.M - m0;
      const rsrc_t rC = make_rsrc(reinterpret_cast<const uint8_t*>(a.C) + (int64_t)m0 * a.ldc * 2,
                                  (rows_left - 1) * a.ldc * 2 + (int64_t)a.N * 2);
      const rsrc_t rX = make_rsrc(AUX ? reinterpret_cast<const uint8_t*>(a.aux) + (int64_t)m0 * a.ldc * 2 : nullptr,
                                  AUX ? (rows_left - 1) * a.ldc * 2 + (int64_t)a.N * 2 : 0);
      const bool resid = XIN && !BWD && a.resid != nullptr;
      const int64_t ldi = BWD ? a.ldc : (resid ? a.ldr : a.ldc);  // operand row stride
      const uint8_t* ibase = BWD ? reinterpret_cast<const uint8_t*>(a.dact)
                                 : (resid ? reinterpret_cast<const uint8_t*>(a.resid)
                                          : reinterpret_cast<const uint8_t*>(a.C));
      const rsrc_t rI = make_rsrc(XIN ? ibase + (int64_t)m0 * ldi * 2 : nullptr,
                                  XIN ? (rows_left - 1) * ldi * 2 + (int64_t)a.N * 2 : 0);
      auto call_off = [&](int call, int64_t ld) -> uint32_t {
        const int i = call >> 1, tt = call & 1;
        const int r = wr * 128 + i * 16 + ii;
        const int n = n0 + wc * 64 + 32 * tt + 8 * g;
        return n < a.N ? (uint32_t)(((int64_t)r * ld + n) * 2) : 0x80000000u;
      };
      typedef __attribute__((ext_vector_type(4))) int i32x4_t;
      i32x4_t in[2][CPI > 0 ? CPI : 1];
      if (NL) {  // batch 0's operands (older than nothing we wait for before consuming them)
#pragma unroll
        for (int q = 0; q < CPI; ++q)
          in[0][q] = __builtin_amdgcn_raw_buffer_load_b128(rI, call_off(q, ldi), 0, 0);
      }
#pragma unroll
      for (int c = 0; c < E; ++c) {
        if (NL && c + 1 < E) {
#pragma unroll
          for (int q = 0; q < CPI; ++q)
            in[(c + 1) & 1][q] = __builtin_amdgcn_raw_buffer_load_b128(rI, call_off((c + 1) * CPI + q, ldi), 0, 0);
        }
        if (NL) {  // batch c's operands: younger ops = batch c + 1's loads + batch c - 1's stores
          if (c == 0) vm_wait<(E > 1 ? NL * CPI : 0)>();
          else if (c + 1 < E) vm_wait<NL * CPI + NS * CPI>();
          else vm_wait<NS * CPI>();
          asm volatile("" ::"v"(in[c & 1][0]));
        }
#pragma unroll
        for (int q = 0; q < CPI; ++q) {
          const int call = c * CPI + q;
          const int i = call >> 1, tt = call & 1;
          const f32x4 lo = acc[i][2 * tt], hi = acc[i][2 * tt + 1];
          const int cn = wc * 64 + 32 * tt + 8 * g;  // column within the tile
          const f32x4 b0 = *reinterpret_cast<const f32x4*>(sbr + cn);
          const f32x4 b1 = *reinterpret_cast<const f32x4*>(sbr + cn + 4);
          float v[8];
          bias_alpha8(v, lo, hi, a.alpha, b0, b1);
          u16x8 xin = (u16x8){0, 0, 0, 0, 0, 0, 0, 0};
          if (NL) xin = __builtin_bit_cast(u16x8, in[c & 1][q]);
          if (BWD) {
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] *= dtab[dtab_index(xin[r])];
          } else if (ACT) {
            if (AUX) {
              u16x8 z;
#pragma unroll
              for (int r = 0; r < 8; ++r) z[r] = f2bf(v[r]);
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4_t, z), rX, call_off(call, a.ldc), 0, 0);
            }
            if (ACT == MMSEQ_ACT_GELU_ERF) {
              gelu_sig8(v);
            } else {
#pragma unroll
              for (int r = 0; r < 8; ++r) v[r] = act_fwd_fast(ACT, v[r]);
            }
          }
          if (!BWD && a.drop.thr) {
            const int m = m0 + wr * 128 + i * 16 + ii;
            float dm[8];
            drop_mul_pairs<4>(a.drop, (uint64_t)m * a.N + (n0 + cn), dm);
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] *= dm[r];
          }
          if (XIN && !BWD) {
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] += bf2f(xin[r]);
          }
          u16x8 o;
#pragma unroll
          for (int r = 0; r < 8; ++r) o[r] = f2bf(v[r]);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4_t, o), rC, call_off(call, a.ldc), 0, 0);
        }
        // last interval: the next tile's k-step 0 landed (its DMA precedes k-step 1's and every
        // epilogue operation)
        if (c == E - 1) vm_wait<6 + EPO>();
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(acc[i][j]));
      for (int c = 0; c < E; ++c) {
        if (c == E - 1) vm_wait<6>();
        __builtin_amdgcn_s_barrier();
      }
    }
    t += E;
    tile += stride;
    rAc = rAn;
    rBc = rBn;
    m0 = m0n;
    n0 = n0n;
    tile_desc(tile + stride, rAn, rBn, m0n, n0n);
  }
  for (; t < total; ++t) __builtin_amdgcn_s_barrier();  // both groups pass 1 + total barriers
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA may outlive the workgroup
}

}  // namespace

// The host entry points below map (act, bwd, xin, aux, q8) to a kernel instantiation in one form:
// a one-line launch macro for the kernel at hand, a ladder over the epilogue flags that is the same
// for both activations (the *_ROW macro), and a switch over the activation (0, GELU, QuickGELU:
// checked before) whose case 0 spells out its own, shorter ladder. Only the combinations listed
// are instantiated.
bool mmseq_gemm256_nt(const GemmArgs& a, bool out_bf16, int num_cu, hipStream_t s, hipError_t* err,
                      int variant, int delay) {
  auto a16 = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
  if (!out_bf16 || a.K % 128 != 0 || a.splitk != 1 || a.N % 8 != 0 || a.ldc % 8 != 0 ||
      (a.accumulate && (a.resid || a.dact)) || (a.dact && a.drop.thr) ||
      (a.resid && (a.ldr % 8 != 0 || !a16(a.resid))) || !a16(a.C) || (a.aux && !a16(a.aux)) ||
      (a.dact && !a16(a.dact)))
    return false;
  if (a.act != 0 && a.act != MMSEQ_ACT_GELU_ERF && a.act != MMSEQ_ACT_QUICKGELU) return false;
  const bool bwd = a.dact != nullptr;
  const bool xin = bwd || a.resid || a.accumulate;
  const bool noepi = a.act == 0 && a.alpha == -12345.0f;  // benchmark hook (tools/gemm_epi_bench.py)
#define NT_ROW(L, ACT_)                \
  if (bwd) L(ACT_, true, true);        \
  else if (xin) L(ACT_, false, true);  \
  else L(ACT_, false, false)
#define NT_LADDER(L)                                       \
  switch (a.act) {                                         \
    case 0:                                                \
      if (noepi) L(-1, false, false);                      \
      else if (xin) L(0, false, true);                     \
      else L(0, false, false);                             \
      break;                                               \
    case MMSEQ_ACT_GELU_ERF: NT_ROW(L, MMSEQ_ACT_GELU_ERF); break; \
    default: NT_ROW(L, MMSEQ_ACT_QUICKGELU);               \
  }
  if (variant == 2) {  // ping-pong: two 4-wave groups of 256 x 128 tiles per 512-thread block
    const int tn = (a.N + 127) / 128;
    const int ntiles = ((a.M + 255) / 256) * tn;
    const int grid = (ntiles + 1) / 2 < num_cu ? (ntiles + 1) / 2 : num_cu;
    const bool aux = a.aux != nullptr;
#define PP(ACT_, BWD_, XIN_, AUX_) \
    hipLaunchKernelGGL((gemm_pp_kernel<ACT_, BWD_, XIN_, AUX_>), dim3(grid), dim3(512), 0, s, a, tn, ntiles, 0)
#define PP_ROW(ACT_)                                   \
    if (bwd) PP(ACT_, true, true, false);              \
    else if (xin && aux) PP(ACT_, false, true, true);  \
    else if (xin) PP(ACT_, false, true, false);        \
    else if (aux) PP(ACT_, false, false, true);        \
    else PP(ACT_, false, false, false)
    switch (a.act) {
      case 0:
        if (noepi) PP(-1, false, false, false);
        else if (xin) PP(0, false, true, false);
        else PP(0, false, false, false);
        break;
      case MMSEQ_ACT_GELU_ERF: PP_ROW(MMSEQ_ACT_GELU_ERF); break;
      default: PP_ROW(MMSEQ_ACT_QUICKGELU);
    }
#undef PP_ROW
#undef PP
  } else if (variant == 1 && a.K % 32 == 0) {  // two 256 x 128 blocks per CU
    const int tn = (a.N + 127) / 128;
    const int ntiles = ((a.M + 255) / 256) * tn;
    const int grid = ntiles < 2 * num_cu ? ntiles : 2 * num_cu;
#define NT2B(ACT_, BWD_, XIN_) \
    hipLaunchKernelGGL((gemm_nt_2b_kernel<ACT_, BWD_, XIN_>), dim3(grid), dim3(256), 0, s, a, tn, ntiles, delay)
    NT_LADDER(NT2B)
#undef NT2B
  } else {
    const int tn = (a.N + 255) / 256;
    const int ntiles = ((a.M + 255) / 256) * tn;
    const int grid = ntiles < num_cu ? ntiles : num_cu;
#define NT8(ACT_, BWD_, XIN_) \
    hipLaunchKernelGGL((gemm256_nt_kernel<ACT_, BWD_, XIN_>), dim3(grid), dim3(512), 0, s, a, tn, ntiles, delay)
    NT_LADDER(NT8)
#undef NT8
  }
#undef NT_LADDER
#undef NT_ROW
  *err = hipGetLastError();
  return true;
}

bool mmseq_gemm256_tn(const GemmArgs& a, hipStream_t s, hipError_t* err) {
  auto a16 = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
  if (a.M % 8 != 0 || a.N % 8 != 0 || a.lda % 8 != 0 || a.ldb % 8 != 0 || !a16(a.A) || !a16(a.B) ||
      (a.splitk > 1 && a.kchunk % 128 != 0) || (a.splitk == 1 && (a.ldc % 4 != 0 || !a16(a.C))))
    return false;
  const int tn = (a.N + 255) / 256;
  const int ntiles = ((a.M + 255) / 256) * tn;
  if (a.cs)
    hipLaunchKernelGGL(gemm256_tn_kernel<true>, dim3(ntiles * a.splitk), dim3(512), 0, s, a, tn, ntiles);
  else
    hipLaunchKernelGGL(gemm256_tn_kernel<false>, dim3(ntiles * a.splitk), dim3(512), 0, s, a, tn, ntiles);
  *err = hipGetLastError();
  return true;
}

bool mmseq_gemm256_nt_q8(const GemmArgs& a, int num_cu, hipStream_t s, hipError_t* err) {
  auto a16 = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
  if (a.K % 128 != 0 || a.N % 32 != 0 || a.ldc % 16 != 0 || a.splitk != 1 || !a.q8_scales ||
      !a16(a.C) || a.resid || a.aux || a.dact || a.accumulate || a.drop.thr)
    return false;
  if (a.act != 0 && a.act != MMSEQ_ACT_GELU_ERF && a.act != MMSEQ_ACT_QUICKGELU) return false;
  const int tn = (a.N + 255) / 256;
  const int ntiles = ((a.M + 255) / 256) * tn;
  const dim3 grid(ntiles < num_cu ? ntiles : num_cu), block(512);
#define NT_Q8(ACT_) \
  hipLaunchKernelGGL((gemm256_nt_kernel<ACT_, false, false, true>), grid, block, 0, s, a, tn, ntiles, 0)
  switch (a.act) {
    case 0: NT_Q8(0); break;
    case MMSEQ_ACT_GELU_ERF: NT_Q8(MMSEQ_ACT_GELU_ERF); break;
    default: NT_Q8(MMSEQ_ACT_QUICKGELU);
  }
#undef NT_Q8
  *err = hipGetLastError();
  return true;
}

// MX-fp8 operands (F8) on the 256 x 256 schedule: A e4m3 [M][lda], B e4m3 [N][ldb] + packed scales
// (fp8.hip); bf16 out (bias, GELU / QuickGELU, residual) or, with a.q8_scales, MX-fp8 out.
bool mmseq_gemm256_nt_f8(const GemmArgs& a, int num_cu, hipStream_t s, hipError_t* err) {
  auto a16 = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
  const bool q8 = a.q8_scales != nullptr;
  if (a.K % 256 != 0 || a.splitk != 1 || a.lda % 16 != 0 || a.ldb % 16 != 0 || !a16(a.A) ||
      !a16(a.B) || !a.f8_sa || !a.f8_sb || a.accumulate || !a16(a.C))
    return false;
  if (a.aux && (!a16(a.aux) || !a.act)) return false;
  // dgrad form: C = (A B^T) * act'(dact) (the activation derivative at the stored pre-activation);
  // with q8_scales the MX-fp8 output (+ its bf16 copy cbf), dact then in cbf's layout (ldcb)
  if (a.dact && (!a.act || a.resid || a.aux || a.bias || a.drop.thr || !a16(a.dact))) return false;
  // MX-fp8 out: no residual / dropout; its optional bf16 copy and aux share ldcb. bf16 out: the
  // plain epilogue (bias, activation + aux, dropout, residual)
  if (q8 ? (a.N % 32 != 0 || a.ldc % 16 != 0 || a.resid || a.drop.thr ||
            ((a.cbf || a.aux) && (a.ldcb % 8 != 0 || (a.cbf && !a16(a.cbf)))))
         : (a.N % 8 != 0 || a.ldc % 8 != 0 || a.cbf || (a.aux && a.ldc % 8 != 0) ||
            (a.resid && (a.ldr % 8 != 0 || !a16(a.resid)))))
    return false;
  if (a.act != 0 && a.act != MMSEQ_ACT_GELU_ERF && a.act != MMSEQ_ACT_QUICKGELU) return false;
  const int tn = (a.N + 255) / 256;
  const int ntiles = ((a.M + 255) / 256) * tn;
  const dim3 grid(ntiles < num_cu ? ntiles : num_cu), block(512);
#define F8_LAUNCH(ACT_, BWD_, XIN_, Q8_) \
  hipLaunchKernelGGL((gemm256_nt_kernel<ACT_, BWD_, XIN_, Q8_, true>), grid, block, 0, s, a, tn, ntiles, 0)
  const bool bwd = a.dact != nullptr, xin = a.resid != nullptr;  // bwd: act != 0 (checked above)
#define F8_ROW(ACT_)                                      \
  if (bwd && q8) F8_LAUNCH(ACT_, true, true, true);       \
  else if (bwd) F8_LAUNCH(ACT_, true, true, false);       \
  else if (q8) F8_LAUNCH(ACT_, false, false, true);       \
  else if (xin) F8_LAUNCH(ACT_, false, true, false);      \
  else F8_LAUNCH(ACT_, false, false, false)
  switch (a.act) {
    case 0:
      if (q8) F8_LAUNCH(0, false, false, true);
      else if (xin) F8_LAUNCH(0, false, true, false);
      else F8_LAUNCH(0, false, false, false);
      break;
    case MMSEQ_ACT_GELU_ERF: F8_ROW(MMSEQ_ACT_GELU_ERF); break;
    default: F8_ROW(MMSEQ_ACT_QUICKGELU);
  }
#undef F8_ROW
#undef F8_LAUNCH
  *err = hipGetLastError();
  return true;
}
