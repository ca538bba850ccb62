/*
 * mmseq — MI355X-native (gfx950 / CDNA4) kernels for the multimodal sequence-ordering hot path
 * of telin0411/multimodal_sequencing (CLIP-ViT -> VisualBERT-style LXRT encoder -> BERSON).
 *
 * C ABI: plain pointers and sizes, no torch types. Every entry point is stream-ordered on the
 * caller's hipStream_t, performs no host synchronisation and no allocation: the caller owns all
 * input, output and workspace buffers. Functions are stateless and reentrant: kernel selection
 * and scratch space are per-call arguments; the only process-wide state is a write-once,
 * per-device table of CU counts. Calls on different streams are independent as long as they do
 * not share output or workspace buffers. On failure they return a negative mmseq_status and
 * mmseq_last_error() describes it (thread-local).
 *
 * The reference has NO native layer: it is 100 % PyTorch, so each entry point
 * below replaces a group of PyTorch ops at the reference site cited next to it. The Python
 * binding that a maintainer adds on the reference side is shown in INTEGRATION.md.
 *
 * Dtypes: MMSEQ_F32 (exact fp32 "parity mode": fp32 MFMA v_mfma_f32_16x16x4_f32) and
 * MMSEQ_BF16 (perf mode: bf16 operands, fp32 accumulate, v_mfma_f32_16x16x32_bf16).
 */
#ifndef MMSEQ_H
#define MMSEQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* mmseq_stream;  /* == hipStream_t; NULL = default stream */
typedef int mmseq_status;
enum { MMSEQ_OK = 0, MMSEQ_EINVAL = -1, MMSEQ_EUNSUPPORTED = -2, MMSEQ_EHIP = -3 };
typedef enum { MMSEQ_F32 = 0, MMSEQ_BF16 = 1 } mmseq_dtype;

/* Activations fused into GEMM epilogues / elementwise kernels:
 *   GELU_ERF   lxrt/modeling.py:116-122 (BertIntermediate)
 *   QUICKGELU  clip/model.py:199-201     (ViT MLP)
 *   TANH       berson/modeling_bert.py:699 (HierarchicalAttention.sentence_tran)
 *   GELU_TANH  berson/neural.py:7-8      (PositionwiseFeedForward) */
typedef enum {
  MMSEQ_ACT_NONE = 0, MMSEQ_ACT_GELU_ERF = 1, MMSEQ_ACT_QUICKGELU = 2, MMSEQ_ACT_TANH = 3,
  MMSEQ_ACT_GELU_TANH = 4
} mmseq_act;

/* Dropout (train mode). Counter-based, one 32-bit hash per element QUAD q = idx >> 2:
 *   key        = splitmix64(seed ^ splitmix64(0x5bd1e995 + stream)); k0 = low word, k1 = high | 1
 *   h          = lowbias32(((uint32_t)q ^ k0) + ((uint32_t)(q >> 32) ^ k1))
 *   m          = h * 0x9E3779B1 (mod 2^32);  h2 = m ^ (m >> 16)
 *   elements 4q, 4q+1 use the low / high 16-bit half of h, elements 4q+2, 4q+3 those of h2;
 *   an element is dropped iff its half < round(p * 2^16) (at least 1).
 * Kept values are scaled by 1/(1-p). The same (seed, stream) regenerates the mask in the backward,
 * so no mask is ever stored (csrc/common.h drop_hash / drop_hash2 / drop_sel are the definition).
 * A NULL pointer or p == 0 means no dropout. */
typedef struct {
  float p;
  uint32_t stream;
  uint64_t seed;
} mmseq_dropout;

const char* mmseq_last_error(void);
const char* mmseq_version(void);

/* ------------------------------------------------------------------------------------------
 * GEMM (replaces every nn.Linear / matmul on the path: lxrt/modeling.py:385-395,437,473,491,
 * 576; clip/model.py:208-214,263,304; berson/modeling_bert.py:697-701,745,882-902; neural.py).
 *
 *   C[b][m][n] = epilogue( alpha * sum_k A(m,k) * B(k,n) )        b < batch
 *   layout "NT" (trans=0): A(m,k) = A[m*lda + k],  B(k,n) = B[n*ldb + k]   (both K-contiguous)
 *   layout "TN" (trans=1): A(m,k) = A[k*lda + m],  B(k,n) = B[k*ldb + n]   (both M/N-contiguous)
 *   epilogue, in order:  v += bias[n] (f32, optional)
 *                        if dact_aux: v *= act'(dact_aux[m][n])          (backward through act)
 *                        else if act: aux_out[m][n] = v (optional); v = act(v)
 *                        v = dropout(v) (optional, idx = (b*M + m)*N + n)
 *                        v += resid[m][n] (optional)   ;   if accumulate: v += C[m][n]
 *   A, B share in_dtype; C, resid, aux_out, dact_aux share out_dtype (aux ld = ldc).
 *   variant: kernel selection for THIS call (tests and microbenchmarks cover every variant):
 *     MMSEQ_GEMM_AUTO (default: 256 x 256 persistent NT/TN kernels for large problems,
 *     128 x 128 double-buffer otherwise), MMSEQ_GEMM_DB128 (128 x 128 double-buffer only),
 *     MMSEQ_GEMM_RING128 (128 x 128 four-slot ring only), MMSEQ_GEMM_BIG_ALWAYS (256 x 256
 *     NT for every eligible NT problem), MMSEQ_GEMM_BIG_256x128 (256 x 128 NT, two blocks/CU),
 *     MMSEQ_GEMM_PINGPONG (bf16 NT: two independent 4-wave groups per CU on 256 x 128 tiles, one
 *     group's epilogue beside the other's main loop), MMSEQ_GEMM_GENERIC (register-staged only).
 *   workspace: caller-owned, 16-byte aligned device scratch for fp32 split-K partial slabs of
 *     this call (NULL / 0 bytes = no split-K). Wgrad-shaped problems (few output tiles, long
 *     K) split K across workgroups and reduce the slabs in a fixed order (bitwise reproducible).
 *     It is only touched by work enqueued on `stream`, so concurrent calls on different
 *     streams need different workspaces; mmseq_gemm_workspace_size() bounds what helps.
 * ------------------------------------------------------------------------------------------ */
typedef enum {
  MMSEQ_GEMM_GENERIC = 0, MMSEQ_GEMM_AUTO = 1, MMSEQ_GEMM_DB128 = 2, MMSEQ_GEMM_RING128 = 3,
  MMSEQ_GEMM_BIG_ALWAYS = 4, MMSEQ_GEMM_BIG_256x128 = 5, MMSEQ_GEMM_PINGPONG = 6
} mmseq_gemm_variant;

mmseq_status mmseq_gemm(int trans, int M, int N, int K, int batch,
                        const void* A, int64_t lda, int64_t strideA,
                        const void* B, int64_t ldb, int64_t strideB,
                        void* C, int64_t ldc, int64_t strideC,
                        const float* bias, int act, void* aux_out, const void* dact_aux,
                        const void* resid, int64_t ldr, int64_t strideR,
                        float alpha, int accumulate, mmseq_dtype in_dtype, mmseq_dtype out_dtype,
                        const mmseq_dropout* drop, int variant, void* workspace,
                        int64_t workspace_bytes, mmseq_stream stream);
/* Bytes of workspace beyond which mmseq_gemm / mmseq_gemm_wgrad change nothing for an M x N x K
 * problem on the current device: the largest amount any of their split-K plans uses when nothing
 * limits it, the wgrad's bias partial rows included (so also nonzero for a wgrad too short to
 * split). A call given this much runs exactly as with any larger workspace; a call given less
 * takes fewer splits or sums the bias gradient without partial rows. */
int64_t mmseq_gemm_workspace_size(int M, int N, int K);
/* Weight + bias gradient of a Linear in one pass (replaces the wgrad GEMM and the bias column sum
 * of every nn.Linear backward on the path): C[M][N] += sum_k A[k][m] B[k][n] (A = dY [K][lda],
 * B = X [K][ldb], fp32 C) and, if bias_grad != NULL, bias_grad[m] += sum_k A[k][m] (fp32).
 * Deterministic (fixed-order split-K reductions). variant / workspace as for mmseq_gemm. */
mmseq_status mmseq_gemm_wgrad(int M, int N, int K, const void* A, int64_t lda, const void* B,
                              int64_t ldb, float* C, int64_t ldc, float* bias_grad,
                              mmseq_dtype in_dtype, int variant, void* workspace,
                              int64_t workspace_bytes, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Fused multi-head attention over a packed QKV activation (lxrt/modeling.py:398-425 with the
 * additive key mask of :1537-1545 / :1071-1094; clip/model.py:219-221 nn.MultiheadAttention).
 *   token t of sequence p has row  qkv + (p*T + t)*ld_qkv ; head h of Q at +q_off + h*64,
 *   K at +k_off + h*64, V at +v_off + h*64. head_dim is 64.
 *   key_bias: [P][T] f32 additive (0 or -10000), or NULL.  out row: out + (p*T+t)*ld_out + h*64.
 *   lse: [P][heads][T] f32 (log-sum-exp of the scaled, biased scores), written by fwd.
 * bwd: delta workspace [P][heads][T] f32; dqkv holds dQ | dK | dV at qkv's column offsets with a
 *   row stride of its own: max(q_off, k_off, v_off) + heads*64 <= ld_dqkv, else MMSEQ_EINVAL.
 * drop: attention-probability dropout (lxrt:421), idx = ((p*heads + h)*T + q)*Tp4 + k with the
 *   row stride Tp4 = T rounded up to a multiple of 4 (a lane's four keys 4g..4g+3 form one quad).
 * variant (per call, bf16 only): 1 = 128-row workgroups with LDS-DMA double-buffered K/V (or
 * Q/dO) tiles and the delta = rowsum(dO * O) reduction fused into the dQ kernel; 0 = 64-row
 * register-staged kernels (cross-check in the tests). fp32 always uses the latter.
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_attn_fwd(int P, int T, int heads, const void* qkv, int64_t ld_qkv,
                            int64_t q_off, int64_t k_off, int64_t v_off, const float* key_bias,
                            float scale, void* out, int64_t ld_out, float* lse,
                            mmseq_dtype dtype, const mmseq_dropout* drop, uint64_t* keep_bits,
                            int variant, mmseq_stream stream);
/* attn_fwd_mxfp8: the bf16 fast forward without dropout (eval) whose output O [P*T][heads*64] is
 *  written in MX-fp8 (mmseq_quant_mxfp8 layout, bit-identical to quantising the bf16 output; the
 *  scales of the rows past P*T up to the next multiple of 64 are left to the caller) for the output
 *  projection's fp8 GEMM (BASELINE config 5; lxrt/modeling.py:398-425, clip/model.py:219-221). */
mmseq_status mmseq_attn_fwd_mxfp8(int P, int T, int heads, const void* qkv, int64_t ld_qkv,
                                  int64_t q_off, int64_t k_off, int64_t v_off,
                                  const float* key_bias, float scale, float* lse, void* q8,
                                  int64_t ldq8, void* q8_scales, mmseq_stream stream);
/* attn_fwd_mxfp8_dual: the same forward for a TRAINING step with the fp8 forward GEMMs (config 5):
 *  the bf16 output O (for the backward; NULL: MX-fp8 only) and its MX-fp8 copy (the output
 *  projection's operand) from one epilogue, with attention-probability dropout and keep bits as in
 *  mmseq_attn_fwd (identical masks, O bit-identical to mmseq_attn_fwd variant 1). */
mmseq_status mmseq_attn_fwd_mxfp8_dual(int P, int T, int heads, const void* qkv, int64_t ld_qkv,
                                       int64_t q_off, int64_t k_off, int64_t v_off,
                                       const float* key_bias, float scale, void* out,
                                       int64_t ld_out, float* lse, const mmseq_dropout* drop,
                                       uint64_t* keep_bits, void* q8, int64_t ldq8,
                                       void* q8_scales, mmseq_stream stream);
mmseq_status mmseq_attn_bwd(int P, int T, int heads, const void* qkv, int64_t ld_qkv,
                            int64_t q_off, int64_t k_off, int64_t v_off, const float* key_bias,
                            float scale, const void* out, int64_t ld_out, const void* dout,
                            int64_t ld_dout, const float* lse, float* delta, void* dqkv,
                            int64_t ld_dqkv, mmseq_dtype dtype, const mmseq_dropout* drop,
                            const uint64_t* keep_bits, int variant, mmseq_stream stream);
/* attn_fwd_rows / attn_bwd_rows: the bf16 fast kernels (variant 1) for the queries 0 .. Tq-1 of
 *  every sequence against all T keys (1 <= Tq <= T): the last joint layer of the BERSON encoder,
 *  whose visual rows' outputs _split_with_none discards (lxrt/modeling.py:611-618,
 *  berson/modeling_bert.py:1289-1290). out / dout hold Tq rows per sequence (row p*Tq + t); lse,
 *  delta and keep_bits keep the [P][heads][T] layout (rows < Tq written; the dropout index is
 *  mmseq_attn_fwd's); dqkv is the full [P*T] layout with dQ = 0 on rows >= Tq (dK / dV over every
 *  key row). Rows < Tq are bit-identical to mmseq_attn_fwd / _bwd with the other rows' dO = 0. */
mmseq_status mmseq_attn_fwd_rows(int P, int T, int Tq, int heads, const void* qkv, int64_t ld_qkv,
                                 int64_t q_off, int64_t k_off, int64_t v_off,
                                 const float* key_bias, float scale, void* out, int64_t ld_out,
                                 float* lse, const mmseq_dropout* drop, uint64_t* keep_bits,
                                 mmseq_stream stream);
mmseq_status mmseq_attn_bwd_rows(int P, int T, int Tq, int heads, const void* qkv, int64_t ld_qkv,
                                 int64_t q_off, int64_t k_off, int64_t v_off,
                                 const float* key_bias, float scale, const void* out,
                                 int64_t ld_out, const void* dout, int64_t ld_dout,
                                 const float* lse, float* delta, void* dqkv, int64_t ld_dqkv,
                                 const mmseq_dropout* drop, const uint64_t* keep_bits,
                                 mmseq_stream stream);
/* attn_bwd_mxfp8: the bf16 fast backward (variant 1) over the packed Q|K|V layout (q_off 0, k_off
 *  heads*64, v_off 2*heads*64) that also writes dQ|dK|dV in MX-fp8 (q8 [P*T][ldq8] e4m3 + packed
 *  scales of the [P*T][3*heads*64] operand, bit-identical to quantising dqkv; padding-row scales
 *  zeroed by the caller): the QKV data-gradient GEMM's operand in config 5's fp8 dgrad. */
mmseq_status mmseq_attn_bwd_mxfp8(int P, int T, int heads, const void* qkv, int64_t ld_qkv,
                                  const float* key_bias, float scale, const void* out,
                                  int64_t ld_out, const void* dout, int64_t ld_dout,
                                  const float* lse, float* delta, void* dqkv, int64_t ld_dqkv,
                                  const mmseq_dropout* drop, const uint64_t* keep_bits, void* q8,
                                  int64_t ldq8, void* q8_scales, mmseq_stream stream);
/* Attention-probability dropout keep-mask cache (bf16 fast kernels): with keep_bits != NULL the
 * forward also stores its counter-based keep mask as bits (word [(p*heads + h)*T + q][kt] for key
 * tile kt < round_up_even(ceil(T/64)); key 64*kt + j at bit ((j >> 2) & 3) * 16 + (j >> 4) * 4 +
 * (j & 3)) and the backward, given the same buffer, reads them instead of hashing every
 * (query, key) element again; NULL in both regenerates the mask. Size in uint64 words: */
int64_t mmseq_attn_keep_bits_words(int P, int T, int heads);

/* Small multi-head attention for the BERSON inter-sentence encoder (neural.py:98-235):
 * [B][T][heads*d] separate q/k/v tensors, T <= 64, d <= 128, fp32, key_bias [B][T] or NULL.
 * probs [B][heads][T][T] (before dropout) are saved by fwd for bwd; drop = probability dropout
 * (neural.py:221), idx = ((b*heads + h)*T + i)*T + j. */
mmseq_status mmseq_small_attn_fwd(int B, int T, int heads, int d, const float* q, const float* k,
                                  const float* v, const float* key_bias, float scale, float* out,
                                  float* probs, const mmseq_dropout* drop, mmseq_stream stream);
mmseq_status mmseq_small_attn_bwd(int B, int T, int heads, int d, const float* q, const float* k,
                                  const float* v, const float* probs, const float* dout,
                                  float scale, float* dq, float* dk, float* dv,
                                  const mmseq_dropout* drop, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (cols), fp32 statistics (lxrt BertLayerNorm eps 1e-12:
 * :353,432,486,577; CLIP fp32 LayerNorm eps 1e-5: clip/model.py:190-196; BERSON eps 1e-6).
 * Row r lives at base + (r / rpb)*bstride + (r % rpb)*ld  (two-level strides let the kernels
 * read/write the text or visual half of the joint [P][T][H] buffer in place; rpb = rows
 * per batch).  fwd: y = LN(x), then dropout(y) if drop_y (idx = r*cols + c).
 * bwd: dy is first multiplied by drop_dy's mask (the fwd drop_y), dx = LN'(dy) (+ dres if
 * non-NULL); if dx_drop, it also receives dx * drop_dx's mask (the gradient of a
 * dropout(dense) + residual sum, idx = r*cols + c, same layout as dx). dgamma/dbeta ACCUMULATE
 * (+=) and need a workspace of mmseq_layernorm_bwd_workspace(rows, cols) floats.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int64_t ld;       /* row stride (elements) inside a batch */
  int64_t bstride;  /* batch stride (elements) */
  int64_t rpb;      /* rows per batch */
} mmseq_rows;

mmseq_status mmseq_layernorm_fwd(int rows, int cols, const void* x, mmseq_rows xl,
                                 const float* gamma, const float* beta, float eps, void* y,
                                 mmseq_rows yl, float* mean, float* rstd, mmseq_dtype x_dtype,
                                 mmseq_dtype y_dtype, const mmseq_dropout* drop_y,
                                 mmseq_stream stream);
/* layernorm_bwd_mxfp8: mmseq_layernorm_bwd (bf16, cols 256..1024 in steps of 256) that also writes
 *  the gradient the next data-gradient GEMM reads — dx_drop when given, else dx (with dres) — in
 *  MX-fp8 (mmseq_quant_mxfp8 layout, bit-identical to quantising it; q_scales must be zeroed by the
 *  caller for the padding rows): config 5's fp8 dgrad (lxrt/modeling.py:428-439,488-493). */
mmseq_status mmseq_layernorm_bwd_mxfp8(int rows, int cols, const void* dy, mmseq_rows dyl,
                                       const void* x, mmseq_rows xl, const float* mean,
                                       const float* rstd, const float* gamma, void* dx,
                                       mmseq_rows dxl, const void* dres, mmseq_rows dresl,
                                       float* dgamma, float* dbeta, float* workspace,
                                       const mmseq_dropout* drop_dy, void* dx_drop,
                                       const mmseq_dropout* drop_dx, void* q, int64_t ldq,
                                       void* q_scales, mmseq_stream stream);
/* layernorm_fwd_mxfp8: bf16 LayerNorm (no dropout) that also writes its output in the MX-fp8 format
 *  of mmseq_quant_mxfp8 (q [rows][ldq] e4m3 + packed scales, bit-identical to quantising the bf16
 *  output), the A operand of the next fp8 GEMM (BASELINE config 5: QKV and FC1 after the LNs of
 *  lxrt/modeling.py:431-439,485-493 and clip/model.py:221-225). cols in {256, 512, 768, 1024};
 *  y may be null when the GEMM is its only consumer. */
mmseq_status mmseq_layernorm_fwd_mxfp8(int rows, int cols, const void* x, mmseq_rows xl,
                                       const float* gamma, const float* beta, float eps, void* y,
                                       mmseq_rows yl, float* mean, float* rstd, void* q,
                                       int64_t ldq, void* q_scales, mmseq_stream stream);
int64_t mmseq_layernorm_bwd_workspace(int rows, int cols);
mmseq_status mmseq_layernorm_bwd(int rows, int cols, const void* dy, mmseq_rows dyl,
                                 const void* x, mmseq_rows xl, const float* mean,
                                 const float* rstd, const float* gamma, void* dx, mmseq_rows dxl,
                                 const void* dres, mmseq_rows dresl, float* dgamma, float* dbeta,
                                 float* workspace, mmseq_dtype dtype,
                                 const mmseq_dropout* drop_dy, void* dx_drop,
                                 const mmseq_dropout* drop_dx, mmseq_stream stream);
/* layernorm_bwd_rows: mmseq_layernorm_bwd with the dropout-masked copy dx_drop in its own row layout
 *  (mmseq_layernorm_bwd writes it in dx's): the last joint layer on the text rows only
 *  (mmseq_attn_fwd_rows) writes the residual branch's dx into its rows of the full-size [P*T]
 *  gradient and the dense branch's masked copy compact (BertSelfOutput, lxrt/modeling.py:431-433). */
mmseq_status mmseq_layernorm_bwd_rows(int rows, int cols, const void* dy, mmseq_rows dyl,
                                      const void* x, mmseq_rows xl, const float* mean,
                                      const float* rstd, const float* gamma, void* dx,
                                      mmseq_rows dxl, const void* dres, mmseq_rows dresl,
                                      float* dgamma, float* dbeta, float* workspace,
                                      mmseq_dtype dtype, const mmseq_dropout* drop_dy,
                                      void* dx_drop, mmseq_rows dx_dropl,
                                      const mmseq_dropout* drop_dx, mmseq_stream stream);
/* layernorm_bwd_ex: mmseq_layernorm_bwd_rows (dx_drop optional, in its own layout dx_dropl) that
 *  also ACCUMULATES into dsum[cols] the column sums of the gradient it writes for the next GEMM —
 *  dx_drop when given, else dx (with dres) — as stored (bf16-rounded in bf16): the bias gradient of
 *  the Linear whose output gradient that is (BertSelfOutput / BertOutput dense and the CLIP
 *  attention out_proj, lxrt/modeling.py:431-433,489-493, clip/model.py:219-221), so that its
 *  weight-gradient GEMM runs without the fused bias pass (mmseq_gemm_wgrad with gb = NULL). The
 *  summed gradient must be in dense rows. Summed in a fixed order (bitwise repeatable). Same
 *  workspace as mmseq_layernorm_bwd. dsum = NULL: exactly mmseq_layernorm_bwd(_rows).
 *  NOTE the two summed quantities: with dx_drop the sum is of dx_drop (the LN gradient through the
 *  dropout mask, WITHOUT dres); without dx_drop it is of dx as written, i.e. INCLUDING dres. The
 *  callers rely on exactly that: the BERT post-LN layers pass dres = NULL (the dense Linear's output
 *  gradient is the LN gradient alone), the CLIP out_proj passes dres because its output gradient
 *  is LN gradient + residual gradient (kernels.py asserts the BERT form). */
mmseq_status mmseq_layernorm_bwd_ex(int rows, int cols, const void* dy, mmseq_rows dyl,
                                    const void* x, mmseq_rows xl, const float* mean,
                                    const float* rstd, const float* gamma, void* dx,
                                    mmseq_rows dxl, const void* dres, mmseq_rows dresl,
                                    float* dgamma, float* dbeta, float* workspace,
                                    mmseq_dtype dtype, const mmseq_dropout* drop_dy,
                                    void* dx_drop, mmseq_rows dx_dropl,
                                    const mmseq_dropout* drop_dx, float* dsum, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Fused text embedding + LayerNorm written straight into the joint buffer (BertEmbeddings,
 * lxrt/modeling.py:356-370; joint concat :1093): for pair p, token t < Lt:
 *   e = word[ids] + pos[t] + type[tt];  joint row (p*ld_pair + t) = LN(e)   (eps as given)
 * bwd recomputes e, applies LN backward and scatters into dword/dpos/dtype (+=), skipping
 * row 0 of every table (padding_idx = 0 on all three, :347-349). dgamma/dbeta accumulate. Every
 * table row's sum runs in a fixed order (rows grouped by id with a radix sort, summed in row
 * order; no float atomics), so the backward is bit-stable run to run. ids (and tt) must lie in
 * [0, rows of their table) and below 2^32 - 1 (not checked on the device: an id outside that
 * range is a caller error); P * Lt < 2^32 - 1; dword and dtype_tab 16-byte aligned (checked).
 * drop: embedding dropout (:369) on the LN output, idx = (p*Lt + t)*H + c.
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_embed_ln_fwd(int P, int Lt, int H, const int64_t* ids, const int64_t* tt,
                                const float* word, const float* pos, const float* type,
                                const float* gamma, const float* beta, float eps, void* joint,
                                int64_t ld_pair, float* mean, float* rstd, mmseq_dtype dtype,
                                const mmseq_dropout* drop, mmseq_stream stream);
mmseq_status mmseq_embed_ln_bwd(int P, int Lt, int H, const int64_t* ids, const int64_t* tt,
                                const float* word, const float* pos, const float* type,
                                const float* gamma, const float* mean, const float* rstd,
                                const void* djoint, int64_t ld_pair, float* dword, float* dpos,
                                float* dtype_tab, float* dgamma, float* dbeta, float* workspace,
                                mmseq_dtype dtype, const mmseq_dropout* drop, mmseq_stream stream);
int64_t mmseq_embed_ln_bwd_workspace(int P, int Lt, int H);

/* ------------------------------------------------------------------------------------------
 * ViT patch path (clip/model.py:262-278 with the img_len=2 quirk).
 *  im2col: images [B][N][3][R][R] f32 + pairs [B][npair][2] -> patches [B*npair][2*g*g] rows of
 *          ld_patch >= 3*ps*ps elements, columns past 3*ps*ps zero (K padded for the GEMM, e.g.
 *          588 -> 640 for ViT-L/14) (pair images gathered on device: no 8x duplicated H2D copy,
 *          process_images :82-97)
 *  embed_fwd: x[p][0] = cls + pos[0]; x[p][1+j] = patch_out[p][j] + pos[j < g*g ? 1+j : j-g*g]
 *             y = LN(x) (ln_pre, eps)   (x saved for bwd as dtype)
 *  embed_bwd: dx = LN'(dy); dcls += sum_p dx[p][0]; dpos[r] += sum of its tokens;
 *             dpatch_out[p][j] = dx[p][1+j]
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_vit_im2col(int B, int N, int npair, int R, int ps, const float* images,
                              const int64_t* pairs, void* patches, int64_t ld_patch,
                              mmseq_dtype dtype, mmseq_stream stream);
mmseq_status mmseq_vit_embed_fwd(int P, int ntok, int W, int npatch_img, const void* patch_out,
                                 const float* cls, const float* pos, const float* gamma,
                                 const float* beta, float eps, void* x, void* y, float* mean,
                                 float* rstd, mmseq_dtype dtype, mmseq_stream stream);
mmseq_status mmseq_vit_embed_bwd(int P, int ntok, int W, int npatch_img, const void* dy,
                                 const void* x, const float* mean, const float* rstd,
                                 const float* gamma, void* dpatch_out, float* dcls, float* dpos,
                                 float* dgamma, float* dbeta, float* workspace, mmseq_dtype dtype,
                                 mmseq_stream stream);
int64_t mmseq_vit_embed_bwd_workspace(int P, int ntok, int W);

/* ------------------------------------------------------------------------------------------
 * Elementwise / reduction utilities.
 * ------------------------------------------------------------------------------------------ */
/* dst[i] = (dst_dtype) src[i] (f32 <-> bf16, or copy), n elements */
mmseq_status mmseq_cast(int64_t n, const void* src, mmseq_dtype src_dtype, void* dst,
                        mmseq_dtype dst_dtype, mmseq_stream stream);
/* dst[c][r] = src[r][c] for an f32 [rows][cols] matrix, written as dst_dtype */
mmseq_status mmseq_transpose_cast(int rows, int cols, const float* src, void* dst,
                                  mmseq_dtype dst_dtype, mmseq_stream stream);
/* transpose_cast_batch: n fp32 matrices transposed (and cast) in one launch: desc[5*m ..] = {rows,
 *  cols, src offset, dst offset, first tile} in elements of src / dst, tiles of 64 x 64 numbered
 *  matrix by matrix (first tile of m = sum of ceil(rows/64)*ceil(cols/64) before it), tiles = the
 *  total; desc in device memory. The per-step refresh of a store's transposed dgrad shadows. */
mmseq_status mmseq_transpose_cast_batch(int n, const int64_t* desc, int64_t tiles, const float* src,
                                        void* dst, mmseq_dtype dd, mmseq_stream stream);
/* out[c] (+)= sum_r x[r][c] in f32 (bias gradients); rows at x + r*ldx. */
mmseq_status mmseq_colsum(int rows, int cols, const void* x, int64_t ldx, float* out,
                          int accumulate, float* workspace, mmseq_dtype dtype,
                          mmseq_stream stream);
int64_t mmseq_colsum_workspace(int rows, int cols);
/* y = act(x) and dx = dy * act'(x), n elements, same dtype */
mmseq_status mmseq_act_fwd(int64_t n, int act, const void* x, void* y, mmseq_dtype dtype,
                           mmseq_stream stream);
mmseq_status mmseq_act_bwd(int64_t n, int act, const void* z, const void* dy, void* dz,
                           mmseq_dtype dtype, mmseq_stream stream);
/* y[i] = x[i] * mask(i) (idx = i); also the backward of itself (the BERSON head's nn.Dropout
 * sites: neural.py:31-32, encoder.py:28). y may alias x. */
mmseq_status mmseq_dropout_apply(int64_t n, const void* x, void* y, mmseq_dtype dtype,
                                 const mmseq_dropout* drop, mmseq_stream stream);
/* sum of squares of n f32 values into out[0] (overwrite), two-pass deterministic */
mmseq_status mmseq_sumsq(int64_t n, const float* x, float* out, float* workspace,
                         mmseq_stream stream);
int64_t mmseq_sumsq_workspace(int64_t n);

/* ------------------------------------------------------------------------------------------
 * Fused AdamW over the flat fp32 parameter buffer (transformers 3.4 AdamW as used at
 * trainers/train.py:172-190,353-363: correct_bias=True, decoupled weight decay applied after
 * the Adam update, grads pre-scaled by clip_grad_norm_(max_norm) computed from sumsq).
 *   clip = min(1, max_norm / (sqrt(*sumsq) + 1e-6)) if max_norm > 0 else 1
 *   m = b1*m + (1-b1)*g*clip ; v = b2*v + (1-b2)*(g*clip)^2
 *   p -= lr * (m/(1-b1^t)) / (sqrt(v/(1-b2^t)) + eps) ... (HF form: step = lr*sqrt(1-b2^t)/(1-b1^t))
 *   p -= lr * wd * p   (for elements with decay_mask != 0; decay_mask may be NULL = all decay)
 * Optionally writes the bf16 shadow copy of the updated parameters (shadow may be NULL).
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_adamw(int64_t n, float* p, const float* g, float* m, float* v,
                         const uint8_t* decay_mask, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int step, float max_norm, const float* sumsq,
                         void* shadow_bf16, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * BERSON pointer scoring (modeling_bert.py:1083-1142, the "pointer-score GEMM" epilogue):
 *   e[b][t][j] = sum_h w[h] * tanh(q[b][t][h] + key[b][t][j][h] + okey[b][j][h]) + w_bias[0]
 *   (w_bias is a device pointer, may be NULL)
 *   e = -1e9 where pointed[b][t][j] != 0 or j >= tgt_len[b];  logp = log_softmax_j(e)
 *   nll[b][t] = -logp[b][t][target[b][t]] if t < tgt_len[b] else 0
 * bwd: given dnll[b][t] (upstream grad of each nll) WRITE dq, dkey and ACCUMULATE (+=) dokey, dw,
 * dw_bias, every sum in a fixed order (bit-stable run to run). Shapes: q [B][N][H],
 * key [B][N][N][H], okey [B][N][H] (f32); workspace: mmseq_pointer_bwd_workspace(B, N, H) floats.
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_pointer_fwd(int B, int N, int H, const float* q, const float* key,
                               const float* okey, const float* w, const float* w_bias,
                               const uint8_t* pointed, const int64_t* tgt_len,
                               const int64_t* target, float* logp, float* nll,
                               mmseq_stream stream);
mmseq_status mmseq_pointer_bwd(int B, int N, int H, const float* q, const float* key,
                               const float* okey, const float* w, const float* logp,
                               const uint8_t* pointed, const int64_t* tgt_len, const int64_t* target, const float* dnll,
                               float* dq, float* dkey, float* dokey, float* dw, float* dw_bias,
                               float* workspace, mmseq_stream stream);
int64_t mmseq_pointer_bwd_workspace(int B, int N, int H);

/* ------------------------------------------------------------------------------------------
 * HierarchicalAttention span pooling (modeling_bert.py:703-741) without host loops:
 *   for pair p, span s in {0,1}: mask_s(t) = 1 for t in [1, sep0] (s=0) / [sep0+1, sep1] (s=1)
 *   a[p][s][t] = mask ? score[p][t] : -10000 ; probs = softmax_t(a); mix[p][s] = probs @ top[p]
 *   top rows: top + p*ld_pair + t*H. probs (before dropout) saved [P][2][Lt] f32 for bwd;
 *   drop = probability dropout (:735), idx = (p*2 + s)*Lt + t.
 * bwd: dscore[p][t] = sum_s mask*probs*(dmix.top - sum_t' probs*dmix.top) (written);
 *      dtop[p][t] += probs^T dmix (accumulated in place)
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_span_pool_fwd(int P, int Lt, int H, const void* top, int64_t ld_pair,
                                 const float* score, const int64_t* sep, float* probs,
                                 float* mix, mmseq_dtype dtype, const mmseq_dropout* drop,
                                 mmseq_stream stream);
mmseq_status mmseq_span_pool_bwd(int P, int Lt, int H, const void* top, int64_t ld_pair,
                                 const float* probs, const int64_t* sep, const float* dmix,
                                 float* dscore, void* dtop, mmseq_dtype dtype,
                                 const mmseq_dropout* drop, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * BERSON pair expansion on device (process_inputs_for_berson.py:13-368 prepare_berson_inputs,
 * parse_input_ids :100-110, pairs_generator :246-261, pairwise labels :162-174).
 *  scan:   per story b (input_ids [B][L], labels [B][N]): steps = the k-th <s> (cls_id) .. k-th
 *          </s> (sep_id); starts/lens [B][N]; pair j of pairs_generator(N) = (a, c):
 *          sep_positions[b][j] = (len_a - 1, len_a + len_c - 1), pairwise_labels[b][j] =
 *          rank[a] < rank[c] with rank = stable argsort(labels[b]); status[0] = max over the
 *          batch of len_a + len_c (atomicMax: zero it first), status[1] = number of stories
 *          that do not hold exactly N well-formed steps (the caller raises, as the reference's
 *          parse does).
 *  expand: rows r = b*N(N-1) + j of [Lp] (Lp = status[0]): ids = <step a><step c> then pad_id;
 *          mask = 1 then pad_id (quirk C.7: pads are attended); token type 1 on step c iff
 *          second_type (cls_id != 0), else 0.
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_pair_scan(int B, int L, int N, const int64_t* input_ids, const int64_t* labels,
                             int64_t cls_id, int64_t sep_id, int64_t* starts, int64_t* lens,
                             int64_t* pairwise_labels, int64_t* sep_positions, int32_t* status,
                             mmseq_stream stream);
mmseq_status mmseq_pair_expand(int B, int L, int N, int Lp, const int64_t* input_ids,
                               const int64_t* starts, const int64_t* lens, int64_t pad_id,
                               int second_type, int64_t* out_ids, int64_t* out_mask,
                               int64_t* out_token_type, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Image preprocessing (trainers/multimodal_utils.py:195-208, datasets/img_utils.py:27-56,
 * 135-144: skimage 0.17.2 resize with anti-aliasing + ToTensor + Normalize) for n decoded RGB
 * uint8 HWC images of any sizes, packed in one buffer:
 *   table [n][4] int64 on the device = (pixel byte offset, H, W, workspace float offset), the
 *   workspace offsets a prefix sum of H * 3 * out_w; max_h / max_w bound every H / W;
 *   out [n][3][out_h][out_w] f32 = (resize(img / 255) - mean[c]) / std[c];
 *   mean / stdev: 3 host floats each. Workspace: mmseq_image_resize_workspace(heights) bytes.
 * ------------------------------------------------------------------------------------------ */
int64_t mmseq_image_resize_workspace(int n_images, const int32_t* heights, int out_w);
mmseq_status mmseq_image_resize_normalize(int n_images, const uint8_t* pixels,
                                          const int64_t* table, int max_h, int max_w, int out_h,
                                          int out_w, const float* mean, const float* stdev,
                                          float* workspace, int64_t workspace_bytes, float* out,
                                          mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * LSTM cell of the pointer decoder (modeling_bert.py:1027-1078, nn.LSTM one step, gates i,f,g,o):
 *  fwd: gates = gx[b] (row stride ld_gx, x W_ih^T + b_ih, all steps from ONE GEMM) + gh
 *       (h W_hh^T + b_hh); c_out = f c + i g; h_out = o tanh(c_out); act [B][4H] = (i,f,g,o).
 *  bwd: dh / dc_next (either may be NULL = zero) -> dgates [B][4H] (pre-activation, shared by the
 *       x and h GEMMs' backward) and dc_prev.
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_lstm_cell_fwd(int B, int H, const float* gx, int64_t ld_gx, const float* gh,
                                 const float* c, float* h_out, float* c_out, float* act,
                                 mmseq_stream stream);
mmseq_status mmseq_lstm_cell_bwd(int B, int H, const float* act, const float* c,
                                 const float* c_out, const float* dh, const float* dc_next,
                                 float* dgates, float* dc_prev, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Beam-search ordering of B stories at once (modeling_bert.py:1368-1402 BertForOrdering.step,
 * :1411-1552 beam_search_pointer, generator.py:8-38 Beam), the beam state resident on the device:
 * one call enqueues the whole decode on `stream`; between enqueue and result it neither
 * synchronises with the host nor copies anything to it. fp32 throughout. Per story, T = N:
 *   start    one candidate [] with score 0, (h, c) = (h0, c0), x = 0, nothing pointed, valid = W
 *   step t   (t = 0 .. T-2) for t >= 1 every live candidate takes x = doc[last] and marks `last`
 *            as pointed; LSTM cell (gates i, f, g, o, both biases); q = query_linear(h')
 *   keys[j]  = pw_k(cat[hist[l1][j], hist[l2][j], forw[j], back[j]]), l1 / l2 the last / second-
 *            to-last pick, their blocks zero while they do not exist (t = 0; t <= 1 for l2);
 *            R[i][j] = hist[i][j] where i != j and neither is pointed, else 0;
 *            forw[i] = sum_j R[i][j] / T, back[j] = sum_i R[i][j] / T
 *   e[j]     = tanh_linear(tanh(q + keys[j] + okey[j])), -1e9 where j is pointed;
 *            logp = log_softmax_j(e)
 *   select   s[w][j] = score[w] - logp[w][j] over the nb live candidates, flat index w*T + j; the
 *            k = min(valid, nb*T) smallest by (s, flat index) are chosen, ties to the lowest flat
 *            index; pointed entries take part with their ~1e9 score and are chosen when k exceeds
 *            the unpointed count (N = 3 with W = 16). A chosen entry is candidate w + [j] with
 *            its parent's (h', c'); those of length T-1 are finished hypotheses (which happens in
 *            step T-2 only, so valid stays W until then), the others the next beam in selection
 *            order
 *   result   order[b] = the finished hypothesis with the smallest score (the first selected on
 *            ties) followed by the smallest index it does not contain; score[b] = its score.
 *            N = 1 gives order [0] and score 0; N = 2 takes a single step.
 * pw_k is linear, so its four input blocks are projected once per story and keys[j] is a sum of
 * projected rows: fp32 sums in another order than the reference's one dot product per key.
 * Supported: 1 <= N <= 16, 1 <= W <= 32, any H with 16 H < 2^30, any B with 2048 B < 2^30; anything else
 * returns MMSEQ_EUNSUPPORTED before anything is launched (as does MMSEQ_EINVAL for a null
 * buffer or a short / unaligned workspace).
 *   doc, okey [B][N][H]   encode()[0] (sentence vectors), encode()[3] (key_linear output)
 *   hist      [B][N][N][H+2] = cat(cls_mat, softmax(cs_mat)), rows contiguous
 *   h0, c0    [B][H]      encode()[2]
 *   w_ih, w_hh [4H][H], b_ih, b_hh [4H]   decoder.{weight,bias}_{ih,hh}_l0
 *   w_q [H][H], b_q [H]   query_linear;   w_pw [H][4(H+2)]  pw_k.weight (no bias)
 *   w_t [H], b_t [1]      tanh_linear     (all weights [out][in] as the head's store holds them)
 *   order [B][N] int64, score [B] f32     outputs
 *   workspace: mmseq_beam_workspace(B, N, H, W) bytes (0 for an unsupported shape), 16-byte
 *     aligned, contents irrelevant on entry: rows of beam slots that are not live are computed
 *     by the GEMMs but never read by another row, so nothing in it, NaN included, reaches a
 *     result. Two calls on the same inputs give bit-identical outputs.
 * Every step reuses the workspace and reads what the step before it wrote there, so the call's
 * work is ordered on `stream` only: a concurrent call on another stream needs its own workspace
 * and outputs, and the inputs must stay unchanged until the work enqueued here has run.
 * ------------------------------------------------------------------------------------------ */
int64_t mmseq_beam_workspace(int B, int N, int H, int W);
mmseq_status mmseq_beam_search(int B, int N, int H, int W, const float* doc, const float* okey,
                               const float* hist, const float* h0, const float* c0,
                               const float* w_ih, const float* b_ih, const float* w_hh,
                               const float* b_hh, const float* w_q, const float* b_q,
                               const float* w_pw, const float* w_t, const float* b_t,
                               int64_t* order, float* score, void* workspace,
                               int64_t workspace_bytes, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Every finished hypothesis of the beam (generator.py:8-38 Beam, its `finished` list): the decode
 * of mmseq_beam_search, same inputs, same workspace (mmseq_beam_workspace), same limits and
 * status codes, same stream ordering; it reports what the last step (t = N-2) selected.
 *   orders [B][W][N] int64, scores [B][W] f32, count [B] int32      outputs
 *   entry i of story b is the i-th entry the last step selected, ascending by (score, flat
 *   index), completed with the smallest index it does not contain. A selected entry whose
 *   N - 1 picks hold a repeat (it took a pointed step somewhere on its way, score ~1e9: k exceeds
 *   the unpointed count, as for N = 3 with W = 16) is no ordering and is left out; the entries
 *   after it move up. count[b] is the number of entries reported; rows count[b] .. W-1 of
 *   orders[b] and scores[b] are NOT written.
 *   N = 1: count 1, order [0], score 0.
 * Entry 0 is mmseq_beam_search's order / score for the same inputs, bit for bit (the two entry
 * points enqueue the same kernels on the same data).
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_beam_search_nbest(int B, int N, int H, int W, const float* doc,
                                     const float* okey, const float* hist, const float* h0,
                                     const float* c0, const float* w_ih, const float* b_ih,
                                     const float* w_hh, const float* b_hh, const float* w_q,
                                     const float* b_q, const float* w_pw, const float* w_t,
                                     const float* b_t, int64_t* orders, float* scores,
                                     int32_t* count, void* workspace, int64_t workspace_bytes,
                                     mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Teacher-forced pointer scores of K candidate orders per story (modeling_bert.py:943-1174, the
 * pointer loop of BertForOrdering._forward run with labels = a candidate, after ONE encode):
 * candidate k of story b is a beam slot that never branches. At step t = 0 .. N-2 it runs exactly
 * the step of mmseq_beam_search above (x = doc[last] or 0, LSTM cell, q, keys from the four
 * projected blocks of hist, e with -1e9 where pointed, log-softmax; the same kernels) and,
 * instead of selecting, adds -logp[orders[k][t]] to its score:
 *   nll[b][k] = sum_{t < N-1} -logp_t[orders[k][t]]        step_nll[b][k][t] = the t-th term
 * summed in step order. Only the first N - 1 entries of a candidate are read; the last one is
 * implied. N = 1 gives nll 0 and writes no step_nll. A candidate scored here and the same order
 * found by mmseq_beam_search agree to fp32 GEMM rounding (the dense parts run at B*K rows here
 * and at B*W rows there), not bit for bit.
 *   doc .. b_t   as mmseq_beam_search
 *   orders       int64; candidate k of story b starts at orders + b * story_stride + k * N.
 *                story_stride = 0: one list [K][N] shared by all stories; K * N: [B][K][N]
 *   nll          [B][K] f32;  step_nll [B][K][N-1] f32 or NULL
 * Invalid candidates: one whose first N - 1 entries hold a value outside [0, N) or a repeat gets
 * nll = +INFINITY and a step_nll row of +INFINITY. Its entries are checked before any of them
 * forms an address (the slot then runs on the order 0, 1, .., N-2 and its result is discarded), so
 * no value in `orders` can cause an out-of-range access, and the other candidates of the call
 * are unaffected bit for bit.
 * Supported: 1 <= N <= 16, K >= 1, B * K * 4H < 2^31, B and H within mmseq_beam_search's limits;
 * anything else returns MMSEQ_EUNSUPPORTED before anything is launched, a null buffer (step_nll
 * excepted), a story_stride that is neither 0 nor >= K * N, or a short / unaligned workspace
 * MMSEQ_EINVAL.
 *   workspace: mmseq_order_score_workspace(B, N, H, K) bytes (0 for an unsupported shape), 16-byte
 *     aligned, contents irrelevant on entry (every element that is read was written by this call
 *     first; NaN in it reaches no output). Nothing is written outside nll, step_nll and the
 *     workspace. Two calls on the same inputs give bit-identical outputs; no atomics.
 * Stream ordering as for mmseq_beam_search.
 * ------------------------------------------------------------------------------------------ */
int64_t mmseq_order_score_workspace(int B, int N, int H, int K);
mmseq_status mmseq_order_score(int B, int N, int H, int K, const float* doc, const float* okey,
                               const float* hist, const float* h0, const float* c0,
                               const float* w_ih, const float* b_ih, const float* w_hh,
                               const float* b_hh, const float* w_q, const float* b_q,
                               const float* w_pw, const float* w_t, const float* b_t,
                               const int64_t* orders, int64_t story_stride, float* nll,
                               float* step_nll, void* workspace, int64_t workspace_bytes,
                               mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Gradient of mmseq_order_score: given dnll[b][k], the upstream gradient of every score, the
 * gradients with respect to the encoder output and the decoder weights, for sequence-level losses
 * over a candidate list (expected risk, likelihood of a set of orders, margins). The ABI keeps no
 * state between calls: this entry recomputes the scorer's forward (its own kernels, the scorer's
 * formulation: GX and the four projected blocks of hist once per story, K slots that never
 * branch), keeps h_t, c_t and the gate activations of every step in its workspace and walks
 * t = N-2 .. 0. With y_t = orders[k][t], S_t = {y_0 .. y_{t-1}}, G = dnll[b][k]:
 *   de_t[j]   = G (p_t[j] - [j = y_t]) for j not in S_t, exactly 0 for j in S_t
 *   dA_t[j]   = de_t[j] w_t (1 - a_t[j]^2),  dq_t = sum_j dA_t[j] (j ascending)
 *   dh_t      = W_hh^T dgates_{t+1} + W_q^T dq_t, then mmseq_lstm_cell_bwd's math on B*K rows
 *   dh0 / dc0 = the slots' sums, k ascending
 * Reductions to per-story rows (dGX, dokey, the four dPROJ blocks) are gathers: one workgroup per
 * destination row loops k ascending, then t ascending. No atomics; two calls on the same inputs
 * give bit-identical outputs. The dense parts run through mmseq_gemm / mmseq_gemm_wgrad in fp32.
 *   doc .. b_t, orders, story_stride   as mmseq_order_score
 *   wt_ih, wt_hh [H][4H], wt_q [H][H], wt_pw [4(H+2)][H]   the weights transposed, [in][out]
 *   dnll         [B][K] f32
 *   WRITTEN      ddoc, dokey [B][N][H], dhist [B][N][N][H+2], dh0, dc0 [B][H]
 *   ACCUMULATED  (+=) dw_ih, db_ih, dw_hh, db_hh, dw_q, db_q, dw_pw, dw_t, db_t, shaped as the
 *                weights
 * An invalid candidate (checked before any entry forms an address, as in mmseq_order_score)
 * contributes exactly zero whatever its dnll holds, NaN included. N = 1: the written gradients are
 * zeros, the accumulated ones untouched, nothing else is launched. N = 2: a single step with
 * x = 0, so ddoc = 0 and dw_ih is unchanged (db_ih is not: b_ih enters step 0).
 * Limits and status codes as mmseq_order_score (MMSEQ_EUNSUPPORTED before anything is launched;
 * a null buffer, a bad story_stride or a short / unaligned workspace MMSEQ_EINVAL).
 *   workspace: mmseq_order_score_bwd_workspace(B, N, H, K) bytes (0 for an unsupported shape),
 *     16-byte aligned, contents irrelevant on entry (NaN in it reaches no output). It holds
 *     about (N-1) B K (N+8) H floats of per-step state, so callers chunk K. Nothing is written outside
 *     the fourteen gradients and the workspace.
 * Stream ordering as for mmseq_beam_search.
 * ------------------------------------------------------------------------------------------ */
int64_t mmseq_order_score_bwd_workspace(int B, int N, int H, int K);
mmseq_status mmseq_order_score_bwd(
    int B, int N, int H, int K, const float* doc, const float* okey, const float* hist,
    const float* h0, const float* c0, const float* w_ih, const float* b_ih, const float* w_hh,
    const float* b_hh, const float* w_q, const float* b_q, const float* w_pw, const float* w_t,
    const float* b_t, const float* wt_ih, const float* wt_hh, const float* wt_q, const float* wt_pw,
    const int64_t* orders, int64_t story_stride, const float* dnll, float* ddoc, float* dokey,
    float* dhist, float* dh0, float* dc0, float* dw_ih, float* db_ih, float* dw_hh, float* db_hh,
    float* dw_q, float* db_q, float* dw_pw, float* dw_t, float* db_t, void* workspace,
    int64_t workspace_bytes, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Ancestral samples from the pointer decoder: S orders per story drawn step by step from the
 * distributions mmseq_order_score scores. Sample s of story b is a beam slot that never branches
 * (the setup, the step and the kernels of mmseq_beam_search; W = nb = S, every step entered with
 * score 0, so the step's row is r[j] = -logp_t[j]); at step t = 0 .. N-2 its pick is
 *   h      = lowbias32(lowbias32((uint32_t)e ^ k0) + ((uint32_t)(e >> 32) ^ k1)), (k0, k1) the
 *            key of (seed, stream_id) as in mmseq_mlm_mask, at the 64-bit element
 *            e = (story0 + b) * 2^32 + (sample0 + s) * (N - 1) + t
 *   u      = (h >> 8) * 2^-24                                   in [0, 1)
 *   total  = sum over the unpointed j, ascending, of expf(-r[j])          (fp32)
 *   pick   = the first unpointed j, ascending, whose running fp32 sum of expf(-r[j]) exceeds
 *            u * total; the last unpointed j when none does
 * and nll[b][s] += r[pick] in step order; the last position takes the one step left. N = 1 gives
 * the order [0] and nll 0. A sample is a pure function of (weights, inputs, seed, stream_id,
 * story0 + b, sample0 + s, t): a call for S samples from sample0 = 0 and calls for parts of them
 * with their sample0 (or parts of the stories with their story0) draw the same picks; their nll
 * agree to fp32 GEMM rounding where the row counts of the dense parts differ.
 *   doc .. b_t   as mmseq_beam_search
 *   orders       [B][S][N] int64, nll [B][S] f32                                   outputs
 *   u            [B][S][N-1] f32 or NULL: the uniforms drawn
 *   step_nlp     [B][S][N-1][N] f32 or NULL: the rows sampled from, +INFINITY where pointed
 * Supported: N, H, B as mmseq_order_score with K = S (else MMSEQ_EUNSUPPORTED, nothing launched);
 * story0, sample0 >= 0, story0 + B < 2^31, (sample0 + S) * 16 < 2^31, no null buffer (u and
 * step_nlp excepted), workspace of mmseq_order_sample_workspace(B, N, H, S) bytes (0 for an
 * unsupported shape), 16-byte aligned, contents irrelevant on entry; else MMSEQ_EINVAL. Nothing
 * is written outside the outputs and the workspace; two calls on the same inputs give
 * bit-identical outputs; no atomics. Stream ordering as for mmseq_beam_search.
 * ------------------------------------------------------------------------------------------ */
int64_t mmseq_order_sample_workspace(int B, int N, int H, int S);
mmseq_status mmseq_order_sample(int B, int N, int H, int S, const float* doc, const float* okey,
                                const float* hist, const float* h0, const float* c0,
                                const float* w_ih, const float* b_ih, const float* w_hh,
                                const float* b_hh, const float* w_q, const float* b_q,
                                const float* w_pw, const float* w_t, const float* b_t,
                                uint64_t seed, uint32_t stream_id, int story0, int sample0,
                                int64_t* orders, float* nll, float* u, float* step_nlp,
                                void* workspace, int64_t workspace_bytes, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * The pointer NLL of ALL N! orders of every story from the prefix tree (csrc/beam.hip, planner in
 * csrc/order_tree_plan.h): orders that share a prefix share its LSTM / pointer steps, so every
 * prefix of every story is stepped exactly once, sum_{t=0..N-2} N!/(N-t)! node-steps per story
 * (N = 9: 260 650) instead of the N! (N-1) (2 903 040) of mmseq_order_score over the same list.
 * The step is mmseq_beam_search's (the same setup and kernels); a child enters with its parent's
 * s entry (score - logp) of its pick, so
 *   nll[b][k] = the running fp32 sum, in step order, of -logp_t[o_t], t = 0 .. N-2, o the k-th
 *               permutation of 0 .. N-1 in lexicographic order (itertools.permutations(range(N))),
 * as mmseq_order_score defines it; the two agree to fp32 GEMM rounding (the dense parts run at
 * other row counts), not bit for bit. Only N - 1 steps run, the last position is implied; N = 1
 * gives nll 0 with nothing launched but the write, N = 2 is a single step.
 * Indexing: a node of level t (t picks made) with index i has the children i (N-t) + r, r counting
 * the still-unpointed steps in ascending order; a node of level N-1 is its order's rank k.
 *   doc .. b_t   as mmseq_beam_search
 *   rows         the caller's cap on the slot rows (over all B stories) one chunk of one level may
 *                hold, >= B * N. Level t owns one state buffer of min(N!/(N-t)!, rows / B) nodes
 *                per story; the tree is walked in chunks (the same node range of every story),
 *                each stepped and then descended below before the next is taken, so any `rows` in
 *                range gives the same set of node-steps. rows beyond (2^31 - 2) / max(4H, 16)
 *                counts as that (the dense parts count elements in 32 bits).
 *   nll          [B][N!] f32                                                          output
 *   orders       [N!][N] int64 or NULL: the same table unranked on the device, one list for all
 *                stories (the story_stride = 0 list of mmseq_order_posterior / mmseq_order_score)
 *   workspace    mmseq_order_tree_workspace(B, N, H, rows) bytes, a function of these four alone
 *                (0 for an unsupported shape or rows < B * N), 16-byte aligned, contents irrelevant
 *                on entry: every element that is read was written by this call first, NaN in it
 *                reaches no output. Nothing is written outside nll, orders and the workspace.
 * The schedule follows from (B, N, rows) on the host: the whole call is enqueued on `stream` with
 * no host synchronisation and no copy to the host; no atomics; two calls on the same inputs (and
 * the same rows) give bit-identical outputs. Calls with different `rows` agree to fp32 GEMM
 * rounding.
 * Supported: 1 <= N <= 9, B * N! < 2^31, B * N * 4H < 2^31, B and H within mmseq_beam_search's
 * limits; anything else returns MMSEQ_EUNSUPPORTED before anything is launched. A null buffer
 * (orders excepted), rows < B * N, or a short / unaligned workspace MMSEQ_EINVAL, likewise with
 * nothing launched. Stream ordering as for mmseq_beam_search.
 * ------------------------------------------------------------------------------------------ */
int64_t mmseq_order_tree_workspace(int B, int N, int H, int64_t rows);
mmseq_status mmseq_order_tree(int B, int N, int H, const float* doc, const float* okey,
                              const float* hist, const float* h0, const float* c0,
                              const float* w_ih, const float* b_ih, const float* w_hh,
                              const float* b_hh, const float* w_q, const float* b_q,
                              const float* w_pw, const float* w_t, const float* b_t, int64_t rows,
                              float* nll, int64_t* orders, void* workspace,
                              int64_t workspace_bytes, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Posterior over K candidate orders per story (csrc/posterior.hip): from their pointer NLLs to
 * marginals, the heaviest candidate and the minimum-risk candidates under the per-story metrics
 * of evaluate.cal_result. One workgroup per story; every sum is taken in f64 in ascending
 * candidate order and rounded once to f32; no atomics, bit-identical between calls.
 *   orders  int64; candidate k of story b starts at orders + b * story_stride + k * N
 *           (story_stride = 0: one list [K][N] for all stories; K * N: [B][K][N])
 *   nll     [B][K] f32
 *   valid   a candidate is valid iff its nll is finite and its N entries are a permutation of
 *           0 .. N-1 (checked before any entry is used as an index); the others weigh 0: +inf
 *           scores, the n-best list's padding rows (order -1, score +inf), samples that failed
 *   mode 0  w_k = exp(m - nll_k), m the smallest valid nll (weights proportional to exp(-nll))
 *   mode 1  w_k = 1 (a list of samples: uniform; a repeated order counts as often as it occurs)
 *   Z = sum w_k, p_k = w_k / Z over the valid candidates
 * Outputs per story (f32 unless stated):
 *   logz               log Z - m (mode 0: logsumexp(-nll), the log of the mass the list covers);
 *                      log(valid count) (mode 1)
 *   position [N][N]    position[t][s] = sum of p_k over the candidates with step s at position t
 *   before   [N][N]    before[a][c]   = sum of p_k over those where a precedes c; diagonal 0
 *   entropy            -sum p_k log p_k, nats
 *   map_index int32, map_prob      the heaviest candidate (the smallest nll; the first valid one
 *                      in mode 1), ties (-0.0 and +0.0 tie) to the lowest index, and its p
 *   mbr_acc_index, mbr_tau_index int32, exp_acc, exp_tau     the valid candidates with the largest
 *                      gain_acc(o) = (sum_t position[t][o_t]) / N                  t ascending
 *                      gain_tau(o) = (sum_{i<j} before[o_i][o_j] - before[o_j][o_i]) / C(N, 2)
 *                                    (i, j) lexicographic; 1 for N = 1
 *                      computed in f64 from the f32-rounded matrices in the order stated, ties to
 *                      the lowest index, and those gains: the expectations under p of
 *                      cal_result's per-story accuracy and Kendall's tau of o
 * A story without a valid candidate gets logz = -INFINITY, zero matrices, indices -1 and 0 in the
 * other outputs. Nothing is written outside the outputs' declared extents.
 * Supported: B >= 0, 1 <= N <= 16, K >= 1, else MMSEQ_EUNSUPPORTED with nothing launched; a mode
 * other than 0 / 1, a null buffer or a story_stride that is neither 0 nor >= K * N MMSEQ_EINVAL.
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_order_posterior(int B, int N, int K, int mode, const int64_t* orders,
                                   int64_t story_stride, const float* nll, float* logz,
                                   float* position, float* before, float* entropy,
                                   int32_t* map_index, float* map_prob, int32_t* mbr_acc_index,
                                   int32_t* mbr_tau_index, float* exp_acc, float* exp_tau,
                                   mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Decoding from the pairwise head (csrc/pairwise.hip). w [B][N][N] f32, w[a][c] = the log-evidence
 * that step a precedes step c (berson.pairwise_weights: log_softmax(cs[a][c])[1] +
 * log_softmax(cs[c][a])[0]; any pairwise score will do); the diagonal is never read. For an order
 * o (o[t] = the step at position t)
 *   G(o) = sum_{i<j} w[o_i][o_j],  pnll(o) = -G(o),  Q(o) = exp(G(o)) / Z.
 * mmseq_pairwise_order: the arg-max of G and the distribution Q, exactly, by dynamic programming
 * over the 2^N subsets S of steps already placed; one workgroup per story, f64 throughout.
 *   g(S, c)   = sum_{a in S} w[a][c], a ascending, from 0.0
 *   h1[full] = 0, h2[full] = -inf; below full {h1[S], h2[S]} = the two largest of
 *               {g(S,c) + h1[S+c], g(S,c) + h2[S+c] : c not in S}: the best and second-best
 *               completion as distinct orders (equal values give h2 = h1)
 *   order     [B][N] int64: from the front, the lowest c not in S with g(S,c) + h1[S+c] == h1[S]:
 *               the lexicographically smallest maximiser
 *   pnll      [B] f32(-h1[0]);  margin [B] f32(h1[0] - h2[0]), +inf for N = 1
 *   la[0] = 0, la[T] = log sum_{c in T} exp(la[T-c] + g(T-c, c));  lb[full] = 0,
 *   lb[S] = log sum_{c not in S} exp(g(S,c) + lb[S+c]): each c ascending, shifted by its largest
 *               term
 *   logz      [B] la[full]
 *   p(S, c)   = exp(((la[S] + g(S,c)) + lb[S+c]) - logz)
 *   position  [B][N][N]: position[t][s] = sum_{|S| = t, s not in S} p(S, s)
 *   before    [B][N][N]: before[a][c] = sum_{S has a, not c} p(S, c); diagonal 0; both S ascending
 *   entropy   [B] logz - sum_{a != c} before[a][c] w[a][c], (a, c) lexicographic, from the f64 sums
 * Every output is rounded once to f32. No atomics: bit-identical between calls and independent of
 * B and of which stories share the launch. A story with a non-finite off-diagonal w gets order -1,
 * pnll +inf, margin 0, logz -inf, zero matrices and entropy 0.
 *   workspace  mmseq_pairwise_order_workspace(B, N) bytes (a positive multiple of 16 for a
 *              supported shape, 0 otherwise), 16-byte aligned, contents irrelevant on entry: the
 *              tables of N = 12; up to N = 11 they live in LDS and it is not touched.
 * Supported: B >= 0, 1 <= N <= 12, else MMSEQ_EUNSUPPORTED with nothing launched or written; a
 * null buffer or a short / unaligned workspace MMSEQ_EINVAL, likewise.
 * mmseq_pairwise_score: pnll[b][k] = f32(-sum_{i<j} w[b][o_i][o_j]), (i, j) lexicographic, in
 * f64, of candidate k of story b at orders + b * story_stride + k * N (story_stride = 0: one list
 * [K][N] for all stories; >= K * N: per story), as mmseq_order_posterior. A candidate that is no
 * permutation of 0 .. N-1 (checked before any entry is used as an index) gets +inf, and so does
 * every candidate of a story with a non-finite off-diagonal w.
 * Supported: B >= 0, 1 <= N <= 16, K >= 1, else MMSEQ_EUNSUPPORTED with nothing launched; a null
 * buffer or a story_stride that is neither 0 nor >= K * N MMSEQ_EINVAL.
 * ------------------------------------------------------------------------------------------ */
int64_t mmseq_pairwise_order_workspace(int B, int N);
mmseq_status mmseq_pairwise_order(int B, int N, const float* w, int64_t* order, float* pnll,
                                  float* margin, float* logz, float* position, float* before,
                                  float* entropy, void* workspace, int64_t workspace_bytes,
                                  mmseq_stream stream);
mmseq_status mmseq_pairwise_score(int B, int N, int K, const float* w, const int64_t* orders,
                                  int64_t story_stride, float* pnll, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * MX-fp8 forward GEMMs (BASELINE config 5 "fp8 MFMA"; v_mfma_scale_f32_16x16x128_f8f6f4).
 *  Format: OCP e4m3 elements, one E8M0 scale (2^(s-127)) per 32 consecutive K-elements of a row
 *  (OCP MX: s = floor(log2 amax) - 8 + 127, elements = x / 2^(s-127) clamped to +-448, RNE).
 *  Scales are stored "packed": byte ((m/64)*(K/32) + kb)*64 + (m%16)*4 + (m%64)/16, for rows up
 *  to the next multiple of 64 (mmseq_mxfp8_scale_bytes).
 *  quant: x [M][K] (bf16 or f32, row stride ldx) -> q [M][K] e4m3 (row stride ldq, % 16 == 0)
 *         + scales. K % 32 == 0.
 *  gemm:  C[m][n] bf16 (ldc) = act(alpha * sum_k A[m][k] B[n][k] + bias[n]) + resid[m][n]
 *         (bias / resid may be NULL; act = mmseq_act); A [M][K], B [N][K] quantised as above,
 *         K % 128 == 0, lda / ldb % 16 == 0. fp32 accumulation.
 * ------------------------------------------------------------------------------------------ */
int64_t mmseq_mxfp8_scale_bytes(int M, int K);
mmseq_status mmseq_quant_mxfp8(int M, int K, const void* x, int64_t ldx, mmseq_dtype dtype,
                               void* q, int64_t ldq, void* scales, mmseq_stream stream);
mmseq_status mmseq_gemm_mxfp8(int M, int N, int K, const void* A, int64_t lda,
                              const void* a_scales, const void* B, int64_t ldb,
                              const void* b_scales, void* C, int64_t ldc, const float* bias,
                              int act, const void* resid, int64_t ldr, float alpha,
                              mmseq_stream stream);
/* gemm_mxfp8_out: bf16 GEMM whose output is written in the format above, for a consumer GEMM
 *  that takes it as its MX-fp8 A operand (the MLP: FC1 + GELU -> FC2, lxrt/modeling.py:467-493)
 *  with no quantisation pass: q [M][N] e4m3 (ldq % 16 == 0) + scales for (M, N) =
 *  quant(bf16(act(A B^T + bias))), bit-identical to mmseq_gemm (bf16 out) + mmseq_quant_mxfp8.
 *  A [M][K], B [N][K] bf16, K % 128 == 0, N % 32 == 0, 16-byte aligned operands. */
mmseq_status mmseq_gemm_mxfp8_out(int M, int N, int K, const void* A, int64_t lda, const void* B,
                                  int64_t ldb, const float* bias, int act, void* q, int64_t ldq,
                                  void* scales, mmseq_stream stream);
/* gemm_mxfp8_q8: MX-fp8 GEMM (A, B and scales as mmseq_gemm_mxfp8) whose output is MX-fp8 as in
 *  mmseq_gemm_mxfp8_out: q [M][N] e4m3 + q_scales = quant(bf16(act(A B^T + bias))), for the MLP's
 *  FC1 -> FC2 chain with both GEMMs on the fp8 MFMA (lxrt/modeling.py:467-493, clip/model.py:
 *  208-214). K % 256 == 0, N % 32 == 0, 16-byte aligned operands, lda / ldb / ldq % 16 == 0. */
mmseq_status mmseq_gemm_mxfp8_q8(int M, int N, int K, const void* A, int64_t lda,
                                 const void* a_scales, const void* B, int64_t ldb,
                                 const void* b_scales, const float* bias, int act, void* q,
                                 int64_t ldq, void* q_scales, mmseq_stream stream);
/* gemm_mxfp8_ex: the training-forward form (config 5 with the fp8 forward GEMMs; backward bf16):
 *  C (bf16 [M][ldc]) = dropout(act(A B^T + bias)) + resid, aux (optional, needs act) = the bf16
 *  pre-activation [M][ldc]; or, with q / q_scales, the MX-fp8 output quant(bf16(act(A B^T + bias)))
 *  (no resid / drop) with C (optional) its bf16 copy and aux the pre-activation (FC1: what the
 *  backward reads and FC2's fp8 operand, lxrt/modeling.py:467-493, clip/model.py:208-214).
 *  With dact (and act, nothing else): the dgrad form C = (A B^T) * act'(dact), dact bf16 [M][ldc]
 *  (the backward's fp8 dgrad: dz = dY W * GELU'(z)); with q as well, q / q_scales = its MX-fp8 (the
 *  next dgrad GEMM's operand) and C the bf16 copy (the weight gradient's operand). The dropout mask is the bf16 GEMM's
 *  (mmseq_gemm) for the same descriptor. K % 256 == 0 and
 *  M, N >= 256 (else MMSEQ_EUNSUPPORTED); ldc, ldr % 8, ldq % 16, 16-byte aligned buffers. */
mmseq_status mmseq_gemm_mxfp8_ex(int M, int N, int K, const void* A, int64_t lda,
                                 const void* a_scales, const void* B, int64_t ldb,
                                 const void* b_scales, void* C, int64_t ldc, const float* bias,
                                 int act, void* aux, const void* dact, const void* resid, int64_t ldr,
                                 const mmseq_dropout* drop, void* q, int64_t ldq, void* q_scales,
                                 mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * CLIP ModifiedResNet / RN50 (clip/model.py:10-187; lxrt/modeling.py:621-705, 1014-1030), NHWC.
 *  conv_im2col: x [U][H][W][C] -> cols [U*Ho*Wo][Kp], column (ky*ks + kx)*C + c (zero in the
 *               padding and past ks*ks*C); the convolution is then the NT GEMM with the weight as
 *               [Cout][Kp] in the same column order. conv_col2im: the dgrad scatter as a gather.
 *  bn_fwd:  y = act((x - mean) * rstd * gamma + beta + resid), relu optional; train: batch
 *           statistics over the rows (Welford partials merged in fixed order), running stats
 *           updated with momentum and the unbiased variance for n_ref elements; eval: running
 *           statistics. mean / rstd [C] are written for the backward. Workspace mmseq_bn_workspace.
 *  bn_bwd:  g = dy * (y > 0 if y != NULL); dgamma += sum g xhat, dbeta += sum g;
 *           dx = gamma rstd (g - mean g - xhat mean(g xhat)) (train) / gamma rstd g (eval);
 *           dres = g when non-NULL (the residual branch).
 *  avgpool2: 2x2 average pool (backward = 1/4 to each input).
 *  attnpool_gather: pair p's two images (pairimg [P][2], unique image ids) -> x [P][2S+1][C]
 *           with the reference's reshape-before-permute token order (clip/model.py:77), the mean
 *           token first and the img_len positional quirk (:79-81); gather_bwd sums the pairs.
 *  attnpool_out: y [rows][2Ch] = cat(a, a) + visual x/y position + token type (G x G grid);
 *           out_bwd: da = both halves summed, token_colsum [T2][2Ch] = sum over pairs.
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_conv_im2col(int U, int H, int W, int C, int ks, int stride, int pad, int Kp,
                               const void* x, void* cols, mmseq_dtype dtype, mmseq_stream stream);
mmseq_status mmseq_conv_col2im(int U, int H, int W, int C, int ks, int stride, int pad, int Kp,
                               const void* dcols, void* dx, mmseq_dtype dtype,
                               mmseq_stream stream);
int64_t mmseq_bn_workspace(int64_t rows, int C);
mmseq_status mmseq_bn_fwd(int64_t rows, int C, const void* x, const float* gamma,
                          const float* beta, const void* resid, int relu, int train, float eps,
                          float momentum, double n_ref, float* mean, float* rstd,
                          float* run_mean, float* run_var, void* y, float* workspace,
                          int64_t workspace_bytes, mmseq_dtype dtype, mmseq_stream stream);
mmseq_status mmseq_bn_bwd(int64_t rows, int C, const void* dy, const void* y, const void* x,
                          const float* mean, const float* rstd, const float* gamma, int train,
                          float* dgamma, float* dbeta, void* dx, void* dres, float* workspace,
                          int64_t workspace_bytes, mmseq_dtype dtype, mmseq_stream stream);
mmseq_status mmseq_avgpool2(int U, int H, int W, int C, const void* x, void* y, int backward,
                            mmseq_dtype dtype, mmseq_stream stream);
mmseq_status mmseq_attnpool_gather(int P, int S, int C, const void* feats,
                                   const int32_t* pairimg, const float* pos, void* x,
                                   mmseq_dtype dtype, mmseq_stream stream);
mmseq_status mmseq_attnpool_gather_bwd(int U, int N, int S, int C, int npair, const void* dx,
                                       const int32_t* rolepairs, void* dfeats,
                                       mmseq_dtype dtype, mmseq_stream stream);
mmseq_status mmseq_attnpool_out(int64_t rows, int T2, int Ch, int G, const void* a,
                                const float* xpos, const float* ypos, const float* ttype,
                                void* y, mmseq_dtype dtype, mmseq_stream stream);
mmseq_status mmseq_attnpool_out_bwd(int P, int T2, int Ch, const void* dy, void* da,
                                    float* token_colsum, mmseq_dtype dtype, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Row selection on activations (text+image pretraining: the PISP patch swap lxrt/modeling.py:
 * 885-942, the MRM masking and its targets :948-1009, the labelled rows of the masked-LM head).
 * Rows are addressed as in mmseq_rows; R_out rows of out / dout, R_in rows of in / din.
 *  fwd: out[r][:] = keep[r] ? in[src[r]][:] : 0 for r < R_out. src int32 [R_out], its entries
 *       unique and in [0, R_in) (an entry outside reads nothing and gives a zero row); keep uint8
 *       [R_out] or NULL (= all kept).
 *  bwd: din (all R_in rows) is zeroed, then din[src[r]][:] = keep[r] ? dout[r][:] : 0. src is
 *       unique, so these are plain stores: no atomics, two calls give the same bits.
 * A permutation (R_out == R_in), a mask (identity src + keep) and a compaction (R_out < R_in) are
 * the same call. bf16 and fp32, 16-byte accesses: cols % 8 == 0, 16-byte aligned bases, ld and
 * bstride multiples of 16 bytes; anything else returns MMSEQ_EUNSUPPORTED with nothing launched.
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_rows_gather_fwd(int R_out, int R_in, int cols, const void* in, mmseq_rows inl,
                                   const int32_t* src, const uint8_t* keep, void* out,
                                   mmseq_rows outl, mmseq_dtype dtype, mmseq_stream stream);
mmseq_status mmseq_rows_gather_bwd(int R_out, int R_in, int cols, const void* dout,
                                   mmseq_rows doutl, const int32_t* src, const uint8_t* keep,
                                   void* din, mmseq_rows dinl, mmseq_dtype dtype,
                                   mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Softmax cross-entropy with mean reduction over the kept rows (the masked-LM loss,
 * lxrt/modeling.py:2260-2266 CrossEntropyLoss(ignore_index) over BertLMPredictionHead :1157-1173):
 * logits [M][ld] bf16 or fp32 with V <= ld valid columns (finite values), labels int64 [M].
 * Columns >= V are never used as data, whatever they hold.
 *  fwd: lse[r] = log sum_c exp(logits[r][c]) (online max / sum in fp32, one workgroup per row);
 *       loss_row[r] = lse[r] - logits[r][label[r]], 0 where label[r] == ignore_index (NaN for any
 *       other label outside [0, V): nothing is read for it); stats[0] = sum(loss_row) / count,
 *       stats[1] = count = rows with label != ignore_index, both summed in a fixed order by one
 *       workgroup (count 0 gives stats[0] = NaN, as the reference's 0 / 0).
 *  bwd: logits is overwritten IN PLACE, in its dtype, by dlogits[r][c] = (exp(x - lse[r]) -
 *       (c == label[r])) * g[0] / count (g: one device float, NULL = 1); exact zeros in ignored
 *       rows and in columns V .. ld-1, so the buffer is the A operand of the dgrad GEMM (K = ld)
 *       and of the weight-gradient GEMM as it stands.
 * ld % (16 bytes) == 0, ld >= V, 16-byte aligned logits; else MMSEQ_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_xent_fwd(int M, int V, const void* logits, int64_t ld, const int64_t* labels,
                            int64_t ignore_index, float* lse, float* loss_row, float* stats,
                            mmseq_dtype dtype, mmseq_stream stream);
mmseq_status mmseq_xent_bwd(int M, int V, void* logits, int64_t ld, const int64_t* labels,
                            int64_t ignore_index, const float* lse, const float* stats,
                            const float* g, mmseq_dtype dtype, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Masked-LM evaluation in the forward's one pass (the counterpart of run_pretraining.py:377-511,
 * whose "{task}_perplexity" is a TODO and which reports no accuracy): logits, labels, ld and the
 * alignment rule as mmseq_xent_fwd; 0 <= k <= MMSEQ_XENT_EVAL_MAX_K, else MMSEQ_EINVAL with
 * nothing launched. Candidates are ordered by (value descending, column ascending), values
 * compared as float (-0.0 ties with +0.0): a total order, so no output depends on a merge order.
 *  lse[r], loss_row[r]: the bits mmseq_xent_fwd writes for the same buffer (same traversal, same
 *       wave-then-workgroup merge), 0 for ignored rows and NaN for any other label outside [0, V).
 *  rank[r] = #{c : x[c] > x[lab]} + #{c < lab : x[c] == x[lab]}, -1 for an ignored row or an
 *       invalid label (nothing is read for either).
 *  topk_idx[r][0..k), topk_logit[r][0..k): the k first candidates of EVERY row (fill-mask needs no
 *       label); entries past V are (-1, -inf). k == 0: both may be NULL, nothing is written.
 *       rank == 0 <=> topk_idx[r][0] == label; 0 <= rank < k <=> the label is among the k.
 *  totals (double[4], NULL skips it): [0] += sum of loss_row over the kept rows, [1] += kept rows,
 *       [2] += rows with rank 0, [3] += rows with 0 <= rank < k; one workgroup, fixed order, no
 *       atomics. An evaluation loop accumulates over its batches and reads 32 bytes back once.
 * mmseq_xent_mean: stats[0] = sum(loss_row) / count, stats[1] = count over the kept rows, the
 *       reduction mmseq_xent_fwd ends with (same bits), for loss_row written by mmseq_xent_eval.
 * ------------------------------------------------------------------------------------------ */
#define MMSEQ_XENT_EVAL_MAX_K 8
mmseq_status mmseq_xent_eval(int M, int V, const void* logits, int64_t ld, const int64_t* labels,
                             int64_t ignore_index, int k, float* lse, float* loss_row,
                             int32_t* rank, int32_t* topk_idx, float* topk_logit, double* totals,
                             mmseq_dtype dtype, mmseq_stream stream);
mmseq_status mmseq_xent_mean(int M, const float* loss_row, const int64_t* labels,
                             int64_t ignore_index, float* stats, mmseq_stream stream);

/* ------------------------------------------------------------------------------------------
 * Pretraining inputs on device (text+image stage): csrc/inputs.hip.
 *
 * mlm_mask: trainers/train_utils.py:19-66 mask_tokens_sentence on input_ids [B][L] IN PLACE, with
 * labels [B][L] written. A token is a candidate iff it is neither pad_id nor cls_id (</s> is
 * maskable, as in the reference); a candidate is selected with probability p; labels = the
 * original id where selected, ignore_index elsewhere; of the selected 80 % become mask_id, half of
 * the rest a word drawn uniformly from [cls_id + 1, vocab), the remainder stay. (The reference
 * draws its Bernoulli for the first n positions, n = the number of non-pad tokens, and asserts
 * that none of them is a pad: for trailing padding that is "the non-pad positions".)
 * Counter-based like the dropout above, a pure function of (seed, stream_id, e = b*L + l), so the
 * launch geometry cannot matter:
 *   (k0, k1)   = the dropout key of (seed, stream_id) (make_drop)
 *   h          = lowbias32(lowbias32((uint32_t)e ^ k0) + ((uint32_t)(e >> 32) ^ k1))
 *                (TWO rounds: with one, the selection bits of elements 64 apart correlate)
 *   h2         = drop_hash2(h); h3 = drop_hash2(h2)
 *   selected   iff candidate and (h & 0xFFFF) < thr, thr = clamp(floor(p * 65536 + 0.5), 0, 65536)
 *              (p = 0 selects nothing, p = 1 every candidate)
 *   -> mask_id iff (h >> 16) < 52429; else -> random word iff (h2 & 0xFFFF) < 32768,
 *   word       = cls_id + 1 + (((uint64_t)h3 * (uint64_t)(vocab - cls_id - 1)) >> 32)
 * 0 <= cls_id + 1 < vocab < 2^31 and B * L < 2^31, else MMSEQ_EINVAL with nothing launched.
 *
 * subsample_text: the text of the n_sub sub-sampled steps per story (lxrt/modeling.py:1986-2032):
 * step k runs from the k-th cls_id to the next one, the last step (k = n_steps - 1) takes
 * L / n_steps tokens; the steps sub_idx[b][0 .. n_sub) (ascending) are concatenated into rows of
 * (L / n_steps) * n_sub and padded with pad_id / 0 / 0 / ignore_index. token_type_ids and labels
 * may be NULL together with their outputs. status[0] += the number of stories with a step index
 * outside [0, n_steps) or without its cls token, a non-last step whose following cls token is
 * missing, or kept steps that overrun the padded length or L (zero it first; the caller raises);
 * such a story's output rows are all padding. One wave per story; 2 <= n_steps <= 64.
 *
 * rows_compact: src[0 .. count) = the r < R, ascending, with labels[r] != ignore_index, and
 * out_labels their labels: torch.nonzero's order, so the masked-LM loss sums the same rows in the
 * same order as with host labels. src / out_labels hold R entries; nothing at or beyond count is
 * written; *count is a plain store. One workgroup, an ordered scan, no atomics: deterministic.
 * ------------------------------------------------------------------------------------------ */
mmseq_status mmseq_mlm_mask(int B, int L, int64_t* input_ids, int64_t* labels, int64_t pad_id,
                            int64_t cls_id, int64_t mask_id, int64_t vocab, int64_t ignore_index,
                            float p, uint64_t seed, uint32_t stream_id, mmseq_stream stream);
mmseq_status mmseq_subsample_text(int B, int L, int n_steps, int n_sub, const int64_t* input_ids,
                                  const int64_t* attention_mask, const int64_t* token_type_ids,
                                  const int64_t* labels, const int64_t* sub_idx, int64_t cls_id,
                                  int64_t pad_id, int64_t ignore_index, int64_t* out_ids,
                                  int64_t* out_mask, int64_t* out_token_type, int64_t* out_labels,
                                  int32_t* status, mmseq_stream stream);
mmseq_status mmseq_rows_compact(int R, const int64_t* labels, int64_t ignore_index, int32_t* src,
                                int64_t* out_labels, int32_t* count, mmseq_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* MMSEQ_H */
