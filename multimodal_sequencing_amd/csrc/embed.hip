// Token-side and patch-side embedding kernels, writing straight into the activation buffers.
//   text:  BertEmbeddings (lxrt/modeling.py:342-370) fused with the image-text concat (:1093)
//   image: CLIP ViT patchify + class token + img_len=2 positional quirk + ln_pre
//          (clip/model.py:262-278), with the per-pair image gather of
//          process_images (process_inputs_for_berson.py:82-97) done on device.
#include "launch_plan.h"
#include "reduce.h"
#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>

namespace {

constexpr int MAXV = 16;
constexpr int RPB = mmseq_plan::EMBED_RPB;  // rows per workgroup of the backward kernels, by their name for it
typedef unsigned short us;

// ---------------------------------------------------------------------------------------------
// text embeddings
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void embed_fwd_kernel(int P, int Lt, int H,
                                                        const int64_t* __restrict__ ids,
                                                        const int64_t* __restrict__ tt,
                                                        const float* __restrict__ word,
                                                        const float* __restrict__ pos,
                                                        const float* __restrict__ type,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps,
                                                        T* __restrict__ joint, int64_t ld_pair,
                                                        float* __restrict__ mean,
                                                        float* __restrict__ rstd, Drop dr) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= (int64_t)P * Lt) return;
  const int p = r / Lt, t = r % Lt;
  const float* wr = word + ids[r] * H;
  const float* pr = pos + (int64_t)t * H;
  const float* tr = type + (tt ? tt[r] : 0) * H;
  float v[MAXV], s = 0.f;
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    int c = j * 64 + lane;
    v[j] = c < H ? wr[c] + pr[c] + tr[c] : 0.f;
    s += v[j];
  }
  const float mu = wave_sum(s) / H;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    int c = j * 64 + lane;
    float d = c < H ? v[j] - mu : 0.f;
    q += d * d;
  }
  const float rs = rsqrtf(wave_sum(q) / H + eps);
  T* out = joint + (int64_t)p * ld_pair + (int64_t)t * H;
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    int c = j * 64 + lane;
    if (c < H)
      Elem<T>::st(out + c, ((v[j] - mu) * rs * gamma[c] + beta[c]) * drop_mul(dr, (uint64_t)r * H + c));
  }
  if (lane == 0) {
    mean[r] = mu;
    rstd[r] = rs;
  }
}

// LN backward on recomputed e; de -> ws_de [P*Lt][H] (f32). The word / type tables' scatter-add
// runs afterwards in a fixed order (table_scatter_det: rows grouped by id, summed in row order), so
// the backward is bit-stable run to run (row 0 skipped: padding_idx = 0 on all three tables,
// lxrt/modeling.py:347-349).
template <typename T>
__global__ __launch_bounds__(256) void embed_bwd_kernel(int P, int Lt, int H,
                                                        const int64_t* __restrict__ ids,
                                                        const int64_t* __restrict__ tt,
                                                        const float* __restrict__ word,
                                                        const float* __restrict__ pos,
                                                        const float* __restrict__ type,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ mean,
                                                        const float* __restrict__ rstd,
                                                        const T* __restrict__ djoint,
                                                        int64_t ld_pair,
                                                        float* __restrict__ ws_de,
                                                        float* __restrict__ ws_ln, Drop dr) {
  __shared__ float red[4][2][1024];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t rows = (int64_t)P * Lt;
  float pg[MAXV], pb[MAXV];
#pragma unroll
  for (int j = 0; j < MAXV; ++j) pg[j] = pb[j] = 0.f;
  const int64_t rbeg = (int64_t)blockIdx.x * RPB;
  for (int64_t r = rbeg + wave; r < rbeg + RPB && r < rows; r += 4) {
    const int p = r / Lt, t = r % Lt;
    const int64_t id = ids[r];
    const int64_t ty = tt ? tt[r] : 0;
    const float* wr = word + id * H;
    const float* pr = pos + (int64_t)t * H;
    const float* tr = type + ty * H;
    const T* dyr = djoint + (int64_t)p * ld_pair + (int64_t)t * H;
    const float mu = mean[r], rs = rstd[r];
    float xh[MAXV], gdy[MAXV], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
      int c = j * 64 + lane;
      if (c < H) {
        float xv = (wr[c] + pr[c] + tr[c] - mu) * rs;
        float d = Elem<T>::ld(dyr + c) * drop_mul(dr, (uint64_t)r * H + c);
        xh[j] = xv;
        gdy[j] = d * gamma[c];
        pg[j] += d * xv;
        pb[j] += d;
        s1 += gdy[j];
        s2 += gdy[j] * xv;
      } else {
        xh[j] = gdy[j] = 0.f;
      }
    }
    s1 = wave_sum(s1) / H;
    s2 = wave_sum(s2) / H;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
      int c = j * 64 + lane;
      if (c < H) {
        float de = rs * (gdy[j] - s1 - xh[j] * s2);
        ws_de[r * H + c] = de;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    int c = j * 64 + lane;
    if (c < H) {
      red[wave][0][c] = pg[j];
      red[wave][1][c] = pb[j];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < H; c += 256) {
    ws_ln[((int64_t)blockIdx.x * 2 + 0) * H + c] =
        red[0][0][c] + red[1][0][c] + red[2][0][c] + red[3][0][c];
    ws_ln[((int64_t)blockIdx.x * 2 + 1) * H + c] =
        red[0][1][c] + red[1][1][c] + red[2][1][c] + red[3][1][c];
  }
}

// ---------------------------------------------------------------------------------------------
// Deterministic embedding-table gradient: table[id] += sum of de[r] over the rows r with ids[r] ==
// id (id 0 skipped, padding_idx), every sum in ascending row order. The rows are grouped by one
// radix sort of the keys (id << 32 | r); the sorted positions are cut into chunks of SEG_C, one
// workgroup per chunk sums each run of equal ids in order; a run wholly inside its chunk is added
// to the table by that workgroup, a run crossing chunk boundaries leaves its pieces in per-chunk
// slots that the segment's first chunk then adds in chunk order. Replaces float atomics, whose
// ordering made two backwards of the same inputs differ.
// ---------------------------------------------------------------------------------------------
constexpr int SEG_C = 64;
constexpr uint32_t SEG_NONE = 0xFFFFFFFFu;  // an id no row has (ids < 2^32 - 1)

__global__ __launch_bounds__(256) void row_keys_kernel(int64_t n, const int64_t* __restrict__ ids,
                                                       uint64_t* __restrict__ keys) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r < n) keys[r] = ((uint64_t)(uint32_t)ids[r] << 32) | (uint64_t)(uint32_t)r;
}

__device__ __forceinline__ uint32_t seg_id(const uint64_t* keys, int64_t n, int64_t i) {
  return (i >= 0 && i < n) ? (uint32_t)(keys[i] >> 32) : SEG_NONE;
}

// one workgroup per chunk of SEG_C sorted positions; thread t owns columns 4t .. 4t + 3 (H <= 1024,
// H % 4 == 0); parts [nch][2][H]: slot 0 = the chunk's first run when it continues a run of the
// previous chunk, slot 1 = its last run when that run starts here and continues into the next chunk
__global__ __launch_bounds__(256) void seg_rows_kernel(int64_t n, int H, const uint64_t* __restrict__ keys,
                                                       const float* __restrict__ de,
                                                       float* __restrict__ table,
                                                       float* __restrict__ parts) {
  __shared__ uint64_t k[SEG_C];
  const int64_t c = blockIdx.x, i0 = c * SEG_C;
  const int cnt = (int)min((int64_t)SEG_C, n - i0);
  const int tid = threadIdx.x;
  if (tid < cnt) k[tid] = keys[i0 + tid];
  __syncthreads();
  const uint32_t prev = seg_id(keys, n, i0 - 1), next = seg_id(keys, n, i0 + cnt);
  const bool act = tid * 4 < H;
  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
  int start = 0;
  for (int j = 0; j < cnt; ++j) {
    const uint32_t id = (uint32_t)(k[j] >> 32);
    const uint32_t row = (uint32_t)k[j];
    if (act) acc += *reinterpret_cast<const f32x4*>(de + (int64_t)row * H + 4 * tid);
    const bool last = j == cnt - 1 || (uint32_t)(k[j + 1] >> 32) != id;
    if (!last) continue;
    if (id != 0 && act) {
      const bool began = start > 0 || prev != id;
      const bool ends = j < cnt - 1 || next != id;
      if (began && ends) {
        f32x4* t = reinterpret_cast<f32x4*>(table + (int64_t)id * H + 4 * tid);
        *t = *t + acc;
      } else {
        *reinterpret_cast<f32x4*>(parts + (c * 2 + (began ? 1 : 0)) * H + 4 * tid) = acc;
      }
    }
    acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    start = j + 1;
  }
}

// one workgroup per chunk: the first chunk of a run that crosses into the next chunk adds the run's
// pieces in chunk order
__global__ __launch_bounds__(256) void seg_join_kernel(int64_t n, int H, const uint64_t* __restrict__ keys,
                                                       float* __restrict__ table,
                                                       const float* __restrict__ parts) {
  const int64_t c = blockIdx.x, i0 = c * SEG_C;
  const int64_t iend = min(n, i0 + SEG_C);  // one past the chunk's last position
  const uint32_t id = seg_id(keys, n, iend - 1);
  if (id == 0 || seg_id(keys, n, iend) != id) return;  // padding row, or the run ends here
  // the run began in an earlier chunk: that chunk joins it
  if (seg_id(keys, n, i0) == id && seg_id(keys, n, i0 - 1) == id) return;
  const int tid = threadIdx.x;
  if (tid * 4 >= H) return;
  f32x4 acc = *reinterpret_cast<const f32x4*>(parts + (c * 2 + 1) * H + 4 * tid);
  for (int64_t cc = c + 1; cc * SEG_C < n; ++cc) {
    acc += *reinterpret_cast<const f32x4*>(parts + (cc * 2 + 0) * H + 4 * tid);
    const int64_t e = min(n, (cc + 1) * SEG_C);
    if (seg_id(keys, n, e - 1) != id || seg_id(keys, n, e) != id) break;
  }
  f32x4* t = reinterpret_cast<f32x4*>(table + (int64_t)id * H + 4 * tid);
  *t = *t + acc;
}

size_t table_scatter_sort_bytes(int64_t n) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_keys(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                           (unsigned int)n, 0, 64);
  return bytes;
}

// workspace (bytes): 2 n keys + the sort's scratch + [nch][2][H] fp32 pieces
int64_t table_scatter_det_bytes(int64_t n, int H) {
  const int64_t nch = (n + SEG_C - 1) / SEG_C;
  return 16 * n + (((int64_t)table_scatter_sort_bytes(n) + 15) & ~15ll) + nch * 2 * H * 4;
}

mmseq_status table_scatter_det(int64_t n, int H, const int64_t* ids, const float* de, float* table,
                               void* ws, hipStream_t s) {
  if (n == 0) return MMSEQ_OK;
  const int64_t nch = (n + SEG_C - 1) / SEG_C;
  uint64_t* kin = reinterpret_cast<uint64_t*>(ws);
  uint64_t* kout = kin + n;
  size_t bytes = table_scatter_sort_bytes(n);
  void* tmp = kout + n;
  float* parts = reinterpret_cast<float*>(reinterpret_cast<char*>(tmp) + ((bytes + 15) & ~size_t(15)));
  hipLaunchKernelGGL(row_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, ids, kin);
  if (rocprim::radix_sort_keys(tmp, bytes, (const uint64_t*)kin, kout, (unsigned int)n, 0, 64, s) !=
      hipSuccess)
    return mmseq_set_error(MMSEQ_EHIP, "embed_bwd: radix sort failed");
  hipLaunchKernelGGL(seg_rows_kernel, dim3((unsigned)nch), dim3(256), 0, s, n, H, kout, de, table, parts);
  hipLaunchKernelGGL(seg_join_kernel, dim3((unsigned)nch), dim3(256), 0, s, n, H, kout, table, parts);
  return mmseq_check_launch("embed_bwd table scatter");
}

// ---------------------------------------------------------------------------------------------
// ViT patch path
// ---------------------------------------------------------------------------------------------
// Any patch size: one workgroup (64 lanes) per patch row; lane t < 3 ps copies the ps pixels of
// (channel t / ps, kernel row t % ps) — contiguous in the image — and the columns K .. ldk - 1 are
// zero-filled (K padded to the GEMM's K granularity, e.g. 588 -> 640 for ViT-L/14).
template <typename T>
__global__ __launch_bounds__(64) void im2col_kernel(int64_t rows, int N, int npair, int R, int ps,
                                                    int64_t ldk, const float* __restrict__ images,
                                                    const int64_t* __restrict__ pairs,
                                                    T* __restrict__ out) {
  const int g = R / ps, gg = g * g, K = 3 * ps * ps;
  const int64_t row = blockIdx.x;
  if (row >= rows) return;
  const int patch = (int)(row % gg);
  const int64_t rest = row / gg;
  const int s = (int)(rest & 1);
  const int64_t pj = rest >> 1;
  const int b = (int)(pj / npair);
  const int img = (int)pairs[pj * 2 + s];
  const int py = patch / g, px = patch % g;
  const float* src_img = images + ((int64_t)b * N + img) * 3 * R * R;
  T* dst = out + row * ldk;
  for (int t = threadIdx.x; t < 3 * ps; t += 64) {
    const int c = t / ps, ky = t % ps;
    const float* src = src_img + ((int64_t)c * R + py * ps + ky) * R + px * ps;
    T* d = dst + (c * ps + ky) * ps;
    for (int kx = 0; kx < ps; ++kx) Elem<T>::st(d + kx, src[kx]);
  }
  for (int col = K + threadIdx.x; col < ldk; col += 64) Elem<T>::st(dst + col, 0.f);
}

// bf16 patches: one row per 96 threads, 8 consecutive pixels of one (channel, patch row) per
// thread (two 16-byte loads, one 16-byte store); the row's pair / image decode is done once
// per row instead of per element (64-bit divisions). Requires ps % 8 == 0 and ldk == K.
__global__ __launch_bounds__(192) void im2col_bf16_kernel(int64_t rows, int N, int npair, int R,
                                                         int ps, const float* __restrict__ images,
                                                         const int64_t* __restrict__ pairs,
                                                         unsigned short* __restrict__ out) {
  const int g = R / ps, gg = g * g, K = 3 * ps * ps;
  const int64_t row = (int64_t)blockIdx.x * 2 + threadIdx.x / 96;
  const int chunk = threadIdx.x % 96;
  if (row >= rows) return;
  const int patch = (int)(row % gg);
  const int64_t rest = row / gg;
  const int s = (int)(rest & 1);
  const int64_t pj = rest >> 1;
  const int b = (int)(pj / npair);
  const int img = (int)pairs[pj * 2 + s];
  const int py = patch / g, px = patch % g;
  const float* src_img = images + ((int64_t)b * N + img) * 3 * R * R;
  for (int c8 = chunk; c8 * 8 < K; c8 += 96) {
    const int col = c8 * 8;
    const int c = col / (ps * ps), ky = (col / ps) % ps, kx = col % ps;
    const float* src = src_img + ((int64_t)c * R + py * ps + ky) * R + px * ps + kx;
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(src);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + 4);
    u16x8 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      o[r] = f2bf(v0[r]);
      o[4 + r] = f2bf(v1[r]);
    }
    *reinterpret_cast<u16x8*>(out + row * K + col) = o;
  }
}

__device__ __forceinline__ int vit_pos_row(int t, int gg) {
  // clip/model.py:271-275 with img_len = 2: rows 0..gg for CLS + img0, rows 0..gg-1 for img1
  return t <= gg ? t : t - gg - 1;
}

template <typename T>
__global__ __launch_bounds__(256) void vit_embed_fwd_kernel(int P, int ntok, int W, int gg,
                                                            const T* __restrict__ patch_out,
                                                            const float* __restrict__ cls,
                                                            const float* __restrict__ pos,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            float eps, T* __restrict__ x,
                                                            T* __restrict__ y,
                                                            float* __restrict__ mean,
                                                            float* __restrict__ rstd) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= (int64_t)P * ntok) return;
  const int p = r / ntok, t = r % ntok;
  const float* pr = pos + (int64_t)vit_pos_row(t, gg) * W;
  const T* src = t > 0 ? patch_out + ((int64_t)p * (ntok - 1) + (t - 1)) * W : nullptr;
  float v[MAXV], s = 0.f;
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    int c = j * 64 + lane;
    float a = 0.f;
    if (c < W) a = (t == 0 ? cls[c] : Elem<T>::ld(src + c)) + pr[c];
    v[j] = a;
    s += a;
  }
  T* xr = x + r * W;
  T* yr = y + r * W;
  // the stored pre-LN x is the rounded value; statistics use the same rounded values so that the
  // backward (which re-reads x) sees a consistent input
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    int c = j * 64 + lane;
    if (c < W) {
      Elem<T>::st(xr + c, v[j]);
      v[j] = Elem<T>::ld(xr + c);
    }
  }
  s = 0.f;
#pragma unroll
  for (int j = 0; j < MAXV; ++j) s += (j * 64 + lane < W) ? v[j] : 0.f;
  const float mu = wave_sum(s) / W;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    int c = j * 64 + lane;
    float d = c < W ? v[j] - mu : 0.f;
    q += d * d;
  }
  const float rs = rsqrtf(wave_sum(q) / W + eps);
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    int c = j * 64 + lane;
    if (c < W) Elem<T>::st(yr + c, (v[j] - mu) * rs * gamma[c] + beta[c]);
  }
  if (lane == 0) {
    mean[r] = mu;
    rstd[r] = rs;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void vit_embed_bwd_kernel(int P, int ntok, int W,
                                                            const T* __restrict__ dy,
                                                            const T* __restrict__ x,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma,
                                                            T* __restrict__ dpatch,
                                                            float* __restrict__ dx0,
                                                            float* __restrict__ ws_ln) {
  __shared__ float red[4][2][1024];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t rows = (int64_t)P * ntok;
  float pg[MAXV], pb[MAXV];
#pragma unroll
  for (int j = 0; j < MAXV; ++j) pg[j] = pb[j] = 0.f;
  const int64_t rbeg = (int64_t)blockIdx.x * RPB;
  for (int64_t r = rbeg + wave; r < rbeg + RPB && r < rows; r += 4) {
    const int p = r / ntok, t = r % ntok;
    const T* xr = x + r * W;
    const T* dyr = dy + r * W;
    const float mu = mean[r], rs = rstd[r];
    float xh[MAXV], gdy[MAXV], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
      int c = j * 64 + lane;
      if (c < W) {
        float xv = (Elem<T>::ld(xr + c) - mu) * rs;
        float d = Elem<T>::ld(dyr + c);
        xh[j] = xv;
        gdy[j] = d * gamma[c];
        pg[j] += d * xv;
        pb[j] += d;
        s1 += gdy[j];
        s2 += gdy[j] * xv;
      } else {
        xh[j] = gdy[j] = 0.f;
      }
    }
    s1 = wave_sum(s1) / W;
    s2 = wave_sum(s2) / W;
#pragma unroll
    for (int j = 0; j < MAXV; ++j) {
      int c = j * 64 + lane;
      if (c < W) {
        float d = rs * (gdy[j] - s1 - xh[j] * s2);
        if (t == 0) dx0[(int64_t)p * W + c] = d;
        else Elem<T>::st(dpatch + ((int64_t)p * (ntok - 1) + t - 1) * W + c, d);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < MAXV; ++j) {
    int c = j * 64 + lane;
    if (c < W) {
      red[wave][0][c] = pg[j];
      red[wave][1][c] = pb[j];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < W; c += 256) {
    ws_ln[((int64_t)blockIdx.x * 2 + 0) * W + c] =
        red[0][0][c] + red[1][0][c] + red[2][0][c] + red[3][0][c];
    ws_ln[((int64_t)blockIdx.x * 2 + 1) * W + c] =
        red[0][1][c] + red[1][1][c] + red[2][1][c] + red[3][1][c];
  }
}

// dpos / dcls reductions over pairs (deterministic, fixed order)
template <typename T>
__global__ __launch_bounds__(256) void vit_pos_kernel(int P, int ntok, int W, int gg,
                                                      const T* __restrict__ dpatch,
                                                      const float* __restrict__ dx0,
                                                      float* __restrict__ dcls,
                                                      float* __restrict__ dpos) {
  const int r = blockIdx.y;  // 0..gg  (gg+1 = cls row)
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= W) return;
  const int64_t ps = (int64_t)(ntok - 1) * W;
  float s = 0.f;
  if (r == gg + 1) {
    for (int p = 0; p < P; ++p) s += dx0[(int64_t)p * W + c];
    dcls[c] += s;
    return;
  }
  // tokens t with vit_pos_row(t) == r: t = r (if r <= gg) and t = r + gg + 1 (if r < gg)
  for (int p = 0; p < P; ++p) {
    const T* dp = dpatch + p * ps;
    if (r == 0) s += dx0[(int64_t)p * W + c];
    else s += Elem<T>::ld(dp + (int64_t)(r - 1) * W + c);
    if (r < gg && r + gg + 1 < ntok) s += Elem<T>::ld(dp + (int64_t)(r + gg) * W + c);
  }
  dpos[(int64_t)r * W + c] += s;
}

// ---- bf16 ViT embedding, W = 256 NJ: half-wave rows, 16-byte accesses (the layout of
// layernorm.hip's ln_fwd16 / ln_bwd16): lane l of a half-wave owns columns (j * 32 + l) * 8 .. +7
__device__ __forceinline__ float hsum32(float v) {  // sum over the 32 lanes of a half-wave
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int NJ>
__global__ __launch_bounds__(256) void vit_embed_fwd16_kernel(int P, int ntok, int gg,
                                                              const us* __restrict__ patch_out,
                                                              const float* __restrict__ cls,
                                                              const float* __restrict__ pos,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              float eps, us* __restrict__ x,
                                                              us* __restrict__ y,
                                                              float* __restrict__ mean,
                                                              float* __restrict__ rstd) {
  constexpr int W = 256 * NJ;
  const int l = threadIdx.x & 31;
  const int64_t r = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  if (r >= (int64_t)P * ntok) return;
  const int p = (int)(r / ntok), t = (int)(r - (int64_t)p * ntok);
  const float* pr = pos + (int64_t)vit_pos_row(t, gg) * W;
  const us* src = patch_out + ((int64_t)p * (ntok - 1) + (t > 0 ? t - 1 : 0)) * W;
  u16x8 raw[NJ];
  if (t > 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) raw[j] = *reinterpret_cast<const u16x8*>(src + (j * 32 + l) * 8);
  }
  // x = bf16(patch + pos) (the class row: bf16(cls + pos)); the statistics use the rounded values
  // the backward re-reads
  float v[NJ][8], s = 0.f;
  us* xr = x + r * W;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = (j * 32 + l) * 8;
    const f32x4 p0 = *reinterpret_cast<const f32x4*>(pr + c), p1 = *reinterpret_cast<const f32x4*>(pr + c + 4);
    float a[8];
    if (t > 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = bf2f(raw[j][e]);
    } else {
      const f32x4 c0 = *reinterpret_cast<const f32x4*>(cls + c), c1 = *reinterpret_cast<const f32x4*>(cls + c + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[e] = c0[e];
        a[4 + e] = c1[e];
      }
    }
    u16x8 xb;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      xb[e] = f2bf(a[e] + (e < 4 ? p0[e] : p1[e - 4]));
      v[j][e] = bf2f(xb[e]);
      s += v[j][e];
    }
    *reinterpret_cast<u16x8*>(xr + c) = xb;
  }
  const float mu = hsum32(s) / W;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = v[j][e] - mu;
      q = fmaf(d, d, q);
    }
  const float rs = rsqrtf(hsum32(q) / W + eps);
  us* yr = y + r * W;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = (j * 32 + l) * 8;
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + c), g1 = *reinterpret_cast<const f32x4*>(gamma + c + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + c), b1 = *reinterpret_cast<const f32x4*>(beta + c + 4);
    u16x8 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o[e] = f2bf(fmaf((v[j][e] - mu) * rs, g0[e], b0[e]));
      o[4 + e] = f2bf(fmaf((v[j][4 + e] - mu) * rs, g1[e], b1[e]));
    }
    *reinterpret_cast<u16x8*>(yr + c) = o;
  }
  if (l == 0) {
    mean[r] = mu;
    rstd[r] = rs;
  }
}

// backward of ln_pre + the embedding sum: RPB rows per block (8 half-waves, RPB / 8 rows each),
// dx of the class rows to dx0 (fp32, [P][W]), of the patch rows to dpatch (bf16, the conv GEMM's
// dY); per-block dgamma / dbeta partials -> ws_ln[block][2][W] (reduced in block order)
template <int NJ>
__global__ __launch_bounds__(256) void vit_embed_bwd16_kernel(int P, int ntok,
                                                              const us* __restrict__ dy,
                                                              const us* __restrict__ x,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ rstd,
                                                              const float* __restrict__ gamma,
                                                              us* __restrict__ dpatch,
                                                              float* __restrict__ dx0,
                                                              float* __restrict__ ws_ln) {
  constexpr int W = 256 * NJ;
  __shared__ float red[4][2][W];
  const int l = threadIdx.x & 31, hw = threadIdx.x >> 5;
  const int64_t rows = (int64_t)P * ntok;
  float pg[NJ][8], pb[NJ][8], gm[NJ][8];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = (j * 32 + l) * 8;
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + c), g1 = *reinterpret_cast<const f32x4*>(gamma + c + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      gm[j][e] = g0[e];
      gm[j][4 + e] = g1[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) pg[j][e] = pb[j][e] = 0.f;
  }
  const int64_t rbeg = (int64_t)blockIdx.x * RPB;
  for (int64_t r = rbeg + hw; r < rbeg + RPB && r < rows; r += 8) {
    const int p = (int)(r / ntok), t = (int)(r - (int64_t)p * ntok);
    const us* xr = x + r * W;
    const us* dyr = dy + r * W;
    u16x8 xa[NJ], da[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      xa[j] = *reinterpret_cast<const u16x8*>(xr + (j * 32 + l) * 8);
      da[j] = *reinterpret_cast<const u16x8*>(dyr + (j * 32 + l) * 8);
    }
    const float mu = mean[r], rs = rstd[r];
    float xh[NJ][8], gdy[NJ][8], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xv = (bf2f(xa[j][e]) - mu) * rs, d = bf2f(da[j][e]);
        xh[j][e] = xv;
        gdy[j][e] = d * gm[j][e];
        pg[j][e] += d * xv;
        pb[j][e] += d;
        s1 += gdy[j][e];
        s2 += gdy[j][e] * xv;
      }
    s1 = hsum32(s1) / W;
    s2 = hsum32(s2) / W;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int c = (j * 32 + l) * 8;
      float d[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = rs * (gdy[j][e] - s1 - xh[j][e] * s2);
      if (t == 0) {
        float* o = dx0 + (int64_t)p * W + c;
        *reinterpret_cast<f32x4*>(o) = (f32x4){d[0], d[1], d[2], d[3]};
        *reinterpret_cast<f32x4*>(o + 4) = (f32x4){d[4], d[5], d[6], d[7]};
      } else {
        u16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = f2bf(d[e]);
        *reinterpret_cast<u16x8*>(dpatch + ((int64_t)p * (ntok - 1) + t - 1) * W + c) = o;
      }
    }
  }
  // the two half-waves of a wave own the same columns: combine them, then the 4 waves in order
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      pg[j][e] += __shfl_xor(pg[j][e], 32, 64);
      pb[j][e] += __shfl_xor(pb[j][e], 32, 64);
    }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 32) == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = (j * 32 + l) * 8 + e;
        red[wave][0][c] = pg[j][e];
        red[wave][1][c] = pb[j][e];
      }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < W; c += 256) {
    ws_ln[((int64_t)blockIdx.x * 2 + 0) * W + c] = red[0][0][c] + red[1][0][c] + red[2][0][c] + red[3][0][c];
    ws_ln[((int64_t)blockIdx.x * 2 + 1) * W + c] = red[0][1][c] + red[1][1][c] + red[2][1][c] + red[3][1][c];
  }
}

// dpos / dcls from the column sums over pairs: sp = sum_p dpatch[p] ((ntok - 1) x W), s0 = sum_p dx0[p]
// (W); pos row r collects token r (r <= gg: the class row for r = 0) and token r + gg + 1 (r < gg)
__global__ __launch_bounds__(256) void vit_pos_fold_kernel(int W, int gg, const float* __restrict__ sp,
                                                           const float* __restrict__ s0,
                                                           float* __restrict__ dcls,
                                                           float* __restrict__ dpos) {
  const int r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= W) return;
  if (r == gg + 1) {
    dcls[c] += s0[c];
    return;
  }
  float v = r == 0 ? s0[c] : sp[(int64_t)(r - 1) * W + c];
  if (r < gg) v += sp[(int64_t)(r + gg) * W + c];
  dpos[(int64_t)r * W + c] += v;
}

}  // namespace

extern "C" mmseq_status mmseq_embed_ln_fwd(int P, int Lt, int H, const int64_t* ids,
                                           const int64_t* tt, const float* word, const float* pos,
                                           const float* type, const float* gamma,
                                           const float* beta, float eps, void* joint,
                                           int64_t ld_pair, float* mean, float* rstd,
                                           mmseq_dtype dtype, const mmseq_dropout* drop,
                                           mmseq_stream stream) {
  MMSEQ_REQUIRE(P >= 0 && Lt > 0 && H > 0 && H <= 1024, "embed: bad sizes");
  MMSEQ_REQUIRE(ids && word && pos && type && gamma && beta && joint && mean && rstd,
                "embed: null buffer");
  if (P == 0) return MMSEQ_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  dim3 grid((unsigned)(((int64_t)P * Lt + 3) / 4));
  if (dtype == MMSEQ_F32)
    hipLaunchKernelGGL(embed_fwd_kernel<float>, grid, dim3(256), 0, s, P, Lt, H, ids, tt, word,
                       pos, type, gamma, beta, eps, (float*)joint, ld_pair, mean, rstd,
                       make_drop(drop));
  else
    hipLaunchKernelGGL(embed_fwd_kernel<unsigned short>, grid, dim3(256), 0, s, P, Lt, H, ids, tt,
                       word, pos, type, gamma, beta, eps, (unsigned short*)joint, ld_pair, mean,
                       rstd, make_drop(drop));
  return mmseq_check_launch("embed_ln_fwd");
}

extern "C" int64_t mmseq_embed_ln_bwd_workspace(int P, int Lt, int H) {
  return mmseq_plan::embed_ln_bwd_layout(P, Lt, H, table_scatter_det_bytes((int64_t)P * Lt, H)).total;
}

extern "C" mmseq_status mmseq_embed_ln_bwd(int P, int Lt, int H, const int64_t* ids,
                                           const int64_t* tt, const float* word, const float* pos,
                                           const float* type, const float* gamma,
                                           const float* mean, const float* rstd,
                                           const void* djoint, int64_t ld_pair, float* dword,
                                           float* dpos, float* dtype_tab, float* dgamma,
                                           float* dbeta, float* workspace, mmseq_dtype dtype,
                                           const mmseq_dropout* drop, mmseq_stream stream) {
  MMSEQ_REQUIRE(P >= 0 && Lt > 0 && H > 0 && H <= 1024 && H % 4 == 0, "embed_bwd: bad sizes");
  MMSEQ_REQUIRE((((uintptr_t)workspace) & 15) == 0, "embed_bwd: workspace not 16-byte aligned");
  MMSEQ_REQUIRE(workspace && djoint && dword && dpos, "embed_bwd: null buffer");
  // the table scatter reads and writes 16-byte rows of dword / dtype_tab (f32x4 at id * H + 4 t)
  MMSEQ_REQUIRE((((uintptr_t)dword) & 15) == 0 && (((uintptr_t)dtype_tab) & 15) == 0,
                "embed_bwd: dword / dtype_tab not 16-byte aligned");
  // sort keys pack (id, row) into 32 bits each; 0xFFFFFFFF is the no-run sentinel
  MMSEQ_REQUIRE((int64_t)P * Lt < (1ll << 32) - 1, "embed_bwd: too many rows");
  if (P == 0) return MMSEQ_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t rows = (int64_t)P * Lt;
  const mmseq_plan::EmbedLnBwdLayout wl =
      mmseq_plan::embed_ln_bwd_layout(P, Lt, H, table_scatter_det_bytes(rows, H));
  const int nb = wl.nb;
  float* ws_de = workspace + wl.de;
  float* ws_ln = workspace + wl.ln;
  if (dtype == MMSEQ_F32)
    hipLaunchKernelGGL(embed_bwd_kernel<float>, dim3(nb), dim3(256), 0, s, P, Lt, H, ids, tt,
                       word, pos, type, gamma, mean, rstd, (const float*)djoint, ld_pair,
                       ws_de, ws_ln, make_drop(drop));
  else
    hipLaunchKernelGGL(embed_bwd_kernel<unsigned short>, dim3(nb), dim3(256), 0, s, P, Lt, H, ids,
                       tt, word, pos, type, gamma, mean, rstd, (const unsigned short*)djoint,
                       ld_pair, ws_de, ws_ln, make_drop(drop));
  mmseq_status st = mmseq_check_launch("embed_ln_bwd");
  if (st) return st;
  {  // word / token-type tables: fixed-order sums per id (no float atomics)
    void* tws = workspace + wl.scatter;
    st = table_scatter_det(rows, H, ids, ws_de, dword, tws, s);
    if (st) return st;
    if (tt && dtype_tab) {
      st = table_scatter_det(rows, H, tt, ws_de, dtype_tab, tws, s);
      if (st) return st;
    }
  }
  // dpos[t] += sum_p de[p][t] for t >= 1 (row 0 = padding_idx): a deterministic column sum over the
  // P pairs of de viewed as [P][Lt * H] (a sequential loop over P per column was latency-bound)
  if (Lt > 1) {
    st = mmseq_colsum(P, (Lt - 1) * H, ws_de + H, (int64_t)Lt * H, dpos + H, 1, workspace + wl.cs,
                      MMSEQ_F32, stream);
    if (st) return st;
  }
  return ln_reduce_partials(nb, H, ws_ln, dgamma, dbeta, s);
}

extern "C" mmseq_status mmseq_vit_im2col(int B, int N, int npair, int R, int ps,
                                         const float* images, const int64_t* pairs, void* patches,
                                         int64_t ld_patch, mmseq_dtype dtype, mmseq_stream stream) {
  MMSEQ_REQUIRE(B >= 0 && N > 0 && npair > 0 && ps > 0 && R % ps == 0, "im2col: bad sizes");
  MMSEQ_REQUIRE(images && pairs && patches, "im2col: null buffer");
  MMSEQ_REQUIRE(ld_patch >= 3 * ps * ps, "im2col: ld_patch < 3 ps^2");
  if (B == 0) return MMSEQ_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t rows = (int64_t)B * npair * 2 * (R / ps) * (R / ps);
  MMSEQ_REQUIRE(rows < (1ll << 31), "im2col: too many patches");
  if (dtype == MMSEQ_BF16 && ps % 8 == 0 && R % 4 == 0 && ld_patch == 3 * ps * ps &&
      (((uintptr_t)images) & 15) == 0 && (((uintptr_t)patches) & 15) == 0) {
    hipLaunchKernelGGL(im2col_bf16_kernel, dim3((unsigned)((rows + 1) / 2)), dim3(192), 0, s, rows, N,
                       npair, R, ps, images, pairs, (unsigned short*)patches);
  } else if (dtype == MMSEQ_F32) {
    hipLaunchKernelGGL(im2col_kernel<float>, dim3((unsigned)rows), dim3(64), 0, s, rows, N, npair,
                       R, ps, ld_patch, images, pairs, (float*)patches);
  } else {
    hipLaunchKernelGGL(im2col_kernel<unsigned short>, dim3((unsigned)rows), dim3(64), 0, s, rows, N,
                       npair, R, ps, ld_patch, images, pairs, (unsigned short*)patches);
  }
  return mmseq_check_launch("vit_im2col");
}

static bool vit_vec16(const void* a, const void* b, const void* c, const void* d, const void* e,
                      const void* f, const void* g) {
  const uintptr_t o = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e |
                      (uintptr_t)f | (uintptr_t)g;
  return (o & 15) == 0;
}

extern "C" mmseq_status mmseq_vit_embed_fwd(int P, int ntok, int W, int npatch_img,
                                            const void* patch_out, const float* cls,
                                            const float* pos, const float* gamma,
                                            const float* beta, float eps, void* x, void* y,
                                            float* mean, float* rstd, mmseq_dtype dtype,
                                            mmseq_stream stream) {
  MMSEQ_REQUIRE(P >= 0 && W > 0 && W <= 1024 && ntok == 1 + 2 * npatch_img,
                "vit_embed: requires img_len = 2 (ntok = 1 + 2*npatch) and W <= 1024");
  if (P == 0) return MMSEQ_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == MMSEQ_BF16 && W % 256 == 0 && vit_vec16(patch_out, x, y, cls, pos, gamma, beta)) {
    const dim3 g8((unsigned)(((int64_t)P * ntok + 7) / 8));
#define VEF(NJ) hipLaunchKernelGGL(vit_embed_fwd16_kernel<NJ>, g8, dim3(256), 0, s, P, ntok, npatch_img, \
                                   (const us*)patch_out, cls, pos, gamma, beta, eps, (us*)x, (us*)y, mean, rstd)
    switch (W / 256) { case 1: VEF(1); break; case 2: VEF(2); break; case 3: VEF(3); break; default: VEF(4); }
#undef VEF
    return mmseq_check_launch("vit_embed_fwd");
  }
  dim3 grid((unsigned)(((int64_t)P * ntok + 3) / 4));
  if (dtype == MMSEQ_F32)
    hipLaunchKernelGGL(vit_embed_fwd_kernel<float>, grid, dim3(256), 0, s, P, ntok, W, npatch_img,
                       (const float*)patch_out, cls, pos, gamma, beta, eps, (float*)x, (float*)y,
                       mean, rstd);
  else
    hipLaunchKernelGGL(vit_embed_fwd_kernel<unsigned short>, grid, dim3(256), 0, s, P, ntok, W,
                       npatch_img, (const unsigned short*)patch_out, cls, pos, gamma, beta, eps,
                       (unsigned short*)x, (unsigned short*)y, mean, rstd);
  return mmseq_check_launch("vit_embed_fwd");
}

extern "C" int64_t mmseq_vit_embed_bwd_workspace(int P, int ntok, int W) {
  return mmseq_plan::vit_embed_bwd_layout(P, ntok, W).total;
}

extern "C" mmseq_status mmseq_vit_embed_bwd(int P, int ntok, int W, int npatch_img,
                                            const void* dy, const void* x, const float* mean,
                                            const float* rstd, const float* gamma,
                                            void* dpatch_out, float* dcls, float* dpos,
                                            float* dgamma, float* dbeta, float* workspace,
                                            mmseq_dtype dtype, mmseq_stream stream) {
  MMSEQ_REQUIRE(P >= 0 && W > 0 && W <= 1024 && ntok == 1 + 2 * npatch_img, "vit_embed_bwd: sizes");
  MMSEQ_REQUIRE(dy && x && dpatch_out && dcls && dpos && workspace, "vit_embed_bwd: null buffer");
  if (P == 0) return MMSEQ_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const mmseq_plan::VitEmbedBwdLayout wl = mmseq_plan::vit_embed_bwd_layout(P, ntok, W);
  const int nb = wl.nb;
  float* dx0 = workspace + wl.dx0;
  float* ws_ln = workspace + wl.ln;
  dim3 gpos((W + 255) / 256, npatch_img + 2);
  if (dtype == MMSEQ_F32) {
    hipLaunchKernelGGL(vit_embed_bwd_kernel<float>, dim3(nb), dim3(256), 0, s, P, ntok, W,
                       (const float*)dy, (const float*)x, mean, rstd, gamma, (float*)dpatch_out,
                       dx0, ws_ln);
    hipLaunchKernelGGL(vit_pos_kernel<float>, gpos, dim3(256), 0, s, P, ntok, W, npatch_img,
                       (const float*)dpatch_out, dx0, dcls, dpos);
  } else if (W % 256 == 0 && vit_vec16(dy, x, dpatch_out, gamma, dx0, nullptr, nullptr)) {
    // 16-byte rows; dpos / dcls from deterministic column sums over the P pairs (a sequential loop
    // over P per column was latency-bound: 557 us at config 3)
#define VEB(NJ) hipLaunchKernelGGL(vit_embed_bwd16_kernel<NJ>, dim3(nb), dim3(256), 0, s, P, ntok, \
                                   (const us*)dy, (const us*)x, mean, rstd, gamma, (us*)dpatch_out, dx0, ws_ln)
    switch (W / 256) { case 1: VEB(1); break; case 2: VEB(2); break; case 3: VEB(3); break; default: VEB(4); }
#undef VEB
    mmseq_status st = mmseq_check_launch("vit_embed_bwd");
    if (st) return st;
    float *sp = workspace + wl.sp, *s0 = workspace + wl.s0, *cws = workspace + wl.cs;
    st = mmseq_colsum(P, (ntok - 1) * W, dpatch_out, (int64_t)(ntok - 1) * W, sp, 0, cws, MMSEQ_BF16,
                      stream);
    if (st) return st;
    st = mmseq_colsum(P, W, dx0, W, s0, 0, cws, MMSEQ_F32, stream);
    if (st) return st;
    hipLaunchKernelGGL(vit_pos_fold_kernel, gpos, dim3(256), 0, s, W, npatch_img, sp, s0, dcls, dpos);
    st = mmseq_check_launch("vit_pos_fold");
    if (st) return st;
    return ln_reduce_partials(nb, W, ws_ln, dgamma, dbeta, s);
  } else {
    hipLaunchKernelGGL(vit_embed_bwd_kernel<unsigned short>, dim3(nb), dim3(256), 0, s, P, ntok,
                       W, (const unsigned short*)dy, (const unsigned short*)x, mean, rstd, gamma,
                       (unsigned short*)dpatch_out, dx0, ws_ln);
    hipLaunchKernelGGL(vit_pos_kernel<unsigned short>, gpos, dim3(256), 0, s, P, ntok, W,
                       npatch_img, (const unsigned short*)dpatch_out, dx0, dcls, dpos);
  }
  mmseq_status st = mmseq_check_launch("vit_embed_bwd");
  if (st) return st;
  return ln_reduce_partials(nb, W, ws_ln, dgamma, dbeta, s);
}
