// Mask loss of the spatial task: TimesformerUniversalVideoInstanceSegmentationHead.forward, training branch
// (reference modeling:1829-1916) — cosine logits of every patch token against a label table, bilinear upsample of the
// [T, L, P, P] patch logits to the mask size (F.interpolate, align_corners=False) and a per-pixel cross-entropy with
// ignore_index = -1 — WITHOUT the upsampled tensor: a pixel's logit vector is a bilinear mix of at most four patch
// logit vectors, so one workgroup per (clip, frame, patch row) walks the pixel rows within one patch pitch of its row
// and keeps the row-interpolated logits of the current pixel row ([P, L] floats, 7 KB) in LDS.
//
//   (a) sf_mask_sim_kernel     c[row, l] = <x_row / |x_row|, E_l>                      fp32 FMAs, 8 rows per workgroup
//   (b) sf_mask_pixel_kernel   per pixel: logsumexp - logit[target]; gradient wrt the patch logits in GATHER form:
//                              thread (px, l) owns dz[py, px, l] and sums the pixels that touch patch (py, px) itself,
//                              in pixel order.  No atomics; every output element has one owner.
//   (c) sf_mask_finish_kernel  per-clip sums of the workgroup partials in a fixed order -> 1 / (valid pixels * B),
//                              loss, d logit_scale, d logit_bias
//   (d) sf_mask_dx_kernel      dz -> dx through the normalisation
// Everything a call needs lives in the caller's workspace (patch similarities, their gradient, 1 / |x|, partials): its
// size grows with B T N L, never with T L H W.  Results are bit-reproducible.
#include "sf_common.h"
#include "sf_internal.h"

#define SF_ML_CLIPS 16        // clips per launch (their tables / masks / sizes travel by value)
#define SF_ML_MAXP 14         // patches per side: N <= 224 -> P <= 14
#define SF_ML_MAXL 128
#define SF_ML_SLOTS 7         // (px, l) pairs per thread: 14 * 128 / 256
#define SF_ML_MAXW 2048
#define SF_ML_ROWS 8          // token rows per workgroup in (a) and (d)
#define SF_ML_MAXD 2048

struct SfMaskClips {
  const float* emb[SF_ML_CLIPS];   // [L, D]
  const int* mask[SF_ML_CLIPS];    // [T, H, W]
  int L[SF_ML_CLIPS];
  int W[SF_ML_CLIPS];
};

__device__ float ml_block_sum(float v, float* red) {
  v = wave_sum_dpp(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}

// PyTorch's source index of a bilinear resize with align_corners=False (area_pixel_compute_source_index): the lower neighbour,
// the upper one clamped to in - 1, and the weight of the upper one
SF_DEVICE void ml_src(int dst, float scale, int in, int& i0, int& i1, float& lam) {
  const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
  i0 = min((int)src, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  lam = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}

// (a) grid (ceil(T N / 8), clips).  The 8 rows sit in LDS; wave w takes labels w, w + 4, ...: one pass over E_l serves all 8 rows.
__global__ __launch_bounds__(256) void sf_mask_sim_kernel(SfMaskClips clips, int clip0, const float* __restrict__ x, int rows, int D,
                                                          size_t clip_stride, float* __restrict__ sim, float* __restrict__ inv_norm) {
  extern __shared__ float xs[];      // [8][D]
  __shared__ float inorm[SF_ML_ROWS];
  const int ci = blockIdx.y, clip = clip0 + ci, L = clips.L[ci];
  const int r0 = blockIdx.x * SF_ML_ROWS, nr = min(SF_ML_ROWS, rows - r0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* xc = x + ((size_t)clip * rows + r0) * D;
  for (int e = threadIdx.x; e < SF_ML_ROWS * D; e += 256) xs[e] = e < nr * D ? xc[e] : 0.f;
  __syncthreads();
  for (int r = wave; r < SF_ML_ROWS; r += 4) {
    float a = 0.f;
    for (int d = lane; d < D; d += 64) a = fmaf(xs[r * D + d], xs[r * D + d], a);
    a = wave_sum_dpp(a);
    if (lane == 0) inorm[r] = 1.f / sqrtf(a);
  }
  __syncthreads();
  if (threadIdx.x < nr) inv_norm[(size_t)clip * rows + r0 + threadIdx.x] = inorm[threadIdx.x];
  const float* E = clips.emb[ci];
  float* out = sim + (size_t)clip * clip_stride + (size_t)r0 * L;
  for (int l = wave; l < L; l += 4) {
    float acc[SF_ML_ROWS];
#pragma unroll
    for (int r = 0; r < SF_ML_ROWS; ++r) acc[r] = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float e = E[(size_t)l * D + d];
#pragma unroll
      for (int r = 0; r < SF_ML_ROWS; ++r) acc[r] = fmaf(e, xs[r * D + d], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < SF_ML_ROWS; ++r) {
      const float v = wave_sum_dpp(acc[r]);
      if (lane == 0 && r < nr) out[(size_t)r * L + l] = v * inorm[r];
    }
  }
}

// (b) grid (P, T, clips), 256 threads.  Dynamic LDS: zy [P L] | lam_x [W] | max_x [W] | isum_x [W] | x0_x [W] | tgt_x [W] | xlo [16] | xhi [16].
// partial[((clip T + t) 16 + py) 4 + {0 loss sum, 1 valid pixels, 2 sum dz, 3 sum dz c}]: loss and count belong to the workgroup
// of a pixel row's LOWER neighbour patch row, so every pixel is counted once.
__global__ __launch_bounds__(256) void sf_mask_pixel_kernel(SfMaskClips clips, int clip0, const float* __restrict__ sim, float* __restrict__ dz,
                                                            float* __restrict__ partial, const float* __restrict__ logit_scale_p,
                                                            const float* __restrict__ logit_bias_p, int T, int P, int H, size_t clip_stride,
                                                            int need_grad) {
  extern __shared__ float sm[];
  __shared__ float red[4];
  const int ci = blockIdx.z, clip = clip0 + ci, L = clips.L[ci], W = clips.W[ci];
  const int t = blockIdx.y, py = blockIdx.x, PL = P * L, tid = threadIdx.x;
  float* zy = sm;
  float* lam_x = zy + SF_ML_MAXP * SF_ML_MAXL;
  float* max_x = lam_x + W;        // row maximum and 1 / sum exp of the pixel: p_l = exp(z_l - max) / sum, so that sum_l p_l = 1 to rounding
  float* isum_x = max_x + W;       // (exp(z_l - logsumexp) would carry the rounding of the logarithm into every p_l with one sign)
  int* x0_x = (int*)(isum_x + W);
  int* tgt_x = x0_x + W;
  int* xlo = tgt_x + W;
  int* xhi = xlo + 16;
  const float s = expf(logit_scale_p[0]), bias = logit_bias_p[0];
  const float* simf = sim + (size_t)clip * clip_stride + (size_t)t * P * PL;
  const int* mask = clips.mask[ci] + (size_t)t * H * W;

  // this thread's (px, l) pairs and their logits on patch rows py - 1, py, py + 1 (clamped)
  float zr[3][SF_ML_SLOTS], cc[SF_ML_SLOTS], acc[SF_ML_SLOTS];
  int kpx[SF_ML_SLOTS], kl[SF_ML_SLOTS];
#pragma unroll
  for (int k = 0; k < SF_ML_SLOTS; ++k) {
    const int idx = tid + k * 256;
    acc[k] = 0.f; cc[k] = 0.f; kpx[k] = 0; kl[k] = 0;
    zr[0][k] = zr[1][k] = zr[2][k] = 0.f;
    if (idx < PL) {
      kpx[k] = idx / L; kl[k] = idx - kpx[k] * L;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int yy = min(max(py - 1 + r, 0), P - 1);
        const float c = simf[(size_t)yy * PL + idx];
        zr[r][k] = fmaf(s, c, bias);
        if (r == 1) cc[k] = c;
      }
    }
  }
  const float scale_x = (float)P / (float)W, scale_y = (float)P / (float)H;
  for (int x = tid; x < W; x += 256) {
    int a0, a1; float lam;
    ml_src(x, scale_x, P, a0, a1, lam);
    x0_x[x] = a0; lam_x[x] = lam;
  }
  __syncthreads();
  if (tid < P) {          // pixels that touch patch column px: contiguous, the source index is monotone
    int lo = W, hi = 0;
    for (int x = 0; x < W; ++x) {
      const int a0 = x0_x[x], a1 = a0 + (a0 < P - 1 ? 1 : 0);
      if (a0 == tid || a1 == tid) { lo = min(lo, x); hi = max(hi, x + 1); }
    }
    xlo[tid] = lo; xhi[tid] = hi;
  }
  __syncthreads();

  float loss_acc = 0.f, cnt_acc = 0.f;
  for (int y = 0; y < H; ++y) {
    int y0, y1; float lamy;
    ml_src(y, scale_y, P, y0, y1, lamy);
    if (y0 != py && y1 != py) continue;                    // workgroup-uniform
    const float wy = (y0 == py ? 1.f - lamy : 0.f) + (y1 == py ? lamy : 0.f);
    const bool own = y0 == py;
    if (wy == 0.f && !own) continue;                       // clamped top border: the upper neighbour's weight is exactly zero
    int any = 0;
    for (int x = tid; x < W; x += 256) {
      int tg = mask[(size_t)y * W + x];
      if (tg < 0 || tg >= L) tg = -1;
      tgt_x[x] = tg;
      any |= tg >= 0;
    }
    if (!__syncthreads_or(any)) continue;                  // a pixel row without a valid target adds nothing
    const bool lo_is_prev = y0 == py - 1;                  // y0 in {py - 1, py}; y1 in {py, py + 1} (or y0 at the border)
    const bool hi_is_next = y1 == py + 1;
#pragma unroll
    for (int k = 0; k < SF_ML_SLOTS; ++k) {
      const int idx = tid + k * 256;
      const float a = lo_is_prev ? zr[0][k] : zr[1][k];
      const float b = hi_is_next ? zr[2][k] : zr[1][k];
      if (idx < PL) zy[idx] = fmaf(lamy, b, (1.f - lamy) * a);
    }
    __syncthreads();
    for (int x = tid; x < W; x += 256) {
      const int tg = tgt_x[x];
      if (tg < 0) continue;
      const int a0 = x0_x[x], a1 = a0 + (a0 < P - 1 ? 1 : 0);
      const float lam = lam_x[x], w0 = 1.f - lam;
      const float* z0 = zy + a0 * L;
      const float* z1 = zy + a1 * L;
      float m = -INFINITY;
      for (int l = 0; l < L; ++l) m = fmaxf(m, fmaf(lam, z1[l], w0 * z0[l]));
      float sum = 0.f;
      for (int l = 0; l < L; ++l) sum += __expf(fmaf(lam, z1[l], w0 * z0[l]) - m);
      max_x[x] = m;
      isum_x[x] = 1.f / sum;
      if (own) { loss_acc += (m - fmaf(lam, z1[tg], w0 * z0[tg])) + logf(sum); cnt_acc += 1.f; }
    }
    __syncthreads();
    if (need_grad) {
#pragma unroll
      for (int k = 0; k < SF_ML_SLOTS; ++k) {
        if (tid + k * 256 >= PL) continue;
        const int px = kpx[k], l = kl[k];
        float a = 0.f;
        for (int x = xlo[px]; x < xhi[px]; ++x) {
          const int tg = tgt_x[x];
          if (tg < 0) continue;
          const int a0 = x0_x[x], a1 = a0 + (a0 < P - 1 ? 1 : 0);
          const float lam = lam_x[x], w0 = 1.f - lam;
          const float p = __expf(fmaf(lam, zy[a1 * L + l], w0 * zy[a0 * L + l]) - max_x[x]) * isum_x[x];
          const float w = (a0 == px ? w0 : 0.f) + (a1 == px ? lam : 0.f);
          a = fmaf(w, p - (tg == l ? 1.f : 0.f), a);
        }
        acc[k] = fmaf(wy, a, acc[k]);
      }
    }
    __syncthreads();
  }
  float sa = 0.f, sc = 0.f;
  if (need_grad) {
    float* dzf = dz + (size_t)clip * clip_stride + ((size_t)t * P + py) * PL;
#pragma unroll
    for (int k = 0; k < SF_ML_SLOTS; ++k) {
      const int idx = tid + k * 256;
      if (idx < PL) { dzf[idx] = acc[k]; sa += acc[k]; sc = fmaf(acc[k], cc[k], sc); }
    }
  }
  loss_acc = ml_block_sum(loss_acc, red);
  cnt_acc = ml_block_sum(cnt_acc, red);      // <= W pixels per row and a few dozen rows: exact in fp32
  sa = ml_block_sum(sa, red);
  sc = ml_block_sum(sc, red);
  if (tid == 0) {
    float* p = partial + (((size_t)clip * T + t) * 16 + py) * 4;
    p[0] = loss_acc; p[1] = cnt_acc; p[2] = sa; p[3] = sc;
  }
}

// (c) one wave: per clip, lane-strided sums of the workgroup partials + the DPP tree (fixed order); the valid-pixel count is added as
// an integer.  clip_scale[i] = 1 / (count_i B), 0 for a clip without a valid pixel (loss 0, no gradient, still counted in the mean).
__global__ __launch_bounds__(64) void sf_mask_finish_kernel(const float* __restrict__ partial, int B, int T, int P,
                                                            const float* __restrict__ logit_scale_p, float* __restrict__ clip_scale,
                                                            float* __restrict__ loss, float* __restrict__ grad_scalars) {
  const float s = expf(logit_scale_p[0]);
  float tl = 0.f, tgs = 0.f, tgb = 0.f;
  for (int i = 0; i < B; ++i) {
    float l = 0.f, sa = 0.f, sc = 0.f;
    int cnt = 0;
    for (int e = threadIdx.x; e < T * P; e += 64) {
      const float* p = partial + (((size_t)i * T + e / P) * 16 + e % P) * 4;
      l += p[0]; cnt += (int)p[1]; sa += p[2]; sc += p[3];
    }
    l = wave_sum_dpp(l); sa = wave_sum_dpp(sa); sc = wave_sum_dpp(sc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    const float sci = cnt > 0 ? 1.f / ((float)cnt * (float)B) : 0.f;
    if (threadIdx.x == 0) clip_scale[i] = sci;
    tl = fmaf(l, sci, tl);
    tgs = fmaf(sc * s, sci, tgs);
    tgb = fmaf(sa, sci, tgb);
  }
  if (threadIdx.x == 0) {
    loss[0] = tl;
    if (grad_scalars) { grad_scalars[0] = tgs; grad_scalars[1] = tgb; }
  }
}

// (d) grid (ceil(T N / 8), clips): g = sum_l dz_l s scale_i E_l,  dx = (g - xhat <xhat, g>) / |x|,  <xhat, g> = sum_l dz_l s scale_i c_l
__global__ __launch_bounds__(256) void sf_mask_dx_kernel(SfMaskClips clips, int clip0, const float* __restrict__ x, int rows, int D,
                                                         size_t clip_stride, const float* __restrict__ sim, const float* __restrict__ dz,
                                                         const float* __restrict__ inv_norm, const float* __restrict__ clip_scale,
                                                         const float* __restrict__ logit_scale_p, float* __restrict__ dx) {
  __shared__ float dzs[SF_ML_ROWS][SF_ML_MAXL];
  __shared__ float dots[SF_ML_ROWS];
  const int ci = blockIdx.y, clip = clip0 + ci, L = clips.L[ci];
  const int r0 = blockIdx.x * SF_ML_ROWS, nr = min(SF_ML_ROWS, rows - r0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float f = expf(logit_scale_p[0]) * clip_scale[clip];
  const float* dzc = dz + (size_t)clip * clip_stride + (size_t)r0 * L;
  const float* simc = sim + (size_t)clip * clip_stride + (size_t)r0 * L;
  for (int e = threadIdx.x; e < SF_ML_ROWS * SF_ML_MAXL; e += 256) {
    const int r = e / SF_ML_MAXL, l = e % SF_ML_MAXL;
    dzs[r][l] = (r < nr && l < L) ? dzc[(size_t)r * L + l] * f : 0.f;
  }
  __syncthreads();
  for (int r = wave; r < SF_ML_ROWS; r += 4) {
    float a = 0.f;
    if (r < nr)
      for (int l = lane; l < L; l += 64) a = fmaf(dzs[r][l], simc[(size_t)r * L + l], a);
    a = wave_sum_dpp(a);
    if (lane == 0) dots[r] = a;
  }
  __syncthreads();
  const float* E = clips.emb[ci];
  const size_t row0 = (size_t)clip * rows + r0;
  for (int d = threadIdx.x; d < D; d += 256) {
    float g[SF_ML_ROWS];
#pragma unroll
    for (int r = 0; r < SF_ML_ROWS; ++r) g[r] = 0.f;
    for (int l = 0; l < L; ++l) {
      const float e = E[(size_t)l * D + d];
#pragma unroll
      for (int r = 0; r < SF_ML_ROWS; ++r) g[r] = fmaf(dzs[r][l], e, g[r]);
    }
#pragma unroll
    for (int r = 0; r < SF_ML_ROWS; ++r)
      if (r < nr) {
        const float in = inv_norm[row0 + r];
        dx[(row0 + r) * D + d] = (g[r] - x[(row0 + r) * D + d] * in * dots[r]) * in;
      }
  }
}

static size_t ml_align(size_t b) { return (b + 255) & ~(size_t)255; }
struct MlLayout { size_t sim, dz, inv_norm, partial, clip_scale, total; };
static MlLayout ml_layout(int B, int T, int N, int L) {
  MlLayout w;
  size_t o = 0;
  w.sim = o; o += ml_align((size_t)B * T * N * L * sizeof(float));
  w.dz = o; o += ml_align((size_t)B * T * N * L * sizeof(float));
  w.inv_norm = o; o += ml_align((size_t)B * T * N * sizeof(float));
  w.partial = o; o += ml_align((size_t)B * T * 16 * 4 * sizeof(float));
  w.clip_scale = o; o += ml_align((size_t)B * sizeof(float));
  w.total = o;
  return w;
}

extern "C" size_t sf_mask_loss_workspace_bytes(int B, int T, int N, int L_max) {
  if (B <= 0 || T <= 0 || N <= 0 || L_max <= 0) return 0;
  return ml_layout(B, T, N, L_max).total;
}

extern "C" int sf_mask_loss(const float* x, int B, int T, int N, int D, const float* const* label_emb, const int32_t* num_labels,
                            const int32_t* const* mask, const int32_t* mask_width, int H, const float* logit_scale,
                            const float* logit_bias, float* loss, float* grad_x, float* grad_scalars, void* workspace,
                            size_t workspace_bytes, sf_stream stream) {
  if (!x || !label_emb || !num_labels || !mask || !mask_width || !logit_scale || !logit_bias || !loss || !workspace)
    return sf_set_err(SF_ERR_INVALID, "sf_mask_loss: null buffer");
  if (B <= 0 || T <= 0 || N <= 0 || D <= 0 || H <= 0) return sf_set_err(SF_ERR_INVALID, "sf_mask_loss: bad shape B=%d T=%d N=%d D=%d H=%d", B, T, N, D, H);
  int P = 1;
  while (P * P < N) ++P;
  if (P * P != N) return sf_set_err(SF_ERR_INVALID, "sf_mask_loss: %d patch tokens per frame are not a square grid", N);
  if (N > 224) return sf_set_err(SF_ERR_CAPACITY, "sf_mask_loss: %d patches per frame > 224 (what the training step takes)", N);
  if (D > SF_ML_MAXD) return sf_set_err(SF_ERR_CAPACITY, "sf_mask_loss: feature width %d > %d (8 token rows in LDS)", D, SF_ML_MAXD);
  int Lmax = 0;
  for (int i = 0; i < B; ++i) {
    if (!label_emb[i] || !mask[i]) return sf_set_err(SF_ERR_INVALID, "sf_mask_loss: clip %d: null label table or mask", i);
    if (num_labels[i] <= 0 || mask_width[i] <= 0) return sf_set_err(SF_ERR_INVALID, "sf_mask_loss: clip %d: %d labels, mask width %d", i, num_labels[i], mask_width[i]);
    if (num_labels[i] > SF_ML_MAXL)
      return sf_set_err(SF_ERR_CAPACITY, "sf_mask_loss: clip %d: %d label classes > %d (the reference trains at most 100 per clip)", i, num_labels[i], SF_ML_MAXL);
    if (mask_width[i] > 4 * H || mask_width[i] > SF_ML_MAXW)
      return sf_set_err(SF_ERR_CAPACITY, "sf_mask_loss: clip %d: mask width %d > min(4 * height %d, %d)", i, mask_width[i], H, SF_ML_MAXW);
    if (num_labels[i] > Lmax) Lmax = num_labels[i];
  }
  const MlLayout w = ml_layout(B, T, N, Lmax);
  if (workspace_bytes < w.total) return sf_set_err(SF_ERR_WORKSPACE, "sf_mask_loss: workspace %zu < %zu bytes", workspace_bytes, w.total);
  char* ws = (char*)workspace;
  float* sim = (float*)(ws + w.sim);
  float* dz = (float*)(ws + w.dz);
  float* inv_norm = (float*)(ws + w.inv_norm);
  float* partial = (float*)(ws + w.partial);
  float* clip_scale = (float*)(ws + w.clip_scale);
  hipStream_t s = (hipStream_t)stream;
  const int rows = T * N, need_grad = (grad_x || grad_scalars) ? 1 : 0;
  const size_t clip_stride = (size_t)rows * Lmax;
  const dim3 row_grid((rows + SF_ML_ROWS - 1) / SF_ML_ROWS, 1);
  const size_t sim_lds = (size_t)SF_ML_ROWS * D * sizeof(float);
  for (int c0 = 0; c0 < B; c0 += SF_ML_CLIPS) {
    const int nc = B - c0 < SF_ML_CLIPS ? B - c0 : SF_ML_CLIPS;
    SfMaskClips clips = {};
    int Wmax = 0;
    for (int i = 0; i < nc; ++i) {
      clips.emb[i] = label_emb[c0 + i]; clips.mask[i] = mask[c0 + i]; clips.L[i] = num_labels[c0 + i]; clips.W[i] = mask_width[c0 + i];
      if (clips.W[i] > Wmax) Wmax = clips.W[i];
    }
    if (sim_lds > 48 * 1024)      // wide rows: past the default dynamic-LDS window
      HIP_TRY(sf_launch_big_lds(sf_mask_sim_kernel, dim3(row_grid.x, nc), dim3(256), sim_lds, s, clips, c0, x, rows, D, clip_stride, sim, inv_norm));
    else
      HIP_TRY(sf_launch(sf_mask_sim_kernel, dim3(row_grid.x, nc), dim3(256), sim_lds, s, clips, c0, x, rows, D, clip_stride, sim, inv_norm));
    const size_t lds = ((size_t)SF_ML_MAXP * SF_ML_MAXL + 5 * (size_t)Wmax + 32) * sizeof(float);
    HIP_TRY(sf_launch(sf_mask_pixel_kernel, dim3(P, T, nc), dim3(256), lds, s, clips, c0, sim, dz, partial, logit_scale, logit_bias, T, P, H,
                      clip_stride, need_grad));
  }
  HIP_TRY(sf_launch(sf_mask_finish_kernel, dim3(1), dim3(64), 0, s, partial, B, T, P, logit_scale, clip_scale, loss, grad_scalars));
  if (grad_x)
    for (int c0 = 0; c0 < B; c0 += SF_ML_CLIPS) {
      const int nc = B - c0 < SF_ML_CLIPS ? B - c0 : SF_ML_CLIPS;
      SfMaskClips clips = {};
      for (int i = 0; i < nc; ++i) { clips.emb[i] = label_emb[c0 + i]; clips.L[i] = num_labels[c0 + i]; }
      HIP_TRY(sf_launch(sf_mask_dx_kernel, dim3(row_grid.x, nc), dim3(256), 0, s, clips, c0, x, rows, D, clip_stride, sim, dz, inv_norm, clip_scale,
                        logit_scale, grad_x));
    }
  return SF_OK;
}
