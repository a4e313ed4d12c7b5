// Row-wise and elementwise kernels of the encoder path: LayerNorm (reference modeling:860-865,
// 878-880, 1251, 1138), patch extraction for the conv-as-GEMM patch embedding (modeling:329-350),
// operand splitting for the bf16x3 mode, and time-embedding row selection (modeling:435-450).
// All of them are HBM-bound: one wave per row, 16-byte vector accesses, wave-shuffle reductions.
#include "sf_common.h"

// ------------------------------------------------------------------------------------------------
// LayerNorm: one wave per row, the row lives in registers (D <= 64*4*MAXV), two-pass statistics.
// ------------------------------------------------------------------------------------------------
template <int MAXV>
__global__ __launch_bounds__(256) void sf_layernorm_kernel(const float* __restrict__ x,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta,
                                                           float* __restrict__ y_f32,
                                                           bf16_t* __restrict__ y_hi,
                                                           bf16_t* __restrict__ y_lo, int rows, int D,
                                                           float eps, const bf16_t* xp_hi, const bf16_t* xp_lo, const bf16_t* xp_lo2,
                                                           float* const* __restrict__ y_f32_ind) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  if (y_f32_ind) y_f32 = *y_f32_ind;
  const int nv = D >> 2;                       // float4 per row
  const f32x4_t* xr = reinterpret_cast<const f32x4_t*>(x + (size_t)row * D);
  // xp_hi / xp_lo: the row arrives as hi + lo bf16 planes (residual stream of the BASELINE-sized bf16 forward) instead of x;
  // y_hi may be xp_hi itself: the row is in registers before the first store
  const u32x2_t* xh = reinterpret_cast<const u32x2_t*>(xp_hi + (size_t)row * D);
  const u32x2_t* xl = reinterpret_cast<const u32x2_t*>(xp_lo + (size_t)row * D);
  const u32x2_t* xl2 = reinterpret_cast<const u32x2_t*>(xp_lo2 + (size_t)row * D);
  f32x4_t v[MAXV];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = i * 64 + lane;
    if (c < nv) {
      if (xp_hi) {
        const u32x2_t h = xh[c], l = xl[c];
        v[i] = (f32x4_t){bf2f(h[0] & 0xffffu) + bf2f(l[0] & 0xffffu), bf2f(h[0] >> 16) + bf2f(l[0] >> 16),
                         bf2f(h[1] & 0xffffu) + bf2f(l[1] & 0xffffu), bf2f(h[1] >> 16) + bf2f(l[1] >> 16)};
        if (xp_lo2) {
          const u32x2_t l2 = xl2[c];
          v[i] += (f32x4_t){bf2f(l2[0] & 0xffffu), bf2f(l2[0] >> 16), bf2f(l2[1] & 0xffffu), bf2f(l2[1] >> 16)};
        }
      } else {
        v[i] = xr[c];
      }
      s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    } else {
      v[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
  }
  const float mean = wave_sum_dpp(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = i * 64 + lane;
    if (c < nv) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = v[i][j] - mean;
        q += d * d;
      }
    }
  }
  const float rstd = rsqrtf(wave_sum_dpp(q) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    const int c = i * 64 + lane;
    if (c < nv) {
      const f32x4_t g = reinterpret_cast<const f32x4_t*>(gamma)[c];
      const f32x4_t b = reinterpret_cast<const f32x4_t*>(beta)[c];
      f32x4_t o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (v[i][j] - mean) * rstd * g[j] + b[j];
      const size_t off = (size_t)row * D + (size_t)c * 4;
      if (y_f32) *reinterpret_cast<f32x4_t*>(y_f32 + off) = o;
      if (y_hi) {
        unsigned int h[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) split_bf(o[j], h[j], l[j]);
        *reinterpret_cast<u32x2_t*>(y_hi + off) = (u32x2_t){h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
        if (y_lo) *reinterpret_cast<u32x2_t*>(y_lo + off) = (u32x2_t){l[0] | (l[1] << 16), l[2] | (l[3] << 16)};
      }
    }
  }
}

hipError_t sf_launch_layernorm(const float* x, const float* gamma, const float* beta, float* y_f32,
                               bf16_t* y_hi, bf16_t* y_lo, int rows, int D, float eps, hipStream_t s, const bf16_t* xp_hi,
                               const bf16_t* xp_lo, const bf16_t* xp_lo2, float* const* y_f32_ind) {
  if (rows <= 0) return hipSuccess;
  if (D % 4 || D > 64 * 4 * 16) return hipErrorInvalidValue;
  const dim3 grid((rows + 3) / 4), block(256);
  const int nv = (D / 4 + 63) / 64;
  if (nv <= 1) return sf_launch(sf_layernorm_kernel<1>, grid, block, 0, s, x, gamma, beta, y_f32, y_hi, y_lo, rows, D, eps, xp_hi, xp_lo, xp_lo2, y_f32_ind);
  if (nv <= 3) return sf_launch(sf_layernorm_kernel<3>, grid, block, 0, s, x, gamma, beta, y_f32, y_hi, y_lo, rows, D, eps, xp_hi, xp_lo, xp_lo2, y_f32_ind);
  if (nv <= 8) return sf_launch(sf_layernorm_kernel<8>, grid, block, 0, s, x, gamma, beta, y_f32, y_hi, y_lo, rows, D, eps, xp_hi, xp_lo, xp_lo2, y_f32_ind);
  return sf_launch(sf_layernorm_kernel<16>, grid, block, 0, s, x, gamma, beta, y_f32, y_hi, y_lo, rows, D, eps, xp_hi, xp_lo, xp_lo2, y_f32_ind);
}

// ------------------------------------------------------------------------------------------------
// The tail models' row pass (SfRowArgs): the detector's post-LN residual rows LN(x + sublayer(x)) and feature heads ReLU(LN(x)) + pe
// or x + pe, the pixel decoder's LayerNorm that also emits the next layer's query operand y + pos.  Any width, so the row is re-read
// from memory in each pass instead of living in registers.  Order: addend, statistics, normalise, ReLU, then the positional addend.
// ADD (p.r), LN (p.gamma) and RELU are template flags: as run-time tests they cost the pixel decoder's post-LN 2.6 % (82.9 against
// 80.8 us per launch at 131 712 rows of 256, MI355X); which outputs are written stays a run-time test, as in both kernels this replaced.
// ------------------------------------------------------------------------------------------------
template <bool ADD, bool LN, bool RELU>
__global__ __launch_bounds__(256) void sf_row_kernel(SfRowArgs p) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.rows) return;
  const int nv = p.D >> 2;
  const f32x4_t* x = reinterpret_cast<const f32x4_t*>(p.x + (size_t)row * p.D);
  const f32x4_t* r = ADD ? reinterpret_cast<const f32x4_t*>(p.r + (size_t)(p.r_mod ? row % p.r_mod : row) * p.D) : nullptr;
  float mean = 0.f, rstd = 1.f;
  if (LN) {
    float s = 0.f;
    for (int c = lane; c < nv; c += 64) {
      f32x4_t v = x[c];
      if (ADD) v += r[c];
      s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    mean = wave_sum(s) / (float)p.D;
    float q = 0.f;
    for (int c = lane; c < nv; c += 64) {
      f32x4_t v = x[c];
      if (ADD) v += r[c];
      v -= mean;
      q += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    rstd = 1.0f / sqrtf(wave_sum(q) / (float)p.D + p.eps);
  }
  const f32x4_t* pe = p.pe ? reinterpret_cast<const f32x4_t*>(p.pe + (size_t)(row % p.pe_mod) * p.D) : nullptr;
  for (int c = lane; c < nv; c += 64) {
    f32x4_t v = x[c];
    if (ADD) v += r[c];
    if (LN) {
      const f32x4_t gm = reinterpret_cast<const f32x4_t*>(p.gamma)[c], bt = reinterpret_cast<const f32x4_t*>(p.beta)[c];
      v = (v - mean) * rstd * gm + bt;
    }
    if (RELU) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
    const size_t o = (size_t)row * p.D + (size_t)c * 4;
    if (p.y) *reinterpret_cast<f32x4_t*>(p.y + o) = v;
    if (p.y_hi) store_planes4(v, p.y_hi, p.y_lo, o);
    if (pe) {
      const f32x4_t e = v + pe[c];
      if (p.q) *reinterpret_cast<f32x4_t*>(p.q + o) = e;
      if (p.q_hi) store_planes4(e, p.q_hi, p.q_lo, o);
    }
  }
}

template <bool ADD, bool LN>
static hipError_t sf_launch_row_as(const SfRowArgs& p, hipStream_t s) {
  const dim3 grid((unsigned)((p.rows + 3) / 4)), block(256);
  return p.relu ? sf_launch(sf_row_kernel<ADD, LN, true>, grid, block, 0, s, p) : sf_launch(sf_row_kernel<ADD, LN, false>, grid, block, 0, s, p);
}
hipError_t sf_launch_row(const SfRowArgs& p, hipStream_t s) {
  if (p.r) return p.gamma ? sf_launch_row_as<true, true>(p, s) : sf_launch_row_as<true, false>(p, s);
  return p.gamma ? sf_launch_row_as<false, true>(p, s) : sf_launch_row_as<false, false>(p, s);
}

// ------------------------------------------------------------------------------------------------
// patchify: pixels [F,C,H,W] -> A[F*N, C*P*P] (bf16 hi/lo), column = (c*P + ph)*P + pw,
// patch n = prow*(W/P) + pcol.  One thread moves 8 consecutive pw pixels (16 B of bf16 out).
// IN = 0 fp32, 1 bf16 (already normalised frames), 2 uint8 raw frames: the image processor's
// rescale + normalize (vqa_enc:1436-1447: x / 255, then (x - mean) / std per channel) is fused here as
// one FMA per pixel, so frames cross PCIe / HBM as bytes.
// ------------------------------------------------------------------------------------------------
template <int IN>
SF_DEVICE void sf_patchify_body(const void* __restrict__ pixels, bf16_t* __restrict__ out_hi, bf16_t* __restrict__ out_lo, int F, int C, int H,
                                int W, int P, int gh, int gw, const SfPixelNorm& norm) {
  const int Kp = C * P * P;
  const int chunks_per_row = Kp >> 3;
  const size_t total = (size_t)F * gh * gw * chunks_per_row;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ck = (int)(i % chunks_per_row);
    const size_t prow = i / chunks_per_row;          // global patch row = f*N + n
    const int n = (int)(prow % (gh * gw));
    const int f = (int)(prow / (gh * gw));
    const int col = ck << 3;
    const int c = col / (P * P), rem = col % (P * P);
    const int ph = rem / P, pw = rem % P;
    const int y = (n / gw) * P + ph, x0 = (n % gw) * P + pw;
    const size_t src = (((size_t)f * C + c) * H + y) * W + x0;
    float v[8];
    if (IN == 2) {
      const u32x2_t raw = *reinterpret_cast<const u32x2_t*>(reinterpret_cast<const unsigned char*>(pixels) + src);
      const float sc = norm.scale[c & 3], sh = norm.shift[c & 3];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = fmaf((float)((raw[j >> 2] >> ((j & 3) * 8)) & 0xffu), sc, sh);
    } else if (IN == 1) {
      const bf16_t* pp = reinterpret_cast<const bf16_t*>(pixels) + src;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = bf2f(pp[j]);
    } else {
      const float* pp = reinterpret_cast<const float*>(pixels) + src;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = pp[j];
    }
    unsigned int h[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split_bf(v[j], h[j], l[j]);
    const size_t o = prow * Kp + col;
    *reinterpret_cast<u32x4_t*>(out_hi + o) =
        (u32x4_t){h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
    if (out_lo)
      *reinterpret_cast<u32x4_t*>(out_lo + o) =
          (u32x4_t){l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16)};
  }
}
template <int IN>
__global__ __launch_bounds__(256) void sf_patchify_kernel(const void* __restrict__ pixels,
                                                          bf16_t* __restrict__ out_hi,
                                                          bf16_t* __restrict__ out_lo, int F, int C, int H,
                                                          int W, int P, int gh, int gw, SfPixelNorm norm,
                                                          const SfStreamParams* __restrict__ sp, SfStreamParams* sp_write,
                                                          SfStreamParams sp_value) {
  if (sp) pixels = sp->pixels;
  if (sp_write && blockIdx.x == 0 && threadIdx.x == 0) *sp_write = sp_value;
  sf_patchify_body<IN>(pixels, out_hi, out_lo, F, C, H, W, P, gh, gw, norm);
}
// Ragged streaming call: the launch also stores the call's stream table (one entry per row group, by thread = entry of workgroup 0)
template <int IN>
__global__ __launch_bounds__(256) void sf_patchify_tab_kernel(const void* __restrict__ pixels, bf16_t* __restrict__ out_hi,
                                                              bf16_t* __restrict__ out_lo, int F, int C, int H, int W, int P, int gh, int gw,
                                                              SfPixelNorm norm, SfStreamParams* sp_write, SfStreamParams sp_value,
                                                              SfStreamSlot* tab_write, SfStreamTable tab_value) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *sp_write = sp_value;
  if (blockIdx.x == 0 && (int)threadIdx.x < tab_value.n) tab_write[threadIdx.x] = tab_value.e[threadIdx.x];
  sf_patchify_body<IN>(pixels, out_hi, out_lo, F, C, H, W, P, gh, gw, norm);
}

// Any patch size / padded patch vectors (14 x 14 patches: K = 588 -> 640): one thread per 8 output columns, element by element;
// columns past C * P * P are zeros (the patch-embedding weight is zero-padded to the same width at upload).
template <int IN>
SF_DEVICE void sf_patchify_generic_body(const void* __restrict__ pixels, bf16_t* __restrict__ out_hi, bf16_t* __restrict__ out_lo, int F, int C,
                                        int H, int W, int P, int gh, int gw, int Kpad, const SfPixelNorm& norm) {
  const int Kr = C * P * P, chunks_per_row = Kpad >> 3;
  const size_t total = (size_t)F * gh * gw * chunks_per_row;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ck = (int)(i % chunks_per_row);
    const size_t prow = i / chunks_per_row;
    const int n = (int)(prow % (gh * gw)), f = (int)(prow / (gh * gw));
    unsigned int h[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = ck * 8 + j;
      float v = 0.f;
      if (col < Kr) {
        const int c = col / (P * P), rem = col % (P * P);
        const size_t src = (((size_t)f * C + c) * H + (n / gw) * P + rem / P) * W + (n % gw) * P + rem % P;
        if (IN == 2) v = fmaf((float)reinterpret_cast<const unsigned char*>(pixels)[src], norm.scale[c & 3], norm.shift[c & 3]);
        else if (IN == 1) v = bf2f(reinterpret_cast<const bf16_t*>(pixels)[src]);
        else v = reinterpret_cast<const float*>(pixels)[src];
      }
      split_bf(v, h[j], l[j]);
    }
    const size_t o = prow * Kpad + (size_t)ck * 8;
    *reinterpret_cast<u32x4_t*>(out_hi + o) = (u32x4_t){h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
    if (out_lo) *reinterpret_cast<u32x4_t*>(out_lo + o) = (u32x4_t){l[0] | (l[1] << 16), l[2] | (l[3] << 16), l[4] | (l[5] << 16), l[6] | (l[7] << 16)};
  }
}
template <int IN>
__global__ __launch_bounds__(256) void sf_patchify_generic_kernel(const void* __restrict__ pixels, bf16_t* __restrict__ out_hi,
                                                                  bf16_t* __restrict__ out_lo, int F, int C, int H, int W, int P, int gh, int gw,
                                                                  int Kpad, SfPixelNorm norm, const SfStreamParams* __restrict__ sp,
                                                                  SfStreamParams* sp_write, SfStreamParams sp_value) {
  if (sp) pixels = sp->pixels;
  if (sp_write && blockIdx.x == 0 && threadIdx.x == 0) *sp_write = sp_value;
  sf_patchify_generic_body<IN>(pixels, out_hi, out_lo, F, C, H, W, P, gh, gw, Kpad, norm);
}
template <int IN>
__global__ __launch_bounds__(256) void sf_patchify_generic_tab_kernel(const void* __restrict__ pixels, bf16_t* __restrict__ out_hi,
                                                                      bf16_t* __restrict__ out_lo, int F, int C, int H, int W, int P, int gh,
                                                                      int gw, int Kpad, SfPixelNorm norm, SfStreamParams* sp_write,
                                                                      SfStreamParams sp_value, SfStreamSlot* tab_write, SfStreamTable tab_value) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *sp_write = sp_value;
  if (blockIdx.x == 0 && (int)threadIdx.x < tab_value.n) tab_write[threadIdx.x] = tab_value.e[threadIdx.x];
  sf_patchify_generic_body<IN>(pixels, out_hi, out_lo, F, C, H, W, P, gh, gw, Kpad, norm);
}

hipError_t sf_launch_patchify(const void* pixels, int pixel_kind, bf16_t* out_hi, bf16_t* out_lo,
                              int F, int C, int H, int W, int P, hipStream_t s, const SfPixelNorm* pnorm, const SfStreamParams* sp,
                              SfStreamParams* sp_write, const SfStreamParams* sp_value, int Kpad, SfStreamSlot* tab_write,
                              const SfStreamTable* tab_value) {
  SfStreamParams spv = {};
  if (sp_write) { if (!sp_value) return hipErrorInvalidValue; spv = *sp_value; }
  // the table rides with the parameter block, on the caller's pixels
  if (tab_write && (!tab_value || !sp_write || sp || tab_value->n <= 0 || tab_value->n > SF_MAX_CALL_STREAMS)) return hipErrorInvalidValue;
  SfPixelNorm norm;
  for (int i = 0; i < 4; ++i) { norm.scale[i] = 1.0f / 127.5f; norm.shift[i] = -1.0f; }    // mean = std = 0.5, rescale 1/255
  if (pnorm) norm = *pnorm;
  if (Kpad <= 0) Kpad = C * P * P;
  if (P % 8 || Kpad != C * P * P || (pixel_kind == 2 && W % 8)) {      // generic path
    if (Kpad % 8 || Kpad < C * P * P || (pixel_kind == 2 && C > 4)) return hipErrorInvalidValue;
    const int gh = H / P, gw = W / P;
    const size_t total = (size_t)F * gh * gw * (Kpad / 8);
    if (!total) return hipSuccess;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (tab_write) {
#define SF_PG_TAB(IN) return sf_launch(sf_patchify_generic_tab_kernel<IN>, dim3(blocks), dim3(256), 0, s, pixels, out_hi, out_lo, F, C, H, W, P, gh, gw, Kpad, norm, sp_write, spv, tab_write, *tab_value)
      if (pixel_kind == 2) SF_PG_TAB(2); else if (pixel_kind == 1) SF_PG_TAB(1); else SF_PG_TAB(0);
#undef SF_PG_TAB
    }
    if (pixel_kind == 2) return sf_launch(sf_patchify_generic_kernel<2>, dim3(blocks), dim3(256), 0, s, pixels, out_hi, out_lo, F, C, H, W, P, gh, gw, Kpad, norm, sp, sp_write, spv);
    if (pixel_kind == 1) return sf_launch(sf_patchify_generic_kernel<1>, dim3(blocks), dim3(256), 0, s, pixels, out_hi, out_lo, F, C, H, W, P, gh, gw, Kpad, norm, sp, sp_write, spv);
    return sf_launch(sf_patchify_generic_kernel<0>, dim3(blocks), dim3(256), 0, s, pixels, out_hi, out_lo, F, C, H, W, P, gh, gw, Kpad, norm, sp, sp_write, spv);
  }
  if (pixel_kind == 2 && C > 4) return hipErrorInvalidValue;
  const int gh = H / P, gw = W / P;
  const size_t total = (size_t)F * gh * gw * (C * P * P / 8);
  if (!total) return hipSuccess;
  const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  if (tab_write) {
#define SF_P_TAB(IN) return sf_launch(sf_patchify_tab_kernel<IN>, dim3(blocks), dim3(256), 0, s, pixels, out_hi, out_lo, F, C, H, W, P, gh, gw, norm, sp_write, spv, tab_write, *tab_value)
    if (pixel_kind == 2) SF_P_TAB(2); else if (pixel_kind == 1) SF_P_TAB(1); else SF_P_TAB(0);
#undef SF_P_TAB
  }
  if (pixel_kind == 2)
    return sf_launch(sf_patchify_kernel<2>, dim3(blocks), dim3(256), 0, s, pixels, out_hi, out_lo, F, C, H, W, P, gh, gw, norm, sp, sp_write, spv);
  if (pixel_kind == 1)
    return sf_launch(sf_patchify_kernel<1>, dim3(blocks), dim3(256), 0, s, pixels, out_hi, out_lo, F, C, H, W, P, gh, gw, norm, sp, sp_write, spv);
  return sf_launch(sf_patchify_kernel<0>, dim3(blocks), dim3(256), 0, s, pixels, out_hi, out_lo, F, C, H, W, P, gh, gw, norm, sp, sp_write, spv);
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sf_split_kernel(const float* __restrict__ x, bf16_t* __restrict__ hi,
                                                       bf16_t* __restrict__ lo, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4_t v = reinterpret_cast<const f32x4_t*>(x)[i];
    unsigned int h[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split_bf(v[j], h[j], l[j]);
    reinterpret_cast<u32x2_t*>(hi)[i] = (u32x2_t){h[0] | (h[1] << 16), h[2] | (h[3] << 16)};
    if (lo) reinterpret_cast<u32x2_t*>(lo)[i] = (u32x2_t){l[0] | (l[1] << 16), l[2] | (l[3] << 16)};
  }
}

hipError_t sf_launch_split(const float* x, bf16_t* hi, bf16_t* lo, size_t n, hipStream_t s) {
  if (n % 4) return hipErrorInvalidValue;
  if (!n) return hipSuccess;
  const size_t n4 = n / 4;
  const int blocks = (int)((n4 + 255) / 256 < 8192 ? (n4 + 255) / 256 : 8192);
  return sf_launch(sf_split_kernel, dim3(blocks), dim3(256), 0, s, x, hi, lo, n4);
}

// ------------------------------------------------------------------------------------------------
// LN-fold entry: bf16 copy of the rows + {sum x, sum x^2} (used once per forward, on the embeddings)
__global__ __launch_bounds__(256) void sf_rowstats_cast_kernel(const float* __restrict__ x, bf16_t* __restrict__ xb,
                                                               bf16_t* __restrict__ xlo, bf16_t* __restrict__ xlo2, float* __restrict__ stats, int rows, int D, int wide) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = D >> 2;
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < nv; c += 64) {
    const f32x4_t v = reinterpret_cast<const f32x4_t*>(x + (size_t)row * D)[c];
    s1 += (v[0] + v[1]) + (v[2] + v[3]);
    s2 += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    const u32x2_t h = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
    *reinterpret_cast<u32x2_t*>(xb + (size_t)row * D + (size_t)c * 4) = h;
    if (xlo) {
      const float r0 = v[0] - bf2f(h[0] & 0xffffu), r1 = v[1] - bf2f(h[0] >> 16), r2 = v[2] - bf2f(h[1] & 0xffffu), r3 = v[3] - bf2f(h[1] >> 16);
      const u32x2_t l = {pack_bf2(r0, r1), pack_bf2(r2, r3)};
      *reinterpret_cast<u32x2_t*>(xlo + (size_t)row * D + (size_t)c * 4) = l;
      if (xlo2)
        *reinterpret_cast<u32x2_t*>(xlo2 + (size_t)row * D + (size_t)c * 4) =
            (u32x2_t){pack_bf2(r0 - bf2f(l[0] & 0xffffu), r1 - bf2f(l[0] >> 16)), pack_bf2(r2 - bf2f(l[1] & 0xffffu), r3 - bf2f(l[1] >> 16))};
    }
  }
  s1 = wave_sum_dpp(s1);
  s2 = wave_sum_dpp(s2);
  if (lane == 0) {          // wide rows ([8]: this pair + empty ones): the accurate mode, and the bf16 mode's four-pair layout
    *reinterpret_cast<f32x4_t*>(stats + (size_t)row * (wide ? 8 : 4)) = (f32x4_t){s1, s2, 0.f, 0.f};
    if (wide) *reinterpret_cast<f32x4_t*>(stats + (size_t)row * 8 + 4) = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
}

hipError_t sf_launch_rowstats_cast(const float* x, bf16_t* xb, float* stats, int rows, int D, hipStream_t s, bf16_t* xlo, bf16_t* xlo2, int wide) {
  if (rows <= 0) return hipSuccess;
  if (D % 4) return hipErrorInvalidValue;
  return sf_launch(sf_rowstats_cast_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, xb, xlo, xlo2, stats, rows, D, (wide || xlo) ? 1 : 0);
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sf_gather_rows_kernel(const float* __restrict__ table,
                                                             float* __restrict__ out, SfRowIndex idx, int D,
                                                             const int* __restrict__ base_dev, const SfStreamSlot* __restrict__ tab) {
  const int t = blockIdx.x;
  const float* src = table + (size_t)(tab ? tab[t].t_row : idx.idx[t] + (base_dev ? *base_dev : 0)) * D;
  for (int i = threadIdx.x; i < D; i += blockDim.x) out[(size_t)t * D + i] = src[i];
}

hipError_t sf_launch_gather_rows(const float* table, float* out, const SfRowIndex& idx, int D, hipStream_t s, const int* base_dev,
                                 const SfStreamSlot* tab) {
  if (idx.n <= 0 || idx.n > 256) return hipErrorInvalidValue;
  return sf_launch(sf_gather_rows_kernel, dim3(idx.n), dim3(256), 0, s, table, out, idx, D, base_dev, tab);
}


// ------------------------------------------------------------------------------------------------
// position + time embedding table: out[(t, n), :] = pos[n, :] + time_rows[t, :]
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sf_pos_time_table_kernel(const float* __restrict__ pos, const float* __restrict__ te,
                                                                float* __restrict__ out, int T, int N, int D4) {
  const size_t total = (size_t)T * N * D4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % D4);
    const size_t row = i / D4;
    const int n = (int)(row % N), t = (int)(row / N);
    reinterpret_cast<f32x4_t*>(out)[i] = reinterpret_cast<const f32x4_t*>(pos)[(size_t)n * D4 + c] + reinterpret_cast<const f32x4_t*>(te)[(size_t)t * D4 + c];
  }
}
hipError_t sf_launch_pos_time_table(const float* pos, const float* time_rows, float* out, int T, int N, int D, hipStream_t s) {
  if (D % 4) return hipErrorInvalidValue;
  const size_t total = (size_t)T * N * (D / 4);
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  return sf_launch(sf_pos_time_table_kernel, dim3(blocks), dim3(256), 0, s, pos, time_rows, out, T, N, D / 4);
}

__global__ __launch_bounds__(256) void sf_copy2_kernel(const float* __restrict__ a_src, float* __restrict__ a_dst, size_t na4,
                                                       const float* __restrict__ b_src, float* __restrict__ b_dst, size_t nb4,
                                                       const SfStreamParams* __restrict__ sp) {
  if (sp) { a_dst = sp->lhs; b_dst = sp->pooler; }
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < na4) reinterpret_cast<f32x4_t*>(a_dst)[i] = reinterpret_cast<const f32x4_t*>(a_src)[i];
  else if (i - na4 < nb4) reinterpret_cast<f32x4_t*>(b_dst)[i - na4] = reinterpret_cast<const f32x4_t*>(b_src)[i - na4];
}

hipError_t sf_launch_copy2(const float* a_src, float* a_dst, size_t na, const float* b_src, float* b_dst, size_t nb, hipStream_t s,
                           const SfStreamParams* sp) {
  if ((na % 4) || (nb % 4)) return hipErrorInvalidValue;
  if (!b_src || (!b_dst && !sp)) nb = 0;
  const size_t n4 = (na + nb) / 4;
  if (!n4) return hipSuccess;
  return sf_launch(sf_copy2_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, a_src, a_dst, na / 4, b_src, b_dst, nb / 4, sp);
}
