// The two streaming kernels of the ViT-Adapter forward (models/modeling_timesformer_siglip_adapter.py) that are neither a GEMM, a
// LayerNorm nor deformable attention.  Both are memory-bound fp32 passes: no MFMA.
//
// Boundary rule (the one sf_msda.hip follows): every address is computed from coordinates that passed a range test against their OWN
// grid.  A 3 x 3 tap outside its level's grid contributes zero and is never read, so it cannot land on the neighbouring level's tokens or
// on the next frame's; a bilinear corner is clamped into the source grid before it becomes an index.
//
//   sf_adapter_dwconv_gelu_kernel   ConvFFN's DWConv + GELU (adapter:244-254, 231-232) on the three-level token tensor [F, 21 n, C]
//                                   (levels 2H x 2W, H x W, H/2 x W/2, n = H/2 * W/2, channels contiguous) in ONE pass instead of three
//                                   transposes to NCHW, three conv2d, three transposes back, a cat and a GELU.  Lanes run along C in
//                                   float4: a pixel's row is read by C / 4 consecutive lanes, so every tap is one contiguous segment.  A
//                                   thread keeps the nine weights and the bias of its four channels in registers and walks
//                                   ADW_PIXELS_PER_THREAD tokens of the block's strip with them; 256 / (C / 4) tokens are in flight per
//                                   step, lanes past the last whole token idle.  One owner per output element, one fixed order of the
//                                   nine taps: bit-reproducible.
//   sf_adapter_fuse_kernel          the tail (adapter:651-673) for one pyramid level: the extractor's tokens (res2: the transposed
//                                   convolution's GEMM output read through the 2 x 2 pixel shuffle) + the bilinear resampling of the kept
//                                   ViT stream (x4, x2, x1, x0.5 by F.interpolate(align_corners=False)'s rule, edge clamping included)
//                                   [+ the spatial prior's c1 at res2], then the eval BatchNorm as a folded affine, written NCHW.  Inputs
//                                   are channel-contiguous and the output is pixel-contiguous: the sums enter sf_nchw_tile.h's tile on
//                                   its rows side and leave on its NCHW side.  c1, which is NCHW already, is added on the way out.
#include "sf_internal.h"
#include "sf_nchw_tile.h"

#define ADW_THREADS 256
#define ADW_PIXELS_PER_THREAD 4

struct SfAdapterDw {
  const float* x; const float* w; const float* b; float* y;
  long long tokens;                      // F * 21 n
  int H, W, C, G;                        // the middle level's grid; channels; lanes per token (C / 4)
  int per_frame;                         // 21 n
  int slots;                             // tokens in flight per step: ADW_THREADS / G
};

__global__ __launch_bounds__(ADW_THREADS) void sf_adapter_dwconv_gelu_kernel(SfAdapterDw p) {
  const int slot = (int)threadIdx.x / p.G, c = ((int)threadIdx.x % p.G) * 4;
  if (slot >= p.slots) return;
  f32x4_t w[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {          // w [C, 3, 3]: tap k of channels c .. c + 3
    w[k][0] = p.w[(size_t)(c + 0) * 9 + k]; w[k][1] = p.w[(size_t)(c + 1) * 9 + k];
    w[k][2] = p.w[(size_t)(c + 2) * 9 + k]; w[k][3] = p.w[(size_t)(c + 3) * 9 + k];
  }
  const f32x4_t bias = *reinterpret_cast<const f32x4_t*>(p.b + c);
  const int n = (p.H / 2) * (p.W / 2);
  const long long strip = (long long)blockIdx.x * p.slots * ADW_PIXELS_PER_THREAD;
  for (int it = 0; it < ADW_PIXELS_PER_THREAD; ++it) {
    const long long tok = strip + (long long)it * p.slots + slot;
    if (tok >= p.tokens) return;
    const long long f = tok / p.per_frame;
    const int t = (int)(tok - f * p.per_frame);
    int Hl, Wl, start;                   // this token's level: its grid and its first token inside the frame
    if (t < 16 * n) { Hl = 2 * p.H; Wl = 2 * p.W; start = 0; }
    else if (t < 20 * n) { Hl = p.H; Wl = p.W; start = 16 * n; }
    else { Hl = p.H / 2; Wl = p.W / 2; start = 20 * n; }
    const int py = (t - start) / Wl, px = (t - start) - py * Wl;
    const float* level = p.x + ((size_t)f * p.per_frame + start) * p.C + c;
    f32x4_t acc = bias;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = py + dy;
      if (yy < 0 || yy >= Hl) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int xx = px + dx;
        if (xx < 0 || xx >= Wl) continue;
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(level + (size_t)(yy * Wl + xx) * p.C);
        acc += w[(dy + 1) * 3 + dx + 1] * v;
      }
    }
    f32x4_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = 0.5f * acc[j] * (1.f + erff(acc[j] * 0.70710678118654752440f));
    *reinterpret_cast<f32x4_t*>(p.y + (size_t)tok * p.C + c) = o;
  }
}

struct SfAdapterFuse {
  const float* tok; const float* vit; const float* c1; const float* scale; const float* shift; float* out;
  long long tok_frame_stride;            // floats between two frames of `tok`
  int level, Hv, Wv, Ho, Wo, D;
  float ratio;                           // source pixels per output pixel: 1 / scale_factor
};

__global__ __launch_bounds__(SF_TILE_THREADS) void sf_adapter_fuse_kernel(SfAdapterFuse p) {
  __shared__ float tile[SF_TILE_CELLS];
  const int f = (int)blockIdx.z, c0 = (int)blockIdx.y * SF_TILE, p0 = (int)blockIdx.x * SF_TILE;
  const int pixels = p.Ho * p.Wo;
  sf_tile_gather_rows(tile, p0, c0, pixels, p.D, [&](int pix, int c) {
    const int y = pix / p.Wo, x = pix - y * p.Wo;
    f32x4_t v;
    if (p.level == 0) {                  // row of the [.., 2Hv * 2Wv, 4 D] GEMM output, column block (dy, dx)
      const int sy = y >> 1, sx = x >> 1, q = (y & 1) * 2 + (x & 1);
      v = *reinterpret_cast<const f32x4_t*>(p.tok + (size_t)f * p.tok_frame_stride + ((size_t)(sy * (p.Wo >> 1) + sx) * 4 + q) * p.D + c);
    } else {
      v = *reinterpret_cast<const f32x4_t*>(p.tok + (size_t)f * p.tok_frame_stride + (size_t)pix * p.D + c);
    }
    if (p.vit) {
      int y0, y1, x0, x1;
      float ly, lx;
      sf_bilinear_axis(y, p.ratio, p.Hv, &y0, &y1, &ly);
      sf_bilinear_axis(x, p.ratio, p.Wv, &x0, &x1, &lx);
      const float* src = p.vit + (size_t)f * p.Hv * p.Wv * p.D + c;
      const f32x4_t v00 = *reinterpret_cast<const f32x4_t*>(src + (size_t)(y0 * p.Wv + x0) * p.D);
      const f32x4_t v01 = *reinterpret_cast<const f32x4_t*>(src + (size_t)(y0 * p.Wv + x1) * p.D);
      const f32x4_t v10 = *reinterpret_cast<const f32x4_t*>(src + (size_t)(y1 * p.Wv + x0) * p.D);
      const f32x4_t v11 = *reinterpret_cast<const f32x4_t*>(src + (size_t)(y1 * p.Wv + x1) * p.D);
      const float hy = 1.f - ly, hx = 1.f - lx;
      v += hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
    }
    return v;
  });
  __syncthreads();
  sf_tile_nchw(f, p0, c0, pixels, p.D, [&](int cell, int ch, size_t o) {
    float v = tile[cell];
    if (p.c1) v += p.c1[o];
    p.out[o] = p.scale[ch] * v + p.shift[ch];
  });
}

// ------------------------------------------------------------------------------------------------
// entry points: every refusal happens before anything is launched
// ------------------------------------------------------------------------------------------------
extern "C" int sf_op_adapter_dwconv_gelu(const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev, int F, int H, int W, int C,
                                         sf_stream stream) {
  const char* who = "sf_op_adapter_dwconv_gelu";
  if (!x_dev || !w_dev || !b_dev || !y_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (F < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return sf_set_err(SF_ERR_INVALID, "%s: F = %d, H = %d, W = %d: F >= 1, H and W even and >= 2 (the levels are 2H x 2W, H x W, H/2 x W/2)", who, F, H, W);
  if (C < 4 || C % 4 || C > 4 * ADW_THREADS) return sf_set_err(SF_ERR_INVALID, "%s: C = %d must be a multiple of 4 in 4..%d", who, C, 4 * ADW_THREADS);
  if (x_dev == y_dev) return sf_set_err(SF_ERR_INVALID, "%s: y must not alias x (every output reads its neighbours' inputs)", who);
  if (((uintptr_t)x_dev | (uintptr_t)y_dev | (uintptr_t)b_dev) & 15) return sf_set_err(SF_ERR_INVALID, "%s: x, y and b must be 16-byte aligned", who);
  const long long per_frame = 21LL * (H / 2) * (W / 2);
  if (per_frame > 0x7fffffffLL / 4) return sf_set_err(SF_ERR_INVALID, "%s: %lld tokens per frame exceed the index range", who, per_frame);
  SfAdapterDw p;
  p.x = x_dev; p.w = w_dev; p.b = b_dev; p.y = y_dev;
  p.tokens = (long long)F * per_frame; p.H = H; p.W = W; p.C = C; p.G = C / 4; p.per_frame = (int)per_frame;
  p.slots = ADW_THREADS / p.G;
  const long long per_block = (long long)p.slots * ADW_PIXELS_PER_THREAD;
  const long long blocks = (p.tokens + per_block - 1) / per_block;
  if (blocks > 0x7fffffffLL) return sf_set_err(SF_ERR_INVALID, "%s: %lld tokens exceed one grid", who, p.tokens);
  HIP_TRY(sf_launch(sf_adapter_dwconv_gelu_kernel, dim3((unsigned)blocks), dim3(ADW_THREADS), 0, (hipStream_t)stream, p));
  return SF_OK;
}

extern "C" int sf_op_adapter_fuse(int level, const float* tokens_dev, long long tokens_frame_stride, const float* vit_dev, const float* c1_dev,
                                  const float* scale_dev, const float* shift_dev, float* out_dev, int F, int H, int W, int D, sf_stream stream) {
  const char* who = "sf_op_adapter_fuse";
  if (level < 0 || level > 3) return sf_set_err(SF_ERR_INVALID, "%s: level = %d outside 0..3 (res2..res5)", who, level);
  if (!tokens_dev || !scale_dev || !shift_dev || !out_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (F < 1 || F > 65535 || H < 1 || W < 1 || H > 4096 || W > 4096) return sf_set_err(SF_ERR_INVALID, "%s: F = %d (1..65535), H = %d, W = %d (1..4096)", who, F, H, W);
  if (level == 3 && ((H & 1) || (W & 1))) return sf_set_err(SF_ERR_INVALID, "%s: level 3 halves the %d x %d grid: H and W must be even", who, H, W);
  if (D < 4 || D % 4) return sf_set_err(SF_ERR_INVALID, "%s: D = %d must be a multiple of 4", who, D);
  if (c1_dev && level != 0) return sf_set_err(SF_ERR_INVALID, "%s: c1 is added at level 0 (res2) only", who);
  SfAdapterFuse p;
  p.level = level; p.Hv = H; p.Wv = W; p.D = D;
  p.Ho = level == 0 ? 4 * H : level == 1 ? 2 * H : level == 2 ? H : H / 2;
  p.Wo = level == 0 ? 4 * W : level == 1 ? 2 * W : level == 2 ? W : W / 2;
  p.ratio = level == 0 ? 0.25f : level == 1 ? 0.5f : level == 2 ? 1.f : 2.f;
  const long long pixels = (long long)p.Ho * p.Wo;
  if (tokens_frame_stride < pixels * D || tokens_frame_stride % 4) return sf_set_err(SF_ERR_INVALID, "%s: tokens_frame_stride = %lld is shorter than a frame of %lld x %d floats, or no multiple of 4", who, tokens_frame_stride, pixels, D);
  if (((uintptr_t)tokens_dev | (uintptr_t)vit_dev) & 15) return sf_set_err(SF_ERR_INVALID, "%s: tokens and vit must be 16-byte aligned", who);
  p.tok = tokens_dev; p.vit = vit_dev; p.c1 = c1_dev; p.scale = scale_dev; p.shift = shift_dev; p.out = out_dev;
  p.tok_frame_stride = tokens_frame_stride;
  dim3 grid;
  if (!sf_tile_grid(F, D, pixels, &grid)) return sf_set_err(SF_ERR_INVALID, "%s: D = %d exceeds one grid", who, D);
  HIP_TRY(sf_launch(sf_adapter_fuse_kernel, grid, dim3(SF_TILE_THREADS), 0, (hipStream_t)stream, p));
  return SF_OK;
}
