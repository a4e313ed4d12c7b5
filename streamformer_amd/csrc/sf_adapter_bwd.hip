// Backward of the two streaming kernels of the ViT-Adapter (sf_adapter.hip), for streamformer_amd/adapter.py with trainable=True.  Both are
// memory-bound fp32 passes in the forward file's style: lanes along C in float4, no MFMA, no atomics, one owner per output element and one
// fixed order per sum, so two runs give the same bits.  The forward file's boundary rule holds here too: every address is computed from
// coordinates that passed a range test against their OWN level's grid, a 3 x 3 tap outside it contributes zero and is never read.
//
// ConvFFN's DWConv + GELU.  The forward saved x only; with z = dwconv(x) + b recomputed in the forward's own tap order (the same bits),
//     g = dy gelu'(z),   gelu'(z) = (1 + erf(z / sqrt 2)) / 2 + z exp(-z^2 / 2) / sqrt(2 pi)      (the derivative of the forward's erf form)
//     db[c] = sum_t g[t, c]     dw[c, k] = sum_t g[t, c] x[t + offset_k, c]     dx[t, c] = sum_k w[c, k] g[t - offset_k, c]
//
//   sf_adapter_dw_bwd_g_kernel      the forward's thread layout (ADW_THREADS / (C / 4) token slots, C / 4 lanes each), a strip of
//                                   `per_thread` tokens per slot.  Writes g to the workspace (when dx is asked for) and keeps the nine
//                                   sum g x_tap and the one sum g of its four channels in registers over its strip (when dw or db is);
//                                   the slots of a workgroup meet through LDS in slot order: one partial row [10, C] per workgroup.
//   sf_adapter_dw_bwd_sum_kernel    dw [C, 3, 3] and db [C]: 16 row lanes take the workgroups' partial rows round-robin in ascending order
//                                   and meet in lane order.
//   sf_adapter_dw_bwd_dx_kernel     the forward kernel with the taps mirrored, on g: a gather over the token's own level grid.
//   sf_adapter_fuse_bwd_kernel      the adjoint of sf_adapter_fuse_kernel in its token operand (the ViT term is a constant, c1's gradient
//                                   is dy itself, the BatchNorm is torch's in training): a pure re-layout.  dy NCHW enters sf_nchw_tile.h's
//                                   tile on its NCHW side and leaves on the rows side, at level 0 through the inverse 2 x 2 pixel shuffle
//                                   into the transposed convolution's GEMM-output layout.  Every output element is written exactly once.
#include "sf_internal.h"
#include "sf_handle.h"
#include "sf_nchw_tile.h"

#define ADW_THREADS 256
#define ADW_PIXELS_PER_THREAD 4          // the dx pass, as the forward
#define ADW_BWD_TARGET_WGS 512           // the g pass lengthens its strips until about this many workgroups are left
#define ADW_SUM_COLS 16
#define ADW_SUM_LANES 16

struct SfAdapterDwBwd {
  const float *x, *w, *b, *dy;
  float *g, *part;                       // workspace: [F * 21 n, C] (null: dx is not asked for), [workgroups, 10, C] (null: neither dw nor db)
  float *dx, *dw, *db;
  long long tokens;                      // F * 21 n
  int H, W, C, G, per_frame, slots;      // as SfAdapterDw
  int per_thread;                        // tokens of one slot's strip in the g pass
  int wgs;                               // workgroups of the g pass = partial rows
};

// the level of token t of a frame: its grid and its first token inside the frame
SF_DEVICE void adw_level(int t, int H, int W, int n, int* Hl, int* Wl, int* start) {
  if (t < 16 * n) { *Hl = 2 * H; *Wl = 2 * W; *start = 0; }
  else if (t < 20 * n) { *Hl = H; *Wl = W; *start = 16 * n; }
  else { *Hl = H / 2; *Wl = W / 2; *start = 20 * n; }
}

__global__ __launch_bounds__(ADW_THREADS) void sf_adapter_dw_bwd_g_kernel(SfAdapterDwBwd p) {
  __shared__ f32x4_t red[ADW_THREADS];
  const int slot = (int)threadIdx.x / p.G, lane = (int)threadIdx.x % p.G, c = lane * 4;
  const bool active = slot < p.slots;
  f32x4_t w[9], sw[9], sb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    sw[k] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    w[k] = sw[k];
  }
  if (active) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      w[k][0] = p.w[(size_t)(c + 0) * 9 + k]; w[k][1] = p.w[(size_t)(c + 1) * 9 + k];
      w[k][2] = p.w[(size_t)(c + 2) * 9 + k]; w[k][3] = p.w[(size_t)(c + 3) * 9 + k];
    }
    const f32x4_t bias = *reinterpret_cast<const f32x4_t*>(p.b + c);
    const int n = (p.H / 2) * (p.W / 2);
    const long long strip = (long long)blockIdx.x * p.slots * p.per_thread;
    for (int it = 0; it < p.per_thread; ++it) {
      const long long tok = strip + (long long)it * p.slots + slot;
      if (tok >= p.tokens) break;
      const long long f = tok / p.per_frame;
      const int t = (int)(tok - f * p.per_frame);
      int Hl, Wl, start;
      adw_level(t, p.H, p.W, n, &Hl, &Wl, &start);
      const int py = (t - start) / Wl, px = (t - start) - py * Wl;
      const float* level = p.x + ((size_t)f * p.per_frame + start) * p.C + c;
      f32x4_t v[9], acc = bias;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int k = (dy + 1) * 3 + dx + 1, yy = py + dy, xx = px + dx;
          if (yy < 0 || yy >= Hl || xx < 0 || xx >= Wl) {
            v[k] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
            continue;
          }
          v[k] = *reinterpret_cast<const f32x4_t*>(level + (size_t)(yy * Wl + xx) * p.C);
          acc += w[k] * v[k];
        }
      }
      const f32x4_t d = *reinterpret_cast<const f32x4_t*>(p.dy + (size_t)tok * p.C + c);
      f32x4_t g;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float z = acc[j];
        g[j] = d[j] * (0.5f * (1.f + erff(z * 0.70710678118654752440f)) + z * expf(-0.5f * z * z) * 0.39894228040143267794f);
      }
      if (p.g) *reinterpret_cast<f32x4_t*>(p.g + (size_t)tok * p.C + c) = g;
      sb += g;
#pragma unroll
      for (int k = 0; k < 9; ++k) sw[k] += g * v[k];
    }
  }
  if (!p.part) return;                   // (uniform over the workgroup)
  float* row = p.part + (size_t)blockIdx.x * 10 * p.C;
#pragma unroll
  for (int k = 0; k < 10; ++k) {         // rows 0..8: the taps of dw, row 9: db; the slots in ascending order
    if (active) red[slot * p.G + lane] = k < 9 ? sw[k] : sb;
    __syncthreads();
    if (active && slot == 0) {
      f32x4_t s = red[lane];
      for (int l = 1; l < p.slots; ++l) s += red[l * p.G + lane];
      *reinterpret_cast<f32x4_t*>(row + (size_t)k * p.C + c) = s;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(ADW_SUM_COLS * ADW_SUM_LANES) void sf_adapter_dw_bwd_sum_kernel(SfAdapterDwBwd p) {
  __shared__ float red[ADW_SUM_LANES][ADW_SUM_COLS];
  const int col = (int)threadIdx.x % ADW_SUM_COLS, rl = (int)threadIdx.x / ADW_SUM_COLS;
  const int i = (int)blockIdx.x * ADW_SUM_COLS + col, cols = 10 * p.C;      // column i of a partial row: tap k = i / C, channel i % C
  float s = 0.f;
  if (i < cols)
    for (int r = rl; r < p.wgs; r += ADW_SUM_LANES) s += p.part[(size_t)r * cols + i];
  red[rl][col] = s;
  __syncthreads();
  if (rl == 0 && i < cols) {
    for (int l = 1; l < ADW_SUM_LANES; ++l) s += red[l][col];
    const int k = i / p.C, ch = i - k * p.C;
    if (k < 9) {
      if (p.dw) p.dw[(size_t)ch * 9 + k] = s;
    } else if (p.db) {
      p.db[ch] = s;
    }
  }
}

__global__ __launch_bounds__(ADW_THREADS) void sf_adapter_dw_bwd_dx_kernel(SfAdapterDwBwd p) {
  const int slot = (int)threadIdx.x / p.G, c = ((int)threadIdx.x % p.G) * 4;
  if (slot >= p.slots) return;
  f32x4_t w[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    w[k][0] = p.w[(size_t)(c + 0) * 9 + k]; w[k][1] = p.w[(size_t)(c + 1) * 9 + k];
    w[k][2] = p.w[(size_t)(c + 2) * 9 + k]; w[k][3] = p.w[(size_t)(c + 3) * 9 + k];
  }
  const int n = (p.H / 2) * (p.W / 2);
  const long long strip = (long long)blockIdx.x * p.slots * ADW_PIXELS_PER_THREAD;
  for (int it = 0; it < ADW_PIXELS_PER_THREAD; ++it) {
    const long long tok = strip + (long long)it * p.slots + slot;
    if (tok >= p.tokens) return;
    const long long f = tok / p.per_frame;
    const int t = (int)(tok - f * p.per_frame);
    int Hl, Wl, start;
    adw_level(t, p.H, p.W, n, &Hl, &Wl, &start);
    const int py = (t - start) / Wl, px = (t - start) - py * Wl;
    const float* level = p.g + ((size_t)f * p.per_frame + start) * p.C + c;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {   // the output at (py - dy, px - dx) read this token through tap (dy, dx)
      const int yy = py - dy;
      if (yy < 0 || yy >= Hl) continue;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int xx = px - dx;
        if (xx < 0 || xx >= Wl) continue;
        acc += w[(dy + 1) * 3 + dx + 1] * *reinterpret_cast<const f32x4_t*>(level + (size_t)(yy * Wl + xx) * p.C);
      }
    }
    *reinterpret_cast<f32x4_t*>(p.dx + (size_t)tok * p.C + c) = acc;
  }
}

struct SfAdapterFuseBwd {
  const float* dy; float* dtok;
  long long tok_frame_stride;            // floats between two frames of `dtok`
  int level, Ho, Wo, D;
};

__global__ __launch_bounds__(SF_TILE_THREADS) void sf_adapter_fuse_bwd_kernel(SfAdapterFuseBwd p) {
  __shared__ float tile[SF_TILE_CELLS];
  const int f = (int)blockIdx.z, c0 = (int)blockIdx.y * SF_TILE, p0 = (int)blockIdx.x * SF_TILE;
  const int pixels = p.Ho * p.Wo;
  sf_tile_nchw(f, p0, c0, pixels, p.D, [&](int cell, int, size_t o) { tile[cell] = p.dy[o]; });
  __syncthreads();
  sf_tile_scatter_rows(tile, p0, c0, pixels, p.D, [&](int pix, int c, f32x4_t v) {
    size_t row = (size_t)pix;
    if (p.level == 0) {                  // row of the [.., 2Hv * 2Wv, 4 D] GEMM output, column block (dy, dx)
      const int y = pix / p.Wo, x = pix - y * p.Wo;
      row = (size_t)((y >> 1) * (p.Wo >> 1) + (x >> 1)) * 4 + (y & 1) * 2 + (x & 1);
    }
    *reinterpret_cast<f32x4_t*>(p.dtok + (size_t)f * p.tok_frame_stride + row * p.D + c) = v;
  });
}

// ------------------------------------------------------------------------------------------------
// entry points: every refusal happens before anything is launched
// ------------------------------------------------------------------------------------------------
struct AdwBwdCarve { size_t g, part, bytes; long long tokens; int per_frame, slots, per_thread, wgs; };      // offsets in floats

// false: the shape is refused (`code` and `why` say how)
static bool adw_bwd_carve(int F, int H, int W, int C, AdwBwdCarve* w, int* code, const char** why) {
  *code = SF_ERR_INVALID;
  if (F < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) { *why = "F >= 1, H and W even and >= 2 (the levels are 2H x 2W, H x W, H/2 x W/2)"; return false; }
  if (C < 4 || C % 4 || C > 4 * ADW_THREADS) { *why = "C must be a multiple of 4 in 4..1024"; return false; }
  *code = SF_ERR_CAPACITY;
  *why = "more than 2^31 - 1 elements";
  const long long n = (long long)(H / 2) * (W / 2);
  if (n > 0x7fffffffLL / 21) return false;
  const long long per_frame = 21 * n;
  if (per_frame > 0x7fffffffLL / F || per_frame * F > 0x7fffffffLL / C) return false;
  w->tokens = per_frame * F;
  w->per_frame = (int)per_frame;
  w->slots = ADW_THREADS / (C / 4);
  long long per_thread = (w->tokens + (long long)w->slots * ADW_BWD_TARGET_WGS - 1) / ((long long)w->slots * ADW_BWD_TARGET_WGS);
  if (per_thread < ADW_PIXELS_PER_THREAD) per_thread = ADW_PIXELS_PER_THREAD;
  w->per_thread = (int)per_thread;
  const long long per_wg = (long long)w->slots * per_thread;
  w->wgs = (int)((w->tokens + per_wg - 1) / per_wg);
  w->g = 0;
  w->part = (((size_t)w->tokens * C * sizeof(float) + 255) & ~(size_t)255) / sizeof(float);
  w->bytes = ((w->part + (size_t)w->wgs * 10 * C) * sizeof(float) + 255) & ~(size_t)255;
  return true;
}

extern "C" size_t sf_op_adapter_dwconv_gelu_backward_workspace_bytes(int F, int H, int W, int C) {
  AdwBwdCarve w;
  int code;
  const char* why;
  return adw_bwd_carve(F, H, W, C, &w, &code, &why) ? w.bytes : 0;
}

extern "C" int sf_op_adapter_dwconv_gelu_backward(const float* x_dev, const float* w_dev, const float* b_dev, const float* dy_dev, float* dx_dev,
                                                  float* dw_dev, float* db_dev, int F, int H, int W, int C, void* workspace_dev,
                                                  size_t workspace_bytes, sf_stream stream) {
  const char* who = "sf_op_adapter_dwconv_gelu_backward";
  if (!x_dev || !w_dev || !b_dev || !dy_dev || !workspace_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (!dx_dev && !dw_dev && !db_dev) return sf_set_err(SF_ERR_INVALID, "%s: no output", who);
  AdwBwdCarve w;
  int code;
  const char* why;
  if (!adw_bwd_carve(F, H, W, C, &w, &code, &why)) return sf_set_err(code, "%s: F = %d, H = %d, W = %d, C = %d: %s", who, F, H, W, C, why);
  if (dx_dev && (dx_dev == x_dev || dx_dev == dy_dev)) return sf_set_err(SF_ERR_INVALID, "%s: dx must not alias x or dy (every element reads its neighbours)", who);
  if (((uintptr_t)x_dev | (uintptr_t)b_dev | (uintptr_t)dy_dev | (uintptr_t)dx_dev) & 15)
    return sf_set_err(SF_ERR_INVALID, "%s: x, b, dy and dx must be 16-byte aligned", who);
  SF_TRY(sf_check_workspace(who, "sf_op_adapter_dwconv_gelu_backward_workspace_bytes", workspace_dev, workspace_bytes, w.bytes));
  hipStream_t s = (hipStream_t)stream;
  SfAdapterDwBwd p;
  memset(&p, 0, sizeof(p));
  p.x = x_dev; p.w = w_dev; p.b = b_dev; p.dy = dy_dev; p.dx = dx_dev; p.dw = dw_dev; p.db = db_dev;
  p.g = dx_dev ? (float*)workspace_dev + w.g : nullptr;
  p.part = (dw_dev || db_dev) ? (float*)workspace_dev + w.part : nullptr;
  p.tokens = w.tokens; p.H = H; p.W = W; p.C = C; p.G = C / 4; p.per_frame = w.per_frame; p.slots = w.slots; p.per_thread = w.per_thread; p.wgs = w.wgs;
  HIP_TRY(sf_launch(sf_adapter_dw_bwd_g_kernel, dim3((unsigned)w.wgs), dim3(ADW_THREADS), 0, s, p));
  if (p.part)
    HIP_TRY(sf_launch(sf_adapter_dw_bwd_sum_kernel, dim3((unsigned)((10 * C + ADW_SUM_COLS - 1) / ADW_SUM_COLS)), dim3(ADW_SUM_COLS * ADW_SUM_LANES), 0, s, p));
  if (dx_dev) {
    const long long per_block = (long long)p.slots * ADW_PIXELS_PER_THREAD;
    HIP_TRY(sf_launch(sf_adapter_dw_bwd_dx_kernel, dim3((unsigned)((p.tokens + per_block - 1) / per_block)), dim3(ADW_THREADS), 0, s, p));
  }
  return SF_OK;
}

extern "C" int sf_op_adapter_fuse_backward(int level, const float* dy_dev, float* d_tokens_dev, long long tokens_frame_stride, int F, int H, int W,
                                           int D, sf_stream stream) {
  const char* who = "sf_op_adapter_fuse_backward";
  if (level < 0 || level > 3) return sf_set_err(SF_ERR_INVALID, "%s: level = %d outside 0..3 (res2..res5)", who, level);
  if (!dy_dev || !d_tokens_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (F < 1 || F > 65535 || H < 1 || W < 1 || H > 4096 || W > 4096) return sf_set_err(SF_ERR_INVALID, "%s: F = %d (1..65535), H = %d, W = %d (1..4096)", who, F, H, W);
  if (level == 3 && ((H & 1) || (W & 1))) return sf_set_err(SF_ERR_INVALID, "%s: level 3 halves the %d x %d grid: H and W must be even", who, H, W);
  if (D < 4 || D % 4) return sf_set_err(SF_ERR_INVALID, "%s: D = %d must be a multiple of 4", who, D);
  SfAdapterFuseBwd p;
  p.level = level; p.D = D;
  p.Ho = level == 0 ? 4 * H : level == 1 ? 2 * H : level == 2 ? H : H / 2;
  p.Wo = level == 0 ? 4 * W : level == 1 ? 2 * W : level == 2 ? W : W / 2;
  const long long pixels = (long long)p.Ho * p.Wo;
  if (tokens_frame_stride < pixels * D || tokens_frame_stride % 4) return sf_set_err(SF_ERR_INVALID, "%s: tokens_frame_stride = %lld is shorter than a frame of %lld x %d floats, or no multiple of 4", who, tokens_frame_stride, pixels, D);
  if ((uintptr_t)d_tokens_dev & 15) return sf_set_err(SF_ERR_INVALID, "%s: d_tokens must be 16-byte aligned", who);
  p.dy = dy_dev; p.dtok = d_tokens_dev; p.tok_frame_stride = tokens_frame_stride;
  dim3 grid;
  if (!sf_tile_grid(F, D, pixels, &grid)) return sf_set_err(SF_ERR_INVALID, "%s: D = %d exceeds one grid", who, D);
  HIP_TRY(sf_launch(sf_adapter_fuse_bwd_kernel, grid, dim3(SF_TILE_THREADS), 0, (hipStream_t)stream, p));
  return SF_OK;
}
