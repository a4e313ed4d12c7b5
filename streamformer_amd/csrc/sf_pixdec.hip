// Mask2Former pixel decoder (the reference's MSDeformAttnPixelDecoder, downstream/OVIS/mask2former/modeling/pixel_decoder/msdeformattn.py):
// the res2..res5 pyramid [F, C_l, H_l, W_l] -> mask_features [F, mask_dim, H, W] of the finest level and the first three entries of the
// reference's `out` list (the transformer encoder's levels coarsest first, then the FPN levels).  Every Linear and convolution runs on the
// encoder's GEMM launchers (sf_launch_gemm, both compute modes, weights rounded / split ONCE at finalize, the convolutions re-laid out
// there), the sampling on sf_msda.hip's fused forward; this file adds the kernels the decoder needs beside them, the launch sequence and
// the C entry points.  All of them are memory-bound fp32 / bf16 passes: no MFMA, no atomics, one owner per output element, one fixed
// reduction order: the forward is bit-reproducible.
//
// Layouts.  "rows": [F, H W, C] fp32, channels contiguous (what a GEMM writes).  "planes": the same as bf16 hi (+ lo in the accurate mode)
// [rows, C], the A operand of a GEMM.  NCHW only at the two ends.
//
//   sf_pixdec_nchw_planes_kernel   NCHW fp32 -> planes.  sf_nchw_tile.h's 64-pixel x 64-channel tile is read on its NCHW side and
//                                  leaves with 8 lanes x 16 bytes along the channels of a pixel.
//   sf_pixdec_rows_nchw_kernel     rows -> NCHW fp32, the tile's two sides as they are.  A frame stride lets it read one level's slice
//                                  of the flattened [F, S, C] tensor.
//   sf_pixdec_gn_stats_kernel      GroupNorm statistics: one workgroup per (frame, group), TWO passes over the group's H W x C / G values,
//                                  both SHIFTED by a sample of the group (sum of x - shift, then of the squared deviations from the
//                                  mean), and the mean is kept as shift + delta, never added up: the error does not grow with
//                                  mean^2 / variance.  Lane partials meet by xor-shuffles, the four waves through LDS in wave order.
//   sf_pixdec_gn_apply_kernel      y = ((x - shift) - delta) rstd gamma + beta [ReLU] [+ bilinear upsample of the previous level's rows,
//                                  F.interpolate(align_corners=False)'s rule at any ratio], 8 channels per work item, written as any of:
//                                  fp32 rows (at a row offset inside longer frames: a level's slice of [F, S, C]), planes of y, planes of
//                                  y + pos[row] (the query operand of the first encoder layer).
//   sf_pixdec_pos_ref_kernel       PositionEmbeddingSine(C / 2, normalize=True) of an all-false mask + level_embed[l] -> pos [S, C], and
//                                  the reference points ((x + 0.5) / W, (y + 0.5) / H) repeated over levels -> [F, S, L, 2].  The angle
//                                  is formed in fp64 and rounded once (accurate sin / cos, never the fast intrinsics).
//   (sf_rowwise.hip)               the row pass sf_row_kernel, through pxd_launch_postln: LayerNorm of a row (the residual was added by
//                                  the GEMM epilogue in front): the fp32 row, its planes and the planes of y + pos[row % S] in one
//                                  pass, so nothing stands between an encoder layer and the next one's two GEMMs.
//   sf_pixdec_im2col_kernel        3 x 3 gather: the nine taps of each pixel side by side, [rows, 9 C] planes in (dy, dx, c) order, 16-byte
//                                  vectors.  Boundary rule (the one sf_msda.hip and sf_adapter.hip state): a tap is addressed only after its
//                                  coordinates passed the range test against the frame's OWN grid; a tap outside is written as zero
//                                  and never read, so it cannot land on the neighbouring row or the next frame.
//
// The 3 x 3 convolution is that gather followed by ONE GEMM with K = 9 C, in chunks of im2col_chunk_rows pixels so that the gathered
// planes stay bounded (SfGemmArgs has no A row pitch; a chunk is a contiguous [rows, 9 C] operand).
#include "sf_pixdec.h"

#define PXD_MAX_LEVELS 4
#define PXD_LN_EPS 1e-5f
#define PXD_DEFAULT_CHUNK_ROWS 16384

// ------------------------------------------------------------------------------------------------
// NCHW <-> rows
// ------------------------------------------------------------------------------------------------
struct SfPxdMove {
  const float* in; float* out; bf16_t* out_hi; bf16_t* out_lo;
  long long frame_stride;               // rows -> NCHW: floats between two frames of `in`
  int C, HW;
};

__global__ __launch_bounds__(SF_TILE_THREADS) void sf_pixdec_nchw_planes_kernel(SfPxdMove p) {
  __shared__ float tile[SF_TILE_CELLS];
  const int f = (int)blockIdx.z, c0 = (int)blockIdx.y * SF_TILE, p0 = (int)blockIdx.x * SF_TILE;
  sf_tile_nchw(f, p0, c0, p.HW, p.C, [&](int cell, int, size_t o) { tile[cell] = p.in[o]; });
  __syncthreads();
  const int c8 = ((int)threadIdx.x % 8) * 8;
  if (c0 + c8 >= p.C) return;
  for (int pp = (int)threadIdx.x / 8; pp < SF_TILE; pp += SF_TILE_THREADS / 8) {
    if (p0 + pp >= p.HW) break;
    store_planes8(tile + pp * SF_TILE_LD + c8, p.out_hi, p.out_lo, ((size_t)f * p.HW + p0 + pp) * p.C + c0 + c8);
  }
}

__global__ __launch_bounds__(SF_TILE_THREADS) void sf_pixdec_rows_nchw_kernel(SfPxdMove p) {
  __shared__ float tile[SF_TILE_CELLS];
  const int f = (int)blockIdx.z, c0 = (int)blockIdx.y * SF_TILE, p0 = (int)blockIdx.x * SF_TILE;
  sf_tile_gather_rows(tile, p0, c0, p.HW, p.C, [&](int pix, int c) {
    return *reinterpret_cast<const f32x4_t*>(p.in + (size_t)f * p.frame_stride + (size_t)pix * p.C + c);
  });
  __syncthreads();
  sf_tile_nchw(f, p0, c0, p.HW, p.C, [&](int cell, int, size_t o) { p.out[o] = tile[cell]; });
}

static int pxd_move_check(const char* who, int F, int C, int HW, int cmul) {
  if (F < 1 || F > 65535) return sf_set_err(SF_ERR_INVALID, "%s: F = %d outside 1..65535", who, F);
  if (C < cmul || C % cmul) return sf_set_err(SF_ERR_INVALID, "%s: C = %d must be a positive multiple of %d", who, C, cmul);
  if (HW < 1) return sf_set_err(SF_ERR_INVALID, "%s: %d pixels per frame", who, HW);
  if ((long long)F * HW * C > 0x7fffffffLL) return sf_set_err(SF_ERR_CAPACITY, "%s: %d frames of %d x %d exceed 2^31 - 1 elements", who, F, HW, C);
  dim3 grid;
  if (!sf_tile_grid(F, C, HW, &grid)) return sf_set_err(SF_ERR_INVALID, "%s: C = %d exceeds one grid", who, C);
  return SF_OK;
}

static hipError_t pxd_launch_nchw_planes(const float* x, bf16_t* hi, bf16_t* lo, int F, int C, int HW, hipStream_t s) {
  SfPxdMove p;
  memset(&p, 0, sizeof(p));
  p.in = x; p.out_hi = hi; p.out_lo = lo; p.C = C; p.HW = HW;
  dim3 grid;
  if (!sf_tile_grid(F, C, HW, &grid)) return hipErrorInvalidValue;
  return sf_launch(sf_pixdec_nchw_planes_kernel, grid, dim3(SF_TILE_THREADS), 0, s, p);
}

static hipError_t pxd_launch_rows_nchw(const float* rows, long long frame_stride, float* out, int F, int C, int HW, hipStream_t s) {
  SfPxdMove p;
  memset(&p, 0, sizeof(p));
  p.in = rows; p.out = out; p.frame_stride = frame_stride; p.C = C; p.HW = HW;
  dim3 grid;
  if (!sf_tile_grid(F, C, HW, &grid)) return hipErrorInvalidValue;
  return sf_launch(sf_pixdec_rows_nchw_kernel, grid, dim3(SF_TILE_THREADS), 0, s, p);
}

// ------------------------------------------------------------------------------------------------
// GroupNorm
// ------------------------------------------------------------------------------------------------
struct SfPxdGn {
  const float* x;                        // [F, HW, C] rows
  float* stats;                          // [F, G, 4] shift, mean - shift, rstd, 0
  const float* gamma; const float* beta;
  const float* prev; long long prev_frame_stride; int Hp, Wp;      // + bilinear upsample of prev [.., Hp Wp, C] (null: none)
  float ry, rx;                          // Hp / H, Wp / W
  float* y; bf16_t* y_hi; bf16_t* y_lo;  // any of them null; rows at out_row0 inside frames of out_frame_rows rows
  const float* pos; bf16_t* q_hi; bf16_t* q_lo;      // planes of y + pos[out_row0 + pixel]
  long long out_frame_rows; int out_row0;
  int F, H, W, HW, C, G, cg, C8, relu;
  float eps;
  unsigned total;                        // F * HW * C8
};

SF_DEVICE float pxd_block_sum(float v, float* red) {      // the same value in every thread; wave order fixed
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(PXD_THREADS) void sf_pixdec_gn_stats_kernel(SfPxdGn p) {
  __shared__ float red[4];
  const int f = (int)blockIdx.x / p.G, g = (int)blockIdx.x % p.G;
  const float* base = p.x + (size_t)f * p.HW * p.C + (size_t)g * p.cg;
  const int n = p.HW * p.cg;
  const float shift = base[0];           // a sample of the group: the sums below are of deviations, whatever the group's mean is
  float s = 0.f;
  for (int i = (int)threadIdx.x; i < n; i += PXD_THREADS) s += base[(size_t)(i / p.cg) * p.C + i % p.cg] - shift;
  const float delta = pxd_block_sum(s, red) / (float)n;      // mean - shift
  float q = 0.f;
  for (int i = (int)threadIdx.x; i < n; i += PXD_THREADS) {
    const float d = (base[(size_t)(i / p.cg) * p.C + i % p.cg] - shift) - delta;
    q += d * d;
  }
  const float var = pxd_block_sum(q, red) / (float)n;
  if (threadIdx.x == 0) {
    float* st = p.stats + (size_t)blockIdx.x * 4;
    st[0] = shift; st[1] = delta; st[2] = 1.0f / sqrtf(var + p.eps); st[3] = 0.f;
  }
}

__global__ __launch_bounds__(PXD_THREADS) void sf_pixdec_gn_apply_kernel(SfPxdGn p) {
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < p.total; i += gridDim.x * blockDim.x) {
    const unsigned r = i / (unsigned)p.C8;
    const int c = (int)(i - r * (unsigned)p.C8) * 8;
    const int f = (int)(r / (unsigned)p.HW), pix = (int)(r - (unsigned)f * p.HW);
    float v[8], gm[8], bt[8];
    pxd_load8(p.x + (size_t)r * p.C + c, v);
    pxd_load8(p.gamma + c, gm);
    pxd_load8(p.beta + c, bt);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float* st = p.stats + ((size_t)f * p.G + (c + j) / p.cg) * 4;
      v[j] = pxd_gn_value(v[j], st, gm[j], bt[j]);
      if (p.relu) v[j] = fmaxf(v[j], 0.f);
    }
    if (p.prev) {
      const int y = pix / p.W, x = pix - y * p.W;
      int y0, y1, x0, x1;
      float ly, lx;
      sf_bilinear_axis(y, p.ry, p.Hp, &y0, &y1, &ly);
      sf_bilinear_axis(x, p.rx, p.Wp, &x0, &x1, &lx);
      const float* src = p.prev + (size_t)f * p.prev_frame_stride + c;
      float v00[8], v01[8], v10[8], v11[8];
      pxd_load8(src + (size_t)(y0 * p.Wp + x0) * p.C, v00); pxd_load8(src + (size_t)(y0 * p.Wp + x1) * p.C, v01);
      pxd_load8(src + (size_t)(y1 * p.Wp + x0) * p.C, v10); pxd_load8(src + (size_t)(y1 * p.Wp + x1) * p.C, v11);
      const float hy = 1.f - ly, hx = 1.f - lx;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] += hy * (hx * v00[j] + lx * v01[j]) + ly * (hx * v10[j] + lx * v11[j]);
    }
    const size_t o = ((size_t)f * p.out_frame_rows + p.out_row0 + pix) * p.C + c;
    if (p.y) {
      *reinterpret_cast<f32x4_t*>(p.y + o) = (f32x4_t){v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4_t*>(p.y + o + 4) = (f32x4_t){v[4], v[5], v[6], v[7]};
    }
    if (p.y_hi) store_planes8(v, p.y_hi, p.y_lo, o);
    if (p.q_hi) {
      float e[8];
      pxd_load8(p.pos + (size_t)(p.out_row0 + pix) * p.C + c, e);
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] += v[j];
      store_planes8(e, p.q_hi, p.q_lo, o);
    }
  }
}

// x, gamma, beta, prev, pos and every output 16-byte aligned, C % (8 * G / gcd) ...: checked by the callers (pxd_gn_check, sf_pixdec.h)
static hipError_t pxd_launch_groupnorm(const SfPxdGn& q, hipStream_t s) {
  SfPxdGn p = q;
  p.HW = p.H * p.W; p.G = PXD_GROUPS; p.cg = p.C / PXD_GROUPS; p.C8 = p.C / 8; p.eps = PXD_GN_EPS;
  p.total = (unsigned)((size_t)p.F * p.HW * p.C8);
  if (p.prev) { p.ry = (float)p.Hp / (float)p.H; p.rx = (float)p.Wp / (float)p.W; }
  hipError_t e = sf_launch(sf_pixdec_gn_stats_kernel, dim3((unsigned)(p.F * p.G)), dim3(PXD_THREADS), 0, s, p);
  if (e != hipSuccess) return e;
  unsigned block;
  const unsigned grid = pxd_stream_grid(p.total, &block);
  return sf_launch(sf_pixdec_gn_apply_kernel, dim3(grid), dim3(block), 0, s, p);
}

// ------------------------------------------------------------------------------------------------
// position table and reference points
// ------------------------------------------------------------------------------------------------
struct SfPxdGeom { int H[PXD_MAX_LEVELS], W[PXD_MAX_LEVELS], start[PXD_MAX_LEVELS]; };
struct SfPxdPos {
  const float* level_embed;              // [L, C]
  float* pos;                            // [S, C]
  float* ref;                            // [F, S, L, 2]
  int F, S, L, C;
  SfPxdGeom g;
};

__global__ __launch_bounds__(PXD_THREADS) void sf_pixdec_pos_ref_kernel(SfPxdPos p) {
  const int npf = p.C / 2;
  const size_t n_pos = (size_t)p.S * p.C, n_ref = (size_t)p.F * p.S * p.L;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pos + n_ref; i += (size_t)gridDim.x * blockDim.x) {
    const bool is_pos = i < n_pos;
    const size_t k = is_pos ? i : i - n_pos;
    const int s = is_pos ? (int)(k / p.C) : (int)((k / p.L) % p.S);
    int l = 0;
    for (int j = 1; j < p.L; ++j) l = s >= p.g.start[j] ? j : l;
    const int pix = s - p.g.start[l], y = pix / p.g.W[l], x = pix - y * p.g.W[l];
    if (is_pos) {
      const int c = (int)(k - (size_t)s * p.C);
      const bool xhalf = c >= npf;
      const int j = xhalf ? c - npf : c;
      const double embed = xhalf ? (double)(x + 1) / ((double)p.g.W[l] + 1e-6) : (double)(y + 1) / ((double)p.g.H[l] + 1e-6);
      const double angle = embed * 6.283185307179586476925 / pow(10000.0, (double)(2 * (j / 2)) / (double)npf);
      const float e = (float)((j & 1) ? cos(angle) : sin(angle));
      p.pos[k] = e + p.level_embed[(size_t)l * p.C + c];
    } else {
      p.ref[k * 2] = ((float)x + 0.5f) / (float)p.g.W[l];
      p.ref[k * 2 + 1] = ((float)y + 0.5f) / (float)p.g.H[l];
    }
  }
}

static int pxd_geom(const char* who, const int32_t* shapes, int L, SfPxdGeom* g, int* S) {
  if (!shapes) return sf_set_err(SF_ERR_INVALID, "%s: null level shapes (a host array of (H, W) pairs)", who);
  if (L < 1 || L > PXD_MAX_LEVELS) return sf_set_err(SF_ERR_INVALID, "%s: %d levels outside 1..%d", who, L, PXD_MAX_LEVELS);
  long long sum = 0;
  memset(g, 0, sizeof(*g));
  for (int l = 0; l < L; ++l) {
    const long long H = shapes[2 * l], W = shapes[2 * l + 1];
    if (H < 1 || W < 1 || H > 4096 || W > 4096) return sf_set_err(SF_ERR_INVALID, "%s: level %d is %lld x %lld (1..4096 each)", who, l, H, W);
    g->H[l] = (int)H; g->W[l] = (int)W; g->start[l] = (int)sum;
    sum += H * W;
  }
  if (sum > 0x7fffffffLL / 1024) return sf_set_err(SF_ERR_CAPACITY, "%s: %lld pixels per frame exceed the index range", who, sum);
  *S = (int)sum;
  return SF_OK;
}

static hipError_t pxd_launch_pos_ref(const SfPxdPos& p, hipStream_t s) {
  const size_t total = (size_t)p.S * p.C + (size_t)p.F * p.S * p.L;
  size_t grid = (total + PXD_THREADS - 1) / PXD_THREADS;
  if (grid > 2048) grid = 2048;
  return sf_launch(sf_pixdec_pos_ref_kernel, dim3((unsigned)grid), dim3(PXD_THREADS), 0, s, p);
}

// ------------------------------------------------------------------------------------------------
// post-LN with planes
// ------------------------------------------------------------------------------------------------
// LayerNorm always; the q planes (y + pos[row % pos_mod]) only where q_hi is given.  Shapes and alignment: checked by the callers.
static hipError_t pxd_launch_postln(const float* x, const SfDevLN& ln, float eps, const float* pos, int pos_mod, float* y, bf16_t* y_hi, bf16_t* y_lo,
                                    bf16_t* q_hi, bf16_t* q_lo, int rows, int C, hipStream_t s) {
  if (!x || !ln.g || !ln.b || rows < 1 || (q_hi && (!pos || pos_mod < 1))) return hipErrorInvalidValue;
  SfRowArgs p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.gamma = ln.g; p.beta = ln.b; p.eps = eps; p.rows = rows; p.D = C;
  p.y = y; p.y_hi = y_hi; p.y_lo = y_lo;
  if (q_hi) { p.pe = pos; p.pe_mod = pos_mod; p.q_hi = q_hi; p.q_lo = q_lo; }
  return sf_launch_row(p, s);
}

// ------------------------------------------------------------------------------------------------
// 3 x 3 gather and the convolution on it
// ------------------------------------------------------------------------------------------------
struct SfPxdCol {
  const bf16_t* in_hi; const bf16_t* in_lo;      // [F, H W, C] planes (lo may be null)
  bf16_t* out_hi; bf16_t* out_lo;                // [n_rows, 9 C]
  int H, W, HW, C, C8;
  long long row0;                                // first pixel row (f * HW + pixel) of this chunk
  unsigned total;                                // n_rows * 9 * C8
};

__global__ __launch_bounds__(PXD_THREADS) void sf_pixdec_im2col_kernel(SfPxdCol p) {
  const unsigned per_row = 9u * (unsigned)p.C8;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < p.total; i += gridDim.x * blockDim.x) {
    const unsigned r = i / per_row, k = i - r * per_row;
    const int tap = (int)(k / (unsigned)p.C8), c = (int)(k - (unsigned)tap * p.C8) * 8;
    const long long row = p.row0 + r;
    const long long f = row / p.HW;
    const int pix = (int)(row - f * p.HW), y = pix / p.W, x = pix - y * p.W;
    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    const bool inside = yy >= 0 && yy < p.H && xx >= 0 && xx < p.W;      // against the frame's own grid, before any address is formed
    u32x4_t h = {0u, 0u, 0u, 0u}, l = {0u, 0u, 0u, 0u};
    if (inside) {
      const size_t e = ((size_t)f * p.HW + (size_t)yy * p.W + xx) * p.C + c;
      h = *reinterpret_cast<const u32x4_t*>(p.in_hi + e);
      if (p.in_lo) l = *reinterpret_cast<const u32x4_t*>(p.in_lo + e);
    }
    const size_t o = (size_t)r * 9 * p.C + (size_t)tap * p.C + c;
    *reinterpret_cast<u32x4_t*>(p.out_hi + o) = h;
    if (p.out_lo) *reinterpret_cast<u32x4_t*>(p.out_lo + o) = l;
  }
}

// rows [row0, row0 + n) of F frames of H x W; n * 9 * C below 2^31 and every pointer 16-byte aligned: checked by the callers
static hipError_t pxd_launch_im2col(const bf16_t* in_hi, const bf16_t* in_lo, bf16_t* out_hi, bf16_t* out_lo, int H, int W, int C, long long row0,
                                    int n, hipStream_t s) {
  SfPxdCol p;
  p.in_hi = in_hi; p.in_lo = in_lo; p.out_hi = out_hi; p.out_lo = out_lo;
  p.H = H; p.W = W; p.HW = H * W; p.C = C; p.C8 = C / 8; p.row0 = row0;
  p.total = (unsigned)((size_t)n * 9 * p.C8);
  unsigned block;
  const unsigned grid = pxd_stream_grid(p.total, &block);
  return sf_launch(sf_pixdec_im2col_kernel, dim3(grid), dim3(block), 0, s, p);
}

static int pxd_chunk_rows(int requested, int C) {
  long long rows = requested > 0 ? requested : PXD_DEFAULT_CHUNK_ROWS;
  const long long cap = 0x7fffffffLL / (9LL * C);      // a chunk's plane is indexed with 32 bits by the GEMMs
  return (int)(rows < cap ? rows : cap);
}

// out [F H W, N] fp32 = conv3x3(in planes, w [N, 9 C] in (dy, dx, c) order), padding 1, no bias; col: [chunk, 9 C] planes
static int pxd_conv3x3(const SfPlanes& in, const SfDevLinear& w, int F, int H, int W, int C, int chunk, const SfPlanes& col, float* out,
                       const SfLinearCaller& lin) {
  const long long rows = (long long)F * H * W;
  for (long long r0 = 0; r0 < rows; r0 += chunk) {
    const int n = (int)(rows - r0 < chunk ? rows - r0 : chunk);
    HIP_TRY(pxd_launch_im2col(in.hi, in.lo, col.hi, col.lo, H, W, C, r0, n, lin.stream));
    HIP_TRY(lin.f32(w, col, n, out + (size_t)r0 * w.N));
  }
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
struct PxdEncLayer {
  SfDevLinear value, front, out, lin1, lin2;      // front: [sampling_offsets; attention_weights]
  SfDevLN norm1, norm2;
};
struct PxdFpn { SfDevLinear lateral, conv; SfDevLN lateral_norm, conv_norm; };

struct sf_pixdec : SfModelHandle {
  sf_pixdec_config cfg;
  int n_tr = 0, n_fpn = 0;
  int tr_level[PXD_MAX_LEVELS];              // input level of transformer level j, coarsest first
  std::vector<SfDevLinear> proj;             // input_proj.{j}.0
  std::vector<SfDevLN> proj_norm;            // input_proj.{j}.1
  const float* level_embed = nullptr;
  std::vector<PxdEncLayer> layers;
  std::vector<PxdFpn> fpn;                   // [k]: adapter_{k + 1} / layer_{k + 1}, input level k
  SfDevLinear mask;
};

static int pxd_log2_floor(int v) {
  int n = 0;
  while ((1 << (n + 1)) <= v) ++n;
  return n;
}

extern "C" int sf_pixdec_create(const sf_pixdec_config* cfg, int device, sf_pixdec** out) {
  const char* who = "sf_pixdec_create";
  if (!cfg || !out) return sf_set_err(SF_ERR_INVALID, "%s: null argument", who);
  const sf_pixdec_config& c = *cfg;
  if (c.norm != SF_PIXDEC_NORM_GN) return sf_set_err(SF_ERR_INVALID, "%s: norm %d: only \"GN\" (GroupNorm(32, conv_dim)) runs natively", who, c.norm);
  if (c.num_levels < 1 || c.num_levels > PXD_MAX_LEVELS) return sf_set_err(SF_ERR_INVALID, "%s: num_levels %d outside 1..%d", who, c.num_levels, PXD_MAX_LEVELS);
  if (c.conv_dim <= 0 || c.conv_dim % 64) return sf_set_err(SF_ERR_INVALID, "%s: conv_dim %d must be a positive multiple of 64 (the GEMM kernels' k-step)", who, c.conv_dim);
  if (c.conv_dim % PXD_GROUPS) return sf_set_err(SF_ERR_INVALID, "%s: conv_dim %d must be a multiple of 32 (GroupNorm(32, conv_dim))", who, c.conv_dim);
  if (c.dim_feedforward <= 0 || c.dim_feedforward % 64) return sf_set_err(SF_ERR_INVALID, "%s: dim_feedforward %d must be a positive multiple of 64 (the GEMM kernels' k-step)", who, c.dim_feedforward);
  if (c.mask_dim < 4 || c.mask_dim % 4) return sf_set_err(SF_ERR_INVALID, "%s: mask_dim %d must be a positive multiple of 4", who, c.mask_dim);
  if (c.nheads < 1 || c.conv_dim % c.nheads || (c.conv_dim / c.nheads) % 8 || c.conv_dim / c.nheads < 8 || c.conv_dim / c.nheads > 128)
    return sf_set_err(SF_ERR_INVALID, "%s: conv_dim / nheads = %d / %d must be a multiple of 8 in 8..128 (deformable attention's channels per head)", who, c.conv_dim, c.nheads);
  if (c.enc_n_points < 1 || c.enc_n_points > 8) return sf_set_err(SF_ERR_INVALID, "%s: enc_n_points %d outside 1..8", who, c.enc_n_points);
  if (c.enc_layers < 0 || c.enc_layers > 64) return sf_set_err(SF_ERR_INVALID, "%s: enc_layers %d outside 0..64", who, c.enc_layers);
  if (c.common_stride < 1) return sf_set_err(SF_ERR_INVALID, "%s: common_stride %d must be >= 1", who, c.common_stride);
  if (c.im2col_chunk_rows < 0) return sf_set_err(SF_ERR_INVALID, "%s: im2col_chunk_rows %d must be >= 0 (0: the library's default)", who, c.im2col_chunk_rows);
  sf_pixdec* h = new sf_pixdec();
  h->cfg = c;
  h->device = device;
  int first_tr = -1;
  for (int l = 0; l < c.num_levels; ++l) {
    if (c.channels[l] <= 0 || c.channels[l] % 64) {
      delete h;
      return sf_set_err(SF_ERR_INVALID, "%s: channels[%d] = %d must be a positive multiple of 64 (the GEMM kernels' k-step)", who, l, c.channels[l]);
    }
    if (c.strides[l] < 1 || (l && c.strides[l] <= c.strides[l - 1])) {
      delete h;
      return sf_set_err(SF_ERR_INVALID, "%s: strides[%d] = %d: the levels are listed by increasing stride", who, l, c.strides[l]);
    }
    if (c.in_transformer[l] && first_tr < 0) first_tr = l;
  }
  for (int l = c.num_levels - 1; l >= 0; --l)
    if (c.in_transformer[l]) h->tr_level[h->n_tr++] = l;
  if (h->n_tr < 1) {
    delete h;
    return sf_set_err(SF_ERR_INVALID, "%s: in_transformer names no level", who);
  }
  h->n_fpn = pxd_log2_floor(c.strides[first_tr]) - pxd_log2_floor(c.common_stride);
  if (h->n_fpn < 0) h->n_fpn = 0;
  if (h->n_fpn > first_tr) {
    const int n_fpn = h->n_fpn;
    delete h;
    return sf_set_err(SF_ERR_INVALID, "%s: common_stride %d asks for %d FPN levels but only %d input levels are finer than the transformer's finest", who,
                      c.common_stride, n_fpn, first_tr);
  }
  const int64_t C = c.conv_dim, Fd = c.dim_feedforward, n_front = (int64_t)c.nheads * h->n_tr * c.enc_n_points;
  SfWeightStore& w = h->weights;
  w.noun = "pixel decoder";
  w.prefix = "sem_seg_head.pixel_decoder.";
  w.dtype_msg = "sf_pixdec_load_tensor: dtype %d unsupported (fp32, fp64, bf16)";
  for (int j = 0; j < h->n_tr; ++j) {
    const std::string p = "input_proj." + std::to_string(j) + ".";
    w.expected[p + "0.weight"] = {C, c.channels[h->tr_level[j]], 1, 1};
    w.expected[p + "0.bias"] = {C};
    w.expect_affine(p + "1.", C);
  }
  w.expected["transformer.level_embed"] = {h->n_tr, C};
  for (int i = 0; i < c.enc_layers; ++i) {
    const std::string p = "transformer.encoder.layers." + std::to_string(i) + ".";
    w.expect_linear(p + "self_attn.sampling_offsets.", 2 * n_front, C);
    w.expect_linear(p + "self_attn.attention_weights.", n_front, C);
    w.expect_linear(p + "self_attn.value_proj.", C, C);
    w.expect_linear(p + "self_attn.output_proj.", C, C);
    w.expect_linear(p + "linear1.", Fd, C);
    w.expect_linear(p + "linear2.", C, Fd);
    w.expect_affine(p + "norm1.", C);
    w.expect_affine(p + "norm2.", C);
  }
  w.expected["mask_features.weight"] = {c.mask_dim, C, 1, 1};
  w.expected["mask_features.bias"] = {c.mask_dim};
  for (int k = 0; k < h->n_fpn; ++k) {
    const std::string a = "adapter_" + std::to_string(k + 1) + ".", l = "layer_" + std::to_string(k + 1) + ".";
    w.expected[a + "weight"] = {C, c.channels[k], 1, 1};
    w.expected[l + "weight"] = {C, C, 3, 3};
    w.expect_affine(a + "norm.", C);
    w.expect_affine(l + "norm.", C);
  }
  *out = h;
  return SF_OK;
}

extern "C" void sf_pixdec_destroy(sf_pixdec* h) { delete h; }

extern "C" int sf_pixdec_load_tensor(sf_pixdec* h, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
  return sf_model_load_tensor(h, "sf_pixdec_load_tensor", key, host_ptr, dtype, shape, ndim);
}

extern "C" int sf_pixdec_missing_weights(sf_pixdec* h) { return sf_model_missing_weights(h); }

// Weights rounded (bf16 mode) or split into hi + lo planes (bf16x3) ONCE, here; the 1 x 1 convolutions are [O, I] as they are, the 3 x 3
// ones are re-laid out [O, (dy, dx, c_in)] for the gathered operand.  Makes the handle's device current and leaves it so.
extern "C" int sf_pixdec_finalize(sf_pixdec* h, int compute) {
  SF_TRY(sf_model_begin_finalize(h, compute));
  const bool lo = compute == SF_COMPUTE_BF16X3;
  const sf_pixdec_config& c = h->cfg;
  const int C = c.conv_dim, Fd = c.dim_feedforward;
  SfWeightStore& w = h->weights;
  auto linear = [&](const std::string& p, int N, int K, bool bias, SfDevLinear* out) {
    return sf_upload_linear(h->dev, w.data(p + "weight"), bias ? &w.data(p + "bias") : nullptr, N, K, N, lo, out);
  };
  h->proj.assign(h->n_tr, SfDevLinear());
  h->proj_norm.assign(h->n_tr, SfDevLN());
  for (int j = 0; j < h->n_tr; ++j) {
    const std::string p = "input_proj." + std::to_string(j) + ".";
    SF_TRY(linear(p + "0.", C, c.channels[h->tr_level[j]], true, &h->proj[j]));
    SF_TRY(sf_upload_ln(h->dev, w, p + "1.", &h->proj_norm[j]));
  }
  SF_TRY(h->dev.upload(w.data("transformer.level_embed"), &h->level_embed));
  h->layers.assign(c.enc_layers, PxdEncLayer());
  const int n_front = c.nheads * h->n_tr * c.enc_n_points;
  for (int i = 0; i < c.enc_layers; ++i) {
    const std::string p = "transformer.encoder.layers." + std::to_string(i) + ".";
    PxdEncLayer& L = h->layers[i];
    SF_TRY(linear(p + "self_attn.value_proj.", C, C, true, &L.value));
    std::vector<float> fw = w.data(p + "self_attn.sampling_offsets.weight"), fb = w.data(p + "self_attn.sampling_offsets.bias");
    const std::vector<float>&aw = w.data(p + "self_attn.attention_weights.weight"), &ab = w.data(p + "self_attn.attention_weights.bias");
    fw.insert(fw.end(), aw.begin(), aw.end());
    fb.insert(fb.end(), ab.begin(), ab.end());
    SF_TRY(sf_upload_linear(h->dev, fw, &fb, 3 * n_front, C, 3 * n_front, lo, &L.front));
    SF_TRY(linear(p + "self_attn.output_proj.", C, C, true, &L.out));
    SF_TRY(linear(p + "linear1.", Fd, C, true, &L.lin1));
    SF_TRY(linear(p + "linear2.", C, Fd, true, &L.lin2));
    SF_TRY(sf_upload_ln(h->dev, w, p + "norm1.", &L.norm1));
    SF_TRY(sf_upload_ln(h->dev, w, p + "norm2.", &L.norm2));
  }
  SF_TRY(linear("mask_features.", c.mask_dim, C, true, &h->mask));
  h->fpn.assign(h->n_fpn, PxdFpn());
  for (int k = 0; k < h->n_fpn; ++k) {
    const std::string a = "adapter_" + std::to_string(k + 1) + ".", l = "layer_" + std::to_string(k + 1) + ".";
    SF_TRY(linear(a, C, c.channels[k], false, &h->fpn[k].lateral));
    const std::vector<float>& src = w.data(l + "weight");      // [O, I, 3, 3] -> [O, (dy, dx), I]
    std::vector<float> re((size_t)C * 9 * C);
    for (int o = 0; o < C; ++o)
      for (int i = 0; i < C; ++i)
        for (int t = 0; t < 9; ++t) re[((size_t)o * 9 + t) * C + i] = src[((size_t)o * C + i) * 9 + t];
    SF_TRY(sf_upload_linear(h->dev, re, nullptr, C, 9 * C, C, lo, &h->fpn[k].conv));
    SF_TRY(sf_upload_ln(h->dev, w, a + "norm.", &h->fpn[k].lateral_norm));
    SF_TRY(sf_upload_ln(h->dev, w, l + "norm.", &h->fpn[k].conv_norm));
  }
  h->finalized = true;
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
struct PxdPlan {
  int F, S;                              // frames; pixels per frame over the transformer's levels
  int H[PXD_MAX_LEVELS], W[PXD_MAX_LEVELS];      // per input level
  int32_t tr_shapes[2 * PXD_MAX_LEVELS], tr_start[PXD_MAX_LEVELS];
  SfPxdGeom geom;                        // the transformer's levels, coarsest first
  int64_t Mt, Mf, Min;                   // rows of the transformer; of the largest FPN level; elements of the largest input level
  int chunk;                             // im2col rows per GEMM
  int n_out;                             // entries of the reference's `out` that are returned: min(3, n_tr + n_fpn)
};

static int pxd_plan(const sf_pixdec* h, int F, const int32_t* level_shapes, int num_levels, PxdPlan* pl) {
  const char* who = "sf_pixdec";
  if (!h) return sf_set_err(SF_ERR_INVALID, "null handle");
  if (F < 1 || F > 65535) return sf_set_err(SF_ERR_INVALID, "%s: %d frames outside 1..65535", who, F);
  if (num_levels != h->cfg.num_levels) return sf_set_err(SF_ERR_INVALID, "%s: %d level shapes given, the decoder was created with %d input levels", who, num_levels, h->cfg.num_levels);
  if (!level_shapes) return sf_set_err(SF_ERR_INVALID, "%s: null level shapes (a host array of (H, W) pairs)", who);
  memset(pl, 0, sizeof(*pl));
  pl->F = F;
  for (int l = 0; l < num_levels; ++l) {
    pl->H[l] = level_shapes[2 * l]; pl->W[l] = level_shapes[2 * l + 1];
    if (pl->H[l] < 1 || pl->W[l] < 1 || pl->H[l] > 4096 || pl->W[l] > 4096)
      return sf_set_err(SF_ERR_INVALID, "%s: level %d is %d x %d (1..4096 each)", who, l, pl->H[l], pl->W[l]);
  }
  for (int j = 0; j < h->n_tr; ++j) {
    pl->tr_shapes[2 * j] = pl->H[h->tr_level[j]];
    pl->tr_shapes[2 * j + 1] = pl->W[h->tr_level[j]];
  }
  SF_TRY(pxd_geom(who, pl->tr_shapes, h->n_tr, &pl->geom, &pl->S));
  for (int j = 0; j < h->n_tr; ++j) pl->tr_start[j] = pl->geom.start[j];
  pl->Mt = (int64_t)F * pl->S;
  for (int j = 0; j < h->n_tr; ++j) {
    const int l = h->tr_level[j];
    pl->Min = std::max(pl->Min, (int64_t)F * pl->H[l] * pl->W[l] * h->cfg.channels[l]);
  }
  for (int k = 0; k < h->n_fpn; ++k) {
    pl->Mf = std::max(pl->Mf, (int64_t)F * pl->H[k] * pl->W[k]);
    pl->Min = std::max(pl->Min, (int64_t)F * pl->H[k] * pl->W[k] * h->cfg.channels[k]);
  }
  const int64_t wide = std::max<int64_t>(std::max(h->cfg.conv_dim, h->cfg.dim_feedforward), std::max(h->cfg.mask_dim, 3 * h->cfg.nheads * h->n_tr * h->cfg.enc_n_points));
  if (pl->Min > 0x7fffffffLL || std::max(pl->Mt, pl->Mf) * wide > 0x7fffffffLL)
    return sf_set_err(SF_ERR_CAPACITY, "%s: %d frames of these levels exceed 2^31 - 1 elements per activation; decode in groups of frames", who, F);
  pl->chunk = pxd_chunk_rows(h->cfg.im2col_chunk_rows, h->cfg.conv_dim);
  if (pl->Mf && pl->chunk > pl->Mf) pl->chunk = (int)pl->Mf;
  pl->n_out = std::min(3, h->n_tr + h->n_fpn);
  return SF_OK;
}

struct PxdWorkspace {
  float *pos, *ref, *stats;
  SfPlanes in;                           // an input level as planes
  float* pre;                            // a GEMM's output in front of its GroupNorm [max rows, C]
  float *src, *tmp, *value, *front, *ctx;
  SfPlanes a, q, c, h;                   // GEMM operands: src, src + pos, the attention's output, the FFN's hidden rows
  SfPlanes sum, col, fo_p;               // FPN: lateral + upsampled, the gathered 3 x 3 operand, the finest output
  float* fo[2];                          // FPN outputs, ping-pong: the previous level is the next one's upsample source
  float* mf;                             // mask_features as rows
  size_t bytes;
};

static PxdWorkspace pxd_carve(const sf_pixdec* h, const PxdPlan& pl, void* base) {
  PxdWorkspace w;
  memset(&w, 0, sizeof(w));
  SfCarver cv(base, h->compute == SF_COMPUTE_BF16X3);
  const size_t C = h->cfg.conv_dim, Fd = h->cfg.dim_feedforward, Mt = (size_t)pl.Mt, Mf = (size_t)pl.Mf;
  const size_t NF = (size_t)3 * h->cfg.nheads * h->n_tr * h->cfg.enc_n_points;
  w.pos = cv.take<float>((size_t)pl.S * C);
  w.ref = cv.take<float>(Mt * h->n_tr * 2);
  w.stats = cv.take<float>((size_t)pl.F * PXD_GROUPS * 4);
  w.in = cv.planes((size_t)pl.Min);
  w.pre = cv.take<float>(std::max(Mt, Mf) * C);
  w.src = cv.take<float>(Mt * C);
  w.a = cv.planes(Mt * C);
  if (h->cfg.enc_layers) {
    w.tmp = cv.take<float>(Mt * C);
    w.value = cv.take<float>(Mt * C);
    w.front = cv.take<float>(Mt * NF);
    w.ctx = cv.take<float>(Mt * C);
    w.q.hi = cv.take<bf16_t>(Mt * C);      // the three hi planes, then the three lo planes
    w.c.hi = cv.take<bf16_t>(Mt * C);
    w.h.hi = cv.take<bf16_t>(Mt * Fd);
    w.q.lo = cv.lo(Mt * C); w.c.lo = cv.lo(Mt * C); w.h.lo = cv.lo(Mt * Fd);
  }
  if (h->n_fpn) {
    w.sum.hi = cv.take<bf16_t>(Mf * C);
    w.col.hi = cv.take<bf16_t>((size_t)pl.chunk * 9 * C);
    w.fo_p.hi = cv.take<bf16_t>(Mf * C);
    w.sum.lo = cv.lo(Mf * C); w.col.lo = cv.lo((size_t)pl.chunk * 9 * C); w.fo_p.lo = cv.lo(Mf * C);
    w.fo[0] = cv.take<float>(Mf * C);
    w.fo[1] = cv.take<float>(Mf * C);
  }
  w.mf = cv.take<float>((h->n_fpn ? Mf : Mt) * h->cfg.mask_dim);
  w.bytes = cv.bytes();
  return w;
}

extern "C" int sf_pixdec_workspace_bytes(sf_pixdec* h, int F, const int32_t* level_shapes, int num_levels, size_t* out) {
  if (!out) return sf_set_err(SF_ERR_INVALID, "null argument");
  PxdPlan pl;
  SF_TRY(pxd_plan(h, F, level_shapes, num_levels, &pl));
  SF_TRY(sf_model_check_finalized(h, "sf_pixdec", true));
  *out = pxd_carve(h, pl, nullptr).bytes;
  return SF_OK;
}

extern "C" int sf_pixdec_num_outputs(sf_pixdec* h, int* num_multi_scale, int* num_fpn_levels) {
  if (!h) return sf_set_err(SF_ERR_INVALID, "null handle");
  if (num_multi_scale) *num_multi_scale = std::min(3, h->n_tr + h->n_fpn);
  if (num_fpn_levels) *num_fpn_levels = h->n_fpn;
  return SF_OK;
}

extern "C" int sf_pixdec_forward(sf_pixdec* h, const float* const* features_dev, int F, const int32_t* level_shapes, int num_levels,
                                 float* mask_features_dev, float* const* multi_scale_dev, int num_multi_scale, void* workspace_dev,
                                 size_t workspace_bytes, sf_stream stream) {
  const char* who = "sf_pixdec_forward";
  PxdPlan pl;
  SF_TRY(pxd_plan(h, F, level_shapes, num_levels, &pl));
  SF_TRY(sf_model_check_finalized(h, "sf_pixdec"));
  if (!features_dev || !mask_features_dev || !multi_scale_dev || !workspace_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (num_multi_scale != pl.n_out) return sf_set_err(SF_ERR_INVALID, "%s: %d multi-scale outputs given, this decoder returns %d (sf_pixdec_num_outputs)", who, num_multi_scale, pl.n_out);
  const sf_pixdec_config& cfg = h->cfg;
  uintptr_t bits = (uintptr_t)mask_features_dev;
  for (int l = 0; l < num_levels; ++l) {
    const bool used = cfg.in_transformer[l] || l < h->n_fpn;
    if (used && !features_dev[l]) return sf_set_err(SF_ERR_INVALID, "%s: features_dev[%d] is null", who, l);
    if (used) bits |= (uintptr_t)features_dev[l];
  }
  for (int i = 0; i < pl.n_out; ++i) {
    if (!multi_scale_dev[i]) return sf_set_err(SF_ERR_INVALID, "%s: multi_scale_dev[%d] is null", who, i);
    bits |= (uintptr_t)multi_scale_dev[i];
  }
  if (bits & 15) return sf_set_err(SF_ERR_INVALID, "%s: features and outputs must be 16-byte aligned", who);
  const PxdWorkspace ws = pxd_carve(h, pl, workspace_dev);
  SF_TRY(sf_check_workspace(who, "sf_pixdec_workspace_bytes", workspace_dev, workspace_bytes, ws.bytes));
  hipStream_t s = (hipStream_t)stream;
  const SfLinearCaller lin{h->compute == SF_COMPUTE_BF16X3, 2, s};      // act 2: ReLU
  const int C = cfg.conv_dim, S = pl.S, L = h->n_tr, Mt = (int)pl.Mt;

  // ---- position table (+ level_embed) and reference points ----
  {
    SfPxdPos p;
    memset(&p, 0, sizeof(p));
    p.level_embed = h->level_embed; p.pos = ws.pos; p.ref = ws.ref; p.F = F; p.S = S; p.L = L; p.C = C; p.g = pl.geom;
    HIP_TRY(pxd_launch_pos_ref(p, s));
  }
  // ---- input projections: 1 x 1 convolution + GroupNorm into the level's slice of [F, S, C], coarsest first ----
  for (int j = 0; j < L; ++j) {
    const int l = h->tr_level[j], HW = pl.H[l] * pl.W[l];
    HIP_TRY(pxd_launch_nchw_planes(features_dev[l], ws.in.hi, ws.in.lo, F, cfg.channels[l], HW, s));
    HIP_TRY(lin.f32(h->proj[j], ws.in, F * HW, ws.pre));
    SfPxdGn n;
    memset(&n, 0, sizeof(n));
    n.x = ws.pre; n.stats = ws.stats; n.gamma = h->proj_norm[j].g; n.beta = h->proj_norm[j].b;
    n.F = F; n.H = pl.H[l]; n.W = pl.W[l]; n.C = C;
    n.y = ws.src; n.y_hi = ws.a.hi; n.y_lo = ws.a.lo;
    if (cfg.enc_layers) { n.pos = ws.pos; n.q_hi = ws.q.hi; n.q_lo = ws.q.lo; }
    n.out_frame_rows = S; n.out_row0 = pl.geom.start[j];
    HIP_TRY(pxd_launch_groupnorm(n, s));
  }
  // ---- encoder layers (post-norm, ReLU) ----
  const int n_front = cfg.nheads * L * cfg.enc_n_points;
  for (int i = 0; i < cfg.enc_layers; ++i) {
    const PxdEncLayer& ly = h->layers[i];
    const bool last = i + 1 == cfg.enc_layers;
    HIP_TRY(lin.f32(ly.value, ws.a, Mt, ws.value));
    HIP_TRY(lin.f32(ly.front, ws.q, Mt, ws.front));
    SF_TRY(sf_op_msda_forward_fused(ws.value, nullptr, pl.tr_shapes, pl.tr_start, ws.front, 3 * n_front, ws.front + 2 * n_front, 3 * n_front, ws.ref, 2,
                                    ws.ctx, F, S, cfg.nheads, C / cfg.nheads, S, L, cfg.enc_n_points, stream));
    HIP_TRY(sf_launch_split(ws.ctx, ws.c.hi, ws.c.lo, (size_t)Mt * C, s));
    HIP_TRY(lin.resid(ly.out, ws.c, Mt, ws.src, ws.tmp));
    HIP_TRY(pxd_launch_postln(ws.tmp, ly.norm1, PXD_LN_EPS, nullptr, 0, ws.src, ws.a.hi, ws.a.lo, nullptr, nullptr, Mt, C, s));
    HIP_TRY(lin.planes(ly.lin1, ws.a, Mt, ws.h, true));
    HIP_TRY(lin.resid(ly.lin2, ws.h, Mt, ws.src, ws.tmp));
    HIP_TRY(pxd_launch_postln(ws.tmp, ly.norm2, PXD_LN_EPS, ws.pos, S, ws.src, ws.a.hi, ws.a.lo, last ? nullptr : ws.q.hi, ws.q.lo, Mt, C, s));
  }
  // ---- the transformer's levels among the outputs ----
  for (int j = 0; j < L && j < pl.n_out; ++j) {
    const int l = h->tr_level[j];
    HIP_TRY(pxd_launch_rows_nchw(ws.src + (size_t)pl.geom.start[j] * C, (long long)S * C, multi_scale_dev[j], F, C, pl.H[l] * pl.W[l], s));
  }
  // ---- FPN levels, coarse to fine ----
  const float* prev = ws.src + (size_t)pl.geom.start[L - 1] * C;
  long long prev_stride = (long long)S * C;
  int Hp = pl.H[h->tr_level[L - 1]], Wp = pl.W[h->tr_level[L - 1]];
  for (int k = h->n_fpn - 1, idx = 0; k >= 0; --k, ++idx) {
    const PxdFpn& fp = h->fpn[k];
    const int H = pl.H[k], W = pl.W[k], M = F * H * W;
    HIP_TRY(pxd_launch_nchw_planes(features_dev[k], ws.in.hi, ws.in.lo, F, cfg.channels[k], H * W, s));
    HIP_TRY(lin.f32(fp.lateral, ws.in, M, ws.pre));
    SfPxdGn n;
    memset(&n, 0, sizeof(n));
    n.x = ws.pre; n.stats = ws.stats; n.gamma = fp.lateral_norm.g; n.beta = fp.lateral_norm.b;
    n.F = F; n.H = H; n.W = W; n.C = C;
    n.prev = prev; n.prev_frame_stride = prev_stride; n.Hp = Hp; n.Wp = Wp;
    n.y_hi = ws.sum.hi; n.y_lo = ws.sum.lo; n.out_frame_rows = H * W;
    HIP_TRY(pxd_launch_groupnorm(n, s));
    SF_TRY(pxd_conv3x3(ws.sum, fp.conv, F, H, W, C, pl.chunk, ws.col, ws.pre, lin));
    float* fo = ws.fo[idx & 1];
    memset(&n, 0, sizeof(n));
    n.x = ws.pre; n.stats = ws.stats; n.gamma = fp.conv_norm.g; n.beta = fp.conv_norm.b; n.relu = 1;
    n.F = F; n.H = H; n.W = W; n.C = C; n.out_frame_rows = H * W;
    n.y = fo;
    if (k == 0) { n.y_hi = ws.fo_p.hi; n.y_lo = ws.fo_p.lo; }
    HIP_TRY(pxd_launch_groupnorm(n, s));
    if (L + idx < pl.n_out) HIP_TRY(pxd_launch_rows_nchw(fo, (long long)H * W * C, multi_scale_dev[L + idx], F, C, H * W, s));
    prev = fo; prev_stride = (long long)H * W * C; Hp = H; Wp = W;
  }
  // ---- mask_features: 1 x 1 convolution with bias on the finest rows ----
  {
    const bool fpn = h->n_fpn > 0;
    const int M = fpn ? F * Hp * Wp : Mt;      // without an FPN level: all rows of [F, S, C]; the finest level's slice leaves
    HIP_TRY(lin.f32(h->mask, fpn ? ws.fo_p : ws.a, M, ws.mf));
    const float* rows = fpn ? ws.mf : ws.mf + (size_t)pl.geom.start[L - 1] * cfg.mask_dim;
    const long long stride = fpn ? (long long)Hp * Wp * cfg.mask_dim : (long long)S * cfg.mask_dim;
    HIP_TRY(pxd_launch_rows_nchw(rows, stride, mask_features_dev, F, cfg.mask_dim, Hp * Wp, s));
  }
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// the kernels alone (parity tests)
// ------------------------------------------------------------------------------------------------
extern "C" int sf_op_pixdec_nchw_to_planes(const float* x_dev, uint16_t* hi_dev, uint16_t* lo_dev, int F, int C, int HW, sf_stream stream) {
  const char* who = "sf_op_pixdec_nchw_to_planes";
  if (!x_dev || !hi_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  SF_TRY(pxd_move_check(who, F, C, HW, 8));
  if (((uintptr_t)x_dev | (uintptr_t)hi_dev | (uintptr_t)lo_dev) & 15) return sf_set_err(SF_ERR_INVALID, "%s: every buffer must be 16-byte aligned", who);
  HIP_TRY(pxd_launch_nchw_planes(x_dev, hi_dev, lo_dev, F, C, HW, (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_op_pixdec_rows_to_nchw(const float* rows_dev, long long frame_stride, float* out_dev, int F, int C, int HW, sf_stream stream) {
  const char* who = "sf_op_pixdec_rows_to_nchw";
  if (!rows_dev || !out_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  SF_TRY(pxd_move_check(who, F, C, HW, 4));
  if (frame_stride < (long long)HW * C || frame_stride % 4) return sf_set_err(SF_ERR_INVALID, "%s: frame_stride = %lld is shorter than a frame of %d x %d floats, or no multiple of 4", who, frame_stride, HW, C);
  if (((uintptr_t)rows_dev | (uintptr_t)out_dev) & 15) return sf_set_err(SF_ERR_INVALID, "%s: every buffer must be 16-byte aligned", who);
  HIP_TRY(pxd_launch_rows_nchw(rows_dev, frame_stride, out_dev, F, C, HW, (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_op_pixdec_groupnorm(const float* x_dev, const float* gamma_dev, const float* beta_dev, int relu, const float* prev_dev, int Hp,
                                      int Wp, const float* pos_dev, float* stats_dev, float* y_dev, uint16_t* y_hi_dev, uint16_t* y_lo_dev,
                                      uint16_t* q_hi_dev, uint16_t* q_lo_dev, int F, int H, int W, int C, sf_stream stream) {
  const char* who = "sf_op_pixdec_groupnorm";
  if (!x_dev || !gamma_dev || !beta_dev || !stats_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (!y_dev && !y_hi_dev && !q_hi_dev) return sf_set_err(SF_ERR_INVALID, "%s: no output", who);
  if ((y_lo_dev && !y_hi_dev) || (q_lo_dev && !q_hi_dev)) return sf_set_err(SF_ERR_INVALID, "%s: a lo plane needs its hi plane", who);
  if (q_hi_dev && !pos_dev) return sf_set_err(SF_ERR_INVALID, "%s: the q planes (y + pos) need pos_dev", who);
  SF_TRY(pxd_gn_check(who, F, H, W, C));
  if (prev_dev && (Hp < 1 || Wp < 1 || Hp > 4096 || Wp > 4096)) return sf_set_err(SF_ERR_INVALID, "%s: the upsampled level is %d x %d", who, Hp, Wp);
  if (prev_dev && (long long)F * Hp * Wp * C > 0x7fffffffLL) return sf_set_err(SF_ERR_CAPACITY, "%s: the upsampled level exceeds 2^31 - 1 elements", who);
  if (((uintptr_t)x_dev | (uintptr_t)gamma_dev | (uintptr_t)beta_dev | (uintptr_t)prev_dev | (uintptr_t)pos_dev | (uintptr_t)y_dev | (uintptr_t)y_hi_dev |
       (uintptr_t)y_lo_dev | (uintptr_t)q_hi_dev | (uintptr_t)q_lo_dev) & 15)
    return sf_set_err(SF_ERR_INVALID, "%s: every buffer must be 16-byte aligned", who);
  SfPxdGn n;
  memset(&n, 0, sizeof(n));
  n.x = x_dev; n.stats = stats_dev; n.gamma = gamma_dev; n.beta = beta_dev; n.relu = relu ? 1 : 0;
  n.prev = prev_dev; n.prev_frame_stride = (long long)Hp * Wp * C; n.Hp = Hp; n.Wp = Wp;
  n.F = F; n.H = H; n.W = W; n.C = C; n.out_frame_rows = (long long)H * W;
  n.y = y_dev; n.y_hi = y_hi_dev; n.y_lo = y_lo_dev; n.pos = pos_dev; n.q_hi = q_hi_dev; n.q_lo = q_lo_dev;
  HIP_TRY(pxd_launch_groupnorm(n, (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_op_pixdec_pos_ref(const float* level_embed_dev, const int32_t* level_shapes, int L, int F, int C, float* pos_dev, float* ref_dev,
                                    sf_stream stream) {
  const char* who = "sf_op_pixdec_pos_ref";
  if (!level_embed_dev || !pos_dev || !ref_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (F < 1) return sf_set_err(SF_ERR_INVALID, "%s: %d frames", who, F);
  if (C < 4 || C % 4) return sf_set_err(SF_ERR_INVALID, "%s: C = %d must be a positive multiple of 4 (sin / cos pairs of the y half and the x half)", who, C);
  SfPxdPos p;
  memset(&p, 0, sizeof(p));
  SF_TRY(pxd_geom(who, level_shapes, L, &p.g, &p.S));
  if ((long long)F * p.S * L * 2 > 0x7fffffffLL || (long long)p.S * C > 0x7fffffffLL) return sf_set_err(SF_ERR_CAPACITY, "%s: tables exceed 2^31 - 1 elements", who);
  p.level_embed = level_embed_dev; p.pos = pos_dev; p.ref = ref_dev; p.F = F; p.L = L; p.C = C;
  HIP_TRY(pxd_launch_pos_ref(p, (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_op_pixdec_postln(const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps, const float* pos_dev, int pos_rows,
                                   float* y_dev, uint16_t* y_hi_dev, uint16_t* y_lo_dev, uint16_t* q_hi_dev, uint16_t* q_lo_dev, int rows, int C,
                                   sf_stream stream) {
  const char* who = "sf_op_pixdec_postln";
  if (!x_dev || !gamma_dev || !beta_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (!y_dev && !y_hi_dev && !q_hi_dev) return sf_set_err(SF_ERR_INVALID, "%s: no output", who);
  if ((y_lo_dev && !y_hi_dev) || (q_lo_dev && !q_hi_dev)) return sf_set_err(SF_ERR_INVALID, "%s: a lo plane needs its hi plane", who);
  if (q_hi_dev && (!pos_dev || pos_rows < 1)) return sf_set_err(SF_ERR_INVALID, "%s: the q planes (y + pos[row %% pos_rows]) need pos_dev and pos_rows >= 1", who);
  if (rows < 1 || C < 4 || C % 4 || (long long)rows * C > 0x7fffffffLL) return sf_set_err(SF_ERR_INVALID, "%s: rows = %d, C = %d (a multiple of 4; rows * C below 2^31)", who, rows, C);
  if (((uintptr_t)x_dev | (uintptr_t)gamma_dev | (uintptr_t)beta_dev | (uintptr_t)pos_dev | (uintptr_t)y_dev | (uintptr_t)y_hi_dev | (uintptr_t)y_lo_dev |
       (uintptr_t)q_hi_dev | (uintptr_t)q_lo_dev) & 15)
    return sf_set_err(SF_ERR_INVALID, "%s: every buffer must be 16-byte aligned", who);
  SfDevLN ln;
  ln.g = gamma_dev; ln.b = beta_dev;
  HIP_TRY(pxd_launch_postln(x_dev, ln, eps, pos_dev, pos_rows, y_dev, y_hi_dev, y_lo_dev, q_hi_dev, q_lo_dev, rows, C, (hipStream_t)stream));
  return SF_OK;
}

static int pxd_col_check(const char* who, int F, int H, int W, int C) {
  if (F < 1 || H < 1 || W < 1 || H > 4096 || W > 4096) return sf_set_err(SF_ERR_INVALID, "%s: F = %d, H = %d, W = %d", who, F, H, W);
  if (C < 64 || C % 64) return sf_set_err(SF_ERR_INVALID, "%s: C = %d must be a positive multiple of 64 (the GEMM kernels' k-step)", who, C);
  if ((long long)F * H * W * C > 0x7fffffffLL) return sf_set_err(SF_ERR_CAPACITY, "%s: %d frames of %d x %d x %d exceed 2^31 - 1 elements", who, F, H, W, C);
  return SF_OK;
}

extern "C" int sf_op_pixdec_im2col(const uint16_t* in_hi_dev, const uint16_t* in_lo_dev, int F, int H, int W, int C, long long row0, int rows,
                                   uint16_t* out_hi_dev, uint16_t* out_lo_dev, sf_stream stream) {
  const char* who = "sf_op_pixdec_im2col";
  if (!in_hi_dev || !out_hi_dev || (!in_lo_dev) != (!out_lo_dev)) return sf_set_err(SF_ERR_INVALID, "%s: hi planes in and out, lo planes both or neither", who);
  SF_TRY(pxd_col_check(who, F, H, W, C));
  if (row0 < 0 || rows < 1 || row0 + rows > (long long)F * H * W || (long long)rows * 9 * C > 0x7fffffffLL)
    return sf_set_err(SF_ERR_INVALID, "%s: rows [%lld, %lld) outside the %d x %d x %d pixels, or above 2^31 - 1 gathered elements", who, row0, row0 + rows, F, H, W);
  if (((uintptr_t)in_hi_dev | (uintptr_t)in_lo_dev | (uintptr_t)out_hi_dev | (uintptr_t)out_lo_dev) & 15)
    return sf_set_err(SF_ERR_INVALID, "%s: every buffer must be 16-byte aligned", who);
  HIP_TRY(pxd_launch_im2col(in_hi_dev, in_lo_dev, out_hi_dev, out_lo_dev, H, W, C, row0, rows, (hipStream_t)stream));
  return SF_OK;
}

extern "C" size_t sf_op_pixdec_conv3x3_workspace_bytes(int F, int H, int W, int C, int chunk_rows) {
  if (F < 1 || H < 1 || W < 1 || C < 1) return 0;
  long long chunk = pxd_chunk_rows(chunk_rows, C);
  if (chunk > (long long)F * H * W) chunk = (long long)F * H * W;
  return ((size_t)chunk * 9 * C * 2 + 256) * 2;
}

extern "C" int sf_op_pixdec_conv3x3(const uint16_t* in_hi_dev, const uint16_t* in_lo_dev, const uint16_t* w_hi_dev, const uint16_t* w_lo_dev, int F,
                                    int H, int W, int C, int N, int chunk_rows, float* out_dev, void* workspace_dev, size_t workspace_bytes,
                                    sf_stream stream) {
  const char* who = "sf_op_pixdec_conv3x3";
  if (!in_hi_dev || !w_hi_dev || !out_dev || !workspace_dev || (!in_lo_dev) != (!w_lo_dev))
    return sf_set_err(SF_ERR_INVALID, "%s: null buffer (lo planes of the input and of the weight: both or neither)", who);
  SF_TRY(pxd_col_check(who, F, H, W, C));
  if (N < 4 || N % 4 || (long long)F * H * W * N > 0x7fffffffLL) return sf_set_err(SF_ERR_INVALID, "%s: N = %d must be a positive multiple of 4", who, N);
  if (chunk_rows < 0) return sf_set_err(SF_ERR_INVALID, "%s: chunk_rows %d must be >= 0 (0: the library's default)", who, chunk_rows);
  if (((uintptr_t)in_hi_dev | (uintptr_t)in_lo_dev | (uintptr_t)w_hi_dev | (uintptr_t)w_lo_dev | (uintptr_t)out_dev) & 15)
    return sf_set_err(SF_ERR_INVALID, "%s: every buffer must be 16-byte aligned", who);
  SF_TRY(sf_check_workspace(who, "sf_op_pixdec_conv3x3_workspace_bytes", workspace_dev, workspace_bytes, sf_op_pixdec_conv3x3_workspace_bytes(F, H, W, C, chunk_rows)));
  long long chunk = pxd_chunk_rows(chunk_rows, C);
  if (chunk > (long long)F * H * W) chunk = (long long)F * H * W;
  const SfLinearCaller lin{in_lo_dev != nullptr, 0, (hipStream_t)stream};
  SfCarver cv(workspace_dev, lin.split, true);      // the workspace holds both planes in either mode
  SfPlanes in;                                       // read only
  in.hi = const_cast<uint16_t*>(in_hi_dev); in.lo = const_cast<uint16_t*>(in_lo_dev);
  SfDevLinear w;
  w.w_hi = w_hi_dev; w.w_lo = w_lo_dev; w.N = N; w.K = 9 * C;
  return pxd_conv3x3(in, w, F, H, W, C, (int)chunk, cv.planes((size_t)chunk * 9 * C), out_dev, lin);
}
