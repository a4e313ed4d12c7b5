// Backward of the pixel decoder's GroupNorm(32, C) and of its fused bilinear upsample-and-add (sf_pixdec.hip's sf_pixdec_gn_apply_kernel),
// for streamformer_amd/pixel_decoder.py with trainable=True.  fp32 rows [F, HW, C] in and out, the forward's statistics
// [F, 32, 4] (shift, mean - shift, rstd) read as they were written and never recomputed.  No MFMA, no atomics: every element and every sum
// has one owner and one order, so two runs give the same bits.
//
// With xhat = ((x - shift) - delta) rstd and g = dy (zeroed where the forward's ReLU clipped: pxd_gn_value(...) <= 0, the forward's own
// expression), per frame f and channel c
//     b[f, c] = sum over pixels of g          a[f, c] = sum over pixels of g xhat
// carry everything: dbeta_c = sum_f b, dgamma_c = sum_f a, and per (frame, group) of n = HW C / 32 values
//     s1 = sum g gamma = sum_{c in group} gamma_c b[f, c]        s2 = sum g gamma xhat = sum_{c in group} gamma_c a[f, c]
//     dx = rstd (g gamma - s1 / n - xhat s2 / n).
//
//   sf_pixdec_gn_bwd_partial_kernel   a workgroup owns a span of whole pixel rows of one frame and reads x and dy in 16-byte vectors
//                                     across all of C (one row is C / 4 lanes side by side: 1 KB per wave at C = 256), a thread keeps
//                                     the two sums of its four channels in registers over the rows it walks, the row lanes of a
//                                     channel meet through LDS in row-lane order: [F, spans, 2, C] partials.  The span is a function of
//                                     (F, HW) alone.
//   sf_pixdec_gn_bwd_frame_kernel     one workgroup per frame adds the spans in ascending order -> [F, 2, C], then the 32 groups'
//                                     (s1 / n, s2 / n) in ascending channel order -> [F, 32, 2].
//   sf_pixdec_gn_bwd_channel_kernel   dbeta, dgamma: the frames in ascending order.
//   sf_pixdec_gn_bwd_dx_kernel        one streaming pass: x and dy read once, dx written once.
//   sf_pixdec_up_bwd_kernel           the adjoint of `+ bilinear upsample of prev` in gather form: a thread owns a coarse pixel x 8
//                                     channels and walks the fine rows and columns whose sf_bilinear_axis taps land on it, in ascending
//                                     (y, x) order.  The walked range is an estimate widened by one on each side; whether a fine index
//                                     taps the coarse one, and with which weight, is decided by sf_bilinear_axis itself, clamping included.
#include "sf_pixdec.h"

#define PXD_BWD_MIN_SPAN_ROWS 64
#define PXD_BWD_TARGET_WGS 1024

struct SfPxdGnBwd {
  const float *x, *stats, *gamma, *beta, *dy;
  float *part, *frame, *gsum;            // workspace: [F, spans, 2, C], [F, 2, C], [F, G, 2]
  float *dx, *dgamma, *dbeta;            // any of them null
  int F, HW, C, cg, relu, span_rows, spans;
  float n;                               // HW * cg
  unsigned total4;                       // F * HW * C / 4
};

__global__ __launch_bounds__(PXD_THREADS) void sf_pixdec_gn_bwd_partial_kernel(SfPxdGnBwd p) {
  __shared__ f32x4_t red[2 * PXD_THREADS];      // [row lane][b, a][channel vector]
  const int f = (int)blockIdx.y, span = (int)blockIdx.x;
  const int nv = p.C / 4, tpr = nv < PXD_THREADS ? nv : PXD_THREADS, lanes = PXD_THREADS / tpr;      // threads per row, rows in flight
  const int rl = (int)threadIdx.x / tpr, vl = (int)threadIdx.x - rl * tpr;
  const int r0 = span * p.span_rows, r1 = r0 + p.span_rows < p.HW ? r0 + p.span_rows : p.HW;
  float* out = p.part + ((size_t)f * p.spans + span) * 2 * p.C;
  for (int vb = 0; vb < nv; vb += tpr) {
    const int c = (vb + vl) * 4;
    f32x4_t sb = {0.f, 0.f, 0.f, 0.f}, sa = {0.f, 0.f, 0.f, 0.f};
    if (rl < lanes && c < p.C) {
      const f32x4_t gm = *reinterpret_cast<const f32x4_t*>(p.gamma + c), bt = *reinterpret_cast<const f32x4_t*>(p.beta + c);
      float st[4][3];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* q = p.stats + ((size_t)f * PXD_GROUPS + (c + j) / p.cg) * 4;
        st[j][0] = q[0]; st[j][1] = q[1]; st[j][2] = q[2];
      }
      for (int r = r0 + rl; r < r1; r += lanes) {
        const size_t o = ((size_t)f * p.HW + r) * p.C + c;
        const f32x4_t x = *reinterpret_cast<const f32x4_t*>(p.x + o);
        f32x4_t g = *reinterpret_cast<const f32x4_t*>(p.dy + o);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float xhat = ((x[j] - st[j][0]) - st[j][1]) * st[j][2];
          if (p.relu && pxd_gn_value(x[j], st[j], gm[j], bt[j]) <= 0.f) g[j] = 0.f;
          sb[j] += g[j];
          sa[j] += g[j] * xhat;
        }
      }
    }
    if (rl < lanes) {
      red[(rl * 2 + 0) * tpr + vl] = sb;
      red[(rl * 2 + 1) * tpr + vl] = sa;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < 2 * tpr; i += PXD_THREADS) {
      const int k = i / tpr, vv = i - k * tpr;
      if (vb + vv < nv) {
        f32x4_t s = red[k * tpr + vv];
        for (int l = 1; l < lanes; ++l) s += red[(l * 2 + k) * tpr + vv];
        *reinterpret_cast<f32x4_t*>(out + (size_t)k * p.C + (size_t)(vb + vv) * 4) = s;
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(PXD_THREADS) void sf_pixdec_gn_bwd_frame_kernel(SfPxdGnBwd p) {
  const int f = (int)blockIdx.x, n2 = 2 * p.C;
  const float* part = p.part + (size_t)f * p.spans * n2;
  float* fr = p.frame + (size_t)f * n2;
  for (int i = (int)threadIdx.x; i < n2; i += PXD_THREADS) {
    float s = part[i];
    for (int k = 1; k < p.spans; ++k) s += part[(size_t)k * n2 + i];
    fr[i] = s;
  }
  __syncthreads();                       // the frame's sums, written above by this workgroup, are read below
  for (int g = (int)threadIdx.x; g < PXD_GROUPS; g += PXD_THREADS) {
    float s1 = 0.f, s2 = 0.f;
    for (int c = g * p.cg; c < (g + 1) * p.cg; ++c) {
      const float gm = p.gamma[c];
      s1 += gm * fr[c];
      s2 += gm * fr[p.C + c];
    }
    float* o = p.gsum + ((size_t)f * PXD_GROUPS + g) * 2;
    o[0] = s1 / p.n; o[1] = s2 / p.n;
  }
}

__global__ __launch_bounds__(PXD_THREADS) void sf_pixdec_gn_bwd_channel_kernel(SfPxdGnBwd p) {
  const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (c >= p.C) return;
  float sb = p.frame[c], sa = p.frame[p.C + c];
  for (int f = 1; f < p.F; ++f) {
    sb += p.frame[(size_t)f * 2 * p.C + c];
    sa += p.frame[(size_t)f * 2 * p.C + p.C + c];
  }
  if (p.dbeta) p.dbeta[c] = sb;
  if (p.dgamma) p.dgamma[c] = sa;
}

__global__ __launch_bounds__(PXD_THREADS) void sf_pixdec_gn_bwd_dx_kernel(SfPxdGnBwd p) {
  const unsigned C4 = (unsigned)p.C / 4;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < p.total4; i += gridDim.x * blockDim.x) {
    const unsigned r = i / C4;
    const int c = (int)(i - r * C4) * 4, f = (int)(r / (unsigned)p.HW);
    const size_t o = (size_t)r * p.C + c;
    const f32x4_t x = *reinterpret_cast<const f32x4_t*>(p.x + o), g = *reinterpret_cast<const f32x4_t*>(p.dy + o);
    const f32x4_t gm = *reinterpret_cast<const f32x4_t*>(p.gamma + c), bt = *reinterpret_cast<const f32x4_t*>(p.beta + c);
    f32x4_t d;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t fg = (size_t)f * PXD_GROUPS + (c + j) / p.cg;
      const float* st = p.stats + fg * 4;
      const float* m = p.gsum + fg * 2;
      const float xhat = ((x[j] - st[0]) - st[1]) * st[2];
      const float gj = (p.relu && pxd_gn_value(x[j], st, gm[j], bt[j]) <= 0.f) ? 0.f : g[j];
      d[j] = st[2] * ((gj * gm[j] - m[0]) - xhat * m[1]);
    }
    *reinterpret_cast<f32x4_t*>(p.dx + o) = d;
  }
}

static int pxd_bwd_span_rows(int F, int HW) {          // pixel rows per workgroup of the partial pass: a function of (F, HW) alone
  long long rows = ((long long)F * HW + PXD_BWD_TARGET_WGS - 1) / PXD_BWD_TARGET_WGS;
  if (rows < PXD_BWD_MIN_SPAN_ROWS) rows = PXD_BWD_MIN_SPAN_ROWS;
  return (int)(rows < HW ? rows : HW);
}

struct PxdBwdCarve { size_t part, frame, gsum, bytes; int span_rows, spans; };      // offsets in floats

static PxdBwdCarve pxd_bwd_carve(int F, int HW, int C) {
  PxdBwdCarve w;
  w.span_rows = pxd_bwd_span_rows(F, HW);
  w.spans = (HW + w.span_rows - 1) / w.span_rows;
  w.part = 0;
  w.frame = w.part + (size_t)F * w.spans * 2 * C;
  w.gsum = w.frame + (size_t)F * 2 * C;
  w.bytes = ((w.gsum + (size_t)F * PXD_GROUPS * 2) * sizeof(float) + 255) & ~(size_t)255;
  return w;
}

extern "C" size_t sf_op_pixdec_groupnorm_backward_workspace_bytes(int F, int H, int W, int C) {
  if (F < 1 || H < 1 || W < 1 || C < 1 || (long long)F * H * W * C > 0x7fffffffLL) return 0;
  return pxd_bwd_carve(F, H * W, C).bytes;
}

extern "C" int sf_op_pixdec_groupnorm_backward(const float* x_dev, const float* stats_dev, const float* gamma_dev, const float* beta_dev, int relu,
                                               const float* dy_dev, float* dx_dev, float* dgamma_dev, float* dbeta_dev, int F, int H, int W, int C,
                                               void* workspace_dev, size_t workspace_bytes, sf_stream stream) {
  const char* who = "sf_op_pixdec_groupnorm_backward";
  if (!x_dev || !stats_dev || !gamma_dev || !beta_dev || !dy_dev || !workspace_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (!dx_dev && !dgamma_dev && !dbeta_dev) return sf_set_err(SF_ERR_INVALID, "%s: no output", who);
  SF_TRY(pxd_gn_check(who, F, H, W, C));
  if (((uintptr_t)x_dev | (uintptr_t)stats_dev | (uintptr_t)gamma_dev | (uintptr_t)beta_dev | (uintptr_t)dy_dev | (uintptr_t)dx_dev | (uintptr_t)dgamma_dev |
       (uintptr_t)dbeta_dev) & 15)
    return sf_set_err(SF_ERR_INVALID, "%s: every buffer must be 16-byte aligned", who);
  const PxdBwdCarve w = pxd_bwd_carve(F, H * W, C);
  SF_TRY(sf_check_workspace(who, "sf_op_pixdec_groupnorm_backward_workspace_bytes", workspace_dev, workspace_bytes, w.bytes));
  hipStream_t s = (hipStream_t)stream;
  SfPxdGnBwd p;
  memset(&p, 0, sizeof(p));
  p.x = x_dev; p.stats = stats_dev; p.gamma = gamma_dev; p.beta = beta_dev; p.dy = dy_dev;
  p.part = (float*)workspace_dev + w.part; p.frame = (float*)workspace_dev + w.frame; p.gsum = (float*)workspace_dev + w.gsum;
  p.dx = dx_dev; p.dgamma = dgamma_dev; p.dbeta = dbeta_dev;
  p.F = F; p.HW = H * W; p.C = C; p.cg = C / PXD_GROUPS; p.relu = relu ? 1 : 0; p.span_rows = w.span_rows; p.spans = w.spans;
  p.n = (float)((long long)p.HW * p.cg);
  p.total4 = (unsigned)((size_t)F * p.HW * C / 4);
  HIP_TRY(sf_launch(sf_pixdec_gn_bwd_partial_kernel, dim3((unsigned)w.spans, (unsigned)F), dim3(PXD_THREADS), 0, s, p));
  HIP_TRY(sf_launch(sf_pixdec_gn_bwd_frame_kernel, dim3((unsigned)F), dim3(PXD_THREADS), 0, s, p));
  if (dgamma_dev || dbeta_dev)
    HIP_TRY(sf_launch(sf_pixdec_gn_bwd_channel_kernel, dim3((unsigned)((C + PXD_THREADS - 1) / PXD_THREADS)), dim3(PXD_THREADS), 0, s, p));
  if (dx_dev) {
    unsigned block;
    const unsigned grid = pxd_stream_grid(p.total4, &block);
    HIP_TRY(sf_launch(sf_pixdec_gn_bwd_dx_kernel, dim3(grid), dim3(block), 0, s, p));
  }
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// the upsample's adjoint
// ------------------------------------------------------------------------------------------------
struct SfPxdUpBwd {
  const float* dy;                       // [F, H W, C]
  float* dprev;                          // [F, Hp Wp, C]
  int H, W, Hp, Wp, C, C8;
  float ry, rx;                          // Hp / H, Wp / W, as the forward forms them
  unsigned total;                        // F * Hp * Wp * C8
};

// Fine indices that may tap coarse index ip: their source coordinate ratio (i + 0.5) - 0.5 lies in (ip - 1, ip + 1) (below 0 it is
// clamped to 0, which only ip = 0 sees and whose range starts at 0 anyway); one more index on each side pays for the rounding here.
SF_DEVICE void pxd_tap_range(int ip, float ratio, int fine, int* lo, int* hi) {
  const int a = (int)floorf(((float)ip - 0.5f) / ratio - 0.5f) - 1, b = (int)ceilf(((float)ip + 1.5f) / ratio - 0.5f) + 1;
  *lo = a < 0 ? 0 : a;
  *hi = b > fine - 1 ? fine - 1 : b;
}

// the weight with which fine index i reads coarse index ip: sf_bilinear_axis's own taps (both land on ip where the second is clamped)
SF_DEVICE float pxd_tap_weight(int i, float ratio, int coarse, int ip) {
  int i0, i1;
  float l1;
  sf_bilinear_axis(i, ratio, coarse, &i0, &i1, &l1);
  return (i0 == ip ? 1.f - l1 : 0.f) + (i1 == ip ? l1 : 0.f);
}

__global__ __launch_bounds__(PXD_THREADS) void sf_pixdec_up_bwd_kernel(SfPxdUpBwd p) {
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < p.total; i += gridDim.x * blockDim.x) {
    const unsigned r = i / (unsigned)p.C8;                     // f * Hp Wp + coarse pixel
    const int c = (int)(i - r * (unsigned)p.C8) * 8;
    const unsigned f = r / (unsigned)(p.Hp * p.Wp);
    const int pix = (int)(r - f * (unsigned)(p.Hp * p.Wp)), yp = pix / p.Wp, xp = pix - yp * p.Wp;
    int ylo, yhi, xlo, xhi;
    pxd_tap_range(yp, p.ry, p.H, &ylo, &yhi);
    pxd_tap_range(xp, p.rx, p.W, &xlo, &xhi);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* src = p.dy + (size_t)f * p.H * p.W * p.C + c;
    for (int y = ylo; y <= yhi; ++y) {
      const float wy = pxd_tap_weight(y, p.ry, p.Hp, yp);
      if (wy == 0.f) continue;
      for (int x = xlo; x <= xhi; ++x) {
        const float wx = pxd_tap_weight(x, p.rx, p.Wp, xp);
        if (wx == 0.f) continue;
        float v[8];
        pxd_load8(src + ((size_t)y * p.W + x) * p.C, v);
        const float w = wy * wx;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += w * v[j];
      }
    }
    float* o = p.dprev + (size_t)r * p.C + c;
    *reinterpret_cast<f32x4_t*>(o) = (f32x4_t){acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4_t*>(o + 4) = (f32x4_t){acc[4], acc[5], acc[6], acc[7]};
  }
}

extern "C" int sf_op_pixdec_upsample_backward(const float* dy_dev, float* d_prev_dev, int F, int H, int W, int Hp, int Wp, int C, sf_stream stream) {
  const char* who = "sf_op_pixdec_upsample_backward";
  if (!dy_dev || !d_prev_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  SF_TRY(pxd_gn_check(who, F, H, W, C));
  if (Hp < 1 || Wp < 1) return sf_set_err(SF_ERR_INVALID, "%s: the upsampled level is %d x %d", who, Hp, Wp);
  if ((long long)F * Hp * Wp * C > 0x7fffffffLL) return sf_set_err(SF_ERR_CAPACITY, "%s: the upsampled level exceeds 2^31 - 1 elements", who);
  if (((uintptr_t)dy_dev | (uintptr_t)d_prev_dev) & 15) return sf_set_err(SF_ERR_INVALID, "%s: every buffer must be 16-byte aligned", who);
  SfPxdUpBwd p;
  memset(&p, 0, sizeof(p));
  p.dy = dy_dev; p.dprev = d_prev_dev; p.H = H; p.W = W; p.Hp = Hp; p.Wp = Wp; p.C = C; p.C8 = C / 8;
  p.ry = (float)Hp / (float)H; p.rx = (float)Wp / (float)W;
  p.total = (unsigned)((size_t)F * Hp * Wp * p.C8);
  unsigned block;
  const unsigned grid = pxd_stream_grid(p.total, &block);
  HIP_TRY(sf_launch(sf_pixdec_up_bwd_kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream, p));
  return SF_OK;
}
