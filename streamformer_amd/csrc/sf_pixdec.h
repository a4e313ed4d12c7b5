// What sf_pixdec.hip (the decoder's forward) and sf_pixdec_bwd.hip (GroupNorm's backward) share: the GroupNorm constants, the 8-channel
// load, the normalised value as ONE expression (the backward's ReLU mask is the forward's, bit for bit, because both compile this
// line), the streaming grid and the shape check of the GroupNorm entries.
#pragma once
#include "sf_handle.h"
#include "sf_nchw_tile.h"

#define PXD_THREADS 256
#define PXD_GROUPS 32
#define PXD_GN_EPS 1e-5f

SF_DEVICE void pxd_load8(const float* q, float v[8]) {
  const f32x4_t a = *reinterpret_cast<const f32x4_t*>(q), b = *reinterpret_cast<const f32x4_t*>(q + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
}

// st: shift, mean - shift, rstd of the element's (frame, group).  (x - shift) - (mean - shift): the mean itself is never rounded
SF_DEVICE float pxd_gn_value(float x, const float* st, float gm, float bt) { return ((x - st[0]) - st[1]) * st[2] * gm + bt; }

static inline unsigned pxd_stream_grid(unsigned total, unsigned* block) {
  *block = total < 65536u ? 64u : 256u;
  const unsigned grid = (total + *block - 1) / *block;
  return grid > 2048u ? 2048u : (grid ? grid : 1u);
}

static inline int pxd_gn_check(const char* who, int F, int H, int W, int C) {
  if (F < 1 || F > 65535 || H < 1 || W < 1) return sf_set_err(SF_ERR_INVALID, "%s: F = %d (1..65535), H = %d, W = %d", who, F, H, W);
  if (C < 64 || C % 64) return sf_set_err(SF_ERR_INVALID, "%s: C = %d must be a positive multiple of 64 (GroupNorm(32, C) in 16-byte vectors)", who, C);
  if ((long long)F * H * W * C > 0x7fffffffLL) return sf_set_err(SF_ERR_CAPACITY, "%s: %d frames of %d x %d x %d exceed 2^31 - 1 elements", who, F, H, W, C);
  return SF_OK;
}
