// The transpose tile between channel-contiguous rows [F, HW, C] and pixel-contiguous NCHW [F, C, HW], shared by sf_pixdec.hip's two
// move kernels, sf_adapter.hip's fuse kernel and its adjoint in sf_adapter_bwd.hip: 64 pixels x 64 channels of fp32 in LDS, rows padded to 65 floats so that a column read
// touches 64 different banks, 256 threads.  The rows side moves 16 lanes x float4 along the channels of a pixel (256 B), the NCHW side
// 64 lanes along the pixels of a channel row (256 B).  A kernel declares `__shared__ float tile[SF_TILE_CELLS]`, takes its tile from
// blockIdx (x: pixels, y: channels, z: frame; sf_tile_grid) and puts __syncthreads() between the two sides.  Also here: the bilinear
// resampling rule both files apply to rows.
#pragma once
#include "sf_common.h"

#define SF_TILE 64                       // pixels and channels of one tile
#define SF_TILE_LD (SF_TILE + 1)
#define SF_TILE_CELLS (SF_TILE * SF_TILE_LD)      // cell (pixel pp, channel cc) at pp * SF_TILE_LD + cc
#define SF_TILE_THREADS 256

// rows -> tile.  load(pix, c): the four values of channels c .. c + 3 of pixel pix (both inside HW x C, C % 4 == 0)
template <typename Load>
SF_DEVICE void sf_tile_gather_rows(float* tile, int p0, int c0, int HW, int C, Load load) {
  const int lane_c = ((int)threadIdx.x % 16) * 4, lane_p = (int)threadIdx.x / 16;
  if (c0 + lane_c >= C) return;
  for (int pp = lane_p; pp < SF_TILE; pp += SF_TILE_THREADS / 16) {
    if (p0 + pp >= HW) break;
    const f32x4_t v = load(p0 + pp, c0 + lane_c);
    float* row = tile + pp * SF_TILE_LD + lane_c;
    row[0] = v[0]; row[1] = v[1]; row[2] = v[2]; row[3] = v[3];
  }
}

// tile -> rows.  store(pix, c, v): the four values of channels c .. c + 3 of pixel pix (both inside HW x C, C % 4 == 0)
template <typename Store>
SF_DEVICE void sf_tile_scatter_rows(const float* tile, int p0, int c0, int HW, int C, Store store) {
  const int lane_c = ((int)threadIdx.x % 16) * 4, lane_p = (int)threadIdx.x / 16;
  if (c0 + lane_c >= C) return;
  for (int pp = lane_p; pp < SF_TILE; pp += SF_TILE_THREADS / 16) {
    if (p0 + pp >= HW) break;
    const float* row = tile + pp * SF_TILE_LD + lane_c;
    store(p0 + pp, c0 + lane_c, (f32x4_t){row[0], row[1], row[2], row[3]});
  }
}

// The NCHW side, either direction.  visit(cell, ch, o): tile cell, channel and element offset into [F, C, HW] of every element of
// frame f's tile inside HW x C
template <typename Visit>
SF_DEVICE void sf_tile_nchw(int f, int p0, int c0, int HW, int C, Visit visit) {
  const int lane = (int)threadIdx.x % 64;
  if (p0 + lane >= HW) return;
  for (int cc = (int)threadIdx.x / 64; cc < SF_TILE; cc += SF_TILE_THREADS / 64) {
    if (c0 + cc >= C) break;
    visit(lane * SF_TILE_LD + cc, c0 + cc, ((size_t)f * C + c0 + cc) * HW + p0 + lane);
  }
}

// The launch grid over [F, C, HW].  False: C needs more channel tiles than grid.y takes (F beyond grid.z: refused by the callers, in
// their own words)
static inline bool sf_tile_grid(int F, int C, long long HW, dim3* grid) {
  *grid = dim3((unsigned)((HW + SF_TILE - 1) / SF_TILE), (unsigned)((C + SF_TILE - 1) / SF_TILE), (unsigned)F);
  return grid->y <= 65535;
}

// one axis of F.interpolate(mode="bilinear", align_corners=False): source index pair and the weight of the second
SF_DEVICE void sf_bilinear_axis(int dst, float ratio, int in, int* i0, int* i1, float* l1) {
  float src = ratio * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  int a = (int)src;
  a = a > in - 1 ? in - 1 : a;
  *i0 = a;
  *i1 = a + 1 <= in - 1 ? a + 1 : in - 1;
  const float l = src - (float)a;
  *l1 = l > 1.f ? 1.f : l;
}
