// The coordinate arithmetic of the mask resampling, shared by sf_vis.hip and sf_seg.hip: one definition, so that every kernel and every
// entry point (which sizes the LDS with these very functions) gets the same bits.
#pragma once
#include <hip/hip_runtime.h>

// F.interpolate(bilinear, align_corners=False) along one axis: output index -> the two source indices and the second one's weight
__host__ __device__ static inline void vis_axis(int dst, float ratio, int in, int* i0, int* i1, float* l1) {
  float src = fmaf(ratio, (float)dst + 0.5f, -0.5f);        // one correctly rounded operation: the same bits on the host and on the device
  src = src < 0.f ? 0.f : src;
  int a = (int)src;
  a = a > in - 1 ? in - 1 : a;
  *i0 = a;
  *i1 = a < in - 1 ? a + 1 : a;
  const float l = src - (float)a;
  *l1 = l > 1.f ? 1.f : l;
}

// the source rows (columns) that output rows (columns) a..b reach: both maps are non-decreasing
__host__ __device__ static inline void vis_reach(int a, int b, float r2, int crop, float r1, int in, int* lo, int* hi) {
  int m0, m1, s0, s1;
  float l;
  vis_axis(a, r2, crop, &m0, &m1, &l);
  vis_axis(m0, r1, in, &s0, &s1, &l);
  *lo = s0;
  vis_axis(b, r2, crop, &m0, &m1, &l);
  vis_axis(m1, r1, in, &s0, &s1, &l);
  *hi = s1;
}
