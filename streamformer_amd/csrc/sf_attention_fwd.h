// Device helpers shared by the head_dim-64 forward attention kernels: the register-staged spatial and temporal kernels
// (sf_attention_spatial.hip, sf_attention_temporal.hip) use all of them, the DMA kernels only HD and the image toolkit of
// sf_attn_image.h, the single-query kernels (sf_attention_decode.hip) only HD.
#pragma once
#include "sf_attn_image.h"
#include "sf_switches.h"
#include <cstdlib>

#define HD 64  // head_dim supported by these kernels (SigLIP-base/large: 64)

// K-tile LDS swizzle: the 16 keys one ds_read_b128 lane group touches are
// {8a + 4hh + r : a in 0..3, r in 0..3}; (r&1) picks the 128-byte half of the 256-byte bank row, so
// the slot XOR must separate (r>>1, a): 8 values.
SF_DEVICE int kswz(int key) { return ((key >> 1) & 1) | (((key >> 3) & 3) << 1); }

// V^T LDS swizzle of the spatial kernel (4 bits: rows are padded to a multiple of 16 chunks)
SF_DEVICE int vswz(int d) { return ((d ^ (d >> 3)) & 7) | (((d >> 3) & 1) << 3); }

// load 8 consecutive elements (bf16 or fp32 storage) as floats
template <bool F32>
SF_DEVICE void load8(const void* base, size_t elem_off, float (&out)[8]) {
  if (F32) {
    const f32x4_t* p = reinterpret_cast<const f32x4_t*>(reinterpret_cast<const float*>(base) + elem_off);
    const f32x4_t a = p[0], b = p[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) { out[j] = a[j]; out[4 + j] = b[j]; }
  } else {
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(reinterpret_cast<const bf16_t*>(base) + elem_off);
#pragma unroll
    for (int j = 0; j < 4; ++j) { out[2 * j] = bf2f(v[j] & 0xffffu); out[2 * j + 1] = bf2f(v[j] >> 16); }
  }
}

// MFMA operand fragment straight from global memory: 8 consecutive elements -> bf16x8 (hi [, lo])
template <bool F32>
SF_DEVICE void load_frag(const void* base, size_t elem_off, bf16x8_t& hi, bf16x8_t& lo) {
  if (F32) {
    float f[8];
    load8<true>(base, elem_off, f);
    unsigned int h[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split_bf(f[j], h[j], l[j]);
    hi = __builtin_bit_cast(bf16x8_t, pack_bf8(h));
    lo = __builtin_bit_cast(bf16x8_t, pack_bf8(l));
  } else {
    hi = *reinterpret_cast<const bf16x8_t*>(reinterpret_cast<const bf16_t*>(base) + elem_off);
    lo = hi;
  }
}

// pack 8 probabilities into the B-operand fragment (hi [, lo])
template <bool ACC>
SF_DEVICE void pack_p(const f32x4_t& a, const f32x4_t& b, bf16x8_t& hi, bf16x8_t& lo) {
  unsigned int h[8], l[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) { split_bf(a[j], h[j], l[j]); split_bf(b[j], h[4 + j], l[4 + j]); }
  hi = __builtin_bit_cast(bf16x8_t, pack_bf8(h));
  if (ACC) lo = __builtin_bit_cast(bf16x8_t, pack_bf8(l));
}

// Softmax numerator over the score tiles of one query column, in place.  `valid(kt2, key)` says whether
// a key takes part.  The scale (> 0) is folded into the exponent: p = 2^((s - max s) * scale * log2 e),
// one FMA + v_exp_f32 per element; tiles known to be fully valid skip the mask.  Returns sum(p).
template <bool ACC, int MAXNT2, typename Valid>
SF_DEVICE float softmax_tiles(f32x4_t (&s)[MAXNT2][2], int nt2, int g, float scale, int first_masked_tile, Valid valid,
                              float* max2_out = nullptr) {
  float mx = -INFINITY;
#pragma unroll
  for (int kt2 = 0; kt2 < MAXNT2; ++kt2) {
    if (kt2 < nt2) {
      if (kt2 >= first_masked_tile) {
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (!valid(kt2, kt2 * 32 + g * 8 + hh * 4 + r)) s[kt2][hh][r] = -INFINITY;
      }
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
        mx = fmaxf(mx, fmaxf(fmaxf(s[kt2][hh][0], s[kt2][hh][1]), fmaxf(s[kt2][hh][2], s[kt2][hh][3])));
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float c = scale * 1.44269504088896340736f;
  const float mc = mx * c;
  if (max2_out) *max2_out = mc;         // row maximum in the base-2 exponent domain
  float sum = 0.f;
#pragma unroll
  for (int kt2 = 0; kt2 < MAXNT2; ++kt2) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float e = 0.f;
        if (kt2 < nt2) {
          const float a = fmaf(s[kt2][hh][r], c, -mc);
          e = __builtin_amdgcn_exp2f(a);      // v_exp_f32 (1 ulp) in both modes: arguments are <= 0, results below 2^-126 may flush
        }
        s[kt2][hh][r] = e;
        sum += e;
      }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  return sum;
}

// the single-query routes of sf_temporal_route (sf_attention_decode.hip); hipErrorInvalidValue for any other route
hipError_t sf_launch_temporal_decode(SfTemporalRoute r, const SfAttnArgs& a, hipStream_t s);
