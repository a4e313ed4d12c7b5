// Multi-scale deformable attention (Deformable DETR's MSDeformAttn; the reference's only native code, ms_deform_im2col_cuda.cuh, under
// downstream/OVIS/mask2former/modeling/pixel_decoder/ops/): out[n, q, m, :] = sum over (level l, point p) of
// attention_weights[n, q, m, l, p] * bilinear(value[n, level l, m, :], sampling_locations[n, q, m, l, p]).  fp32 FMA, no MFMA, no LDS.
//
// Sampling rule (the CUDA kernel's, equal to grid_sample(bilinear, zeros, align_corners=False)): pixel coordinate = loc * size - 0.5; a
// sample counts only if -1 < h < H and -1 < w < W (a NaN coordinate fails the test and contributes nothing); each of the four corners
// is bounds-checked on its own.  Every address is derived from coordinates that passed these tests, so no location can index outside
// `value`.
//
//   sf_msda_forward_kernel<FUSED>   gather.  A group of G = pow2ceil(D / 4) lanes owns one (n, q, m): lane j holds channels 4 j .. 4 j + 3
//                                   (lanes with 4 j >= D idle), reads its L * P locations and weights from one address per group (one
//                                   fetch, broadcast), loads one float4 per corner and stores one float4.  64 / G groups share a wave.
//                                   FUSED: the locations come from the raw sampling_offsets rows and the reference points, the weights from
//                                   a softmax over the L * P raw logits (max pass, sum pass, exp again in the sampling loop, one division at
//                                   the end), masked value rows read as zero: none of the three intermediates exists in memory.
//   sf_msda_backward_kernel         scatter.  A group of G = min(pow2ceil(D), 64) lanes owns one (n, q, m): lane c holds channel c (and
//                                   c + 64 when D > 64), so one wave-instruction of atomicAdd(float*) adds 256 contiguous bytes at D >= 64
//                                   and two 128-byte row segments at D = 32 (the full-rate shapes of the chip's float atomics; one lane per
//                                   row is 17 x slower).  grad_sampling_locations and grad_attention_weights have one owner per
//                                   (n, q, m, l, p): their sum over D is an xor-butterfly inside the group, a fixed order, written by the
//                                   group's first lane — bit-reproducible, never zeroed, never added to.  grad_value is the sum of atomics in
//                                   arrival order: NOT bit-reproducible.
#include "sf_common.h"
#include "sf_internal.h"
#include "sf_launch.h"

#include <string.h>

#define MSDA_MAX_LEVELS 8
#define MSDA_MAX_POINTS 8
#define MSDA_THREADS 256

struct SfMsdaGeom {                 // by value in the kernel arguments
  int H[MSDA_MAX_LEVELS], W[MSDA_MAX_LEVELS], start[MSDA_MAX_LEVELS];
};

struct SfMsda {
  const float* value;               // [N, S, M, D]
  const unsigned char* pad;         // [N, S] or null (FUSED only)
  const float* loc;                 // [N, Lq, M, L, P, 2]                 (unfused)
  const float* attn;                // [N, Lq, M, L, P]                    (unfused)
  const float* offs; const float* logits;      // rows of offs_ld / logits_ld floats: [N * Lq, M * L * P * 2] / [N * Lq, M * L * P]   (FUSED)
  const float* ref;                 // [N, Lq, L, ref_dim]                 (FUSED)
  const float* grad_out;            // [N, Lq, M * D]                      (backward)
  float* out;                       // [N, Lq, M * D]                      (forward)
  float* grad_value; float* grad_loc; float* grad_attn;
  long long groups;                 // N * Lq * M
  int S, M, D, Lq, L, P, G, ref_dim, offs_ld, logits_ld;
  SfMsdaGeom g;
};

struct MsdaTap {                    // one sample's four corners
  bool inside;
  int h_low, w_low;
  float lh, lw;
};

SF_DEVICE MsdaTap msda_tap(float x, float y, int H, int W) {
  MsdaTap t;
  const float h_im = y * (float)H - 0.5f, w_im = x * (float)W - 0.5f;
  t.inside = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
  const float hf = floorf(h_im), wf = floorf(w_im);
  t.h_low = t.inside ? (int)hf : 0;
  t.w_low = t.inside ? (int)wf : 0;
  t.lh = h_im - hf;
  t.lw = w_im - wf;
  return t;
}

template <bool FUSED>
__global__ __launch_bounds__(MSDA_THREADS) void sf_msda_forward_kernel(SfMsda p) {
  const int G = p.G;
  const long long gid = ((long long)blockIdx.x * MSDA_THREADS + threadIdx.x) / G;
  const int c = ((int)threadIdx.x % G) * 4;
  if (gid >= p.groups || c >= p.D) return;
  const int m = (int)(gid % p.M);
  const long long nq = gid / p.M, n = nq / p.Lq;
  const int LP = p.L * p.P;
  const size_t row = (size_t)p.M * p.D;                         // floats between two pixels of `value`
  const float* vbase = p.value + (size_t)n * p.S * row + (size_t)m * p.D + c;
  const unsigned char* pad = FUSED && p.pad ? p.pad + (size_t)n * p.S : nullptr;
  const float* loc = nullptr; const float* attn = nullptr; const float* ref = nullptr;
  float mx = 0.f, denom = 1.f;
  if (FUSED) {
    loc = p.offs + (size_t)nq * p.offs_ld + (size_t)m * LP * 2;
    attn = p.logits + (size_t)nq * p.logits_ld + (size_t)m * LP;
    ref = p.ref + (size_t)nq * p.L * p.ref_dim;
    mx = attn[0];
    for (int i = 1; i < LP; ++i) mx = fmaxf(mx, attn[i]);
    denom = 0.f;
    for (int i = 0; i < LP; ++i) denom += expf(attn[i] - mx);
  } else {
    loc = p.loc + (size_t)gid * LP * 2;
    attn = p.attn + (size_t)gid * LP;
  }
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  for (int l = 0; l < p.L; ++l) {
    const int H = p.g.H[l], W = p.g.W[l], start = p.g.start[l];
    for (int k = 0; k < p.P; ++k) {
      const int i = l * p.P + k;
      float x = loc[2 * i], y = loc[2 * i + 1], a = attn[i];
      if (FUSED) {
        a = expf(a - mx);
        if (p.ref_dim == 2) {
          x = ref[l * 2] + x / (float)W;
          y = ref[l * 2 + 1] + y / (float)H;
        } else {
          x = ref[l * 4] + x / (float)p.P * ref[l * 4 + 2] * 0.5f;
          y = ref[l * 4 + 1] + y / (float)p.P * ref[l * 4 + 3] * 0.5f;
        }
      }
      const MsdaTap t = msda_tap(x, y, H, W);
      if (!t.inside) continue;
      const float hh = 1.f - t.lh, hw = 1.f - t.lw;
      const bool top = t.h_low >= 0, bottom = t.h_low + 1 <= H - 1, left = t.w_low >= 0, right = t.w_low + 1 <= W - 1;
      const int s00 = start + t.h_low * W + t.w_low;            // read only where its corner is live
      const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
      f32x4_t v1 = zero, v2 = zero, v3 = zero, v4 = zero;
      if (top && left && !(pad && pad[s00])) v1 = *reinterpret_cast<const f32x4_t*>(vbase + (size_t)s00 * row);
      if (top && right && !(pad && pad[s00 + 1])) v2 = *reinterpret_cast<const f32x4_t*>(vbase + (size_t)(s00 + 1) * row);
      if (bottom && left && !(pad && pad[s00 + W])) v3 = *reinterpret_cast<const f32x4_t*>(vbase + (size_t)(s00 + W) * row);
      if (bottom && right && !(pad && pad[s00 + W + 1])) v4 = *reinterpret_cast<const f32x4_t*>(vbase + (size_t)(s00 + W + 1) * row);
      const float w1 = hh * hw, w2 = hh * t.lw, w3 = t.lh * hw, w4 = t.lh * t.lw;
      acc += a * (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4);
    }
  }
  if (FUSED) acc = acc / denom;
  *reinterpret_cast<f32x4_t*>(p.out + (size_t)gid * p.D + c) = acc;
}

__global__ __launch_bounds__(MSDA_THREADS) void sf_msda_backward_kernel(SfMsda p) {
  const int G = p.G;
  const long long gid = ((long long)blockIdx.x * MSDA_THREADS + threadIdx.x) / G;
  const int lane = (int)threadIdx.x % G;
  if (gid >= p.groups) return;                                  // whole groups leave: the butterflies below stay inside one group
  const int m = (int)(gid % p.M);
  const long long nq = gid / p.M, n = nq / p.Lq;
  const int LP = p.L * p.P;
  const size_t row = (size_t)p.M * p.D;
  const size_t voff = (size_t)n * p.S * row + (size_t)m * p.D;
  const float* loc = p.loc + (size_t)gid * LP * 2;
  const float* attn = p.attn + (size_t)gid * LP;
  const int ch[2] = {lane, lane + 64};
  const bool live[2] = {lane < p.D, lane + 64 < p.D};
  float tg[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) tg[j] = live[j] ? p.grad_out[(size_t)gid * p.D + ch[j]] : 0.f;
  for (int l = 0; l < p.L; ++l) {
    const int H = p.g.H[l], W = p.g.W[l], start = p.g.start[l];
    for (int k = 0; k < p.P; ++k) {
      const int i = l * p.P + k;
      const float a = attn[i];
      const MsdaTap t = msda_tap(loc[2 * i], loc[2 * i + 1], H, W);
      float ga = 0.f, gw = 0.f, gh = 0.f;
      if (t.inside) {                                           // uniform over the group
        const float hh = 1.f - t.lh, hw = 1.f - t.lw;
        const bool top = t.h_low >= 0, bottom = t.h_low + 1 <= H - 1, left = t.w_low >= 0, right = t.w_low + 1 <= W - 1;
        const size_t o00 = voff + (size_t)(long long)(start + t.h_low * W + t.w_low) * row;
        const float w1 = hh * hw, w2 = hh * t.lw, w3 = t.lh * hw, w4 = t.lh * t.lw;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (!live[j]) continue;
          const float tgv = tg[j] * a;
          float v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f;
          if (top && left) { const size_t o = o00 + ch[j]; v1 = p.value[o]; atomicAdd(p.grad_value + o, w1 * tgv); }
          if (top && right) { const size_t o = o00 + row + ch[j]; v2 = p.value[o]; atomicAdd(p.grad_value + o, w2 * tgv); }
          if (bottom && left) { const size_t o = o00 + (size_t)W * row + ch[j]; v3 = p.value[o]; atomicAdd(p.grad_value + o, w3 * tgv); }
          if (bottom && right) { const size_t o = o00 + (size_t)(W + 1) * row + ch[j]; v4 = p.value[o]; atomicAdd(p.grad_value + o, w4 * tgv); }
          const float grad_h = -hw * v1 - t.lw * v2 + hw * v3 + t.lw * v4;
          const float grad_w = -hh * v1 + hh * v2 - t.lh * v3 + t.lh * v4;
          ga += tg[j] * (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4);
          gw += grad_w * tgv;
          gh += grad_h * tgv;
        }
      }
      for (int o = G >> 1; o > 0; o >>= 1) {
        ga += __shfl_xor(ga, o);
        gw += __shfl_xor(gw, o);
        gh += __shfl_xor(gh, o);
      }
      if (lane == 0) {
        p.grad_attn[(size_t)gid * LP + i] = ga;
        p.grad_loc[((size_t)gid * LP + i) * 2] = (float)W * gw;
        p.grad_loc[((size_t)gid * LP + i) * 2 + 1] = (float)H * gh;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------------
static int msda_pow2ceil(int v) {
  int g = 1;
  while (g < v) g <<= 1;
  return g;
}

// every refusal happens here, before anything is launched; fills the geometry and the shape fields of `p`
static int msda_plan(const char* who, const int32_t* shapes, const int32_t* level_start, int N, int S, int M, int D, int Lq, int L, int P, int lanes_per_channel4,
                     SfMsda* p, unsigned* blocks) {
  if (!shapes || !level_start) return sf_set_err(SF_ERR_INVALID, "%s: null spatial_shapes / level_start_index (host arrays)", who);
  if (D < 8 || D > 128 || D % 8) return sf_set_err(SF_ERR_INVALID, "%s: D = %d (channels per head) must be a multiple of 8 in 8..128", who, D);
  if (L < 1 || L > MSDA_MAX_LEVELS) return sf_set_err(SF_ERR_INVALID, "%s: L = %d levels outside 1..%d", who, L, MSDA_MAX_LEVELS);
  if (P < 1 || P > MSDA_MAX_POINTS) return sf_set_err(SF_ERR_INVALID, "%s: P = %d points outside 1..%d", who, P, MSDA_MAX_POINTS);
  if (N < 1 || S < 1 || M < 1 || Lq < 1) return sf_set_err(SF_ERR_INVALID, "%s: N = %d, S = %d, M = %d, Lq = %d must all be >= 1", who, N, S, M, Lq);
  memset(p, 0, sizeof(*p));
  long long sum = 0;
  for (int l = 0; l < L; ++l) {
    const long long H = shapes[2 * l], W = shapes[2 * l + 1], st = level_start[l];
    if (H < 1 || W < 1 || H * W > S) return sf_set_err(SF_ERR_INVALID, "%s: spatial_shapes[%d] = %lld x %lld", who, l, H, W);
    if (st < 0 || st + H * W > S) return sf_set_err(SF_ERR_INVALID, "%s: level_start_index[%d] = %lld with %lld x %lld pixels leaves S = %d", who, l, st, H, W, S);
    p->g.H[l] = (int)H; p->g.W[l] = (int)W; p->g.start[l] = (int)st;
    sum += H * W;
  }
  if (sum != S) return sf_set_err(SF_ERR_INVALID, "%s: spatial_shapes sum to %lld pixels, S = %d", who, sum, S);
  p->groups = (long long)N * Lq * M;
  p->S = S; p->M = M; p->D = D; p->Lq = Lq; p->L = L; p->P = P;
  p->G = lanes_per_channel4 ? msda_pow2ceil(D / 4) : (D >= 64 ? 64 : msda_pow2ceil(D));
  const long long per_block = MSDA_THREADS / p->G;
  const long long nb = (p->groups + per_block - 1) / per_block;
  if (nb > 0x7fffffffLL) return sf_set_err(SF_ERR_INVALID, "%s: N * Lq * M = %lld (q, head) pairs exceed one grid", who, p->groups);
  *blocks = (unsigned)nb;
  return SF_OK;
}

extern "C" int sf_op_msda_forward(const float* value_dev, const int32_t* spatial_shapes, const int32_t* level_start_index,
                                  const float* sampling_locations_dev, const float* attention_weights_dev, float* out_dev, int N, int S,
                                  int M, int D, int Lq, int L, int P, sf_stream stream) {
  SfMsda p;
  unsigned blocks = 0;
  const int rc = msda_plan("sf_op_msda_forward", spatial_shapes, level_start_index, N, S, M, D, Lq, L, P, 1, &p, &blocks);
  if (rc) return rc;
  if (!value_dev || !sampling_locations_dev || !attention_weights_dev || !out_dev) return sf_set_err(SF_ERR_INVALID, "sf_op_msda_forward: null buffer");
  if (((uintptr_t)value_dev | (uintptr_t)out_dev) & 15) return sf_set_err(SF_ERR_INVALID, "sf_op_msda_forward: value and out must be 16-byte aligned");
  p.value = value_dev; p.loc = sampling_locations_dev; p.attn = attention_weights_dev; p.out = out_dev;
  HIP_TRY(sf_launch(sf_msda_forward_kernel<false>, dim3(blocks), dim3(MSDA_THREADS), 0, (hipStream_t)stream, p));
  return SF_OK;
}

extern "C" int sf_op_msda_forward_fused(const float* value_dev, const uint8_t* padding_mask_dev, const int32_t* spatial_shapes,
                                        const int32_t* level_start_index, const float* offsets_dev, int offsets_ld, const float* logits_dev,
                                        int logits_ld, const float* reference_points_dev, int ref_dim, float* out_dev, int N, int S, int M,
                                        int D, int Lq, int L, int P, sf_stream stream) {
  SfMsda p;
  unsigned blocks = 0;
  const int rc = msda_plan("sf_op_msda_forward_fused", spatial_shapes, level_start_index, N, S, M, D, Lq, L, P, 1, &p, &blocks);
  if (rc) return rc;
  if (ref_dim != 2 && ref_dim != 4) return sf_set_err(SF_ERR_INVALID, "sf_op_msda_forward_fused: ref_dim = %d (last dim of reference_points) must be 2 or 4", ref_dim);
  if ((long long)offsets_ld < (long long)M * L * P * 2 || (long long)logits_ld < (long long)M * L * P)
    return sf_set_err(SF_ERR_INVALID, "sf_op_msda_forward_fused: offsets_ld = %d / logits_ld = %d shorter than a row of %d heads x %d levels x %d points", offsets_ld, logits_ld, M, L, P);
  if (!value_dev || !offsets_dev || !logits_dev || !reference_points_dev || !out_dev) return sf_set_err(SF_ERR_INVALID, "sf_op_msda_forward_fused: null buffer");
  if (((uintptr_t)value_dev | (uintptr_t)out_dev) & 15) return sf_set_err(SF_ERR_INVALID, "sf_op_msda_forward_fused: value and out must be 16-byte aligned");
  p.value = value_dev; p.pad = padding_mask_dev; p.offs = offsets_dev; p.logits = logits_dev; p.ref = reference_points_dev; p.out = out_dev;
  p.ref_dim = ref_dim; p.offs_ld = offsets_ld; p.logits_ld = logits_ld;
  HIP_TRY(sf_launch(sf_msda_forward_kernel<true>, dim3(blocks), dim3(MSDA_THREADS), 0, (hipStream_t)stream, p));
  return SF_OK;
}

extern "C" int sf_op_msda_backward(const float* value_dev, const int32_t* spatial_shapes, const int32_t* level_start_index,
                                   const float* sampling_locations_dev, const float* attention_weights_dev, const float* grad_out_dev,
                                   float* grad_value_dev, float* grad_sampling_locations_dev, float* grad_attention_weights_dev, int N,
                                   int S, int M, int D, int Lq, int L, int P, sf_stream stream) {
  SfMsda p;
  unsigned blocks = 0;
  const int rc = msda_plan("sf_op_msda_backward", spatial_shapes, level_start_index, N, S, M, D, Lq, L, P, 0, &p, &blocks);
  if (rc) return rc;
  if (!value_dev || !sampling_locations_dev || !attention_weights_dev || !grad_out_dev || !grad_value_dev || !grad_sampling_locations_dev ||
      !grad_attention_weights_dev)
    return sf_set_err(SF_ERR_INVALID, "sf_op_msda_backward: null buffer");
  p.value = value_dev; p.loc = sampling_locations_dev; p.attn = attention_weights_dev; p.grad_out = grad_out_dev;
  p.grad_value = grad_value_dev; p.grad_loc = grad_sampling_locations_dev; p.grad_attn = grad_attention_weights_dev;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(grad_value_dev, 0, (size_t)N * S * M * D * sizeof(float), s));
  HIP_TRY(sf_launch(sf_msda_backward_kernel, dim3(blocks), dim3(MSDA_THREADS), 0, s, p));
  return SF_OK;
}
