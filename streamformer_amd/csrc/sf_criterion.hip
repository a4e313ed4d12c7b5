// Mask2Former criterion: the device side of HungarianMatcher and SetCriterion (mask2former/modeling/matcher.py, criterion.py) for every
// decoder layer of a training step at once.  All fp32, on the caller's stream, without allocation or host synchronisation.
//
// Sampling is F.grid_sample(bilinear, zeros, align_corners=False) of a point in [0, 1)^2 (x first): pixel = ((2 c - 1 + 1) size - 1) / 2 in
// grid_sample's own operation order, four corners weighted nw, ne, sw, se, each bounds-checked on its own (crit_tap / crit_fetch; the rule
// sf_msda.hip states).  A target mask has a SCALE size (what the coordinate is multiplied with) and an EXTENT (what may be read): equal in
// the matcher; in the losses the scale is the batch's largest mask, as nested_tensor_from_tensor_list pads, and the extent the mask's own.
//
//   sf_crit_cost_kernel          grid (chunks of 512 points, tiles of 64 queries, L B).  Per sub-step of 64 points wave w samples ITS 16
//                                query rows (x and sigmoid(x)) and every fourth target row into LDS, keeps the row sums of softplus(x),
//                                sigmoid(x) and t in registers, and contracts x t^T and sigmoid(x) t^T on v_mfma_f32_16x16x4_f32
//                                (A = 16 queries x 4 points, B = 4 points x 16 targets).  Partials per chunk; no [Q, K] tensor, no atomics.
//   sf_crit_cost_finish_kernel   one thread per (layer, image, query, target): adds the partials in chunk order, the softmax probability of
//                                the target's class, the weighted sum.  Columns >= G_b are not written.
//   sf_crit_loss_kernel          one workgroup (1024 threads) per matched pair: the pair's mask at the oversampled points stays in LDS; a
//                                four-pass radix select on the bits of |x| finds the threshold of the `uncertain` smallest; an ordered
//                                compaction (two block scans) emits them in index order, ties at the threshold to the lower index; the random
//                                points follow.  Every thread sums its own points in a fixed order, then waves and threads in a fixed order.
//   sf_crit_loss_finish_kernel   per layer, the pairs' terms in pair order, over num_masks.
//   sf_crit_loss_bwd_kernel      one workgroup per pair: resamples x and t at the saved points, scatters d x into the pair's plane, in LDS when
//                                it fits (one flush) and else straight to memory; float atomics, arrival order: NOT bit-reproducible.
//   sf_crit_class_*              target classes from the pair table, sum of class weights per layer, one wave per row (log-softmax, weighted
//                                NLL and its gradient), per-layer sum in a fixed order.
#include "sf_internal.h"
#include "sf_common.h"
#include "sf_launch.h"
#include "sf_handle.h"

#define CRIT_MAX_LAYERS 16                 // layer pointers travel as a kernel argument
#define CRIT_MAX_IMAGES 32                 // so do the per-image target tables
#define CRIT_MAX_G 128                     // targets per image: a wave holds 2 x 8 accumulator tiles
#define CRIT_MAX_Q 4096
#define CRIT_MAX_C 4096
#define CRIT_QT 64                         // queries per workgroup of the cost kernel: 16 per wave
#define CRIT_KS 64                         // points per sub-step: one per lane
#define CRIT_CHUNK 512                     // points per workgroup
#define CRIT_LD (CRIT_KS + 4)              // row pitch: 16 rows x 4 points of an MFMA operand read land on 64 different banks
#define CRIT_LT 1024                       // threads of the loss kernel
#define CRIT_LOSS_MISC (256 + CRIT_LT + 64 + 8)      // floats of LDS beside the values: histogram, scan, wave partials, select state
#define CRIT_MAX_OVER 39424                // oversampled points per pair: (39424 + 1352) * 4 = 163104 of the CU's 163840 bytes of LDS
#define CRIT_BT 512                        // threads of the backward kernel
#define CRIT_BWD_PLANE (32 * 1024)         // floats of a predicted plane the backward kernel keeps in LDS (128 KB)

struct CritLayers { const float* logits[CRIT_MAX_LAYERS]; const float* masks[CRIT_MAX_LAYERS]; };
struct CritTargets {
  const float* masks[CRIT_MAX_IMAGES];     // [G, H, W] fp32
  const long long* labels[CRIT_MAX_IMAGES];
  int G[CRIT_MAX_IMAGES], H[CRIT_MAX_IMAGES], W[CRIT_MAX_IMAGES];
};
struct CritTap { int o[4]; float w[4]; };  // corner offsets in the plane and weights; a corner outside the extent has weight 0 and offset 0

SF_DEVICE void crit_tap(float cx, float cy, int SH, int SW, int h, int w, CritTap* t) {
  const float ix = (((2.f * cx - 1.f) + 1.f) * (float)SW - 1.f) * 0.5f, iy = (((2.f * cy - 1.f) + 1.f) * (float)SH - 1.f) * 0.5f;
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy;
  const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix, wy1 = iy - fy, wy0 = (fy + 1.f) - iy;
  const float ww[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int x = x0 + (c & 1), y = y0 + (c >> 1);
    const bool in = x >= 0 && x < w && y >= 0 && y < h;
    t->o[c] = in ? y * w + x : 0;
    t->w[c] = in ? ww[c] : 0.f;
  }
}
SF_DEVICE float crit_fetch(const float* plane, const CritTap& t) {
  float a = plane[t.o[0]] * t.w[0];
  a += plane[t.o[1]] * t.w[1];
  a += plane[t.o[2]] * t.w[2];
  a += plane[t.o[3]] * t.w[3];
  return a;
}
SF_DEVICE float crit_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
SF_DEVICE float crit_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// ------------------------------------------------------------------------------------------------
// 1. cost matrices
// ------------------------------------------------------------------------------------------------
struct CritCostArgs {
  CritLayers lay; CritTargets tg;
  const float* coords;                     // [L, B, K, 2]
  float *p_xt, *p_st, *p_sp, *p_ss, *p_tt; // partials per chunk: [L B, nch, Q, Gmax] x 2, [L B, nch, Q] x 2, [L B, nch, Gmax]
  int B, Q, H, W, K, Gmax, nch, C1;
};

template <int GT>      // target tiles of 16 held by a wave, ceil(Gmax / 16) <= GT
__global__ __launch_bounds__(256) void sf_crit_cost_kernel(CritCostArgs p) {
  extern __shared__ __attribute__((aligned(16))) float crit_smem[];
  float* xs = crit_smem;                                      // [64][CRIT_LD]
  float* sg = xs + CRIT_QT * CRIT_LD;                         // [64][CRIT_LD]
  float* ts = sg + CRIT_QT * CRIT_LD;                         // [GT 16][CRIT_LD]
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g4 = lane >> 4;
  const int ch = (int)blockIdx.x, qt = (int)blockIdx.y, lb = (int)blockIdx.z, l = lb / p.B, b = lb - l * p.B;
  const int G = p.tg.G[b];
  if (G == 0) return;                                         // the whole workgroup
  const int gt_used = (G + 15) >> 4, th = p.tg.H[b], tw = p.tg.W[b];
  const size_t plane = (size_t)p.H * p.W, tplane = (size_t)th * tw;
  const float* pm = p.lay.masks[l] + (size_t)b * p.Q * plane;
  const float* tm = p.tg.masks[b];
  const float* cd = p.coords + (size_t)lb * p.K * 2;
  const int k_begin = ch * CRIT_CHUNK, k_end = min(k_begin + CRIT_CHUNK, p.K), q_base = qt * CRIT_QT + wave * 16;
  f32x4_t axt[GT], ast[GT];
  float sp[16], ss[16], tt[GT * 4];
#pragma unroll
  for (int t = 0; t < GT; ++t) { axt[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; ast[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
  for (int i = 0; i < 16; ++i) { sp[i] = 0.f; ss[i] = 0.f; }
#pragma unroll
  for (int i = 0; i < GT * 4; ++i) tt[i] = 0.f;
  for (int k0 = k_begin; k0 < k_end; k0 += CRIT_KS) {
    const int k = k0 + lane;
    const bool live = k < k_end;
    const float cx = live ? cd[2 * (size_t)k] : 0.f, cy = live ? cd[2 * (size_t)k + 1] : 0.f;
    CritTap tp, tq;
    crit_tap(cx, cy, p.H, p.W, p.H, p.W, &tp);
    crit_tap(cx, cy, th, tw, th, tw, &tq);
    __syncthreads();                                          // the last sub-step's operand reads are done
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int q = q_base + i;
      float x = 0.f, s = 0.f;
      if (live && q < p.Q) {
        x = crit_fetch(pm + (size_t)q * plane, tp);
        s = crit_sigmoid(x);
        sp[i] += crit_softplus(x);
        ss[i] += s;
      }
      xs[(wave * 16 + i) * CRIT_LD + lane] = x;
      sg[(wave * 16 + i) * CRIT_LD + lane] = s;
    }
#pragma unroll
    for (int i = 0; i < GT * 4; ++i) {
      const int g = wave + 4 * i;
      float t = 0.f;
      if (live && g < G) {
        t = crit_fetch(tm + (size_t)g * tplane, tq);
        tt[i] += t;
      }
      ts[g * CRIT_LD + lane] = t;
    }
    __syncthreads();
    const float* a = xs + (wave * 16 + l15) * CRIT_LD + g4;   // A[query l15][point g4]
    const float* a2 = sg + (wave * 16 + l15) * CRIT_LD + g4;
    const float* bp = ts + l15 * CRIT_LD + g4;                // B[point g4][target l15]
    for (int kk = 0; kk < CRIT_KS; kk += 4) {
      const float av = a[kk], sv = a2[kk];
#pragma unroll
      for (int t = 0; t < GT; ++t)
        if (t < gt_used) {
          const float bv = bp[t * 16 * CRIT_LD + kk];
          axt[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, axt[t], 0, 0, 0);
          ast[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(sv, bv, ast[t], 0, 0, 0);
        }
    }
  }
  const size_t slot = (size_t)lb * p.nch + ch;
#pragma unroll
  for (int t = 0; t < GT; ++t)                                // D: target l15, queries 4 g4 + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q_base + 4 * g4 + r, g = t * 16 + l15;
      if (q < p.Q && g < G) {
        const size_t o = (slot * p.Q + q) * p.Gmax + g;
        p.p_xt[o] = axt[t][r];
        p.p_st[o] = ast[t][r];
      }
    }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float a = wave_sum_dpp(sp[i]), s = wave_sum_dpp(ss[i]);
    const int q = q_base + i;
    if (lane == 0 && q < p.Q) { p.p_sp[slot * p.Q + q] = a; p.p_ss[slot * p.Q + q] = s; }
  }
#pragma unroll
  for (int i = 0; i < GT * 4; ++i) {
    const float t = wave_sum_dpp(tt[i]);
    const int g = wave + 4 * i;
    if (lane == 0 && qt == 0 && g < G) p.p_tt[slot * p.Gmax + g] = t;
  }
}

__global__ __launch_bounds__(256) void sf_crit_cost_finish_kernel(CritCostArgs p, float w_class, float w_mask, float w_dice, float* cost, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int g = (int)(idx % p.Gmax), q = (int)((idx / p.Gmax) % p.Q), lb = (int)(idx / ((long long)p.Gmax * p.Q)), l = lb / p.B, b = lb - l * p.B;
  if (g >= p.tg.G[b]) return;
  float xt = 0.f, st = 0.f, sp = 0.f, ss = 0.f, tt = 0.f;
  for (int c = 0; c < p.nch; ++c) {                            // chunk order
    const size_t slot = (size_t)lb * p.nch + c, o = (slot * p.Q + q) * p.Gmax + g;
    xt += p.p_xt[o]; st += p.p_st[o]; sp += p.p_sp[slot * p.Q + q]; ss += p.p_ss[slot * p.Q + q]; tt += p.p_tt[slot * p.Gmax + g];
  }
  const float* row = p.lay.logits[l] + ((size_t)b * p.Q + q) * p.C1;
  const long long label = p.tg.labels[b][g];
  float m = -INFINITY, s = 0.f;
  for (int c = 0; c < p.C1; ++c) m = fmaxf(m, row[c]);
  for (int c = 0; c < p.C1; ++c) s += expf(row[c] - m);
  const float prob = (label >= 0 && label < p.C1) ? expf(row[label] - m) / s : 0.f;
  const float cost_mask = (sp - xt) / (float)p.K;
  const float cost_dice = 1.f - (2.f * st + 1.f) / (ss + tt + 1.f);
  cost[idx] = w_mask * cost_mask + w_class * (-prob) + w_dice * cost_dice;
}

// ------------------------------------------------------------------------------------------------
// 3. mask losses of the matched pairs
// ------------------------------------------------------------------------------------------------
struct CritLossArgs {
  CritLayers lay; CritTargets tg;
  const int32_t* pairs;                    // [N, 4]: layer, image, query, target
  const float* over;                       // [N, KO, 2]
  const float* rnd;                        // [N, K - KU, 2]
  float* coords_out;                       // [N, K, 2]
  float* sums;                             // [N, 4]: sum sigmoid, sum t, sum sigmoid t, unused
  float* terms;                            // [N, 2]: mean bce, dice
  int32_t* idx_out;                        // [N, KU] or null
  int B, Q, H, W, K, KO, KU, Hmax, Wmax, seg;
};

SF_DEVICE int crit_excl_scan(int v, int* buf, int tid) {      // over the CRIT_LT threads
  buf[tid] = v;
  __syncthreads();
  for (int o = 1; o < CRIT_LT; o <<= 1) {
    const int a = tid >= o ? buf[tid - o] : 0;
    __syncthreads();
    buf[tid] += a;
    __syncthreads();
  }
  const int r = buf[tid] - v;
  __syncthreads();
  return r;
}

SF_DEVICE void crit_point_terms(float x, float t, float* acc) {
  const float s = crit_sigmoid(x);
  acc[0] += (fmaxf(x, 0.f) - x * t) + log1pf(expf(-fabsf(x)));
  acc[1] += s;
  acc[2] += t;
  acc[3] += s * t;
}

__global__ __launch_bounds__(CRIT_LT) void sf_crit_loss_kernel(CritLossArgs p) {
  extern __shared__ __attribute__((aligned(16))) float crit_smem[];
  float* val = crit_smem;                                     // [KO]
  int* hist = reinterpret_cast<int*>(val + p.KO);             // [256]
  int* scan = hist + 256;                                     // [CRIT_LT]
  float* red = reinterpret_cast<float*>(scan + CRIT_LT);      // [16][4]
  int* sel = reinterpret_cast<int*>(red + 64);                // [2]
  const int tid = (int)threadIdx.x, n = (int)blockIdx.x;
  const int l = p.pairs[4 * n], b = p.pairs[4 * n + 1], q = p.pairs[4 * n + 2], g = p.pairs[4 * n + 3];
  const int th = p.tg.H[b], tw = p.tg.W[b];
  const float* pm = p.lay.masks[l] + ((size_t)b * p.Q + q) * p.H * p.W;
  const float* tm = p.tg.masks[b] + (size_t)g * th * tw;
  const float* ov = p.over + (size_t)n * p.KO * 2;
  for (int i = tid; i < p.KO; i += CRIT_LT) {
    CritTap tp;
    crit_tap(ov[2 * (size_t)i], ov[2 * (size_t)i + 1], p.H, p.W, p.H, p.W, &tp);
    val[i] = crit_fetch(pm, tp);
  }
  __syncthreads();
  // radix select: thr = the bit pattern of the KU-th smallest |x|, less = how many lie strictly below it
  unsigned thr = 0;
  int want = p.KU - 1, less = 0;
  if (p.KU > 0)
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const unsigned hi = pass ? 0xffffffffu << (shift + 8) : 0u;
      for (int i = tid; i < 256; i += CRIT_LT) hist[i] = 0;
      __syncthreads();
      for (int i = tid; i < p.KO; i += CRIT_LT) {
        const unsigned key = __float_as_uint(fabsf(val[i]));
        if (((key ^ thr) & hi) == 0) atomicAdd(&hist[(key >> shift) & 255], 1);      // integer counts: any order gives the same histogram
      }
      __syncthreads();
      if (tid == 0) {
        int cum = 0, bin = 0;
        for (; bin < 255; ++bin) {
          if (cum + hist[bin] > want) break;
          cum += hist[bin];
        }
        sel[0] = bin; sel[1] = cum;
      }
      __syncthreads();
      thr |= (unsigned)sel[0] << shift;
      want -= sel[1];
      less += sel[1];
      __syncthreads();
    }
  const int ties_needed = p.KU - less;
  // ordered compaction: thread t owns the points [t seg, (t + 1) seg)
  const int i0 = min(tid * p.seg, p.KO), i1 = min(i0 + p.seg, p.KO);
  int c_less = 0, c_tie = 0;
  if (p.KU > 0)
    for (int i = i0; i < i1; ++i) {
      const unsigned key = __float_as_uint(fabsf(val[i]));
      c_less += key < thr;
      c_tie += key == thr;
    }
  const int tie_before = crit_excl_scan(c_tie, scan, tid);
  const int take = min(max(ties_needed - tie_before, 0), c_tie);         // ties at the threshold go to the lower index
  int pos = crit_excl_scan(c_less + take, scan, tid);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  float* co = p.coords_out + (size_t)n * p.K * 2;
  if (p.KU > 0) {
    int taken = 0;
    for (int i = i0; i < i1; ++i) {
      const float x = val[i];
      const unsigned key = __float_as_uint(fabsf(x));
      bool pick = key < thr;
      if (key == thr && taken < take) { pick = true; ++taken; }
      if (!pick) continue;
      const float cx = ov[2 * (size_t)i], cy = ov[2 * (size_t)i + 1];
      CritTap tq;
      crit_tap(cx, cy, p.Hmax, p.Wmax, th, tw, &tq);
      crit_point_terms(x, crit_fetch(tm, tq), acc);
      if (pos < p.KU) {                                       // always: the counts add up to KU
        co[2 * (size_t)pos] = cx; co[2 * (size_t)pos + 1] = cy;
        if (p.idx_out) p.idx_out[(size_t)n * p.KU + pos] = i;
      }
      ++pos;
    }
  }
  const int KR = p.K - p.KU;
  const float* rn = p.rnd + (size_t)n * KR * 2;
  for (int j = tid; j < KR; j += CRIT_LT) {
    const float cx = rn[2 * (size_t)j], cy = rn[2 * (size_t)j + 1];
    CritTap tp, tq;
    crit_tap(cx, cy, p.H, p.W, p.H, p.W, &tp);
    crit_tap(cx, cy, p.Hmax, p.Wmax, th, tw, &tq);
    crit_point_terms(crit_fetch(pm, tp), crit_fetch(tm, tq), acc);
    co[2 * (size_t)(p.KU + j)] = cx; co[2 * (size_t)(p.KU + j) + 1] = cy;
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float s = wave_sum_dpp(acc[v]);
    if ((tid & 63) == 0) red[(tid >> 6) * 4 + v] = s;
  }
  __syncthreads();
  if (tid == 0) {
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int w = 0; w < CRIT_LT / 64; ++w)
      for (int v = 0; v < 4; ++v) t[v] += red[w * 4 + v];
    p.terms[2 * (size_t)n] = t[0] / (float)p.K;
    p.terms[2 * (size_t)n + 1] = 1.f - (2.f * t[3] + 1.f) / ((t[1] + t[2]) + 1.f);
    float* s = p.sums + 4 * (size_t)n;
    s[0] = t[1]; s[1] = t[2]; s[2] = t[3]; s[3] = 0.f;
  }
}

struct CritLayerStart { int at[CRIT_MAX_LAYERS + 1]; };

__global__ __launch_bounds__(64) void sf_crit_loss_finish_kernel(const float* terms, CritLayerStart st, int L, float num_masks, float* out, int out_stride) {
  const int l = (int)threadIdx.x;
  if (l >= L) return;
  float m = 0.f, d = 0.f;
  for (int n = st.at[l]; n < st.at[l + 1]; ++n) { m += terms[2 * (size_t)n]; d += terms[2 * (size_t)n + 1]; }      // pair order
  out[(size_t)l * out_stride] = m / num_masks;
  out[(size_t)l * out_stride + 1] = d / num_masks;
}

// ------------------------------------------------------------------------------------------------
// 4. backward of the mask losses
// ------------------------------------------------------------------------------------------------
struct CritBwdArgs {
  CritLayers lay; CritTargets tg;
  const int32_t* pairs; const float* coords; const float* sums; const float* up;      // up [L, 2]: d / d loss_mask_l, d / d loss_dice_l
  float* grad;                             // [L, B, Q, H, W], zeroed by the entry point
  int B, Q, H, W, K, Hmax, Wmax, in_lds;
  float num_masks;
};

__global__ __launch_bounds__(CRIT_BT) void sf_crit_loss_bwd_kernel(CritBwdArgs p) {
  extern __shared__ __attribute__((aligned(16))) float crit_smem[];
  const int tid = (int)threadIdx.x, n = (int)blockIdx.x, hw = p.H * p.W;
  const int l = p.pairs[4 * n], b = p.pairs[4 * n + 1], q = p.pairs[4 * n + 2], g = p.pairs[4 * n + 3];
  const int th = p.tg.H[b], tw = p.tg.W[b];
  const float* pm = p.lay.masks[l] + ((size_t)b * p.Q + q) * hw;
  const float* tm = p.tg.masks[b] + (size_t)g * th * tw;
  float* gp = p.grad + (((size_t)l * p.B + b) * p.Q + q) * hw;
  float* dst = p.in_lds ? crit_smem : gp;
  if (p.in_lds) {
    for (int i = tid; i < hw; i += CRIT_BT) crit_smem[i] = 0.f;
    __syncthreads();
  }
  const float S = p.sums[4 * (size_t)n], T = p.sums[4 * (size_t)n + 1], A = p.sums[4 * (size_t)n + 2], den = (S + T) + 1.f;
  const float um = p.up[2 * l] / (p.num_masks * (float)p.K), ud = p.up[2 * l + 1] / p.num_masks;
  const float* co = p.coords + (size_t)n * p.K * 2;
  for (int j = tid; j < p.K; j += CRIT_BT) {
    const float cx = co[2 * (size_t)j], cy = co[2 * (size_t)j + 1];
    CritTap tp, tq;
    crit_tap(cx, cy, p.H, p.W, p.H, p.W, &tp);
    crit_tap(cx, cy, p.Hmax, p.Wmax, th, tw, &tq);
    const float s = crit_sigmoid(crit_fetch(pm, tp)), t = crit_fetch(tm, tq);
    const float d_dice = -(2.f * t * den - (2.f * A + 1.f)) / (den * den);        // d dice / d sigmoid_j
    const float d = um * (s - t) + ud * d_dice * s * (1.f - s);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (tp.w[c] != 0.f) atomicAdd(&dst[tp.o[c]], tp.w[c] * d);
  }
  if (p.in_lds) {
    __syncthreads();
    for (int i = tid; i < hw; i += CRIT_BT)
      if (crit_smem[i] != 0.f) atomicAdd(&gp[i], crit_smem[i]);             // added, not stored: a foreign matcher may name a query twice
  }
}

// ------------------------------------------------------------------------------------------------
// 5. class loss
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sf_crit_class_fill_kernel(int32_t* tc, long long rows, int no_object) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < rows) tc[i] = no_object;
}
__global__ __launch_bounds__(256) void sf_crit_class_scatter_kernel(int32_t* tc, const int32_t* pairs, int N, CritTargets tg, int B, int Q, int C1) {
  const int n = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (n >= N) return;
  const int l = pairs[4 * n], b = pairs[4 * n + 1], q = pairs[4 * n + 2], g = pairs[4 * n + 3];
  const long long y = tg.labels[b][g];
  tc[((size_t)l * B + b) * Q + q] = (y >= 0 && y < C1) ? (int)y : C1 - 1;         // a label outside the table counts as no-object
}
// one wave per layer: the sum of the rows' class weights, lane-strided then the DPP tree
__global__ __launch_bounds__(64) void sf_crit_class_wsum_kernel(const int32_t* tc, const float* weight, int R, float* wsum) {
  const int l = (int)blockIdx.x;
  float a = 0.f;
  for (int r = (int)threadIdx.x; r < R; r += 64) a += weight[tc[(size_t)l * R + r]];
  a = wave_sum_dpp(a);
  if (threadIdx.x == 0) wsum[l] = a;
}
// one wave per row, four rows per workgroup (the row passes' shape, sf_rowwise.hip)
__global__ __launch_bounds__(256) void sf_crit_class_row_kernel(CritLayers lay, const int32_t* tc, const float* weight, const float* wsum, int R, int C1,
                                                                long long rows, float* rowloss, float* grad) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int l = (int)(row / R);
  const float* x = lay.logits[l] + (size_t)(row - (long long)l * R) * C1;
  float m = -INFINITY;
  for (int c = lane; c < C1; c += 64) m = fmaxf(m, x[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C1; c += 64) s += expf(x[c] - m);
  s = wave_sum(s);
  const int y = tc[row];
  const float wy = weight[y], f = wy / wsum[l];
  if (lane == 0) rowloss[row] = wy * ((m + logf(s)) - x[y]);
  if (grad)
    for (int c = lane; c < C1; c += 64) grad[(size_t)row * C1 + c] = f * (expf(x[c] - m) / s - (c == y ? 1.f : 0.f));
}
__global__ __launch_bounds__(64) void sf_crit_class_finish_kernel(const float* rowloss, const float* wsum, int R, float* out, int out_stride) {
  const int l = (int)blockIdx.x;
  float a = 0.f;
  for (int r = (int)threadIdx.x; r < R; r += 64) a += rowloss[(size_t)l * R + r];
  a = wave_sum_dpp(a);
  if (threadIdx.x == 0) out[(size_t)l * out_stride] = a / wsum[l];
}

// ------------------------------------------------------------------------------------------------
// entry points: every refusal happens before anything is launched
// ------------------------------------------------------------------------------------------------
static size_t crit_align(size_t b) { return (b + 255) & ~(size_t)255; }

static int crit_shape(const char* who, int L, int B, int Q, int H, int W) {
  if (L < 1 || B < 1 || Q < 1 || H < 1 || W < 1) return sf_set_err(SF_ERR_INVALID, "%s: L = %d, B = %d, Q = %d, H = %d, W = %d: all >= 1", who, L, B, Q, H, W);
  if (L > CRIT_MAX_LAYERS) return sf_set_err(SF_ERR_CAPACITY, "%s: L = %d layers exceed %d", who, L, CRIT_MAX_LAYERS);
  if (B > CRIT_MAX_IMAGES) return sf_set_err(SF_ERR_CAPACITY, "%s: B = %d images exceed %d", who, B, CRIT_MAX_IMAGES);
  if (Q > CRIT_MAX_Q) return sf_set_err(SF_ERR_CAPACITY, "%s: Q = %d queries exceed %d", who, Q, CRIT_MAX_Q);
  if ((long long)H * W > 0x3fffffffLL || (long long)B * Q * H * W > 0x7fffffffffLL) return sf_set_err(SF_ERR_CAPACITY, "%s: a predicted plane exceeds the index range", who);
  return SF_OK;
}
static int crit_layers(const char* who, const float* const* logits, const float* const* masks, int L, CritLayers* out) {
  for (int l = 0; l < L; ++l) {
    if ((logits && !logits[l]) || (masks && !masks[l])) return sf_set_err(SF_ERR_INVALID, "%s: layer %d: null tensor", who, l);
    out->logits[l] = logits ? logits[l] : nullptr;
    out->masks[l] = masks ? masks[l] : nullptr;
  }
  return SF_OK;
}
static int crit_targets(const char* who, const float* const* masks, const long long* const* labels, const int32_t* G, const int32_t* H, const int32_t* W, int B,
                        CritTargets* out, int* Gmax, int* Hmax, int* Wmax) {
  *Gmax = 0; *Hmax = 1; *Wmax = 1;
  for (int b = 0; b < B; ++b) {
    if (G[b] < 0) return sf_set_err(SF_ERR_INVALID, "%s: image %d: %d targets", who, b, G[b]);
    if (G[b] > CRIT_MAX_G) return sf_set_err(SF_ERR_CAPACITY, "%s: image %d: %d targets exceed %d", who, b, G[b], CRIT_MAX_G);
    if (G[b] > 0 && ((masks && !masks[b]) || (labels && !labels[b]))) return sf_set_err(SF_ERR_INVALID, "%s: image %d: null target tensor", who, b);
    if (G[b] > 0 && masks && (H[b] < 1 || W[b] < 1 || (long long)H[b] * W[b] > 0x3fffffffLL)) return sf_set_err(SF_ERR_INVALID, "%s: image %d: target masks of %d x %d", who, b, H[b], W[b]);
    out->masks[b] = masks ? masks[b] : nullptr;
    out->labels[b] = labels ? labels[b] : nullptr;
    out->G[b] = G[b]; out->H[b] = masks ? H[b] : 1; out->W[b] = masks ? W[b] : 1;
    if (G[b] > *Gmax) *Gmax = G[b];
    if (masks) { if (H[b] > *Hmax) *Hmax = H[b]; if (W[b] > *Wmax) *Wmax = W[b]; }      // an image without targets pads the batch as well
  }
  return SF_OK;
}

struct CritCostLayout { size_t xt, st, sp, ss, tt, total; int nch; };
static CritCostLayout crit_cost_layout(int L, int B, int Q, int Gmax, int K) {
  CritCostLayout w;
  w.nch = (K + CRIT_CHUNK - 1) / CRIT_CHUNK;
  const size_t slots = (size_t)L * B * w.nch;
  size_t o = 0;
  w.xt = o; o += crit_align(slots * Q * Gmax * sizeof(float));
  w.st = o; o += crit_align(slots * Q * Gmax * sizeof(float));
  w.sp = o; o += crit_align(slots * Q * sizeof(float));
  w.ss = o; o += crit_align(slots * Q * sizeof(float));
  w.tt = o; o += crit_align(slots * Gmax * sizeof(float));
  w.total = o;
  return w;
}

extern "C" size_t sf_op_crit_costs_workspace_bytes(int L, int B, int Q, int G_max, int K) {
  if (L < 1 || B < 1 || Q < 1 || G_max < 0 || K < 1) return 0;
  return crit_cost_layout(L, B, Q, G_max > 0 ? G_max : 1, K).total;
}

extern "C" int sf_op_crit_costs(const float* const* pred_logits, const float* const* pred_masks, int L, int B, int Q, int C1, int H, int W,
                                const float* const* tgt_masks, const int64_t* const* tgt_labels, const int32_t* tgt_G, const int32_t* tgt_H,
                                const int32_t* tgt_W, const float* coords_dev, int K, int G_max, float w_class, float w_mask, float w_dice,
                                float* cost_dev, void* workspace, size_t workspace_bytes, sf_stream stream) {
  const char* who = "sf_op_crit_costs";
  if (!pred_logits || !pred_masks || !tgt_masks || !tgt_labels || !tgt_G || !tgt_H || !tgt_W || !coords_dev || !cost_dev || !workspace)
    return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  SF_TRY(crit_shape(who, L, B, Q, H, W));
  if (C1 < 1 || K < 1) return sf_set_err(SF_ERR_INVALID, "%s: C + 1 = %d, K = %d: both >= 1", who, C1, K);
  if (C1 > CRIT_MAX_C) return sf_set_err(SF_ERR_CAPACITY, "%s: %d class logits exceed %d", who, C1, CRIT_MAX_C);
  CritCostArgs p;
  SF_TRY(crit_layers(who, pred_logits, pred_masks, L, &p.lay));
  int gmax, hmax, wmax;
  SF_TRY(crit_targets(who, tgt_masks, reinterpret_cast<const long long* const*>(tgt_labels), tgt_G, tgt_H, tgt_W, B, &p.tg, &gmax, &hmax, &wmax));
  if (G_max < gmax || G_max < 1) return sf_set_err(SF_ERR_INVALID, "%s: G_max = %d is below the largest image's %d targets (or below 1)", who, G_max, gmax);
  if (G_max > CRIT_MAX_G) return sf_set_err(SF_ERR_CAPACITY, "%s: G_max = %d exceeds %d", who, G_max, CRIT_MAX_G);
  const CritCostLayout w = crit_cost_layout(L, B, Q, G_max, K);
  SF_TRY(sf_check_workspace(who, "sf_op_crit_costs_workspace_bytes", workspace, workspace_bytes, w.total));
  if (gmax == 0) return SF_OK;                                 // no target anywhere: nothing is written
  char* ws = (char*)workspace;
  p.coords = coords_dev;
  p.p_xt = (float*)(ws + w.xt); p.p_st = (float*)(ws + w.st); p.p_sp = (float*)(ws + w.sp); p.p_ss = (float*)(ws + w.ss); p.p_tt = (float*)(ws + w.tt);
  p.B = B; p.Q = Q; p.H = H; p.W = W; p.K = K; p.Gmax = G_max; p.nch = w.nch; p.C1 = C1;
  const int gt = (gmax + 15) / 16;
  const dim3 grid((unsigned)w.nch, (unsigned)((Q + CRIT_QT - 1) / CRIT_QT), (unsigned)(L * B));
  const hipStream_t s = (hipStream_t)stream;
  if (gt <= 1) HIP_TRY(sf_launch_big_lds(sf_crit_cost_kernel<1>, grid, dim3(256), (size_t)(2 * CRIT_QT + 16) * CRIT_LD * 4, s, p));
  else if (gt <= 2) HIP_TRY(sf_launch_big_lds(sf_crit_cost_kernel<2>, grid, dim3(256), (size_t)(2 * CRIT_QT + 32) * CRIT_LD * 4, s, p));
  else if (gt <= 4) HIP_TRY(sf_launch_big_lds(sf_crit_cost_kernel<4>, grid, dim3(256), (size_t)(2 * CRIT_QT + 64) * CRIT_LD * 4, s, p));
  else HIP_TRY(sf_launch_big_lds(sf_crit_cost_kernel<8>, grid, dim3(256), (size_t)(2 * CRIT_QT + 128) * CRIT_LD * 4, s, p));
  const long long total = (long long)L * B * Q * G_max;
  HIP_TRY(sf_launch(sf_crit_cost_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, w_class, w_mask, w_dice, cost_dev, total));
  return SF_OK;
}

extern "C" int sf_op_crit_losses_capacity(void) { return CRIT_MAX_OVER; }

extern "C" size_t sf_op_crit_losses_workspace_bytes(int N) { return N < 0 ? 0 : crit_align((size_t)(N > 0 ? N : 1) * 2 * sizeof(float)); }

static int crit_pairs(const char* who, const int32_t* layer_start, int L, int N) {
  if (layer_start[0] != 0 || layer_start[L] != N) return sf_set_err(SF_ERR_INVALID, "%s: layer_start must run from 0 to N = %d", who, N);
  for (int l = 0; l < L; ++l)
    if (layer_start[l + 1] < layer_start[l]) return sf_set_err(SF_ERR_INVALID, "%s: layer_start decreases at layer %d", who, l);
  return SF_OK;
}

extern "C" int sf_op_crit_losses(const float* const* pred_masks, int L, int B, int Q, int H, int W, const float* const* tgt_masks, const int32_t* tgt_G,
                                 const int32_t* tgt_H, const int32_t* tgt_W, const int32_t* pairs_dev, const int32_t* layer_start, int N,
                                 const float* over_dev, const float* rand_dev, int K, int K_over, int K_uncertain, float num_masks,
                                 float* losses_dev, int losses_stride, float* coords_out_dev, float* sums_dev, int32_t* idx_out_dev, void* workspace,
                                 size_t workspace_bytes, sf_stream stream) {
  const char* who = "sf_op_crit_losses";
  if (!pred_masks || !tgt_masks || !tgt_G || !tgt_H || !tgt_W || !layer_start || !losses_dev || !workspace) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  SF_TRY(crit_shape(who, L, B, Q, H, W));
  if (N < 0 || K < 1 || K_over < K_uncertain || K_uncertain < 0 || K_uncertain > K || losses_stride < 2 || !(num_masks > 0.f))
    return sf_set_err(SF_ERR_INVALID, "%s: N = %d, K = %d, K_over = %d, K_uncertain = %d, stride %d, num_masks %g", who, N, K, K_over, K_uncertain, losses_stride, (double)num_masks);
  if (K_over > CRIT_MAX_OVER)
    return sf_set_err(SF_ERR_CAPACITY, "%s: %d oversampled points per pair exceed %d (a pair's values stay in the CU's LDS)", who, K_over, CRIT_MAX_OVER);
  if (N > 0 && (!pairs_dev || !coords_out_dev || !sums_dev || (K_over > 0 && !over_dev) || (K > K_uncertain && !rand_dev)))
    return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  CritLossArgs p;
  SF_TRY(crit_layers(who, nullptr, pred_masks, L, &p.lay));
  int gmax, hmax, wmax;
  SF_TRY(crit_targets(who, tgt_masks, nullptr, tgt_G, tgt_H, tgt_W, B, &p.tg, &gmax, &hmax, &wmax));
  SF_TRY(crit_pairs(who, layer_start, L, N));
  SF_TRY(sf_check_workspace(who, "sf_op_crit_losses_workspace_bytes", workspace, workspace_bytes, sf_op_crit_losses_workspace_bytes(N)));
  const hipStream_t s = (hipStream_t)stream;
  p.pairs = pairs_dev; p.over = over_dev; p.rnd = rand_dev; p.coords_out = coords_out_dev; p.sums = sums_dev; p.terms = (float*)workspace; p.idx_out = idx_out_dev;
  p.B = B; p.Q = Q; p.H = H; p.W = W; p.K = K; p.KO = K_over; p.KU = K_uncertain; p.Hmax = hmax; p.Wmax = wmax;
  p.seg = ((K_over + CRIT_LT - 1) / CRIT_LT) | 1;             // odd: the threads of a wave walk different LDS banks
  if (N > 0) HIP_TRY(sf_launch_big_lds(sf_crit_loss_kernel, dim3((unsigned)N), dim3(CRIT_LT), ((size_t)K_over + CRIT_LOSS_MISC) * 4, s, p));
  CritLayerStart st = {};
  for (int l = 0; l <= L; ++l) st.at[l] = layer_start[l];
  HIP_TRY(sf_launch(sf_crit_loss_finish_kernel, dim3(1), dim3(64), 0, s, (const float*)workspace, st, L, num_masks, losses_dev, losses_stride));
  return SF_OK;
}

extern "C" int sf_op_crit_losses_backward(const float* const* pred_masks, int L, int B, int Q, int H, int W, const float* const* tgt_masks,
                                          const int32_t* tgt_G, const int32_t* tgt_H, const int32_t* tgt_W, const int32_t* pairs_dev, int N,
                                          const float* coords_dev, const float* sums_dev, int K, float num_masks, const float* upstream_dev,
                                          float* grad_pred_masks_dev, sf_stream stream) {
  const char* who = "sf_op_crit_losses_backward";
  if (!pred_masks || !tgt_masks || !tgt_G || !tgt_H || !tgt_W || !upstream_dev || !grad_pred_masks_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  SF_TRY(crit_shape(who, L, B, Q, H, W));
  if (N < 0 || K < 1 || !(num_masks > 0.f)) return sf_set_err(SF_ERR_INVALID, "%s: N = %d, K = %d, num_masks %g", who, N, K, (double)num_masks);
  if (N > 0 && (!pairs_dev || !coords_dev || !sums_dev)) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  CritBwdArgs p;
  SF_TRY(crit_layers(who, nullptr, pred_masks, L, &p.lay));
  int gmax, hmax, wmax;
  SF_TRY(crit_targets(who, tgt_masks, nullptr, tgt_G, tgt_H, tgt_W, B, &p.tg, &gmax, &hmax, &wmax));
  const hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(grad_pred_masks_dev, 0, (size_t)L * B * Q * H * W * sizeof(float), s));
  if (N == 0) return SF_OK;
  p.pairs = pairs_dev; p.coords = coords_dev; p.sums = sums_dev; p.up = upstream_dev; p.grad = grad_pred_masks_dev;
  p.B = B; p.Q = Q; p.H = H; p.W = W; p.K = K; p.Hmax = hmax; p.Wmax = wmax; p.num_masks = num_masks;
  p.in_lds = (long long)H * W <= CRIT_BWD_PLANE ? 1 : 0;
  HIP_TRY(sf_launch_big_lds(sf_crit_loss_bwd_kernel, dim3((unsigned)N), dim3(CRIT_BT), p.in_lds ? (size_t)H * W * 4 : 0, s, p));
  return SF_OK;
}

struct CritClassLayout { size_t tc, wsum, rowloss, total; };
static CritClassLayout crit_class_layout(int L, long long R) {
  CritClassLayout w;
  size_t o = 0;
  w.tc = o; o += crit_align((size_t)L * R * sizeof(int32_t));
  w.wsum = o; o += crit_align((size_t)L * sizeof(float));
  w.rowloss = o; o += crit_align((size_t)L * R * sizeof(float));
  w.total = o;
  return w;
}

extern "C" size_t sf_op_crit_class_loss_workspace_bytes(int L, int B, int Q) {
  if (L < 1 || B < 1 || Q < 1) return 0;
  return crit_class_layout(L, (long long)B * Q).total;
}

extern "C" int sf_op_crit_class_loss(const float* const* pred_logits, int L, int B, int Q, int C1, const int32_t* pairs_dev, int N,
                                     const int64_t* const* tgt_labels, const int32_t* tgt_G, const float* weight_dev, float* losses_dev,
                                     int losses_stride, float* grad_dev, int32_t* target_classes_out_dev, void* workspace, size_t workspace_bytes,
                                     sf_stream stream) {
  const char* who = "sf_op_crit_class_loss";
  if (!pred_logits || !tgt_labels || !tgt_G || !weight_dev || !losses_dev || !workspace) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  SF_TRY(crit_shape(who, L, B, Q, 1, 1));
  if (C1 < 1 || N < 0 || losses_stride < 1 || (N > 0 && !pairs_dev)) return sf_set_err(SF_ERR_INVALID, "%s: C + 1 = %d, N = %d, stride %d", who, C1, N, losses_stride);
  if (C1 > CRIT_MAX_C) return sf_set_err(SF_ERR_CAPACITY, "%s: %d class logits exceed %d", who, C1, CRIT_MAX_C);
  CritLayers lay;
  SF_TRY(crit_layers(who, pred_logits, nullptr, L, &lay));
  CritTargets tg;
  int gmax, hmax, wmax;
  SF_TRY(crit_targets(who, nullptr, reinterpret_cast<const long long* const*>(tgt_labels), tgt_G, nullptr, nullptr, B, &tg, &gmax, &hmax, &wmax));
  const long long R = (long long)B * Q, rows = R * L;
  const CritClassLayout w = crit_class_layout(L, R);
  SF_TRY(sf_check_workspace(who, "sf_op_crit_class_loss_workspace_bytes", workspace, workspace_bytes, w.total));
  char* ws = (char*)workspace;
  int32_t* tc = target_classes_out_dev ? target_classes_out_dev : (int32_t*)(ws + w.tc);
  float* wsum = (float*)(ws + w.wsum);
  float* rowloss = (float*)(ws + w.rowloss);
  const hipStream_t s = (hipStream_t)stream;
  HIP_TRY(sf_launch(sf_crit_class_fill_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, tc, rows, C1 - 1));
  if (N > 0) HIP_TRY(sf_launch(sf_crit_class_scatter_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, tc, pairs_dev, N, tg, B, Q, C1));
  HIP_TRY(sf_launch(sf_crit_class_wsum_kernel, dim3((unsigned)L), dim3(64), 0, s, (const int32_t*)tc, weight_dev, (int)R, wsum));
  HIP_TRY(sf_launch(sf_crit_class_row_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, lay, (const int32_t*)tc, weight_dev, (const float*)wsum, (int)R, C1,
                    rows, rowloss, grad_dev));
  HIP_TRY(sf_launch(sf_crit_class_finish_kernel, dim3((unsigned)L), dim3(64), 0, s, (const float*)rowloss, (const float*)wsum, (int)R, losses_dev, losses_stride));
  return SF_OK;
}
