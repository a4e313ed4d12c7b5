// Image segmentation: the three kernels between the mask decoder's per-image outputs and the semantic and panoptic results of
// MaskFormer's semantic_inference / panoptic_inference (mask2former/maskformer_model.py).  Instance inference needs none of them: it is
// sf_op_vis_scores + sf_op_vis_postprocess with an index table [K, 1].  All fp32, bit-reproducible (every float sum has one fixed order,
// only integer counts go through atomics), on the caller's stream, without allocation or host synchronisation.
//
// Geometry is sf_op_vis_postprocess's: source h x w, resample to Hp x Wp, keep the top left Hc x Wc, resample to H x W, both resamples by
// F.interpolate(bilinear, align_corners=False)'s rule, composed per output pixel with the arithmetic of sf_vis_postprocess_kernel (the
// same coordinate function, sf_vis_axis.h, and the same order of the lerps): r_q(y, x).  Neither [Q, Hp, Wp] nor [Q, H, W] is formed.
//
//   sf_seg_semantic_kernel         out[c, y, x] = sum_q probs[q, c] sigmoid(r_q(y, x)).  A workgroup (four waves) owns 64 pixels of one
//                                  output row.  Queries go in chunks of 32: the chunk's source boxes and its rows of the class table are
//                                  staged in LDS, wave w writes sigmoid(r_q) of queries w, w + 4, .. for the 64 pixels to LDS, then every
//                                  wave contracts ITS 16 pixels with every class tile on v_mfma_f32_16x16x4_f32 (A = classes x 4 queries,
//                                  B = 4 queries x 16 pixels), one accumulator per class tile: a query-ordered fmaf chain per output
//                                  element.  A lane ends with four classes of one pixel; 16 lanes store 64 consecutive bytes of a class row.
//   sf_seg_panoptic_argmax_kernel  one thread per pixel of a 4 x 64 tile walks the KEPT queries (labels[q] != num_classes and
//                                  max_scores[q] > threshold, decided here) in query order and keeps the first largest
//                                  max_scores[q] sigmoid(r_q), with that query's r_q >= 0: code = 2 q + bit, or -1.  Per query the three
//                                  integer counts are gathered in LDS (a ballot per wave for r_q >= 0) and added to counts_dev once per tile.
//   sf_seg_panoptic_relabel_kernel code -> segment id, elementwise.
#include "sf_internal.h"
#include "sf_common.h"
#include "sf_launch.h"
#include "sf_handle.h"
#include "sf_vis_axis.h"

#define SEG_THREADS 256
#define SEG_TILE_W 64                      // pixels of a row per workgroup: 16 per wave, one MFMA N tile
#define SEG_PAN_TILE_H 4                   // the panoptic tile: 4 rows x 64 columns, one pixel per thread
#define SEG_QC 32                          // queries per chunk of the semantic kernel
#define SEG_SIG_LD (SEG_TILE_W + 16)       // row pitch of the sigmoid tile: rows k and k + 1 of an MFMA B read land on different banks
#define SEG_MAX_Q 512
#define SEG_MAX_C 256
#define SEG_LDS_MAX (128 * 1024)

struct SfSegGeo {
  int h, w, Hc, Wc, H, W;
  float ry1, rx1, ry2, rx2;                // source pixels per padded pixel; cropped pixels per output pixel
};

// one output coordinate: its two taps of the cropped intermediate, each with two source taps (relative to the staged box) and a weight
struct SfSegAxis { int i[2][2]; float l[2]; float l2; };

SF_DEVICE void seg_axis(int dst, float r2, int crop, float r1, int in, int lo, int extent, SfSegAxis* a) {
  int M[2];
  vis_axis(dst, r2, crop, &M[0], &M[1], &a->l2);
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    vis_axis(M[t], r1, in, &a->i[t][0], &a->i[t][1], &a->l[t]);
    a->i[t][0] = min(max(a->i[t][0] - lo, 0), extent - 1);      // the clamps are never active: the box was sized by vis_reach
    a->i[t][1] = min(max(a->i[t][1] - lo, 0), extent - 1);
  }
}

// r_q at one pixel from a staged box of pitch bw: the expression of sf_vis_postprocess_kernel
SF_DEVICE float seg_sample(const float* box, int bw, const SfSegAxis& y, const SfSegAxis& x) {
  float mid[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const float v00 = box[y.i[a][0] * bw + x.i[b][0]], v01 = box[y.i[a][0] * bw + x.i[b][1]];
      const float v10 = box[y.i[a][1] * bw + x.i[b][0]], v11 = box[y.i[a][1] * bw + x.i[b][1]];
      mid[a][b] = (1.f - y.l[a]) * ((1.f - x.l[b]) * v00 + x.l[b] * v01) + y.l[a] * ((1.f - x.l[b]) * v10 + x.l[b] * v11);
    }
  return (1.f - y.l2) * ((1.f - x.l2) * mid[0][0] + x.l2 * mid[0][1]) + y.l2 * ((1.f - x.l2) * mid[1][0] + x.l2 * mid[1][1]);
}

SF_DEVICE float seg_sigmoid(float o) { return 1.f / (1.f + expf(-o)); }

// the staged box of a tile of output rows y0..y1 and columns x0..x1, cut to `floats` (never needed: the entry points sized the LDS with
// vis_reach over every tile and added slack; kept so that a mistake there could only give wrong pixels, never an access outside the LDS)
SF_DEVICE void seg_box(const SfSegGeo& g, int y0, int y1, int x0, int x1, int floats, int* sy_lo, int* sx_lo, int* bh, int* bw) {
  int sy_hi, sx_hi;
  vis_reach(y0, y1, g.ry2, g.Hc, g.ry1, g.h, sy_lo, &sy_hi);
  vis_reach(x0, x1, g.rx2, g.Wc, g.rx1, g.w, sx_lo, &sx_hi);
  *bw = sx_hi - *sx_lo + 1;
  *bh = sy_hi - *sy_lo + 1;
  if (*bh * *bw > floats) {
    *bw = min(*bw, floats);
    *bh = max(floats / *bw, 1);
  }
}

// ------------------------------------------------------------------------------------------------
// a. semantic map
// ------------------------------------------------------------------------------------------------
struct SfSegSem {
  const float* src; const float* probs; float* out;
  int Q, C, ctiles, ld_p, box_floats;
  SfSegGeo g;
};

template <int CT>      // class tiles of 16 held by a wave, ceil(C / 16) <= CT
__global__ __launch_bounds__(SEG_THREADS) void sf_seg_semantic_kernel(SfSegSem p) {
  extern __shared__ __attribute__((aligned(16))) float seg_smem[];
  float* pt = seg_smem;                                       // [SEG_QC][ld_p]: the chunk's rows of the class table, zero padded
  float* sig = pt + SEG_QC * p.ld_p;                          // [SEG_QC][SEG_SIG_LD]
  float* box = sig + SEG_QC * SEG_SIG_LD;                     // [SEG_QC][box_floats]
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, g4 = lane >> 4;
  const int y = (int)blockIdx.y, x_first = (int)blockIdx.x * SEG_TILE_W, x_last = min(x_first + SEG_TILE_W, p.g.W) - 1;
  int sy_lo, sx_lo, bh, bw;
  seg_box(p.g, y, y, x_first, x_last, p.box_floats, &sy_lo, &sx_lo, &bh, &bw);
  const int n = bh * bw, cp = p.ctiles * 16;
  SfSegAxis ay, ax;                                           // of the pixel this thread makes sigmoids for; past W the last one again
  seg_axis(y, p.g.ry2, p.g.Hc, p.g.ry1, p.g.h, sy_lo, bh, &ay);
  seg_axis(min(x_first + lane, p.g.W - 1), p.g.rx2, p.g.Wc, p.g.rx1, p.g.w, sx_lo, bw, &ax);
  f32x4_t acc[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < p.Q; q0 += SEG_QC) {
    const int nq = min(SEG_QC, p.Q - q0), nq4 = (nq + 3) & ~3;
    __syncthreads();                                          // the last chunk's reads are done
    for (int i = tid; i < nq4 * cp; i += SEG_THREADS) {
      const int r = i / cp, c = i - r * cp;
      pt[r * p.ld_p + c] = (r < nq && c < p.C) ? p.probs[(size_t)(q0 + r) * p.C + c] : 0.f;
    }
    for (int i = tid; i < nq * n; i += SEG_THREADS) {
      const int qq = i / n, j = i - qq * n, r = j / bw, c = j - r * bw;
      box[qq * p.box_floats + j] = p.src[((size_t)(q0 + qq) * p.g.h + sy_lo + r) * p.g.w + sx_lo + c];
    }
    __syncthreads();
    for (int qq = wave; qq < nq4; qq += SEG_THREADS / 64)     // rows nq..nq4 of the last k step are zeros
      sig[qq * SEG_SIG_LD + lane] = qq < nq ? seg_sigmoid(seg_sample(box + qq * p.box_floats, bw, ay, ax)) : 0.f;
    __syncthreads();
    const float* a = pt + g4 * p.ld_p + l15;                  // A[class l15][query g4]
    const float* b = sig + g4 * SEG_SIG_LD + wave * 16 + l15; // B[query g4][pixel l15]
    for (int k = 0; k < nq4; k += 4) {
      const float bv = b[k * SEG_SIG_LD];
#pragma unroll
      for (int t = 0; t < CT; ++t)
        if (t < p.ctiles) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[k * p.ld_p + t * 16], bv, acc[t], 0, 0, 0);
    }
  }
  const int xo = x_first + wave * 16 + l15;                   // D: pixel l15, classes 4 g4 + r
  if (xo >= p.g.W) return;
#pragma unroll
  for (int t = 0; t < CT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = t * 16 + 4 * g4 + r;
      if (c < p.C) p.out[((size_t)c * p.g.H + y) * p.g.W + xo] = acc[t][r];
    }
}

// ------------------------------------------------------------------------------------------------
// b. panoptic argmax and counts, c. relabel
// ------------------------------------------------------------------------------------------------
struct SfSegPan {
  const float* src; const float* max_scores; const int32_t* labels; int32_t* code; int32_t* counts;
  int Q, num_classes, qc, box_floats, cnt_floats;
  float thr;
  SfSegGeo g;
};

__global__ __launch_bounds__(SEG_THREADS) void sf_seg_panoptic_argmax_kernel(SfSegPan p) {
  extern __shared__ __attribute__((aligned(16))) float seg_smem[];
  int* cnt = reinterpret_cast<int*>(seg_smem);                // [Q][3]: won, r_q >= 0, both
  float* box = seg_smem + p.cnt_floats;                       // [qc][box_floats]
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int y_first = (int)blockIdx.y * SEG_PAN_TILE_H, x_first = (int)blockIdx.x * SEG_TILE_W;
  const int y = y_first + (tid >> 6), x = x_first + lane;
  const bool inside = y < p.g.H && x < p.g.W;
  for (int i = tid; i < 3 * p.Q; i += SEG_THREADS) cnt[i] = 0;
  int sy_lo, sx_lo, bh, bw;
  seg_box(p.g, y_first, min(y_first + SEG_PAN_TILE_H, p.g.H) - 1, x_first, min(x_first + SEG_TILE_W, p.g.W) - 1, p.box_floats, &sy_lo, &sx_lo, &bh, &bw);
  const int n = bh * bw;
  SfSegAxis ay, ax;
  seg_axis(min(y, p.g.H - 1), p.g.ry2, p.g.Hc, p.g.ry1, p.g.h, sy_lo, bh, &ay);
  seg_axis(min(x, p.g.W - 1), p.g.rx2, p.g.Wc, p.g.rx1, p.g.w, sx_lo, bw, &ax);
  float best = -INFINITY;
  int arg = -1, bit = 0;
  for (int q0 = 0; q0 < p.Q; q0 += p.qc) {
    const int nq = min(p.qc, p.Q - q0);
    __syncthreads();                                          // the last chunk's reads are done (and, the first time, cnt is zero)
    for (int i = tid; i < nq * n; i += SEG_THREADS) {
      const int qq = i / n, j = i - qq * n, r = j / bw, c = j - r * bw, q = q0 + qq;
      if (p.labels[q] != p.num_classes && p.max_scores[q] > p.thr)
        box[qq * p.box_floats + j] = p.src[((size_t)q * p.g.h + sy_lo + r) * p.g.w + sx_lo + c];
    }
    __syncthreads();
    for (int qq = 0; qq < nq; ++qq) {                         // query order: the reference's compacted order
      const int q = q0 + qq;
      const float s = p.max_scores[q];
      if (p.labels[q] == p.num_classes || !(s > p.thr)) continue;      // the same in every thread
      const float o = seg_sample(box + qq * p.box_floats, bw, ay, ax);
      const unsigned long long pos = __ballot(inside && o >= 0.f);
      if (lane == 0 && pos) atomicAdd(&cnt[3 * q + 1], __popcll(pos));
      const float v = s * seg_sigmoid(o);
      if (v > best) { best = v; arg = q; bit = o >= 0.f ? 1 : 0; }     // strictly above: the first index keeps a tie
    }
  }
  if (inside) {
    p.code[(size_t)y * p.g.W + x] = arg < 0 ? -1 : 2 * arg + bit;
    if (arg >= 0) {
      atomicAdd(&cnt[3 * arg], 1);
      if (bit) atomicAdd(&cnt[3 * arg + 2], 1);
    }
  }
  __syncthreads();
  for (int i = tid; i < 3 * p.Q; i += SEG_THREADS)
    if (cnt[i]) atomicAdd(&p.counts[i], cnt[i]);              // integers: any order gives the same sum
}

__global__ __launch_bounds__(SEG_THREADS) void sf_seg_panoptic_relabel_kernel(const int32_t* code, const int32_t* __restrict__ segment_of_query, int Q, long long pixels,
                                                                              int32_t* out) {      // out may be code: one element, one thread
  const long long i = (long long)blockIdx.x * SEG_THREADS + threadIdx.x;
  if (i >= pixels) return;
  const int c = code[i];
  out[i] = (c >= 0 && (c & 1) && (c >> 1) < Q) ? segment_of_query[c >> 1] : 0;
}

// ------------------------------------------------------------------------------------------------
// entry points: every refusal happens before anything is launched
// ------------------------------------------------------------------------------------------------
static int seg_geometry(const char* who, int h, int w, int Hp, int Wp, int Hc, int Wc, int H, int W, SfSegGeo* g) {
  if (h < 1 || w < 1 || H < 1 || W < 1) return sf_set_err(SF_ERR_INVALID, "%s: h = %d, w = %d, H = %d, W = %d: all >= 1", who, h, w, H, W);
  if (Hc < 1 || Wc < 1 || Hc > Hp || Wc > Wp) return sf_set_err(SF_ERR_INVALID, "%s: the crop %d x %d must lie inside the padded size %d x %d", who, Hc, Wc, Hp, Wp);
  if ((long long)h * w > 0x7fffffffLL || (long long)H * W > 0x7fffffffLL || H > 65535) return sf_set_err(SF_ERR_CAPACITY, "%s: a plane exceeds the index range (H up to 65535)", who);
  g->h = h; g->w = w; g->Hc = Hc; g->Wc = Wc; g->H = H; g->W = W;
  g->ry1 = (float)h / (float)Hp; g->rx1 = (float)w / (float)Wp; g->ry2 = (float)Hc / (float)H; g->rx2 = (float)Wc / (float)W;
  return SF_OK;
}

// the largest source box of any tile of tile_h x SEG_TILE_W output pixels, from the kernels' own index rule, plus two pixels of slack per axis
static int seg_box_floats(const SfSegGeo& g, int tile_h) {
  int bh = 1, bw = 1, lo, hi;
  for (int y = 0; y < g.H; y += tile_h) {
    vis_reach(y, y + tile_h < g.H ? y + tile_h - 1 : g.H - 1, g.ry2, g.Hc, g.ry1, g.h, &lo, &hi);
    bh = hi - lo + 1 > bh ? hi - lo + 1 : bh;
  }
  for (int x = 0; x < g.W; x += SEG_TILE_W) {
    vis_reach(x, x + SEG_TILE_W < g.W ? x + SEG_TILE_W - 1 : g.W - 1, g.rx2, g.Wc, g.rx1, g.w, &lo, &hi);
    bw = hi - lo + 1 > bw ? hi - lo + 1 : bw;
  }
  bh = bh + 2 < g.h ? bh + 2 : g.h;
  bw = bw + 2 < g.w ? bw + 2 : g.w;
  const long long n = (long long)bh * bw;
  return n > 0x3fffffffLL ? 0x3fffffff : (int)n;
}

extern "C" int sf_op_seg_semantic(const float* masks_dev, const float* probs_dev, int Q, int C, int h, int w, int Hp, int Wp, int Hc, int Wc, int H, int W,
                                  float* out_dev, sf_stream stream) {
  const char* who = "sf_op_seg_semantic";
  if (!masks_dev || !probs_dev || !out_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (Q < 1 || C < 1) return sf_set_err(SF_ERR_INVALID, "%s: Q = %d, C = %d: both >= 1", who, Q, C);
  if (Q > SEG_MAX_Q) return sf_set_err(SF_ERR_CAPACITY, "%s: Q = %d queries exceed %d", who, Q, SEG_MAX_Q);
  if (C > SEG_MAX_C) return sf_set_err(SF_ERR_CAPACITY, "%s: C = %d classes exceed %d (a wave holds every class tile of its pixels)", who, C, SEG_MAX_C);
  SfSegSem p;
  SF_TRY(seg_geometry(who, h, w, Hp, Wp, Hc, Wc, H, W, &p.g));
  p.src = masks_dev; p.probs = probs_dev; p.out = out_dev; p.Q = Q; p.C = C;
  p.ctiles = (C + 15) / 16;
  const int cp = p.ctiles * 16;
  p.ld_p = (cp & 31) == 16 ? cp : cp + 16;                    // an odd multiple of 16: rows k and k + 1 of an MFMA A read land on different banks
  p.box_floats = seg_box_floats(p.g, 1);
  const size_t lds = ((size_t)SEG_QC * (p.ld_p + SEG_SIG_LD) + (size_t)SEG_QC * p.box_floats) * 4;
  if (lds > SEG_LDS_MAX) return sf_set_err(SF_ERR_CAPACITY, "%s: a 1 x %d output tile reaches %d source pixels per query, more than the LDS holds for %d queries (the output is too small for the masks)", who, SEG_TILE_W, p.box_floats, SEG_QC);
  const dim3 grid((unsigned)((W + SEG_TILE_W - 1) / SEG_TILE_W), (unsigned)H);
  const hipStream_t s = (hipStream_t)stream;
  if (p.ctiles <= 1) HIP_TRY(sf_launch_big_lds(sf_seg_semantic_kernel<1>, grid, dim3(SEG_THREADS), lds, s, p));
  else if (p.ctiles <= 2) HIP_TRY(sf_launch_big_lds(sf_seg_semantic_kernel<2>, grid, dim3(SEG_THREADS), lds, s, p));
  else if (p.ctiles <= 4) HIP_TRY(sf_launch_big_lds(sf_seg_semantic_kernel<4>, grid, dim3(SEG_THREADS), lds, s, p));
  else if (p.ctiles <= 8) HIP_TRY(sf_launch_big_lds(sf_seg_semantic_kernel<8>, grid, dim3(SEG_THREADS), lds, s, p));
  else HIP_TRY(sf_launch_big_lds(sf_seg_semantic_kernel<16>, grid, dim3(SEG_THREADS), lds, s, p));
  return SF_OK;
}

extern "C" int sf_op_seg_panoptic_argmax(const float* masks_dev, const float* max_scores_dev, const int32_t* labels_dev, int Q, int num_classes,
                                         float object_mask_threshold, int h, int w, int Hp, int Wp, int Hc, int Wc, int H, int W, int32_t* code_dev,
                                         int32_t* counts_dev, sf_stream stream) {
  const char* who = "sf_op_seg_panoptic_argmax";
  if (!masks_dev || !max_scores_dev || !labels_dev || !code_dev || !counts_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (Q < 1) return sf_set_err(SF_ERR_INVALID, "%s: Q = %d (>= 1)", who, Q);
  if (Q > SEG_MAX_Q) return sf_set_err(SF_ERR_CAPACITY, "%s: Q = %d queries exceed %d", who, Q, SEG_MAX_Q);
  SfSegPan p;
  SF_TRY(seg_geometry(who, h, w, Hp, Wp, Hc, Wc, H, W, &p.g));
  if ((H + SEG_PAN_TILE_H - 1) / SEG_PAN_TILE_H > 65535) return sf_set_err(SF_ERR_CAPACITY, "%s: H = %d exceeds one grid", who, H);
  p.src = masks_dev; p.max_scores = max_scores_dev; p.labels = labels_dev; p.code = code_dev; p.counts = counts_dev;
  p.Q = Q; p.num_classes = num_classes; p.thr = object_mask_threshold;
  p.cnt_floats = (3 * Q + 3) & ~3;
  p.box_floats = seg_box_floats(p.g, SEG_PAN_TILE_H);
  const long long room = ((long long)SEG_LDS_MAX / 4 - p.cnt_floats) / p.box_floats;
  if (room < 1) return sf_set_err(SF_ERR_CAPACITY, "%s: a %d x %d output tile reaches %d source pixels, more than the LDS holds (the output is too small for the masks)", who, SEG_PAN_TILE_H, SEG_TILE_W, p.box_floats);
  // a chunk of at most 16 KB of boxes, so that several workgroups share a CU, and never less than one query
  const long long modest = (16 * 1024 / 4) / p.box_floats;
  p.qc = (int)(modest < 1 ? 1 : modest);
  p.qc = p.qc > Q ? Q : p.qc;
  const size_t lds = ((size_t)p.cnt_floats + (size_t)p.qc * p.box_floats) * 4;
  const hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(counts_dev, 0, (size_t)Q * 3 * sizeof(int32_t), s));
  const dim3 grid((unsigned)((W + SEG_TILE_W - 1) / SEG_TILE_W), (unsigned)((H + SEG_PAN_TILE_H - 1) / SEG_PAN_TILE_H));
  HIP_TRY(sf_launch_big_lds(sf_seg_panoptic_argmax_kernel, grid, dim3(SEG_THREADS), lds, s, p));
  return SF_OK;
}

extern "C" int sf_op_seg_panoptic_relabel(const int32_t* code_dev, const int32_t* segment_of_query_dev, int Q, long long pixels, int32_t* panoptic_dev,
                                          sf_stream stream) {
  const char* who = "sf_op_seg_panoptic_relabel";
  if (!code_dev || !segment_of_query_dev || !panoptic_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (Q < 1 || pixels < 1) return sf_set_err(SF_ERR_INVALID, "%s: Q = %d, pixels = %lld: both >= 1", who, Q, pixels);
  const long long blocks = (pixels + SEG_THREADS - 1) / SEG_THREADS;
  if (blocks > 0x7fffffffLL) return sf_set_err(SF_ERR_CAPACITY, "%s: %lld pixels exceed one grid", who, pixels);
  HIP_TRY(sf_launch(sf_seg_panoptic_relabel_kernel, dim3((unsigned)blocks), dim3(SEG_THREADS), 0, (hipStream_t)stream, code_dev, segment_of_query_dev, Q, pixels,
                    panoptic_dev));
  return SF_OK;
}
