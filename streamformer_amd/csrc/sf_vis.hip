// Video instance segmentation: the four kernels between the mask decoder's per-frame outputs and a list of instances
// (ctvis/modeling/tracker/simple_tracker.py, ctvis/utils/utils.py mask_nms, ctvis_model.py inference_video).  All fp32, none needs MFMA:
// three small frame-local passes that run once per clip before the host's association loop, and the mask resampling, which moves the
// bytes.  Every output element has one owner and every sum one fixed order (wave shuffles, then the block's waves in order, then one
// owner pass over the block partials): bit-reproducible, no float atomics.
//
//   sf_vis_scores_kernel       one wave per row of pred_logits [rows, C + 1]: softmax over the whole row, the last class dropped; the
//                              largest score and its FIRST index (torch.max's rule on ties), optionally all C scores.
//   sf_vis_pack_kernel         one workgroup per mask row [pixels]: bit p & 31 of word p / 32 is x[p] > 0 (what mask_nms's
//                              sigmoid(x) > 0.5 decides), tail bits zero, and the row's area.  A lane reads four pixels (16 bytes when the
//                              row length allows it), eight lanes make a word.
//   sf_vis_inter_kernel        one workgroup per (frame, i): row i's words sit in LDS, wave j sums popcount(row i & row j).
//   sf_vis_postprocess_kernel  inference_video's two chained F.interpolate(bilinear, align_corners=False) with the crop between them,
//                              composed per output pixel: the output pixel mixes four pixels of the CROPPED intermediate (edge clamp at
//                              the crop's last row / column, never a padded pixel), each of those mixes four source pixels.  A workgroup
//                              owns 16 rows x 256 columns of one (instance, frame) plane and stages the source box those pixels reach in
//                              LDS; a thread makes 16 consecutive pixels of a row and stores them as one 16-byte word of bool bytes (and
//                              four float4 of logits, on request).  An index of -1 (or outside the detections) writes zeros and adds
//                              nothing.  Identity geometry gathers rows unchanged (SimpleTracker's dense masks).
//   sf_vis_reduce_kernel       the owner pass: per instance the sum of its workgroups' (sigmoid sum, pixel count) partials in a fixed
//                              order.  The one place that is not fp32: the fp32 partials are added in fp64 (and the counts in int64) and
//                              rounded to fp32 once, so that the numerator does not depend on the number of tiles; still deterministic.
#include "sf_internal.h"
#include "sf_common.h"
#include "sf_launch.h"
#include "sf_handle.h"
#include "sf_vis_axis.h"      // vis_axis, vis_reach: the coordinate arithmetic, shared with sf_seg.hip

#define VIS_THREADS 256
#define VIS_WAVES (VIS_THREADS / 64)
#define VIS_TILE_H 16
#define VIS_TILE_W 256
#define VIS_PX 16                         // pixels of a row per thread
#define VIS_INTER_MAX_WORDS 16384         // row i in 64 KB of LDS
#define VIS_BOX_MAX_BYTES (63 * 1024)     // a tile's source box: what a kernel gets without raising its dynamic-LDS limit, less the static words

// ------------------------------------------------------------------------------------------------
// a. scores
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VIS_THREADS) void sf_vis_scores_kernel(const float* __restrict__ logits, long long rows, int C1, float* __restrict__ max_scores,
                                                                    int32_t* __restrict__ labels, float* __restrict__ scores) {
  const int lane = (int)threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * VIS_WAVES + ((int)threadIdx.x >> 6);
  if (row >= rows) return;                // whole waves leave: the shuffles below see full waves
  const float* x = logits + row * C1;
  float m = -INFINITY;
  for (int c = lane; c < C1; c += 64) m = fmaxf(m, x[c]);
  for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  float s = 0.f;
  for (int c = lane; c < C1; c += 64) s += expf(x[c] - m);
  for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
  const int C = C1 - 1;
  float best = -1.f;
  int arg = 0x7fffffff;
  for (int c = lane; c < C; c += 64) {
    const float p = expf(x[c] - m) / s;
    if (scores) scores[row * C + c] = p;
    if (p > best) { best = p; arg = c; }  // c increases: the first index of a lane's ties stays
  }
  for (int o = 32; o; o >>= 1) {
    const float ob = __shfl_xor(best, o);
    const int oa = __shfl_xor(arg, o);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
  }
  if (lane == 0) { max_scores[row] = best; labels[row] = arg; }
}

// ------------------------------------------------------------------------------------------------
// b. packed masks and areas
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VIS_THREADS) void sf_vis_pack_kernel(const float* __restrict__ masks, int P, int words, int vec, uint32_t* __restrict__ bits,
                                                                  int32_t* __restrict__ area) {
  __shared__ int wave_area[VIS_WAVES];
  const float* x = masks + (size_t)blockIdx.x * P;
  uint32_t* out = bits + (size_t)blockIdx.x * words;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  int count = 0;
  for (int base = 0; base < P; base += 4 * VIS_THREADS) {     // every thread runs every step: the shuffles see full waves
    const int p = base + 4 * tid;
    uint32_t nib = 0;
    if (vec && p + 3 < P) {
      const f32x4_t v = *reinterpret_cast<const f32x4_t*>(x + p);
      nib = (v[0] > 0.f ? 1u : 0u) | (v[1] > 0.f ? 2u : 0u) | (v[2] > 0.f ? 4u : 0u) | (v[3] > 0.f ? 8u : 0u);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (p + j < P && x[p + j] > 0.f) nib |= 1u << j;
    }
    count += __popc(nib);
    uint32_t word = nib << (4 * (lane & 7));
    word |= __shfl_xor(word, 1);
    word |= __shfl_xor(word, 2);
    word |= __shfl_xor(word, 4);
    if ((lane & 7) == 0 && p < P) out[p >> 5] = word;         // p is a multiple of 32 here; pixels past P added no bits
  }
  for (int o = 32; o; o >>= 1) count += __shfl_xor(count, o);
  if (lane == 0) wave_area[tid >> 6] = count;
  __syncthreads();
  if (tid == 0) {
    int a = 0;
    for (int w = 0; w < VIS_WAVES; ++w) a += wave_area[w];
    area[blockIdx.x] = a;
  }
}

// ------------------------------------------------------------------------------------------------
// c. intersections
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VIS_THREADS) void sf_vis_inter_kernel(const uint32_t* __restrict__ bits, int Q, int words, int32_t* __restrict__ inter) {
  extern __shared__ __attribute__((aligned(16))) uint32_t row_i[];
  const int f = (int)blockIdx.y, i = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63;
  const uint32_t* frame = bits + (size_t)f * Q * words;
  for (int w = tid; w < words; w += VIS_THREADS) row_i[w] = frame[(size_t)i * words + w];
  __syncthreads();
  for (int j = tid >> 6; j < Q; j += VIS_WAVES) {
    const uint32_t* rj = frame + (size_t)j * words;
    int n = 0;
    for (int w = lane; w < words; w += 64) n += __popc(row_i[w] & rj[w]);
    for (int o = 32; o; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) inter[((size_t)f * Q + i) * Q + j] = n;
  }
}

// ------------------------------------------------------------------------------------------------
// d. mask post-processing
// ------------------------------------------------------------------------------------------------
struct SfVisPost {
  const float* src; const int32_t* index; uint8_t* masks; float* logits; float* part_num; int32_t* part_den;
  int R, h, w, Hc, Wc, H, W;
  float ry1, rx1, ry2, rx2;               // source pixels per padded pixel; cropped pixels per output pixel
  int lds_floats;
};

__global__ __launch_bounds__(VIS_THREADS) void sf_vis_postprocess_kernel(SfVisPost p) {
  extern __shared__ __attribute__((aligned(16))) float box[];
  __shared__ float wave_num[VIS_WAVES];
  __shared__ int wave_den[VIS_WAVES];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int plane = (int)blockIdx.z;                          // k * F + f
  const int y_first = (int)blockIdx.y * VIS_TILE_H, x_first = (int)blockIdx.x * VIS_TILE_W;
  const int y = y_first + tid / (VIS_TILE_W / VIS_PX), x0 = x_first + (tid % (VIS_TILE_W / VIS_PX)) * VIS_PX;
  const size_t part = ((size_t)plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  const int row = p.index[plane];
  const bool absent = row < 0 || row >= p.R;                  // the same in every thread of the workgroup
  float v[VIS_PX];
#pragma unroll
  for (int j = 0; j < VIS_PX; ++j) v[j] = 0.f;
  float num = 0.f;
  int den = 0;
  if (!absent) {
    int sy_lo, sy_hi, sx_lo, sx_hi;
    const int y_last = min(y_first + VIS_TILE_H, p.H) - 1, x_last = min(x_first + VIS_TILE_W, p.W) - 1;
    vis_reach(y_first, y_last, p.ry2, p.Hc, p.ry1, p.h, &sy_lo, &sy_hi);
    vis_reach(x_first, x_last, p.rx2, p.Wc, p.rx1, p.w, &sx_lo, &sx_hi);
    int bw = sx_hi - sx_lo + 1, bh = sy_hi - sy_lo + 1;
    // Never taken: the entry point sized the LDS with this very function over every tile (vis_axis is one fmaf and exact float
    // operations, so host and device agree bit for bit) and added slack.  Kept so that a mistake there could only give wrong pixels in
    // tests, never an access outside the LDS or the source plane.
    if (bh * bw > p.lds_floats) {
      bw = min(bw, p.lds_floats);
      bh = max(p.lds_floats / bw, 1);
    }
    const float* plane_src = p.src + (size_t)row * p.h * p.w;
    for (int i = tid; i < bh * bw; i += VIS_THREADS) {
      const int r = i / bw, c = i - r * bw;
      box[i] = plane_src[(size_t)(sy_lo + r) * p.w + sx_lo + c];
    }
    __syncthreads();
    if (y < p.H) {
      int Y[2], ya[2][2];
      float ly2, lya[2];
      vis_axis(y, p.ry2, p.Hc, &Y[0], &Y[1], &ly2);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        vis_axis(Y[a], p.ry1, p.h, &ya[a][0], &ya[a][1], &lya[a]);
        ya[a][0] = min(max(ya[a][0] - sy_lo, 0), bh - 1) * bw;
        ya[a][1] = min(max(ya[a][1] - sy_lo, 0), bh - 1) * bw;
      }
#pragma unroll
      for (int j = 0; j < VIS_PX; ++j) {
        const int x = x0 + j;
        if (x >= p.W) break;
        int X[2], xb[2][2];
        float lx2, lxb[2];
        vis_axis(x, p.rx2, p.Wc, &X[0], &X[1], &lx2);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          vis_axis(X[b], p.rx1, p.w, &xb[b][0], &xb[b][1], &lxb[b]);
          xb[b][0] = min(max(xb[b][0] - sx_lo, 0), bw - 1);
          xb[b][1] = min(max(xb[b][1] - sx_lo, 0), bw - 1);
        }
        float mid[2][2];                                      // the four pixels of the cropped intermediate
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const float v00 = box[ya[a][0] + xb[b][0]], v01 = box[ya[a][0] + xb[b][1]];
            const float v10 = box[ya[a][1] + xb[b][0]], v11 = box[ya[a][1] + xb[b][1]];
            mid[a][b] = (1.f - lya[a]) * ((1.f - lxb[b]) * v00 + lxb[b] * v01) + lya[a] * ((1.f - lxb[b]) * v10 + lxb[b] * v11);
          }
        const float o = (1.f - ly2) * ((1.f - lx2) * mid[0][0] + lx2 * mid[0][1]) + ly2 * ((1.f - lx2) * mid[1][0] + lx2 * mid[1][1]);
        v[j] = o;
        if (o > 0.f) { num += 1.f / (1.f + expf(-o)); den += 1; }
      }
    }
  }
  if (y < p.H && x0 < p.W) {
    const size_t at = ((size_t)plane * p.H + y) * p.W + x0;
    if (p.masks) {
      if ((p.W & 15) == 0) {                                  // x0 is a multiple of 16: an aligned 16-byte word of bool bytes
        u32x4_t wd;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          wd[q] = (v[4 * q] > 0.f ? 1u : 0u) | (v[4 * q + 1] > 0.f ? 0x100u : 0u) | (v[4 * q + 2] > 0.f ? 0x10000u : 0u) | (v[4 * q + 3] > 0.f ? 0x1000000u : 0u);
        *reinterpret_cast<u32x4_t*>(p.masks + at) = wd;
      } else {
#pragma unroll
        for (int j = 0; j < VIS_PX; ++j)
          if (x0 + j < p.W) p.masks[at + j] = v[j] > 0.f ? 1 : 0;
      }
    }
    if (p.logits) {
      if ((p.W & 3) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (x0 + 4 * q < p.W) {
            f32x4_t o4 = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
            *reinterpret_cast<f32x4_t*>(p.logits + at + 4 * q) = o4;
          }
      } else {
#pragma unroll
        for (int j = 0; j < VIS_PX; ++j)
          if (x0 + j < p.W) p.logits[at + j] = v[j];
      }
    }
  }
  if (!p.part_num) return;
  for (int o = 32; o; o >>= 1) { num += __shfl_xor(num, o); den += __shfl_xor(den, o); }
  if (lane == 0) { wave_num[tid >> 6] = num; wave_den[tid >> 6] = den; }
  __syncthreads();
  if (tid == 0) {
    float n = 0.f;
    int d = 0;
    for (int w = 0; w < VIS_WAVES; ++w) { n += wave_num[w]; d += wave_den[w]; }
    p.part_num[part] = n;
    p.part_den[part] = d;
  }
}

__global__ __launch_bounds__(VIS_THREADS) void sf_vis_reduce_kernel(const float* __restrict__ part_num, const int32_t* __restrict__ part_den, long long per_instance,
                                                                    float* __restrict__ numerator, long long* __restrict__ denominator) {
  __shared__ double sn[VIS_THREADS];
  __shared__ long long sd[VIS_THREADS];
  const int tid = (int)threadIdx.x;
  const float* pn = part_num + (size_t)blockIdx.x * per_instance;
  const int32_t* pd = part_den + (size_t)blockIdx.x * per_instance;
  double n = 0.0;                          // the partials are fp32; their sum is kept wider so that it does not depend on the tile count
  long long d = 0;
  for (long long i = tid; i < per_instance; i += VIS_THREADS) { n += (double)pn[i]; d += pd[i]; }
  sn[tid] = n;
  sd[tid] = d;
  __syncthreads();
  for (int s = VIS_THREADS / 2; s; s >>= 1) {
    if (tid < s) { sn[tid] += sn[tid + s]; sd[tid] += sd[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) { numerator[blockIdx.x] = (float)sn[0]; denominator[blockIdx.x] = sd[0]; }
}

// ------------------------------------------------------------------------------------------------
// entry points: every refusal happens before anything is launched
// ------------------------------------------------------------------------------------------------
extern "C" int sf_op_vis_scores(const float* logits_dev, long long rows, int classes_plus_one, float* max_scores_dev, int32_t* labels_dev,
                                float* scores_dev, sf_stream stream) {
  const char* who = "sf_op_vis_scores";
  if (!logits_dev || !max_scores_dev || !labels_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (rows < 1 || classes_plus_one < 2) return sf_set_err(SF_ERR_INVALID, "%s: rows = %lld (>= 1), classes + 1 = %d (>= 2: one class and the no-object column)", who, rows, classes_plus_one);
  const long long blocks = (rows + VIS_WAVES - 1) / VIS_WAVES;
  if (blocks > 0x7fffffffLL) return sf_set_err(SF_ERR_CAPACITY, "%s: %lld rows exceed one grid", who, rows);
  HIP_TRY(sf_launch(sf_vis_scores_kernel, dim3((unsigned)blocks), dim3(VIS_THREADS), 0, (hipStream_t)stream, logits_dev, rows, classes_plus_one,
                    max_scores_dev, labels_dev, scores_dev));
  return SF_OK;
}

extern "C" int sf_op_vis_pack_masks(const float* masks_dev, long long rows, int pixels, uint32_t* bits_dev, int32_t* area_dev, sf_stream stream) {
  const char* who = "sf_op_vis_pack_masks";
  if (!masks_dev || !bits_dev || !area_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (rows < 1 || rows > 0x7fffffffLL || pixels < 1 || pixels > 0x7fffffff - 4 * VIS_THREADS) return sf_set_err(SF_ERR_INVALID, "%s: rows = %lld, pixels = %d: both >= 1 and within one grid", who, rows, pixels);
  const int vec = (pixels & 3) == 0 && ((uintptr_t)masks_dev & 15) == 0;
  HIP_TRY(sf_launch(sf_vis_pack_kernel, dim3((unsigned)rows), dim3(VIS_THREADS), 0, (hipStream_t)stream, masks_dev, pixels, (pixels + 31) / 32, vec,
                    bits_dev, area_dev));
  return SF_OK;
}

extern "C" int sf_op_vis_mask_iou(const uint32_t* bits_dev, int F, int Q, int pixels, int32_t* inter_dev, sf_stream stream) {
  const char* who = "sf_op_vis_mask_iou";
  if (!bits_dev || !inter_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (F < 1 || F > 65535 || Q < 1 || pixels < 1) return sf_set_err(SF_ERR_INVALID, "%s: F = %d (1..65535), Q = %d, pixels = %d (>= 1)", who, F, Q, pixels);
  const int words = (pixels + 31) / 32;
  if (words > VIS_INTER_MAX_WORDS) return sf_set_err(SF_ERR_CAPACITY, "%s: %d pixels per mask exceed %d (a row is held in LDS)", who, pixels, 32 * VIS_INTER_MAX_WORDS);
  HIP_TRY(sf_launch(sf_vis_inter_kernel, dim3((unsigned)Q, (unsigned)F), dim3(VIS_THREADS), (size_t)words * 4, (hipStream_t)stream, bits_dev, Q, words, inter_dev));
  return SF_OK;
}

static inline long long vis_tiles(int H, int W) { return (long long)((H + VIS_TILE_H - 1) / VIS_TILE_H) * ((W + VIS_TILE_W - 1) / VIS_TILE_W); }

extern "C" size_t sf_op_vis_postprocess_workspace_bytes(int K, int F, int H, int W) {
  if (K < 1 || F < 1 || H < 1 || W < 1) return 0;
  return (size_t)K * F * vis_tiles(H, W) * 8 + 256;
}

extern "C" int sf_op_vis_postprocess(const float* masks_dev, int R, int h, int w, const int32_t* index_dev, int K, int F, int Hp, int Wp, int Hc, int Wc,
                                     int H, int W, uint8_t* out_masks_dev, float* out_logits_dev, float* numerator_dev, int64_t* denominator_dev,
                                     void* workspace_dev, size_t workspace_bytes, sf_stream stream) {
  const char* who = "sf_op_vis_postprocess";
  if (!masks_dev || !index_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (!out_masks_dev && !out_logits_dev) return sf_set_err(SF_ERR_INVALID, "%s: neither masks nor logits are wanted", who);
  if (!numerator_dev != !denominator_dev) return sf_set_err(SF_ERR_INVALID, "%s: numerator and denominator come together", who);
  if (R < 1 || h < 1 || w < 1 || K < 1 || F < 1 || H < 1 || W < 1) return sf_set_err(SF_ERR_INVALID, "%s: R = %d, h = %d, w = %d, K = %d, F = %d, H = %d, W = %d: all >= 1", who, R, h, w, K, F, H, W);
  if (Hc < 1 || Wc < 1 || Hc > Hp || Wc > Wp) return sf_set_err(SF_ERR_INVALID, "%s: the crop %d x %d must lie inside the padded size %d x %d", who, Hc, Wc, Hp, Wp);
  if ((long long)K * F > 65535) return sf_set_err(SF_ERR_CAPACITY, "%s: K * F = %lld planes exceed one grid (65535)", who, (long long)K * F);
  if ((long long)h * w > 0x7fffffffLL || H > 65535 * VIS_TILE_H) return sf_set_err(SF_ERR_CAPACITY, "%s: a plane exceeds the index range", who);
  if (((uintptr_t)out_masks_dev | (uintptr_t)out_logits_dev) & 15) return sf_set_err(SF_ERR_INVALID, "%s: outputs must be 16-byte aligned", who);
  SfVisPost p;
  p.src = masks_dev; p.index = index_dev; p.masks = out_masks_dev; p.logits = out_logits_dev; p.part_num = nullptr; p.part_den = nullptr;
  p.R = R; p.h = h; p.w = w; p.Hc = Hc; p.Wc = Wc; p.H = H; p.W = W;
  p.ry1 = (float)h / (float)Hp; p.rx1 = (float)w / (float)Wp; p.ry2 = (float)Hc / (float)H; p.rx2 = (float)Wc / (float)W;
  const int ty = (H + VIS_TILE_H - 1) / VIS_TILE_H, tx = (W + VIS_TILE_W - 1) / VIS_TILE_W;
  const long long per_instance = (long long)F * ty * tx;
  if (numerator_dev) {
    SF_TRY(sf_check_workspace(who, "sf_op_vis_postprocess_workspace_bytes", workspace_dev, workspace_bytes, sf_op_vis_postprocess_workspace_bytes(K, F, H, W)));
    p.part_num = (float*)workspace_dev;
    p.part_den = (int32_t*)workspace_dev + (size_t)K * per_instance;
  }
  // the largest source box of any tile, from the kernel's own index rule (bit-identical on host and device), plus two pixels of slack
  // per axis
  int bh = 1, bw = 1, lo, hi;
  for (int t = 0; t < ty; ++t) {
    vis_reach(t * VIS_TILE_H, (t + 1) * VIS_TILE_H < H ? (t + 1) * VIS_TILE_H - 1 : H - 1, p.ry2, Hc, p.ry1, h, &lo, &hi);
    bh = hi - lo + 1 > bh ? hi - lo + 1 : bh;
  }
  for (int t = 0; t < tx; ++t) {
    vis_reach(t * VIS_TILE_W, (t + 1) * VIS_TILE_W < W ? (t + 1) * VIS_TILE_W - 1 : W - 1, p.rx2, Wc, p.rx1, w, &lo, &hi);
    bw = hi - lo + 1 > bw ? hi - lo + 1 : bw;
  }
  bh = bh + 2 < h ? bh + 2 : h;
  bw = bw + 2 < w ? bw + 2 : w;
  const size_t lds = (size_t)bh * bw * 4;
  if (lds > VIS_BOX_MAX_BYTES) return sf_set_err(SF_ERR_CAPACITY, "%s: a %d x %d output tile reaches %d x %d source pixels, more than the LDS holds (the output is too small for the masks)", who, VIS_TILE_H, VIS_TILE_W, bh, bw);
  p.lds_floats = bh * bw;
  const dim3 grid((unsigned)tx, (unsigned)ty, (unsigned)(K * F));
  HIP_TRY(sf_launch(sf_vis_postprocess_kernel, grid, dim3(VIS_THREADS), lds, (hipStream_t)stream, p));
  if (numerator_dev)
    HIP_TRY(sf_launch(sf_vis_reduce_kernel, dim3((unsigned)K), dim3(VIS_THREADS), 0, (hipStream_t)stream, (const float*)p.part_num, (const int32_t*)p.part_den,
                      per_instance, numerator_dev, (long long*)denominator_dev));
  return SF_OK;
}
