// Caption-driven heads: the C entry of the temporal grounding loss (kernel in sf_loss.hip) and the evaluation output of the
// referring segmentation head (TimesformerVideoContrastiveCrossEntropySegmentationHead.forward, eval branch, reference
// modeling:2004-2018): dense caption-to-patch logits
//   out[m, j] = exp(logit_scale) * <x[m] / |x[m]|, text[j] / |text[j]|> + logit_bias        x [M, D], text [n, D], fp32 throughout
// sf_dense_text_logits_kernel is built as a streaming kernel (M D 4 bytes in, M n 4 out; 77 MB + 0.8 MB at 25 088 x 768 x 8): one wave owns a row,
// holds it in registers (one float4 per 256 features per lane, loaded once), and takes the row's norm and its n dot products from
// those registers against the NORMALISED captions in LDS (ds_read_b128, lane-contiguous: conflict-free).  The next row's loads are
// issued before the current row's arithmetic, so each wave keeps two rows in flight.  A table that does not fit the LDS budget
// (n D' 4 > 128 KB, D' = D rounded up to 256) is walked in equal chunks, and ALL of x is read again for every chunk (from the
// Infinity Cache where it fits): up to 42 captions at D = 768 are one pass, 43..64 are two.  The grid is two workgroups per CU, but
// they are co-resident only while two LDS images fit a CU's 160 KB: up to 26 captions at D = 768 (3 KB each); above that one
// workgroup (8 waves) runs per CU at a time and the latency hiding halves.  The case it is laid out for is the small table
// (n = 8: 24 KB); the large ones are functional.  Its time against the torch sequence is not measured yet (tools/text_heads_bench.py).  Every output element has one owner and a fixed summation order: bit-reproducible.
#include "sf_common.h"
#include "sf_internal.h"

#define SF_TL_THREADS 512
#define SF_TL_WAVES (SF_TL_THREADS / 64)
#define SF_TL_MAXN 64
#define SF_TL_MAXKV 8                          // float4 slots per lane: D <= 8 * 256
#define SF_TL_LDS_BYTES (128 * 1024)

template <int KV>
SF_DEVICE void tl_load_row(const float* __restrict__ x, size_t row, int D, int lane, float4 (&r)[KV]) {
  const float4* p = (const float4*)(x + row * (size_t)D);
#pragma unroll
  for (int k = 0; k < KV; ++k) {
    const int q = k * 64 + lane;                // float4 index inside the row
    r[k] = (q * 4 < D) ? p[q] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// grid: persistent workgroups of 8 waves; wave w of workgroup g takes rows g * 8 + w, + gridDim.x * 8, ...
// dynamic LDS: [chunk][KV * 256] normalised captions (zero-padded past D)
template <int KV>
__global__ __launch_bounds__(SF_TL_THREADS) void sf_dense_text_logits_kernel(const float* __restrict__ x,
                                                                            const float* __restrict__ text, int M, int D, int n,
                                                                            int chunk, const float* __restrict__ logit_scale_p,
                                                                            const float* __restrict__ logit_bias_p,
                                                                            float* __restrict__ out) {
  extern __shared__ float4 tl_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float s = expf(logit_scale_p[0]), bias = logit_bias_p[0];
  const int stride = gridDim.x * SF_TL_WAVES;
  for (int j0 = 0; j0 < n; j0 += chunk) {
    const int nj = min(chunk, n - j0);
    __syncthreads();                            // the previous chunk's readers are done
    for (int j = wave; j < nj; j += SF_TL_WAVES) {
      const float* t = text + (size_t)(j0 + j) * D;
      float tv[KV * 4];
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < KV; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int d = (k * 64 + lane) * 4 + c;
          tv[k * 4 + c] = d < D ? t[d] : 0.f;
          a = fmaf(tv[k * 4 + c], tv[k * 4 + c], a);
        }
      const float inv = 1.f / sqrtf(wave_sum_dpp(a));
#pragma unroll
      for (int k = 0; k < KV; ++k)
        tl_lds[(j * KV + k) * 64 + lane] = make_float4(tv[k * 4] * inv, tv[k * 4 + 1] * inv, tv[k * 4 + 2] * inv, tv[k * 4 + 3] * inv);
    }
    __syncthreads();
    int row = blockIdx.x * SF_TL_WAVES + wave;
    float4 cur[KV], nxt[KV];
    if (row < M) tl_load_row<KV>(x, (size_t)row, D, lane, cur);
    for (; row < M; row += stride) {
      const int next = row + stride;
      if (next < M) tl_load_row<KV>(x, (size_t)next, D, lane, nxt);
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < KV; ++k) {
        a = fmaf(cur[k].x, cur[k].x, a); a = fmaf(cur[k].y, cur[k].y, a);
        a = fmaf(cur[k].z, cur[k].z, a); a = fmaf(cur[k].w, cur[k].w, a);
      }
      const float f = s / sqrtf(wave_sum_dpp(a));
      float mine = 0.f;
      for (int j = 0; j < nj; ++j) {
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < KV; ++k) {
          const float4 e = tl_lds[(j * KV + k) * 64 + lane];
          dot = fmaf(cur[k].x, e.x, dot); dot = fmaf(cur[k].y, e.y, dot);
          dot = fmaf(cur[k].z, e.z, dot); dot = fmaf(cur[k].w, e.w, dot);
        }
        dot = wave_sum_dpp(dot);
        if (lane == j) mine = fmaf(f, dot, bias);
      }
      if (lane < nj) out[(size_t)row * n + j0 + lane] = mine;     // one coalesced store per row
#pragma unroll
      for (int k = 0; k < KV; ++k) cur[k] = nxt[k];
    }
  }
}

template <int KV>
static int tl_launch(const float* x, const float* text, int M, int D, int n, int chunk, const float* ls, const float* lb, float* out,
                     hipStream_t s) {
  const size_t lds = (size_t)chunk * KV * 64 * sizeof(float4);
  int grid = (M + SF_TL_WAVES - 1) / SF_TL_WAVES;
  if (grid > 512) grid = 512;                   // two workgroups per CU; co-resident (16 waves, two rows each in flight) while 2 x lds <= 160 KB
  HIP_TRY(sf_launch_big_lds(sf_dense_text_logits_kernel<KV>, dim3(grid), dim3(SF_TL_THREADS), lds, s, x, text, M, D, n, chunk, ls, lb, out));
  return SF_OK;
}

extern "C" int sf_dense_text_logits(const float* x, const float* text, int M, int D, int n, const float* logit_scale,
                                    const float* logit_bias, float* out, sf_stream stream) {
  if (!x || !text || !logit_scale || !logit_bias || !out) return sf_set_err(SF_ERR_INVALID, "sf_dense_text_logits: null buffer");
  if (M <= 0 || D <= 0 || n <= 0) return sf_set_err(SF_ERR_INVALID, "sf_dense_text_logits: bad shape M=%d D=%d n=%d", M, D, n);
  if (n > SF_TL_MAXN) return sf_set_err(SF_ERR_CAPACITY, "sf_dense_text_logits: %d captions > %d (one lane per caption of a row)", n, SF_TL_MAXN);
  if (D % 4 != 0) return sf_set_err(SF_ERR_INVALID, "sf_dense_text_logits: feature width %d is not a multiple of 4 (16-byte row loads)", D);
  if (D > SF_TL_MAXKV * 256) return sf_set_err(SF_ERR_CAPACITY, "sf_dense_text_logits: feature width %d > %d (a row lives in one wave's registers)", D, SF_TL_MAXKV * 256);
  if (((uintptr_t)x & 15) != 0) return sf_set_err(SF_ERR_INVALID, "sf_dense_text_logits: x is not 16-byte aligned");
  if ((size_t)M * (size_t)n > (size_t)0x7fffffff) return sf_set_err(SF_ERR_CAPACITY, "sf_dense_text_logits: M * n = %zu outputs > 2^31 - 1", (size_t)M * (size_t)n);
  const int KV = (D + 255) / 256;
  const int cap = SF_TL_LDS_BYTES / (KV * 1024);               // captions per LDS image: >= 16
  const int passes = (n + cap - 1) / cap;
  const int chunk = (n + passes - 1) / passes;
  hipStream_t s = (hipStream_t)stream;
  switch (KV) {
    case 1: return tl_launch<1>(x, text, M, D, n, chunk, logit_scale, logit_bias, out, s);
    case 2: return tl_launch<2>(x, text, M, D, n, chunk, logit_scale, logit_bias, out, s);
    case 3: return tl_launch<3>(x, text, M, D, n, chunk, logit_scale, logit_bias, out, s);
    case 4: return tl_launch<4>(x, text, M, D, n, chunk, logit_scale, logit_bias, out, s);
    case 5: return tl_launch<5>(x, text, M, D, n, chunk, logit_scale, logit_bias, out, s);
    case 6: return tl_launch<6>(x, text, M, D, n, chunk, logit_scale, logit_bias, out, s);
    case 7: return tl_launch<7>(x, text, M, D, n, chunk, logit_scale, logit_bias, out, s);
    default: return tl_launch<8>(x, text, M, D, n, chunk, logit_scale, logit_bias, out, s);
  }
}

extern "C" int sf_grounding_loss(const float* pooler, const float* text, const float* labels, int B, int T, int D,
                                 const float* logit_scale, const float* logit_bias, float* loss, float* grad_pooler,
                                 float* grad_scalars, float* logits_out, void* workspace, size_t workspace_bytes, sf_stream stream) {
  if (!pooler || !text || !labels || !loss || !logit_scale || !logit_bias || !workspace) return sf_set_err(SF_ERR_INVALID, "sf_grounding_loss: null buffer");
  if (B <= 0 || T <= 0 || D <= 0) return sf_set_err(SF_ERR_INVALID, "sf_grounding_loss: bad shape B=%d T=%d D=%d", B, T, D);
  if ((size_t)B * (size_t)T > (size_t)(1 << 24)) return sf_set_err(SF_ERR_CAPACITY, "sf_grounding_loss: %zu frame rows > 2^24", (size_t)B * (size_t)T);
  if (workspace_bytes < sf_loss_partial_bytes(B * T))
    return sf_set_err(SF_ERR_WORKSPACE, "sf_grounding_loss: workspace %zu < %zu bytes (sf_loss_workspace_bytes)", workspace_bytes, sf_loss_partial_bytes(B * T));
  HIP_TRY(sf_launch_grounding_loss(pooler, text, labels, B, T, D, logit_scale, logit_bias, loss, grad_pooler, grad_scalars, logits_out,
                                   (float*)workspace, (hipStream_t)stream));
  return SF_OK;
}
