// Mask logits for training (streamformer_amd/mask_decoder.py, the trainable decoders): every prediction head's
//     logits[f, q, p] = sum_c me[f, q, c] feat[f, c, p]                     me [F, Q, Dm], feat [F, Dm, P], P = H W
// at full mask-feature resolution, and its two gradients
//     d_me[f, q, c] = sum_p d_logits[f, q, p] feat[f, c, p]                 d_feat[f, c, p] = sum_q me[f, q, c] d_logits[f, q, p].
// All fp32 with exact products (v_mfma_f32_16x16x4_f32), every output element has one owner and one summation order, no atomics.
// A workgroup is 256 threads = 4 waves on one 64-pixel tile of one frame; the grid is F x pixel tiles (spans of them in the backward),
// whatever Q is.  The MFMA sums over its k index, so operand pairs may take k in any order as long as both take the same: a lane reads
// 16 bytes (four consecutive c of me, four consecutive pixels of feat) and feeds them to four MFMAs in a row.  The pixel side is
// always the M side of a tile whose result goes to pixels, so a lane ends with four consecutive pixels: 16-byte stores.
//
//   sf_masklogits_fwd_kernel   feat is staged through LDS in chunks of 64 c ([64][68] floats, 17 KB; rows of 64 pixels, 16-byte loads
//                              along p when P % 4 == 0, else scalar).  Wave w owns pixels 16 w .. 16 w + 15 and up to 8 query tiles at a
//                              time (32 accumulator registers; 128 queries a pass, further passes restage).  Per 16 c: four LDS reads of
//                              feat, one 16-byte global read of me per query tile, 4 MFMAs per query tile.
//   sf_masklogits_bwd_kernel   a workgroup owns a SPAN of consecutive pixel tiles of one frame.  Per tile the d_logits tile of up to 128
//                              queries is staged ONCE in LDS ([128][68] floats, 34 KB) and used for both products:
//                                d_feat: wave w owns pixels 16 w .. + 15 and 256 c (16 accumulators; c = 64 T + 4 l + s of lane l, so me is
//                                        read 16 bytes along c), k runs over the queries, d_logits from LDS;
//                                d_me:   wave w owns c 64 w .. 64 w + 63 of the 256 and all 128 queries (32 accumulators = 128 registers
//                                        that live across the span), k runs over the tile's 64 pixels in four chains of 16 that meet as
//                                        a tree, feat 16 bytes along p from global, d_logits 16 bytes along p from LDS.
//                              At the end of the span the d_me partial goes to the workspace [F, spans, Q, Dm].  Dm above 256 and Q above
//                              128 are further passes over the span (d_feat of a later query chunk is added by the element's own thread).
//   sf_masklogits_reduce_kernel  d_me[f, q, c] = the spans' partials in ascending span order.
#include "sf_handle.h"

typedef __attribute__((ext_vector_type(4))) float ml4_t;

#define MLG_PT 64              // pixels of a tile
#define MLG_LD 68              // LDS row pitch: rows 4 g apart land 16 banks apart
#define MLG_KC 64              // c of a staged feat chunk (forward)
#define MLG_QB 8               // query tiles a wave holds (forward)
#define MLG_QC 128             // queries of a staged d_logits chunk (backward)
#define MLG_CB 256             // c of a backward pass
#define MLG_MAX_DM 1024
#define MLG_MAX_SPAN 64
#define MLG_TARGET_WGS 512

struct SfMlg {
  const float* me;             // [F, Q, Dm]
  const float* feat;           // [F, Dm, P]
  const float* dl;             // [F, Q, P]  (backward)
  float* logits;               // [F, Q, P]  (forward)
  float* d_me_part;            // [F, spans, Q, Dm] or null
  float* d_feat;               // [F, Dm, P] or null
  int F, Q, Dm, P, span, spans, accumulate;
};

SF_DEVICE ml4_t ml_mfma(float a, float b, ml4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// four consecutive floats of a row of n, from index i (a multiple of 4); past the end: zeros.  VEC: n % 4 == 0 and the row is 16-byte aligned
template <bool VEC>
SF_DEVICE ml4_t ml_load4(const float* row, int i, int n) {
  ml4_t v = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {
    if (i < n) v = *reinterpret_cast<const ml4_t*>(row + i);
  } else {
    if (i < n) v[0] = row[i];
    if (i + 1 < n) v[1] = row[i + 1];
    if (i + 2 < n) v[2] = row[i + 2];
    if (i + 3 < n) v[3] = row[i + 3];
  }
  return v;
}

template <bool VEC>
SF_DEVICE void ml_store4(float* row, int i, int n, ml4_t v, bool add) {
  if (VEC) {
    if (i < n) {
      ml4_t* d = reinterpret_cast<ml4_t*>(row + i);
      *d = add ? *d + v : v;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (i + r < n) row[i + r] = add ? row[i + r] + v[r] : v[r];
  }
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void sf_masklogits_fwd_kernel(SfMlg p) {
  __shared__ __attribute__((aligned(16))) float fs[MLG_KC * MLG_LD];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  const int f = (int)blockIdx.y, p0 = (int)blockIdx.x * MLG_PT, Q = p.Q, Dm = p.Dm, P = p.P;
  const int qtiles = (Q + 15) >> 4;
  const float* feat = p.feat + (size_t)f * Dm * P;
  const float* me = p.me + (size_t)f * Q * Dm;
  for (int qb = 0; qb < qtiles; qb += MLG_QB) {
    ml4_t acc[MLG_QB];
#pragma unroll
    for (int t = 0; t < MLG_QB; ++t) acc[t] = (ml4_t){0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < Dm; c0 += MLG_KC) {
      __syncthreads();                                   // the previous chunk has been read
      for (int i = (int)threadIdx.x; i < MLG_KC * (MLG_PT / 4); i += 256) {
        const int row = i >> 4, col = (i & 15) * 4;
        ml4_t v = {0.f, 0.f, 0.f, 0.f};
        if (c0 + row < Dm) v = ml_load4<VEC>(feat + (size_t)(c0 + row) * P, p0 + col, P);
        *reinterpret_cast<ml4_t*>(fs + row * MLG_LD + col) = v;
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < MLG_KC / 16; ++j) {
        const int c = c0 + 16 * j + 4 * g;               // k index (g, r) of step j is channel c + r on both sides
        if (c0 + 16 * j >= Dm) break;
        float a[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = fs[(16 * j + 4 * g + r) * MLG_LD + 16 * wave + l15];
#pragma unroll
        for (int t = 0; t < MLG_QB; ++t) {
          if (qb + t < qtiles) {
            const int q = (qb + t) * 16 + l15;
            const ml4_t b = c < Dm ? *reinterpret_cast<const ml4_t*>(me + (size_t)(q < Q ? q : Q - 1) * Dm + c) : (ml4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t] = ml_mfma(a[r], b[r], acc[t]);
          }
        }
      }
    }
    // lane (query l15 of its tile, g) holds pixels p0 + 16 wave + 4 g .. + 3
#pragma unroll
    for (int t = 0; t < MLG_QB; ++t) {
      const int q = (qb + t) * 16 + l15;
      if (qb + t < qtiles && q < Q) ml_store4<VEC>(p.logits + ((size_t)f * Q + q) * P, p0 + 16 * wave + 4 * g, P, acc[t], false);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void sf_masklogits_bwd_kernel(SfMlg p) {
  __shared__ __attribute__((aligned(16))) float ds[MLG_QC * MLG_LD];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
  const int f = (int)blockIdx.y, sp = (int)blockIdx.x, Q = p.Q, Dm = p.Dm, P = p.P;
  const int tiles = (P + MLG_PT - 1) / MLG_PT;
  const int t_begin = sp * p.span, t_end = t_begin + p.span < tiles ? t_begin + p.span : tiles;
  const float* feat = p.feat + (size_t)f * Dm * P;
  const float* me = p.me + (size_t)f * Q * Dm;
  const float* dl = p.dl + (size_t)f * Q * P;
  float* d_feat = p.d_feat ? p.d_feat + (size_t)f * Dm * P : nullptr;
  float* part = p.d_me_part ? p.d_me_part + ((size_t)f * p.spans + sp) * Q * Dm : nullptr;
  for (int cb = 0; cb < Dm; cb += MLG_CB) {
    for (int qc = 0; qc < Q; qc += MLG_QC) {
      const int qn = Q - qc < MLG_QC ? Q - qc : MLG_QC;      // queries of this chunk
      const int qt = (qn + 15) >> 4;                         // their 16-query tiles
      ml4_t am[4][MLG_QC / 16];                              // d_me: [c tile of the wave's 64][query tile]
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int u = 0; u < MLG_QC / 16; ++u) am[t][u] = (ml4_t){0.f, 0.f, 0.f, 0.f};
      for (int tile = t_begin; tile < t_end; ++tile) {
        const int p0 = tile * MLG_PT;
        __syncthreads();                                 // the previous tile has been read
        for (int i = (int)threadIdx.x; i < qt * 16 * (MLG_PT / 4); i += 256) {
          const int row = i >> 4, col = (i & 15) * 4;
          ml4_t v = {0.f, 0.f, 0.f, 0.f};
          if (row < qn) v = ml_load4<VEC>(dl + (size_t)(qc + row) * P, p0 + col, P);
          *reinterpret_cast<ml4_t*>(ds + row * MLG_LD + col) = v;
        }
        __syncthreads();
        if (d_feat) {
          // tile [pixel 16 wave + ..][c]: A = d_logits (LDS), B = me; k index (g, r) of step jj is query 16 jj + 4 g + r.
          // Accumulator (T, s) is c = cb + 64 T + 4 l15 + s: the lane reads me 16 bytes along c.
          ml4_t af[4][4];
#pragma unroll
          for (int T = 0; T < 4; ++T)
#pragma unroll
            for (int s = 0; s < 4; ++s) af[T][s] = (ml4_t){0.f, 0.f, 0.f, 0.f};
          for (int jj = 0; jj < qt; ++jj) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int ql = 16 * jj + 4 * g + r;        // rows at or past qn are staged as zeros; their me row is clamped
              const float a = ds[ql * MLG_LD + 16 * wave + l15];
              const float* mrow = me + (size_t)(ql < qn ? qc + ql : Q - 1) * Dm;
#pragma unroll
              for (int T = 0; T < 4; ++T) {
                const int c = cb + 64 * T + 4 * l15;
                if (cb + 64 * T < Dm) {
                  const ml4_t b = c < Dm ? *reinterpret_cast<const ml4_t*>(mrow + c) : (ml4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                  for (int s = 0; s < 4; ++s) af[T][s] = ml_mfma(a, b[s], af[T][s]);
                }
              }
            }
          }
          const bool add = p.accumulate || qc > 0;       // a later query chunk adds to what this thread stored for the earlier one
#pragma unroll
          for (int T = 0; T < 4; ++T)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
              const int c = cb + 64 * T + 4 * l15 + s;
              if (c < Dm) ml_store4<VEC>(d_feat + (size_t)c * P, p0 + 16 * wave + 4 * g, P, af[T][s], add);
            }
        }
        if (part) {
          // tile [c][query]: A = feat (global, 16 bytes along p), B = d_logits (LDS, 16 bytes along p); k index (g, r) of step j is
          // pixel 16 j + 4 g + r.  The tile's 64 pixels are summed in four chains of 16 (one per j) that meet as a tree, and the
          // tile's sum is added to the span's: short chains, and four independent MFMA chains in flight.
          ml4_t a[MLG_PT / 16][4];
#pragma unroll
          for (int j = 0; j < MLG_PT / 16; ++j)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const int c = cb + 64 * wave + 16 * t + l15;
              a[j][t] = c < Dm ? ml_load4<VEC>(feat + (size_t)c * P, p0 + 16 * j + 4 * g, P) : (ml4_t){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
          for (int u = 0; u < MLG_QC / 16; ++u) {
            if (u < qt) {
              ml4_t b[MLG_PT / 16];
#pragma unroll
              for (int j = 0; j < MLG_PT / 16; ++j) b[j] = *reinterpret_cast<const ml4_t*>(ds + (16 * u + l15) * MLG_LD + 16 * j + 4 * g);
#pragma unroll
              for (int t = 0; t < 4; ++t) {
                ml4_t ch[MLG_PT / 16];
#pragma unroll
                for (int j = 0; j < MLG_PT / 16; ++j) ch[j] = (ml4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                  for (int j = 0; j < MLG_PT / 16; ++j) ch[j] = ml_mfma(a[j][t][r], b[j][r], ch[j]);
                am[t][u] += (ch[0] + ch[1]) + (ch[2] + ch[3]);
              }
            }
          }
        }
      }
      if (part) {                                        // lane (query l15 of tile u, g) holds c = cb + 64 wave + 16 t + 4 g .. + 3
#pragma unroll
        for (int u = 0; u < MLG_QC / 16; ++u) {
          const int ql = 16 * u + l15;
          if (u < qt && ql < qn) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              const int c = cb + 64 * wave + 16 * t + 4 * g;
              if (c < Dm) *reinterpret_cast<ml4_t*>(part + (size_t)(qc + ql) * Dm + c) = am[t][u];
            }
          }
        }
      }
    }
  }
}

// d_me[f, q, c] = sum over the spans in ascending order; n4 = Q * Dm / 4 float4 per (frame, span)
__global__ __launch_bounds__(256) void sf_masklogits_reduce_kernel(const ml4_t* __restrict__ part, ml4_t* __restrict__ out, int spans, size_t n4, size_t total4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t f = i / n4, e = i - f * n4;
    const ml4_t* src = part + f * spans * n4 + e;
    ml4_t v = src[0];
    for (int s = 1; s < spans; ++s) v += src[(size_t)s * n4];
    out[i] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// entries
// ------------------------------------------------------------------------------------------------
static int mlg_span(int F, int P) {                      // pixel tiles per backward workgroup: a function of the shape alone
  const long long tiles = (P + MLG_PT - 1) / MLG_PT;
  long long span = (long long)F * tiles / MLG_TARGET_WGS;
  if (span < 1) span = 1;
  if (span > MLG_MAX_SPAN) span = MLG_MAX_SPAN;
  return (int)span;
}

static int mlg_check_shape(const char* who, int F, int Q, int Dm, int P) {
  if (F < 1 || F > 65535 || Q < 1 || Q > 65535 || P < 1 || P > (1 << 24))
    return sf_set_err(SF_ERR_INVALID, "%s: bad shape F=%d (1..65535) Q=%d (1..65535) P=%d (1..%d)", who, F, Q, P, 1 << 24);
  if (Dm < 4 || Dm % 4 || Dm > MLG_MAX_DM) return sf_set_err(SF_ERR_INVALID, "%s: mask_dim = %d must be a multiple of 4 up to %d", who, Dm, MLG_MAX_DM);
  if ((long long)F * std::max(Q, Dm) * P > 0x7fffffffLL || (long long)F * Q * Dm > 0x7fffffffLL)
    return sf_set_err(SF_ERR_CAPACITY, "%s: more than 2^31 - 1 elements", who);
  return SF_OK;
}

extern "C" int sf_op_masklogits_forward(const float* mask_embed_dev, const float* mask_features_dev, float* logits_dev, int F, int Q, int mask_dim, int P,
                                        sf_stream stream) {
  const char* who = "sf_op_masklogits_forward";
  if (!mask_embed_dev || !mask_features_dev || !logits_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  SF_TRY(mlg_check_shape(who, F, Q, mask_dim, P));
  if (((uintptr_t)mask_embed_dev | (uintptr_t)mask_features_dev | (uintptr_t)logits_dev) & 15)
    return sf_set_err(SF_ERR_INVALID, "%s: buffers must be 16-byte aligned", who);
  SfMlg a;
  memset(&a, 0, sizeof(a));
  a.me = mask_embed_dev; a.feat = mask_features_dev; a.logits = logits_dev; a.F = F; a.Q = Q; a.Dm = mask_dim; a.P = P;
  const dim3 grid((unsigned)((P + MLG_PT - 1) / MLG_PT), (unsigned)F);
  if (P % 4 == 0) HIP_TRY(sf_launch(sf_masklogits_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a));
  else HIP_TRY(sf_launch(sf_masklogits_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a));
  return SF_OK;
}

extern "C" size_t sf_op_masklogits_backward_workspace_bytes(int F, int Q, int mask_dim, int P) {
  if (F < 1 || Q < 1 || mask_dim < 1 || P < 1) return 0;
  const int span = mlg_span(F, P), tiles = (P + MLG_PT - 1) / MLG_PT, spans = (tiles + span - 1) / span;
  return ((size_t)F * spans * Q * mask_dim * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" int sf_op_masklogits_backward(const float* d_logits_dev, const float* mask_embed_dev, const float* mask_features_dev, float* d_mask_embed_dev,
                                         float* d_mask_features_dev, int accumulate, int F, int Q, int mask_dim, int P, void* workspace_dev,
                                         size_t workspace_bytes, sf_stream stream) {
  const char* who = "sf_op_masklogits_backward";
  if (!d_logits_dev || !mask_embed_dev || !mask_features_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (!d_mask_embed_dev && !d_mask_features_dev) return sf_set_err(SF_ERR_INVALID, "%s: no output", who);
  SF_TRY(mlg_check_shape(who, F, Q, mask_dim, P));
  if (((uintptr_t)d_logits_dev | (uintptr_t)mask_embed_dev | (uintptr_t)mask_features_dev | (uintptr_t)d_mask_embed_dev | (uintptr_t)d_mask_features_dev |
       (uintptr_t)workspace_dev) & 15)
    return sf_set_err(SF_ERR_INVALID, "%s: buffers must be 16-byte aligned", who);
  if (d_mask_embed_dev) {
    if (!workspace_dev) return sf_set_err(SF_ERR_INVALID, "%s: the partial sums of d_mask_embed need the workspace", who);
    SF_TRY(sf_check_workspace(who, "sf_op_masklogits_backward_workspace_bytes", workspace_dev, workspace_bytes,
                              sf_op_masklogits_backward_workspace_bytes(F, Q, mask_dim, P)));
  }
  hipStream_t s = (hipStream_t)stream;
  SfMlg a;
  memset(&a, 0, sizeof(a));
  a.me = mask_embed_dev; a.feat = mask_features_dev; a.dl = d_logits_dev; a.d_feat = d_mask_features_dev;
  a.d_me_part = d_mask_embed_dev ? (float*)workspace_dev : nullptr;
  a.F = F; a.Q = Q; a.Dm = mask_dim; a.P = P; a.accumulate = accumulate ? 1 : 0;
  const int tiles = (P + MLG_PT - 1) / MLG_PT;
  a.span = mlg_span(F, P);
  a.spans = (tiles + a.span - 1) / a.span;
  const dim3 grid((unsigned)a.spans, (unsigned)F);
  if (P % 4 == 0) HIP_TRY(sf_launch(sf_masklogits_bwd_kernel<true>, grid, dim3(256), 0, s, a));
  else HIP_TRY(sf_launch(sf_masklogits_bwd_kernel<false>, grid, dim3(256), 0, s, a));
  if (d_mask_embed_dev) {
    const size_t n4 = (size_t)Q * mask_dim / 4, total4 = n4 * F;
    size_t blocks = (total4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    HIP_TRY(sf_launch(sf_masklogits_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const ml4_t*)workspace_dev, (ml4_t*)d_mask_embed_dev,
                      a.spans, n4, total4));
  }
  return SF_OK;
}
