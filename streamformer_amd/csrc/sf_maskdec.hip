// Mask2Former masked-attention decoder (the reference's MultiScaleMaskedTransformerDecoder and its CTVIS subclass
// CLMultiScaleMaskedTransformerDecoder, downstream/OVIS/mask2former/modeling/transformer_decoder/mask2former_transformer_decoder.py and
// downstream/OVIS/ctvis/modeling/transformer_decoder/cl_mask2former_transformer_decoder.py): three multi-scale features + mask_features ->
// per-frame class logits, masks and (CL) queries, re-identification embeddings and boxes.  Inference only, post-norm.  Frames are the
// batch everywhere: rows are [F, Q, C] and [F, HW, C]; the reference's [Q, B, C] order never exists.  Every Linear runs on the encoder's
// GEMM launchers (sf_launch_gemm, both compute modes, weights rounded / split ONCE at finalize), the row passes on sf_row_kernel; this
// file adds the kernels those do not cover, the launch sequence and the C entry points.
//
//   (sf_maskattn.hip)             sf_maskdec_attention_kernel through mka_launch_forward (sf_maskattn.h): ctx[f, q, h, :] =
//                                 softmax_j(scale Q . (K_j + kpos_j) | mask[f, q, j]) V_j in fp32, the mask bit-packed [F, Q, ceil(HW / 32)]
//                                 (bit set = key hidden) and shared by the heads; a null mask is the unmasked Q x Q self-attention.
//                                 Workgroup shape, skip rule and the training path are described there.
//   sf_maskdec_interp_kernel      mask_features [F, Dm, H, W] -> [F, Dm, h w] by F.interpolate(bilinear, align_corners=False)'s rule.
//                                 Interpolation is linear, so the FEATURES are resampled once per level and call, and every layer of the
//                                 level thresholds mask_embed . resampled features: the [F, Q, H, W] logits of an intermediate layer are
//                                 never formed.
//   sf_maskdec_mask_kernel        logits[f, q, p] = mask_embed[f, q, :] . feat[f, :, p] in fp32 (four interleaved chains over the channels,
//                                 summed as a tree).  One workgroup per (16 queries, frame); its four waves take 64-pixel chunks in turn.
//                                 Either the packed attention mask (bit = logit < 0, one ballot per query and chunk; then the reference's
//                                 rule, a row with every bit set is cleared, decided across the waves in LDS) or the fp32 logits
//                                 (pred_masks, and the aux outputs), never both in one launch.
//   sf_maskdec_box_kernel         BitMasks(mask > 0).get_bounding_boxes() / (w, h, w, h): one wave per (frame, query) over the final masks.
//   sf_maskdec_cut_kernel         [rows, Cp] (class columns padded for the GEMM) -> [rows, classes + 1].
//   (sf_rowwise.hip)              sf_row_kernel through mkd_row: query_feat replicated over the frames, every post-LN residual row,
//                                 decoder_norm; its q planes (y + query_embed[row % Q]) are the operand of the next q (| k) projection.
//
// Decomposition of the cross-attention keys (the one of sf_oad's stage 0): K = W_k (src + pos) + b_k = W_k src + (W_k pos + b_k).  The
// second term depends on the level's shape only: the sine table (sf_op_pixdec_pos_ref's arithmetic) goes through each layer's k
// projection once per call into the workspace, and the kernel adds it while it stages a key.  level_embed is folded into the bias of
// input_proj; without an input projection it is folded into that table and into the v bias (W_v level_embed + b_v), so src is never
// rewritten.  Self-attention runs on the same kernel with a null mask: sf_op_oad_attention caps a call at SF_OAD_MAX_CALL_STREAMS
// streams and puts one wave on a tile, which at F = 128 would mean chunked launches of a quarter of the waves.
#include "sf_handle.h"
#include "sf_nchw_tile.h"

typedef __attribute__((ext_vector_type(4))) float mf4_t;

#define MKD_LEVELS 3
#define MKD_LN_EPS 1e-5f
#define MKD_WAVES 4
#define MKD_MAX_LAYERS 64
#define MKD_MAX_MASK_DIM 1024

// ------------------------------------------------------------------------------------------------
// mask features at a level's resolution; mask logits -> packed attention mask, or fp32 masks; boxes; class columns
// ------------------------------------------------------------------------------------------------
struct SfMkdInterp { const float* in; float* out; int H, W, h, w; float ry, rx; size_t total; };      // total = F * Dm * h * w

#include "sf_maskattn.h"
__global__ __launch_bounds__(256) void sf_maskdec_interp_kernel(SfMkdInterp p) {
  const size_t hw = (size_t)p.h * p.w;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t fc = i / hw;
    const int pix = (int)(i - fc * hw), y = pix / p.w, x = pix - y * p.w;
    int y0, y1, x0, x1;
    float ly, lx;
    sf_bilinear_axis(y, p.ry, p.H, &y0, &y1, &ly);
    sf_bilinear_axis(x, p.rx, p.W, &x0, &x1, &lx);
    const float* src = p.in + fc * (size_t)p.H * p.W;
    const float hy = 1.f - ly, hx = 1.f - lx;
    p.out[i] = hy * (hx * src[y0 * p.W + x0] + lx * src[y0 * p.W + x1]) + ly * (hx * src[y1 * p.W + x0] + lx * src[y1 * p.W + x1]);
  }
}

static hipError_t mkd_launch_interp(const float* in, float* out, int F, int Dm, int H, int W, int h, int w, hipStream_t s) {
  SfMkdInterp p;
  p.in = in; p.out = out; p.H = H; p.W = W; p.h = h; p.w = w;
  p.ry = (float)H / (float)h; p.rx = (float)W / (float)w;
  p.total = (size_t)F * Dm * h * w;
  size_t grid = (p.total + 255) / 256;
  if (grid > 4096) grid = 4096;
  return sf_launch(sf_maskdec_interp_kernel, dim3((unsigned)grid), dim3(256), 0, s, p);
}

struct SfMkdMask {
  const float* me;        // [F, Q, Dm]
  const float* feat;      // [F, Dm, P]
  uint32_t* bits;         // [F, Q, words], or null
  float* logits;          // [F, Q, P], or null
  int F, Q, Dm, P, words;
};

__global__ __launch_bounds__(64 * MKD_WAVES) void sf_maskdec_mask_kernel(SfMkdMask p) {
  extern __shared__ __attribute__((aligned(16))) float mm_smem[];      // mask_embed of 16 queries [16][Dm], then [MKD_WAVES] flag words
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int q0 = (int)blockIdx.x * 16, f = (int)blockIdx.y, Dm = p.Dm, P = p.P;
  unsigned* flags = reinterpret_cast<unsigned*>(mm_smem + 16 * Dm);
  for (int i = (int)threadIdx.x; i < 16 * (Dm >> 2); i += 64 * MKD_WAVES) {
    const int qq = i / (Dm >> 2), c = (i - qq * (Dm >> 2)) * 4;
    mf4_t v = {0.f, 0.f, 0.f, 0.f};
    if (q0 + qq < p.Q) v = *reinterpret_cast<const mf4_t*>(p.me + ((size_t)f * p.Q + q0 + qq) * Dm + c);
    *reinterpret_cast<mf4_t*>(mm_smem + qq * Dm + c) = v;
  }
  __syncthreads();
  const int chunks = (P + 63) >> 6;
  unsigned full = 0xffffu;                               // bit q: every pixel of this wave's chunks so far is below zero
  for (int ch = wave; ch < chunks; ch += MKD_WAVES) {
    const int pix = ch * 64 + lane;
    const bool valid = pix < P;
    const float* fp = p.feat + (size_t)f * Dm * P + (valid ? pix : P - 1);
    float acc[16][4];
#pragma unroll
    for (int qq = 0; qq < 16; ++qq) { acc[qq][0] = 0.f; acc[qq][1] = 0.f; acc[qq][2] = 0.f; acc[qq][3] = 0.f; }
    for (int c = 0; c < Dm; c += 4) {
      const float v0 = fp[(size_t)c * P], v1 = fp[(size_t)(c + 1) * P], v2 = fp[(size_t)(c + 2) * P], v3 = fp[(size_t)(c + 3) * P];
#pragma unroll
      for (int qq = 0; qq < 16; ++qq) {
        const mf4_t m = *reinterpret_cast<const mf4_t*>(mm_smem + qq * Dm + c);      // the same address in every lane: a broadcast
        acc[qq][0] = fmaf(m[0], v0, acc[qq][0]); acc[qq][1] = fmaf(m[1], v1, acc[qq][1]);
        acc[qq][2] = fmaf(m[2], v2, acc[qq][2]); acc[qq][3] = fmaf(m[3], v3, acc[qq][3]);
      }
    }
    const unsigned long long in_range = __ballot(valid);
#pragma unroll
    for (int qq = 0; qq < 16; ++qq) {
      const float logit = (acc[qq][0] + acc[qq][1]) + (acc[qq][2] + acc[qq][3]);
      if (q0 + qq >= p.Q) continue;
      const size_t row = (size_t)f * p.Q + q0 + qq;
      if (p.logits && valid) p.logits[row * P + pix] = logit;
      if (p.bits) {
        const unsigned long long neg = __ballot(valid && logit < 0.f);
        if (neg != in_range) full &= ~(1u << qq);
        const int word = ch * 2 + lane;
        if (lane < 2 && word < p.words) p.bits[row * p.words + word] = lane ? (unsigned)(neg >> 32) : (unsigned)neg;
      }
    }
  }
  if (!p.bits) return;
  // the reference's rule: a row with every bit set is cleared (attn_mask[where(attn_mask.sum(-1) == HW)] = False)
  if (lane == 0) flags[wave] = full;
  __syncthreads();
  unsigned all = 0xffffu;
#pragma unroll
  for (int w = 0; w < MKD_WAVES; ++w) all &= flags[w];
  if (!all) return;
  for (int ch = wave; ch < chunks; ch += MKD_WAVES) {
    const int word = ch * 2 + lane;
    if (lane < 2 && word < p.words)
      for (int qq = 0; qq < 16; ++qq)
        if (((all >> qq) & 1u) && q0 + qq < p.Q) p.bits[((size_t)f * p.Q + q0 + qq) * p.words + word] = 0u;
  }
}

static hipError_t mkd_launch_mask(const SfMkdMask& p, hipStream_t s) {
  if (!p.me || !p.feat || (!p.bits) == (!p.logits) || p.F < 1 || p.F > 65535 || p.Q < 1 || p.P < 1) return hipErrorInvalidValue;
  if (p.Dm < 4 || p.Dm % 4 || p.Dm > MKD_MAX_MASK_DIM || (p.bits && p.words < (p.P + 31) / 32)) return hipErrorInvalidValue;
  if (((uintptr_t)p.me & 15) || ((uintptr_t)p.feat | (uintptr_t)p.bits | (uintptr_t)p.logits) & 3) return hipErrorInvalidValue;
  const size_t lds = (size_t)16 * p.Dm * sizeof(float) + MKD_WAVES * sizeof(unsigned);
  return sf_launch_big_lds(sf_maskdec_mask_kernel, dim3((unsigned)((p.Q + 15) / 16), (unsigned)p.F), dim3(64 * MKD_WAVES), lds, s, p);
}

// one wave per (frame, query): (min x, min y, max x + 1, max y + 1) over the pixels above zero, divided by (W, H, W, H); zeros if none
__global__ __launch_bounds__(256) void sf_maskdec_box_kernel(const float* __restrict__ masks, float* __restrict__ boxes, int rows, int H, int W) {
  const int lane = (int)threadIdx.x & 63;
  const int row = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (row >= rows) return;
  const float* m = masks + (size_t)row * H * W;
  int x0 = W, y0 = H, x1 = -1, y1 = -1;
  for (int i = lane; i < H * W; i += 64) {
    if (m[i] > 0.f) {
      const int y = i / W, x = i - y * W;
      x0 = x < x0 ? x : x0; y0 = y < y0 ? y : y0; x1 = x > x1 ? x : x1; y1 = y > y1 ? y : y1;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int a = __shfl_xor(x0, o, 64), b = __shfl_xor(y0, o, 64), c = __shfl_xor(x1, o, 64), d = __shfl_xor(y1, o, 64);
    x0 = a < x0 ? a : x0; y0 = b < y0 ? b : y0; x1 = c > x1 ? c : x1; y1 = d > y1 ? d : y1;
  }
  if (lane < 4) {
    float v = 0.f;
    if (x1 >= 0) v = lane == 0 ? (float)x0 / (float)W : lane == 1 ? (float)y0 / (float)H : lane == 2 ? (float)(x1 + 1) / (float)W : (float)(y1 + 1) / (float)H;
    boxes[(size_t)row * 4 + lane] = v;
  }
}

__global__ __launch_bounds__(256) void sf_maskdec_cut_kernel(const float* __restrict__ in, float* __restrict__ out, int rows, int Cp, int C) {
  const size_t total = (size_t)rows * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / C;
    out[i] = in[r * Cp + (i - r * C)];
  }
}

static unsigned mkd_stream_grid(size_t total) {
  const size_t grid = (total + 255) / 256;
  return (unsigned)(grid > 2048 ? 2048 : (grid ? grid : 1));
}

// shapes and alignment: checked by the callers
static hipError_t mkd_row(const float* x, const float* r, int r_mod, const SfDevLN* ln, const float* pe, int pe_mod, float* y, bf16_t* y_hi, bf16_t* y_lo,
                          bf16_t* q_hi, bf16_t* q_lo, int rows, int C, hipStream_t s) {
  SfRowArgs p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.r = r; p.r_mod = r_mod; p.rows = rows; p.D = C; p.eps = MKD_LN_EPS;
  if (ln) { p.gamma = ln->g; p.beta = ln->b; }
  p.y = y; p.y_hi = y_hi; p.y_lo = y_lo;
  if (q_hi) { p.pe = pe; p.pe_mod = pe_mod; p.q_hi = q_hi; p.q_lo = q_lo; }
  return sf_launch_row(p, s);
}

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
struct MkdLayer {
  SfDevLinear cq, ckv, ck, co;           // cross-attention: q; [k (no bias) ; v]; k with its bias (the position table's projection); out
  SfDevLinear sqk, sv, so;               // self-attention: [q ; k]; v; out
  SfDevLinear lin1, lin2;
  SfDevLN cnorm, snorm, fnorm;
};

struct sf_maskdec : SfModelHandle {
  sf_maskdec_config cfg;
  bool proj = false;                     // input_proj holds convolutions
  int Cp = 0, hd = 0;                    // class columns padded for the GEMM; channels per head
  SfDevLinear in_proj[MKD_LEVELS];       // bias + level_embed[l]
  const float* pos_level = nullptr;      // what the position table adds per level: zeros with input_proj, else level_embed
  std::vector<MkdLayer> layers;
  SfDevLN dnorm;
  const float* query_feat = nullptr;
  const float* query_embed = nullptr;
  SfDevLinear cls, mlp[3];
  std::vector<SfDevLinear> reid;
};

static std::string mkd_idx(const char* a, int i, const char* b) { return std::string(a) + std::to_string(i) + b; }

extern "C" int sf_maskdec_create(const sf_maskdec_config* cfg, int device, sf_maskdec** out) {
  const char* who = "sf_maskdec_create";
  if (!cfg || !out) return sf_set_err(SF_ERR_INVALID, "%s: null argument", who);
  const sf_maskdec_config& c = *cfg;
  if (c.pre_norm) return sf_set_err(SF_ERR_INVALID, "%s: pre_norm: only the post-norm decoder (pre_norm=False, every shipped config) runs natively", who);
  if (!c.mask_classification) return sf_set_err(SF_ERR_INVALID, "%s: mask_classification must be set (the reference supports nothing else either)", who);
  const struct { const char* name; int v; } widths[] = {{"hidden_dim", c.hidden_dim}, {"dim_feedforward", c.dim_feedforward}, {"mask_dim", c.mask_dim}, {"in_channels", c.in_channels}};
  for (const auto& w : widths)
    if (w.v <= 0 || w.v % 64) return sf_set_err(SF_ERR_INVALID, "%s: %s %d must be a positive multiple of 64 (the GEMM kernels' k-step)", who, w.name, w.v);
  if (c.mask_dim > MKD_MAX_MASK_DIM) return sf_set_err(SF_ERR_INVALID, "%s: mask_dim %d above %d (16 mask embeddings in LDS)", who, c.mask_dim, MKD_MAX_MASK_DIM);
  if (c.nheads < 1 || c.hidden_dim % c.nheads || (c.hidden_dim / c.nheads) % 8 || c.hidden_dim / c.nheads < 8 || c.hidden_dim / c.nheads > 128)
    return sf_set_err(SF_ERR_INVALID, "%s: hidden_dim / nheads = %d / %d must be a multiple of 8 in 8..128 (the attention kernel's head width)", who, c.hidden_dim, c.nheads);
  if (c.num_queries < 1 || c.num_queries > 65535) return sf_set_err(SF_ERR_INVALID, "%s: num_queries %d outside 1..65535", who, c.num_queries);
  if (c.num_classes < 1 || c.num_classes > 65535) return sf_set_err(SF_ERR_INVALID, "%s: num_classes %d outside 1..65535", who, c.num_classes);
  if (c.dec_layers < 0 || c.dec_layers > MKD_MAX_LAYERS) return sf_set_err(SF_ERR_INVALID, "%s: dec_layers %d outside 0..%d", who, c.dec_layers, MKD_MAX_LAYERS);
  if (c.reid_layers < -1 || c.reid_layers > 16) return sf_set_err(SF_ERR_INVALID, "%s: reid_layers %d outside -1..16 (-1: no reid_embed, 0: identity)", who, c.reid_layers);
  if (c.reid_layers > 1 && (c.reid_hidden_dim <= 0 || c.reid_hidden_dim % 64))
    return sf_set_err(SF_ERR_INVALID, "%s: reid_hidden_dim %d must be a positive multiple of 64 (the GEMM kernels' k-step)", who, c.reid_hidden_dim);
  const bool proj = c.in_channels != c.hidden_dim || c.enforce_input_project;
  sf_maskdec* h = new sf_maskdec();
  h->cfg = c;
  h->device = device;
  h->proj = proj;
  h->hd = c.hidden_dim / c.nheads;
  h->Cp = (c.num_classes + 1 + 15) / 16 * 16;
  const int64_t C = c.hidden_dim, Fd = c.dim_feedforward;
  SfWeightStore& w = h->weights;
  w.noun = "mask decoder";
  w.prefix = "sem_seg_head.predictor.";
  w.dtype_msg = "sf_maskdec_load_tensor: dtype %d unsupported (fp32, fp64, bf16)";
  for (int i = 0; i < c.dec_layers; ++i) {
    for (const std::string& p : {mkd_idx("transformer_self_attention_layers.", i, ".self_attn."), mkd_idx("transformer_cross_attention_layers.", i, ".multihead_attn.")}) {
      w.expected[p + "in_proj_weight"] = {3 * C, C};
      w.expected[p + "in_proj_bias"] = {3 * C};
      w.expect_linear(p + "out_proj.", C, C);
    }
    w.expect_affine(mkd_idx("transformer_self_attention_layers.", i, ".norm."), C);
    w.expect_affine(mkd_idx("transformer_cross_attention_layers.", i, ".norm."), C);
    w.expect_linear(mkd_idx("transformer_ffn_layers.", i, ".linear1."), Fd, C);
    w.expect_linear(mkd_idx("transformer_ffn_layers.", i, ".linear2."), C, Fd);
    w.expect_affine(mkd_idx("transformer_ffn_layers.", i, ".norm."), C);
  }
  w.expect_affine("decoder_norm.", C);
  w.expected["query_feat.weight"] = {c.num_queries, C};
  w.expected["query_embed.weight"] = {c.num_queries, C};
  w.expected["level_embed.weight"] = {MKD_LEVELS, C};
  if (proj)
    for (int l = 0; l < MKD_LEVELS; ++l) {
      w.expected[mkd_idx("input_proj.", l, ".weight")] = {C, c.in_channels, 1, 1};
      w.expected[mkd_idx("input_proj.", l, ".bias")] = {C};
    }
  w.expect_linear("class_embed.", c.num_classes + 1, C);
  w.expect_linear("mask_embed.layers.0.", C, C);
  w.expect_linear("mask_embed.layers.1.", C, C);
  w.expect_linear("mask_embed.layers.2.", c.mask_dim, C);
  for (int n = 0; n < c.reid_layers; ++n)
    w.expect_linear(mkd_idx("reid_embed.layers.", n, "."), n + 1 == c.reid_layers ? C : c.reid_hidden_dim, n == 0 ? C : c.reid_hidden_dim);
  *out = h;
  return SF_OK;
}

extern "C" void sf_maskdec_destroy(sf_maskdec* h) { delete h; }

extern "C" int sf_maskdec_load_tensor(sf_maskdec* h, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
  return sf_model_load_tensor(h, "sf_maskdec_load_tensor", key, host_ptr, dtype, shape, ndim);
}

extern "C" int sf_maskdec_missing_weights(sf_maskdec* h) { return sf_model_missing_weights(h); }

// Weights rounded (bf16 mode) or split into hi + lo planes (bf16x3) ONCE, here.  Makes the handle's device current and leaves it so.
extern "C" int sf_maskdec_finalize(sf_maskdec* h, int compute) {
  SF_TRY(sf_model_begin_finalize(h, compute));
  const bool lo = compute == SF_COMPUTE_BF16X3;
  const sf_maskdec_config& c = h->cfg;
  const int C = c.hidden_dim, Fd = c.dim_feedforward;
  SfWeightStore& w = h->weights;
  auto linear = [&](const std::string& p, int N, int K, int Np, SfDevLinear* out) {
    return sf_upload_linear(h->dev, w.data(p + "weight"), &w.data(p + "bias"), N, K, Np, lo, out);
  };
  const std::vector<float>& le = w.data("level_embed.weight");
  if (h->proj) {
    for (int l = 0; l < MKD_LEVELS; ++l) {
      std::vector<float> b = w.data(mkd_idx("input_proj.", l, ".bias"));
      for (int n = 0; n < C; ++n) b[n] += le[(size_t)l * C + n];
      SF_TRY(sf_upload_linear(h->dev, w.data(mkd_idx("input_proj.", l, ".weight")), &b, C, c.in_channels, C, lo, &h->in_proj[l]));
    }
    SF_TRY(h->dev.upload(std::vector<float>((size_t)MKD_LEVELS * C, 0.f), &h->pos_level));
  } else {
    SF_TRY(h->dev.upload(le, &h->pos_level));
  }
  h->layers.assign(c.dec_layers, MkdLayer());
  for (int i = 0; i < c.dec_layers; ++i) {
    MkdLayer& L = h->layers[i];
    const int lvl = i % MKD_LEVELS;
    {
      const std::string p = mkd_idx("transformer_cross_attention_layers.", i, ".multihead_attn.");
      const std::vector<float>& iw = w.data(p + "in_proj_weight");
      const std::vector<float>& ib = w.data(p + "in_proj_bias");
      SfDevLinear all;
      SF_TRY(sf_upload_linear(h->dev, iw, nullptr, 3 * C, C, 3 * C, lo, &all));
      std::vector<float> bq(ib.begin(), ib.begin() + C), bk(ib.begin() + C, ib.begin() + 2 * C), bkv((size_t)2 * C, 0.f);
      for (int n = 0; n < C; ++n) {
        double v = ib[(size_t)2 * C + n];
        if (!h->proj)      // src = x + level_embed: W_v level_embed joins the bias (W_k level_embed rides with the position table)
          for (int k = 0; k < C; ++k) v += (double)iw[((size_t)2 * C + n) * C + k] * (double)le[(size_t)lvl * C + k];
        bkv[(size_t)C + n] = (float)v;
      }
      const float *dq, *dk, *dkv;
      SF_TRY(h->dev.upload(bq, &dq));
      SF_TRY(h->dev.upload(bk, &dk));
      SF_TRY(h->dev.upload(bkv, &dkv));
      L.cq = sf_linear_rows(all, 0, C, dq);
      L.ck = sf_linear_rows(all, C, C, dk);
      L.ckv = sf_linear_rows(all, C, 2 * C, dkv);
      SF_TRY(linear(p + "out_proj.", C, C, C, &L.co));
      SF_TRY(sf_upload_ln(h->dev, w, mkd_idx("transformer_cross_attention_layers.", i, ".norm."), &L.cnorm));
    }
    {
      const std::string p = mkd_idx("transformer_self_attention_layers.", i, ".self_attn.");
      SfDevLinear all;
      SF_TRY(sf_upload_linear(h->dev, w.data(p + "in_proj_weight"), &w.data(p + "in_proj_bias"), 3 * C, C, 3 * C, lo, &all));
      L.sqk = sf_linear_rows(all, 0, 2 * C, all.bias);
      L.sv = sf_linear_rows(all, 2 * C, C, all.bias + 2 * C);
      SF_TRY(linear(p + "out_proj.", C, C, C, &L.so));
      SF_TRY(sf_upload_ln(h->dev, w, mkd_idx("transformer_self_attention_layers.", i, ".norm."), &L.snorm));
    }
    SF_TRY(linear(mkd_idx("transformer_ffn_layers.", i, ".linear1."), Fd, C, Fd, &L.lin1));
    SF_TRY(linear(mkd_idx("transformer_ffn_layers.", i, ".linear2."), C, Fd, C, &L.lin2));
    SF_TRY(sf_upload_ln(h->dev, w, mkd_idx("transformer_ffn_layers.", i, ".norm."), &L.fnorm));
  }
  SF_TRY(sf_upload_ln(h->dev, w, "decoder_norm.", &h->dnorm));
  SF_TRY(h->dev.upload(w.data("query_feat.weight"), &h->query_feat));
  SF_TRY(h->dev.upload(w.data("query_embed.weight"), &h->query_embed));
  SF_TRY(linear("class_embed.", c.num_classes + 1, C, h->Cp, &h->cls));
  SF_TRY(linear("mask_embed.layers.0.", C, C, C, &h->mlp[0]));
  SF_TRY(linear("mask_embed.layers.1.", C, C, C, &h->mlp[1]));
  SF_TRY(linear("mask_embed.layers.2.", c.mask_dim, C, c.mask_dim, &h->mlp[2]));
  h->reid.assign(c.reid_layers > 0 ? c.reid_layers : 0, SfDevLinear());
  for (int n = 0; n < c.reid_layers; ++n) {
    const int N = n + 1 == c.reid_layers ? C : c.reid_hidden_dim, K = n == 0 ? C : c.reid_hidden_dim;
    SF_TRY(linear(mkd_idx("reid_embed.layers.", n, "."), N, K, N, &h->reid[n]));
  }
  h->finalized = true;
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
struct MkdPlan {
  int F, H, W, S;
  int h[MKD_LEVELS], w[MKD_LEVELS], hw[MKD_LEVELS], start[MKD_LEVELS], words[MKD_LEVELS];
  int32_t shapes[2 * MKD_LEVELS];
  int max_hw;
  size_t kpos_rows;                      // sum over the layers of their level's pixels
};

static int mkd_plan(const sf_maskdec* h, int F, const int32_t* level_shapes, int H, int W, MkdPlan* pl) {
  const char* who = "sf_maskdec";
  if (!h) return sf_set_err(SF_ERR_INVALID, "null handle");
  if (F < 1 || F > 65535) return sf_set_err(SF_ERR_INVALID, "%s: %d frames outside 1..65535", who, F);
  if (!level_shapes) return sf_set_err(SF_ERR_INVALID, "%s: null level shapes (a host array of three (H, W) pairs)", who);
  if (H < 1 || W < 1 || H > 4096 || W > 4096) return sf_set_err(SF_ERR_INVALID, "%s: mask_features are %d x %d (1..4096 each)", who, H, W);
  memset(pl, 0, sizeof(*pl));
  pl->F = F; pl->H = H; pl->W = W;
  const sf_maskdec_config& c = h->cfg;
  const long long wide = std::max(std::max(3 * c.hidden_dim, c.dim_feedforward), std::max(h->Cp, std::max(c.mask_dim, std::max(c.reid_hidden_dim, c.in_channels))));
  for (int l = 0; l < MKD_LEVELS; ++l) {
    const int hh = level_shapes[2 * l], ww = level_shapes[2 * l + 1];
    if (hh < 1 || ww < 1 || hh > 4096 || ww > 4096) return sf_set_err(SF_ERR_INVALID, "%s: level %d is %d x %d (1..4096 each)", who, l, hh, ww);
    if ((long long)F * hh * ww * wide > 0x7fffffffLL)
      return sf_set_err(SF_ERR_CAPACITY, "%s: %d frames of level %d exceed 2^31 - 1 elements per activation; decode in groups of frames", who, F, l);
    pl->h[l] = hh; pl->w[l] = ww; pl->hw[l] = hh * ww; pl->start[l] = pl->S; pl->words[l] = (hh * ww + 31) / 32;
    pl->shapes[2 * l] = hh; pl->shapes[2 * l + 1] = ww;
    pl->S += hh * ww;
    pl->max_hw = std::max(pl->max_hw, hh * ww);
  }
  if ((long long)F * c.num_queries * std::max<long long>((long long)H * W, wide) > 0x7fffffffLL || (long long)F * c.mask_dim * H * W > 0x7fffffffLL)
    return sf_set_err(SF_ERR_CAPACITY, "%s: %d frames of %d queries on %d x %d exceed 2^31 - 1 elements per activation; decode in groups of frames", who, F, c.num_queries, H, W);
  for (int i = 0; i < c.dec_layers; ++i) pl->kpos_rows += (size_t)pl->hw[i % MKD_LEVELS];
  return SF_OK;
}

struct MkdWorkspace {
  float *pos, *ref, *kpos;
  SfPlanes pos_p, xin, src[MKD_LEVELS];
  float* feat[MKD_LEVELS];               // mask_features at the level's resolution [F, Dm, hw]
  float *kv, *out, *tmp, *qkv, *dn, *me, *cls, *embeds;
  SfPlanes y, q, ctx, hid, dnp, ma, mb, ra, rb;
  uint32_t* bits;
  size_t bytes;
};

static MkdWorkspace mkd_carve(const sf_maskdec* h, const MkdPlan& pl, void* base) {
  MkdWorkspace w;
  memset(&w, 0, sizeof(w));
  SfCarver cv(base, h->compute == SF_COMPUTE_BF16X3);
  const sf_maskdec_config& c = h->cfg;
  const size_t C = c.hidden_dim, M = (size_t)pl.F * c.num_queries;
  w.pos = cv.take<float>((size_t)pl.S * C);
  w.ref = cv.take<float>((size_t)pl.S * MKD_LEVELS * 2);
  w.kpos = cv.take<float>(std::max<size_t>(pl.kpos_rows, 1) * C);
  w.pos_p = cv.planes((size_t)pl.S * C);
  if (h->proj) w.xin = cv.planes((size_t)pl.F * pl.max_hw * c.in_channels);
  for (int l = 0; l < MKD_LEVELS; ++l) {
    w.src[l] = cv.planes((size_t)pl.F * pl.hw[l] * C);
    w.feat[l] = cv.take<float>((size_t)pl.F * c.mask_dim * pl.hw[l]);
  }
  w.kv = cv.take<float>((size_t)pl.F * pl.max_hw * 2 * C);
  w.out = cv.take<float>(M * C);
  w.tmp = cv.take<float>(M * C);
  w.qkv = cv.take<float>(M * 3 * C);
  w.dn = cv.take<float>(M * C);
  w.me = cv.take<float>(M * c.mask_dim);
  w.cls = cv.take<float>(M * h->Cp);
  w.embeds = cv.take<float>(M * C);
  w.y = cv.planes(M * C); w.q = cv.planes(M * C); w.ctx = cv.planes(M * C); w.dnp = cv.planes(M * C); w.ma = cv.planes(M * C); w.mb = cv.planes(M * C);
  w.hid = cv.planes(M * c.dim_feedforward);
  if (c.reid_layers > 1) { w.ra = cv.planes(M * c.reid_hidden_dim); w.rb = cv.planes(M * c.reid_hidden_dim); }
  int words = 1;
  for (int l = 0; l < MKD_LEVELS; ++l) words = std::max(words, pl.words[l]);
  w.bits = cv.take<uint32_t>(M * words);
  w.bytes = cv.bytes();
  return w;
}

extern "C" int sf_maskdec_workspace_bytes(sf_maskdec* h, int F, const int32_t* level_shapes, int H, int W, size_t* out) {
  if (!out) return sf_set_err(SF_ERR_INVALID, "null argument");
  MkdPlan pl;
  SF_TRY(mkd_plan(h, F, level_shapes, H, W, &pl));
  SF_TRY(sf_model_check_finalized(h, "sf_maskdec", true));
  *out = mkd_carve(h, pl, nullptr).bytes;
  return SF_OK;
}

extern "C" int sf_maskdec_forward(sf_maskdec* h, const float* const* x_dev, const float* mask_features_dev, int F, const int32_t* level_shapes, int H,
                                  int W, const sf_maskdec_outputs* outputs, void* workspace_dev, size_t workspace_bytes, sf_stream stream) {
  const char* who = "sf_maskdec_forward";
  MkdPlan pl;
  SF_TRY(mkd_plan(h, F, level_shapes, H, W, &pl));
  SF_TRY(sf_model_check_finalized(h, "sf_maskdec"));
  if (!x_dev || !mask_features_dev || !outputs || !workspace_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  const sf_maskdec_outputs& o = *outputs;
  if (!o.pred_logits || !o.pred_masks) return sf_set_err(SF_ERR_INVALID, "%s: pred_logits and pred_masks are required", who);
  const sf_maskdec_config& c = h->cfg;
  const bool cl = c.reid_layers >= 0;
  if (!cl && (o.pred_embeds || o.aux_embeds)) return sf_set_err(SF_ERR_INVALID, "%s: this decoder has no reid_embed (pred_embeds / aux_embeds must be NULL)", who);
  uintptr_t bits = (uintptr_t)mask_features_dev | (uintptr_t)o.pred_logits | (uintptr_t)o.pred_masks | (uintptr_t)o.pred_queries | (uintptr_t)o.pred_embeds |
                   (uintptr_t)o.pred_bboxes | (uintptr_t)o.aux_logits | (uintptr_t)o.aux_masks | (uintptr_t)o.aux_queries | (uintptr_t)o.aux_embeds |
                   (uintptr_t)o.attn_masks;
  for (int l = 0; l < MKD_LEVELS; ++l) {
    if (!x_dev[l]) return sf_set_err(SF_ERR_INVALID, "%s: x_dev[%d] is null", who, l);
    bits |= (uintptr_t)x_dev[l];
  }
  if (bits & 15) return sf_set_err(SF_ERR_INVALID, "%s: features and outputs must be 16-byte aligned", who);
  const MkdWorkspace ws = mkd_carve(h, pl, workspace_dev);
  SF_TRY(sf_check_workspace(who, "sf_maskdec_workspace_bytes", workspace_dev, workspace_bytes, ws.bytes));
  hipStream_t s = (hipStream_t)stream;
  const bool split = h->compute == SF_COMPUTE_BF16X3;
  const int C = c.hidden_dim, Q = c.num_queries, M = F * Q, Dm = c.mask_dim, heads = c.nheads, hd = h->hd, L = c.dec_layers, K1 = c.num_classes + 1;
  const float scale = 1.0f / sqrtf((float)hd);
  const SfLinearCaller lin{split, 2, s};      // act 2: ReLU

  // ---- what depends on the shapes only: the sine table (+ level_embed without input_proj) and its k projection per layer ----
  SF_TRY(sf_op_pixdec_pos_ref(h->pos_level, pl.shapes, MKD_LEVELS, 1, C, ws.pos, ws.ref, stream));
  HIP_TRY(sf_launch_split(ws.pos, ws.pos_p.hi, ws.pos_p.lo, (size_t)pl.S * C, s));
  std::vector<const float*> kpos(L);
  {
    size_t row = 0;
    for (int i = 0; i < L; ++i) {
      const int l = i % MKD_LEVELS;
      float* dst = ws.kpos + row * C;
      HIP_TRY(lin.f32(h->layers[i].ck, ws.pos_p.at((size_t)pl.start[l] * C), pl.hw[l], dst));
      kpos[i] = dst;
      row += (size_t)pl.hw[l];
    }
  }
  // ---- per level: src as GEMM operand planes, and mask_features at the level's resolution ----
  SfPlanes src[MKD_LEVELS];
  for (int l = 0; l < MKD_LEVELS; ++l) {
    src[l] = ws.src[l];
    if (h->proj) {
      SF_TRY(sf_op_pixdec_nchw_to_planes(x_dev[l], ws.xin.hi, ws.xin.lo, F, c.in_channels, pl.hw[l], stream));
      HIP_TRY(lin.planes(h->in_proj[l], ws.xin, F * pl.hw[l], src[l], false));
    } else {
      SF_TRY(sf_op_pixdec_nchw_to_planes(x_dev[l], src[l].hi, src[l].lo, F, C, pl.hw[l], stream));
    }
    bool used = L > 0 && l == 0;                         // the mask of layer i has the resolution of level i % 3
    for (int i = 1; i < L; ++i) used = used || i % MKD_LEVELS == l;
    if (used) HIP_TRY(mkd_launch_interp(mask_features_dev, ws.feat[l], F, Dm, H, W, pl.h[l], pl.w[l], s));
  }
  // ---- queries: query_feat replicated over the frames, and the planes of query_feat + query_embed ----
  HIP_TRY(hipMemsetAsync(ws.tmp, 0, (size_t)M * C * sizeof(float), s));
  HIP_TRY(mkd_row(ws.tmp, h->query_feat, Q, nullptr, h->query_embed, Q, ws.out, nullptr, nullptr, ws.q.hi, ws.q.lo, M, C, s));

  size_t mask_off = 0;                                   // words of the exported masks so far
  for (int i = 0; i <= L; ++i) {
    const bool last = i == L;
    if (i > 0) {
      const MkdLayer& ly = h->layers[i - 1];
      const int l = (i - 1) % MKD_LEVELS, hw = pl.hw[l];
      const uint32_t* mask = o.attn_masks ? o.attn_masks + (mask_off - (size_t)M * pl.words[l]) : ws.bits;
      // cross-attention
      HIP_TRY(lin.f32(ly.cq, ws.q, M, ws.qkv, C));
      HIP_TRY(lin.f32(ly.ckv, src[l], F * hw, ws.kv, 2 * C));
      SfMkaFwd a;
      memset(&a, 0, sizeof(a));
      a.q = ws.qkv; a.k = ws.kv; a.v = ws.kv + C; a.kpos = kpos[i - 1]; a.mask = mask;
      a.ctx_hi = ws.ctx.hi; a.ctx_lo = ws.ctx.lo;
      a.q_pitch = C; a.kv_pitch = 2 * C; a.pos_pitch = C;
      a.F = F; a.Tq = Q; a.Tk = hw; a.heads = heads; a.hd = hd; a.words = pl.words[l]; a.scale = scale;
      HIP_TRY(mka_launch_forward(a, s));
      HIP_TRY(lin.resid(ly.co, ws.ctx, M, ws.out, ws.tmp));
      HIP_TRY(mkd_row(ws.tmp, nullptr, 0, &ly.cnorm, h->query_embed, Q, ws.out, ws.y.hi, ws.y.lo, ws.q.hi, ws.q.lo, M, C, s));
      // self-attention: q = k = x + query_embed, v = x
      HIP_TRY(lin.f32(ly.sqk, ws.q, M, ws.qkv, 3 * C));
      HIP_TRY(lin.f32(ly.sv, ws.y, M, ws.qkv + 2 * C, 3 * C));
      memset(&a, 0, sizeof(a));
      a.q = ws.qkv; a.k = ws.qkv + C; a.v = ws.qkv + 2 * C;
      a.ctx_hi = ws.ctx.hi; a.ctx_lo = ws.ctx.lo;
      a.q_pitch = 3 * C; a.kv_pitch = 3 * C;
      a.F = F; a.Tq = Q; a.Tk = Q; a.heads = heads; a.hd = hd; a.scale = scale;
      HIP_TRY(mka_launch_forward(a, s));
      HIP_TRY(lin.resid(ly.so, ws.ctx, M, ws.out, ws.tmp));
      HIP_TRY(mkd_row(ws.tmp, nullptr, 0, &ly.snorm, nullptr, 0, ws.out, ws.y.hi, ws.y.lo, nullptr, nullptr, M, C, s));
      // FFN
      HIP_TRY(lin.planes(ly.lin1, ws.y, M, ws.hid, true));
      HIP_TRY(lin.resid(ly.lin2, ws.hid, M, ws.out, ws.tmp));
      HIP_TRY(mkd_row(ws.tmp, nullptr, 0, &ly.fnorm, h->query_embed, Q, ws.out, nullptr, nullptr, last ? nullptr : ws.q.hi, ws.q.lo, M, C, s));
    }
    // ---- prediction heads on decoder_norm(output) ----
    float* dn = last ? (o.pred_queries ? o.pred_queries : ws.dn) : (o.aux_queries ? o.aux_queries + (size_t)i * M * C : ws.dn);
    HIP_TRY(mkd_row(ws.out, nullptr, 0, &h->dnorm, nullptr, 0, dn, ws.dnp.hi, ws.dnp.lo, nullptr, nullptr, M, C, s));
    float* logits = last ? o.pred_logits : (o.aux_logits ? o.aux_logits + (size_t)i * M * K1 : nullptr);
    if (logits) {
      HIP_TRY(lin.f32(h->cls, ws.dnp, M, ws.cls, h->Cp));
      HIP_TRY(sf_launch(sf_maskdec_cut_kernel, dim3(mkd_stream_grid((size_t)M * K1)), dim3(256), 0, s, (const float*)ws.cls, logits, M, h->Cp, K1));
    }
    float* embeds = last ? o.pred_embeds : (o.aux_embeds ? o.aux_embeds + (size_t)i * M * C : nullptr);
    if (embeds) {
      if (c.reid_layers == 0) HIP_TRY(hipMemcpyAsync(embeds, dn, (size_t)M * C * sizeof(float), hipMemcpyDeviceToDevice, s));
      SfPlanes in = ws.dnp;
      for (int n = 0; n < c.reid_layers; ++n) {
        if (n + 1 == c.reid_layers) { HIP_TRY(lin.f32(h->reid[n], in, M, embeds, C)); break; }
        const SfPlanes out = n & 1 ? ws.rb : ws.ra;
        HIP_TRY(lin.planes(h->reid[n], in, M, out, true));
        in = out;
      }
    }
    HIP_TRY(lin.planes(h->mlp[0], ws.dnp, M, ws.ma, true));
    HIP_TRY(lin.planes(h->mlp[1], ws.ma, M, ws.mb, true));
    HIP_TRY(lin.f32(h->mlp[2], ws.mb, M, ws.me, Dm));
    SfMkdMask m;
    memset(&m, 0, sizeof(m));
    m.me = ws.me; m.F = F; m.Q = Q; m.Dm = Dm;
    float* full = last ? o.pred_masks : (o.aux_masks ? o.aux_masks + (size_t)i * M * H * W : nullptr);
    if (full) {
      m.feat = mask_features_dev; m.P = H * W; m.logits = full;
      HIP_TRY(mkd_launch_mask(m, s));
      if (last && o.pred_bboxes) HIP_TRY(sf_launch(sf_maskdec_box_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, (const float*)full, o.pred_bboxes, M, H, W));
    }
    if (!last) {
      const int l = i % MKD_LEVELS;
      m.feat = ws.feat[l]; m.P = pl.hw[l]; m.words = pl.words[l]; m.logits = nullptr;
      m.bits = o.attn_masks ? o.attn_masks + mask_off : ws.bits;
      HIP_TRY(mkd_launch_mask(m, s));
      mask_off += (size_t)M * pl.words[l];
    }
  }
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// the kernels alone (parity tests)
// ------------------------------------------------------------------------------------------------
// the box kernel alone, over masks some other kernel made (the training path's full-resolution logits)
extern "C" int sf_op_maskdec_boxes(const float* masks_dev, float* boxes_dev, int rows, int H, int W, sf_stream stream) {
  const char* who = "sf_op_maskdec_boxes";
  if (!masks_dev || !boxes_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (rows < 1 || H < 1 || W < 1 || H > 4096 || W > 4096) return sf_set_err(SF_ERR_INVALID, "%s: rows = %d, H = %d, W = %d", who, rows, H, W);
  if ((long long)rows * H * W > 0x7fffffffLL) return sf_set_err(SF_ERR_CAPACITY, "%s: more than 2^31 - 1 elements", who);
  if (((uintptr_t)masks_dev | (uintptr_t)boxes_dev) & 15) return sf_set_err(SF_ERR_INVALID, "%s: every buffer must be 16-byte aligned", who);
  HIP_TRY(sf_launch(sf_maskdec_box_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, masks_dev, boxes_dev, rows, H, W));
  return SF_OK;
}

extern "C" size_t sf_op_maskdec_mask_workspace_bytes(int F, int mask_dim, int h, int w) {
  if (F < 1 || mask_dim < 1 || h < 1 || w < 1) return 0;
  return ((size_t)F * mask_dim * h * w * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" int sf_op_maskdec_mask(const float* mask_embed_dev, const float* mask_features_dev, int F, int Q, int mask_dim, int H, int W, int h, int w,
                                  uint32_t* bits_dev, float* logits_dev, float* boxes_dev, void* workspace_dev, size_t workspace_bytes, sf_stream stream) {
  const char* who = "sf_op_maskdec_mask";
  if (!mask_embed_dev || !mask_features_dev) return sf_set_err(SF_ERR_INVALID, "%s: null buffer", who);
  if (!bits_dev && !logits_dev) return sf_set_err(SF_ERR_INVALID, "%s: no output", who);
  if (boxes_dev && !logits_dev) return sf_set_err(SF_ERR_INVALID, "%s: the boxes are taken from the masks (logits_dev)", who);
  if (F < 1 || F > 65535 || Q < 1 || H < 1 || W < 1 || H > 4096 || W > 4096) return sf_set_err(SF_ERR_INVALID, "%s: F = %d (1..65535), Q = %d, H = %d, W = %d", who, F, Q, H, W);
  if (mask_dim < 4 || mask_dim % 4 || mask_dim > MKD_MAX_MASK_DIM) return sf_set_err(SF_ERR_INVALID, "%s: mask_dim = %d must be a multiple of 4 up to %d", who, mask_dim, MKD_MAX_MASK_DIM);
  if (bits_dev && (h < 1 || w < 1 || h > 4096 || w > 4096)) return sf_set_err(SF_ERR_INVALID, "%s: the mask's resolution is %d x %d", who, h, w);
  if ((long long)F * std::max(Q, mask_dim) * H * W > 0x7fffffffLL || (bits_dev && (long long)F * std::max(Q, mask_dim) * h * w > 0x7fffffffLL))
    return sf_set_err(SF_ERR_CAPACITY, "%s: more than 2^31 - 1 elements", who);
  if (((uintptr_t)mask_embed_dev | (uintptr_t)mask_features_dev | (uintptr_t)bits_dev | (uintptr_t)logits_dev | (uintptr_t)boxes_dev) & 15)
    return sf_set_err(SF_ERR_INVALID, "%s: every buffer must be 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  SfMkdMask m;
  memset(&m, 0, sizeof(m));
  m.me = mask_embed_dev; m.F = F; m.Q = Q; m.Dm = mask_dim;
  if (bits_dev) {
    if (!workspace_dev) return sf_set_err(SF_ERR_INVALID, "%s: the resampled features need the workspace", who);
    SF_TRY(sf_check_workspace(who, "sf_op_maskdec_mask_workspace_bytes", workspace_dev, workspace_bytes, sf_op_maskdec_mask_workspace_bytes(F, mask_dim, h, w)));
    HIP_TRY(mkd_launch_interp(mask_features_dev, (float*)workspace_dev, F, mask_dim, H, W, h, w, s));
    m.feat = (const float*)workspace_dev; m.P = h * w; m.words = (h * w + 31) / 32; m.bits = bits_dev;
    HIP_TRY(mkd_launch_mask(m, s));
  }
  if (logits_dev) {
    m.feat = mask_features_dev; m.P = H * W; m.words = 0; m.bits = nullptr; m.logits = logits_dev;
    HIP_TRY(mkd_launch_mask(m, s));
    if (boxes_dev) HIP_TRY(sf_launch(sf_maskdec_box_kernel, dim3((unsigned)((F * Q + 3) / 4)), dim3(256), 0, s, (const float*)logits_dev, boxes_dev, F * Q, H, W));
  }
  return SF_OK;
}
