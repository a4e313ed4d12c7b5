// SigLIP text tower (HF SiglipTextModel; the reference's frozen `self.text_encoder(ids)[1]`, modeling:1680, 1756, 1997, 2104, 2217, 2315,
// 2385): token ids -> last_hidden_state [B, L, D] and pooler_output [B, projection].  The Linears run on the GEMM launchers of the
// encoder (sf_launch_gemm, both compute modes) and the LayerNorms on sf_launch_layernorm; this file adds the three kernels the video
// side never needed, their launch sequence and the C entry points.
//
//   sf_text_embed_kernel       rows[b * L + l] = token_embedding[ids[b, l]] + position_embedding[l], fp32, 16-byte loads and stores;
//                              an id outside [0, vocab) is clamped (memory safety only: the Python layer refuses it before launch).
//                              The first LayerNorm of layer 0 follows as its own launch and emits the GEMM's operand planes.
//   sf_text_attention_kernel   softmax(scale q k^T + key_mask) v, non-causal, one WORKGROUP (4 waves) per (caption, head).  K and V of the
//                              head are staged ONCE as fp32 images [ceil16(L)][head_dim + 4] in LDS (rows past L zero-filled), then wave w
//                              takes the 16-query tiles w, w + 4, ...  Arithmetic and lane layout are those of sf_attention_generic.hip
//                              (v_mfma_f32_16x16x4_f32, exact fp32 products, flash-style running max / sum over 16-key tiles, two
//                              xor-shuffles per row statistic), so any head_dim that is a multiple of 8 up to 128 runs, and the inputs
//                              are the fp32 qkv rows in BOTH compute modes: one kernel, no operand rounding.  A masked key (mask byte 0)
//                              gets the score -inf, i.e. weight exactly 0, for every query of its caption; query rows at padded
//                              positions are computed like any other (HF's additive mask).  A caption without any valid key would
//                              have a zero sum: the Python layer refuses it, and the kernel writes zeros instead of dividing.
//                              LDS: 2 * ceil16(L) * (head_dim + 4) * 4 bytes = 34 KB at L = 64 / head_dim 64 (four workgroups per CU),
//                              132 KB at the limits L = 128 / head_dim 128.  Every output element has one owner and a fixed summation
//                              order (no atomics): bit-reproducible.
//   sf_text_pool_kernel        per caption: the LAST position's row (l = L - 1 whatever the mask says, as SiglipTextModel does) ->
//                              final_layer_norm (two-pass statistics) -> head Linear [P, D] + bias, fp32 FMAs.  A workgroup holds 8
//                              normalised rows in LDS and owns 64 output columns, so a weight row is read once per 8 captions.
//   sf_text_group_mean_kernel  class-prompt tables (modeling:2207-2223): L2-normalise each pooled row, average G consecutive rows,
//                              normalise again; one wave per label, fixed order.
//
// Unmasked calls run the same attention kernel (key_mask = null): sf_launch_spatial_attention rounds q / k / v to bf16 in the bf16 mode at
// head_dim 64, which is not this kernel's fp32 contract, so routing there would make the result depend on whether a mask was passed.
#include "sf_handle.h"

typedef __attribute__((ext_vector_type(4))) float tf4_t;

#define SF_TEXT_MAX_L 128
#define SF_TEXT_MAX_D 4096
#define SF_TEXT_POOL_ROWS 8        // captions per workgroup of the pooled head
#define SF_TEXT_POOL_COLS 64       // output columns per workgroup

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sf_text_embed_kernel(const int* __restrict__ ids, const float* __restrict__ tok,
                                                            const float* __restrict__ pos, float* __restrict__ out, int rows, int L,
                                                            int D4, int vocab) {
  const size_t total = (size_t)rows * D4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int r = (int)(i / D4), c = (int)(i - (size_t)r * D4);
    int id = ids[r];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const tf4_t a = reinterpret_cast<const tf4_t*>(tok)[(size_t)id * D4 + c];
    const tf4_t b = reinterpret_cast<const tf4_t*>(pos)[(size_t)(r % L) * D4 + c];
    reinterpret_cast<tf4_t*>(out)[i] = a + b;
  }
}

struct SfTextAttn {
  const float* qkv;              // [B * L, 3 D]: q | k | v columns as the packed Linear emits them
  const unsigned char* mask;     // [B, L], 0 = masked key; nullptr = every key valid
  float* ctx_f32;                // [B * L, D] or nullptr
  bf16_t* ctx_hi; bf16_t* ctx_lo;   // [B * L, D] operand planes of the out_proj GEMM, or nullptr (lo: accurate mode only)
  int B, L, heads, D;
  float scale;
};

SF_DEVICE tf4_t ta_mfma(float a, float b, tf4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

template <int HDQ>      // HDQ = head_dim / 4 <= 32
__global__ __launch_bounds__(256) void sf_text_attention_kernel(SfTextAttn p) {
  extern __shared__ __attribute__((aligned(16))) float ta_smem[];
  constexpr int HD = HDQ * 4, LD = HD + 4, NT = (HD + 15) / 16, CH = HD / 4;
  const int L = p.L, Lp = (L + 15) & ~15;
  float* kt = ta_smem;
  float* vt = kt + Lp * LD;
  const int b = blockIdx.x / p.heads, h = blockIdx.x % p.heads;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const size_t row0 = (size_t)b * L, pitch = (size_t)3 * p.D;
  // ---- K and V of this (caption, head), once: 16-byte row loads, rows past L zero (their keys are masked below; 0 * p stays finite) ----
  for (int c = threadIdx.x; c < Lp * CH; c += 256) {
    const int row = c / CH, cc = c % CH;
    tf4_t kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
    if (row < L) {
      const float* src = p.qkv + (row0 + row) * pitch + p.D + h * HD + cc * 4;
      kv = *reinterpret_cast<const tf4_t*>(src);
      vv = *reinterpret_cast<const tf4_t*>(src + p.D);
    }
    *reinterpret_cast<tf4_t*>(kt + row * LD + cc * 4) = kv;
    *reinterpret_cast<tf4_t*>(vt + row * LD + cc * 4) = vv;
  }
  __syncthreads();
  const unsigned char* mrow = p.mask ? p.mask + row0 : nullptr;
  const float c2 = p.scale * 1.44269504088896340736f;
  for (int qt = wave; qt < Lp / 16; qt += 4) {
    // this lane's query (l15 of the tile) and its HDQ contiguous dims; lanes past L repeat the last query and store nothing
    const int qi = qt * 16 + l15;
    float qreg[HDQ];
    {
      const float* q = p.qkv + (row0 + (qi < L ? qi : L - 1)) * pitch + h * HD + g * HDQ;
#pragma unroll
      for (int s = 0; s < HDQ; ++s) qreg[s] = q[s];
    }
    tf4_t o_acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) o_acc[t] = (tf4_t){0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    for (int k0 = 0; k0 < L; k0 += 16) {
      // S^T tile: keys k0 + l15 (A operand) x queries (B operand); lane (query l15, g) receives keys k0 + 4 g + r
      tf4_t s4 = {0.f, 0.f, 0.f, 0.f};
      {
        const float* kr = kt + (k0 + l15) * LD + g * HDQ;
#pragma unroll
        for (int s = 0; s < HDQ; ++s) s4 = ta_mfma(kr[s], qreg[s], s4);
      }
      float mx = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + 4 * g + r;
        const bool ok = key < L && (!mrow || mrow[key] != 0);
        s4[r] = ok ? s4[r] : -INFINITY;
        mx = fmaxf(mx, s4[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      // no valid key so far (m_new = -inf): keep zeros, exp2(-inf - (-inf)) would be NaN
      const float corr = m_new == -INFINITY ? 1.f : __builtin_amdgcn_exp2f((m_run - m_new) * c2);
      float psum = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s4[r] = m_new == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((s4[r] - m_new) * c2);
        psum += s4[r];
      }
      psum += __shfl_xor(psum, 16, 64);
      psum += __shfl_xor(psum, 32, 64);
      l_run = l_run * corr + psum;
      m_run = m_new;
      // O^T += V^T P^T: lane (dim l15 of the 16-dim tile, g) supplies V[k0 + 4 g + r][d]
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        o_acc[t] *= corr;
        const int d = t * 16 + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = d < HD ? vt[(k0 + 4 * g + r) * LD + d] : 0.f;
          o_acc[t] = ta_mfma(v, s4[r], o_acc[t]);
        }
      }
    }
    if (qi >= L) continue;
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;      // all keys masked: zeros, never a division by a zero sum
    const size_t ob = (row0 + qi) * p.D + h * HD;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int d = t * 16 + 4 * g;
      if (d < HD) {                                 // HD % 4 == 0: the four dims of a lane are all inside or all outside
        const tf4_t o = o_acc[t] * inv;
        if (p.ctx_f32) *reinterpret_cast<tf4_t*>(p.ctx_f32 + ob + d) = o;
        if (p.ctx_hi) store_planes4(o, p.ctx_hi, p.ctx_lo, ob + d);
      }
    }
  }
}

// grid (ceil(B / 8), ceil(P / 64)); dynamic LDS: 8 rows of D floats
__global__ __launch_bounds__(256) void sf_text_pool_kernel(const float* __restrict__ x, int B, int L, int D,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                           const float* __restrict__ w, const float* __restrict__ bias, int P,
                                                           float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float tp_rows[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cap0 = blockIdx.x * SF_TEXT_POOL_ROWS;
  for (int r = wave; r < SF_TEXT_POOL_ROWS; r += 4) {
    const int cap = cap0 + r;
    float* dst = tp_rows + (size_t)r * D;
    if (cap >= B) {
      for (int d = lane; d < D; d += 64) dst[d] = 0.f;
      continue;
    }
    const float* src = x + ((size_t)cap * L + (L - 1)) * D;
    if (!gamma) {                                   // rows that are normalised already
      for (int d = lane; d < D; d += 64) dst[d] = src[d];
      continue;
    }
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s += src[d];
    const float mean = wave_sum(s) / (float)D;
    float v = 0.f;
    for (int d = lane; d < D; d += 64) { const float c = src[d] - mean; v = fmaf(c, c, v); }
    const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)D + eps);
    for (int d = lane; d < D; d += 64) dst[d] = (src[d] - mean) * rstd * gamma[d] + beta[d];
  }
  __syncthreads();
  const int D4 = D / 4;
  const int pc0 = blockIdx.y * SF_TEXT_POOL_COLS;
  for (int j = wave; j < SF_TEXT_POOL_COLS; j += 4) {
    const int col = pc0 + j;
    if (col >= P) break;                            // wave-uniform
    float acc[SF_TEXT_POOL_ROWS];
#pragma unroll
    for (int r = 0; r < SF_TEXT_POOL_ROWS; ++r) acc[r] = 0.f;
    const tf4_t* wr = reinterpret_cast<const tf4_t*>(w + (size_t)col * D);
    for (int q = lane; q < D4; q += 64) {
      const tf4_t wv = wr[q];
#pragma unroll
      for (int r = 0; r < SF_TEXT_POOL_ROWS; ++r) {
        const tf4_t xv = *reinterpret_cast<const tf4_t*>(tp_rows + (size_t)r * D + q * 4);
        acc[r] = fmaf(wv[0], xv[0], acc[r]); acc[r] = fmaf(wv[1], xv[1], acc[r]);
        acc[r] = fmaf(wv[2], xv[2], acc[r]); acc[r] = fmaf(wv[3], xv[3], acc[r]);
      }
    }
    const float bv = bias ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < SF_TEXT_POOL_ROWS; ++r) {
      const float t = wave_sum(acc[r]);
      if (lane == 0 && cap0 + r < B) out[(size_t)(cap0 + r) * P + col] = t + bv;
    }
  }
}

// one wave per label: out[j] = normalise(mean_g normalise(in[j * G + g]))
__global__ __launch_bounds__(256) void sf_text_group_mean_kernel(const float* __restrict__ in, float* __restrict__ out, int labels, int G,
                                                                 int P) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= labels) return;
  float* o = out + (size_t)j * P;
  for (int gi = 0; gi < G; ++gi) {
    const float* r = in + ((size_t)j * G + gi) * P;
    float s = 0.f;
    for (int d = lane; d < P; d += 64) s = fmaf(r[d], r[d], s);
    const float inv = 1.0f / sqrtf(wave_sum(s));
    for (int d = lane; d < P; d += 64) o[d] = (gi ? o[d] : 0.f) + r[d] * inv;      // element d belongs to this lane alone
  }
  float s = 0.f;
  const float ig = 1.0f / (float)G;
  for (int d = lane; d < P; d += 64) { const float m = o[d] * ig; s = fmaf(m, m, s); }
  const float inv = 1.0f / sqrtf(wave_sum(s));
  for (int d = lane; d < P; d += 64) o[d] = o[d] * ig * inv;
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
static hipError_t text_launch_embed(const int* ids, const float* tok, const float* pos, float* out, int rows, int L, int D, int vocab,
                                    hipStream_t s) {
  const size_t total = (size_t)rows * (D / 4);
  size_t grid = (total + 255) / 256;
  if (grid > 4096) grid = 4096;
  return sf_launch(sf_text_embed_kernel, dim3((unsigned)grid), dim3(256), 0, s, ids, tok, pos, out, rows, L, D / 4, vocab);
}

static hipError_t text_launch_attention(const SfTextAttn& p, hipStream_t s) {
  if (p.B <= 0 || p.L <= 0 || p.L > SF_TEXT_MAX_L || p.heads <= 0 || p.D % p.heads) return hipErrorInvalidValue;
  const int hd = p.D / p.heads;
  if (hd < 8 || hd > 128 || hd % 8) return hipErrorInvalidValue;
  if (((uintptr_t)p.qkv & 15) || ((uintptr_t)p.ctx_f32 & 15) || ((uintptr_t)p.ctx_hi & 7) || ((uintptr_t)p.ctx_lo & 7)) return hipErrorInvalidValue;
  if ((size_t)p.B * p.heads > 0x7fffffffu) return hipErrorInvalidValue;
  const int Lp = (p.L + 15) & ~15;
  const size_t lds = (size_t)2 * Lp * (hd + 4) * sizeof(float);      // <= 132 KB at L = 128, head_dim 128
  const dim3 grid((unsigned)(p.B * p.heads)), block(256);
  switch (hd / 8) {
#define TA_CASE(E) case E: return sf_launch_big_lds(sf_text_attention_kernel<2 * E>, grid, block, lds, s, p);
    TA_CASE(1) TA_CASE(2) TA_CASE(3) TA_CASE(4) TA_CASE(5) TA_CASE(6) TA_CASE(7) TA_CASE(8)
    TA_CASE(9) TA_CASE(10) TA_CASE(11) TA_CASE(12) TA_CASE(13) TA_CASE(14) TA_CASE(15) TA_CASE(16)
#undef TA_CASE
    default: return hipErrorInvalidValue;
  }
}

// out [B, P] (group == 0), or the normalised group means [B / group, P] with `scratch` [B, P] holding the pooled rows
static hipError_t text_launch_pool(const float* x, int B, int L, int D, const float* gamma, const float* beta, float eps, const float* w,
                                   const float* bias, int P, int group, float* out, float* scratch, hipStream_t s) {
  if (B <= 0 || L <= 0 || P <= 0 || D <= 0 || D % 4 || D > SF_TEXT_MAX_D || group < 0) return hipErrorInvalidValue;
  if (group && (B % group || !scratch)) return hipErrorInvalidValue;
  if (((uintptr_t)x & 15) || ((uintptr_t)w & 15)) return hipErrorInvalidValue;
  float* pooled = group ? scratch : out;
  const dim3 grid((unsigned)((B + SF_TEXT_POOL_ROWS - 1) / SF_TEXT_POOL_ROWS), (unsigned)((P + SF_TEXT_POOL_COLS - 1) / SF_TEXT_POOL_COLS));
  const hipError_t e = sf_launch_big_lds(sf_text_pool_kernel, grid, dim3(256), (size_t)SF_TEXT_POOL_ROWS * D * sizeof(float), s, x, B, L, D, gamma,
                                         beta, eps, w, bias, P, pooled);
  if (e != hipSuccess || !group) return e;
  const int labels = B / group;
  return sf_launch(sf_text_group_mean_kernel, dim3((unsigned)((labels + 3) / 4)), dim3(256), 0, s, pooled, out, labels, group, P);
}

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
struct TextLayer { SfDevLN ln1, ln2; SfDevLinear qkv, out, fc1, fc2; };

struct sf_text : SfModelHandle {              // weights: q / k / v arrive separately and are packed at finalize
  sf_text_config cfg;
  int D = 0, I = 0, hd = 0;                   // I: intermediate_size padded to a multiple of 64 (zero weights, act(0) = 0)
  const float* tok = nullptr; const float* pos = nullptr;
  std::vector<TextLayer> layers;
  SfDevLN final_ln;
  const float* head_w = nullptr; const float* head_b = nullptr;      // fp32 [P, D], [P]
};

struct TextWorkspace {
  float* resid; float* qkv; float* pooled;
  SfPlanes xn, ctx, mid;      // GEMM operands: the normalised rows, the attention's output, the MLP's hidden rows
  size_t bytes;
};

static TextWorkspace text_carve(const sf_text* t, void* base, int B, int L) {
  TextWorkspace w;
  SfCarver c(base, t->compute == SF_COMPUTE_BF16X3, true);      // the lo planes are set aside in either mode
  const size_t M = (size_t)B * L, D = t->D, I = t->I;
  w.resid = c.take<float>(M * D);
  w.qkv = c.take<float>(M * 3 * D);
  w.pooled = c.take<float>((size_t)B * t->cfg.projection);
  w.xn = c.planes(M * D);
  w.ctx = c.planes(M * D);
  w.mid = c.planes(M * I);
  w.bytes = c.bytes();
  return w;
}

static void text_expected(sf_text* t) {
  const sf_text_config& c = t->cfg;
  const int64_t D = c.hidden, I = c.intermediate;
  t->weights.noun = "text model";
  t->weights.prefix = "text_model.";
  t->weights.dtype_msg = "sf_text_load_tensor: dtype %d unsupported (fp32, fp64, bf16)";
  SfWeightStore& w = t->weights;
  w.expected["embeddings.token_embedding.weight"] = {c.vocab, D};
  w.expected["embeddings.position_embedding.weight"] = {c.positions, D};
  for (int i = 0; i < c.layers; ++i) {
    const std::string p = "encoder.layers." + std::to_string(i) + ".";
    w.expect_affine(p + "layer_norm1.", D);
    w.expect_affine(p + "layer_norm2.", D);
    for (const char* a : {"q_proj.", "k_proj.", "v_proj.", "out_proj."}) w.expect_linear(p + "self_attn." + a, D, D);
    w.expect_linear(p + "mlp.fc1.", I, D);
    w.expect_linear(p + "mlp.fc2.", D, I);
  }
  w.expect_affine("final_layer_norm.", D);
  w.expect_linear("head.", c.projection, D);
}

extern "C" int sf_text_create(const sf_text_config* cfg, int device, sf_text** out) {
  if (!cfg || !out) return sf_set_err(SF_ERR_INVALID, "sf_text_create: null argument");
  const sf_text_config& c = *cfg;
  if (c.hidden <= 0 || c.heads <= 0 || c.hidden % c.heads)
    return sf_set_err(SF_ERR_INVALID, "sf_text_create: hidden %d not divisible by heads %d", c.hidden, c.heads);
  const int hd = c.hidden / c.heads;
  if (hd < 8 || hd > 128 || hd % 8)
    return sf_set_err(SF_ERR_INVALID, "sf_text_create: head_dim %d unsupported: multiples of 8 from 8 to 128", hd);
  if (c.hidden % 64) return sf_set_err(SF_ERR_INVALID, "sf_text_create: hidden %d must be a multiple of 64 (the GEMM kernels' k-step)", c.hidden);
  if (c.hidden > SF_TEXT_MAX_D) return sf_set_err(SF_ERR_CAPACITY, "sf_text_create: hidden %d > %d (the pooled head keeps 8 rows in LDS)", c.hidden, SF_TEXT_MAX_D);
  if (c.vocab <= 0 || c.layers <= 0 || c.intermediate <= 0 || c.projection <= 0)
    return sf_set_err(SF_ERR_INVALID, "sf_text_create: vocab, layers, intermediate and projection must be positive");
  if (c.positions <= 0) return sf_set_err(SF_ERR_INVALID, "sf_text_create: positions must be positive");
  if (c.positions > SF_TEXT_MAX_L)
    return sf_set_err(SF_ERR_CAPACITY, "sf_text_create: %d positions > %d (the attention kernel stages a caption's K and V in LDS)", c.positions, SF_TEXT_MAX_L);
  if (c.act < 0 || c.act > 2) return sf_set_err(SF_ERR_INVALID, "sf_text_create: unsupported act code %d (0 erf GELU, 1 tanh GELU, 2 ReLU)", c.act);
  if (!(c.eps > 0.f)) return sf_set_err(SF_ERR_INVALID, "sf_text_create: eps must be positive");
  sf_text* t = new sf_text();
  t->cfg = c;
  t->device = device;
  t->D = c.hidden;
  t->I = (c.intermediate + 63) / 64 * 64;
  t->hd = hd;
  text_expected(t);
  *out = t;
  return SF_OK;
}

extern "C" void sf_text_destroy(sf_text* t) { delete t; }

extern "C" int sf_text_load_tensor(sf_text* t, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
  return sf_model_load_tensor(t, "sf_text_load_tensor", key, host_ptr, dtype, shape, ndim);
}

extern "C" int sf_text_missing_weights(sf_text* t) { return sf_model_missing_weights(t); }

extern "C" int sf_text_finalize(sf_text* t, int compute) {
  SF_TRY(sf_model_begin_finalize(t, compute));
  const int D = t->D, I = t->I, Ir = t->cfg.intermediate;
  const bool split = compute == SF_COMPUTE_BF16X3;
  SfDeviceAllocs& dev = t->dev;
  auto H = [&](const std::string& k) -> std::vector<float>& { return t->weights.data(k); };
  SF_TRY(dev.upload(H("embeddings.token_embedding.weight"), &t->tok));
  SF_TRY(dev.upload(H("embeddings.position_embedding.weight"), &t->pos));
  t->layers.assign(t->cfg.layers, TextLayer());
  for (int i = 0; i < t->cfg.layers; ++i) {
    const std::string p = "encoder.layers." + std::to_string(i) + ".";
    TextLayer& l = t->layers[i];
    SF_TRY(sf_upload_ln(dev, t->weights, p + "layer_norm1.", &l.ln1));
    SF_TRY(sf_upload_ln(dev, t->weights, p + "layer_norm2.", &l.ln2));
    {   // q_proj | k_proj | v_proj -> one [3D, D] Linear
      std::vector<float> w, b;
      w.reserve((size_t)3 * D * D); b.reserve((size_t)3 * D);
      for (const char* a : {"q_proj", "k_proj", "v_proj"}) {
        const std::vector<float>& wa = H(p + "self_attn." + a + ".weight");
        const std::vector<float>& ba = H(p + "self_attn." + a + ".bias");
        w.insert(w.end(), wa.begin(), wa.end());
        b.insert(b.end(), ba.begin(), ba.end());
      }
      SF_TRY(sf_upload_linear(dev, w, &b, 3 * D, D, 3 * D, split, &l.qkv));
    }
    SF_TRY(sf_upload_linear(dev, H(p + "self_attn.out_proj.weight"), &H(p + "self_attn.out_proj.bias"), D, D, D, split, &l.out));
    {   // intermediate_size zero-padded to I: rows of fc1 (and their bias), columns of fc2
      std::vector<float> w1((size_t)I * D, 0.f), b1((size_t)I, 0.f), w2((size_t)D * I, 0.f);
      const std::vector<float>& a1 = H(p + "mlp.fc1.weight");
      const std::vector<float>& c1 = H(p + "mlp.fc1.bias");
      const std::vector<float>& a2 = H(p + "mlp.fc2.weight");
      std::copy(a1.begin(), a1.end(), w1.begin());
      std::copy(c1.begin(), c1.end(), b1.begin());
      for (int r = 0; r < D; ++r) std::copy(a2.begin() + (size_t)r * Ir, a2.begin() + (size_t)(r + 1) * Ir, w2.begin() + (size_t)r * I);
      SF_TRY(sf_upload_linear(dev, w1, &b1, I, D, I, split, &l.fc1));
      SF_TRY(sf_upload_linear(dev, w2, &H(p + "mlp.fc2.bias"), D, I, D, split, &l.fc2));
    }
  }
  SF_TRY(sf_upload_ln(dev, t->weights, "final_layer_norm.", &t->final_ln));
  SF_TRY(dev.upload(H("head.weight"), &t->head_w));
  SF_TRY(dev.upload(H("head.bias"), &t->head_b));
  t->finalized = true;
  return SF_OK;
}

static int text_check_call(const sf_text* t, int B, int L) {
  if (!t) return sf_set_err(SF_ERR_INVALID, "null handle");
  SF_TRY(sf_model_check_finalized(t, "sf_text"));
  if (B <= 0 || L <= 0) return sf_set_err(SF_ERR_INVALID, "sf_text: bad shape B=%d L=%d", B, L);
  if (L > t->cfg.positions) return sf_set_err(SF_ERR_CAPACITY, "sf_text: sequence length %d > %d positions", L, t->cfg.positions);
  if ((size_t)B * L * 3 * t->D > (size_t)0x7fffffff || (size_t)B * L * t->I > (size_t)0x7fffffff)
    return sf_set_err(SF_ERR_CAPACITY, "sf_text: %d captions of %d tokens exceed 2^31 - 1 elements per activation; encode in chunks", B, L);
  return SF_OK;
}

extern "C" int sf_text_workspace_bytes(sf_text* t, int B, int L, size_t* out) {
  if (!out) return sf_set_err(SF_ERR_INVALID, "null argument");
  int rc = text_check_call(t, B, L);
  if (rc) return rc;
  *out = text_carve(t, nullptr, B, L).bytes;
  return SF_OK;
}

// group == 0: pooled_out [B, P]; group > 0: the normalised means of `group` consecutive captions, [B / group, P]
static int text_forward(sf_text* t, const int32_t* ids, const uint8_t* mask, int B, int L, int group, float* last_hidden, float* pooled_out,
                        void* workspace, size_t workspace_bytes, hipStream_t s) {
  int rc = text_check_call(t, B, L);
  if (rc) return rc;
  if (!ids || !pooled_out || !workspace) return sf_set_err(SF_ERR_INVALID, "sf_text_forward: null buffer");
  if (group < 0 || (group && B % group)) return sf_set_err(SF_ERR_INVALID, "sf_text: %d captions are not whole groups of %d", B, group);
  const TextWorkspace ws = text_carve(t, workspace, B, L);
  SF_TRY(sf_check_workspace("sf_text_forward", "sf_text_workspace_bytes", workspace, workspace_bytes, ws.bytes));
  const sf_text_config& c = t->cfg;
  const int D = t->D, M = B * L;
  const SfLinearCaller lin{t->compute == SF_COMPUTE_BF16X3, c.act, s};
  HIP_TRY(text_launch_embed(ids, t->tok, t->pos, ws.resid, M, L, D, c.vocab, s));
  for (const TextLayer& l : t->layers) {
    HIP_TRY(sf_launch_layernorm(ws.resid, l.ln1.g, l.ln1.b, nullptr, ws.xn.hi, ws.xn.lo, M, D, c.eps, s));
    HIP_TRY(lin.f32(l.qkv, ws.xn, M, ws.qkv));
    {
      SfTextAttn a;
      memset(&a, 0, sizeof(a));
      a.qkv = ws.qkv; a.mask = mask; a.ctx_hi = ws.ctx.hi; a.ctx_lo = ws.ctx.lo;
      a.B = B; a.L = L; a.heads = c.heads; a.D = D; a.scale = 1.0f / sqrtf((float)t->hd);
      HIP_TRY(text_launch_attention(a, s));
    }
    HIP_TRY(lin.resid(l.out, ws.ctx, M, ws.resid, ws.resid));
    HIP_TRY(sf_launch_layernorm(ws.resid, l.ln2.g, l.ln2.b, nullptr, ws.xn.hi, ws.xn.lo, M, D, c.eps, s));
    HIP_TRY(lin.planes(l.fc1, ws.xn, M, ws.mid, true));
    HIP_TRY(lin.resid(l.fc2, ws.mid, M, ws.resid, ws.resid));
  }
  if (last_hidden) HIP_TRY(sf_launch_layernorm(ws.resid, t->final_ln.g, t->final_ln.b, last_hidden, nullptr, nullptr, M, D, c.eps, s));
  HIP_TRY(text_launch_pool(ws.resid, B, L, D, t->final_ln.g, t->final_ln.b, c.eps, t->head_w, t->head_b, c.projection, group, pooled_out,
                           ws.pooled, s));
  return SF_OK;
}

extern "C" int sf_text_forward(sf_text* t, const int32_t* ids_dev, const uint8_t* mask_dev, int B, int L, float* last_hidden_dev,
                               float* pooled_dev, void* workspace_dev, size_t workspace_bytes, sf_stream stream) {
  return text_forward(t, ids_dev, mask_dev, B, L, 0, last_hidden_dev, pooled_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

extern "C" int sf_text_forward_groups(sf_text* t, const int32_t* ids_dev, const uint8_t* mask_dev, int B, int L, int group, float* table_dev,
                                      void* workspace_dev, size_t workspace_bytes, sf_stream stream) {
  if (group <= 0) return sf_set_err(SF_ERR_INVALID, "sf_text_forward_groups: group must be positive");
  return text_forward(t, ids_dev, mask_dev, B, L, group, nullptr, table_dev, workspace_dev, workspace_bytes, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------
// single operators (parity tests)
// ------------------------------------------------------------------------------------------------
extern "C" int sf_op_text_attention(const float* qkv_dev, const uint8_t* mask_dev, float* ctx_dev, int B, int L, int heads, int head_dim,
                                    sf_stream stream) {
  if (!qkv_dev || !ctx_dev) return sf_set_err(SF_ERR_INVALID, "sf_op_text_attention: null buffer");
  if (B <= 0 || heads <= 0) return sf_set_err(SF_ERR_INVALID, "sf_op_text_attention: bad shape B=%d heads=%d", B, heads);
  if (L < 1 || L > SF_TEXT_MAX_L) return sf_set_err(SF_ERR_CAPACITY, "sf_op_text_attention: sequence length %d outside 1..%d", L, SF_TEXT_MAX_L);
  if (head_dim < 8 || head_dim > 128 || head_dim % 8) return sf_set_err(SF_ERR_INVALID, "sf_op_text_attention: head_dim must be a multiple of 8 in 8..128");
  if (((uintptr_t)qkv_dev & 15) || ((uintptr_t)ctx_dev & 15)) return sf_set_err(SF_ERR_INVALID, "sf_op_text_attention: buffers must be 16-byte aligned");
  SfTextAttn a;
  memset(&a, 0, sizeof(a));
  a.qkv = qkv_dev; a.mask = mask_dev; a.ctx_f32 = ctx_dev;
  a.B = B; a.L = L; a.heads = heads; a.D = heads * head_dim; a.scale = 1.0f / sqrtf((float)head_dim);
  HIP_TRY(text_launch_attention(a, (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_op_text_pool(const float* x_dev, int B, int L, int D, const float* gamma_dev, const float* beta_dev, float eps,
                               const float* w_dev, const float* bias_dev, int P, int group, float* out_dev, float* scratch_dev,
                               sf_stream stream) {
  if (!x_dev || !w_dev || !out_dev || (!gamma_dev) != (!beta_dev)) return sf_set_err(SF_ERR_INVALID, "sf_op_text_pool: null buffer");
  if (B <= 0 || L <= 0 || D <= 0 || P <= 0 || D % 4) return sf_set_err(SF_ERR_INVALID, "sf_op_text_pool: bad shape B=%d L=%d D=%d P=%d (D a multiple of 4)", B, L, D, P);
  if (D > SF_TEXT_MAX_D) return sf_set_err(SF_ERR_CAPACITY, "sf_op_text_pool: width %d > %d", D, SF_TEXT_MAX_D);
  if (group < 0 || (group && (B % group || !scratch_dev)))
    return sf_set_err(SF_ERR_INVALID, "sf_op_text_pool: group %d needs B %% group == 0 and a scratch buffer of B * P floats", group);
  if (((uintptr_t)x_dev & 15) || ((uintptr_t)w_dev & 15)) return sf_set_err(SF_ERR_INVALID, "sf_op_text_pool: x and w must be 16-byte aligned");
  HIP_TRY(text_launch_pool(x_dev, B, L, D, gamma_dev, beta_dev, eps, w_dev, bias_dev, P, group, out_dev, scratch_dev, (hipStream_t)stream));
  return SF_OK;
}
