// Online action detection: the reference's streaming LSTR detector (downstream/OAD, models/lstr.py:255-355 LSTRStream.stream_inference,
// transformer/transformer.py, transformer/multihead_attention.py, feature_head.py), inference only, several independent streams per call.
// The Linears run on the encoder's GEMM launchers (sf_launch_gemm, both compute modes, weights rounded / split ONCE at finalize); this
// file adds the kernels the encoder never needed, the launch sequence, the per-stream device state and the C entry points.
//
//   sf_oad_attention_kernel    ctx = softmax(scale q (k + k_pos)^T + mask (+ causal)) (v + v_pos), fp32, Tq != Tk, head_dim any multiple of 8
//                              up to 256.  One workgroup = ONE wave = one 16-query tile of one (stream, head): the grid is streams x heads x
//                              ceil(Tq / 16), so a single stream of 4 heads x 32 work frames still spreads over 8 workgroups.  Arithmetic and
//                              lane layout are those of sf_text_attention_kernel (v_mfma_f32_16x16x4_f32, exact fp32 products, running max /
//                              sum over 16-key tiles, two xor-shuffles per row statistic).  The key tile is 16 keys = one MFMA tile: K + k_pos
//                              and V + v_pos of the tile are summed while they are staged as fp32 images [16][head_dim + 4] in LDS, 33 KB at
//                              head_dim 256 (four workgroups per CU in 160 KB); a larger tile would buy a single wave nothing.  Keys come
//                              from a ring: key j of stream s is row (ring_start[s] + j) mod Tk of the stream's block, while k_pos / v_pos
//                              and the mask are indexed by the window position j.  A key whose mask is -inf is staged as ZERO rows and
//                              scored -inf: it contributes exactly zero whatever its rows hold.  A query without a visible key gets zeros
//                              (never a division by a zero sum).  One owner per output element, fixed order: bit-reproducible.
//   (sf_rowwise.hip)           the row pass sf_row_kernel, through oad_launch_row: [ReLU] [LN] (x [+ r[row % r_mod]]) [+ pe[row % pe_mod]] ->
//                              fp32 and bf16 hi / lo planes (the next GEMM's operand).  Serves the post-LN residual rows
//                              LN(x + sublayer(x)), in place (y == r), the feature head ReLU(LN(x)) (+ pe) and the identity feature
//                              head (x + pe).
//   sf_oad_rows_kernel         row gather / scatter by a table passed by value (fp32 -> fp32 and / or planes): the new K | V rows into the
//                              rings, stage 0's result into the state, the cached compressed memory of a call's streams into one matrix,
//                              query embeddings replicated per stream.
//   sf_oad_scores_kernel       [rows, Cp] (classifier columns padded for the GEMM) -> [rows, C], optional softmax; one wave per row.
//
// Decomposition of stage 0 (multihead_attention.py:182-280): k = W_k x WITHOUT bias, k_pos = W_k pe[i] + b_k, likewise v; a projected row
// never changes while it ages, only its positional addend does.  The state keeps W_k x | W_v x per stream in a ring; a step projects
// only the new sample.  What does not depend on the input is computed once in sf_oad_finalize: the stage-0 queries' self-attention +
// norm1 (tgt0), their q projection (q0), and k_pos | v_pos.
#include "sf_handle.h"

typedef __attribute__((ext_vector_type(4))) float of4_t;

#define OAD_MAX_D 4096
#define OAD_MAX_S SF_OAD_MAX_CALL_STREAMS

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
struct SfOadAttn {
  const float* q; const float* k; const float* v;      // fp32 rows; a head's columns at h * hd
  const float* kpos; const float* vpos;                // [Tk, pos_pitch] by window position, or null
  const float* mask;                                   // additive rows of Tk floats, or null
  float* ctx_f32; bf16_t* ctx_hi; bf16_t* ctx_lo;      // [streams * Tq, heads * hd]; any of them null
  long long q_sstride;                                 // elements between the streams' query blocks (0: shared queries)
  int q_pitch, kv_pitch, pos_pitch;                    // elements per row
  int streams, Tq, Tk, heads, hd, causal;
  float scale;
  int kv_row0[OAD_MAX_S];                              // first row of stream s's K / V block
  int ring_start[OAD_MAX_S];                           // row of the oldest key inside the block
  int mask_row[OAD_MAX_S];                             // mask row of stream s
};

SF_DEVICE of4_t oa_mfma(float a, float b, of4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

template <int NT>      // NT = ceil(head_dim / 16) <= 16
__global__ __launch_bounds__(64) void sf_oad_attention_kernel(SfOadAttn p) {
  extern __shared__ __attribute__((aligned(16))) float oa_smem[];
  const int HD = p.hd, LD = HD + 4, HDQ = HD >> 2, Tq = p.Tq, Tk = p.Tk;
  float* kt = oa_smem;
  float* vt = kt + 16 * LD;
  const int qtiles = (Tq + 15) >> 4;
  int b = blockIdx.x;
  const int qt = b % qtiles; b /= qtiles;
  const int h = b % p.heads, s = b / p.heads;
  const int lane = threadIdx.x, l15 = lane & 15, g = lane >> 4;
  const int qi = qt * 16 + l15, qrow = qi < Tq ? qi : Tq - 1;      // lanes past Tq repeat the last query and store nothing
  const int off = Tk - Tq;                                          // causal: key j visible iff j <= query + off
  float qreg[NT * 4];
  {
    // k-index (g, i) of the score MFMAs is dim 4 i + g: the four g-groups of a wave read four CONSECUTIVE LDS banks of a K row (and
    // the 16 rows sit 4 banks apart through the + 4 pad) instead of the same bank, which dim g * HDQ + i gave at head_dim 256
    const float* q = p.q + (size_t)s * p.q_sstride + (size_t)qrow * p.q_pitch + h * HD + g;
#pragma unroll
    for (int i = 0; i < NT * 4; ++i) qreg[i] = i < HDQ ? q[4 * i] : 0.f;
  }
  const float* mrow = p.mask ? p.mask + (size_t)p.mask_row[s] * Tk : nullptr;
  const size_t kv0 = (size_t)p.kv_row0[s];
  const int start = p.ring_start[s];
  of4_t o_acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) o_acc[t] = (of4_t){0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  int kend = Tk;
  if (p.causal) { const int e = qt * 16 + 16 + off; kend = e < Tk ? e : Tk; }      // tiles no query of this tile can see are skipped
  for (int k0 = 0; k0 < kend; k0 += 16) {
    __syncthreads();
    // ---- K + k_pos and V + v_pos of 16 keys; rows past Tk and masked keys are zero (0 * p stays finite) ----
    for (int c = lane; c < 16 * HDQ; c += 64) {
      const int row = c / HDQ, cc = c - row * HDQ, key = k0 + row;
      of4_t kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
      if (key < Tk && !(mrow && mrow[key] == -INFINITY)) {
        int slot = start + key;
        slot = slot >= Tk ? slot - Tk : slot;
        const size_t e = (kv0 + slot) * p.kv_pitch + h * HD + cc * 4;
        kv = *reinterpret_cast<const of4_t*>(p.k + e);
        vv = *reinterpret_cast<const of4_t*>(p.v + e);
        if (p.kpos) {
          const size_t ep = (size_t)key * p.pos_pitch + h * HD + cc * 4;
          kv += *reinterpret_cast<const of4_t*>(p.kpos + ep);
          vv += *reinterpret_cast<const of4_t*>(p.vpos + ep);
        }
      }
      *reinterpret_cast<of4_t*>(kt + row * LD + cc * 4) = kv;
      *reinterpret_cast<of4_t*>(vt + row * LD + cc * 4) = vv;
    }
    __syncthreads();
    // S^T tile: keys k0 + l15 (A operand) x queries (B operand); lane (query l15, g) receives keys k0 + 4 g + r
    // eight independent accumulation chains, summed as a tree: one chain of head_dim / 4 dependent fp32 adds (64 at head_dim 256, on raw
    // dot products of magnitude ~ 50) lost 2 - 3 x what a blocked sum loses, and the score's error is the softmax weight's relative error
    of4_t s4;
    {
      of4_t part[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) part[j] = (of4_t){0.f, 0.f, 0.f, 0.f};
      const float* kr = kt + l15 * LD + g;
#pragma unroll
      for (int i = 0; i < NT * 4; ++i)
        if (i < HDQ) part[i & 7] = oa_mfma(kr[4 * i], qreg[i], part[i & 7]);
      s4 = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
    }
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = k0 + 4 * g + r;
      bool ok = key < Tk && (!p.causal || key <= qrow + off);
      float mk = 0.f;
      if (ok && mrow) { mk = mrow[key]; ok = mk != -INFINITY; }
      s4[r] = ok ? fmaf(s4[r], p.scale, mk) : -INFINITY;
      mx = fmaxf(mx, s4[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    // no visible key so far (m_new = -inf): keep zeros, exp(-inf - (-inf)) would be NaN.  expf, not v_exp_f32 on a product with log2(e):
    // the product's rounding at |score - max| ~ 10 alone costs as much as everything else in this kernel, and the work here is tiny
    const float corr = m_new == -INFINITY ? 1.f : expf(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s4[r] = m_new == -INFINITY ? 0.f : expf(s4[r] - m_new);
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
        const float v = d < HD ? vt[(4 * g + r) * LD + d] : 0.f;
        o_acc[t] = oa_mfma(v, s4[r], o_acc[t]);
      }
    }
  }
  if (qi >= Tq) return;
  const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;      // no visible key: zeros
  const size_t ob = ((size_t)s * Tq + qi) * ((size_t)p.heads * HD) + h * HD;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int d = t * 16 + 4 * g;
    if (d < HD) {                                   // HD % 4 == 0: the four dims of a lane are all inside or all outside
      const of4_t o = o_acc[t] * inv;
      if (p.ctx_f32) *reinterpret_cast<of4_t*>(p.ctx_f32 + ob + d) = o;
      if (p.ctx_hi) store_planes4(o, p.ctx_hi, p.ctx_lo, ob + d);
    }
  }
}

struct SfOadRows { int n; int src[OAD_MAX_S], dst[OAD_MAX_S], cnt[OAD_MAX_S]; };      // entry e: cnt rows from src row to dst row

// grid (x, entries)
__global__ __launch_bounds__(256) void sf_oad_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, bf16_t* __restrict__ hi,
                                                          bf16_t* __restrict__ lo, int D4, SfOadRows t) {
  const int e = blockIdx.y;
  const unsigned total = (unsigned)t.cnt[e] * (unsigned)D4;
  const size_t s0 = (size_t)t.src[e] * D4, d0 = (size_t)t.dst[e] * D4;
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const of4_t v = reinterpret_cast<const of4_t*>(src)[s0 + i];
    if (dst) reinterpret_cast<of4_t*>(dst)[d0 + i] = v;
    if (hi) store_planes4(v, hi, lo, (d0 + i) * 4);
  }
}

__global__ __launch_bounds__(256) void sf_oad_scores_kernel(const float* __restrict__ in, float* __restrict__ out, int rows, int Cp, int C,
                                                            int probs) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* x = in + (size_t)row * Cp;
  float* y = out + (size_t)row * C;
  if (!probs) {
    for (int c = lane; c < C; c += 64) y[c] = x[c];
    return;
  }
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, x[c]);
  m = wave_max(m);
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(x[c] - m);
  s = wave_sum(s);
  for (int c = lane; c < C; c += 64) y[c] = expf(x[c] - m) / s;
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// every pointer 16-byte aligned (planes 8), pitches multiples of 4, hd % 8 == 0 in 8..256: checked here
static hipError_t oad_launch_attention(const SfOadAttn& p, hipStream_t s) {
  if (p.streams < 1 || p.streams > OAD_MAX_S || p.Tq < 1 || p.Tk < 1 || p.heads < 1) return hipErrorInvalidValue;
  if (p.hd < 8 || p.hd > 256 || p.hd % 8) return hipErrorInvalidValue;
  if (!p.q || !p.k || !p.v || (!p.kpos) != (!p.vpos)) return hipErrorInvalidValue;
  if (((uintptr_t)p.q | (uintptr_t)p.k | (uintptr_t)p.v | (uintptr_t)p.kpos | (uintptr_t)p.vpos | (uintptr_t)p.ctx_f32) & 15) return hipErrorInvalidValue;
  if (((uintptr_t)p.ctx_hi | (uintptr_t)p.ctx_lo) & 7) return hipErrorInvalidValue;
  if ((p.q_pitch | p.kv_pitch | p.pos_pitch | (int)(p.q_sstride & 3)) & 3) return hipErrorInvalidValue;
  for (int i = 0; i < p.streams; ++i)
    if (p.ring_start[i] < 0 || p.ring_start[i] >= p.Tk || p.kv_row0[i] < 0 || p.mask_row[i] < 0) return hipErrorInvalidValue;
  const int64_t blocks = (int64_t)p.streams * p.heads * ((p.Tq + 15) / 16);
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const size_t lds = (size_t)2 * 16 * (p.hd + 4) * sizeof(float);      // 33 KB at head_dim 256
  const dim3 grid((unsigned)blocks), block(64);
  switch ((p.hd + 15) / 16) {
#define OA_CASE(E) case E: return sf_launch(sf_oad_attention_kernel<E>, grid, block, lds, s, p);
    OA_CASE(1) OA_CASE(2) OA_CASE(3) OA_CASE(4) OA_CASE(5) OA_CASE(6) OA_CASE(7) OA_CASE(8)
    OA_CASE(9) OA_CASE(10) OA_CASE(11) OA_CASE(12) OA_CASE(13) OA_CASE(14) OA_CASE(15) OA_CASE(16)
#undef OA_CASE
    default: return hipErrorInvalidValue;
  }
}

static hipError_t oad_launch_row(const SfRowArgs& p, hipStream_t s) {
  if (p.rows <= 0) return hipSuccess;
  if (p.D < 4 || p.D % 4 || p.D > OAD_MAX_D || !p.x || (p.pe && p.pe_mod < 1) || (!p.gamma) != (!p.beta)) return hipErrorInvalidValue;
  return sf_launch_row(p, s);
}

static hipError_t oad_launch_rows(const float* src, float* dst, bf16_t* hi, bf16_t* lo, int D, const SfOadRows& t, hipStream_t s) {
  if (t.n <= 0) return hipSuccess;
  if (t.n > OAD_MAX_S || D % 4) return hipErrorInvalidValue;
  int most = 0;
  for (int i = 0; i < t.n; ++i) most = t.cnt[i] > most ? t.cnt[i] : most;
  if (most <= 0) return hipSuccess;
  unsigned gx = (unsigned)(((size_t)most * (D / 4) + 255) / 256);
  if (gx > 256u) gx = 256u;
  return sf_launch(sf_oad_rows_kernel, dim3(gx, (unsigned)t.n), dim3(256), 0, s, src, dst, hi, lo, D / 4, t);
}

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
namespace {
struct OadLayer {
  bool decoder = false;
  SfDevLinear self_in, self_out, cross_q, cross_kv, cross_out, lin1, lin2;
  SfDevLN n1, n2, n3;
};
struct OadModule {
  int queries = -1;                    // -1: encoder layers
  std::vector<OadLayer> layers;
  bool norm = false;
  SfDevLN fn;
  const float* qw = nullptr;           // enc_queries.j.weight [queries, d]
};
struct OadAct { float* f = nullptr; SfPlanes p; };      // an activation [rows, d]: fp32 + the GEMM operand planes
struct OadWorkspace {
  OadAct a[3];                         // rotating activations [R, d]
  SfPlanes in;                         // split inputs [R, d_in]
  float *tmp, *qkv, *q, *kv;           // GEMM outputs [R, d], [R, 3d], [R, d], [R, 2d]
  SfPlanes ctx, mid;                   // [R, d], [R, ffn]
  float* scores;                       // [n W, Cp]
  size_t bytes;
};
}  // namespace

struct sf_oad : SfModelHandle {
  sf_oad_config cfg;
  int d = 0, hd = 0, Cp = 0, Q0 = 0, maxT = 0;      // Cp: classes padded to 16 columns; maxT: longest sequence of any stage
  SfDevLinear fh_long, fh_work, cls;
  SfDevLN fh_long_ln, fh_work_ln;
  std::vector<OadModule> enc;
  OadModule dec;
  const float* pe = nullptr;           // [L + W, d]
  float* pos_kv = nullptr;             // [L, 2d]: k_pos | v_pos of stage 0
  OadAct tgt0;                         // [Q0, d] stage-0 queries after self-attention + norm1
  float* q0 = nullptr;                 // [Q0, d] their q projection
};

struct sf_oad_state {
  sf_oad* det = nullptr;
  int streams = 0;
  float* ring = nullptr;               // [streams, L, 2d]
  float* mem0 = nullptr;               // [streams, Q0, d]
  std::vector<int> head, fill;         // head: slot of the oldest sample
};

static void oad_expect_layer(sf_oad* h, const std::string& p, bool decoder) {
  const int64_t d = h->d, F = h->cfg.ffn;
  SfWeightStore& w = h->weights;
  for (const char* a : {"self_attn.", "multihead_attn."}) {
    if (!decoder && a[0] == 'm') continue;
    w.expected[p + a + "in_proj_weight"] = {3 * d, d};
    w.expected[p + a + "in_proj_bias"] = {3 * d};
    w.expect_linear(p + a + "out_proj.", d, d);
  }
  w.expect_linear(p + "linear1.", F, d);
  w.expect_linear(p + "linear2.", d, F);
  w.expect_affine(p + "norm1.", d);
  w.expect_affine(p + "norm2.", d);
  if (decoder) w.expect_affine(p + "norm3.", d);
}

extern "C" int sf_oad_create(const sf_oad_config* cfg, int device, sf_oad** out) {
  if (!cfg || !out) return sf_set_err(SF_ERR_INVALID, "sf_oad_create: null argument");
  const sf_oad_config& c = *cfg;
  if (c.d_in <= 0 || c.d_in % 64 || c.d_model <= 0 || c.d_model % 64 || c.ffn <= 0 || c.ffn % 64)
    return sf_set_err(SF_ERR_INVALID, "sf_oad_create: d_in %d, d_model %d and ffn %d must be positive multiples of 64 (the GEMM kernels' k-step)", c.d_in, c.d_model, c.ffn);
  if (c.d_model > OAD_MAX_D || c.d_in > OAD_MAX_D) return sf_set_err(SF_ERR_CAPACITY, "sf_oad_create: d_model %d / d_in %d > %d", c.d_model, c.d_in, OAD_MAX_D);
  if (!c.linear_enabled && c.d_in != c.d_model) return sf_set_err(SF_ERR_INVALID, "sf_oad_create: LINEAR_ENABLED False needs d_model == d_in (%d != %d)", c.d_model, c.d_in);
  if (c.heads <= 0 || c.d_model % c.heads) return sf_set_err(SF_ERR_INVALID, "sf_oad_create: d_model %d not divisible by heads %d", c.d_model, c.heads);
  const int hd = c.d_model / c.heads;
  if (hd < 8 || hd > 256 || hd % 8) return sf_set_err(SF_ERR_INVALID, "sf_oad_create: head_dim %d unsupported: multiples of 8 from 8 to 256", hd);
  if (c.long_samples < 1 || c.work_samples < 1 || c.classes < 1) return sf_set_err(SF_ERR_INVALID, "sf_oad_create: long_samples, work_samples and classes must be positive");
  if (c.act != 0 && c.act != 2) return sf_set_err(SF_ERR_INVALID, "sf_oad_create: act %d (0 erf GELU, 2 ReLU)", c.act);
  if (c.enc_modules < 1 || c.enc_modules > SF_OAD_MAX_ENC_MODULES) return sf_set_err(SF_ERR_INVALID, "sf_oad_create: %d enc_modules outside 1..%d", c.enc_modules, SF_OAD_MAX_ENC_MODULES);
  if (c.enc_queries[0] < 1) return sf_set_err(SF_ERR_INVALID, "sf_oad_create: enc_modules[0] needs queries (the stream path compresses the long memory with them)");
  if (c.enc_layers[0] != 1) return sf_set_err(SF_ERR_INVALID, "sf_oad_create: enc_modules[0] has %d layers; the stream path takes exactly one", c.enc_layers[0]);
  for (int j = 0; j < c.enc_modules; ++j)
    if ((c.enc_queries[j] < 1 && c.enc_queries[j] != -1) || c.enc_layers[j] < 1) return sf_set_err(SF_ERR_INVALID, "sf_oad_create: enc_modules[%d] = [%d, %d]", j, c.enc_queries[j], c.enc_layers[j]);
  if (c.dec_layers < 1) return sf_set_err(SF_ERR_INVALID, "sf_oad_create: dec_layers %d", c.dec_layers);
  if (!(c.eps > 0.f)) return sf_set_err(SF_ERR_INVALID, "sf_oad_create: eps must be positive");
  sf_oad* h = new sf_oad();
  h->cfg = c;
  h->device = device;
  h->d = c.d_model;
  h->hd = hd;
  h->Cp = (c.classes + 15) / 16 * 16;
  h->Q0 = c.enc_queries[0];
  h->maxT = c.long_samples > c.work_samples ? c.long_samples : c.work_samples;
  const int64_t d = h->d;
  h->weights.noun = "detector";
  h->weights.dtype_msg = "sf_oad_load_tensor: dtype %d unsupported (fp32, fp64, bf16)";
  SfWeightStore& w = h->weights;
  auto& e = w.expected;
  if (c.linear_enabled)
    for (const char* fh : {"feature_head_long.", "feature_head_work."}) {
      const std::string p = std::string(fh) + "visual_linear.";
      w.expect_linear(p + "0.", d, c.d_in);
      w.expect_affine(p + "1.", d);
    }
  for (int j = 0; j < c.enc_modules; ++j) {
    const std::string m = "enc_modules." + std::to_string(j) + ".";
    if (c.enc_queries[j] > 0) {
      e["enc_queries." + std::to_string(j) + ".weight"] = {c.enc_queries[j], d};
      if (c.enc_queries[j] > h->maxT) h->maxT = c.enc_queries[j];
    }
    for (int l = 0; l < c.enc_layers[j]; ++l) oad_expect_layer(h, m + "layers." + std::to_string(l) + ".", c.enc_queries[j] > 0);
    if (c.enc_norm[j]) w.expect_affine(m + "norm.", d);
  }
  for (int l = 0; l < c.dec_layers; ++l) oad_expect_layer(h, "dec_modules.layers." + std::to_string(l) + ".", true);
  if (c.dec_norm) w.expect_affine("dec_modules.norm.", d);
  w.expect_linear("classifier.", c.classes, d);
  e["pos_encoding.pe"] = {c.long_samples + c.work_samples, d};      // at least that many rows; [rows, 1, d] accepted
  *out = h;
  return SF_OK;
}

extern "C" void sf_oad_destroy(sf_oad* h) { delete h; }

extern "C" int sf_oad_load_tensor(sf_oad* h, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim) {
  const char* who = "sf_oad_load_tensor";
  SF_TRY(sf_model_load_args(h, who, key, host_ptr, shape, ndim));
  if (strcmp(key, "pos_encoding.pe")) return sf_model_load_tensor(h, who, key, host_ptr, dtype, shape, ndim);
  // the reference's buffer [max_len, 1, d]: the first L + W rows are kept
  const int64_t rows = h->weights.expected.at(key)[0];
  const bool ok = (ndim == 2 || (ndim == 3 && shape[1] == 1)) && shape[ndim - 1] == h->d && shape[0] >= rows;
  if (!ok) return sf_set_err(SF_ERR_INVALID, "'%s': [rows >= %lld, d_model] or [rows, 1, d_model] expected", key, (long long)rows);
  std::string err;
  const int rc = h->weights.stage(key, host_ptr, dtype, (size_t)rows * h->d, shape, ndim, &err);
  return sf_model_staged(h, rc, err);
}

extern "C" int sf_oad_missing_weights(sf_oad* h) { return sf_model_missing_weights(h); }

// [N, K] weight + bias -> the planes of the handle's compute mode; rows zero-padded to Np
static int oad_upload_linear(sf_oad* h, const std::vector<float>& w, const std::vector<float>& bias, int N, int K, int Np, SfDevLinear* out) {
  return sf_upload_linear(h->dev, w, &bias, N, K, Np, h->compute == SF_COMPUTE_BF16X3, out);
}

static int oad_upload_layer(sf_oad* h, const std::string& p, bool decoder, bool stage0, OadLayer* l) {
  const int d = h->d, F = h->cfg.ffn;
  auto H = [&](const std::string& k) -> std::vector<float>& { return h->weights.data(p + k); };
  l->decoder = decoder;
  SF_TRY(oad_upload_linear(h, H("self_attn.in_proj_weight"), H("self_attn.in_proj_bias"), 3 * d, d, 3 * d, &l->self_in));
  SF_TRY(oad_upload_linear(h, H("self_attn.out_proj.weight"), H("self_attn.out_proj.bias"), d, d, d, &l->self_out));
  if (decoder) {
    SfDevLinear in;
    SF_TRY(oad_upload_linear(h, H("multihead_attn.in_proj_weight"), H("multihead_attn.in_proj_bias"), 3 * d, d, 3 * d, &in));
    l->cross_q = sf_linear_rows(in, 0, d, in.bias);
    l->cross_kv = sf_linear_rows(in, d, 2 * d, stage0 ? nullptr : in.bias + d);      // stage 0: the bias belongs to k_pos | v_pos
    SF_TRY(oad_upload_linear(h, H("multihead_attn.out_proj.weight"), H("multihead_attn.out_proj.bias"), d, d, d, &l->cross_out));
  }
  SF_TRY(oad_upload_linear(h, H("linear1.weight"), H("linear1.bias"), F, d, F, &l->lin1));
  SF_TRY(oad_upload_linear(h, H("linear2.weight"), H("linear2.bias"), d, F, d, &l->lin2));
  SF_TRY(sf_upload_ln(h->dev, h->weights, p + "norm1.", &l->n1));
  SF_TRY(sf_upload_ln(h->dev, h->weights, p + "norm2.", &l->n2));
  if (decoder) SF_TRY(sf_upload_ln(h->dev, h->weights, p + "norm3.", &l->n3));
  return SF_OK;
}

static OadWorkspace oad_carve(const sf_oad* h, void* base, int n) {
  OadWorkspace w;
  SfCarver c(base, h->compute == SF_COMPUTE_BF16X3, true);      // the lo planes are set aside in either mode
  const size_t R = (size_t)n * h->maxT, d = h->d, F = h->cfg.ffn;
  for (int i = 0; i < 3; ++i) { w.a[i].f = c.take<float>(R * d); w.a[i].p = c.planes(R * d); }
  w.in = c.planes(R * h->cfg.d_in);
  w.tmp = c.take<float>(R * d); w.qkv = c.take<float>(R * 3 * d); w.q = c.take<float>(R * d); w.kv = c.take<float>(R * 2 * d);
  w.ctx = c.planes(R * d);
  w.mid = c.planes(R * F);
  w.scores = c.take<float>((size_t)n * h->cfg.work_samples * h->Cp);
  w.bytes = c.bytes();
  return w;
}

// ------------------------------------------------------------------------------------------------
// the launch sequence
// ------------------------------------------------------------------------------------------------
namespace {
struct OadRun {
  sf_oad* h;
  OadWorkspace ws;
  hipStream_t s;
  SfLinearCaller lin;

  OadRun(sf_oad* det, void* workspace, int n, hipStream_t stream)
      : h(det), ws(oad_carve(det, workspace, n)), s(stream), lin{det->compute == SF_COMPUTE_BF16X3, det->cfg.act, stream} {}
  // y = LN(x + r[row % r_mod]) -> fp32 + planes (y.f may be r)
  int add_ln(const float* x, const float* r, int r_mod, const SfDevLN& ln, const OadAct& y, int rows) {
    SfRowArgs p;
    memset(&p, 0, sizeof(p));
    p.x = x; p.r = r; p.r_mod = r_mod; p.gamma = ln.g; p.beta = ln.b; p.eps = h->cfg.eps;
    p.y = y.f; p.y_hi = y.p.hi; p.y_lo = y.p.lo; p.rows = rows; p.D = h->d;
    HIP_TRY(oad_launch_row(p, s));
    return SF_OK;
  }
  SfOadAttn attn_args(int n, int Tq, int Tk, int causal) {
    SfOadAttn a;
    memset(&a, 0, sizeof(a));
    a.ctx_hi = ws.ctx.hi; a.ctx_lo = ws.ctx.lo;
    a.streams = n; a.Tq = Tq; a.Tk = Tk; a.heads = h->cfg.heads; a.hd = h->hd; a.causal = causal;
    a.scale = 1.0f / sqrtf((float)h->hd);
    for (int i = 0; i < n; ++i) { a.kv_row0[i] = i * Tk; a.mask_row[i] = i; }
    return a;
  }
  // x = LN1(x + out_proj(attention(in_proj(x))))
  int self_block(const OadLayer& l, const OadAct& x, int n, int T, int causal) {
    const int d = h->d, M = n * T;
    HIP_TRY(lin.f32(l.self_in, x.p, M, ws.qkv));
    SfOadAttn a = attn_args(n, T, T, causal);
    a.q = ws.qkv; a.k = ws.qkv + d; a.v = ws.qkv + 2 * d;
    a.q_pitch = a.kv_pitch = 3 * d; a.q_sstride = (long long)T * 3 * d;
    HIP_TRY(oad_launch_attention(a, s));
    HIP_TRY(lin.f32(l.self_out, ws.ctx, M, ws.tmp));
    return add_ln(ws.tmp, x.f, 0, l.n1, x, M);
  }
  // x = LN2(x + out_proj(attention(q(x), kv(mem))))
  int cross_block(const OadLayer& l, const OadAct& x, int n, int T, const OadAct& mem, int Tm) {
    const int d = h->d, M = n * T;
    HIP_TRY(lin.f32(l.cross_q, x.p, M, ws.q));
    HIP_TRY(lin.f32(l.cross_kv, mem.p, n * Tm, ws.kv));
    SfOadAttn a = attn_args(n, T, Tm, 0);
    a.q = ws.q; a.q_pitch = d; a.q_sstride = (long long)T * d;
    a.k = ws.kv; a.v = ws.kv + d; a.kv_pitch = 2 * d;
    HIP_TRY(oad_launch_attention(a, s));
    HIP_TRY(lin.f32(l.cross_out, ws.ctx, M, ws.tmp));
    return add_ln(ws.tmp, x.f, 0, l.n2, x, M);
  }
  // x = LN(x + linear2(act(linear1(x))))
  int ffn_block(const OadLayer& l, const SfDevLN& ln, const OadAct& x, int M) {
    HIP_TRY(lin.planes(l.lin1, x.p, M, ws.mid, true));
    HIP_TRY(lin.f32(l.lin2, ws.mid, M, ws.tmp));
    return add_ln(ws.tmp, x.f, 0, ln, x, M);
  }
  // the module's final norm, out of place on the encoder's LayerNorm kernel
  int final_norm(const SfDevLN& ln, const OadAct& x, const OadAct& y, int M) {
    HIP_TRY(sf_launch_layernorm(x.f, ln.g, ln.b, y.f, y.p.hi, y.p.lo, M, h->d, h->cfg.eps, s));
    return SF_OK;
  }
};
}  // namespace

// Makes the handle's device current and leaves it so, as the other handles' finalize do.
extern "C" int sf_oad_finalize(sf_oad* h, int compute) {
  SF_TRY(sf_model_begin_finalize(h, compute));
  const sf_oad_config& c = h->cfg;
  const int d = h->d, L = c.long_samples, Q0 = h->Q0;
  auto H = [&](const std::string& k) -> std::vector<float>& { return h->weights.data(k); };
  if (c.linear_enabled) {
    SF_TRY(oad_upload_linear(h, H("feature_head_long.visual_linear.0.weight"), H("feature_head_long.visual_linear.0.bias"), d, c.d_in, d, &h->fh_long));
    SF_TRY(oad_upload_linear(h, H("feature_head_work.visual_linear.0.weight"), H("feature_head_work.visual_linear.0.bias"), d, c.d_in, d, &h->fh_work));
    SF_TRY(sf_upload_ln(h->dev, h->weights, "feature_head_long.visual_linear.1.", &h->fh_long_ln));
    SF_TRY(sf_upload_ln(h->dev, h->weights, "feature_head_work.visual_linear.1.", &h->fh_work_ln));
  }
  h->enc.assign(c.enc_modules, OadModule());
  for (int j = 0; j < c.enc_modules; ++j) {
    OadModule& m = h->enc[j];
    const std::string p = "enc_modules." + std::to_string(j) + ".";
    m.queries = c.enc_queries[j];
    m.norm = c.enc_norm[j] != 0;
    if (m.queries > 0) SF_TRY(h->dev.upload(H("enc_queries." + std::to_string(j) + ".weight"), &m.qw));
    m.layers.assign(c.enc_layers[j], OadLayer());
    for (int l = 0; l < c.enc_layers[j]; ++l) SF_TRY(oad_upload_layer(h, p + "layers." + std::to_string(l) + ".", m.queries > 0, j == 0, &m.layers[l]));
    if (m.norm) SF_TRY(sf_upload_ln(h->dev, h->weights, p + "norm.", &m.fn));
  }
  h->dec.norm = c.dec_norm != 0;
  h->dec.layers.assign(c.dec_layers, OadLayer());
  for (int l = 0; l < c.dec_layers; ++l) SF_TRY(oad_upload_layer(h, "dec_modules.layers." + std::to_string(l) + ".", true, false, &h->dec.layers[l]));
  if (h->dec.norm) SF_TRY(sf_upload_ln(h->dev, h->weights, "dec_modules.norm.", &h->dec.fn));
  SF_TRY(oad_upload_linear(h, H("classifier.weight"), H("classifier.bias"), c.classes, d, h->Cp, &h->cls));
  SF_TRY(h->dev.upload(H("pos_encoding.pe"), &h->pe));
  // ---- what does not depend on the input: k_pos | v_pos = W_kv pe[:L] + b_kv; tgt0 = norm1(queries + self_attn(queries)); q0 = W_q tgt0 + b_q ----
  {
    SF_TRY(h->dev.alloc((size_t)L * 2 * d * 4, (void**)&h->pos_kv));
    SF_TRY(h->dev.alloc((size_t)Q0 * d * 4, (void**)&h->tgt0.f));
    SF_TRY(h->dev.alloc((size_t)Q0 * d * 2, (void**)&h->tgt0.p.hi));
    h->tgt0.p.lo = nullptr;
    if (compute == SF_COMPUTE_BF16X3) SF_TRY(h->dev.alloc((size_t)Q0 * d * 2, (void**)&h->tgt0.p.lo));
    SF_TRY(h->dev.alloc((size_t)Q0 * d * 4, (void**)&h->q0));
    void* wsp = nullptr;
    const size_t bytes = oad_carve(h, nullptr, 1).bytes;
    HIP_TRY(hipMalloc(&wsp, bytes));
    OadRun r(h, wsp, 1, (hipStream_t)0);
    const OadLayer& l0 = h->enc[0].layers[0];
    int rc = SF_OK;
    do {
      hipError_t e;
      if ((e = sf_launch_split(h->pe, r.ws.a[0].p.hi, r.ws.a[0].p.lo, (size_t)L * d, r.s)) != hipSuccess) { rc = sf_set_err(SF_ERR_HIP, "sf_oad_finalize: %s", hipGetErrorString(e)); break; }
      SfDevLinear kvb = l0.cross_kv;
      kvb.bias = l0.cross_q.bias + d;      // the k | v rows of in_proj_bias
      if ((e = r.lin.f32(kvb, r.ws.a[0].p, L, h->pos_kv)) != hipSuccess) { rc = sf_set_err(SF_ERR_HIP, "sf_oad_finalize: %s", hipGetErrorString(e)); break; }
      SfOadRows t;
      memset(&t, 0, sizeof(t));
      t.n = 1; t.cnt[0] = Q0;
      if ((e = oad_launch_rows(h->enc[0].qw, h->tgt0.f, h->tgt0.p.hi, h->tgt0.p.lo, d, t, r.s)) != hipSuccess) { rc = sf_set_err(SF_ERR_HIP, "sf_oad_finalize: %s", hipGetErrorString(e)); break; }
      if ((rc = r.self_block(l0, h->tgt0, 1, Q0, 0))) break;
      if ((e = r.lin.f32(l0.cross_q, h->tgt0.p, Q0, h->q0)) != hipSuccess) { rc = sf_set_err(SF_ERR_HIP, "sf_oad_finalize: %s", hipGetErrorString(e)); break; }
    } while (0);
    const hipError_t es = hipDeviceSynchronize();
    (void)hipFree(wsp);
    if (rc) return rc;
    HIP_TRY(es);
  }
  h->finalized = true;
  return SF_OK;
}

extern "C" int sf_oad_workspace_bytes(sf_oad* h, int streams, size_t* out) {
  if (!h || !out) return sf_set_err(SF_ERR_INVALID, "null argument");
  SF_TRY(sf_model_check_finalized(h, "sf_oad", true));
  if (streams < 1 || streams > OAD_MAX_S) return sf_set_err(SF_ERR_INVALID, "sf_oad: %d streams per call outside 1..%d", streams, OAD_MAX_S);
  *out = oad_carve(h, nullptr, streams).bytes;
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// state
// ------------------------------------------------------------------------------------------------
extern "C" int sf_oad_state_create(sf_oad* h, int streams, sf_oad_state** out) {
  if (!h || !out) return sf_set_err(SF_ERR_INVALID, "sf_oad_state_create: null argument");
  if (streams < 1 || (int64_t)streams * h->cfg.long_samples > 0x3fffffff / (2 * h->d))
    return sf_set_err(SF_ERR_INVALID, "sf_oad_state_create: %d streams", streams);
  HIP_TRY(hipSetDevice(h->device));
  sf_oad_state* st = new sf_oad_state();
  st->det = h;
  st->streams = streams;
  st->head.assign(streams, 0);
  st->fill.assign(streams, 0);
  const size_t rb = (size_t)streams * h->cfg.long_samples * 2 * h->d * 4, mb = (size_t)streams * h->Q0 * h->d * 4;
  if (hipMalloc((void**)&st->ring, rb) != hipSuccess || hipMalloc((void**)&st->mem0, mb) != hipSuccess ||
      hipMemset(st->ring, 0, rb) != hipSuccess || hipMemset(st->mem0, 0, mb) != hipSuccess) {
    sf_oad_state_destroy(st);
    return sf_set_err(SF_ERR_HIP, "sf_oad_state_create: device allocation of %zu bytes failed", rb + mb);
  }
  *out = st;
  return SF_OK;
}

extern "C" void sf_oad_state_destroy(sf_oad_state* st) {
  if (!st) return;
  if (st->ring) (void)hipFree(st->ring);
  if (st->mem0) (void)hipFree(st->mem0);
  delete st;
}

// host integers only: an empty stream's rows are never read (its first step writes the whole window)
extern "C" int sf_oad_state_reset(sf_oad_state* st, int stream) {
  if (!st) return sf_set_err(SF_ERR_INVALID, "null state");
  if (stream >= st->streams) return sf_set_err(SF_ERR_INVALID, "sf_oad_state_reset: stream %d of %d", stream, st->streams);
  for (int i = 0; i < st->streams; ++i)
    if (stream < 0 || i == stream) { st->head[i] = 0; st->fill[i] = 0; }
  return SF_OK;
}

extern "C" int sf_oad_state_fill(sf_oad_state* st, int stream) {
  if (!st || stream < 0 || stream >= st->streams) return sf_set_err(SF_ERR_INVALID, "sf_oad_state_fill: bad state or stream");
  return st->fill[stream];
}

extern "C" int sf_oad_state_copy(sf_oad_state* dst, int ds, sf_oad_state* src, int ss, sf_stream stream) {
  if (!dst || !src || dst->det != src->det) return sf_set_err(SF_ERR_INVALID, "sf_oad_state_copy: the states belong to different detectors");
  if (ds < 0 || ds >= dst->streams || ss < 0 || ss >= src->streams) return sf_set_err(SF_ERR_INVALID, "sf_oad_state_copy: stream %d -> %d out of range", ss, ds);
  const sf_oad* h = src->det;
  const size_t rn = (size_t)h->cfg.long_samples * 2 * h->d, mn = (size_t)h->Q0 * h->d;
  if (dst != src || ds != ss) {
    HIP_TRY(hipMemcpyAsync(dst->ring + ds * rn, src->ring + ss * rn, rn * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIP_TRY(hipMemcpyAsync(dst->mem0 + ds * mn, src->mem0 + ss * mn, mn * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  dst->head[ds] = src->head[ss];
  dst->fill[ds] = src->fill[ss];
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// step
// ------------------------------------------------------------------------------------------------
// Ring heads and fill counts advance only after the whole long-memory section (ring write, stage 0, cache write) was enqueued without an
// error: a step that fails in it leaves the stream's counters where they were, and the next step overwrites the same slot and the cache.
extern "C" int sf_oad_step(sf_oad* h, sf_oad_state* st, const int32_t* ids, int n, const float* work_dev, const float* long_dev,
                           const int32_t* long_rows, const float* mask_dev, float* out_dev, int probs, void* workspace, size_t workspace_bytes,
                           sf_stream stream) {
  if (!h || !st || st->det != h) return sf_set_err(SF_ERR_INVALID, "sf_oad_step: null handle, or a state of another detector");
  SF_TRY(sf_model_check_finalized(h, "sf_oad"));
  if (n < 1 || n > OAD_MAX_S) return sf_set_err(SF_ERR_INVALID, "sf_oad_step: %d streams per call outside 1..%d", n, OAD_MAX_S);
  if (!ids || !long_rows || !work_dev || !out_dev || !workspace) return sf_set_err(SF_ERR_INVALID, "sf_oad_step: null buffer");
  const sf_oad_config& c = h->cfg;
  const int d = h->d, L = c.long_samples, W = c.work_samples, Q0 = h->Q0;
  int Rl = 0, n0 = 0;
  for (int i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= st->streams) return sf_set_err(SF_ERR_INVALID, "sf_oad_step: stream %d of %d", ids[i], st->streams);
    for (int j = 0; j < i; ++j)
      if (ids[j] == ids[i]) return sf_set_err(SF_ERR_INVALID, "sf_oad_step: stream %d twice in one call", ids[i]);
    const int fill = st->fill[ids[i]], lr = long_rows[i];
    if (fill == 0 && lr != L) return sf_set_err(SF_ERR_STATE, "sf_oad_step: stream %d is empty: its first step takes the whole window of %d long samples, not %d", ids[i], L, lr);
    if (fill != 0 && lr != 0 && lr != 1) return sf_set_err(SF_ERR_INVALID, "sf_oad_step: stream %d holds its window: a step takes one new long sample or none, not %d (reset the stream first)", ids[i], lr);
    Rl += lr;
    n0 += lr > 0;
  }
  if (Rl && !long_dev) return sf_set_err(SF_ERR_INVALID, "sf_oad_step: long samples announced but long_dev is null");
  if (((uintptr_t)work_dev | (uintptr_t)long_dev | (uintptr_t)mask_dev | (uintptr_t)out_dev) & 15) return sf_set_err(SF_ERR_INVALID, "sf_oad_step: buffers must be 16-byte aligned");
  OadRun r(h, workspace, n, (hipStream_t)stream);
  SF_TRY(sf_check_workspace("sf_oad_step", "sf_oad_workspace_bytes", workspace, workspace_bytes, r.ws.bytes));
  const OadWorkspace& ws = r.ws;
  hipStream_t s = r.s;
  int rc;
  OadAct x = ws.a[0], mem = ws.a[1], spare = ws.a[2];
  auto row_head = [&](const float* in, const SfDevLN* ln, const float* pe, int pe_mod, const OadAct& y, bool want_f32, int rows) {
    SfRowArgs p;
    memset(&p, 0, sizeof(p));
    p.x = in; p.eps = c.eps; p.rows = rows; p.D = d;
    if (ln) { p.gamma = ln->g; p.beta = ln->b; p.relu = 1; }
    p.pe = pe; p.pe_mod = pe_mod;
    float* f32 = want_f32 ? y.f : nullptr;
    if (pe) { p.q = f32; p.q_hi = y.p.hi; p.q_lo = y.p.lo; }      // the one output is the row with its position added
    else { p.y = f32; p.y_hi = y.p.hi; p.y_lo = y.p.lo; }
    return oad_launch_row(p, s);
  };
  // ---- work memory: feature head + pe[L : L + W] ----
  if (c.linear_enabled) {
    HIP_TRY(sf_launch_split(work_dev, ws.in.hi, ws.in.lo, (size_t)n * W * c.d_in, s));
    HIP_TRY(r.lin.f32(h->fh_work, ws.in, n * W, ws.tmp));
    HIP_TRY(row_head(ws.tmp, &h->fh_work_ln, h->pe + (size_t)L * d, W, x, true, n * W));
  } else {
    HIP_TRY(row_head(work_dev, nullptr, h->pe + (size_t)L * d, W, x, true, n * W));
  }
  // ---- long memory: feature head of the new samples, W_k x | W_v x into the rings, compression stage 0 ----
  if (Rl) {
    if (c.linear_enabled) {
      HIP_TRY(sf_launch_split(long_dev, ws.in.hi, ws.in.lo, (size_t)Rl * c.d_in, s));
      HIP_TRY(r.lin.f32(h->fh_long, ws.in, Rl, ws.tmp));
      HIP_TRY(row_head(ws.tmp, &h->fh_long_ln, nullptr, 0, spare, false, Rl));
    } else {
      HIP_TRY(sf_launch_split(long_dev, spare.p.hi, spare.p.lo, (size_t)Rl * d, s));
    }
    const OadLayer& l0 = h->enc[0].layers[0];
    HIP_TRY(r.lin.f32(l0.cross_kv, spare.p, Rl, ws.kv));
    SfOadRows put, keep;
    memset(&put, 0, sizeof(put));
    memset(&keep, 0, sizeof(keep));
    SfOadAttn a = r.attn_args(n0, Q0, L, 0);
    int src = 0, k = 0;
    int new_head[OAD_MAX_S];      // committed to the state only after every launch of this section was accepted
    for (int i = 0; i < n; ++i) {
      const int lr = long_rows[i], id = ids[i];
      if (!lr) continue;
      put.src[k] = src; put.cnt[k] = lr;
      put.dst[k] = id * L + (lr == L ? 0 : st->head[id]);      // one sample: over the oldest
      new_head[k] = lr == L ? 0 : (st->head[id] + 1) % L;
      a.kv_row0[k] = id * L; a.ring_start[k] = new_head[k]; a.mask_row[k] = i;
      keep.src[k] = k * Q0; keep.dst[k] = id * Q0; keep.cnt[k] = Q0;
      src += lr;
      ++k;
    }
    put.n = keep.n = n0;
    HIP_TRY(oad_launch_rows(ws.kv, st->ring, nullptr, nullptr, 2 * d, put, s));
    a.q = h->q0; a.q_pitch = d; a.q_sstride = 0;
    a.k = st->ring; a.v = st->ring + d; a.kv_pitch = 2 * d;
    a.kpos = h->pos_kv; a.vpos = h->pos_kv + d; a.pos_pitch = 2 * d;
    a.mask = mask_dev;
    HIP_TRY(oad_launch_attention(a, s));
    HIP_TRY(r.lin.f32(l0.cross_out, ws.ctx, n0 * Q0, ws.tmp));
    if ((rc = r.add_ln(ws.tmp, h->tgt0.f, Q0, l0.n2, mem, n0 * Q0))) return rc;
    if ((rc = r.ffn_block(l0, l0.n3, mem, n0 * Q0))) return rc;
    if (h->enc[0].norm) {
      if ((rc = r.final_norm(h->enc[0].fn, mem, spare, n0 * Q0))) return rc;
      std::swap(mem, spare);
    }
    HIP_TRY(oad_launch_rows(mem.f, st->mem0, nullptr, nullptr, d, keep, s));
    k = 0;
    for (int i = 0; i < n; ++i)
      if (long_rows[i]) { st->head[ids[i]] = new_head[k++]; st->fill[ids[i]] = L; }
  }
  // ---- the compressed memory of every stream of the call, cached or new ----
  int Tm = Q0;
  {
    SfOadRows get;
    memset(&get, 0, sizeof(get));
    get.n = n;
    for (int i = 0; i < n; ++i) { get.src[i] = ids[i] * Q0; get.dst[i] = i * Q0; get.cnt[i] = Q0; }
    HIP_TRY(oad_launch_rows(st->mem0, mem.f, mem.p.hi, mem.p.lo, d, get, s));
  }
  // ---- later compression stages ----
  for (size_t j = 1; j < h->enc.size(); ++j) {
    const OadModule& m = h->enc[j];
    if (m.queries > 0) {
      const int Q = m.queries;
      SfOadRows rep;
      memset(&rep, 0, sizeof(rep));
      rep.n = n;
      for (int i = 0; i < n; ++i) { rep.src[i] = 0; rep.dst[i] = i * Q; rep.cnt[i] = Q; }
      HIP_TRY(oad_launch_rows(m.qw, spare.f, spare.p.hi, spare.p.lo, d, rep, s));
      for (const OadLayer& l : m.layers) {
        if ((rc = r.self_block(l, spare, n, Q, 0))) return rc;
        if ((rc = r.cross_block(l, spare, n, Q, mem, Tm))) return rc;
        if ((rc = r.ffn_block(l, l.n3, spare, n * Q))) return rc;
      }
      std::swap(mem, spare);
      Tm = Q;
    } else {
      for (const OadLayer& l : m.layers) {
        if ((rc = r.self_block(l, mem, n, Tm, 0))) return rc;
        if ((rc = r.ffn_block(l, l.n2, mem, n * Tm))) return rc;
      }
    }
    if (m.norm) {
      if ((rc = r.final_norm(m.fn, mem, spare, n * Tm))) return rc;
      std::swap(mem, spare);
    }
  }
  // ---- work decoder and classifier ----
  for (const OadLayer& l : h->dec.layers) {
    if ((rc = r.self_block(l, x, n, W, 1))) return rc;
    if ((rc = r.cross_block(l, x, n, W, mem, Tm))) return rc;
    if ((rc = r.ffn_block(l, l.n3, x, n * W))) return rc;
  }
  if (h->dec.norm) {
    if ((rc = r.final_norm(h->dec.fn, x, spare, n * W))) return rc;
    std::swap(x, spare);
  }
  HIP_TRY(r.lin.f32(h->cls, x.p, n * W, ws.scores));
  HIP_TRY(sf_launch(sf_oad_scores_kernel, dim3((unsigned)((n * W + 3) / 4)), dim3(256), 0, s, ws.scores, out_dev, n * W, h->Cp, c.classes, probs));
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// the attention kernel alone (parity tests)
// ------------------------------------------------------------------------------------------------
extern "C" int sf_op_oad_attention(const float* q_dev, int q_streams, const float* k_dev, const float* v_dev, const int32_t* ring_start,
                                   const float* k_pos_dev, const float* v_pos_dev, const float* mask_dev, float* ctx_dev, int streams, int Tq,
                                   int Tk, int heads, int head_dim, int causal, sf_stream stream) {
  if (!q_dev || !k_dev || !v_dev || !ctx_dev) return sf_set_err(SF_ERR_INVALID, "sf_op_oad_attention: null buffer");
  if (streams < 1 || streams > OAD_MAX_S) return sf_set_err(SF_ERR_INVALID, "sf_op_oad_attention: %d streams outside 1..%d", streams, OAD_MAX_S);
  if (q_streams != 1 && q_streams != streams) return sf_set_err(SF_ERR_INVALID, "sf_op_oad_attention: q_streams %d (1 = shared, or %d)", q_streams, streams);
  if (Tq < 1 || Tk < 1 || heads < 1) return sf_set_err(SF_ERR_INVALID, "sf_op_oad_attention: bad shape Tq=%d Tk=%d heads=%d", Tq, Tk, heads);
  if (head_dim < 8 || head_dim > 256 || head_dim % 8) return sf_set_err(SF_ERR_INVALID, "sf_op_oad_attention: head_dim must be a multiple of 8 in 8..256");
  if ((!k_pos_dev) != (!v_pos_dev)) return sf_set_err(SF_ERR_INVALID, "sf_op_oad_attention: k_pos and v_pos come together");
  if ((int64_t)streams * (Tq > Tk ? Tq : Tk) * heads * head_dim > (int64_t)0x7fffffff) return sf_set_err(SF_ERR_CAPACITY, "sf_op_oad_attention: more than 2^31 - 1 elements");
  if (((uintptr_t)q_dev | (uintptr_t)k_dev | (uintptr_t)v_dev | (uintptr_t)k_pos_dev | (uintptr_t)v_pos_dev | (uintptr_t)mask_dev | (uintptr_t)ctx_dev) & 15)
    return sf_set_err(SF_ERR_INVALID, "sf_op_oad_attention: buffers must be 16-byte aligned");
  const int D = heads * head_dim;
  SfOadAttn a;
  memset(&a, 0, sizeof(a));
  a.q = q_dev; a.k = k_dev; a.v = v_dev; a.kpos = k_pos_dev; a.vpos = v_pos_dev; a.mask = mask_dev; a.ctx_f32 = ctx_dev;
  a.q_sstride = q_streams == 1 ? 0 : (long long)Tq * D;
  a.q_pitch = a.kv_pitch = a.pos_pitch = D;
  a.streams = streams; a.Tq = Tq; a.Tk = Tk; a.heads = heads; a.hd = head_dim; a.causal = causal ? 1 : 0;
  a.scale = 1.0f / sqrtf((float)head_dim);
  for (int i = 0; i < streams; ++i) {
    a.kv_row0[i] = i * Tk; a.mask_row[i] = i;
    a.ring_start[i] = ring_start ? ring_start[i] : 0;
    if (a.ring_start[i] < 0 || a.ring_start[i] >= Tk) return sf_set_err(SF_ERR_INVALID, "sf_op_oad_attention: ring_start[%d] = %d outside 0..%d", i, a.ring_start[i], Tk - 1);
  }
  HIP_TRY(oad_launch_attention(a, (hipStream_t)stream));
  return SF_OK;
}
