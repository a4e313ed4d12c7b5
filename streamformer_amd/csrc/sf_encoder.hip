// C-ABI implementation: handle, weight packing, and the launch schedule of the encoder forward
// (reference TimesformerMultiTaskingModelSigLIP.forward, modeling:1299-1354; layer body :934-1004;
// streaming copy vqa_enc:1316-1392).  See include/streamformer_hip.h for the contract.
// The streaming entries are sf_stream.hip, the single operators sf_ops.hip, the bench hooks sf_bench.hip; what they and this file
// share is sf_encoder.h.
#include "sf_encoder.h"
#include "sf_switches.h"
#include "sf_pool_head.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define SF_ABI_VERSION 5
static const int kLoraRank = 32;  // modeling:1280-1281

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
int sf_set_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// ------------------------------------------------------------------------------------------------
// expected weights
// ------------------------------------------------------------------------------------------------
static void build_expected(sf_encoder* e) {
  const sf_config& c = e->cfg;
  const int64_t D = c.hidden_size, I = c.intermediate_size, P = c.patch_size, C = c.num_channels;
  const int64_t N = e->N, T = c.num_frames;
  e->weights.prefix = "timesformer.";      // wrapper checkpoints (base_model_prefix, modeling:1073)
  e->weights.accept_f16 = true;
  e->weights.exact_shape = false;          // checkpoints carry e.g. the gating scalar as [] or [1], the tables with or without a leading 1
  auto& x = e->weights.expected;
  x["embeddings.position_embeddings"] = {1, N, D};
  x["embeddings.time_embeddings"] = {1, T, D};
  x["embeddings.patch_embeddings.projection.weight"] = {D, C, P, P};
  x["embeddings.patch_embeddings.projection.bias"] = {D};
  auto lin = [&](const std::string& p, int64_t out, int64_t in, bool bias) {
    x[p + ".weight"] = {out, in};
    if (bias) x[p + ".bias"] = {out};
  };
  auto ln = [&](const std::string& p) { x[p + ".weight"] = {D}; x[p + ".bias"] = {D}; };
  for (int i = 0; i < c.num_hidden_layers; ++i) {
    const std::string p = "encoder.layer." + std::to_string(i) + ".";
    x[p + "temporal_attention_gating"] = {};
    ln(p + "temporal_layernorm");
    lin(p + "temporal_attention.attention.qkv", 3 * D, D, c.qkv_bias);
    lin(p + "temporal_attention.output.dense", D, D, true);
    lin(p + "temporal_dense", D, D, true);
    ln(p + "layernorm_before");
    lin(p + "attention.attention.qkv", 3 * D, D, c.qkv_bias);
    lin(p + "attention.output.dense", D, D, true);
    if (c.add_lora_spatial) {
      x[p + "attention.attention.qkv_lora_a.weight"] = {kLoraRank, D};
      x[p + "attention.attention.qkv_lora_b.weight"] = {3 * D, kLoraRank};
      x[p + "attention.output.dense_lora_a.weight"] = {kLoraRank, D};
      x[p + "attention.output.dense_lora_b.weight"] = {D, kLoraRank};
    }
    ln(p + "layernorm_after");
    lin(p + "intermediate.dense", I, D, true);
    lin(p + "output.dense", D, I, true);
  }
  ln("post_layernorm");
  x["head.probe"] = {1, 1, D};
  x["head.attention.in_proj_weight"] = {3 * D, D};
  x["head.attention.in_proj_bias"] = {3 * D};
  lin("head.attention.out_proj", D, D, true);
  ln("head.layernorm");
  lin("head.mlp.fc1", I, D, true);
  lin("head.mlp.fc2", D, I, true);
}

// ------------------------------------------------------------------------------------------------
// lifetime
// ------------------------------------------------------------------------------------------------
extern "C" int sf_abi_version(void) { return SF_ABI_VERSION; }
extern "C" const char* sf_last_error(void) { return g_err; }

extern "C" int sf_create(const sf_config* cfg, int device, sf_encoder** out) {
  if (!cfg || !out) return sf_set_err(SF_ERR_INVALID, "sf_create: null argument");
  const sf_config& c = *cfg;
  if (c.hidden_size <= 0 || c.num_attention_heads <= 0 || c.hidden_size % c.num_attention_heads)
    return sf_set_err(SF_ERR_INVALID, "hidden_size %d not divisible by heads %d", c.hidden_size, c.num_attention_heads);
  {   // head_dim 64: the tuned attention kernels; any other multiple of 8 up to 128 (SigLIP-so400m: 72): sf_attention_generic.hip
    const int hd = c.hidden_size / c.num_attention_heads;
    if (hd < 8 || hd > 128 || hd % 8)
      return sf_set_err(SF_ERR_INVALID, "head_dim %d unsupported: multiples of 8 from 8 to 128 (64 runs on the tuned kernels, the others on the generic fp32 attention kernel)", hd);
  }
  if (c.num_attention_heads > 16)
    return sf_set_err(SF_ERR_INVALID, "%d attention heads unsupported: the pooling-head kernels hold at most 16 heads per MFMA tile", c.num_attention_heads);
  // intermediate_size and C*P*P need no alignment: the weights are zero-padded to multiples of 64 at upload (gelu(0) = 0 and zero
  // weight columns make the padding exact): SigLIP-so400m has I = 4304 and 14 x 14 patches (K = 588)
  if (c.hidden_size % 64 || c.intermediate_size <= 0 || c.patch_size <= 0 || c.num_channels <= 0)
    return sf_set_err(SF_ERR_INVALID, "hidden_size must be a multiple of 64; intermediate_size, patch_size, num_channels positive");
  if (c.image_size % c.patch_size) return sf_set_err(SF_ERR_INVALID, "image_size not a multiple of patch_size");
  if (c.hidden_act < 0 || c.hidden_act > 2) return sf_set_err(SF_ERR_INVALID, "unsupported hidden_act code %d", c.hidden_act);
  if (c.num_frames <= 0 || c.num_frames > 256) return sf_set_err(SF_ERR_INVALID, "num_frames must be in 1..256");
  sf_encoder* e = new sf_encoder();
  e->cfg = c;
  e->device = device;
  e->D = c.hidden_size;
  e->I = (c.intermediate_size + 63) / 64 * 64;          // padded: rows / columns past cfg.intermediate_size are zero weights
  e->L = c.num_hidden_layers;
  e->N = (c.image_size / c.patch_size) * (c.image_size / c.patch_size);
  e->Kp = (c.num_channels * c.patch_size * c.patch_size + 63) / 64 * 64;      // padded patch-vector length (zero columns)
  e->hd = c.hidden_size / c.num_attention_heads;
  build_expected(e);
  *out = e;
  return SF_OK;
}

static uint64_t next_generation() {
  static uint64_t g = 0;      // a handle is used from one thread at a time; creation from several threads is serialised by the caller
  return ++g;
}

extern "C" void sf_destroy(sf_encoder* e) {
  if (!e) return;
  e->dev.free_all();
  delete e;
}

// ------------------------------------------------------------------------------------------------
// weights
// ------------------------------------------------------------------------------------------------
extern "C" int sf_load_tensor(sf_encoder* e, const char* key, const void* host_ptr, int dtype,
                              const int64_t* shape, int ndim) {
  if (!e || !key || !host_ptr || ndim < 0 || (ndim && !shape)) return sf_set_err(SF_ERR_INVALID, "sf_load_tensor: null argument");
  std::string err;
  const int rc = e->weights.load(key, host_ptr, dtype, shape, ndim, &err);
  if (rc) return sf_set_err(rc, "%s", err.c_str());
  e->finalized = false;
  return SF_OK;
}

extern "C" int sf_set_pixel_normalization(sf_encoder* e, const float* mean, const float* std, int channels, float rescale) {
  if (!e || !mean || !std || channels < 1 || channels > 4) return sf_set_err(SF_ERR_INVALID, "bad pixel normalisation");
  for (int c = 0; c < 4; ++c) {
    const int k = c < channels ? c : channels - 1;
    if (!(std[k] > 0.f)) return sf_set_err(SF_ERR_INVALID, "image_std must be positive");
    e->pixel_norm.scale[c] = rescale / std[k];       // (x * rescale - mean) / std
    e->pixel_norm.shift[c] = -mean[k] / std[k];
  }
  return SF_OK;
}

extern "C" int sf_missing_weights(sf_encoder* e) {
  if (!e) return sf_set_err(SF_ERR_INVALID, "null handle");
  std::string err;
  const int missing = e->weights.missing(&err);
  if (missing) sf_set_err(SF_ERR_STATE, "%s", err.c_str());
  return missing;
}

// force_split: the pooling head's small Linears keep the lo plane in bf16 mode too
static int upload_linear(sf_encoder* e, const std::vector<float>& w, const std::vector<float>* bias, int N, int K, DevLinear* out,
                         bool force_split = false) {
  return sf_upload_linear(e->dev, w, bias, N, K, N, force_split || e->compute == SF_COMPUTE_BF16X3, out);
}

// LayerNorm(gamma, beta) followed by Linear(W, b)  ==  rstd * (x W'^T - mean * s) + b'
// with W' = W * gamma (per input column), b' = b + W beta, s_n = sum_k W'[n,k] (of the ROUNDED W').
static int upload_folded_linear(sf_encoder* e, const std::vector<float>& w, const std::vector<float>* bias,
                                const std::vector<float>& gamma, const std::vector<float>& beta, int N, int K,
                                DevLinear* out, bool frag_copy = false) {
  std::vector<float> wf(w.size()), bf(N), sn(N);
  const bool split = e->compute == SF_COMPUTE_BF16X3;      // the MFMAs then see hi + lo planes of W'
  for (int n = 0; n < N; ++n) {
    double bb = bias ? (double)(*bias)[n] : 0.0, ss = 0.0;
    for (int k = 0; k < K; ++k) {
      const float wv = w[(size_t)n * K + k];
      const float wg = (float)((double)wv * (double)gamma[k]);
      wf[(size_t)n * K + k] = wg;
      const float hi = sf_host_bf2f(sf_host_f2bf(wg));
      ss += (double)hi + (split ? (double)sf_host_bf2f(sf_host_f2bf(wg - hi)) : 0.0);
      bb += (double)wv * (double)beta[k];
    }
    bf[n] = (float)bb;
    sn[n] = (float)ss;
  }
  int rc = upload_linear(e, wf, &bf, N, K, out);
  if (rc) return rc;
  if (frag_copy && !split && N % 16 == 0 && K % 32 == 0) {
    // fragment-major copy: [n-tile t][k-step j][lane = 16 g + l15][8] = W'[16 t + l15][32 j + 8 g ..]: the 64 lanes of a wave read ONE
    // contiguous KiB per MFMA operand (the row-major matrix gives every 16-lane group 16 different lines of 16 bytes each)
    const int NK = K / 32;
    std::vector<uint16_t> fr((size_t)N * K);
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k)
        fr[((((size_t)(n / 16) * NK + k / 32) * 64) + ((k % 32) / 8) * 16 + n % 16) * 8 + k % 8] = sf_host_f2bf(wf[(size_t)n * K + k]);
    if ((rc = e->dev.upload(fr, &out->w_frag))) return rc;
  }
  return e->dev.upload(sn, &out->ln_s);
}

static int upload_ln(sf_encoder* e, const std::string& p, DevLN* out) {
  SF_TRY(e->dev.upload(e->weights.data(p + ".weight"), &out->g));
  return e->dev.upload(e->weights.data(p + ".bias"), &out->b);
}

// W += B A  (lora_b [out, r] x lora_a [r, in]); accumulate in double
static void merge_lora_into(std::vector<float>& w, const std::vector<float>& a, const std::vector<float>& b,
                            int out, int in, int r) {
  for (int o = 0; o < out; ++o)
    for (int i = 0; i < in; ++i) {
      double acc = 0.0;
      for (int k = 0; k < r; ++k) acc += (double)b[(size_t)o * r + k] * (double)a[(size_t)k * in + i];
      w[(size_t)o * in + i] = (float)((double)w[(size_t)o * in + i] + acc);
    }
}

// What a parked stream's K/V were computed with (sf_cache_stream_meta::packing): the configuration, the packing options and every
// staged weight, hashed in key order — the same number for the same weights in any process, unlike `generation`.  The compute mode
// stays out: it is a field of its own.  Four multiply-xor lanes over 64-bit words (one pass over the fp32 master copy).
static uint64_t weights_fingerprint(const sf_encoder* e, int merge_lora, int fuse_temporal_proj) {
  const uint64_t kMul = 0x9e3779b97f4a7c15ull;
  auto mix = [&](uint64_t h, uint64_t v) { h = (h ^ v) * kMul; return h ^ (h >> 29); };
  uint64_t h = 0x53464b56ull;
  uint32_t cw[sizeof(sf_config) / 4];
  memcpy(cw, &e->cfg, sizeof(cw));
  for (uint32_t w : cw) h = mix(h, w);
  h = mix(h, (uint64_t)(merge_lora != 0) * 2 + (fuse_temporal_proj != 0));
  for (const auto& kv : e->weights.host) {
    for (char ch : kv.first) h = mix(h, (uint8_t)ch);
    const std::vector<float>& d = kv.second.data;
    h = mix(h, d.size());
    uint64_t lane[4] = {h, h ^ 1, h ^ 2, h ^ 3};
    const size_t words = d.size() / 2, quads = words / 4;
    const char* p = reinterpret_cast<const char*>(d.data());
    for (size_t q = 0; q < quads; ++q) {
      uint64_t w[4];
      memcpy(w, p + q * 32, 32);
      for (int k = 0; k < 4; ++k) lane[k] = (lane[k] ^ w[k]) * kMul;
    }
    for (size_t i = quads * 8; i < d.size(); ++i) {
      uint32_t u;
      memcpy(&u, &d[i], 4);
      lane[i & 3] = mix(lane[i & 3], u);
    }
    for (int k = 0; k < 4; ++k) h = mix(h, lane[k]);
  }
  return h ? h : 1;      // 0 is "no packing"
}

extern "C" int sf_finalize_weights(sf_encoder* e, int compute, int merge_lora, int fuse_temporal_proj) {
  if (!e) return sf_set_err(SF_ERR_INVALID, "null handle");
  SF_TRY(sf_check_compute_mode(compute));
  if (sf_missing_weights(e)) return SF_ERR_STATE;
  if (e->cfg.add_lora_spatial && !merge_lora)
    return sf_set_err(SF_ERR_INVALID, "un-merged LoRA execution is a training-time path; the inference forward needs merge_lora=1");
  HIP_TRY(hipSetDevice(e->device));
  e->dev.free_all();
  e->compute = compute;
  e->fused_temporal = fuse_temporal_proj != 0;
  const int D = e->D, I = e->I, Ir = e->cfg.intermediate_size;
  auto H = [&](const std::string& k) -> std::vector<float>& { return e->weights.data(k); };
  auto Hopt = [&](const std::string& k) -> std::vector<float>* { return e->weights.host.count(k) ? &e->weights.data(k) : nullptr; };
  // zero padding of a [rows, cols] matrix to [rows_p, cols_p] (intermediate_size -> I, C*P*P -> Kp); a no-op copy when nothing changes
  auto pad2 = [](const std::vector<float>& w, int rows, int cols, int rows_p, int cols_p) {
    if (rows == rows_p && cols == cols_p) return w;
    std::vector<float> o((size_t)rows_p * cols_p, 0.f);
    for (int r = 0; r < rows; ++r) std::copy(w.begin() + (size_t)r * cols, w.begin() + (size_t)(r + 1) * cols, o.begin() + (size_t)r * cols_p);
    return o;
  };
  auto pad1 = [](const std::vector<float>* b, int n, int n_p) {
    std::vector<float> o((size_t)n_p, 0.f);
    if (b) std::copy(b->begin(), b->begin() + n, o.begin());
    return o;
  };
  {
    const int Kr = e->cfg.num_channels * e->cfg.patch_size * e->cfg.patch_size;
    const std::vector<float> wp = pad2(H("embeddings.patch_embeddings.projection.weight"), D, Kr, D, e->Kp);
    SF_TRY(upload_linear(e, wp, Hopt("embeddings.patch_embeddings.projection.bias"), D, e->Kp, &e->patch));
  }
  SF_TRY(e->dev.upload(H("embeddings.position_embeddings"), &e->pos));
  SF_TRY(e->dev.upload(H("embeddings.time_embeddings"), &e->time_tab));
  e->layers.assign(e->L, DevLayer());
  for (int i = 0; i < e->L; ++i) {
    const std::string p = "encoder.layer." + std::to_string(i) + ".";
    DevLayer& l = e->layers[i];
    l.gate_tanh = std::tanh(H(p + "temporal_attention_gating")[0]);
    SF_TRY(upload_ln(e, p + "temporal_layernorm", &l.ln_t));
    SF_TRY(upload_ln(e, p + "layernorm_before", &l.ln_b));
    SF_TRY(upload_ln(e, p + "layernorm_after", &l.ln_a));
    SF_TRY(upload_linear(e, H(p + "temporal_attention.attention.qkv.weight"), Hopt(p + "temporal_attention.attention.qkv.bias"), 3 * D, D, &l.t_qkv));
    SF_TRY(upload_folded_linear(e, H(p + "temporal_attention.attention.qkv.weight"), Hopt(p + "temporal_attention.attention.qkv.bias"),
                             H(p + "temporal_layernorm.weight"), H(p + "temporal_layernorm.bias"), 3 * D, D, &l.t_qkv_f,
                             SF_LAB_SWITCH("SF_STREAM_QKV_FUSE") && e->compute == SF_COMPUTE_BF16 && D % 128 == 0 && D <= 768));
#ifdef SF_LAB      // lab library only: the permuted copy for sf_gemm_qkv.hip's fused tile (profiles/r04_qkv_fused_ab.txt)
    if (e->compute == SF_COMPUTE_BF16 && D % 128 == 0 && SF_LAB_SWITCH("SF_QKV_FUSED")) {
      // row 384 j + 64 i + c of the permuted matrix = row (i / 2) D + (2 j + (i & 1)) 64 + c of the original (i = 0..5: q0 q1 k0 k1 v0 v1)
      const std::vector<float>& w0 = H(p + "temporal_attention.attention.qkv.weight");
      const std::vector<float>* b0 = Hopt(p + "temporal_attention.attention.qkv.bias");
      std::vector<float> wp(w0.size()), bp(3 * (size_t)D, 0.f);
      for (int r = 0; r < 3 * D; ++r) {
        const int j = r / 384, i = (r % 384) / 64, cc = r % 64;
        const int src = (i >> 1) * D + (2 * j + (i & 1)) * 64 + cc;
        std::copy(w0.begin() + (size_t)src * D, w0.begin() + (size_t)(src + 1) * D, wp.begin() + (size_t)r * D);
        if (b0) bp[r] = (*b0)[src];
      }
      SF_TRY(upload_folded_linear(e, wp, b0 ? &bp : nullptr, H(p + "temporal_layernorm.weight"), H(p + "temporal_layernorm.bias"), 3 * D, D, &l.t_qkv_fp));
    }
#endif
    if (e->fused_temporal) {
      // temporal_dense(output.dense(x)) = (W2 W1) x + (W2 b1 + b2)      (modeling:947-954)
      const std::vector<float>& w1 = H(p + "temporal_attention.output.dense.weight");
      const std::vector<float>& b1 = H(p + "temporal_attention.output.dense.bias");
      const std::vector<float>& w2 = H(p + "temporal_dense.weight");
      const std::vector<float>& b2 = H(p + "temporal_dense.bias");
      std::vector<float> wf((size_t)D * D), bf(D);
      std::vector<double> row(D);
      for (int o = 0; o < D; ++o) {
        std::fill(row.begin(), row.end(), 0.0);
        double bb = b2[o];
        for (int k = 0; k < D; ++k) {
          const double a = w2[(size_t)o * D + k];
          bb += a * b1[k];
          const float* w1r = &w1[(size_t)k * D];
          for (int j = 0; j < D; ++j) row[j] += a * w1r[j];
        }
        for (int j = 0; j < D; ++j) wf[(size_t)o * D + j] = (float)row[j];
        bf[o] = (float)bb;
      }
      SF_TRY(upload_linear(e, wf, &bf, D, D, &l.t_fused));
    } else {
      SF_TRY(upload_linear(e, H(p + "temporal_attention.output.dense.weight"), Hopt(p + "temporal_attention.output.dense.bias"), D, D, &l.t_out));
      SF_TRY(upload_linear(e, H(p + "temporal_dense.weight"), Hopt(p + "temporal_dense.bias"), D, D, &l.t_dense));
    }
    std::vector<float> wq = H(p + "attention.attention.qkv.weight");
    std::vector<float> wo = H(p + "attention.output.dense.weight");
    if (e->cfg.add_lora_spatial) {
      merge_lora_into(wq, H(p + "attention.attention.qkv_lora_a.weight"), H(p + "attention.attention.qkv_lora_b.weight"), 3 * D, D, kLoraRank);
      merge_lora_into(wo, H(p + "attention.output.dense_lora_a.weight"), H(p + "attention.output.dense_lora_b.weight"), D, D, kLoraRank);
    }
    SF_TRY(upload_linear(e, wq, Hopt(p + "attention.attention.qkv.bias"), 3 * D, D, &l.s_qkv));
    SF_TRY(upload_folded_linear(e, wq, Hopt(p + "attention.attention.qkv.bias"), H(p + "layernorm_before.weight"),
                             H(p + "layernorm_before.bias"), 3 * D, D, &l.s_qkv_f));
    {
      const std::vector<float> wu = pad2(H(p + "intermediate.dense.weight"), Ir, D, I, D);
      const std::vector<float> bu = pad1(Hopt(p + "intermediate.dense.bias"), Ir, I);
      const std::vector<float> wd = pad2(H(p + "output.dense.weight"), D, Ir, D, I);
      SF_TRY(upload_folded_linear(e, wu, &bu, H(p + "layernorm_after.weight"), H(p + "layernorm_after.bias"), I, D, &l.up_f));
      SF_TRY(upload_linear(e, wo, Hopt(p + "attention.output.dense.bias"), D, D, &l.s_out));
      SF_TRY(upload_linear(e, wu, &bu, I, D, &l.up));
      SF_TRY(upload_linear(e, wd, Hopt(p + "output.dense.bias"), D, I, &l.down));
    }
  }
  SF_TRY(upload_ln(e, "post_layernorm", &e->post_ln));
  SF_TRY(upload_ln(e, "head.layernorm", &e->head_ln));
  {
    // nn.MultiheadAttention packed in_proj rows are [q; k; v] (modeling:1135-1137).  The query is
    // the learned probe only, identical for every frame: project and scale it once, in double.
    const std::vector<float>& w = H("head.attention.in_proj_weight");
    const std::vector<float>& b = H("head.attention.in_proj_bias");
    const std::vector<float>& probe = H("head.probe");
    std::vector<double> q(D);
    const int hd = e->hd;
    const double sc = 1.0 / std::sqrt((double)hd);
    for (int o = 0; o < D; ++o) {
      double acc = b[o];
      for (int k = 0; k < D; ++k) acc += (double)w[(size_t)o * D + k] * probe[k];
      q[o] = acc * sc;
    }
    // The keys only ever meet this one query, so the key projection folds into it: score_hn = (Wk_h^T q_h) . x_n + q_h . bk_h, and
    // the second term is constant over n — the softmax drops it.  U_h = Wk_h^T q_h, in double; the values need no projection of
    // the tokens either: ctx_h = Wv_h (sum_n p_hn x_n) + bv_h.
    const int heads = e->cfg.num_attention_heads;
    std::vector<uint16_t> uh((size_t)16 * D, 0), ul((size_t)16 * D, 0);
    std::vector<float> uf((size_t)16 * D, 0.f);
    for (int h = 0; h < heads; ++h)
      for (int d = 0; d < D; ++d) {
        double acc = 0.0;
        for (int j = 0; j < hd; ++j) acc += (double)w[((size_t)D + h * hd + j) * D + d] * q[h * hd + j];
        const float v = (float)acc;
        uf[(size_t)h * D + d] = v;
        uh[(size_t)h * D + d] = sf_host_f2bf(v);
        ul[(size_t)h * D + d] = sf_host_f2bf(v - sf_host_bf2f(uh[(size_t)h * D + d]));
      }
    SF_TRY(e->dev.upload(uh, &e->head_u_hi));
    SF_TRY(e->dev.upload(ul, &e->head_u_lo));
    SF_TRY(e->dev.upload(uf, &e->head_u));          // fp32 copy for the generic-width kernel (sf_launch_pool_generic)
    std::vector<float> wv(w.begin() + (size_t)2 * D * D, w.end());
    std::vector<float> bv(b.begin() + 2 * D, b.end());
    SF_TRY(e->dev.upload(wv, &e->head_wv));
    SF_TRY(e->dev.upload(bv, &e->head_bv));
  }
  SF_TRY(upload_linear(e, H("head.attention.out_proj.weight"), Hopt("head.attention.out_proj.bias"), D, D, &e->head_out, true));
  {
    const std::vector<float> w1 = pad2(H("head.mlp.fc1.weight"), Ir, D, I, D);
    const std::vector<float> b1 = pad1(Hopt("head.mlp.fc1.bias"), Ir, I);
    const std::vector<float> w2 = pad2(H("head.mlp.fc2.weight"), D, Ir, D, I);
    SF_TRY(upload_linear(e, w1, &b1, I, D, &e->head_fc1, true));
    SF_TRY(upload_linear(e, w2, Hopt("head.mlp.fc2.bias"), D, I, &e->head_fc2, true));
  }
  e->finalized = true;
  e->generation = next_generation();   // caches created against an earlier packing are refused from here on
  e->fingerprint = weights_fingerprint(e, merge_lora, fuse_temporal_proj);
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// workspace carving (struct Workspace: sf_encoder.h)
// ------------------------------------------------------------------------------------------------
Workspace carve(const sf_encoder* e, void* base, int B, int T, int N, bool need_tqkv) {
  Workspace w;
  SfCarver c(base);
  const size_t M = (size_t)B * T * N, F = (size_t)B * T;
  const size_t D = e->D, I = e->I;
  const bool acc = e->compute == SF_COMPUTE_BF16X3;
  const size_t wide = D > (size_t)e->Kp ? D : (size_t)e->Kp;
  w.resid = c.take<float>(M * D);
  w.te_rows = c.take<float>((size_t)((!need_tqkv && B > T) ? B : T) * D);      // streaming: a ragged call gathers one time row per stream
  w.ln_stats = c.take<float>(M * 8);                  // rows of 8 floats in both modes (SfGemmArgs::ln_stats_wide)
  w.embed_tab = (!acc && M >= 2048) ? c.take<float>((size_t)T * N * D) : nullptr;
  w.patch_buf = (!acc && M >= 2048) ? c.take<bf16_t>(M * (size_t)e->Kp) : nullptr;
  w.xn_hi = c.take<bf16_t>(M * wide);
  w.xn_lo = acc ? c.take<bf16_t>(M * wide) : nullptr;
  w.ctx_hi = c.take<bf16_t>(M * D);
  w.ctx_lo = acc ? c.take<bf16_t>(M * D) : nullptr;
  if (!e->fused_temporal) {
    w.tmp_hi = c.take<bf16_t>(M * D);
    w.tmp_lo = acc ? c.take<bf16_t>(M * D) : nullptr;
  } else {
    w.tmp_hi = w.tmp_lo = nullptr;
  }
  w.mid_hi = c.take<bf16_t>(M * I);
  w.mid_lo = acc ? c.take<bf16_t>(M * I) : nullptr;
  w.qkv = c.take<char>(M * 3 * D * (acc ? 4 : 2));
  w.tqkv = need_tqkv ? (void*)c.take<char>(M * 3 * D * (acc ? 4 : 2)) : nullptr;
  w.attn_out = c.take<float>(F * D);
  w.head_ctx = c.take<float>(F * D);
  w.head_mid = c.take<float>(F * I);
  {
    size_t pz = sf_pool_z_floats((int)F, N, e->cfg.num_attention_heads, (int)D);
    const size_t pgen = sf_pool_generic_scratch_floats((int)F, N, e->cfg.num_attention_heads, (int)D);      // generic widths: scores + z
    w.pool_z = c.take<float>(pz > pgen ? pz : pgen);
  }
  w.pool_ml = c.take<float>(sf_pool_ml_floats((int)F, N, e->cfg.num_attention_heads));
  w.pc_hi = c.take<bf16_t>(F * D);          // the pooling head's one-row-per-frame tensors keep hi + lo planes in both modes
  w.pc_lo = c.take<bf16_t>(F * D);
  w.hn_hi = c.take<bf16_t>(F * D);
  w.hn_lo = c.take<bf16_t>(F * D);
  w.hm_hi = c.take<bf16_t>(F * I);
  w.hm_lo = c.take<bf16_t>(F * I);
  w.res_bf = (M <= (size_t)sf_infold_max_rows()) ? c.take<bf16_t>(M * D) : nullptr;      // accurate mode (round 6): the hi plane; the lo plane travels in xn_lo
  // lo plane of the residual stream: bf16 mode at BASELINE-sized M (pm / gm); accurate mode at small M (round 6: in-kernel LayerNorm fold of streamed frames)
  w.res_lo = ((!acc && M > (size_t)sf_infold_max_rows()) || (acc && M <= (size_t)sf_infold_max_rows())) ? c.take<bf16_t>(M * D) : nullptr;
  w.res_lo2 = (acc && M >= 2048) ? c.take<bf16_t>(M * D) : nullptr;
  w.lhs_stage = !need_tqkv ? c.take<float>(M * D) : nullptr;       // streaming carve (the cache holds the temporal qkv)
  w.pool_stage = !need_tqkv ? c.take<float>(F * D) : nullptr;
  w.bytes = (c.off + 255) & ~(size_t)255;
  return w;
}

// ------------------------------------------------------------------------------------------------
// the launch schedule
// ------------------------------------------------------------------------------------------------
// The fields every Linear of the forward shares; a call site then sets what is special about it (outputs, residual, LayerNorm
// fold, row remap) by field name and launches with the same `split`.
SfGemmArgs linear_args(const sf_encoder* e, const DevLinear& lin, const bf16_t* a_hi, const bf16_t* a_lo, int M, int epi, bool split) {
  SfGemmArgs g = sf_linear_args(lin, a_hi, a_lo, M, epi, e->cfg.hidden_act, split);
  g.ln_eps = e->cfg.layer_norm_eps; g.ln_stats_wide = 1;
  return g;
}

// ---- which LayerNorm fold a shape can take: each predicate asks the kernels' own *_supported functions with the shapes of a layer's
// residual producers (N = D, K = D and K = I) and folded consumers (qkv: N = 3 D, MLP-up: N = I; K = D).  The operand pointers of
// such a probe only say "present".
static bf16_t* const kSetB = (bf16_t*)1;
static float* const kSetF = (float*)1;
static SfGemmArgs probe_args(const sf_encoder* e, int M, int N, int K, int epi) {
  SfGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.M = M; g.N = N; g.K = K; g.ldc = N; g.epi = epi; g.act = e->cfg.hidden_act; g.ln_stats_wide = 1;
  return g;
}
template <typename Takes>
static bool takes_both_k(const sf_encoder* e, SfGemmArgs producer, Takes&& takes) {      // a residual producer at K = D and at K = I
  producer.K = e->D;
  if (!takes(producer)) return false;
  producer.K = e->I;
  return takes(producer);
}
static bool bf16_consumers_on_g256(const sf_encoder* e, int M) {
  return sf_gemm256_supported(probe_args(e, M, 3 * e->D, e->D, SF_EPI_BF16), false) && sf_gemm256_supported(probe_args(e, M, e->I, e->D, SF_EPI_ACT_BF16), false);
}

// bf16 mode, two clips per call (sf_tile_fold_min_rows() <= M <= sf_tile_max_rows()): the narrow tile kernel stays the residual producer (it
// beats the panel kernel there) but emits the row statistics, so that the folded consumers can run on the 256^2 kernel (which beats the
// wide tiles there)
static bool ln_fold_tile_ok(const sf_encoder* e, int M) {
  if (e->compute != SF_COMPUTE_BF16 || sf_sw(SW_DISABLE_LN_FOLD)) return false;
  SfGemmArgs g = probe_args(e, M, e->D, e->D, SF_EPI_RESID_F32);
  g.out_f32 = kSetF; g.resid = kSetF; g.out_hi = kSetB; g.ln_stats_out = kSetF;
  return takes_both_k(e, g, [](const SfGemmArgs& a) { return sf_gemm_tile_supported(a, false); }) && bf16_consumers_on_g256(e, M);
}

// bf16 mode, BASELINE-sized M: the panel kernel as every residual producer (it emits the row statistics) and the 256^2 kernel as
// every consumer (it applies them).  SF_DISABLE_LN_FOLD is the A/B switch of this fold and of the two next to it.
static bool ln_fold_panel_ok(const sf_encoder* e, int M) {
  if (e->compute != SF_COMPUTE_BF16 || sf_sw(SW_DISABLE_LN_FOLD)) return false;
  return takes_both_k(e, probe_args(e, M, e->D, e->D, SF_EPI_RESID_F32), [](const SfGemmArgs& a) { return sf_gemm_panel_supported(a, false); }) &&
         bf16_consumers_on_g256(e, M);
}

// The plane-form fold on the 256^2 kernel as producer (hi + lo planes in / out + one {sum x, sum x^2} pair per 256-column tile, four per
// row) and consumer (its LNF instances sum the pairs): D a multiple of 256 up to 1024.
//   accurate mode (split): the residual stream itself is the hi + lo planes that are the folded Linears' operands (xn_hi / xn_lo); they
//     hold x to 2^-18 relative, the precision every bf16x3 operand has anyway.  SF_DISABLE_ACC_FOLD restores fp32 residual + LayerNorm (A/B).
//   bf16 mode: widths the panel kernel does not take (D = 1024, a ViT-L-shaped encoder), which would otherwise pay three standalone
//     LayerNorm launches per layer (9.7 % of the ViT-L forward).
static bool ln_fold_planes_g256_ok(const sf_encoder* e, int M, bool split) {
  if ((e->D % 256) || e->D > 1024) return false;
  SfGemmArgs g = probe_args(e, M, e->D, e->D, SF_EPI_RESID_F32);
  if (split) { g.a_lo = kSetB; g.w_lo = kSetB; }
  g.out_hi = kSetB; g.out_lo = kSetB; g.ln_stats_out = kSetF; g.resid_hi = kSetB; g.resid_lo = kSetB;
  if (!takes_both_k(e, g, [split](const SfGemmArgs& a) { return sf_gemm256_supported(a, split); })) return false;
  g.ln_stats_out = nullptr; g.resid_hi = g.resid_lo = nullptr; g.ln_stats = kSetF; g.ln_s = kSetF;
  if (split) g.out_hi = nullptr; else g.out_lo = nullptr;      // (the probes name one output plane: lo in the accurate mode, hi in bf16 mode)
  g.epi = SF_EPI_BF16; g.K = e->D; g.N = g.ldc = 3 * e->D;
  if (!sf_gemm256_supported(g, split)) return false;
  g.epi = SF_EPI_ACT_BF16; g.N = g.ldc = e->I;
  return sf_gemm256_supported(g, split);
}
static bool ln_fold_acc_ok(const sf_encoder* e, int M) {
  return e->compute == SF_COMPUTE_BF16X3 && !sf_sw(SW_DISABLE_ACC_FOLD) && ln_fold_planes_g256_ok(e, M, true);
}
static bool ln_fold_g256_ok(const sf_encoder* e, int M) {
  return e->compute == SF_COMPUTE_BF16 && !sf_sw(SW_DISABLE_LN_FOLD) && ln_fold_planes_g256_ok(e, M, false);
}

// Small M (the per-frame streaming step): the skinny GEMM derives the row statistics itself from the A fragments it reads anyway,
// every residual producer only adds the bf16 copy of its output rows.  Accurate mode: the consumers take x as hi + lo planes and sum
// the statistics of hi + lo (32 x 32 skinny kernel only).  SF_DISABLE_STREAM_FOLD: A/B.
static bool ln_fold_small_ok(const sf_encoder* e, int M) {
  if (M > sf_infold_max_rows() || sf_sw(SW_DISABLE_STREAM_FOLD)) return false;
  const bool acc = e->compute == SF_COMPUTE_BF16X3;
  auto takes = [acc](const SfGemmArgs& g) { return sf_gemm_skinny_supported(g, acc) || (!acc && sf_gemm_tile_supported(g, false)); };
  SfGemmArgs g = probe_args(e, M, 3 * e->D, e->D, acc ? SF_EPI_F32 : SF_EPI_BF16);
  if (acc) { g.a_lo = kSetB; g.w_lo = kSetB; g.out_lo = kSetB; g.out_f32 = kSetF; }
  g.ln_inkernel = 1; g.ln_s = kSetF; g.out_hi = kSetB;
  if (!takes(g)) return false;
  g.epi = SF_EPI_ACT_BF16; g.N = g.ldc = e->I;
  if (!takes(g)) return false;
  g.ln_inkernel = 0; g.ln_s = nullptr; g.epi = SF_EPI_RESID_F32; g.N = g.ldc = e->D;      // producers (they add the bf16 copy)
  g.out_f32 = kSetF; g.resid = kSetF;
  return takes_both_k(e, g, takes);
}

// the head's per-frame tail on one to four rows runs as row-vector launches (sf_launch_rowlin)
static bool sf_head_rows_ok(const sf_encoder* e, int F) {
  return e->head_out.w_lo && e->head_fc1.w_lo && e->head_fc2.w_lo && sf_rowlin_supported(F, e->D, e->D) && sf_rowlin_supported(F, e->I, e->D) &&
         sf_rowlin_supported(F, e->D, e->I);
}

// T <= 256 (SfRowIndex): every entry point has checked it (the streaming entry through the cache capacity)
static int time_rows(const sf_encoder* e, int t_past, int T, bool streaming, SfRowIndex* idx) {
  const int nf = e->cfg.num_frames;
  idx->n = T;
  if (streaming) {
    // vqa_enc:328-369: direct rows; the reference raises past num_frames rows
    if (t_past + T > nf)
      return sf_set_err(SF_ERR_CAPACITY, "streaming needs time-embedding row %d but config.num_frames is %d", t_past + T - 1, nf);
    for (int t = 0; t < T; ++t) idx->idx[t] = t_past + t;
  } else if (T <= nf) {
    for (int t = 0; t < T; ++t) idx->idx[t] = t;          // modeling:436-439 slice
  } else {
    // F.interpolate(mode="nearest") (modeling:441-447): src = floor(dst * scale), scale = float(in)/out
    const float scale = (float)nf / (float)T;
    for (int t = 0; t < T; ++t) {
      int src = (int)floorf((float)t * scale);
      idx->idx[t] = src < nf - 1 ? src : nf - 1;
    }
  }
  return SF_OK;
}

// What the row count alone decides about the bf16-mode schedule: true when the residual projections at M rows run on hi + lo planes
// with LayerNorm row sums for the next folded Linear (ForwardPlan's `fold + pm`).  plan_forward asks further for what a request and
// its workspace must allow (a complete forward of whole clips on the panel embedding route); sf_bench_gemm times the projection
// alone and takes this answer as it is.  fs: the folds the answer was made from.
bool resid_planes_at(const sf_encoder* e, int M, FoldShape* fs) {
  FoldShape f;
  f.tile_fold = ln_fold_tile_ok(e, M); f.small_fold = ln_fold_small_ok(e, M);
  f.stats_fold = f.tile_fold || (!f.small_fold && ln_fold_panel_ok(e, M));
  if (fs) *fs = f;
  return f.stats_fold && !f.tile_fold && e->compute != SF_COMPUTE_BF16X3 && !sf_sw(SW_DISABLE_RESID_PLANES);
}

ForwardPlan plan_forward(const sf_encoder* e, const ForwardRequest& rq, const Workspace& ws) {
  ForwardPlan p = {};
  p.rq = rq;
  if (p.rq.lb < 0) p.rq.lb = e->L;
  const int D = e->D, T = rq.T, stages = rq.stages;
  const int N = (rq.H / e->cfg.patch_size) * (rq.W / e->cfg.patch_size), M = rq.B * T * N;
  const bool acc = e->compute == SF_COMPUTE_BF16X3, streaming = rq.streaming;
  const bool complete = (stages & 7) == 7 && !rq.hidden_states;      // the fp32 tensor is the interface of the stage-wise entry points
  p.N = N; p.M = M; p.F = rq.B * T; p.acc = acc;
  p.qkv_epi = acc ? SF_EPI_F32 : SF_EPI_BF16; p.esz = acc ? 4 : 2;
  p.scale = 1.0f / sqrtf((float)e->hd);
  p.t_row = rq.pos ? rq.pos->t_row : rq.t_past; p.slot = rq.pos ? rq.pos->slot : rq.t_past; p.tk = rq.pos ? rq.pos->tk : rq.t_past + T;

  FoldShape fs;
  const bool resid_planes = resid_planes_at(e, M, &fs);
  const bool tile_fold = fs.tile_fold, small_fold = fs.small_fold, stats_fold = fs.stats_fold;
  const bool small_bufs = ws.res_bf && (!acc || ws.res_lo) && small_fold;
  p.zero_stats = stats_fold && !streaming && (stages & 3);

  // ---- embeddings.  Panel route: out = table[m % (T N)] + patches W^T + b with table = pos + time rows; pm asks it for plane outputs
  const bool panel_embed = stats_fold && !streaming && (stages & 2) && ws.embed_tab && ws.patch_buf && e->Kp % 32 == 0 && e->Kp >= 128 && D == 768 &&
                           !sf_sw(SW_EMBED_VIA_GEMM128);
  const bool pm_wanted = panel_embed && resid_planes && complete && ws.res_lo;      // (panel_embed has stats_fold in it)
  if (stages & 1) {
    p.patches = panel_embed ? ws.patch_buf : ws.xn_hi;
    SfGemmArgs g;
    memset(&g, 0, sizeof(g));
    g.a_hi = p.patches; g.a_lo = acc ? ws.xn_lo : nullptr;
    g.w_hi = e->patch.w_hi; g.w_lo = acc ? e->patch.w_lo : nullptr;
    g.bias = e->patch.bias;
    g.M = M; g.N = D; g.K = e->Kp;
    g.out_f32 = ws.resid; g.ldc = D;
    SfGemmArgs gp = g;
    gp.epi = SF_EPI_RESID_F32; gp.alpha = 1.f; gp.resid = ws.embed_tab; gp.resid_mod = T * N;
    gp.out_hi = ws.xn_hi; gp.ln_stats_out = ws.ln_stats; gp.ln_stats_wide = 1;
    if (pm_wanted) {
      SfGemmArgs gq = gp;
      gq.out_f32 = nullptr; gq.out_lo = ws.res_lo;
      p.pm = sf_gemm_panel_supported(gq, false);
      if (p.pm) gp = gq;
    }
    // pos + time rows added in the epilogue: the statistics-producing narrow tile (tile-fold), or whatever sf_launch_gemm picks
    g.epi = SF_EPI_EMBED_F32; g.pos = rq.pos_dev ? rq.pos_dev : e->pos; g.time_rows = ws.te_rows; g.Np = N; g.Tn = rq.tab ? rq.B : T;      // ragged call: one gathered time row per group
    SfGemmArgs gt = g;
    gt.out_hi = ws.xn_hi; gt.ln_stats_out = ws.ln_stats; gt.ln_stats_wide = 1;
    if (!acc && !streaming && (stages & 2) && p.patches != ws.xn_hi && tile_fold && sf_gemm_tile_supported(gt, false)) {      // (A must not alias out_hi)
      p.embed_route = EMBED_TILE; p.embed = gt;
    } else if (panel_embed && sf_gemm_panel_supported(gp, false)) {
      p.embed_route = EMBED_PANEL; p.embed = gp;
    } else {
      // streamed frame inside the position-free graph: the time-embedding row straight from the table — exactly when sf_launch_gemm
      // takes the skinny kernel
      p.time_folded = rq.sp && T == 1 && !stats_fold && !sf_sw(SW_DISABLE_SKINNY) && sf_gemm_skinny_supported(g, acc);
      if (p.time_folded) { g.time_rows = e->time_tab; g.time_base_dev = &rq.sp->t_row; g.grp_tab = rq.tab; }
      if (small_bufs && (stages & 2)) { g.out_hi = ws.res_bf; if (acc) g.out_lo = ws.res_lo; }   // layer 0's folded qkv reads bf16(x) (accurate: hi + lo)
      p.embed_route = EMBED_GEMM; p.embed = g;
    }
  }

  // ---- the schedule of the layers
  p.tplanes = acc && !rq.layer_tqkv && rq.cap == T && rq.t_past == 0 && sf_temporal_planes_ok(T, T);
  p.planes = acc && sf_spatial_planes_ok(N, rq.attentions != nullptr);
  p.tsz = p.tplanes ? 2 : p.esz; p.sesz = p.planes ? 2 : p.esz;
  p.fold = stats_fold && !streaming;
  p.sfold = !p.fold && small_bufs;
  p.xm = p.tplanes && p.planes && !streaming && complete && ln_fold_acc_ok(e, M);
  p.gm = !acc && !p.fold && !p.sfold && !streaming && complete && ws.res_lo != nullptr && ln_fold_g256_ok(e, M);
  p.anyfold = p.fold || p.sfold || p.xm || p.gm;
  p.rplanes = p.pm || p.xm || p.gm;
  p.seed_stats = p.fold && (stages & 2) && p.embed_route != EMBED_TILE && p.embed_route != EMBED_PANEL;
  p.seed_split = p.sfold && (stages & 2) && !(stages & 1) && !(rq.ready & 2);
  p.resid = p.rplanes ? nullptr : ws.resid;
  p.fold_hi = (p.fold || p.xm || p.gm) ? ws.xn_hi : (p.sfold ? ws.res_bf : nullptr);
  p.fold_st = (p.fold || p.xm || p.gm) ? ws.ln_stats : nullptr;
  p.plo = (p.pm || p.gm) ? ws.res_lo : (p.xm ? ws.xn_lo : ((p.sfold && acc) ? ws.res_lo : nullptr));
  p.plo2 = (p.xm && !sf_sw(SW_ACC_TWO_PLANES)) ? ws.res_lo2 : nullptr;      // A/B: drop the third plane (max-abs 1.4e-4 instead of 5e-5)
  p.ln_in = p.sfold ? ws.res_bf : ws.xn_hi;
  p.ln_in_lo = (p.sfold && acc) ? ws.res_lo : ws.xn_lo;

  p.head_generic = e->hd != 64 || D > 1024;
  p.head_rows = rq.pooler && sf_head_rows_ok(e, p.F);
  return p;
}

// a residual producer: x += alpha (A W^T + b) in the plan's form of the residual stream, with what the next folded consumer needs
static hipError_t launch_resid_linear(const sf_encoder* e, const ForwardPlan& p, const DevLinear& lin, const bf16_t* a_hi, const bf16_t* a_lo,
                                      float alpha, hipStream_t s) {
  SfGemmArgs g = linear_args(e, lin, a_hi, a_lo, p.M, SF_EPI_RESID_F32, p.acc);
  g.alpha = alpha;
  g.resid = p.resid; g.out_f32 = p.resid;
  g.resid_hi = p.rplanes ? p.fold_hi : nullptr; g.resid_lo = p.plo; g.resid_lo2 = p.plo2;
  g.out_hi = p.fold_hi; g.out_lo = p.plo; g.out_lo2 = p.plo2;       // planes: in place; otherwise the bf16 copy of the new rows
  g.ln_stats_out = p.fold_st;
  return sf_launch_gemm(g, p.acc, s);
}

// one of the three Linears behind a LayerNorm: the folded weights on the plan's operand, or the plain ones on LayerNorm's output
static SfGemmArgs ln_linear_args(const sf_encoder* e, const ForwardPlan& p, const DevLinear& plain, const DevLinear& folded, int epi) {
  const DevLinear& lin = p.anyfold ? folded : plain;
  SfGemmArgs g = linear_args(e, lin, p.ln_in, p.ln_in_lo, p.M, epi, p.acc);
  g.ln_stats = p.fold_st; g.ln_inkernel = p.sfold;
  g.ln_s = (p.fold_st || p.sfold) ? lin.ln_s : nullptr;
  return g;
}
// q / k / v leave their GEMM as bf16, fp32 (accurate), or hi + lo bf16 planes in the bytes of the fp32 tensor
static void set_qkv_out(SfGemmArgs& g, void* qkv, bool planes, const ForwardPlan& p) {
  if (planes) g.epi = SF_EPI_BF16;
  g.out_f32 = (float*)qkv; g.out_hi = (bf16_t*)qkv;
  g.out_lo = planes ? (bf16_t*)qkv + (size_t)p.M * g.N : nullptr;
}
static void set_qkv_in(SfAttnArgs& a, const sf_encoder* e, void* qkv, bool planes, size_t esz, const ForwardPlan& p, const Workspace& ws) {
  const int D = e->D;
  a.q = qkv; a.k = (char*)qkv + (size_t)D * esz; a.v = (char*)qkv + (size_t)2 * D * esz;
  a.in_is_f32 = p.acc && !planes; a.lo_plane_off = planes ? (long long)p.M * 3 * D : 0;
  a.row_pitch_q = 3 * D; a.row_pitch_kv = 3 * D; a.heads = e->cfg.num_attention_heads; a.scale = p.scale; a.head_dim = e->hd;
  a.N = p.N; a.ctx_hi = ws.ctx_hi; a.ctx_lo = ws.ctx_lo; a.D = D;
}

// ---- stage 1: patch + position + time embeddings -> ws.resid (pm: -> the planes)
static int forward_embeddings(sf_encoder* e, const ForwardPlan& p, const Workspace& ws, hipStream_t s) {
  const ForwardRequest& rq = p.rq;
  const sf_config& c = e->cfg;
  SfRowIndex idx;
  int rc = rq.tab ? SF_OK : time_rows(e, p.t_row, rq.T, rq.streaming, &idx);      // (ragged call: the entry point has checked every stream's row)
  if (rc) return rc;
  if (rq.sp) { for (int t = 0; t < rq.T; ++t) idx.idx[t] = t; }
  if (rq.tab) idx.n = rq.B;
  if (!p.time_folded) HIP_TRY(sf_launch_gather_rows(e->time_tab, ws.te_rows, idx, e->D, s, rq.sp ? &rq.sp->t_row : nullptr, rq.tab));
  if (!(rq.ready & 1))
    HIP_TRY(sf_launch_patchify(rq.pixels, rq.pixel_dtype == SF_U8 ? 2 : (rq.pixel_dtype == SF_BF16 ? 1 : 0), p.patches, ws.xn_lo, p.F, c.num_channels, rq.H, rq.W,
                               c.patch_size, s, &e->pixel_norm, nullptr, nullptr, nullptr, e->Kp));
  if (p.embed_route == EMBED_TILE) {
    HIP_TRY(sf_launch_gemm_tile(p.embed, s));
  } else if (p.embed_route == EMBED_PANEL) {
    HIP_TRY(sf_launch_pos_time_table(rq.pos_dev ? rq.pos_dev : e->pos, ws.te_rows, ws.embed_tab, rq.T, p.N, e->D, s));
    HIP_TRY(sf_launch_gemm_panel(p.embed, s));
  } else {
    HIP_TRY(sf_launch_gemm(p.embed, p.acc, s));
  }
  return SF_OK;
}

// ---- stage 2: one layer on the residual stream
static int forward_layer(sf_encoder* e, const ForwardPlan& p, const Workspace& ws, int li, hipStream_t s) {
  const ForwardRequest& rq = p.rq;
  const sf_config& c = e->cfg;
  const DevLayer& l = e->layers[li];
  const int D = e->D, M = p.M, N = p.N, T = rq.T, heads = c.num_attention_heads;
  const bool acc = p.acc;
  const SfStreamParams* sp = rq.sp;
  if (rq.hidden_states)
    HIP_TRY(hipMemcpyAsync(rq.hidden_states + (size_t)li * M * D, ws.resid, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s));
  // ---- temporal attention (modeling:937-958) ---------------------------------------------------
  if (!p.anyfold) HIP_TRY(sf_launch_layernorm(ws.resid, l.ln_t.g, l.ln_t.b, nullptr, ws.xn_hi, ws.xn_lo, M, D, c.layer_norm_eps, s));
  void* tq = rq.layer_tqkv ? rq.layer_tqkv[li] : ws.tqkv;
  // lab library, SF_QKV_FUSED=1 (bf16 mode, whole 16-frame clips, no cache): qkv projection + temporal attention in ONE launch
  // (sf_gemm_qkv.hip; bit-identical, -0.27 ms of kernel time per forward under rocprof, +0.07 ms on the wall clock: docs/history.md H.4)
  bool t_fused_attn = false;
#ifdef SF_LAB
  if (p.fold && !acc && !rq.layer_tqkv && rq.cap == T && rq.t_past == 0 && p.tk == T && !sp && l.t_qkv_fp.w_hi) {
    SfQkvArgs q;
    memset(&q, 0, sizeof(q));
    q.a = p.ln_in; q.w = l.t_qkv_fp.w_hi; q.bias = l.t_qkv_fp.bias; q.ln_s = l.t_qkv_fp.ln_s; q.ln_stats = p.fold_st; q.ln_eps = c.layer_norm_eps;
    q.M = M; q.K = D; q.D = D; q.B = rq.B; q.T = T; q.NP = N; q.out = ws.ctx_hi; q.scale = p.scale; q.causal = c.enable_causal_temporal;
    if (sf_gemm_qkv_supported(q, true)) {
      HIP_TRY(prof_span(e, 3, s, [&]() { return sf_launch_gemm_qkv(q, true, s); }));
      t_fused_attn = true;
    }
  }
#endif
#ifdef SF_LAB
  // lab library, SF_STREAM_QKV_FUSE=1 (one streamed frame per stream, bf16 mode, cache of <= 64 frames): projection + cache append +
  // single-query attention in one launch (tools/lab/sf_stream_fused.hip; bit-identical, 15.0 against 6.1 + 7.4 us: a CU's ingest)
  if (!t_fused_attn && p.sfold && !acc && T == 1 && rq.layer_tqkv && l.t_qkv_f.ln_s && !rq.tab) {
    SfStreamQkvArgs q;
    memset(&q, 0, sizeof(q));
    q.a = p.ln_in; q.w_frag = l.t_qkv_f.w_frag; q.bias = l.t_qkv_f.bias; q.ln_s = l.t_qkv_f.ln_s; q.ln_eps = c.layer_norm_eps;
    q.M = M; q.K = l.t_qkv_f.K; q.D = D; q.heads = heads; q.N = N;
    q.cache = (bf16_t*)tq; q.cap = rq.cap; q.slot = p.slot; q.Tk = p.tk; q.pos_dev = sp ? &sp->slot : nullptr;
    q.ctx = ws.ctx_hi; q.scale = p.scale;
    if (l.t_qkv_f.N == 3 * D && sf_stream_qkv_decode_supported(q)) {
      HIP_TRY(prof_span(e, 3, s, [&]() { return sf_launch_stream_qkv_decode(q, s); }));
      t_fused_attn = true;
    }
  }
#endif
  if (!t_fused_attn) {
    SfGemmArgs g = ln_linear_args(e, p, l.t_qkv, l.t_qkv_f, p.qkv_epi);
    set_qkv_out(g, tq, p.tplanes, p);
    // the new frames' rows go to their slots of the [B, cap, N, 3D] cache (position from the device block inside the position-free graph)
    g.grp_rows = T * N; g.grp_stride = rq.cap * N; g.grp_off = sp ? 0 : p.slot * N;
    g.grp_off_dev = sp ? &sp->slot : nullptr; g.grp_off_scale = N;
    g.grp_tab = rq.tab;                                                                    // ragged call: slab and slot per row group
    if (g.grp_stride == g.grp_rows && g.grp_off == 0 && !g.grp_off_dev) g.grp_rows = 0;   // identity remap (full clip)
    HIP_TRY(sf_launch_gemm(g, acc, s));
    SfAttnArgs a;
    memset(&a, 0, sizeof(a));
    set_qkv_in(a, e, tq, p.tplanes, p.tsz, p, ws);
    a.B = rq.B; a.Tq = T; a.Tk = p.tk; a.Tcap = rq.cap; a.t_past = p.tk - T;
    a.causal = c.enable_causal_temporal; a.Tq_cap = rq.cap; a.q_t0 = p.slot;
    a.pos_dev = sp ? &sp->slot : nullptr; a.tab = rq.tab;
    HIP_TRY(prof_span(e, 3, s, [&]() { return sf_launch_temporal_attention(a, acc, s); }));
  }
  if (e->fused_temporal) {
    HIP_TRY(prof_span(e, 0, s, [&]() { return launch_resid_linear(e, p, l.t_fused, ws.ctx_hi, ws.ctx_lo, l.gate_tanh, s); }));
  } else {
    SfGemmArgs g = linear_args(e, l.t_out, ws.ctx_hi, ws.ctx_lo, M, SF_EPI_BF16, acc);
    g.out_hi = ws.tmp_hi; g.out_lo = ws.tmp_lo;
    HIP_TRY(sf_launch_gemm(g, acc, s));
    HIP_TRY(launch_resid_linear(e, p, l.t_dense, ws.tmp_hi, ws.tmp_lo, l.gate_tanh, s));
  }
  // ---- spatial attention (modeling:962-996) ------------------------------------------------------
  if (!p.anyfold) HIP_TRY(sf_launch_layernorm(ws.resid, l.ln_b.g, l.ln_b.b, nullptr, ws.xn_hi, ws.xn_lo, M, D, c.layer_norm_eps, s));
  // lab library, SF_SQKV_PANEL=1: the folded spatial qkv projection on the panel tile (768 tiles of 196 x 384 = three whole rounds)
  bool s_qkv_panel = false;
#ifdef SF_LAB
  static const bool s_panel_on = SF_LAB_SWITCH("SF_SQKV_PANEL") != 0;
  if (s_panel_on && p.fold && !acc && p.qkv_epi == SF_EPI_BF16 && l.s_qkv_f.ln_s) {
    SfQkvArgs q;
    memset(&q, 0, sizeof(q));
    q.a = p.ln_in; q.w = l.s_qkv_f.w_hi; q.bias = l.s_qkv_f.bias; q.ln_s = l.s_qkv_f.ln_s; q.ln_stats = p.fold_st; q.ln_eps = c.layer_norm_eps;
    q.M = M; q.K = D; q.D = D; q.out = (bf16_t*)ws.qkv;
    if (sf_gemm_qkv_supported(q, false)) {
      HIP_TRY(sf_launch_gemm_qkv(q, false, s));
      s_qkv_panel = true;
    }
  }
#endif
  if (!s_qkv_panel) {
    SfGemmArgs g = ln_linear_args(e, p, l.s_qkv, l.s_qkv_f, p.qkv_epi);
    set_qkv_out(g, ws.qkv, p.planes, p);
    HIP_TRY(sf_launch_gemm(g, acc, s));
  }
  {
    SfAttnArgs a;
    memset(&a, 0, sizeof(a));
    set_qkv_in(a, e, ws.qkv, p.planes, p.sesz, p, ws);
    a.frames = p.F;
    a.probs = rq.attentions ? rq.attentions + (size_t)(li - rq.la) * p.F * heads * N * N : nullptr;
    HIP_TRY(prof_span(e, 2, s, [&]() { return sf_launch_spatial_attention(a, acc, s); }));
  }
  HIP_TRY(prof_span(e, 0, s, [&]() { return launch_resid_linear(e, p, l.s_out, ws.ctx_hi, ws.ctx_lo, 1.f, s); }));
  // ---- MLP (modeling:997-1000) ---------------------------------------------------------------------
  if (!p.anyfold) HIP_TRY(sf_launch_layernorm(ws.resid, l.ln_a.g, l.ln_a.b, nullptr, ws.xn_hi, ws.xn_lo, M, D, c.layer_norm_eps, s));
  {
    SfGemmArgs g = ln_linear_args(e, p, l.up, l.up_f, SF_EPI_ACT_BF16);
    g.out_hi = ws.mid_hi; g.out_lo = ws.mid_lo;
    HIP_TRY(sf_launch_gemm(g, acc, s));
  }
  HIP_TRY(prof_span(e, 1, s, [&]() { return launch_resid_linear(e, p, l.down, ws.mid_hi, ws.mid_lo, 1.f, s); }));
  return SF_OK;
}

// ---- stages 4 / 8: post LayerNorm + pooling head (modeling:1330-1340, 1141-1154)
// (the head reads the fp32 tokens: no bf16 copy of the normalised rows is written)
static int forward_post_head(sf_encoder* e, const ForwardPlan& p, const Workspace& ws, hipStream_t s) {
  const ForwardRequest& rq = p.rq;
  const sf_config& c = e->cfg;
  const int D = e->D, F = p.F, N = p.N, heads = c.num_attention_heads;
  const SfStreamParams* sp = rq.sp;
  if (rq.stages & 4)       // plane forms: the rows arrive as the planes of the residual stream
    HIP_TRY(sf_launch_layernorm(ws.resid, e->post_ln.g, e->post_ln.b, rq.last_hidden, nullptr, nullptr, p.M, D, c.layer_norm_eps, s,
                                p.rplanes ? ws.xn_hi : nullptr, p.plo, p.plo2, sp ? &sp->lhs : nullptr));   // sp: straight into the caller's tensor
  if (!rq.pooler) return SF_OK;
  // The probe attention without projecting the tokens (sf_pool_head.hip): scores = x . U, z_h = sum_n p_hn x_n on the fp32
  // tokens, ctx_h = Wv_h z_h + bv_h — bf16x3 / fp32 arithmetic in BOTH modes (the [M, 2D] k / v tensor and its 59 GFLOP are gone).
  // stage 8: the head alone on tokens the caller has already normalised (model.head(x)): they sit in ws.resid
  const float* tok = (rq.stages & 4) ? rq.last_hidden : ws.resid;
  const float* const* tok_ind = (sp && (rq.stages & 4)) ? reinterpret_cast<const float* const*>(&sp->lhs) : nullptr;
  if (p.head_generic) {      // the whole probe attention of a frame in one fp32 workgroup
    SfPoolGenArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.x = tok; ga.x_ind = tok_ind;
    ga.u = e->head_u; ga.wv = e->head_wv; ga.ldw = D; ga.bv = e->head_bv;
    ga.F = F; ga.N = N; ga.heads = heads; ga.hd = e->hd; ga.D = D;
    ga.scratch = ws.pool_z;
    if (p.head_rows) ga.ctx_f32 = ws.head_ctx; else { ga.ctx_hi = ws.pc_hi; ga.ctx_lo = ws.pc_lo; }
    HIP_TRY(sf_launch_pool_generic(ga, s));
  } else {
    SfPoolArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.x = tok; pa.x_ind = tok_ind;
    pa.u_hi = e->head_u_hi; pa.u_lo = e->head_u_lo; pa.zpart = ws.pool_z; pa.ml = ws.pool_ml;
    pa.F = F; pa.N = N; pa.heads = heads; pa.D = D; pa.S = sf_pool_splits(F, N, heads); pa.normalize = pa.S == 1;
    HIP_TRY(sf_launch_pool_probe(pa, s));
    SfPoolCtxArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.zpart = ws.pool_z; ca.ml = ws.pool_ml; ca.wv = e->head_wv; ca.ldw = D; ca.bv = e->head_bv;
    ca.ctx_hi = ws.pc_hi; ca.ctx_lo = ws.pc_lo; ca.F = F; ca.heads = heads; ca.D = D; ca.S = pa.S;
    if (p.head_rows) { ca.ctx_hi = ca.ctx_lo = nullptr; ca.ctx_f32 = ws.head_ctx; }
    HIP_TRY(sf_launch_pool_ctx(ca, s));
  }
  if (p.head_rows) {
    // One to four rows (streamed frames): the per-frame tail as three row-vector launches with fp32 activations — out_proj,
    // LayerNorm + fc1 + GELU, fc2 + residual (written straight into the caller's pooler_output inside the position-free graph)
    SfRowLinArgs r;
    memset(&r, 0, sizeof(r));
    r.F = F; r.act = -1;
    r.x = ws.head_ctx; r.ldx = D; r.K = D; r.N = D; r.w_hi = e->head_out.w_hi; r.w_lo = e->head_out.w_lo; r.bias = e->head_out.bias;
    r.out = ws.attn_out; r.ldo = D;
    HIP_TRY(sf_launch_rowlin(r, s));
    r.x = ws.attn_out; r.ln_g = e->head_ln.g; r.ln_b = e->head_ln.b; r.ln_eps = c.layer_norm_eps; r.N = e->I; r.act = c.hidden_act;
    r.w_hi = e->head_fc1.w_hi; r.w_lo = e->head_fc1.w_lo; r.bias = e->head_fc1.bias; r.out = ws.head_mid; r.ldo = e->I;
    HIP_TRY(sf_launch_rowlin(r, s));
    r.x = ws.head_mid; r.ldx = e->I; r.K = e->I; r.N = D; r.ln_g = r.ln_b = nullptr; r.act = -1;
    r.w_hi = e->head_fc2.w_hi; r.w_lo = e->head_fc2.w_lo; r.bias = e->head_fc2.bias; r.resid = ws.attn_out; r.ldr = D;
    r.out = rq.pooler; r.ldo = D; r.out_ind = sp ? &sp->pooler : nullptr;
    HIP_TRY(sf_launch_rowlin(r, s));
    return SF_OK;
  }
  // one row per frame from here on (F rows: 0.03 % of the forward's FLOPs): hi + lo planes and three bf16 products per operand pair in
  // BOTH modes (the head's Linears keep their lo plane in bf16 mode too) — pooler_output is the product both loss heads and the feature
  // dumps consume, and the bf16 mode's own head added 1.5e-2 of max-abs error to it on top of what the encoder's tokens carry
  // (tools/pool_err.py)
  SfGemmArgs g = linear_args(e, e->head_out, ws.pc_hi, ws.pc_lo, F, SF_EPI_F32, true);
  g.out_f32 = ws.attn_out;
  HIP_TRY(sf_launch_gemm(g, true, s));
  HIP_TRY(sf_launch_layernorm(ws.attn_out, e->head_ln.g, e->head_ln.b, nullptr, ws.hn_hi, ws.hn_lo, F, D, c.layer_norm_eps, s));
  g = linear_args(e, e->head_fc1, ws.hn_hi, ws.hn_lo, F, SF_EPI_ACT_BF16, true);
  g.out_hi = ws.hm_hi; g.out_lo = ws.hm_lo;
  HIP_TRY(sf_launch_gemm(g, true, s));
  g = linear_args(e, e->head_fc2, ws.hm_hi, ws.hm_lo, F, SF_EPI_RESID_F32, true);
  g.out_f32 = rq.pooler; g.resid = ws.attn_out;
  HIP_TRY(sf_launch_gemm(g, true, s));
  return SF_OK;
}

// One call of the encoder over T new frames, as planned.
int run_plan(sf_encoder* e, const ForwardPlan& p, const Workspace& ws, hipStream_t s) {
  const ForwardRequest& rq = p.rq;
  const size_t hs_stride = (size_t)p.M * e->D;
  int rc;
  if (p.zero_stats) HIP_TRY(hipMemsetAsync(ws.ln_stats, 0, (size_t)p.M * 8 * sizeof(float), s));
  if ((rq.stages & 1) && (rc = forward_embeddings(e, p, ws, s))) return rc;
  // what the schedule reads that the embeddings (or the caller of sf_layers) left as fp32 rows only
  if (p.seed_stats) HIP_TRY(sf_launch_rowstats_cast(ws.resid, ws.xn_hi, ws.ln_stats, p.M, e->D, s, nullptr, nullptr, 1));
  if (p.xm) HIP_TRY(sf_launch_rowstats_cast(ws.resid, ws.xn_hi, ws.ln_stats, p.M, e->D, s, ws.xn_lo, p.plo2));      // embeddings -> planes + wide statistics
  if (p.gm) HIP_TRY(sf_launch_rowstats_cast(ws.resid, ws.xn_hi, ws.ln_stats, p.M, e->D, s, ws.res_lo, nullptr));
  if (p.seed_split) HIP_TRY(sf_launch_split(ws.resid, ws.res_bf, p.acc ? ws.res_lo : nullptr, hs_stride, s));
  if (rq.stages & 2) {
    for (int li = rq.la; li < rq.lb; ++li)
      if ((rc = forward_layer(e, p, ws, li, s))) return rc;
    if (rq.hidden_states && rq.lb == e->L)
      HIP_TRY(hipMemcpyAsync(rq.hidden_states + (size_t)e->L * hs_stride, ws.resid, hs_stride * 4, hipMemcpyDeviceToDevice, s));
  }
  return (rq.stages & 12) ? forward_post_head(e, p, ws, s) : SF_OK;
}
int run_forward(sf_encoder* e, const ForwardRequest& rq, const Workspace& ws, hipStream_t s) {
  return run_plan(e, plan_forward(e, rq, ws), ws, s);
}

int check_geometry(const sf_encoder* e, int B, int T, int H, int W, const float* pos_dev, int* N_out) {
  if (!e) return sf_set_err(SF_ERR_INVALID, "null handle");
  const int P = e->cfg.patch_size;
  if (B <= 0 || T <= 0 || H < P || W < P) return sf_set_err(SF_ERR_INVALID, "bad geometry B=%d T=%d H=%d W=%d", B, T, H, W);
  const int N = (H / P) * (W / P);
  if (N > 2048) return sf_set_err(SF_ERR_INVALID, "%d patches per frame; the attention kernels handle <= 2048", N);
  if (!pos_dev && !(N == e->N && H == W))
    return sf_set_err(SF_ERR_INVALID, "input %dx%d differs from image_size %d: pass a resized position table (pos_dev)", H, W, e->cfg.image_size);
  if ((size_t)B * T * N > (size_t)1 << 30) return sf_set_err(SF_ERR_INVALID, "too many token rows");
  *N_out = N;
  return SF_OK;
}

extern "C" int sf_workspace_bytes(sf_encoder* e, int B, int T, int H, int W, size_t* out) {
  int N;
  const float* dummy = (const float*)1;
  int rc = check_geometry(e, B, T, H, W, dummy, &N);
  if (rc) return rc;
  if (!out) return sf_set_err(SF_ERR_INVALID, "null out");
  if (!e->finalized) return sf_set_err(SF_ERR_STATE, "sf_finalize_weights has not run");
  *out = carve(e, nullptr, B, T, N, true).bytes;
  return SF_OK;
}

static int forward_common(sf_encoder* e, const void* pixels, int pixel_dtype, int B, int T, int H, int W, float* last_hidden,
                          float* pooler, float* hidden_states, float* attentions, const float* pos_dev, void* workspace,
                          size_t workspace_bytes, sf_stream stream) {
  int N;
  int rc = check_geometry(e, B, T, H, W, pos_dev, &N);
  if (rc) return rc;
  if (!e->finalized) return sf_set_err(SF_ERR_STATE, "sf_finalize_weights has not run");
  if (!pixels || !last_hidden || !workspace) return sf_set_err(SF_ERR_INVALID, "null buffer");
  if (pixel_dtype != SF_F32 && pixel_dtype != SF_BF16 && pixel_dtype != SF_U8) return sf_set_err(SF_ERR_INVALID, "pixels must be fp32, bf16 or uint8");
  if (T > 256) return sf_set_err(SF_ERR_INVALID, "at most 256 frames per clip");
  Workspace ws = carve(e, workspace, B, T, N, true);
  if (ws.bytes > workspace_bytes) return sf_set_err(SF_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, ws.bytes);
  ForwardRequest rq;
  rq.pixels = pixels; rq.pixel_dtype = pixel_dtype; rq.B = B; rq.T = T; rq.H = H; rq.W = W; rq.pos_dev = pos_dev;
  rq.last_hidden = last_hidden; rq.pooler = pooler; rq.hidden_states = hidden_states; rq.attentions = attentions;
  rq.cap = T;
  return run_forward(e, rq, ws, (hipStream_t)stream);
}

extern "C" int sf_forward(sf_encoder* e, const void* pixels, int pixel_dtype, int B, int T, int H, int W,
                          float* last_hidden, float* pooler, float* hidden_states, const float* pos_dev,
                          void* workspace, size_t workspace_bytes, sf_stream stream) {
  return forward_common(e, pixels, pixel_dtype, B, T, H, W, last_hidden, pooler, hidden_states, nullptr, pos_dev, workspace,
                        workspace_bytes, stream);
}

// One forward with HIP events around the launches of four kernel classes (see sf_encoder::prof): the in-situ launch durations the
// bench's roofline reports — isolated back-to-back launches of the same kernel run on an Infinity-Cache-warm working set and read
// 4 % faster.  out_ms[2 c] = mean milliseconds per launch of class c, out_ms[2 c + 1] = launches of that class.
extern "C" int sf_forward_profile(sf_encoder* e, const void* pixels, int pixel_dtype, int B, int T, int H, int W, float* last_hidden,
                                  float* pooler, void* workspace, size_t workspace_bytes, sf_stream stream, float* out_ms) {
  if (!e || !out_ms) return sf_set_err(SF_ERR_INVALID, "null argument");
  e->prof.clear();
  e->prof_on = true;
  int rc = forward_common(e, pixels, pixel_dtype, B, T, H, W, last_hidden, pooler, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream);
  e->prof_on = false;
  hipError_t se = hipStreamSynchronize((hipStream_t)stream);
  double sum[4] = {0, 0, 0, 0};
  int cnt[4] = {0, 0, 0, 0};
  for (auto& sp : e->prof) {
    float ms = 0.f;
    if (rc == SF_OK && se == hipSuccess && hipEventElapsedTime(&ms, sp.e0, sp.e1) == hipSuccess && sp.cls >= 0 && sp.cls < 4) { sum[sp.cls] += ms; cnt[sp.cls]++; }
    (void)hipEventDestroy(sp.e0);
    (void)hipEventDestroy(sp.e1);
  }
  e->prof.clear();
  for (int c = 0; c < 4; ++c) { out_ms[2 * c] = cnt[c] ? (float)(sum[c] / cnt[c]) : 0.f; out_ms[2 * c + 1] = (float)cnt[c]; }
  if (rc != SF_OK) return rc;
  if (se != hipSuccess) return sf_set_err(SF_ERR_HIP, "sf_forward_profile: %s", hipGetErrorString(se));
  return SF_OK;
}

extern "C" int sf_forward_attentions(sf_encoder* e, const void* pixels, int pixel_dtype, int B, int T, int H, int W,
                                     float* last_hidden, float* pooler, float* hidden_states, float* attentions,
                                     const float* pos_dev, void* workspace, size_t workspace_bytes, sf_stream stream) {
  return forward_common(e, pixels, pixel_dtype, B, T, H, W, last_hidden, pooler, hidden_states, attentions, pos_dev, workspace,
                        workspace_bytes, stream);
}

// ---- sub-module entry points: the reference's model.embeddings / model.encoder.layer[i] / post_layernorm + head
// called one at a time (adapter and classification users, modeling_timesformer_siglip_adapter.py:424-425,
// downstream/AR/models/modeling_timesformer_video_classification.py:121-134).  hidden is the caller's
// residual stream, fp32 frame-major [B,T,N,D], updated in place by sf_layers.
static int stage_common(sf_encoder* e, const void* pixels, int pixel_dtype, int B, int T, int H, int W, float* hidden,
                        float* last_hidden, float* pooler, float* attentions, const float* pos_dev, void* workspace,
                        size_t workspace_bytes, sf_stream stream, int stages, int la, int lb) {
  int N;
  int rc = check_geometry(e, B, T, H, W, pos_dev, &N);
  if (rc) return rc;
  if (!e->finalized) return sf_set_err(SF_ERR_STATE, "sf_finalize_weights has not run");
  if (!hidden || !workspace) return sf_set_err(SF_ERR_INVALID, "null buffer");
  if (T > 256) return sf_set_err(SF_ERR_INVALID, "at most 256 frames per clip");
  if ((stages & 2) && (la < 0 || lb > e->L || la > lb)) return sf_set_err(SF_ERR_INVALID, "layer range [%d, %d) outside [0, %d)", la, lb, e->L);
  Workspace ws = carve(e, workspace, B, T, N, true);
  if (ws.bytes > workspace_bytes) return sf_set_err(SF_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, ws.bytes);
  ws.resid = hidden;                       // the caller's tensor IS the residual stream
  ForwardRequest rq;
  rq.pixels = pixels; rq.pixel_dtype = pixel_dtype; rq.B = B; rq.T = T; rq.H = H; rq.W = W; rq.pos_dev = pos_dev;
  rq.last_hidden = last_hidden; rq.pooler = pooler; rq.attentions = attentions;
  rq.cap = T;
  rq.stages = stages; rq.la = la; rq.lb = lb;
  return run_forward(e, rq, ws, (hipStream_t)stream);
}

extern "C" int sf_embed(sf_encoder* e, const void* pixels, int pixel_dtype, int B, int T, int H, int W, float* hidden_out,
                        const float* pos_dev, void* workspace, size_t workspace_bytes, sf_stream stream) {
  if (!pixels) return sf_set_err(SF_ERR_INVALID, "null pixels");
  if (pixel_dtype != SF_F32 && pixel_dtype != SF_BF16 && pixel_dtype != SF_U8) return sf_set_err(SF_ERR_INVALID, "pixels must be fp32, bf16 or uint8");
  return stage_common(e, pixels, pixel_dtype, B, T, H, W, hidden_out, nullptr, nullptr, nullptr, pos_dev, workspace, workspace_bytes,
                      stream, 1, 0, 0);
}

extern "C" int sf_layers(sf_encoder* e, float* hidden, int B, int T, int H, int W, int layer_begin, int layer_end,
                         float* attentions, void* workspace, size_t workspace_bytes, sf_stream stream) {
  // geometry only sizes the workspace here: a non-null table pointer passes the resolution check
  const float* pos_ok = e ? e->pos : nullptr;
  return stage_common(e, nullptr, SF_F32, B, T, H, W, hidden, nullptr, nullptr, attentions, pos_ok, workspace, workspace_bytes, stream,
                      2, layer_begin, layer_end);
}

extern "C" int sf_post_head(sf_encoder* e, float* hidden, int B, int T, int H, int W, float* last_hidden, float* pooler,
                            void* workspace, size_t workspace_bytes, sf_stream stream) {
  // last_hidden != NULL: post_layernorm(hidden) -> last_hidden, then the head on it -> pooler (may be NULL);
  // last_hidden == NULL: `hidden` is already normalised, the head alone -> pooler
  if (!last_hidden && !pooler) return sf_set_err(SF_ERR_INVALID, "nothing to compute");
  return stage_common(e, nullptr, SF_F32, B, T, H, W, hidden, last_hidden, pooler, nullptr, e ? e->pos : nullptr, workspace,
                      workspace_bytes, stream, last_hidden ? 4 : 8, 0, 0);
}
