// C-ABI implementation: handle, weight packing, and the launch schedule of the encoder forward
// (reference TimesformerMultiTaskingModelSigLIP.forward, modeling:1299-1354; layer body :934-1004;
// streaming copy vqa_enc:1316-1392).  See include/streamformer_hip.h for the contract.
#include "sf_handle.h"
#include "sf_switches.h"
#include "sf_pool_head.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <tuple>
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
#define set_err sf_set_err

// ------------------------------------------------------------------------------------------------
// handle (weight staging, uploads and the common GEMM arguments: sf_weights.h, sf_handle.h)
// ------------------------------------------------------------------------------------------------
struct DevLinear : SfDevLinear {
  const float* ln_s = nullptr;    // LN-folded variants only: s_n = sum_k bf16(W'[n,k])
  const bf16_t* w_frag = nullptr; // t_qkv_f, bf16 mode: w_hi in MFMA-fragment order for sf_stream_fused.hip (SfStreamQkvArgs::w_frag)
};
using DevLN = SfDevLN;
struct DevLayer {
  DevLN ln_t, ln_b, ln_a;
  DevLinear t_qkv, t_out, t_dense, t_fused, s_qkv, s_out, up, down;
  DevLinear t_qkv_f, s_qkv_f, up_f;   // the preceding LayerNorm folded in (W' = W*gamma, b' = b + W beta; hi + lo planes in the accurate mode)
  DevLinear t_qkv_fp;                 // t_qkv_f with its rows permuted for sf_gemm_qkv.hip's fused tile: [q | k | v] of two heads per 384 rows (bf16 mode)
  float gate_tanh = 0.f;
};

struct sf_encoder {
  sf_config cfg;
  int device = 0;
  int N = 0, D = 0, I = 0, L = 0, Kp = 0, hd = 64;      // I, Kp: padded to multiples of 64 (see sf_create)
  SfWeightStore weights;
  bool finalized = false;
  int compute = SF_COMPUTE_BF16;
  bool fused_temporal = false;
  SfDeviceAllocs dev;       // dev.uploaded: the bytes of the packed weights
  // device weights
  DevLinear patch;
  float* pos = nullptr;       // [N,D]
  float* time_tab = nullptr;  // [num_frames,D]
  std::vector<DevLayer> layers;
  DevLN post_ln, head_ln;
  DevLinear head_out, head_fc1, head_fc2;
  // pooling head with the k / v projections of the tokens folded away (sf_pool_head.hip): U_h = Wk_h^T q_h as hi + lo bf16
  // planes [16, D] (q = the projected, scaled probe), the value projection and its bias in fp32
  bf16_t* head_u_hi = nullptr; bf16_t* head_u_lo = nullptr;
  float* head_u = nullptr;    // [16, D] fp32
  float* head_wv = nullptr;   // [D, D]
  float* head_bv = nullptr;   // [D]
  uint64_t generation = 0;    // process-unique id of this handle's current weight packing (bumped by every finalize)
  uint64_t fingerprint = 0;   // content hash of what that packing was made from (weights_fingerprint): travels with a parked stream
  SfPixelNorm pixel_norm = {{1.0f / 127.5f, 1.0f / 127.5f, 1.0f / 127.5f, 1.0f / 127.5f}, {-1.f, -1.f, -1.f, -1.f}};
  // sf_forward_profile: HIP events around the launches of four kernel classes INSIDE a real forward (0: N = 768 residual projection
  // at K = D, 1: the same at K = I, 2: spatial attention, 3: temporal attention)
  struct ProfSpan { int cls; hipEvent_t e0, e1; };
  bool prof_on = false;
  std::vector<ProfSpan> prof;
};
// run `launch` between two events on `s` when the encoder is in profiling mode
template <typename F>
static hipError_t prof_span(const sf_encoder* ce, int cls, hipStream_t s, F&& launch) {
  sf_encoder* e = const_cast<sf_encoder*>(ce);
  if (!e->prof_on) return launch();
  sf_encoder::ProfSpan sp;
  sp.cls = cls;
  hipError_t err = hipEventCreate(&sp.e0);
  if (err != hipSuccess) return err;
  err = hipEventCreate(&sp.e1);
  if (err != hipSuccess) return err;
  (void)hipEventRecord(sp.e0, s);
  err = launch();
  (void)hipEventRecord(sp.e1, s);
  e->prof.push_back(sp);
  return err;
}

struct sf_cache {
  sf_encoder* enc = nullptr;
  uint64_t enc_generation = 0;   // packing of the encoder this cache was sized for (element size, device, weights)
  int B = 0, cap = 0, H = 0, W = 0, N = 0;
  std::vector<int> lens;    // frames seen per stream; the lockstep entry points need them level
  int len() const { int m = 0; for (int v : lens) m = v > m ? v : m; return m; }      // the largest (every stream's, when level)
  bool level() const { for (int v : lens) if (v != lens[0]) return false; return true; }
  void advance(int T) { for (int& v : lens) v += T; }
  std::vector<void*> qkv;   // per layer [B, cap, N, 3D] (bf16 or fp32 by compute mode)
  size_t bytes = 0;
  // hipGraph of the per-call launch sequence: everything between the patch extraction (reads the caller's pixels) and the
  // copy-out (writes the caller's outputs) is replayed as one graph launch.  The key names what is compiled into a capture;
  // the entry holds what else it is valid for (the addresses its nodes carry).
  enum GraphKind { PER_POSITION, POSITION_FREE, RAGGED };      // lockstep, several frames per call / lockstep, one frame / named streams
  struct GraphKey {
    int kind = PER_POSITION;
    int rows = 0, T_new = 0;          // row groups (streams) and frames per stream of the call
    int at = 0;                       // PER_POSITION: frames cached; otherwise the key-pass class (key_pass_class)
    int pooler = 0, pixel_kind = 0;   // pooler_output wanted; 0 fp32, 1 bf16, 2 uint8 frames
    bool operator<(const GraphKey& o) const {
      return std::tie(kind, rows, T_new, at, pooler, pixel_kind) < std::tie(o.kind, o.rows, o.T_new, o.at, o.pooler, o.pixel_kind);
    }
  };
  struct GraphEntry {
    hipGraphExec_t exec = nullptr;
    void* ws = nullptr;
    const float* pos = nullptr;
  };
  std::map<GraphKey, GraphEntry> graphs;
  // Keys that have run eagerly once, so that the lazy per-kernel set-up (sf_launch_big_lds: the dynamic-LDS attribute; device queries) of
  // the instances that pass ran has happened before a capture is opened.  The lockstep entry warms once per cache, under kLockstepWarm;
  // the ragged entry once per key (another row count selects other GEMM kernels).  The set-up is per kernel instance: one the warm pass
  // did not run (a temporal or pooling instance of a longer cache, and the same holds for the GEMM families) gets its attribute at its
  // first launch, which may be inside a hipStreamCaptureModeThreadLocal capture; setting the attribute is not a stream operation.
  std::set<GraphKey> warmed;
  hipStream_t cap_stream = nullptr;   // captures are recorded on a private stream (the caller's may be the null stream, which
                                      // cannot capture) and replayed on the caller's
  int policy = 0;                     // 0 = stop at capacity (the reference raises there), 1 = sliding window over the last `cap` frames
  SfStreamParams* dparams = nullptr;  // device block {pixels, outputs, position} of the single-frame graph (one graph for all positions)
  SfStreamSlot* dtable = nullptr;     // behind it: the stream table of a ragged call, SF_MAX_CALL_STREAMS entries (sf_forward_stream_slots)
};

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
  if (!cfg || !out) return set_err(SF_ERR_INVALID, "sf_create: null argument");
  const sf_config& c = *cfg;
  if (c.hidden_size <= 0 || c.num_attention_heads <= 0 || c.hidden_size % c.num_attention_heads)
    return set_err(SF_ERR_INVALID, "hidden_size %d not divisible by heads %d", c.hidden_size, c.num_attention_heads);
  {   // head_dim 64: the tuned attention kernels; any other multiple of 8 up to 128 (SigLIP-so400m: 72): sf_attention_generic.hip
    const int hd = c.hidden_size / c.num_attention_heads;
    if (hd < 8 || hd > 128 || hd % 8)
      return set_err(SF_ERR_INVALID, "head_dim %d unsupported: multiples of 8 from 8 to 128 (64 runs on the tuned kernels, the others on the generic fp32 attention kernel)", hd);
  }
  if (c.num_attention_heads > 16)
    return set_err(SF_ERR_INVALID, "%d attention heads unsupported: the pooling-head kernels hold at most 16 heads per MFMA tile", c.num_attention_heads);
  // intermediate_size and C*P*P need no alignment: the weights are zero-padded to multiples of 64 at upload (gelu(0) = 0 and zero
  // weight columns make the padding exact): SigLIP-so400m has I = 4304 and 14 x 14 patches (K = 588)
  if (c.hidden_size % 64 || c.intermediate_size <= 0 || c.patch_size <= 0 || c.num_channels <= 0)
    return set_err(SF_ERR_INVALID, "hidden_size must be a multiple of 64; intermediate_size, patch_size, num_channels positive");
  if (c.image_size % c.patch_size) return set_err(SF_ERR_INVALID, "image_size not a multiple of patch_size");
  if (c.hidden_act < 0 || c.hidden_act > 2) return set_err(SF_ERR_INVALID, "unsupported hidden_act code %d", c.hidden_act);
  if (c.num_frames <= 0 || c.num_frames > 256) return set_err(SF_ERR_INVALID, "num_frames must be in 1..256");
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
  if (!e || !key || !host_ptr || ndim < 0 || (ndim && !shape)) return set_err(SF_ERR_INVALID, "sf_load_tensor: null argument");
  std::string err;
  const int rc = e->weights.load(key, host_ptr, dtype, shape, ndim, &err);
  if (rc) return set_err(rc, "%s", err.c_str());
  e->finalized = false;
  return SF_OK;
}

extern "C" int sf_set_pixel_normalization(sf_encoder* e, const float* mean, const float* std, int channels, float rescale) {
  if (!e || !mean || !std || channels < 1 || channels > 4) return set_err(SF_ERR_INVALID, "bad pixel normalisation");
  for (int c = 0; c < 4; ++c) {
    const int k = c < channels ? c : channels - 1;
    if (!(std[k] > 0.f)) return set_err(SF_ERR_INVALID, "image_std must be positive");
    e->pixel_norm.scale[c] = rescale / std[k];       // (x * rescale - mean) / std
    e->pixel_norm.shift[c] = -mean[k] / std[k];
  }
  return SF_OK;
}

extern "C" int sf_missing_weights(sf_encoder* e) {
  if (!e) return set_err(SF_ERR_INVALID, "null handle");
  std::string err;
  const int missing = e->weights.missing(&err);
  if (missing) set_err(SF_ERR_STATE, "%s", err.c_str());
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
  if (!e) return set_err(SF_ERR_INVALID, "null handle");
  SF_TRY(sf_check_compute_mode(compute));
  if (sf_missing_weights(e)) return SF_ERR_STATE;
  if (e->cfg.add_lora_spatial && !merge_lora)
    return set_err(SF_ERR_INVALID, "un-merged LoRA execution is a training-time path; the inference forward needs merge_lora=1");
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
// workspace carving
// ------------------------------------------------------------------------------------------------
struct Workspace {
  float* resid; float* te_rows; float* ln_stats;
  float* embed_tab; bf16_t* patch_buf;  // pos + time table [T*N, D]; patch matrix [M, Kp] when the embedding GEMM runs on the
                                        // panel kernel (its bf16 output goes to xn_hi, so the A operand needs its own buffer)
  bf16_t *xn_hi, *xn_lo, *ctx_hi, *ctx_lo, *tmp_hi, *tmp_lo, *mid_hi, *mid_lo;
  void* qkv;          // spatial qkv; fast: bf16 [M,3D], accurate: fp32 [M,3D]
  void* tqkv;         // temporal qkv of the current layer when no cache is used
  float* attn_out;    // head: [F, D]
  float *head_ctx, *head_mid;      // head tail on one to four rows (streamed frames): fp32 context [F, D] and MLP activation [F, I]
  float *pool_z, *pool_ml;         // head: weighted token sums [F, S, heads, D] and {max, sum} [F, S, heads, 2] per token split
  bf16_t *pc_hi, *pc_lo, *hn_hi, *hn_lo, *hm_hi, *hm_lo;
  float *lhs_stage, *pool_stage;   // streaming only: graph-owned outputs, copied to the caller's tensors after the replay
  bf16_t* res_bf;                  // small-M LayerNorm fold: bf16 copy of the residual stream (A operand of the folded Linears)
  bf16_t* res_lo;                  // BASELINE-sized M, bf16 mode: lo plane of the residual stream (hi plane = xn_hi), see SfGemmArgs::resid_hi
  bf16_t* res_lo2;                 // accurate mode: third plane of the residual stream (hi = xn_hi, lo = xn_lo), see SfGemmArgs::resid_lo2
  size_t bytes;
};

static Workspace carve(const sf_encoder* e, void* base, int B, int T, int N, bool need_tqkv) {
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
static SfGemmArgs linear_args(const sf_encoder* e, const DevLinear& lin, const bf16_t* a_hi, const bf16_t* a_lo, int M, int epi, bool split) {
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
      return set_err(SF_ERR_CAPACITY, "streaming needs time-embedding row %d but config.num_frames is %d", t_past + T - 1, nf);
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

// Where a streamed frame goes: its time-embedding row, its slot in the KV-cache, and the keys its query sees (cached + itself).
struct StreamPos { int t_row, slot, tk; };

// What one call of the encoder over T new frames is asked to do (filled by name at the entry points).
struct ForwardRequest {
  const void* pixels = nullptr; int pixel_dtype = SF_F32;
  int B = 0, T = 0, H = 0, W = 0;
  float* last_hidden = nullptr; float* pooler = nullptr; float* hidden_states = nullptr; float* attentions = nullptr;
  const float* pos_dev = nullptr;        // resized position table, or null for the encoder's own
  void* const* layer_tqkv = nullptr;     // streaming: per-layer temporal qkv caches [B, cap, N, 3D]; null: ws.tqkv, rewritten by every layer
  int cap = 0, t_past = 0;               // frames a cache row holds (T without a cache), frames already in it
  bool streaming = false;
  // stages: 1 = embeddings -> ws.resid, 2 = layers [la, lb) on ws.resid, 4 = post-LayerNorm + pooling head,
  // 8 = pooling head alone on already-normalised tokens in ws.resid
  // (the sub-module entry points run them one at a time on a caller-owned residual stream)
  int stages = 7, la = 0, lb = -1;       // lb < 0: to the last layer
  // ready: 1 = the patch matrix is already in the workspace (the streaming entry extracts it outside its graph),
  //        2 = ws.res_bf already holds bf16(residual) (a later layer range of the same call)
  int ready = 0;
  // sp (streaming, T == 1, graph capture): the cache position is read on the DEVICE from sp->t_past by the kernels that need
  // it (time-embedding row, KV-cache append row, single-query attention); t_past here only selects kernel variants
  const SfStreamParams* sp = nullptr;
  // pos (streaming): the position of the first new frame, from stream_position(); null: (t_past, t_past, t_past + T)
  const StreamPos* pos = nullptr;
  // tab (streaming, T == 1, with sp): the call is ragged — row group g is one frame of cache slab tab[g].stream at that entry's own
  // position (device table); B counts the groups of the call, pos carries the largest tk (kernel variants only)
  const SfStreamSlot* tab = nullptr;
};

enum EmbedRoute { EMBED_NONE, EMBED_TILE, EMBED_PANEL, EMBED_GEMM };

// Every schedule decision of one forward, made by plan_forward() before the first launch and only read afterwards.
//
// The residual stream x and the LayerNorms in front of the three folded Linears of a layer (temporal qkv, spatial qkv, MLP-up: weights
// W' = W gamma, ln_s = row sums of W') take one of these forms; `M` = B T N token rows:
//
//   schedule   taken when                                                      residual stream             LayerNorm of the consumers
//   ---------  --------------------------------------------------------------  --------------------------  ------------------------------------
//   fold       bf16, whole clips (not streaming), ln_fold_panel_ok (BASELINE-   fp32 ws.resid + bf16 copy   statistics rows ws.ln_stats written by
//              sized M, D = 768) and not sfold-sized                            in ws.xn_hi                 the panel producers, applied by the
//                                                                                                           256^2 consumers
//   fold + pm  fold, and: complete forward (stages 1|2|4) without               hi = ws.xn_hi, lo =         as fold (every producer moves 154 MB
//              hidden_states, panel embedding route with plane outputs,         ws.res_lo (no fp32)         instead of 192)
//              no SF_DISABLE_RESID_PLANES
//   tile-fold  bf16, whole clips, ln_fold_tile_ok (two clips per call)          as fold                     as fold, narrow tile kernel as producer
//   sfold      not fold; M <= sf_infold_max_rows() (streamed frames, a few      fp32 ws.resid + bf16 copy   inside the skinny / tile consumers
//              frames per call), ln_fold_small_ok, ws.res_bf carved             ws.res_bf (accurate: + lo   (ln_inkernel), no statistics buffer
//                                                                               plane ws.res_lo)
//   xm         accurate, complete forward of whole clips without hidden_states  hi = ws.xn_hi, lo =         ws.ln_stats: one pair per 256-column
//              or cache, temporal + spatial attention on planes, ln_fold_acc_ok ws.xn_lo, lo2 = ws.res_lo2  tile of the bf16x3 256^2 producer
//              (M > 6272, or D = 1024 from 2048 rows)                           (SF_ACC_TWO_PLANES: no lo2)
//   gm         bf16, neither fold nor sfold, complete forward of whole clips    hi = ws.xn_hi, lo =         as xm, bf16 256^2 kernel
//              without hidden_states, ln_fold_g256_ok (D = 1024)                ws.res_lo
//   plain      everything else                                                  fp32 ws.resid               three sf_launch_layernorm per layer
//                                                                                                           into ws.xn_hi (/ xn_lo)
//
// In the plane forms (pm, xm, gm) ws.resid is written by the embeddings only; the post-LayerNorm reads the planes.
struct ForwardPlan {
  ForwardRequest rq;                     // lb resolved
  int N, M, F;                           // patches per frame, token rows, frames
  bool acc;                              // fp32-accurate mode: every GEMM operand as hi + lo planes
  int qkv_epi; size_t esz;               // qkv tensors: bf16, or fp32 in the accurate mode
  float scale;
  int t_row, slot, tk;                   // time-embedding row, cache slot of the first new frame, keys the new frames see
  // embeddings
  bool zero_stats;                       // statistics rows of the bf16 fold are four pairs; the 384-column panel kernel fills pairs 0 and 2 only
  bool time_folded;                      // the embedding GEMM reads its time row from the table (row index in the device block): no gather
  EmbedRoute embed_route;                // EMBED_TILE / EMBED_PANEL also emit bf16(x) + row statistics; EMBED_GEMM: sf_launch_gemm's choice
  bf16_t* patches;                       // the patch matrix: ws.patch_buf in front of the tile / panel routes (their bf16 output goes to xn_hi)
  SfGemmArgs embed;
  // the schedule (table above)
  bool fold, sfold, xm, gm, pm;
  bool anyfold;                          // fold || sfold || xm || gm: folded weights, no LayerNorm launch
  bool rplanes;                          // pm || xm || gm
  bool seed_stats;                       // fold, embeddings without statistics (generic route, or sf_layers on the caller's tensor)
  bool seed_split;                       // sfold entered through sf_layers: ws.res_bf (+ lo) from the caller's tensor
  float* resid;                          // fp32 residual stream, null in the plane forms
  bf16_t* fold_hi;                       // what a producer writes next to (or instead of) it: the consumers' A operand
  bf16_t* plo; bf16_t* plo2;             // lo / third plane
  float* fold_st;                        // statistics rows, null when no buffer carries them
  const bf16_t* ln_in; const bf16_t* ln_in_lo;      // A operand of the three LayerNorm'd Linears
  // attention inputs of the accurate mode as hi + lo bf16 planes in the bytes of the fp32 tensor (DMA kernels) instead of fp32
  bool tplanes, planes;                  // temporal: whole short clip without a cache; spatial: <= 224 tokens, no probabilities wanted
  size_t tsz, sesz;                      // element size of the temporal / spatial qkv tensor
  // head
  bool head_generic;                     // widths the MFMA probe kernels do not cover
  bool head_rows;                        // one to four frames: row-vector tail, pooler_output written by its last launch
};

static ForwardPlan plan_forward(const sf_encoder* e, const ForwardRequest& rq, const Workspace& ws) {
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

  const bool tile_fold = ln_fold_tile_ok(e, M), small_fold = ln_fold_small_ok(e, M);
  const bool stats_fold = tile_fold || (!small_fold && ln_fold_panel_ok(e, M));      // bf16 mode: a fold with a statistics buffer
  const bool small_bufs = ws.res_bf && (!acc || ws.res_lo) && small_fold;
  p.zero_stats = stats_fold && !streaming && (stages & 3);

  // ---- embeddings.  Panel route: out = table[m % (T N)] + patches W^T + b with table = pos + time rows; pm asks it for plane outputs
  const bool panel_embed = stats_fold && !streaming && (stages & 2) && ws.embed_tab && ws.patch_buf && e->Kp % 32 == 0 && e->Kp >= 128 && D == 768 &&
                           !sf_sw(SW_EMBED_VIA_GEMM128);
  const bool pm_wanted = panel_embed && !tile_fold && !acc && complete && ws.res_lo && !sf_sw(SW_DISABLE_RESID_PLANES);
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
static int run_plan(sf_encoder* e, const ForwardPlan& p, const Workspace& ws, hipStream_t s) {
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
static int run_forward(sf_encoder* e, const ForwardRequest& rq, const Workspace& ws, hipStream_t s) {
  return run_plan(e, plan_forward(e, rq, ws), ws, s);
}

static int check_geometry(const sf_encoder* e, int B, int T, int H, int W, const float* pos_dev, int* N_out) {
  if (!e) return set_err(SF_ERR_INVALID, "null handle");
  const int P = e->cfg.patch_size;
  if (B <= 0 || T <= 0 || H < P || W < P) return set_err(SF_ERR_INVALID, "bad geometry B=%d T=%d H=%d W=%d", B, T, H, W);
  const int N = (H / P) * (W / P);
  if (N > 2048) return set_err(SF_ERR_INVALID, "%d patches per frame; the attention kernels handle <= 2048", N);
  if (!pos_dev && !(N == e->N && H == W))
    return set_err(SF_ERR_INVALID, "input %dx%d differs from image_size %d: pass a resized position table (pos_dev)", H, W, e->cfg.image_size);
  if ((size_t)B * T * N > (size_t)1 << 30) return set_err(SF_ERR_INVALID, "too many token rows");
  *N_out = N;
  return SF_OK;
}

extern "C" int sf_workspace_bytes(sf_encoder* e, int B, int T, int H, int W, size_t* out) {
  int N;
  const float* dummy = (const float*)1;
  int rc = check_geometry(e, B, T, H, W, dummy, &N);
  if (rc) return rc;
  if (!out) return set_err(SF_ERR_INVALID, "null out");
  if (!e->finalized) return set_err(SF_ERR_STATE, "sf_finalize_weights has not run");
  *out = carve(e, nullptr, B, T, N, true).bytes;
  return SF_OK;
}

static int forward_common(sf_encoder* e, const void* pixels, int pixel_dtype, int B, int T, int H, int W, float* last_hidden,
                          float* pooler, float* hidden_states, float* attentions, const float* pos_dev, void* workspace,
                          size_t workspace_bytes, sf_stream stream) {
  int N;
  int rc = check_geometry(e, B, T, H, W, pos_dev, &N);
  if (rc) return rc;
  if (!e->finalized) return set_err(SF_ERR_STATE, "sf_finalize_weights has not run");
  if (!pixels || !last_hidden || !workspace) return set_err(SF_ERR_INVALID, "null buffer");
  if (pixel_dtype != SF_F32 && pixel_dtype != SF_BF16 && pixel_dtype != SF_U8) return set_err(SF_ERR_INVALID, "pixels must be fp32, bf16 or uint8");
  if (T > 256) return set_err(SF_ERR_INVALID, "at most 256 frames per clip");
  Workspace ws = carve(e, workspace, B, T, N, true);
  if (ws.bytes > workspace_bytes) return set_err(SF_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, ws.bytes);
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
  if (!e || !out_ms) return set_err(SF_ERR_INVALID, "null argument");
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
  if (se != hipSuccess) return set_err(SF_ERR_HIP, "sf_forward_profile: %s", hipGetErrorString(se));
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
  if (!e->finalized) return set_err(SF_ERR_STATE, "sf_finalize_weights has not run");
  if (!hidden || !workspace) return set_err(SF_ERR_INVALID, "null buffer");
  if (T > 256) return set_err(SF_ERR_INVALID, "at most 256 frames per clip");
  if ((stages & 2) && (la < 0 || lb > e->L || la > lb)) return set_err(SF_ERR_INVALID, "layer range [%d, %d) outside [0, %d)", la, lb, e->L);
  Workspace ws = carve(e, workspace, B, T, N, true);
  if (ws.bytes > workspace_bytes) return set_err(SF_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, ws.bytes);
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
  if (!pixels) return set_err(SF_ERR_INVALID, "null pixels");
  if (pixel_dtype != SF_F32 && pixel_dtype != SF_BF16 && pixel_dtype != SF_U8) return set_err(SF_ERR_INVALID, "pixels must be fp32, bf16 or uint8");
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
  if (!last_hidden && !pooler) return set_err(SF_ERR_INVALID, "nothing to compute");
  return stage_common(e, nullptr, SF_F32, B, T, H, W, hidden, last_hidden, pooler, nullptr, e ? e->pos : nullptr, workspace,
                      workspace_bytes, stream, last_hidden ? 4 : 8, 0, 0);
}

// ------------------------------------------------------------------------------------------------
// streaming
// ------------------------------------------------------------------------------------------------
extern "C" int sf_cache_create(sf_encoder* e, int B, int max_frames, int H, int W, sf_cache** out) {
  int N;
  const float* dummy = (const float*)1;
  int rc = check_geometry(e, B, 1, H, W, dummy, &N);
  if (rc) return rc;
  if (!out || max_frames <= 0 || max_frames > 256) return set_err(SF_ERR_INVALID, "max_frames must be in 1..256");
  if (!e->finalized) return set_err(SF_ERR_STATE, "sf_finalize_weights has not run");
  HIP_TRY(hipSetDevice(e->device));
  sf_cache* c = new sf_cache();
  c->enc = e; c->enc_generation = e->generation; c->B = B; c->cap = max_frames; c->H = H; c->W = W; c->N = N;
  c->lens.assign(B, 0);
  const size_t per = (size_t)B * max_frames * N * 3 * e->D * (e->compute == SF_COMPUTE_BF16X3 ? 4 : 2);
  for (int i = 0; i < e->L; ++i) {
    void* p = nullptr;
    hipError_t err = hipMalloc(&p, per);
    if (err != hipSuccess) {
      for (void* q : c->qkv) (void)hipFree(q);
      delete c;
      return set_err(SF_ERR_HIP, "hipMalloc(%zu) for the KV-cache: %s", per, hipGetErrorString(err));
    }
    c->qkv.push_back(p);
  }
  c->bytes = per * e->L;
  // the parameter block, and behind it (256-byte aligned) the stream table of a ragged call
  if (hipMalloc((void**)&c->dparams, 256 + sizeof(SfStreamSlot) * SF_MAX_CALL_STREAMS) != hipSuccess) {
    for (void* q : c->qkv) (void)hipFree(q);
    delete c;
    return set_err(SF_ERR_HIP, "hipMalloc for the stream parameter block failed");
  }
  static_assert(sizeof(SfStreamParams) <= 256, "the stream table sits 256 bytes behind the parameter block");
  c->dtable = reinterpret_cast<SfStreamSlot*>(reinterpret_cast<char*>(c->dparams) + 256);
  *out = c;
  return SF_OK;
}
extern "C" int sf_cache_reset(sf_cache* c) {
  if (!c) return set_err(SF_ERR_INVALID, "null cache");
  c->lens.assign(c->B, 0);
  return SF_OK;
}
extern "C" int sf_cache_reset_stream(sf_cache* c, int stream) {
  if (!c) return set_err(SF_ERR_INVALID, "null cache");
  if (stream < 0 || stream >= c->B) return set_err(SF_ERR_INVALID, "stream %d outside this cache's %d streams", stream, c->B);
  c->lens[stream] = 0;
  return SF_OK;
}
extern "C" int sf_cache_length(const sf_cache* c) { return c ? c->len() : 0; }
extern "C" int sf_cache_stream_length(const sf_cache* c, int stream) { return (c && stream >= 0 && stream < c->B) ? c->lens[stream] : 0; }
extern "C" int sf_cache_set_policy(sf_cache* c, int policy) {
  if (!c || (policy != 0 && policy != 1)) return set_err(SF_ERR_INVALID, "policy must be 0 (stop at capacity) or 1 (sliding window)");
  if (c->len() != 0) return set_err(SF_ERR_STATE, "the policy of a cache is chosen while it is empty");
  c->policy = policy;
  return SF_OK;
}
extern "C" size_t sf_cache_bytes(const sf_cache* c) { return c ? c->bytes : 0; }
static void drop_graphs(sf_cache* c) {
  for (auto& kv : c->graphs)
    if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  c->graphs.clear();
}
extern "C" void sf_cache_destroy(sf_cache* c) {
  if (!c) return;
  drop_graphs(c);
  if (c->cap_stream) (void)hipStreamDestroy(c->cap_stream);
  for (void* q : c->qkv) (void)hipFree(q);
  if (c->dparams) (void)hipFree(c->dparams);
  delete c;
}
extern "C" int sf_stream_workspace_bytes(sf_encoder* e, const sf_cache* c, int T_new, size_t* out) {
  if (!e || !c || !out || T_new <= 0) return set_err(SF_ERR_INVALID, "bad argument");
  if (c->enc != e || c->enc_generation != e->generation) return set_err(SF_ERR_STATE, "cache does not belong to this encoder's current weight packing");
  *out = carve(e, nullptr, c->B, T_new, c->N, false).bytes;
  return SF_OK;
}
// What the lockstep entry records in sf_cache::warmed: no key of a call equals it, a call has rows >= 1.
static const sf_cache::GraphKey kLockstepWarm = {};

// The cache was created by this encoder, as it is packed now.
static int check_cache_owner(const sf_encoder* e, const sf_cache* c) {
  if (!e || !c || c->enc != e) return set_err(SF_ERR_INVALID, "cache does not belong to this encoder");
  // a handle address can be reused after sf_destroy, and sf_finalize_weights may have changed the compute mode (cache element
  // size) or the device: the generation stamp tells a cache of an earlier packing from a current one
  if (c->enc_generation != e->generation)
    return set_err(SF_ERR_STATE, "cache was created for an earlier weight packing of this encoder (sf_finalize_weights ran since): create a new cache");
  return SF_OK;
}

// ---- parking a stream (kernels: sf_cache_park.hip) -------------------------------------------------------------------------------
static size_t cache_elem_bytes(const sf_encoder* e) { return e->compute == SF_COMPUTE_BF16X3 ? 4 : 2; }
// bytes of the k | v columns of `held` frames over all layers
static size_t stream_blob_bytes(const sf_cache* c, int held) {
  return (size_t)c->enc->L * held * c->N * 2 * c->enc->D * cache_elem_bytes(c->enc);
}
static int check_stream_id(const sf_cache* c, int stream) {
  if (stream < 0 || stream >= c->B) return set_err(SF_ERR_INVALID, "stream %d outside this cache's %d streams (ids are 0 .. %d)", stream, c->B, c->B - 1);
  return SF_OK;
}
extern "C" int sf_cache_stream_blob_bytes(const sf_cache* c, int stream, size_t* out) {
  if (!c || !out) return set_err(SF_ERR_INVALID, "null argument");
  if (int rc = check_stream_id(c, stream)) return rc;
  const int seen = c->lens[stream];
  *out = stream_blob_bytes(c, seen < c->cap ? seen : c->cap);
  return SF_OK;
}
// one launch for up to SF_PARK_MAX_LAYERS layers (every model the library accepts today), further launches beyond
static int park_stream(const sf_encoder* e, const sf_cache* c, int stream, int held, void* blob, bool do_export, hipStream_t s) {
  const size_t esz = cache_elem_bytes(e), row = (size_t)3 * e->D * esz;
  SfParkArgs a;
  memset(&a, 0, sizeof(a));
  a.blob = (char*)blob; a.row_bytes = row; a.kv_off = (size_t)e->D * esz; a.slab_off = (size_t)stream * c->cap * c->N * row;
  a.vpr = (uint32_t)(2 * e->D * esz / 16);
  const size_t nvec = (size_t)held * c->N * a.vpr;
  if (nvec > 0x7fffffffu) return set_err(SF_ERR_CAPACITY, "a stream of %zu bytes per layer is beyond one export launch", nvec * 16);
  a.nvec = (uint32_t)nvec; a.layer_blob_bytes = nvec * 16;
  for (int l0 = 0; l0 < e->L; l0 += SF_PARK_MAX_LAYERS) {
    const int n = e->L - l0 < SF_PARK_MAX_LAYERS ? e->L - l0 : SF_PARK_MAX_LAYERS;
    for (int l = 0; l < n; ++l) a.layer[l] = (char*)c->qkv[l0 + l];
    a.layer0 = l0;
    HIP_TRY(sf_launch_cache_park(a, n, do_export, s));
  }
  return SF_OK;
}
extern "C" int sf_cache_export_stream(sf_encoder* e, sf_cache* c, int stream, void* blob, size_t bytes, sf_cache_stream_meta* meta,
                                      sf_stream s) {
  int rc = check_cache_owner(e, c);
  if (rc) return rc;
  if (!meta) return set_err(SF_ERR_INVALID, "null meta_out");
  if ((rc = check_stream_id(c, stream))) return rc;
  const int seen = c->lens[stream], held = seen < c->cap ? seen : c->cap;
  const size_t need = stream_blob_bytes(c, held);
  if (bytes != need) return set_err(SF_ERR_INVALID, "blob of %zu bytes; stream %d holds %d frames = %zu bytes (sf_cache_stream_blob_bytes)", bytes, stream, held, need);
  if (need && (!blob || ((size_t)blob & 15))) return set_err(SF_ERR_INVALID, "the blob must be a 16-byte aligned device buffer");
  if (need && (rc = park_stream(e, c, stream, held, blob, true, (hipStream_t)s))) return rc;
  memset(meta, 0, sizeof(*meta));
  meta->format = SF_STREAM_BLOB_KV1; meta->compute = e->compute; meta->frames_seen = seen; meta->frames_held = held;
  meta->max_frames = c->cap; meta->policy = c->policy; meta->H = c->H; meta->W = c->W;
  meta->layers = e->L; meta->hidden_size = e->D; meta->patches = c->N; meta->elem_bytes = (int32_t)cache_elem_bytes(e);
  meta->packing = e->fingerprint; meta->blob_bytes = need;
  return SF_OK;
}
extern "C" int sf_cache_import_stream(sf_encoder* e, sf_cache* c, int stream, const void* blob, size_t bytes,
                                      const sf_cache_stream_meta* m, sf_stream s) {
  int rc = check_cache_owner(e, c);
  if (rc) return rc;
  if (!m) return set_err(SF_ERR_INVALID, "null meta");
  if ((rc = check_stream_id(c, stream))) return rc;
  if (m->format != SF_STREAM_BLOB_KV1) return set_err(SF_ERR_INVALID, "format: blob tag 0x%08x is not SF_STREAM_BLOB_KV1", m->format);
  if (m->compute != e->compute)
    return set_err(SF_ERR_INVALID, "compute mode: the stream was parked in mode %d, this encoder is packed for mode %d", m->compute, e->compute);
  if (m->H != c->H || m->W != c->W) return set_err(SF_ERR_INVALID, "resolution: the stream was parked at %dx%d, this cache is %dx%d", m->H, m->W, c->H, c->W);
  if (m->max_frames != c->cap)
    return set_err(SF_ERR_INVALID, "max_frames: the stream was parked from a cache of %d frames, this one holds %d (restoring into another "
                   "capacity is not supported)", m->max_frames, c->cap);
  if (m->policy != c->policy) return set_err(SF_ERR_INVALID, "policy: the stream was parked under policy %d, this cache has policy %d", m->policy, c->policy);
  if (m->layers != e->L || m->hidden_size != e->D || m->patches != c->N || m->elem_bytes != (int32_t)cache_elem_bytes(e))
    return set_err(SF_ERR_INVALID, "geometry: blob of %d layers x %d patches x width %d x %d bytes, cache of %d x %d x %d x %zu", m->layers, m->patches,
                   m->hidden_size, m->elem_bytes, e->L, c->N, e->D, cache_elem_bytes(e));
  if (m->frames_seen < 0 || m->frames_held != (m->frames_seen < c->cap ? m->frames_seen : c->cap) || (c->policy != 1 && m->frames_seen > c->cap))
    return set_err(SF_ERR_INVALID, "frames: %d seen / %d held do not describe a stream of a %d-frame cache", m->frames_seen, m->frames_held, c->cap);
  if (m->packing != e->fingerprint)
    return set_err(SF_ERR_STATE, "packing: the stream was parked by other weights (fingerprint %016llx, this encoder %016llx): its keys and values "
                   "mean nothing here", (unsigned long long)m->packing, (unsigned long long)e->fingerprint);
  const size_t need = stream_blob_bytes(c, m->frames_held);
  if (bytes != need || m->blob_bytes != need)
    return set_err(SF_ERR_INVALID, "byte count: blob of %zu bytes (meta says %llu), %d frames are %zu", bytes, (unsigned long long)m->blob_bytes,
                   m->frames_held, need);
  if (need && (!blob || ((size_t)blob & 15))) return set_err(SF_ERR_INVALID, "the blob must be a 16-byte aligned device buffer");
  if (need && (rc = park_stream(e, c, stream, m->frames_held, const_cast<void*>(blob), false, (hipStream_t)s))) return rc;
  c->lens[stream] = m->frames_seen;      // the next frame's time row, slot and key count follow from it (stream_position)
  return SF_OK;
}

// What the streaming entries share once the cache is known to be the encoder's: the checked arguments of a call of `rows` streams.
struct StreamCall {
  Workspace ws;
  ForwardRequest rq;      // input, geometry and cache filled in; the entry sets the outputs and the position
  hipStream_t s = nullptr;
  int pk = 0;             // pixel kind of sf_launch_patchify
  bool graph_ok = false;  // graphs are not switched off and the caller is not capturing the stream itself
};
// lockstep: the call advances every stream of the cache, which must be level.  positions(): the entry's position refusals; they come
// before the workspace refusal.
template <typename Positions>
static int open_stream_call(sf_encoder* e, sf_cache* c, int rows, int T_new, bool lockstep, const void* pixels, int pixel_dtype,
                            const float* last_hidden, const float* pos_dev, void* workspace, size_t workspace_bytes, sf_stream stream,
                            Positions&& positions, StreamCall* call) {
  int N;
  int rc = check_geometry(e, rows, T_new, c->H, c->W, pos_dev, &N);
  if (rc) return rc;
  if (lockstep && !c->level())
    return set_err(SF_ERR_STATE, "the streams of this cache are at different positions (longest %d frames): advance them with sf_forward_stream_slots "
                   "(stream_ids= in Python), or level them with sf_cache_reset", c->len());
  if (!pixels || !last_hidden || !workspace) return set_err(SF_ERR_INVALID, "null buffer");
  if (pixel_dtype != SF_F32 && pixel_dtype != SF_BF16 && pixel_dtype != SF_U8) return set_err(SF_ERR_INVALID, "pixels must be fp32, bf16 or uint8");
  if ((rc = positions())) return rc;
  call->ws = carve(e, workspace, rows, T_new, N, false);
  if (call->ws.bytes > workspace_bytes) return set_err(SF_ERR_WORKSPACE, "workspace %zu < required %zu bytes", workspace_bytes, call->ws.bytes);
  call->pk = pixel_dtype == SF_U8 ? 2 : (pixel_dtype == SF_BF16 ? 1 : 0);
  call->s = (hipStream_t)stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(call->s, &cap);
  call->graph_ok = !sf_sw(SW_DISABLE_STREAM_GRAPH) && cap == hipStreamCaptureStatusNone;
  ForwardRequest& rq = call->rq;
  rq.pixels = pixels; rq.pixel_dtype = pixel_dtype; rq.B = rows; rq.T = T_new; rq.H = c->H; rq.W = c->W; rq.pos_dev = pos_dev;
  rq.layer_tqkv = c->qkv.data(); rq.cap = c->cap; rq.streaming = true;
  return SF_OK;
}

// Position of the first of T_new frames that follow `len` cached ones, or the refusal (stream: the id a ragged call names, -1 for a
// lockstep call).  Sliding window (policy 1, beyond the reference, which raises at num_frames): once the cache is full the new
// frame overwrites the oldest slot, its query sees the last `cap` frames, and frames past the time-embedding table reuse its
// last row (the nearest-neighbour extension modeling:441-447 applies to long clips).
static int stream_position(const sf_cache* c, int len, int T_new, int stream, StreamPos* out) {
  const int nf = c->enc->cfg.num_frames, cap = c->cap;
  if (c->policy == 1 && T_new == 1) {
    *out = {len < nf ? len : nf - 1, len % cap, len + 1 < cap ? len + 1 : cap};
    return SF_OK;
  }
  if (c->policy == 1 && len + T_new > (cap < nf ? cap : nf))
    return set_err(SF_ERR_CAPACITY, "a sliding-window cache that is full (%d of %d frames) advances one frame per call, got %d", len, cap, T_new);
  if (len + T_new > cap)
    return stream < 0 ? set_err(SF_ERR_CAPACITY, "cache holds %d of %d frames; %d more do not fit", len, cap, T_new)
                      : set_err(SF_ERR_CAPACITY, "stream %d holds %d of %d frames; one more does not fit: leave it out of the call, or restart it with "
                                "sf_cache_reset_stream", stream, len, cap);
  if (len + T_new > nf)
    return stream < 0 ? set_err(SF_ERR_CAPACITY, "streaming needs time-embedding row %d but config.num_frames is %d", len + T_new - 1, nf)
                      : set_err(SF_ERR_CAPACITY, "stream %d needs time-embedding row %d but config.num_frames is %d: leave it out of the call, or restart it "
                                "with sf_cache_reset_stream", stream, len + T_new - 1, nf);
  *out = {len, len, len + T_new};
  return SF_OK;
}

// The single-query attention compiles in its number of 64-key passes, 1 / 2 / 4: the only thing about a position that a
// position-free capture fixes (at most three graphs per call shape).
static int key_pass_class(int tk) {
  const int kp = (tk + 63) >> 6;
  return kp <= 1 ? 1 : (kp <= 2 ? 2 : 4);
}
// A key count of the class that this cache can reach: it selects the kernels, which read the live position from the device.
static StreamPos class_position(const sf_cache* c, int kcls) {
  const int nf = c->enc->cfg.num_frames;
  int tk = kcls * 64;
  if (tk > c->cap) tk = c->cap;
  if (c->policy != 1 && tk > nf) tk = nf;
  return {0, 0, tk};
}

// The forward of a position-free call (one frame per stream; ragged: the named streams through the device table): patch matrix
// already extracted by the launch that delivered the parameter block, last_hidden_state written straight into the caller's tensor
// through the block, pooler_output too when the head's row-vector tail runs (<= 4 rows): no staging copy at the end.
static int run_position_free(sf_encoder* e, sf_cache* c, const StreamCall& call, int kcls, bool ragged, bool pooler, hipStream_t on) {
  const StreamPos rep = class_position(c, kcls);
  ForwardRequest rq = call.rq;
  rq.last_hidden = call.ws.lhs_stage; rq.pooler = pooler ? call.ws.pool_stage : nullptr;
  rq.ready = 1; rq.sp = c->dparams; rq.tab = ragged ? c->dtable : nullptr; rq.pos = &rep;
  const ForwardPlan plan = plan_forward(e, rq, call.ws);
  int rc = run_plan(e, plan, call.ws, on);
  if (rc == SF_OK && pooler && !plan.head_rows)      // the F-row tail left pooler_output in the workspace
    HIP_TRY(sf_launch_copy2(nullptr, nullptr, 0, call.ws.pool_stage, nullptr, (size_t)plan.F * e->D, on, c->dparams));
  return rc;
}

// The graph of `key`, valid for this workspace and position table: the cached one, or a capture of run(cap_stream).
template <typename Run>
static int stream_graph(sf_cache* c, const sf_cache::GraphKey& key, void* workspace, const float* pos_dev, Run&& run, hipGraphExec_t* exec) {
  sf_cache::GraphEntry& g = c->graphs[key];
  if (g.exec && (g.ws != workspace || g.pos != pos_dev)) {      // its nodes carry addresses of another workspace
    (void)hipGraphExecDestroy(g.exec);
    g.exec = nullptr;
  }
  if (!g.exec) {
    hipGraph_t graph = nullptr;
    if (!c->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = run(c->cap_stream);
    const hipError_t ce = hipStreamEndCapture(c->cap_stream, &graph);
    hipError_t ie = hipSuccess;
    if (rc == SF_OK && ce == hipSuccess && graph) ie = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (!g.exec) {
      c->graphs.erase(key);
      if (rc != SF_OK) return rc;
      if (ie != hipSuccess) return set_err(SF_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ie));
      return set_err(SF_ERR_HIP, "stream capture failed: %s", hipGetErrorString(ce));
    }
    g.ws = workspace; g.pos = pos_dev;
  }
  *exec = g.exec;
  return SF_OK;
}

// slab < 0: every stream of the cache advances T_new frames from the one position they share (the lockstep call).
// slab >= 0: that stream alone, as a B = 1 call on its slab of every layer's cache (the prefill of a stream that joins a ragged cache);
// always eager — a prefill happens once per stream, and its position-keyed graph would be captured for a single replay.
static int forward_stream_impl(sf_encoder* e, sf_cache* c, const void* pixels, int pixel_dtype, int T_new,
                               float* last_hidden, float* pooler, float* hidden_states, float* attentions, const float* pos_dev,
                               void* workspace, size_t workspace_bytes, sf_stream stream, int slab = -1) {
  int rc = check_cache_owner(e, c);
  if (rc) return rc;
  const int len = slab < 0 ? c->len() : c->lens[slab];
  StreamCall call;
  StreamPos pos;
  if ((rc = open_stream_call(e, c, slab < 0 ? c->B : 1, T_new, slab < 0, pixels, pixel_dtype, last_hidden, pos_dev, workspace, workspace_bytes, stream,
                             [&]() { return stream_position(c, len, T_new, -1, &pos); }, &call))) return rc;
  const Workspace& ws = call.ws;
  ForwardRequest& rq = call.rq;
  hipStream_t s = call.s;
  rq.pos = &pos;
  std::vector<void*> slab_qkv;
  if (slab >= 0) {
    const size_t per = (size_t)c->cap * c->N * 3 * e->D * (e->compute == SF_COMPUTE_BF16X3 ? 4 : 2);
    for (void* q : c->qkv) slab_qkv.push_back((char*)q + (size_t)slab * per);
    rq.layer_tqkv = slab_qkv.data();
  }
  auto eager = [&]() -> int {
    ForwardRequest q = rq;
    q.last_hidden = last_hidden; q.pooler = pooler; q.hidden_states = hidden_states; q.attentions = attentions;
    const int r = run_forward(e, q, ws, s);
    if (r == SF_OK) { if (slab < 0) c->advance(T_new); else c->lens[slab] += T_new; }
    return r;
  };
  // ---- graph replay (the per-frame sequence is ~100 dependent launches of a few microseconds) -----------------
  // Not when the caller wants the per-layer hidden states (memcpy nodes to caller memory), is capturing the stream
  // itself, or asked for eager launches.
  if (slab >= 0 || !call.graph_ok || hidden_states || attentions) return eager();
  // One new frame per call (the streaming step proper): ONE graph per cache serves every position.  The caller's tensors
  // and the position reach the kernels through a small device block that the patch extraction writes in front of the replay;
  // only the key-pass class is compiled in.
  // Several frames per call keep one graph per (position, count): their attention kernels take the position by value.
  const bool posfree = T_new == 1 && !sf_sw(SW_STREAM_GRAPH_PER_POSITION);
  if (!posfree && T_new == 1 && c->policy == 1) return set_err(SF_ERR_STATE, "SF_STREAM_GRAPH_PER_POSITION cannot serve a sliding-window cache");
  if (!c->warmed.count(kLockstepWarm)) {      // first graph-eligible call of this cache
    rc = eager();
    if (rc == SF_OK) c->warmed.insert(kLockstepWarm);
    return rc;
  }
  const int F = c->B * T_new, kcls = key_pass_class(pos.tk);
  sf_cache::GraphKey key;
  key.kind = posfree ? sf_cache::POSITION_FREE : sf_cache::PER_POSITION; key.rows = c->B; key.T_new = T_new; key.at = posfree ? kcls : len;
  key.pooler = pooler != nullptr; key.pixel_kind = posfree ? call.pk : 0;      // (per position: the patch extraction stays outside the graph)
  // patch extraction reads the caller's frames: outside the graphs.  For the position-free graph the same launch stores the call's
  // parameter block {pixels, outputs, position} that the graph's kernels read, after the graph is there
  SfStreamParams v;
  v.pixels = pixels; v.lhs = last_hidden; v.pooler = pooler; v.t_row = pos.t_row; v.slot = pos.slot; v.tk = pos.tk;
  auto patchify = [&](bool deliver) {
    return sf_launch_patchify(pixels, call.pk, ws.xn_hi, ws.xn_lo, F, e->cfg.num_channels, c->H, c->W, e->cfg.patch_size, s, &e->pixel_norm, nullptr,
                              deliver ? c->dparams : nullptr, deliver ? &v : nullptr, e->Kp);
  };
  if (!posfree) HIP_TRY(patchify(false));
  hipGraphExec_t exec = nullptr;
  rc = stream_graph(c, key, workspace, pos_dev, [&](hipStream_t on) -> int {
    if (posfree) return run_position_free(e, c, call, kcls, false, pooler != nullptr, on);
    ForwardRequest q = rq;      // at this position, into graph-owned outputs
    q.last_hidden = ws.lhs_stage; q.pooler = pooler ? ws.pool_stage : nullptr; q.ready = 1;
    return run_forward(e, q, ws, on);
  }, &exec);
  if (rc) return rc;
  if (posfree) HIP_TRY(patchify(true));
  // (Launching the embedding + first layers eagerly to cover the replay's host-side submit time measured no gain: 0.78 vs 0.77 ms.)
  HIP_TRY(hipGraphLaunch(exec, s));
  if (!posfree)
    HIP_TRY(sf_launch_copy2(ws.lhs_stage, last_hidden, (size_t)F * c->N * e->D, pooler ? ws.pool_stage : nullptr, pooler, (size_t)F * e->D, s));
  c->advance(T_new);
  return SF_OK;
}

extern "C" int sf_forward_stream(sf_encoder* e, sf_cache* c, const void* pixels, int pixel_dtype, int T_new,
                                 float* last_hidden, float* pooler, float* hidden_states, const float* pos_dev, void* workspace,
                                 size_t workspace_bytes, sf_stream stream) {
  return forward_stream_impl(e, c, pixels, pixel_dtype, T_new, last_hidden, pooler, hidden_states, nullptr, pos_dev, workspace, workspace_bytes,
                             stream);
}
// output_attentions while streaming (timesformer_encoder.py:494, 557, 633, 659, 720-754): the spatial attention probabilities of
// the NEW frames, [L, B * T_new, heads, N, N] fp32, as sf_forward_attentions returns them for whole clips
extern "C" int sf_forward_stream_attentions(sf_encoder* e, sf_cache* c, const void* pixels, int pixel_dtype, int T_new,
                                            float* last_hidden, float* pooler, float* hidden_states, float* attentions,
                                            const float* pos_dev, void* workspace, size_t workspace_bytes, sf_stream stream) {
  if (!attentions) return set_err(SF_ERR_INVALID, "null attentions buffer");
  return forward_stream_impl(e, c, pixels, pixel_dtype, T_new, last_hidden, pooler, hidden_states, attentions, pos_dev, workspace,
                             workspace_bytes, stream);
}

// Ragged streaming: the named streams of one batched cache advance, each from its own position.  One frame per stream (the streaming
// step proper): the same launch sequence as the lockstep call of n_streams rows, with {slab, time row, slot, keys} of every row group
// read from a device table that the patch extraction writes next to the parameter block — so one captured graph per (rows, key-pass
// class, pooler, pixel kind) serves every combination of positions.  The key-pass class comes from the longest stream of the call;
// shorter ones are masked by the kernels' own key < tk test.
extern "C" int sf_forward_stream_slots(sf_encoder* e, sf_cache* c, const void* pixels, int pixel_dtype, int T_new, const int* streams,
                                       int n_streams, float* last_hidden, float* pooler, const float* pos_dev, void* workspace,
                                       size_t workspace_bytes, sf_stream stream) {
  int rc = check_cache_owner(e, c);
  if (rc) return rc;
  if (!streams || n_streams <= 0) return set_err(SF_ERR_INVALID, "name at least one stream");
  if (T_new <= 0) return set_err(SF_ERR_INVALID, "T_new must be positive");
  {
    std::vector<char> named(c->B, 0);
    for (int i = 0; i < n_streams; ++i) {
      const int st = streams[i];
      if (st < 0 || st >= c->B) return set_err(SF_ERR_INVALID, "stream %d outside this cache's %d streams (ids are 0 .. %d)", st, c->B, c->B - 1);
      if (named[st]) return set_err(SF_ERR_INVALID, "stream %d named twice: a stream advances once per call, pass several frames of one stream as T_new > 1", st);
      named[st] = 1;
    }
  }
  if (T_new > 1) {
    if (n_streams != 1)
      return set_err(SF_ERR_INVALID, "T_new = %d with %d streams: several frames per call are the prefill of ONE stream — call once per stream with "
                     "n_streams = 1, then advance the streams together one frame per call", T_new, n_streams);
    return forward_stream_impl(e, c, pixels, pixel_dtype, T_new, last_hidden, pooler, nullptr, nullptr, pos_dev, workspace, workspace_bytes, stream,
                               streams[0]);
  }
  if (n_streams > SF_MAX_CALL_STREAMS)
    return set_err(SF_ERR_INVALID, "%d streams in one call; the stream table holds %d: split the call", n_streams, SF_MAX_CALL_STREAMS);
  const int n = n_streams;
  // every stream's position, checked before anything is launched
  SfStreamTable tv;
  memset(&tv, 0, sizeof(tv));
  tv.n = n;
  int max_tk = 0;
  auto positions = [&]() -> int {
    for (int i = 0; i < n; ++i) {
      StreamPos p;
      if (int r = stream_position(c, c->lens[streams[i]], 1, streams[i], &p)) return r;
      tv.e[i] = {streams[i], p.t_row, p.slot, p.tk};
      max_tk = p.tk > max_tk ? p.tk : max_tk;
    }
    return SF_OK;
  };
  StreamCall call;
  if ((rc = open_stream_call(e, c, n, 1, false, pixels, pixel_dtype, last_hidden, pos_dev, workspace, workspace_bytes, stream, positions, &call))) return rc;
  const int kcls = key_pass_class(max_tk);
  sf_cache::GraphKey key;
  key.kind = sf_cache::RAGGED; key.rows = n; key.T_new = 1; key.at = kcls; key.pooler = pooler != nullptr; key.pixel_kind = call.pk;
  // the launch that extracts the patch matrix delivers the parameter block and the table
  const Workspace& ws = call.ws;
  hipStream_t s = call.s;
  SfStreamParams v;
  v.pixels = pixels; v.lhs = last_hidden; v.pooler = pooler; v.t_row = tv.e[0].t_row; v.slot = tv.e[0].slot; v.tk = max_tk;
  auto deliver = [&]() -> hipError_t {
    return sf_launch_patchify(pixels, call.pk, ws.xn_hi, ws.xn_lo, n, e->cfg.num_channels, c->H, c->W, e->cfg.patch_size, s, &e->pixel_norm, nullptr,
                              c->dparams, &v, e->Kp, c->dtable, &tv);
  };
  auto run = [&](hipStream_t on) -> int { return run_position_free(e, c, call, kcls, true, pooler != nullptr, on); };
  if (call.graph_ok && c->warmed.count(key)) {
    hipGraphExec_t exec = nullptr;
    if ((rc = stream_graph(c, key, workspace, pos_dev, run, &exec))) return rc;
    HIP_TRY(deliver());
    HIP_TRY(hipGraphLaunch(exec, s));
  } else {      // graphs off, or the first call of this key
    HIP_TRY(deliver());
    if ((rc = run(s))) return rc;
    if (call.graph_ok) c->warmed.insert(key);
  }
  for (int i = 0; i < n; ++i) c->lens[streams[i]] += 1;
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// single operators (parity tests)
// ------------------------------------------------------------------------------------------------
__global__ void sf_combine_kernel(const bf16_t* hi, const bf16_t* lo, float* out, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = bf2f(hi[i]) + (lo ? bf2f(lo[i]) : 0.f);
}

extern "C" int sf_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int D,
                               float eps, sf_stream stream) {
  HIP_TRY(sf_launch_layernorm(x, gamma, beta, y, nullptr, nullptr, rows, D, eps, (hipStream_t)stream));
  return SF_OK;
}

extern "C" size_t sf_op_linear_workspace_bytes(int M, int N, int K) {
  return ((size_t)M * K * 2 + (size_t)N * K * 2 + (size_t)M * N * 2) * 2 + 4096;
}

extern "C" int sf_op_linear(const float* x, const float* w, const float* b, const float* resid, float alpha, int gelu,
                            float* y, int M, int N, int K, int compute, void* workspace, size_t workspace_bytes,
                            sf_stream stream) {
  if (workspace_bytes < sf_op_linear_workspace_bytes(M, N, K)) return set_err(SF_ERR_WORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const bool split = compute == SF_COMPUTE_BF16X3;
  SfCarver c(workspace);
  bf16_t* xh = c.take<bf16_t>((size_t)M * K); bf16_t* xl = c.take<bf16_t>((size_t)M * K);
  bf16_t* wh = c.take<bf16_t>((size_t)N * K); bf16_t* wl = c.take<bf16_t>((size_t)N * K);
  bf16_t* oh = c.take<bf16_t>((size_t)M * N); bf16_t* ol = c.take<bf16_t>((size_t)M * N);
  HIP_TRY(sf_launch_split(x, xh, split ? xl : nullptr, (size_t)M * K, s));
  HIP_TRY(sf_launch_split(w, wh, split ? wl : nullptr, (size_t)N * K, s));
  SfGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.a_hi = xh; g.a_lo = split ? xl : nullptr; g.w_hi = wh; g.w_lo = split ? wl : nullptr; g.bias = b;
  g.M = M; g.N = N; g.K = K; g.ldc = N; g.alpha = alpha; g.resid = resid; g.act = 0;
  if (gelu) {
    g.epi = SF_EPI_ACT_BF16; g.out_hi = oh; g.out_lo = split ? ol : nullptr;
    HIP_TRY(sf_launch_gemm(g, split, s));
    HIP_TRY(sf_launch(sf_combine_kernel, dim3(1024), dim3(256), 0, s, oh, split ? ol : nullptr, y, (size_t)M * N));
  } else {
    g.epi = resid ? SF_EPI_RESID_F32 : SF_EPI_F32; g.out_f32 = y;
    HIP_TRY(sf_launch_gemm(g, split, s));
  }
  return SF_OK;
}

// One forward GEMM with every field of SfGemmArgs the forward sets, on the operand planes as given: the parity tests' way to each
// family and epilogue alone.  Everything the host can check is checked before anything is launched; a named family launches only what
// its own sf_gemm_*_supported accepts.
static const char* gemm_family_name(int f) {
  static const char* const names[] = {"none", "skinny", "tile", "panel", "256^2", "128^2", "256-column + 128-column tail", "lab pipe", "lab pp"};
  return f >= 0 && f <= 8 ? names[f] : "?";
}
extern "C" int sf_op_gemm(const sf_gemm_desc* d, int family, int* family_taken, sf_stream stream) {
  if (family_taken) *family_taken = SF_GEMM_FAM_NONE;
  if (!d) return set_err(SF_ERR_INVALID, "sf_op_gemm: null descriptor");
  if (family < 0 || family > SF_GEMM_FAM_G128) return set_err(SF_ERR_INVALID, "sf_op_gemm: family %d is not one of 0 (dispatch) .. 5", family);
  const bool split = d->split != 0;
  if (d->M <= 0 || d->N <= 0 || d->K <= 0) return set_err(SF_ERR_INVALID, "sf_op_gemm: bad shape M=%d N=%d K=%d", d->M, d->N, d->K);
  if (d->ldc < d->N) return set_err(SF_ERR_INVALID, "sf_op_gemm: ldc %d < N %d", d->ldc, d->N);
  if (!d->a_hi || !d->w_hi) return set_err(SF_ERR_INVALID, "sf_op_gemm: a_hi and w_hi are required");
  if (split && (!d->a_lo || !d->w_lo)) return set_err(SF_ERR_INVALID, "sf_op_gemm: split needs a_lo and w_lo");
  if (!split && (d->a_lo || d->w_lo)) return set_err(SF_ERR_INVALID, "sf_op_gemm: a_lo / w_lo given without split");
  if (d->act < 0 || d->act > 2) return set_err(SF_ERR_INVALID, "sf_op_gemm: act %d is not 0 (erf GELU), 1 (tanh GELU) or 2 (ReLU)", d->act);
  if (d->resid_mod < 0) return set_err(SF_ERR_INVALID, "sf_op_gemm: resid_mod %d < 0", d->resid_mod);
  if (d->resid_mod > 0 && !d->resid) return set_err(SF_ERR_INVALID, "sf_op_gemm: resid_mod needs the fp32 resid table");
  if ((d->resid_hi != nullptr) != (d->resid_lo != nullptr)) return set_err(SF_ERR_INVALID, "sf_op_gemm: resid_hi and resid_lo come together");
  if (d->resid_lo2 && !d->resid_hi) return set_err(SF_ERR_INVALID, "sf_op_gemm: resid_lo2 needs resid_hi and resid_lo");
  if (d->resid && d->resid_hi) return set_err(SF_ERR_INVALID, "sf_op_gemm: resid and resid_hi / resid_lo are two forms of one operand: give one");
  if (d->out_lo && !d->out_hi) return set_err(SF_ERR_INVALID, "sf_op_gemm: out_lo needs out_hi");
  if (d->out_lo2 && !d->out_lo) return set_err(SF_ERR_INVALID, "sf_op_gemm: out_lo2 needs out_hi and out_lo");
  if (!d->ln_inkernel && (d->ln_stats != nullptr) != (d->ln_s != nullptr))
    return set_err(SF_ERR_INVALID, "sf_op_gemm: ln_stats and ln_s come together");
  if (d->ln_inkernel && !d->ln_s) return set_err(SF_ERR_INVALID, "sf_op_gemm: ln_inkernel needs ln_s");
  if (d->ln_inkernel && d->ln_stats) return set_err(SF_ERR_INVALID, "sf_op_gemm: ln_inkernel and ln_stats are two forms of one fold: give one");
  if ((d->ln_stats || d->ln_inkernel) && d->ln_stats_out) return set_err(SF_ERR_INVALID, "sf_op_gemm: a fold consumer does not produce statistics");
  if (d->grp_rows < 0 || (d->grp_rows > 0 && (d->grp_stride < d->grp_rows || d->grp_off < 0)))
    return set_err(SF_ERR_INVALID, "sf_op_gemm: row remap grp_rows=%d grp_stride=%d grp_off=%d (stride >= rows > 0, off >= 0)", d->grp_rows, d->grp_stride, d->grp_off);
  switch (d->epi) {
    case SF_EPI_F32:
      if (!d->out_f32) return set_err(SF_ERR_INVALID, "sf_op_gemm: SF_EPI_F32 needs out_f32");
      break;
    case SF_EPI_BF16: case SF_EPI_ACT_BF16:
      if (!d->out_hi) return set_err(SF_ERR_INVALID, "sf_op_gemm: a bf16 epilogue needs out_hi");
      break;
    case SF_EPI_RESID_F32:
      if (!d->resid && !d->resid_hi) return set_err(SF_ERR_INVALID, "sf_op_gemm: SF_EPI_RESID_F32 needs resid or resid_hi / resid_lo");
      if (d->resid && !d->out_f32) return set_err(SF_ERR_INVALID, "sf_op_gemm: an fp32 residual needs out_f32");
      if (d->resid_hi && (!d->out_hi || !d->out_lo)) return set_err(SF_ERR_INVALID, "sf_op_gemm: a plane-form residual needs out_hi and out_lo");
      break;
    case SF_EPI_EMBED_F32:
      if (!d->out_f32 || !d->pos || !d->time_rows || d->Np <= 0 || d->Tn <= 0)
        return set_err(SF_ERR_INVALID, "sf_op_gemm: SF_EPI_EMBED_F32 needs out_f32, pos, time_rows, Np > 0 and Tn > 0");
      break;
    default: return set_err(SF_ERR_INVALID, "sf_op_gemm: unknown epilogue %d", d->epi);
  }
  if (d->epi != SF_EPI_RESID_F32 && (d->resid || d->resid_hi)) return set_err(SF_ERR_INVALID, "sf_op_gemm: a residual is given to epilogue %d", d->epi);
  if (d->ln_stats_out && !d->out_hi) return set_err(SF_ERR_INVALID, "sf_op_gemm: ln_stats_out comes with the bf16 plane out_hi the consumer reads");
  SfGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.a_hi = d->a_hi; g.a_lo = d->a_lo; g.w_hi = d->w_hi; g.w_lo = d->w_lo; g.bias = d->bias;
  g.M = d->M; g.N = d->N; g.K = d->K; g.epi = d->epi; g.act = d->act; g.alpha = d->alpha;
  g.resid = d->resid; g.resid_mod = d->resid_mod; g.resid_hi = d->resid_hi; g.resid_lo = d->resid_lo; g.resid_lo2 = d->resid_lo2;
  g.pos = d->pos; g.time_rows = d->time_rows; g.Np = d->Np; g.Tn = d->Tn;
  g.out_f32 = d->out_f32; g.out_hi = d->out_hi; g.out_lo = d->out_lo; g.out_lo2 = d->out_lo2; g.ldc = d->ldc;
  g.grp_rows = d->grp_rows; g.grp_stride = d->grp_stride; g.grp_off = d->grp_off;
  g.ln_stats_out = d->ln_stats_out; g.ln_stats = d->ln_stats; g.ln_s = d->ln_s; g.ln_eps = d->ln_eps;
  g.ln_stats_wide = d->ln_stats_wide; g.ln_inkernel = d->ln_inkernel;
  SfGemmFamily fam = SF_GEMM_FAM_NONE;
  if (family == 0) {
    fam = sf_gemm_family(g, split);
    if (fam == SF_GEMM_FAM_NONE) return set_err(SF_ERR_INVALID, "sf_op_gemm: no GEMM family takes this call");
  } else {
    bool ok = false;
    switch (family) {
      case SF_GEMM_FAM_SKINNY: ok = sf_gemm_skinny_supported(g, split); break;
      case SF_GEMM_FAM_TILE: ok = sf_gemm_tile_supported(g, split); break;
      case SF_GEMM_FAM_PANEL: ok = sf_gemm_panel_supported(g, split); break;
      case SF_GEMM_FAM_G256: ok = sf_gemm256_supported(g, split); break;
      default: ok = sf_gemm128_supported(g, split); break;
    }
    if (!ok) return set_err(SF_ERR_INVALID, "sf_op_gemm: the %s family does not take this call (its sf_gemm_*_supported says no)", gemm_family_name(family));
    fam = (SfGemmFamily)family;
  }
  // fields that only some kernels read: the others would ignore them (or read a null buffer in their place), so the call is refused
  const bool p256 = fam == SF_GEMM_FAM_PANEL || fam == SF_GEMM_FAM_G256;
  const char* stray = nullptr;
  if (g.resid_mod > 0 && fam != SF_GEMM_FAM_PANEL) stray = "resid_mod (panel kernel only)";
  else if (g.resid_hi && !p256) stray = "resid_hi / resid_lo (panel and 256^2 kernels only)";
  else if ((g.resid_lo2 || g.out_lo2) && fam != SF_GEMM_FAM_G256) stray = "resid_lo2 / out_lo2 (256^2 kernel only)";
  else if (g.ln_stats && fam != SF_GEMM_FAM_G256) stray = "ln_stats (256^2 kernel only)";
  else if (g.ln_stats_out && !p256 && fam != SF_GEMM_FAM_TILE) stray = "ln_stats_out (tile, panel and 256^2 kernels only)";
  else if (g.ln_inkernel && fam != SF_GEMM_FAM_SKINNY && fam != SF_GEMM_FAM_TILE) stray = "ln_inkernel (skinny and tile kernels only)";
  else if (g.grp_rows > 0 && (fam == SF_GEMM_FAM_PANEL || fam == SF_GEMM_FAM_TILE) && g.epi != SF_EPI_BF16 && g.epi != SF_EPI_ACT_BF16) stray = "the row remap (not on this kernel's fp32 epilogues)";
  else if ((fam == SF_GEMM_FAM_G128 || fam == SF_GEMM_FAM_COLSPLIT) && !sf_gemm128_supported(g, split)) stray = "a field the 128^2 kernel does not read";
  else if (fam == SF_GEMM_FAM_SKINNY && g.epi == SF_EPI_RESID_F32 && !g.resid) stray = "a plane-form residual";
  if (stray) return set_err(SF_ERR_INVALID, "sf_op_gemm: the %s family does not read %s", gemm_family_name(fam), stray);
  HIP_TRY(sf_launch_gemm_family(fam, g, split, (hipStream_t)stream));
  if (family_taken) *family_taken = (int)fam;
  return SF_OK;
}

extern "C" size_t sf_op_attention_workspace_bytes(int groups, int L, int heads, int head_dim) {
  const size_t rows = (size_t)groups * L, D = (size_t)heads * head_dim;
  return rows * 3 * D * 2 * 2 + rows * D * 2 * 2 + 4096;     // qkv hi (+ lo) planes, ctx hi + lo
}

extern "C" int sf_op_attention(const float* qkv, float* ctx, int groups, int L, int heads, int head_dim, int causal,
                               int temporal_layout, int N_tokens, int compute, void* workspace, size_t workspace_bytes,
                               sf_stream stream) {
  if (head_dim < 8 || head_dim > 128 || head_dim % 8) return set_err(SF_ERR_INVALID, "head_dim must be a multiple of 8 in 8..128");
  if (workspace_bytes < sf_op_attention_workspace_bytes(groups, L, heads, head_dim)) return set_err(SF_ERR_WORKSPACE, "workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const bool acc = compute == SF_COMPUTE_BF16X3;
  const int D = heads * head_dim;
  const size_t rows = (size_t)groups * L;
  SfCarver c(workspace);
  bf16_t* ch = c.take<bf16_t>(rows * D);
  bf16_t* cl = c.take<bf16_t>(rows * D);
  bf16_t* qb = c.take<bf16_t>(rows * 3 * D);
  const void* base = qkv;
  size_t esz = 4;
  const bool planes = acc && head_dim == 64 && (temporal_layout ? sf_temporal_planes_ok(L, L) : sf_spatial_planes_ok(L, false));
  bf16_t* ql = nullptr;
  if (!acc || planes) {
    if (planes) ql = c.take<bf16_t>(rows * 3 * D);
    HIP_TRY(sf_launch_split(qkv, qb, ql, rows * 3 * D, s));
    base = qb;
    esz = 2;
  }
  SfAttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = base; a.k = (const char*)base + (size_t)D * esz; a.v = (const char*)base + (size_t)2 * D * esz;
  a.in_is_f32 = acc && !planes; a.lo_plane_off = planes ? (long long)(ql - qb) : 0;
  a.row_pitch_q = 3 * D; a.row_pitch_kv = 3 * D; a.heads = heads; a.scale = 1.0f / sqrtf((float)head_dim);
  a.ctx_hi = ch; a.ctx_lo = cl; a.D = D; a.head_dim = head_dim;
  if (temporal_layout) {
    // rows are [B, L, N_tokens, 3D] with groups = B * N_tokens sequences of length L
    if (N_tokens <= 0 || groups % N_tokens) return set_err(SF_ERR_INVALID, "groups must be a multiple of N_tokens");
    a.N = N_tokens; a.B = groups / N_tokens; a.Tq = L; a.Tk = L; a.Tcap = L; a.t_past = 0; a.causal = causal;
    a.Tq_cap = L; a.q_t0 = 0;
    HIP_TRY(sf_launch_temporal_attention(a, acc, s));
  } else {
    if (causal) return set_err(SF_ERR_INVALID, "the spatial layout has no causal variant");
    a.N = L; a.frames = groups;
    HIP_TRY(sf_launch_spatial_attention(a, acc, s));
  }
  HIP_TRY(sf_launch(sf_combine_kernel, dim3(1024), dim3(256), 0, s, ch, acc ? cl : nullptr, ctx, rows * D));
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// loss heads
// ------------------------------------------------------------------------------------------------
extern "C" size_t sf_loss_workspace_bytes(int B, int T) {
  return sf_loss_partial_bytes(B > 0 && T > 0 ? B * T : 1);
}
extern "C" int sf_retrieval_loss(const float* pooler, const float* text, int B, int T, int D, int Bt, int pos_offset,
                                 const float* logit_scale, const float* logit_bias, float* loss, float* grad_pooler,
                                 float* grad_scalars, void* workspace, size_t workspace_bytes, sf_stream stream) {
  if (!pooler || !text || !loss || !logit_scale || !logit_bias || !workspace) return set_err(SF_ERR_INVALID, "sf_retrieval_loss: null buffer");
  if (B <= 0 || Bt <= 0 || T <= 0 || D <= 0) return set_err(SF_ERR_INVALID, "sf_retrieval_loss: bad shape B=%d Bt=%d T=%d D=%d", B, Bt, T, D);
  if (D > 2048) return set_err(SF_ERR_CAPACITY, "sf_retrieval_loss: feature width %d > 2048 (256 threads x 8 features)", D);
  if (pos_offset >= 0 && pos_offset + B > Bt)
    return set_err(SF_ERR_INVALID, "sf_retrieval_loss: positives %d..%d fall outside the %d text rows", pos_offset, pos_offset + B - 1, Bt);
  if (workspace_bytes < sf_loss_partial_bytes(B)) return set_err(SF_ERR_WORKSPACE, "loss workspace %zu < %zu bytes", workspace_bytes, sf_loss_partial_bytes(B));
  HIP_TRY(sf_launch_retrieval_loss(pooler, text, B, T, D, Bt, pos_offset, logit_scale, logit_bias, loss, grad_pooler,
                                   grad_scalars, (float*)workspace, (hipStream_t)stream));
  return SF_OK;
}
extern "C" int sf_localization_loss(const float* pooler, const float* label_emb, const int32_t* labels, int B, int T,
                                    int D, int L, const float* logit_scale, const float* logit_bias, float* loss,
                                    float* grad_pooler, float* grad_scalars, void* workspace, size_t workspace_bytes,
                                    sf_stream stream) {
  if (!pooler || !label_emb || !labels || !loss || !logit_scale || !logit_bias || !workspace) return set_err(SF_ERR_INVALID, "sf_localization_loss: null buffer");
  if (B <= 0 || T <= 0 || D <= 0 || L <= 0) return set_err(SF_ERR_INVALID, "sf_localization_loss: bad shape B=%d T=%d D=%d L=%d", B, T, D, L);
  if (L > 4096) return set_err(SF_ERR_CAPACITY, "sf_localization_loss: %d label classes > 4096 (one LDS row of similarities per frame)", L);
  if (workspace_bytes < sf_loss_partial_bytes(B * T)) return set_err(SF_ERR_WORKSPACE, "loss workspace %zu < %zu bytes", workspace_bytes, sf_loss_partial_bytes(B * T));
  HIP_TRY(sf_launch_localization_loss(pooler, label_emb, labels, B, T, D, L, logit_scale, logit_bias, loss, grad_pooler,
                                      grad_scalars, (float*)workspace, (hipStream_t)stream));
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// bench hook: time the dominant GEMM with HIP events on the caller's stream
// ------------------------------------------------------------------------------------------------
extern "C" int sf_bench_gemm(sf_encoder* e, int M, int which, int iters, void* workspace, size_t workspace_bytes,
                             sf_stream stream, float* mean_ms_out, double* flops_out) {
  if (!e || !e->finalized || e->layers.empty()) return set_err(SF_ERR_STATE, "encoder not finalized");
  if (iters <= 0 || M <= 0 || !workspace || !mean_ms_out) return set_err(SF_ERR_INVALID, "bad argument");
  const DevLayer& l = e->layers[0];
  // which 0..3 = MLP-up, MLP-down, qkv, attention out-proj with the epilogues the forward gives them; 4 / 5 = out-proj / MLP-down PLAIN (bf16
  // output, no residual, no row sums): the like-for-like partner of a vendor-library GEMM (bench.py roofline.yardstick_tflops)
  const bool plain = which == 4 || which == 5;
  if (plain) which = which == 4 ? 3 : 1;
  const DevLinear* lin = which == 0 ? &l.up : which == 1 ? &l.down : which == 2 ? &l.s_qkv : &l.s_out;
  const bool acc = e->compute == SF_COMPUTE_BF16X3;
  SfCarver c(workspace);
  bf16_t* ah = c.take<bf16_t>((size_t)M * lin->K);
  bf16_t* al = c.take<bf16_t>((size_t)M * lin->K);
  bf16_t* oh = c.take<bf16_t>((size_t)M * lin->N);
  bf16_t* ol = c.take<bf16_t>((size_t)M * lin->N);
  float* of = c.take<float>((size_t)M * lin->N);
  if (c.off > workspace_bytes) return set_err(SF_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, c.off);
  hipStream_t s = (hipStream_t)stream;
  const int epi = plain ? (acc ? SF_EPI_F32 : SF_EPI_BF16) : which == 0 ? SF_EPI_ACT_BF16 : which == 2 ? (acc ? SF_EPI_F32 : SF_EPI_BF16) : SF_EPI_RESID_F32;
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  if (acc && epi == SF_EPI_RESID_F32) oh = nullptr;     // the accurate mode keeps no bf16 copy of the residual (no LayerNorm fold)
  // bf16 mode at BASELINE-sized M: the residual projections as the forward launches them — hi + lo planes in and out, LayerNorm
  // row sums of the next Linear (ForwardPlan's `fold + pm`); fp32 residual + bf16 copy otherwise
  const bool pm = !sf_sw(SW_DISABLE_RESID_PLANES) && !acc && epi == SF_EPI_RESID_F32 && !ln_fold_tile_ok(e, M) && !ln_fold_small_ok(e, M) &&
                  ln_fold_panel_ok(e, M);
  float* st = pm ? c.take<float>((size_t)M * 8) : nullptr;
  if (c.off > workspace_bytes) return set_err(SF_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, c.off);
  if (st) HIP_TRY(hipMemsetAsync(st, 0, (size_t)M * 8 * sizeof(float), (hipStream_t)stream));
  SfGemmArgs g = linear_args(e, *lin, ah, al, M, epi, acc);
  g.alpha = 0.f; g.out_hi = oh;
  if (pm) { g.out_lo = ol; g.resid_hi = oh; g.resid_lo = ol; g.ln_stats_out = st; }
  else { g.out_f32 = of; g.resid = of; g.out_lo = acc ? ol : nullptr; }
  auto go = [&]() { return sf_launch_gemm(g, acc, s); };
  HIP_TRY(go());   // warm
  HIP_TRY(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) HIP_TRY(go());
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *mean_ms_out = ms / iters;
  if (flops_out) *flops_out = 2.0 * M * (double)lin->N * (double)lin->K;
  return SF_OK;
}

extern "C" int sf_bench_attention(sf_encoder* e, int B, int T, int which, int iters, void* workspace,
                                  size_t workspace_bytes, sf_stream stream, float* mean_ms_out, double* bytes_out,
                                  double* flops_out) {
  if (!e || !e->finalized) return set_err(SF_ERR_STATE, "encoder not finalized");
  if (iters <= 0 || B <= 0 || T <= 0 || !workspace || !mean_ms_out) return set_err(SF_ERR_INVALID, "bad argument");
  const bool acc = e->compute == SF_COMPUTE_BF16X3;
  const int D = e->D, N = e->N, heads = e->cfg.num_attention_heads;
  const size_t M = (size_t)B * T * N, esz = acc ? 4 : 2;
  SfCarver c(workspace);
  char* qkv = c.take<char>(M * 3 * D * esz);
  bf16_t* ch = c.take<bf16_t>(M * D);
  bf16_t* cl = c.take<bf16_t>(M * D);
  if (c.off > workspace_bytes) return set_err(SF_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, c.off);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipMemsetAsync(qkv, 0x3c, M * 3 * D * esz, s));   // finite, non-trivial bit pattern
  SfAttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = qkv; a.k = qkv + (size_t)D * esz; a.v = qkv + (size_t)2 * D * esz;
  a.in_is_f32 = acc; a.row_pitch_q = 3 * D; a.row_pitch_kv = 3 * D; a.heads = heads; a.scale = 0.125f;
  a.ctx_hi = ch; a.ctx_lo = cl; a.D = D; a.N = N;
  if (which == 0 && acc && sf_spatial_planes_ok(N, false)) {      // what the forward does: hi + lo planes in the fp32 tensor's bytes
    a.k = qkv + (size_t)D * 2; a.v = qkv + (size_t)2 * D * 2;
    a.in_is_f32 = 0; a.lo_plane_off = (long long)M * 3 * D;
  }
  if (which == 1 && acc && sf_temporal_planes_ok(T, T)) {
    a.k = qkv + (size_t)D * 2; a.v = qkv + (size_t)2 * D * 2;
    a.in_is_f32 = 0; a.lo_plane_off = (long long)M * 3 * D;
  }
  if (which == 0) {
    a.frames = B * T;
  } else {
    a.B = B; a.Tq = T; a.Tk = T; a.Tcap = T; a.t_past = 0; a.causal = e->cfg.enable_causal_temporal; a.Tq_cap = T; a.q_t0 = 0;
  }
  auto launch = [&]() { return which == 0 ? sf_launch_spatial_attention(a, acc, s) : sf_launch_temporal_attention(a, acc, s); };
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  HIP_TRY(launch());
  HIP_TRY(hipEventRecord(e0, s));
  for (int i = 0; i < iters; ++i) HIP_TRY(launch());
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipEventSynchronize(e1));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *mean_ms_out = ms / iters;
  if (bytes_out) *bytes_out = (double)M * 3 * D * esz + (double)M * D * 2 * (acc ? 2 : 1);
  if (flops_out) {
    const double L = which == 0 ? N : T;        // 2 matmuls of L x L x 64 per (sequence, head), full (not causal-halved)
    const double seqs = which == 0 ? (double)B * T : (double)B * N;
    *flops_out = seqs * heads * 2.0 * (2.0 * L * L * 64.0);
  }
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// launch floor (bench hook): a graph of dependent empty kernels
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sf_null_kernel(int* sink) {
  if (sink && threadIdx.x == 1024) *sink = 0;     // never true: the kernel has no memory traffic
}
extern "C" int sf_bench_launch_floor(int device, int launches, int iters, sf_stream stream, float* us_per_launch_out) {
  if (launches <= 0 || iters <= 0 || !us_per_launch_out) return set_err(SF_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  hipStream_t cap = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&cap, hipStreamNonBlocking));
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipError_t err = hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal);
  if (err == hipSuccess) {
    for (int i = 0; i < launches && err == hipSuccess; ++i) err = sf_launch(sf_null_kernel, dim3(256), dim3(256), 0, cap, (int*)nullptr);
    const hipError_t end = hipStreamEndCapture(cap, &graph);
    if (err == hipSuccess) err = end;
  }
  if (err == hipSuccess) err = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  float ms = 0.f;
  if (err == hipSuccess) {
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipGraphLaunch(exec, s);
    (void)hipStreamSynchronize(s);
    (void)hipEventRecord(e0, s);
    for (int i = 0; i < iters; ++i) (void)hipGraphLaunch(exec, s);
    (void)hipEventRecord(e1, s);
    err = hipEventSynchronize(e1);
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  }
  if (exec) (void)hipGraphExecDestroy(exec);
  if (graph) (void)hipGraphDestroy(graph);
  (void)hipStreamDestroy(cap);
  if (err != hipSuccess) return set_err(SF_ERR_HIP, "sf_bench_launch_floor: %s", hipGetErrorString(err));
  *us_per_launch_out = 1e3f * ms / ((float)iters * (float)launches);
  return SF_OK;
}
