// C-ABI implementation of the training step (include/streamformer_hip.h, "training step" section):
// flat fp32 parameter layout, bf16 working weights, forward with saved activations, staged backward,
// fused AdamW.  Reference: autograd through TimesformerMultiTaskingModelSigLIP.forward
// (modeling:1299-1354; layer :934-1004; head :1141-1154; embeddings :413-457) under the step
// semantics of tools/finetune_tools.py:395-573 and the optimizer grouping of optim_factory.py:59-104.
#include "sf_internal.h"
#include "sf_common.h"
#include "sf_switches.h"
#include "sf_train.h"
#include "sf_pool_head.h"
#include "sf_weights.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static const int kRank = 32;   // modeling:1280-1281

struct TParam {
  std::string name;
  int64_t shape[4];
  int ndim;
  size_t numel, off;
  bool trainable, decay;
};

struct TLin {                    // y = x W^T + b over the flat buffer
  int N = 0, K = 0;
  int Nw = 0, Kw = 0;               // extents of the bf16 working copies and activations: N / K, or zero-padded to multiples of 64
                                    // (intermediate_size, C*P*P); gradients and parameters keep N x K
  int pw = -1; size_t pw_off = 0;   // weight: param index + float offset inside it
  int pb = -1; size_t pb_off = 0;   // bias (pb < 0: none)
  int pla = -1, plb = -1;           // LoRA factors (spatial qkv / output.dense)
  int pgate = -1;                   // temporal_dense: forward weight = tanh(gate) * W
  bf16_t* w = nullptr;              // [N,K] working copy
  bf16_t* wT = nullptr;             // [K,N] for the input-gradient GEMM
  bf16_t* la_bf = nullptr;          // LoRA A [r,K] and B^T [r,N] (factor gradients through skinny GEMMs)
  bf16_t* lbT_bf = nullptr;
  float* bias_scaled = nullptr;     // tanh(gate) * b, or the bias zero-padded to Nw
  bool need_wT = true;
  bool per_frame = false;           // runs over the B*T frame rows of the pooling head, not the B*T*N token rows
};

struct TLayer {
  int gate, ln_t_g, ln_t_b, ln_b_g, ln_b_b, ln_a_g, ln_a_b;
  TLin t_qkv, t_out, t_dense, s_qkv, s_out, up, down;
  size_t seg_off, seg_end;
  // temporal_dense o temporal_attention.output.dense as one projection (drop rates 0): W_f = tanh(g) W_d W_o [D, D], its transpose,
  // b_f = tanh(g) (W_d b_o + b_d); refreshed with the working weights (sf_launch_fuse_temporal)
  bf16_t* wf = nullptr; bf16_t* wfT = nullptr; float* bf = nullptr;
};
static const int kHeadLins = 5, kLayerLins = 7;   // sf_trainer::lins: patch, head_kv, head_out, fc1, fc2, then every layer's seven

// Dropout sites: a mask is keyed by layer * SITE_STRIDE + site (sf_drop_make), the backward replays it by naming the same site; embeddings: layer L
enum Site : unsigned {
  SITE_TEMPORAL_OUT = 0, SITE_SPATIAL_OUT = 1,        // the two SelfOutputs (modeling:761, 752)
  SITE_MLP_ACT = 2, SITE_MLP_OUT = 3,                 // behind the activation and the MLP output (modeling:822, 835)
  SITE_TEMPORAL_PROBS = 4, SITE_SPATIAL_PROBS = 5,    // attention probabilities
  SITE_EMBED_POS = 0, SITE_EMBED_TIME = 1,            // pos_drop / time_drop (modeling:374, 378)
  SITE_STRIDE = 8
};

// What sf_trainer_forward decided, filled once after its checks: everything the backward knows about the last forward.
struct StepPlan {
  bool valid = false;               // a forward has run to its end
  int B = 0, T = 0, N = 0, L = 0, M = 0, F = 0;      // M = B*T*N token rows, F = B*T frame rows
  const float* dp = nullptr;        // drop_path factors (device, caller-owned), [L][B*N + B*T + B]; nullptr = none
  float drop_hidden = 0.f, drop_attn = 0.f;
  unsigned seed = 0u;
  bool tfuse = false;               // the temporal branch's two projections ran as one
  bool scaled() const { return dp || drop_hidden > 0.f; }       // a row factor sits on every residual branch
  // grouped launch and side stream need a layer's operands untouched until its end (the row factors reuse d_ctx / d_tout); read per backward
  bool group_wgrads() const { return !scaled() && sf_sw(SW_WGRAD_UNGROUPED) == nullptr; }
  const float* dp_layer(int li, size_t off) const { return dp ? dp + (size_t)li * ((size_t)B * N + (size_t)B * T + (size_t)B) + off : nullptr; }
  const float* dp_temporal(int li) const { return dp_layer(li, 0); }
  const float* dp_spatial(int li) const { return dp_layer(li, (size_t)B * N); }
  const float* dp_mlp(int li) const { return dp_layer(li, (size_t)B * N + (size_t)B * T); }
  SfDrop hidden_site(int li, Site k) const { return sf_drop_make(drop_hidden, seed, (unsigned)li * SITE_STRIDE + k); }
  SfDrop attn_site(int li, Site k) const { return sf_drop_make(drop_attn, seed, (unsigned)li * SITE_STRIDE + k); }
  SfDrop embed_site(Site k) const { return hidden_site(L, k); }
};

// The rank-32 LoRA gradients of a layer (two projections, two small weight-gradient GEMMs + reductions per adapted Linear:
// ~1.8 ms per step at 8 clips, all bandwidth- / latency-bound launches that depend on nothing downstream) run on a library-owned
// side stream, forked from and joined into the caller's stream inside every layer: they fill the gaps of the MFMA-bound chain.  So does the
// D x D algebra of the fused temporal projections (six small launches per layer), joined one layer LATER (its inputs alternate by layer parity)
struct SideStream {
  hipStream_t stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_small[2] = {nullptr, nullptr};
  int small_pending = 0;            // bit p: ev_small[p] has been recorded and not yet waited for
  int state = 0;                    // 0 = not tried, 1 = available, -1 = unavailable (creation failed / SF_TRAIN_SIDE_STREAM=0)
  bool join_marked = false;         // ev_join already stands in front of later side work (mark_join)
  bool ready() {                    // created on first use; SF_TRAIN_SIDE_STREAM=0 keeps everything on the caller's stream (A/B)
    if (state == 0) {
      const char* e = sf_sw(SW_TRAIN_SIDE_STREAM);
      state = -1;
      auto event = [](hipEvent_t* ev) { return hipEventCreateWithFlags(ev, hipEventDisableTiming) == hipSuccess; };
      if (!(e && e[0] == '0') && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess && event(&ev_fork) && event(&ev_join) &&
          event(&ev_small[0]) && event(&ev_small[1]))
        state = 1;
    }
    return state == 1;
  }
  // the side stream continues behind everything `from` has enqueued so far
  hipError_t fork(hipStream_t from) { hipError_t e = hipEventRecord(ev_fork, from); return e != hipSuccess ? e : hipStreamWaitEvent(stream, ev_fork, 0); }
  // join(): `into` waits for the side work enqueued so far, or only up to the last mark_join() when there was one
  hipError_t mark_join() { join_marked = true; return hipEventRecord(ev_join, stream); }
  hipError_t join(hipStream_t into) {
    const hipError_t e = join_marked ? hipSuccess : hipEventRecord(ev_join, stream);
    join_marked = false;
    return e != hipSuccess ? e : hipStreamWaitEvent(into, ev_join, 0);
  }
  hipError_t mark_small(int par) { small_pending |= 1 << par; return hipEventRecord(ev_small[par], stream); }
  hipError_t wait_small(hipStream_t into, int par) {
    if (!(small_pending & (1 << par))) return hipSuccess;
    small_pending &= ~(1 << par);
    return hipStreamWaitEvent(into, ev_small[par], 0);
  }
  hipError_t drain(hipStream_t into) { hipError_t e = wait_small(into, 0); return e != hipSuccess ? e : wait_small(into, 1); }
  void destroy() {
    if (stream) (void)hipStreamDestroy(stream);
    for (hipEvent_t e : {ev_fork, ev_join, ev_small[0], ev_small[1]}) if (e) (void)hipEventDestroy(e);
  }
};

struct sf_trainer {
  sf_config cfg;
  int device;
  int D, I, L, heads, N, Kp, C, P;
  int hd;                           // head_dim: 64 runs the tuned attention / pooling kernels, other widths the generic ones
  int Ip, Kpp;                      // I and Kp padded to multiples of 64 (working copies and activations only)
  float scale;                      // head_dim^-0.5
  bool lora, freeze;
  std::vector<TParam> params;
  size_t total = 0, n_train = 0;
  int p_pos, p_time, p_probe, p_inw, p_inb, post_g, post_b, hln_g, hln_b;
  TLin patch, head_kv, head_out, fc1, fc2;
  std::vector<TLayer> layers;
  std::vector<TLin*> lins;          // every Linear above: kHeadLins, then kLayerLins per layer
  size_t emb_off, emb_end, tail_off, tail_end;
  // device state
  int* seg_end = nullptr;
  unsigned char* seg_decay = nullptr;
  unsigned char* seg_train = nullptr;
  int nseg = 0;
  bf16_t* arena = nullptr;
  float* farena = nullptr;          // scaled biases, head query, reduction scratch
  float* head_q = nullptr;
  float* head_u = nullptr;          // pooling head: U_h = Wk_h^T q_h, fp32 [16, D] (+ hi / lo bf16 planes), refreshed with the weights
  bf16_t* head_u_hi = nullptr; bf16_t* head_u_lo = nullptr;
  float* red_partial = nullptr;
  SfPrepJob* prep_jobs = nullptr;   // device table for sf_trainer_sync_weights
  int n_prep_jobs = 0, prep_tiles = 0;
  SfFuseJob* fuse_jobs = nullptr;   // device table of the fused temporal projections (one per layer)
  const float* params_dev = nullptr;
  StepPlan plan;                    // the last forward (plan.valid): its backward follows it
  const float* dp_scales = nullptr; // drop_path factors of the next forward (device, caller-owned), nullptr = none
  int dp_B = 0, dp_T = 0;
  float drop_hidden = 0.f, drop_attn = 0.f;     // dropout of the NEXT forward (sf_trainer_set_dropout)
  unsigned drop_seed = 0u;
  int n_extra = 0, extra_seg0 = 0;  // the scalar slots are the last n_extra trainable segments
  bool extra_steps_set = false;
  int extra_steps[64] = {};
  int* guard_flag = nullptr;          // non-finite guard (sf_trainer_set_nonfinite_guard): device int32[2], caller-owned
  const float* guard_loss = nullptr;  // optional device loss scalar checked next to the gradient's sum of squares
  float* guard_sumsq = nullptr;       // library-owned scalar the guard's own sum-of-squares pass writes
  SideStream side;
};

// ---- creation: config checks, parameter declaration, offsets, segment table, working arena + job tables ----------------------------
static int check_config(const sf_config& c, int n_extra) {
  // the width rules of sf_create: head_dim 64 on the tuned kernels, any other multiple of 8 up to 128 on the generic ones
  if (c.num_attention_heads <= 0 || c.hidden_size <= 0 || c.hidden_size % c.num_attention_heads)
    return sf_set_err(SF_ERR_INVALID, "hidden_size %d not divisible by heads %d", c.hidden_size, c.num_attention_heads);
  if (c.num_attention_heads > 16)
    return sf_set_err(SF_ERR_INVALID, "%d attention heads unsupported: training handles at most 16 heads", c.num_attention_heads);
  const int hd = c.hidden_size / c.num_attention_heads;
  if (hd < 8 || hd > 128 || hd % 8) return sf_set_err(SF_ERR_INVALID, "head_dim %d unsupported: training takes multiples of 8 from 8 to 128", hd);
  if (c.hidden_size % 64) return sf_set_err(SF_ERR_INVALID, "hidden_size %d unsupported: training needs a multiple of 64", c.hidden_size);
  if (c.intermediate_size <= 0 || c.intermediate_size % 4 || c.patch_size <= 0 || c.num_channels <= 0 ||
      (c.num_channels * c.patch_size * c.patch_size) % 4)
    return sf_set_err(SF_ERR_INVALID, "intermediate_size %d / patch vector %d: training needs positive multiples of 4", c.intermediate_size,
                      c.num_channels * c.patch_size * c.patch_size);
  if (c.hidden_act != 0) return sf_set_err(SF_ERR_INVALID, "training supports hidden_act=gelu only");
  if (c.image_size % c.patch_size) return sf_set_err(SF_ERR_INVALID, "image_size %% patch_size != 0");
  if (n_extra < 0 || n_extra > 64) return sf_set_err(SF_ERR_INVALID, "n_extra out of range");
  const int N = (c.image_size / c.patch_size) * (c.image_size / c.patch_size);
  if (N > 224) return sf_set_err(SF_ERR_INVALID, "%d patches per frame; kernels handle <= 224", N);
  return SF_OK;
}

static int add_param(sf_trainer* t, const std::string& name, std::initializer_list<int64_t> shape, bool trainable) {
  TParam p;
  p.name = name;
  p.ndim = (int)shape.size();
  p.numel = 1;
  int i = 0;
  for (int64_t d : shape) { p.shape[i++] = d; p.numel *= (size_t)d; }
  for (; i < 4; ++i) p.shape[i] = 1;
  p.off = 0;
  p.trainable = trainable;
  // optim_factory.py:72-77: 1-D parameters and "*.bias" are not decayed; everything else (incl. 0-dim) is
  const bool is_bias = name.size() >= 5 && name.compare(name.size() - 5, 5, ".bias") == 0;
  p.decay = !(p.ndim == 1 || is_bias);
  t->params.push_back(p);
  return (int)t->params.size() - 1;
}
static void ln_params(sf_trainer* t, const std::string& prefix, int* gamma, int* beta) {
  *gamma = add_param(t, prefix + ".weight", {t->D}, true);
  *beta = add_param(t, prefix + ".bias", {t->D}, true);
}
static void lin_params(sf_trainer* t, TLin* l, const std::string& prefix, int N, int K, bool bias, bool trainable, bool lora = false) {
  l->N = N; l->K = K; l->Nw = N; l->Kw = K;
  l->pw = add_param(t, prefix + ".weight", {N, K}, trainable);
  l->pb = bias ? add_param(t, prefix + ".bias", {N}, trainable) : -1;
  if (lora) {
    l->pla = add_param(t, prefix + "_lora_a.weight", {kRank, K}, true);
    l->plb = add_param(t, prefix + "_lora_b.weight", {N, kRank}, true);
  }
}

// parameter list in model order (names = reference state_dict keys), the Linears and their working extents
static void declare_params(sf_trainer* t) {
  const sf_config& c = t->cfg;
  const int D = t->D, I = t->I;
  t->p_pos = add_param(t, "embeddings.position_embeddings", {1, t->N, D}, true);
  t->p_time = add_param(t, "embeddings.time_embeddings", {1, c.num_frames, D}, true);
  t->patch.N = D; t->patch.K = t->Kp; t->patch.Nw = D; t->patch.Kw = t->Kpp; t->patch.need_wT = false;
  t->patch.pw = add_param(t, "embeddings.patch_embeddings.projection.weight", {D, t->C, t->P, t->P}, true);
  t->patch.pb = add_param(t, "embeddings.patch_embeddings.projection.bias", {D}, true);
  t->layers.resize(t->L);
  for (int i = 0; i < t->L; ++i) {
    TLayer& l = t->layers[i];
    const std::string p = "encoder.layer." + std::to_string(i) + ".";
    const bool sp_train = !t->freeze;
    l.gate = add_param(t, p + "temporal_attention_gating", {}, true);
    ln_params(t, p + "temporal_layernorm", &l.ln_t_g, &l.ln_t_b);
    lin_params(t, &l.t_qkv, p + "temporal_attention.attention.qkv", 3 * D, D, c.qkv_bias != 0, true);
    lin_params(t, &l.t_out, p + "temporal_attention.output.dense", D, D, true, true);
    lin_params(t, &l.t_dense, p + "temporal_dense", D, D, true, true);
    l.t_dense.pgate = l.gate;
    ln_params(t, p + "layernorm_before", &l.ln_b_g, &l.ln_b_b);
    lin_params(t, &l.s_qkv, p + "attention.attention.qkv", 3 * D, D, c.qkv_bias != 0, sp_train, t->lora);
    lin_params(t, &l.s_out, p + "attention.output.dense", D, D, true, sp_train, t->lora);
    ln_params(t, p + "layernorm_after", &l.ln_a_g, &l.ln_a_b);
    lin_params(t, &l.up, p + "intermediate.dense", I, D, true, true);
    lin_params(t, &l.down, p + "output.dense", D, I, true, true);
  }
  ln_params(t, "post_layernorm", &t->post_g, &t->post_b);
  t->p_probe = add_param(t, "head.probe", {1, 1, D}, true);
  t->p_inw = add_param(t, "head.attention.in_proj_weight", {3 * D, D}, true);
  t->p_inb = add_param(t, "head.attention.in_proj_bias", {3 * D}, true);
  t->head_kv.N = 2 * D; t->head_kv.K = D; t->head_kv.Nw = 2 * D; t->head_kv.Kw = D;
  t->head_kv.pw = t->p_inw; t->head_kv.pw_off = (size_t)D * D;
  t->head_kv.pb = t->p_inb; t->head_kv.pb_off = (size_t)D;
  lin_params(t, &t->head_out, "head.attention.out_proj", D, D, true, true);
  ln_params(t, "head.layernorm", &t->hln_g, &t->hln_b);
  lin_params(t, &t->fc1, "head.mlp.fc1", I, D, true, true);
  lin_params(t, &t->fc2, "head.mlp.fc2", D, I, true, true);
  for (int i = 0; i < t->n_extra; ++i) add_param(t, "extra." + std::to_string(i), {}, true);
  // zero-padded working extents of the MLPs (intermediate_size) and the patch projection (C*P*P): gelu(0) = 0 and zero weight
  // rows / columns make the padding exact; it never reaches the parameter / gradient layout
  for (TLayer& l : t->layers) { l.up.Nw = t->Ip; l.down.Kw = t->Ip; }
  t->fc1.Nw = t->Ip; t->fc2.Kw = t->Ip;
  t->head_out.per_frame = t->fc1.per_frame = t->fc2.per_frame = true;
  t->lins = {&t->patch, &t->head_kv, &t->head_out, &t->fc1, &t->fc2};
  for (TLayer& l : t->layers) for (TLin* x : {&l.t_qkv, &l.t_out, &l.t_dense, &l.s_qkv, &l.s_out, &l.up, &l.down}) t->lins.push_back(x);
}

static size_t round_up(size_t n, size_t q) { return (n + q - 1) & ~(q - 1); }      // q a power of two
static size_t seg_floats(const TParam& p) { return round_up(p.numel, 64); }        // every parameter starts on a 64-float boundary

// Offset order IS this order: the trainable parameters in declaration order, then the frozen ones in declaration order.
template <typename Fn> static void in_offset_order(sf_trainer* t, Fn fn) {
  for (bool trainable : {true, false}) for (TParam& p : t->params) if (p.trainable == trainable) fn(p);
}

static int assign_offsets(sf_trainer* t) {
  size_t off = 0;
  int ntr = 0;
  in_offset_order(t, [&](TParam& p) {
    p.off = off;
    off += seg_floats(p);
    if (p.trainable) { t->n_train = off; ++ntr; }
  });
  t->total = off;
  if (t->total >= ((size_t)1 << 31)) return sf_set_err(SF_ERR_INVALID, "model too large for int32 segment offsets");
  auto seg_end_of = [&](int idx) { const TParam& p = t->params[idx]; return p.off + seg_floats(p); };
  t->emb_off = t->params[t->p_pos].off;
  t->emb_end = seg_end_of(t->patch.pb);
  for (TLayer& l : t->layers) {
    l.seg_off = t->params[l.gate].off;
    l.seg_end = seg_end_of(l.down.pb);
  }
  t->tail_off = t->params[t->post_g].off;
  t->tail_end = t->n_train;
  t->extra_seg0 = ntr - t->n_extra;   // trainable segments come first in offset order, the extras last among them
  return SF_OK;
}

template <typename T> static int upload(T** dst, const std::vector<T>& v, const char* what) {
  if (hipMalloc(dst, v.size() * sizeof(T)) != hipSuccess) return sf_set_err(SF_ERR_HIP, "hipMalloc failed (%s)", what);
  if (!v.empty() && hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
    return sf_set_err(SF_ERR_HIP, "hipMemcpy failed (%s)", what);
  return SF_OK;
}

// the optimizer's segment table: one segment per parameter, by offset
static int upload_segments(sf_trainer* t) {
  std::vector<int> ends;
  std::vector<unsigned char> decay, train;
  in_offset_order(t, [&](TParam& p) { ends.push_back((int)(p.off + seg_floats(p))); decay.push_back(p.decay); train.push_back(p.trainable); });
  t->nseg = (int)ends.size();
  int rc = upload(&t->seg_end, ends, "segment table");
  if (!rc) rc = upload(&t->seg_decay, decay, "segment table");
  return rc ? rc : upload(&t->seg_train, train, "segment table");
}

// The bf16 / fp32 working arenas, carved like the workspace (SfCarver): null bases count, real bases assign.  Weights round to 128 elements, vectors to 64 floats.
struct ArenaCarver {
  bf16_t* b; float* f;
  size_t nb = 0, nf = 0;
  bf16_t* take_b(size_t n) { bf16_t* p = b ? b + nb : nullptr; nb += n; return p; }
  float* take_f(size_t n) { float* p = f ? f + nf : nullptr; nf += n; return p; }
};
static ArenaCarver carve_arena(sf_trainer* t, bf16_t* b, float* f) {
  ArenaCarver a{b, f};
  const size_t D = t->D;
  for (TLin* x : t->lins) {
    const size_t n = round_up((size_t)x->Nw * x->Kw, 128);
    x->w = a.take_b(n);
    if (x->need_wT) x->wT = a.take_b(n);
    if (x->pla >= 0) {
      x->la_bf = a.take_b(round_up((size_t)kRank * x->K, 128));
      x->lbT_bf = a.take_b(round_up((size_t)kRank * x->N, 128));
    }
    const bool pad_bias = x->pgate < 0 && x->Nw != x->N && x->pb >= 0;
    if (x->pgate >= 0 || pad_bias) x->bias_scaled = a.take_f(round_up((size_t)x->Nw, 64));
  }
  t->head_q = a.take_f(D + 64);
  t->head_u = a.take_f(16 * D);                          // the head's folded key projection
  t->head_u_hi = a.take_b(16 * D);
  t->head_u_lo = a.take_b(16 * D);
  for (TLayer& l : t->layers) {                          // fused temporal projections
    l.wf = a.take_b(D * D);
    l.wfT = a.take_b(D * D);
    l.bf = a.take_f(D);
  }
  t->red_partial = a.take_f(2048);                       // reduction scratch
  return a;
}

static int build_arena(sf_trainer* t) {
  const ArenaCarver need = carve_arena(t, nullptr, nullptr);
  if (hipMalloc(&t->arena, need.nb * sizeof(bf16_t)) != hipSuccess || hipMalloc(&t->farena, need.nf * sizeof(float)) != hipSuccess)
    return sf_set_err(SF_ERR_HIP, "hipMalloc failed (working weights, %zu bytes)", need.nb * 2);
  const bool padded = t->Ip != t->I || t->Kpp != t->Kp;
  if (padded && (hipMemset(t->arena, 0, need.nb * sizeof(bf16_t)) != hipSuccess || hipMemset(t->farena, 0, need.nf * sizeof(float)) != hipSuccess))
    return sf_set_err(SF_ERR_HIP, "hipMemset failed (padded working weights)");
  carve_arena(t, t->arena, t->farena);
  // one-launch weight refresh: job table with offsets into the flat parameter buffer
  std::vector<SfPrepJob> jobs;
  int tiles = 0;
  auto push = [&](long w_off, long la, long lb, int rank, long gate, long bias, bf16_t* w_bf, bf16_t* wT_bf, float* bias_out, int N, int K,
                  int ldw, int ldt) {
    SfPrepJob j;
    j.w_off = w_off; j.la_off = la; j.lb_off = lb; j.gate_off = gate; j.bias_off = bias;
    j.w_bf = w_bf; j.wT_bf = wT_bf; j.bias_out = bias_out; j.N = N; j.K = K; j.rank = rank; j.tile0 = tiles;
    j.ldw = ldw; j.ldt = ldt;
    tiles += ((N + SF_PREP_TILE - 1) / SF_PREP_TILE) * ((K + SF_PREP_TILE - 1) / SF_PREP_TILE);
    jobs.push_back(j);
  };
  auto off = [&](int idx, size_t extra = 0) -> long { return idx < 0 ? -1 : (long)(t->params[idx].off + extra); };
  for (TLin* x : t->lins) {
    push(off(x->pw, x->pw_off), off(x->pla), off(x->plb), kRank, off(x->pgate), x->bias_scaled ? off(x->pb, x->pb_off) : -1, x->w, x->wT,
         x->bias_scaled, x->N, x->K, x->Kw, x->Nw);
    if (x->pla >= 0) {
      push(off(x->pla), -1, -1, 0, -1, -1, x->la_bf, nullptr, nullptr, kRank, x->K, x->K, kRank);
      push(off(x->plb), -1, -1, 0, -1, -1, nullptr, x->lbT_bf, nullptr, x->N, kRank, kRank, x->N);
    }
  }
  t->n_prep_jobs = (int)jobs.size(); t->prep_tiles = tiles;
  std::vector<SfFuseJob> fj;
  for (TLayer& l : t->layers) {
    SfFuseJob j;
    j.wd = l.t_dense.w; j.woT = l.t_out.wT; j.wf = l.wf; j.wfT = l.wfT; j.bf = l.bf;
    j.wd_off = off(l.t_dense.pw); j.bo_off = off(l.t_out.pb); j.bd_off = off(l.t_dense.pb); j.gate_off = off(l.gate);
    fj.push_back(j);
  }
  const int rc = upload(&t->prep_jobs, jobs, "prep table");
  return rc ? rc : upload(&t->fuse_jobs, fj, "fuse table");
}

extern "C" int sf_trainer_create(const sf_config* cfg, int device, int freeze_spatial, int n_extra, sf_trainer** out) {
  if (!cfg || !out) return sf_set_err(SF_ERR_INVALID, "sf_trainer_create: null argument");
  const sf_config& c = *cfg;
  int rc = check_config(c, n_extra);
  if (rc) return rc;
  if (hipSetDevice(device) != hipSuccess) return sf_set_err(SF_ERR_HIP, "hipSetDevice(%d) failed", device);
  sf_trainer* t = new sf_trainer();
  t->cfg = c; t->device = device;
  t->D = c.hidden_size; t->I = c.intermediate_size; t->L = c.num_hidden_layers; t->heads = c.num_attention_heads;
  t->C = c.num_channels; t->P = c.patch_size;
  t->N = (c.image_size / c.patch_size) * (c.image_size / c.patch_size);
  t->Kp = t->C * t->P * t->P;
  t->hd = t->D / t->heads;
  t->scale = 1.0f / sqrtf((float)t->hd);          // 0.125 exactly at head_dim 64
  t->Ip = (t->I + 63) / 64 * 64;
  t->Kpp = (t->Kp + 63) / 64 * 64;
  t->lora = c.add_lora_spatial != 0;
  t->freeze = freeze_spatial != 0;
  t->n_extra = n_extra;
  declare_params(t);
  rc = assign_offsets(t);
  if (!rc) rc = upload_segments(t);
  if (!rc) rc = build_arena(t);
  if (rc) { sf_trainer_destroy(t); return rc; }       // the one failure exit: whatever was allocated so far goes with the handle
  *out = t;
  return SF_OK;
}

extern "C" void sf_trainer_destroy(sf_trainer* t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  for (void* p : {(void*)t->seg_end, (void*)t->seg_decay, (void*)t->seg_train, (void*)t->arena, (void*)t->farena, (void*)t->prep_jobs,
                  (void*)t->fuse_jobs, (void*)t->guard_sumsq})
    if (p) (void)hipFree(p);
  t->side.destroy();
  delete t;
}

extern "C" int sf_trainer_num_params(const sf_trainer* t) { return t ? (int)t->params.size() : 0; }

extern "C" int sf_trainer_param_info(const sf_trainer* t, int index, char* name_out, int name_cap, int64_t* offset_out,
                                     int64_t* numel_out, int64_t* shape_out, int* ndim_out, int* trainable_out,
                                     int* decay_out) {
  if (!t || index < 0 || index >= (int)t->params.size()) return sf_set_err(SF_ERR_INVALID, "param index out of range");
  const TParam& p = t->params[index];
  if (name_out && name_cap > 0) snprintf(name_out, (size_t)name_cap, "%s", p.name.c_str());
  if (offset_out) *offset_out = (int64_t)p.off;
  if (numel_out) *numel_out = (int64_t)p.numel;
  if (shape_out) for (int i = 0; i < 4; ++i) shape_out[i] = p.shape[i];
  if (ndim_out) *ndim_out = p.ndim;
  if (trainable_out) *trainable_out = p.trainable;
  if (decay_out) *decay_out = p.decay;
  return SF_OK;
}

extern "C" int sf_trainer_total_floats(const sf_trainer* t, int64_t* total_out, int64_t* trainable_out) {
  if (!t) return sf_set_err(SF_ERR_INVALID, "null handle");
  if (total_out) *total_out = (int64_t)t->total;
  if (trainable_out) *trainable_out = (int64_t)t->n_train;
  return SF_OK;
}

extern "C" int sf_trainer_num_stages(const sf_trainer* t) { return t ? t->L + 2 : 0; }

extern "C" int sf_trainer_stage_range(const sf_trainer* t, int stage, int64_t* offset_out, int64_t* numel_out) {
  if (!t || stage < 0 || stage > t->L + 1) return sf_set_err(SF_ERR_INVALID, "stage out of range");
  size_t a, b;
  if (stage == 0) { a = t->tail_off; b = t->tail_end; }
  else if (stage == t->L + 1) { a = t->emb_off; b = t->emb_end; }
  else { const TLayer& l = t->layers[t->L - stage]; a = l.seg_off; b = l.seg_end; }
  if (offset_out) *offset_out = (int64_t)a;
  if (numel_out) *numel_out = (int64_t)(b - a);
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// working weights
// ------------------------------------------------------------------------------------------------
static inline const float* PP(const sf_trainer* t, const float* base, int idx, size_t extra = 0) {
  return idx < 0 ? nullptr : base + t->params[idx].off + extra;
}
static inline float* GG(const sf_trainer* t, float* grads, int idx, size_t extra = 0) {
  return (idx < 0 || !t->params[idx].trainable) ? nullptr : grads + t->params[idx].off + extra;
}
static inline const float* lin_bias(const sf_trainer* t, const TLin& l) {
  return l.bias_scaled ? l.bias_scaled : PP(t, t->params_dev, l.pb, l.pb_off);
}

extern "C" int sf_trainer_sync_weights(sf_trainer* t, const float* params_dev, sf_stream stream) {
  if (!t || !params_dev) return sf_set_err(SF_ERR_INVALID, "null argument");
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(t->device));
  t->params_dev = params_dev;
  HIP_TRY(sf_launch_prep_weights_batched(params_dev, t->prep_jobs, t->n_prep_jobs, t->prep_tiles, s));
  // nn.MultiheadAttention scales q by head_dim^-0.5 after the in-projection (modeling:1145-1149)
  HIP_TRY(sf_launch_head_query(PP(t, params_dev, t->p_probe), PP(t, params_dev, t->p_inw), PP(t, params_dev, t->p_inb), t->scale,
                               t->head_q, t->D, s));
  // the temporal branch's two projections as one (used by forwards without drop_path / hidden dropout): from the fresh bf16 copies
  HIP_TRY(sf_launch_fuse_temporal(params_dev, t->fuse_jobs, t->L, t->D, s));
  // the keys of the pooling head only meet that one query: U_h = Wk_h^T q_h (sf_pool_head.hip)
  if (t->hd == 64)
    HIP_TRY(sf_launch_pool_u(PP(t, params_dev, t->p_inw, (size_t)t->D * t->D), t->head_q, t->head_u, t->head_u_hi, t->head_u_lo, t->heads, t->D, s));
  else
    HIP_TRY(sf_launch_pool_u_generic(PP(t, params_dev, t->p_inw, (size_t)t->D * t->D), t->head_q, t->head_u, t->heads, t->hd, t->D, s));
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------------
struct TSavedLayer {
  float *h1, *h2;
  bf16_t *ln_t, *tqkv, *ctx_t, *t_out, *ln_b, *sqkv, *ctx_s, *ln_a, *pre, *act;
  float* lse_s;      // spatial attention log-sum-exp [F, heads, N] (head_dim 64; the generic backward recomputes it)
};
struct TWs {
  // saved by the forward
  bf16_t* patches; float* te_rows;
  std::vector<float*> h;               // L+1 residual snapshots
  std::vector<TSavedLayer> sl;
  bf16_t *xn, *pc, *hn, *hm_pre, *hm;
  float* attn_out;
  float *pz, *pprobs, *pml, *pzpart;   // pooling head: z_h = sum_n p_hn x_n [F, heads, D], the raw scores [F, heads, N], {max, sum} and partial sums per token split
  // backward scratch
  bf16_t* d_ln_bf;
  float *g, *d_ln, *wg_partial, *dw_scratch, *cs, *ln_partial, *cs_partial, *s_tn;
  bf16_t *g_bf, *d_wide, *d_ctx, *d_tout, *lora_u, *lora_v;
  float *wg_partial_side, *cs_partial_side;          // the side stream's own scratch (LoRA gradients, see sf_trainer::side)
  float* dw_scratch2; bf16_t* g1_bf;                 // fused temporal projections: g^T t_out [D, D] fp32 and bf16(g^T ctx) [D, D]
  float *g1_alt, *cs_alt;                            // second G1 / cs buffers: layers alternate, the side stream reads one layer behind
  bf16_t *lora_u_side, *lora_v_side;
  bf16_t *g_bf1, *g_bf2, *d_wide_s, *d_wide_t;       // a layer's weight-gradient operands stay intact until its grouped launch
  float *gh, *d_hn, *d_pc, *dq_total, *pdz, *pdu;
  bf16_t* pds;                         // pooling head: score gradients [M, 32] (the dY operand of dU = ds^T x)
  bf16_t *gh_bf, *d_hm;
  float *pgen, *pgstat;                // generic-width pooling head: raw scores [F, heads, N] + z [F, heads, D]; backward statistics [F, heads, 4]
  size_t bytes;
};

static size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

static TWs tcarve(const sf_trainer* t, void* base, int B, int T) {
  TWs w;
  SfCarver c(base);
  const size_t D = t->D, I = t->Ip, N = t->N;     // activations carry the padded intermediate width
  const size_t M = (size_t)B * T * N, F = (size_t)B * T;
  w.patches = c.take<bf16_t>(M * t->Kpp);
  w.te_rows = c.take<float>((size_t)T * D);
  w.h.resize(t->L + 1);
  w.sl.resize(t->L);
  for (int i = 0; i <= t->L; ++i) w.h[i] = c.take<float>(M * D);
  for (int i = 0; i < t->L; ++i) {
    TSavedLayer& s = w.sl[i];
    s.h1 = c.take<float>(M * D); s.h2 = c.take<float>(M * D);
    s.ln_t = c.take<bf16_t>(M * D); s.tqkv = c.take<bf16_t>(M * 3 * D); s.ctx_t = c.take<bf16_t>(M * D);
    s.t_out = c.take<bf16_t>(M * D);
    s.ln_b = c.take<bf16_t>(M * D); s.sqkv = c.take<bf16_t>(M * 3 * D); s.ctx_s = c.take<bf16_t>(M * D);
    s.ln_a = c.take<bf16_t>(M * D); s.pre = c.take<bf16_t>(M * I); s.act = c.take<bf16_t>(M * I);
    s.lse_s = c.take<float>(F * (size_t)t->heads * N);
  }
  w.xn = c.take<bf16_t>(M * D); w.pc = c.take<bf16_t>(F * D);
  w.pz = c.take<float>(F * (size_t)t->heads * D); w.pprobs = c.take<float>(F * (size_t)t->heads * N);
  w.pml = c.take<float>(sf_pool_ml_floats((int)F, (int)N, t->heads));
  w.pzpart = c.take<float>(sf_pool_z_floats((int)F, (int)N, t->heads, (int)D));
  w.attn_out = c.take<float>(F * D); w.hn = c.take<bf16_t>(F * D);
  w.hm_pre = c.take<bf16_t>(F * I); w.hm = c.take<bf16_t>(F * I);
  // scratch
  w.g = c.take<float>(M * D); w.d_ln = c.take<float>(M * D);
  w.d_ln_bf = reinterpret_cast<bf16_t*>(w.d_ln);          // per-layer LayerNorm input gradients travel as bf16
  w.g_bf = c.take<bf16_t>(M * D);
  w.d_wide = c.take<bf16_t>(M * max_sz(I, 3 * D));
  w.d_ctx = c.take<bf16_t>(M * D); w.d_tout = c.take<bf16_t>(M * D);
  w.g_bf1 = c.take<bf16_t>(M * D); w.g_bf2 = c.take<bf16_t>(M * D);
  w.d_wide_s = c.take<bf16_t>(M * 3 * D); w.d_wide_t = c.take<bf16_t>(M * 3 * D);
  w.lora_u = c.take<bf16_t>(M * kRank); w.lora_v = c.take<bf16_t>(M * kRank);
  w.lora_u_side = c.take<bf16_t>(M * kRank); w.lora_v_side = c.take<bf16_t>(M * kRank);
  // wg_partial serves every weight-gradient launch of the caller's stream: the largest request over the trainer's own Linears at
  // the rows they run with (the layers all have the first one's shapes), the rank-32 LoRA / pooling-head products, and one
  // layer's Linears in one grouped launch
  const int Mi = (int)M, Fi = (int)F, Di = t->D;
  const size_t nlin = t->lins.size() < (size_t)(kHeadLins + kLayerLins) ? t->lins.size() : (size_t)(kHeadLins + kLayerLins);
  size_t wp = 0;
  int tiles = 0, n1 = 0;
  for (size_t i = 0; i < nlin; ++i) {
    const TLin& x = *t->lins[i];
    wp = max_sz(wp, sf_wgrad_partial_floats(x.per_frame ? Fi : Mi, x.N, x.K));
    if (i >= (size_t)kHeadLins && sf_wgrad_groupable(Mi, x.N, x.K)) { tiles += (x.N / 256) * (x.K / 256); n1 += x.N; }
  }
  for (int n = 1; n <= tiles; ++n) wp = max_sz(wp, sf_wgrad_group_partial_floats(Mi, n, n1));
  wp = max_sz(wp, sf_wgrad_partial_floats(Mi, 3 * Di, kRank)); wp = max_sz(wp, sf_wgrad_partial_floats(Mi, kRank, Di));
  // never launched (weight gradients keep the unpadded N x K), kept because the byte count would change without it: at widths that
  // do not group (so400m: 1152 x 4352) the padded MLP shape is the largest single request
  if (t->Ip != t->I) { wp = max_sz(wp, sf_wgrad_partial_floats(Mi, Di, t->Ip)); wp = max_sz(wp, sf_wgrad_partial_floats(Mi, t->Ip, Di)); }
  w.wg_partial = c.take<float>(wp);
  {
    size_t ws2 = 0;
    ws2 = max_sz(ws2, sf_wgrad_partial_floats(Mi, 3 * Di, kRank)); ws2 = max_sz(ws2, sf_wgrad_partial_floats(Mi, kRank, Di));
    ws2 = max_sz(ws2, sf_wgrad_partial_floats(Mi, Di, kRank));
    ws2 = max_sz(ws2, sf_wgrad_partial_floats(Di, Di, Di));      // temporal_fused_grads on the side stream: dW_o = (tanh(g) W_d)^T G1, M = D
    w.wg_partial_side = c.take<float>(ws2);
  }
  w.dw_scratch = c.take<float>((size_t)3 * D * D);
  w.dw_scratch2 = c.take<float>((size_t)D * D); w.g1_bf = c.take<bf16_t>((size_t)D * D);
  w.g1_alt = c.take<float>((size_t)D * D); w.cs_alt = c.take<float>(max_sz(I, 3 * D));
  w.cs = c.take<float>(max_sz(I, 3 * D));
  w.ln_partial = c.take<float>(sf_ln_bwd_partial_floats(t->D));
  w.cs_partial = c.take<float>(sf_colsum_partial_floats((int)max_sz(I, 3 * D)));
  w.cs_partial_side = c.take<float>(sf_colsum_partial_floats((int)max_sz(I, 3 * D)));
  w.s_tn = c.take<float>((size_t)T * N * D);
  w.gh = c.take<float>(F * D); w.d_hn = c.take<float>(F * D); w.d_pc = c.take<float>(F * D);
  w.dq_total = c.take<float>(D);
  w.pdz = c.take<float>(F * (size_t)t->heads * D); w.pdu = c.take<float>((size_t)32 * D); w.pds = c.take<bf16_t>(M * 32);
  w.gh_bf = c.take<bf16_t>(F * D); w.d_hm = c.take<bf16_t>(F * I);
  w.pgen = w.pgstat = nullptr;
  if (t->hd != 64) {
    w.pgen = c.take<float>(sf_pool_generic_scratch_floats((int)F, (int)N, t->heads, (int)D));
    w.pgstat = c.take<float>(F * (size_t)t->heads * 4);
  }
  w.bytes = (c.off + 255) & ~(size_t)255;
  return w;
}

static int check_bt(const sf_trainer* t, int B, int T) {
  if (!t) return sf_set_err(SF_ERR_INVALID, "null handle");
  if (B <= 0 || T <= 0) return sf_set_err(SF_ERR_INVALID, "bad geometry B=%d T=%d", B, T);
  if (T > t->cfg.num_frames) return sf_set_err(SF_ERR_INVALID, "training needs T <= config.num_frames (%d > %d)", T, t->cfg.num_frames);
  if (T > 32) return sf_set_err(SF_ERR_INVALID, "temporal attention backward handles T <= 32 (got %d)", T);
  if ((size_t)B * T * t->N * (size_t)(t->Ip > 3 * t->D ? t->Ip : 3 * t->D) * 2 >= ((size_t)1 << 32))
    return sf_set_err(SF_ERR_INVALID, "batch too large for 32-bit buffer offsets");
  return SF_OK;
}

extern "C" int sf_trainer_workspace_bytes(const sf_trainer* t, int B, int T, size_t* out) {
  int rc = check_bt(t, B, T);
  if (rc) return rc;
  if (!out) return sf_set_err(SF_ERR_INVALID, "null out");
  *out = tcarve(t, nullptr, B, T).bytes;
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// GEMM helpers
// ------------------------------------------------------------------------------------------------
static hipError_t tgemm(const bf16_t* a, const bf16_t* w, const float* bias, int M, int N, int K, int epi, hipStream_t s,
                        float* out_f32, bf16_t* out_bf, const float* resid = nullptr) {
  return sf_launch_gemm(sf_train_gemm_args(a, w, bias, M, N, K, epi, out_f32, out_bf, resid), false, s);
}
// y = x W^T + b
static hipError_t lin_fwd(const sf_trainer* t, const TLin& l, const bf16_t* x, int M, int epi, hipStream_t s, float* out_f32,
                          bf16_t* out_bf, const float* resid = nullptr) {
  return tgemm(x, l.w, lin_bias(t, l), M, l.Nw, l.Kw, epi, s, out_f32, out_bf, resid);
}
// dx = dy W   (dy [M,N] -> dx [M,K]); the forward-scaled weight is used as is
static hipError_t lin_dgrad(const TLin& l, const bf16_t* dy, int M, hipStream_t s, float* out_f32, bf16_t* out_bf) {
  return tgemm(dy, l.wT, nullptr, M, l.Kw, l.Nw, out_f32 ? SF_EPI_F32 : SF_EPI_BF16, s, out_f32, out_bf);
}
// pre = x W^T + b and act = gelu(pre): one launch where the 256^2 kernel takes the shape, else GEMM + GELU pass
static hipError_t lin_fwd_gelu(const sf_trainer* t, const TLin& l, const bf16_t* x, int M, hipStream_t s, bf16_t* pre, bf16_t* act) {
  SfGemmArgs g = sf_train_gemm_args(x, l.w, lin_bias(t, l), M, l.Nw, l.Kw, SF_EPI_BF16, nullptr, pre, nullptr);
  g.aux_mode = 1; g.aux = act;
  if (sf_gemm256_aux_supported(g)) return sf_launch_gemm(g, false, s);
  g.aux_mode = 0; g.aux = nullptr;
  hipError_t e = sf_launch_gemm(g, false, s);
  return e != hipSuccess ? e : sf_launch_gelu_fwd(pre, act, (size_t)M * l.Nw, s);
}
// d_pre = (dy W) * gelu'(pre): same
static hipError_t lin_dgrad_dgelu(const TLin& l, const bf16_t* dy, int M, hipStream_t s, bf16_t* d_pre, bf16_t* pre) {
  SfGemmArgs g = sf_train_gemm_args(dy, l.wT, nullptr, M, l.Kw, l.Nw, SF_EPI_BF16, nullptr, d_pre, nullptr);
  g.aux_mode = 2; g.aux = pre;                // read only in this mode (the field is the forward's output pointer)
  if (sf_gemm256_aux_supported(g)) return sf_launch_gemm(g, false, s);
  g.aux_mode = 0; g.aux = nullptr;
  hipError_t e = sf_launch_gemm(g, false, s);
  return e != hipSuccess ? e : sf_launch_gelu_bwd(d_pre, pre, (size_t)M * l.Kw, s);
}

// the step's context: one forward or one backward call on one stream
struct StepCtx {
  sf_trainer* t;
  const TWs* ws;
  const StepPlan* p;
  hipStream_t s;
  float* grads = nullptr;             // backward only
  SfWgradGroup* group = nullptr;      // the layer's grouped weight-gradient launch; nullptr: every job launches where it is submitted
  bool on_side = false;               // this context launches on the side stream and uses the side scratch
  bf16_t* lora_u() const { return on_side ? ws->lora_u_side : ws->lora_u; }
  bf16_t* lora_v() const { return on_side ? ws->lora_v_side : ws->lora_v; }
  float* wg_partial() const { return on_side ? ws->wg_partial_side : ws->wg_partial; }
  float* cs_partial() const { return on_side ? ws->cs_partial_side : ws->cs_partial; }
  StepCtx on_side_stream() const { StepCtx c = *this; c.s = t->side.stream; c.on_side = true; c.group = nullptr; return c; }
  // a Linear whose [N1, N2] is made of 256^2 tiles can wait for the layer's grouped launch
  bool can_queue(int M, int N1, int N2) const { return group && sf_wgrad_groupable(M, N1, N2) && group->njobs < SF_WG_MAX_JOBS; }
};

// ------------------------------------------------------------------------------------------------
// forward (activations kept)
// ------------------------------------------------------------------------------------------------
static int tforward_embeddings(const StepCtx& c, const void* pixels, int pixel_dtype) {
  const sf_trainer* t = c.t;
  const TWs& ws = *c.ws;
  const StepPlan& p = *c.p;
  const sf_config& cf = t->cfg;
  hipStream_t s = c.s;
  const int D = t->D;
  const float* P0 = t->params_dev;
  SfRowIndex idx;
  idx.n = p.T;
  for (int i = 0; i < p.T; ++i) idx.idx[i] = i;             // modeling:436-439 (T <= num_frames)
  HIP_TRY(sf_launch_gather_rows(PP(t, P0, t->p_time), ws.te_rows, idx, D, s));
  HIP_TRY(sf_launch_patchify(pixels, pixel_dtype == SF_U8 ? 2 : (pixel_dtype == SF_BF16 ? 1 : 0), ws.patches, nullptr, p.F, cf.num_channels, cf.image_size, cf.image_size,
                             cf.patch_size, s, nullptr, nullptr, nullptr, nullptr, t->Kpp));
  SfGemmArgs g;
  memset(&g, 0, sizeof(g));
  g.a_hi = ws.patches; g.w_hi = t->patch.w; g.bias = PP(t, P0, t->patch.pb);
  g.M = p.M; g.N = D; g.K = t->Kpp; g.epi = SF_EPI_EMBED_F32;
  g.pos = PP(t, P0, t->p_pos); g.time_rows = ws.te_rows; g.Np = p.N; g.Tn = p.T;
  g.out_f32 = ws.h[0]; g.ldc = D;
  if (p.drop_hidden > 0.f) {
    // pos_drop(patches + pos) then time_drop(. + time) (modeling:374, 378): the GEMM adds a zero time table, one elementwise pass does the rest
    HIP_TRY(hipMemsetAsync(ws.g, 0, (size_t)p.T * D * sizeof(float), s));
    g.time_rows = ws.g;
    HIP_TRY(sf_launch_gemm(g, false, s));
    HIP_TRY(sf_launch_embed_dropout(ws.h[0], ws.te_rows, p.M, D, p.T, p.N, p.embed_site(SITE_EMBED_POS), p.embed_site(SITE_EMBED_TIME), s));
  } else {
    HIP_TRY(sf_launch_gemm(g, false, s));
  }
  return SF_OK;
}

// the arguments of a training attention call over a layer's saved qkv rows: temporal (sequences of T frames per patch) or spatial
static SfAttnArgs tattn_args(const StepCtx& c, int li, bool temporal, const bf16_t* qkv, bf16_t* ctx, float* lse_s) {
  const sf_trainer* t = c.t;
  const StepPlan& p = *c.p;
  const int D = t->D;
  SfAttnArgs a;
  memset(&a, 0, sizeof(a));
  a.q = qkv; a.k = qkv + D; a.v = qkv + 2 * D;
  a.row_pitch_q = 3 * D; a.row_pitch_kv = 3 * D; a.heads = t->heads; a.scale = t->scale;
  a.N = p.N; a.ctx_hi = ctx; a.D = D; a.head_dim = t->hd;
  if (temporal) {
    a.B = p.B; a.Tq = p.T; a.Tk = p.T; a.Tcap = p.T; a.t_past = 0; a.causal = t->cfg.enable_causal_temporal;
    a.Tq_cap = p.T; a.q_t0 = 0;
  } else {
    a.frames = p.F;
    if (t->hd == 64) a.lse2_out = lse_s;      // the generic backward recomputes the row statistics
  }
  if (p.drop_attn > 0.f) a.drop = p.attn_site(li, temporal ? SITE_TEMPORAL_PROBS : SITE_SPATIAL_PROBS);
  return a;
}

// out = resid + branch(x): the GEMM's residual epilogue, or with row factors (drop_path / dropout, modeling:752 / 761, 835, 980, 1000) an fp32 branch and a scaled add
static hipError_t branch_add(const StepCtx& c, const TLin& l, const bf16_t* x, const float* resid, float* out, const float* dp, int mode, SfDrop drop) {
  const StepPlan& p = *c.p;
  if (!p.scaled()) return lin_fwd(c.t, l, x, p.M, SF_EPI_RESID_F32, c.s, out, nullptr, resid);
  hipError_t e = lin_fwd(c.t, l, x, p.M, SF_EPI_F32, c.s, c.ws->g, nullptr);
  return e != hipSuccess ? e : sf_launch_resid_rowscale(out, resid, c.ws->g, dp, p.M, c.t->D, mode, p.T, p.N, c.s, drop);
}

static int tforward_layer(const StepCtx& c, int li) {
  const sf_trainer* t = c.t;
  const TWs& ws = *c.ws;
  const StepPlan& p = *c.p;
  hipStream_t s = c.s;
  const TLayer& l = t->layers[li];
  const TSavedLayer& sv = ws.sl[li];
  const int D = t->D, N = p.N, T = p.T, M = p.M;
  const float eps = t->cfg.layer_norm_eps;
  const float* P0 = t->params_dev;
  const float* h = ws.h[li];
  const bool hd = p.drop_hidden > 0.f;
  // temporal attention (modeling:937-958)
  HIP_TRY(sf_launch_layernorm(h, PP(t, P0, l.ln_t_g), PP(t, P0, l.ln_t_b), nullptr, sv.ln_t, nullptr, M, D, eps, s));
  HIP_TRY(lin_fwd(t, l.t_qkv, sv.ln_t, M, SF_EPI_BF16, s, nullptr, sv.tqkv));
  HIP_TRY(sf_launch_temporal_attention(tattn_args(c, li, true, sv.tqkv, sv.ctx_t, nullptr), false, s));
  if (p.tfuse) {
    // h1 = h + ctx W_f^T + b_f: output.dense and temporal_dense (modeling:947-958) have nothing between them at drop rates 0
    HIP_TRY(tgemm(sv.ctx_t, l.wf, l.bf, M, D, D, SF_EPI_RESID_F32, s, sv.h1, nullptr, h));
  } else {
    HIP_TRY(lin_fwd(t, l.t_out, sv.ctx_t, M, SF_EPI_BF16, s, nullptr, sv.t_out));
    // drop_path (modeling:949) sits between the attention output and temporal_dense: the saved t_out IS the dropped tensor
    // hidden dropout of the temporal SelfOutput (modeling:761) rides on the same pass
    if (p.scaled()) HIP_TRY(sf_launch_rowscale_bf16(sv.t_out, sv.t_out, p.dp_temporal(li), M, D, 0, T, N, s, p.hidden_site(li, SITE_TEMPORAL_OUT)));
    HIP_TRY(lin_fwd(t, l.t_dense, sv.t_out, M, SF_EPI_RESID_F32, s, sv.h1, nullptr, h));      // h1 = h + tanh(g) * dense(.)
  }
  // spatial attention (modeling:962-996)
  HIP_TRY(sf_launch_layernorm(sv.h1, PP(t, P0, l.ln_b_g), PP(t, P0, l.ln_b_b), nullptr, sv.ln_b, nullptr, M, D, eps, s));
  HIP_TRY(lin_fwd(t, l.s_qkv, sv.ln_b, M, SF_EPI_BF16, s, nullptr, sv.sqkv));
  HIP_TRY(sf_launch_spatial_attention(tattn_args(c, li, false, sv.sqkv, sv.ctx_s, sv.lse_s), false, s));
  HIP_TRY(branch_add(c, l.s_out, sv.ctx_s, sv.h1, sv.h2, p.dp_spatial(li), 1, p.hidden_site(li, SITE_SPATIAL_OUT)));      // h2 = h1 + out(ctx)
  // MLP (modeling:997-1000)
  HIP_TRY(sf_launch_layernorm(sv.h2, PP(t, P0, l.ln_a_g), PP(t, P0, l.ln_a_b), nullptr, sv.ln_a, nullptr, M, D, eps, s));
  HIP_TRY(lin_fwd_gelu(t, l.up, sv.ln_a, M, s, sv.pre, sv.act));
  if (hd) HIP_TRY(sf_launch_rowscale_bf16(sv.act, sv.act, nullptr, M, t->Ip, 0, T, N, s, p.hidden_site(li, SITE_MLP_ACT)));      // dropout behind the activation (modeling:822): the saved act IS the dropped tensor
  HIP_TRY(branch_add(c, l.down, sv.act, sv.h2, ws.h[li + 1], p.dp_mlp(li), 2, p.hidden_site(li, SITE_MLP_OUT)));              // out = h2 + mlp
  return SF_OK;
}

// post LayerNorm + pooling head (modeling:1330-1340, 1141-1154)
// The probe attention reads the fp32 tokens and never projects them to k / v (sf_pool_head.hip): scores = x . U, z_h = sum_n p_hn x_n,
// ctx_h = Wv_h z_h + bv_h.  The caller's last_hidden_state (or, without one, the backward's scratch) holds the fp32 rows; the
// backward itself works from the bf16 copy ws.xn, so the caller may do with its tensor what it likes.
static int tforward_head(const StepCtx& c, float* last_hidden, float* pooler) {
  const sf_trainer* t = c.t;
  const TWs& ws = *c.ws;
  hipStream_t s = c.s;
  const int D = t->D, N = c.p->N, heads = t->heads, M = c.p->M, F = c.p->F;
  const float eps = t->cfg.layer_norm_eps;
  const float* P0 = t->params_dev;
  float* xf = last_hidden ? last_hidden : ws.g;
  HIP_TRY(sf_launch_layernorm(ws.h[t->L], PP(t, P0, t->post_g), PP(t, P0, t->post_b), xf, ws.xn, nullptr, M, D, eps, s));
  if (t->hd != 64) {
    // generic widths: raw scores and z stay in ws.pgen for the backward (sf_pool_generic_bwd.hip)
    SfPoolGenArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.x = xf; ga.u = t->head_u; ga.wv = PP(t, P0, t->p_inw, (size_t)2 * D * D); ga.ldw = D; ga.bv = PP(t, P0, t->p_inb, (size_t)2 * D);
    ga.ctx_hi = ws.pc; ga.scratch = ws.pgen; ga.F = F; ga.N = N; ga.heads = heads; ga.hd = t->hd; ga.D = D;
    HIP_TRY(sf_launch_pool_generic(ga, s));
  } else {
    SfPoolArgs pa;
    memset(&pa, 0, sizeof(pa));
    // token splits as in inference (a frame's tokens over S workgroups): the raw scores and {max, sum} per split are kept, the backward
    // finishes the softmax itself; the combined, normalised sums z land in ws.pz (directly when S == 1)
    const int S = sf_pool_splits(F, N, heads);
    pa.x = xf; pa.u_hi = t->head_u_hi; pa.u_lo = t->head_u_lo; pa.zpart = S == 1 ? ws.pz : ws.pzpart; pa.probs = ws.pprobs; pa.probs_raw = 1; pa.ml = ws.pml;
    pa.F = F; pa.N = N; pa.heads = heads; pa.D = D; pa.S = S; pa.normalize = S == 1;
    HIP_TRY(sf_launch_pool_probe(pa, s));
    SfPoolCtxArgs ca;
    memset(&ca, 0, sizeof(ca));
    ca.zpart = pa.zpart; ca.ml = ws.pml; ca.z_out = S == 1 ? nullptr : ws.pz;
    ca.wv = PP(t, P0, t->p_inw, (size_t)2 * D * D); ca.ldw = D; ca.bv = PP(t, P0, t->p_inb, (size_t)2 * D);
    ca.ctx_hi = ws.pc; ca.F = F; ca.heads = heads; ca.D = D; ca.S = S;
    HIP_TRY(sf_launch_pool_ctx(ca, s));
  }
  HIP_TRY(lin_fwd(t, t->head_out, ws.pc, F, SF_EPI_F32, s, ws.attn_out, nullptr));
  HIP_TRY(sf_launch_layernorm(ws.attn_out, PP(t, P0, t->hln_g), PP(t, P0, t->hln_b), nullptr, ws.hn, nullptr, F, D, eps, s));
  HIP_TRY(lin_fwd(t, t->fc1, ws.hn, F, SF_EPI_BF16, s, nullptr, ws.hm_pre));
  HIP_TRY(sf_launch_gelu_fwd(ws.hm_pre, ws.hm, (size_t)F * t->Ip, s));
  HIP_TRY(lin_fwd(t, t->fc2, ws.hm, F, SF_EPI_RESID_F32, s, pooler, nullptr, ws.attn_out));
  return SF_OK;
}

extern "C" int sf_trainer_forward(sf_trainer* t, const void* pixels, int pixel_dtype, int B, int T, float* last_hidden,
                                  float* pooler, void* workspace, size_t workspace_bytes, sf_stream stream) {
  int rc = check_bt(t, B, T);
  if (rc) return rc;
  if (!t->params_dev) return sf_set_err(SF_ERR_STATE, "sf_trainer_sync_weights has not been called");
  if (!pixels || !workspace || !pooler) return sf_set_err(SF_ERR_INVALID, "null argument");
  if (pixel_dtype != SF_F32 && pixel_dtype != SF_BF16 && pixel_dtype != SF_U8)
    return sf_set_err(SF_ERR_INVALID, "pixels must be fp32, bf16 or uint8 (uint8: (x/255 - 0.5)/0.5 fused)");
  HIP_TRY(hipSetDevice(t->device));
  const TWs ws = tcarve(t, workspace, B, T);
  if (workspace_bytes < ws.bytes) return sf_set_err(SF_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, ws.bytes);
  t->plan.valid = false;
  if (t->drop_attn > 0.f && (T > 16 || t->N > 224)) return sf_set_err(SF_ERR_INVALID, "attention dropout needs clips of <= 16 frames and <= 224 patches per frame");
  if (t->drop_attn > 0.f && t->hd != 64) return sf_set_err(SF_ERR_INVALID, "attention dropout needs head_dim 64 (got %d)", t->hd);
  if (t->dp_scales && (t->dp_B != B || t->dp_T != T))
    return sf_set_err(SF_ERR_INVALID, "drop_path factors were set for B=%d T=%d, the forward runs B=%d T=%d", t->dp_B, t->dp_T, B, T);
  StepPlan p;
  p.B = B; p.T = T; p.N = t->N; p.L = t->L; p.M = B * T * t->N; p.F = B * T;
  p.dp = t->dp_scales;
  p.drop_hidden = t->drop_hidden; p.drop_attn = t->drop_attn; p.seed = t->drop_seed;
  // the temporal branch's two projections as one: only without drop_path / hidden dropout (both sit between them);
  // SF_TRAIN_UNFUSED_TEMPORAL keeps the two launches (A/B, and the path the drop rates use)
  p.tfuse = !p.scaled() && sf_sw(SW_TRAIN_UNFUSED_TEMPORAL) == nullptr;
  const StepCtx c{t, &ws, &p, (hipStream_t)stream};
  if ((rc = tforward_embeddings(c, pixels, pixel_dtype)) != SF_OK) return rc;
  for (int li = 0; li < t->L; ++li)
    if ((rc = tforward_layer(c, li)) != SF_OK) return rc;
  if ((rc = tforward_head(c, last_hidden, pooler)) != SF_OK) return rc;
  p.valid = true;
  t->plan = p;
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
// One weight-gradient job, out (+)= dy^T x over M token rows (+ dbias += colsum dy), and the three routes it can take.  A Linear's operands
// carry the working (padded) pitches, its gradient keeps N x K.
static SfWgradJob wgrad_job(const bf16_t* dy, int ldy, const bf16_t* x, int ldx, int N1, int N2, float* out, float* dbias, int accumulate) {
  SfWgradJob j;
  memset(&j, 0, sizeof(j));
  j.dy = dy; j.x = x; j.out = out; j.dbias = dbias; j.ldy = ldy; j.ldx = ldx; j.N1 = N1; j.N2 = N2; j.ldo = N2; j.alpha = 1.f; j.accumulate = accumulate;
  return j;
}
static SfWgradJob lin_job(const TLin& l, const bf16_t* dy, const bf16_t* x, float* gw, float* gb) { return wgrad_job(dy, l.Nw, x, l.Kw, l.N, l.K, gw, gb, 1); }
// the temporal branch's token-contracting product G = g^T x [D, D] and cs = colsum g, written (not accumulated) into scratch
static SfWgradJob temporal_job(const bf16_t* g, const bf16_t* x, int D, float* G, float* cs) { return wgrad_job(g, D, x, D, D, D, G, cs, 0); }
// the layer's group (StepCtx::can_queue) / the grouped kernel at once, as a group of one / sf_launch_wgrad at once (bias_scratch: with the column-sum scratch)
enum WgRoute { WG_QUEUE, WG_LONE_GROUP, WG_DIRECT };
static hipError_t submit(const StepCtx& c, const SfWgradJob& j, int M, WgRoute route, bool bias_scratch) {
  if (route == WG_QUEUE) { c.group->job[c.group->njobs++] = j; return hipSuccess; }
  if (route == WG_LONE_GROUP) {
    SfWgradGroup g;
    memset(&g, 0, sizeof(g));
    g.njobs = 1; g.M = M; g.partial = c.wg_partial(); g.job[0] = j;
    return sf_launch_wgrad_group(g, c.s);
  }
  SfWgradArgs a;
  memset(&a, 0, sizeof(a));
  a.dy = j.dy; a.ldy = j.ldy; a.x = j.x; a.ldx = j.ldx; a.M = M; a.N1 = j.N1; a.N2 = j.N2; a.out = j.out; a.ldo = j.ldo;
  a.accumulate = j.accumulate; a.alpha = j.alpha; a.partial = c.wg_partial();
  a.dbias = j.dbias; a.dbias_scratch = bias_scratch ? c.cs_partial() : nullptr;
  return sf_launch_wgrad(a, c.s);
}

// weight + bias gradients of one Linear: dW (+)= dy^T x, db += colsum(dy); LoRA factors from dW_eff.  A dense one may wait in the layer's group.
static hipError_t lin_wgrad(const StepCtx& c, const TLin& l, const bf16_t* dy, const bf16_t* x, int M) {
  const sf_trainer* t = c.t;
  float* gw = GG(t, c.grads, l.pw, l.pw_off);
  float* gb = GG(t, c.grads, l.pb, l.pb_off);
  if (l.pla < 0 && gw && c.can_queue(M, l.N, l.K)) return submit(c, lin_job(l, dy, x, gw, gb), M, WG_QUEUE, true);
  hipError_t e = hipSuccess;
  if (l.pla >= 0) {
    // W_eff = W + B A (modeling:541-545):  dB = dy^T (x A^T),  dA = (dy B)^T x  — two rank-32 projections
    // and two skinny weight-gradient GEMMs instead of the full [N,K] one (the base weight is frozen)
    if ((e = tgemm(x, l.la_bf, nullptr, M, kRank, l.K, SF_EPI_BF16, c.s, nullptr, c.lora_u())) != hipSuccess) return e;
    if ((e = tgemm(dy, l.lbT_bf, nullptr, M, kRank, l.N, SF_EPI_BF16, c.s, nullptr, c.lora_v())) != hipSuccess) return e;
    float* gB = GG(t, c.grads, l.plb);
    float* gA = GG(t, c.grads, l.pla);
    if (gB && (e = submit(c, wgrad_job(dy, l.N, c.lora_u(), kRank, l.N, kRank, gB, nullptr, 1), M, WG_DIRECT, false)) != hipSuccess) return e;
    if (gA && (e = submit(c, wgrad_job(c.lora_v(), kRank, x, l.K, kRank, l.K, gA, nullptr, 1), M, WG_DIRECT, false)) != hipSuccess) return e;
  }
  if (gw) e = submit(c, lin_job(l, dy, x, gw, gb), M, WG_DIRECT, true);      // bias gradient rides on the same launch
  else if (gb) e = sf_launch_colsum_bf16(dy, M, l.N, l.Nw, 1.f, gb, 1, c.cs_partial(), c.s);
  return e;
}

// weight gradients of a spatial Linear; those of a LoRA-adapted one are forked onto the side stream behind everything the caller's
// stream has enqueued so far (its operands are complete there); the caller joins at the end of the layer
static hipError_t lin_wgrad_side(const StepCtx& c, const TLin& l, const bf16_t* dy, const bf16_t* x, int M, bool* forked) {
  // only the rank-32 factor gradients go to the side stream: ws.wg_partial_side is sized for those shapes.  A LoRA-adapted Linear whose
  // base weight is NOT frozen (add_lora_spatial without frozen_spatial: scripts/pretrain_streamformer.sh:32-33) also needs the full
  // [N, K] gradient and stays on the caller's stream with the full-size scratch; so does everything when the layer does not group.
  if (!c.group || l.pla < 0 || GG(c.t, c.grads, l.pw, l.pw_off) != nullptr || !c.t->side.ready()) return lin_wgrad(c, l, dy, x, M);
  hipError_t e = c.t->side.fork(c.s);
  if (e != hipSuccess) return e;
  *forked = true;
  return lin_wgrad(c.on_side_stream(), l, dy, x, M);
}

static int backward_head(const StepCtx& c, const float* d_pooler, const float* d_lhs) {
  const sf_trainer* t = c.t;
  const TWs& ws = *c.ws;
  hipStream_t s = c.s;
  const int D = t->D, N = c.p->N, M = c.p->M, F = c.p->F;
  const float eps = t->cfg.layer_norm_eps;
  const float* P0 = t->params_dev;
  // pooler = attn_out + fc2(gelu(fc1(LN(attn_out))))
  HIP_TRY(sf_launch_split(d_pooler, ws.gh_bf, nullptr, (size_t)F * D, s));
  HIP_TRY(lin_dgrad(t->fc2, ws.gh_bf, F, s, nullptr, ws.d_hm));
  HIP_TRY(lin_wgrad(c, t->fc2, ws.gh_bf, ws.hm, F));
  HIP_TRY(sf_launch_gelu_bwd(ws.d_hm, ws.hm_pre, (size_t)F * t->Ip, s));
  HIP_TRY(lin_dgrad(t->fc1, ws.d_hm, F, s, ws.d_hn, nullptr));
  HIP_TRY(lin_wgrad(c, t->fc1, ws.d_hm, ws.hn, F));
  HIP_TRY(sf_launch_ln_bwd(ws.attn_out, ws.d_hn, 0, PP(t, P0, t->hln_g), d_pooler, ws.gh, ws.gh_bf, GG(t, c.grads, t->hln_g), GG(t, c.grads, t->hln_b), ws.ln_partial, F, D, eps, s));
  // attn_out = out_proj(ctx)   (gh_bf = bf16(gh) written by the LayerNorm backward)
  HIP_TRY(lin_dgrad(t->head_out, ws.gh_bf, F, s, ws.d_pc, nullptr));
  HIP_TRY(lin_wgrad(c, t->head_out, ws.gh_bf, ws.pc, F));
  // probe attention over the N tokens of every frame
  // ctx_h = Wv_h z_h + bv_h: dz, dWv, dbv (the value rows are in_proj rows [2D, 3D))
  const bool gen = t->hd != 64;
  const float* pz = gen ? ws.pgen + (size_t)F * t->heads * N : ws.pz;
  if (gen) {
    HIP_TRY(sf_launch_pool_ctx_bwd_generic(ws.d_pc, PP(t, P0, t->p_inw, (size_t)2 * D * D), D, pz, ws.pdz, GG(t, c.grads, t->p_inw, (size_t)2 * D * D),
                                           GG(t, c.grads, t->p_inb, (size_t)2 * D), F, t->heads, t->hd, D, s));
    SfPoolGenBwdArgs pb;
    memset(&pb, 0, sizeof(pb));
    pb.x_bf = ws.xn; pb.scores = ws.pgen; pb.z = pz; pb.dz = ws.pdz; pb.u = t->head_u; pb.d_lhs = d_lhs; pb.dx = ws.d_ln; pb.ds_bf = ws.pds;
    pb.stats = ws.pgstat; pb.F = F; pb.N = N; pb.heads = t->heads; pb.D = D;
    HIP_TRY(sf_launch_pool_probe_bwd_generic(pb, s));
  } else {
    HIP_TRY(sf_launch_pool_ctx_bwd(ws.d_pc, t->head_kv.wT, 2 * D, D, ws.pz, ws.pdz, GG(t, c.grads, t->p_inw, (size_t)2 * D * D), D,
                                   GG(t, c.grads, t->p_inb, (size_t)2 * D), F, t->heads, D, s));
    // p = softmax(x . U), z = p x: dx (+ the gradient that arrives through last_hidden_state) and the score gradients ds
    SfPoolBwdArgs pb;
    memset(&pb, 0, sizeof(pb));
    pb.x_bf = ws.xn; pb.probs = ws.pprobs; pb.probs_raw = 1; pb.ml = ws.pml; pb.ml_splits = sf_pool_splits(F, N, t->heads); pb.z = ws.pz; pb.dz = ws.pdz; pb.u = t->head_u; pb.d_lhs = d_lhs; pb.dx = ws.d_ln; pb.ds_bf = ws.pds;
    pb.F = F; pb.N = N; pb.heads = t->heads; pb.D = D;
    HIP_TRY(sf_launch_pool_probe_bwd(pb, s));
  }
  // dU = ds^T x over all token rows ([32, D], rows >= heads zero), then U_h = Wk_h^T q_h: dWk_h += q_h dU_h^T, dq_h = Wk_h dU_h.
  // The key bias gets no gradient: its term q_h . bk_h is constant over the keys and cancels in the softmax.
  HIP_TRY(submit(c, wgrad_job(ws.pds, 32, ws.xn, D, 32, D, ws.pdu, nullptr, 0), M, WG_DIRECT, false));
  if (gen)
    HIP_TRY(sf_launch_pool_u_bwd_generic(ws.pdu, PP(t, P0, t->p_inw, (size_t)D * D), t->head_q, GG(t, c.grads, t->p_inw, (size_t)D * D), ws.dq_total,
                                         t->hd, D, s));
  else
    HIP_TRY(sf_launch_pool_u_bwd(ws.pdu, PP(t, P0, t->p_inw, (size_t)D * D), t->head_q, GG(t, c.grads, t->p_inw, (size_t)D * D), ws.dq_total, D, s));
  HIP_TRY(sf_launch_head_query_bwd(ws.dq_total, PP(t, P0, t->p_probe), PP(t, P0, t->p_inw), t->scale, GG(t, c.grads, t->p_inw),
                                   GG(t, c.grads, t->p_inb), GG(t, c.grads, t->p_probe), D, s));
  // post_layernorm: g = dLN(h_L)
  HIP_TRY(sf_launch_ln_bwd(ws.h[t->L], ws.d_ln, 0, PP(t, P0, t->post_g), nullptr, ws.g, ws.g_bf, GG(t, c.grads, t->post_g), GG(t, c.grads, t->post_b), ws.ln_partial, M, D, eps, s));
  return SF_OK;
}

// The D x D algebra behind the temporal branch's product G = g^T x and cs = colsum g (both complete in c's stream order).
// Two projections (x = t_out): dW_d += tanh(g) G, db_d += tanh(g) cs, dgate += (1 - tanh^2)(<G, W_d> + <cs, b_d>)  (sf_launch_gate_grad).
// Fused (x = ctx, G is G1): g^T t_out = G1 W_o^T + cs b_o^T takes G's place, and
//   dW_o += (tanh(g) W_d)^T G1,  db_o += (tanh(g) W_d)^T cs                    (all D x D; bf16 operands like every backward GEMM)
static hipError_t temporal_grads(const StepCtx& c, const TLayer& l, const float* G, const float* cs) {
  const sf_trainer* t = c.t;
  const TWs& ws = *c.ws;
  const float* P0 = t->params_dev;
  hipStream_t s = c.s;
  const int D = t->D;
  const bool fused = c.p->tfuse;
  hipError_t e;
  if (fused) {
    if ((e = sf_launch_split(G, ws.g1_bf, nullptr, (size_t)D * D, s)) != hipSuccess) return e;
    if ((e = tgemm(ws.g1_bf, l.t_out.w, nullptr, D, D, D, SF_EPI_F32, s, ws.dw_scratch2, nullptr)) != hipSuccess) return e;
    G = ws.dw_scratch2;
  }
  if ((e = sf_launch_gate_grad(G, cs, PP(t, P0, l.t_dense.pw), PP(t, P0, l.t_dense.pb), PP(t, P0, l.gate),
                               GG(t, c.grads, l.t_dense.pw), GG(t, c.grads, l.t_dense.pb), GG(t, c.grads, l.gate), t->red_partial, D, D, s,
                               fused ? PP(t, P0, l.t_out.pb) : nullptr)) != hipSuccess || !fused) return e;
  if (float* gwo = GG(t, c.grads, l.t_out.pw))
    if ((e = submit(c, wgrad_job(l.t_dense.w, D, ws.g1_bf, D, D, D, gwo, nullptr, 1), D, WG_DIRECT, false)) != hipSuccess) return e;
  if (float* gbo = GG(t, c.grads, l.t_out.pb))
    if ((e = sf_launch_matvec_t_bf16(l.t_dense.w, D, cs, gbo, D, D, s)) != hipSuccess) return e;
  return hipSuccess;
}

// h1 = h + tanh(gate) * dense(out(ctx)): the gradient g (ws.g_bf2) through the temporal branch's projections, down to d_ctx.
// G / cs: g^T x and colsum g, two buffers by layer parity when fused (the side stream reads one layer behind); queued: finish_temporal_proj runs the algebra
struct TemporalProj { float* G; float* cs; bool queued; };
static int backward_temporal_proj(const StepCtx& c, int li, TemporalProj* tp) {
  const sf_trainer* t = c.t;
  const TWs& ws = *c.ws;
  const StepPlan& p = *c.p;
  hipStream_t s = c.s;
  const TLayer& l = t->layers[li];
  const TSavedLayer& sv = ws.sl[li];
  const int D = t->D, M = p.M;
  const bool alt = p.tfuse && (li & 1);
  tp->G = alt ? ws.g1_alt : ws.dw_scratch;
  tp->cs = alt ? ws.cs_alt : ws.cs;
  HIP_TRY(hipMemsetAsync(tp->cs, 0, (size_t)D * sizeof(float), s));
  const bf16_t* x;
  if (p.tfuse) {
    // forward ran h1 = h + ctx W_f^T + b_f with W_f = tanh(g) W_d W_o.  One input-gradient GEMM, d_ctx = g W_f, and ONE token-
    // contracting GEMM, G1 = g^T ctx [D, D] (+ cs = colsum g): everything else is D x D algebra (temporal_grads)
    HIP_TRY(tgemm(ws.g_bf2, l.wfT, nullptr, M, D, D, SF_EPI_BF16, s, nullptr, ws.d_ctx));
    x = sv.ctx_t;
  } else {
    HIP_TRY(lin_dgrad(l.t_dense, ws.g_bf2, M, s, nullptr, ws.d_tout));               // wT already carries tanh(gate)
    x = sv.t_out;                                                                    // unscaled G = g^T t_out
  }
  tp->queued = c.can_queue(M, D, D);
  const WgRoute route = tp->queued ? WG_QUEUE : (p.tfuse && sf_wgrad_groupable(M, D, D)) ? WG_LONE_GROUP : WG_DIRECT;
  HIP_TRY(submit(c, temporal_job(ws.g_bf2, x, D, tp->G, tp->cs), M, route, true));
  if (!tp->queued) HIP_TRY(temporal_grads(c, l, tp->G, tp->cs));
  if (!p.tfuse) {
    if (p.scaled()) HIP_TRY(sf_launch_rowscale_bf16(ws.d_tout, ws.d_tout, p.dp_temporal(li), M, D, 0, p.T, p.N, s, p.hidden_site(li, SITE_TEMPORAL_OUT)));     // through the drop_path / dropout in front of temporal_dense
    HIP_TRY(lin_dgrad(l.t_out, ws.d_tout, M, s, nullptr, ws.d_ctx));
    HIP_TRY(lin_wgrad(c, l.t_out, ws.d_tout, sv.ctx_t, M));
  }
  return SF_OK;
}
// behind the layer's grouped launch: the algebra of a queued product.  The fused form goes to the side stream, joined one layer later
// (wait_small); LoRA work enqueued there before it is marked complete first, so that the end-of-layer join does not wait for these launches
static int finish_temporal_proj(const StepCtx& c, int li, const TemporalProj& tp, bool lora_forked) {
  if (!tp.queued) return SF_OK;
  const TLayer& l = c.t->layers[li];
  SideStream& side = c.t->side;
  if (c.p->tfuse && side.ready()) {       // queued: the layer groups, so its operands stay intact for the side stream too
    if (lora_forked) HIP_TRY(side.mark_join());
    HIP_TRY(side.fork(c.s));
    HIP_TRY(temporal_grads(c.on_side_stream(), l, tp.G, tp.cs));
    HIP_TRY(side.mark_small(li & 1));
  } else {
    HIP_TRY(temporal_grads(c, l, tp.G, tp.cs));
  }
  return SF_OK;
}

static SfAttnBwdArgs tattn_bwd_args(const StepCtx& c, int li, bool temporal, const bf16_t* qkv, const bf16_t* o, const bf16_t* d_o, bf16_t* d_qkv,
                                    const float* lse_s) {
  const sf_trainer* t = c.t;
  const StepPlan& p = *c.p;
  SfAttnBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.qkv = qkv; a.ld_qkv = 3 * t->D; a.o = o; a.ld_o = t->D; a.d_o = d_o; a.d_qkv = d_qkv;
  a.heads = t->heads; a.D = t->D; a.scale = t->scale; a.head_dim = t->hd;
  if (temporal) { a.L = p.T; a.nseq = p.B * p.N; a.seq_rows = p.N; a.causal = t->cfg.enable_causal_temporal; }
  else { a.L = p.N; a.nseq = p.F; a.seq_rows = 1; a.causal = 0; if (t->hd == 64) a.lse2 = lse_s; }
  if (p.drop_attn > 0.f) a.drop = p.attn_site(li, temporal ? SITE_TEMPORAL_PROBS : SITE_SPATIAL_PROBS);
  return a;
}

static int backward_layer(const StepCtx& step, int li) {
  const sf_trainer* t = step.t;
  const TWs& ws = *step.ws;
  const StepPlan& p = *step.p;
  hipStream_t s = step.s;
  const TLayer& l = t->layers[li];
  const TSavedLayer& sv = ws.sl[li];
  const int D = t->D, N = p.N, T = p.T, M = p.M;
  const float eps = t->cfg.layer_norm_eps;
  const float* P0 = t->params_dev;
  // one encoder layer's weight gradients, batched: a groupable Linear is queued with its operands and launched together with the
  // others at the end of the layer.  The side stream has the same condition: its operands must stay untouched until then.
  // With drop_path / dropout (a row factor on every branch gradient: 0 or 1 / keep per sample group, or the forward's mask) every
  // launch is immediate.
  SfWgradGroup group;
  memset(&group, 0, sizeof(group));
  group.M = M; group.partial = ws.wg_partial;
  StepCtx c = step;
  c.group = p.group_wgrads() ? &group : nullptr;
  bool forked = false;
  // g (fp32) and its bf16 copy are both written by the LayerNorm backward that produced them; the bf16 copy rotates through
  // g_bf -> g_bf1 -> g_bf2 -> g_bf inside the layer and the three attention / MLP gradients have their own wide buffers, so
  // that every queued weight gradient still finds its operands at the end of the layer
  // ---- MLP: out = h2 + down(gelu(up(LN_a(h2)))) --------------------------------------------------------
  const bf16_t* gy = ws.g_bf;
  if (p.scaled()) { HIP_TRY(sf_launch_rowscale_bf16(ws.g_bf, ws.d_ctx, p.dp_mlp(li), M, D, 2, T, N, s, p.hidden_site(li, SITE_MLP_OUT))); gy = ws.d_ctx; }
  HIP_TRY(lin_dgrad_dgelu(l.down, gy, M, s, ws.d_wide, sv.pre));            // d pre = (g W_down) * gelu'(pre)  [M,I]
  if (p.drop_hidden > 0.f) HIP_TRY(sf_launch_rowscale_bf16(ws.d_wide, ws.d_wide, nullptr, M, t->Ip, 0, T, N, s, p.hidden_site(li, SITE_MLP_ACT)));      // ... through the activation's dropout mask (elementwise factors commute)
  HIP_TRY(lin_wgrad(c, l.down, gy, sv.act, M));
  HIP_TRY(lin_dgrad(l.up, ws.d_wide, M, s, nullptr, ws.d_ln_bf));
  HIP_TRY(lin_wgrad(c, l.up, ws.d_wide, sv.ln_a, M));
  HIP_TRY(sf_launch_ln_bwd(sv.h2, ws.d_ln_bf, 1, PP(t, P0, l.ln_a_g), ws.g, ws.g, ws.g_bf1, GG(t, c.grads, l.ln_a_g), GG(t, c.grads, l.ln_a_b), ws.ln_partial, M, D, eps, s));
  // ---- spatial: h2 = h1 + out(attn(qkv(LN_b(h1)))) ---------------------------------------------------------
  gy = ws.g_bf1;
  if (p.scaled()) { HIP_TRY(sf_launch_rowscale_bf16(ws.g_bf1, ws.d_tout, p.dp_spatial(li), M, D, 1, T, N, s, p.hidden_site(li, SITE_SPATIAL_OUT))); gy = ws.d_tout; }
  HIP_TRY(lin_dgrad(l.s_out, gy, M, s, nullptr, ws.d_ctx));
  HIP_TRY(lin_wgrad_side(c, l.s_out, gy, sv.ctx_s, M, &forked));
  HIP_TRY(sf_launch_spatial_attention_bwd(tattn_bwd_args(c, li, false, sv.sqkv, sv.ctx_s, ws.d_ctx, ws.d_wide_s, sv.lse_s), s));
  HIP_TRY(lin_wgrad_side(c, l.s_qkv, ws.d_wide_s, sv.ln_b, M, &forked));
  HIP_TRY(lin_dgrad(l.s_qkv, ws.d_wide_s, M, s, nullptr, ws.d_ln_bf));
  HIP_TRY(sf_launch_ln_bwd(sv.h1, ws.d_ln_bf, 1, PP(t, P0, l.ln_b_g), ws.g, ws.g, ws.g_bf2, GG(t, c.grads, l.ln_b_g), GG(t, c.grads, l.ln_b_b), ws.ln_partial, M, D, eps, s));
  // ---- temporal: h1 = h + tanh(gate) * dense(out(attn(qkv(LN_t(h))))) ----------------------------------------
  TemporalProj tp;
  int rc = backward_temporal_proj(c, li, &tp);
  if (rc) return rc;
  HIP_TRY(sf_launch_temporal_attention_bwd(tattn_bwd_args(c, li, true, sv.tqkv, sv.ctx_t, ws.d_ctx, ws.d_wide_t, nullptr), s));
  HIP_TRY(lin_wgrad(c, l.t_qkv, ws.d_wide_t, sv.ln_t, M));
  HIP_TRY(lin_dgrad(l.t_qkv, ws.d_wide_t, M, s, nullptr, ws.d_ln_bf));
  if (group.njobs > 0) HIP_TRY(sf_launch_wgrad_group(group, s));
  if ((rc = finish_temporal_proj(c, li, tp, forked)) != SF_OK) return rc;
  HIP_TRY(sf_launch_ln_bwd(ws.h[li], ws.d_ln_bf, 1, PP(t, P0, l.ln_t_g), ws.g, ws.g, ws.g_bf, GG(t, c.grads, l.ln_t_g), GG(t, c.grads, l.ln_t_b), ws.ln_partial, M, D, eps, s));
  if (forked) HIP_TRY(c.t->side.join(s));
  // the PREVIOUS layer's D x D algebra (other parity) must be done before the next layer reuses its G1 / cs buffers
  HIP_TRY(c.t->side.wait_small(s, (li & 1) ^ 1));
  return SF_OK;
}

static int backward_embeddings(const StepCtx& c) {
  const sf_trainer* t = c.t;
  const TWs& ws = *c.ws;
  const StepPlan& p = *c.p;
  hipStream_t s = c.s;
  const int D = t->D, N = p.N, B = p.B, T = p.T, M = p.M;
  // h0 = patches W^T + b + pos[n] + time[t]   (modeling:336-350, 413-457)
  const bool hd = p.drop_hidden > 0.f;
  float* gt = GG(t, c.grads, t->p_time);
  if (hd) {
    // h0 = m_time o (m_pos o (patches W^T + b + pos) + time): the time table sees m_time o g, everything else m_pos o m_time o g
    HIP_TRY(sf_launch_dropout_f32(ws.g, nullptr, (size_t)M * D, p.embed_site(SITE_EMBED_TIME), s));
    HIP_TRY(sf_launch_sum_rows(ws.g, ws.s_tn, T * N, T * N, 1, 0, B, (long)T * N, D, 0, s));
    if (gt) HIP_TRY(sf_launch_sum_rows(ws.s_tn, gt, T, T, N, 0, N, 1, D, 1, s));
    HIP_TRY(sf_launch_dropout_f32(ws.g, ws.g_bf, (size_t)M * D, p.embed_site(SITE_EMBED_POS), s));
  }
  HIP_TRY(lin_wgrad(c, t->patch, ws.g_bf, ws.patches, M));
  HIP_TRY(sf_launch_sum_rows(ws.g, ws.s_tn, T * N, T * N, 1, 0, B, (long)T * N, D, 0, s));       // sum over batch
  if (float* gp = GG(t, c.grads, t->p_pos)) HIP_TRY(sf_launch_sum_rows(ws.s_tn, gp, N, N, 1, 0, T, N, D, 1, s));
  if (!hd && gt) HIP_TRY(sf_launch_sum_rows(ws.s_tn, gt, T, T, N, 0, N, 1, D, 1, s));
  return SF_OK;
}

extern "C" int sf_trainer_backward(sf_trainer* t, const float* d_pooler, const float* d_lhs, float* grads, int stage_first,
                                   int stage_last, void* workspace, size_t workspace_bytes, sf_stream stream) {
  if (!t || !grads || !workspace) return sf_set_err(SF_ERR_INVALID, "null argument");
  if (!t->plan.valid) return sf_set_err(SF_ERR_STATE, "sf_trainer_backward needs a preceding sf_trainer_forward");
  if (stage_first < 0 || stage_last > t->L + 1 || stage_first > stage_last) return sf_set_err(SF_ERR_INVALID, "bad stage range");
  if (stage_first == 0 && !d_pooler) return sf_set_err(SF_ERR_INVALID, "stage 0 needs d_pooler");
  HIP_TRY(hipSetDevice(t->device));
  const TWs ws = tcarve(t, workspace, t->plan.B, t->plan.T);
  if (workspace_bytes < ws.bytes) return sf_set_err(SF_ERR_WORKSPACE, "workspace too small: %zu < %zu", workspace_bytes, ws.bytes);
  const StepCtx c{t, &ws, &t->plan, (hipStream_t)stream, grads};
  for (int st = stage_first; st <= stage_last; ++st) {
    int rc;
    if (st == 0) rc = backward_head(c, d_pooler, d_lhs);
    else if (st == t->L + 1) rc = backward_embeddings(c);
    else rc = backward_layer(c, t->L - st);
    if (rc) return rc;
  }
  // every gradient slice of the stages just run must be complete in the caller's stream order when this call returns (the
  // caller all-reduces them): join what is still on the side stream
  HIP_TRY(t->side.drain((hipStream_t)stream));
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// optimizer
// ------------------------------------------------------------------------------------------------
extern "C" int sf_trainer_adamw_step(sf_trainer* t, float* params, float* grads, float* m, float* v, int step, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                     const float* grad_sumsq_dev, float clip_norm, int zero_grads, sf_stream stream) {
  if (!t || !params || !grads || !m || !v) return sf_set_err(SF_ERR_INVALID, "null argument");
  if (step < 1) return sf_set_err(SF_ERR_INVALID, "step counts from 1");
  HIP_TRY(hipSetDevice(t->device));
  SfAdamWArgs a;
  a.p = params; a.g = grads; a.m = m; a.v = v; a.n = t->n_train;
  a.seg_end = t->seg_end; a.seg_decay = t->seg_decay; a.seg_train = t->seg_train; a.nseg = t->nseg;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay;
  a.bias_correction1 = 1.0f - powf(beta1, (float)step);
  a.bias_correction2 = 1.0f - powf(beta2, (float)step);
  a.grad_scale = grad_scale;
  a.clip_sumsq = grad_sumsq_dev; a.clip_norm = clip_norm; a.zero_grads = zero_grads;
  a.extra_seg0 = t->extra_seg0;
  a.n_extra = t->extra_steps_set ? t->n_extra : 0;
  for (int i = 0; i < 64; ++i) a.extra_steps[i] = t->extra_steps[i];
  if (grad_sumsq_dev && !(clip_norm > 0.f)) return sf_set_err(SF_ERR_INVALID, "clip_norm must be positive");
  a.guard_flag = t->guard_flag; a.guard_sumsq = nullptr; a.guard_loss = t->guard_loss;
  if (t->guard_flag) {
    // the clip pass already holds sum g^2 of this gradient; otherwise one deterministic pass over the trainable prefix (~0.1 ms)
    if (grad_sumsq_dev) a.guard_sumsq = grad_sumsq_dev;
    else {
      if (!t->guard_sumsq) HIP_TRY(hipMalloc((void**)&t->guard_sumsq, sizeof(float)));
      HIP_TRY(sf_launch_sumsq(grads, t->n_train, t->guard_sumsq, t->red_partial, (hipStream_t)stream));
      a.guard_sumsq = t->guard_sumsq;
    }
  }
  HIP_TRY(sf_launch_adamw(a, (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_trainer_set_dropout(sf_trainer* t, float hidden_p, float attn_p, uint32_t seed) {
  if (!t) return sf_set_err(SF_ERR_INVALID, "null argument");
  if (!(hidden_p >= 0.f && hidden_p < 1.f) || !(attn_p >= 0.f && attn_p < 1.f)) return sf_set_err(SF_ERR_INVALID, "dropout probabilities must be in [0, 1)");
  t->drop_hidden = hidden_p; t->drop_attn = attn_p; t->drop_seed = seed;
  return SF_OK;
}

extern "C" int sf_trainer_set_nonfinite_guard(sf_trainer* t, int32_t* flag_dev, const float* loss_dev) {
  if (!t) return sf_set_err(SF_ERR_INVALID, "null argument");
  t->guard_flag = (int*)flag_dev;
  t->guard_loss = flag_dev ? loss_dev : nullptr;
  return SF_OK;
}

extern "C" int sf_trainer_set_drop_path(sf_trainer* t, const float* scales_dev, int B, int T) {
  if (!t) return sf_set_err(SF_ERR_INVALID, "null argument");
  if (scales_dev && (B <= 0 || T <= 0)) return sf_set_err(SF_ERR_INVALID, "bad geometry B=%d T=%d", B, T);
  t->dp_scales = scales_dev; t->dp_B = B; t->dp_T = T;
  return SF_OK;
}

extern "C" int sf_trainer_set_extra_steps(sf_trainer* t, const int32_t* steps, int n) {
  if (!t) return sf_set_err(SF_ERR_INVALID, "null argument");
  if (!steps || n == 0) { t->extra_steps_set = false; return SF_OK; }
  if (n != t->n_extra) return sf_set_err(SF_ERR_INVALID, "sf_trainer_set_extra_steps: %d entries for %d slots", n, t->n_extra);
  for (int i = 0; i < n; ++i) {
    if (steps[i] < 0) return sf_set_err(SF_ERR_INVALID, "negative step count");
    t->extra_steps[i] = steps[i];
  }
  t->extra_steps_set = true;
  return SF_OK;
}

extern "C" int sf_trainer_grad_sumsq(sf_trainer* t, const float* grads, float* out, sf_stream stream) {
  if (!t || !grads || !out) return sf_set_err(SF_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(t->device));
  HIP_TRY(sf_launch_sumsq(grads, t->n_train, out, t->red_partial, (hipStream_t)stream));
  return SF_OK;
}

// ------------------------------------------------------------------------------------------------
// single backward operators (parity tests)
// ------------------------------------------------------------------------------------------------
extern "C" int sf_op_wgrad(const void* dy, int ldy, const void* x, int ldx, int M, int N1, int N2, float alpha, int accumulate,
                           float* out, int ldo, float* dbias, sf_stream stream) {
  if (!dy || !x || !out) return sf_set_err(SF_ERR_INVALID, "null argument");
  float* partial = nullptr;
  HIP_TRY(hipMalloc(&partial, (sf_wgrad_partial_floats(M, N1, N2) + sf_colsum_partial_floats(N1)) * sizeof(float)));
  SfWgradArgs a;
  memset(&a, 0, sizeof(a));
  a.dy = (const bf16_t*)dy; a.ldy = ldy; a.x = (const bf16_t*)x; a.ldx = ldx; a.M = M; a.N1 = N1; a.N2 = N2;
  a.out = out; a.ldo = ldo; a.accumulate = accumulate; a.alpha = alpha; a.partial = partial;
  a.dbias = dbias; a.dbias_scratch = partial + sf_wgrad_partial_floats(M, N1, N2);
  hipError_t e = sf_launch_wgrad(a, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(partial);
  if (e != hipSuccess) return sf_set_err(SF_ERR_HIP, "sf_op_wgrad: %s", hipGetErrorString(e));
  return SF_OK;
}

extern "C" int sf_op_attention_bwd(const void* qkv, const void* o, const void* d_o, void* d_qkv, int layout, int nseq, int L,
                                   int seq_rows, int heads, int causal, sf_stream stream) {
  if (!qkv || !o || !d_o || !d_qkv) return sf_set_err(SF_ERR_INVALID, "null argument");
  SfAttnBwdArgs a;
  memset(&a, 0, sizeof(a));
  const int D = heads * 64;
  a.qkv = (const bf16_t*)qkv; a.ld_qkv = 3 * D; a.o = (const bf16_t*)o; a.ld_o = D; a.d_o = (const bf16_t*)d_o;
  a.d_qkv = (bf16_t*)d_qkv; a.heads = heads; a.D = D; a.scale = 0.125f; a.L = L; a.nseq = nseq; a.seq_rows = seq_rows;
  a.causal = causal;
  HIP_TRY(layout == 0 ? sf_launch_spatial_attention_bwd(a, (hipStream_t)stream) : sf_launch_temporal_attention_bwd(a, (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_op_attention_bwd_hd(const void* qkv, const void* o, const void* d_o, void* d_qkv, int layout, int nseq, int L,
                                      int seq_rows, int heads, int head_dim, int causal, sf_stream stream) {
  if (!qkv || !o || !d_o || !d_qkv) return sf_set_err(SF_ERR_INVALID, "null argument");
  if (heads <= 0 || head_dim < 8 || head_dim > 128 || head_dim % 8)
    return sf_set_err(SF_ERR_INVALID, "sf_op_attention_bwd_hd: head_dim %d (multiples of 8 up to 128), heads %d", head_dim, heads);
  SfAttnBwdArgs a;
  memset(&a, 0, sizeof(a));
  const int D = heads * head_dim;
  a.qkv = (const bf16_t*)qkv; a.ld_qkv = 3 * D; a.o = (const bf16_t*)o; a.ld_o = D; a.d_o = (const bf16_t*)d_o;
  a.d_qkv = (bf16_t*)d_qkv; a.heads = heads; a.D = D; a.scale = 1.0f / sqrtf((float)head_dim); a.L = L; a.nseq = nseq; a.seq_rows = seq_rows;
  a.causal = causal; a.head_dim = head_dim;
  HIP_TRY(layout == 0 ? sf_launch_spatial_attention_bwd(a, (hipStream_t)stream) : sf_launch_temporal_attention_bwd(a, (hipStream_t)stream));
  return SF_OK;
}

extern "C" int sf_op_layernorm_bwd(const float* x, const float* dy, const float* gamma, const float* g_in, float* dx,
                                   float* d_gamma, float* d_beta, int rows, int D, float eps, sf_stream stream) {
  if (!x || !dy || !gamma || !dx) return sf_set_err(SF_ERR_INVALID, "null argument");
  float* partial = nullptr;
  HIP_TRY(hipMalloc(&partial, sf_ln_bwd_partial_floats(D) * sizeof(float)));
  hipError_t e = sf_launch_ln_bwd(x, dy, 0, gamma, g_in, dx, nullptr, d_gamma, d_beta, partial, rows, D, eps, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(partial);
  if (e != hipSuccess) return sf_set_err(SF_ERR_HIP, "sf_op_layernorm_bwd: %s", hipGetErrorString(e));
  return SF_OK;
}
