// The encoder's handle, the workspace of one call, and the request -> plan -> launch interface of its forward: what sf_encoder.hip
// (handle, weights, plan, forward) shares with sf_stream.hip (KV-cache, graphs, streaming entries) and sf_bench.hip (bench hooks).
// Private to the library.
#pragma once
#include "sf_handle.h"

#include <vector>

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

// ------------------------------------------------------------------------------------------------
// the workspace of one call (carve), its request and its plan (plan_forward)
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

// What the row count alone decides about the bf16-mode schedule (resid_planes_at)
struct FoldShape { bool tile_fold, small_fold, stats_fold; };      // stats_fold: a fold with a statistics buffer

// ------------------------------------------------------------------------------------------------
// sf_encoder.hip, for the other units (library-internal: not in the dynamic symbol table)
// ------------------------------------------------------------------------------------------------
#pragma GCC visibility push(hidden)
int check_geometry(const sf_encoder* e, int B, int T, int H, int W, const float* pos_dev, int* N_out);
Workspace carve(const sf_encoder* e, void* base, int B, int T, int N, bool need_tqkv);      // base null: sizing (Workspace::bytes)
ForwardPlan plan_forward(const sf_encoder* e, const ForwardRequest& rq, const Workspace& ws);
int run_plan(sf_encoder* e, const ForwardPlan& p, const Workspace& ws, hipStream_t s);       // one call of the encoder over T new frames, as planned
int run_forward(sf_encoder* e, const ForwardRequest& rq, const Workspace& ws, hipStream_t s);      // plan_forward + run_plan
// the fields every Linear of the forward shares (sf_linear_args with the encoder's activation and LayerNorm epsilon)
SfGemmArgs linear_args(const sf_encoder* e, const DevLinear& lin, const bf16_t* a_hi, const bf16_t* a_lo, int M, int epi, bool split);
// bf16 mode: the residual projections at M rows run on hi + lo planes with LayerNorm row sums (fs: the folds the answer was made from)
bool resid_planes_at(const sf_encoder* e, int M, FoldShape* fs = nullptr);
#pragma GCC visibility pop
