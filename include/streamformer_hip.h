/*
 * streamformer_hip.h — C ABI of the MI355X (gfx950) StreamFormer encoder hot path.
 *
 * The reference has no FFI seam: the path is a torch.nn.Module,
 * TimesformerMultiTaskingModelSigLIP (reference models/modeling_timesformer_siglip.py:1241-1354).
 * This header is the boundary a binding would use instead of that module's forward; the Python
 * mirror of the module (streamformer_amd/modeling.py) binds it with ctypes, INTEGRATION.md shows
 * the stub.  Each entry point cites the reference interface it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.  Every function returns 0 on
 *     success or a negative sf_status; sf_last_error() gives the message of the last failure on the
 *     calling thread.
 *   - All device buffers passed in (pixels, outputs, workspace) are CALLER-allocated and
 *     caller-owned; the library never frees them and never synchronises the stream.  Weights and
 *     KV-caches are library-owned device memory.
 *   - All work is enqueued on the caller's hipStream_t (pass torch.cuda.current_stream()).
 *   - A handle is bound to one device and may be used from one thread at a time.
 *   - Layout: activations are FRAME-major [B, T, N, D] row-major (token row = (b*T + t)*N + n),
 *     not the reference's patch-major (B, N*T, D) (modeling:452-457).
 */
#ifndef STREAMFORMER_HIP_H
#define STREAMFORMER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sf_encoder sf_encoder;   /* opaque: config + packed weights on one device        */
typedef struct sf_cache sf_cache;       /* opaque: temporal K/V cache of one stream (all layers) */
typedef void* sf_stream;                /* hipStream_t                                          */

typedef enum {
  SF_OK = 0,
  SF_ERR_INVALID = -1,      /* bad argument / unsupported configuration                      */
  SF_ERR_STATE = -2,        /* call order (e.g. forward before finalize, missing weight)     */
  SF_ERR_HIP = -3,          /* HIP runtime error (message carries hipGetErrorString)         */
  SF_ERR_WORKSPACE = -4,    /* workspace too small                                           */
  SF_ERR_UNKNOWN_KEY = -5,  /* sf_load_tensor: not a weight of this model (ignored keys OK)  */
  SF_ERR_CAPACITY = -6      /* streaming past the cache / time-embedding capacity            */
} sf_status;

typedef enum { SF_F32 = 0, SF_BF16 = 1, SF_F16 = 2, SF_F64 = 3, SF_U8 = 4 } sf_dtype;

/* Arithmetic mode of the matrix products (reported as "dtype" by bench.py):
 *   SF_COMPUTE_BF16   : bf16 operands, fp32 accumulate, one MFMA pass            (throughput)
 *   SF_COMPUTE_BF16X3 : x = xh+xl, w = wh+wl, xh*wh + xh*wl + xl*wh, fp32 acc   (fp32-accurate)
 * Residual stream, LayerNorm statistics, softmax and GELU are fp32 in both.                   */
typedef enum { SF_COMPUTE_BF16 = 0, SF_COMPUTE_BF16X3 = 1 } sf_compute;

/* Plain-old-data mirror of StreamformerConfig (reference models/configuration_streamformer.py:90-135). */
typedef struct {
  int32_t image_size, patch_size, num_channels, num_frames;
  int32_t hidden_size, num_hidden_layers, num_attention_heads, intermediate_size;
  int32_t hidden_act;              /* 0 = "gelu" (exact erf); 1 = "gelu_new"/tanh; 2 = "relu" */
  int32_t qkv_bias;                /* bool */
  int32_t enable_causal_temporal;  /* bool: causal (modeling:887) vs bidirectional (:894)     */
  int32_t add_lora_spatial;        /* bool: expect *_lora_{a,b}.weight (rank 32, modeling:1280) */
  float layer_norm_eps;
} sf_config;

/* ---- lifetime ------------------------------------------------------------------------------ */
/* replaces TimesformerMultiTaskingModelSigLIP.__init__ (modeling:1244-1258) */
int sf_create(const sf_config* cfg, int device, sf_encoder** out);
void sf_destroy(sf_encoder* enc);
const char* sf_last_error(void);
int sf_abi_version(void);

/* ---- weights: replaces from_pretrained()/load_state_dict() (modeling:1066-1075) -------------
 * `key` is the reference state_dict key, without any "timesformer." prefix.
 * The host buffer is borrowed only for the duration of the call.  Keys that are not weights of
 * this model return SF_ERR_UNKNOWN_KEY (callers may ignore it for buffers such as "...mask").   */
int sf_load_tensor(sf_encoder* enc, const char* key, const void* host_ptr, int dtype,
                   const int64_t* shape, int ndim);
/* Packs weights for the kernels and uploads them.  merge_lora: fold W += B*A (inference).
 * fuse_temporal_proj: fold temporal_dense o temporal_attention.output.dense into one matrix
 * (modeling:947-954 are two Linear layers with nothing in between).                            */
int sf_finalize_weights(sf_encoder* enc, int compute, int merge_lora, int fuse_temporal_proj);
/* number of weight tensors still missing (0 when complete); names via sf_last_error()          */
int sf_missing_weights(sf_encoder* enc);
/* TimesformerImageProcessor's arithmetic for SF_U8 frames (vqa_enc:1400-1447): y = (x * rescale - mean[c]) / std[c].
 * Defaults: mean = std = 0.5, rescale = 1/255.  The bicubic resize stays with the caller.          */
int sf_set_pixel_normalization(sf_encoder* enc, const float* mean, const float* std, int channels, float rescale);

/* ---- full-clip forward: replaces .forward(pixel_values) (modeling:1299-1354) -----------------
 * pixels_dev         [B,T,C,H,W] contiguous, dtype pixel_dtype: SF_F32 / SF_BF16 = normalised frames;
 *                    SF_U8 = raw frames, the image processor's rescale + normalize (see
 *                    sf_set_pixel_normalization) is fused into the patch-extraction kernel
 * last_hidden_dev    fp32 [B,T,N,D]   (post-LayerNorm tokens, modeling:1330,1342-1346)
 * pooler_dev         fp32 [B,T,D]     (modeling:1338-1340)
 * hidden_states_dev  NULL, or fp32 [L+1,B,T,N,D]: the input of every layer + the last output
 *                    (modeling:1031-1051), FRAME-major (the Python mirror permutes views)
 * pos_dev            NULL to use the loaded position table (needs H==W==image_size), else an
 *                    fp32 [N',D] table already resized on the host (modeling:380-411)
 */
int sf_workspace_bytes(sf_encoder* enc, int B, int T, int H, int W, size_t* out);
int sf_forward(sf_encoder* enc, const void* pixels_dev, int pixel_dtype, int B, int T, int H, int W,
               float* last_hidden_dev, float* pooler_dev, float* hidden_states_dev,
               const float* pos_dev, void* workspace_dev, size_t workspace_bytes, sf_stream stream);

/* Measurement hook: ONE forward (same arguments as sf_forward, no hidden states) with HIP events around the launches of four kernel
 * classes INSIDE it — 0: N = 768 residual projection at K = hidden_size, 1: the same at K = intermediate_size, 2: spatial attention,
 * 3: temporal attention.  Synchronises the stream.  out_ms_host[2 c] = mean milliseconds per launch of class c (the event pair also
 * spans the launch boundary in front of the kernel), out_ms_host[2 c + 1] = number of launches.  bench.py's `roofline` uses it.   */
int sf_forward_profile(sf_encoder* enc, const void* pixels_dev, int pixel_dtype, int B, int T, int H, int W,
                       float* last_hidden_dev, float* pooler_dev, void* workspace_dev, size_t workspace_bytes,
                       sf_stream stream, float* out_ms_host);

/* same, additionally returning the spatial attention probabilities of every layer
 * (output_attentions=True, modeling:703-716, 1052-1057): attentions_dev fp32 [L, B*T, heads, N, N]
 * (any N the attention kernels take: above 224 patches the streamed-keys kernel makes a second sweep).  */
int sf_forward_attentions(sf_encoder* enc, const void* pixels_dev, int pixel_dtype, int B, int T, int H, int W,
                          float* last_hidden_dev, float* pooler_dev, float* hidden_states_dev,
                          float* attentions_dev, const float* pos_dev, void* workspace_dev,
                          size_t workspace_bytes, sf_stream stream);

/* ---- the forward in three stages, for callers that interleave their own modules ------------------
 * (reference sub-module users: `blk(x, T, output_attentions=False)[0]` over encoder.layer in the
 * ViT-Adapter interaction blocks, models/modeling_timesformer_siglip_adapter.py:424-425; the
 * embeddings -> encoder -> post_layernorm -> head sequence of the video classifier,
 * downstream/AR/models/modeling_timesformer_video_classification.py:121-134).
 * hidden_dev: the caller's residual stream, fp32 FRAME-major [B,T,N,D] (the reference's patch-major
 * (B, N*T, D) is a permuted view of it); sf_layers updates it in place.
 * attentions_dev (optional): fp32 [layer_end-layer_begin, B*T, heads, N, N].  Workspace: sf_workspace_bytes. */
int sf_embed(sf_encoder* enc, const void* pixels_dev, int pixel_dtype, int B, int T, int H, int W,
             float* hidden_out_dev, const float* pos_dev, void* workspace_dev, size_t workspace_bytes,
             sf_stream stream);                                         /* TimesformerEmbeddingsSigLIP.forward, modeling:413-457 */
int sf_layers(sf_encoder* enc, float* hidden_dev, int B, int T, int H, int W, int layer_begin, int layer_end,
              float* attentions_dev, void* workspace_dev, size_t workspace_bytes, sf_stream stream);
                                                                        /* TimesformerLayerSigLIP.forward x (end-begin), modeling:934-1004 */
int sf_post_head(sf_encoder* enc, float* hidden_dev, int B, int T, int H, int W, float* last_hidden_dev,
                 float* pooler_dev, void* workspace_dev, size_t workspace_bytes, sf_stream stream);
                                                                        /* post_layernorm + head, modeling:1330-1340, 1141-1154;
                                                                           last_hidden_dev == NULL: head alone on normalised tokens */

/* ---- streaming forward with a temporal KV-cache ----------------------------------------------
 * replaces forward(..., past_key_values, use_cache=True) of the VideoQA copy
 * (reference downstream/VideoQA/llava/model/multimodal_encoder/timesformer_encoder.py:1316-1392;
 * cache update :517-518, offset causal mask :522-546, time-embedding offset :328-369).
 * The cache holds, per layer, the temporal K/V rows of every frame seen so far.                 */
int sf_cache_create(sf_encoder* enc, int B, int max_frames, int H, int W, sf_cache** out);
int sf_cache_reset(sf_cache* cache);            /* TimesformerVisionTower.clear_cache (:1528) */
int sf_cache_length(const sf_cache* cache);
/* Bounded-memory policy of a stream that outlives the cache (choose while the cache is empty): 0 (default) = stop at capacity
 * with SF_ERR_CAPACITY — the reference raises at config.num_frames (timesformer_encoder.py:343-348); 1 = SLIDING WINDOW: once
 * `max_frames` frames are cached every further single-frame call overwrites the oldest one, its temporal query sees the last
 * `max_frames` frames, and frames past the time-embedding table reuse its last row.  An extension beyond the reference
 * (SURVEY.md section 8 f-2 asks for a bounded-memory policy); sf_cache_length keeps counting the frames seen.                 */
int sf_cache_set_policy(sf_cache* cache, int policy);     /* DynamicCache.get_seq_length()              */
size_t sf_cache_bytes(const sf_cache* cache);
void sf_cache_destroy(sf_cache* cache);
int sf_stream_workspace_bytes(sf_encoder* enc, const sf_cache* cache, int T_new, size_t* out);
/* hidden_states_dev: NULL, or fp32 [L+1, B, T_new, N, D] — the new frames' input to every layer + the last output
 * (output_hidden_states=True together with use_cache=True: the vision tower's call form, vqa_enc:1536).
 * A cache is tied to the weight packing it was created against: after another sf_finalize_weights on the same
 * handle (or a new handle at a recycled address) sf_forward_stream returns SF_ERR_STATE instead of touching it. */
int sf_forward_stream(sf_encoder* enc, sf_cache* cache, const void* pixels_dev, int pixel_dtype,
                      int T_new, float* last_hidden_dev, float* pooler_dev, float* hidden_states_dev,
                      const float* pos_dev, void* workspace_dev, size_t workspace_bytes, sf_stream stream);
/* The same call with output_attentions (timesformer_encoder.py:494, 557, 633, 659, 720-754): attentions_dev receives the
 * spatial attention probabilities of the NEW frames, [L, B * T_new, heads, N, N] fp32, as sf_forward_attentions
 * returns them for whole clips.  Runs the launches eagerly (no graph replay).                                            */
int sf_forward_stream_attentions(sf_encoder* enc, sf_cache* cache, const void* pixels_dev, int pixel_dtype, int T_new,
                                 float* last_hidden_dev, float* pooler_dev, float* hidden_states_dev, float* attentions_dev,
                                 const float* pos_dev, void* workspace_dev, size_t workspace_bytes, sf_stream stream);

/* ---- independent stream positions in one batched cache --------------------------------------------
 * Each of the B streams (slabs) of a cache keeps its own position, so sessions may join, skip calls, restart and leave on their
 * own while sharing calls.  The entry points above advance ALL streams together and need them level: sf_cache_length is the
 * longest stream's count, sf_forward_stream on a cache whose streams differ returns SF_ERR_STATE, sf_cache_reset clears all.   */
int sf_cache_stream_length(const sf_cache* cache, int stream);      /* frames seen by one stream (0 for an id out of range) */
int sf_cache_reset_stream(sf_cache* cache, int stream);             /* that stream starts over; the others keep their positions */
/* Advances the `n_streams` DISTINCT streams named in the HOST array `streams` (slab indices of the cache), each from its own
 * position.  pixels_dev [n_streams, T_new, C, H, W]; last_hidden_dev [n_streams, T_new, N, D] and pooler_dev [n_streams, T_new, D]
 * (or NULL) come back in the order of `streams`.
 *   T_new == 1: any subset.  Same launch sequence as the lockstep call of n_streams rows, replayed from one captured graph per
 *     (n_streams, 64-key pass class of the longest stream, pooler, pixel type) whatever the positions are; at most 64 streams
 *     per call.  Under the sliding-window policy wrapped and fresh streams may share a call.
 *   T_new  > 1: n_streams == 1 only — the prefill of a stream that joins.
 * Capacity and the time-embedding table are checked for every named stream before anything is launched (SF_ERR_CAPACITY names
 * the stream; the cache is unchanged).  A workspace of sf_stream_workspace_bytes(enc, cache, T_new) — sized for the cache's full
 * batch — is sufficient for any subset.                                                                                          */
int sf_forward_stream_slots(sf_encoder* enc, sf_cache* cache, const void* pixels_dev, int pixel_dtype, int T_new,
                            const int* streams, int n_streams, float* last_hidden_dev, float* pooler_dev,
                            const float* pos_dev, void* workspace_dev, size_t workspace_bytes, sf_stream stream);

/* ---- parking a stream: its cached K/V out of the slab and back into any slab ------------------------
 * (HF's DynamicCache is plain tensors a caller may copy or offload; this is the way out of, and back into, library-owned memory.)
 * A stream that pauses, yields its slab, moves to another cache or process, or branches is exported to a caller-owned DEVICE blob and
 * imported later: into the same slab, another one, or a slab of another cache of the same weights, compute mode, resolution,
 * max_frames and policy (any batch size).  Importing one blob into two slabs forks the stream.
 * The blob holds the K and V columns of the frames the stream HOLDS (min(frames seen, max_frames)), all layers, in the cache's own
 * element type: [layers][frames_held * patches][2 * hidden_size], frames in RING-SLOT order.  Import puts every frame back into the
 * slot it came from and restores the frame count, so the stream's next position (time-embedding row, slot, keys seen) is the one
 * the source would have had and its continuation is bit-identical.  One kernel launch each way, on the caller's stream.        */
#define SF_STREAM_BLOB_KV1 0x31564b53u          /* "SKV1": K|V rows in slot order, uncompressed */
typedef struct {
  uint32_t format;                              /* SF_STREAM_BLOB_KV1                                              */
  int32_t compute;                              /* sf_compute of the packing: decides elem_bytes                   */
  int32_t frames_seen, frames_held;             /* the stream's count; min(frames_seen, max_frames) of them cached */
  int32_t max_frames, policy;                   /* of the cache (sf_cache_create, sf_cache_set_policy)             */
  int32_t H, W;                                 /* resolution of the cache                                         */
  int32_t layers, hidden_size, patches;         /* packed geometry: L, D, N                                        */
  int32_t elem_bytes;                           /* 2 (bf16) or 4 (fp32)                                            */
  uint64_t packing;                             /* fingerprint of the configuration and weights that computed the K/V;
                                                   equal for equal weights, in any process                        */
  uint64_t blob_bytes;                          /* layers * frames_held * patches * 2 * hidden_size * elem_bytes   */
} sf_cache_stream_meta;
/* bytes of that stream's blob as it stands (0 for a stream that holds nothing) */
int sf_cache_stream_blob_bytes(const sf_cache* cache, int stream, size_t* out);
/* blob_dev: 16-byte aligned device buffer of exactly `bytes` = sf_cache_stream_blob_bytes; meta_out: HOST, filled in.  The stream
 * itself is left as it is (release or reset it separately).                                                                    */
int sf_cache_export_stream(sf_encoder* enc, sf_cache* cache, int stream, void* blob_dev, size_t bytes,
                           sf_cache_stream_meta* meta_out, sf_stream s);
/* Everything is checked before anything is launched or changed; a refusal names the field and leaves the slab untouched:
 * SF_ERR_INVALID for a stream id out of range, another format, compute mode, resolution, max_frames, policy or geometry, an
 * inconsistent frame count or a wrong byte count; SF_ERR_STATE for a blob computed by other weights (`packing`), or a cache of an
 * earlier packing of the encoder.  Restoring into a cache of another max_frames is not supported.                              */
int sf_cache_import_stream(sf_encoder* enc, sf_cache* cache, int stream, const void* blob_dev, size_t bytes,
                           const sf_cache_stream_meta* meta, sf_stream s);

/* ---- single operators (each is one kernel of the path; used by the parity tests) ----------- */
/* nn.LayerNorm(D, eps) rows (modeling:860-865,878-880,1251): x fp32 [rows,D] -> y fp32 [rows,D] */
int sf_op_layernorm(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* y_dev,
                    int rows, int D, float eps, sf_stream stream);
/* nn.Linear (+ optional exact-erf GELU, + optional residual): y = act(x W^T + b) [+ alpha*() + r]
 * x fp32 [M,K], w fp32 [N,K], b fp32 [N] or NULL, resid fp32 [M,N] or NULL, y fp32 [M,N].
 * Operands are rounded/split on device exactly as the encoder does for `compute`.               */
int sf_op_linear(const float* x_dev, const float* w_dev, const float* b_dev, const float* resid_dev,
                 float alpha, int gelu, float* y_dev, int M, int N, int K, int compute,
                 void* workspace_dev, size_t workspace_bytes, sf_stream stream);
size_t sf_op_linear_workspace_bytes(int M, int N, int K);
/* One forward GEMM, C[M,N] = A[M,K] W[N,K]^T + fused epilogue, with every field the forward sets (csrc/sf_common.h, SfGemmArgs, field
 * for field and under the same names), on operand planes the CALLER rounded: bf16 bit patterns, hi = bf16(v), lo = bf16(v - hi).
 *   split        0: bf16 mode (a_lo = w_lo = NULL); 1: the three-product accurate mode
 *   epi          0 F32: out_f32 = acc + bias;  1 BF16 / 2 ACT_BF16: out_hi (+ out_lo) = [act](acc + bias), act 0 erf GELU, 1 tanh GELU,
 *                2 ReLU;  3 RESID_F32: resid + alpha (acc + bias), resid fp32 (row m % resid_mod of a table when resid_mod > 0) to
 *                out_f32, or planes resid_hi + resid_lo (+ resid_lo2) to out_hi + out_lo (+ out_lo2);  4 EMBED_F32: out_f32 = acc + bias
 *                + pos[m % Np] + time_rows[(m / Np) % Tn]
 *   ldc          row pitch, in elements, of every output AND of resid / resid_hi / resid_lo / resid_lo2 (>= N; pos, time_rows: N)
 *   grp_*        grp_rows > 0: row m is written at (m / grp_rows) * grp_stride + grp_off + m % grp_rows
 *   ln_stats_out producer of a LayerNorm fold: {sum x, sum x^2} pairs of the new residual rows, 4 floats per row, 8 when ln_stats_wide
 *   ln_stats, ln_s, ln_eps   consumer: y = rstd (acc - mean ln_s[n]) + bias, w = W gamma, ln_s[n] = sum_k bf16(w)[n,k], bias = b + W beta;
 *                ln_inkernel = 1: no ln_stats, the kernel sums the rows of A it reads
 * family 0 dispatches as the forward does; 1 skinny, 2 tile, 3 panel, 4 256^2, 5 128^2 name a family, which runs only if its own
 * support check accepts the call.  *family_taken (may be NULL): what ran; 6 = the 256-column kernel + a 128-column tail on the 128^2
 * kernel.  A call no kernel takes, a null buffer its epilogue needs, or a field the chosen kernel does not read is SF_ERR_INVALID
 * with nothing launched.                                                                                                        */
typedef struct {
  int32_t split;
  const uint16_t* a_hi; const uint16_t* a_lo;      /* [M,K] */
  const uint16_t* w_hi; const uint16_t* w_lo;      /* [N,K] */
  const float* bias;                               /* [N] or NULL */
  int32_t M, N, K, epi, act;
  float alpha;
  const float* resid; int32_t resid_mod;
  const uint16_t* resid_hi; const uint16_t* resid_lo; const uint16_t* resid_lo2;
  const float* pos; const float* time_rows; int32_t Np, Tn;
  float* out_f32; uint16_t* out_hi; uint16_t* out_lo; uint16_t* out_lo2; int32_t ldc;
  int32_t grp_rows, grp_stride, grp_off;
  float* ln_stats_out; const float* ln_stats; const float* ln_s; float ln_eps; int32_t ln_stats_wide, ln_inkernel;
} sf_gemm_desc;
int sf_op_gemm(const sf_gemm_desc* d, int family, int* family_taken, sf_stream stream);
/* softmax(q k^T / sqrt(d)) v per head over `groups` independent sequences
 * (modeling:688-717 spatial; :575-615 temporal with causal=1 and past offset).
 * qkv fp32 [groups, Lq|Lk, 3*D] packed as the qkv Linear emits it; ctx fp32 [groups, Lq, D].
 * Spatial: seq stride = rows are contiguous tokens.  Temporal goes through the same entry with
 * `row_stride` (in rows) between consecutive sequence positions.                                */
int sf_op_attention(const float* qkv_dev, float* ctx_dev, int groups, int L, int heads, int head_dim,
                    int causal, int temporal_layout, int N_tokens, int compute,
                    void* workspace_dev, size_t workspace_bytes, sf_stream stream);
size_t sf_op_attention_workspace_bytes(int groups, int L, int heads, int head_dim);
/* Which spatial-attention kernel sf_op_attention(frames, N, heads, head_dim, ..., temporal_layout = 0, compute) runs, without running
 * it; `probs` / `dropout` > 0 ask the same for a call that also wants the probabilities (output_attentions) / dropout on them, which
 * the encoder and the training step make.  Nothing is launched and no device memory is touched.
 * *route: 0 no kernel takes the call, 1 the generic kernel (head_dim != 64), 2 / 3 N > 224 on bf16 / fp32 rows, 4 DMA-staged bf16 rows,
 * 5 the same with 13 key tiles at compile time (193 .. 208 tokens), 6 the same with dropout, 7 / 8 DMA-staged hi + lo planes / with 13
 * tiles, 9 / 10 register-staged bf16 / fp32 rows.  *qsplit: workgroups per (frame, head).  *lds: dynamic LDS bytes of the launch.
 * Any of the three may be NULL.                                                                                                      */
int sf_op_spatial_attention_plan(int frames, int N, int heads, int head_dim, int compute, int probs, float dropout,
                                 int* route, int* qsplit, size_t* lds);
/* Temporal attention over a KV-cache the CALLER built: the streaming step (Tq = 1), chunked prefill (Tq > 1 behind a past), the position
 * read from device memory and the table of a ragged call — the kernels of a stream, without an encoder around them.
 * cache fp32 [slabs, cap, N_tokens, 3*D], q | k | v per row (the encoder's cache layout); it is converted to what `compute` keeps in a real
 * stream (bf16 rows; the accurate mode reads the fp32 rows as they are).  ctx fp32 [B * Tq * N_tokens, D].
 * Sequence (b, n): query t < Tq is row q_t0 + t of slab b, keys and values are rows 0 .. Tk - 1 of that slab; causal: key j is visible
 * to query t iff j <= t_past + t.  Rows the call does not name are not read.
 *   pos_dev  (Tq = 1) two ints {slot, tk} in device memory: the query row and the number of keys, all of them visible
 *   tab      (Tq = 1) B entries in device memory: sequence b reads slab tab[b].stream, query row tab[b].slot, tab[b].tk keys, all
 *            visible; its context row stays row b.  With either, Tk bounds every tk and picks the kernel instance; t_row is unused.
 * *route_out (may be NULL): the kernel and instance that ran — 1..3 single query fp32 rows (64 / 128 / 256 keys), 4..5 single query
 * bf16 whole lines (64 / 128), 6..8 single query bf16 lane = key (64 / 128 / 256), 9 DMA-staged bf16, 10 DMA-staged planes (not reached
 * from here), 11..14 MFMA fp32 rows (32 / 64 / 128 / 256 keys), 15..18 MFMA bf16 rows, 19 the generic kernel (head_dim != 64).
 * *waves_out (may be NULL): waves per workgroup of that launch.
 * SF_ERR_INVALID, with nothing launched, for query rows or keys outside the cache, a device position outside it, tab / pos_dev with
 * Tq != 1 or on a route that does not read them, and every call no kernel takes.                                                  */
typedef struct { int32_t stream, t_row, slot, tk; } sf_stream_slot;
int sf_op_attention_cached(const float* cache_dev, float* ctx_dev, int slabs, int cap, int N_tokens, int heads, int head_dim,
                           int compute, int B, int Tq, int Tk, int q_t0, int t_past, int causal, const int* pos_dev,
                           const sf_stream_slot* tab_dev, int* route_out, int* waves_out,
                           void* workspace_dev, size_t workspace_bytes, sf_stream stream);
size_t sf_op_attention_cached_workspace_bytes(int slabs, int cap, int N_tokens, int heads, int head_dim, int B, int Tq);

/* ---- loss heads of the multitask pre-training step (BASELINE config #3) ---------------------
 * retrieval: TimesformerVideoRetrievalHead.forward + SigLipLoss._loss (modeling:2324-2351,221-237)
 * localization: TimesformerUniversalLocalizationHead.forward (modeling:2238-2282)
 * pooler fp32 [B,T,D]; text fp32 [Bt,D] (un-normalised); label_emb fp32 [L,D]; labels int32 [B,T]
 * (-1 = background).  pos_offset: column of `text` that is row 0's positive (rank*B when `text` is
 * the all-gathered [world*B, D] table, modeling:250-280; -1 = negatives only).
 * logit_scale_dev / logit_bias_dev: DEVICE pointers to one fp32 each (the heads' parameters, modeling:1363-1364;
 * in a training step they point into the flat parameter buffer, so no host round trip sits between
 * forward and backward).  workspace_dev: caller-owned scratch of sf_loss_workspace_bytes(B, T) bytes
 * (per-row partial sums, reduced in a fixed order: the losses are bit-reproducible).
 * There is no limit on Bt (the text table is walked in chunks); D <= 2048, L <= 4096 (SF_ERR_CAPACITY).
 * Outputs: loss_dev fp32 [1]; grad_pooler_dev fp32 [B,T,D] or NULL;
 * grad_scalars_dev fp32 [2] = d loss / d (logit_scale, logit_bias) or NULL.                     */
size_t sf_loss_workspace_bytes(int B, int T);
int sf_retrieval_loss(const float* pooler_dev, const float* text_dev, int B, int T, int D, int Bt,
                      int pos_offset, const float* logit_scale_dev, const float* logit_bias_dev,
                      float* loss_dev, float* grad_pooler_dev, float* grad_scalars_dev,
                      void* workspace_dev, size_t workspace_bytes, sf_stream stream);
int sf_localization_loss(const float* pooler_dev, const float* label_emb_dev, const int32_t* labels_dev,
                         int B, int T, int D, int L, const float* logit_scale_dev, const float* logit_bias_dev,
                         float* loss_dev, float* grad_pooler_dev, float* grad_scalars_dev,
                         void* workspace_dev, size_t workspace_bytes, sf_stream stream);

/* ---- caption-driven heads ---------------------------------------------------------------------
 * Temporal grounding, TimesformerTemporalGroundingHead.forward (modeling:2373-2397): ONE caption per clip supervises every frame.
 *   logit[b,t] = exp(logit_scale) * <p[b,t] / |p[b,t]|, c[b] / |c[b]|> + logit_bias
 *   y[b,t]     = -1 where labels[b,t] == 0, else labels[b,t] as given (the reference's masked_fill; no host check)
 *   loss       = -sum_{b,t} logsigmoid(y * logit) / B
 * pooler_dev fp32 [B,T,D]; text_dev fp32 [B,D] (un-normalised, no gradient: frozen text tower); labels_dev fp32 [B,T].
 * Conventions of sf_localization_loss: DEVICE scalars, workspace of sf_loss_workspace_bytes(B, T), bit-reproducible.
 * Outputs: loss_dev fp32 [1]; grad_pooler_dev fp32 [B,T,D] or NULL; grad_scalars_dev fp32 [2] or NULL; logits_out_dev fp32 [B,T] or NULL. */
int sf_grounding_loss(const float* pooler_dev, const float* text_dev, const float* labels_dev, int B, int T, int D,
                      const float* logit_scale_dev, const float* logit_bias_dev, float* loss_dev, float* grad_pooler_dev,
                      float* grad_scalars_dev, float* logits_out_dev, void* workspace_dev, size_t workspace_bytes,
                      sf_stream stream);
/* Evaluation output of the referring segmentation head (modeling:2004-2018): dense caption-to-patch logits
 *   out[m, j] = exp(logit_scale) * <x[m] / |x[m]|, text[j] / |text[j]|> + logit_bias
 * x_dev fp32 [M,D] (the dense projection's output rows, 16-byte aligned), text_dev fp32 [n,D] (un-normalised), out_dev fp32 [M,n].
 * fp32 arithmetic throughout, one pass over x for tables of up to 128 KB (42 captions at D = 768), no workspace, bit-reproducible.
 * D a multiple of 4; capacity (SF_ERR_CAPACITY): n <= 64, D <= 2048.                                                              */
int sf_dense_text_logits(const float* x_dev, const float* text_dev, int M, int D, int n, const float* logit_scale_dev,
                         const float* logit_bias_dev, float* out_dev, sf_stream stream);

/* ---- spatial task: mask loss of the video instance segmentation head ------------------------
 * TimesformerUniversalVideoInstanceSegmentationHead.forward, training branch (modeling:1829-1916), per clip i:
 *   z[t,n,l] = <x[i,t,n] / |x[i,t,n]|, E_i[l]> * exp(logit_scale) + logit_bias
 *   logits   = bilinear resize of z viewed as [T, L_i, P, P] to (H, W_i), align_corners = False   (F.interpolate)
 *   loss_i   = mean over the pixels whose target is in [0, L_i) of logsumexp_l(logits) - logits[target]
 *              (0, and no gradient, for a clip without such a pixel);   loss = (1 / B) sum_i loss_i
 * evaluated WITHOUT the upsampled tensor (csrc/sf_mask_loss.hip): the workspace holds patch logits, never pixels.
 * x_dev fp32 [B,T,N,D] (N = P * P patch tokens, frame-major).  The per-clip arguments are HOST arrays of B entries:
 * label_emb_dev[i] = device fp32 [num_labels[i], D], used as given; mask_dev[i] = device int32 [T, H, mask_width[i]],
 * any value outside [0, num_labels[i]) (-1 by convention) = ignore.  logit_scale_dev / logit_bias_dev: DEVICE pointers to one
 * fp32 each.  Outputs: loss_dev fp32 [1]; grad_x_dev fp32 [B,T,N,D] or NULL; grad_scalars_dev fp32 [2] =
 * d loss / d (logit_scale, logit_bias) or NULL.  Bit-reproducible (no atomics); the valid-pixel count stays on the device.
 * Capacity (SF_ERR_CAPACITY): N <= 224, num_labels <= 128, D <= 2048, mask_width <= min(4 H, 2048).
 * workspace: the query below with L_max = the largest num_labels[i].                                                    */
size_t sf_mask_loss_workspace_bytes(int B, int T, int N, int L_max);
int sf_mask_loss(const float* x_dev, int B, int T, int N, int D, const float* const* label_emb_dev,
                 const int32_t* num_labels, const int32_t* const* mask_dev, const int32_t* mask_width, int H,
                 const float* logit_scale_dev, const float* logit_bias_dev, float* loss_dev, float* grad_x_dev,
                 float* grad_scalars_dev, void* workspace_dev, size_t workspace_bytes, sf_stream stream);

/* Dense feature projection of the same head (modeling:1786-1795) on M = B*T*N token rows, in the training arithmetic
 * (bf16 operands, fp32 accumulation):  a = x Wv^T + bv;  y = a Wo^T + bo;  out = y + fc2(gelu(fc1(LayerNorm(y)))).
 * params: HOST array of 10 device fp32 pointers in the order w_v.weight [D,D], w_v.bias, v_proj.weight [D,D], v_proj.bias,
 * head_layernorm.weight, head_layernorm.bias, head_mlp.fc1.weight [I,D], fc1.bias, head_mlp.fc2.weight [D,I], fc2.bias
 * (erf GELU).  forward keeps what backward needs in the caller's workspace; backward must follow forward on the same
 * workspace and OVERWRITES d_x_dev fp32 [M,D] and the ten gradient tensors grads[i] (same order and shapes).
 * D a multiple of 64; I is zero-padded to a multiple of 64 inside.                                                    */
size_t sf_dense_head_workspace_bytes(int M, int D, int I);
int sf_dense_head_forward(const float* x_dev, int M, int D, int I, float eps, const float* const* params,
                          float* out_dev, void* workspace_dev, size_t workspace_bytes, sf_stream stream);
int sf_dense_head_backward(const float* d_out_dev, int M, int D, int I, float eps, const float* const* params,
                           float* d_x_dev, float* const* grads, void* workspace_dev, size_t workspace_bytes,
                           sf_stream stream);

/* ---- training step (BASELINE configs #3 / #4) ------------------------------
 * Replaces, for one micro-batch: the autograd graph of TimesformerMultiTaskingModelSigLIP.forward
 * (modeling:1299-1354) as driven by train_one_epoch_multi_task (tools/finetune_tools.py:395-573:
 * forward -> task-head loss -> loss/update_freq -> backward -> optimizer step every update_freq
 * micro-steps) and torch.optim.AdamW as optim_factory.py:59-104 configures it (no weight decay for
 * 1-D parameters and "*.bias"; frozen parameters skipped).
 *
 * State layout: ALL parameters live in ONE caller-owned flat fp32 device buffer (so the gradient
 * buffer of the same layout can be all-reduced by RCCL in a few large slices); each
 * segment starts on a multiple of 64 floats.  Trainable parameters come first, in model order
 * (embeddings, layers 0..L-1, post_layernorm, head, extra scalars), frozen ones (the spatial
 * qkv / output.dense base weights when freeze_spatial=1, modeling:1284-1297) after them.
 * Names are the reference state_dict keys; `extra.<i>` are caller-defined trainable
 * scalars (task heads' logit_scale / logit_bias, modeling:1363-1364).
 * Compute mode is SF_COMPUTE_BF16 (bf16 MFMA operands, fp32 accumulation, fp32 master weights,
 * fp32 residual stream and its gradient).                                                        */
typedef struct sf_trainer sf_trainer;
int sf_trainer_create(const sf_config* cfg, int device, int freeze_spatial, int n_extra, sf_trainer** out);
void sf_trainer_destroy(sf_trainer* tr);
int sf_trainer_num_params(const sf_trainer* tr);
/* shape_out: up to 4 dims; trainable/decay: the optim_factory.py:70-77 grouping                 */
int sf_trainer_param_info(const sf_trainer* tr, int index, char* name_out, int name_cap, int64_t* offset_out,
                          int64_t* numel_out, int64_t* shape_out, int* ndim_out, int* trainable_out,
                          int* decay_out);
/* total floats of the flat buffer, and the length of its trainable prefix                        */
int sf_trainer_total_floats(const sf_trainer* tr, int64_t* total_out, int64_t* trainable_out);
/* backward runs in stages so the caller can all-reduce finished gradient slices while earlier
 * layers are still being differentiated: stage 0 = pooling head + post_layernorm,
 * stage 1+k = layer L-1-k, stage L+1 = embeddings.  The slice [offset, offset+numel) of the
 * gradient buffer is final when the stage returns.                                              */
int sf_trainer_num_stages(const sf_trainer* tr);
int sf_trainer_stage_range(const sf_trainer* tr, int stage, int64_t* offset_out, int64_t* numel_out);
/* fp32 master -> bf16 working weights (row-major and transposed copies, LoRA merged as
 * W + B A (modeling:541-545), temporal_dense scaled by tanh(gate) (modeling:954-958)).  Call after
 * every optimizer step; params_dev must stay valid until the next call.                          */
int sf_trainer_sync_weights(sf_trainer* tr, const float* params_dev, sf_stream stream);
int sf_trainer_workspace_bytes(const sf_trainer* tr, int B, int T, size_t* out);
/* drop_path (stochastic depth, modeling:460-486, 846-856) of the forwards that follow: scales_dev = DEVICE array, per layer
 * [B*N temporal | B*T spatial | B MLP] factors (0 = branch dropped for that sample group, 1 / keep_prob = kept), L layers back to
 * back; the reference draws one Bernoulli per dim-0 entry of the tensor each branch returns ((B*N,T,D), (B*T,N,D), (B,N*T,D)).
 * The backward of a forward applies the factors that forward used.  NULL = none (eval, or drop_path_rate 0).  The array is
 * caller-owned and must stay valid until the matching backward has run.                                                        */
int sf_trainer_set_drop_path(sf_trainer* tr, const float* scales_dev, int B, int T);
/* Dropout of the forwards that follow (config.hidden_dropout_prob / attention_probs_dropout_prob; reference sites modeling:374, 378
 * (position / time embeddings), 752 / 761 (both SelfOutput projections), 822 (MLP activation), 835 (MLP output), 556 / 603 / 669 / 705
 * (attention probabilities)).  Masks are COUNTER-BASED: element idx of site k is kept iff hash(idx, hash(k, seed)) < keep * 2^32 and
 * scaled by 1 / keep, so no mask tensor exists and the backward of a forward replays the masks from the seed that forward used
 * (the CPU oracle evaluates the same integer hash).  0 / 0 switches dropout off (eval).                                           */
int sf_trainer_set_dropout(sf_trainer* tr, float hidden_p, float attention_p, uint32_t seed);
/* Non-finite guard of the optimizer step (tools/finetune_tools.py:533-541 stops the run on a non-finite loss; the GradScaler of
 * utils.py:515-551 skips a step whose gradients hold inf / NaN).  flag_dev = DEVICE int32[2], caller-owned and zero-initialised:
 * every sf_trainer_adamw_step that follows checks sum g^2 of the gradient (and *loss_dev, a device float, when not NULL) ON THE
 * DEVICE; if either is inf / NaN the update is skipped as a whole (parameters and moments untouched, gradients still cleared
 * when zero_grads) and flag_dev = {1 (sticky), number of skipped steps}.  No host synchronisation: the caller reads the flag at
 * its next host touch.  flag_dev = NULL switches the guard off.                                                              */
int sf_trainer_set_nonfinite_guard(sf_trainer* tr, int32_t* flag_dev, const float* loss_dev);
/* forward with every activation the backward needs kept in the workspace                         */
int sf_trainer_forward(sf_trainer* tr, const void* pixels_dev, int pixel_dtype, int B, int T,
                       float* last_hidden_dev, float* pooler_dev, void* workspace_dev,
                       size_t workspace_bytes, sf_stream stream);
/* grads_dev += d loss / d params for stages [stage_first, stage_last]; d_pooler_dev fp32 [B,T,D],
 * d_last_hidden_dev fp32 [B,T,N,D] or NULL.  Must follow sf_trainer_forward on the same workspace. */
int sf_trainer_backward(sf_trainer* tr, const float* d_pooler_dev, const float* d_last_hidden_dev,
                        float* grads_dev, int stage_first, int stage_last, void* workspace_dev,
                        size_t workspace_bytes, sf_stream stream);
/* torch.optim.AdamW update of the trainable prefix; `step` counts from 1; grad_scale multiplies
 * the gradient first (1/world for averaging).  grad_sumsq_dev (optional, DEVICE pointer to the
 * output of sf_trainer_grad_sumsq): torch.nn.utils.clip_grad_norm_(max_norm = clip_norm) applied
 * inside the kernel — total_norm = sqrt(sum) * grad_scale, coefficient min(1, clip_norm / (total_norm + 1e-6)) —
 * so clipping needs no host synchronisation.  zero_grads != 0: grads_dev is cleared by the same pass
 * (optimizer.zero_grad(), tools/finetune_tools.py:566).                                            */
int sf_trainer_adamw_step(sf_trainer* tr, float* params_dev, float* grads_dev, float* exp_avg_dev,
                          float* exp_avg_sq_dev, int step, float lr, float beta1, float beta2, float eps,
                          float weight_decay, float grad_scale, const float* grad_sumsq_dev, float clip_norm,
                          int zero_grads, sf_stream stream);
/* Per-slot step counts of the `n_extra` scalar slots ("extra.<i>": the task heads' logit_scale / logit_bias) for
 * the adamw steps that follow: steps_host[i] > 0 = update slot i with bias corrections of that step count,
 * 0 = leave slot i untouched (its gradient is still cleared).  torch.optim.AdamW skips parameters whose .grad is
 * None and counts `step` per parameter: a head whose task was not scheduled in an accumulation window gets
 * neither weight decay nor moment decay (tools/finetune_tools.py:560-570 + zero_grad(set_to_none)).  n = 0
 * (or steps_host NULL) restores the default: every slot follows the step passed to sf_trainer_adamw_step.     */
int sf_trainer_set_extra_steps(sf_trainer* tr, const int32_t* steps_host, int n);
/* out_dev[0] = sum of squares of the trainable gradient prefix (for clip_grad_norm_)             */
int sf_trainer_grad_sumsq(sf_trainer* tr, const float* grads_dev, float* out_dev, sf_stream stream);

/* single backward operators (parity tests).  bf16 tensors are raw uint16 device buffers.         */
/* C[N1,N2] = alpha * dY^T X  (+ C) : dy [M,ldy], x [M,ldx] bf16; out fp32 [N1,ldo];
 * dbias_dev (optional) fp32 [N1] += alpha * column sums of dY (the bias gradient of the same Linear) */
int sf_op_wgrad(const void* dy_dev, int ldy, const void* x_dev, int ldx, int M, int N1, int N2, float alpha,
                int accumulate, float* out_dev, int ldo, float* dbias_dev, sf_stream stream);
/* attention backward; layout 0 = spatial (nseq sequences of L consecutive token rows),
 * 1 = temporal (token row of (b, t, n) = (b*L + t)*seq_rows + n, nseq = B*seq_rows).
 * qkv/d_qkv bf16 [rows, 3D], o/d_o bf16 [rows, D].                                               */
int sf_op_attention_bwd(const void* qkv_dev, const void* o_dev, const void* d_o_dev, void* d_qkv_dev, int layout,
                        int nseq, int L, int seq_rows, int heads, int causal, sf_stream stream);
/* the same at any head_dim that is a multiple of 8 up to 128 (D = heads * head_dim, scale head_dim^-0.5): 64 runs the kernels of
 * sf_op_attention_bwd (bit-identical results), other widths the generic fp32 kernel (spatial L <= 224, temporal L <= 32)          */
int sf_op_attention_bwd_hd(const void* qkv_dev, const void* o_dev, const void* d_o_dev, void* d_qkv_dev, int layout,
                           int nseq, int L, int seq_rows, int heads, int head_dim, int causal, sf_stream stream);
/* LayerNorm backward: dx = g_in + dLN(x; dy), d_gamma/d_beta accumulated                          */
int sf_op_layernorm_bwd(const float* x_dev, const float* dy_dev, const float* gamma_dev, const float* g_in_dev,
                        float* dx_dev, float* d_gamma_dev, float* d_beta_dev, int rows, int D, float eps,
                        sf_stream stream);

/* ---- SigLIP text tower: captions and class prompts from token ids ----------------------------------
 * Replaces the frozen `self.text_encoder = SiglipTextModel.from_pretrained(...)` of the multitask wrapper (modeling:1365-1375) as the
 * task heads call it: `self.text_encoder(ids)[1]` / `self.text_encoder(**tokenizer_output)[1]` (modeling:1680, 1756, 1997, 2104, 2217,
 * 2315, 2385).  Inference only.  Pre-LN layers as in SigLIP: LN1 -> packed qkv -> attention -> out_proj + residual -> LN2 -> fc1 + act ->
 * fc2 + residual, then final_layer_norm; the Linears run on the encoder's GEMM kernels in the `compute` mode of sf_text_finalize,
 * residual stream, LayerNorm, softmax and the pooled head in fp32 in both.  Kernels: csrc/sf_text.hip.                           */
typedef struct sf_text sf_text;
typedef struct {
  int32_t vocab, positions;        /* vocab_size, max_position_embeddings (<= 128: SF_ERR_CAPACITY)            */
  int32_t hidden, layers, heads;   /* width rules of sf_create: hidden % 64 == 0, head_dim a multiple of 8 in 8..128 */
  int32_t intermediate;            /* any positive size (zero-padded to a multiple of 64 at upload)              */
  int32_t projection;              /* projection_size: rows of `head`                                            */
  int32_t act;                     /* 0 = "gelu" (erf); 1 = "gelu_pytorch_tanh" (SigLIP); 2 = "relu"             */
  float eps;                       /* layer_norm_eps                                                             */
} sf_text_config;
int sf_text_create(const sf_text_config* cfg, int device, sf_text** out);
void sf_text_destroy(sf_text* text);
/* `key`: a key of HF's SiglipTextModel state dict, with or without a leading "text_model." (embeddings.token_embedding.weight,
 * embeddings.position_embedding.weight, encoder.layers.<i>.{layer_norm1,layer_norm2,self_attn.{q,k,v,out}_proj,mlp.fc1,mlp.fc2}.{weight,bias},
 * final_layer_norm.*, head.*).  dtype SF_F32 / SF_F64 / SF_BF16; the host buffer is borrowed for the call.  q_proj, k_proj and v_proj
 * are packed into one [3 hidden, hidden] Linear by sf_text_finalize.  Other keys: SF_ERR_UNKNOWN_KEY.                              */
int sf_text_load_tensor(sf_text* text, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
int sf_text_finalize(sf_text* text, int compute);
int sf_text_missing_weights(sf_text* text);       /* count; names via sf_last_error() */
int sf_text_workspace_bytes(sf_text* text, int B, int L, size_t* out);
/* ids_dev int32 [B, L]; an id outside [0, vocab) is clamped by the kernel (memory safety only: check ids on the host).
 * mask_dev uint8 [B, L] or NULL: the tokenizer's attention_mask, 0 = padding.  A masked key gets zero weight for every query of its
 * caption (HF's additive -inf); query rows of padded positions are still computed.  Every caption needs at least one valid key: the
 * mask lives on the device, so that check belongs to the caller (the Python layer raises); the kernel writes zeros for such a caption
 * instead of dividing by a zero sum.
 * last_hidden_dev fp32 [B, L, hidden] or NULL (final_layer_norm of every row); pooled_dev fp32 [B, projection] = head(final_layer_norm(
 * row L - 1)) whatever the mask says, as SiglipTextModel pools.  workspace: 256-byte aligned, sf_text_workspace_bytes(B, L).
 * Refused before anything is launched: L > positions and activations past 2^31 - 1 elements (SF_ERR_CAPACITY), bad shapes (SF_ERR_INVALID). */
int sf_text_forward(sf_text* text, const int32_t* ids_dev, const uint8_t* mask_dev, int B, int L, float* last_hidden_dev,
                    float* pooled_dev, void* workspace_dev, size_t workspace_bytes, sf_stream stream);
/* Class-prompt tables (modeling:2207-2223): the same forward on B = labels * group captions, prompts of one label consecutive; every
 * pooled row is L2-normalised, each `group` consecutive rows are averaged and the mean is normalised again: table_dev fp32
 * [B / group, projection], unit-norm rows.                                                                                        */
int sf_text_forward_groups(sf_text* text, const int32_t* ids_dev, const uint8_t* mask_dev, int B, int L, int group, float* table_dev,
                           void* workspace_dev, size_t workspace_bytes, sf_stream stream);
/* single operators of the tower (parity tests).
 * attention: ctx[b, l, h] = softmax(head_dim^-0.5 q k^T + key_mask) v, non-causal; qkv_dev fp32 [B * L, 3 * heads * head_dim] (q | k | v
 * columns), mask_dev uint8 [B, L] or NULL, ctx_dev fp32 [B * L, heads * head_dim]; L in 1..128, head_dim a multiple of 8 in 8..128;
 * fp32 arithmetic, bit-reproducible.
 * pool: x_dev fp32 [B * L, D] -> row L - 1 of every caption -> LayerNorm(gamma, beta, eps) (both NULL: rows used as they are) ->
 * w_dev [P, D] + bias_dev [P] (or NULL).  group == 0: out_dev [B, P].  group >= 1: out_dev [B / group, P] = normalised means of the
 * normalised rows, scratch_dev fp32 [B, P] required.                                                                              */
int sf_op_text_attention(const float* qkv_dev, const uint8_t* mask_dev, float* ctx_dev, int B, int L, int heads, int head_dim,
                         sf_stream stream);
int sf_op_text_pool(const float* x_dev, int B, int L, int D, const float* gamma_dev, const float* beta_dev, float eps,
                    const float* w_dev, const float* bias_dev, int P, int group, float* out_dev, float* scratch_dev, sf_stream stream);

/* ---- Video-LLM connector: projector, spatial pooling and newline tokens ---------------------------
 * The tail between the vision tower's features and the language model's input embeddings in the reference's VideoQA model
 * (llava_arch: mm_projector :213, get_2dPool :171-190, the newline placement :261-288 and :351-390): feats [F, P * P, in_dim] ->
 * rows [tokens, out_dim].  Inference only.  The Linears run on the encoder's GEMM kernels in the `compute` mode of
 * sf_connector_finalize (weights rounded / split once, there); the average and bilinear pools are applied in FRONT of the last
 * Linear, with which they commute (their taps sum to 1), so that GEMM runs on P'^2 rows per frame; max keeps the reference's order.
 * Kernel: csrc/sf_connector.hip.                                                                                                  */
typedef struct sf_connector sf_connector;
typedef struct {
  int32_t in_dim, out_dim;     /* mm_hidden_size, LLM hidden_size; both % 64 == 0, else SF_ERR_INVALID  */
  int32_t depth;               /* Linears in the projector: 0 = identity (in_dim == out_dim), 1 = "linear", n = "mlp{n}x_gelu" (erf GELU between) */
  int32_t pool_mode;           /* 0 none, 1 average, 2 max, 3 bilinear                                   */
  int32_t pool_stride;         /* >= 1; 1 forces pool_mode none                                           */
  int32_t newline;             /* 0 no_token, 1 one_token (one row after the last frame), 2 frame, 3 grid */
} sf_connector_config;
int sf_connector_create(const sf_connector_config* cfg, int device, sf_connector** out);
void sf_connector_destroy(sf_connector* conn);
/* `key`, with or without a leading "model.": mm_projector.{0,2,4,...}.{weight,bias} (the nn.Sequential indices of the reference
 * builder, depth >= 2), mm_projector.{weight,bias} (depth 1), image_newline [out_dim] (required only when newline != 0).  dtype
 * SF_F32 / SF_F64 / SF_BF16; the host buffer is borrowed for the call.  Other keys: SF_ERR_UNKNOWN_KEY; a wrong shape: SF_ERR_INVALID. */
int sf_connector_load_tensor(sf_connector* conn, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
/* Uploads the weights to the handle's device.  Makes that device current (hipSetDevice) and leaves it current on return.          */
int sf_connector_finalize(sf_connector* conn, int compute);
int sf_connector_missing_weights(sf_connector* conn);       /* count; names via sf_last_error() */
/* Rows of the output for F frames of P x P patches.  P' = ceil(P / stride) (bilinear) or floor(P / stride) (average, max);
 * no_token F P'^2, one_token F P'^2 + 1, frame F (P'^2 + 1), grid F P' (P' + 1).                                                   */
int sf_connector_num_tokens(sf_connector* conn, int F, int P, int64_t* out);
int sf_connector_workspace_bytes(sf_connector* conn, int F, int P, size_t* out);      /* after sf_connector_finalize */
/* feats_dev fp32 [F, P * P, in_dim]; out_dev [sf_connector_num_tokens, out_dim] in out_dtype (SF_F32, or SF_BF16 rounded to nearest
 * even).  Row of frame f, cell (oy, ox): grid f P' (P' + 1) + oy (P' + 1) + ox with a newline row after every grid row; frame
 * f (P'^2 + 1) + oy P' + ox with a newline row after every frame; no_token / one_token f P'^2 + oy P' + ox, one_token adds one newline
 * row at F P'^2.  workspace: 256-byte aligned, sf_connector_workspace_bytes(F, P).  Refused before anything is launched: F < 1, P < 1
 * or P' < 1 and a misaligned buffer (SF_ERR_INVALID), an activation past 2^31 - 1 elements (SF_ERR_CAPACITY), a short workspace
 * (SF_ERR_WORKSPACE), a handle that is not finalized (SF_ERR_STATE).  The call sets no device: the handle's device must be current
 * in the calling thread, and `stream` and every buffer must belong to it.                                                         */
int sf_connector_forward(sf_connector* conn, const float* feats_dev, int F, int P, void* out_dev, int out_dtype, void* workspace_dev,
                         size_t workspace_bytes, sf_stream stream);
/* The pool-and-layout kernel alone (parity tests), in one of its two input forms.
 * fp32 form: in_f32_dev [F, P * P, C] -> out_dev [rows, C] in out_dtype (SF_F32 / SF_BF16); in_hi_dev, in_lo_dev, out_hi_dev and
 * out_lo_dev NULL.  Plane form: in_hi_dev (+ in_lo_dev or NULL) bf16 planes of the same tensor, summed in fp32 -> out_hi_dev
 * (+ out_lo_dev or NULL), hi = bf16(y), lo = bf16(y - hi); in_f32_dev and out_dev NULL.  Taps as PyTorch's F.avg_pool2d /
 * F.max_pool2d (floor(P / stride) cells per side) and F.interpolate(mode="bilinear", align_corners=False) (ceil(P / stride)); rows and
 * newline rows (newline_dev fp32 [C], may be NULL for newline 0) as sf_connector_forward places them.  C % 8 == 0, every buffer
 * 16-byte aligned; one fixed summation order per element, bit-reproducible.  max takes a tap when it is greater or a NaN, as
 * F.max_pool2d does: a NaN in a window is the window's result, and of two zeros the first in row-major order stays.              */
int sf_op_connector_pool(const float* in_f32_dev, const uint16_t* in_hi_dev, const uint16_t* in_lo_dev, int F, int P, int C,
                         int pool_mode, int pool_stride, int newline, const float* newline_dev, void* out_dev, int out_dtype,
                         uint16_t* out_hi_dev, uint16_t* out_lo_dev, sf_stream stream);

/* ---- online action detection: the streaming LSTR detector -------------------------------------
 * The reference's downstream/OAD LSTRStream.stream_inference path (inference only, INPUT.MODALITY 'visual'): feature head, a
 * long-memory window of L samples compressed by enc_modules (stage 0 through the decomposition k = W_k x, k_pos = W_k pe[i] + b_k,
 * likewise v, over a per-stream ring of projected rows), a causal work-memory decoder and the classifier.  Keys of
 * sf_oad_load_tensor are the reference's state-dict names ("feature_head_long.visual_linear.0.weight", "enc_queries.0.weight",
 * "enc_modules.0.layers.0.multihead_attn.in_proj_weight", "dec_modules.layers.1.linear1.weight", "classifier.bias",
 * "pos_encoding.pe" with at least L + W rows).  Weights are rounded / split once at sf_oad_finalize, which also computes what does
 * not depend on the input: stage 0's query self-attention + norm1, their q projection, and k_pos / v_pos.
 * Kernels: csrc/sf_oad.hip.                                                                                                       */
typedef struct sf_oad sf_oad;
typedef struct sf_oad_state sf_oad_state;
#define SF_OAD_MAX_ENC_MODULES 8
#define SF_OAD_MAX_CALL_STREAMS 64
typedef struct {
  int32_t d_in, d_model, heads, ffn;            /* d_model == d_in when linear_enabled == 0; d_in, d_model, ffn multiples of 64 */
  int32_t long_samples, work_samples, classes; /* L, W, DATA.NUM_CLASSES                                                      */
  int32_t act;                                  /* 0 erf GELU, 2 ReLU                                                          */
  int32_t linear_enabled;                       /* MODEL.FEATURE_HEAD.LINEAR_ENABLED                                           */
  int32_t enc_modules;                          /* 1..SF_OAD_MAX_ENC_MODULES entries of ENC_MODULE [queries | -1, layers, norm]  */
  int32_t enc_queries[SF_OAD_MAX_ENC_MODULES], enc_layers[SF_OAD_MAX_ENC_MODULES], enc_norm[SF_OAD_MAX_ENC_MODULES];
  int32_t dec_layers, dec_norm;                 /* DEC_MODULE [-1, layers, norm]                                               */
  float eps;                                    /* nn.LayerNorm's 1e-5                                                         */
} sf_oad_config;
int sf_oad_create(const sf_oad_config* cfg, int device, sf_oad** out);
void sf_oad_destroy(sf_oad* det);
int sf_oad_load_tensor(sf_oad* det, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
int sf_oad_finalize(sf_oad* det, int compute);             /* makes the handle's device current; launches and synchronises */
int sf_oad_missing_weights(sf_oad* det);                   /* count; names via sf_last_error() */
int sf_oad_workspace_bytes(sf_oad* det, int streams, size_t* out);      /* after sf_oad_finalize; streams of one call */
/* Device-resident state of `streams` independent streams: the ring of projected long-memory rows [L, 2 d_model] (k | v, fp32) and
 * the cached output of compression stage 0 [Q0, d_model] per stream.  Ring head and fill count are host integers.                 */
int sf_oad_state_create(sf_oad* det, int streams, sf_oad_state** out);
void sf_oad_state_destroy(sf_oad_state* st);
int sf_oad_state_reset(sf_oad_state* st, int stream);      /* stream < 0: all of them */
int sf_oad_state_fill(sf_oad_state* st, int stream);       /* long samples held: 0 (empty) or L; negative: error */
/* dst's stream dst_stream becomes a copy of src's stream src_stream (same detector), enqueued on `stream`                         */
int sf_oad_state_copy(sf_oad_state* dst, int dst_stream, sf_oad_state* src, int src_stream, sf_stream stream);
/* One step of n <= SF_OAD_MAX_CALL_STREAMS distinct streams (stream_ids: HOST array).  work_dev fp32 [n, W, d_in]; long_rows: HOST
 * array, per stream 0 (reuse the cached compressed memory), 1 (one new sample, the oldest drops out) or L (the whole window, oldest
 * first: only on an empty stream, and an empty stream takes nothing else); long_dev fp32 [sum long_rows, d_in] in call order;
 * mask_dev fp32 [n, L] additive key mask by window position (0 = oldest), -inf allowed, read for streams with long_rows > 0 (NULL:
 * none; a row of only -inf is the caller's error and yields zeros).  out_dev fp32 [n, W, classes]: scores, or their softmax when
 * probs != 0.  No allocation and no host synchronisation; every kernel has one fixed summation order.                             */
int sf_oad_step(sf_oad* det, sf_oad_state* st, const int32_t* stream_ids, int n, const float* work_dev, const float* long_dev,
                const int32_t* long_rows, const float* mask_dev, float* out_dev, int probs, void* workspace_dev, size_t workspace_bytes,
                sf_stream stream);
/* The attention kernel alone (parity tests): ctx[s, i, h, :] = softmax_j(scale q . (k_j + k_pos_j) + mask[s, j] (+ causal)) (v_j + v_pos_j),
 * fp32.  q_dev [q_streams, Tq, heads * head_dim] with q_streams = 1 (shared by every stream) or streams; k_dev, v_dev
 * [streams, Tk, heads * head_dim]; key j of stream s is row (ring_start[s] + j) mod Tk (ring_start: HOST array or NULL = 0);
 * k_pos_dev / v_pos_dev [Tk, heads * head_dim] by key position j, or NULL; mask_dev [streams, Tk] additive or NULL; causal: key j
 * visible to query i iff j <= i + Tk - Tq.  A key whose mask is -inf contributes exactly zero whatever its rows hold; a query without
 * a visible key gets zeros.  head_dim a multiple of 8 in 8..256, Tq, Tk >= 1, streams <= SF_OAD_MAX_CALL_STREAMS, buffers 16-byte
 * aligned.  ctx_dev [streams, Tq, heads * head_dim].                                                                              */
int sf_op_oad_attention(const float* q_dev, int q_streams, const float* k_dev, const float* v_dev, const int32_t* ring_start,
                        const float* k_pos_dev, const float* v_pos_dev, const float* mask_dev, float* ctx_dev, int streams, int Tq, int Tk,
                        int heads, int head_dim, int causal, sf_stream stream);

/* ---- multi-scale deformable attention (Deformable DETR's MSDeformAttn; the reference's CUDA op under
 * downstream/OVIS/mask2former/modeling/pixel_decoder/ops/, used by the Mask2Former pixel decoder and the ViT-Adapter) ----------
 * out[n, q, m, :] = sum over levels l and points p of attention_weights[n, q, m, l, p] * bilinear(value[n, level l, m, :], location),
 * all fp32.  value_dev [N, S, M, D]; spatial_shapes [L, 2] = (H_l, W_l) and level_start_index [L] are HOST arrays, copied into the
 * kernel arguments; sampling_locations_dev [N, Lq, M, L, P, 2] normalised (x, y); attention_weights_dev [N, Lq, M, L, P];
 * out_dev [N, Lq, M * D].  Sampling as the CUDA kernel and grid_sample(bilinear, zeros, align_corners=False): pixel = loc * size - 0.5,
 * a sample counts iff -1 < h < H and -1 < w < W, each corner bounds-checked on its own.  D a multiple of 8 in 8..128, L and P in 1..8,
 * N, S, M, Lq >= 1, sum of H_l * W_l == S, every level inside [0, S), value and out 16-byte aligned: anything else, and a null
 * pointer, is SF_ERR_INVALID before anything is launched.  One owner per output element, one fixed order: bit-reproducible.      */
int sf_op_msda_forward(const float* value_dev, const int32_t* spatial_shapes, const int32_t* level_start_index,
                       const float* sampling_locations_dev, const float* attention_weights_dev, float* out_dev, int N, int S, int M,
                       int D, int Lq, int L, int P, sf_stream stream);
/* The same with the front of MSDeformAttn.forward (modules/ms_deform_attn.py:102-112) folded in: offsets_dev holds the RAW rows of
 * the sampling_offsets Linear, [N * Lq] rows of offsets_ld floats of which the first M * L * P * 2 are read; logits_dev the raw rows
 * of the attention_weights Linear, logits_ld floats each, the first M * L * P read (both may be column ranges of one GEMM output);
 * reference_points_dev [N, Lq, L, ref_dim].  The softmax over L * P and the sampling location (ref_dim 2: ref + offset / (W_l, H_l);
 * ref_dim 4: ref_xy + offset / P * ref_wh * 0.5) are computed in the kernel; padding_mask_dev [N, S] uint8 or NULL: a non-zero
 * entry makes that value row read as zeros.  Neither the locations, nor the softmax, nor a masked copy of value is ever stored.  */
int sf_op_msda_forward_fused(const float* value_dev, const uint8_t* padding_mask_dev, const int32_t* spatial_shapes,
                             const int32_t* level_start_index, const float* offsets_dev, int offsets_ld, const float* logits_dev,
                             int logits_ld, const float* reference_points_dev, int ref_dim, float* out_dev, int N, int S, int M, int D,
                             int Lq, int L, int P, sf_stream stream);
/* Backward of sf_op_msda_forward for grad_out_dev [N, Lq, M * D]: grad_value_dev [N, S, M, D] is zeroed by the call and then
 * accumulated with float atomics, grad_sampling_locations_dev [N, Lq, M, L, P, 2] and grad_attention_weights_dev [N, Lq, M, L, P]
 * are written once by their one owner.  The latter two are bit-reproducible; grad_value is a sum in arrival order and is not.    */
int sf_op_msda_backward(const float* value_dev, const int32_t* spatial_shapes, const int32_t* level_start_index,
                        const float* sampling_locations_dev, const float* attention_weights_dev, const float* grad_out_dev,
                        float* grad_value_dev, float* grad_sampling_locations_dev, float* grad_attention_weights_dev, int N, int S,
                        int M, int D, int Lq, int L, int P, sf_stream stream);

/* ---- the ViT-Adapter's two streaming kernels (models/modeling_timesformer_siglip_adapter.py; csrc/sf_adapter.hip) -----------------
 * ConvFFN's depthwise 3x3 + exact-erf GELU (adapter:244-254, 231-232) on the three-level token tensor: x_dev, y_dev fp32
 * [F, 21 * (H/2 * W/2), C], levels 2H x 2W, H x W, H/2 x W/2 in that order, channels contiguous; w_dev [C, 3, 3], b_dev [C].  ONE shared
 * 3x3 filter per channel, zero padding 1, applied to each level on its own grid: a tap outside its level's grid contributes zero and is
 * never read.  H, W even, C a multiple of 4 up to 1024, x, y, b 16-byte aligned, y must not alias x.  Bit-reproducible.             */
int sf_op_adapter_dwconv_gelu(const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev, int F, int H, int W, int C,
                              sf_stream stream);
/* One level of the adapter's tail (adapter:651-673), written NCHW: level 0..3 = res2..res5 of a ViT grid of H x W patches,
 *   out[f, c, y, x] = scale[c] * (tokens[f, pix, c] + bilinear(vit[f, :, c])(y, x) [+ c1[f, c, y, x]]) + shift[c]
 * out_dev fp32 [F, D, Ho, Wo] with (Ho, Wo) = (4H, 4W), (2H, 2W), (H, W), (H/2, W/2).  tokens_dev: levels 1..3 fp32 rows of D floats,
 * pixel-major, frame f at tokens_dev + f * tokens_frame_stride floats (a level's slice of the [F, 21 n, D] tensor); level 0 the
 * transposed convolution as a GEMM output, [F, 2H * 2W, 4 D] with columns (dy, dx, c)-major, read through the 2 x 2 pixel shuffle.
 * vit_dev fp32 [F, H * W, D] or NULL (add_vit_feature=False): resampled x4, x2, x1, x0.5 by F.interpolate(mode="bilinear",
 * align_corners=False)'s rule, edges clamped.  c1_dev fp32 [F, D, 4H, 4W] or NULL, level 0 only.  scale_dev / shift_dev [D]: the eval
 * BatchNorm folded on the host (and the transposed convolution's bias at level 0).  D a multiple of 4; level 3 needs H and W even.  */
int sf_op_adapter_fuse(int level, const float* tokens_dev, long long tokens_frame_stride, const float* vit_dev, const float* c1_dev,
                       const float* scale_dev, const float* shift_dev, float* out_dev, int F, int H, int W, int D, sf_stream stream);

/* The two backward entries of the adapter's training path (streamformer_amd/adapter.py with trainable=True; csrc/sf_adapter_bwd.hip).
 * Backward of sf_op_adapter_dwconv_gelu: x_dev is the forward's input (z = dwconv(x) + b is recomputed, y is not needed), dy_dev the
 * gradient of its output, both [F, 21 * (H/2 * W/2), C].  Outputs, any subset (not none): dx_dev like x_dev, dw_dev [C, 3, 3], db_dev [C];
 * an output that is not asked for stays unwritten and each equals what the joint call writes, bit for bit.  g = dy gelu'(z) (the exact
 * derivative of the erf form) goes to the workspace; a workgroup keeps the sums of dw and db over its strip of tokens and writes one
 * partial row, the rows are added in ascending order by a second launch, dx is a gather over the token's own level grid: no atomics,
 * bit-reproducible, three launches at most, the caller's stream, no allocation.  The workspace is the g tensor rounded up to 256 bytes
 * followed by one row of 10 C floats per workgroup (a function of F, H, W, C alone).  Refused before anything is launched: a NULL
 * buffer, F < 1, H or W odd or < 2, C no multiple of 4 in 4..1024, x, b, dy or dx not 16-byte aligned, dx aliasing x or dy
 * (SF_ERR_INVALID), more than 2^31 - 1 elements (SF_ERR_CAPACITY; the sizer then returns 0), a short workspace (SF_ERR_WORKSPACE;
 * 256-byte aligned).                                                                                                                  */
size_t sf_op_adapter_dwconv_gelu_backward_workspace_bytes(int F, int H, int W, int C);
int sf_op_adapter_dwconv_gelu_backward(const float* x_dev, const float* w_dev, const float* b_dev, const float* dy_dev, float* dx_dev,
                                       float* dw_dev, float* db_dev, int F, int H, int W, int C, void* workspace_dev, size_t workspace_bytes,
                                       sf_stream stream);
/* The adjoint of sf_op_adapter_fuse in its token operand, a re-layout: dy_dev fp32 NCHW [F, D, Ho, Wo] of level 0..3 -> d_tokens_dev in
 * the layout sf_op_adapter_fuse reads its tokens in (levels 1..3: rows of D floats, frame f at d_tokens_dev + f * tokens_frame_stride
 * floats, so a level's slice of a [F, 21 n, D] tensor can be the target and the other slices stay untouched; level 0: [F, 2H * 2W, 4 D]
 * through the inverse 2 x 2 pixel shuffle).  Every output element is written exactly once.  The ViT term is constant under a frozen
 * backbone and c1's gradient is dy itself.  The refusals of sf_op_adapter_fuse; d_tokens_dev 16-byte aligned.                        */
int sf_op_adapter_fuse_backward(int level, const float* dy_dev, float* d_tokens_dev, long long tokens_frame_stride, int F, int H, int W, int D,
                                sf_stream stream);

/* ---- Mask2Former pixel decoder: mask features and multi-scale features from res2..res5 -------------------------------------------
 * The reference's MSDeformAttnPixelDecoder (downstream/OVIS/mask2former/modeling/pixel_decoder/msdeformattn.py): 1 x 1 input projections
 * + GroupNorm(32), a deformable-attention transformer encoder over the chosen levels (post-norm, ReLU, sine position table + level
 * embedding), FPN levels (lateral 1 x 1, bilinear upsample + add, 3 x 3, GroupNorm, ReLU) for the finer ones and the 1 x 1 mask_features
 * convolution.  Same protocol as the connector: create (the width rules are checked there, the field named), stage the weights under
 * the reference's state-dict names (a leading "sem_seg_head.pixel_decoder." is dropped), finalize in a compute mode (weights rounded /
 * split once; the convolution weights re-laid out for the GEMMs there).  The handle is inference only (training runs on the Python
 * module's autograd graph and the two backward entries below), no padding masks.  Kernels: csrc/sf_pixdec.hip, csrc/sf_pixdec_bwd.hip. */
typedef struct sf_pixdec sf_pixdec;
#define SF_PIXDEC_MAX_LEVELS 4
#define SF_PIXDEC_NORM_GN 0
typedef struct {
  int32_t num_levels;                          /* input levels (res2 .. res5), 1..4, listed by increasing stride              */
  int32_t channels[SF_PIXDEC_MAX_LEVELS];      /* multiples of 64                                                             */
  int32_t strides[SF_PIXDEC_MAX_LEVELS];
  int32_t in_transformer[SF_PIXDEC_MAX_LEVELS];/* 1: the level enters the transformer encoder                                 */
  int32_t conv_dim, mask_dim, nheads, dim_feedforward, enc_layers, enc_n_points, common_stride;
  int32_t norm;                                /* SF_PIXDEC_NORM_GN                                                           */
  int32_t im2col_chunk_rows;                   /* pixels per gathered 3 x 3 operand; 0: the library's default (16384)         */
} sf_pixdec_config;
int sf_pixdec_create(const sf_pixdec_config* cfg, int device, sf_pixdec** out);
void sf_pixdec_destroy(sf_pixdec* dec);
/* host_ptr: contiguous host memory of dtype SF_F32, SF_F64 or SF_BF16 with exactly the reference's shape (convolutions [O, I, kh, kw]). */
int sf_pixdec_load_tensor(sf_pixdec* dec, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
/* Makes the handle's device current and leaves it so. */
int sf_pixdec_finalize(sf_pixdec* dec, int compute);
int sf_pixdec_missing_weights(sf_pixdec* dec);              /* count; names via sf_last_error() */
/* How many entries of the reference's `out` list sf_pixdec_forward returns (min(3, transformer levels + FPN levels)) and how many FPN
 * levels the strides ask for.  Either pointer may be NULL.                                                                          */
int sf_pixdec_num_outputs(sf_pixdec* dec, int* num_multi_scale, int* num_fpn_levels);
/* level_shapes: HOST array of (H, W) per input level, independent of each other (no halving is assumed).  After sf_pixdec_finalize. */
int sf_pixdec_workspace_bytes(sf_pixdec* dec, int F, const int32_t* level_shapes, int num_levels, size_t* out);
/* features_dev: HOST array of num_levels device pointers, level l fp32 [F, channels[l], H_l, W_l] (a level neither the transformer nor an
 * FPN level reads may be NULL).  mask_features_dev fp32 [F, mask_dim, H, W] of the finest level the decoder reaches.  multi_scale_dev:
 * HOST array of num_multi_scale device pointers, fp32 [F, conv_dim, H, W] each: the first entries of the reference's `out`, i.e. the
 * transformer's levels coarsest first, then the FPN levels coarse to fine; entry 0 is the reference's transformer_encoder_features.
 * No allocation, no host synchronisation, one workspace (256-byte aligned), the caller's stream; bit-reproducible.  Refused before
 * anything is launched: not finalized (SF_ERR_STATE), a level count other than the config's, F outside 1..65535, a NULL or not 16-byte
 * aligned buffer (SF_ERR_INVALID), a short workspace (SF_ERR_WORKSPACE), activations above 2^31 - 1 elements (SF_ERR_CAPACITY).      */
int sf_pixdec_forward(sf_pixdec* dec, const float* const* features_dev, int F, const int32_t* level_shapes, int num_levels,
                      float* mask_features_dev, float* const* multi_scale_dev, int num_multi_scale, void* workspace_dev,
                      size_t workspace_bytes, sf_stream stream);
/* The decoder's kernels alone.  "rows" are fp32 [F, H W, C] with channels contiguous, "planes" the same as bf16 hi (+ lo = bf16(x - hi),
 * may be NULL) bit patterns, the A operand of the GEMMs.  Every buffer 16-byte aligned.
 * NCHW fp32 [F, C, HW] -> planes (C % 8 == 0), and rows (frame f at rows_dev + f * frame_stride floats) -> NCHW fp32 (C % 4 == 0).  */
int sf_op_pixdec_nchw_to_planes(const float* x_dev, uint16_t* hi_dev, uint16_t* lo_dev, int F, int C, int HW, sf_stream stream);
int sf_op_pixdec_rows_to_nchw(const float* rows_dev, long long frame_stride, float* out_dev, int F, int C, int HW, sf_stream stream);
/* GroupNorm(32, C) (eps 1e-5) over rows x_dev per (frame, group), two-pass shifted statistics into stats_dev [F, 32, 4] (shift, mean - shift, rstd, 0), then
 * y = gn(x) [ReLU] [+ bilinear upsample of prev_dev rows [F, Hp Wp, C] to H x W, F.interpolate(align_corners=False)'s rule].  Outputs,
 * any subset: y_dev rows, y planes, q planes = y + pos_dev[pixel] (pos_dev fp32 [H W, C]).  C % 64 == 0.                              */
int sf_op_pixdec_groupnorm(const float* x_dev, const float* gamma_dev, const float* beta_dev, int relu, const float* prev_dev, int Hp,
                           int Wp, const float* pos_dev, float* stats_dev, float* y_dev, uint16_t* y_hi_dev, uint16_t* y_lo_dev,
                           uint16_t* q_hi_dev, uint16_t* q_lo_dev, int F, int H, int W, int C, sf_stream stream);
/* pos_dev [S, C] = PositionEmbeddingSine(C / 2, normalize=True) of an all-false mask + level_embed_dev[l] over the L levels of
 * level_shapes (HOST (H, W) pairs), S = sum H W; ref_dev [F, S, L, 2] = ((x + 0.5) / W, (y + 0.5) / H) repeated over levels.          */
int sf_op_pixdec_pos_ref(const float* level_embed_dev, const int32_t* level_shapes, int L, int F, int C, float* pos_dev, float* ref_dev,
                         sf_stream stream);
/* LayerNorm of rows x_dev [rows, C] (the residual already added): any subset of y_dev fp32, y planes, q planes = y + pos_dev[row % pos_rows]. */
int sf_op_pixdec_postln(const float* x_dev, const float* gamma_dev, const float* beta_dev, float eps, const float* pos_dev, int pos_rows,
                        float* y_dev, uint16_t* y_hi_dev, uint16_t* y_lo_dev, uint16_t* q_hi_dev, uint16_t* q_lo_dev, int rows, int C,
                        sf_stream stream);
/* The nine 3 x 3 taps (padding 1) of pixel rows [row0, row0 + rows) of planes [F, H W, C] side by side: out planes [rows, 9 C] in
 * (dy, dx, c) order.  A tap outside its frame's grid is written as zero and never read.  C % 64 == 0.                                */
int sf_op_pixdec_im2col(const uint16_t* in_hi_dev, const uint16_t* in_lo_dev, int F, int H, int W, int C, long long row0, int rows,
                        uint16_t* out_hi_dev, uint16_t* out_lo_dev, sf_stream stream);
/* The 3 x 3 convolution as the decoder runs it: that gather in chunks of chunk_rows pixels (0: the default), each followed by one GEMM
 * with K = 9 C against w planes [N, 9 C] in (dy, dx, c_in) order; out_dev fp32 rows [F H W, N].  With lo planes the accurate mode.      */
size_t sf_op_pixdec_conv3x3_workspace_bytes(int F, int H, int W, int C, int chunk_rows);
int sf_op_pixdec_conv3x3(const uint16_t* in_hi_dev, const uint16_t* in_lo_dev, const uint16_t* w_hi_dev, const uint16_t* w_lo_dev, int F,
                         int H, int W, int C, int N, int chunk_rows, float* out_dev, void* workspace_dev, size_t workspace_bytes,
                         sf_stream stream);
/* GroupNorm's backward for training (streamformer_amd/pixel_decoder.py with trainable=True; csrc/sf_pixdec_bwd.hip).  x_dev, dy_dev and
 * dx_dev are rows [F, H W, C]; stats_dev is what sf_op_pixdec_groupnorm wrote for x_dev and is not recomputed; relu as in that call (the
 * gradient is zeroed where the forward clipped, decided by the forward's own expression).  Outputs, any subset (not none): dx_dev,
 * dgamma_dev [C], dbeta_dev [C]; each equals what the joint call writes, bit for bit.  A workgroup sums a span of whole pixel rows of one
 * frame, the spans (a function of F and H W alone) are added in ascending order by a second launch: no atomics, bit-reproducible.  The
 * caller's stream, no allocation, no host synchronisation.  Refused before anything is launched: a NULL or not 16-byte aligned buffer,
 * C no positive multiple of 64, F outside 1..65535, H or W < 1 (SF_ERR_INVALID), more than 2^31 - 1 elements (SF_ERR_CAPACITY), a short
 * workspace (SF_ERR_WORKSPACE; 256-byte aligned).                                                                                    */
size_t sf_op_pixdec_groupnorm_backward_workspace_bytes(int F, int H, int W, int C);
int sf_op_pixdec_groupnorm_backward(const float* x_dev, const float* stats_dev, const float* gamma_dev, const float* beta_dev, int relu,
                                    const float* dy_dev, float* dx_dev, float* dgamma_dev, float* dbeta_dev, int F, int H, int W, int C,
                                    void* workspace_dev, size_t workspace_bytes, sf_stream stream);
/* The adjoint of sf_op_pixdec_groupnorm's `+ bilinear upsample of prev_dev`: d_prev_dev rows [F, Hp Wp, C] from dy_dev rows [F, H W, C],
 * at any ratio.  Gather form: each coarse pixel adds the fine pixels whose taps land on it in ascending (y, x) order; no atomics,
 * bit-reproducible.  The same refusals (no workspace).                                                                               */
int sf_op_pixdec_upsample_backward(const float* dy_dev, float* d_prev_dev, int F, int H, int W, int Hp, int Wp, int C, sf_stream stream);

/* ---- Mask2Former masked-attention decoder: queries -> class logits, masks, re-identification embeddings ----------------------------
 * The reference's MultiScaleMaskedTransformerDecoder (downstream/OVIS/mask2former/modeling/transformer_decoder/
 * mask2former_transformer_decoder.py) and its CTVIS subclass CLMultiScaleMaskedTransformerDecoder (reid_layers >= 0: reid_embed,
 * pred_queries, pred_bboxes): per layer masked cross-attention over one of three feature levels, self-attention, FFN (post-norm, ReLU),
 * and after every layer the prediction heads, whose thresholded low-resolution mask is the next layer's attention mask.  The consumer of
 * sf_pixdec_forward's four outputs as they are.  Same protocol as sf_pixdec: create (the width rules are checked there, the field
 * named), stage the weights under the reference's state-dict names (a leading "sem_seg_head.predictor." is dropped), finalize in a
 * compute mode.  Inference only, post-norm only, no padding masks.  Kernels: csrc/sf_maskdec.hip.                                   */
typedef struct sf_maskdec sf_maskdec;
#define SF_MASKDEC_LEVELS 3
typedef struct {
  int32_t in_channels, hidden_dim, num_queries, nheads, dim_feedforward, dec_layers, mask_dim, num_classes;   /* widths: multiples of 64 */
  int32_t enforce_input_project;               /* input_proj is a 1 x 1 convolution iff this or in_channels != hidden_dim          */
  int32_t pre_norm;                            /* must be 0                                                                         */
  int32_t mask_classification;                 /* must be 1                                                                         */
  int32_t reid_layers;                         /* -1: no reid_embed (the base class); 0: identity; n: an MLP of n layers            */
  int32_t reid_hidden_dim;                     /* read when reid_layers > 1                                                         */
} sf_maskdec_config;
/* Device buffers of one forward, fp32 unless said otherwise; M = F * num_queries rows.  pred_logits [M, num_classes + 1] and pred_masks
 * [M, H, W] are required; pred_queries [M, hidden_dim] (decoder_norm's rows), pred_embeds [M, hidden_dim] (reid_layers >= 0 only) and
 * pred_bboxes [M, 4] ((min x, min y, max x + 1, max y + 1) / (W, H, W, H) over the pixels of pred_masks above zero, zeros without one)
 * may be NULL.  aux_*: the same per entry of the reference's aux_outputs, [dec_layers, ...] each, or NULL (nothing of it is computed
 * then).  attn_masks: uint32, every layer's packed attention mask one after the other, layer i [M, ceil(h w / 32)] words at the
 * resolution of level i % 3, bit (j & 31) of word j / 32 set = key j hidden, or NULL.                                               */
typedef struct {
  float* pred_logits; float* pred_masks; float* pred_queries; float* pred_embeds; float* pred_bboxes;
  float* aux_logits; float* aux_masks; float* aux_queries; float* aux_embeds;
  uint32_t* attn_masks;
} sf_maskdec_outputs;
int sf_maskdec_create(const sf_maskdec_config* cfg, int device, sf_maskdec** out);
void sf_maskdec_destroy(sf_maskdec* dec);
/* host_ptr: contiguous host memory of dtype SF_F32, SF_F64 or SF_BF16 with exactly the reference's shape. */
int sf_maskdec_load_tensor(sf_maskdec* dec, const char* key, const void* host_ptr, int dtype, const int64_t* shape, int ndim);
/* Makes the handle's device current and leaves it so. */
int sf_maskdec_finalize(sf_maskdec* dec, int compute);
int sf_maskdec_missing_weights(sf_maskdec* dec);            /* count; names via sf_last_error() */
/* level_shapes: HOST array of three (h, w) pairs, the multi-scale features in the order they are passed; H, W: mask_features. */
int sf_maskdec_workspace_bytes(sf_maskdec* dec, int F, const int32_t* level_shapes, int H, int W, size_t* out);
/* x_dev: HOST array of three device pointers, level l fp32 [F, in_channels, h_l, w_l]; mask_features_dev fp32 [F, mask_dim, H, W]:
 * what sf_pixdec_forward wrote, no layout change between the two.  No allocation, no host synchronisation, one workspace (256-byte
 * aligned), the caller's stream; bit-reproducible.  Refused before anything is launched: not finalized (SF_ERR_STATE), F outside
 * 1..65535, a NULL or not 16-byte aligned buffer (SF_ERR_INVALID), a short workspace (SF_ERR_WORKSPACE), activations above 2^31 - 1
 * elements (SF_ERR_CAPACITY).                                                                                                       */
int sf_maskdec_forward(sf_maskdec* dec, const float* const* x_dev, const float* mask_features_dev, int F, const int32_t* level_shapes, int H,
                       int W, const sf_maskdec_outputs* outputs, void* workspace_dev, size_t workspace_bytes, sf_stream stream);
/* The decoder's kernels alone (parity tests).  Masked attention, fp32: ctx[f, q, h, :] = softmax_j(q . (k_j + k_pos_j) / sqrt(head_dim)
 * over the keys whose mask bit is clear) v_j.  q_dev rows [F Q] of q_pitch floats, k_dev / v_dev rows [F HW] of kv_pitch floats, a
 * head's columns at h * head_dim; k_pos_dev [HW] rows of pos_pitch floats or NULL; mask_dev uint32 [F, Q, ceil(HW / 32)] shared by the
 * heads, or NULL (nothing hidden).  A query without a visible key gets zeros.  A 16-key tile hidden from all 16 queries of a workgroup
 * is skipped without being loaded unless no_skip is set; both ways give the same bits.  Outputs, any subset: ctx_dev fp32
 * [F Q, heads * head_dim], the same as bf16 hi (+ lo) planes.  head_dim a multiple of 8 in 8..128, buffers 16-byte aligned.           */
int sf_op_maskdec_attention(const float* q_dev, int q_pitch, const float* k_dev, const float* v_dev, int kv_pitch, const float* k_pos_dev,
                            int pos_pitch, const uint32_t* mask_dev, float* ctx_dev, uint16_t* ctx_hi_dev, uint16_t* ctx_lo_dev, int F, int Q,
                            int HW, int heads, int head_dim, int no_skip, sf_stream stream);
/* Mask logits mask_embed_dev [F, Q, mask_dim] . mask_features_dev [F, mask_dim, H, W], fp32.  bits_dev (or NULL): the packed attention
 * mask [F, Q, ceil(h w / 32)] at resolution h x w, bit set iff the logit of the features resampled to h x w by
 * F.interpolate(bilinear, align_corners=False)'s rule is below zero, and a row with every bit set cleared; the resampled features go
 * through workspace_dev (sf_op_maskdec_mask_workspace_bytes).  logits_dev (or NULL): the logits at H x W, [F, Q, H, W]; boxes_dev (or
 * NULL, needs logits_dev): [F, Q, 4] as pred_bboxes above.  mask_dim a multiple of 4 up to 1024.                                     */
size_t sf_op_maskdec_mask_workspace_bytes(int F, int mask_dim, int h, int w);
int sf_op_maskdec_mask(const float* mask_embed_dev, const float* mask_features_dev, int F, int Q, int mask_dim, int H, int W, int h, int w,
                       uint32_t* bits_dev, float* logits_dev, float* boxes_dev, void* workspace_dev, size_t workspace_bytes, sf_stream stream);
/* The boxes alone, of masks_dev [rows, H, W] made elsewhere (sf_op_masklogits_forward): boxes_dev [rows, 4] as pred_bboxes above.    */
int sf_op_maskdec_boxes(const float* masks_dev, float* boxes_dev, int rows, int H, int W, sf_stream stream);

/* ---- masked attention for training (streamformer_amd/masked_attention.py): the decoder's attention kernel with the row statistics a
 * backward needs, that backward, and the mask packer.  All fp32 with exact products, no float atomics, bit-reproducible, the caller's
 * stream, no allocation, no host synchronisation.  Rows as in sf_op_maskdec_attention: q_dev [F Q] rows of q_pitch floats, k_dev /
 * v_dev [F HW] rows of kv_pitch floats (column ranges of one [rows, 3 C] buffer work), a head's columns at h * head_dim; mask_dev
 * uint32 [F, Q, ceil(HW / 32)] shared by the heads, [F, heads, Q, ceil(HW / 32)] with mask_per_head, or NULL (nothing hidden); bits of
 * keys at or past HW are never read.  Refused before any launch with SF_ERR_INVALID: a NULL required buffer, a buffer that is not
 * 16-byte aligned, a pitch below heads * head_dim or not a multiple of 4, head_dim not a multiple of 8 in 8..128, F, Q or heads outside
 * 1..65535, HW outside 1..2^24; SF_ERR_CAPACITY above 2^31 - 1 elements.                                                            */
/* ctx_dev [F Q, heads * head_dim]: bit for bit what sf_op_maskdec_attention writes without k_pos_dev.  stats_dev [F, heads, Q] or
 * NULL: the log-sum-exp of the scaled scores over the visible keys; +inf for a query without a visible key (its ctx is zeros).      */
int sf_op_maskattn_forward(const float* q_dev, int q_pitch, const float* k_dev, const float* v_dev, int kv_pitch, const uint32_t* mask_dev,
                           int mask_per_head, float* ctx_dev, float* stats_dev, int F, int Q, int HW, int heads, int head_dim, int no_skip,
                           sf_stream stream);
/* ctx_dev and stats_dev as the forward wrote them, d_ctx_dev [F Q, heads * head_dim].  With delta = rowsum(d_ctx o ctx) and
 * P = exp(q . k / sqrt(head_dim) - stats) on the visible keys: dv = P^T d_ctx, dS = P o (d_ctx v^T - delta), dq = dS k / sqrt(head_dim),
 * dk = dS^T q / sqrt(head_dim).  dq_dev [F Q] rows of dq_pitch floats, dk_dev / dv_dev [F HW] rows of dkv_pitch floats; every element
 * of the heads' columns is written: exact zeros in dk / dv for a key no query sees and in dq for a query that sees no key.  Two
 * launches; a key tile (dq) or query tile (dk, dv) with nothing visible is skipped without being loaded unless no_skip is set; both
 * ways give the same bits.                                                                                                          */
int sf_op_maskattn_backward(const float* q_dev, int q_pitch, const float* k_dev, const float* v_dev, int kv_pitch, const uint32_t* mask_dev,
                            int mask_per_head, const float* ctx_dev, const float* stats_dev, const float* d_ctx_dev, float* dq_dev, int dq_pitch,
                            float* dk_dev, float* dv_dev, int dkv_pitch, int F, int Q, int HW, int heads, int head_dim, int no_skip,
                            sf_stream stream);
/* mask_dev bytes [rows, HW] (a bool tensor, any leading shape flattened), non-zero = hidden -> bits_dev uint32 [rows, ceil(HW / 32)],
 * bit (j & 31) of word j / 32 set = key j hidden: the layout sf_op_maskdec_mask writes.  The padding bits of the last word are set.  */
int sf_op_maskattn_pack(const uint8_t* mask_dev, uint32_t* bits_dev, long long rows, int HW, sf_stream stream);

/* ---- mask logits for training (streamformer_amd/mask_decoder.py with trainable=True; csrc/sf_masklogits.hip): the product of every
 * prediction head at full mask-feature resolution and its gradients.  All fp32 with exact products, one owner and one summation order
 * per output element, no float atomics, bit-reproducible, the caller's stream, no allocation, no host synchronisation.  The grid is
 * F x 64-pixel tiles (the backward: spans of them), whatever Q is.  mask_embed_dev [F, Q, mask_dim], mask_features_dev
 * [F, mask_dim, P] with P = H W, logits [F, Q, P].  Refused before any launch with SF_ERR_INVALID: a NULL required buffer, a buffer
 * that is not 16-byte aligned, mask_dim not a multiple of 4 in 4..1024, F or Q outside 1..65535, P outside 1..2^24; SF_ERR_CAPACITY
 * when F max(Q, mask_dim) P or F Q mask_dim exceeds 2^31 - 1.  The bits are not those of sf_op_maskdec_mask's logits.               */
/* logits_dev[f, q, p] = sum_c mask_embed[f, q, c] mask_features[f, c, p].                                                            */
int sf_op_masklogits_forward(const float* mask_embed_dev, const float* mask_features_dev, float* logits_dev, int F, int Q, int mask_dim, int P,
                             sf_stream stream);
/* d_mask_embed_dev[f, q, c] = sum_p d_logits[f, q, p] mask_features[f, c, p] and d_mask_features_dev[f, c, p] =
 * sum_q mask_embed[f, q, c] d_logits[f, q, p]; either may be NULL (not both).  accumulate != 0: d_mask_features_dev is added to, not
 * overwritten (the heads of a decoder share one buffer; the order of the additions is the order of the calls); d_mask_embed_dev is
 * always overwritten.  Each d_logits tile is read once for both products.  d_mask_embed_dev is summed over spans of pixel tiles:
 * partial sums go to workspace_dev (sf_op_masklogits_backward_workspace_bytes; not needed without d_mask_embed_dev) and a second
 * launch adds them in ascending order.                                                                                               */
size_t sf_op_masklogits_backward_workspace_bytes(int F, int Q, int mask_dim, int P);
int sf_op_masklogits_backward(const float* d_logits_dev, const float* mask_embed_dev, const float* mask_features_dev, float* d_mask_embed_dev,
                              float* d_mask_features_dev, int accumulate, int F, int Q, int mask_dim, int P, void* workspace_dev,
                              size_t workspace_bytes, sf_stream stream);

/* ---- video instance segmentation: the kernels between the mask decoder and a list of instances ---------------------------------
 * (the CTVIS SimpleTracker's frame-local front and CTVISModel.inference_video; streamformer_amd/vis.py runs the association loop on
 * the host).  All fp32, bit-reproducible, the caller's stream, no allocation, no host synchronisation.                              */
/* Rows of logits_dev [rows, classes + 1]: softmax over the row without its last column.  max_scores_dev [rows] and labels_dev [rows]
 * (the first index of the largest score); scores_dev (or NULL): all [rows, classes] scores.                                         */
int sf_op_vis_scores(const float* logits_dev, long long rows, int classes_plus_one, float* max_scores_dev, int32_t* labels_dev,
                     float* scores_dev, sf_stream stream);
/* masks_dev [rows, pixels] -> bits_dev [rows, ceil(pixels / 32)], bit p & 31 of word p / 32 set iff x[p] > 0, tail bits zero, and
 * area_dev [rows], the number of set bits.                                                                                          */
int sf_op_vis_pack_masks(const float* masks_dev, long long rows, int pixels, uint32_t* bits_dev, int32_t* area_dev, sf_stream stream);
/* bits_dev [F, Q, ceil(pixels / 32)] as sf_op_vis_pack_masks wrote it -> inter_dev [F, Q, Q], popcount(row i & row j) inside each
 * frame.  The IoU (i + 1e-6) / (area_i + area_j - i + 1e-6) and the NMS scan are the host's.  pixels up to 524288.                  */
int sf_op_vis_mask_iou(const uint32_t* bits_dev, int F, int Q, int pixels, int32_t* inter_dev, sf_stream stream);
/* masks_dev [R, h, w], the detections' mask logits; index_dev int32 [K, F], a row of masks_dev or -1 (absent: zeros, adds nothing).
 * Per (k, f): resample h x w to Hp x Wp, keep the top left Hc x Wc, resample that to H x W, both by F.interpolate(bilinear,
 * align_corners=False)'s rule, composed in one pass; the second resample clamps at the crop's edge.  Outputs, any subset (NULL: not
 * wanted, at least one of the first two): out_masks_dev [K, F, H, W] bytes, 1 where the logit is above zero; out_logits_dev fp32
 * [K, F, H, W]; numerator_dev fp32 [K], the sum of sigmoid(logit) over the set pixels, with denominator_dev int64 [K], their number
 * (both or neither; they need the workspace, 256-byte aligned).  Hp = Hc = H = h (and the same for w) gathers rows unchanged.
 * K * F up to 65535; SF_ERR_CAPACITY when a 16 x 256 output tile reaches more than 63 KB of source pixels (a strong downscale).     */
size_t sf_op_vis_postprocess_workspace_bytes(int K, int F, int H, int W);
int sf_op_vis_postprocess(const float* masks_dev, int R, int h, int w, const int32_t* index_dev, int K, int F, int Hp, int Wp, int Hc, int Wc,
                          int H, int W, uint8_t* out_masks_dev, float* out_logits_dev, float* numerator_dev, int64_t* denominator_dev,
                          void* workspace_dev, size_t workspace_bytes, sf_stream stream);

/* ---- image segmentation: the kernels between the mask decoder and MaskFormer's semantic and panoptic results ---------------------
 * (semantic_inference and panoptic_inference of mask2former/maskformer_model.py; streamformer_amd/segmentation.py runs the segment rule
 * on the host; instance inference is sf_op_vis_scores + sf_op_vis_postprocess with an index table [K, 1]).  All fp32, bit-reproducible,
 * the caller's stream, no allocation, no host synchronisation.  The geometry arguments are sf_op_vis_postprocess's: masks_dev [Q, h, w]
 * resampled to Hp x Wp, cropped to the top left Hc x Wc, resampled to H x W, composed per output pixel: r_q(y, x).                  */
/* out_dev [C, H, W] = sum over q of probs_dev [Q, C] (what sf_op_vis_scores writes to scores_dev) times sigmoid(r_q), in query order on
 * fp32 MFMA.  Q up to 512, C up to 256; SF_ERR_CAPACITY above, and when a 1 x 64 output tile reaches more source pixels per query than
 * the LDS holds for a chunk of 32 queries (a strong downscale).                                                                      */
int sf_op_seg_semantic(const float* masks_dev, const float* probs_dev, int Q, int C, int h, int w, int Hp, int Wp, int Hc, int Wc, int H, int W,
                       float* out_dev, sf_stream stream);
/* Query q is kept iff labels_dev[q] != num_classes and max_scores_dev[q] > object_mask_threshold (decided on the device).  code_dev
 * int32 [H, W]: 2 q + (r_q >= 0) of the kept query with the largest max_scores[q] * sigmoid(r_q), the first index on ties, or -1 when no
 * query is kept.  counts_dev int32 [Q, 3] (zeroed here): pixels won, pixels with r_q >= 0, pixels with both; zeros for a query that is
 * not kept.  Q up to 512; SF_ERR_CAPACITY above, and when a 4 x 64 output tile reaches more source pixels than the LDS holds.        */
int sf_op_seg_panoptic_argmax(const float* masks_dev, const float* max_scores_dev, const int32_t* labels_dev, int Q, int num_classes,
                              float object_mask_threshold, int h, int w, int Hp, int Wp, int Hc, int Wc, int H, int W, int32_t* code_dev,
                              int32_t* counts_dev, sf_stream stream);
/* panoptic_dev int32 [pixels] = segment_of_query_dev[q] (int32 [Q], 0 = dropped) where code_dev holds 2 q + 1, else 0.  panoptic_dev may
 * be code_dev.                                                                                                                        */
int sf_op_seg_panoptic_relabel(const int32_t* code_dev, const int32_t* segment_of_query_dev, int Q, long long pixels, int32_t* panoptic_dev,
                               sf_stream stream);

/* ---- Mask2Former criterion (mask2former/modeling/matcher.py, criterion.py): every decoder layer of a training step per call --------
 * All fp32, the caller's stream, no allocation, no host synchronisation.  Layers travel as HOST arrays of L device pointers (the final
 * layer and the auxiliary ones are separate tensors of one shape): pred_logits[l] [B, Q, C1] with C1 = classes + 1, pred_masks[l]
 * [B, Q, H, W].  Targets travel as HOST arrays over the B images: tgt_masks[b] device fp32 [G_b, H_b, W_b], tgt_labels[b] device int64
 * [G_b], tgt_G / tgt_H / tgt_W host int32 (an image with G_b = 0 may have null pointers).  Points are (x, y) in [0, 1) and are sampled
 * by F.grid_sample(bilinear, zeros, align_corners=False)'s rule, every corner bounds-checked on its own.  Limits (SF_ERR_CAPACITY, before
 * any launch): L up to 16, B up to 32, G_b up to 128, Q and C1 up to 4096.                                                            */
/* cost_dev [L, B, Q, G_max] = w_mask cost_mask + w_class cost_class + w_dice cost_dice of HungarianMatcher.memory_efficient_forward at
 * the points coords_dev [L, B, K, 2]; columns >= G_b are NOT written.  The two [Q, K] x [K, G] contractions run on fp32 MFMA over
 * chunks of 512 points whose partials a second kernel adds in chunk order: bit-reproducible, no [Q, K] tensor in memory.              */
size_t sf_op_crit_costs_workspace_bytes(int L, int B, int Q, int G_max, int K);
int sf_op_crit_costs(const float* const* pred_logits, const float* const* pred_masks, int L, int B, int Q, int C1, int H, int W,
                     const float* const* tgt_masks, const int64_t* const* tgt_labels, const int32_t* tgt_G, const int32_t* tgt_H,
                     const int32_t* tgt_W, const float* coords_dev, int K, int G_max, float w_class, float w_mask, float w_dice,
                     float* cost_dev, void* workspace, size_t workspace_bytes, sf_stream stream);
/* SetCriterion.loss_masks of the N matched pairs of all layers: pairs_dev int32 [N, 4] = (layer, image, query, target), grouped by
 * layer, layer_start host int32 [L + 1].  Per pair one workgroup keeps the predicted mask at the K_over points over_dev [N, K_over, 2] in
 * LDS (K_over up to sf_op_crit_losses_capacity() = 39424, SF_ERR_CAPACITY above), selects the K_uncertain points of smallest |x| by a
 * radix select on the bit pattern (ties at the threshold go to the LOWER index; chosen points are emitted in index order), appends
 * rand_dev [N, K - K_uncertain, 2], samples the target (coordinates scale by the batch's largest mask, reads outside a mask's own extent
 * are zero, as nested_tensor_from_tensor_list pads) and reduces in a fixed order: bit-reproducible.  losses_dev[l * losses_stride + 0 / 1]
 * = loss_mask / loss_dice of layer l (sum over its pairs in pair order, over num_masks).  coords_out_dev [N, K, 2] and sums_dev [N, 4]
 * (sum sigmoid, sum t, sum sigmoid t, 0) are what the backward needs; idx_out_dev int32 [N, K_uncertain] (may be null) the chosen
 * indices.                                                                                                                            */
int sf_op_crit_losses_capacity(void);
size_t sf_op_crit_losses_workspace_bytes(int N);
int sf_op_crit_losses(const float* const* pred_masks, int L, int B, int Q, int H, int W, const float* const* tgt_masks, const int32_t* tgt_G,
                      const int32_t* tgt_H, const int32_t* tgt_W, const int32_t* pairs_dev, const int32_t* layer_start, int N,
                      const float* over_dev, const float* rand_dev, int K, int K_over, int K_uncertain, float num_masks,
                      float* losses_dev, int losses_stride, float* coords_out_dev, float* sums_dev, int32_t* idx_out_dev, void* workspace,
                      size_t workspace_bytes, sf_stream stream);
/* grad_pred_masks_dev [L, B, Q, H, W] (zeroed here: planes of unmatched queries stay zero) from the saved coordinates and sums and
 * upstream_dev [L, 2] = d / d loss_mask_l, d / d loss_dice_l.  A pair's plane of up to 32768 pixels is accumulated in LDS and flushed
 * once, a larger one goes straight to memory; float atomics either way, so the sums are in arrival order: NOT bit-reproducible (as
 * grad_value of sf_op_msda_backward).  No workspace.                                                                                  */
int sf_op_crit_losses_backward(const float* const* pred_masks, int L, int B, int Q, int H, int W, const float* const* tgt_masks,
                               const int32_t* tgt_G, const int32_t* tgt_H, const int32_t* tgt_W, const int32_t* pairs_dev, int N,
                               const float* coords_dev, const float* sums_dev, int K, float num_masks, const float* upstream_dev,
                               float* grad_pred_masks_dev, sf_stream stream);
/* SetCriterion.loss_labels of all layers: F.cross_entropy(weight = weight_dev [C1], mean reduction) of the L B Q rows, the target class
 * of a row being its pair's label and C1 - 1 (no-object) for an unmatched query or a label outside the table.  losses_dev[l *
 * losses_stride] = loss_ce of layer l; grad_dev [L, B, Q, C1] (may be null) its gradient; target_classes_out_dev int32 [L, B, Q] (may be
 * null) the target classes.  One wave per row, per-layer sums in a fixed order: bit-reproducible.                                     */
size_t sf_op_crit_class_loss_workspace_bytes(int L, int B, int Q);
int sf_op_crit_class_loss(const float* const* pred_logits, int L, int B, int Q, int C1, const int32_t* pairs_dev, int N,
                          const int64_t* const* tgt_labels, const int32_t* tgt_G, const float* weight_dev, float* losses_dev,
                          int losses_stride, float* grad_dev, int32_t* target_classes_out_dev, void* workspace, size_t workspace_bytes,
                          sf_stream stream);

/* ---- CTVIS contrastive loss (ctvis/modeling/cl_plugin/ct_cl_plugin.py, CTCLPlugin): loss_reid and loss_aux_reid of a training step ----
 * All fp32, the caller's stream, no allocation, no host synchronisation, a launch count independent of the shapes, no float atomics and
 * fixed reduction orders (bit-reproducible).  embeds_dev [R, C] is pred_embeds with R = B F Q rows; C is a multiple of 8 up to 256
 * (SF_ERR_CAPACITY otherwise), F at most 32.  The host decides the data-dependent bookkeeping and passes it as int32 device tables
 * (streamformer_amd/cl_plugin.py builds them): track_rows [T, F] the matched row of a (video, instance) at the frames it is present in,
 * else -1; track_items [T, F] the item anchored at (track, frame) or -1; items [I, 8] = (track, frame, anchor row, positive kind,
 * positive index, first negative, negatives, positive frame) with kind 0 an embedding row and kind 1 row t F + f of sg; neg [NE] the
 * items' negative rows; row_start [R + 1] / row_items [NE] per row the items listing it as a negative, in plan order.  max_neg is the
 * largest negative count of an item (up to 4096).  An entry out of range reads row 0 and never outside a buffer.
 * sf_op_clp_tracks: the similarity-guided embeddings sg_dev [T, F, C] (zeros before a track's first present frame, repeated over absent
 * frames) and stats_dev [T, F, 2] = (sim, beta = max(0, sim)) per present frame, 0 elsewhere.                                          */
int sf_op_clp_tracks(const float* embeds_dev, int R, int C, const int32_t* track_rows_dev, int T, int F, float* sg_dev, float* stats_dev,
                     sf_stream stream);
/* Per item log(1 + sum exp(d_neg - d_pos)) (maximum subtracted) and mean((cos - label)^2) over its 1 + n rows: item_out_dev [I, 4] =
 * (contras, aux, d_pos, 1 / |anchor|); losses_dev [2] = their sums in item order over I (zeros when I = 0).                            */
int sf_op_clp_items(const float* embeds_dev, int R, int C, const float* sg_dev, int T, int F, const int32_t* items_dev, int I,
                    const int32_t* neg_dev, int NE, int max_neg, float* losses_dev, float* item_out_dev, sf_stream stream);
/* grad_embeds_dev [R, C] for upstream_dev [2] = d / d (loss_reid, loss_aux_reid): a gather per row over the items that list it as a
 * negative, then per track the anchor and positive terms and the recurrence of sg backwards (through beta where sim > 0).  Every row
 * is written; rows nobody references are exact zeros.                                                                                */
size_t sf_op_clp_backward_workspace_bytes(int I, int T, int F, int C);
int sf_op_clp_backward(const float* embeds_dev, int R, int C, const float* sg_dev, const float* stats_dev, const int32_t* track_rows_dev,
                       const int32_t* track_items_dev, int T, int F, const int32_t* items_dev, int I, const int32_t* neg_dev, int NE,
                       int max_neg, const int32_t* row_start_dev, const int32_t* row_items_dev, const float* item_out_dev,
                       const float* upstream_dev, float* grad_embeds_dev, void* workspace, size_t workspace_bytes, sf_stream stream);

/* ---- introspection for bench/roofline ------------------------------------------------------- */
/* Enqueue `iters` back-to-back launches of the dominant GEMM (the MLP up-projection shape of the
 * loaded model at M rows) between two HIP events on `stream` and return the mean launch time.   */
int sf_bench_gemm(sf_encoder* enc, int M, int which, int iters, void* workspace_dev,
                  size_t workspace_bytes, sf_stream stream, float* mean_ms_out, double* flops_out);

/* Same for the attention kernels at the loaded model's shape: which = 0 spatial (B*T frames of N
 * tokens), 1 temporal (B*N sequences of T frames).  bytes_out = algorithmic bytes per launch
 * (read q,k,v once + write ctx once, in the storage type of the compute mode).                  */
int sf_bench_attention(sf_encoder* enc, int B, int T, int which, int iters, void* workspace_dev,
                       size_t workspace_bytes, sf_stream stream, float* mean_ms_out, double* bytes_out,
                       double* flops_out);

/* Environment switches (A/B and tuning knobs of the measurements; csrc/sf_switches.h holds the one table): the library reads them
 * once, at first use.  sf_reload_switches() re-reads the environment (tests flip a switch inside a process);
 * sf_switch_info(i, 0) / (i, 1) return name / description of switch i, NULL past the end.                                      */
void sf_reload_switches(void);
const char* sf_switch_info(int index, int what);

/* Launch floor of this device: `launches` dependent EMPTY kernels (256 workgroups of 256 threads) captured into one hipGraph and
 * replayed `iters` times; mean microseconds per launch.  What a chain of dependent launches costs when the kernels do nothing —
 * the yardstick next to the streamed frame's ~100-launch graph (bench.py `streaming.launch_floor`).                              */
int sf_bench_launch_floor(int device, int launches, int iters, sf_stream stream, float* us_per_launch_out);

#ifdef __cplusplus
}
#endif
#endif /* STREAMFORMER_HIP_H */
